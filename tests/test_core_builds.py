"""core_builds.py itself: libraries built around different scenes share no type name and no unique symbol, so each renders its own
scene whichever was loaded first; a tag is given out once; and the configuration line is the one every part's test used to write."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import core_builds as CB
import lambert_scenes as L
import orc
import slab_scenes as S

W, H, SPP, CHUNK = 28, 20, 4, 3


def sphere_then_rect(rt):
    """lights_rect_and_sphere with the light list in the other order"""
    return L.sphere_beside_rects(rt, lights=("sphere", "xz"))


# two pairs of one-scene libraries, every scene unit 0 of its own.  The first pair holds no light.  The second holds the same two lights
# in opposite orders: Topo::light_kind is read through a drawn index, so the compiler emits it as a unique symbol, and a library that
# read the other's table would take a rect for a sphere
PAIRS = {"plain": (S.under_translate, S.under_flip), "lit": (L.lights_rect_and_sphere, sphere_then_rect)}


@pytest.fixture(scope="module")
def libs(rt, tmp_path_factory):
    """pair -> [(tag, scene, library path, library)]"""
    work = tmp_path_factory.mktemp("core_builds")
    made = {pair: [(f"core_builds_{pair}_{f.__name__}", f(rt)) for f in fs] for pair, fs in PAIRS.items()}
    builds = {tag: CB.static_command(work / tag, tag, [(tag, sc, CB.topo_text(sc, "Topo"))]) for two in made.values() for tag, sc in two}
    CB.build_all([cmd for _, cmd in builds.values()])
    return {pair: [(tag, sc, builds[tag][0], orc.declare_flat(C.CDLL(builds[tag][0]))) for tag, sc in two] for pair, two in made.items()}


def symbols(so):
    """(type, name) of the library's defined dynamic symbols"""
    rows = [ln.split() for ln in subprocess.check_output(["nm", "-D", "--defined-only", so]).decode().splitlines()]
    return {(r[-2], r[-1]) for r in rows if len(r) >= 3}


@pytest.mark.parametrize("pair", list(PAIRS))
def test_each_library_renders_its_own_scene(libs, pair):
    (_, a_sc, _, _), (_, b_sc, _, _) = libs[pair]
    assert CB.topo_text(a_sc, "Topo") != CB.topo_text(b_sc, "Topo")   # the two units' tables do differ
    for _, sc, _, lib in libs[pair]:
        assert lib.orcflat_n_static() == 1
        a, sa = orc.flat_render(sc, W, H, SPP, chunk=CHUNK)
        b, sb = orc.flat_render(sc, W, H, SPP, chunk=CHUNK, variant=100, lib=lib)
        assert sa["segments"] == sb["segments"]
        assert np.array_equal(a, b, equal_nan=True)
        assert np.any(a > 0.0)


@pytest.mark.parametrize("pair", list(PAIRS))
def test_the_libraries_share_no_symbol_that_names_a_topo(libs, pair):
    """every library defines symbols that carry its unit's type name, and no two libraries define the same one; the lit pair's are
    unique symbols (`u`), the kind of which a process holds one object per name"""
    named, unique = [], []
    for tag, _, so, _ in libs[pair]:
        syms = symbols(so)
        named.append({name for _, name in syms if "Topo" in name})
        unique.append({name for kind, name in syms if kind == "u"})
        assert named[-1] and all(f"Topo_{tag}_0" in name for name in named[-1]), (tag, sorted(named[-1]))
        assert unique[-1] <= named[-1]
    assert not (named[0] & named[1]), sorted(named[0] & named[1])
    if pair == "lit":
        assert all(any("light_kind" in name for name in u) for u in unique), unique


def test_a_tag_is_given_out_once(libs, tmp_path):
    tag, sc, _, _ = libs["plain"][1]
    with pytest.raises(ValueError):
        CB.claim_tag(tag)
    with pytest.raises(ValueError):
        CB.static_command(tmp_path, tag, [("again", sc, CB.topo_text(sc, "Topo"))])
    with pytest.raises(ValueError):
        CB.claim_tag("not an identifier")


@pytest.mark.parametrize("arm", [5, 6])
def test_the_configuration_line_is_the_one_the_parts_tests_wrote(rt, arm):
    """the line as test_slab_reuse.py, test_hit_static.py and the others spelled it, with the names mapped; for a scene without media
    that is also test_box_free.py's `RtCfg<false, ...`"""
    sc, k = rt.Scene.reference(arm, build_seed=1), 3
    info = sc.info()
    assert info["has_media"] == (arm == 6)
    old = (f"typedef RtCfg<{'true' if info['has_media'] else 'false'}, {'true' if info['has_textures'] else 'false'}, "
           f"{'true' if info['has_moving'] else 'false'}, true, {max(2, info['scope_depth'])}, Topo{k}> CfgS{k};\n")
    topo = CB.topo_text(sc, "Topo")
    text = CB.unit_text(sc, topo, "t", k)
    assert text.startswith(topo.replace("struct Topo", f"struct Topo_t_{k}", 1)) and topo.count("Topo") == 1
    line = text[len(topo) + len(f"_t_{k}"):]
    assert re.sub(rf"Topo_t_{k}\b", f"Topo{k}", line).replace(f"Cfg_t_{k}", f"CfgS{k}") == old
