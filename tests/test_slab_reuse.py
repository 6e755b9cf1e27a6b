"""Slab products a box shares with the boxes above it (Topo::reuse, rt_aabb_hit_chain in rt_core.h): the table the library
generates, checked against the flat scene in plain Python, and the unrolled sweep built on the CPU around the library's own
table (Scene.kernel_source) against the generic sweep, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import core_builds as CB
import orc
import slab_scenes as S
from dual import random_scene_pair

# random graphs (dual.random_scene_pair), all with wrappers nested at least twice and entries in their tables; the last three with media
RANDOM_SEEDS = (3011, 3016, 3012, 3002, 3015, 3004)


def scenes(rt):
    out = [("cornell", rt.Scene.reference(5, build_seed=1)), ("cornel_smoke", rt.Scene.reference(6, build_seed=1)),
           ("cornell_seed3_drawn_axes", rt.Scene.reference(5, build_seed=3).set_bvh_build("reference"))]
    out += [(f"random{seed}", random_scene_pair(seed)[0]) for seed in RANDOM_SEEDS]
    out += [(f.__name__, f(rt)) for f in S.HAND_BUILT]
    return out


@pytest.fixture(scope="module")
def cases(rt):
    return scenes(rt)


@pytest.fixture(scope="module")
def static_lib(cases, tmp_path_factory):
    work = tmp_path_factory.mktemp("slab_reuse")
    counters = ("std::atomic<unsigned long long> orc_slab_forms[2];\n"
                'extern "C" unsigned long long orc_slab_form_count(int literal) { return orc_slab_forms[literal].exchange(0); }\n')
    # which form each box test of the unrolled sweep took (RT_STAT_SLAB, rt_core.h), counted for the whole library
    (work / "slab_stat.h").write_text("#include <atomic>\nextern std::atomic<unsigned long long> orc_slab_forms[2];\n"
                                      "#define RT_STAT_SLAB(literal) ((void)orc_slab_forms[literal].fetch_add(1, std::memory_order_relaxed))\n")
    lib = CB.static_lib(work, "slab_reuse", [(name, sc, CB.topo_text(sc, "Topo")) for name, sc in cases], ("-include", "slab_stat.h"),
                        prologue=counters)
    lib.orc_slab_form_count.restype = C.c_ulonglong
    lib.orc_slab_form_count.argtypes = [C.c_int]
    return lib


def test_table_names_only_boxes_above_in_the_same_ray_space(cases):
    """Over Scene.flat(0): every entry that names another node names a BVH node above it, no Translate, RotateY or ConstantMedium
    between them, with the same 8 bytes in that plane; Cornell has the 44 entries and 16 whole axes the tree holds."""
    by_name = dict(cases)
    for name, sc in cases:
        table, nodes = S.check_table(sc)
        if sc.info()["has_media"]:   # scenes with media take whole axes only (jit.cpp)
            assert all(r[a] == r[a + 3] for r in table for a in range(3)), name
    assert S.counts(S.reuse_table(by_name["cornell"])) == (44, 16)
    other, pairs = S.counts(S.reuse_table(by_name["cornel_smoke"]))
    assert other == 2 * pairs > 0
    for seed in RANDOM_SEEDS:
        sc = by_name[f"random{seed}"]
        assert sc.info()["scope_depth"] >= 2 and S.counts(S.reuse_table(sc))[0] > 0, seed
    assert sum(1 for seed in RANDOM_SEEDS if by_name[f"random{seed}"].info()["has_media"]) >= 2


def test_table_on_the_hand_built_scenes(cases):
    by_name = dict(cases)
    # the child's box is the parent's: all six planes, three whole axes; both are BVH1 nodes
    t, n = S.check_table(by_name["child_equals_parent"])
    k = S.kinds(n)
    hit = [i for i, r in enumerate(t) if all(x != i for x in r)]
    assert len(hit) == 1 and k[hit[0]] == S.BVH1 and len(set(t[hit[0]])) == 1 and k[t[hit[0]][0]] == S.BVH1
    assert n['d'][hit[0]].tobytes() == n['d'][t[hit[0]][0]].tobytes()
    # equal bounds in another subtree only: there is such a pair of boxes, and the table names neither for the other
    t, n = S.check_table(by_name["sibling_only"])
    k = S.kinds(n)
    found = 0
    for i in range(len(n)):
        for j in range(i):
            if k[i] <= S.BVH1 and k[j] <= S.BVH1 and int(n['skip'][j]) <= i:   # j's subtree ended before i
                for p in range(6):
                    if n['d'][i][p].tobytes() == n['d'][j][p].tobytes() and all(n['d'][a][p].tobytes() != n['d'][i][p].tobytes()
                                                                                  for a in S.same_space_bvh_ancestors(n, 0, i)):
                        assert t[i][p] == i
                        found += 1
    assert found >= 4
    # below a Translate: the same numbers as the box above it, another ray space -- nothing is taken
    t, n = S.check_table(by_name["under_translate"])
    k = S.kinds(n)
    tr = k.index(S.TRANSLATE)
    inner, outer = tr + 1, 0
    assert k[inner] == S.BVH1 and sum(n['d'][inner][p].tobytes() == n['d'][outer][p].tobytes() for p in range(6)) >= 5
    assert S.counts(t) == (0, 0)
    # below a FlipFace: the box above it is taken, whole
    t, n = S.check_table(by_name["under_flip"])
    k = S.kinds(n)
    fl = k.index(S.FLIP)
    assert k[fl + 1] == S.BVH2 and t[fl + 1] == [fl - 1] * 6 and k[fl - 1] == S.BVH1


def test_unrolled_sweep_with_the_table_equals_generic_sweep(cases, static_lib):
    lib = static_lib
    assert lib.orcflat_n_static() == len(cases)
    lib.orc_slab_form_count(0), lib.orc_slab_form_count(1)
    for k, (name, sc) in enumerate(cases):
        W, H, spp = CB.small_frame(name)
        a, sa = orc.flat_render(sc, W, H, spp, chunk=3)
        b, sb = orc.flat_render(sc, W, H, spp, chunk=3, variant=100 + k, lib=lib)
        fast, literal = lib.orc_slab_form_count(0), lib.orc_slab_form_count(1)
        assert sa["segments"] == sb["segments"], name
        assert np.array_equal(a, b, equal_nan=True), name
        assert fast > 0, name
        if name == "nan_best_t":
            # the sweep order the docstring of the scene relies on: root, the rect, a box, a sphere, a box
            assert S.kinds(S.nodes_of(sc))[:5] == [S.BVH2, 5, S.BVH2, 2, S.BVH2]
            # ... and that last box, tested in the fast form, takes its x and y pairs from the box the literal form filled
            t = S.reuse_table(sc)
            assert literal > 0 and t[4][0] == t[4][3] == t[4][1] == t[4][4] == 2
        if name == "nan_some_rays":
            assert literal > 0   # the rays that reach the rect, and what their paths do afterwards; the others stay in the fast form


def test_kernel_source_hook(rt):
    """rt1w_scene_kernel_source: the generated unit as text, both precisions around the same tables; refused where there is no
    specialised kernel."""
    a = rt.Scene.reference(5, build_seed=1)
    src, src32 = a.kernel_source(), a.kernel_source(f32=True)
    assert src.count("reuse[29][6]") == 1 and "#define RT_F32 1" in src32 and "#define RT_F32 1" not in src
    assert src[src.index("struct TopoJit"):] == src32[src32.index("struct TopoJit"):]
    with pytest.raises(rt.Rt1wError) as e:
        rt.Scene.reference(0, build_seed=1, aspect_ratio=1.5).kernel_source()
    assert e.value.code == rt.ERR_UNSUPPORTED
