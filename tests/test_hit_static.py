"""The static hit record of the scene-specialised kernels (rt_core.h: RtHitShape, rt_finish_hit_static; the sort class and the
wrapper of a hit as compile-time functions of the leaf): the flat core built on the CPU around the library's own generated Topo
(Scene.kernel_source) against the generic core, bit for bit, and what the generated text declares."""
import numpy as np
import pytest

import core_builds as CB
import hit_scenes as H
import orc
import slab_scenes as S

STRIPPED = ("cornell", "two_chains", "many_chains")   # also built from their Topo without the new members


def scenes(rt):
    out = [("cornell", rt.Scene.reference(5, build_seed=1)), ("cornel_smoke", rt.Scene.reference(6, build_seed=1)),
           ("earth", rt.Scene.reference(3, build_seed=1)), ("two_spheres_checker", rt.Scene.reference(1, build_seed=1))]
    out += [(f.__name__, f(rt)) for f in H.HAND_BUILT]
    return out


@pytest.fixture(scope="module")
def cases(rt):
    return scenes(rt)


# the parts of the static form that are built (rt_core.h: RT_HIT_STATIC): the shipped mix, and every part -- the class and the wrapper
# from the leaf and the material word in the wrapper's place, which stay behind the switch
@pytest.fixture(scope="module", params=[None, 15], ids=["shipped", "every_part"])
def static_lib(request, cases, tmp_path_factory):
    work = tmp_path_factory.mktemp("hit_static")
    by_name = dict(cases)
    topos = [(name, sc, CB.topo_text(sc, "Topo")) for name, sc in cases]
    topos += [(name + "_stripped", by_name[name], H.strip_new_members(CB.topo_text(by_name[name], "Topo"))) for name in STRIPPED]
    flags = () if request.param is None else (f"-DRT_HIT_STATIC={request.param}",)
    return CB.static_lib(work, f"hit_static_{request.param}", topos, flags), [(name, sc) for name, sc, _ in topos]


shape_of = CB.small_frame


@pytest.fixture(scope="module")
def generic_frames(cases):
    """the generic core's frame and statistics of every scene, rendered once"""
    return {name: orc.flat_render(sc, *shape_of(name), chunk=3) for name, sc in cases}


def test_tables_agree_with_the_flat_nodes(cases):
    for name, sc in cases:
        nodes = S.nodes_of(sc)
        wrap, mat_kind = H.tables(sc)
        assert len(wrap) == len(mat_kind) == len(nodes), name
        for i, nd in enumerate(nodes):
            k = int(nd['kind']) & 0xFF
            assert wrap[i] == (H.NONE if k <= S.BVH1 else int(nd['b'])), (name, i)
            leaf = H.SPHERE <= k <= H.YZ or k == H.MEDIUM
            assert mat_kind[i] == (int(nd['mat']) >> 16 if leaf else 0), (name, i)


def test_hand_built_scenes_have_the_chains_they_are_named_for(cases):
    by_name = dict(cases)
    kinds = lambda name, chain: [int(S.nodes_of(by_name[name])['kind'][j]) & 0xFF for j in chain]
    chains = {name: H.chains(S.nodes_of(sc), H.tables(sc)[0]) for name, sc in cases}
    assert chains["cornell"] and len(chains["cornell"]) == 1 and kinds("cornell", chains["cornell"][0]) == [H.TRANSLATE, H.ROTATE_Y]
    assert len(chains["two_chains"]) == 2 and all(kinds("two_chains", c) == [H.TRANSLATE, H.ROTATE_Y] for c in chains["two_chains"])
    assert sorted(kinds("translate_only_rotate_only", c) for c in chains["translate_only_rotate_only"]) == [[H.TRANSLATE], [H.ROTATE_Y]]
    assert [kinds("depth_three", c) for c in chains["depth_three"]] == [[H.TRANSLATE, H.ROTATE_Y, H.TRANSLATE]]
    assert [kinds("flip_above_bvh", c) for c in chains["flip_above_bvh"]] == [[H.FLIP]]
    nodes = S.nodes_of(by_name["flip_above_bvh"])
    assert sum(1 for k in nodes['kind'] if int(k) == (H.XZ | 0x100)) >= 1   # and the directly flipped leaf, folded
    leaf_kinds = {int(k) & 0xFF for k in S.nodes_of(by_name["sphere_under_wrappers"])['kind']}
    assert H.SPHERE in leaf_kinds and H.MSPHERE in leaf_kinds and len(chains["sphere_under_wrappers"]) == 2
    assert len(chains["many_chains"]) == H.N_MANY > H.MAX_CHAINS and len(S.nodes_of(by_name["many_chains"])) > 64
    # arm 6: its boxes are boundaries of media (never a path's closest hit), the media themselves stand outside every wrapper
    smoke = S.nodes_of(by_name["cornel_smoke"])
    assert any((int(k) & 0xFF) == H.MEDIUM for k in smoke['kind'])
    # arm 3: the image texture reads (u, v)
    assert any(m & 0x100 for m in H.tables(by_name["earth"])[1])


def test_new_members_hold_indices_and_kinds_only(rt, cases):
    by_name = dict(cases)
    for name, sc in cases:
        text = H.members_text(sc)
        assert "." not in text and text == H.members_text(sc, f32=True), name   # no floating-point literal; both precisions alike
        src = sc.kernel_source()
        assert src.index("skip[") < src.index("wrap[") < src.index("mat_kind[") < src.index("reuse["), name
    # other angles, offsets, sizes and colours: the same text (what else the key holds, which bounds coincide, is the reuse table's)
    moved = H.two_chains(rt, variant=True)
    assert H.members_text(moved) == H.members_text(by_name["two_chains"])
    assert not np.array_equal(S.nodes_of(moved)['d'], S.nodes_of(by_name["two_chains"])['d'])


def test_static_hit_record_equals_generic_core(static_lib, cases, generic_frames):
    lib, topos = static_lib
    assert lib.orcflat_n_static() == len(topos) == len(cases) + len(STRIPPED)
    for k, (name, sc) in enumerate(topos):
        base = name[:-len("_stripped")] if name.endswith("_stripped") else name
        a, sa = generic_frames[base]
        b, sb = orc.flat_render(sc, *shape_of(base), chunk=3, variant=100 + k, lib=lib)
        assert sa["segments"] == sb["segments"], name
        assert np.array_equal(a, b, equal_nan=True), name
        assert np.any(a > 0.0), name   # a frame of zeros would compare nothing


@pytest.mark.parametrize("build", H.HAND_BUILT, ids=lambda f: f.__name__)
def test_pinned_objects_are_reached(rt, generic_frames, build):
    """a condition on the scenes, not on the code: without a pinned object the generic frame is another one"""
    name = build.__name__
    a, _ = generic_frames[name]
    for k in range(H.PINNED[name]):
        b, _ = orc.flat_render(build(rt, omit=k), *shape_of(name), chunk=3)
        assert not np.array_equal(a, b, equal_nan=True), (name, k)
