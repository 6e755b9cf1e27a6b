"""Static lights and wall frames in the Lambertian shading of the scene-specialised kernels (rt_core.h: RtLightShape, RtLambertWalls,
rt_wall_frame): the flat core built on the CPU around the library's own generated Topo (Scene.kernel_source) against the generic
core, bit for bit, and what the generated text declares."""
import numpy as np
import pytest

import core_builds as CB
import lambert_scenes as L
import orc
import slab_scenes as S

STRIPPED = ("cornell", "sphere_beside_rects", "lights_three")   # also built from their Topo without the new members


def scenes(rt):
    out = [("cornell", rt.Scene.reference(5, build_seed=1)), ("cornel_smoke", rt.Scene.reference(6, build_seed=1)),
           ("simple_light", rt.Scene.reference(4, build_seed=1)), ("two_spheres_checker", rt.Scene.reference(1, build_seed=1))]
    out += [(f.__name__, f(rt)) for f in L.HAND_BUILT]
    return out


@pytest.fixture(scope="module")
def cases(rt):
    return scenes(rt)


@pytest.fixture(scope="module")
def static_lib(cases, tmp_path_factory):
    work = tmp_path_factory.mktemp("lambert_static")
    by_name = dict(cases)
    topos = [(name, sc, CB.topo_text(sc, "Topo")) for name, sc in cases]
    topos += [(name + "_stripped", by_name[name], L.strip_new_members(CB.topo_text(by_name[name], "Topo"))) for name in STRIPPED]
    return CB.static_lib(work, "lambert_static", topos), [(name, sc) for name, sc, _ in topos]


@pytest.fixture(scope="module")
def generic_frames(cases):
    """the generic core's frame and statistics of every scene, rendered once"""
    out = {}
    for name, sc in cases:
        W, H, spp = CB.small_frame(name)
        out[name] = (W, H, spp) + orc.flat_render(sc, W, H, spp, chunk=3)
    return out


def test_generated_unit_declares_lights_and_walls(rt, cases):
    by_name = dict(cases)
    # Cornell: two lights, the XZ rect and the sphere, and no Lambertian surface but unwrapped axis rects (box1 is metal, the sphere glass)
    assert L.shape(by_name["cornell"]) == ([L.XZ, L.SPHERE], False, (True, True, True))
    # cornel_smoke: the same walls and light list of one; its Lambertian boxes sit below Translate / RotateY (inside the media)
    kinds, general, walls = L.shape(by_name["cornel_smoke"])
    assert kinds == [L.XZ] and walls == (True, True, True)
    # simple_light has no light list (main.rs passes none), two_spheres no rects at all
    assert L.shape(by_name["simple_light"])[0] == [] and L.shape(by_name["two_spheres_checker"]) == ([], True, (False, False, False))
    for f in L.HAND_BUILT:
        assert L.shape(by_name[f.__name__]) == L.EXPECTED_SHAPE[f.__name__], f.__name__
    # the folded FlipFace is in the leaf's kind word, and the leaf still counts as a plain rect (no general path in that unit)
    nodes = S.nodes_of(by_name["rect_under_flip"])
    assert any(int(k) == (L.XZ | L.LEAF_FLIPPED) for k in nodes['kind'])
    # both precisions carry the same members, and they come before the reuse table that ends the struct
    src, src32 = by_name["cornell"].kernel_source(), by_name["cornell"].kernel_source(f32=True)
    assert src[src.index("struct TopoJit"):] == src32[src32.index("struct TopoJit"):]
    assert src.index("n_lights") < src.index("lambert_general") < src.index("reuse[")


def test_new_members_name_kinds_not_coordinates(rt):
    """the members' text is the same wherever the lights are and differs with their kinds: moving a light keeps what they contribute to
    the kernel key (lights_three puts its two XZ lights at different places and heights)"""
    def members(sc):
        src = sc.kernel_source()
        return src[src.index("    static constexpr uint32_t n_lights"):src.index("    static constexpr uint32_t reuse[")]
    three = members(L.lights_three(rt))
    assert "light_kind[3] = {5u, 2u, 5u}" in three and "." not in three   # no floating-point literal at all
    assert members(L.sphere_beside_rects(rt)) == members(L.rect_under_translate(rt)) != members(L.lights_one_sphere(rt))
    assert L.sphere_beside_rects(rt).kernel_key() != L.lights_one_sphere(rt).kernel_key()


def test_static_lambert_equals_generic_core(static_lib, cases, generic_frames):
    lib, topos = static_lib
    assert lib.orcflat_n_static() == len(topos) == len(cases) + len(STRIPPED)
    for k, (name, sc) in enumerate(topos):
        W, H, spp, a, sa = generic_frames[name[:-len("_stripped")] if name.endswith("_stripped") else name]
        b, sb = orc.flat_render(sc, W, H, spp, chunk=3, variant=100 + k, lib=lib)
        assert sa["segments"] == sb["segments"], name
        assert np.array_equal(a, b, equal_nan=True), name
        assert np.any(a > 0.0), name   # a frame of zeros would compare nothing
