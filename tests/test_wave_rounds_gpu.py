"""The rejection samplers' rounds spread over the lanes of a wave (csrc/rt_core.h: rt_wave_rounds -- the Metal scatter's unit sphere,
which ships, and the camera's unit disk, which stays behind the switch) on the GPU: the reordering kernels with the form,
scene-specialised and generic, give the frames of the CPU build of the core, which keeps the loops, and of the same specialised kernel
built with -DRT_WAVE_ROUNDS=0 (the loops) and -DRT_WAVE_ROUNDS=3 (both parts), bit for bit.  The arithmetic and the assignment of
rounds to lanes are checked on the CPU in test_wave_rounds.py."""
import numpy as np
import pytest

import core_builds as CB
import lambert_scenes as L
import orc

pytestmark = pytest.mark.gpu


def _room(s, objects, aperture=0.0):
    s.set_world(s.bvh_node(objects + [L._xz_light(s)]))
    s.set_lights([L._xz_light(s)])
    s.set_background((0.5, 0.7, 1.0))
    s.set_camera((2.0, 2.0, 7.5), (2.0, 1.5, 0.0), (0, 1, 0), 50.0, 1.0, aperture, 6.0, 0.0, 1.0)
    s.commit()
    return s


def cornell(rt):
    return rt.Scene.reference(5, build_seed=1)


def metal_enclosure(rt):
    """six fuzzy metal walls around the camera and the light: every path's every bounce draws in the unit sphere, so whole waves
    want a sample and K is 1"""
    s = rt.Scene(build_seed=1)
    m = lambda k: s.metal((0.9 - 0.05 * k, 0.8, 0.6 + 0.05 * k), 0.3 + 0.1 * k)
    walls = [s.xz_rect(0.0, 4.0, 0.0, 8.0, 0.0, m(0)), s.xz_rect(0.0, 4.0, 0.0, 8.0, 4.0, m(1)), s.xy_rect(0.0, 4.0, 0.0, 4.0, 0.0, m(2)),
             s.xy_rect(0.0, 4.0, 0.0, 4.0, 8.0, m(3)), s.yz_rect(0.0, 4.0, 0.0, 8.0, 0.0, m(4)), s.yz_rect(0.0, 4.0, 0.0, 8.0, 4.0, m(5))]
    return _room(s, walls)


def metal_marble(rt):
    """one small fuzzy metal sphere in a Lambertian corner: a wave holds a few lanes that want a sample (K at its cap) or none"""
    s = rt.Scene(build_seed=1)
    return _room(s, L._corner(s) + [s.sphere((2.0, 0.9, 1.5), 0.45, s.metal((0.8, 0.85, 0.88), 0.6))])


def open_lens(rt):
    """aperture 0.6: the unit disk's values reach the ray (a metal box is there too)"""
    s = rt.Scene(build_seed=1)
    box = s.translate(s.rotate_y(s.aabox((0.0, 0.0, 0.0), (1.0, 1.6, 1.0), s.metal((0.8, 0.85, 0.88), 0.2)), 18.0), (0.5, 0.0, 1.2))
    return _room(s, L._corner(s) + [box], aperture=0.6)


SCENES = {f.__name__: f for f in (cornell, metal_enclosure, metal_marble, open_lens)}


@pytest.fixture(scope="module")
def kernels(rt, gpu_ctx_factory, tmp_path_factory):
    """name -> (scene, context with the kernel as shipped, with the loops, with both parts of the form); built once per scene"""
    cache = str(tmp_path_factory.mktemp("wave_rounds_kcache"))
    made = {}

    def get(name):
        if name not in made:
            sc = SCENES[name](rt)
            made[name] = (sc,) + tuple(CB.specialised(gpu_ctx_factory, sc, cache, o) for o in (None, "-DRT_WAVE_ROUNDS=0", "-DRT_WAVE_ROUNDS=3"))
        return made[name]

    return get


# scene, width, height, spp, chunk (0: the library's), max_depth
FRAMES = [("cornell", 32, 32, 8, 0, 50), ("cornell", 32, 32, 8, 0, 3),
          ("cornell", 8, 4, 8, 8, 50),          # 32 work items: half of the only wave that works has retired from the start
          ("metal_enclosure", 16, 16, 4, 0, 50), ("metal_enclosure", 16, 16, 4, 0, 3),
          ("metal_marble", 16, 16, 8, 0, 50), ("metal_marble", 8, 4, 8, 8, 50),
          ("open_lens", 16, 16, 8, 0, 50), ("open_lens", 16, 16, 8, 0, 3)]


@pytest.mark.parametrize("name,W,H,spp,chunk,depth", FRAMES, ids=lambda v: str(v))
def test_frames_equal_the_loops(kernels, name, W, H, spp, chunk, depth):
    sc, on, off, both = kernels(name)
    a, sa = on.render(W, H, spp, max_depth=depth, chunk=chunk)
    o, so = off.render(W, H, spp, max_depth=depth, chunk=sa["chunk"])
    b, sb = both.render(W, H, spp, max_depth=depth, chunk=sa["chunk"])
    g, sg = on.render(W, H, spp, max_depth=depth, chunk=sa["chunk"], generic=True)
    f, sf = orc.flat_render(sc, W, H, spp, max_depth=depth, chunk=sa["chunk"])
    assert all((s["sorted"] & 5) == 5 for s in (sa, so, sb)) and (sg["sorted"] & 5) == 1   # reordering kernels: three specialised, one generic
    assert sa["segments"] == so["segments"] == sb["segments"] == sg["segments"] == sf["segments"]
    assert np.array_equal(a, f, equal_nan=True), "specialised kernel with the wave form differs from the CPU build of the core"
    assert np.array_equal(a, o, equal_nan=True), "the wave form and the loops differ in the same kernel"
    assert np.array_equal(b, o, equal_nan=True), "the sphere's and the disk's wave forms together differ from the loops"
    assert np.array_equal(g, f, equal_nan=True), "generic reordering kernel differs from the CPU build of the core"
    assert np.any(a > 0.0)
    if depth == 50:
        assert sa["segments"] > W * H * spp * 3 // 2   # paths do bounce


def test_the_lens_sample_reaches_the_ray(rt, kernels):
    """the open lens blurs: its frame is not the pinhole's"""
    sc, on, off, both = kernels("open_lens")
    a, _ = on.render(16, 16, 8)
    s = rt.Scene(build_seed=1)
    box = s.translate(s.rotate_y(s.aabox((0.0, 0.0, 0.0), (1.0, 1.6, 1.0), s.metal((0.8, 0.85, 0.88), 0.2)), 18.0), (0.5, 0.0, 1.2))
    pin = _room(s, L._corner(s) + [box], aperture=0.0)
    p, _ = orc.flat_render(pin, 16, 16, 8)
    assert not np.array_equal(a, p)
