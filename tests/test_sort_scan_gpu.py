"""The sort's class bases from one wave scan (csrc/rt_kernel_sorted.h: RT_SORT_SCAN; include/rt1w_num.h: rt_sort_scan, rt_sort_slot)
and the wrappers' kinds as template arguments of the unrolled sweeps (csrc/rt_core.h: rt_scope_in_k, RT_SCOPE_STATIC) on the GPU.  Neither
touches a path's arithmetic, so the frames of the scene-specialised kernel as shipped = the same unit built with both switches at 0
(every lane sums every count; the wrapper dispatched on its record: the text before this change) = with either switch alone = the generic
reordering kernel (which takes the scan too) = the CPU build of the core, bit for bit.  The slot arithmetic is checked on the CPU in
test_sort_scan.py."""
import numpy as np
import pytest

import core_builds as CB
import hit_scenes as H
import orc
import test_wave_rounds_gpu as WR

pytestmark = pytest.mark.gpu


def cornell(rt):
    return rt.Scene.reference(5, build_seed=1)


def cornell_smoke(rt):
    """arm 6: the boundaries of its media hit the class OTHER; a unit with media keeps its boxes (rt_sweep_static)"""
    return rt.Scene.reference(6, build_seed=1)


def translate_only(rt):
    return H.translate_only_rotate_only(rt, omit=1)


def rotate_y_only(rt):
    return H.translate_only_rotate_only(rt, omit=0)


# metal_enclosure: every bounce is Metal, so one class fills whole waves and the other counts are zero
SCENES = {"cornell": cornell, "cornell_smoke": cornell_smoke, "metal_enclosure": WR.metal_enclosure, "two_chains": H.two_chains,
          "translate_only": translate_only, "rotate_y_only": rotate_y_only}
BUILDS = (None, "-DRT_SORT_SCAN=0 -DRT_SCOPE_STATIC=0", "-DRT_SCOPE_STATIC=0", "-DRT_SORT_SCAN=0")


@pytest.fixture(scope="module")
def kernels(rt, gpu_ctx_factory, tmp_path_factory):
    """name -> (scene, contexts with the kernel as shipped, with neither part, with the scan alone, with the static kinds alone)"""
    cache = str(tmp_path_factory.mktemp("sort_scan_kcache"))
    made = {}

    def get(name):
        if name not in made:
            sc = SCENES[name](rt)
            made[name] = (sc,) + tuple(CB.specialised(gpu_ctx_factory, sc, cache, o) for o in BUILDS)
        return made[name]

    return get


# 8x4 at 8 spp in one chunk: 32 work items, fewer than one workgroup sorts, so lanes are idle from the first iteration on and three of
# the four waves hold nothing else; 24x24 at 4 spp: several workgroups, the last one partly idle.  A case renders in about 0.1 s; the
# first case of a scene compiles its four kernels as well.
FRAMES = [(name, W, H_, spp, chunk, depth) for name in SCENES for (W, H_, spp, chunk) in ((8, 4, 8, 8), (24, 24, 4, 0)) for depth in (3, 50)]


@pytest.mark.parametrize("name,W,H_,spp,chunk,depth", FRAMES, ids=lambda v: str(v))
def test_frames_equal_the_double_loop(kernels, name, W, H_, spp, chunk, depth):
    sc, on, neither, scan, static = kernels(name)
    a, sa = on.render(W, H_, spp, max_depth=depth, chunk=chunk)
    others = [c.render(W, H_, spp, max_depth=depth, chunk=sa["chunk"]) for c in (neither, scan, static)]
    g, sg = on.render(W, H_, spp, max_depth=depth, chunk=sa["chunk"], generic=True)
    f, sf = orc.flat_render(sc, W, H_, spp, max_depth=depth, chunk=sa["chunk"])
    assert (sa["sorted"] & 5) == 5 and all((s["sorted"] & 5) == 5 for _, s in others) and (sg["sorted"] & 5) == 1   # reordering kernels: four specialised, one generic
    assert sa["segments"] == sg["segments"] == sf["segments"] and all(s["segments"] == sf["segments"] for _, s in others)
    assert np.array_equal(a, f, equal_nan=True), "the kernel as shipped differs from the CPU build of the core"
    for (o, _), what in zip(others, ("neither part", "the scan alone", "the static wrapper kinds alone")):
        assert np.array_equal(o, a, equal_nan=True), "the kernel as shipped differs from the same unit with " + what
    assert np.array_equal(g, f, equal_nan=True), "generic reordering kernel differs from the CPU build of the core"
    assert np.any(a > 0.0)
    if depth == 50:
        assert sa["segments"] > W * H_ * spp * 3 // 2   # paths do bounce


def test_the_four_builds_are_four_kernels(kernels):
    """the switches reach the run-time compiler: four different code objects"""
    assert len({c.specialise()["key"] for c in kernels("cornell")[1:]}) == 4
