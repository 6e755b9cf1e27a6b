"""The sweep without box tests on the GPU (rt_core.h: rt_sweep_free, rt_box_free_verify): frames of the scene-specialised kernel as shipped
= the same kernel built with -DRT_BOX_FREE=0 (every box tested: the text before the box-free sweep) = built with
-DRT_DIV_SHARED_FORCE_SLOW=1 (every wave runs the second, boxed sweep as well) = the generic kernel = the CPU build of the core,
byte for byte.  The scenes are those of test_box_free.py: every media-free scene with a rect and at most 64 nodes; slab_scenes.py's two
send waves to the second sweep for real (zero direction components, 0 / 0 quotients)."""
import numpy as np
import pytest

import box_free_scenes as B
import core_builds as CB
import orc

pytestmark = pytest.mark.gpu

NAMES = ("cornell", "arm4", "coplanar_pair", "two_chains", "translate_only_rotate_only", "depth_three", "flip_above_bvh",
         "sphere_under_wrappers", "nan_best_t", "nan_some_rays")
BUILDS = (None, "-DRT_BOX_FREE=0", "-DRT_DIV_SHARED_FORCE_SLOW=1")


@pytest.fixture(scope="module")
def kernels(rt, gpu_ctx_factory, tmp_path_factory):
    """name -> (scene, context with the kernel as shipped, with every box tested, with the second sweep forced); built once per scene"""
    cache = str(tmp_path_factory.mktemp("box_free_kcache"))
    scenes = B.scenes(rt)
    assert tuple(scenes) == NAMES   # the list above is the CPU test's
    made = {}

    def get(name):
        if name not in made:
            sc = scenes[name]
            made[name] = (sc,) + tuple(CB.specialised(gpu_ctx_factory, sc, cache, o) for o in BUILDS)
        return made[name]

    return get


# every scene at 32x32 with depth 50 and depth 3 and at 8x4 (32 work items: half of the only wave that works has retired from the
# start), 8 spp.  A case renders in about 0.1 s; the first case of a scene compiles its three kernels as well (a few seconds: no scene
# here has more than 41 nodes)
FRAMES = [(name, W, H, 8, chunk, depth) for name in NAMES for (W, H, chunk, depth) in ((32, 32, 0, 50), (32, 32, 0, 3), (8, 4, 8, 50), (8, 4, 8, 3))]


@pytest.mark.parametrize("name,W,H,spp,chunk,depth", FRAMES, ids=lambda v: str(v))
def test_frames_equal_the_boxed_sweep(kernels, name, W, H, spp, chunk, depth):
    sc, on, off, slow = kernels(name)
    a, sa = on.render(W, H, spp, max_depth=depth, chunk=chunk)
    o, so = off.render(W, H, spp, max_depth=depth, chunk=sa["chunk"])
    w, sw = slow.render(W, H, spp, max_depth=depth, chunk=sa["chunk"])
    g, sg = on.render(W, H, spp, max_depth=depth, chunk=sa["chunk"], generic=True)
    f, sf = orc.flat_render(sc, W, H, spp, max_depth=depth, chunk=sa["chunk"])
    assert all(s["sorted"] & 4 for s in (sa, so, sw)) and not (sg["sorted"] & 4)   # three specialised kernels, one generic
    assert sa["segments"] == so["segments"] == sw["segments"] == sg["segments"] == sf["segments"]
    assert np.array_equal(a, f, equal_nan=True), "the box-free sweep differs from the CPU build of the core"
    assert np.array_equal(a, o, equal_nan=True), "the box-free sweep differs from the same kernel with every box tested"
    assert np.array_equal(w, o, equal_nan=True), "the second sweep differs from the kernel with every box tested"
    assert np.array_equal(g, f, equal_nan=True), "generic kernel differs from the CPU build of the core"
    assert np.any(a > 0.0)


def test_the_three_builds_are_three_kernels(kernels):
    """the switches reach the run-time compiler: three different code objects, and the shipped unit does declare the sweep"""
    sc, on, off, slow = kernels("cornell")
    assert len({c.specialise()["key"] for c in (on, off, slow)}) == 3
    assert B.declared(sc)[1]
