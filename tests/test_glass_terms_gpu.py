"""The glass and light bounces without their scene-only terms (rt_core.h: RT_MAT_DERIVED, RT_NORMAL_SHARED, RT_LOBE_SHARED) in the
run-time-compiled units, on the GPU, where the real wave masks and the real reciprocal seed are.

Frames: the kernel as shipped = each part alone = all three = none (the text before the change) = the generic kernel = the CPU build of
the core, byte for byte, segment counts equal; one single-precision render (that build takes none of the parts) and the stack-walk
kernel on glass (arm 0, which reads the same records)."""
import numpy as np
import pytest

import core_builds as CB
import glass_scenes as G
import orc

pytestmark = pytest.mark.gpu

SCENES = {f.__name__: f for f in G.SPECIALISED}
ON = {"A": "-DRT_MAT_DERIVED=1", "B": "-DRT_NORMAL_SHARED=1", "C": "-DRT_LOBE_SHARED=1"}


def _opts(parts):
    """every switch said, so that a build does not depend on the committed defaults"""
    return " ".join(ON[k] if k in parts else G.OFF[k] for k in "ABC")


# None: as shipped.  Then each part alone, all three together, and none
BUILDS = (None, _opts("A"), _opts("B"), _opts("C"), _opts("ABC"), _opts(""))


@pytest.fixture(scope="module")
def kernels(rt, gpu_ctx_factory, tmp_path_factory):
    """name -> (scene, [a context per build]); built once per scene"""
    cache = str(tmp_path_factory.mktemp("glass_terms_kcache"))
    made = {}

    def get(name):
        if name not in made:
            sc = SCENES[name](rt)
            made[name] = (sc, [CB.specialised(gpu_ctx_factory, sc, cache, o) for o in BUILDS])
        return made[name]

    return get


FRAMES = [(name, W, H, chunk) for name in SCENES for (W, H, chunk) in G.FRAMES]


@pytest.mark.parametrize("name,W,H,chunk", FRAMES, ids=lambda v: str(v))
def test_frames_equal_under_every_switch(kernels, name, W, H, chunk):
    sc, ctxs = kernels(name)
    a, sa = ctxs[0].render(W, H, 8, chunk=chunk)
    assert sa["sorted"] & 4
    f, sf = orc.flat_render(sc, W, H, 8, chunk=sa["chunk"])
    g, sg = ctxs[0].render(W, H, 8, chunk=sa["chunk"], generic=True)
    assert not (sg["sorted"] & 4)
    assert sa["segments"] == sf["segments"] == sg["segments"]
    assert np.array_equal(a, f, equal_nan=True), "the shipped kernel differs from the CPU build of the core"
    assert np.array_equal(g, f, equal_nan=True), "the generic kernel differs from the CPU build of the core"
    for opts, ctx in zip(BUILDS[1:], ctxs[1:]):
        o, so = ctx.render(W, H, 8, chunk=sa["chunk"])
        assert so["sorted"] & 4 and so["segments"] == sa["segments"], opts
        assert np.array_equal(o.view(np.uint64), a.view(np.uint64)), opts + " changes the frame"
    assert np.any(a > 0.0)


def test_the_builds_are_different_kernels(kernels):
    """the switches reach the run-time compiler: a code object per setting, and the shipped unit is one of them by its instructions
    only (its key is its own: the options are part of a key)"""
    _, ctxs = kernels("cornell")
    assert len({c.specialise()["key"] for c in ctxs}) == len(BUILDS)


def test_f32_render_takes_none_of_the_parts(rt, gpu_ctx_factory):
    """single precision on Cornell: the specialised and the generic f32 kernels agree, and with 64-bit elementary functions the frame is
    the CPU twin's, which computes 1 / ir and r0 from d[0] as ever"""
    sc = G.cornell(rt)
    ctx = gpu_ctx_factory(sc)
    a, sa = ctx.render(32, 32, 8, f32=True)
    b, sb = ctx.render(32, 32, 8, f32=True, generic=True, chunk=sa["chunk"])
    assert (sa["sorted"] & 4) and not (sb["sorted"] & 4)
    assert sa["segments"] == sb["segments"] and np.array_equal(a, b, equal_nan=True)
    with rt.f32_exact():
        e, se = ctx.render(32, 32, 8, f32=True, generic=True, chunk=1)
    t, st = orc.flat_f32_render(sc, 32, 32, 8, chunk=1, variant=se["variant"])
    assert se["segments"] == st["segments"] and np.array_equal(e, t, equal_nan=True)


def test_stack_walk_kernel_on_glass(rt, gpu_ctx_factory):
    """arm 0 cropped: the pair-walk kernel reads the same Dielectric records"""
    sc = G.random_scene(rt)
    W, H = G.ARM0_FRAME
    ctx = gpu_ctx_factory(sc)
    a, sa = ctx.render(W, H, 8, tile=G.ARM0_TILE)
    f, sf = orc.flat_render(sc, W, H, 8, tile=G.ARM0_TILE, chunk=sa["chunk"])
    assert sa["segments"] == sf["segments"] and np.array_equal(a, f, equal_nan=True)
    assert np.any(a > 0.0)
