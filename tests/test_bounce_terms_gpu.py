"""The sphere light's cone evaluated once per Lambertian bounce (rt_core.h: RT_LIGHT_CONE) and the sweep's verdict tokens from the mask
of a compare the leaf makes anyway (RT_AHEAD_WORD 2) in the scene-specialised kernels, on the GPU, where the real wave masks are.

Frames: the kernel as shipped = the same kernel with each switch at its other setting alone (the cone out is the text before both)
= with both parts in = the generic kernel = the CPU build of the core, byte for byte, segment counts equal."""
import numpy as np
import pytest

import bounce_scenes as Bn
import core_builds as CB
import orc

pytestmark = pytest.mark.gpu

# arm 5, arm 6 and the sphere-only room of the issue, and the room whose floor reaches into the light sphere (the NaN cone on the device)
SCENES = {f.__name__: f for f in (Bn.cornell, Bn.cornel_smoke, Bn.sphere_only, Bn.inside_light)}
# None: as shipped (the cone in, the tokens behind their switch).  Then each switch alone at its other setting -- the cone out (the
# text before this change), the tokens in (both parts) -- and the tokens alone.
BUILDS = (None, "-DRT_LIGHT_CONE=0", "-DRT_AHEAD_WORD=2", "-DRT_AHEAD_WORD=2 -DRT_LIGHT_CONE=0")


@pytest.fixture(scope="module")
def kernels(rt, gpu_ctx_factory, tmp_path_factory):
    """name -> (scene, [a context per build]); built once per scene"""
    cache = str(tmp_path_factory.mktemp("bounce_terms_kcache"))
    made = {}

    def get(name):
        if name not in made:
            sc = SCENES[name](rt)
            made[name] = (sc, [CB.specialised(gpu_ctx_factory, sc, cache, o) for o in BUILDS])
        return made[name]

    return get


FRAMES = [(name, W, H, chunk, depth) for name in SCENES for (W, H, chunk, depth) in Bn.FRAMES]

@pytest.mark.parametrize("name,W,H,chunk,depth", FRAMES, ids=lambda v: str(v))
def test_frames_equal_under_every_switch(kernels, name, W, H, chunk, depth):
    sc, ctxs = kernels(name)
    a, sa = ctxs[0].render(W, H, 8, max_depth=depth, chunk=chunk)
    assert sa["sorted"] & 4
    f, sf = orc.flat_render(sc, W, H, 8, max_depth=depth, chunk=sa["chunk"])
    g, sg = ctxs[0].render(W, H, 8, max_depth=depth, chunk=sa["chunk"], generic=True)
    assert not (sg["sorted"] & 4)
    assert sa["segments"] == sf["segments"] == sg["segments"]
    assert np.array_equal(a, f, equal_nan=True), "the shipped kernel differs from the CPU build of the core"
    assert np.array_equal(g, f, equal_nan=True), "the generic kernel differs from the CPU build of the core"
    for opts, ctx in zip(BUILDS[1:], ctxs[1:]):
        o, so = ctx.render(W, H, 8, max_depth=depth, chunk=sa["chunk"])
        assert so["sorted"] & 4 and so["segments"] == sa["segments"], opts
        assert np.array_equal(o.view(np.uint64), a.view(np.uint64)), opts + " changes the frame"
    assert np.any(a > 0.0)


def test_the_builds_are_different_kernels(kernels):
    """the switches reach the run-time compiler: a code object per setting"""
    _, ctxs = kernels("cornell")
    assert len({c.specialise()["key"] for c in ctxs}) == len(BUILDS)
