"""The scene-specialised kernels with the light list walked at compile time and constant wall frames (rt_core.h: RtLightShape,
RtLambertWalls) on the GPU: the same bits as the generic kernels and as the CPU build of the core.  What the generated units
declare is checked in test_lambert_static.py."""
import numpy as np
import pytest

import core_builds as CB
import lambert_scenes as L

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("arm,W,H,spp", [(5, 96, 96, 16), (6, 64, 64, 12), (5, 8, 8, 4)])
def test_reference_arms_specialised_generic_and_cpu_core_agree(rt, gpu_ctx_factory, arm, W, H, spp):
    """the 8x8 Cornell frame is smaller than a workgroup"""
    sc = rt.Scene.reference(arm, build_seed=1)
    assert L.shape(sc)[0][0] == L.XZ
    CB.agree_specialised_generic_core(gpu_ctx_factory(sc), sc, W, H, spp)


@pytest.mark.parametrize("build", L.HAND_BUILT, ids=lambda f: f.__name__)
def test_hand_built_scenes_compiled_at_run_time(rt, gpu_ctx_factory, tmp_path, monkeypatch, build):
    monkeypatch.setenv("RT1W_KERNEL_CACHE", str(tmp_path / "kcache"))
    sc = build(rt)
    assert L.shape(sc) == L.EXPECTED_SHAPE[build.__name__]
    assert np.any(CB.agree_compiled_at_run_time(gpu_ctx_factory(sc), sc) > 0.0)


def test_f32_specialised_cornell_equals_f32_generic(rt, gpu_ctx_factory):
    sc = rt.Scene.reference(5, build_seed=1)
    CB.agree_f32_specialised_generic(gpu_ctx_factory(sc))
