"""The scene-specialised kernels with the static hit record (rt_core.h: RtHitShape, rt_finish_hit_static, the set tests of the
Lambertian branch: the parts RT_HIT_STATIC ships) on the GPU: the same bits as the generic kernels and as the CPU build of the core.  What the generated units declare, and that the hand-built scenes reach what they pin, is checked in test_hit_static.py."""
import numpy as np
import pytest

import core_builds as CB
import hit_scenes as H

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("arm,W,H_,spp", [(5, 96, 96, 16), (6, 64, 64, 12), (5, 8, 8, 4)])
def test_reference_arms_specialised_generic_and_cpu_core_agree(rt, gpu_ctx_factory, arm, W, H_, spp):
    """arm 6: the closest hit can be a medium, and its boxes sit under wrappers; the 8x8 Cornell frame is smaller than a workgroup"""
    sc = rt.Scene.reference(arm, build_seed=1)
    assert "wrap[" in sc.kernel_source() and "mat_kind[" in sc.kernel_source()
    CB.agree_specialised_generic_core(gpu_ctx_factory(sc), sc, W, H_, spp)


@pytest.mark.parametrize("build", H.HAND_BUILT, ids=lambda f: f.__name__)
def test_hand_built_scenes_compiled_at_run_time(rt, gpu_ctx_factory, tmp_path, monkeypatch, build):
    monkeypatch.setenv("RT1W_KERNEL_CACHE", str(tmp_path / "kcache"))
    sc = build(rt)
    assert np.any(CB.agree_compiled_at_run_time(gpu_ctx_factory(sc), sc) > 0.0)


def test_f32_specialised_cornell_equals_f32_generic(rt, gpu_ctx_factory):
    sc = rt.Scene.reference(5, build_seed=1)
    CB.agree_f32_specialised_generic(gpu_ctx_factory(sc))
