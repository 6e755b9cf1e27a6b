"""The scene-specialised kernels with slab products taken from the boxes above (Topo::reuse, rt_aabb_hit_chain) on the GPU:
the same bits as the generic kernels and as the CPU build of the core.  The table itself is checked in test_slab_reuse.py."""
import pytest

import core_builds as CB
import slab_scenes as S

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("arm,W,H,spp", [(5, 96, 96, 16), (6, 64, 64, 12)])
def test_reference_arms_specialised_generic_and_cpu_core_agree(rt, gpu_ctx_factory, arm, W, H, spp):
    sc = rt.Scene.reference(arm, build_seed=1)
    assert S.counts(S.reuse_table(sc))[0] > 0
    CB.agree_specialised_generic_core(gpu_ctx_factory(sc), sc, W, H, spp)


@pytest.mark.parametrize("build", S.HAND_BUILT, ids=lambda f: f.__name__)
def test_hand_built_scenes_compiled_at_run_time(rt, gpu_ctx_factory, tmp_path, monkeypatch, build):
    monkeypatch.setenv("RT1W_KERNEL_CACHE", str(tmp_path / "kcache"))
    sc = build(rt)
    CB.agree_compiled_at_run_time(gpu_ctx_factory(sc), sc)


def test_f32_specialised_cornell_equals_f32_generic(rt, gpu_ctx_factory):
    sc = rt.Scene.reference(5, build_seed=1)
    CB.agree_f32_specialised_generic(gpu_ctx_factory(sc))
