"""The scene-specialised kernels with the static hit record (rt_core.h: RtHitShape, rt_finish_hit_static, the set tests of the
Lambertian branch: the parts RT_HIT_STATIC ships) on the GPU: the same bits as the generic kernels and as the CPU build of the core.  What the generated units declare, and that the hand-built scenes reach what they pin, is checked in test_hit_static.py."""
import numpy as np
import pytest

import hit_scenes as H
import orc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("arm,W,H_,spp", [(5, 96, 96, 16), (6, 64, 64, 12), (5, 8, 8, 4)])
def test_reference_arms_specialised_generic_and_cpu_core_agree(rt, gpu_ctx_factory, arm, W, H_, spp):
    """arm 6: the closest hit can be a medium, and its boxes sit under wrappers; the 8x8 Cornell frame is smaller than a workgroup"""
    sc = rt.Scene.reference(arm, build_seed=1)
    assert "wrap[" in sc.kernel_source() and "mat_kind[" in sc.kernel_source()
    ctx = gpu_ctx_factory(sc)
    assert ctx.specialised(), "no precompiled kernel found next to the library"
    a, sa = ctx.render(W, H_, spp)
    b, sb = ctx.render(W, H_, spp, generic=True)
    f, sf = orc.flat_render(sc, W, H_, spp, chunk=sa["chunk"])
    assert (sa["sorted"] & 4) and not (sb["sorted"] & 4)
    assert sa["segments"] == sb["segments"] == sf["segments"]
    assert np.array_equal(a, b, equal_nan=True) and np.array_equal(a, f, equal_nan=True)


@pytest.mark.parametrize("build", H.HAND_BUILT, ids=lambda f: f.__name__)
def test_hand_built_scenes_compiled_at_run_time(rt, gpu_ctx_factory, tmp_path, monkeypatch, build):
    monkeypatch.setenv("RT1W_KERNEL_CACHE", str(tmp_path / "kcache"))
    sc = build(rt)
    ctx = gpu_ctx_factory(sc)
    b, sb = ctx.render(32, 32, 4)
    assert not (sb["sorted"] & 4)
    info = ctx.specialise()
    assert info["active"] and not info["from_cache"]
    a, sa = ctx.render(32, 32, 4)
    f, sf = orc.flat_render(sc, 32, 32, 4, chunk=sa["chunk"])
    assert (sa["sorted"] & 4) and sa["segments"] == sb["segments"] == sf["segments"]
    assert np.array_equal(a, b, equal_nan=True) and np.array_equal(a, f, equal_nan=True)
    assert np.any(a > 0.0)


def test_f32_specialised_cornell_equals_f32_generic(rt, gpu_ctx_factory):
    sc = rt.Scene.reference(5, build_seed=1)
    ctx = gpu_ctx_factory(sc)
    a, sa = ctx.render(64, 64, 8, f32=True)
    b, sb = ctx.render(64, 64, 8, f32=True, generic=True)
    assert (sa["sorted"] & 4) and not (sb["sorted"] & 4)
    assert sa["segments"] == sb["segments"] and np.array_equal(a, b, equal_nan=True)
