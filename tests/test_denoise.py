"""Feature-guided denoiser (rt1w_denoise / rt1w_denoise_device / rt1w_render_denoised, include/rt1w.h): an edge-avoiding a-trous filter over
a frame and its first-hit feature buffers.  CPU tier: the CPU twin (librt1w_lab.so: rt1w_lab_denoise_host, the kernels' own rt_denoise.h
built for the host) on the ABI surface, on synthetic images whose answer follows from the definitions, and on three noisy renders against
converged ones.  GPU tier: the kernels bit for bit against the twin at every level and both forms of the level kernel, the entry forms
against each other, non-interference with the render entries, and full frames."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import orc
from orc import rt as _rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
ULP = 2.0 ** -53

# the quality cases: arm -> (width, height, reference spp); the noisy frame is 16 spp with global_seed 0, the reference global_seed 1
QUALITY = {5: (96, 96, 4096), 4: (128, 72, 2048), 7: (64, 64, 2048)}
# mse(denoised) / mse(noisy) measured with the twin and the default parameters
MEASURED_RATIO = {5: 0.3037, 4: 0.1388, 7: 0.3469}


def generate_reference_frames():
    """Writes tests/golden/denoise_ref_arm{5,4,7}.npy: the converged frames of the quality test, rendered by this project's own CPU
    build of the core (about 20 s on 16 cores).  Run by hand when a quality case changes: python -c 'import test_denoise as t;
    t.generate_reference_frames()' from tests/."""
    rt = _rt()
    for arm, (w, h, spp) in QUALITY.items():
        ref, _ = orc.flat_render(rt.Scene.reference(arm, build_seed=1), w, h, spp, global_seed=1)
        np.save(os.path.join(GOLD, f"denoise_ref_arm{arm}.npy"), ref)


def _flat_guides(h, w, colour=(0.25, 0.5, 0.75), albedo=(0.5, 0.25, 1.0), normal=(0.0, 0.6, 0.8), depth=3.0, cov=1.0):
    frame = np.empty((h, w, 3))
    frame[:] = colour
    aov = np.empty((h, w, 8))
    aov[..., 0:3] = albedo
    aov[..., 3:6] = normal
    aov[..., 6] = depth
    aov[..., 7] = cov
    return frame, aov


# ------------------------------------------------------------------------------------------------------------------ CPU tier --

def test_abi_surface(rt):
    """The three entries are exported with the declared signatures, rt1w_denoise_params is 40 bytes without padding on both sides,
    and the twin refuses what the header says is invalid."""
    for name in ("rt1w_denoise", "rt1w_denoise_device", "rt1w_render_denoised"):
        assert hasattr(rt._lib, name)
    assert rt._lib.rt1w_denoise.argtypes[1]._type_ is rt.DenoiseParams and len(rt._lib.rt1w_denoise.argtypes) == 6
    assert len(rt._lib.rt1w_denoise_device.argtypes) == 6 and len(rt._lib.rt1w_render_denoised.argtypes) == 5
    assert rt._lib.rt1w_abi_sizeof(4) == C.sizeof(rt.DenoiseParams) == 40
    assert rt.DenoiseParams.sigma_colour.offset == 16 and rt.DenoiseParams.sigma_depth.offset == 32
    assert rt._lib.rt1w_abi_sizeof(5) == 0
    hdr = open(os.path.join(ROOT, "include", "rt1w.h")).read()
    assert "#define RT1W_DENOISE_KEEP_ALBEDO 1u" in hdr and rt.DENOISE_KEEP_ALBEDO == 1
    fn = rt.load_lab().rt1w_lab_denoise_host
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(rt.DenoiseParams), C.c_void_p, C.c_void_p, C.c_void_p]
    frame, aov = _flat_guides(4, 4)
    out = np.empty_like(frame)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    ok = rt.DenoiseParams(4, 4, 0, 0, 0.0, 0.0, 0.0)
    assert fn(C.byref(ok), ptr(frame), ptr(aov), ptr(out)) == 0
    assert fn(None, ptr(frame), ptr(aov), ptr(out)) == rt.ERR_INVALID
    assert fn(C.byref(ok), None, ptr(aov), ptr(out)) == rt.ERR_INVALID
    assert fn(C.byref(ok), ptr(frame), None, ptr(out)) == rt.ERR_INVALID
    assert fn(C.byref(ok), ptr(frame), ptr(aov), None) == rt.ERR_INVALID
    for bad in (rt.DenoiseParams(0, 4, 0, 0, 0, 0, 0), rt.DenoiseParams(4, 0, 0, 0, 0, 0, 0), rt.DenoiseParams(4, 4, 9, 0, 0, 0, 0),
                rt.DenoiseParams(4, 4, 0, 2, 0, 0, 0), rt.DenoiseParams(4, 4, 0, 0, -1.0, 0, 0), rt.DenoiseParams(4, 4, 0, 0, 0, 0, float("nan"))):
        assert fn(C.byref(bad), ptr(frame), ptr(aov), ptr(out)) == rt.ERR_INVALID
    assert fn(C.byref(rt.DenoiseParams(4, 4, 8, 1, 0, 0, 0)), ptr(frame), ptr(aov), ptr(out)) == 0
    with pytest.raises(rt.Rt1wError) as e:
        rt.denoise_host(frame, aov, iterations=9)
    assert e.value.code == rt.ERR_INVALID


@pytest.mark.parametrize("w,h", [(1, 1), (3, 7), (257, 5), (40, 33)])
@pytest.mark.parametrize("iterations", [1, 5, 8])
@pytest.mark.parametrize("keep", [False, True])
def test_flat_image_stays_flat(rt, w, h, iterations, keep):
    """Constant colour and guides: every weight is h(dx, dy) times a common factor, so the output is the input up to rounding.  A level
    is two sums of at most 25 terms and a division (about 53 roundings), 8 levels at most, demodulation two more: 512 * 2^-53 relative."""
    frame, aov = _flat_guides(h, w)
    out = rt.denoise_host(frame, aov, iterations=iterations, keep_albedo=keep)
    rel = np.abs(out - frame) / frame
    print("flat", w, h, iterations, keep, "max rel / ulp", rel.max() / ULP)
    assert np.all(rel <= 512 * ULP)
    # misses: zero normal, infinite depth, zero coverage
    frame, aov = _flat_guides(h, w, normal=(0.0, 0.0, 0.0), depth=np.inf, cov=0.0)
    out = rt.denoise_host(frame, aov, iterations=iterations, keep_albedo=keep)
    assert np.all(np.abs(out - frame) / frame <= 512 * ULP)


@pytest.mark.parametrize("kind", ["normals", "hit_miss"])
@pytest.mark.parametrize("iterations", [1, 5, 8])
def test_marked_edges_are_not_crossed(rt, kind, iterations):
    """Two regions whose guides give the cross-edge taps a weight of exactly 0 (perpendicular normals; a hit region against a miss
    region): colours 0 + noise on one side, 1 + noise on the other, albedo 1.  Every output pixel stays inside the closed range of its
    own side's inputs, widened by 512 * 2^-53 of the largest input for the rounding of the weighted means."""
    h, w = 37, 50
    rng = np.random.default_rng(7)
    left = np.zeros((h, w), dtype=bool)
    left[:, : w // 2] = True
    left[h // 2:, : w // 2 + 7] = True  # a step in the edge, so that taps cross it in both axes
    frame = np.where(left[..., None], 0.0, 1.0) + rng.uniform(0.0, 0.2, (h, w, 3))
    _, aov = _flat_guides(h, w, albedo=(1.0, 1.0, 1.0), normal=(1.0, 0.0, 0.0))
    if kind == "normals":
        aov[~left, 3:6] = (0.0, 1.0, 0.0)
    else:
        aov[~left, 3:6] = 0.0
        aov[~left, 6] = np.inf
        aov[~left, 7] = 0.0
    out = rt.denoise_host(frame, aov, iterations=iterations)
    slack = 512 * ULP * np.abs(frame).max()
    for side in (left, ~left):
        lo, hi = frame[side].min(), frame[side].max()
        print(kind, iterations, "side range", lo, hi, "output range", out[side].min(), out[side].max())
        assert out[side].min() >= lo - slack and out[side].max() <= hi + slack
    assert out[left].max() < 0.5 < out[~left].min()
    # and the filter does filter: inside a side the spread shrinks
    assert out[left].std() < 0.5 * frame[left].std()


def test_non_finite_inputs(rt):
    """A NaN pixel and an inf pixel in the frame come out as they went in and poison nobody."""
    h, w = 24, 31
    rng = np.random.default_rng(3)
    frame, aov = _flat_guides(h, w)
    frame += rng.uniform(0.0, 0.1, frame.shape)
    frame[5, 6] = np.nan
    frame[17, 20, 1] = np.inf
    for keep in (False, True):
        for it in (1, 5, 8):
            out = rt.denoise_host(frame, aov, iterations=it, keep_albedo=keep)
            assert np.all(np.isnan(out[5, 6])) and out[17, 20, 1] == np.inf
            bad = ~np.isfinite(out)
            bad[5, 6] = False
            bad[17, 20] = False
            assert not bad.any()
    # guides may be anything too: a NaN normal and a NaN depth reject, they do not spread
    aov[9, 9, 3:7] = np.nan
    frame[5, 6] = 0.3
    frame[17, 20] = 0.3
    assert np.all(np.isfinite(rt.denoise_host(frame, aov)))


def _disp(c):
    return np.sqrt(np.clip(c, 0.0, 0.999))  # the displayed value, src/color.rs:56-65


def _mse(a, b):
    return float(np.mean((_disp(a) - _disp(b)) ** 2))


@pytest.mark.parametrize("arm", sorted(QUALITY))
def test_quality_against_converged_frames(rt, arm):
    """The reason for the feature: a 16 spp frame filtered with the default parameters is closer to the converged frame (another seed)
    than the 16 spp frame itself, in the mean squared error of the displayed values over all pixels -- and by at least half of what
    was measured when the defaults were chosen (ratios 0.3037 Cornell, 0.1388 simple_light, 0.3469 final_scene)."""
    w, h, _ = QUALITY[arm]
    sc = rt.Scene.reference(arm, build_seed=1)
    noisy, _ = orc.flat_render(sc, w, h, 16)
    aov = rt.aov_host(sc, w, h, 16)
    ref = np.load(os.path.join(GOLD, f"denoise_ref_arm{arm}.npy"))
    assert ref.shape == noisy.shape
    den = rt.denoise_host(noisy, aov)
    m_noisy, m_den = _mse(noisy, ref), _mse(den, ref)
    print(f"arm {arm}: mse noisy {m_noisy:.6g} denoised {m_den:.6g} ratio {m_den / m_noisy:.4f}")
    assert m_den < m_noisy
    assert m_den / m_noisy <= (MEASURED_RATIO[arm] + 1.0) / 2.0


# ------------------------------------------------------------------------------------------------------------------ GPU tier --

def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.gpu
@pytest.mark.parametrize("arm", [0, 4, 5, 6, 7])
def test_gpu_equals_twin_bit_for_bit(rt, gpu_ctx_factory, arm):
    """rt1w_denoise == the CPU twin on rendered frames: every level count that crosses a boundary between the staged and the direct form
    of the level kernel (1, 2, 5, 8), with and without demodulation, non-default sigmas, sizes that are not multiples of the 8 x 8 block
    or the 16 x 16 workgroup tile, and images smaller than the largest step."""
    W, H = 203, 149
    sc = rt.Scene.reference(arm, build_seed=1, aspect_ratio=W / H)
    ctx = gpu_ctx_factory(sc)
    frame, _ = ctx.render(W, H, 8)
    aov = ctx.render_aov(W, H, 8)
    for it in (1, 2, 5, 8):
        for keep in (False, True):
            got, st = ctx.denoise(frame, aov, iterations=it, keep_albedo=keep, with_stats=True)
            assert _same(got, rt.denoise_host(frame, aov, iterations=it, keep_albedo=keep)), (arm, it, keep)
            assert st["passes"] == 1 and st["block"] == 256 and st["grid"] == ((W + 15) // 16) * ((H + 15) // 16) and st["kernel_ms"] > 0
    kw = dict(sigma_colour=0.3, sigma_normal=7.0, sigma_depth=0.9, iterations=4)
    assert _same(ctx.denoise(frame, aov, **kw), rt.denoise_host(frame, aov, **kw))
    assert _same(ctx.denoise(frame, aov), rt.denoise_host(frame, aov))  # all defaults
    for (y0, y1, x0, x1) in ((10, 15, 20, 25), (7, 8, 0, 203), (0, 149, 100, 101), (3, 20, 5, 22), (0, 16, 0, 16), (1, 34, 2, 35)):
        f, a = np.ascontiguousarray(frame[y0:y1, x0:x1]), np.ascontiguousarray(aov[y0:y1, x0:x1])
        for it in (2, 8):
            assert _same(ctx.denoise(f, a, iterations=it), rt.denoise_host(f, a, iterations=it)), (arm, f.shape, it)
    if arm == 5:  # images longer than a frame row in one direction only: 1 x 300 and 300 x 1
        line = np.ascontiguousarray(np.concatenate([frame[40], frame[41, :97]])[None])
        la = np.ascontiguousarray(np.concatenate([aov[40], aov[41, :97]])[None])
        assert line.shape == (1, 300, 3)
        for it in (5, 8):
            assert _same(ctx.denoise(line, la, iterations=it), rt.denoise_host(line, la, iterations=it))
            lt, lat = np.ascontiguousarray(line.transpose(1, 0, 2)), np.ascontiguousarray(la.transpose(1, 0, 2))
            assert _same(ctx.denoise(lt, lat, iterations=it), rt.denoise_host(lt, lat, iterations=it))
        nf = frame.copy()
        nf[30, 40] = np.nan
        nf[80, 90, 2] = np.inf
        assert _same(ctx.denoise(nf, aov), rt.denoise_host(nf, aov))


_TORCH_CHILD = r"""
import sys, importlib
import numpy as np
import torch
root, arm, W, H = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
sys.path.insert(0, root)
rt = importlib.import_module("raytracing-1w_amd")
ctx = rt.Context(rt.Scene.reference(arm, build_seed=1, aspect_ratio=W / H), 0)
frame, _ = ctx.render(W, H, 8, global_seed=3)
aov = ctx.render_aov(W, H, 8, global_seed=3)
host = ctx.denoise(frame, aov)
same = lambda a, b: a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
tf, ta = torch.from_numpy(frame).cuda(), torch.from_numpy(aov).cuda()
to = torch.zeros_like(tf)
torch.cuda.synchronize()
ctx.denoise_device(tf.data_ptr(), ta.data_ptr(), to.data_ptr(), W, H)
assert same(to.cpu().numpy(), host), "device form differs from the host form"
assert same(tf.cpu().numpy(), frame), "the input frame was written"
ctx.denoise_device(tf.data_ptr(), ta.data_ptr(), tf.data_ptr(), W, H)
assert same(tf.cpu().numpy(), host), "in-place form differs"
ctx.close()
print("TORCH-FORMS-OK")
"""


@pytest.mark.gpu
@pytest.mark.parametrize("arm", [5, 7])
def test_gpu_entry_forms_agree(rt, gpu_ctx_factory, arm):
    """The device form on torch tensors (out of place and in place) equals the host form; rt1w_render_denoised equals render + render_aov
    + denoise, also on a sub-tile; what it refuses is refused with the flag's name."""
    W, H = 120, 90
    sc = rt.Scene.reference(arm, build_seed=1, aspect_ratio=W / H)
    ctx = gpu_ctx_factory(sc)
    frame, _ = ctx.render(W, H, 8, global_seed=3)
    aov = ctx.render_aov(W, H, 8, global_seed=3)
    host = ctx.denoise(frame, aov)
    # torch has to initialise the HIP runtime before librt1w.so does (bench.py's order), so the tensors live in a process of their own
    child = subprocess.run([sys.executable, "-c", _TORCH_CHILD, ROOT, str(arm), str(W), str(H)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=240)
    assert child.returncode == 0 and "TORCH-FORMS-OK" in child.stdout, child.stdout[-3000:]
    # the same through plain device memory of the HIP runtime this process already uses
    hip = C.CDLL("libamdhip64.so")
    bufs = []
    for a in (frame, aov, np.zeros_like(frame)):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(a.nbytes)) == 0
        assert hip.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0  # HostToDevice
        bufs.append(p)

    def fetch(p, like):
        out = np.empty_like(like)
        assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), p, C.c_size_t(out.nbytes), 2) == 0  # DeviceToHost
        return out
    st = ctx.denoise_device(bufs[0].value, bufs[1].value, bufs[2].value, W, H)
    assert st["passes"] == 1 and st["kernel_ms"] > 0 and st["total_ms"] > 0
    assert _same(fetch(bufs[2], frame), host)
    assert _same(fetch(bufs[0], frame), frame) and _same(fetch(bufs[1], aov)[..., :6], aov[..., :6])  # inputs untouched
    ctx.denoise_device(bufs[0].value, bufs[1].value, bufs[0].value, W, H)  # in place
    assert _same(fetch(bufs[0], frame), host)
    for p in bufs:
        hip.hipFree(p)
    one, st1 = ctx.render_denoised(W, H, 8, global_seed=3, with_stats=True)
    assert _same(one, host)
    assert st1["paths"] == W * H * 8 and st1["passes"] >= 1 and st1["block"] == 256
    dn = dict(iterations=3, keep_albedo=True, sigma_colour=2.0)
    assert _same(ctx.render_denoised(W, H, 8, global_seed=3, denoise=dn), ctx.denoise(frame, aov, **dn))
    tile = (16, 9, 70, 50)
    ft, _ = ctx.render(W, H, 8, tile=tile, sample_offset=4)
    at = ctx.render_aov(W, H, 8, tile=tile, sample_offset=4)
    assert _same(ctx.render_denoised(W, H, 8, tile=tile, sample_offset=4), ctx.denoise(ft, at))
    assert _same(ctx.denoise(ft, at), rt.denoise_host(ft, at))
    for flags, name in ((rt.OUT_SUM, "RT1W_OUT_SUM"), (rt.OUT_FRAME, "RT1W_OUT_FRAME"), (rt.RNG_REFERENCE, "RT1W_RNG_REFERENCE"),
                        (rt.PROBE_COHERENT, "RT1W_PROBE_COHERENT")):
        with pytest.raises(rt.Rt1wError) as e:
            ctx.render_denoised(W, H, 8, flags=flags)
        assert e.value.code == rt.ERR_INVALID and name in str(e.value)
    with pytest.raises(rt.Rt1wError) as e:
        ctx.render_denoised(W, H, 8, tile=(0, 0, W, 30), strips=(10, 30))
    assert e.value.code == rt.ERR_INVALID and "strip_rows" in str(e.value)
    with pytest.raises(rt.Rt1wError) as e:
        ctx.render_denoised(W, H, 8, precision=1)
    assert e.value.code == rt.ERR_INVALID and "RT1W_PRECISION_F32" in str(e.value)
    with pytest.raises(rt.Rt1wError) as e:
        ctx.render_denoised(W, H, 8, denoise=dict(iterations=9))
    assert e.value.code == rt.ERR_INVALID
    p = ctx._params(W, H, 8, 50, None, 0, 0, 0, False)
    bad = rt.DenoiseParams(W + 1, H, 0, 0, 0.0, 0.0, 0.0)
    out = np.empty((H, W, 3))
    assert rt._lib.rt1w_render_denoised(ctx._h, C.byref(p), C.byref(bad), out.ctypes.data_as(C.c_void_p), None) == rt.ERR_INVALID
    good = rt.DenoiseParams(W, H, 0, 0, 0.0, 0.0, 0.0)
    assert rt._lib.rt1w_render_denoised(ctx._h, C.byref(p), C.byref(good), out.ctypes.data_as(C.c_void_p), None) == 0
    with pytest.raises(rt.Rt1wError) as e:
        ctx.denoise(frame, aov, iterations=9)
    assert e.value.code == rt.ERR_INVALID and "8 iterations" in str(e.value)


@pytest.mark.gpu
def test_gpu_renders_are_unchanged_by_a_denoise(rt, gpu_ctx_factory):
    """The filter shares the context's framebuffer and stream with the render entries: a beauty render and an AOV render after a denoise
    (and after the one-call form) equal the ones before it, bit for bit."""
    sc = rt.Scene.reference(5, build_seed=1)
    ctx = gpu_ctx_factory(sc)
    f0, s0 = ctx.render(90, 70, 8)
    a0 = ctx.render_aov(90, 70, 8)
    ctx.denoise(np.ones((200, 300, 3)), np.ones((200, 300, 8)))  # larger than anything rendered so far: the buffers grow
    ctx.render_denoised(90, 70, 8)
    f1, s1 = ctx.render(90, 70, 8)
    a1 = ctx.render_aov(90, 70, 8)
    assert _same(f0, f1) and _same(a0, a1) and s0["segments"] == s1["segments"]


@pytest.mark.gpu
@pytest.mark.parametrize("arm,size", [(5, 600), (7, 800)])
def test_gpu_full_frames(rt, gpu_ctx_factory, arm, size):
    """render_denoised of C3 (Cornell 600 x 600 x 16) and C4 (final_scene 800 x 800 x 16): finite, and equal to the twin run over the
    same frame and feature buffers on 4096 seeded pixels plus the four corners."""
    sc = rt.Scene.reference(arm, build_seed=1)
    ctx = gpu_ctx_factory(sc)
    out, st = ctx.render_denoised(size, size, 16, with_stats=True)
    assert out.shape == (size, size, 3) and np.all(np.isfinite(out))
    frame, sb = ctx.render(size, size, 16)
    aov = ctx.render_aov(size, size, 16)
    twin = rt.denoise_host(frame, aov)
    rng = np.random.default_rng(2010)
    ys = np.concatenate([rng.integers(0, size, 4096), [0, 0, size - 1, size - 1]])
    xs = np.concatenate([rng.integers(0, size, 4096), [0, size - 1, 0, size - 1]])
    assert _same(np.ascontiguousarray(out[ys, xs]), np.ascontiguousarray(twin[ys, xs]))
    print(f"arm {arm} {size}x{size}x16: render_denoised kernel {st['kernel_ms']:.2f} ms (beauty alone {sb['kernel_ms']:.2f}), total {st['total_ms']:.2f} ms")
