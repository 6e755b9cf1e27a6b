"""Variance-guided denoiser (rt1w_batch_variance / rt1w_denoise_var / rt1w_render_denoised_var and their device forms, include/rt1w.h): the
variance of the mean of K sample batches, and the a-trous filter whose colour term is scaled by it.  CPU tier: the CPU twins
(librt1w_lab.so: rt1w_lab_batch_variance_host, rt1w_lab_denoise_var_host, the kernels' own rt_denoise_var.h built for the host) on the
ABI surface, on inputs whose answer follows by hand, and on noisy renders at 16 and 256 spp against converged ones.  GPU tier: the kernels
bit for bit against the twins at every level and both forms of the level kernel, the one call against the composition of the public
calls, non-interference with the render entries, and full frames."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
ULP = 2.0 ** -53

# the quality cases: arm -> (width, height); the converged frames are tests/golden/denoise_ref_arm*.npy (tests/test_denoise.py writes them)
QUALITY = {5: (96, 96), 4: (128, 72), 7: (64, 64)}
BATCHES = 4  # the default of rt1w_render_denoised_var
# mse(denoised) / mse(noisy) of the displayed values, measured with the twin at the defaults (4 batches, sigma_variance 3; DESIGN.md
# section 15).  Keys: (arm, spp).  rt1w_denoise's own ratios on the same frames: 0.3037, 1.6743, 0.1388, 0.5980, 0.3469, 0.5157.
MEASURED_RATIO = {(5, 16): 0.1262, (5, 256): 0.2445, (4, 16): 0.0959, (4, 256): 0.2049, (7, 16): 0.2900, (7, 256): 0.3309}


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
    """The five entries are exported with the declared arity, rt1w_denoise_params and rt1w_abi_sizeof are what they were, and the twins
    refuse what the header says is invalid: a batch count outside 2 .. 16, an empty batch, more than 2^32 - 1 samples, an spp the batch
    count does not divide, a negative or NaN sigma_variance."""
    arity = {"rt1w_batch_variance": 11, "rt1w_batch_variance_device": 11, "rt1w_denoise_var": 8, "rt1w_denoise_var_device": 8,
             "rt1w_render_denoised_var": 9}
    lib = C.CDLL(rt.LIB_PATH)
    for name, n in arity.items():
        assert hasattr(lib, name), name
        assert len(getattr(rt._lib, name).argtypes) == n, name
    hdr = open(os.path.join(ROOT, "include", "rt1w.h")).read()
    for name, n in arity.items():
        decl = hdr[hdr.index("int " + name + "("):]
        assert decl[:decl.index(";")].count(",") + 1 == n, name
    assert rt._lib.rt1w_abi_sizeof(4) == C.sizeof(rt.DenoiseParams) == 40 and rt._lib.rt1w_abi_sizeof(5) == 0
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    lab = rt.load_lab()
    bv = lab.rt1w_lab_batch_variance_host
    bv.restype = C.c_int
    bv.argtypes = [C.c_uint32] * 5 + [C.c_void_p] * 4
    frame, aov = _flat_guides(4, 4)
    sums = np.ones((16, 4, 4, 3))
    var = np.empty((4, 4))
    assert bv(4, 4, 2, 1, 0, ptr(sums), ptr(aov), ptr(frame), ptr(var)) == 0
    assert bv(4, 4, 16, 7, 1, ptr(sums), ptr(aov), ptr(frame), ptr(var)) == 0
    for (w, h, k, n, flags) in ((4, 4, 1, 4, 0), (4, 4, 0, 4, 0), (4, 4, 17, 1, 0), (4, 4, 2, 0, 0), (4, 4, 2, 2 ** 31, 0),
                                (4, 4, 16, 2 ** 28, 0), (0, 4, 2, 1, 0), (4, 0, 2, 1, 0), (4, 4, 2, 1, 2)):
        assert bv(w, h, k, n, flags, ptr(sums), ptr(aov), ptr(frame), ptr(var)) == rt.ERR_INVALID, (w, h, k, n, flags)
    assert bv(4, 4, 15, (2 ** 32 - 1) // 15, 0, ptr(sums), ptr(aov), ptr(frame), ptr(var)) == 0  # K n = 2^32 - 1 exactly
    for i in range(4):
        args = [ptr(sums), ptr(aov), ptr(frame), ptr(var)]
        args[i] = None
        assert bv(4, 4, 2, 1, 0, *args) == rt.ERR_INVALID
    dv = lab.rt1w_lab_denoise_var_host
    dv.restype = C.c_int
    dv.argtypes = [C.POINTER(rt.DenoiseParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]
    out = np.empty_like(frame)
    ok = rt.DenoiseParams(4, 4, 0, 0, 0.0, 0.0, 0.0)
    assert dv(C.byref(ok), ptr(frame), ptr(aov), ptr(var), 0.0, ptr(out)) == 0
    assert dv(C.byref(ok), ptr(frame), ptr(aov), ptr(var), 0.5, ptr(out)) == 0
    for bad in (-1.0, -1e-300, float("nan"), float("inf")):
        assert dv(C.byref(ok), ptr(frame), ptr(aov), ptr(var), bad, ptr(out)) == rt.ERR_INVALID
    assert dv(C.byref(rt.DenoiseParams(4, 4, 9, 0, 0, 0, 0)), ptr(frame), ptr(aov), ptr(var), 0.0, ptr(out)) == rt.ERR_INVALID
    assert dv(C.byref(ok), ptr(frame), ptr(aov), None, 0.0, ptr(out)) == rt.ERR_INVALID
    # sigma_colour is ignored, not validated away: a huge one changes nothing
    a = rt.denoise_var_host(frame, aov, var, sigma_colour=1e300)
    assert np.array_equal(a, rt.denoise_var_host(frame, aov, var))
    split = lab.rt1w_lab_denoised_var_split
    split.restype = C.c_int
    split.argtypes = [C.c_uint32, C.c_uint32, C.c_double, C.POINTER(C.c_uint32 * 2)]
    kn = (C.c_uint32 * 2)()
    assert split(16, 0, 0.0, C.byref(kn)) == 0 and tuple(kn) == (4, 4)  # 0 batches = 4
    assert split(48, 16, 2.0, C.byref(kn)) == 0 and tuple(kn) == (16, 3)
    for spp, k, sv in ((18, 4, 0.0), (6, 0, 0.0), (16, 1, 0.0), (34, 17, 0.0), (16, 4, -1.0), (16, 4, float("nan"))):
        assert split(spp, k, sv, C.byref(kn)) == rt.ERR_INVALID, (spp, k, sv)
    with pytest.raises(rt.Rt1wError) as e:
        rt.batch_variance_host(np.ones((1, 4, 4, 3)), aov, 4)
    assert e.value.code == rt.ERR_INVALID
    with pytest.raises(rt.Rt1wError) as e:
        rt.denoise_var_host(frame, aov, var, sigma_variance=-2.0)
    assert e.value.code == rt.ERR_INVALID


def _batch_order_sum(sums):
    total = sums[0].copy()
    for s in sums[1:]:
        total = total + s
    return total


def test_variance_known_answers(rt):
    """KEEP_ALBEDO, grey batches of n = 4 samples whose means are chosen so that the answer follows by hand.  lum(m, m, m) = c m with
    c = (0.2126 + 0.7152) + 0.0722 within an ulp of 1, so: equal batches give exactly 0; means 1 and 3 give lbar = 2 c, deviations
    -c and +c, var = 2 c^2 / (2 * 1) = c^2; means 1, 3, 1, 3 give 4 c^2 / (4 * 3) = c^2 / 3.  Fewer than 16 roundings each: 16 * 2^-53
    relative.  frame is rt1w_resolve of the sums added in batch order, bit for bit.  A NaN batch gives var 0."""
    h, w, n = 5, 7, 4
    _, aov = _flat_guides(h, w)

    def grey(means):
        s = np.empty((len(means), h, w, 3))
        for k, m in enumerate(means):
            s[k] = m * n
        return s
    c2 = ((0.2126 + 0.7152) + 0.0722) ** 2
    for means, expect in (((2.5, 2.5), 0.0), ((0.3, 0.3, 0.3, 0.3), 0.0), ((1.0, 3.0), c2), ((1.0, 3.0, 1.0, 3.0), c2 / 3.0),
                          ((3.0, 1.0, 3.0, 1.0), c2 / 3.0)):
        sums = grey(means)
        frame, var = rt.batch_variance_host(sums, aov, n, keep_albedo=True)
        print("means", means, "var", var[0, 0], "expected", expect)
        assert np.all(np.abs(var - expect) <= 16 * ULP * expect)
        assert np.array_equal(frame, rt.resolve(_batch_order_sum(sums), len(means) * n))
    # demodulation: a grey albedo of 1/2 doubles every luminance (the division is exact), so the variance is 4 times as large
    aov[..., 0:3] = 0.5
    _, var = rt.batch_variance_host(grey((1.0, 3.0)), aov, n)
    assert np.all(np.abs(var - 4.0 * c2) <= 16 * ULP * 4.0 * c2)
    # and the albedo floor: 0, NaN and 0.001 are all taken as 0.01
    aov[..., 0:3] = 0.0
    aov[0, 0, 0:3] = np.nan
    aov[0, 1, 0:3] = 0.001
    _, var = rt.batch_variance_host(grey((1.0, 3.0)), aov, n)
    assert np.all(np.abs(var - 1e4 * c2) <= 64 * ULP * 1e4 * c2)
    # a rendered-looking case: distinct channels per batch, every pixel its own values; against the definition in numpy
    rng = np.random.default_rng(11)
    sums = rng.uniform(0.0, 8.0, (4, h, w, 3))
    aov[..., 0:3] = rng.uniform(0.005, 1.0, (h, w, 3))
    frame, var = rt.batch_variance_host(sums, aov, n)
    A = np.maximum(aov[..., 0:3], 0.01)
    lk = ((sums / n) / A) @ np.array([0.2126, 0.7152, 0.0722])
    want = ((lk - lk.mean(0)) ** 2).sum(0) / (4 * 3)
    assert np.all(np.abs(var - want) <= 1e-12 * want) and np.array_equal(frame, rt.resolve(_batch_order_sum(sums), 16))
    # not finite: the pixel has no estimate; the frame scrubs the NaN of the SUM as rt1w_resolve does
    sums[2, 1, 2, 0] = np.nan
    sums[1, 3, 4, 2] = np.inf
    frame, var2 = rt.batch_variance_host(sums, aov, n)
    assert var2[1, 2] == 0.0 and var2[3, 4] == 0.0 and frame[1, 2, 0] == 0.0 and frame[3, 4, 2] == np.inf
    var2[1, 2], var2[3, 4] = var[1, 2], var[3, 4]
    assert np.array_equal(var2, var) and np.array_equal(frame, rt.resolve(_batch_order_sum(sums), 16))


@pytest.mark.parametrize("w,h", [(1, 1), (3, 7), (257, 5), (40, 33)])
@pytest.mark.parametrize("iterations", [1, 5, 8])
@pytest.mark.parametrize("keep", [False, True])
def test_flat_image_stays_flat(rt, w, h, iterations, keep):
    """Constant colour and guides, ANY variance: where two values are equal the colour term is 0 whatever the variances, where rounding
    has parted them the tap is either taken or not, and a weighted mean of values within the bound stays within it.  A level is two
    sums of at most 25 terms and a division (about 53 roundings), 8 levels at most, demodulation two more: 512 * 2^-53 relative."""
    frame, aov = _flat_guides(h, w)
    rng = np.random.default_rng(w * 100 + h)
    wild = rng.uniform(0.0, 1.0, (h, w)) ** 8
    wild.flat[:: 5] = 0.0
    wild.flat[1:: 7] = np.nan
    wild.flat[2:: 11] = -1.0
    wild.flat[3:: 13] = np.inf
    for var in (np.zeros((h, w)), np.full((h, w), 1e-30), np.full((h, w), 1e6), wild):
        out = rt.denoise_var_host(frame, aov, var, iterations=iterations, keep_albedo=keep)
        rel = np.abs(out - frame) / frame
        assert np.all(rel <= 512 * ULP), rel.max() / ULP
    # misses: zero normal, infinite depth, zero coverage
    frame, aov = _flat_guides(h, w, normal=(0.0, 0.0, 0.0), depth=np.inf, cov=0.0)
    out = rt.denoise_var_host(frame, aov, wild, iterations=iterations, keep_albedo=keep)
    assert np.all(np.abs(out - frame) / frame <= 512 * ULP)


@pytest.mark.parametrize("iterations", [1, 5, 8])
@pytest.mark.parametrize("keep", [False, True])
def test_converged_input_comes_back(rt, iterations, keep):
    """var == 0 everywhere and pairwise distinct luminances: every tap but the centre has x_colour = d^2 / 0 = +inf, weight 0, so a level
    is c' = (w c) / w with w = 9/64 and the filter is the identity up to that rounding and the demodulation: within 2 ulp."""
    h, w = 23, 38
    rng = np.random.default_rng(5)
    frame, aov = _flat_guides(h, w)
    frame = rng.uniform(0.05, 1.0, frame.shape)
    A = np.ones(3) if keep else np.array([0.5, 0.25, 1.0])
    lum = (frame / A) @ np.array([0.2126, 0.7152, 0.0722])
    assert len(np.unique(lum)) == lum.size
    out = rt.denoise_var_host(frame, aov, np.zeros((h, w)), iterations=iterations, keep_albedo=keep)
    err = np.abs(out - frame) / np.spacing(frame)
    print("converged", iterations, keep, "max error in ulp", err.max())
    assert err.max() <= 2.0
    # the same with a variance that is not usable (negative, NaN): taken as 0
    bad = np.full((h, w), -1.0)
    bad[::2] = np.nan
    assert np.array_equal(rt.denoise_var_host(frame, aov, bad, iterations=iterations, keep_albedo=keep), out)


@pytest.mark.parametrize("kind", ["normals", "hit_miss"])
@pytest.mark.parametrize("iterations", [1, 5, 8])
def test_marked_edges_are_not_crossed(rt, kind, iterations):
    """The construction of tests/test_denoise.py: two regions whose guides give the cross-edge taps a weight of exactly 0 (perpendicular
    normals; a hit region against a miss region), colours 0 + noise on one side, 1 + noise on the other, albedo 1.  The variance is the
    noise's own (uniform on 0 .. 0.2: 0.04 / 12), and once absurdly large, which would let the colour term accept anything: every output
    pixel stays inside the closed range of its own side's inputs, widened by 512 * 2^-53 of the largest input."""
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
    slack = 512 * ULP * np.abs(frame).max()
    for v in (0.04 / 12.0, 1e12):
        out = rt.denoise_var_host(frame, aov, np.full((h, w), v), iterations=iterations)
        for side in (left, ~left):
            lo, hi = frame[side].min(), frame[side].max()
            print(kind, iterations, v, "side range", lo, hi, "output range", out[side].min(), out[side].max())
            assert out[side].min() >= lo - slack and out[side].max() <= hi + slack
        assert out[left].max() < 0.5 < out[~left].min()
        # and the filter does filter: inside a side the spread shrinks
        assert out[left].std() < 0.5 * frame[left].std()


def test_non_finite_inputs(rt):
    """A NaN pixel and an inf pixel in the frame come out as they went in and poison nobody, whatever the variance says there."""
    h, w = 24, 31
    rng = np.random.default_rng(3)
    frame, aov = _flat_guides(h, w)
    frame += rng.uniform(0.0, 0.1, frame.shape)
    frame[5, 6] = np.nan
    frame[17, 20, 1] = np.inf
    var = np.full((h, w), 0.01 / 12.0)
    var[5, 6] = 0.0        # what rt1w_batch_variance writes for such a pixel
    var[17, 20] = np.inf   # and what a careless host might
    var[11, 3] = np.nan
    for keep in (False, True):
        for it in (1, 5, 8):
            out = rt.denoise_var_host(frame, aov, var, iterations=it, keep_albedo=keep)
            assert np.all(np.isnan(out[5, 6])) and out[17, 20, 1] == np.inf
            bad = ~np.isfinite(out)
            bad[5, 6] = False
            bad[17, 20] = False
            assert not bad.any()
    # guides may be anything too: a NaN normal and a NaN depth reject, they do not spread
    aov[9, 9, 3:7] = np.nan
    frame[5, 6] = 0.3
    frame[17, 20] = 0.3
    assert np.all(np.isfinite(rt.denoise_var_host(frame, aov, var)))


def _disp(c):
    return np.sqrt(np.clip(c, 0.0, 0.999))  # the displayed value, src/color.rs:56-65 (as test_denoise.py)


def _mse(a, b):
    return float(np.mean((_disp(a) - _disp(b)) ** 2))


@functools.lru_cache(maxsize=None)
def _quality_case(arm, spp):
    """(mse of the noisy frame, of the variance-guided result, of rt1w_denoise's result) against the converged frame; computed once"""
    rt = orc.rt()
    w, h = QUALITY[arm]
    sc = rt.Scene.reference(arm, build_seed=1)
    n = spp // BATCHES
    sums = np.stack([orc.flat_render(sc, w, h, n, sample_offset=k * n, out_sum=True)[0] for k in range(BATCHES)])
    aov = rt.aov_host(sc, w, h, spp)
    ref = np.load(os.path.join(GOLD, f"denoise_ref_arm{arm}.npy"))
    frame, var = rt.batch_variance_host(sums, aov, n)
    assert ref.shape == frame.shape
    return _mse(frame, ref), _mse(rt.denoise_var_host(frame, aov, var), ref), _mse(rt.denoise_host(frame, aov), ref)


@pytest.mark.parametrize("spp", [16, 256])
@pytest.mark.parametrize("arm", sorted(QUALITY))
def test_quality_against_converged_frames(rt, arm, spp):
    """The reason for the feature.  4 batches of spp / 4 samples (global_seed 0), filtered with the defaults, against the converged frame
    (another seed), in the mean squared error of the displayed values over all pixels: (a) better than the frame it was given at 16 AND
    at 256 spp -- rt1w_denoise makes Cornell at 256 spp worse, ratio 1.67, printed for contrast; (b) by at least half of what was
    measured when the defaults were chosen; (c) at 16 spp no worse than rt1w_denoise on the same frame."""
    m_noisy, m_var, m_fixed = _quality_case(arm, spp)
    ratio, fixed = m_var / m_noisy, m_fixed / m_noisy
    print(f"arm {arm} {spp} spp: mse noisy {m_noisy:.6g} variance-guided {m_var:.6g} ratio {ratio:.4f}; rt1w_denoise ratio {fixed:.4f}")
    assert ratio < 1.0
    assert ratio <= (MEASURED_RATIO[(arm, spp)] + 1.0) / 2.0
    if spp == 16:
        assert ratio <= fixed


# ------------------------------------------------------------------------------------------------------------------ GPU tier --

def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _gpu_batches(ctx, W, H, spp, k, **kw):
    n = spp // k
    return np.stack([ctx.render(W, H, n, sample_offset=kw.get("sample_offset", 0) + b * n, out_sum=True,
                                **{a: v for a, v in kw.items() if a != "sample_offset"})[0] for b in range(k)]), n


@pytest.mark.gpu
@pytest.mark.parametrize("arm", [0, 5, 7])
def test_gpu_equals_twin_bit_for_bit(rt, gpu_ctx_factory, arm):
    """rt1w_batch_variance (frame and var) and rt1w_denoise_var == the CPU twins on rendered batches: 2 and 4 batches, both flag
    settings, every level count that crosses a boundary between the staged and the direct form of the level kernel (1, 2, 5, 8), a
    non-default sigma_variance, sizes that are not multiples of the 8 x 8 block or the 16 x 16 tile, images smaller than the largest step,
    and a frame with a NaN and an inf pixel."""
    W, H = 203, 149
    sc = rt.Scene.reference(arm, build_seed=1, aspect_ratio=W / H)
    ctx = gpu_ctx_factory(sc)
    aov = ctx.render_aov(W, H, 8)
    for k in (2, 4):
        sums, n = _gpu_batches(ctx, W, H, 8, k)
        for keep in (False, True):
            frame, var, st = ctx.batch_variance(sums, aov, n, keep_albedo=keep, with_stats=True)
            tf, tv = rt.batch_variance_host(sums, aov, n, keep_albedo=keep)
            assert _same(frame, tf) and _same(var, tv), (arm, k, keep)
            assert st["block"] == 256 and st["grid"] == ((W + 15) // 16) * ((H + 15) // 16) and st["kernel_ms"] > 0
            assert var.min() >= 0.0 and np.all(np.isfinite(var)) and var.max() > 0.0
            for it in ((1, 2, 5, 8) if k == 4 else (5,)):
                got, st = ctx.denoise_var(frame, aov, var, iterations=it, keep_albedo=keep, with_stats=True)
                assert _same(got, rt.denoise_var_host(frame, aov, var, iterations=it, keep_albedo=keep)), (arm, k, keep, it)
                assert st["passes"] == 1 and st["block"] == 256 and st["grid"] == ((W + 15) // 16) * ((H + 15) // 16) and st["kernel_ms"] > 0
    kw = dict(sigma_variance=0.7, sigma_normal=7.0, sigma_depth=0.9, iterations=4)
    assert _same(ctx.denoise_var(frame, aov, var, **kw), rt.denoise_var_host(frame, aov, var, **kw))
    assert _same(ctx.denoise_var(frame, aov, var), rt.denoise_var_host(frame, aov, var))  # all defaults
    assert not _same(ctx.denoise_var(frame, aov, var), ctx.denoise_var(frame, aov, var, sigma_variance=0.7))
    for (y0, y1, x0, x1) in ((10, 15, 20, 25), (7, 8, 0, 203), (0, 149, 100, 101), (0, 16, 0, 16), (1, 34, 2, 35)):
        s = np.ascontiguousarray(sums[:, y0:y1, x0:x1])
        f, a, v = (np.ascontiguousarray(b[y0:y1, x0:x1]) for b in (frame, aov, var))
        cf, cv = ctx.batch_variance(s, a, n, keep_albedo=True)
        assert _same(cf, f) and _same(cv, v)  # per pixel: a crop's variance is the variance's crop
        for it in (2, 8):
            assert _same(ctx.denoise_var(f, a, v, iterations=it), rt.denoise_var_host(f, a, v, iterations=it)), (arm, f.shape, it)
    if arm == 5:
        ns = sums.copy()
        ns[1, 30, 40] = np.nan
        ns[3, 80, 90, 2] = np.inf
        nf, nv = ctx.batch_variance(ns, aov, n)
        tf, tv = rt.batch_variance_host(ns, aov, n)
        assert _same(nf, tf) and _same(nv, tv) and nv[30, 40] == 0.0 and nv[80, 90] == 0.0
        nf[30, 40] = np.nan  # the frame entry scrubs a NaN sum; a frame from elsewhere may still hold one
        assert _same(ctx.denoise_var(nf, aov, nv), rt.denoise_var_host(nf, aov, nv))


class _DeviceBuffers:
    """plain device memory of the HIP runtime this process already uses"""

    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")
        self.made = []

    def alloc(self, nbytes):
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), C.c_size_t(nbytes)) == 0
        self.made.append(p)
        return p.value

    def fetch(self, p, shape):
        out = np.empty(shape)
        assert self.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(p), C.c_size_t(out.nbytes), 2) == 0  # DeviceToHost
        return out

    def free(self):
        for p in self.made:
            self.hip.hipFree(p)


@pytest.mark.gpu
@pytest.mark.parametrize("arm", [5, 7])
def test_gpu_one_call_equals_composition(rt, gpu_ctx_factory, arm):
    """rt1w_render_denoised_var == K renders with RT1W_OUT_SUM + the (deep) feature buffers + rt1w_batch_variance + rt1w_denoise_var, bit
    for bit, with max_specular 0 and 8, through the host forms and through the device forms; what it refuses."""
    W, H, spp, K = 96, 96, 8, 4
    sc = rt.Scene.reference(arm, build_seed=1, aspect_ratio=W / H)
    ctx = gpu_ctx_factory(sc)
    sums, n = _gpu_batches(ctx, W, H, spp, K, global_seed=3)
    dev = _DeviceBuffers()
    npix = W * H
    d_sums, d_aov, d_frame, d_var = dev.alloc(K * npix * 24), dev.alloc(npix * 64), dev.alloc(npix * 24), dev.alloc(npix * 8)
    for ms in (0, 8):
        aov = ctx.render_aov_deep(W, H, spp, max_specular=ms, global_seed=3)
        if ms == 0:
            assert _same(aov, ctx.render_aov(W, H, spp, global_seed=3))
        frame, var = ctx.batch_variance(sums, aov, n)
        host = ctx.denoise_var(frame, aov, var)
        one, st = ctx.render_denoised_var(W, H, spp, batches=K, max_specular=ms, global_seed=3, with_stats=True)
        assert _same(one, host), (arm, ms)
        assert st["paths"] == W * H * spp and st["passes"] >= K and st["block"] == 256 and st["kernel_ms"] > 0
        for b in range(K):
            ctx.render_device(d_sums + b * npix * 24, W, H, n, sample_offset=b * n, global_seed=3, out_sum=True)
        ctx.render_aov_deep_device(d_aov, W, H, spp, max_specular=ms, global_seed=3)
        ctx.batch_variance_device(d_sums, d_aov, d_frame, d_var, W, H, K, n)
        assert _same(dev.fetch(d_frame, (H, W, 3)), frame) and _same(dev.fetch(d_var, (H, W)), var)
        assert _same(dev.fetch(d_sums, (K, H, W, 3)), sums)  # inputs untouched
        sd = ctx.denoise_var_device(d_frame, d_aov, d_var, d_frame, W, H)  # in place
        assert sd["passes"] == 1 and sd["kernel_ms"] > 0 and sd["total_ms"] > 0
        assert _same(dev.fetch(d_frame, (H, W, 3)), host)
    dev.free()
    assert _same(ctx.render_denoised_var(W, H, spp, global_seed=3), ctx.render_denoised_var(W, H, spp, batches=4, global_seed=3))  # 0 = 4
    # other parameters, a sub-tile and a sample offset: 2 batches, keep_albedo, 3 levels, its own sigma_variance
    tile, dn = (16, 9, 70, 50), dict(iterations=3, keep_albedo=True)
    ts, tn = _gpu_batches(ctx, W, H, spp, 2, tile=tile, sample_offset=4)
    ta = ctx.render_aov(W, H, spp, tile=tile, sample_offset=4)
    tf, tv = ctx.batch_variance(ts, ta, tn, keep_albedo=True)
    assert _same(ctx.render_denoised_var(W, H, spp, batches=2, sigma_variance=1.5, tile=tile, sample_offset=4, denoise=dn),
                 ctx.denoise_var(tf, ta, tv, sigma_variance=1.5, **dn))
    for kw in (dict(batches=3), dict(batches=1), dict(batches=17), dict(sigma_variance=-1.0), dict(sigma_variance=float("nan")),
               dict(max_specular=65), dict(max_fuzz=-1.0), dict(denoise=dict(iterations=9))):
        with pytest.raises(rt.Rt1wError) as e:
            ctx.render_denoised_var(W, H, spp, **kw)
        assert e.value.code == rt.ERR_INVALID, kw
    for flags, name in ((rt.OUT_SUM, "RT1W_OUT_SUM"), (rt.OUT_FRAME, "RT1W_OUT_FRAME"), (rt.RNG_REFERENCE, "RT1W_RNG_REFERENCE"),
                        (rt.PROBE_COHERENT, "RT1W_PROBE_COHERENT")):
        with pytest.raises(rt.Rt1wError) as e:
            ctx.render_denoised_var(W, H, spp, flags=flags)
        assert e.value.code == rt.ERR_INVALID and name in str(e.value)
    with pytest.raises(rt.Rt1wError) as e:
        ctx.render_denoised_var(W, H, spp, tile=(0, 0, W, 30), strips=(10, 30))
    assert e.value.code == rt.ERR_INVALID and "strip_rows" in str(e.value)
    with pytest.raises(rt.Rt1wError) as e:
        ctx.render_denoised_var(W, H, spp, precision=1)
    assert e.value.code == rt.ERR_INVALID and "RT1W_PRECISION_F32" in str(e.value)
    with pytest.raises(rt.Rt1wError) as e:
        ctx.batch_variance(np.ones((17, 4, 4, 3)), np.ones((4, 4, 8)), 1)
    assert e.value.code == rt.ERR_INVALID and "batches" in str(e.value)
    with pytest.raises(rt.Rt1wError) as e:
        ctx.denoise_var(np.ones((4, 4, 3)), np.ones((4, 4, 8)), np.ones((4, 4)), sigma_variance=-1.0)
    assert e.value.code == rt.ERR_INVALID and "sigma_variance" in str(e.value)


@pytest.mark.gpu
def test_gpu_renders_are_unchanged_by_a_variance_denoise(rt, gpu_ctx_factory):
    """The entries share the context's framebuffer, colour buffers and stream with the render and denoise entries, and own the batch
    buffer: a beauty render, an AOV render and a fixed-sigma denoise after them equal the ones before, bit for bit, and the context
    survives the batch buffer growing (more pixels, then more batches)."""
    sc = rt.Scene.reference(5, build_seed=1)
    ctx = gpu_ctx_factory(sc)
    f0, s0 = ctx.render(90, 70, 8)
    a0 = ctx.render_aov(90, 70, 8)
    d0 = ctx.render_denoised(90, 70, 8)
    v0 = ctx.render_denoised_var(90, 70, 8)
    ctx.render_denoised_var(200, 150, 4, batches=2)   # larger than anything so far: every buffer grows
    ctx.render_denoised_var(200, 150, 16, batches=16)  # and the batch buffer once more
    ctx.batch_variance(np.ones((16, 160, 300, 3)), np.ones((160, 300, 8)), 1)
    ctx.denoise_var(np.ones((200, 300, 3)), np.ones((200, 300, 8)), np.ones((200, 300)))
    f1, s1 = ctx.render(90, 70, 8)
    a1 = ctx.render_aov(90, 70, 8)
    assert _same(f0, f1) and _same(a0, a1) and s0["segments"] == s1["segments"]
    assert _same(d0, ctx.render_denoised(90, 70, 8)) and _same(v0, ctx.render_denoised_var(90, 70, 8))


@pytest.mark.gpu
@pytest.mark.parametrize("arm,size", [(5, 600), (7, 800)])
def test_gpu_full_frames(rt, gpu_ctx_factory, arm, size):
    """render_denoised_var of C3 (Cornell 600 x 600 x 16) and C4 (final_scene 800 x 800 x 16) with 4 batches: finite, and equal to the
    twins run over the same batch sums and feature buffers on 4096 seeded pixels plus the four corners."""
    sc = rt.Scene.reference(arm, build_seed=1)
    ctx = gpu_ctx_factory(sc)
    out, st = ctx.render_denoised_var(size, size, 16, batches=4, with_stats=True)
    assert out.shape == (size, size, 3) and np.all(np.isfinite(out))
    sums, n = _gpu_batches(ctx, size, size, 16, 4)
    aov = ctx.render_aov(size, size, 16)
    frame, var = rt.batch_variance_host(sums, aov, n)
    twin = rt.denoise_var_host(frame, aov, var)
    rng = np.random.default_rng(2017)
    ys = np.concatenate([rng.integers(0, size, 4096), [0, 0, size - 1, size - 1]])
    xs = np.concatenate([rng.integers(0, size, 4096), [0, size - 1, 0, size - 1]])
    assert _same(np.ascontiguousarray(out[ys, xs]), np.ascontiguousarray(twin[ys, xs]))
    _, sb = ctx.render(size, size, 16)
    _, _, sv = ctx.batch_variance(sums, aov, n, with_stats=True)
    _, sd = ctx.denoise_var(frame, aov, var, with_stats=True)
    print(f"arm {arm} {size}x{size}x16: render_denoised_var kernels {st['kernel_ms']:.2f} ms (beauty alone {sb['kernel_ms']:.2f}, variance pass "
          f"{sv['kernel_ms']:.3f}, filter {sd['kernel_ms']:.2f}), total {st['total_ms']:.2f} ms")
