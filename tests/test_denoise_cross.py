"""Cross-filtered half buffers (rt1w_denoise_cross, rt1w_denoise_cross_device, rt1w_render_adaptive_cross, include/rt1w.h).  CPU tier: the
CPU twin (librt1w_lab.so: rt1w_lab_denoise_cross_host) against the long-double statement tests/dn_cross_reference.py, the degenerate identity
that ties it to rt1w_denoise_var_halves, the refusals, the calibration of the error map, the quality of the filter alone and of the whole
plan composed in Python.  GPU tier: the kernels bit for bit against the twin, host against device form, the one call against the composition
of the public device entries.  The plan, the device buffers and the quality denominators are tests/test_adaptive_filtered.py's."""
import ctypes as C
import functools
import json
import os
import sys

import numpy as np
import pytest

import orc
import dn_cross_reference as XR
import test_adaptive_filtered as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
REFUSALS = os.path.join(GOLD, "denoise_cross_refusals.json")
LUM = TF.LUM
_same = TF._same

# frame mean of err_px x its denominator over the seed-to-seed variance of the filtered frame's luminance (test_calibration); the shared
# weights of rt1w_denoise_var_halves measure 0.205 by the same protocol.  A NEGATIVE result: the cross weights do not bring the ratio towards
# 1 (estimate 0.00313, truth 0.0189: the frame filtered with weights from half the samples varies more from seed to seed, and the estimate
# does not follow).  With sigma_variance = 1e6 (guides only) both filters are the same and measure MEASURED_CALIBRATION_GUIDES: the guides,
# rendered per seed and common to both halves, are a cause no choice of colour term removes
MEASURED_CALIBRATION_CROSS = 0.166
MEASURED_CALIBRATION_GUIDES = 0.561
# mse(out) / mse(noisy frame), displayed values, the filter alone on uniform 4 batches dealt into halves; keys (arm, spp).  rt1w_denoise_var
# on the same samples: tests/test_denoise_var.py's MEASURED_RATIO
MEASURED_FILTER_RATIO = {(5, 16): 0.1760, (5, 256): 0.2968, (4, 16): 0.1131, (4, 256): 0.2382, (7, 16): 0.2804, (7, 256): 0.3651}
# mse(rt1w_render_adaptive_cross's frame) / mse(uniform 4 batches + rt1w_batch_variance + rt1w_denoise_var), the cases and denominators of
# tests/test_adaptive_filtered.py's MEASURED_RATIO
# A NEGATIVE result as well: every case is above 1 (geometric mean 1.120 against the shared weights' 0.947)
MEASURED_RATIO_CROSS = {(5, 32): 1.0679, (5, 128): 1.1421, (4, 32): 1.0847, (4, 128): 1.0745, (7, 32): 1.2633, (7, 128): 1.1010}


# ------------------------------------------------------------------------------------------------------------------ CPU tier --

def _synthetic():
    """31 x 24 with every edge the definition names; (frame, aov, var, half_a, half_b)"""
    h, w = 24, 31
    rng = np.random.default_rng(41)
    aov = TF._guides(h, w, rng)
    aov[..., 6] = 3.0 + 0.01 * np.arange(w)[None, :]            # a gentle slope: depth weights strictly between 0 and 1
    aov[:, 20:, 6] += 4.0                                       # a depth step
    aov[0:6, 0:8, 3:6] = 0.0
    aov[0:6, 0:8, 6] = np.inf                                   # misses against hits
    aov[12:, 0:10, 3:6] = (1.0, 0.0, 0.0)                       # perpendicular to (0, 0.6, 0.8)
    aov[8:12, 12:16, 7] = 0.5                                   # a coverage step
    a = rng.uniform(0.2, 2.0, (h, w, 3))
    b = rng.uniform(0.2, 2.0, (h, w, 3))
    var = rng.uniform(0.02, 0.3, (h, w))
    flat = (slice(16, 22), slice(22, 29))                       # la_p == la_q with va = 0: constant demodulated halves, no variance
    A = np.maximum(aov[..., 0:3], 0.01)
    a[flat] = 0.5 * A[flat]
    b[flat] = 0.25 * A[flat]                                    # powers of two: the quotients are exact
    var[flat] = 0.0
    a[5, 15, 1] = np.nan                                        # a NaN centre in one half only
    b[9, 25, 0] = np.inf                                        # an inf tap
    var[3, 20] = -1.0
    var[4, 21] = np.nan
    frame = (a + b) * 0.5
    frame[5, 15] = (a[5, 15, 0], 0.3, a[5, 15, 2])              # the frame itself is finite there
    frame[9, 25] = 1.0
    return frame, aov, var, a, b


def _against_statement(rt, bufs, kw, need):
    frame, aov, var, ha, hb = bufs
    out, err, rec = rt.denoise_cross_host(frame, aov, var, ha, hb, with_record=True, **kw)
    w_out, wa, wb, we, undecidable = XR.denoise_cross(frame, aov, var, ha, hb, **kw)
    A = np.ones(3) if kw.get("keep_albedo") else np.where(np.isfinite(aov[..., 0:3]) & (aov[..., 0:3] > 0.01), aov[..., 0:3], 0.01)
    with np.errstate(all="ignore"):
        fa, fb = rec[..., 0:3] * A, rec[..., 5:8] * A
        la, lb = fa @ LUM, fb @ LUM
        fin = np.isfinite(fa).all(-1) & np.isfinite(fb).all(-1) & np.isfinite(out).all(-1) & ~undecidable
        for x in (wa, wb, w_out):
            fin &= np.isfinite(np.asarray(x, dtype=np.float64)).all(-1)

        def rel(got, want):
            floor = np.maximum(np.abs(want[fin]).max(-1, keepdims=True) * 1e-3, 1e-300)
            return float((np.abs(got - want)[fin] / np.maximum(np.abs(want[fin]), floor)).max())
        cond = fin & (np.abs(la - lb) >= 0.05 * 0.5 * np.abs(la + lb)) & (la != lb)
        re = float((np.abs(err - we)[cond] / we[cond]).max())
        # the pixels the statement itself passes through or finds not finite: the twin agrees on which they are
        assert np.array_equal(np.isfinite(out).all(-1), np.isfinite(np.asarray(w_out, dtype=np.float64)).all(-1))
        ra, rb, ro = rel(fa, wa), rel(fb, wb), rel(out, w_out)
    print("pixels", int(fin.sum()), "conditioned", int(cond.sum()), "a'", ra, "b'", rb, "out", ro, "err_px", re)
    assert cond.sum() >= need and fin.sum() >= need
    assert ra <= 1e-12 and rb <= 1e-12 and ro <= 1e-12 and re <= 1e-12
    return out, err, rec


def test_twin_against_the_independent_statement(rt):
    """rt1w_lab_denoise_cross_host against tests/dn_cross_reference.py (long double, exp and **) within 1e-12 relative -- a', b', out, and
    err_px where |lum a' - lum b'| is at least 0.05 of their mean (the difference of two nearly equal luminances has no relative accuracy) --
    on a synthetic image with a miss against hits, perpendicular normals, a depth step, la_p == la_q with va = 0, a NaN centre in one half
    only, an inf tap, negative and NaN var; at 1, 2 and 5 levels, both flag settings and a second sigma_variance; and on rendered halves."""
    syn = _synthetic()
    for kw in ({}, dict(iterations=1), dict(iterations=2, keep_albedo=True), dict(sigma_variance=1.25, iterations=3)):
        out, err, rec = _against_statement(rt, syn, kw, 300)
        assert np.all(err >= 0.0) and np.all(np.isfinite(err))
        # the NaN centre passes its whole record through: half A not finite there, half B's value untouched
        assert np.isnan(rec[5, 15, 1]) and np.isnan(rec[5, 15, 3]) and np.isnan(out[5, 15, 1]) and err[5, 15] == 0.0
        A = np.ones(3) if kw.get("keep_albedo") else np.maximum(syn[1][5, 15, 0:3], 0.01)
        assert _same(rec[5, 15, 5:8], syn[4][5, 15] / A)
        assert np.isinf(rec[9, 25, 5]) and np.all(np.isfinite(rec[9, 24])) and np.all(np.isfinite(rec[10, 25]))   # the inf tap is taken by nobody
        if kw.get("iterations") == 1:   # la_p == la_q with va = 0: two rings inside the flat region every tap is kept and the values stay, exactly
            assert np.all(rec[18:20, 24:27, 0:3] == 0.5) and np.all(rec[18:20, 24:27, 5:8] == 0.25) and np.all(err[18:20, 24:27] > 0.0)
            assert not rec[18:20, 24:27, 4].any() and not rec[18:20, 24:27, 9].any()
    _against_statement(rt, TF._rendered(5), {}, 500)
    _against_statement(rt, TF._rendered(7), dict(iterations=2), 500)


def test_frame_is_read_for_its_finiteness_only(rt):
    """`frame` gives no value: another finite frame gives the same bits.  Where frame / A_p has no finite luminance the pixel is passed
    through and no neighbour takes it, whatever the halves hold there."""
    frame, aov, var, ha, hb = TF._rendered(5)
    want = rt.denoise_cross_host(frame, aov, var, ha, hb, with_record=True)
    got = rt.denoise_cross_host(frame * 3.0 + 1.0, aov, var, ha, hb, with_record=True)
    assert all(_same(g, t) for g, t in zip(got, want))
    f2 = frame.copy()
    f2[20, 24, 1] = np.inf
    out, err, rec = rt.denoise_cross_host(f2, aov, var, ha, hb, with_record=True, iterations=1)
    A = np.maximum(aov[20, 24, 0:3], 0.01)
    assert _same(rec[20, 24, 0:3], ha[20, 24] / A) and _same(rec[20, 24, 5:8], hb[20, 24] / A) and np.isinf(rec[20, 24, 3]) and np.isinf(rec[20, 24, 8])
    base = rt.denoise_cross_host(frame, aov, var, ha, hb, iterations=1)[0]
    near = np.zeros(base.shape[:2], dtype=bool)
    near[18:23, 22:27] = True
    assert _same(out[~near], base[~near]) and np.all(np.isfinite(out[near]))


def test_degenerate_identity(rt):
    """What ties the new text to the old.  With half_a == half_b == frame, bit for bit: each half's level record (a', la') is
    rt1w_lab_denoise_var_halves_host's (r, g, b, l) of that frame -- given half_a = half_b = frame and the variance buffer 2 var -- and
    err_px is exactly 0 wherever it is finite (it always is: a value that is not finite is written as 0)."""
    cases = [(TF._rendered(5), {}), (TF._rendered(7), dict(iterations=3)), (TF._rendered(5), dict(iterations=2, keep_albedo=True)),
             (TF._hostile(np.random.default_rng(5)), {}), (TF._hostile(np.random.default_rng(6)), dict(keep_albedo=True, iterations=3)),
             (TF._rendered(7), dict(sigma_variance=1.5))]
    for i, ((frame, aov, var, _, _), kw) in enumerate(cases):
        var = np.where(var > 1e300, 0.0, var)
        out, err, rec = rt.denoise_cross_host(frame, aov, var, frame, frame, with_record=True, **kw)
        h_out, h_err, h_a, h_b = rt.denoise_var_halves_host(frame, aov, 2.0 * var, frame, frame, with_halves=True, **kw)
        assert not err.any() and not np.signbit(err).any(), i
        assert _same(rec[..., 0:5], rec[..., 5:10]), i
        A = np.ones(3) if kw.get("keep_albedo") else np.where(np.isfinite(aov[..., 0:3]) & (aov[..., 0:3] > 0.01), aov[..., 0:3], 0.01)
        with np.errstate(all="ignore"):
            assert _same(rec[..., 0:3] * A, h_out) and _same(rec[..., 0:3] * A, h_a), i      # the same products rt_dv_finish_pixel takes
            l = (0.2126 * rec[..., 0] + 0.7152 * rec[..., 1]) + 0.0722 * rec[..., 2]
        through = ~np.isfinite(rec[..., 3])                     # a centre passed through keeps the luminance the prepare pass gave it
        assert _same(rec[..., 3][~through], l[~through]), i
        if kw.get("keep_albedo"):
            assert _same(rec[..., 0:3], h_out), i               # A = 1: the record itself


DENOISE = dict(width=32, height=32, iterations=2, flags=0, sigma_colour=0.0, sigma_normal=0.0, sigma_depth=0.0)
NAN, INF = float("nan"), float("inf")
# the checks in the order the entries make them (rt1w_denoise_var_halves's): (case, members of p, other arguments)
CHAIN = [("null context", {}, dict(ctx=None)), ("null params", None, {}), ("width 0", dict(width=0), {}), ("iterations 9", dict(iterations=9), {}),
         ("unknown denoise flag", dict(flags=2), {}), ("sigma NaN", dict(sigma_colour=NAN), {}), ("sigma_variance NaN", {}, dict(sigma_variance=NAN)),
         ("null frame", {}, dict(frame=None))]
MORE = [("height 0", dict(height=0), {}), ("sigma negative", dict(sigma_colour=-1.0), {}), ("sigma infinite", dict(sigma_colour=INF), {}),
        ("sigma_normal NaN", dict(sigma_normal=NAN), {}), ("sigma_depth NaN", dict(sigma_depth=NAN), {}),
        ("sigma_variance negative", {}, dict(sigma_variance=-1.0)), ("sigma_variance infinite", {}, dict(sigma_variance=INF))] + \
       [("null " + k, {}, {k: None}) for k in ("aov", "var", "half_a", "half_b", "out", "err_px")]
ORDER = ("ctx", "p", "frame", "aov", "var", "half_a", "half_b", "sigma_variance", "out", "err_px", "stats")


def _cases():
    """the singles, then the pairs of neighbours in the chain: the text of a pair is its first defect's, which pins the order"""
    pairs = []
    for (n1, p1, a1), (n2, p2, a2) in zip(CHAIN, CHAIN[1:]):
        pairs.append((f"{n1} + {n2}", None if p1 is None or p2 is None else dict(p1, **p2), dict(a1, **a2)))
    return CHAIN + MORE + pairs


def _call(rt, fn_name, ctx_handle, pm, am, buf):
    a = dict(ctx=ctx_handle, sigma_variance=0.0, stats=None, **{k: buf.ctypes.data for k in ("frame", "aov", "var", "half_a", "half_b", "out", "err_px")})
    a.update(am)
    p = None if pm is None else rt.DenoiseParams(**dict(DENOISE, **pm))
    a["p"] = None if p is None else C.byref(p)
    rc = getattr(rt._lib, fn_name)(*[a[k] for k in ORDER])
    return [int(rc), rt.last_error() if rc < 0 else ""]


def _refusals(rt, ctx_handle, entries=("rt1w_denoise_cross", "rt1w_denoise_cross_device")):
    """no case gets as far as following a pointer: the device form takes the same host buffer"""
    buf = np.zeros(32 * 32 * 8)
    return {e: [[name] + _call(rt, e, ctx_handle, pm, am, buf) for name, pm, am in _cases()] for e in entries}


def test_refusals_without_a_context_and_of_the_twin(rt):
    """The recording tests/golden/denoise_cross_refusals.json (`python tests/test_denoise_cross.py --record` on a GPU) holds code, text and
    order of what the two entries refuse: rt1w_denoise_var_halves's checks.  Without a GPU: the recording's cases are this file's and all
    refused with RT1W_ERR_INVALID; every case whose first defect needs no context to be seen (null context, null params) answers as
    recorded; the ABI surface; and the twin refuses every case the entries refuse for its parameters or buffers."""
    want = json.load(open(REFUSALS))
    names = [n for n, _, _ in _cases()]
    assert sorted(want) == ["rt1w_denoise_cross", "rt1w_denoise_cross_device"]
    for e, cs in want.items():
        assert [c[0] for c in cs] == names, "the recording's cases are not the cases of this file: record again"
        assert all(c[1] == rt.ERR_INVALID and c[2] for c in cs), e
        assert cs == want["rt1w_denoise_cross"], "host and device form refuse alike"
    got = _refusals(rt, None)
    for e in want:
        for g, w_ in zip(got[e], want[e]):
            assert g[1] == rt.ERR_INVALID, g
            if g[0].startswith("null context") or g[0].startswith("null params"):
                assert g == w_, (e, g, w_)
    lib = C.CDLL(rt.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "rt1w.h")).read()
    for name, n in {"rt1w_denoise_cross": 11, "rt1w_denoise_cross_device": 11, "rt1w_render_adaptive_cross": 9}.items():
        assert hasattr(lib, name) and len(getattr(rt._lib, name).argtypes) == n, name
        decl = hdr[hdr.index("int " + name + "("):]
        assert decl[:decl.index(";")].count(",") + 1 == n, name
    z3, z1, g = np.zeros((4, 6, 3)), np.zeros((4, 6)), TF._guides(4, 6)
    rt.denoise_cross_host(z3, g, z1, z3, z3)
    for _, pm, am in CHAIN[2:7] + MORE[:7]:
        kw = {k: v for k, v in (pm or {}).items() if k in ("iterations", "sigma_colour", "sigma_normal", "sigma_depth")}
        if "flags" in (pm or {}) or "width" in (pm or {}) or "height" in (pm or {}):
            continue                                            # the binding derives them from the buffers: through ctypes below
        with pytest.raises(rt.Rt1wError):
            rt.denoise_cross_host(z3, g, z1, z3, z3, sigma_variance=am.get("sigma_variance", 0.0), **kw)
    fn = rt.load_lab().rt1w_lab_denoise_cross_host
    buf = np.zeros(32 * 32 * 10)
    ptr = buf.ctypes.data_as(C.c_void_p)
    for name, pm, am in _cases():
        if "ctx" in am and len(am) == 1 and pm == {}:
            continue                                            # the twin has no context
        p = None if pm is None else rt.DenoiseParams(**dict(DENOISE, **pm))
        args = [None if am.get(k, 1) is None else ptr for k in ("frame", "aov", "var", "half_a", "half_b")]
        tail = [None if am.get(k, 1) is None else ptr for k in ("out", "err_px")]
        rc = fn(None if p is None else C.byref(p), *args, C.c_double(am.get("sigma_variance", 0.0)), *tail, None)
        assert rc == rt.ERR_INVALID, name
    # rt1w_render_adaptive_cross: rt1w_render_adaptive_filtered's refusals, in its order, under its own name
    filt = json.load(open(TF.REFUSALS))
    rgb = np.zeros((32, 32, 3))
    for name, pm, am, sv in TF.REFUSAL_CASES:
        p = rt.RenderParams()
        for k, v in dict(TF.RENDER, **pm).items():
            setattr(p, k, v)
        a = rt.adaptive_params(**dict(TF.ADAPTIVE, **am))
        rc = rt._lib.rt1w_render_adaptive_cross(None, C.byref(p), C.byref(a), None, sv, rgb.ctypes.data_as(C.c_void_p), None, None, None)
        assert [rc, rt.last_error()] == [filt[name][0], filt[name][1].replace("rt1w_render_adaptive_filtered", "rt1w_render_adaptive_cross")], name


def _calibration(rt, sigma_variance):
    """the protocol of tests/test_adaptive_filtered.py::test_calibration with rt1w_lab_denoise_cross_host: (estimate, truth, ratio)"""
    est, lums = [], []
    for g in range(24):
        frame, aov, var, ha, hb = _calibration_halves(g)
        out, err = rt.denoise_cross_host(frame, aov, var, ha, hb, sigma_variance=sigma_variance)
        lo = out @ LUM
        est.append(float(np.mean(err * (np.maximum(lo, 0.0) + 0.01))))
        lums.append(lo)
    truth = float(np.mean(np.var(np.stack(lums), axis=0, ddof=1)))
    return float(np.mean(est)), truth, float(np.mean(est)) / truth


@functools.lru_cache(maxsize=None)
def _calibration_halves(g):
    rt = orc.rt()
    W = H = 40
    n = 4
    sc = rt.Scene.reference(5, build_seed=1)
    aov = rt.aov_host(sc, W, H, 4 * n, global_seed=g)
    acc = [np.zeros((H, W, 8)), np.zeros((H, W, 8))]
    for b in range(4):
        acc[b & 1] = rt.accum_merge_host(acc[b & 1], orc.flat_render(sc, W, H, n, sample_offset=b * n, out_sum=True, global_seed=g)[0], aov, n)
    frame, var, ha, hb, _ = rt.halves_resolve_host(acc[0], acc[1], n)
    return frame, aov, var, ha, hb


def test_calibration(rt):
    """The protocol of tests/test_adaptive_filtered.py::test_calibration, unchanged -- Cornell 40 x 40, 2 pairs of 4 samples, 24
    global_seeds; estimate = the frame mean of err_px x its denominator; truth = the seed-to-seed variance of lum(out) -- with
    rt1w_lab_denoise_cross_host in place of rt1w_lab_denoise_var_halves_host.  MEASURED_CALIBRATION_CROSS against the shared weights' 0.205;
    the guides-only figure (sigma_variance = 1e6) locates what remains: the guides are rendered per seed and are common to both halves.
    One squared difference per pixel is a one-degree-of-freedom estimate: a factor 2 of the measurement either way, the existing rule."""
    est, truth, ratio = _calibration(rt, 0.0)
    print(f"cross: estimate {est:.6g} truth {truth:.6g} ratio {ratio:.4f} (measured {MEASURED_CALIBRATION_CROSS}; shared weights {TF.MEASURED_CALIBRATION})")
    ge, gt, gr = _calibration(rt, 1e6)
    print(f"guides only: estimate {ge:.6g} truth {gt:.6g} ratio {gr:.4f} (measured {MEASURED_CALIBRATION_GUIDES})")
    assert MEASURED_CALIBRATION_CROSS / 2.0 <= ratio <= MEASURED_CALIBRATION_CROSS * 2.0
    assert MEASURED_CALIBRATION_GUIDES / 2.0 <= gr <= MEASURED_CALIBRATION_GUIDES * 2.0


@functools.lru_cache(maxsize=None)
def _filter_case(arm, spp):
    """(mse of the noisy frame, of rt1w_denoise_cross's out, of rt1w_denoise_var's) against the converged frame: uniform 4 batches of
    spp / 4 samples, global_seed 0, batches 0 and 2 into A, 1 and 3 into B"""
    rt = orc.rt()
    w, h = TF.QUALITY[arm]
    sc = rt.Scene.reference(arm, build_seed=1)
    n = spp // 4
    aov = rt.aov_host(sc, w, h, spp)
    acc = [np.zeros((h, w, 8)), np.zeros((h, w, 8))]
    for b in range(4):
        acc[b & 1] = rt.accum_merge_host(acc[b & 1], orc.flat_render(sc, w, h, n, sample_offset=b * n, out_sum=True)[0], aov, n)
    frame, var, ha, hb, _ = rt.halves_resolve_host(acc[0], acc[1], n)
    ref = np.load(os.path.join(GOLD, f"denoise_ref_arm{arm}.npy"))
    return TF._mse(frame, ref), TF._mse(rt.denoise_cross_host(frame, aov, var, ha, hb)[0], ref), TF._mse(rt.denoise_var_host(frame, aov, var), ref)


@pytest.mark.parametrize("spp", [16, 256])
@pytest.mark.parametrize("arm", sorted(TF.QUALITY))
def test_filter_quality_against_converged_frames(rt, arm, spp):
    """The filter alone on the three frames of tests/test_denoise.py: mse(displayed out) / mse(displayed noisy frame) against the converged
    frame.  By the project's rule: below 1, and at or below the midpoint between the measurement and 1.  rt1w_denoise_var on the same
    frame and variance is printed beside it (DESIGN.md section 18 has the table)."""
    m_noisy, m_cross, m_var = _filter_case(arm, spp)
    ratio, measured = m_cross / m_noisy, MEASURED_FILTER_RATIO[(arm, spp)]
    print(f"arm {arm} {spp} spp: mse noisy {m_noisy:.6g} cross {m_cross:.6g} ratio {ratio:.4f} (measured {measured}); rt1w_denoise_var ratio {m_var / m_noisy:.4f}")
    assert ratio < 1.0
    assert ratio <= (measured + 1.0) / 2.0


def _compose_cpu(rt, sc, W, H, ad, check=None):
    """tests/test_adaptive_filtered.py's plan over the twins, with rt1w_lab_denoise_cross_host as its filter"""
    n, P = ad["batch_spp"], ad["pilot_batches"]
    chunk = sc.default_chunk(W, H, n)
    aov = rt.aov_host(sc, W, H, P * n)

    def render(rects):
        return [orc.flat_render(sc, W, H, n, tile=r, sample_offset=off, out_sum=True, chunk=chunk)[0] for r, off in rects]

    def merge(acc, sums, n, x0, y0):
        return rt.accum_merge_host(acc, sums, aov, n, x0=x0, y0=y0)
    return TF._compose(rt, W, H, ad, aov, render, merge, rt.halves_resolve_host, rt.denoise_cross_host, rt.tile_error_map_host, check) + (aov,)


def test_the_loop_is_what_it_says(rt):
    """The plan of rt1w_render_adaptive_filtered composed in Python from the twins with the cross filter in step 3, Cornell 64 x 64: budget
    and max_spp hold, counts are multiples of 2 n, m_A == m_B at every estimate, it adapts over more than one round, and the output is the
    LAST round's estimate -- rt1w_lab_denoise_cross_host of the final halves' resolve, frame and error map -- not rt1w_denoise_var's bits."""
    W = H = 64
    ad = TF.LOOP
    n = ad["batch_spp"]
    sc = rt.Scene.reference(5, build_seed=1)
    seen = []

    def check(acc, m, spp):
        assert np.array_equal(acc[0][..., 3], acc[1][..., 3])
        seen.append((acc[0].copy(), acc[1].copy()))
    out, spp, err_px, m, rounds, launches, aov = _compose_cpu(rt, sc, W, H, ad, check=check)
    print("rounds", rounds, "launches", launches, "pairs per tile", np.unique(m, return_counts=True))
    assert rounds >= 2 and launches == 2 + rounds and m.max() > m.min() and len(seen) == rounds + 1
    assert spp.sum() <= ad["budget_spp"] * W * H and spp.max() <= 16 and spp.min() >= 4 and np.all(spp % (2 * n) == 0)
    assert np.array_equal(spp, np.repeat(np.repeat(m, 16, axis=0), 16, axis=1)[:H, :W] * 2 * n)
    frame, var, ha, hb, s2 = rt.halves_resolve_host(*seen[-1], n)
    w_out, w_err = rt.denoise_cross_host(frame, aov, var, ha, hb)
    assert _same(out, w_out) and _same(err_px, w_err) and _same(spp, s2) and err_px.max() > 0.0
    assert not _same(out, rt.denoise_var_host(frame, aov, var))


def quality_case(arm, budget):
    """tests/test_adaptive_filtered.py's quality_case with the cross filter: (mse of the call's frame, of the uniform filtered frame, spp, rounds)"""
    rt = orc.rt()
    W, H = TF.QUALITY[arm]
    sc = rt.Scene.reference(arm, build_seed=1)
    ref = np.load(os.path.join(GOLD, f"denoise_ref_arm{arm}.npy"))
    n = max(1, budget // 8)
    ad = dict(tile=16, batch_spp=n, pilot_batches=4, budget_spp=budget, max_spp=8 * budget)
    out, spp, err_px, m, rounds, launches, aov = _compose_cpu(rt, sc, W, H, ad)
    assert spp.sum() <= budget * W * H
    return TF._mse(out, ref), TF._uniform_filtered_mse(arm, budget), float(spp.mean()), rounds


@pytest.mark.parametrize("budget", [32, 128])
@pytest.mark.parametrize("arm", sorted(TF.QUALITY))
def test_quality_against_converged_frames(rt, arm, budget):
    """The six cases of tests/test_adaptive_filtered.py::test_quality_against_converged_frames with the same denominators (uniform 4 batches
    + rt1w_batch_variance + rt1w_denoise_var at `budget` samples) and the same two-sided rule: where it measured better than uniform it
    keeps at least half of that, elsewhere it does not get worse than 1.1 x the measurement (DESIGN.md section 18 has the table)."""
    m_ad, m_un, mean_spp, rounds = quality_case(arm, budget)
    ratio, measured = m_ad / m_un, MEASURED_RATIO_CROSS[(arm, budget)]
    print(f"arm {arm} budget {budget}: mse cross adaptive {m_ad:.6g} uniform filtered {m_un:.6g} ratio {ratio:.4f} (measured {measured}; shared weights "
          f"{TF.MEASURED_RATIO[(arm, budget)]}); spent {mean_spp:.2f} per pixel in {rounds} rounds")
    if measured < 1.0:
        assert ratio <= (measured + 1.0) / 2.0
    else:
        assert ratio <= 1.1 * measured


# ------------------------------------------------------------------------------------------------------------------ GPU tier --

def _check_device(rt, ctx, dev, frame, aov, var, ha, hb, all_forms=False, **kw):
    """the device form == the twin, bit for bit, out and err_px; all_forms: also the host form and the device form in place"""
    H, W = var.shape
    t_out, t_err = rt.denoise_cross_host(frame, aov, var, ha, hb, **kw)
    d = [dev.put(x) for x in (frame, aov, var, ha, hb)]
    d_out, d_err = dev.alloc(frame.nbytes), dev.alloc(var.nbytes)
    st = ctx.denoise_cross_device(*d, d_out, d_err, W, H, **kw)
    assert _same(dev.fetch(d_out, frame.shape), t_out) and _same(dev.fetch(d_err, var.shape), t_err), kw
    assert st["block"] == 256 and st["grid"] == ((W + 15) // 16) * ((H + 15) // 16) and st["kernel_ms"] > 0 and st["passes"] == 1
    if all_forms:
        out, err, sh = ctx.denoise_cross(frame, aov, var, ha, hb, with_stats=True, **kw)
        assert _same(out, t_out) and _same(err, t_err) and sh["grid"] == st["grid"] and sh["block"] == 256   # host form == device form
        ctx.denoise_cross_device(*d, d[0], d_err, W, H, **kw)                                              # d_out == d_frame
        assert _same(dev.fetch(d[0], frame.shape), t_out) and _same(dev.fetch(d_err, var.shape), t_err)
    return t_out, t_err


@pytest.mark.gpu
@pytest.mark.parametrize("arm", [5, 7])
def test_gpu_kernels_equal_twin(rt, gpu_ctx_factory, arm):
    """rt1w_denoise_cross == the CPU twin bit for bit, out and err_px, on halves made through the GPU entries at 203 x 149 (no multiple of 8
    or 16; with 5 levels step 16 leaves the image on both axes): 1, 2 and 5 levels (one staged, both staged, staged and direct), both flag
    settings, a second sigma_variance; host form, device form and the device form in place."""
    W, H, n = TF.W_GPU, TF.H_GPU, 2
    sc = rt.Scene.reference(arm, build_seed=1, aspect_ratio=W / H)
    ctx = gpu_ctx_factory(sc)
    dev = TF._DeviceBuffers()
    try:
        a, b, aov = TF._gpu_halves(rt, ctx, sc, W, H, n, 4)
        frame, var, ha, hb, _ = ctx.halves_resolve(a, b, n)
        out, err = _check_device(rt, ctx, dev, frame, aov, var, ha, hb, all_forms=True)
        assert err.max() > 0.0 and not _same(out, rt.denoise_var_host(frame, aov, var))
        for kw in (dict(iterations=1), dict(iterations=2), dict(iterations=2, keep_albedo=True), dict(keep_albedo=True), dict(sigma_variance=1.5)):
            _check_device(rt, ctx, dev, frame, aov, var, ha, hb, **kw)
    finally:
        dev.free()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(5, 5), (1, 300), (300, 1), (37, 21)])
def test_gpu_small_and_hostile(rt, gpu_ctx_factory, shape):
    """(width, height) down to one column and one row, and 37 x 21, where a staged halo crosses an image edge and a workgroup edge at once.
    NaN, inf, negative and NaN var at a tile corner (15, 15), (16, 16) and on the halo ring (17, 17), (18, 14), clamped into the image; then an
    empty half (half_b all zero).  Result == the twin bit for bit, all forms, out aliasing frame."""
    w, h = shape
    ctx = gpu_ctx_factory(rt.Scene.reference(5, build_seed=1))
    dev = TF._DeviceBuffers()
    rng = np.random.default_rng(1000 * w + h)
    try:
        aov = TF._guides(h, w, rng)
        aov[..., 3:6] = rng.normal(size=(h, w, 3))
        aov[..., 6] = rng.uniform(1.0, 9.0, (h, w))
        ha, hb = rng.uniform(0.0, 2.0, (h, w, 3)), rng.uniform(0.0, 2.0, (h, w, 3))
        var = rng.uniform(0.0, 0.3, (h, w))
        at = lambda x, y: (min(y, h - 1), min(x, w - 1))
        frame = (ha + hb) * 0.5
        ha[at(15, 15)] = np.nan
        hb[at(16, 16)][1] = np.inf
        frame[at(17, 17)] = np.inf
        var[at(18, 14)] = -1.0
        var[at(14, 18)] = np.nan
        aov[at(16, 15)][6] = np.inf
        aov[at(16, 15)][3:6] = 0.0
        for kw in ({}, dict(iterations=2, keep_albedo=True)):
            _check_device(rt, ctx, dev, frame, aov, var, ha, hb, all_forms=True, **kw)
        _check_device(rt, ctx, dev, frame, aov, var, ha, np.zeros_like(hb), all_forms=True)
    finally:
        dev.free()


class _CrossContext:
    """a context whose rt1w_denoise_var_halves_device is rt1w_denoise_cross_device: tests/test_adaptive_filtered.py's composition over the
    public device entries then is rt1w_render_adaptive_cross's; the renders' segments are summed on the way"""

    def __init__(self, ctx):
        self._ctx, self.segments = ctx, 0

    def __getattr__(self, name):
        return getattr(self._ctx, name)

    def denoise_var_halves_device(self, *a, **kw):
        return self._ctx.denoise_cross_device(*a, **kw)

    def render_device(self, *a, **kw):
        st = self._ctx.render_device(*a, **kw)
        self.segments += st["segments"]
        return st

    def render_tiles_device(self, *a, **kw):
        st = self._ctx.render_tiles_device(*a, **kw)
        self.segments += st["segments"]
        return st


@pytest.mark.gpu
@pytest.mark.parametrize("arm,size", [(5, (48, 40)), (7, (40, 40))])
def test_gpu_one_call_equals_composition(rt, gpu_ctx_factory, arm, size):
    """rt1w_render_adaptive_cross == the plan composed over the public device entries with rt1w_denoise_cross_device in step 3, bit for bit:
    frame, spp map and error map; paths, segments, passes and rounds.  Afterwards rt1w_render_adaptive_filtered of the same context still
    returns its own composition's bits."""
    W, H = size
    ad = dict(tile=16, **TF.GPU_AD)
    sc = rt.Scene.reference(arm, build_seed=1, aspect_ratio=W / H)
    ctx = gpu_ctx_factory(sc)
    dev = TF._DeviceBuffers()
    try:
        cross = _CrossContext(ctx)
        out, spp, err_px, rounds, launches, paths = TF._compose_device(rt, cross, sc, W, H, ad, dev, global_seed=3)
        one, ospp, oerr, st = ctx.render_adaptive_cross(W, H, adaptive=ad, global_seed=3, with_stats=True)
        assert _same(one, out) and _same(ospp, spp) and _same(oerr, err_px), arm
        assert st["paths"] == paths == int(spp.sum()) and st["segments"] == cross.segments and st["n_chunks"] == rounds and rounds >= 1
        assert st["passes"] == launches == 2 + rounds
        assert st["block"] == 256 and st["grid"] == ((W + 15) // 16) * ((H + 15) // 16) and st["kernel_ms"] > 0 and st["total_ms"] > 0
        assert spp.sum() <= 8 * W * H and spp.max() <= 16 and spp.min() >= 4 and np.all(spp % 4 == 0)
        assert np.all(np.isfinite(oerr)) and oerr.max() > 0.0
        f_out, f_spp, f_err, _, _, _ = TF._compose_device(rt, ctx, sc, W, H, ad, dev, global_seed=3)
        got = ctx.render_adaptive_filtered(W, H, adaptive=ad, global_seed=3)
        assert _same(got[0], f_out) and _same(got[1], f_spp) and _same(got[2], f_err) and not _same(f_out, out)
        with pytest.raises(rt.Rt1wError) as e:
            ctx.render_adaptive_cross(W, H, adaptive=dict(ad, pilot_batches=3, budget_spp=16))
        assert e.value.code == rt.ERR_INVALID
    finally:
        dev.free()


@pytest.mark.gpu
def test_gpu_refusals(rt, gpu_ctx_factory):
    """code, text and order of what rt1w_denoise_cross and its device form refuse == the recording, and == what rt1w_denoise_var_halves
    and its device form answer to the same calls.  Every case returns before any launch."""
    ctx = gpu_ctx_factory(rt.Scene.reference(0, build_seed=1))
    want = json.load(open(REFUSALS))
    got = _refusals(rt, ctx._h)
    assert got == want
    old = _refusals(rt, ctx._h, ("rt1w_denoise_var_halves", "rt1w_denoise_var_halves_device"))
    assert old["rt1w_denoise_var_halves"] == got["rt1w_denoise_cross"] and old["rt1w_denoise_var_halves_device"] == got["rt1w_denoise_cross_device"]


if __name__ == "__main__" and "--record" in sys.argv:
    for p_ in (ROOT, os.path.join(ROOT, "tests")):
        sys.path.insert(0, p_)
    _rt = orc.rt()
    assert _rt.device_count() >= 1, "recording needs a GPU"
    _ctx = _rt.Context(_rt.Scene.reference(0, build_seed=1), 0)
    _got = _refusals(_rt, _ctx._h)
    _ctx.close()
    assert all(c[1] < 0 for cs in _got.values() for c in cs), "a case was not refused"
    _to = sys.argv[sys.argv.index("--record") + 1] if len(sys.argv) > sys.argv.index("--record") + 1 else REFUSALS
    with open(_to, "w") as f:
        json.dump(_got, f, indent=0, sort_keys=True)
        f.write("\n")
    print("recorded", _to)
