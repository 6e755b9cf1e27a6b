"""Adaptive sampling steered by the filtered frame's half-buffer error (rt1w_halves_resolve, rt1w_denoise_var_halves, rt1w_tile_error_map and
their device forms, rt1w_render_adaptive_filtered, include/rt1w.h).  CPU tier: the ABI surface and the refusals that need no GPU, the CPU
twins (librt1w_lab.so: rt1w_lab_halves_resolve_host, rt1w_lab_denoise_var_halves_host, rt1w_lab_tile_error_map_host) on inputs whose answer
follows by hand and against the long-double statement tests/dn_halves_reference.py, the whole plan composed in Python over orc.flat_render,
the calibration of the estimate and the quality against converged frames.  GPU tier: the kernels bit for bit against the twins, `out`
against rt1w_denoise_var, the one call against the composition of the public device entries, and non-interference."""
import ctypes as C
import functools
import json
import os
import sys

import numpy as np
import pytest

import orc
import dn_halves_reference as HR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
REFUSALS = os.path.join(GOLD, "adaptive_filtered_refusals.json")
LUM = np.array([0.2126, 0.7152, 0.0722])

# the quality cases of tests/test_adaptive.py: arm -> (width, height); converged frames tests/golden/denoise_ref_arm*.npy
QUALITY = {5: (96, 96), 4: (128, 72), 7: (64, 64)}
# mse(rt1w_render_adaptive_filtered's frame) / mse(uniform 4 batches + rt1w_batch_variance + rt1w_denoise_var at `budget` samples), displayed
# values, measured with the twins at tile 16 and otherwise default parameters, global_seed 0.  Keys: (arm, budget).
# The existing path (rt1w_render_adaptive + filter) has tests/test_adaptive.py's MEASURED_RATIO_FILTERED: geometric mean 0.985.
MEASURED_RATIO = {(5, 32): 0.7839, (5, 128): 0.8911, (4, 32): 0.9252, (4, 128): 0.9171, (7, 32): 1.2476, (7, 128): 0.9776}
# frame mean of err_px x its denominator over the seed-to-seed variance of the filtered frame's luminance (test_calibration)
MEASURED_CALIBRATION = 0.205


def _same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _guides(h, w, rng=None):
    aov = np.empty((h, w, 8))
    aov[..., 0:3] = (0.5, 0.25, 1.0) if rng is None else rng.uniform(0.005, 1.0, (h, w, 3))
    aov[..., 3:6] = (0.0, 0.6, 0.8)
    aov[..., 6] = 3.0
    aov[..., 7] = 1.0
    return aov


def _tiles(W, H, tile):
    return (W + tile - 1) // tile, (H + tile - 1) // tile


def _pair_params(ad):
    """what rt1w_adaptive_select is called with: a pair is one batch of 2 n samples"""
    return dict(ad, batch_spp=2 * ad["batch_spp"], pilot_batches=max(2, ad["pilot_batches"] // 2))


def _hostile(rng):
    """67 x 45: NaN / inf values, misses, zero normals, a zero-variance region; (frame, aov, var, half_a, half_b)"""
    h, w = 45, 67
    aov = _guides(h, w, rng)
    aov[..., 3:6] = rng.normal(size=(h, w, 3))
    aov[..., 6] = rng.uniform(1.0, 9.0, (h, w))
    aov[..., 7] = rng.uniform(0.0, 1.0, (h, w))
    aov[10:14, 20:30, 3:6] = 0.0
    aov[10:14, 20:30, 6] = np.inf                         # misses
    aov[3, 4, 0] = np.nan
    aov[5, 6, 3] = np.inf
    aov[30, 40, 0:3] = 0.0                                # albedo below the floor
    a = rng.uniform(0.0, 2.0, (h, w, 3))
    b = rng.uniform(0.0, 2.0, (h, w, 3))
    frame = (a + b) * 0.5
    var = rng.uniform(0.0, 0.3, (h, w))
    var[:, 50:] = 0.0
    var[7, 7] = np.nan
    var[8, 8] = -1.0
    frame[20, 20] = np.nan
    frame[21, 33, 1] = np.inf
    a[22, 22, 0] = np.nan
    b[23, 24, 2] = np.inf
    a[40, 60] = -3.0
    return frame, aov, var, a, b


# ---- the plan, restated in Python over any (render, merge, resolve, filter, tile error): what rt1w_render_adaptive_filtered says it does ----

def _compose(rt, W, H, ad, aov, render, merge, resolve, filt, tile_error, check=None):
    """returns (out, spp, err_px, pairs per tile, rounds, render launches).  render(rects with offsets) -> list of sums, one launch"""
    tile, n, P = ad["tile"], ad["batch_spp"], ad["pilot_batches"]
    acc = [np.zeros((H, W, 8)), np.zeros((H, W, 8))]
    launches = 0
    for b in range(P):
        acc[b & 1] = merge(acc[b & 1], render([((0, 0, W, H), b * n)])[0], n, 0, 0)
        launches += 1
    tx_n, ty_n = _tiles(W, H, tile)
    m = np.full((ty_n, tx_n), P // 2, dtype=np.uint32)
    rounds = 0
    while True:
        frame, var, ha, hb, spp = resolve(acc[0], acc[1], n)
        if check:
            check(acc, m, spp)
        out, err_px = filt(frame, aov, var, ha, hb)
        taken = rt.adaptive_select(W, H, tile_error(err_px, tile), m, **_pair_params(ad))
        if not taken:
            return out, spp, err_px, m, rounds, launches
        assert len(set(taken)) == len(taken)
        rounds += 1
        rects = [(((t % tx_n) * tile, (t // tx_n) * tile, min(tile, W - (t % tx_n) * tile), min(tile, H - (t // tx_n) * tile)),
                  (2 * int(m.flat[t]) + half) * n) for half in (0, 1) for t in taken]
        sums = render(rects)
        launches += 1
        for k, (rect, _) in enumerate(rects):
            half = k // len(taken)
            acc[half] = merge(acc[half], sums[k], n, rect[0], rect[1])
        for t in taken:
            m.flat[t] += 1


def _compose_cpu(rt, sc, W, H, ad, global_seed=0, check=None):
    n, P = ad["batch_spp"], ad["pilot_batches"]
    chunk = sc.default_chunk(W, H, n)  # of the WHOLE frame, passed explicitly to every rectangle
    aov = rt.aov_host(sc, W, H, P * n, global_seed=global_seed)

    def render(rects):
        return [orc.flat_render(sc, W, H, n, tile=r, sample_offset=off, out_sum=True, chunk=chunk, global_seed=global_seed)[0] for r, off in rects]

    def merge(acc, sums, n, x0, y0):
        return rt.accum_merge_host(acc, sums, aov, n, x0=x0, y0=y0)
    return _compose(rt, W, H, ad, aov, render, merge, rt.halves_resolve_host, rt.denoise_var_halves_host, rt.tile_error_map_host, check) + (aov,)


# ------------------------------------------------------------------------------------------------------------------ CPU tier --

RENDER = dict(width=32, height=32, x0=0, y0=0, tile_w=32, tile_h=32, spp=4, sample_offset=0, max_depth=8, global_seed=0, chunk=0, flags=0)
ADAPTIVE = dict(tile=16, batch_spp=2, pilot_batches=2, budget_spp=8, max_spp=16)
# (case, render members, adaptive members, sigma_variance): each refused with RT1W_ERR_INVALID before the context is looked at
REFUSAL_CASES = [("pilot_batches 3", {}, dict(pilot_batches=3, budget_spp=16), 0.0), ("pilot_batches 5", {}, dict(pilot_batches=5, budget_spp=16), 0.0),
                 ("RT1W_UNSORTED", dict(flags=2), {}, 0.0), ("RT1W_WAVEFRONT", dict(flags=16), {}, 0.0), ("RT1W_OUT_SUM", dict(flags=1), {}, 0.0),
                 ("RT1W_GENERIC | RT1W_LDS_NODES", dict(flags=12), {}, 0.0), ("tile 16 x 32", dict(tile_w=16), {}, 0.0),
                 ("tile at y0 16", dict(y0=16, tile_h=16), {}, 0.0), ("sigma_variance negative", {}, {}, -1.0),
                 ("sigma_variance NaN", {}, {}, float("nan")), ("sigma_variance infinite", {}, {}, float("inf")),
                 ("odd pilot and a bad sigma_variance: the sigma is checked first", {}, dict(pilot_batches=3, budget_spp=16), -1.0),
                 ("odd pilot and a bad flag: the plan is checked first", dict(flags=2), dict(pilot_batches=3, budget_spp=16), 0.0),
                 ("tile 24", {}, dict(tile=24), 0.0), ("budget below two pairs", {}, dict(budget_spp=4), 0.0)]


def _refusals(rt):
    out = {}
    rgb = np.zeros((32, 32, 3))
    for name, pm, am, sv in REFUSAL_CASES:
        p = rt.RenderParams()
        for k, v in dict(RENDER, **pm).items():
            setattr(p, k, v)
        a = rt.adaptive_params(**dict(ADAPTIVE, **am))
        rc = rt._lib.rt1w_render_adaptive_filtered(None, C.byref(p), C.byref(a), None, sv, rgb.ctypes.data_as(C.c_void_p), None, None, None)
        out[name] = [rc, rt.last_error()]
    return out


def test_abi_surface_and_refusals(rt):
    """The seven entries are exported with the declared arity.  rt1w_render_adaptive_filtered checks what the parameters alone decide before
    it looks at the context, so these refusals need no GPU: an odd pilot_batches, p->flags outside {0, RT1W_GENERIC}, a tile that is not the
    frame and a bad sigma_variance all answer RT1W_ERR_INVALID, with the texts recorded in tests/golden/adaptive_filtered_refusals.json
    (`python tests/test_adaptive_filtered.py --record`); a call without any defect then reaches the context check."""
    arity = {"rt1w_halves_resolve": 12, "rt1w_halves_resolve_device": 12, "rt1w_denoise_var_halves": 11, "rt1w_denoise_var_halves_device": 11,
             "rt1w_tile_error_map": 7, "rt1w_tile_error_map_device": 7, "rt1w_render_adaptive_filtered": 9}
    lib = C.CDLL(rt.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "rt1w.h")).read()
    for name, n in arity.items():
        assert hasattr(lib, name), name
        assert len(getattr(rt._lib, name).argtypes) == n, name
        decl = hdr[hdr.index("int " + name + "("):]
        assert decl[:decl.index(";")].count(",") + 1 == n, name
    got = _refusals(rt)
    want = json.load(open(REFUSALS))
    assert sorted(got) == sorted(want)
    for name in got:
        assert got[name] == want[name], (name, got[name], want[name])
        assert got[name][0] == rt.ERR_INVALID, name
    assert "pilot_batches must be even" in got["pilot_batches 3"][1] and "RT1W_GENERIC" in got["RT1W_UNSORTED"][1]
    assert "whole frame" in got["tile 16 x 32"][1] and "sigma_variance" in got["sigma_variance NaN"][1]
    assert "sigma_variance" in got["odd pilot and a bad sigma_variance: the sigma is checked first"][1]
    assert "pilot_batches" in got["odd pilot and a bad flag: the plan is checked first"][1]
    p = rt.RenderParams()
    for k, v in RENDER.items():
        setattr(p, k, v)
    a = rt.adaptive_params(**ADAPTIVE)
    rgb = np.zeros((32, 32, 3))
    for flags in (0, rt.GENERIC):
        p.flags = flags
        assert rt._lib.rt1w_render_adaptive_filtered(None, C.byref(p), C.byref(a), None, 0.0, rgb.ctypes.data_as(C.c_void_p), None, None, None) == rt.ERR_INVALID
        assert "null argument" in rt.last_error()
    # the twins' refusals
    z8, z3, z1 = np.zeros((4, 6, 8)), np.zeros((4, 6, 3)), np.zeros((4, 6))
    with pytest.raises(rt.Rt1wError):
        rt.halves_resolve_host(z8, z8, 0)
    for tile in (0, 8, 24, 272):
        with pytest.raises(rt.Rt1wError):
            rt.tile_error_map_host(z1, tile)
    for kw in (dict(sigma_variance=-1.0), dict(sigma_variance=float("nan")), dict(iterations=9)):
        with pytest.raises(rt.Rt1wError):
            rt.denoise_var_halves_host(z3, _guides(4, 6), z1, z3, z3, **kw)


def test_halves_resolve_known_answers(rt):
    """K batches dealt to A (even) and B (odd): frame is rt1w_resolve of S_A + S_B, the halves of S_A and S_B with their own counts, spp = m n,
    all by hand and bit for bit; var against the long-double statement of its meaning and against rt1w_accum_resolve of ONE accumulator that
    got the same batches, within 1e-12 (batches with rms deviation >= 0.05 of their mean: tests/test_adaptive.py has the clause); m_A != m_B;
    marked and empty pixels give 0."""
    h, w, n = 9, 21, 4
    rng = np.random.default_rng(17)
    aov = _guides(h, w, rng)
    for keep in (False, True):
        for K in (6, 5, 2, 3):                                        # 5, 3: m_A = m_B + 1
            sums = rng.uniform(0.0, 8.0, (K, h, w, 3))
            A_ = np.ones(3) if keep else np.maximum(aov[..., 0:3], 0.01)
            lk = ((sums / n) / A_) @ LUM
            if K >= 5:
                assert np.all(lk.std(0) > 0.05 * lk.mean(0))
            acc = [np.zeros((h, w, 8)), np.zeros((h, w, 8))]
            one = np.zeros((h, w, 8))
            for k in range(K):
                acc[k & 1] = rt.accum_merge_host(acc[k & 1], sums[k], aov, n, keep_albedo=keep)
                one = rt.accum_merge_host(one, sums[k], aov, n, keep_albedo=keep)
            frame, var, ha, hb, spp = rt.halves_resolve_host(acc[0], acc[1], n)
            assert _same(frame, rt.resolve(acc[0][..., 0:3] + acc[1][..., 0:3], K * n)) and np.all(spp == K * n)
            assert _same(ha, rt.resolve(acc[0][..., 0:3], ((K + 1) // 2) * n)) and _same(hb, rt.resolve(acc[1][..., 0:3], (K // 2) * n))
            want = HR.halves_variance(sums[0::2], sums[1::2], aov, n, keep_albedo=keep)
            rel = np.abs(var - want) / want
            rel1 = np.abs(var - rt.accum_resolve_host(one, n)[1]) / var
            print("keep", keep, "K", K, "var against the long-double statement", float(rel.max()), "against one accumulator", float(rel1.max()))
            if K >= 5:
                assert rel.max() <= 1e-12 and rel1.max() <= 1e-12
            else:                                                     # 2 or 3 batches: no conditioning clause holds; the definition, loosely
                assert rel.max() <= 1e-9
    # m < 2, one half empty: no variance; the empty half is (0, 0, 0)
    a1 = rt.accum_merge_host(np.zeros((h, w, 8)), sums[0], aov, n)
    f, v, ha, hb, s = rt.halves_resolve_host(a1, np.zeros((h, w, 8)), n)
    assert np.all(v == 0.0) and np.all(s == n) and not hb.any() and _same(ha, rt.resolve(sums[0], n)) and _same(f, rt.resolve(sums[0] + 0.0, n))
    fe = rt.halves_resolve_host(np.zeros((h, w, 8)), np.zeros((h, w, 8)), n)
    assert not any(x.any() for x in fe)
    # a marked pixel in either half: var 0 there, the neighbours untouched; a NaN sum is scrubbed as rt1w_resolve does
    bad = sums.copy()
    bad[1, 2, 3, 0] = np.nan                                          # batch 1 -> B
    bad[2, 4, 5, 2] = np.inf                                          # batch 2 -> A
    acc = [np.zeros((h, w, 8)), np.zeros((h, w, 8))]
    for k in range(3):
        acc[k & 1] = rt.accum_merge_host(acc[k & 1], bad[k], aov, n)
    acc[1] = rt.accum_merge_host(acc[1], bad[0], aov, n)
    f, v, ha, hb, s = rt.halves_resolve_host(acc[0], acc[1], n)
    assert v[2, 3] == 0.0 and v[4, 5] == 0.0 and f[2, 3, 0] == 0.0 and hb[2, 3, 0] == 0.0 and ha[4, 5, 2] == np.inf and np.all(s == 4 * n)
    ok = np.ones((h, w), dtype=bool)
    ok[2, 3] = ok[4, 5] = False
    assert np.all(v[ok] > 0.0)
    # equal halves: delta = 0 and both M2 are 0, so var is exactly 0
    e = [rt.accum_merge_host(np.zeros((h, w, 8)), sums[1], aov, n) for _ in range(2)]
    assert np.all(rt.halves_resolve_host(e[0], e[1], n)[1] == 0.0)


@functools.lru_cache(maxsize=None)
def _rendered(arm):
    """a rendered 48 x 40 frame in two halves of two batches each: (frame, aov, var, half_a, half_b)"""
    rt = orc.rt()
    W, H, n = 48, 40, 2
    sc = rt.Scene.reference(arm, build_seed=1, aspect_ratio=W / H)
    aov = rt.aov_host(sc, W, H, 4 * n)
    acc = [np.zeros((H, W, 8)), np.zeros((H, W, 8))]
    for b in range(4):
        acc[b & 1] = rt.accum_merge_host(acc[b & 1], orc.flat_render(sc, W, H, n, sample_offset=b * n, out_sum=True)[0], aov, n)
    frame, var, ha, hb, _ = rt.halves_resolve_host(acc[0], acc[1], n)
    return frame, aov, var, ha, hb


def test_filter_twin(rt):
    """`out` is rt1w_lab_denoise_var_host's, bit for bit, on rendered frames (arms 5 and 7) and on the hostile buffer, with and without
    KEEP_ALBEDO and with zero variance everywhere; equal halves give an error map of exactly +0.0; a', b' and err_px against the
    long-double statement within 1e-12 where |lum a' - lum b'| is at least 0.05 of their mean (the difference of two nearly equal
    luminances has no relative accuracy: the variance's clause, for the same reason) and the reference can decide the pixel."""
    cases = [(_rendered(5), {}), (_rendered(7), {}), (_rendered(5), dict(iterations=2, keep_albedo=True)),
             (_hostile(np.random.default_rng(5)), {}), (_hostile(np.random.default_rng(6)), dict(keep_albedo=True, iterations=3))]
    for i, ((frame, aov, var, ha, hb), kw) in enumerate(cases):
        for v in (np.zeros_like(var), var):                           # the last one, the variance itself, is compared below
            out, err, fa, fb = rt.denoise_var_halves_host(frame, aov, v, ha, hb, with_halves=True, **kw)
            assert _same(out, rt.denoise_var_host(frame, aov, v, **kw)), i
            assert np.all(err >= 0.0) and np.all(np.isfinite(err)) and not np.signbit(err).any()
            o0, e0 = rt.denoise_var_halves_host(frame, aov, v, frame, frame, **kw)
            assert _same(o0, out) and not e0.any() and not np.signbit(e0).any(), i
        assert err.max() > 0.0
        if i >= 3 and kw.get("iterations"):
            continue
        want_out, wa, wb, we, undecidable = HR.denoise_var_halves(frame, aov, var, ha, hb, **kw)
        with np.errstate(all="ignore"):
            la, lb = fa @ LUM, fb @ LUM
            fin = np.isfinite(fa).all(-1) & np.isfinite(fb).all(-1) & np.isfinite(out).all(-1) & ~undecidable
            fin &= np.isfinite(np.asarray(wa, dtype=np.float64)).all(-1) & np.isfinite(np.asarray(wb, dtype=np.float64)).all(-1)
            cond = fin & (np.abs(la - lb) >= 0.05 * 0.5 * np.abs(la + lb)) & (la != lb)   # black pixels: both 0, err_px exactly 0
            ra = np.abs(fa - wa)[fin] / np.maximum(np.abs(wa[fin]), np.maximum(np.abs(wa[fin]).max(-1, keepdims=True) * 1e-3, 1e-300))
            rb = np.abs(fb - wb)[fin] / np.maximum(np.abs(wb[fin]), np.maximum(np.abs(wb[fin]).max(-1, keepdims=True) * 1e-3, 1e-300))
            re = np.abs(err - we)[cond] / we[cond]
        print("case", i, "pixels", int(fin.sum()), "conditioned", int(cond.sum()), "a'", float(ra.max()), "b'", float(rb.max()), "err_px", float(re.max()))
        assert cond.sum() >= 100
        assert ra.max() <= 1e-12 and rb.max() <= 1e-12 and re.max() <= 1e-12


def _tile_map_by_hand(e, tile):
    """the header's definition in numpy scalars: the value (negative or not finite: 0), the block tree, the blocks in row-major order"""
    H, W = e.shape
    tx_n, ty_n = _tiles(W, H, tile)
    out = np.zeros((ty_n, tx_n))
    for ty in range(ty_n):
        for tx in range(tx_n):
            total = np.float64(0.0)
            for by in range(tile // 16):
                for bx in range(tile // 16):
                    X0, Y0 = tx * tile + bx * 16, ty * tile + by * 16
                    if X0 >= W or Y0 >= H:
                        continue
                    v = np.zeros(256)
                    blk = e[Y0:Y0 + 16, X0:X0 + 16]
                    v.reshape(16, 16)[:blk.shape[0], :blk.shape[1]] = np.where(np.isfinite(blk) & (blk >= 0), blk, 0.0)
                    stride = 128
                    while stride >= 1:
                        v[:stride] = v[:stride] + v[stride:2 * stride]
                        stride //= 2
                    total = total + v[0]
            px = (min(W, (tx + 1) * tile) - tx * tile) * (min(H, (ty + 1) * tile) - ty * tile)
            out[ty, tx] = total / np.float64(px)
    return out


@pytest.mark.parametrize("shape", [(5, 17), (16, 16), (149, 203)])
def test_tile_error_map_by_hand(rt, shape):
    """Values spanning 16 decades, so the sum depends on the association: the twin takes the header's, bit for bit, at tiles 16, 32 and 48,
    and differs from a sequential sum; negative, NaN and inf values count as 0."""
    H, W = shape
    rng = np.random.default_rng(H * 1000 + W)
    e = 10.0 ** rng.uniform(-12, 4, (H, W))
    e[H // 2, W // 3] = np.nan
    e[H // 3, W // 2] = np.inf
    e[0, 0] = -1.0
    e[H - 1, W - 1] = -np.inf
    for tile in (16, 32, 48):
        got = rt.tile_error_map_host(e, tile)
        assert got.shape == _tiles(W, H, tile)[::-1] and _same(got, _tile_map_by_hand(e, tile)), tile
    got = rt.tile_error_map_host(e, 16)
    blk = e[:16, :16]
    clean = np.where(np.isfinite(blk) & (blk >= 0), blk, 0.0)
    seq = 0.0
    for x in clean.ravel():
        seq += x
    assert abs(got[0, 0] - clean.sum() / clean.size) <= 1e-12 * got[0, 0]
    if clean.size == 256:
        assert got[0, 0] != seq / 256.0, "the values do not tell the tree from a sequential sum"
    assert _same(rt.tile_error_map_host(np.full((H, W), np.nan), 16), np.zeros(_tiles(W, H, 16)[::-1]))


LOOP = dict(tile=16, batch_spp=2, pilot_batches=2, budget_spp=8, max_spp=16)


def test_the_loop_is_what_it_says(rt):
    """The whole plan composed in Python from orc.flat_render of tiles, the twins and rt1w_adaptive_select (called with batch_spp = 2 n and
    the tiles' pair counts), Cornell 96 x 96: the budget and max_spp hold and the budget is used, every pixel's count is a multiple of 2 n,
    m_A == m_B at every estimate, it adapts over more than one round, every pixel's S_A / S_B is the batch-order sum of the whole frame's
    even / odd batches, and the output is the last round's filtered frame: rt1w_lab_denoise_var_host of the final halves' resolve."""
    W = H = 96
    n = LOOP["batch_spp"]
    sc = rt.Scene.reference(5, build_seed=1)
    seen = []

    def check(acc, m, spp):
        assert np.array_equal(acc[0][..., 3], acc[1][..., 3])                       # m_A == m_B at every estimate
        assert np.array_equal(acc[0][..., 3], np.repeat(np.repeat(m, 16, axis=0), 16, axis=1)[:H, :W])
        seen.append((acc[0].copy(), acc[1].copy()))
    out, spp, err_px, m, rounds, launches, aov = _compose_cpu(rt, sc, W, H, LOOP, check=check)
    print("rounds", rounds, "launches", launches, "pairs per tile", np.unique(m, return_counts=True))
    assert rounds >= 2 and launches == 2 + rounds and m.max() > m.min() and len(seen) == rounds + 1
    assert spp.sum() <= LOOP["budget_spp"] * W * H and spp.sum() > (LOOP["budget_spp"] - 2) * W * H
    assert spp.max() <= 16 and spp.min() >= 4 and np.all(spp % (2 * n) == 0)
    mp = np.repeat(np.repeat(m, 16, axis=0), 16, axis=1)[:H, :W]
    assert np.array_equal(spp, mp * 2 * n)
    chunk = sc.default_chunk(W, H, n)
    a, b = seen[-1]
    for half, acc in ((0, a), (1, b)):
        whole = [orc.flat_render(sc, W, H, n, sample_offset=(2 * j + half) * n, out_sum=True, chunk=chunk)[0] for j in range(int(m.max()))]
        want = whole[0].copy()
        for j in range(1, int(m.max())):
            want = np.where((mp > j)[..., None], want + whole[j], want)
        assert _same(acc[..., 0:3], want), half
    frame, var, ha, hb, s2 = rt.halves_resolve_host(a, b, n)
    assert _same(out, rt.denoise_var_host(frame, aov, var)) and _same(spp, s2)      # the last filtered frame is the output
    assert _same(err_px, rt.denoise_var_halves_host(frame, aov, var, ha, hb)[1]) and err_px.max() > 0.0


def test_calibration(rt):
    """What the estimate claims to measure: the seed-to-seed variance of the filtered frame.  Cornell 40 x 40, every pixel 2 pairs of 4
    samples (uniform: no adaptivity, so no selection bias), 24 independent global_seeds.  Estimate: the frame mean of err_px x its
    denominator, (lum a' - lum b')^2 / 4, averaged over the seeds' own maps.  Truth: the per-pixel variance over the seeds of the luminance
    of the filtered frame that would be displayed, frame mean.  The ratio measured with the twins is MEASURED_CALIBRATION = 0.205: the
    estimate UNDERSTATES the seed-to-seed variance five times here.  The formula is not what is off -- the same expression on the unfiltered
    halves measured 1.02 of their frames' variance -- the shared weights are: they are computed from the noisy frame and from guides that
    are themselves rendered per seed, and both halves see the same weights, so the part of the error that comes through the weights is
    common to a' and b' and cancels in their difference (0.56 with the colour term switched off, guides alone).
    Cross-filtering each half with the other's weights is the known remedy and is out of scope.  One squared difference per pixel is a
    one-degree-of-freedom estimate, so the assertion is a factor 2 of the measurement either way: it covers the frame average's spread."""
    W = H = 40
    n, seeds = 4, 24
    sc = rt.Scene.reference(5, build_seed=1)
    est, lums = [], []
    for g in range(seeds):
        aov = rt.aov_host(sc, W, H, 4 * n, global_seed=g)
        acc = [np.zeros((H, W, 8)), np.zeros((H, W, 8))]
        for b in range(4):
            acc[b & 1] = rt.accum_merge_host(acc[b & 1], orc.flat_render(sc, W, H, n, sample_offset=b * n, out_sum=True, global_seed=g)[0], aov, n)
        frame, var, ha, hb, _ = rt.halves_resolve_host(acc[0], acc[1], n)
        out, err = rt.denoise_var_halves_host(frame, aov, var, ha, hb)
        lo = out @ LUM
        est.append(float(np.mean(err * (np.maximum(lo, 0.0) + 0.01))))
        lums.append(lo)
    truth = float(np.mean(np.var(np.stack(lums), axis=0, ddof=1)))
    ratio = float(np.mean(est)) / truth
    print(f"estimate {np.mean(est):.6g} (single seeds {min(est):.6g} .. {max(est):.6g}) truth {truth:.6g} ratio {ratio:.4f} (measured {MEASURED_CALIBRATION})")
    assert MEASURED_CALIBRATION / 2.0 <= ratio <= MEASURED_CALIBRATION * 2.0


def _disp(c):
    return np.sqrt(np.clip(c, 0.0, 0.999))  # the displayed value, src/color.rs:56-65 (as test_adaptive.py)


def _mse(a, b):
    return float(np.mean((_disp(a) - _disp(b)) ** 2))


@functools.lru_cache(maxsize=None)
def _uniform_filtered_mse(arm, budget):
    """the denominator of tests/test_adaptive.py's MEASURED_RATIO_FILTERED: uniform 4 batches + rt1w_batch_variance + rt1w_denoise_var"""
    rt = orc.rt()
    W, H = QUALITY[arm]
    sc = rt.Scene.reference(arm, build_seed=1)
    ref = np.load(os.path.join(GOLD, f"denoise_ref_arm{arm}.npy"))
    k = budget // 4
    sums = np.stack([orc.flat_render(sc, W, H, k, sample_offset=b * k, out_sum=True)[0] for b in range(4)])
    uaov = rt.aov_host(sc, W, H, budget)
    uframe, uvar = rt.batch_variance_host(sums, uaov, k)
    return _mse(rt.denoise_var_host(uframe, uaov, uvar), ref)


def quality_case(arm, budget, **over):
    """(mse of the call's frame as the twins compose it, mse of the uniform filtered frame, mean spp, rounds); over: plan members"""
    rt = orc.rt()
    W, H = QUALITY[arm]
    sc = rt.Scene.reference(arm, build_seed=1)
    ref = np.load(os.path.join(GOLD, f"denoise_ref_arm{arm}.npy"))
    n = max(1, budget // 8)                  # the defaults of rt1w_adaptive_params, spelled out
    ad = dict(dict(tile=16, batch_spp=n, pilot_batches=4, budget_spp=budget, max_spp=8 * budget), **over)
    out, spp, err_px, m, rounds, launches, aov = _compose_cpu(rt, sc, W, H, ad)
    assert spp.sum() <= budget * W * H
    return _mse(out, ref), _uniform_filtered_mse(arm, budget), float(spp.mean()), rounds


@pytest.mark.parametrize("budget", [32, 128])
@pytest.mark.parametrize("arm", sorted(QUALITY))
def test_quality_against_converged_frames(rt, arm, budget):
    """mse(the call's out) / mse(uniform 4 batches + rt1w_batch_variance + rt1w_denoise_var at `budget` samples), displayed values against
    the converged frame, tile 16 and otherwise default parameters, global_seed 0.  By the project's rule: where it measured better than
    uniform it must keep at least half of that, elsewhere it must not get worse than 1.1 x the measurement (DESIGN.md section 17 has the
    table and the comparison with the existing path's 0.985)."""
    m_ad, m_un, mean_spp, rounds = quality_case(arm, budget)
    ratio, measured = m_ad / m_un, MEASURED_RATIO[(arm, budget)]
    print(f"arm {arm} budget {budget}: mse filtered-error adaptive {m_ad:.6g} uniform filtered {m_un:.6g} ratio {ratio:.4f} (measured {measured}); "
          f"spent {mean_spp:.2f} per pixel in {rounds} rounds")
    if measured < 1.0:
        assert ratio <= (measured + 1.0) / 2.0
    else:
        assert ratio <= 1.1 * measured


# ------------------------------------------------------------------------------------------------------------------ GPU tier --

W_GPU, H_GPU = 203, 149   # not a multiple of 8 or 16; with 5 levels, step 16 reaches outside on both axes
GPU_AD = dict(batch_spp=2, pilot_batches=2, budget_spp=8, max_spp=16)


class _DeviceBuffers:
    """plain device memory of the HIP runtime this process already uses (as tests/test_adaptive.py)"""

    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")
        self.made = []

    def alloc(self, nbytes, zero=False):
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), C.c_size_t(nbytes)) == 0
        self.made.append(p)
        if zero:
            assert self.hip.hipMemset(p, 0, C.c_size_t(nbytes)) == 0
        return p.value

    def put(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        p = self.alloc(a.nbytes)
        assert self.hip.hipMemcpy(C.c_void_p(p), a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0  # HostToDevice
        return p

    def fetch(self, p, shape):
        out = np.empty(shape)
        assert self.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(p), C.c_size_t(out.nbytes), 2) == 0  # DeviceToHost
        return out

    def free(self):
        for p in self.made:
            self.hip.hipFree(p)


def _gpu_halves(rt, ctx, sc, W, H, n, batches):
    """rendered batches dealt to two accumulators through the GPU entries; (acc_a, acc_b, aov)"""
    chunk = sc.default_chunk(W, H, n)
    aov = ctx.render_aov(W, H, batches * n)
    acc = [np.zeros((H, W, 8)), np.zeros((H, W, 8))]
    for b in range(batches):
        acc[b & 1] = ctx.accum_merge(acc[b & 1], ctx.render(W, H, n, sample_offset=b * n, out_sum=True, chunk=chunk)[0], aov, n)
    return acc[0], acc[1], aov


def _check_filter(rt, ctx, dev, frame, aov, var, ha, hb, **kw):
    """host form, device form and the device form in place == the twin, bit for bit; out == rt1w_denoise_var_device of the same buffers"""
    H, W = var.shape
    t_out, t_err = rt.denoise_var_halves_host(frame, aov, var, ha, hb, **kw)
    out, err, st = ctx.denoise_var_halves(frame, aov, var, ha, hb, with_stats=True, **kw)
    assert _same(out, t_out) and _same(err, t_err)
    assert st["block"] == 256 and st["grid"] == ((W + 15) // 16) * ((H + 15) // 16) and st["kernel_ms"] > 0 and st["passes"] == 1
    d = [dev.put(x) for x in (frame, aov, var, ha, hb)]
    d_out, d_err, d_ref = dev.alloc(frame.nbytes), dev.alloc(var.nbytes), dev.alloc(frame.nbytes)
    ctx.denoise_var_halves_device(*d, d_out, d_err, W, H, **kw)
    ctx.denoise_var_device(d[0], d[1], d[2], d_ref, W, H, **kw)
    assert _same(dev.fetch(d_out, frame.shape), t_out) and _same(dev.fetch(d_err, var.shape), t_err)
    assert _same(dev.fetch(d_ref, frame.shape), t_out)                       # out == rt1w_denoise_var_device, bit for bit
    ctx.denoise_var_halves_device(*d, d[0], d_err, W, H, **kw)               # d_out == d_frame
    assert _same(dev.fetch(d[0], frame.shape), t_out) and _same(dev.fetch(d_err, var.shape), t_err)
    return t_err


@pytest.mark.gpu
@pytest.mark.parametrize("arm", [5, 7])
def test_gpu_kernels_equal_twins(rt, gpu_ctx_factory, arm):
    """rt1w_halves_resolve, rt1w_denoise_var_halves and rt1w_tile_error_map == the CPU twins bit for bit on rendered halves at 203 x 149
    (uneven counts included), host and device forms, the filter also in place, tiles 16 and 48; `out` == rt1w_denoise_var_device."""
    W, H, n = W_GPU, H_GPU, 2
    sc = rt.Scene.reference(arm, build_seed=1, aspect_ratio=W / H)
    ctx = gpu_ctx_factory(sc)
    dev = _DeviceBuffers()
    try:
        a, b, aov = _gpu_halves(rt, ctx, sc, W, H, n, 4)
        a2 = ctx.accum_merge(a, ctx.render(W, H, n, tile=(30, 140, 50, 9), sample_offset=8, out_sum=True, chunk=sc.default_chunk(W, H, n))[0], aov, n, x0=30, y0=140)
        for (pa, pb) in ((a, b), (a2, b)):                                   # the second: m_A != m_B on a rectangle
            got = ctx.halves_resolve(pa, pb, n, with_stats=True)
            want = rt.halves_resolve_host(pa, pb, n)
            assert all(_same(g, t) for g, t in zip(got[:5], want))
            assert got[5]["block"] == 256 and got[5]["grid"] == ((W + 15) // 16) * ((H + 15) // 16)
        d = [dev.put(a), dev.put(b)] + [dev.alloc(W * H * k * 8) for k in (3, 1, 3, 3, 1)]
        ctx.halves_resolve_device(*d, W, H, n)
        frame, var, ha, hb, spp = want = rt.halves_resolve_host(a, b, n)
        assert all(_same(dev.fetch(p, t.shape), t) for p, t in zip(d[2:], want)) and var.max() > 0.0
        err_px = _check_filter(rt, ctx, dev, frame, aov, var, ha, hb)
        assert err_px.max() > 0.0
        _check_filter(rt, ctx, dev, frame, aov, var, ha, hb, keep_albedo=True, iterations=3)
        for tile in (16, 48):
            err, st = ctx.tile_error_map(err_px, tile, with_stats=True)
            assert _same(err, rt.tile_error_map_host(err_px, tile)) and st["grid"] == err.size and st["block"] == 256 and err.max() > 0.0
            d_err = dev.alloc(err.nbytes)
            ctx.tile_error_map_device(dev.put(err_px), d_err, W, H, tile)
            assert _same(dev.fetch(d_err, err.shape), err)
    finally:
        dev.free()


@pytest.mark.gpu
def test_gpu_small_and_hostile(rt, gpu_ctx_factory):
    """17 x 5 (one partial workgroup, every step beyond 1 reaches outside) and the hostile 67 x 45 buffer: kernels == twins, all forms."""
    ctx = gpu_ctx_factory(rt.Scene.reference(5, build_seed=1))
    dev = _DeviceBuffers()
    rng = np.random.default_rng(9)
    try:
        h, w = 5, 17
        aov = _guides(h, w, rng)
        ha, hb = rng.uniform(0.0, 2.0, (h, w, 3)), rng.uniform(0.0, 2.0, (h, w, 3))
        err_px = _check_filter(rt, ctx, dev, (ha + hb) * 0.5, aov, rng.uniform(0.0, 0.2, (h, w)), ha, hb)
        assert _same(ctx.tile_error_map(err_px, 16), rt.tile_error_map_host(err_px, 16))
        for seed, kw in ((5, {}), (6, dict(keep_albedo=True))):
            frame, aov, var, ha, hb = _hostile(np.random.default_rng(seed))
            err_px = _check_filter(rt, ctx, dev, frame, aov, var, ha, hb, **kw)
            _check_filter(rt, ctx, dev, frame, aov, np.zeros_like(var), ha, hb, **kw)
            bad = err_px.copy()
            bad[3, 3], bad[4, 4], bad[5, 5] = np.nan, -2.0, np.inf
            for tile in (16, 32):
                assert _same(ctx.tile_error_map(bad, tile), rt.tile_error_map_host(bad, tile))
        acc = rng.uniform(0.0, 4.0, (2, h, w, 8))
        acc[..., 3] = rng.integers(0, 4, (2, h, w))
        acc[0, 1, 2, 5] = rt.ACCUM_NO_ESTIMATE
        assert all(_same(g, t) for g, t in zip(ctx.halves_resolve(acc[0], acc[1], 3), rt.halves_resolve_host(acc[0], acc[1], 3)))
    finally:
        dev.free()


def _compose_device(rt, ctx, sc, W, H, ad, dev, global_seed=0):
    """the plan over the public DEVICE entries: (out, spp, err_px, rounds, render launches, paths)"""
    tile, n = ad["tile"], ad["batch_spp"]
    npix = W * H
    chunk = sc.default_chunk(W, H, n)
    tx_n, ty_n = _tiles(W, H, tile)
    d_aov, d_sums = dev.alloc(npix * 64), dev.alloc(max(npix, 2 * tx_n * ty_n * tile * tile) * 24)
    d_acc = [dev.alloc(npix * 64, zero=True), dev.alloc(npix * 64, zero=True)]
    d_err, d_frame, d_var, d_spp, d_epx = dev.alloc(tx_n * ty_n * 8), dev.alloc(npix * 24), dev.alloc(npix * 8), dev.alloc(npix * 8), dev.alloc(npix * 8)
    d_ha, d_hb = dev.alloc(npix * 24), dev.alloc(npix * 24)
    ctx.render_aov_device(d_aov, W, H, ad["pilot_batches"] * n, global_seed=global_seed)
    stat = dict(paths=0, launches=0)
    P = ad["pilot_batches"]
    for b in range(P):
        st = ctx.render_device(d_sums, W, H, n, sample_offset=b * n, global_seed=global_seed, chunk=chunk, out_sum=True)
        stat["paths"] += st["paths"]
        ctx.accum_merge_device(d_acc[b & 1], d_sums, d_aov, W, H, (0, 0, W, H), n)
        stat["launches"] += 1
    m = np.full((ty_n, tx_n), P // 2, dtype=np.uint32)
    rounds = 0
    while True:
        ctx.halves_resolve_device(d_acc[0], d_acc[1], d_frame, d_var, d_ha, d_hb, d_spp, W, H, n)
        ctx.denoise_var_halves_device(d_frame, d_aov, d_var, d_ha, d_hb, d_frame, d_epx, W, H)
        ctx.tile_error_map_device(d_epx, d_err, W, H, tile)
        taken = rt.adaptive_select(W, H, dev.fetch(d_err, (ty_n, tx_n)), m, **_pair_params(ad))
        if not taken:
            break
        rounds += 1
        tiles = [((t % tx_n) * tile, (t // tx_n) * tile, (2 * int(m.flat[t]) + half) * n) for half in (0, 1) for t in taken]
        st = ctx.render_tiles_device(d_sums, W, H, n, tile, tiles, global_seed=global_seed, chunk=chunk, out_sum=True)
        stat["paths"] += st["paths"]
        stat["launches"] += 1
        k = len(taken)
        ctx.accum_merge_tiles_device(d_acc[0], d_sums, d_aov, W, H, tile, tiles[:k], n)
        ctx.accum_merge_tiles_device(d_acc[1], d_sums + k * tile * tile * 24, d_aov, W, H, tile, tiles[k:], n)
        for t in taken:
            m.flat[t] += 1
    return dev.fetch(d_frame, (H, W, 3)), dev.fetch(d_spp, (H, W)), dev.fetch(d_epx, (H, W)), rounds, stat["launches"], stat["paths"]


@pytest.mark.gpu
@pytest.mark.parametrize("tile", [16, 48])
@pytest.mark.parametrize("arm", [5, 7])
def test_gpu_one_call_equals_composition(rt, gpu_ctx_factory, arm, tile):
    """rt1w_render_adaptive_filtered == the plan composed in Python over the public device entries, bit for bit: out_rgb, out_spp and
    out_err; stats.passes = the pilot's launches + the rounds, n_chunks = the rounds, paths = the samples spent; and what it refuses."""
    W, H = W_GPU, H_GPU
    ad = dict(tile=tile, **GPU_AD)
    sc = rt.Scene.reference(arm, build_seed=1, aspect_ratio=W / H)
    ctx = gpu_ctx_factory(sc)
    dev = _DeviceBuffers()
    try:
        out, spp, err_px, rounds, launches, paths = _compose_device(rt, ctx, sc, W, H, ad, dev, global_seed=3)
        one, ospp, oerr, st = ctx.render_adaptive_filtered(W, H, adaptive=ad, global_seed=3, with_stats=True)
        assert _same(one, out) and _same(ospp, spp) and _same(oerr, err_px), (arm, tile)
        assert st["paths"] == paths == int(spp.sum()) and st["n_chunks"] == rounds and rounds >= 1 and st["passes"] == launches == 2 + rounds
        assert st["block"] == 256 and st["grid"] == ((W + 15) // 16) * ((H + 15) // 16) and st["kernel_ms"] > 0 and st["total_ms"] > 0
        assert spp.sum() <= 8 * W * H and spp.max() <= 16 and spp.min() >= 4 and np.all(spp % 4 == 0) and spp.max() > spp.min()
        assert np.all(np.isfinite(oerr)) and oerr.max() > 0.0
    finally:
        dev.free()
    if tile != 16:
        return
    for bad in (dict(adaptive=dict(ad, pilot_batches=3, budget_spp=16)), dict(adaptive=dict(ad, tile=24)), dict(adaptive=dict(ad, max_spp=3)),
                dict(adaptive=dict(ad, size=44)), dict(adaptive=ad, sigma_variance=-1.0), dict(adaptive=ad, denoise=dict(iterations=9)),
                dict(adaptive=ad, tile=(0, 0, W, 30)), dict(adaptive=ad, sample_offset=2 ** 32 - 10), dict(adaptive=ad, flags=rt.UNSORTED),
                dict(adaptive=ad, flags=rt.OUT_SUM), dict(adaptive=ad, precision=1)):
        with pytest.raises(rt.Rt1wError) as e:
            ctx.render_adaptive_filtered(W, H, **bad)
        assert e.value.code == rt.ERR_INVALID, bad
    assert _same(ctx.render_adaptive_filtered(W, H, adaptive=ad, global_seed=3, flags=rt.GENERIC)[0], out)


@pytest.mark.gpu
def test_gpu_nothing_else_moves(rt, gpu_ctx_factory):
    """The entries share the context's framebuffer, batch, accumulator and filter buffers with the others: rt1w_render, rt1w_denoise_var
    (through rt1w_render_denoised_var) and rt1w_render_adaptive after a call return the bits they returned before it."""
    sc = rt.Scene.reference(5, build_seed=1)
    ctx = gpu_ctx_factory(sc)
    ad = dict(tile=16, **GPU_AD)
    f0, s0 = ctx.render(90, 70, 8)
    v0 = ctx.render_denoised_var(90, 70, 8)
    r0, p0 = ctx.render_adaptive(90, 70, adaptive=ad, filter=True)
    q0 = ctx.render_adaptive_filtered(90, 70, adaptive=ad)
    ctx.render_adaptive_filtered(200, 150, adaptive=dict(ad, tile=32))        # larger than anything so far: every buffer grows
    f1, s1 = ctx.render(90, 70, 8)
    assert _same(f0, f1) and s0["segments"] == s1["segments"]
    assert _same(v0, ctx.render_denoised_var(90, 70, 8))
    r1, p1 = ctx.render_adaptive(90, 70, adaptive=ad, filter=True)
    assert _same(r0, r1) and _same(p0, p1)
    assert all(_same(x, y) for x, y in zip(q0, ctx.render_adaptive_filtered(90, 70, adaptive=ad)))


if __name__ == "__main__" and "--record" in sys.argv:
    sys.path.insert(0, ROOT)
    with open(REFUSALS, "w") as f:
        json.dump(_refusals(orc.rt()), f, indent=1)
        f.write("\n")
    print("recorded", REFUSALS)
