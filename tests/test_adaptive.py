"""Adaptive sampling (rt1w_accum_merge / rt1w_accum_resolve / rt1w_accum_tile_error and their device forms, rt1w_adaptive_select,
rt1w_render_adaptive, include/rt1w.h): a per-pixel accumulator of sample batches, the error of a tile, and a plan that spends a sample budget
on the tiles that need it.  CPU tier: the CPU twins (librt1w_lab.so: rt1w_lab_accum_merge_host, rt1w_lab_accum_resolve_host,
rt1w_lab_tile_error_host, the kernels' own rt_adaptive.h built for the host) and rt1w_adaptive_select on the ABI surface, on inputs whose
answer follows by hand, on the whole plan composed in Python over orc.flat_render, and on quality against converged frames.  GPU tier: the
kernels bit for bit against the twins, the one call against the composition of the public device entries and of the twins,
non-interference with the render entries, and one full frame."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
ULP = 2.0 ** -53
LUM = np.array([0.2126, 0.7152, 0.0722])

# the quality cases of tests/test_denoise_var.py: arm -> (width, height); converged frames tests/golden/denoise_ref_arm*.npy
QUALITY = {5: (96, 96), 4: (128, 72), 7: (64, 64)}
# mse(adaptive frame) / mse(uniform render of budget samples per pixel), displayed values, both unfiltered, measured with the twins at tile 16
# and otherwise default parameters.  Keys: (arm, budget).
MEASURED_RATIO = {(5, 32): 0.8742, (5, 128): 0.8437, (4, 32): 0.6248, (4, 128): 0.6717, (7, 32): 1.0145, (7, 128): 0.9871}
# the same with the variance-guided filter on both sides (adaptive + denoise_var against uniform 4 batches + batch_variance + denoise_var)
MEASURED_RATIO_FILTERED = {(5, 32): 0.8111, (5, 128): 0.9238, (4, 32): 0.9890, (4, 128): 0.9862, (7, 32): 1.2576, (7, 128): 0.9913}


def _same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _batch_order_sum(sums):
    total = sums[0].copy()
    for s in sums[1:]:
        total = total + s
    return total


def _guides(h, w, albedo=(0.5, 0.25, 1.0)):
    aov = np.empty((h, w, 8))
    aov[..., 0:3] = albedo
    aov[..., 3:6] = (0.0, 0.6, 0.8)
    aov[..., 6] = 3.0
    aov[..., 7] = 1.0
    return aov


# ---- the plan, restated in Python over any (render, merge, tile_error): what rt1w_render_adaptive says it does ----

def _tiles(W, H, tile):
    return (W + tile - 1) // tile, (H + tile - 1) // tile


def _runs(taken, m, tile, W, H, one_by_one=False):
    """taken tiles -> rectangles (x0, y0, w, h, m): adjacent in one tile row with equal m = one rectangle"""
    tx_n, _ = _tiles(W, H, tile)
    runs = []
    prev = None
    for t in sorted(taken):
        tx, ty = t % tx_n, t // tx_n
        x0, y0 = tx * tile, ty * tile
        tw, th = min(tile, W - x0), min(tile, H - y0)
        mt = int(m.flat[t])
        if not one_by_one and prev is not None and t == prev + 1 and tx != 0 and runs[-1][4] == mt:
            runs[-1][2] += tw
        else:
            runs.append([x0, y0, tw, th, mt])
        prev = t
    return [tuple(r) for r in runs]


def _compose(rt, W, H, ad, aov, render, merge, tile_error, one_by_one=False):
    """pilot, rounds, batches; returns (acc, m per tile, rounds, launches).  render(rect, sample_offset) -> sums of the rectangle"""
    tile, n, P = ad["tile"], ad["batch_spp"], ad["pilot_batches"]
    acc = np.zeros((H, W, 8))
    launches = 0
    for b in range(P):
        acc = merge(acc, render((0, 0, W, H), b * n), aov, n, 0, 0)
        launches += 1
    tx_n, ty_n = _tiles(W, H, tile)
    m = np.full((ty_n, tx_n), P, dtype=np.uint32)
    rounds = 0
    while True:
        err = tile_error(acc, tile)
        taken = rt.adaptive_select(W, H, err, m, **ad)
        if not taken:
            break
        assert len(set(taken)) == len(taken)
        rounds += 1
        for (x0, y0, tw, th, mt) in _runs(taken, m, tile, W, H, one_by_one):
            acc = merge(acc, render((x0, y0, tw, th), mt * n), aov, n, x0, y0)
            launches += 1
        for t in taken:
            m.flat[t] += 1
    return acc, m, rounds, launches


def _compose_cpu(rt, sc, W, H, ad, one_by_one=False, global_seed=0):
    n, P = ad["batch_spp"], ad["pilot_batches"]
    chunk = sc.default_chunk(W, H, n)  # of the WHOLE frame, passed explicitly to every rectangle
    aov = rt.aov_host(sc, W, H, P * n, global_seed=global_seed)

    def render(rect, off):
        return orc.flat_render(sc, W, H, n, tile=rect, sample_offset=off, out_sum=True, chunk=chunk, global_seed=global_seed)[0]

    def merge(acc, sums, aov, n, x0, y0):
        return rt.accum_merge_host(acc, sums, aov, n, x0=x0, y0=y0)
    return _compose(rt, W, H, ad, aov, render, merge, rt.tile_error_host, one_by_one) + (aov,)


# ------------------------------------------------------------------------------------------------------------------ CPU tier --

def test_abi_surface(rt):
    """The eight entries are exported with the declared arity; rt1w_adaptive_params carries its own size, which is checked, and is not one
    of rt1w_abi_sizeof's; every refusal of the plan and of the twins."""
    arity = {"rt1w_accum_merge": 13, "rt1w_accum_merge_device": 13, "rt1w_accum_resolve": 9, "rt1w_accum_resolve_device": 9,
             "rt1w_accum_tile_error": 7, "rt1w_accum_tile_error_device": 7, "rt1w_adaptive_select": 9, "rt1w_render_adaptive": 8}
    lib = C.CDLL(rt.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "rt1w.h")).read()
    for name, n in arity.items():
        assert hasattr(lib, name), name
        assert len(getattr(rt._lib, name).argtypes) == n, name
        decl = hdr[hdr.index("int " + name + "("):]
        assert decl[:decl.index(";")].count(",") + 1 == n, name
    assert rt._lib.rt1w_abi_sizeof(5) == 0 and rt._lib.rt1w_abi_sizeof(4) == 40
    assert C.sizeof(rt.AdaptiveParams) == 48 and rt.AdaptiveParams.size.offset == 0
    assert "#define RT1W_ACCUM_NO_ESTIMATE (-1.0)" in hdr and rt.ACCUM_NO_ESTIMATE == -1.0
    err = np.ones((2, 3))
    m = np.full((2, 3), 2, dtype=np.uint32)
    ok = dict(tile=16, batch_spp=2, pilot_batches=2, budget_spp=8, max_spp=16)
    assert rt.adaptive_select(40, 20, err, m, **ok) == [0]          # round_share 1/4 of 800 pixels: the first tile, always
    assert rt.adaptive_select(40, 20, err, m) == [0]                # all defaults
    for bad in (dict(size=44), dict(size=0), dict(size=52), dict(tile=24), dict(tile=8), dict(tile=272), dict(tile=17), dict(pilot_batches=1),
                dict(pilot_batches=17), dict(max_spp=3), dict(budget_spp=3), dict(target_error=-1e-300), dict(target_error=float("nan")),
                dict(target_error=float("inf")), dict(round_share=-0.5), dict(round_share=1.5), dict(round_share=float("nan")), dict(flags=2)):
        with pytest.raises(rt.Rt1wError) as e:
            rt.adaptive_select(40, 20, err, m, **{**ok, **bad})
        assert e.value.code == rt.ERR_INVALID, bad
    with pytest.raises(rt.Rt1wError) as e:                           # a tile grid that is not the frame's
        rt.adaptive_select(50, 20, err, m, **ok)
    assert e.value.code == rt.ERR_INVALID
    # the twins' refusals
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    lab = rt.load_lab()
    mg = lab.rt1w_lab_accum_merge_host
    mg.restype = C.c_int
    mg.argtypes = [C.c_uint32] * 8 + [C.c_void_p] * 3
    acc, aov, sums = np.zeros((4, 6, 8)), _guides(4, 6), np.ones((4, 6, 3))
    assert mg(6, 4, 0, 0, 6, 4, 1, 0, ptr(sums), ptr(aov), ptr(acc)) == 0
    assert mg(6, 4, 5, 3, 1, 1, 7, 1, ptr(sums), ptr(aov), ptr(acc)) == 0
    for (w, h, x0, y0, tw, th, n, fl) in ((6, 4, 0, 0, 7, 4, 1, 0), (6, 4, 1, 0, 6, 4, 1, 0), (6, 4, 0, 1, 6, 4, 1, 0), (6, 4, 6, 0, 1, 1, 1, 0),
                                          (6, 4, 0, 0, 0, 4, 1, 0), (6, 4, 0, 0, 6, 0, 1, 0), (6, 4, 0, 0, 6, 4, 0, 0), (6, 4, 0, 0, 6, 4, 1, 2),
                                          (0, 4, 0, 0, 1, 1, 1, 0), (6, 4, 2 ** 32 - 1, 0, 2, 1, 1, 0)):
        assert mg(w, h, x0, y0, tw, th, n, fl, ptr(sums), ptr(aov), ptr(acc)) == rt.ERR_INVALID, (w, h, x0, y0, tw, th, n, fl)
    for i in range(3):
        args = [ptr(sums), ptr(aov), ptr(acc)]
        args[i] = None
        assert mg(6, 4, 0, 0, 6, 4, 1, 0, *args) == rt.ERR_INVALID
    with pytest.raises(rt.Rt1wError):
        rt.accum_resolve_host(acc, 0)
    for tile in (0, 8, 24, 272):
        with pytest.raises(rt.Rt1wError):
            rt.tile_error_host(acc, tile)


def test_merge_known_answers(rt):
    """K batches of a whole frame merged in order: S is the batch-order sum bit for bit, frame is rt1w_resolve of it, spp = K n, and var is
    rt1w_batch_variance's within 1e-12 relative -- Welford against two passes is not bit-equal; both are within a few ulp of the exact
    variance as long as it is not small against the mean squared, so the batches here keep their rms deviation above 0.05 of their mean
    (tests/test_denoise_reference.py has the argument).  Equal batches: var == 0 and err == 0 exactly."""
    h, w, n, K = 9, 21, 4, 6
    rng = np.random.default_rng(16)
    aov = _guides(h, w)
    aov[..., 0:3] = rng.uniform(0.005, 1.0, (h, w, 3))
    for keep in (False, True):
        sums = rng.uniform(0.0, 8.0, (K, h, w, 3))
        A = np.ones(3) if keep else np.maximum(aov[..., 0:3], 0.01)
        lk = ((sums / n) / A) @ LUM
        assert np.all(lk.std(0) > 0.05 * lk.mean(0))
        acc = np.zeros((h, w, 8))
        for k in range(K):
            acc = rt.accum_merge_host(acc, sums[k], aov, n, keep_albedo=keep)
            assert np.all(acc[..., 3] == k + 1)
        assert _same(acc[..., 0:3], _batch_order_sum(sums))
        frame, var, spp = rt.accum_resolve_host(acc, n)
        tf, tv = rt.batch_variance_host(sums, aov, n, keep_albedo=keep)
        rel = np.abs(var - tv) / tv
        print("keep", keep, "max relative difference of Welford and two-pass variance", rel.max())
        assert _same(frame, tf) and np.all(spp == K * n) and rel.max() <= 1e-12
        # the plain pair: against the definition in numpy
        lp = (sums / n) @ LUM
        want = ((lp - lp.mean(0)) ** 2).sum(0)
        assert np.all(np.abs(acc[..., 7] - want) <= 1e-12 * want) and np.all(np.abs(acc[..., 6] - lp.mean(0)) <= 1e-13 * lp.mean(0))
    # m < 2: no variance, no error
    one = rt.accum_merge_host(np.zeros((h, w, 8)), sums[0], aov, n)
    f1, v1, s1 = rt.accum_resolve_host(one, n)
    assert np.all(v1 == 0.0) and np.all(s1 == n) and _same(f1, rt.resolve(sums[0], n)) and np.all(rt.tile_error_host(one, 16) == 0.0)
    fe, ve, se = rt.accum_resolve_host(np.zeros((h, w, 8)), n)   # empty
    assert not fe.any() and not ve.any() and not se.any()
    # equal batches: d = 0 at every step after the first, so M2 stays exactly 0
    acc = np.zeros((h, w, 8))
    for k in range(5):
        acc = rt.accum_merge_host(acc, sums[1], aov, n)
    _, var, spp = rt.accum_resolve_host(acc, n)
    assert np.all(var == 0.0) and np.all(acc[..., 5] == 0.0) and np.all(acc[..., 7] == 0.0) and np.all(spp == 5 * n)
    assert np.all(rt.tile_error_host(acc, 16) == 0.0)
    # a rectangle touches its pixels only
    part = rt.accum_merge_host(acc, sums[2][2:5, 3:10], aov, n, x0=3, y0=2)
    inside = np.zeros((h, w), dtype=bool)
    inside[2:5, 3:10] = True
    assert _same(part[~inside], acc[~inside]) and np.all(part[inside][:, 3] == 6)
    full = rt.accum_merge_host(acc, sums[2], aov, n)
    assert _same(part[inside], full[inside])


def test_non_finite_batches(rt):
    """A NaN batch and an inf batch: still added to S and m; both Welford pairs keep their means, get the marker in M2 and stay marked;
    resolve gives var 0 (and scrubs a NaN sum as rt1w_resolve does), the tile error counts the pixel as 0; the neighbours are untouched."""
    h, w, n = 6, 7, 2
    rng = np.random.default_rng(4)
    aov = _guides(h, w)
    sums = rng.uniform(0.5, 2.0, (4, h, w, 3))
    clean = np.zeros((h, w, 8))
    for k in range(4):
        clean = rt.accum_merge_host(clean, sums[k], aov, n)
    bad = sums.copy()
    bad[2, 1, 2, 0] = np.nan
    bad[1, 3, 4, 2] = np.inf
    acc = np.zeros((h, w, 8))
    for k in range(4):
        acc = rt.accum_merge_host(acc, bad[k], aov, n)
        if k == 1:
            assert acc[3, 4, 5] == rt.ACCUM_NO_ESTIMATE and acc[3, 4, 7] == rt.ACCUM_NO_ESTIMATE and acc[1, 2, 5] >= 0.0
            mean_before = acc[3, 4, [4, 6]].copy()
    assert np.all(acc[..., 3] == 4)
    assert acc[1, 2, 5] == acc[1, 2, 7] == acc[3, 4, 5] == acc[3, 4, 7] == rt.ACCUM_NO_ESTIMATE
    assert np.array_equal(acc[3, 4, [4, 6]], mean_before)      # untouched since the batch that marked it
    assert np.isnan(acc[1, 2, 0]) and acc[3, 4, 2] == np.inf
    ok = np.ones((h, w), dtype=bool)
    ok[1, 2] = ok[3, 4] = False
    assert _same(acc[ok], clean[ok])
    frame, var, spp = rt.accum_resolve_host(acc, n)
    assert var[1, 2] == 0.0 and var[3, 4] == 0.0 and frame[1, 2, 0] == 0.0 and frame[3, 4, 2] == np.inf and np.all(spp == 8)
    assert _same(frame, rt.resolve(_batch_order_sum(bad), 8))
    c2 = clean.copy()
    c2[1, 2, 7] = c2[3, 4, 7] = 0.0   # what these pixels add to the tile's sum: 0
    assert _same(rt.tile_error_host(acc, 16), rt.tile_error_host(c2, 16))
    # a demodulated luminance that overflows while the plain one does not marks both pairs too
    big = np.full((1, 1, 3), 1e307)
    a1 = rt.accum_merge_host(np.zeros((1, 1, 8)), big, np.zeros((1, 1, 8)), 1)
    assert a1[0, 0, 5] == a1[0, 0, 7] == rt.ACCUM_NO_ESTIMATE and a1[0, 0, 3] == 1.0


def _tile_error_by_hand(acc, tile):
    """the header's definition, in numpy scalars: e_p, the block tree over the row-major index, the blocks in row-major order"""
    H, W = acc.shape[:2]
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
                    for ly in range(16):
                        for lx in range(16):
                            x, y = X0 + lx, Y0 + ly
                            if x < W and y < H:
                                m, mean, m2 = acc[y, x, 3], acc[y, x, 6], acc[y, x, 7]
                                if m >= 2 and m2 >= 0:
                                    e = (m2 / (m * (m - 1.0))) / ((mean if mean > 0 else 0.0) + 0.01)
                                    v[ly * 16 + lx] = e if np.isfinite(e) else 0.0
                    stride = 128
                    while stride >= 1:
                        v[:stride] = v[:stride] + v[stride:2 * stride]
                        stride //= 2
                    total = total + v[0]
            px = (min(W, (tx + 1) * tile) - tx * tile) * (min(H, (ty + 1) * tile) - ty * tile)
            out[ty, tx] = total / np.float64(px)
    return out


def test_tile_error_by_hand(rt):
    """17 x 33 with tile 16: partial tiles on both edges (a 1-pixel column, a 1-pixel row, a 1 x 1 corner).  The values span 16 decades, so
    their sum depends on the association: the twin must take the header's -- checked against it restated in numpy, bit for bit, and shown
    to differ from numpy's own pairwise sum; then tile 32 over the same frame (blocks in row-major order inside a tile)."""
    H, W = 33, 17
    rng = np.random.default_rng(33)
    acc = np.zeros((H, W, 8))
    acc[..., 3] = rng.integers(2, 9, (H, W))
    acc[..., 6] = rng.uniform(-0.2, 2.0, (H, W))          # negative means are clamped to 0
    acc[..., 7] = 10.0 ** rng.uniform(-12, 4, (H, W))
    acc[5, 3, 3] = 1.0                                    # m < 2
    acc[6, 3, 7] = rt.ACCUM_NO_ESTIMATE
    acc[7, 3, 7] = np.inf
    acc[8, 3, 6] = np.nan                                 # a NaN mean counts as 0
    for tile in (16, 32):
        got = rt.tile_error_host(acc, tile)
        want = _tile_error_by_hand(acc, tile)
        assert got.shape == want.shape == _tiles(W, H, tile)[::-1]
        assert _same(got, want), (tile, got, want)
    got = rt.tile_error_host(acc, 16)
    m, mean, m2 = acc[:16, :16, 3], acc[:16, :16, 6], acc[:16, :16, 7]
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where((m >= 2) & (m2 >= 0), (m2 / (m * (m - 1.0))) / (np.maximum(np.nan_to_num(mean), 0.0) + 0.01), 0.0)
    e[~np.isfinite(e)] = 0.0
    seq = 0.0
    for x in e.ravel():
        seq += x
    assert abs(got[0, 0] - e.sum() / 256) <= 1e-12 * got[0, 0]
    assert got[0, 0] != seq / 256.0, "the values do not tell the tree from a sequential sum"
    # the 1 x 1 corner tile: its one pixel's e_p over 1 pixel
    y, x = 32, 16
    assert got[2, 1] == (acc[y, x, 7] / (acc[y, x, 3] * (acc[y, x, 3] - 1.0))) / (max(acc[y, x, 6], 0.0) + 0.01)


def test_select(rt):
    """One round: order by err descending with ties by index, target_error and max_spp cut candidates, the round's share and the budget
    end it, at least one tile is taken while the budget allows, and nothing taken means the loop ends."""
    W, H, tile = 64, 48, 16                  # 4 x 3 tiles of 256 pixels, 3072 pixels
    base = dict(tile=tile, batch_spp=2, pilot_batches=2, budget_spp=64, max_spp=64)
    err = np.array([[1.0, 5.0, 3.0, 5.0], [0.5, 9.0, 0.0, 3.0], [2.0, 2.0, 7.0, 1.0]])
    m = np.full((3, 4), 2, dtype=np.uint32)
    order = [5, 10, 1, 3, 2, 7, 8, 9, 0, 11, 4]          # err descending, ties (5.0: 1, 3; 3.0: 2, 7; 2.0: 8, 9) by index; tile 6 has err 0
    assert rt.adaptive_select(W, H, err, m, round_share=1.0, **base) == order
    assert rt.adaptive_select(W, H, err, m, round_share=0.25, **base) == order[:3]       # 768 pixels a round
    assert rt.adaptive_select(W, H, err, m, round_share=0.26, **base) == order[:3]
    assert rt.adaptive_select(W, H, err, m, round_share=0.01, **base) == order[:1]       # always at least one
    assert rt.adaptive_select(W, H, err, m, round_share=1.0, target_error=2.0, **base) == order[:6]   # err > target, not >=
    assert rt.adaptive_select(W, H, err, m, round_share=1.0, target_error=9.0, **base) == []
    m2 = m.copy()
    m2.flat[5] = 32                          # (m + 1) n = 66 > max_spp
    m2.flat[10] = 31                         # 64 <= 64: still a candidate
    assert rt.adaptive_select(W, H, err, m2, round_share=1.0, **{**base, "budget_spp": 2000}) == order[1:]
    # the budget: pilot spent 4 of `budget` samples per pixel; each tile costs 512 pixel-samples of budget * 3072
    for budget, n_taken in ((4, 0), (5, 6), (6, 11), (7, 11)):
        got = rt.adaptive_select(W, H, err, m, round_share=1.0, **{**base, "budget_spp": budget})
        assert got == order[:n_taken], (budget, got)
        spent = 4 * W * H + 512 * len(got)
        assert spent <= budget * W * H
    assert rt.adaptive_select(W, H, err, m, round_share=1.0, **{**base, "budget_spp": 4}) == []        # nothing fits: the loop ends
    # partial tiles count their own pixels: 40 x 20 has tiles of 256, 256, 128 / 64, 64, 32 pixels
    e2 = np.array([[1.0, 2.0, 3.0], [6.0, 5.0, 4.0]])
    mm = np.full((2, 3), 2, dtype=np.uint32)
    assert rt.adaptive_select(40, 20, e2, mm, round_share=0.2, **base) == [3, 4, 5]    # 64 + 64 + 32 = 160 = 0.2 * 800; + 128 would pass it
    assert rt.adaptive_select(40, 20, e2, mm, round_share=1.0, **{**base, "budget_spp": 5}) == [3, 4, 5, 2]  # 800 pixel-samples left: 2 (64 + 64 + 32 + 128) = 576, + 512 > 800
    # a NaN error is no candidate
    e3 = e2.copy()
    e3[1, 0] = np.nan
    assert rt.adaptive_select(40, 20, e3, mm, round_share=1.0, **base) == [4, 5, 2, 1, 0]
    # capacity: the count comes back whatever fits
    a = rt.adaptive_params(round_share=1.0, **base)
    out = np.zeros(2, dtype=np.uint32)
    n = rt._lib.rt1w_adaptive_select(C.byref(a), 4, 3, W, H, err.ctypes.data_as(C.c_void_p), m.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), 2)
    assert n == 11 and list(out) == order[:2]
    assert rt._lib.rt1w_adaptive_select(C.byref(a), 4, 3, W, H, err.ctypes.data_as(C.c_void_p), m.ctypes.data_as(C.c_void_p), None, 0) == 11


LOOP = dict(tile=16, batch_spp=2, pilot_batches=2, budget_spp=8, max_spp=16)


@functools.lru_cache(maxsize=None)
def _loop_case(one_by_one):
    rt = orc.rt()
    sc = rt.Scene.reference(5, build_seed=1)
    return (sc,) + _compose_cpu(rt, sc, 96, 96, LOOP, one_by_one=one_by_one)


def test_the_loop_is_what_it_says(rt):
    """The whole plan composed in Python from orc.flat_render of rectangles, the twins and rt1w_adaptive_select, Cornell 96 x 96, tile 16,
    2 samples a batch, pilot 2, budget 8, at most 16: (a) every pixel's S is the batch-order sum of flat_render of the WHOLE frame at that
    pixel's sample ranges, bit for bit; (b) adjacent taken tiles rendered as one rectangle or one by one: the same bits; (c) the budget
    and max_spp hold and every count is a multiple of the batch."""
    W = H = 96
    sc, acc, m, rounds, launches, aov = _loop_case(False)
    _, acc1, m1, rounds1, launches1, _ = _loop_case(True)
    print("rounds", rounds, "launches", launches, "one by one", launches1, "batches per tile", np.unique(m, return_counts=True))
    assert rounds >= 2 and launches < launches1 and m.max() > m.min()          # it adapts, and grouping groups
    assert _same(acc, acc1) and np.array_equal(m, m1) and rounds == rounds1     # (b)
    n = LOOP["batch_spp"]
    chunk = sc.default_chunk(W, H, n)
    whole = [orc.flat_render(sc, W, H, n, sample_offset=k * n, out_sum=True, chunk=chunk)[0] for k in range(int(m.max()))]
    mp = np.repeat(np.repeat(m, 16, axis=0), 16, axis=1)[:H, :W]
    want = whole[0].copy()
    for k in range(1, int(m.max())):
        want = np.where((mp > k)[..., None], want + whole[k], want)
    assert _same(acc[..., 0:3], want)                                           # (a)
    frame, var, spp = rt.accum_resolve_host(acc, n)
    assert np.array_equal(spp, mp * n) and np.array_equal(acc[..., 3], mp)
    assert spp.sum() <= LOOP["budget_spp"] * W * H and spp.max() <= 16 and np.all(spp % 2 == 0) and spp.min() >= 4   # (c)
    assert spp.sum() > (LOOP["budget_spp"] - 1) * W * H                        # and the budget is used


def _disp(c):
    return np.sqrt(np.clip(c, 0.0, 0.999))  # the displayed value, src/color.rs:56-65 (as test_denoise_var.py)


def _mse(a, b):
    return float(np.mean((_disp(a) - _disp(b)) ** 2))


@functools.lru_cache(maxsize=None)
def _quality_case(arm, budget):
    """mse against the converged frame of (adaptive, uniform, adaptive filtered, uniform filtered) and the samples adaptive spent"""
    rt = orc.rt()
    W, H = QUALITY[arm]
    sc = rt.Scene.reference(arm, build_seed=1)
    ref = np.load(os.path.join(GOLD, f"denoise_ref_arm{arm}.npy"))
    n = max(1, budget // 8)                  # the defaults of rt1w_adaptive_params, spelled out
    ad = dict(tile=16, batch_spp=n, pilot_batches=4, budget_spp=budget, max_spp=8 * budget)
    acc, m, rounds, launches, aov = _compose_cpu(rt, sc, W, H, ad)
    frame, var, spp = rt.accum_resolve_host(acc, n)
    assert spp.sum() <= budget * W * H
    # uniform: `budget` samples for every pixel -- at least what the adaptive frame spent -- as 4 batches, so that the filter has its variance
    k = budget // 4
    sums = np.stack([orc.flat_render(sc, W, H, k, sample_offset=b * k, out_sum=True)[0] for b in range(4)])
    uaov = rt.aov_host(sc, W, H, budget)
    uframe, uvar = rt.batch_variance_host(sums, uaov, k)
    return (_mse(frame, ref), _mse(uframe, ref), _mse(rt.denoise_var_host(frame, aov, var), ref), _mse(rt.denoise_var_host(uframe, uaov, uvar), ref),
            float(spp.sum()) / (W * H), rounds, launches, float(spp.max()))


@pytest.mark.parametrize("budget", [32, 128])
@pytest.mark.parametrize("arm", sorted(QUALITY))
def test_quality_against_converged_frames(rt, arm, budget):
    """The reason for the feature.  The adaptive frame of a budget of 32 / 128 mean samples per pixel (tile 16, the other parameters at
    their defaults, global_seed 0) against the uniform render of `budget` samples for every pixel, both unfiltered, in the mean squared
    error of the displayed values against the converged frame (another seed).  Where adaptive sampling measured better than uniform it
    must keep at least half of that; where it measured no better (DESIGN.md section 16 says where and why) it must not get worse than
    1.1 x what was measured.  Arm 4 -- one small light, a mostly dark frame -- must come out below 1 at both budgets."""
    m_ad, m_un, f_ad, f_un, mean_spp, rounds, launches, top = _quality_case(arm, budget)
    ratio, measured = m_ad / m_un, MEASURED_RATIO[(arm, budget)]
    print(f"arm {arm} budget {budget}: mse adaptive {m_ad:.6g} uniform {m_un:.6g} ratio {ratio:.4f} (measured {measured}); spent {mean_spp:.2f} "
          f"per pixel, most {top:.0f}, {rounds} rounds, {launches} launches")
    if measured < 1.0:
        assert ratio <= (measured + 1.0) / 2.0
    else:
        assert ratio <= 1.1 * measured
    if arm == 4:
        assert ratio < 1.0


@pytest.mark.parametrize("budget", [32, 128])
@pytest.mark.parametrize("arm", sorted(QUALITY))
def test_quality_with_the_filter(rt, arm, budget):
    """The same with rt1w_denoise_var on both sides: adaptive (guides of the pilot's samples, Welford variance) against uniform (4 batches,
    rt1w_batch_variance, guides of all samples) at `budget` samples.  Recorded; asserted only not to get worse than 1.1 x the measurement."""
    m_ad, m_un, f_ad, f_un, *_ = _quality_case(arm, budget)
    ratio = f_ad / f_un
    print(f"arm {arm} budget {budget}: filtered mse adaptive {f_ad:.6g} uniform {f_un:.6g} ratio {ratio:.4f} (measured {MEASURED_RATIO_FILTERED[(arm, budget)]})")
    assert ratio <= 1.1 * MEASURED_RATIO_FILTERED[(arm, budget)]


# ------------------------------------------------------------------------------------------------------------------ GPU tier --

W_GPU, H_GPU = 203, 149   # not a multiple of 8 or 16
GPU_AD = dict(batch_spp=2, pilot_batches=2, budget_spp=8, max_spp=16)


@pytest.mark.gpu
@pytest.mark.parametrize("arm", [0, 5, 7])
def test_gpu_kernels_equal_twins(rt, gpu_ctx_factory, arm):
    """rt1w_accum_merge, rt1w_accum_resolve and rt1w_accum_tile_error == the CPU twins bit for bit on rendered batches: whole-frame
    merges, rectangles at the right and bottom edge, 1 x 1, one full row, one full column, tiles 16 and 48, both flag settings, a frame
    with a NaN and an inf batch pixel; grid / block as documented."""
    W, H, n = W_GPU, H_GPU, 2
    sc = rt.Scene.reference(arm, build_seed=1, aspect_ratio=W / H)
    ctx = gpu_ctx_factory(sc)
    chunk = sc.default_chunk(W, H, n)
    aov = ctx.render_aov(W, H, 4)
    b = [ctx.render(W, H, n, sample_offset=k * n, out_sum=True, chunk=chunk)[0] for k in range(3)]
    for keep in (False, True):
        g = t = np.zeros((H, W, 8))
        for k in range(2):
            g, st = ctx.accum_merge(g, b[k], aov, n, keep_albedo=keep, with_stats=True)
            t = rt.accum_merge_host(t, b[k], aov, n, keep_albedo=keep)
            assert _same(g, t), (arm, keep, k)
            assert st["block"] == 256 and st["grid"] == ((W + 15) // 16) * ((H + 15) // 16) and st["kernel_ms"] > 0 and st["passes"] == 1
        for (x0, y0, tw, th) in ((190, 10, 13, 20), (30, 140, 50, 9), (187, 133, 16, 16), (77, 51, 1, 1), (0, 60, W, 1), (101, 0, 1, H), (16, 32, 48, 16)):
            s = np.ascontiguousarray(b[2][y0:y0 + th, x0:x0 + tw])   # a rectangle's sums are the frame's sums there (same chunk)
            g2, st = ctx.accum_merge(g, s, aov, n, x0=x0, y0=y0, keep_albedo=keep, with_stats=True)
            assert _same(g2, rt.accum_merge_host(t, s, aov, n, x0=x0, y0=y0, keep_albedo=keep)), (arm, keep, x0, y0, tw, th)
            assert st["grid"] == ((tw + 15) // 16) * ((th + 15) // 16) and st["block"] == 256
            if tw * th > 1:
                g, t = g2, rt.accum_merge_host(t, s, aov, n, x0=x0, y0=y0, keep_albedo=keep)   # uneven counts for what follows
        frame, var, spp, st = ctx.accum_resolve(g, n, with_stats=True)
        tf, tv, ts = rt.accum_resolve_host(t, n)
        assert _same(frame, tf) and _same(var, tv) and _same(spp, ts) and spp.max() > spp.min() and var.max() > 0.0 and var.min() >= 0.0
        assert st["block"] == 256 and st["grid"] == ((W + 15) // 16) * ((H + 15) // 16)
        for tile in (16, 48):
            err, st = ctx.accum_tile_error(g, tile, with_stats=True)
            assert err.shape == ((H + tile - 1) // tile, (W + tile - 1) // tile) and _same(err, rt.tile_error_host(t, tile)), (arm, keep, tile)
            assert st["block"] == 256 and st["grid"] == err.size and err.max() > 0.0
    # a rendered rectangle is the frame's rectangle (what the plan rests on), through the GPU
    rect = (187, 133, 16, 16)
    assert _same(ctx.render(W, H, n, tile=rect, sample_offset=2 * n, out_sum=True, chunk=chunk)[0], b[2][133:149, 187:203])
    if arm == 5:
        bad = [x.copy() for x in b]
        bad[0][30, 40] = np.nan
        bad[1][80, 90, 2] = np.inf
        g = t = np.zeros((H, W, 8))
        for k in range(3):
            g = ctx.accum_merge(g, bad[k], aov, n)
            t = rt.accum_merge_host(t, bad[k], aov, n)
            assert _same(g, t)
        assert g[30, 40, 5] == g[80, 90, 7] == rt.ACCUM_NO_ESTIMATE and g[30, 40, 3] == 3.0
        for got, want in zip(ctx.accum_resolve(g, n), rt.accum_resolve_host(t, n)):
            assert _same(got, want)
        assert _same(ctx.accum_tile_error(g, 16), rt.tile_error_host(t, 16))
    for kw in (dict(x0=200, y0=0), dict(x0=0, y0=140)):
        with pytest.raises(rt.Rt1wError) as e:
            ctx.accum_merge(g, b[0][:16, :16], aov, n, **kw)
        assert e.value.code == rt.ERR_INVALID
    with pytest.raises(rt.Rt1wError) as e:
        ctx.accum_tile_error(g, 24)
    assert e.value.code == rt.ERR_INVALID and "tile" in str(e.value)


class _DeviceBuffers:
    """plain device memory of the HIP runtime this process already uses (as tests/test_denoise_var.py)"""

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

    def fetch(self, p, shape):
        out = np.empty(shape)
        assert self.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(p), C.c_size_t(out.nbytes), 2) == 0  # DeviceToHost
        return out

    def free(self):
        for p in self.made:
            self.hip.hipFree(p)


def _compose_device(rt, ctx, sc, W, H, ad, dev, filtered, global_seed=0):
    """the plan over the public DEVICE entries: (frame, spp, rounds, launches, paths)"""
    tile, n, P = ad["tile"], ad["batch_spp"], ad["pilot_batches"]
    npix = W * H
    chunk = sc.default_chunk(W, H, n)
    tx_n, ty_n = _tiles(W, H, tile)
    d_aov, d_sums, d_acc = dev.alloc(npix * 64), dev.alloc(npix * 24), dev.alloc(npix * 64, zero=True)
    d_err, d_frame, d_var, d_spp = dev.alloc(tx_n * ty_n * 8), dev.alloc(npix * 24), dev.alloc(npix * 8), dev.alloc(npix * 8)
    ctx.render_aov_device(d_aov, W, H, P * n, global_seed=global_seed)
    paths = 0
    launches = 0

    def batch(rect, mt):
        nonlocal paths, launches
        st = ctx.render_device(d_sums, W, H, n, tile=rect, sample_offset=mt * n, global_seed=global_seed, chunk=chunk, out_sum=True)
        ctx.accum_merge_device(d_acc, d_sums, d_aov, W, H, rect, n)
        paths += st["paths"]
        launches += 1
    for b in range(P):
        batch((0, 0, W, H), b)
    m = np.full((ty_n, tx_n), P, dtype=np.uint32)
    rounds = 0
    while True:
        ctx.accum_tile_error_device(d_acc, d_err, W, H, tile)
        taken = rt.adaptive_select(W, H, dev.fetch(d_err, (ty_n, tx_n)), m, **ad)
        if not taken:
            break
        rounds += 1
        for (x0, y0, tw, th, mt) in _runs(taken, m, tile, W, H):
            batch((x0, y0, tw, th), mt)
        for t in taken:
            m.flat[t] += 1
    ctx.accum_resolve_device(d_acc, d_frame, d_var, d_spp, W, H, n)
    if filtered:
        ctx.denoise_var_device(d_frame, d_aov, d_var, d_frame, W, H)
    return dev.fetch(d_frame, (H, W, 3)), dev.fetch(d_spp, (H, W)), rounds, launches, paths


@pytest.mark.gpu
@pytest.mark.parametrize("tile", [16, 48])
@pytest.mark.parametrize("arm", [5, 7])
def test_gpu_one_call_equals_composition(rt, gpu_ctx_factory, arm, tile):
    """rt1w_render_adaptive == the plan composed in Python over the public device entries, bit for bit, frame and spp map, with and without
    the filter; and == the CPU-tier composition of the twins over orc.flat_render.  What it refuses."""
    W, H = W_GPU, H_GPU
    ad = dict(tile=tile, **GPU_AD)
    sc = rt.Scene.reference(arm, build_seed=1, aspect_ratio=W / H)
    ctx = gpu_ctx_factory(sc)
    dev = _DeviceBuffers()
    try:
        for filtered in (False, True):
            frame, spp, rounds, launches, paths = _compose_device(rt, ctx, sc, W, H, ad, dev, filtered, global_seed=3)
            one, ospp, st = ctx.render_adaptive(W, H, adaptive=ad, filter=filtered, global_seed=3, with_stats=True)
            assert _same(one, frame) and _same(ospp, spp), (arm, tile, filtered)
            assert st["paths"] == paths == int(spp.sum()) and st["n_chunks"] == rounds and rounds >= 1 and st["passes"] >= launches
            assert st["block"] == 256 and st["grid"] == ((W + 15) // 16) * ((H + 15) // 16) and st["kernel_ms"] > 0 and st["total_ms"] > 0
            assert spp.sum() <= 8 * W * H and spp.max() <= 16 and spp.min() >= 4 and np.all(spp % 2 == 0) and spp.max() > spp.min()
    finally:
        dev.free()
    acc, m, crounds, _, aov = _compose_cpu(rt, sc, W, H, ad, global_seed=3)
    cf, cv, cs = rt.accum_resolve_host(acc, ad["batch_spp"])
    assert _same(cs, spp) and crounds == rounds
    assert _same(rt.denoise_var_host(cf, aov, cv), frame)       # `frame` is the filtered composition of the last pass
    assert _same(ctx.render_adaptive(W, H, adaptive=ad, global_seed=3)[0], cf)
    if tile != 16:
        return
    for bad in (dict(adaptive=dict(ad, tile=24)), dict(adaptive=dict(ad, pilot_batches=1)), dict(adaptive=dict(ad, pilot_batches=17)),
                dict(adaptive=dict(ad, max_spp=3)), dict(adaptive=dict(ad, target_error=-1.0)), dict(adaptive=dict(ad, target_error=float("inf"))),
                dict(adaptive=dict(ad, size=44)), dict(adaptive=ad, sigma_variance=-1.0), dict(adaptive=ad, denoise=dict(iterations=9)),
                dict(adaptive=ad, tile=(0, 0, W, 30)), dict(adaptive=ad, sample_offset=2 ** 32 - 10)):
        with pytest.raises(rt.Rt1wError) as e:
            ctx.render_adaptive(W, H, **bad)
        assert e.value.code == rt.ERR_INVALID, bad
    for flags, name in ((rt.OUT_SUM, "RT1W_OUT_SUM"), (rt.OUT_FRAME, "RT1W_OUT_FRAME"), (rt.RNG_REFERENCE, "RT1W_RNG_REFERENCE"),
                        (rt.PROBE_COHERENT, "RT1W_PROBE_COHERENT")):
        with pytest.raises(rt.Rt1wError) as e:
            ctx.render_adaptive(W, H, adaptive=ad, flags=flags)
        assert e.value.code == rt.ERR_INVALID and name in str(e.value)
    with pytest.raises(rt.Rt1wError) as e:
        ctx.render_adaptive(W, H, adaptive=ad, tile=(0, 0, W, 30), strips=(10, 30))
    assert e.value.code == rt.ERR_INVALID and "strip_rows" in str(e.value)
    with pytest.raises(rt.Rt1wError) as e:
        ctx.render_adaptive(W, H, adaptive=ad, precision=1)
    assert e.value.code == rt.ERR_INVALID and "RT1W_PRECISION_F32" in str(e.value)


@pytest.mark.gpu
def test_gpu_renders_are_unchanged_by_an_adaptive_call(rt, gpu_ctx_factory):
    """The entry shares the context's framebuffer, batch buffer and stream with the render entries and owns the accumulator buffer: a
    plain render, an AOV render and a variance-guided denoise after it equal the ones before, bit for bit, and the buffers grow."""
    sc = rt.Scene.reference(5, build_seed=1)
    ctx = gpu_ctx_factory(sc)
    f0, s0 = ctx.render(90, 70, 8)
    a0 = ctx.render_aov(90, 70, 8)
    v0 = ctx.render_denoised_var(90, 70, 8)
    ad = dict(tile=16, **GPU_AD)
    r0, p0 = ctx.render_adaptive(90, 70, adaptive=ad)
    ctx.render_adaptive(200, 150, adaptive=dict(ad, tile=32), filter=True)   # larger than anything so far: every buffer grows
    f1, s1 = ctx.render(90, 70, 8)
    assert _same(f0, f1) and s0["segments"] == s1["segments"] and _same(a0, ctx.render_aov(90, 70, 8))
    assert _same(v0, ctx.render_denoised_var(90, 70, 8))
    r1, p1 = ctx.render_adaptive(90, 70, adaptive=ad)
    assert _same(r0, r1) and _same(p0, p1)


@pytest.mark.gpu
def test_gpu_full_frame(rt, gpu_ctx_factory):
    """Cornell 600 x 600, a budget of 16 samples per pixel, every other parameter at its default: completes, stays within the budget and
    max_spp, and stats.paths is the sum of the spp map."""
    sc = rt.Scene.reference(5, build_seed=1)
    ctx = gpu_ctx_factory(sc)
    frame, spp, st = ctx.render_adaptive(600, 600, adaptive=dict(budget_spp=16), with_stats=True)
    print(f"C3 adaptive budget 16: {st['n_chunks']} rounds, {st['passes']} render launches, kernels {st['kernel_ms']:.2f} ms, total {st['total_ms']:.2f} ms, "
          f"spp {spp.min():.0f} .. {spp.max():.0f}, mean {spp.mean():.3f}")
    assert frame.shape == (600, 600, 3) and np.all(np.isfinite(frame))
    assert st["paths"] == int(spp.sum()) and spp.sum() <= 16 * 600 * 600 and spp.max() <= 128 and spp.min() >= 8 and st["n_chunks"] >= 1
    assert spp.sum() > 15 * 600 * 600 and spp.max() > spp.min()
