"""Full-count guides for adaptive sampling (rt1w_render_aov_tiles, rt1w_guides_merge_tiles, rt1w_guides_resolve and their device forms,
rt1w_render_adaptive_guided, include/rt1w.h).  CPU tier: the ABI surface and the refusals that need no GPU, the tile sums' twin against the
rectangle entry's twin bit for bit, merge and resolve by hand, the association bound of several merges, the whole plan composed from the twins
and its quality against converged frames.  GPU tier: the kernels bit for bit against the twins and against rt1w_render_aov_device, the one
call against the composition of the public device entries, and non-interference."""
import ctypes as C
import functools
import json
import os
import sys

import numpy as np
import pytest

import orc
import test_adaptive_filtered as TF   # the plan of rt1w_render_adaptive_filtered restated in Python, its quality cases and device buffers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
REFUSALS = os.path.join(GOLD, "guides_refusals.json")
LUM = TF.LUM
_same = TF._same

# mse(rt1w_render_adaptive_guided's frame) / mse(uniform 4 batches + rt1w_batch_variance + rt1w_denoise_var at `budget` samples, guides over all
# `budget` samples), displayed values, measured with the twins at tile 16 and otherwise default parameters, global_seed 0 (DESIGN.md section
# 19).  Keys: (arm, budget).  rt1w_render_adaptive_filtered has TF.MEASURED_RATIO beside it: geometric mean 0.947.
MEASURED_RATIO = {(5, 32): 0.7907, (5, 128): 0.8944, (4, 32): 0.7483, (4, 128): 0.8235, (7, 32): 1.1288, (7, 128): 0.9386}
# test_calibration's protocol of tests/test_adaptive_filtered.py through the guide accumulator (uniform sampling: the guides are full-count there already)
MEASURED_CALIBRATION = 0.205


def _all_tiles(W, H, tile, offset=0):
    return [(x, y, offset) for y in range(0, H, tile) for x in range(0, W, tile)]


def _finish(sums, spp):
    """the contract's finish of raw sums [..., 8]: 0-5 and 7 s / spp, 6 s7 > 0 ? s6 / s7 : +inf"""
    out = sums / np.float64(spp)
    with np.errstate(all="ignore"):
        out[..., 6] = np.where(sums[..., 7] > 0, sums[..., 6] / sums[..., 7], np.inf)
    return out


def _check_tile_sums(sums, W, H, spp, tile, tiles, rect_aov):
    """every tile's pixels inside the frame finish to rect_aov(rectangle, absolute offset)'s bits; the others are +0.0"""
    assert sums.shape == (len(tiles), tile, tile, 8)
    for k, (x, y, off) in enumerate(tiles):
        tw, th = min(tile, W - x), min(tile, H - y)
        assert _same(_finish(sums[k, :th, :tw], spp), rect_aov((x, y, tw, th), off)), (k, x, y, off)
        outside = np.concatenate([sums[k, th:].ravel(), sums[k, :, tw:].ravel()])
        assert not outside.any() and not np.signbit(outside).any(), k


def _lists(W, H, tile, rng):
    """one tile; every tile shuffled, one of them once more with another offset"""
    every = _all_tiles(W, H, tile, 4)
    order = [every[i] for i in rng.permutation(len(every))]
    return [[every[-1]], order + [(every[0][0], every[0][1], 9)]]


# ---- the plan, restated in Python over the twins: what rt1w_render_adaptive_guided says it does ----

def _compose_cpu(rt, sc, W, H, ad, global_seed=0, check=None):
    """returns (out, spp, err_px, pairs per tile, rounds, render launches, pilot feature buffer, gacc)"""
    tile, n, P = ad["tile"], ad["batch_spp"], ad["pilot_batches"]
    chunk = sc.default_chunk(W, H, n)
    every = _all_tiles(W, H, tile)
    gacc = rt.guides_merge_tiles_host(np.zeros((H, W, 9)), rt.aov_tiles_host(sc, W, H, P * n, tile, every, global_seed=global_seed), P * n, tile, every)
    pilot_aov = rt.guides_resolve_host(gacc)
    acc = [np.zeros((H, W, 8)), np.zeros((H, W, 8))]
    launches = 0
    for b in range(P):
        sums = orc.flat_render(sc, W, H, n, sample_offset=b * n, out_sum=True, chunk=chunk, global_seed=global_seed)[0]
        acc[b & 1] = rt.accum_merge_host(acc[b & 1], sums, pilot_aov, n)
        launches += 1
    tx_n, ty_n = TF._tiles(W, H, tile)
    m = np.full((ty_n, tx_n), P // 2, dtype=np.uint32)
    rounds = 0
    while True:
        frame, var, ha, hb, spp = rt.halves_resolve_host(acc[0], acc[1], n)
        guides = rt.guides_resolve_host(gacc)
        if check:
            check(acc, m, spp, gacc, guides, pilot_aov)
        out, err_px = rt.denoise_var_halves_host(frame, guides, var, ha, hb)
        taken = rt.adaptive_select(W, H, rt.tile_error_map_host(err_px, tile), m, **TF._pair_params(ad))
        if not taken:
            return out, spp, err_px, m, rounds, launches, pilot_aov, gacc
        rounds += 1
        launches += 1
        corners = [((t % tx_n) * tile, (t // tx_n) * tile) for t in taken]
        for half in (0, 1):
            for t, (x, y) in zip(taken, corners):
                rect = (x, y, min(tile, W - x), min(tile, H - y))
                sums = orc.flat_render(sc, W, H, n, tile=rect, sample_offset=(2 * int(m.flat[t]) + half) * n, out_sum=True, chunk=chunk, global_seed=global_seed)[0]
                acc[half] = rt.accum_merge_host(acc[half], sums, pilot_aov, n, x0=x, y0=y)
        tl = [(x, y, 2 * int(m.flat[t]) * n) for t, (x, y) in zip(taken, corners)]
        gacc = rt.guides_merge_tiles_host(gacc, rt.aov_tiles_host(sc, W, H, 2 * n, tile, tl, global_seed=global_seed), 2 * n, tile, tl)
        for t in taken:
            m.flat[t] += 1


# ------------------------------------------------------------------------------------------------------------------ CPU tier --

RENDER = dict(width=40, height=24, x0=0, y0=0, tile_w=40, tile_h=24, spp=3, sample_offset=0, max_depth=8, global_seed=0, chunk=0, flags=0)
TILES = [(0, 0, 0), (16, 0, 0)]
# (case, render members, tile, tiles): rt1w_render_aov_tiles refuses each before the context is looked at
AOV_TILES_CASES = [("tile 24", {}, 24, TILES), ("tile 8", {}, 8, TILES), ("tile 272", {}, 272, TILES), ("x0 off the grid", {}, 16, [(8, 0, 0)]),
                   ("y0 outside the frame", {}, 16, [(0, 32, 0)]), ("x0 outside the frame", {}, 16, [(48, 0, 0)]),
                   ("reserved 1", {}, 16, [(0, 0, 0, 1)]), ("no tile", {}, 16, []), ("spp 0", dict(spp=0), 16, TILES),
                   ("RT1W_OUT_SUM", dict(flags=1), 16, TILES), ("RT1W_GENERIC", dict(flags=8), 16, TILES), ("unknown flag", dict(flags=1 << 20), 16, TILES),
                   ("RT1W_PRECISION_F32", dict(precision=1), 16, TILES), ("precision 7", dict(precision=7), 16, TILES),
                   ("interleaved strips", dict(strip_rows=2, strip_period=4), 16, TILES), ("width 1", dict(width=1), 16, [(0, 0, 0)]),
                   ("sample index overflow", dict(sample_offset=2 ** 32 - 8), 16, [(0, 0, 0), (16, 0, 6)])]
# (case, width, height, tile, tiles, spp): rt1w_guides_merge_tiles likewise
MERGE_CASES = [("a tile twice", 40, 24, 16, [(0, 0, 0), (16, 0, 0), (0, 0, 7)], 3), ("spp 0", 40, 24, 16, TILES, 0), ("tile 24", 40, 24, 24, TILES, 3),
               ("x0 off the grid", 40, 24, 16, [(8, 0, 0)], 3), ("y0 outside the frame", 40, 24, 16, [(0, 32, 0)], 3), ("reserved 1", 40, 24, 16, [(0, 0, 0, 1)], 3),
               ("no tile", 40, 24, 16, [], 3), ("width 0", 0, 24, 16, TILES, 3)]
ADAPTIVE = dict(tile=16, batch_spp=2, pilot_batches=2, budget_spp=8, max_spp=16)


def _refusals(rt):
    """{entry: {case: [code, text]}} with a null context everywhere"""
    out = {"rt1w_render_aov_tiles": {}, "rt1w_guides_merge_tiles": {}, "rt1w_guides_resolve": {}, "rt1w_render_adaptive_guided": {}}
    buf = np.zeros(3 * 32 * 32 * 9)
    ptr = buf.ctypes.data_as(C.c_void_p)
    for name, pm, tile, tiles in AOV_TILES_CASES:
        p = rt.RenderParams()
        for k, v in dict(RENDER, **pm).items():
            setattr(p, k, v)
        rec, n = rt._tile_list(tiles)
        for fn in (rt._lib.rt1w_render_aov_tiles, rt._lib.rt1w_render_aov_tiles_device):
            got = [fn(None, C.byref(p), tile, rec, n, ptr, None), rt.last_error()]
            assert out["rt1w_render_aov_tiles"].setdefault(name, got) == got            # host and device form refuse alike
    for name, w, h, tile, tiles, spp in MERGE_CASES:
        rec, n = rt._tile_list(tiles)
        for fn in (rt._lib.rt1w_guides_merge_tiles, rt._lib.rt1w_guides_merge_tiles_device):
            got = [fn(None, w, h, tile, rec, n, spp, ptr, ptr, None), rt.last_error()]
            assert out["rt1w_guides_merge_tiles"].setdefault(name, got) == got
    for name, w, h in (("width 0", 0, 24), ("height 2^30 + 1", 40, 2 ** 30 + 1)):
        out["rt1w_guides_resolve"][name] = [rt._lib.rt1w_guides_resolve(None, w, h, ptr, ptr, None), rt.last_error()]
    rgb = np.zeros((32, 32, 3))
    for name, pm, am, sv in TF.REFUSAL_CASES:                                           # the plan's refusals, under this entry's name
        p = rt.RenderParams()
        for k, v in dict(TF.RENDER, **pm).items():
            setattr(p, k, v)
        a = rt.adaptive_params(**dict(TF.ADAPTIVE, **am))
        rc = rt._lib.rt1w_render_adaptive_guided(None, C.byref(p), C.byref(a), None, sv, rgb.ctypes.data_as(C.c_void_p), None, None, None)
        out["rt1w_render_adaptive_guided"][name] = [rc, rt.last_error()]
    return out


def test_abi_surface_and_refusals(rt):
    """The seven entries are exported with the declared arity, the twins exist.  What the parameters and the list alone decide is refused
    before the context is looked at, so these refusals need no GPU; the texts are recorded in tests/golden/guides_refusals.json (`python
    tests/test_guides.py --record`).  rt1w_render_adaptive_guided refuses what rt1w_render_adaptive_filtered refuses, the same texts with
    its own name where the entry is named.  A call without any defect then reaches the context check."""
    arity = {"rt1w_render_aov_tiles": 7, "rt1w_render_aov_tiles_device": 7, "rt1w_guides_merge_tiles": 10, "rt1w_guides_merge_tiles_device": 10,
             "rt1w_guides_resolve": 6, "rt1w_guides_resolve_device": 6, "rt1w_render_adaptive_guided": 9}
    lib = C.CDLL(rt.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "rt1w.h")).read()
    for name, n in arity.items():
        assert hasattr(lib, name), name
        assert len(getattr(rt._lib, name).argtypes) == n, name
        decl = hdr[hdr.index("int " + name + "("):]
        assert decl[:decl.index(";")].count(",") + 1 == n, name
    lab = rt.load_lab()
    for name in ("rt1w_lab_aov_tiles_host", "rt1w_lab_guides_merge_tiles_host", "rt1w_lab_guides_resolve_host"):
        assert hasattr(lab, name), name
    got = _refusals(rt)
    want = json.load(open(REFUSALS))
    assert sorted(got) == sorted(want)
    for entry in got:
        assert sorted(got[entry]) == sorted(want[entry]), entry
        for name in got[entry]:
            assert got[entry][name] == want[entry][name], (entry, name, got[entry][name], want[entry][name])
            unsupported = entry == "rt1w_render_aov_tiles" and name in ("RT1W_PRECISION_F32", "precision 7")
            assert got[entry][name][0] == (rt.ERR_UNSUPPORTED if unsupported else rt.ERR_INVALID), (entry, name)
    assert "twice" in got["rt1w_guides_merge_tiles"]["a tile twice"][1] and "spp" in got["rt1w_guides_merge_tiles"]["spp 0"][1]
    assert "f64 only" in got["rt1w_render_aov_tiles"]["RT1W_PRECISION_F32"][1] and "strips" in got["rt1w_render_aov_tiles"]["interleaved strips"][1]
    theirs = json.load(open(TF.REFUSALS))
    for name, (rc, text) in got["rt1w_render_adaptive_guided"].items():
        assert [rc, text] == [theirs[name][0], theirs[name][1].replace("rt1w_render_adaptive_filtered", "rt1w_render_adaptive_guided")], name
    assert "rt1w_render_adaptive_guided" in got["rt1w_render_adaptive_guided"]["tile 16 x 32"][1]
    # without a defect: the context check
    p = rt.RenderParams()
    for k, v in RENDER.items():
        setattr(p, k, v)
    buf = np.zeros(2 * 16 * 16 * 9)
    ptr = buf.ctypes.data_as(C.c_void_p)
    rec, n = rt._tile_list(TILES + [(0, 0, 5)])                                          # a repeat with another offset is no defect here
    assert rt._lib.rt1w_render_aov_tiles(None, C.byref(p), 16, rec, n, ptr, None) == rt.ERR_INVALID and "null argument" in rt.last_error()
    rec, n = rt._tile_list(TILES)
    assert rt._lib.rt1w_guides_merge_tiles(None, 40, 24, 16, rec, n, 3, ptr, ptr, None) == rt.ERR_INVALID and "null argument" in rt.last_error()
    assert rt._lib.rt1w_guides_resolve(None, 40, 24, ptr, ptr, None) == rt.ERR_INVALID and "null argument" in rt.last_error()
    a = rt.adaptive_params(**ADAPTIVE)
    for k, v in TF.RENDER.items():
        setattr(p, k, v)
    assert rt._lib.rt1w_render_adaptive_guided(None, C.byref(p), C.byref(a), None, 0.0, ptr, None, None, None) == rt.ERR_INVALID
    assert "null argument" in rt.last_error()
    # the twins refuse what the entries refuse
    sc = rt.Scene.reference(5, build_seed=1)
    for name, pm, tile, tiles in AOV_TILES_CASES:
        kw = dict(spp=dict(RENDER, **pm)["spp"], sample_offset=pm.get("sample_offset", 0), flags=pm.get("flags", 0), f32=pm.get("precision") == 1,
                  strips=(2, 4) if "strip_rows" in pm else None)
        if name in ("precision 7",):
            continue
        with pytest.raises(rt.Rt1wError) as e:
            rt.aov_tiles_host(sc, pm.get("width", 40), 24, kw.pop("spp"), tile, tiles, **kw)
        assert e.value.code == got["rt1w_render_aov_tiles"][name][0], name
    for name, w, h, tile, tiles, spp in MERGE_CASES:
        with pytest.raises(rt.Rt1wError):
            rt.guides_merge_tiles_host(np.zeros((max(h, 1), max(w, 1), 9)) if w else np.zeros((24, 0, 9)), np.zeros((len(tiles), tile, tile, 8)), spp, tile, tiles)


@functools.lru_cache(maxsize=None)
def _scene(arm, W, H):
    return orc.rt().Scene.reference(arm, build_seed=1, aspect_ratio=W / H)


@pytest.mark.parametrize("arm", [5, 0, 7])
def test_tile_sums_against_the_rectangle_entry(rt, arm):
    """rt1w_lab_aov_tiles_host on 40 x 24 with tile 16 (both edges clip a tile) and tile 32, and on a 10 x 7 frame, 3 samples: every tile
    of a shuffled list, one tile repeated with another offset, finishes to rt1w_lab_aov_host of its clipped rectangle at its absolute
    offset, bit for bit; pixels beyond the frame are +0.0; the list's order changes nothing."""
    rng = np.random.default_rng(arm)
    for W, H, tiles_of in ((40, 24, (16, 32)), (10, 7, (16,))):
        sc = _scene(arm, W, H)
        rect = functools.lru_cache(maxsize=None)(lambda r, off: rt.aov_host(sc, W, H, 3, tile=r, sample_offset=off, global_seed=2))
        for tile in tiles_of:
            for tiles in _lists(W, H, tile, rng):
                sums = rt.aov_tiles_host(sc, W, H, 3, tile, tiles, sample_offset=1, global_seed=2)
                _check_tile_sums(sums, W, H, 3, tile, tiles, lambda r, off: rect(r, off + 1))
                again = rt.aov_tiles_host(sc, W, H, 3, tile, tiles[::-1], sample_offset=1, global_seed=2)
                assert _same(again[::-1], sums)
                assert (W, H) != (40, 24) or len(tiles) == 1 or sums[..., 7].max() == 3.0   # pixels whose every sample hit


def _hostile_gacc(rng, H=21, W=37):
    """(gacc, tile sums of every 16-tile, the list): empty pixels, pixels without a hit, inf / NaN sums, negative zeros"""
    g = np.zeros((H, W, 9))
    g[..., 0:3] = rng.uniform(0.0, 8.0, (H, W, 3))
    g[..., 3:6] = rng.uniform(-8.0, 8.0, (H, W, 3))
    g[..., 7] = rng.integers(0, 9, (H, W))
    g[..., 6] = rng.uniform(1.0, 50.0, (H, W)) * g[..., 7]
    g[..., 8] = 8.0
    g[0:5, 0:9] = 0.0                      # empty pixels
    g[6, 6, 7] = g[6, 6, 6] = 0.0          # merged, no hit yet
    g[7, 7, 0] = np.inf
    g[8, 8, 4] = np.nan
    g[9, 9, 6] = np.inf
    g[10, 10, 3] = -0.0
    tiles = _all_tiles(W, H, 16)
    s = np.zeros((len(tiles), 16, 16, 8))
    s[..., 0:3] = rng.uniform(0.0, 4.0, s.shape[:3] + (3,))
    s[..., 3:6] = rng.uniform(-4.0, 4.0, s.shape[:3] + (3,))
    s[..., 7] = rng.integers(0, 5, s.shape[:3])
    s[..., 6] = rng.uniform(1.0, 50.0, s.shape[:3]) * s[..., 7]
    s[0, 1, 1, 3] = -0.0                   # into an empty pixel: the sign of the zero is kept
    s[0, 2, 2, 1] = np.nan
    s[0, 6, 6, 6:8] = 0.0                  # no hit again: +inf depth after the merge too
    s[0, 12, 12, 0] = np.inf
    return g, s, tiles


def _merge_by_hand(g, s, tile, tiles, spp):
    out = g.copy()
    H, W = g.shape[:2]
    for k, (x, y, _) in enumerate(tiles):
        for ly in range(min(tile, H - y)):
            for lx in range(min(tile, W - x)):
                r = out[y + ly, x + lx]
                if r[8] == 0.0:
                    r[0:8] = s[k, ly, lx]
                    r[8] = np.float64(spp)
                else:
                    r[0:8] = r[0:8] + s[k, ly, lx]
                    r[8] = r[8] + np.float64(spp)
    return out


def _resolve_by_hand(g):
    with np.errstate(all="ignore"):
        n = g[..., 8:9]
        aov = g[..., 0:8] / n
        aov[..., 6] = np.where(g[..., 7] > 0, g[..., 6] / g[..., 7], np.inf)
        empty = g[..., 8] == 0.0
        aov[empty] = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, np.inf, 0.0)
    return aov


def test_merge_and_resolve_by_hand(rt):
    """The header's definitions in numpy on a synthetic 37 x 21 accumulator (tiles clipped on both edges): the first merge takes the sums as
    they are (a -0.0 stays -0.0), the second adds, N counts the samples, an empty pixel resolves to (0, 0, 0, 0, 0, 0, +inf, 0), a pixel
    without a hit to +inf depth, inf / NaN sums are carried; pixels of a tile beyond the frame are skipped."""
    rng = np.random.default_rng(19)
    g, s, tiles = _hostile_gacc(rng)
    m1 = rt.guides_merge_tiles_host(g, s, 4, 16, tiles)
    assert _same(m1, _merge_by_hand(g, s, 16, tiles, 4))
    assert np.signbit(m1[1, 1, 3]) and m1[1, 1, 8] == 4.0 and m1[12, 12, 8] == 12.0 and np.isnan(m1[2, 2, 1]) and np.isinf(m1[12, 12, 0])
    m2 = rt.guides_merge_tiles_host(m1, s[::-1], 2, 16, tiles[::-1])                      # a second merge adds, whatever the list's order
    assert _same(m2, _merge_by_hand(m1, s[::-1], 16, tiles[::-1], 2)) and m2[1, 1, 8] == 6.0
    part = rt.guides_merge_tiles_host(g, s[1:2], 4, 16, tiles[1:2])                      # one tile: the others keep their bits
    want = _merge_by_hand(g, s[1:2], 16, tiles[1:2], 4)
    assert _same(part, want) and _same(part[:, :16], g[:, :16])
    for acc in (np.zeros_like(g), g, m1, m2):
        aov = rt.guides_resolve_host(acc)
        assert _same(aov, _resolve_by_hand(acc))
    aov = rt.guides_resolve_host(m1)
    empty = rt.guides_resolve_host(np.zeros((3, 5, 9)))
    assert _same(empty, np.broadcast_to(np.array([0, 0, 0, 0, 0, 0, np.inf, 0.0]), (3, 5, 8)))
    assert aov[6, 6, 6] == np.inf and aov[6, 6, 7] == 0.0 and np.isnan(aov[2, 2, 1]) and np.isinf(aov[12, 12, 0]) and np.isnan(aov[8, 8, 4])


@pytest.mark.parametrize("arm", [5, 0, 7])
def test_association_of_two_merges(rt, arm):
    """Two merges (a samples, then b at offset a) against one rt1w_lab_aov_host of a + b samples, 40 x 24: the hit count (and so the
    coverage) is exact; albedo and depth, sums of a + b non-negative terms added in another association, agree within (a + b) 2^-52
    relative; the normal, whose terms have magnitude <= 1, within (a + b) 2^-52 absolute.  One merge alone is the entry's bits."""
    W, H, a, b = 40, 24, 3, 5
    sc = _scene(arm, W, H)
    tiles = _all_tiles(W, H, 16)
    s1 = rt.aov_tiles_host(sc, W, H, a, 16, tiles)
    s2 = rt.aov_tiles_host(sc, W, H, b, 16, tiles, sample_offset=a)
    g1 = rt.guides_merge_tiles_host(np.zeros((H, W, 9)), s1, a, 16, tiles)
    assert _same(rt.guides_resolve_host(g1), rt.aov_host(sc, W, H, a))
    g2 = rt.guides_merge_tiles_host(g1, s2, b, 16, tiles)
    got, want = rt.guides_resolve_host(g2), rt.aov_host(sc, W, H, a + b)
    assert np.all(g2[..., 8] == a + b)
    assert _same(got[..., 7], want[..., 7]) and np.array_equal(g2[..., 7], want[..., 7] * (a + b))
    bound = (a + b) * 2.0 ** -52
    hit = want[..., 7] > 0
    assert np.array_equal(np.isinf(got[..., 6]), ~hit) and np.array_equal(np.isinf(want[..., 6]), ~hit)
    rel = np.abs(got[..., 0:3] - want[..., 0:3]) / np.maximum(np.abs(want[..., 0:3]), 1e-300)
    rel_d = np.abs(got[..., 6][hit] - want[..., 6][hit]) / want[..., 6][hit]
    err_n = np.abs(got[..., 3:6] - want[..., 3:6])
    print(f"arm {arm}: albedo {rel.max():.3g} depth {rel_d.max():.3g} relative, normal {err_n.max():.3g} absolute; bound {bound:.3g}")
    assert rel.max() <= bound and rel_d.max() <= bound and err_n.max() <= bound


LOOP = TF.LOOP


def test_the_loop_is_what_it_says(rt):
    """The plan composed from the twins at the LOOP settings of tests/test_adaptive_filtered.py, Cornell 48 x 40: at every estimate every
    pixel's N equals its entry in the spp map; the pilot feature buffer is rt1w_lab_aov_host over the pilot's samples, bit for bit, and
    stays what demodulates the merges; with rounds the guide buffer differs from the pilot's on taken tiles only, and there it is within
    the association bound of rt1w_lab_aov_host over the tile's samples; with a budget equal to the pilot the output is the bits of the
    rt1w_render_adaptive_filtered composition."""
    W, H = 48, 40
    n, P = LOOP["batch_spp"], LOOP["pilot_batches"]
    sc = _scene(5, W, H)
    seen = []

    def check(acc, m, spp, gacc, guides, pilot_aov):
        assert np.array_equal(gacc[..., 8], spp)                                         # N == the spp map at every estimate
        assert np.array_equal(acc[0][..., 3], acc[1][..., 3])
        seen.append((m.copy(), guides.copy()))
    out, spp, err_px, m, rounds, launches, pilot_aov, gacc = _compose_cpu(rt, sc, W, H, LOOP, check=check)
    print("rounds", rounds, "pairs per tile", np.unique(m, return_counts=True))
    assert rounds >= 2 and launches == P + rounds and m.max() > m.min() and len(seen) == rounds + 1
    assert _same(pilot_aov, rt.aov_host(sc, W, H, P * n)) and _same(seen[0][1], pilot_aov)
    mp = np.repeat(np.repeat(m, 16, axis=0), 16, axis=1)[:H, :W]
    assert np.array_equal(spp, mp * 2 * n) and spp.sum() <= LOOP["budget_spp"] * W * H
    final = seen[-1][1]
    moved = (final.view(np.uint64) != pilot_aov.view(np.uint64)).any(-1)
    assert moved.any() and not moved[mp == P // 2].any()                                 # untouched tiles keep the pilot's bits
    for j in np.unique(m):
        N = 2 * int(j) * n
        want = rt.aov_host(sc, W, H, N)
        sel = mp == j
        assert _same(final[sel][:, 7], want[sel][:, 7])
        assert np.all(np.abs(final[sel][:, 0:3] - want[sel][:, 0:3]) <= N * 2.0 ** -52 * np.abs(want[sel][:, 0:3]))
        assert np.all(np.abs(final[sel][:, 3:6] - want[sel][:, 3:6]) <= N * 2.0 ** -52)
    # budget == the pilot (two pairs: the least the pair plan accepts): no round takes a tile, and the guides are the pilot's
    flat = dict(LOOP, pilot_batches=4, budget_spp=4 * n)
    o1, s1, e1, m1, r1, l1, a1, g1 = _compose_cpu(rt, sc, W, H, flat)
    o0, s0, e0, m0, r0, l0, a0 = TF._compose_cpu(rt, sc, W, H, flat)
    assert r1 == r0 == 0 and _same(o1, o0) and _same(s1, s0) and _same(e1, e0) and _same(a1, a0)
    # and with rounds the frame is no longer that composition's
    assert not _same(out, TF._compose_cpu(rt, sc, W, H, LOOP)[0])


def test_calibration(rt):
    """tests/test_adaptive_filtered.py's calibration protocol with the guides read from the guide accumulator: Cornell 40 x 40, every pixel
    2 pairs of 4 samples, 24 global_seeds.  Sampling is uniform there, so the pilot's guides ARE full-count and the map is that test's map
    bit for bit: the ratio stays 0.205.  Full-count guides do not touch what makes the estimate understate (the shared weights)."""
    W = H = 40
    n, seeds = 4, 24
    sc = rt.Scene.reference(5, build_seed=1)
    tiles = _all_tiles(W, H, 16)
    est, lums = [], []
    for g in range(seeds):
        gacc = rt.guides_merge_tiles_host(np.zeros((H, W, 9)), rt.aov_tiles_host(sc, W, H, 4 * n, 16, tiles, global_seed=g), 4 * n, 16, tiles)
        aov = rt.guides_resolve_host(gacc)
        if g == 0:
            assert _same(aov, rt.aov_host(sc, W, H, 4 * n, global_seed=g))
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
    print(f"estimate {np.mean(est):.6g} truth {truth:.6g} ratio {ratio:.4f} (measured {MEASURED_CALIBRATION})")
    assert MEASURED_CALIBRATION / 2.0 <= ratio <= MEASURED_CALIBRATION * 2.0


def quality_case(arm, budget):
    """(mse of the guided call's frame as the twins compose it, mse of the uniform filtered frame with full-budget guides, mean spp, rounds)"""
    rt = orc.rt()
    W, H = TF.QUALITY[arm]
    sc = rt.Scene.reference(arm, build_seed=1)
    ref = np.load(os.path.join(GOLD, f"denoise_ref_arm{arm}.npy"))
    n = max(1, budget // 8)                  # the defaults of rt1w_adaptive_params, spelled out
    ad = dict(tile=16, batch_spp=n, pilot_batches=4, budget_spp=budget, max_spp=8 * budget)
    out, spp, err_px, m, rounds = _compose_cpu(rt, sc, W, H, ad)[:5]
    assert spp.sum() <= budget * W * H
    return TF._mse(out, ref), TF._uniform_filtered_mse(arm, budget), float(spp.mean()), rounds


@pytest.mark.parametrize("budget", [32, 128])
@pytest.mark.parametrize("arm", sorted(TF.QUALITY))
def test_quality_against_converged_frames(rt, arm, budget):
    """mse(the guided call's out) / mse(uniform 4 batches + rt1w_batch_variance + rt1w_denoise_var at `budget` samples, its guides over all
    `budget` samples), displayed values against the converged frame, tile 16 and otherwise default parameters, global_seed 0: the six cases
    and the denominator of DESIGN.md section 17.  By the project's rule: where it measured better than uniform it must keep at least half of
    that, elsewhere it must not get worse than 1.1 x the measurement (section 19 has the table beside section 17's row)."""
    m_ad, m_un, mean_spp, rounds = quality_case(arm, budget)
    ratio, measured = m_ad / m_un, MEASURED_RATIO[(arm, budget)]
    print(f"arm {arm} budget {budget}: mse guided adaptive {m_ad:.6g} uniform filtered {m_un:.6g} ratio {ratio:.4f} (measured {measured}, "
          f"filtered {TF.MEASURED_RATIO[(arm, budget)]}); spent {mean_spp:.2f} per pixel in {rounds} rounds")
    if measured < 1.0:
        assert ratio <= (measured + 1.0) / 2.0
    else:
        assert ratio <= 1.1 * measured


# ------------------------------------------------------------------------------------------------------------------ GPU tier --

W_GPU, H_GPU = 72, 40   # the width no multiple of 16: partly filled waves and a clipped tile column; the height clips tile 32's second row


@pytest.mark.gpu
@pytest.mark.parametrize("arm", [5, 0, 7])
def test_gpu_tile_sums_equal_twin_and_rectangle_entry(rt, gpu_ctx_factory, arm):
    """rt1w_render_aov_tiles == rt1w_lab_aov_tiles_host bit for bit at 72 x 40 and 10 x 7, 3 samples, tile 16 (one workgroup per tile) and 32
    (four), for one tile, every tile shuffled and a tile repeated with another offset, every variant valid for the scene, host and device
    forms; the finished sums == rt1w_render_aov_device of each clipped rectangle; paths == segments == in-frame pixels x spp, grid =
    n_tiles (tile / 16)^2."""
    rng = np.random.default_rng(arm)
    dev = TF._DeviceBuffers()
    try:
        for W, H, tiles_of in ((W_GPU, H_GPU, (16, 32)), (10, 7, (16,))):
            sc = _scene(arm, W, H)
            ctx = gpu_ctx_factory(sc)
            variants = [None] + ([v for v in _valid_variants(sc.info())] if (W, H) == (W_GPU, H_GPU) else [])
            d_rect = dev.alloc(32 * 32 * 64)

            @functools.lru_cache(maxsize=None)
            def rect(r, off):
                ctx.render_aov_device(d_rect, W, H, 3, tile=r, sample_offset=off, global_seed=2)
                return dev.fetch(d_rect, (r[3], r[2], 8))
            for tile in tiles_of:
                for tiles in _lists(W, H, tile, rng):
                    inside = sum(min(tile, W - x) * min(tile, H - y) for x, y, _ in tiles)
                    want = rt.aov_tiles_host(sc, W, H, 3, tile, tiles, sample_offset=1, global_seed=2)
                    d_out = dev.alloc(want.nbytes)
                    for v in variants if len(tiles) > 1 else [None]:
                        got, st = ctx.render_aov_tiles(W, H, 3, tile, tiles, sample_offset=1, global_seed=2, variant=v, with_stats=True)
                        assert _same(got, want if v is None else rt.aov_tiles_host(sc, W, H, 3, tile, tiles, sample_offset=1, global_seed=2, variant=v)), (W, tile, v)
                        assert st["paths"] == st["segments"] == inside * 3 and st["grid"] == len(tiles) * (tile // 16) ** 2 and st["block"] == 256
                        assert st["passes"] == 1 and st["kernel_ms"] > 0 and st["variant"] == (sc.info()["variant"] if v is None else v)
                        sd = ctx.render_aov_tiles_device(d_out, W, H, 3, tile, tiles, sample_offset=1, global_seed=2, variant=v)
                        assert _same(dev.fetch(d_out, want.shape), got) and sd["paths"] == st["paths"] and sd["grid"] == st["grid"]
                    _check_tile_sums(want, W, H, 3, tile, tiles, lambda r, off: rect(r, off + 1))
    finally:
        dev.free()


def _valid_variants(info):
    media, tex, ms, sd = info["has_media"], info["has_textures"], info["has_moving"], info["scope_depth"]
    v = [1, 3, 4]
    if not media and not tex and not ms and sd <= 2:
        v.append(0)
    if not media:
        v.append(2)
    if not media and sd == 0:
        v.append(5)
    return sorted(v)


@pytest.mark.gpu
def test_gpu_merge_and_resolve_equal_twins(rt, gpu_ctx_factory):
    """rt1w_guides_merge_tiles and rt1w_guides_resolve == their twins bit for bit, host and device forms: rendered sums at 72 x 40 with tile
    16 and 32 (two merges, the second of a part of the frame), and the hostile synthetic accumulator at 37 x 21."""
    W, H = W_GPU, H_GPU
    sc = _scene(5, W, H)
    ctx = gpu_ctx_factory(sc)
    dev = TF._DeviceBuffers()
    try:
        for tile in (16, 32):
            every = _all_tiles(W, H, tile)
            part = [(x, y, 3) for x, y, _ in every[1::2]]
            s1, s2 = ctx.render_aov_tiles(W, H, 3, tile, every), ctx.render_aov_tiles(W, H, 2, tile, part)
            g1, st = ctx.guides_merge_tiles(np.zeros((H, W, 9)), s1, 3, tile, every, with_stats=True)
            assert _same(g1, rt.guides_merge_tiles_host(np.zeros((H, W, 9)), s1, 3, tile, every))
            assert st["grid"] == len(every) * (tile // 16) ** 2 and st["block"] == 256 and st["paths"] == W * H
            g2 = ctx.guides_merge_tiles(g1, s2, 2, tile, part)
            assert _same(g2, rt.guides_merge_tiles_host(g1, s2, 2, tile, part)) and g2[..., 8].max() == 5.0 and g2[..., 8].min() == 3.0
            a1, sr = ctx.guides_resolve(g1, with_stats=True)
            assert _same(a1, rt.guides_resolve_host(g1)) and _same(a1, ctx.render_aov(W, H, 3))  # one merge: the entry's bits
            assert sr["grid"] == ((W + 15) // 16) * ((H + 15) // 16) and sr["block"] == 256
            assert _same(ctx.guides_resolve(g2), rt.guides_resolve_host(g2))
            d_g, d_s, d_a = dev.put(g1), dev.put(s2), dev.alloc(W * H * 64)
            ctx.guides_merge_tiles_device(d_g, d_s, W, H, tile, part, 2)
            ctx.guides_resolve_device(d_g, d_a, W, H)
            assert _same(dev.fetch(d_g, g2.shape), g2) and _same(dev.fetch(d_a, (H, W, 8)), rt.guides_resolve_host(g2))
        g, s, tiles = _hostile_gacc(np.random.default_rng(19))
        m1 = ctx.guides_merge_tiles(g, s, 4, 16, tiles)
        assert _same(m1, rt.guides_merge_tiles_host(g, s, 4, 16, tiles))
        for acc in (np.zeros_like(g), g, m1):
            assert _same(ctx.guides_resolve(acc), rt.guides_resolve_host(acc))
    finally:
        dev.free()


GPU_AD = dict(batch_spp=2, pilot_batches=2, budget_spp=8, max_spp=16)


def _compose_device(rt, ctx, sc, W, H, ad, dev, global_seed=0):
    """the plan over the public DEVICE entries: (out, spp, err_px, rounds, render launches, paths)"""
    tile, n, P = ad["tile"], ad["batch_spp"], ad["pilot_batches"]
    npix = W * H
    chunk = sc.default_chunk(W, H, n)
    tx_n, ty_n = TF._tiles(W, H, tile)
    nt = tx_n * ty_n
    d_aov, d_guides, d_sums = dev.alloc(npix * 64), dev.alloc(npix * 64), dev.alloc(max(npix, 2 * nt * tile * tile) * 24)
    d_asums, d_gacc = dev.alloc(nt * tile * tile * 64), dev.alloc(npix * 72, zero=True)
    d_acc = [dev.alloc(npix * 64, zero=True), dev.alloc(npix * 64, zero=True)]
    d_err, d_frame, d_var, d_spp, d_epx = dev.alloc(nt * 8), dev.alloc(npix * 24), dev.alloc(npix * 8), dev.alloc(npix * 8), dev.alloc(npix * 8)
    d_ha, d_hb = dev.alloc(npix * 24), dev.alloc(npix * 24)
    every = _all_tiles(W, H, tile)
    ctx.render_aov_tiles_device(d_asums, W, H, P * n, tile, every, global_seed=global_seed)
    ctx.guides_merge_tiles_device(d_gacc, d_asums, W, H, tile, every, P * n)
    ctx.guides_resolve_device(d_gacc, d_aov, W, H)
    stat = dict(paths=0, launches=0)
    for b in range(P):
        st = ctx.render_device(d_sums, W, H, n, sample_offset=b * n, global_seed=global_seed, chunk=chunk, out_sum=True)
        stat["paths"] += st["paths"]
        ctx.accum_merge_device(d_acc[b & 1], d_sums, d_aov, W, H, (0, 0, W, H), n)
        stat["launches"] += 1
    m = np.full((ty_n, tx_n), P // 2, dtype=np.uint32)
    rounds = 0
    while True:
        ctx.halves_resolve_device(d_acc[0], d_acc[1], d_frame, d_var, d_ha, d_hb, d_spp, W, H, n)
        ctx.guides_resolve_device(d_gacc, d_guides, W, H)
        ctx.denoise_var_halves_device(d_frame, d_guides, d_var, d_ha, d_hb, d_frame, d_epx, W, H)
        ctx.tile_error_map_device(d_epx, d_err, W, H, tile)
        taken = rt.adaptive_select(W, H, dev.fetch(d_err, (ty_n, tx_n)), m, **TF._pair_params(ad))
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
        ctx.render_aov_tiles_device(d_asums, W, H, 2 * n, tile, tiles[:k], global_seed=global_seed)
        ctx.guides_merge_tiles_device(d_gacc, d_asums, W, H, tile, tiles[:k], 2 * n)
        for t in taken:
            m.flat[t] += 1
    assert np.array_equal(dev.fetch(d_gacc, (H, W, 9))[..., 8], dev.fetch(d_spp, (H, W)))
    return dev.fetch(d_frame, (H, W, 3)), dev.fetch(d_spp, (H, W)), dev.fetch(d_epx, (H, W)), rounds, stat["launches"], stat["paths"]


@pytest.mark.gpu
@pytest.mark.parametrize("tile", [16, 32])
@pytest.mark.parametrize("arm", [5, 7])
def test_gpu_one_call_equals_composition(rt, gpu_ctx_factory, arm, tile):
    """rt1w_render_adaptive_guided == the plan composed in Python over the public device entries, bit for bit, 48 x 40: out_rgb, out_spp and
    out_err; stats.passes = the pilot's launches + the rounds (trace kernels only), n_chunks = the rounds, paths = the samples spent; with
    a budget equal to the pilot the three outputs are the bits of rt1w_render_adaptive_filtered."""
    W, H = 48, 40
    ad = dict(tile=tile, **GPU_AD)
    sc = _scene(arm, W, H)
    ctx = gpu_ctx_factory(sc)
    dev = TF._DeviceBuffers()
    try:
        out, spp, err_px, rounds, launches, paths = _compose_device(rt, ctx, sc, W, H, ad, dev, global_seed=3)
        one, ospp, oerr, st = ctx.render_adaptive_guided(W, H, adaptive=ad, global_seed=3, with_stats=True)
        assert _same(one, out) and _same(ospp, spp) and _same(oerr, err_px), (arm, tile)
        assert st["paths"] == paths == int(spp.sum()) and st["n_chunks"] == rounds and rounds >= 1 and st["passes"] == launches == 2 + rounds
        assert st["block"] == 256 and st["grid"] == ((W + 15) // 16) * ((H + 15) // 16) and st["kernel_ms"] > 0 and st["total_ms"] > 0
        assert spp.max() > spp.min() and np.all(np.isfinite(oerr)) and oerr.max() > 0.0
        flat = dict(ad, pilot_batches=4, budget_spp=8)                              # two pairs: the least the pair plan accepts
        g, f = ctx.render_adaptive_guided(W, H, adaptive=flat, global_seed=3, with_stats=True), ctx.render_adaptive_filtered(W, H, adaptive=flat, global_seed=3, with_stats=True)
        assert all(_same(x, y) for x, y in zip(g[:3], f[:3])) and g[3]["n_chunks"] == 0 and g[3]["passes"] == f[3]["passes"] == 4
    finally:
        dev.free()
    if tile != 16:
        return
    for bad in (dict(adaptive=dict(ad, pilot_batches=3, budget_spp=16)), dict(adaptive=dict(ad, tile=24)), dict(adaptive=ad, sigma_variance=-1.0),
                dict(adaptive=ad, tile=(0, 0, W, 30)), dict(adaptive=ad, sample_offset=2 ** 32 - 10), dict(adaptive=ad, flags=rt.UNSORTED),
                dict(adaptive=ad, precision=1)):
        with pytest.raises(rt.Rt1wError) as e:
            ctx.render_adaptive_guided(W, H, **bad)
        assert e.value.code == rt.ERR_INVALID, bad


@pytest.mark.gpu
def test_gpu_nothing_else_moves(rt, gpu_ctx_factory):
    """The new entries share the context's framebuffer, batch, accumulator, filter and tile-list buffers with the others: rt1w_render_aov,
    rt1w_render_adaptive_filtered and rt1w_render_tiles after a guided call return the bits they returned before it."""
    sc = rt.Scene.reference(5, build_seed=1)
    ctx = gpu_ctx_factory(sc)
    ad = dict(tile=16, **GPU_AD)
    tiles = [(16, 0, 2), (0, 16, 0), (64, 48, 5)]
    a0 = ctx.render_aov(72, 56, 4)
    q0 = ctx.render_adaptive_filtered(72, 56, adaptive=ad)
    t0, s0 = ctx.render_tiles(72, 56, 2, 16, tiles, out_sum=True)
    ctx.render_adaptive_guided(72, 56, adaptive=ad)
    ctx.render_adaptive_guided(150, 100, adaptive=dict(ad, tile=32))                     # larger than anything so far: every buffer grows
    assert _same(a0, ctx.render_aov(72, 56, 4))
    assert all(_same(x, y) for x, y in zip(q0, ctx.render_adaptive_filtered(72, 56, adaptive=ad)))
    t1, s1 = ctx.render_tiles(72, 56, 2, 16, tiles, out_sum=True)
    assert _same(t0, t1) and s0["segments"] == s1["segments"]


if __name__ == "__main__" and "--record" in sys.argv:
    sys.path.insert(0, ROOT)
    with open(REFUSALS, "w") as f:
        json.dump(_refusals(orc.rt()), f, indent=1)
        f.write("\n")
