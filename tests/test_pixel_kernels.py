"""The one work mapping of the per-pixel kernel units (csrc/rt_pixel_kernels.h: a lane's pixel with the workgroups in row order over a
width, the tile-list decode, the grids, the launch tail) and aov.hip's own mapping (aov_lane_pixel), under every kernel that takes its
mapping from there: the device entries against their CPU twins, bit for bit, at the shapes where a mapping goes wrong.  Synthetic inputs
except for the AOV kernels, which need a scene.  Every buffer an entry writes lies between two guard bands that must come back intact.
(The a-trous filters, the header's other users, have tests/test_atrous_skeleton.py.)"""
import numpy as np
import pytest

import test_adaptive_filtered as TF
import test_atrous_skeleton as TA

_same = TF._same

GUARD = 256  # doubles in front of and behind every buffer written
PATTERN = np.uint64(0x7FF4C0DEC0DE5A5A)  # a NaN no kernel computes

# a single lane; exactly one workgroup's block; one pixel over and under the block's edge; several blocks each way; the two degenerate strips
FRAMES = [(1, 1), (16, 16), (17, 15), (37, 21), (1, 300), (300, 1)]
# (x0, y0, tw, th) in a 37 x 21 frame: the whole frame, an interior rectangle that starts and ends off the block grid, the last pixel
RECTS = [(0, 0, 37, 21), (5, 3, 19, 10), (36, 20, 1, 1)]
LIST_FRAME = (40, 24)
# (tile, [(x0, y0, sample_offset)]) in a 40 x 24 frame: all six 16-tiles in reverse order (the right column clipped to 8 columns, the top row
# to 8 rows); two 32-tiles, both clipped by the frame, (2 x 2 workgroups each), the second first; a list of one
LISTS = [(16, [(32, 16, 0), (16, 16, 3), (0, 16, 0), (32, 0, 1), (16, 0, 0), (0, 0, 2)]),
         (32, [(32, 0, 1), (0, 0, 0)]),
         (16, [(16, 0, 5)])]
# (x0, y0, tw, th) of a 40 x 24 frame for the AOV kernels: one lane; one 8 x 8 block and a bit; 5 x 3 blocks, the last workgroup half empty
AOV_TILES = [(7, 5, 1, 1), (3, 2, 9, 7), (5, 4, 33, 17)]
AOV_SPP = 2
# what the parent commit's library reported for these calls (arm 5, 2 spp, the tiles and lists above, in their order), recorded once on the
# GPU: paths, segments, chunk, n_chunks, variant, passes
AOV_STATS = [(2, 2, 2, 1, 0, 1), (126, 126, 2, 1, 0, 1), (1122, 1122, 2, 1, 0, 1)]
AOV_DEEP_STATS = [(2, 2, 2, 1, 0, 1), (126, 137, 2, 1, 0, 1), (1122, 1457, 2, 1, 0, 1)]
AOV_TILES_STATS = [(1920, 1920, 2, 1, 0, 1), (1920, 1920, 2, 1, 0, 1), (512, 512, 2, 1, 0, 1)]
STATS_KEYS = ("paths", "segments", "chunk", "n_chunks", "variant", "passes")


class _Guarded:
    """device buffers between guard bands: out(shape[, init]) -> address; check(address) -> the array, the bands verified"""

    def __init__(self, dev):
        self.dev, self.made = dev, {}

    def out(self, shape, init=None):
        n = int(np.prod(shape))
        host = np.full(n + 2 * GUARD, PATTERN, dtype=np.uint64)
        if init is not None:
            host[GUARD:GUARD + n] = np.ascontiguousarray(init, dtype=np.float64).reshape(-1).view(np.uint64)
        base = self.dev.put(host.view(np.float64))
        self.made[base + 8 * GUARD] = (base, tuple(shape), n)
        return base + 8 * GUARD

    def check(self, p):
        base, shape, n = self.made[p]
        got = self.dev.fetch(base, (n + 2 * GUARD,)).view(np.uint64)
        assert np.all(got[:GUARD] == PATTERN) and np.all(got[GUARD + n:] == PATTERN), "a guard band was written"
        return got[GUARD:GUARD + n].view(np.float64).reshape(shape)


def _ceil(a, b):
    return (a + b - 1) // b


def _frame_stats(st, w, h):
    assert st["block"] == 256 and st["grid"] == _ceil(w, 16) * _ceil(h, 16), (st, w, h)


def _accumulator(rt, w, h, rng, batches=3, n=2):
    """an accumulator of `batches` merged synthetic batches (the twin's), and the feature buffers that demodulated them"""
    aov = TF._guides(h, w, rng)
    acc = np.zeros((h, w, 8))
    for _ in range(batches):
        acc = rt.accum_merge_host(acc, rng.uniform(0.0, 2.0 * n, (h, w, 3)), aov, n)
    return acc, aov


def _guide_accumulator(rt, w, h, rng, spp=2):
    """a guide accumulator holding `spp` samples in every pixel (the twin's merge of every 16-tile of the frame)"""
    tiles = [(x, y, 0) for y in range(0, h, 16) for x in range(0, w, 16)]
    sums = rng.uniform(0.0, spp, (len(tiles), 16, 16, 8))
    return rt.guides_merge_tiles_host(np.zeros((h, w, 9)), sums, spp, 16, tiles)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", FRAMES)
def test_gpu_frame_kernels_equal_twins(rt, gpu_ctx_factory, w, h):
    """accum_resolve, halves_resolve, guides_resolve, batch_variance (2 batches) and temporal_accumulate: workgroups in row order over the
    frame; accum_tile_error and tile_error_map at tile 16 and 32: one workgroup per tile, its own loop over the lane's position"""
    ctx = gpu_ctx_factory(rt.Scene.reference(5, build_seed=1))
    rng = np.random.default_rng(1000 * w + h)
    dev = TF._DeviceBuffers()
    g = _Guarded(dev)
    try:
        n = 2
        acc_a, aov = _accumulator(rt, w, h, rng)
        acc_b, _ = _accumulator(rt, w, h, rng)
        d_a, d_b, d_aov = dev.put(acc_a), dev.put(acc_b), dev.put(aov)

        outs = [g.out(s) for s in ((h, w, 3), (h, w), (h, w))]
        _frame_stats(ctx.accum_resolve_device(d_a, *outs, w, h, n), w, h)
        for p, t in zip(outs, rt.accum_resolve_host(acc_a, n)):
            assert _same(g.check(p), t), ("accum_resolve", w, h)

        outs = [g.out(s) for s in ((h, w, 3), (h, w), (h, w, 3), (h, w, 3), (h, w))]
        _frame_stats(ctx.halves_resolve_device(d_a, d_b, *outs, w, h, n), w, h)
        for p, t in zip(outs, rt.halves_resolve_host(acc_a, acc_b, n)):
            assert _same(g.check(p), t), ("halves_resolve", w, h)

        gacc = _guide_accumulator(rt, w, h, rng)
        out = g.out((h, w, 8))
        _frame_stats(ctx.guides_resolve_device(dev.put(gacc), out, w, h), w, h)
        assert _same(g.check(out), rt.guides_resolve_host(gacc)), ("guides_resolve", w, h)

        sums = rng.uniform(0.0, 2.0 * n, (2, h, w, 3))
        outs = [g.out((h, w, 3)), g.out((h, w))]
        _frame_stats(ctx.batch_variance_device(dev.put(sums), d_aov, *outs, w, h, 2, n), w, h)
        for p, t in zip(outs, rt.batch_variance_host(sums, aov, n)):
            assert _same(g.check(p), t), ("batch_variance", w, h)

        # the same camera for both frames: every pixel reprojects onto itself, so the gathers run; a quarter of the pixels fail the depth test
        cam = ctx.get_camera().array()
        buf = TA._inputs(w, h, 7 * w + h)
        prev_aov = buf["aov"].copy()
        prev_aov[rng.uniform(size=(h, w)) < 0.25, 6] += 4.0
        prev_hist, prev_len = rng.uniform(0.0, 2.0, (h, w, 3)), np.floor(rng.uniform(0.0, 6.0, (h, w)))
        outs = [g.out((h, w, 3)), g.out((h, w)), g.out((h, w, 3))]
        st = ctx.temporal_accumulate_device(dev.put(buf["frame"]), dev.put(buf["aov"]), cam, dev.put(prev_hist), dev.put(prev_len), dev.put(prev_aov), cam,
                                            *outs, w, h)
        _frame_stats(st, w, h)
        expect = rt.temporal_host(buf["frame"], buf["aov"], cam, prev_hist, prev_len, prev_aov, cam)
        if w * h > 1:
            assert np.any(expect[1] > 1.0), "no pixel found its history: the gathers did not run"
        for p, t in zip(outs, expect):
            assert _same(g.check(p), t), ("temporal_accumulate", w, h)

        err_px = rng.uniform(0.0, 1.0, (h, w))
        d_err_px = dev.put(err_px)
        for tile in (16, 32):
            tx, ty = _ceil(w, tile), _ceil(h, tile)
            out = g.out((ty, tx))
            st = ctx.accum_tile_error_device(d_a, out, w, h, tile)
            assert st["block"] == 256 and st["grid"] == tx * ty, (st, w, h, tile)
            assert _same(g.check(out), rt.tile_error_host(acc_a, tile)), ("accum_tile_error", w, h, tile)
            out = g.out((ty, tx))
            st = ctx.tile_error_map_device(d_err_px, out, w, h, tile)
            assert st["block"] == 256 and st["grid"] == tx * ty, (st, w, h, tile)
            assert _same(g.check(out), rt.tile_error_map_host(err_px, tile)), ("tile_error_map", w, h, tile)
    finally:
        dev.free()


@pytest.mark.gpu
def test_gpu_rectangle_merge_equals_twin(rt, gpu_ctx_factory):
    """accum_merge: workgroups in row order over the rectangle's width, the pixel offset by the rectangle's corner"""
    ctx = gpu_ctx_factory(rt.Scene.reference(5, build_seed=1))
    w, h, n = 37, 21, 2
    rng = np.random.default_rng(3721)
    dev = TF._DeviceBuffers()
    g = _Guarded(dev)
    try:
        acc, aov = _accumulator(rt, w, h, rng)
        d_aov = dev.put(aov)
        for keep_albedo in (False, True):
            for x0, y0, tw, th in RECTS:
                sums = rng.uniform(0.0, 2.0 * n, (th, tw, 3))
                d_acc = g.out((h, w, 8), acc)
                st = ctx.accum_merge_device(d_acc, dev.put(sums), d_aov, w, h, (x0, y0, tw, th), n, keep_albedo=keep_albedo)
                _frame_stats(st, tw, th)
                assert _same(g.check(d_acc), rt.accum_merge_host(acc, sums, aov, n, x0=x0, y0=y0, keep_albedo=keep_albedo)), (x0, y0, tw, th, keep_albedo)
    finally:
        dev.free()


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(LISTS)))
def test_gpu_list_kernels_equal_twins(rt, gpu_ctx_factory, case):
    """accum_merge_tiles, guides_merge_tiles and render_aov_tiles (arm 5, 2 spp): (tile / 16)^2 workgroups per tile of the list, tile after
    tile.  The accumulators are compared whole -- the pixels no tile covers stay -- and so are the sums, whose pixels beyond the frame are +0.0"""
    sc = rt.Scene.reference(5, build_seed=1)
    ctx = gpu_ctx_factory(sc)
    w, h = LIST_FRAME
    tile, tiles = LISTS[case]
    grid = len(tiles) * (tile // 16) ** 2
    rng = np.random.default_rng(4024 + case)
    dev = TF._DeviceBuffers()
    g = _Guarded(dev)
    try:
        n = 2
        acc, aov = _accumulator(rt, w, h, rng)
        sums = rng.uniform(0.0, 2.0 * n, (len(tiles), tile, tile, 3))
        d_acc = g.out((h, w, 8), acc)
        st = ctx.accum_merge_tiles_device(d_acc, dev.put(sums), dev.put(aov), w, h, tile, tiles, n)
        assert st["block"] == 256 and st["grid"] == grid, st
        assert _same(g.check(d_acc), rt.accum_merge_tiles_host(acc, sums, aov, n, tile, tiles)), ("accum_merge_tiles", tile, tiles)

        gacc = _guide_accumulator(rt, w, h, rng)
        gsums = rng.uniform(0.0, float(n), (len(tiles), tile, tile, 8))
        d_gacc = g.out((h, w, 9), gacc)
        st = ctx.guides_merge_tiles_device(d_gacc, dev.put(gsums), w, h, tile, tiles, n)
        assert st["block"] == 256 and st["grid"] == grid, st
        assert _same(g.check(d_gacc), rt.guides_merge_tiles_host(gacc, gsums, n, tile, tiles)), ("guides_merge_tiles", tile, tiles)

        out = g.out((len(tiles), tile, tile, 8))
        st = ctx.render_aov_tiles_device(out, w, h, AOV_SPP, tile, tiles)
        assert st["block"] == 256 and st["grid"] == grid, st
        assert tuple(st[k] for k in STATS_KEYS) == AOV_TILES_STATS[case], st
        assert _same(g.check(out), rt.aov_tiles_host(sc, w, h, AOV_SPP, tile, tiles)), ("render_aov_tiles", tile, tiles)
    finally:
        dev.free()


@pytest.mark.gpu
@pytest.mark.parametrize("deep", [False, True])
def test_gpu_aov_kernels_equal_twins(rt, gpu_ctx_factory, deep):
    """render_aov_device and render_aov_deep_device (arm 5, 2 spp): 8 x 8 blocks numbered wave by wave over the tile, four to a workgroup"""
    sc = rt.Scene.reference(5, build_seed=1)
    ctx = gpu_ctx_factory(sc)
    w, h = LIST_FRAME
    dev = TF._DeviceBuffers()
    g = _Guarded(dev)
    try:
        for i, t in enumerate(AOV_TILES):
            out = g.out((t[3], t[2], 8))
            if deep:
                st = ctx.render_aov_deep_device(out, w, h, AOV_SPP, tile=t)
                expect, twin = rt.aov_host(sc, w, h, AOV_SPP, tile=t, max_specular=8, with_stats=True)
                assert st["segments"] == twin["segments"], (st, twin["segments"])
            else:
                st = ctx.render_aov_device(out, w, h, AOV_SPP, tile=t)
                expect = rt.aov_host(sc, w, h, AOV_SPP, tile=t)
            assert st["block"] == 256 and st["grid"] == _ceil(_ceil(t[2], 8) * _ceil(t[3], 8), 4), (st, t)
            assert tuple(st[k] for k in STATS_KEYS) == (AOV_DEEP_STATS if deep else AOV_STATS)[i], (st, t)
            assert _same(g.check(out), expect), (deep, t)
    finally:
        dev.free()
