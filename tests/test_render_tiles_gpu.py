"""A list of tiles in one launch, GPU tier (include/rt1w.h: rt1w_render_tiles, rt1w_accum_merge_tiles, RT1W_ADAPTIVE_ONE_LAUNCH): the tile-list
form of every f64 render kernel the plan reaches against rt1w_render_device of each tile's rectangle, bit for bit; the list merge against
its CPU twin and the rectangle merges; the plan with one launch per round against the plan without."""
import ctypes as C

import numpy as np
import pytest

import orc
from dual import random_scene_pair

W, H, T = 72, 40, 16          # a 5 x 3 grid of tiles: the right column is 8 pixels wide, the top row 8 high
SPP = 3
LAST = 2 ** 32 - 1 - SPP      # the largest sample offset a tile of SPP samples can have
# out of order: the corner, a right-edge tile, a top-edge tile, interior tiles; offsets 0, 3, 6 .. and the largest
LIST = [(64, 32, 0), (16, 16, 3), (64, 0, 6), (0, 32, LAST), (48, 16, 9), (0, 0, 12), (32, 32, 15)]
AD = dict(batch_spp=2, pilot_batches=2, budget_spp=8, max_spp=16)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _clip(x0, y0, w=W, h=H, t=T):
    return min(t, w - x0), min(t, h - y0)


class _Device:
    """plain device memory of the HIP runtime this process already uses"""

    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")
        self.made = []

    def alloc(self, nbytes):
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), C.c_size_t(nbytes)) == 0
        self.made.append(p)
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


@pytest.fixture
def dev():
    d = _Device()
    yield d
    d.free()


def _scene(rt, case):
    kind, arg, near_far = case
    sc = rt.Scene.reference(arg, build_seed=1, aspect_ratio=W / H) if kind == "arm" else random_scene_pair(arg)[0]
    if near_far:
        sc.set_walk_order(True)
    return sc


# (what, arm or seed, RT1W_WALK_NEAR_FAR) -> the stats.sorted bits of the kernel that must run (1 reordering kernel, 128 pair walk,
# 256 sphere-media build, 512 finished paths reordered, 1024 node cache) and its variant
CASES = {
    "arm0": (("arm", 0, False), 128 | 512, 5),
    "arm2": (("arm", 2, False), 1, 1),
    "arm5": (("arm", 5, False), 1, 0),
    "arm6": (("arm", 6, False), 1, 1),
    "arm7": (("arm", 7, False), 256 | 512 | 1024, 3),
    "arm7_near_far": (("arm", 7, True), 256 | 512 | 1024, 4),
    "graph_v2": (("graph", 2009, False), 512 | 1024, 2),
    "graph_v3": (("graph", 2003, False), 512 | 1024, 3),
    "graph_v4_plain": (("graph", 2003, True), 0, 4),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_gpu_tiles_equal_their_rectangles(rt, gpu_ctx_factory, dev, name):
    """Seven tiles in one launch == rt1w_render_device of each tile's clipped rectangle with RT1W_OUT_SUM, the tile's absolute sample offset
    and the same chunk, bit for bit; pixels beyond the frame are +0.0; segments add up; stats.sorted is the generic rectangle render's.
    spp 3 with chunk 2 (a short last chunk) and chunk 0 (the whole frame's default).
    Rows of the dispatch table (csrc/context.hip: render_plan with flags 0, no scene-specialised kernel) reached: arm0 the pair walk that
    reorders the finished paths (V5); arm2 and arm6 the reordering kernel V1 (textures; media); arm5 the reordering kernel V0; arm7 the
    sphere-media stack walk with the node cache, V3, and under RT1W_WALK_NEAR_FAR V4; graph_v2 / graph_v3 (random graphs of
    tests/test_random_scenes.py's maker) the stack walk with the node cache for V2 and for V3 with general media boundaries;
    graph_v4_plain the plain kernel V4 falls back to.  Not reached: the stack walks without the node cache (a context whose walk table
    could not be built), the V5 stack walks and the pair walk without reordering (sphere scenes outside the pair walk's scope)."""
    case, bits, variant = CASES[name]
    sc = _scene(rt, case)
    ctx = gpu_ctx_factory(sc)
    d_rect = dev.alloc(T * T * 3 * 8)
    for chunk in (2, 0):
        tiles, st = ctx.render_tiles(W, H, SPP, T, LIST, out_sum=True, chunk=chunk)
        explicit = chunk or sc.default_chunk(W, H, SPP)
        assert st["sorted"] == bits and st["variant"] == variant, (name, st)
        assert st["chunk"] == min(explicit, SPP) and st["passes"] == 1 and st["paths"] == SPP * sum(tw * th for tw, th in (_clip(x, y) for x, y, _ in LIST))
        segments = 0
        for k, (x0, y0, off) in enumerate(LIST):
            tw, th = _clip(x0, y0)
            sr = ctx.render_device(d_rect, W, H, SPP, tile=(x0, y0, tw, th), sample_offset=off, out_sum=True, chunk=explicit, generic=True)
            rect = dev.fetch(d_rect, (th, tw, 3))
            assert _same(tiles[k, :th, :tw], rect), (name, chunk, k)
            assert sr["sorted"] == st["sorted"] and sr["variant"] == st["variant"]
            segments += sr["segments"]
            beyond = np.ones((T, T), dtype=bool)
            beyond[:th, :tw] = False
            assert np.all(tiles[k][beyond].view(np.uint64) == 0), (name, chunk, k)       # exactly +0.0
        assert st["segments"] == segments, (name, chunk)
    if name == "arm5":
        # the scene-specialised kernel renders the same bits: the contract holds against the default render too
        x0, y0, off = LIST[1]
        assert _same(tiles[1], ctx.render(W, H, SPP, tile=(x0, y0, T, T), sample_offset=off, out_sum=True, chunk=sc.default_chunk(W, H, SPP))[0])


@pytest.mark.gpu
def test_gpu_bit_neutrality_and_passes(rt, gpu_ctx_factory, dev):
    """All 15 tiles of the frame == the whole-frame RT1W_OUT_SUM render; the order of the list and repeats do not matter; n_tiles = 1; the
    means form == rt1w_resolve of the sums; a render in two sample passes == the same render in one; the device form == the host form."""
    sc = rt.Scene.reference(5, build_seed=1, aspect_ratio=W / H)
    ctx = gpu_ctx_factory(sc)
    every = [(x0, y0, 0) for y0 in range(0, H, T) for x0 in range(0, W, T)]
    whole = ctx.render(W, H, 5, out_sum=True, global_seed=9)[0]
    tiles, st = ctx.render_tiles(W, H, 5, T, every, out_sum=True, global_seed=9)
    assert st["paths"] == 5 * W * H
    for k, (x0, y0, _) in enumerate(every):
        tw, th = _clip(x0, y0)
        assert _same(tiles[k, :th, :tw], np.ascontiguousarray(whole[y0:y0 + th, x0:x0 + tw])), k
    back = ctx.render_tiles(W, H, 5, T, every[::-1] + every[3:5], out_sum=True, global_seed=9)[0]
    assert _same(back[:15], np.ascontiguousarray(tiles[::-1])) and _same(back[15:], np.ascontiguousarray(tiles[3:5]))
    one, s1 = ctx.render_tiles(W, H, 5, T, every[7:8], out_sum=True, global_seed=9)
    assert _same(one[0], tiles[7]) and s1["paths"] == 5 * T * T
    means = ctx.render_tiles(W, H, 5, T, every, global_seed=9)[0]
    assert _same(means, rt.resolve(tiles, 5))
    assert _same(ctx.render_tiles(W, H, 5, T, every, generic=True, global_seed=9)[0], means)         # RT1W_GENERIC is a no-op
    # sample_offset of the call is added to every tile's own
    moved = ctx.render_tiles(W, H, SPP, T, [(x, y, o % 100) for x, y, o in LIST], out_sum=True, sample_offset=7)[0]
    assert _same(moved, ctx.render_tiles(W, H, SPP, T, [(x, y, o % 100 + 7) for x, y, o in LIST], out_sum=True)[0])
    # 30 chunks of 7 x 256 pixels x 24 bytes = 42 KiB each: 24 fit one MiB, so two passes
    long1, sa = ctx.render_tiles(W, H, 60, T, [(x, y, o % 100) for x, y, o in LIST], out_sum=True, chunk=2)
    long2, sb = ctx.render_tiles(W, H, 60, T, [(x, y, o % 100) for x, y, o in LIST], out_sum=True, chunk=2, partial_mib=1)
    assert sa["passes"] == 1 and sb["passes"] == 2 and sa["n_chunks"] == sb["n_chunks"] == 30
    assert _same(long1, long2) and sa["segments"] == sb["segments"]
    d_out = dev.alloc(len(LIST) * T * T * 3 * 8)
    sd = ctx.render_tiles_device(d_out, W, H, 60, T, [(x, y, o % 100) for x, y, o in LIST], out_sum=True, chunk=2, partial_mib=1)
    assert _same(dev.fetch(d_out, long2.shape), long2) and sd["passes"] == 2 and sd["segments"] == sb["segments"]


@pytest.mark.gpu
def test_gpu_merge_and_refusals(rt, gpu_ctx_factory, dev):
    """rt1w_accum_merge_tiles and its device form == the CPU twin == the sequence of rt1w_accum_merge_device calls on the clipped rectangles;
    what the two new entries refuse."""
    sc = rt.Scene.reference(5, build_seed=1, aspect_ratio=W / H)
    ctx = gpu_ctx_factory(sc)
    aov = ctx.render_aov(W, H, 4)
    n = 2
    tiles = [(x, y, 0) for x, y, _ in LIST]
    batches = [ctx.render_tiles(W, H, n, T, [(x, y, b * n) for x, y, _ in LIST], out_sum=True)[0] for b in range(3)]
    batches[1][1, 5, 9, 1] = np.nan
    d_aov, d_acc_l, d_acc_r = dev.put(aov), dev.put(np.zeros((H, W, 8))), dev.put(np.zeros((H, W, 8)))
    g = t = np.zeros((H, W, 8))
    for keep in (False, True):
        for b in range(3):
            g, st = ctx.accum_merge_tiles(g, batches[b], aov, n, T, tiles, keep_albedo=keep, with_stats=True)
            t = rt.accum_merge_tiles_host(t, batches[b], aov, n, T, tiles, keep_albedo=keep)
            assert _same(g, t), (keep, b)
            assert st["grid"] == len(tiles) * (T // 16) ** 2 and st["block"] == 256 and st["passes"] == 1
            assert st["paths"] == sum(tw * th for tw, th in (_clip(x, y) for x, y, _ in tiles))
            sd = ctx.accum_merge_tiles_device(d_acc_l, dev.put(batches[b]), d_aov, W, H, T, tiles, n, keep_albedo=keep)
            assert sd["grid"] == st["grid"]
            for k in reversed(range(len(tiles))):
                (x0, y0, _), (tw, th) = tiles[k], _clip(*tiles[k][:2])
                ctx.accum_merge_device(d_acc_r, dev.put(batches[b][k, :th, :tw]), d_aov, W, H, (x0, y0, tw, th), n, keep_albedo=keep)
            assert _same(dev.fetch(d_acc_l, (H, W, 8)), g) and _same(dev.fetch(d_acc_r, (H, W, 8)), g), (keep, b)
    assert g[21, 25, 5] == rt.ACCUM_NO_ESTIMATE
    big = ctx.accum_merge_tiles(np.zeros((96, 100, 8)), np.ones((2, 48, 48, 3)), np.ones((96, 100, 8)), n, 48, [(96, 48), (0, 0)], with_stats=True)
    assert big[1]["grid"] == 2 * 9 and _same(big[0], rt.accum_merge_tiles_host(np.zeros((96, 100, 8)), np.ones((2, 48, 48, 3)), np.ones((96, 100, 8)), n, 48, [(96, 48), (0, 0)]))

    def refused(code, fn, *a, **kw):
        with pytest.raises(rt.Rt1wError) as e:
            fn(*a, **kw)
        assert e.value.code == code, (a, kw)

    zero, s1 = np.zeros((H, W, 8)), np.zeros((1, T, T, 3))
    for bad in ([(0, 0), (0, 0)], [(8, 0)], [(0, 24)], [(80, 0)], [(0, 48)], [(0, 0, 0, 1)], []):
        refused(rt.ERR_INVALID, ctx.accum_merge_tiles, zero, np.zeros((len(bad), T, T, 3)), aov, n, T, bad)
    for tile in (8, 24, 272):
        refused(rt.ERR_INVALID, ctx.accum_merge_tiles, zero, np.zeros((1, tile, tile, 3)), aov, n, tile, [(0, 0)])
    refused(rt.ERR_INVALID, ctx.accum_merge_tiles, zero, s1, aov, 0, T, [(0, 0)])
    for bad in ([(8, 0)], [(0, 24)], [(80, 0)], [(0, 48)], [(0, 0, 0, 1)], [], [(0, 0, 2 ** 32 - SPP)]):
        refused(rt.ERR_INVALID, ctx.render_tiles, W, H, SPP, T, bad)
    for tile in (8, 24, 272):
        refused(rt.ERR_INVALID, ctx.render_tiles, W, H, SPP, tile, [(0, 0)])
    refused(rt.ERR_INVALID, ctx.render_tiles, W, H, SPP, T, [(0, 0, LAST)], sample_offset=1)
    refused(rt.ERR_INVALID, ctx.render_tiles, W, H, 0, T, [(0, 0)])
    for flags in (rt.UNSORTED, rt.OUT_FRAME, rt.RNG_REFERENCE, rt.PROBE_COHERENT, rt.WAVEFRONT, rt.LDS_NODES, rt.CLASSIC_WALK, rt.NO_NODE_CACHE, 1 << 8):
        refused(rt.ERR_INVALID, ctx.render_tiles, W, H, SPP, T, [(0, 0)], flags=flags)
    refused(rt.ERR_INVALID, ctx.render_tiles, W, H, SPP, T, [(0, 0)], strips=(8, 16))
    refused(rt.ERR_UNSUPPORTED, ctx.render_tiles, W, H, SPP, T, [(0, 0)], f32=True)
    assert ctx.render_tiles(W, H, SPP, T, [(0, 0), (0, 0, 3)], out_sum=True)[1]["paths"] == 2 * SPP * T * T   # a repeat with another offset is a render's right


@pytest.mark.gpu
@pytest.mark.parametrize("arm,w,h,tile", [(5, 96, 96, 16), (7, 90, 70, 32)])
def test_gpu_plan_with_one_launch_per_round(rt, gpu_ctx_factory, arm, w, h, tile):
    """rt1w_render_adaptive with RT1W_ADAPTIVE_ONE_LAUNCH == the call without it: frame and spp map bit for bit, paths, segments and rounds
    equal, unfiltered and filtered; passes = the pilot's launches + one per round; a plain render before and after is unchanged."""
    sc = rt.Scene.reference(arm, build_seed=1, aspect_ratio=w / h)
    ctx = gpu_ctx_factory(sc)
    f0, s0 = ctx.render(w, h, 8)
    ad = dict(tile=tile, **AD)
    for filtered in (False, True):
        a, aspp, sa = ctx.render_adaptive(w, h, adaptive=ad, filter=filtered, global_seed=3, with_stats=True)
        b, bspp, sb = ctx.render_adaptive(w, h, adaptive=dict(ad, one_launch=True), filter=filtered, global_seed=3, with_stats=True)
        assert _same(a, b) and _same(aspp, bspp), (arm, filtered)
        assert sa["paths"] == sb["paths"] == int(bspp.sum()) and sa["segments"] == sb["segments"] and sa["n_chunks"] == sb["n_chunks"] >= 1
        assert sb["passes"] == AD["pilot_batches"] + sb["n_chunks"] and sa["passes"] >= sb["passes"]
        assert bspp.max() > bspp.min()
    f1, s1 = ctx.render(w, h, 8)
    assert _same(f0, f1) and s0["segments"] == s1["segments"]
    with pytest.raises(rt.Rt1wError) as e:
        ctx.render_adaptive(w, h, adaptive=dict(ad, one_launch=True), flags=rt.UNSORTED)
    assert e.value.code == rt.ERR_INVALID
    with pytest.raises(rt.Rt1wError) as e:
        ctx.render_adaptive(w, h, adaptive=dict(ad, flags=2))
    assert e.value.code == rt.ERR_INVALID
