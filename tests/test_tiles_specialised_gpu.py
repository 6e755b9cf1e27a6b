"""The tile-list form of the scene-specialised kernels, GPU tier (include/rt1w.h: RT1W_TILES_SPECIALISED, RT1W_SPECIALISE_TILES): a list of
tiles rendered with the flag against rt1w_render_device of each tile's rectangle on the specialised rectangle kernel and against the
same list without the flag, bit for bit; the item fetches of a long list; the fallback to the generic tile form; the adaptive entries'
rounds; the refusals.  Shapes, list and plan are those of test_render_tiles_gpu.py."""
import ctypes as C
import os

import numpy as np
import pytest

import spec_graphs as G
from test_render_tiles_gpu import AD, H, LIST, SPP, T, W, _clip, _same, dev  # noqa: F401  (dev: the fixture)

pytestmark = pytest.mark.gpu

BIG_GRAPH = ("lattice", 19, 65)     # 65 nodes: the generic code is a stack walk, the specialised kernel a sweep
SMALL_GRAPH = ("random", 3007, None)  # 11 nodes: a quick run-time compile
GRAPH_VIEW = dict(look_from=(1.0, 1.5, 7.0), look_at=(0.0, 0.0, 0.0), vup=(0.0, 1.0, 0.0), vfov_deg=50.0, aspect_ratio=W / H, aperture=0.0,
                  focus_dist=6.0, time0=0.0, time1=1.0)


def _own_cache(monkeypatch, tmp_path):
    """an empty user cache, and no f32 build behind specialise() (RT1W_NO_JIT stops that one alone: a compile the tests here do not need)"""
    monkeypatch.setenv("RT1W_KERNEL_CACHE", str(tmp_path))
    monkeypatch.setenv("RT1W_NO_JIT", "1")
    monkeypatch.delenv("RT1W_JIT_EXTRA_OPTS", raising=False)


def _check_list(ctx, sc, dev, d_rect, chunk, what):
    """LIST with the flag == every tile's clipped rectangle on the specialised rectangle kernel == LIST without the flag"""
    tiles, st = ctx.render_tiles(W, H, SPP, T, LIST, out_sum=True, chunk=chunk, specialised=True)
    plain, sp = ctx.render_tiles(W, H, SPP, T, LIST, out_sum=True, chunk=chunk)
    explicit = chunk or sc.default_chunk(W, H, SPP)
    assert st["sorted"] & 5 == 5 and not (sp["sorted"] & 4), (what, st, sp)
    assert st["block"] in (128, 256, 512) and st["grid"] >= 1 and st["variant"] == sp["variant"]
    assert st["chunk"] == sp["chunk"] == min(explicit, SPP) and st["n_chunks"] == sp["n_chunks"] and st["passes"] == 1
    assert st["paths"] == sp["paths"] == SPP * sum(tw * th for tw, th in (_clip(x, y) for x, y, _ in LIST))
    assert _same(tiles, plain), (what, chunk)
    assert st["segments"] == sp["segments"]
    segments = 0
    for k, (x0, y0, off) in enumerate(LIST):
        tw, th = _clip(x0, y0)
        sr = ctx.render_device(d_rect, W, H, SPP, tile=(x0, y0, tw, th), sample_offset=off, out_sum=True, chunk=explicit)
        assert sr["sorted"] & 4, (what, sr)
        assert _same(tiles[k, :th, :tw], dev.fetch(d_rect, (th, tw, 3))), (what, chunk, k)
        segments += sr["segments"]
        beyond = np.ones((T, T), dtype=bool)
        beyond[:th, :tw] = False
        assert np.all(tiles[k][beyond].view(np.uint64) == 0), (what, chunk, k)       # exactly +0.0
    assert st["segments"] == segments, (what, chunk)
    return tiles


@pytest.mark.parametrize("what", ["arm5", "arm6", "arm2", "graph65"])
def test_gpu_specialised_tiles_equal_their_rectangles(rt, gpu_ctx_factory, dev, tmp_path, monkeypatch, what):
    """arm5: V0 at four waves, the exchange in two parts; arm6: media; arm2: a noise texture, so three waves and one part; graph65: a
    lattice graph of 65 nodes, whose generic tile form is a stack walk and whose tile form is compiled here (one cache of its own)."""
    if what == "graph65":
        _own_cache(monkeypatch, tmp_path)
        sc = G.build(BIG_GRAPH)[0]
        assert sc.info()["n_nodes"] == 65
        view = GRAPH_VIEW
    else:
        arm = int(what[3:])
        sc = rt.Scene.reference(arm, build_seed=1, aspect_ratio=W / H)
        view = rt.orbit_camera(rt.reference_camera(arm, W / H), 25.0)
    key = sc.kernel_key(tiles=True)
    ctx = rt.Context(sc, 0)
    try:
        if what == "graph65":
            info = ctx.specialise(tiles=True)
            assert info["active"] and not info["from_cache"] and info["key"] == sc.kernel_key()
            assert {f"sweep_{key}", f"sweep_{info['key']}"} == {n.rsplit("-", 1)[0] for n in os.listdir(tmp_path) if n.endswith(".hsaco")}
        d_rect = dev.alloc(T * T * 3 * 8)
        first = None
        for chunk in (2, 0):
            tiles = _check_list(ctx, sc, dev, d_rect, chunk, what)
            first = tiles if first is None else first
        ctx.set_camera(**view)   # the camera travels by value: the same kernel, another picture
        assert sc.kernel_key(tiles=True) == key
        moved = _check_list(ctx, sc, dev, d_rect, 2, what + " moved")
        assert not _same(moved, first)
    finally:
        ctx.close()


def test_gpu_later_item_fetches_span_two_tiles(rt, gpu_ctx_factory):
    """More items than twice the lanes of the persistent grid: every wave fetches again, 64 consecutive items that start anywhere, so a
    fetch spans two tiles and the lookup of rt_tile_item takes its second round.  All 36 tiles of a 96 x 96 frame, one sample per item,
    against the whole-frame render; in several sample passes the same bits."""
    w = h = 96
    sc = rt.Scene.reference(5, build_seed=1, aspect_ratio=1.0)
    ctx = gpu_ctx_factory(sc)
    every = [(x0, y0, 0) for y0 in range(0, h, T) for x0 in range(0, w, T)]
    s0 = ctx.render_tiles(w, h, 1, T, every, out_sum=True, chunk=1, specialised=True)[1]
    assert s0["sorted"] & 5 == 5
    lanes = s0["grid"] * s0["block"]
    spp = 2 * lanes // (len(every) * T * T) + 1   # the smallest with n_tiles T^2 n_chunks > 2 grid block
    tiles, st = ctx.render_tiles(w, h, spp, T, every, out_sum=True, chunk=1, specialised=True)
    assert st["sorted"] & 5 == 5 and (st["grid"], st["block"]) == (s0["grid"], s0["block"]) and st["n_chunks"] == spp and st["passes"] == 1
    assert len(every) * T * T * st["n_chunks"] > 2 * st["grid"] * st["block"] >= len(every) * T * T * (st["n_chunks"] - 1)
    whole, sw = ctx.render(w, h, spp, out_sum=True, chunk=1)
    assert sw["sorted"] & 4 and sw["segments"] == st["segments"] and st["paths"] == sw["paths"] == w * h * spp
    for k, (x0, y0, _) in enumerate(every):
        assert _same(tiles[k], np.ascontiguousarray(whole[y0:y0 + T, x0:x0 + T])), k
    again, sa = ctx.render_tiles(w, h, spp, T, every, out_sum=True, chunk=1, specialised=True, partial_mib=1)
    assert sa["passes"] >= 2 and sa["sorted"] & 5 == 5 and _same(again, tiles) and sa["segments"] == st["segments"]


def test_gpu_fallback_to_the_generic_tile_form(rt, gpu_ctx_factory, tmp_path, monkeypatch):
    """No error where there is no tile form to load: a scene of more than 256 nodes; a graph whose kernels nobody has compiled (and a
    tile render never compiles); a context specialised without RT1W_SPECIALISE_TILES.  With it, the flag is honoured."""
    sc7 = rt.Scene.reference(7, build_seed=1, aspect_ratio=W / H)
    ctx = gpu_ctx_factory(sc7)
    a, sa = ctx.render_tiles(W, H, SPP, T, LIST, out_sum=True, specialised=True)
    b, sb = ctx.render_tiles(W, H, SPP, T, LIST, out_sum=True)
    assert not (sa["sorted"] & 4) and _same(a, b)
    assert {k: v for k, v in sa.items() if not k.endswith("_ms")} == {k: v for k, v in sb.items() if not k.endswith("_ms")}

    _own_cache(monkeypatch, tmp_path)
    sc = G.build(SMALL_GRAPH)[0]
    ctx = rt.Context(sc, 0)
    try:
        a, sa = ctx.render_tiles(W, H, SPP, T, LIST, out_sum=True, specialised=True)
        b, sb = ctx.render_tiles(W, H, SPP, T, LIST, out_sum=True)
        assert not (sa["sorted"] & 4) and sa["sorted"] == sb["sorted"] and (sa["grid"], sa["block"]) == (sb["grid"], sb["block"]) and _same(a, b)
        assert [n for n in os.listdir(tmp_path) if n.endswith(".hsaco")] == []
        assert ctx.specialise()["active"]            # the rectangle kernel alone
        assert len([n for n in os.listdir(tmp_path) if n.endswith(".hsaco")]) == 1
        a, sa = ctx.render_tiles(W, H, SPP, T, LIST, out_sum=True, specialised=True)
        assert not (sa["sorted"] & 4) and _same(a, b)
        with pytest.raises(rt.Rt1wError) as e:       # the tile form's failure is the call's
            ctx.specialise(cached_only=True, tiles=True)
        assert e.value.code == rt.ERR_STATE
        info = ctx.specialise(tiles=True)
        assert info["active"] and info["from_cache"] and info["compile_ms"] > 0.0 and info["key"] == sc.kernel_key()
        assert len([n for n in os.listdir(tmp_path) if n.endswith(".hsaco")]) == 2
        a, sa = ctx.render_tiles(W, H, SPP, T, LIST, out_sum=True, specialised=True)
        assert sa["sorted"] & 5 == 5 and _same(a, b) and sa["segments"] == sb["segments"]
        assert not (ctx.render_tiles(W, H, SPP, T, LIST, out_sum=True)[1]["sorted"] & 4)   # without the flag: as ever
    finally:
        ctx.close()
    # another context of the scene finds the tile form in the cache at its first tile render, whatever its first render asked for
    ctx = rt.Context(sc, 0)
    try:
        assert not (ctx.render_tiles(W, H, SPP, T, LIST, out_sum=True)[1]["sorted"] & 4)
        a, sa = ctx.render_tiles(W, H, SPP, T, LIST, out_sum=True, specialised=True)
        assert sa["sorted"] & 5 == 5 and _same(a, b)
    finally:
        ctx.close()


def test_gpu_adaptive_rounds_on_the_specialised_tile_form(rt, gpu_ctx_factory):
    """The adaptive entries hand the flag to their renders: the same frame, counts, error map and statistics as without it."""
    w = h = 96
    sc = rt.Scene.reference(5, build_seed=1, aspect_ratio=1.0)
    ctx = gpu_ctx_factory(sc)
    f0, s0 = ctx.render(w, h, 8)
    ad = dict(tile=16, **AD)
    a, aspp, sa = ctx.render_adaptive(w, h, adaptive=dict(ad, one_launch=True), global_seed=3, with_stats=True)
    b, bspp, sb = ctx.render_adaptive(w, h, adaptive=dict(ad, one_launch=True), global_seed=3, with_stats=True, flags=rt.TILES_SPECIALISED)
    assert _same(a, b) and _same(aspp, bspp) and bspp.max() > bspp.min()
    assert all(sa[k] == sb[k] for k in ("paths", "segments", "n_chunks", "passes")) and sb["n_chunks"] >= 1
    # without RT1W_ADAPTIVE_ONE_LAUNCH the bit reaches rectangle renders only, which ignore it
    c, cspp = ctx.render_adaptive(w, h, adaptive=ad, global_seed=3, flags=rt.TILES_SPECIALISED)
    assert _same(a, c) and _same(aspp, cspp)
    for entry in (ctx.render_adaptive_filtered, ctx.render_adaptive_guided):
        x = entry(w, h, adaptive=ad, global_seed=3, with_stats=True)
        y = entry(w, h, adaptive=ad, global_seed=3, with_stats=True, flags=rt.TILES_SPECIALISED)
        assert _same(x[0], y[0]) and _same(x[1], y[1]) and _same(x[2], y[2]), entry.__name__
        assert all(x[3][k] == y[3][k] for k in ("paths", "segments", "n_chunks", "passes")) and y[3]["n_chunks"] >= 1
    f1, s1 = ctx.render(w, h, 8)
    assert _same(f0, f1) and s0["segments"] == s1["segments"]


def test_gpu_refusals(rt, gpu_ctx_factory):
    sc = rt.Scene.reference(5, build_seed=1, aspect_ratio=W / H)
    ctx = gpu_ctx_factory(sc)

    def refused(code, text, fn, *a, **kw):
        with pytest.raises(rt.Rt1wError) as e:
            fn(*a, **kw)
        assert e.value.code == code and text in str(e.value), (str(e.value), kw)

    refused(rt.ERR_INVALID, "RT1W_TILES_SPECIALISED and RT1W_GENERIC exclude each other", ctx.render_tiles, W, H, SPP, T, [(0, 0)], specialised=True, generic=True)
    refused(rt.ERR_UNSUPPORTED, "the tile-list kernels are f64 only", ctx.render_tiles, W, H, SPP, T, [(0, 0)], specialised=True, f32=True)
    refused(rt.ERR_INVALID, "rt1w_render_aov_tiles: flags 0 or RT1W_FORCE_VARIANT only", ctx.render_aov_tiles, W, H, SPP, T, [(0, 0)], flags=rt.TILES_SPECIALISED)
    refused(rt.ERR_INVALID, "rt1w_render_tiles: flags 0, RT1W_OUT_SUM or RT1W_GENERIC only", ctx.render_tiles, W, H, SPP, T, [(0, 0)], specialised=True,
            flags=rt.UNSORTED)
    ad = dict(tile=16, **AD)
    refused(rt.ERR_INVALID, "adaptive: with RT1W_ADAPTIVE_ONE_LAUNCH p->flags must be 0 or RT1W_GENERIC (rt1w_render_tiles runs the generic kernels)",
            ctx.render_adaptive, W, H, adaptive=dict(ad, one_launch=True), flags=rt.TILES_SPECIALISED | rt.UNSORTED)
    for bad in (rt.TILES_SPECIALISED | rt.GENERIC, rt.TILES_SPECIALISED | rt.NO_NODE_CACHE):
        refused(rt.ERR_INVALID, "rt1w_render_adaptive_filtered: p->flags must be 0 or RT1W_GENERIC (the rounds go through rt1w_render_tiles, which runs "
                "the generic kernels)", ctx.render_adaptive_filtered, W, H, adaptive=ad, flags=bad)
    # the rectangle entries ignore the bit, as they ignore unknown bits
    p = ctx._params(W, H, SPP, 50, None, 0, 0, 0, False)
    p.flags |= rt.TILES_SPECIALISED
    out, st = np.empty((H, W, 3)), rt.Stats()
    assert rt._lib.rt1w_render(ctx._h, C.byref(p), out.ctypes.data_as(C.c_void_p), C.byref(st)) == 0 and st.sorted & 4
    assert _same(out, ctx.render(W, H, SPP)[0])
