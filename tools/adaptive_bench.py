#!/usr/bin/env python3
"""Cost of adaptive sampling (rt1w_render_adaptive, csrc/adaptive.hip + the plan in csrc/rt_adaptive_plan.h) against one render of the same
samples.

For C3 (Cornell 600 x 600) and C4 (final_scene 800 x 800) at budgets of 64 and 256 mean samples per pixel, default parameters, one child
process per case:
  * the whole call rt1w_render_adaptive (median total_ms of `--reps` calls after one warm-up), its rounds and render launches;
  * rt1w_render of the same total samples (spp = the budget: the call spends it to within one tile), in the same process and, with
    `--parent-root DIR` (a built checkout of the parent commit), in a child of its own that imports that checkout's package and so runs
    the parent commit's librt1w.so: the comparison the feature answers to;
  * the difference in beauty samples per pixel: (adaptive - uniform) / (uniform / spp);
  * the split of the call, from one composition of the public device entries whose own timers are summed by kind: the render launches
    (total_ms of every rt1w_render_device, kernel_ms alongside), the merge and tile-error kernels (total_ms and kernel_ms), and the
    per-round device->host copy of the tile errors (host clock around the copy).
With `--one-launch` every case gets a second column: the call with RT1W_ADAPTIVE_ONE_LAUNCH (every round one rt1w_render_tiles_device of all
its tiles and one rt1w_accum_merge_tiles_device), its launches, and the same split from the composition over those two entries.  `--case
NAME:BUDGET` (repeatable; c3:16 is Cornell 600 x 600 at a budget of 16) replaces the default cases.
With `--filtered` every case gets a third column, written to a file of its own (`--filtered-out`, default
profiles/adaptive_filtered_bench.json): rt1w_render_adaptive_filtered (the plan steered by the filtered frame's half-buffer error) at the same
budget, against rt1w_render_adaptive with RT1W_ADAPTIVE_ONE_LAUNCH and the variance-guided filter (this library's and, with `--parent-root`,
the parent commit's) and against rt1w_render_denoised_var of the same mean sample count; the split of the call by kind from a composition
of the public device entries (render launches, filter passes, resolve + tile-error kernels, merges, the err copies); and the level kernel
of rt1w_denoise_var_halves against rt1w_denoise_var's per step, as differences of kernel_ms between `iterations` k and k - 1.
With `--cross` every case gets a column of its own file (`--cross-out`, default profiles/adaptive_cross_bench.json): rt1w_render_adaptive_cross
against rt1w_render_adaptive_filtered at the same budget in one process, and the level kernel of rt1w_denoise_cross against
rt1w_denoise_var_halves's per step; `--cross-root LABEL=DIR` repeats it with the library of another built checkout (the staged-against-direct
A/B: one built with EXTRA_HIPFLAGS=-DRT_DC_STAGED_LEVELS=0).  `--cross` alone runs only that column.
With `--guided` every case gets a column of its own file (`--guided-out`, default profiles/adaptive_guided_bench.json): rt1w_render_adaptive_guided
against rt1w_render_adaptive_filtered at the same budget in one process; the share of the call its guide passes take (rt1w_render_aov_tiles,
rt1w_guides_merge_tiles, rt1w_guides_resolve), from a composition of the public device entries; and the tile-list AOV kernel over every tile
of the frame against rt1w_render_aov_device of the whole frame at the same samples, as segments per second.  `--guided` alone runs only that
column.
Writes one JSON file (default profiles/adaptive_bench.json).  Times are wall-clock medians of a few calls on a shared machine: read them
to two digits.

usage: python3 tools/adaptive_bench.py [--out FILE] [--reps N] [--parent-root BUILT-CHECKOUT-OF-THE-PARENT] [--one-launch] [--filtered [--filtered-out FILE]]
       [--cross [--cross-out FILE] [--cross-root LABEL=DIR ...]] [--guided [--guided-out FILE]] [--case NAME:BUDGET ...]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = [("c3", 5, 600, 600), ("c4", 7, 800, 800)]
BUDGETS = (64, 256)
TILE, PILOT, SHARE, BATCH_DIV, MAX_FACTOR = 16, 4, 0.25, 8, 8   # the defaults of rt1w_adaptive_params, spelled out for the composition


def _rt():
    import importlib
    sys.path.insert(0, os.environ.get("ADAPTIVE_BENCH_ROOT") or ROOT)
    return importlib.import_module("raytracing-1w_amd")


def child_uniform(arm, W, H, spp, reps):
    rt = _rt()
    ctx = rt.Context(rt.Scene.reference(arm, build_seed=1), 0)
    tot, ker = [], []
    for i in range(1 + reps):
        _, st = ctx.render(W, H, spp)
        if i:
            tot.append(st["total_ms"]); ker.append(st["kernel_ms"])
    ctx.close()
    print("ADJSON " + json.dumps({"total_ms": tot, "kernel_ms": ker, "lib": rt.LIB_PATH}), flush=True)


def _runs(taken, m, tx_n, W, H):
    runs, prev = [], None
    for t in sorted(taken):
        tx, ty = t % tx_n, t // tx_n
        x0, y0 = tx * TILE, ty * TILE
        tw, th, mt = min(TILE, W - x0), min(TILE, H - y0), int(m.flat[t])
        if prev is not None and t == prev + 1 and tx != 0 and runs[-1][4] == mt:
            runs[-1][2] += tw
        else:
            runs.append([x0, y0, tw, th, mt])
        prev = t
    return runs


def child_adaptive(arm, W, H, budget, reps, one=False):
    import numpy as np
    rt = _rt()
    sc = rt.Scene.reference(arm, build_seed=1)
    ctx = rt.Context(sc, 0)
    ad = dict(budget_spp=budget, one_launch=True) if one else dict(budget_spp=budget)
    calls = []
    for i in range(1 + reps):
        _, spp, st = ctx.render_adaptive(W, H, adaptive=ad, with_stats=True)
        if i:
            calls.append(st)
    # the split: the same plan over the public device entries, their own timers summed by kind
    hip = C.CDLL("libamdhip64.so")

    def alloc(nbytes):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(nbytes)) == 0
        return p.value
    n = max(1, budget // BATCH_DIV)
    full = dict(tile=TILE, batch_spp=n, pilot_batches=PILOT, budget_spp=budget, max_spp=MAX_FACTOR * budget, round_share=SHARE)
    npix = W * H
    tx_n, ty_n = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    chunk = sc.default_chunk(W, H, n)
    d_aov, d_sums, d_acc, d_err = alloc(npix * 64), alloc(max(npix, tx_n * ty_n * TILE * TILE) * 24), alloc(npix * 64), alloc(tx_n * ty_n * 8)
    assert hip.hipMemset(C.c_void_p(d_acc), 0, C.c_size_t(npix * 64)) == 0
    ctx.render_aov_device(d_aov, W, H, PILOT * n)
    part = {k: 0.0 for k in ("render_total_ms", "render_kernel_ms", "merge_total_ms", "merge_kernel_ms", "error_total_ms", "error_kernel_ms", "copy_ms")}
    launches = 0

    def batch(rect, mt):
        nonlocal launches
        s = ctx.render_device(d_sums, W, H, n, tile=tuple(rect), sample_offset=mt * n, chunk=chunk, out_sum=True)
        g = ctx.accum_merge_device(d_acc, d_sums, d_aov, W, H, tuple(rect), n)
        part["render_total_ms"] += s["total_ms"]; part["render_kernel_ms"] += s["kernel_ms"]
        part["merge_total_ms"] += g["total_ms"]; part["merge_kernel_ms"] += g["kernel_ms"]
        launches += 1

    def batch_tiles(taken, m):
        nonlocal launches
        tiles = [((t % tx_n) * TILE, (t // tx_n) * TILE, int(m.flat[t]) * n) for t in taken]
        s = ctx.render_tiles_device(d_sums, W, H, n, TILE, tiles, chunk=chunk, out_sum=True)
        g = ctx.accum_merge_tiles_device(d_acc, d_sums, d_aov, W, H, TILE, tiles, n)
        part["render_total_ms"] += s["total_ms"]; part["render_kernel_ms"] += s["kernel_ms"]
        part["merge_total_ms"] += g["total_ms"]; part["merge_kernel_ms"] += g["kernel_ms"]
        launches += 1
    for b in range(PILOT):
        batch((0, 0, W, H), b)
    m = np.full((ty_n, tx_n), PILOT, dtype=np.uint32)
    err = np.empty((ty_n, tx_n))
    rounds = 0
    while True:
        e = ctx.accum_tile_error_device(d_acc, d_err, W, H, TILE)
        part["error_total_ms"] += e["total_ms"]; part["error_kernel_ms"] += e["kernel_ms"]
        t0 = time.perf_counter()
        assert hip.hipMemcpy(err.ctypes.data_as(C.c_void_p), C.c_void_p(d_err), C.c_size_t(err.nbytes), 2) == 0
        part["copy_ms"] += (time.perf_counter() - t0) * 1e3
        taken = rt.adaptive_select(W, H, err, m, **full)
        if not taken:
            break
        rounds += 1
        if one:
            batch_tiles(taken, m)
        else:
            for r in _runs(taken, m, tx_n, W, H):
                batch(r[:4], r[4])
        for t in taken:
            m.flat[t] += 1
    assert rounds == calls[-1]["n_chunks"] and launches <= calls[-1]["passes"], "the composition is not the call's plan"
    for p in (d_aov, d_sums, d_acc, d_err):
        hip.hipFree(C.c_void_p(p))
    ctx.close()
    print("ADJSON " + json.dumps({"total_ms": [c["total_ms"] for c in calls], "kernel_ms": [c["kernel_ms"] for c in calls], "rounds": rounds,
                                  "launches": launches, "passes": calls[-1]["passes"], "spent_spp": float(spp.mean()), "max_spp": float(spp.max()),
                                  "min_spp": float(spp.min()), "split": part}), flush=True)


def child_filtered(arm, W, H, budget, reps):
    """rt1w_render_adaptive_filtered: the call, its split over the public device entries, the filter per step"""
    import numpy as np
    rt = _rt()
    sc = rt.Scene.reference(arm, build_seed=1)
    ctx = rt.Context(sc, 0)
    calls = []
    for i in range(1 + reps):
        _, spp, _, st = ctx.render_adaptive_filtered(W, H, adaptive=dict(budget_spp=budget), with_stats=True)
        if i:
            calls.append(st)
    hip = C.CDLL("libamdhip64.so")

    def alloc(nbytes):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(nbytes)) == 0
        return p.value
    n = max(1, budget // BATCH_DIV)
    pair = dict(tile=TILE, batch_spp=2 * n, pilot_batches=max(2, PILOT // 2), budget_spp=budget, max_spp=MAX_FACTOR * budget, round_share=SHARE)
    npix = W * H
    tx_n, ty_n = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    chunk = sc.default_chunk(W, H, n)
    d_aov, d_sums, d_err = alloc(npix * 64), alloc(max(npix, 2 * tx_n * ty_n * TILE * TILE) * 24), alloc(tx_n * ty_n * 8)
    d_acc = [alloc(npix * 64), alloc(npix * 64)]
    d_frame, d_var, d_spp, d_epx, d_ha, d_hb = alloc(npix * 24), alloc(npix * 8), alloc(npix * 8), alloc(npix * 8), alloc(npix * 24), alloc(npix * 24)
    for a in d_acc:
        assert hip.hipMemset(C.c_void_p(a), 0, C.c_size_t(npix * 64)) == 0
    ctx.render_aov_device(d_aov, W, H, PILOT * n)
    kinds = ("render", "merge", "filter", "resolve_error")
    part = {f"{k}_{t}": 0.0 for k in kinds for t in ("total_ms", "kernel_ms")}
    part["copy_ms"] = 0.0

    def add(kind, st):
        part[kind + "_total_ms"] += st["total_ms"]; part[kind + "_kernel_ms"] += st["kernel_ms"]
    for b in range(PILOT):
        add("render", ctx.render_device(d_sums, W, H, n, sample_offset=b * n, chunk=chunk, out_sum=True))
        add("merge", ctx.accum_merge_device(d_acc[b & 1], d_sums, d_aov, W, H, (0, 0, W, H), n))
    m = np.full((ty_n, tx_n), PILOT // 2, dtype=np.uint32)
    err = np.empty((ty_n, tx_n))
    rounds = 0
    while True:
        add("resolve_error", ctx.halves_resolve_device(d_acc[0], d_acc[1], d_frame, d_var, d_ha, d_hb, d_spp, W, H, n))
        add("filter", ctx.denoise_var_halves_device(d_frame, d_aov, d_var, d_ha, d_hb, d_frame, d_epx, W, H))
        add("resolve_error", ctx.tile_error_map_device(d_epx, d_err, W, H, TILE))
        t0 = time.perf_counter()
        assert hip.hipMemcpy(err.ctypes.data_as(C.c_void_p), C.c_void_p(d_err), C.c_size_t(err.nbytes), 2) == 0
        part["copy_ms"] += (time.perf_counter() - t0) * 1e3
        taken = rt.adaptive_select(W, H, err, m, **pair)
        if not taken:
            break
        rounds += 1
        tiles = [((t % tx_n) * TILE, (t // tx_n) * TILE, (2 * int(m.flat[t]) + half) * n) for half in (0, 1) for t in taken]
        add("render", ctx.render_tiles_device(d_sums, W, H, n, TILE, tiles, chunk=chunk, out_sum=True))
        k = len(taken)
        add("merge", ctx.accum_merge_tiles_device(d_acc[0], d_sums, d_aov, W, H, TILE, tiles[:k], n))
        add("merge", ctx.accum_merge_tiles_device(d_acc[1], d_sums + k * TILE * TILE * 24, d_aov, W, H, TILE, tiles[k:], n))
        for t in taken:
            m.flat[t] += 1
    assert rounds == calls[-1]["n_chunks"], "the composition is not the call's plan"
    # the filters per step on the last round's buffers: kernel_ms(iterations k) - kernel_ms(iterations k - 1), medians of `reps`
    d_out = alloc(npix * 24)
    steps = {"halves": [], "var": []}
    for name in steps:
        prev = 0.0
        for it in range(1, 6):
            ms = []
            for i in range(1 + max(reps, 3)):
                st = (ctx.denoise_var_halves_device(d_frame, d_aov, d_var, d_ha, d_hb, d_out, d_epx, W, H, iterations=it) if name == "halves"
                      else ctx.denoise_var_device(d_frame, d_aov, d_var, d_out, W, H, iterations=it))
                if i:
                    ms.append(st["kernel_ms"])
            cur = statistics.median(ms)
            steps[name].append(cur - prev)   # the first entry holds the prepare pass too
            prev = cur
    ctx.close()
    print("ADJSON " + json.dumps({"total_ms": [c["total_ms"] for c in calls], "kernel_ms": [c["kernel_ms"] for c in calls], "rounds": rounds,
                                  "passes": calls[-1]["passes"], "spent_spp": float(spp.mean()), "max_spp": float(spp.max()), "min_spp": float(spp.min()),
                                  "split": part, "filter_ms_by_iterations_step": steps,
                                  "halves_over_var_per_step": [a / b for a, b in zip(steps["halves"], steps["var"])]}), flush=True)


def child_cross(arm, W, H, budget, reps):
    """rt1w_render_adaptive_cross against rt1w_render_adaptive_filtered at the same budget, and the level kernel of rt1w_denoise_cross against
    rt1w_denoise_var_halves's per step (differences of kernel_ms between `iterations` k and k - 1), all in one process, on the halves the
    pilot of the plan leaves"""
    rt = _rt()
    sc = rt.Scene.reference(arm, build_seed=1)
    ctx = rt.Context(sc, 0)
    calls = {"cross": [], "filtered": []}
    for i in range(1 + reps):
        for name, fn in (("cross", ctx.render_adaptive_cross), ("filtered", ctx.render_adaptive_filtered)):
            _, spp, _, st = fn(W, H, adaptive=dict(budget_spp=budget), with_stats=True)
            if i:
                calls[name].append(dict(total_ms=st["total_ms"], kernel_ms=st["kernel_ms"], rounds=st["n_chunks"], spent_spp=float(spp.mean())))
    hip = C.CDLL("libamdhip64.so")

    def alloc(nbytes):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(nbytes)) == 0
        return p.value
    n = max(1, budget // BATCH_DIV)
    npix = W * H
    d_aov, d_sums = alloc(npix * 64), alloc(npix * 24)
    d_acc = [alloc(npix * 64), alloc(npix * 64)]
    d_frame, d_var, d_spp, d_epx, d_ha, d_hb, d_out = (alloc(npix * k) for k in (24, 8, 8, 8, 24, 24, 24))
    for a in d_acc:
        assert hip.hipMemset(C.c_void_p(a), 0, C.c_size_t(npix * 64)) == 0
    ctx.render_aov_device(d_aov, W, H, PILOT * n)
    for b in range(PILOT):
        ctx.render_device(d_sums, W, H, n, sample_offset=b * n, chunk=sc.default_chunk(W, H, n), out_sum=True)
        ctx.accum_merge_device(d_acc[b & 1], d_sums, d_aov, W, H, (0, 0, W, H), n)
    ctx.halves_resolve_device(d_acc[0], d_acc[1], d_frame, d_var, d_ha, d_hb, d_spp, W, H, n)
    steps = {"cross": [], "halves": []}
    for name in steps:
        fn = ctx.denoise_cross_device if name == "cross" else ctx.denoise_var_halves_device
        prev = 0.0
        for it in range(1, 6):
            ms = [fn(d_frame, d_aov, d_var, d_ha, d_hb, d_out, d_epx, W, H, iterations=it)["kernel_ms"] for _ in range(1 + max(reps, 5))][1:]
            cur = statistics.median(ms)
            steps[name].append(cur - prev)   # the first entry holds the prepare pass too
            prev = cur
    ctx.close()
    print("ADJSON " + json.dumps({"calls": calls, "filter_ms_by_iterations_step": steps, "lib": os.path.relpath(rt.LIB_PATH, ROOT),
                                  "cross_over_halves_per_step": [a / b for a, b in zip(steps["cross"], steps["halves"])]}), flush=True)


def child_guided(arm, W, H, budget, reps):
    """rt1w_render_adaptive_guided against rt1w_render_adaptive_filtered at the same budget in one process; the guided call's split over the
    public device entries with the guide passes as kinds of their own; the tile-list AOV kernel against rt1w_render_aov_device"""
    import numpy as np
    rt = _rt()
    sc = rt.Scene.reference(arm, build_seed=1)
    ctx = rt.Context(sc, 0)
    calls = {"guided": [], "filtered": []}
    for i in range(1 + reps):
        for name, fn in (("guided", ctx.render_adaptive_guided), ("filtered", ctx.render_adaptive_filtered)):
            _, spp, _, st = fn(W, H, adaptive=dict(budget_spp=budget), with_stats=True)
            if i:
                calls[name].append(dict(total_ms=st["total_ms"], kernel_ms=st["kernel_ms"], rounds=st["n_chunks"], passes=st["passes"], spent_spp=float(spp.mean())))
    hip = C.CDLL("libamdhip64.so")

    def alloc(nbytes):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(nbytes)) == 0
        return p.value
    n = max(1, budget // BATCH_DIV)
    pair = dict(tile=TILE, batch_spp=2 * n, pilot_batches=max(2, PILOT // 2), budget_spp=budget, max_spp=MAX_FACTOR * budget, round_share=SHARE)
    npix = W * H
    tx_n, ty_n = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    nt = tx_n * ty_n
    chunk = sc.default_chunk(W, H, n)
    d_aov, d_guides, d_sums, d_err = alloc(npix * 64), alloc(npix * 64), alloc(max(npix, 2 * nt * TILE * TILE) * 24), alloc(nt * 8)
    d_asums, d_gacc = alloc(nt * TILE * TILE * 64), alloc(npix * 72)
    d_acc = [alloc(npix * 64), alloc(npix * 64)]
    d_frame, d_var, d_spp, d_epx, d_ha, d_hb = alloc(npix * 24), alloc(npix * 8), alloc(npix * 8), alloc(npix * 8), alloc(npix * 24), alloc(npix * 24)
    for a, k in ((d_acc[0], 64), (d_acc[1], 64), (d_gacc, 72)):
        assert hip.hipMemset(C.c_void_p(a), 0, C.c_size_t(npix * k)) == 0
    kinds = ("render", "merge", "filter", "resolve_error", "aov_tiles", "guides_merge", "guides_resolve")
    part = {f"{k}_{t}": 0.0 for k in kinds for t in ("total_ms", "kernel_ms")}
    part["copy_ms"] = 0.0

    def add(kind, st):
        part[kind + "_total_ms"] += st["total_ms"]; part[kind + "_kernel_ms"] += st["kernel_ms"]
    every = [(x, y, 0) for y in range(0, H, TILE) for x in range(0, W, TILE)]
    add("aov_tiles", ctx.render_aov_tiles_device(d_asums, W, H, PILOT * n, TILE, every))
    add("guides_merge", ctx.guides_merge_tiles_device(d_gacc, d_asums, W, H, TILE, every, PILOT * n))
    add("guides_resolve", ctx.guides_resolve_device(d_gacc, d_aov, W, H))
    for b in range(PILOT):
        add("render", ctx.render_device(d_sums, W, H, n, sample_offset=b * n, chunk=chunk, out_sum=True))
        add("merge", ctx.accum_merge_device(d_acc[b & 1], d_sums, d_aov, W, H, (0, 0, W, H), n))
    m = np.full((ty_n, tx_n), PILOT // 2, dtype=np.uint32)
    err = np.empty((ty_n, tx_n))
    rounds = 0
    while True:
        add("resolve_error", ctx.halves_resolve_device(d_acc[0], d_acc[1], d_frame, d_var, d_ha, d_hb, d_spp, W, H, n))
        add("guides_resolve", ctx.guides_resolve_device(d_gacc, d_guides, W, H))
        add("filter", ctx.denoise_var_halves_device(d_frame, d_guides, d_var, d_ha, d_hb, d_frame, d_epx, W, H))
        add("resolve_error", ctx.tile_error_map_device(d_epx, d_err, W, H, TILE))
        t0 = time.perf_counter()
        assert hip.hipMemcpy(err.ctypes.data_as(C.c_void_p), C.c_void_p(d_err), C.c_size_t(err.nbytes), 2) == 0
        part["copy_ms"] += (time.perf_counter() - t0) * 1e3
        taken = rt.adaptive_select(W, H, err, m, **pair)
        if not taken:
            break
        rounds += 1
        tiles = [((t % tx_n) * TILE, (t // tx_n) * TILE, (2 * int(m.flat[t]) + half) * n) for half in (0, 1) for t in taken]
        add("render", ctx.render_tiles_device(d_sums, W, H, n, TILE, tiles, chunk=chunk, out_sum=True))
        k = len(taken)
        add("merge", ctx.accum_merge_tiles_device(d_acc[0], d_sums, d_aov, W, H, TILE, tiles[:k], n))
        add("merge", ctx.accum_merge_tiles_device(d_acc[1], d_sums + k * TILE * TILE * 24, d_aov, W, H, TILE, tiles[k:], n))
        add("aov_tiles", ctx.render_aov_tiles_device(d_asums, W, H, 2 * n, TILE, tiles[:k]))
        add("guides_merge", ctx.guides_merge_tiles_device(d_gacc, d_asums, W, H, TILE, tiles[:k], 2 * n))
        for t in taken:
            m.flat[t] += 1
    assert rounds == calls["guided"][-1]["rounds"], "the composition is not the call's plan"
    guide_total = sum(part[k + "_total_ms"] for k in ("aov_tiles", "guides_merge", "guides_resolve"))
    guide_kernel = sum(part[k + "_kernel_ms"] for k in ("aov_tiles", "guides_merge", "guides_resolve"))
    all_total = sum(v for k, v in part.items() if k.endswith("_total_ms")) + part["copy_ms"]
    all_kernel = sum(v for k, v in part.items() if k.endswith("_kernel_ms"))
    # the tile-list AOV kernel over every tile of the frame against rt1w_render_aov_device of the whole frame, the same samples
    spp_k = PILOT * n
    tile_ms, rect_ms, seg = [], [], {}
    for i in range(1 + max(reps, 5)):
        st, sr = ctx.render_aov_tiles_device(d_asums, W, H, spp_k, TILE, every), ctx.render_aov_device(d_aov, W, H, spp_k)
        seg = {"tiles": st["segments"], "rectangle": sr["segments"]}
        if i:
            tile_ms.append(st["kernel_ms"]); rect_ms.append(sr["kernel_ms"])
    t_ms, r_ms = statistics.median(tile_ms), statistics.median(rect_ms)
    ctx.close()
    print("ADJSON " + json.dumps({"calls": calls, "split": part, "guide_share_of_total_ms": guide_total / all_total,
                                  "guide_share_of_kernel_ms": guide_kernel / all_kernel, "lib": os.path.relpath(rt.LIB_PATH, ROOT),
                                  "aov_kernel": {"spp": spp_k, "segments": seg, "tiles_kernel_ms": t_ms, "rectangle_kernel_ms": r_ms,
                                                 "tiles_segments_per_s": seg["tiles"] / (t_ms * 1e-3), "rectangle_segments_per_s": seg["rectangle"] / (r_ms * 1e-3),
                                                 "tiles_over_rectangle_rate": (seg["tiles"] / t_ms) / (seg["rectangle"] / r_ms)}}), flush=True)


def child_existing(arm, W, H, budget, reps, spp_uniform):
    """what the new call is compared with: rt1w_render_adaptive with RT1W_ADAPTIVE_ONE_LAUNCH and the filter, and rt1w_render_denoised_var of
    `spp_uniform` samples (a multiple of 4)"""
    rt = _rt()
    ctx = rt.Context(rt.Scene.reference(arm, build_seed=1), 0)
    out = {"adaptive_one_launch_filter": [], "denoised_var": [], "lib": rt.LIB_PATH, "denoised_var_spp": spp_uniform}
    for i in range(1 + reps):
        _, _, st = ctx.render_adaptive(W, H, adaptive=dict(budget_spp=budget, one_launch=True), filter=True, with_stats=True)
        _, sv = ctx.render_denoised_var(W, H, spp_uniform, with_stats=True)
        if i:
            out["adaptive_one_launch_filter"].append(st["total_ms"]); out["denoised_var"].append(sv["total_ms"])
    ctx.close()
    print("ADJSON " + json.dumps(out), flush=True)


def run_child(args, root=None):
    env = dict(os.environ)
    if root:
        env["ADAPTIVE_BENCH_ROOT"] = os.path.abspath(root)
    out = subprocess.run([sys.executable, os.path.abspath(__file__)] + [str(a) for a in args], env=env, capture_output=True, text=True, timeout=900)
    for line in out.stdout.splitlines():
        if line.startswith("ADJSON "):
            return json.loads(line[7:])
    raise RuntimeError(f"child {args} failed:\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive_bench.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--one-launch", action="store_true")
    ap.add_argument("--case", action="append", default=None)
    ap.add_argument("--filtered", action="store_true")
    ap.add_argument("--filtered-out", default=os.path.join(ROOT, "profiles", "adaptive_filtered_bench.json"))
    ap.add_argument("--cross", action="store_true")
    ap.add_argument("--cross-out", default=os.path.join(ROOT, "profiles", "adaptive_cross_bench.json"))
    ap.add_argument("--cross-root", action="append", default=None,
                    help="LABEL=BUILT-CHECKOUT: the cross column again with that checkout's library, e.g. one built with -DRT_DC_STAGED_LEVELS=0")
    ap.add_argument("--guided", action="store_true")
    ap.add_argument("--guided-out", default=os.path.join(ROOT, "profiles", "adaptive_guided_bench.json"))
    ap.add_argument("--child", nargs="*")
    a = ap.parse_args()
    if a.child:
        kind, arm, W, H, n, reps = a.child[0], *map(int, a.child[1:])
        if kind == "uniform":
            return child_uniform(arm, W, H, n, reps)
        if kind == "filtered":
            return child_filtered(arm, W, H, n, reps)
        if kind == "cross":
            return child_cross(arm, W, H, n, reps)
        if kind == "guided":
            return child_guided(arm, W, H, n, reps)
        if kind.startswith("existing"):
            return child_existing(arm, W, H, n, reps, int(kind[8:]))
        return child_adaptive(arm, W, H, n, reps, one=kind == "adaptive1")
    by_name = {c[0]: c for c in CONFIGS}
    cases = [(by_name[c.split(":")[0]], int(c.split(":")[1])) for c in a.case] if a.case else [(c, b) for c in CONFIGS for b in BUDGETS]
    rows, frows, crows, grows = [], [], [], []
    for (name, arm, W, H), budget in cases:
        if a.cross:
            cr = {"this library": run_child(["--child", "cross", arm, W, H, budget, a.reps])}
            for spec in a.cross_root or []:
                label, root = spec.split("=", 1)
                cr[label] = run_child(["--child", "cross", arm, W, H, budget, a.reps], root=root)
            for label, c in cr.items():
                med = {k: statistics.median(x["total_ms"] for x in v) for k, v in c["calls"].items()}
                print(f"{name} budget {budget} [{label}]: cross {med['cross']:.1f} ms ({c['calls']['cross'][-1]['rounds']} rounds), filtered error "
                      f"{med['filtered']:.1f} ms ({c['calls']['filtered'][-1]['rounds']} rounds); cross / halves level kernel per step "
                      f"{['%.2f' % x for x in c['cross_over_halves_per_step']]} (ms {['%.3f' % x for x in c['filter_ms_by_iterations_step']['cross']]} / "
                      f"{['%.3f' % x for x in c['filter_ms_by_iterations_step']['halves']]})", flush=True)
            crows.append({"config": name, "arm": arm, "width": W, "height": H, "budget_spp": budget, "cross": cr})
        if a.guided:
            g = run_child(["--child", "guided", arm, W, H, budget, a.reps])
            med = {k: statistics.median(x["total_ms"] for x in v) for k, v in g["calls"].items()}
            k = g["aov_kernel"]
            print(f"{name} budget {budget}: guided {med['guided']:.1f} ms ({g['calls']['guided'][-1]['rounds']} rounds), filtered error {med['filtered']:.1f} ms "
                  f"({g['calls']['filtered'][-1]['rounds']} rounds), ratio {med['guided'] / med['filtered']:.2f}; guide passes {100 * g['guide_share_of_total_ms']:.1f} % "
                  f"of the call's entries ({100 * g['guide_share_of_kernel_ms']:.1f} % of kernel time); tile-list AOV kernel {k['tiles_kernel_ms']:.3f} ms against "
                  f"{k['rectangle_kernel_ms']:.3f} ms at {k['spp']} spp: {k['tiles_over_rectangle_rate']:.2f} of its segments per second", flush=True)
            grows.append({"config": name, "arm": arm, "width": W, "height": H, "budget_spp": budget, "guided_total_ms": med["guided"],
                          "filtered_total_ms": med["filtered"], "guided_over_filtered": med["guided"] / med["filtered"], "guided": g})
        if not (a.cross or a.guided) or a.filtered or a.one_launch:
            ad = run_child(["--child", "adaptive", arm, W, H, budget, a.reps])
            one = run_child(["--child", "adaptive1", arm, W, H, budget, a.reps]) if a.one_launch else None
            un = run_child(["--child", "uniform", arm, W, H, budget, a.reps])
            par = run_child(["--child", "uniform", arm, W, H, budget, a.reps], root=a.parent_root) if a.parent_root else None
            base = statistics.median((par or un)["total_ms"])
            call = statistics.median(ad["total_ms"])
            row = {"config": name, "arm": arm, "width": W, "height": H, "budget_spp": budget, "adaptive": ad, "uniform_this_library": un,
                   "uniform_parent_library": par, "adaptive_total_ms": call, "uniform_total_ms": base,
                   "baseline": "parent library" if par else "this library",
                   "extra_beauty_spp": (call - base) / (base / budget)}
            if one:
                call1 = statistics.median(one["total_ms"])
                row.update({"adaptive_one_launch": one, "adaptive_one_launch_total_ms": call1,
                            "extra_beauty_spp_one_launch": (call1 - base) / (base / budget)})
                print(f"{name} budget {budget}: one launch per round {call1:.1f} ms ({one['rounds']} rounds, {one['launches']} launches, "
                      f"{one['passes']} passes); split {one['split']}", flush=True)
            print(f"{name} budget {budget}: adaptive {call:.1f} ms ({ad['rounds']} rounds, {ad['launches']} launches), uniform {base:.1f} ms, "
                  f"+{row['extra_beauty_spp']:.1f} beauty spp; split {ad['split']}", flush=True)
            rows.append(row)
            if a.filtered:
                fl = run_child(["--child", "filtered", arm, W, H, budget, a.reps])
                spp4 = max(4, int(round(fl["spent_spp"] / 4.0)) * 4)
                ex = run_child(["--child", f"existing{spp4}", arm, W, H, budget, a.reps])
                exp = run_child(["--child", f"existing{spp4}", arm, W, H, budget, a.reps], root=a.parent_root) if a.parent_root else None
                frow = {"config": name, "arm": arm, "width": W, "height": H, "budget_spp": budget, "filtered": fl, "existing_this_library": ex,
                        "existing_parent_library": exp, "filtered_total_ms": statistics.median(fl["total_ms"]),
                        "adaptive_one_launch_filter_total_ms": statistics.median((exp or ex)["adaptive_one_launch_filter"]),
                        "denoised_var_total_ms": statistics.median((exp or ex)["denoised_var"]), "baseline": "parent library" if exp else "this library"}
                print(f"{name} budget {budget}: filtered error {frow['filtered_total_ms']:.1f} ms ({fl['rounds']} rounds, {fl['passes']} passes), adaptive one launch + "
                      f"filter {frow['adaptive_one_launch_filter_total_ms']:.1f} ms, denoised_var at {spp4} spp {frow['denoised_var_total_ms']:.1f} ms; split {fl['split']}; "
                      f"halves / var level kernel per step {['%.2f' % x for x in fl['halves_over_var_per_step']]}", flush=True)
                frows.append(frow)
    if a.cross:
        os.makedirs(os.path.dirname(a.cross_out), exist_ok=True)
        with open(a.cross_out, "w") as f:
            json.dump({"tool": "tools/adaptive_bench.py --cross", "reps": a.reps, "rows": crows}, f, indent=1)
            f.write("\n")
    if a.guided:
        os.makedirs(os.path.dirname(a.guided_out), exist_ok=True)
        with open(a.guided_out, "w") as f:
            json.dump({"tool": "tools/adaptive_bench.py --guided", "reps": a.reps, "rows": grows}, f, indent=1)
            f.write("\n")
    if not rows:
        return
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/adaptive_bench.py", "reps": a.reps, "rows": rows}, f, indent=1)
        f.write("\n")
    if a.filtered:
        with open(a.filtered_out, "w") as f:
            json.dump({"tool": "tools/adaptive_bench.py --filtered", "reps": a.reps, "rows": frows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
