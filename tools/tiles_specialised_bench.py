#!/usr/bin/env python3
"""The tile-list form of the scene-specialised kernels (RT1W_TILES_SPECIALISED) against the generic tile-list kernels and against the
specialised rectangle kernel, in one process per scene.

For cornell_box (arm 5) and cornell_smoke (arm 6) at 600 x 600:
  * rt1w_render_tiles_device over all tiles of the frame, T = 16 and T = 64, at 16 and 256 spp, with and without the flag (without it:
    the generic tile-list kernel, which is what the parent commit runs);
  * rt1w_render_device of the whole frame at the same spp: the specialised rectangle kernel, the ceiling;
  * rt1w_render_adaptive_filtered at budgets of 16 and 128 mean samples per pixel, with and without the flag.
Every variant is warmed up once, then the variants of a group alternate, `--reps` (5) rounds.  kernel_ms is the stats' (device events),
total_ms the host clock of the call.  A difference between two variants COUNTS only where the two ranges of repeats do not overlap
(`separated`).  Writes one JSON file (default profiles/tiles_specialised_bench.json), one line per variant in "lines".

usage: python3 tools/tiles_specialised_bench.py [--out FILE] [--reps N] [--size N]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))
SCENES = (("cornell_box", 5), ("cornell_smoke", 6))


def summary(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def alternate(variants, reps):
    """variants: {name: callable -> stats dict}; one warm-up each, then `reps` rounds over all of them"""
    got = {n: {"kernel_ms": [], "total_ms": []} for n in variants}
    for n, fn in variants.items():
        got[n]["sorted"] = fn()["sorted"]
    for _ in range(reps):
        for n, fn in variants.items():
            st = fn()
            got[n]["kernel_ms"].append(st["kernel_ms"])
            got[n]["total_ms"].append(st["total_ms"])
    return got


def compare(lines, a, b, field):
    """a over b by medians of `field`, and whether the two ranges of repeats are apart"""
    xa, xb = lines[a][field], lines[b][field]
    return {"of": a, "over": b, "field": field, "ratio_of_medians": round(statistics.median(xa) / statistics.median(xb), 3),
            "separated": max(xa) < min(xb) or max(xb) < min(xa)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tiles_specialised_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", type=int, default=600)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    rt = importlib.import_module("raytracing-1w_amd")
    hip = C.CDLL("libamdhip64.so")
    W = H = a.size
    d_out = C.c_void_p()
    assert hip.hipMalloc(C.byref(d_out), C.c_size_t(((W + 63) // 64 * 64) * ((H + 63) // 64 * 64) * 3 * 8)) == 0
    lines, comparisons = {}, []
    for scene, arm in SCENES:
        sc = rt.Scene.reference(arm, build_seed=1)
        ctx = rt.Context(sc, 0)
        for spp in (16, 256):
            chunk = sc.default_chunk(W, H, spp)
            group = {f"{scene} {W}x{H} {spp} spp rectangle (rt1w_render_device)":
                     lambda spp=spp, chunk=chunk: ctx.render_device(d_out.value, W, H, spp, out_sum=True, chunk=chunk)}
            for T in (16, 64):
                every = [(x0, y0, 0) for y0 in range(0, H, T) for x0 in range(0, W, T)]
                for flag in (False, True):
                    group[f"{scene} {W}x{H} {spp} spp tiles T={T} {'specialised' if flag else 'generic'}"] = \
                        lambda spp=spp, chunk=chunk, T=T, every=every, flag=flag: ctx.render_tiles_device(d_out.value, W, H, spp, T, every, out_sum=True,
                                                                                                        chunk=chunk, specialised=flag)
            got = alternate(group, a.reps)
            lines.update(got)
            names = list(group)
            for T, (g, s) in ((16, names[1:3]), (64, names[3:5])):
                assert got[s]["sorted"] & 4 and not (got[g]["sorted"] & 4), (g, s, got[g]["sorted"], got[s]["sorted"])
                comparisons.append(compare(lines, g, s, "kernel_ms"))      # > 1: the specialised tile form is faster by that factor
                comparisons.append(compare(lines, g, s, "total_ms"))
                comparisons.append(compare(lines, s, names[0], "kernel_ms"))  # the tile form over the rectangle kernel
        for budget in (16, 128):
            group = {}
            for flag in (False, True):
                group[f"{scene} {W}x{H} rt1w_render_adaptive_filtered budget {budget} {'specialised' if flag else 'generic'} rounds"] = \
                    lambda budget=budget, flag=flag: ctx.render_adaptive_filtered(W, H, adaptive=dict(budget_spp=budget), with_stats=True,
                                                                                   flags=rt.TILES_SPECIALISED if flag else 0)[3]
            got = alternate(group, a.reps)
            lines.update(got)
            g, s = list(group)
            comparisons.append(compare(lines, g, s, "kernel_ms"))
            comparisons.append(compare(lines, g, s, "total_ms"))
        ctx.close()
    out = {"what": "RT1W_TILES_SPECIALISED against the generic tile-list kernels (= the parent commit's) and the rectangle kernel; ms",
           "reps": a.reps, "device": rt.device_name(0) if hasattr(rt, "device_name") else None,
           "lines": [dict(name=n, sorted=v["sorted"], kernel_ms=summary(v["kernel_ms"]), total_ms=summary(v["total_ms"]),
                          kernel_ms_all=[round(x, 3) for x in v["kernel_ms"]], total_ms_all=[round(x, 3) for x in v["total_ms"]]) for n, v in lines.items()],
           "comparisons": comparisons}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for ln in out["lines"]:
        print(f"{ln['name']:96s} kernel {ln['kernel_ms']['median']:9.3f} [{ln['kernel_ms']['min']:.3f}, {ln['kernel_ms']['max']:.3f}]  total {ln['total_ms']['median']:9.3f}")
    for c in comparisons:
        print(f"{c['field']:9s} {c['ratio_of_medians']:6.3f} {'separated' if c['separated'] else 'overlapping'}  {c['of']}  /  {c['over']}")


if __name__ == "__main__":
    main()
