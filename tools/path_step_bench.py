#!/usr/bin/env python3
"""Rate of the path states (rt1w_path_step_device, csrc/path_step.hip) in levels per second, against the radiance queries on the same rays.

Workloads: Cornell 600 x 600 x 4 and final_scene 800 x 800 x 4 camera states from rt1w_path_begin_device (samples 0 .. 3 of every pixel,
max_depth 50), as torch tensors [n, 16].  Three forms carry a copy of them to the end:
  (i)   one call with steps = 64;
  (ii)  one call per level over the whole list, until a call traces nothing;
  (iii) one call per level, the dead states dropped by torch (a boolean mask) between calls.
The yardstick is rt1w_ray_color_device on the same rays -- read in place from the states (stride 16), with the states' stream positions
as start words, 1 spp in work items of 1: the render kernels' ray-list form, which reorders paths; the step kernel does not.  Its
streams are keyed first_stream + r rather than by pixel, so its paths are other paths of the same distribution; its segment count
stands beside the step forms'.

A level is a level that traced a ray (rt1w_stats.segments).  Two clocks: `kernel` sums rt1w_stats.kernel_ms of the calls (HIP events
around each launch), `wall` is a host clock from before the first call to a device synchronise behind the last, so it holds the
launches' gaps, the entries' own synchronisation and, in (iii), torch's compaction.  A repetition runs the four in turn after one
warm-up of each; the figure is the median of `--runs` repetitions, the spread their range.  No profiler.  Needs a GPU.

RT1W_LIB selects another build of the library (make path_step_w3: the step kernels at three waves per SIMD); --out says where to write.

usage: python3 tools/path_step_bench.py [--out FILE] [--runs N]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("cornell", 5, 600, 600), ("final_scene", 7, 800, 800)]
SAMPLES, MAX_DEPTH = 4, 50


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "path_step_bench.json"))
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    import torch
    sys.path.insert(0, ROOT)
    rt = importlib.import_module("raytracing-1w_amd")

    rows = []
    for name, arm, W, H in CASES:
        sc = rt.Scene.reference(arm, build_seed=1)
        ctx = rt.Context(sc, 0)
        i, j, s = torch.meshgrid(torch.arange(W, dtype=torch.int32), torch.arange(H, dtype=torch.int32), torch.arange(SAMPLES, dtype=torch.int32), indexing="ij")
        pixels = torch.stack([i, j, s], dim=-1).permute(1, 0, 2, 3).reshape(-1, 3).contiguous().cuda()  # pixel-major, row by row
        n = pixels.shape[0]
        fresh = ctx.path_begin(W, H, pixels, max_depth=MAX_DEPTH, device=True)
        words = (fresh[:, 14].view(torch.int64) >> 32).to(torch.int32).contiguous()  # bytes 116-119 of a state
        d_rgb = torch.zeros((n, 3), dtype=torch.float64, device="cuda")

        def timed(run, copy=True):
            states = fresh.clone() if copy else None  # outside the clock
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            kernel_ms, segments, calls = run(states)
            torch.cuda.synchronize()
            return {"wall_ms": (time.perf_counter() - t0) * 1e3, "kernel_ms": kernel_ms, "segments": segments, "calls": calls}

        def one_call(states):
            st = ctx.path_step(states, 64, device=True)
            return st["kernel_ms"], st["segments"], 1

        def per_level(states, compact):
            kernel_ms, segments, calls = 0.0, 0, 0
            while states.shape[0]:
                st = ctx.path_step(states, 1, device=True)
                kernel_ms, segments, calls = kernel_ms + st["kernel_ms"], segments + st["segments"], calls + 1
                if st["segments"] == 0:
                    break
                if compact:
                    states = states[(states[:, 15].view(torch.int64) >> 32) & 1 == 1]  # status, bit 0: alive
            return kernel_ms, segments, calls

        def yardstick(_):
            st = ctx.ray_color_device(fresh.data_ptr(), d_rgb.data_ptr(), n, words.data_ptr(), stride=16, spp=1, chunk=1, max_depth=MAX_DEPTH, out_sum=True)
            return st["kernel_ms"], st["segments"], 1
        forms = [("one_call_64", lambda: timed(one_call)), ("per_level", lambda: timed(lambda s: per_level(s, False))),
                 ("per_level_compacted", lambda: timed(lambda s: per_level(s, True))), ("ray_color", lambda: timed(yardstick, copy=False))]
        for _, f in forms:
            f()  # warm-up of every shape
        runs = {k: [] for k, _ in forms}
        for _ in range(a.runs):
            for k, f in forms:
                runs[k].append(f())
        row = {"case": name, "arm": arm, "frame": [W, H], "samples": SAMPLES, "states": n, "max_depth": MAX_DEPTH, "forms": {}}
        for k, _ in forms:
            r = runs[k]
            rate_k = [x["segments"] / x["kernel_ms"] / 1e3 for x in r]  # M levels / s
            rate_w = [x["segments"] / x["wall_ms"] / 1e3 for x in r]
            row["forms"][k] = {"segments": r[0]["segments"], "calls": r[0]["calls"],
                               "Mlevels_per_s_kernel": statistics.median(rate_k), "kernel_range": [min(rate_k), max(rate_k)],
                               "Mlevels_per_s_wall": statistics.median(rate_w), "wall_range": [min(rate_w), max(rate_w)]}
        y = row["forms"]["ray_color"]
        for k in ("one_call_64", "per_level", "per_level_compacted"):
            row["forms"][k]["of_ray_color_kernel"] = row["forms"][k]["Mlevels_per_s_kernel"] / y["Mlevels_per_s_kernel"]
            row["forms"][k]["of_ray_color_wall"] = row["forms"][k]["Mlevels_per_s_wall"] / y["Mlevels_per_s_wall"]
        print(json.dumps(row), flush=True)
        rows.append(row)
        ctx.close()
    doc = {"tool": "tools/path_step_bench.py", "version": rt.version(), "library": os.path.basename(rt.LIB_PATH), "runs": a.runs,
           "what": "levels that traced a ray per second (millions) of rt1w_path_step_device in three forms and of rt1w_ray_color_device on the same rays; "
                   "kernel: over the summed rt1w_stats.kernel_ms; wall: over a host clock around the form, device synchronised; median and range over the runs",
           "cases": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
