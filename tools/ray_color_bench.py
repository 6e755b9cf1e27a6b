#!/usr/bin/env python3
"""Rate of the radiance queries (rt1w_ray_color_device, csrc/context_rays.hip: the render kernels' ray-list form) against the render
kernels themselves.

Cases: Cornell 600 x 600 and final_scene 800 x 800, each with the camera rays of the frame (one per pixel, with the stream positions
behind the camera's draws: rt1w_lab_camera_rays_pos_host) and with the bounce-2 rays of the same paths (rt1w_lab_dump_rays: incoherent),
16 samples per ray.  Beside each figure stands rt1w_render_device with RT1W_GENERIC on the same frame at the same spp and chunk -- the same
kernels with the camera in the ray record's place and the 8 x 8 pixel blocks in the list order's -- from the same process, the two calls
alternating.  The ratio of the two on the camera rays is what fetching 56-byte ray records and losing the pixel blocking cost.

Times are the entries' own rt1w_stats.kernel_ms (HIP events around the launches of the call, resolve included); a repetition is `--reps`
calls of each after one warm-up call of each, the figure the median of `--runs` repetitions, the spread their range.  No profiler.  Needs a
GPU: without one the context cannot be made and the tool fails.

usage: python3 tools/ray_color_bench.py [--out FILE] [--reps N] [--runs N]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("c3", 5, 600, 600), ("c4", 7, 800, 800)]
SPP = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ray_color_bench.json"))
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    import numpy as np
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    rt = importlib.import_module("raytracing-1w_amd")
    import walk_lab as wl
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]

    def to_device(x):
        x = np.ascontiguousarray(x)
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), max(x.nbytes, 16)) == 0 and hip.hipMemcpy(p, x.ctypes.data, x.nbytes, 1) == 0
        return p.value

    rows = []
    for name, arm, W, H in CASES:
        sc = rt.Scene.reference(arm, build_seed=1)
        ctx = rt.Context(sc, 0)
        chunk = sc.default_chunk(W, H, SPP)
        cam, word = rt.camera_rays_pos_host(sc, W, H, 1)
        lab = wl.Lab(ctx)
        b2 = lab.dump_rays(W, H, 1, 3)[2]
        lab.close()
        b2 = b2[b2[:, 7] != 0.0]
        d_img = to_device(np.zeros((H, W, 3)))
        for kind, rays, words in (("camera", cam.reshape(-1, 8), word.reshape(-1)), ("bounce 2", b2, None)):
            n = len(rays)
            d_rays, d_out = to_device(rays), to_device(np.zeros((n, 3)))
            d_word = None if words is None else to_device(words)

            def query():
                return ctx.ray_color_device(d_rays, d_out, n, d_word, stride=8, spp=SPP, chunk=chunk)

            def render():
                return ctx.render_device(d_img, W, H, SPP, chunk=chunk, generic=True)
            q_rate, r_rate, ratio, st, rs = [], [], [], None, None
            for _ in range(a.runs):
                query(), render()
                q_ms = r_ms = 0.0
                for _ in range(a.reps):
                    st, rs = query(), render()
                    q_ms += st["kernel_ms"]
                    r_ms += rs["kernel_ms"]
                q_rate.append(a.reps * st["paths"] / q_ms / 1e3)  # M ray samples / s
                r_rate.append(a.reps * rs["paths"] / r_ms / 1e3)
                ratio.append(q_rate[-1] / r_rate[-1])
            row = {"case": f"{name} {kind}", "arm": arm, "frame": [W, H], "rays": n, "spp": SPP, "chunk": st["chunk"], "sorted": st["sorted"],
                   "variant": st["variant"], "grid": st["grid"], "segments_per_ray_sample": st["segments"] / st["paths"],
                   "render_segments_per_path": rs["segments"] / rs["paths"],
                   "ray_color_Msamples_per_s": statistics.median(q_rate), "ray_color_range": [min(q_rate), max(q_rate)],
                   "render_generic_Mpaths_per_s": statistics.median(r_rate), "render_generic_range": [min(r_rate), max(r_rate)],
                   "ratio": statistics.median(ratio), "ratio_range": [min(ratio), max(ratio)]}
            print(json.dumps(row), flush=True)
            rows.append(row)
            for p in (d_rays, d_out, d_word):
                if p:
                    hip.hipFree(p)
        hip.hipFree(d_img)
        ctx.close()
    doc = {"tool": "tools/ray_color_bench.py", "version": rt.version(), "reps": a.reps, "runs": a.runs,
           "what": "rt1w_ray_color_device against rt1w_render_device with RT1W_GENERIC on the same frame, spp and chunk; rates from rt1w_stats.kernel_ms, "
                   "median and range over the runs; ratio = ray_color / render in samples per second",
           "cases": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
