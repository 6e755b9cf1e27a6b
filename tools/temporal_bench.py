#!/usr/bin/env python3
"""Cost of temporal accumulation (rt1w_temporal_accumulate_device, csrc/temporal.hip), of its form with second moments and the variance
pass (rt1w_temporal_moments_device, rt1w_temporal_variance_device, csrc/temporal_var.hip) and of a frame of an animation through
rt1w_render_temporal and rt1w_render_temporal_var.

For C3 (Cornell 600 x 600), C4 (final_scene 800 x 800) and C5 (Cornell 3840 x 2160), one child process per case runs under
`rocprofv3 --kernel-trace --stats` (a run of its own, no counters): it renders two frames 2 degrees apart and their feature buffers on the
device, accumulates the first as a first frame, then calls rt1w_temporal_accumulate_device of the second against it (`--warmup` +
`--reps` calls) and, in the same process and on the same frame, rt1w_denoise_var_device with one level, whose prepare pass
(rt_dv_prepare_kernel) is the closest existing one-lane-per-pixel kernel.  From the kernel trace: the mean time of the two kernels over
the calls after the warm-up.  From the child: whole calls of rt1w_render_temporal (with the filter, the camera turned before every call)
against rt1w_render_denoised at the same spp, alternating (median of the timed calls).
The same loop calls rt1w_temporal_moments_device on the accumulate call's inputs (256 B per pixel against 240: prev_m2 in, m2 out) and
rt1w_temporal_variance_device twice: on the first frame's state, where every length is 1 and every lane walks the 7 x 7 window, and on a
later frame's -- the second frame accumulated against first-frame lengths scaled to 4, so that a pixel with history has length 5 and only
the disoccluded ones enter the window loop.  A pixel of the variance pass reads hist, m2, len and guides and writes var (24 + 8 + 8 + 64 +
8 = 112 B), the window's taps coming from the neighbours' lines.  The same process runs rt1w_denoise_var_device with the default five
levels on the frame: the sum of its five level kernels is what the first-frame variance kernel is held against.  The whole calls add
rt1w_render_temporal_var and rt1w_render_denoised_var with 4 batches at the same spp: one render launch against four.
Derived: the ratio to the prepare kernel, and the bytes per second of the accumulation against the bytes the design must move per pixel --
the current frame and guides (24 + 64 B), every previous pixel's history, length and guides once (24 + 8 + 64 B), the three outputs
(24 + 8 + 24 B): 240 B; the prepare kernel moves 24 + 64 + 8 in and 40 + 64 out: 200 B.  Writes one JSON file (default
profiles/temporal_bench.json).

usage: python3 tools/temporal_bench.py [--case c3] [--case c4] [--case c5] [--reps N] [--warmup N] [--out FILE]
"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {"c3": (5, 600, 600, 16, 1.0), "c4": (7, 800, 800, 16, 1.0), "c5": (5, 3840, 2160, 4, 16.0 / 9.0)}
WHOLE_CALLS = 5
BYTES_ACCUMULATE, BYTES_PREPARE, BYTES_MOMENTS, BYTES_VARIANCE = 240, 200, 256, 112


def child(arm, W, H, spp, aspect, warmup, reps):
    import importlib
    import torch
    sys.path.insert(0, ROOT)
    rt = importlib.import_module("raytracing-1w_amd")
    ctx = rt.Context(rt.Scene.reference(arm, build_seed=1, aspect_ratio=aspect), 0)
    args = rt.reference_camera(arm, aspect_ratio=aspect)
    f64 = dict(dtype=torch.float64, device="cuda")
    frames, aovs, cams = [], [], []
    for k in range(2):
        ctx.set_camera(**rt.orbit_camera(args, 2.0 * k))
        frames.append(torch.empty((H, W, 3), **f64)); aovs.append(torch.empty((H, W, 8), **f64)); cams.append(ctx.get_camera())
        ctx.render_device(frames[k].data_ptr(), W, H, spp, global_seed=k)
        ctx.render_aov_device(aovs[k].data_ptr(), W, H, spp, global_seed=k)
    hist = [torch.zeros((H, W, 3), **f64), torch.empty((H, W, 3), **f64)]
    ln = [torch.zeros((H, W), **f64), torch.empty((H, W), **f64)]
    out, var = torch.empty((H, W, 3), **f64), torch.zeros((H, W), **f64)
    m2 = [torch.zeros((H, W), **f64), torch.empty((H, W), **f64)]
    mhist, mlen, mout, tvar = torch.empty((H, W, 3), **f64), torch.empty((H, W), **f64), torch.empty((H, W, 3), **f64), torch.empty((H, W), **f64)
    torch.cuda.synchronize()
    acc = lambda cur, prev, k: ctx.temporal_accumulate_device(frames[cur].data_ptr(), aovs[cur].data_ptr(), cams[cur], hist[1 - k].data_ptr(), ln[1 - k].data_ptr(),
                                                              aovs[prev].data_ptr(), cams[prev], hist[k].data_ptr(), ln[k].data_ptr(), out.data_ptr(), W, H)
    acc(0, 0, 1)                      # the first frame: hist[1], ln[1]
    # the same first frame with its second moment (m2[1]; hist and len are the same bits), then the second frame against lengths scaled to 4
    ctx.temporal_moments_device(frames[0].data_ptr(), aovs[0].data_ptr(), cams[0], hist[0].data_ptr(), m2[0].data_ptr(), ln[0].data_ptr(), aovs[0].data_ptr(),
                                cams[0], mhist.data_ptr(), m2[1].data_ptr(), mlen.data_ptr(), mout.data_ptr(), W, H)
    long_len = ln[1] * 4.0
    mom = lambda: ctx.temporal_moments_device(frames[1].data_ptr(), aovs[1].data_ptr(), cams[1], hist[1].data_ptr(), m2[1].data_ptr(), long_len.data_ptr(),
                                              aovs[0].data_ptr(), cams[0], mhist.data_ptr(), m2[0].data_ptr(), mlen.data_ptr(), mout.data_ptr(), W, H)
    res = {"accumulate_total_ms": [], "accumulate_event_ms": [], "temporal_call_ms": [], "temporal_kernel_ms": [], "denoised_call_ms": [],
           "denoised_kernel_ms": [], "moments_event_ms": [], "temporal_var_call_ms": [], "temporal_var_kernel_ms": [], "denoised_var_call_ms": [],
           "denoised_var_kernel_ms": []}
    for i in range(warmup + reps):
        st = acc(1, 0, 0)
        ctx.denoise_var_device(frames[1].data_ptr(), aovs[1].data_ptr(), var.data_ptr(), out.data_ptr(), W, H, iterations=1)
        sm = mom()
        ctx.temporal_variance_device(hist[1].data_ptr(), m2[1].data_ptr(), ln[1].data_ptr(), aovs[0].data_ptr(), tvar.data_ptr(), W, H)    # a first frame
        ctx.temporal_variance_device(mhist.data_ptr(), m2[0].data_ptr(), mlen.data_ptr(), aovs[1].data_ptr(), tvar.data_ptr(), W, H)       # a later frame
        ctx.denoise_var_device(mout.data_ptr(), aovs[1].data_ptr(), tvar.data_ptr(), out.data_ptr(), W, H)
        if i >= warmup:
            res["accumulate_total_ms"].append(st["total_ms"]); res["accumulate_event_ms"].append(st["kernel_ms"])
            res["moments_event_ms"].append(sm["kernel_ms"])
    share = float((ln[0] > 1).double().mean().item())
    share_spatial = float((mlen < 4).double().mean().item())
    finite = bool(torch.isfinite(hist[0]).all().item())
    for i in range(2 + WHOLE_CALLS):  # whole calls, alternating so that a drift of the clocks meets both alike
        ctx.set_camera(**rt.orbit_camera(args, 2.0 * i))
        _, sd = ctx.render_denoised(W, H, spp, global_seed=i, with_stats=True)
        _, stt = ctx.render_temporal(W, H, spp, global_seed=i, filter=True, with_stats=True)
        _, sv = ctx.render_temporal_var(W, H, spp, global_seed=i, with_stats=True)
        _, sb = ctx.render_denoised_var(W, H, spp, batches=4, global_seed=i, with_stats=True)
        if i >= 2:
            res["temporal_var_call_ms"].append(sv["total_ms"]); res["temporal_var_kernel_ms"].append(sv["kernel_ms"])
            res["denoised_var_call_ms"].append(sb["total_ms"]); res["denoised_var_kernel_ms"].append(sb["kernel_ms"])
            res["denoised_call_ms"].append(sd["total_ms"]); res["denoised_kernel_ms"].append(sd["kernel_ms"])
            res["temporal_call_ms"].append(stt["total_ms"]); res["temporal_kernel_ms"].append(stt["kernel_ms"])
    ctx.close()
    print("TMJSON " + json.dumps(dict(res, grid=st["grid"], block=st["block"], finite=finite, share_with_history=share, share_spatial_later=share_spatial, spp=spp)), flush=True)


def kernel_ms(d, name, skip, take, stride=1, phase=0):
    """mean ms of dispatches skip .. skip + take - 1 (in start order; of every `stride`-th one from `phase` on, if given) of the kernel whose
    name holds `name`, from the kernel trace under d"""
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if name in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    rows = sorted(rows)[phase::stride]
    assert len(rows) >= skip + take, (name, len(rows), skip, take)
    return statistics.mean((e - s) * 1e-6 for s, e in rows[skip:skip + take])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_bench.json"))
    ap.add_argument("--case", action="append", choices=sorted(CONFIGS), help="default: all three")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--child", nargs=5, metavar=("ARM", "W", "H", "SPP", "ASPECT"))
    a = ap.parse_args()
    if a.child:
        return child(int(a.child[0]), int(a.child[1]), int(a.child[2]), int(a.child[3]), float(a.child[4]), a.warmup, a.reps)
    rows = []
    for name in a.case or sorted(CONFIGS):
        arm, W, H, spp, aspect = CONFIGS[name]
        d = tempfile.mkdtemp(prefix="temporal_bench_")
        cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
               sys.executable, os.path.abspath(__file__), "--child", str(arm), str(W), str(H), str(spp), repr(aspect),
               "--reps", str(a.reps), "--warmup", str(a.warmup)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        line = [l for l in p.stdout.splitlines() if l.startswith("TMJSON ")]
        if p.returncode != 0 or not line:
            sys.stdout.write(p.stdout[-4000:])
            sys.exit(f"{name}: child failed with exit status {p.returncode}")
        res = json.loads(line[-1][len("TMJSON "):])
        acc = kernel_ms(d, "rt_tm_accumulate_kernel", 1 + a.warmup, a.reps)   # after the first frame's launch and the warm-up
        prep = kernel_ms(d, "rt_dv_prepare_kernel", 2 * a.warmup, 2 * a.reps)             # two filter calls per iteration
        mom = kernel_ms(d, "rt_tv_moments_kernel", 1 + a.warmup, a.reps)
        var_first = kernel_ms(d, "rt_tv_variance_kernel", a.warmup, a.reps, 2, 0)
        var_later = kernel_ms(d, "rt_tv_variance_kernel", a.warmup, a.reps, 2, 1)
        levels = sum(kernel_ms(d, "rt_dv_level_kernel", a.warmup, a.reps, 6, ph) for ph in range(1, 6))   # per iteration: the one-level call's, then the default filter's five
        shutil.rmtree(d, ignore_errors=True)
        npix = W * H
        med = statistics.median
        row = {"workload": name, "arm": arm, "width": W, "height": H, "spp": res["spp"], "grid": res["grid"], "block": res["block"],
               "output_finite": res["finite"], "share_with_history": res["share_with_history"],
               "accumulate_kernel_ms": acc, "prepare_kernel_ms": prep, "accumulate_over_prepare": acc / prep,
               "accumulate_ns_per_pixel": acc * 1e6 / npix, "accumulate_bytes_per_pixel": BYTES_ACCUMULATE, "prepare_bytes_per_pixel": BYTES_PREPARE,
               "accumulate_gb_per_s": npix * BYTES_ACCUMULATE / (acc * 1e-3) * 1e-9, "prepare_gb_per_s": npix * BYTES_PREPARE / (prep * 1e-3) * 1e-9,
               "accumulate_event_ms_median": med(res["accumulate_event_ms"]), "accumulate_call_ms_median": med(res["accumulate_total_ms"]),
               "calls": len(res["accumulate_total_ms"]),
               "render_temporal_call_ms_median": med(res["temporal_call_ms"]), "render_temporal_kernel_ms_median": med(res["temporal_kernel_ms"]),
               "render_denoised_call_ms_median": med(res["denoised_call_ms"]), "render_denoised_kernel_ms_median": med(res["denoised_kernel_ms"]),
               "whole_calls": len(res["temporal_call_ms"]),
               "moments_kernel_ms": mom, "moments_over_accumulate": mom / acc, "moments_bytes_per_pixel": BYTES_MOMENTS,
               "moments_gb_per_s": npix * BYTES_MOMENTS / (mom * 1e-3) * 1e-9, "moments_event_ms_median": med(res["moments_event_ms"]),
               "variance_first_frame_kernel_ms": var_first, "variance_later_frame_kernel_ms": var_later, "variance_later_share_spatial": res["share_spatial_later"],
               "variance_first_over_prepare": var_first / prep, "variance_later_over_prepare": var_later / prep, "variance_bytes_per_pixel": BYTES_VARIANCE,
               "variance_first_gb_per_s": npix * BYTES_VARIANCE / (var_first * 1e-3) * 1e-9,
               "variance_later_gb_per_s": npix * BYTES_VARIANCE / (var_later * 1e-3) * 1e-9,
               "denoise_var_five_levels_kernel_ms": levels, "variance_first_over_five_levels": var_first / levels,
               "render_temporal_var_call_ms_median": med(res["temporal_var_call_ms"]), "render_temporal_var_kernel_ms_median": med(res["temporal_var_kernel_ms"]),
               "render_denoised_var_call_ms_median": med(res["denoised_var_call_ms"]), "render_denoised_var_kernel_ms_median": med(res["denoised_var_kernel_ms"]),
               "render_temporal_var_over_render_temporal": med(res["temporal_var_call_ms"]) / med(res["temporal_call_ms"]),
               "render_temporal_var_over_render_denoised_var": med(res["temporal_var_call_ms"]) / med(res["denoised_var_call_ms"]),
               "render_temporal_over_render_denoised": med(res["temporal_call_ms"]) / med(res["denoised_call_ms"])}
        rows.append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/temporal_bench.py", "reps": a.reps, "warmup": a.warmup, "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
