#!/usr/bin/env python3
"""Cost of the feature-guided denoiser (rt1w_denoise_device, csrc/denoise.hip) against the beauty render of the same frame.

For C3 (Cornell 600 x 600), C4 (final_scene 800 x 800) and C5 (Cornell 3840 x 2160), one child process per frame size runs under
`rocprofv3 --kernel-trace --stats` (a run of its own): it renders the frame and its feature buffers on the device, then calls
rt1w_denoise_device with the default 5 levels (`--warmup` + `--reps` calls).  From the kernel trace: the time of the prepare pass and of
every level, by position in the call (mean over the calls after the warm-up).  From the child: the whole-call time (median of the
timed calls) and the beauty kernel time per sample (C3 / C4 through render, C5 through render_rows at a small spp).
Derived: the filter's cost in samples (whole call / beauty time per spp) and the bytes per second of the levels against the bytes the
design must move (one colour read, one guide read and one colour write per pixel and level: 32 + 40 + 32 B; the last level writes 24 B
and reads the guide's albedo).  Writes one JSON file (default profiles/denoise_bench.json).

usage: python3 tools/denoise_bench.py [--out FILE] [--reps N] [--lib PATH-TO-librt1w.so] [--label TEXT] [--variance]
`--lib` measures another build, e.g. the all-direct form (-DRT_DENOISE_LDS_MASK=0) for the per-step A/B of the staged against the direct
level kernel.
`--variance` measures the variance-guided filter (rt1w_denoise_var_device, csrc/denoise_var.hip) against the fixed-sigma one: in the same
process and on the same frames the child renders 4 sample batches, takes their frame and variance (rt1w_batch_variance_device) and calls
the two filters in turn; the rows then hold every level's time for both, their ratio per step, the batch-variance pass, and the whole
call rt1w_render_denoised_var against the beauty render of the same samples, in beauty samples per pixel.  Default output
profiles/denoise_var_bench.json.
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
CONFIGS = [("c3", 5, 600, 600, 16, 1.0), ("c4", 7, 800, 800, 16, 1.0), ("c5", 5, 3840, 2160, 4, 16.0 / 9.0)]
LEVELS = 5
BATCHES = 4      # --variance: the default of rt1w_render_denoised_var
WHOLE_CALLS = 5  # --variance: timed calls of rt1w_render_denoised_var and of the beauty render


def child_variance(arm, W, H, spp, aspect, warmup, reps):
    """both filters in turn on one frame; spp is a multiple of BATCHES"""
    import importlib
    import torch
    sys.path.insert(0, ROOT)
    rt = importlib.import_module("raytracing-1w_amd")
    ctx = rt.Context(rt.Scene.reference(arm, build_seed=1, aspect_ratio=aspect), 0)
    n = spp // BATCHES
    f64 = dict(dtype=torch.float64, device="cuda")
    sums, aov = torch.empty((BATCHES, H, W, 3), **f64), torch.empty((H, W, 8), **f64)
    frame, var, out = torch.empty((H, W, 3), **f64), torch.empty((H, W), **f64), torch.empty((H, W, 3), **f64)
    for k in range(BATCHES):
        ctx.render_device(sums[k].data_ptr(), W, H, n, sample_offset=k * n, out_sum=True)
    ctx.render_aov_device(aov.data_ptr(), W, H, spp)
    torch.cuda.synchronize()
    res = {"fixed_total_ms": [], "var_total_ms": [], "variance_pass_ms": [], "call_total_ms": [], "call_kernel_ms": [], "beauty_total_ms": [],
           "beauty_kernel_ms": []}
    for i in range(warmup + reps):
        sv = ctx.batch_variance_device(sums.data_ptr(), aov.data_ptr(), frame.data_ptr(), var.data_ptr(), W, H, BATCHES, n)
        s0 = ctx.denoise_device(frame.data_ptr(), aov.data_ptr(), out.data_ptr(), W, H)
        s1 = ctx.denoise_var_device(frame.data_ptr(), aov.data_ptr(), var.data_ptr(), out.data_ptr(), W, H)
        if i >= warmup:
            res["variance_pass_ms"].append(sv["kernel_ms"])
            res["fixed_total_ms"].append(s0["total_ms"])
            res["var_total_ms"].append(s1["total_ms"])
    finite = bool(torch.isfinite(out).all().item())
    for i in range(2 + WHOLE_CALLS):  # whole calls, alternating so that a drift of the clocks meets both alike
        _, sb = ctx.render(W, H, spp)
        _, sc = ctx.render_denoised_var(W, H, spp, batches=BATCHES, with_stats=True)
        if i >= 2:
            res["beauty_total_ms"].append(sb["total_ms"]); res["beauty_kernel_ms"].append(sb["kernel_ms"])
            res["call_total_ms"].append(sc["total_ms"]); res["call_kernel_ms"].append(sc["kernel_ms"])
    ctx.close()
    print("DNJSON " + json.dumps(dict(res, grid=s1["grid"], block=s1["block"], finite=finite, spp=spp, batches=BATCHES)), flush=True)


def child(arm, W, H, spp, aspect, warmup, reps):
    import importlib
    import torch
    sys.path.insert(0, ROOT)
    rt = importlib.import_module("raytracing-1w_amd")
    sc = rt.Scene.reference(arm, build_seed=1, aspect_ratio=aspect)
    ctx = rt.Context(sc, 0)
    if W * H > 1000000:  # the big frame strip-wise, as a host would
        ctx.render_rows(W, H, spp)
        _, b = ctx.render_rows(W, H, spp)
    else:
        ctx.render(W, H, spp)
        _, b = ctx.render(W, H, spp)
    frame = torch.empty((H, W, 3), dtype=torch.float64, device="cuda")
    aov = torch.empty((H, W, 8), dtype=torch.float64, device="cuda")
    out = torch.empty_like(frame)
    ctx.render_device(frame.data_ptr(), W, H, spp)
    ctx.render_aov_device(aov.data_ptr(), W, H, spp)
    torch.cuda.synchronize()
    total, kern, st = [], [], None
    for i in range(warmup + reps):
        st = ctx.denoise_device(frame.data_ptr(), aov.data_ptr(), out.data_ptr(), W, H)
        if i >= warmup:
            total.append(st["total_ms"])
            kern.append(st["kernel_ms"])
    finite = bool(torch.isfinite(out).all().item())
    ctx.close()
    print("DNJSON " + json.dumps({"total_ms": total, "kernel_ms_events": kern, "grid": st["grid"], "block": st["block"], "finite": finite,
                                  "beauty_kernel_ms": b["kernel_ms"], "beauty_spp": spp, "beauty_paths": b["paths"]}), flush=True)


def level_times(d, warmup, reps, prefixes=("rt_dn_",), extra_calls=0):
    """[prepare, level 0, ...] mean ms and kernel names, from the kernel trace under d: the dispatches of the filter whose kernels' names
    hold one of `prefixes`, in start order; the `extra_calls` calls after the timed ones are left out"""
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if any(p in r["Kernel_Name"] for p in prefixes):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    per_call = LEVELS + 1
    assert len(rows) == per_call * (warmup + reps + extra_calls), (len(rows), per_call, warmup, reps, extra_calls)
    rows = rows[:per_call * (warmup + reps)]
    rows = rows[per_call * warmup:]
    ms, names = [], []
    for k in range(per_call):
        sel = rows[k::per_call]
        assert len({n for _, _, n in sel}) == 1
        ms.append(statistics.mean((e - s) * 1e-6 for s, e, _ in sel))
        names.append(sel[0][2])
    return ms, names


def variance_row(name, arm, W, H, res, d, warmup, reps):
    """one row of profiles/denoise_var_bench.json from the child's answer and the kernel trace under d"""
    fixed, fixed_names = level_times(d, warmup, reps)
    var, var_names = level_times(d, warmup, reps, ("rt_dv_prepare_kernel", "rt_dv_level_kernel"), extra_calls=2 + WHOLE_CALLS)
    med = statistics.median
    beauty_per_spp = med(res["beauty_kernel_ms"]) / res["spp"]
    return {"workload": name, "arm": arm, "width": W, "height": H, "levels": LEVELS, "spp": res["spp"], "batches": res["batches"],
            "grid": res["grid"], "block": res["block"], "output_finite": res["finite"],
            "fixed_prepare_ms": fixed[0], "fixed_level_ms": fixed[1:], "fixed_level_kernels": fixed_names[1:],
            "var_prepare_ms": var[0], "var_level_ms": var[1:], "var_level_kernels": var_names[1:],
            "level_ratio_var_over_fixed": [v / f for v, f in zip(var[1:], fixed[1:])],
            "levels_ratio_var_over_fixed": sum(var[1:]) / sum(fixed[1:]),
            "bytes_per_tap_ratio_expected": (40 + 40) / (32 + 40),
            "variance_pass_ms_median": med(res["variance_pass_ms"]),
            "fixed_call_ms_median": med(res["fixed_total_ms"]), "var_call_ms_median": med(res["var_total_ms"]), "calls": len(res["var_total_ms"]),
            "beauty_call_ms_median": med(res["beauty_total_ms"]), "beauty_kernel_ms_median": med(res["beauty_kernel_ms"]),
            "render_denoised_var_call_ms_median": med(res["call_total_ms"]), "render_denoised_var_kernel_ms_median": med(res["call_kernel_ms"]),
            "whole_calls": len(res["call_total_ms"]), "beauty_ms_per_spp": beauty_per_spp,
            "filter_cost_in_samples": (med(res["variance_pass_ms"]) + med(res["var_total_ms"])) / beauty_per_spp,
            "whole_call_extra_cost_in_samples": (med(res["call_total_ms"]) - med(res["beauty_total_ms"])) / beauty_per_spp}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default profiles/denoise_bench.json, with --variance profiles/denoise_var_bench.json")
    ap.add_argument("--variance", action="store_true", help="the variance-guided filter against the fixed-sigma one, on the same frames")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lib", default=None, help="another build of librt1w.so (RT1W_LIB), e.g. the all-direct level kernel")
    ap.add_argument("--label", default="default build")
    ap.add_argument("--only", default=None, help="one of c3, c4, c5")
    ap.add_argument("--child", nargs=5, metavar=("ARM", "W", "H", "SPP", "ASPECT"))
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "denoise_var_bench.json" if a.variance else "denoise_bench.json")
    if a.child:
        return (child_variance if a.variance else child)(int(a.child[0]), int(a.child[1]), int(a.child[2]), int(a.child[3]), float(a.child[4]), a.warmup, a.reps)
    env = dict(os.environ)
    if a.lib:
        env["RT1W_LIB"] = os.path.abspath(a.lib)
    rows = []
    for name, arm, W, H, spp, aspect in CONFIGS:
        if a.only and a.only != name:
            continue
        d = tempfile.mkdtemp(prefix="denoise_bench_")
        cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
               sys.executable, os.path.abspath(__file__), "--child", str(arm), str(W), str(H), str(spp), repr(aspect),
               "--reps", str(a.reps), "--warmup", str(a.warmup)] + (["--variance"] if a.variance else [])
        p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        line = [l for l in p.stdout.splitlines() if l.startswith("DNJSON ")]
        if p.returncode != 0 or not line:
            sys.stdout.write(p.stdout[-4000:])
            sys.exit(f"{name}: child failed with exit status {p.returncode}")
        res = json.loads(line[-1][len("DNJSON "):])
        if a.variance:
            rows.append(variance_row(name, arm, W, H, res, d, a.warmup, a.reps))
            shutil.rmtree(d, ignore_errors=True)
            print(json.dumps({k: v for k, v in rows[-1].items() if not k.endswith("_kernels")}), flush=True)
            continue
        ms, names = level_times(d, a.warmup, a.reps)
        shutil.rmtree(d, ignore_errors=True)
        npix = W * H
        call_ms = statistics.median(res["total_ms"])
        beauty_per_spp = res["beauty_kernel_ms"] / res["beauty_spp"]
        level_bytes = [npix * (32 + 40 + (24 + 24 if k == LEVELS - 1 else 32)) for k in range(LEVELS)]
        row = {"workload": name, "arm": arm, "width": W, "height": H, "levels": LEVELS, "grid": res["grid"], "block": res["block"],
               "output_finite": res["finite"],
               "prepare_ms": ms[0], "level_ms": ms[1:], "level_kernels": names[1:], "kernels_ms_sum": sum(ms),
               "kernel_ms_events_median": statistics.median(res["kernel_ms_events"]),
               "call_ms_median": call_ms, "calls": len(res["total_ms"]),
               "beauty_kernel_ms": res["beauty_kernel_ms"], "beauty_spp": res["beauty_spp"], "beauty_ms_per_spp": beauty_per_spp,
               "cost_in_samples": call_ms / beauty_per_spp,
               "level_gb_per_s": [b / (t * 1e-3) * 1e-9 for b, t in zip(level_bytes, ms[1:])],
               "level_ns_per_pixel": [t * 1e6 / npix for t in ms[1:]]}
        rows.append(row)
        print(json.dumps({k: row[k] for k in row if k != "level_kernels"}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/denoise_bench.py", "label": a.label, "lib": a.lib or "librt1w.so", "reps": a.reps, "warmup": a.warmup,
                   "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
