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

usage: python3 tools/denoise_bench.py [--out FILE] [--reps N] [--lib PATH-TO-librt1w.so] [--label TEXT]
`--lib` measures another build, e.g. the all-direct form (-DRT_DENOISE_LDS_MASK=0) for the per-step A/B of the staged against the direct
level kernel.
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


def level_times(d, warmup, reps):
    """[prepare, level 0, ...] mean ms and kernel names, from the kernel trace under d: the filter's dispatches in start order"""
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if "rt_dn_" in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    per_call = LEVELS + 1
    assert len(rows) == per_call * (warmup + reps), (len(rows), per_call, warmup, reps)
    rows = rows[per_call * warmup:]
    ms, names = [], []
    for k in range(per_call):
        sel = rows[k::per_call]
        assert len({n for _, _, n in sel}) == 1
        ms.append(statistics.mean((e - s) * 1e-6 for s, e, _ in sel))
        names.append(sel[0][2])
    return ms, names


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_bench.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lib", default=None, help="another build of librt1w.so (RT1W_LIB), e.g. the all-direct level kernel")
    ap.add_argument("--label", default="default build")
    ap.add_argument("--only", default=None, help="one of c3, c4, c5")
    ap.add_argument("--child", nargs=5, metavar=("ARM", "W", "H", "SPP", "ASPECT"))
    a = ap.parse_args()
    if a.child:
        return child(int(a.child[0]), int(a.child[1]), int(a.child[2]), int(a.child[3]), float(a.child[4]), a.warmup, a.reps)
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
               "--reps", str(a.reps), "--warmup", str(a.warmup)]
        p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        line = [l for l in p.stdout.splitlines() if l.startswith("DNJSON ")]
        if p.returncode != 0 or not line:
            sys.stdout.write(p.stdout[-4000:])
            sys.exit(f"{name}: child failed with exit status {p.returncode}")
        res = json.loads(line[-1][len("DNJSON "):])
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
