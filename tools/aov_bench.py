#!/usr/bin/env python3
"""Rate of the first-hit feature buffers (rt1w_render_aov, csrc/aov.hip) against the beauty render on the same frame.

For C3 (Cornell 600 x 600) and C4 (final_scene 800 x 800) at 16 and 64 AOV samples per pixel, one child process per configuration runs
under `rocprofv3 --kernel-trace --stats` (a run of its own): it renders the AOV buffers (1 warm-up + `--reps`) and, in the same process,
the beauty frame at the same spp (1 warm-up + 1).  The AOV kernel time is the rocprofv3 mean of the rt_aov_kernel calls; primary
segments/s = pixels * spp / that time.  The beauty rate is stats.segments / stats.kernel_ms (HIP events) of the timed render.
Writes one JSON file (default profiles/aov_bench.json).

--deep N adds the deep feature buffers (rt1w_render_aov_deep, max_specular = N, max_fuzz 0) to every configuration: the rocprofv3 mean
of the rt_aov_deep_kernel calls, rays traced / that time, and -- from a second child without the profiler, so that the kernel means
hold the stand-alone calls only -- the whole-call times (median and range of `--reps` calls) of rt1w_render_denoised_deep against
rt1w_render_denoised with the extra cost in beauty samples per pixel.  The intended record is
`--deep 8 --reps 20 --out profiles/aov_deep_bench.json`; that run has not been made yet.

usage: python3 tools/aov_bench.py [--out FILE] [--reps N] [--lib PATH-TO-librt1w.so] [--label TEXT] [--aov-only] [--deep N]
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = [("c3", 5, 600, 600, 16), ("c3", 5, 600, 600, 64), ("c4", 7, 800, 800, 16), ("c4", 7, 800, 800, 64)]


def child(arm, W, H, spp, reps, aov_only, deep=None):
    """the kernels, under the profiler: reps + 1 calls of the first-hit kernel, two beauty renders, reps + 1 calls of the deep kernel"""
    import importlib
    sys.path.insert(0, ROOT)
    rt = importlib.import_module("raytracing-1w_amd")
    sc = rt.Scene.reference(arm, build_seed=1)
    ctx = rt.Context(sc, 0)
    ctx.render_aov(W, H, spp)
    ms = []
    st = None
    for _ in range(reps):
        _, st = ctx.render_aov(W, H, spp, with_stats=True)
        ms.append(st["kernel_ms"])
    res = {"aov_event_ms": ms, "aov_variant": st["variant"], "aov_grid": st["grid"], "aov_block": st["block"], "paths": st["paths"]}
    if not aov_only:
        ctx.render(W, H, spp)
        _, b = ctx.render(W, H, spp)
        res.update({"beauty_kernel_ms": b["kernel_ms"], "beauty_segments": b["segments"], "beauty_sorted": b["sorted"],
                    "beauty_segments_per_s": b["segments"] / (b["kernel_ms"] * 1e-3)})
    if deep is not None:
        ctx.render_aov_deep(W, H, spp, max_specular=deep)
        ms = []
        for _ in range(reps):
            _, st = ctx.render_aov_deep(W, H, spp, max_specular=deep, with_stats=True)
            ms.append(st["kernel_ms"])
        res.update({"deep_event_ms": ms, "deep_segments": st["segments"]})
    ctx.close()
    print("AOVJSON " + json.dumps(res), flush=True)


def child_calls(arm, W, H, spp, reps, deep):
    """the one-call forms, in a process of their own without the profiler (their AOV kernels would otherwise mix into the kernel means):
    whole-call times of rt1w_render_denoised and rt1w_render_denoised_deep, alternating so that a drift of the clocks meets both alike"""
    import importlib
    sys.path.insert(0, ROOT)
    rt = importlib.import_module("raytracing-1w_amd")
    ctx = rt.Context(rt.Scene.reference(arm, build_seed=1), 0)
    ctx.render_denoised(W, H, spp)
    ctx.render_denoised_deep(W, H, spp, max_specular=deep)
    first, dp = [], []
    for _ in range(reps):
        first.append(ctx.render_denoised(W, H, spp, with_stats=True)[1]["total_ms"])
        dp.append(ctx.render_denoised_deep(W, H, spp, max_specular=deep, with_stats=True)[1]["total_ms"])
    ctx.close()
    print("AOVJSON " + json.dumps({"denoised_total_ms": first, "denoised_deep_total_ms": dp}), flush=True)


def kernel_stats(d):
    """name -> (calls, mean ns) from rocprofv3's kernel_stats.csv under d"""
    out = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            out[r["Name"]] = (int(r["Calls"]), float(r["AverageNs"]))
    return out


def make_row(config, res, ks, reps, aov_only=False, deep=None, calls=None):
    """one row of the result file from a child's report `res`, the profiler's kernel statistics `ks` and, with `deep`, the report
    `calls` of the one-call child"""
    name, arm, W, H, spp = config
    aov = [(k, v) for k, v in ks.items() if "rt_aov_kernel" in k]
    assert len(aov) == 1, sorted(ks)
    kname, (n_calls, mean_ns) = aov[0]
    assert n_calls == reps + 1, (n_calls, reps)
    row = {"workload": name, "arm": arm, "width": W, "height": H, "aov_spp": spp, "aov_kernel": kname, "aov_calls": n_calls,
           "aov_kernel_ms_rocprof": mean_ns * 1e-6, "aov_segments_per_s": res["paths"] / (mean_ns * 1e-9),
           "aov_kernel_ms_events": res["aov_event_ms"], "aov_variant": res["aov_variant"],
           "aov_grid": res["aov_grid"], "aov_block": res["aov_block"]}
    if not aov_only:
        row.update({"beauty_kernel_ms_events": res["beauty_kernel_ms"], "beauty_segments": res["beauty_segments"],
                    "beauty_segments_per_s": res["beauty_segments_per_s"], "beauty_sorted_bits": res["beauty_sorted"],
                    "aov_over_beauty": row["aov_segments_per_s"] / res["beauty_segments_per_s"]})
    if deep is not None:
        dk = [(k, v) for k, v in ks.items() if "rt_aov_deep_kernel" in k]
        assert len(dk) == 1 and dk[0][1][0] == reps + 1, sorted(ks)
        mean_ns = dk[0][1][1]
        med = lambda v: sorted(v)[len(v) // 2]
        first, dp = calls["denoised_total_ms"], calls["denoised_deep_total_ms"]
        row.update({"max_specular": deep, "deep_kernel_ms_rocprof": mean_ns * 1e-6, "deep_kernel_ms_events": res["deep_event_ms"],
                    "deep_segments": res["deep_segments"], "deep_segments_per_sample": res["deep_segments"] / res["paths"],
                    "deep_segments_per_s": res["deep_segments"] / (mean_ns * 1e-9),
                    "denoised_total_ms_median": med(first), "denoised_total_ms_range": [min(first), max(first)],
                    "denoised_deep_total_ms_median": med(dp), "denoised_deep_total_ms_range": [min(dp), max(dp)]})
        if not aov_only:
            row["deep_over_beauty"] = row["deep_segments_per_s"] / res["beauty_segments_per_s"]
            row["deep_extra_beauty_samples_per_pixel"] = (med(dp) - med(first)) / (res["beauty_kernel_ms"] / spp)
    return row


def run_child(cmd, env, what):
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    line = [l for l in p.stdout.splitlines() if l.startswith("AOVJSON ")]
    if p.returncode != 0 or not line:
        sys.stdout.write(p.stdout[-4000:])
        sys.exit(f"{what}: child failed with exit status {p.returncode}")
    return json.loads(line[-1][len("AOVJSON "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aov_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lib", default=None, help="another build of librt1w.so (RT1W_LIB), e.g. an A/B of the lane mapping")
    ap.add_argument("--label", default="default build")
    ap.add_argument("--aov-only", action="store_true")
    ap.add_argument("--deep", type=int, default=None, metavar="N", help="also measure rt1w_render_aov_deep with max_specular = N")
    ap.add_argument("--child", nargs=4, type=int, metavar=("ARM", "W", "H", "SPP"))
    ap.add_argument("--child-calls", nargs=4, type=int, metavar=("ARM", "W", "H", "SPP"))
    a = ap.parse_args()
    if a.child:
        return child(*a.child, a.reps, a.aov_only, a.deep)
    if a.child_calls:
        return child_calls(*a.child_calls, a.reps, a.deep)
    env = dict(os.environ)
    if a.lib:
        env["RT1W_LIB"] = os.path.abspath(a.lib)
    rows = []
    for config in CONFIGS:
        name, arm, W, H, spp = config
        d = tempfile.mkdtemp(prefix="aov_bench_")
        me = [sys.executable, os.path.abspath(__file__), "--reps", str(a.reps)] + (["--deep", str(a.deep)] if a.deep is not None else [])
        cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + me + \
              ["--child", str(arm), str(W), str(H), str(spp)] + (["--aov-only"] if a.aov_only else [])
        res = run_child(cmd, env, f"{name} {spp} spp")
        ks = kernel_stats(d)
        shutil.rmtree(d, ignore_errors=True)
        calls = None
        if a.deep is not None:
            calls = run_child(["timeout", "-k", "10", "300"] + me + ["--child-calls", str(arm), str(W), str(H), str(spp)], env,
                              f"{name} {spp} spp, one-call forms")
        row = make_row(config, res, ks, a.reps, a.aov_only, a.deep, calls)
        rows.append(row)
        print(json.dumps({k: row[k] for k in row if k not in ("aov_kernel", "aov_kernel_ms_events", "deep_kernel_ms_events")}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/aov_bench.py", "label": a.label, "lib": a.lib or "librt1w.so", "reps": a.reps, "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
