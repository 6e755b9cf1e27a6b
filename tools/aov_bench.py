#!/usr/bin/env python3
"""Rate of the first-hit feature buffers (rt1w_render_aov, csrc/aov.hip) against the beauty render on the same frame.

For C3 (Cornell 600 x 600) and C4 (final_scene 800 x 800) at 16 and 64 AOV samples per pixel, one child process per configuration runs
under `rocprofv3 --kernel-trace --stats` (a run of its own): it renders the AOV buffers (1 warm-up + `--reps`) and, in the same process,
the beauty frame at the same spp (1 warm-up + 1).  The AOV kernel time is the rocprofv3 mean of the rt_aov_kernel calls; primary
segments/s = pixels * spp / that time.  The beauty rate is stats.segments / stats.kernel_ms (HIP events) of the timed render.
Writes one JSON file (default profiles/aov_bench.json).

usage: python3 tools/aov_bench.py [--out FILE] [--reps N] [--lib PATH-TO-librt1w.so] [--label TEXT] [--aov-only]
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


def child(arm, W, H, spp, reps, aov_only):
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
    ctx.close()
    print("AOVJSON " + json.dumps(res), flush=True)


def kernel_stats(d):
    """name -> (calls, mean ns) from rocprofv3's kernel_stats.csv under d"""
    out = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            out[r["Name"]] = (int(r["Calls"]), float(r["AverageNs"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aov_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lib", default=None, help="another build of librt1w.so (RT1W_LIB), e.g. an A/B of the lane mapping")
    ap.add_argument("--label", default="default build")
    ap.add_argument("--aov-only", action="store_true")
    ap.add_argument("--child", nargs=4, type=int, metavar=("ARM", "W", "H", "SPP"))
    a = ap.parse_args()
    if a.child:
        return child(*a.child, a.reps, a.aov_only)
    env = dict(os.environ)
    if a.lib:
        env["RT1W_LIB"] = os.path.abspath(a.lib)
    rows = []
    for name, arm, W, H, spp in CONFIGS:
        d = tempfile.mkdtemp(prefix="aov_bench_")
        cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
               sys.executable, os.path.abspath(__file__), "--child", str(arm), str(W), str(H), str(spp), "--reps", str(a.reps)]
        if a.aov_only:
            cmd.append("--aov-only")
        p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        line = [l for l in p.stdout.splitlines() if l.startswith("AOVJSON ")]
        if p.returncode != 0 or not line:
            sys.stdout.write(p.stdout[-4000:])
            sys.exit(f"{name} {spp} spp: child failed with exit status {p.returncode}")
        res = json.loads(line[-1][len("AOVJSON "):])
        ks = kernel_stats(d)
        shutil.rmtree(d, ignore_errors=True)
        aov = [(k, v) for k, v in ks.items() if "rt_aov_kernel" in k]
        assert len(aov) == 1, sorted(ks)
        kname, (calls, mean_ns) = aov[0]
        assert calls == a.reps + 1, (calls, a.reps)
        row = {"workload": name, "arm": arm, "width": W, "height": H, "aov_spp": spp, "aov_kernel": kname, "aov_calls": calls,
               "aov_kernel_ms_rocprof": mean_ns * 1e-6, "aov_segments_per_s": res["paths"] / (mean_ns * 1e-9),
               "aov_kernel_ms_events": res["aov_event_ms"], "aov_variant": res["aov_variant"],
               "aov_grid": res["aov_grid"], "aov_block": res["aov_block"]}
        if not a.aov_only:
            row.update({"beauty_kernel_ms_events": res["beauty_kernel_ms"], "beauty_segments": res["beauty_segments"],
                        "beauty_segments_per_s": res["beauty_segments_per_s"], "beauty_sorted_bits": res["beauty_sorted"],
                        "aov_over_beauty": row["aov_segments_per_s"] / res["beauty_segments_per_s"]})
        rows.append(row)
        print(json.dumps({k: row[k] for k in row if k not in ("aov_kernel", "aov_kernel_ms_events")}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/aov_bench.py", "label": a.label, "lib": a.lib or "librt1w.so", "reps": a.reps, "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
