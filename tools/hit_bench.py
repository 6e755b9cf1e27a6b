#!/usr/bin/env python3
"""Rate of the ray queries (rt1w_hit_device, csrc/hit.hip) in both forms of its ray I/O, against the first-hit AOV kernel.

Cases: Cornell 600 x 600 and final_scene 800 x 800, each with the camera rays of the frame at 4 spp and with the bounce-2 rays of the same
paths (rt1w_lab_dump_rays: incoherent).  A preparation child (default library, no profiler) writes each case's rays to a file.  Then every
column -- one case in one form -- is a process of its own under `rocprofv3 --kernel-trace --stats` (a run of its own, no counters): it
uploads the rays once and calls rt1w_hit_device 1 + `--reps` times; on the camera-ray cases it also calls rt1w_render_aov 1 + `--reps`
times on the same frame, the yardstick: the same walk and record without ray I/O.  The kernel times are the profiler's means.  The whole
set of columns is run `--runs` times; the spread of a form is the range of its geometric mean over the four cases across those runs.

The direct form is the default build's; the staged form is `make -C raytracing-1w_amd/csrc hit_staged` (librt1w_hit_staged.so), chosen
through RT1W_LIB.  Rule for the default, set before measuring: the form with the better geometric mean over the four cases; if the two
differ by less than the run-to-run spread, the direct form stays.

usage: python3 tools/hit_bench.py [--out FILE] [--reps N] [--runs N] [--staged PATH-TO-librt1w_hit_staged.so]
"""
import argparse
import csv
import ctypes as C
import glob
import json
import math
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("c3 camera", 5, 600, 600, "camera"), ("c3 bounce 2", 5, 600, 600, "bounce"),
         ("c4 camera", 7, 800, 800, "camera"), ("c4 bounce 2", 7, 800, 800, "bounce")]
SPP = 4
BYTES_PER_RAY = 72 + 96  # in and out; the node indices (4 bytes more) are not asked for
COPY_RATE = 6.29e12      # bytes/s, the copy rate of DESIGN.md section 20


def _rt():
    import importlib
    sys.path.insert(0, ROOT)
    return importlib.import_module("raytracing-1w_amd")


def prepare(directory):
    """the four ray files, with the default library: camera rays from the twin's hook, bounce-2 rays from the trace harness"""
    import numpy as np
    rt = _rt()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import walk_lab as wl
    for arm, W, H in ((5, 600, 600), (7, 800, 800)):
        sc = rt.Scene.reference(arm, build_seed=1)
        cam = rt.camera_rays_host(sc, W, H, SPP).reshape(-1, 8)[:, :7]
        ctx = rt.Context(sc, 0)
        lab = wl.Lab(ctx)
        b2 = lab.dump_rays(W, H, SPP, 3)[2]
        lab.close()
        ctx.close()
        b2 = b2[b2[:, 7] != 0.0][:, :7]
        for kind, r in (("camera", cam), ("bounce", b2)):
            full = np.concatenate([r, np.full((len(r), 1), 0.001), np.full((len(r), 1), np.inf)], axis=1)
            np.save(os.path.join(directory, f"rays_{arm}_{kind}.npy"), full)
    print("HITJSON {}", flush=True)


def child(arm, W, H, kind, directory, reps):
    """one column, under the profiler: the ray queries and, on camera rays, the first-hit AOV kernel of the same frame"""
    import numpy as np
    rt = _rt()
    rays = np.load(os.path.join(directory, f"rays_{arm}_{kind}.npy"))
    n = len(rays)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    ctx = rt.Context(rt.Scene.reference(arm, build_seed=1), 0)
    d_rays, d_out = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(d_rays), rays.nbytes) == 0 and hip.hipMalloc(C.byref(d_out), n * 96) == 0
    assert hip.hipMemcpy(d_rays, rays.ctypes.data, rays.nbytes, 1) == 0
    ms, st = [], None
    for k in range(reps + 1):
        st = ctx.hit_device(d_rays.value, d_out.value, None, n)
        ms.append(st["kernel_ms"])
    out = np.empty((n, 12))
    assert hip.hipMemcpy(out.ctypes.data, d_out, out.nbytes, 2) == 0
    res = {"rays": n, "hits": int(out[:, 0].sum()), "hit_event_ms": ms[1:], "variant": st["variant"], "grid": st["grid"], "block": st["block"]}
    if kind == "camera":
        for k in range(reps + 1):
            ctx.render_aov(W, H, SPP)
        res["aov_paths"] = W * H * SPP
    ctx.close()
    print("HITJSON " + json.dumps(res), flush=True)


def kernel_stats(d):
    """name -> (calls, mean ns) from rocprofv3's kernel_stats.csv under d"""
    out = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            out[r["Name"]] = (int(r["Calls"]), float(r["AverageNs"]))
    return out


def run_child(cmd, env, what):
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    line = [l for l in p.stdout.splitlines() if l.startswith("HITJSON ")]
    if p.returncode != 0 or not line:
        sys.stdout.write(p.stdout[-4000:])
        sys.exit(f"{what}: child failed with exit status {p.returncode}")
    return json.loads(line[-1][len("HITJSON "):])


def geomean(v):
    return math.exp(sum(math.log(x) for x in v) / len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hit_bench.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--staged", default=os.path.join(ROOT, "raytracing-1w_amd", "librt1w_hit_staged.so"))
    ap.add_argument("--prepare", metavar="DIR")
    ap.add_argument("--child", nargs=5, metavar=("ARM", "W", "H", "KIND", "DIR"))
    a = ap.parse_args()
    if a.prepare:
        return prepare(a.prepare)
    if a.child:
        return child(int(a.child[0]), int(a.child[1]), int(a.child[2]), a.child[3], a.child[4], a.reps)
    me = [sys.executable, os.path.abspath(__file__), "--reps", str(a.reps)]
    work = tempfile.mkdtemp(prefix="hit_bench_")
    run_child(["timeout", "-k", "10", "600"] + me + ["--prepare", work], dict(os.environ), "ray files")
    forms = {"direct": None, "staged": os.path.abspath(a.staged)}
    if not os.path.exists(forms["staged"]):
        sys.exit(f"{forms['staged']} is missing: make -C raytracing-1w_amd/csrc hit_staged")
    runs = []
    for run in range(a.runs):
        rows = []
        for name, arm, W, H, kind in CASES:
            row = {"case": name, "arm": arm, "width": W, "height": H, "spp": SPP, "rays_of": kind}
            for form, lib in forms.items():
                env = dict(os.environ)
                if lib:
                    env["RT1W_LIB"] = lib
                d = tempfile.mkdtemp(prefix="hit_bench_prof_")
                cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + me + \
                      ["--child", str(arm), str(W), str(H), kind, work]
                res = run_child(cmd, env, f"{name}, {form}")
                ks = kernel_stats(d)
                shutil.rmtree(d, ignore_errors=True)
                hk = [(k, v) for k, v in ks.items() if "rt_hit_kernel" in k]
                assert len(hk) == 1 and hk[0][1][0] == a.reps + 1, sorted(ks)
                mean_s = hk[0][1][1] * 1e-9
                row.update({"rays": res["rays"], "hits": res["hits"], "variant": res["variant"], "grid": res["grid"],
                            f"{form}_kernel_ms": mean_s * 1e3, f"{form}_rays_per_s": res["rays"] / mean_s,
                            f"{form}_bytes_per_s": res["rays"] * BYTES_PER_RAY / mean_s,
                            f"{form}_share_of_copy_rate": res["rays"] * BYTES_PER_RAY / mean_s / COPY_RATE,
                            f"{form}_event_ms_median": sorted(res["hit_event_ms"])[len(res["hit_event_ms"]) // 2]})
                if kind == "camera":
                    ak = [(k, v) for k, v in ks.items() if "rt_aov_kernel" in k]
                    assert len(ak) == 1 and ak[0][1][0] == a.reps + 1, sorted(ks)
                    row[f"aov_segments_per_s_beside_{form}"] = res["aov_paths"] / (ak[0][1][1] * 1e-9)
            rows.append(row)
            print(json.dumps({"run": run, **row}), flush=True)
        runs.append({"rows": rows, "geomean_rays_per_s": {f: geomean([r[f"{f}_rays_per_s"] for r in rows]) for f in forms}})
    shutil.rmtree(work, ignore_errors=True)
    gm = {f: [r["geomean_rays_per_s"][f] for r in runs] for f in forms}
    summary = {f: {"geomean_rays_per_s_median": sorted(v)[len(v) // 2], "geomean_rays_per_s_range": [min(v), max(v)],
                   "spread": (max(v) - min(v)) / sorted(v)[len(v) // 2]} for f, v in gm.items()}
    ratio = summary["staged"]["geomean_rays_per_s_median"] / summary["direct"]["geomean_rays_per_s_median"]
    spread = max(s["spread"] for s in summary.values())
    summary["staged_over_direct"] = ratio
    summary["default_by_the_rule"] = "staged" if ratio - 1.0 > spread else "direct"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/hit_bench.py", "reps": a.reps, "runs_made": a.runs, "bytes_per_ray": BYTES_PER_RAY, "copy_rate": COPY_RATE,
                   "summary": summary, "runs": runs}, f, indent=1)
        f.write("\n")
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
