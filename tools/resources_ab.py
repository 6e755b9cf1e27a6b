#!/usr/bin/env python3
"""Resources of every render kernel on two trees, side by side: the scene-specialised kernels rt1w_precompile writes (arms 1-6 at build
seed 1, the f32 builds of arms 5 and 6) and every kernel of the hipcc-built render units.  Nothing here runs on a GPU.

usage: tools/resources_ab.py PARENT_TREE THIS_TREE > profiles/NAME_resources.txt     (both trees built: csrc/rt1w_precompile exists)

Per kernel and tree: static VALU / SALU instructions (llvm-objdump -d of the code object, mnemonics that start with v_ / s_), VGPRs,
spilled VGPRs, scratch bytes per lane, LDS bytes per block, waves per SIMD.  The hipcc units are compiled device-only with the
Makefile's options and -Rpass-analysis=kernel-resource-usage (the remarks tools/kernel_resources.py summarises); the precompiled
kernels come from the run-time compiler, which prints no remarks, so their figures are the notes of the code object (llvm-readelf
--notes) and their waves are what the register count allows (512 / VGPRs rounded up to 8, at most 8)."""
import collections
import os
import re
import subprocess
import sys
import tempfile

UNITS = ("context", "context_ref", "context_f32", "context_tiles", "aov", "aov_tiles")
LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def static_counts(co):
    """{symbol: (VALU, SALU)} of a code object"""
    txt = subprocess.run([LLVM + "/llvm-objdump", "-d", co], capture_output=True, text=True, check=True).stdout
    out, sym = collections.defaultdict(lambda: [0, 0]), None
    for ln in txt.splitlines():
        m = re.match(r"^[0-9a-f]+ <([^>]+)>:", ln)
        if m:
            sym = m.group(1)
            continue
        m = re.match(r"^\s+([vs])_\w+", ln)
        if m and sym:
            out[sym][0 if m.group(1) == "v" else 1] += 1
    return out


def demangle(names):
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    out = []
    for d in dem:
        d = re.sub(r"\(anonymous namespace\)::", "", d)
        d = re.sub(r"^void ", "", re.sub(r"\(Rt(SceneView|Frame).*", "", d))
        out.append(d)
    return out


def makefile_flags(csrc):
    mk = open(os.path.join(csrc, "Makefile")).read()
    kopts = re.search(r"^KOPTS := (.*)$", mk, re.M).group(1).split()
    root = os.path.dirname(os.path.dirname(csrc))
    return ["-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-ffp-contract=off", "--offload-arch=gfx950", "-Wno-unused-result"] + kopts + \
           ["-I" + os.path.join(root, "include"), "-I" + csrc]


def hipcc_units(tree, work):
    """[(unit, kernel, row)] in the order the compiler reports them"""
    csrc = os.path.join(tree, "raytracing-1w_amd", "csrc")
    flags = makefile_flags(csrc)
    procs = []
    for u in UNITS:
        co = os.path.join(work, u + ".co")
        procs.append((u, co, subprocess.Popen([HIPCC] + flags + ["--cuda-device-only", "--no-gpu-bundle-output", "-Rpass-analysis=kernel-resource-usage", "-c",
                                                                  os.path.join(csrc, u + ".hip"), "-o", co], stderr=subprocess.PIPE, text=True)))
    rows = []
    for u, co, p in procs:
        err = p.communicate()[1]
        assert p.returncode == 0, err[-2000:]
        counts = static_counts(co)
        for b in re.split(r"(?=remark: [^\n]*Function Name)", err):
            m = re.search(r"Function Name: (\S+)", b)
            if not m:
                continue
            g = lambda k: int(re.search(k + r": (\d+)", b).group(1))
            valu, salu = counts.get(m.group(1), (0, 0))
            rows.append((u, m.group(1), dict(valu=valu, salu=salu, vgpr=g("VGPRs") + g("AGPRs"), vspill=g("VGPRs Spill"),
                                             scratch=g(r"ScratchSize \[bytes/lane\]"), lds=g(r"LDS Size \[bytes/block\]"), waves=g(r"Occupancy \[waves/SIMD\]"))))
    return rows


def precompiled(tree, work):
    csrc = os.path.join(tree, "raytracing-1w_amd", "csrc")
    kdir = os.path.join(work, "kernels")
    os.makedirs(kdir, exist_ok=True)
    log = subprocess.run([os.path.join(csrc, "rt1w_precompile"), kdir, "1"], capture_output=True, text=True, check=True)
    rows = []
    for ln in (log.stdout + log.stderr).splitlines():
        m = re.match(r"(arm \d+ seed 1(?: f32)?):.*-> (\S+\.hsaco)", ln)
        if not m:
            continue
        notes = subprocess.run([LLVM + "/llvm-readelf", "--notes", m.group(2)], capture_output=True, text=True, check=True).stdout
        g = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", notes).group(1))
        valu, salu = static_counts(m.group(2))["rt_jit_sorted"]
        vgpr = g("vgpr_count")
        rows.append(("precompiled", m.group(1), dict(valu=valu, salu=salu, vgpr=vgpr, vspill=g("vgpr_spill_count"), scratch=g("private_segment_fixed_size"),
                                                     lds=g("group_segment_fixed_size"), waves=min(8, 512 // max(8, (vgpr + 7) // 8 * 8)))))
    return rows


def main():
    parent, this = (os.path.abspath(p) for p in sys.argv[1:3])
    sides = []
    for tree in (parent, this):
        with tempfile.TemporaryDirectory() as work:
            sides.append(precompiled(tree, work) + hipcc_units(tree, work))
    names = demangle([k for _, k, _ in sides[0]])
    assert [(u, k) for u, k, _ in sides[0]] == [(u, k) for u, k, _ in sides[1]], "the two trees do not have the same kernels"
    fmt = lambda r: f"{r['valu']:5d} / {r['salu']:4d} / {r['vgpr']:3d} / {r['vspill']:3d} / {r['scratch']:4d} / {r['lds']:5d} / {r['waves']}"
    print("columns: static VALU / static SALU / VGPRs / spilled VGPRs / scratch bytes per lane / LDS bytes per block / waves per SIMD")
    unit = None
    lost, gained = [], []
    for (u, _, a), (_, _, b), name in zip(sides[0], sides[1], names):
        if u != unit:
            unit = u
            print(f"\n[{u}]")
        print(f"  {name}\n      parent    {fmt(a)}\n      this tree {fmt(b)}")
        if b["waves"] < a["waves"]:
            lost.append(f"{u}: {name}")
        if b["scratch"] > a["scratch"]:
            gained.append(f"{u}: {name}: {a['scratch']} -> {b['scratch']} B")
    print("\nkernels that lose a wave: " + ("none" if not lost else ""))
    for x in lost:
        print("  " + x)
    print("kernels that gain scratch: " + ("none" if not gained else ""))
    for x in gained:
        print("  " + x)
    tot = [sum(r["valu"] for _, _, r in side) for side in sides]
    print(f"\nstatic VALU over all rows: {tot[0]} -> {tot[1]}")


if __name__ == "__main__":
    main()
