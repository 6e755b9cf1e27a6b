"""Which kernel each render flag reaches on each reference scene (GPU tier).

Every flag combination of the matrix below is rendered once on a small frame of every reference arm (build_seed 1), and what the
stats report -- variant, stats.sorted bits, workgroup size, chunking -- or the error code of a refusal is compared with
tests/golden/kernel_choice.json.  A change to the dispatch of csrc/context.hip that was not meant fails here, and the failing row
names the arm and the mode; a change that was meant updates a line of the fixture.  Grid sizes are not recorded: occupancy may move
with a kernel change for good reasons.  Kernels compiled at run time are kept out of the matrix: it runs with RT1W_KERNEL_CACHE
pointed at an empty directory, so the specialised kernels it can find are the ones the build precompiled.

Recording the fixture (on the GPU, from a revision whose dispatch is the one to pin):
    python tests/test_kernel_choice.py tests/golden/kernel_choice.json
"""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "kernel_choice.json")

# frame sizes of test_gpu_parity.SMALL; 2 samples per pixel are enough to choose a kernel
SIZES = {0: (96, 64), 1: (64, 36), 2: (64, 36), 3: (64, 36), 4: (64, 36), 5: (64, 64), 6: (64, 64), 7: (64, 64)}
SPP = 2
MODES = [("default", {}), ("unsorted", {"unsorted": True}), ("generic", {"generic": True}), ("lds_nodes", {"lds_nodes": True}),
         ("classic_walk", {"classic_walk": True}), ("no_node_cache", {"no_node_cache": True}),
         ("reference_stream", {"reference_stream": True}),
         ("f32", {"f32": True}), ("f32+unsorted", {"f32": True, "unsorted": True}), ("f32+classic_walk", {"f32": True, "classic_walk": True}),
         ("wavefront", {"wavefront": True})] + [(f"variant={v}", {"variant": v}) for v in range(6)] + [("render_rows", None)]
RECORDED = ("variant", "sorted", "block", "chunk", "n_chunks")


def choice_matrix(rt, extra=False):
    """{"<arm>/<mode>": {variant, sorted, block, chunk, n_chunks} or {"error": code}}, one fresh context per arm, modes in MODES
    order.  extra: also grid, segments and the sha256 of the frame (old-against-new comparisons of two builds)."""
    import hashlib
    rows = {}
    for arm, (w, h) in SIZES.items():
        ctx = rt.Context(rt.Scene.reference(arm, build_seed=1), 0)
        try:
            for name, kw in MODES:
                try:
                    img, st = ctx.render_rows(w, h, SPP) if kw is None else ctx.render(w, h, SPP, **kw)
                except rt.Rt1wError as e:
                    rows[f"{arm}/{name}"] = {"error": e.code}
                    continue
                row = {k: int(st[k]) for k in RECORDED}
                if extra:
                    row.update(grid=int(st["grid"]), segments=int(st["segments"]), sha256=hashlib.sha256(img.tobytes()).hexdigest())
                rows[f"{arm}/{name}"] = row
        finally:
            ctx.close()
    return rows


def dump(rows, path):
    """one row per line, so that a change of the dispatch is a readable diff"""
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(f"  {json.dumps(k)}: {json.dumps(v, sort_keys=True)}" for k, v in rows.items()) + "\n}\n")


@pytest.mark.gpu
def test_kernel_choice_matches_the_fixture(rt, tmp_path, monkeypatch):
    monkeypatch.setenv("RT1W_KERNEL_CACHE", str(tmp_path))
    assert rt.device_count() >= 1, "no HIP device visible: GPU tests must run on the GPU box"
    want = json.load(open(FIXTURE))
    got = choice_matrix(rt)
    assert sorted(got) == sorted(want)
    wrong = [f"{k}: got {got[k]}, fixture {want[k]}" for k in want if got[k] != want[k]]
    assert not wrong, "kernel choice differs from tests/golden/kernel_choice.json:\n" + "\n".join(wrong)


if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(HERE), HERE]
    import tempfile
    import orc
    with tempfile.TemporaryDirectory() as cache:
        os.environ["RT1W_KERNEL_CACHE"] = cache
        dump(choice_matrix(orc.rt(), extra="--extra" in sys.argv), [a for a in sys.argv[1:] if not a.startswith("--")][0])
