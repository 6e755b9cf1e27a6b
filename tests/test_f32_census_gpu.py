"""The census of non-finite samples in single precision (tests/golden/f32_nonfinite_census.json) on the GPU: around every listed sample
-- the ones that stay non-finite and the ones the draw contract fixed -- the f32 kernels built with 64-bit elementary functions
(rt.f32_exact()) equal the CPU twin bit for bit, non-finite raw sums included, and the product's kernels are finite on every sample
marked fixed.  A 1x1 tile with the listed sample alone and an 8x8 tile with four samples around it, of a 600x600 frame: a few hundred
paths per case."""
import numpy as np
import pytest

import orc
from test_f32_census import CENSUS, entries, scene_of

pytestmark = pytest.mark.gpu

FIXED = [(CENSUS["fixed_by_draw_contract"]["frame"], e) for e in CENSUS["fixed_by_draw_contract"]["samples"]]
CASES = [(name, e, not e["decision"].startswith("fixed")) for name, _, e in entries()] + [(name, e, False) for name, e in FIXED]


def tiles_of(f, e):
    """(tile, spp, sample_offset): the listed sample alone on its pixel, and among four samples of the 8x8 pixels around it"""
    row, col = e["pixel"]
    x0, y0 = min(max(col - 3, 0), f["W"] - 8), min(max(row - 3, 0), f["H"] - 8)
    return (((col, row, 1, 1), 1, e["sample"]), ((x0, y0, 8, 8), 4, max(e["sample"] - 1, 0)))


@pytest.mark.parametrize("case", CASES, ids=[f"{n}-{e['pixel'][0]}_{e['pixel'][1]}-s{e['sample']}" for n, e, _ in CASES])
def test_exact_build_equals_the_twin_around_a_listed_sample(rt, gpu_ctx_factory, case):
    name, e, non_finite = case
    f = CENSUS["frames"][name]
    sc = scene_of(rt, f)
    ctx = gpu_ctx_factory(sc)
    for tile, spp, offset in tiles_of(f, e):
        want, sw = orc.flat_f32_render(sc, f["W"], f["H"], spp, tile=tile, sample_offset=offset, chunk=1, out_sum=True, threads=1)
        with rt.f32_exact():
            got, sg = ctx.render(f["W"], f["H"], spp, tile=tile, sample_offset=offset, chunk=1, out_sum=True, f32=True, generic=True)
        assert sg["sorted"] & 32, "not an f32 render"
        row, col = e["pixel"][0] - tile[1], e["pixel"][1] - tile[0]
        print(f"\n{name} {e['pixel']} sample {e['sample']} tile {tile}: exact {got[row, col]} twin {want[row, col]} segments {sg['segments']} / {sw['segments']}")
        assert sg["segments"] == sw["segments"] and np.array_equal(got, want, equal_nan=True), (tile, got[row, col], want[row, col])
        assert np.isfinite(want[row, col]).all() != non_finite, (tile, want[row, col])
        others = np.ones(want.shape[:2], dtype=bool)
        others[row, col] = False
        assert np.isfinite(want[others]).all(), tile


@pytest.mark.parametrize("case", FIXED, ids=[f"{e['pixel'][0]}_{e['pixel'][1]}-s{e['sample']}" for _, e in FIXED])
def test_product_build_is_finite_on_a_fixed_sample(rt, gpu_ctx_factory, case):
    """The product's own f32 kernels (sinf and friends; the scene-specialised kernel where there is one, and the generic one) on the
    samples whose cosine lobe drew 1.0f before the draw contract."""
    name, e = case
    f = CENSUS["frames"][name]
    ctx = gpu_ctx_factory(scene_of(rt, f))
    for tile, spp, offset in tiles_of(f, e):
        for generic in (False, True):
            got, st = ctx.render(f["W"], f["H"], spp, tile=tile, sample_offset=offset, chunk=1, out_sum=True, f32=True, generic=generic)
            assert st["sorted"] & 32 and np.isfinite(got).all(), (tile, generic, got)
            assert got.max() > 0.0 or spp == 1, (tile, generic)
