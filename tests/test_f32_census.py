"""The census of non-finite samples in single precision (tests/golden/f32_nonfinite_census.json; `make_golden.py census` makes it) on
the CPU twin of the f32 kernels: every sample it lists is non-finite exactly as listed, every sample the draw contract fixed is finite,
and the one mechanism the census names is the literal oracle's too.  1x1 tiles of a 600x600 frame, one sample each: milliseconds."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import orc

HERE = os.path.dirname(os.path.abspath(__file__))
CENSUS = json.load(open(os.path.join(HERE, "golden", "f32_nonfinite_census.json")))


def frames():
    return [(name, f) for name, f in CENSUS["frames"].items()]


def entries():
    return [(name, f, e) for name, f in frames() for e in f["entries"]]


_SCENES = {}


def scene_of(rt, f):
    key = (f["arm"], f["aspect"])
    if key not in _SCENES:
        _SCENES[key] = rt.Scene.reference(f["arm"], build_seed=1, aspect_ratio=f["aspect"])
    return _SCENES[key]


def one_sample(rt, f, pixel, sample, **kw):
    row, col = pixel
    return orc.flat_f32_render(scene_of(rt, f), f["W"], f["H"], 1, tile=(col, row, 1, 1), sample_offset=sample, out_sum=True, threads=1, **kw)


def test_the_census_is_complete_and_decided():
    """Every frame's zero pixels are accounted for -- a non-finite sample each, or listed as finite -- every entry has a cause and a
    decision, and none blames a draw at the closed end of its interval: that cause is gone (tests/test_f32_draws.py)."""
    assert set(CENSUS["frames"]) == {"cornell_600x600x256", "random_scene_300x200x64", "cornell_smoke_200x200x64", "final_scene_200x200x64"}
    for name, f in frames():
        assert len({tuple(e["pixel"]) for e in f["entries"]}) + f["finite_zero_pixels"]["count"] == f["twin_zero_pixels"], name
        for e in f["entries"]:
            assert len(e["cause"]) > 40 and e["decision"].split(":")[0] in ("kept and pinned", "fixed", "open"), (name, e["pixel"])
            assert not any(w in e["cause"] for w in ("1.0f", "closed end", "equals high", "== high", "rounds to")), (name, e["pixel"])
    assert CENSUS["cornell_literal_zero_pixel_count"] == CENSUS["frames"]["cornell_600x600x256"]["literal_zero_pixels"]["count"]


@pytest.mark.parametrize("i", range(len(entries())))
def test_a_listed_sample_is_non_finite_as_listed(rt, i):
    """The 1x1 single-sample render of the twin: non-finite raw sum where the decision keeps the sample (finite where it says fixed),
    first at the listed max_depth, with the listed segment count; and the literal f32 oracle is non-finite on that sample where the
    census says `literal_too`."""
    name, f, e = entries()[i]
    raw, st = one_sample(rt, f, e["pixel"], e["sample"])
    kept = not e["decision"].startswith("fixed")
    assert np.isfinite(raw).all() != kept, (name, e["pixel"], e["sample"], raw)
    if kept:
        assert st["segments"] == e["segments"]
        assert [repr(float(v)) for v in raw[0, 0]] == e["raw_sum"]
        assert not np.isfinite(one_sample(rt, f, e["pixel"], e["sample"], max_depth=e["bounce"])[0]).all()
        if e["bounce"] > 1:
            assert np.isfinite(one_sample(rt, f, e["pixel"], e["sample"], max_depth=e["bounce"] - 1)[0]).all()
    row, col = e["pixel"]
    lit, _ = orc.OracleScene(f["arm"], build_seed=1, aspect_ratio=f["aspect"], f32=True).render(
        f["W"], f["H"], 1, tile=(col, row, 1, 1), sample_offset=e["sample"], out_sum=True, threads=1)
    assert (not np.isfinite(lit).all()) == e["literal_too"], (name, e["pixel"], lit)


def test_the_mechanism_is_the_literal_oracles(rt):
    """Every listed sample of Cornell dies of one thing: the light's pdf_value for a direction with dir.y == 0 from a point at the height
    of the light's plane (aarect.rs:84-138: t = 0 / 0 passes every rejection).  The literal f32 oracle's own XZRect::pdf_value, asked
    with the listed origin and direction, is NaN too -- also for the samples on which its own path does not come by there -- and a
    direction that is a float's step off the plane gives it a finite value."""
    orc.F32.orc_light_pdf_value.restype = C.c_float
    orc.F32.orc_light_pdf_value.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    light = np.array([213.0, 343.0, 227.0, 332.0, 554.0], dtype=np.float32)   # main.rs: the Cornell box's light, x0 x1 z0 z1 k

    def pdf(o, v):
        o, v = np.array(o, dtype=np.float32), np.array(v, dtype=np.float32)
        return orc.F32.orc_light_pdf_value(2, light.ctypes.data_as(C.c_void_p), o.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p))

    listed = [e for _, _, e in entries()]
    assert len(listed) >= 5
    for e in listed:
        o, v = e["shade_origin"], e["shade_direction"]
        assert o[1] == 554.0 and v[1] == 0.0, e["pixel"]
        assert np.isnan(pdf(o, v)), e["pixel"]
        below = [o[0], float(np.nextafter(np.float32(554.0), np.float32(0.0))), o[2]]
        up = [v[0], 554.0 - below[1], v[2]]
        assert np.isfinite(pdf(below, up)) and pdf(below, up) > 0.0, e["pixel"]


@pytest.mark.parametrize("i", range(len(CENSUS["fixed_by_draw_contract"]["samples"])))
def test_a_draw_sample_is_finite_now(rt, i):
    """The three samples of the Cornell frame whose cosine lobe drew r2 = 1.0f before the draw contract (found on the parent's twin):
    finite now, and their pixels are not black at 256 samples."""
    f = CENSUS["frames"][CENSUS["fixed_by_draw_contract"]["frame"]]
    e = CENSUS["fixed_by_draw_contract"]["samples"][i]
    raw, _ = one_sample(rt, f, e["pixel"], e["sample"])
    assert np.isfinite(raw).all(), (e, raw)
    row, col = e["pixel"]
    img, _ = orc.flat_f32_render(scene_of(rt, f), f["W"], f["H"], f["spp"], tile=(col, row, 1, 1), threads=1)
    assert np.isfinite(img).all() and (img > 0).all(), (e, img)


def test_the_finite_zero_pixel_of_cornell(rt):
    """[338, 276] is black in f32 without any non-finite sample: all 256 raw sums are exactly zero (the mirror's view of the open side),
    in the literal oracle as well."""
    f = CENSUS["frames"]["cornell_600x600x256"]
    assert f["finite_zero_pixels"]["pixels"] == [[338, 276]]
    raw, _ = orc.flat_f32_render(scene_of(rt, f), 600, 600, 256, tile=(276, 338, 1, 1), out_sum=True, chunk=1, threads=1)
    assert (raw == 0).all()
    lit, _ = orc.OracleScene(5, build_seed=1, f32=True).render(600, 600, 256, tile=(276, 338, 1, 1), out_sum=True, threads=1)
    assert (lit == 0).all()
