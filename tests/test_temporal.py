"""Temporal accumulation (rt1w_context_set_camera / rt1w_temporal_accumulate / rt1w_render_temporal, include/rt1w.h): a live context's
camera, the reprojection of the previous frame's history and one call that runs a frame of an animation.  CPU tier: the CPU twin
(librt1w_lab.so: rt1w_lab_temporal_host, the kernel's own rt_temporal.h built for the host) on the ABI surface and its refusals, against
the independent statement tests/tm_reference.py, on images whose answer follows from the definition, the camera function, and an
orbit of 8 noisy frames against converged ones.  GPU tier: the kernel bit for bit against the twin, a moved camera against a fresh
scene, the one call against the composition of the public entries, and the kernel's resources."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import orc
import tm_reference as TM
from orc import rt as _rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
REFUSALS = os.path.join(GOLD, "temporal_refusals.json")
ULP = 2.0 ** -53

# the quality cases: arm -> (width, height); 8 frames of 4 spp, the camera turned ORBIT_DEG per frame about look_at's vertical axis,
# global_seed = frame index; the reference is 2048 spp with global_seed 1000 at the LAST camera (tests/golden/temporal_ref_arm*.npy)
QUALITY = {5: (96, 96), 4: (128, 72)}
FRAMES, SPP, ORBIT_DEG, REF_SPP, REF_SEED = 8, 4, 1.0, 2048, 1000
# mse of the displayed last frame, measured with the twins:
#   "a": temporal / the last frame alone;  "b": (temporal + rt1w_denoise) / (the last frame alone + rt1w_denoise)
# and the share of the last frame's hit pixels with len > 1 at this orbit: 0.989 (arm 5), 0.981 (arm 4)
MEASURED_RATIO = {"a": {5: 0.1550, 4: 0.2158}, "b": {5: 0.7209, 4: 0.9358}}


def generate_reference_frames():
    """Writes tests/golden/temporal_ref_arm{5,4}.npy: the converged frames of the quality test at the last camera of the orbit, rendered
    by this project's own CPU build of the core (about 15 s on 16 cores).  Run by hand when a quality case changes: python -c 'import
    test_temporal as t; t.generate_reference_frames()' from tests/."""
    rt = _rt()
    for arm, (w, h) in QUALITY.items():
        sc = rt.Scene.reference(arm, build_seed=1)
        rt.scene_set_camera_host(sc, **rt.orbit_camera(rt.reference_camera(arm), ORBIT_DEG * (FRAMES - 1)))
        ref, _ = orc.flat_render(sc, w, h, REF_SPP, global_seed=REF_SEED)
        np.save(os.path.join(GOLD, f"temporal_ref_arm{arm}.npy"), ref)


ARGS = dict(look_from=(0.0, 0.0, 10.0), look_at=(0.0, 0.0, 0.0), vup=(0.0, 1.0, 0.0), vfov_deg=40.0, aspect_ratio=4.0 / 3.0, aperture=0.0,
            focus_dist=10.0, time0=0.0, time1=1.0)
_SCENES = {}


def _camera(rt, **args):
    """the 24 doubles of a camera made from `args`, through the one camera function (the lab hook on a committed scene)"""
    sc = _SCENES.setdefault("cam", rt.Scene.reference(1, build_seed=1))
    rt.scene_set_camera_host(sc, **dict(ARGS, **args))
    return rt.scene_camera_host(sc).array()


def _plane_depth(cam, w, h):
    """distance along the ray from the lens centre through every pixel centre to the plane z = 0: the first-hit depth of a wall there"""
    o, llc, hor, ver = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    y, x = np.mgrid[0:h, 0:w]
    d = llc + ((x + 0.5) / (w - 1))[..., None] * hor + ((y + 0.5) / (h - 1))[..., None] * ver - o
    t = -o[2] / d[..., 2]
    return t * np.linalg.norm(d, axis=-1)


def _plane_pair(rt, w, h, cur_args, prev_args, seed):
    """A wall at z = 0 seen by two cameras: (cur_frame, cur_aov, cur_cam, prev_hist, prev_len, prev_aov, prev_cam), random colours,
    albedo and history lengths 1 .. 40"""
    rng = np.random.default_rng(seed)
    cc, pc = _camera(rt, **cur_args), _camera(rt, **prev_args)
    frame, hist = rng.uniform(0.1, 1.0, (h, w, 3)), rng.uniform(0.1, 1.0, (h, w, 3))
    ln = rng.integers(1, 41, (h, w)).astype(np.float64)
    aovs = []
    for cam in (cc, pc):
        aov = np.zeros((h, w, 8))
        aov[..., 0:3] = rng.uniform(0.005, 1.0, (h, w, 3))   # below the floor here and there
        aov[..., 3:6] = (0.0, 0.0, 1.0)
        aov[..., 6] = _plane_depth(cam, w, h)
        aov[..., 7] = 1.0
        aovs.append(aov)
    return frame, aovs[0], cc, hist, ln, aovs[1], pc


# ------------------------------------------------------------------------------------------------------------------ CPU tier --

def _cases(rt):
    """(name, params, which buffer is null or aliased) of everything the accumulate entries refuse for their parameters or buffers"""
    P = rt.TemporalParams
    ok = (6, 4, 0, 0, 0.0, 0.0)
    out = [("null params", None, None)]
    for name, p in (("width 0", (0, 4, 0, 0, 0, 0)), ("height 0", (6, 0, 0, 0, 0, 0)), ("unknown flag", (6, 4, 2, 0, 0, 0)),
                    ("depth_tol negative", (6, 4, 0, 0, -0.1, 0)), ("depth_tol NaN", (6, 4, 0, 0, float("nan"), 0)),
                    ("depth_tol infinite", (6, 4, 0, 0, float("inf"), 0)), ("normal_min negative", (6, 4, 0, 0, 0, -0.5)),
                    ("normal_min NaN", (6, 4, 0, 0, 0, float("nan"))), ("normal_min > 1", (6, 4, 0, 0, 0, 1.5))):
        out.append((name, P(*p), None))
    for k, b in enumerate(("cur_frame", "cur_aov", "cur_cam", "prev_hist", "prev_len", "prev_aov", "prev_cam", "hist", "len", "frame_out")):
        out.append(("null " + b, P(*ok), ("null", k)))
    for name, pair in (("hist is cur_frame", (7, 0)), ("hist is prev_hist", (7, 3)), ("len is prev_len", (8, 4)), ("frame_out is cur_frame", (9, 0)),
                       ("frame_out is hist", (9, 7)), ("frame_out overlaps hist", (9, 7, 8))):
        out.append((name, P(*ok), ("alias",) + pair))
    return out


TEXT = {"null params": "null argument", "width 0": "temporal: width and height must be 1 .. 2^30", "height 0": "temporal: width and height must be 1 .. 2^30",
        "unknown flag": "temporal: unknown flag (flags: 0 or RT1W_DENOISE_KEEP_ALBEDO)", "depth_tol": "temporal: depth_tol must be finite and >= 0 (0 = default)",
        "normal_min": "temporal: normal_min must be 0 .. 1 (0 = default)", "null cur_cam": "null camera", "null prev_cam": "null camera", "null": "null buffer",
        "alias": "temporal: hist, len and frame_out must not overlap each other or an input"}


def _call_args(rt, case, typed):
    """the ten buffer / camera arguments of a 6 x 4 call with `case`'s defect (typed: as the entries' argtypes take them, else plain
    addresses), and what keeps them alive"""
    _, _, how = case
    cam = rt.Camera.of(_camera(rt))
    bufs = [np.zeros((4, 6, 3)), np.zeros((4, 6, 8)), cam, np.zeros((4, 6, 3)), np.zeros((4, 6)), np.zeros((4, 6, 8)), cam, np.zeros((4, 6, 3)),
            np.zeros((4, 6)), np.zeros((4, 6, 3))]
    addr = [C.addressof(b) if isinstance(b, rt.Camera) else b.ctypes.data for b in bufs]
    if how and how[0] == "null":
        addr[how[1]] = None
    if how and how[0] == "alias":
        addr[how[1]] = addr[how[2]] + (how[3] if len(how) > 3 else 0)
    ptr = [None if q is None else (C.cast(q, C.POINTER(rt.Camera)) if typed and k in (2, 6) else C.c_void_p(q)) for k, q in enumerate(addr)]
    return ptr, bufs


def _refusals(rt, ctx):
    """[name, code, text] of every case through the twin (ctx None) or the two entries"""
    got = {}
    fns = {"rt1w_lab_temporal_host": rt.load_lab().rt1w_lab_temporal_host} if ctx is None else \
        {n: getattr(rt._lib, n) for n in ("rt1w_temporal_accumulate", "rt1w_temporal_accumulate_device")}
    for name, fn in fns.items():
        rows = []
        for case in _cases(rt):
            ptr, keep = _call_args(rt, case, ctx is not None)
            p = C.byref(case[1]) if case[1] is not None else None
            if ctx is None:
                fn.restype = C.c_int
                fn.argtypes = [C.c_void_p] * 12
                rows.append([case[0], fn(p, *ptr, None), ""])
            else:
                rc = fn(ctx._h, p, *ptr, C.byref(rt.Stats()))
                rows.append([case[0], rc, rt.last_error() if rc < 0 else ""])
        got[name] = rows
    return got


def _expected_text(name):
    first = name.split(" ")[0]
    return TEXT[name] if name in TEXT else TEXT[first] if first in ("depth_tol", "normal_min", "null") else TEXT["alias"]


def test_refusals_and_abi(rt):
    """Arity against the header, the rt1w_abi_sizeof code of rt1w_camera (6: 5 stays the code that answers 0), the layouts, and every
    refusal: the recording tests/golden/temporal_refusals.json holds case, code and text of what the two accumulate entries refuse, in
    this file's order; the twin refuses every one of them, and the camera function refuses what rt1w_scene_set_camera refuses."""
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rt1w.h")).read(), flags=re.S)
    for name, n in {"rt1w_context_set_camera": 10, "rt1w_context_get_camera": 2, "rt1w_temporal_accumulate": 13, "rt1w_temporal_accumulate_device": 13,
                    "rt1w_render_temporal": 6, "rt1w_temporal_reset": 1, "rt1w_reference_camera": 7}.items():
        assert len(getattr(rt._lib, name).argtypes) == n, name
        decl = hdr[hdr.index("int " + name + "("):]
        assert decl[:decl.index(";")].count(",") + 1 == n, name
    assert rt._lib.rt1w_abi_sizeof(6) == C.sizeof(rt.Camera) == 192 and rt._lib.rt1w_abi_sizeof(5) == 0 and rt._lib.rt1w_abi_sizeof(7) == 0
    assert C.sizeof(rt.TemporalParams) == 32 and rt.TemporalParams.depth_tol.offset == 16 and rt.Camera.lens_radius.offset == 168
    want = json.load(open(REFUSALS))
    names = [c[0] for c in _cases(rt)]
    assert sorted(want) == ["rt1w_temporal_accumulate", "rt1w_temporal_accumulate_device"]
    for e, cs in want.items():
        assert [c[0] for c in cs] == names, "the recording's cases are not the cases of this file"
        assert all(c[1] == rt.ERR_INVALID and c[2] == _expected_text(c[0]) for c in cs), e
    for row in _refusals(rt, None)["rt1w_lab_temporal_host"]:
        assert row[1] == rt.ERR_INVALID, row
    ptr, keep = _call_args(rt, ("ok", None, None), False)
    fn = rt.load_lab().rt1w_lab_temporal_host
    assert fn(C.byref(rt.TemporalParams(6, 4, 1, 3, 0.1, 1.0)), *ptr, None) == 0
    ptr, keep = _call_args(rt, ("ok", None, None), True)
    # without a context the entries answer "null argument" before anything else
    for name in ("rt1w_temporal_accumulate", "rt1w_temporal_accumulate_device"):
        assert getattr(rt._lib, name)(None, C.byref(rt.TemporalParams(6, 4, 0, 0, 0, 0)), *ptr, None) == rt.ERR_INVALID and rt.last_error() == "null argument"
    assert rt._lib.rt1w_context_set_camera(None, *[rt._v3(v) for v in ((0, 0, 1), (0, 0, 0), (0, 1, 0))], 40.0, 1.0, 0.0, 10.0, 0.0, 1.0) == rt.ERR_INVALID
    assert rt._lib.rt1w_context_get_camera(None, None) == rt.ERR_INVALID and rt._lib.rt1w_temporal_reset(None) == rt.ERR_INVALID
    assert rt._lib.rt1w_render_temporal(None, None, None, None, None, None) == rt.ERR_INVALID
    sc = rt.Scene.reference(1, build_seed=1)
    for bad in (dict(time0=1.0, time1=1.0), dict(time0=2.0, time1=1.0), dict(time0=float("nan"))):
        with pytest.raises(rt.Rt1wError) as e:
            rt.scene_set_camera_host(sc, **dict(ARGS, **bad))
        assert e.value.code == rt.ERR_INVALID
    fn = C.CDLL(os.path.join(os.path.dirname(rt.LIB_PATH), "librt1w_lab.so")).rt1w_lab_scene_set_camera   # untyped: a null vector
    fn.argtypes = [C.c_void_p] * 4 + [C.c_double] * 6
    assert fn(sc._h, None, rt._v3((0, 0, 0)), rt._v3((0, 1, 0)), 40.0, 1.0, 0.0, 10.0, 0.0, 1.0) == rt.ERR_INVALID


def _synthetic(rt):
    """41 x 30, a wall seen by two cameras 3 degrees apart (the current one with a lens), holding every case the definition names"""
    w, h = 41, 30
    f, a, cc, hist, ln, pa, pc = _plane_pair(rt, w, h, dict(aperture=0.4, look_from=(0.3, 0.2, 10.0)), dict(look_from=(0.9, 0.0, 9.5), look_at=(0.4, 0.1, 0.0)), 5)
    assert cc[21] > 0.0                                       # lens_radius > 0
    a[3:6, 4:9, 3:6], a[3:6, 4:9, 6], a[3:6, 4:9, 7] = 0.0, np.inf, 0.0   # misses
    a[10:12, 20:24, 6] = -4.0                                  # a finite depth that puts the point behind both cameras
    pa[:, :8, 6] *= 1.5                                        # a depth edge in the previous frame
    pa[24:, :, 3:6] = (1.0, 0.0, 0.0)                          # a normal edge in the previous frame
    ln[7, 25], ln[8, 30], ln[20, 33] = 0.0, 0.0, np.inf        # taps without history, a length that is not finite
    hist[9, 28, 1], hist[22, 36, 0] = np.nan, np.inf           # values that are not finite
    pa[5, 35, 6], pa[6, 36, 7] = np.nan, 0.0
    return f, a, cc, hist, ln, pa, pc


@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("max_history", [0, 4])
def test_twin_against_the_independent_statement(rt, keep, max_history):
    """tests/tm_reference.py restates the header's prose in numpy long double.  Twin and statement agree within 1e-12 relative on hist,
    len and frame_out (1e-12 absolute on the taps' weights), and on which pixels have history, everywhere but on the pixels the statement marks as sitting within 1e-9 of one
    of the definition's tests; the synthetic pair holds every case the definition names (each counted below)."""
    args = _synthetic(rt)
    hist, ln, out, rec = rt.temporal_host(*args, with_record=True, keep_albedo=keep, max_history=max_history)
    rh, rl, ro, rrec, near = TM.accumulate(*args, keep_albedo=keep, max_history=max_history)
    f, a, cc, ph, pl, pa, pc = args
    hit = (a[..., 7] > 0) & np.isfinite(a[..., 6])
    has = rrec[..., 7] > 0
    nvalid = (rrec[..., 2:6] > 0).sum(axis=-1)
    cap = (max_history or 32) - 1
    counts = {"miss": int((~hit).sum()), "behind": int((hit & (a[..., 6] < 0)).sum()), "outside": int((hit & (a[..., 6] > 0) & ~has & (rrec[..., 0] == 0) & (rrec[..., 1] == 0)).sum()),
              "split": int((has & (nvalid < 4)).sum()), "capped": int((has & (rl == cap + 1)).sum()), "near": int(near.sum())}
    print(keep, max_history, counts)
    assert counts["miss"] == 15 and counts["behind"] == 8 and counts["outside"] > 20 and counts["split"] > 40 and counts["capped"] > 20 and has.sum() > 600
    assert counts["near"] < 0.02 * near.size
    ok = ~near
    assert np.array_equal(rec[..., 7][ok] > 0, has[ok])
    assert np.all(ln[~hit] == 1.0) and np.all(ln[hit & (a[..., 6] < 0)] == 1.0)
    # a split by the depth edge and by the normal edge: pixels with history whose taps straddle column 8 / row 24
    ix, iy = np.floor(rrec[..., 0].astype(np.float64)), np.floor(rrec[..., 1].astype(np.float64))
    assert (has & (ix == 7) & (nvalid < 4)).sum() > 5 and (has & (iy == 23) & (nvalid < 4)).sum() > 5
    for got, want, name in ((hist, rh, "hist"), (ln, rl, "len"), (out, ro, "frame_out"), (rec[..., 2:7], rrec[..., 2:7], "weights")):
        g, wv = got[ok], want[ok].astype(np.float64)
        fin = np.isfinite(wv)
        assert np.array_equal(np.isfinite(g), fin), name
        err = np.abs(g[fin] - want[ok][fin]).astype(np.float64)
        rel = err / np.maximum(np.abs(wv[fin]), 1e-300)
        print(name, "max rel", rel[np.abs(wv[fin]) > 0].max() if (np.abs(wv[fin]) > 0).any() else 0.0)
        # the weights are differences of a position and its floor: 1e-12 of their scale, which is 1
        assert np.all(err <= 1e-12) if name == "weights" else np.all(rel <= 1e-12), name
    # a tap that is not finite poisons nobody: only the current frame's own NaN could come out, and there is none
    assert np.isfinite(hist).all() and np.isfinite(out).all() and np.isfinite(ln).all()


def test_no_history_gives_the_current_frame(rt):
    """prev_len = 0 everywhere: len = 1, hist = cur_frame / A and frame_out = (cur_frame / A) * A -- cur_frame within 2 roundings
    where A is the raw albedo, and its very bits with RT1W_DENOISE_KEEP_ALBEDO."""
    f, a, cc, hist, ln, pa, pc = _plane_pair(rt, 33, 19, {}, dict(look_from=(0.5, 0.0, 10.0)), 11)
    h2, l2, out = rt.temporal_host(f, a, cc, hist, np.zeros_like(ln), pa, pc)
    A = np.where(a[..., 0:3] > 0.01, a[..., 0:3], 0.01)
    assert np.all(l2 == 1.0) and np.array_equal(h2, f / A) and np.array_equal(out, (f / A) * A)
    assert np.all(np.abs(out - f) <= 2 * ULP * f)
    h3, l3, out3 = rt.temporal_host(f, a, cc, hist, np.zeros_like(ln), pa, pc, keep_albedo=True)
    assert np.all(l3 == 1.0) and np.array_equal(h3, f) and np.array_equal(out3, f)


@pytest.mark.parametrize("length,max_history", [(5.0, 0), (40.0, 0), (40.0, 8), (3.0, 1)])
def test_identical_cameras_constant_history(rt, length, max_history):
    """The same camera twice and a constant prev_hist: every pixel away from the image's edge reprojects onto itself (fx, fy within
    1e-9 of x, y), has len = min(prev_len, max_history - 1) + 1 and hist = (N' h + c) / (N' + 1) to 1e-12."""
    w, h = 37, 26
    f, a, cc, hist, ln, pa, pc = _plane_pair(rt, w, h, {}, {}, 13)
    hist[:] = (0.3, 0.6, 0.9)
    ln[:] = length
    h2, l2, out, rec = rt.temporal_host(f, a, cc, hist, ln, a, cc, with_record=True, max_history=max_history)
    y, x = np.mgrid[0:h, 0:w]
    inner = (slice(1, h - 1), slice(1, w - 1))
    assert np.abs(rec[..., 0] - x)[inner].max() < 1e-9 and np.abs(rec[..., 1] - y)[inner].max() < 1e-9
    n = min(length, (max_history or 32) - 1)
    assert np.all(np.abs(l2[inner] - (n + 1)) <= 1e-12 * (n + 1))
    A = np.where(a[..., 0:3] > 0.01, a[..., 0:3], 0.01)
    want = (n * hist + f / A) / (n + 1)
    assert np.all(np.abs(h2 - want)[inner] <= 1e-12 * want[inner]) and np.all(np.abs(out - want * A)[inner] <= 1e-12 * (want * A)[inner])


@pytest.mark.parametrize("shift", [3, -5])
def test_translation_by_whole_pixels(rt, shift):
    """A fronto-parallel textured wall at the focus distance and a previous camera moved parallel to it by `shift` pixels' width there:
    the history of pixel x comes from pixel x - shift of the previous frame.  The position is within 1e-9 of that pixel's centre, so
    the four weights, whichever side of the integer the position rounds to, are within 1e-9 of one 1 and three 0."""
    w, h = 40, 30
    pitch = 10.0 * (2.0 * np.tan(np.radians(20.0)) * 4.0 / 3.0) / (w - 1)   # focus_dist * viewport width / (w - 1)
    f, a, cc, hist, ln, pa, pc = _plane_pair(rt, w, h, {}, dict(look_from=(shift * pitch, 0.0, 10.0), look_at=(shift * pitch, 0.0, 0.0)), 17)
    h2, l2, out, rec = rt.temporal_host(f, a, cc, hist, ln, pa, pc, with_record=True, keep_albedo=True)
    y, x = np.mgrid[0:h, 0:w]
    src = x - shift
    ok = (src >= 1) & (src < w - 1) & (y >= 1) & (y < h - 1)
    assert ok.sum() > 0.7 * w * h
    assert np.abs(rec[..., 0] - src)[ok].max() < 1e-9 and np.abs(rec[..., 1] - y)[ok].max() < 1e-9
    wts = np.sort(rec[..., 2:6], axis=-1)[ok]
    assert np.abs(wts[:, 3] - 1.0).max() < 1e-9 and np.abs(wts[:, :3]).max() < 1e-9 and np.all(rec[..., 7][ok] == 1.0)
    n = np.minimum(ln[y, np.clip(src, 0, w - 1)], 31.0)
    want = (n[..., None] * hist[y, np.clip(src, 0, w - 1)] + f) / (n[..., None] + 1)
    assert np.all(np.abs(h2 - want)[ok] <= 1e-7 * want[ok]) and np.all(np.abs(l2 - (n + 1))[ok] <= 1e-7 * (n + 1)[ok])
    # pixels whose source lies beyond the previous frame's edge start anew
    gone = (src < -1) | (src > w)
    assert gone.any() and np.all(l2[gone] == 1.0) and np.array_equal(h2[gone], f[gone])


def _small_scene(rt, args):
    s = rt.Scene(build_seed=1)
    s.set_world(s.bvh_node([s.sphere((0, 0, 0), 1.0, s.lambertian(s.solid_color((0.5, 0.5, 0.5))))]))
    s.set_lights([])
    s.set_background((0.5, 0.5, 0.5))
    s.set_camera(**args)
    s.commit()
    return s


def test_camera_function_is_the_scenes(rt):
    """The lab hook that applies a camera to a committed scene -- the function rt1w_context_set_camera calls -- gives, bit for bit, the
    ten quantities of a scene committed with those arguments; setting the scene's own arguments back gives the original's; the flat
    record the CPU build of the core renders from follows; rt1w_reference_camera's arguments are those of the arms."""
    new = dict(ARGS, look_from=(3.0, 1.5, -7.0), look_at=(0.1, 0.2, 0.3), vup=(0.1, 1.0, 0.0), vfov_deg=33.0, aspect_ratio=1.7, aperture=0.3,
               focus_dist=6.5, time0=0.25, time1=0.75)
    a, b = _small_scene(rt, ARGS), _small_scene(rt, new)
    cam_a, cam_b = rt.scene_camera_host(a).array(), rt.scene_camera_host(b).array()
    assert not np.array_equal(cam_a, cam_b)
    flat_a = a.flat(6).copy()
    rt.scene_set_camera_host(a, **new)
    assert rt.scene_camera_host(a).array().tobytes() == cam_b.tobytes() and a.flat(6).tobytes() == b.flat(6).tobytes()
    rt.scene_set_camera_host(a, **ARGS)
    assert rt.scene_camera_host(a).array().tobytes() == cam_a.tobytes() and a.flat(6).tobytes() == flat_a.tobytes()
    assert cam_b[21] == 0.15 and cam_b[22] == 0.25 and cam_b[23] == 0.75 and tuple(cam_b[0:3]) == (3.0, 1.5, -7.0)
    for arm in (0, 4, 5, 7):
        sc = rt.Scene.reference(arm, build_seed=1) if arm != 7 else None
        if sc is not None:
            own = rt.scene_camera_host(sc).array()
            rt.scene_set_camera_host(sc, **rt.reference_camera(arm))
            assert rt.scene_camera_host(sc).array().tobytes() == own.tobytes(), arm
    assert rt.reference_camera(7)["look_from"] == (478.0, 278.0, -600.0) and rt.reference_camera(0)["aperture"] == 0.1
    turned = rt.orbit_camera(rt.reference_camera(5), 90.0)["look_from"]
    assert np.allclose(turned, (278.0 - 800.0, 278.0, 0.0), atol=1e-9)


def _disp(c):
    return np.sqrt(np.clip(np.nan_to_num(c, nan=0.0), 0.0, 0.999))


def _mse(a, b):
    return float(np.mean((_disp(a) - _disp(b)) ** 2))


@pytest.fixture(scope="module")
def orbits(rt):
    """the 8-frame orbits of the quality cases, composed with the twins: arm -> (last frame alone, temporal frame, last guides, len)"""
    res = {}
    for arm, (w, h) in QUALITY.items():
        sc = rt.Scene.reference(arm, build_seed=1)
        args = rt.reference_camera(arm)
        hist, ln, paov, pcam = np.zeros((h, w, 3)), np.zeros((h, w)), np.zeros((h, w, 8)), None
        for k in range(FRAMES):
            rt.scene_set_camera_host(sc, **rt.orbit_camera(args, ORBIT_DEG * k))
            cam = rt.scene_camera_host(sc)
            frame, _ = orc.flat_render(sc, w, h, SPP, global_seed=k)
            aov = rt.aov_host(sc, w, h, SPP, global_seed=k)
            hist, ln, out = rt.temporal_host(frame, aov, cam, hist, ln, paov, pcam if pcam is not None else cam)
            paov, pcam = aov, cam
        res[arm] = (frame, out, aov, ln)
    return res


def _assert_ratio(ratio, measured):
    """the project's standing rule for a measured quality ratio"""
    if measured < 1.0:
        assert ratio < 1.0 and ratio <= (measured + 1.0) / 2.0
    else:
        assert ratio <= 1.1 * measured   # a negative result, reported as one


@pytest.mark.parametrize("arm", sorted(QUALITY))
def test_quality_of_an_orbit(rt, orbits, arm):
    """The reason for the feature.  8 frames of 4 spp on an orbit of 1 degree per frame, against a converged frame at the last camera:
    the mean squared error of the displayed values of (a) the temporal frame over the last frame alone, (b) the same two after
    rt1w_denoise with the last frame's guides.  Measured (MEASURED_RATIO): (a) 0.155 and 0.216, (b) 0.721 and 0.936 -- the filter
    already removes most of what the history removes, so temporal + filter gains little over the filter alone on these scenes.
    Condition on the orbit: at least half of the last frame's hit pixels carry history."""
    frame, out, aov, ln = orbits[arm]
    ref = np.load(os.path.join(GOLD, f"temporal_ref_arm{arm}.npy"))
    hit = aov[..., 7] > 0
    share = float(np.mean(ln[hit] > 1))
    a = _mse(out, ref) / _mse(frame, ref)
    b = _mse(rt.denoise_host(out, aov), ref) / _mse(rt.denoise_host(frame, aov), ref)
    print(f"arm {arm}: temporal / single {a:.4f} (measured {MEASURED_RATIO['a'][arm]}), with the filter {b:.4f} (measured {MEASURED_RATIO['b'][arm]}), "
          f"share of hit pixels with history {share:.4f}, mean len {ln[hit].mean():.2f}")
    assert share >= 0.5
    _assert_ratio(a, MEASURED_RATIO["a"][arm])
    _assert_ratio(b, MEASURED_RATIO["b"][arm])


# ------------------------------------------------------------------------------------------------------------------ GPU tier --

def _wrap(a, h, w):
    """an h x w image cut from `a`, repeated where it is larger"""
    return np.ascontiguousarray(np.take(np.take(a, np.arange(h), axis=0, mode="wrap"), np.arange(w), axis=1, mode="wrap"))


@pytest.mark.gpu
@pytest.mark.parametrize("arm", [0, 5, 7])
def test_kernel_equals_twin(rt, gpu_ctx_factory, arm):
    """Two cameras 2 degrees apart, 203 x 149 at 4 spp: the kernel's hist, len and frame_out are the twin's bits, with both flag settings,
    max_history 2 and 32 (the lengths fed in reach 5), on the frame and on 5 x 5, 1 x 300 and 300 x 1 images cut from it (partial
    blocks, taps past every edge, one lane column or row per workgroup)."""
    w, h = 203, 149
    args = rt.reference_camera(arm, aspect_ratio=w / h)
    ctx = gpu_ctx_factory(rt.Scene.reference(arm, build_seed=1, aspect_ratio=w / h))
    frames = []
    for k in range(2):
        ctx.set_camera(**rt.orbit_camera(args, 2.0 * k))
        frames.append((ctx.render(w, h, 4, global_seed=k)[0], ctx.render_aov(w, h, 4, global_seed=k), ctx.get_camera().array()))
    (f0, a0, c0), (f1, a1, c1) = frames
    hist0, len0, out0 = ctx.temporal_accumulate(f0, a0, c0, np.zeros_like(f0), np.zeros((h, w)), a0, c0)
    t = rt.temporal_host(f0, a0, c0, np.zeros_like(f0), np.zeros((h, w)), a0, c0)
    assert all(np.array_equal(g, e, equal_nan=True) for g, e in zip((hist0, len0, out0), t)) and np.all(len0 == 1.0)
    len0 = len0 * (1.0 + (np.arange(w) % 5))   # 1 .. 5
    shared = 0
    for ch, cw in ((h, w), (5, 5), (300, 1), (1, 300)):
        cut = [_wrap(x, ch, cw) for x in (f1, a1, hist0, len0, a0)]
        for keep in (False, True):
            for mh in (2, 32):
                got = ctx.temporal_accumulate(cut[0], cut[1], c1, cut[2], cut[3], cut[4], c0, keep_albedo=keep, max_history=mh)
                want = rt.temporal_host(cut[0], cut[1], c1, cut[2], cut[3], cut[4], c0, keep_albedo=keep, max_history=mh)
                for g, e, name in zip(got, want, ("hist", "len", "frame_out")):
                    assert np.array_equal(g, e, equal_nan=True), (arm, ch, cw, keep, mh, name)
                if (ch, cw) == (h, w):
                    shared = float(np.mean(got[1] > 1))
    print("arm", arm, "share of pixels with history", shared)
    assert shared > 0.1   # the comparison is of the gather, not of first frames: a tenth of the frame at the least reprojects
    ctx.set_camera(**args)


@pytest.mark.gpu
def test_entries_refuse_as_recorded(rt, gpu_ctx_factory):
    """With a context the two accumulate entries answer every case of tests/golden/temporal_refusals.json with its code and text, and
    rt1w_render_temporal and rt1w_context_set_camera refuse what the header says."""
    ctx = gpu_ctx_factory(rt.Scene.reference(5, build_seed=1))
    assert _refusals(rt, ctx) == json.load(open(REFUSALS))
    for bad, text in ((dict(tile=(0, 0, 32, 64)), "whole image"), (dict(flags=rt.OUT_SUM), "RT1W_OUT_SUM"), (dict(f32=True), "RT1W_PRECISION_F32"),
                      (dict(strips=(2, 4), tile=(0, 0, 64, 32)), "strip_rows"), (dict(temporal=dict(depth_tol=-1.0)), "depth_tol"),
                      (dict(temporal=dict(normal_min=2.0)), "normal_min"), (dict(denoise=dict(iterations=9)), "iterations")):
        with pytest.raises(rt.Rt1wError) as e:
            ctx.render_temporal(64, 64, 1, **bad)
        assert e.value.code == rt.ERR_INVALID and text in str(e.value), (bad, str(e.value))
    with pytest.raises(rt.Rt1wError) as e:
        ctx.set_camera(**dict(rt.reference_camera(5), time0=1.0, time1=0.5))
    assert e.value.code == rt.ERR_INVALID and "time0 < time1" in str(e.value)


def _fresh(rt, arm, aspect, args):
    """a scene of `arm` whose camera is `args` for everything made from it: the arm built, then the camera function applied"""
    sc = rt.Scene.reference(arm, build_seed=1, aspect_ratio=aspect)
    rt.scene_set_camera_host(sc, **args)
    return sc


@pytest.mark.gpu
@pytest.mark.parametrize("arm", [5, 0, 7])
def test_set_camera_equals_a_fresh_scene(rt, gpu_ctx_factory, arm):
    """set_camera(new) then a render is, bit for bit, the render of a fresh context of a scene with the camera `new`: the scene's own
    kernel (arm 5 the scene-specialised sweep, 0 the pair walk, 7 the stack walk with its walk table), the feature buffers and a tile
    list; for arm 5 also f32 mode (its f32 scene built before AND after the camera moves) and the reference-stream mode.  get_camera
    follows.  Another context of the same scene keeps its camera, and with the original arguments set back the render is the original's."""
    w, h, spp = 64, 48, 4
    aspect = w / h
    own = rt.reference_camera(arm, aspect_ratio=aspect)
    new = rt.orbit_camera(dict(own, vfov_deg=own["vfov_deg"] * 0.9, aperture=0.05), 7.0)
    tiles = [(0, 0, 0), (48, 32, 2), (16, 16, 0)]
    modes = [dict(), dict(f32=True), dict(reference_stream=True)] if arm == 5 else [dict()]

    def everything(c):
        out = [c.render(w, h, spp, global_seed=3, **m)[0] for m in modes]
        return out + [c.render_aov(w, h, spp, global_seed=3), c.render_tiles(w, h, spp, 16, tiles, global_seed=3)[0]]

    sc = rt.Scene.reference(arm, build_seed=1, aspect_ratio=aspect)
    ctx, other = gpu_ctx_factory(sc), gpu_ctx_factory(sc)
    original = everything(ctx)                     # builds the f32 scene of arm 5 with the scene's own camera
    cam0 = ctx.get_camera().array()
    ctx.set_camera(**new)
    moved = everything(ctx)
    fresh_ctx = gpu_ctx_factory(_fresh(rt, arm, aspect, new))
    fresh = everything(fresh_ctx)
    assert ctx.get_camera().array().tobytes() == fresh_ctx.get_camera().array().tobytes() != cam0.tobytes()
    for k, (a, b, o) in enumerate(zip(moved, fresh, original)):
        assert np.array_equal(a, b, equal_nan=True), (arm, k)
        assert not np.array_equal(a, o, equal_nan=True), (arm, k)
    if arm == 5:                                   # the f32 scene built only after the camera moved
        late = gpu_ctx_factory(sc)
        late.set_camera(**new)
        assert np.array_equal(late.render(w, h, spp, global_seed=3, f32=True)[0], fresh[1], equal_nan=True)
    assert other.get_camera().array().tobytes() == cam0.tobytes()
    assert np.array_equal(other.render(w, h, spp, global_seed=3)[0], original[0], equal_nan=True)
    assert rt.scene_camera_host(sc).array().tobytes() == cam0.tobytes()     # the scene object is not touched
    ctx.set_camera(**own)
    assert ctx.get_camera().array().tobytes() == cam0.tobytes()
    for a, o in zip(everything(ctx), original):
        assert np.array_equal(a, o, equal_nan=True), arm


@pytest.mark.gpu
@pytest.mark.parametrize("filtered", [False, True])
def test_one_call_equals_composition(rt, gpu_ctx_factory, filtered):
    """rt1w_render_temporal over 3 frames of an orbit is, bit for bit, the public entries called in sequence (render, render_aov,
    temporal_accumulate with the previous call's outputs, denoise), with and without the filter; after temporal_reset the next frame
    is a first frame; a change of size starts anew; a plain render afterwards does not see the temporal state."""
    w = h = 72
    args = rt.reference_camera(5)
    sc = rt.Scene.reference(5, build_seed=1)
    one, parts = gpu_ctx_factory(sc), gpu_ctx_factory(sc)
    plain = one.render(w, h, 4, global_seed=9)[0]
    tk = dict(max_history=3)
    hist, ln, paov, pcam = np.zeros((h, w, 3)), np.zeros((h, w)), np.zeros((h, w, 8)), None
    firsts = []
    for k in range(3):
        cam_args = rt.orbit_camera(args, 1.5 * k)
        one.set_camera(**cam_args)
        parts.set_camera(**cam_args)
        got, st = one.render_temporal(w, h, 4, global_seed=k, temporal=tk, filter=filtered, with_stats=True)
        frame, aov, cam = parts.render(w, h, 4, global_seed=k)[0], parts.render_aov(w, h, 4, global_seed=k), parts.get_camera()
        hist, ln, want = parts.temporal_accumulate(frame, aov, cam, hist, ln, paov, pcam if pcam is not None else cam, **tk)
        paov, pcam = aov, cam
        if filtered:
            want = parts.denoise(want, aov)
        assert np.array_equal(got, want, equal_nan=True), k
        assert st["paths"] == w * h * 4 and st["kernel_ms"] > 0 and st["total_ms"] >= st["kernel_ms"]
        if k == 0:
            firsts.append(got)
    assert float(np.mean(ln > 1)) > 0.5 and ln.max() == 3.0
    # reset: the next frame is a first frame again
    one.temporal_reset()
    one.set_camera(**args)
    assert np.array_equal(one.render_temporal(w, h, 4, global_seed=0, temporal=tk, filter=filtered), firsts[0], equal_nan=True)
    # another size starts anew, and coming back does too
    small = one.render_temporal(48, 40, 4, global_seed=0, filter=filtered)
    one.temporal_reset()
    assert np.array_equal(one.render_temporal(48, 40, 4, global_seed=0, filter=filtered), small, equal_nan=True)
    assert np.array_equal(one.render_temporal(w, h, 4, global_seed=0, temporal=tk, filter=filtered), firsts[0], equal_nan=True)
    assert np.array_equal(one.render(w, h, 4, global_seed=9)[0], plain, equal_nan=True)


@pytest.mark.gpu
def test_cli_writes_the_frames_of_an_orbit(rt, gpu_ctx_factory, tmp_path):
    """rt1w --frames 2 --orbit 3 --denoise writes NAME_0000.ppm and NAME_0001.ppm: the text of Context.render_temporal's frames with the
    camera turned 3 degrees before the second and the seed counting up."""
    import subprocess
    exe = os.path.join(os.path.dirname(rt.LIB_PATH), "rt1w")
    out = str(tmp_path / "orbit.ppm")
    subprocess.run([exe, "--scene", "5", "--width", "48", "--height", "48", "--spp", "2", "--seed", "5", "--frames", "2", "--orbit", "3", "--denoise",
                    "--out", out], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    ctx = gpu_ctx_factory(rt.Scene.reference(5, build_seed=1))
    args = rt.reference_camera(5)
    for k in range(2):
        ctx.set_camera(**rt.orbit_camera(args, 3.0 * k))
        want = rt.format_ppm(ctx.render_temporal(48, 48, 2, global_seed=5 + k, filter=True))
        assert open(str(tmp_path / f"orbit_{k:04d}.ppm")).read() == want, k
    assert not os.path.exists(str(tmp_path / "orbit_0002.ppm")) and not os.path.exists(out)


@pytest.mark.gpu
def test_kernel_uses_no_scratch(rt):
    """The build keeps the compiler's resource remarks of temporal.hip in csrc/temporal.resources and fails on scratch; what it wrote
    says: one kernel, no scratch, no spills, no LDS."""
    text = open(os.path.join(ROOT, "raytracing-1w_amd", "csrc", "temporal.resources")).read()
    assert text.count("Function Name:") == 1 and "rt_tm_accumulate_kernel" in text
    for key in ("ScratchSize [bytes/lane]", "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]"):
        assert re.findall(re.escape(key) + r": (\d+)", text) == ["0"], key


if __name__ == "__main__":
    import sys
    if "--record" in sys.argv:
        rt_ = _rt()
        rows = [[c[0], rt_.ERR_INVALID, _expected_text(c[0])] for c in _cases(rt_)]
        json.dump({"rt1w_temporal_accumulate": rows, "rt1w_temporal_accumulate_device": rows}, open(REFUSALS, "w"), indent=0)
