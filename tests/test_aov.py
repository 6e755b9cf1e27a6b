"""First-hit feature buffers (rt1w_render_aov / rt1w_render_aov_device, include/rt1w.h): albedo, normal, depth, coverage of every
sample's camera ray.  CPU tier: the CPU twin (librt1w_lab.so: rt1w_lab_aov_host, the kernels' own rt_aov.h built for the host) against
the literal oracle and against known answers of the Cornell box; the ABI surface.  GPU tier: the kernels bit for bit against the twin,
the tile forms against each other, non-interference with the beauty render, and full-size frames."""
import ctypes as C
import os
import re
import subprocess
import time

import numpy as np
import pytest

from orc import OracleScene, rt as _rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rt():
    return _rt()


def _camera_bg(scene):
    """camera (origin, lower_left_corner, horizontal, vertical, u, v, w, lens_radius, time0, time1) and background of a scene"""
    cb = np.frombuffer(scene.flat(6).tobytes()[:27 * 8], dtype=np.float64)
    return {"origin": cb[0:3], "llc": cb[3:6], "h": cb[6:9], "v": cb[9:12], "lens": cb[21], "bg": cb[24:27]}


# ------------------------------------------------------------------------------------------------------------------ CPU tier --

@pytest.mark.parametrize("arm,tile,spp", [(0, (150, 100, 24, 16), 4), (1, (100, 80, 20, 16), 6), (2, (180, 60, 16, 16), 8),
                                          (3, (160, 70, 24, 16), 5)])
def test_twin_coverage_equals_the_literal_oracles_misses(rt, arm, tile, spp):
    """max_depth = 1 in the literal recursive oracle returns background x (#misses) per pixel on arms 0-3 (no emitters): the integer miss
    count of every pixel must be what the twin's coverage says.  Checks the camera rays (arm 0: aperture 0.1, moving spheres) and the
    hit / miss decision of every sample independently of rt_core.h."""
    W, H = 400, 225
    sc = rt.Scene.reference(arm, build_seed=1)
    bg = _camera_bg(sc)["bg"]
    k = int(np.argmax(bg))
    assert bg[k] > 0
    lit, _ = OracleScene(arm, build_seed=1).render(W, H, spp, max_depth=1, tile=tile, out_sum=True)
    misses = lit[..., k] / bg[k]
    assert np.all(np.abs(misses - np.round(misses)) < 1e-9)
    misses = np.round(misses).astype(int)
    aov = rt.aov_host(sc, W, H, spp, tile=tile)
    hits = np.round(aov[..., 7] * spp).astype(int)
    assert np.array_equal(hits, spp - misses)
    # the misses' albedo is the background, the hits' normals are unit vectors facing the camera: pixels that all hit or all missed
    full_miss, full_hit = misses == spp, misses == 0
    assert np.all(aov[full_miss][:, :3] == bg) and np.all(aov[full_miss][:, 3:6] == 0) and np.all(np.isinf(aov[full_miss][:, 6]))
    assert np.all(np.isfinite(aov[full_hit][:, 6])) and np.all(aov[full_hit][:, 6] > 0)


def _project(cam, P, W, H):
    """image (i, j) of world point P (the pinhole camera of camera.rs:61-73)"""
    A = np.stack([cam["h"], cam["v"], -(P - cam["origin"])], axis=1)
    u, v, _ = np.linalg.solve(A, cam["origin"] - cam["llc"])
    return u * (W - 1), v * (H - 1)


def _corner_rays(cam, i, j, W, H):
    """the camera rays of the four corners of pixel (i, j)'s jitter square (lens radius 0)"""
    for a in (0.0, 1.0):
        for b in (0.0, 1.0):
            d = cam["llc"] + (i + a) / (W - 1) * cam["h"] + (j + b) / (H - 1) * cam["v"] - cam["origin"]
            yield cam["origin"], d


def _slab(o, d, lo, hi):
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (lo - o) / d, (hi - o) / d
    tn, tf = np.nanmax(np.minimum(t0, t1)), np.nanmin(np.maximum(t0, t1))
    return tn <= tf and tf > 0, tn


def test_twin_cornell_known_answers(rt):
    """Arm 5 (Cornell box): pixels at least 2 px inside the projected red wall, green wall, floor, light and the tall box's front face.
    Albedo and normal are exactly the surface's; the light is seen from below through its FlipFace (albedo 15); the aluminium box's
    normal is its face normal rotated by the scene's own RotateY sin / cos; depth lies within the pixel-jitter bound."""
    W = H = 600
    spp = 2  # sums of two equal values: the means are exact
    sc = rt.Scene.reference(5, build_seed=1)
    cam = _camera_bg(sc)
    assert cam["lens"] == 0.0
    nodes = sc.flat(0).tobytes()
    rot = [np.frombuffer(nodes[k * 96 + 8:k * 96 + 24], dtype=np.float64) for k in range(len(nodes) // 96)
           if (int.from_bytes(nodes[k * 96:k * 96 + 4], "little") & 0xFF) == 8]
    assert len(rot) == 1
    sn, cs = rot[0]
    # occluders for the walls: the tall box's and the glass sphere's world bounds
    corners = np.array([[x, y, z] for x in (0, 165) for y in (0, 330) for z in (0, 165)], dtype=np.float64)
    world = np.stack([cs * corners[:, 0] + sn * corners[:, 2], corners[:, 1], -sn * corners[:, 0] + cs * corners[:, 2]], 1) + [265, 0, 295]
    occ = [(world.min(0), world.max(0)), (np.array([100.0, 0, 100]), np.array([280.0, 180, 280]))]
    # (point on the surface, axis, plane k, in-plane bounds (a0, a1, b0, b1) on the other two axes, albedo, normal)
    surfaces = {
        "red": ((0.0, 420.0, 300.0), 0, 0.0, (0, 555, 0, 555), (0.65, 0.05, 0.05), (1.0, 0.0, 0.0)),
        "green": ((555.0, 420.0, 300.0), 0, 555.0, (0, 555, 0, 555), (0.12, 0.45, 0.15), (-1.0, 0.0, 0.0)),
        "floor": ((450.0, 0.0, 100.0), 1, 0.0, (0, 555, 0, 555), (0.73, 0.73, 0.73), (0.0, 1.0, 0.0)),
        "light": ((278.0, 554.0, 280.0), 1, 554.0, (213, 343, 227, 332), (15.0, 15.0, 15.0), (0.0, -1.0, 0.0)),
    }
    for name, (P, ax, k, (a0, a1, b0, b1), alb, nrm) in surfaces.items():
        pi, pj = _project(cam, np.array(P), W, H)
        i, j = int(pi), int(pj)
        box = (i - 2, j - 2, 5, 5)
        # every corner ray of the 5 x 5 block meets the plane inside the rect (margin 1), and nothing of the scene in front of it
        dmin, dmax = np.inf, 0.0
        oth = [x for x in range(3) if x != ax]
        for ii in range(i - 2, i + 3):
            for jj in range(j - 2, j + 3):
                for o, d in _corner_rays(cam, ii, jj, W, H):
                    t = (k - o[ax]) / d[ax]
                    p = o + t * d
                    assert a0 + 1 <= p[oth[0]] <= a1 - 1 and b0 + 1 <= p[oth[1]] <= b1 - 1, name
                    for lo, hi in occ:
                        hit, tn = _slab(o, d, lo, hi)
                        assert not (hit and tn < t), name
                    if ii == i and jj == j:
                        dist = t * np.linalg.norm(d)
                        dmin, dmax = min(dmin, dist), max(dmax, dist)
        aov = rt.aov_host(sc, W, H, spp, tile=box)
        c = aov[2, 2]
        assert np.all(aov[..., 0:3] == np.array(alb)), name
        assert np.all(aov[..., 3:6] == np.array(nrm)), name
        assert np.all(aov[..., 7] == 1.0), name
        assert dmin * (1 - 1e-12) <= c[6] <= dmax * (1 + 1e-12), (name, dmin, c[6], dmax)
    # the tall aluminium box's front face (local z = 0): a 5 x 5 block around the projection of its centre
    loc = np.array([82.5, 200.0, 0.0])
    P = np.array([cs * loc[0] + sn * loc[2], loc[1], -sn * loc[0] + cs * loc[2]]) + [265, 0, 295]
    pi, pj = _project(cam, P, W, H)
    i, j = int(pi), int(pj)
    for ii in range(i - 2, i + 3):
        for jj in range(j - 2, j + 3):
            for o, d in _corner_rays(cam, ii, jj, W, H):
                # into the box's space (Translate, then RotateY as hittable.rs:238-251) and onto its z = 0 face
                o2, d2 = o - [265, 0, 295], d
                ol = np.array([cs * o2[0] - sn * o2[2], o2[1], sn * o2[0] + cs * o2[2]])
                dl = np.array([cs * d2[0] - sn * d2[2], d2[1], sn * d2[0] + cs * d2[2]])
                t = -ol[2] / dl[2]
                p = ol + t * dl
                assert 1 <= p[0] <= 164 and 1 <= p[1] <= 329
                hit, tn = _slab(o, d, *occ[1])
                assert not (hit and tn < t)
    aov = rt.aov_host(sc, W, H, spp, tile=(i - 2, j - 2, 5, 5))
    assert np.all(aov[..., 0:3] == np.array([0.8, 0.85, 0.88]))
    assert np.all(np.abs(aov[..., 3:6] - np.array([-sn, 0.0, -cs])) <= 1e-12)
    assert np.all(aov[..., 7] == 1.0)


def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rt1w.h")).read(), flags=re.S)
    return set(re.findall(r"\b(rt1w_[a-z0-9_]+)\s*\(", src))


def test_aov_abi_surface(rt):
    """Both entries are declared, exported, mirrored in INTEGRATION.md section 2, and refuse a null context / null params."""
    assert {"rt1w_render_aov", "rt1w_render_aov_device"} <= _declared()
    assert "#define RT1W_AOV_CHANNELS 8" in open(os.path.join(ROOT, "include", "rt1w.h")).read()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", rt.LIB_PATH]).decode()
    assert re.search(r"\brt1w_render_aov\b", syms) and re.search(r"\brt1w_render_aov_device\b", syms)
    assert "rt1w_internal_aov" not in syms and "rt1w_lab_aov_host" not in syms
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    block = md[md.index("## 2."):md.index("## 3.")]
    assert "pub fn rt1w_render_aov(" in block and "pub fn rt1w_render_aov_device(" in block
    p = rt.RenderParams(64, 64, 0, 0, 64, 64, 1, 0, 50, 0, 0, 0, 0, 0, 0, 0)
    buf = np.zeros(64 * 64 * 8)
    assert rt._lib.rt1w_render_aov(None, C.byref(p), buf.ctypes.data_as(C.c_void_p), None) == rt.ERR_INVALID
    assert rt._lib.rt1w_render_aov(None, None, buf.ctypes.data_as(C.c_void_p), None) == rt.ERR_INVALID
    assert rt._lib.rt1w_render_aov_device(None, C.byref(p), C.c_void_p(16), None) == rt.ERR_INVALID
    assert rt._lib.rt1w_render_aov_device(None, None, C.c_void_p(16), None) == rt.ERR_INVALID


# what every entry refuses in an rt1w_render_params (include/rt1w.h; csrc/render_params.h: params_check, the text the entries and the
# twin share): name -> (fields changed in a good 64 x 16 frame with an 8-row tile, the documented return code)
_BAD_PARAMS = {
    "tile outside the image": (dict(x0=60, tile_w=8), "ERR_INVALID"),
    "tile below the image": (dict(y0=12), "ERR_INVALID"),
    "spp 0": (dict(spp=0), "ERR_INVALID"),
    "strip_rows without strip_period": (dict(strip_rows=2), "ERR_INVALID"),
    "strip_period without strip_rows": (dict(strip_period=4), "ERR_INVALID"),
    "strip_period below strip_rows": (dict(strip_rows=4, strip_period=2), "ERR_INVALID"),
    # tile row 7 is image row 0 + (7 // 2) * 8 + 7 % 2 = 25 of 16, while y0 + tile_h = 8 fits: the twin used to render this
    "last interleaved strip outside the image": (dict(strip_rows=2, strip_period=8), "ERR_INVALID"),
    # the last sample index would be 2^32: the twin used to render this too
    "sample_offset + spp over 2^32 - 1": (dict(sample_offset=0xFFFFFFFF, spp=1), "ERR_INVALID"),
    "sample_offset + spp over 2^32 - 1, large spp": (dict(sample_offset=0x80000000, spp=0x80000000), "ERR_INVALID"),
    "unknown precision": (dict(precision=7), "ERR_UNSUPPORTED"),
    "f32": (dict(precision=1), "ERR_UNSUPPORTED"),   # a known precision, but the AOV entries are f64 only
}


@pytest.mark.parametrize("case", sorted(_BAD_PARAMS))
def test_twin_refuses_what_the_entries_refuse(rt, case):
    """The twin is the expected side of the GPU bit-equality tests, so it must refuse the parameter sets the entries refuse, with
    the same code: both twins (first hit and deep) run the entries' own check.  The unchanged frame, the largest sample range and
    an interleaved tile whose last strip just fits are accepted."""
    lab = rt.load_lab()
    sc = rt.Scene.reference(5, build_seed=1)
    out = np.zeros(8 * 64 * 8)

    def twins(p):
        lab.rt1w_lab_aov_host.restype = lab.rt1w_lab_aov_deep_host.restype = C.c_int
        lab.rt1w_lab_aov_host.argtypes = [C.c_void_p, C.POINTER(rt.RenderParams), C.c_void_p]
        lab.rt1w_lab_aov_deep_host.argtypes = [C.c_void_p, C.POINTER(rt.RenderParams), C.c_uint32, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
        return (lab.rt1w_lab_aov_host(sc._h, C.byref(p), out.ctypes.data_as(C.c_void_p)),
                lab.rt1w_lab_aov_deep_host(sc._h, C.byref(p), 2, 0.0, out.ctypes.data_as(C.c_void_p), None, None))

    def params(**changed):
        p = rt.RenderParams(64, 16, 0, 0, 64, 8, 1, 0, 50, 0, 0, 0, 0, 0, 0, 0)
        for k, v in changed.items():
            setattr(p, k, v)
        return p

    assert twins(params()) == (rt.OK, rt.OK)
    assert twins(params(sample_offset=0xFFFFFFFE, spp=1)) == (rt.OK, rt.OK)
    assert twins(params(strip_rows=2, strip_period=4)) == (rt.OK, rt.OK)   # tile row 7 is image row 13 of 16
    changed, code = _BAD_PARAMS[case]
    assert twins(params(**changed)) == (getattr(rt, code), getattr(rt, code)), case


# ------------------------------------------------------------------------------------------------------------------ GPU tier --

def _valid_variants(info):
    media, tex, ms, sd = info["has_media"], info["has_textures"], info["has_moving"], info["scope_depth"]
    v = [1, 3, 4]
    if not media and not tex and not ms and sd <= 2:
        v.append(0)
    if not media:
        v.append(2)
    if not media and sd == 0:
        v.append(5)
    return sorted(v)


@pytest.mark.gpu
def test_gpu_aov_bit_identical_to_the_twin(rt):
    """All eight arms, small crops at several spp, non-zero sample_offset and global_seed; every variant valid for the scene; arms 0 and
    7 under the SAH tree and the near-far order."""
    W, H = 96, 64
    for arm in range(8):
        sc = rt.Scene.reference(arm, build_seed=1)
        ctx = rt.Context(sc, 0)
        for spp, tile, so, gs in ((1, (0, 0, W, H), 0, 0), (3, (13, 7, 41, 29), 5, 11), (8, (40, 20, 17, 9), 1000, 3)):
            a = ctx.render_aov(W, H, spp, tile=tile, sample_offset=so, global_seed=gs)
            b = rt.aov_host(sc, W, H, spp, tile=tile, sample_offset=so, global_seed=gs)
            assert np.array_equal(a, b), (arm, spp, tile)
        for v in _valid_variants(sc.info()):
            a, st = ctx.render_aov(W, H, 2, tile=(5, 3, 37, 21), sample_offset=7, global_seed=2, variant=v, with_stats=True)
            assert st["variant"] == v
            assert np.array_equal(a, rt.aov_host(sc, W, H, 2, tile=(5, 3, 37, 21), sample_offset=7, global_seed=2, variant=v)), (arm, v)
        ctx.close()
    for arm in (0, 7):
        for mode in ("sah", "near_far"):
            sc = rt.Scene.reference(arm, build_seed=1)
            sc = sc.set_bvh_build("sah") if mode == "sah" else sc.set_walk_order(True)
            ctx = rt.Context(sc, 0)
            a, st = ctx.render_aov(W, H, 4, tile=(8, 8, 48, 40), sample_offset=3, global_seed=9, with_stats=True)
            assert st["variant"] == sc.info()["variant"]  # the scene's own variant: V4 where the near-far order annotated the tree (arm 7)
            assert np.array_equal(a, rt.aov_host(sc, W, H, 4, tile=(8, 8, 48, 40), sample_offset=3, global_seed=9)), (arm, mode)
            ctx.close()


class _DeviceBuffer:
    """device memory from the HIP runtime librt1w.so itself uses (what a torch tensor's data_ptr() would hand over)"""

    def __init__(self, nbytes):
        self.hip = C.CDLL("libamdhip64.so")
        self.nbytes = nbytes
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), C.c_size_t(nbytes)) == 0
        self.ptr = p.value

    def to_host(self, shape):
        out = np.empty(shape, dtype=np.float64)
        assert out.nbytes == self.nbytes
        assert self.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(self.ptr), C.c_size_t(self.nbytes), 2) == 0  # DeviceToHost
        return out

    def free(self):
        self.hip.hipFree(C.c_void_p(self.ptr))


@pytest.mark.gpu
def test_gpu_aov_tiles_strips_device_and_frame_agree(rt):
    """Tile, strip-interleaved tile and full frame agree pixel for pixel; the device entry into device memory equals the host entry;
    the argument errors that need a context."""
    W, H, spp = 80, 60, 3
    for arm in (5, 7):
        sc = rt.Scene.reference(arm, build_seed=1)
        ctx = rt.Context(sc, 0)
        full = ctx.render_aov(W, H, spp, sample_offset=2, global_seed=4)
        tile = ctx.render_aov(W, H, spp, tile=(10, 20, 30, 25), sample_offset=2, global_seed=4)
        assert np.array_equal(tile, full[20:45, 10:40])
        # rank 1 of 3 with strips of 4 rows: tile row r = image row 4 + (r // 4) * 12 + r % 4
        rows = [4 + (r // 4) * 12 + r % 4 for r in range(20)]
        strip = ctx.render_aov(W, H, spp, tile=(0, 4, W, 20), strips=(4, 12), sample_offset=2, global_seed=4)
        assert np.array_equal(strip, full[rows])
        dev = _DeviceBuffer(H * W * 8 * 8)
        st = ctx.render_aov_device(dev.ptr, W, H, spp, sample_offset=2, global_seed=4)
        assert st["paths"] == W * H * spp == st["segments"]
        assert np.array_equal(dev.to_host((H, W, 8)), full)
        dev.free()
        buf = np.zeros((H, W, 8))
        p = ctx._params(W, H, spp, 50, None, 0, 0, 0, False)
        assert rt._lib.rt1w_render_aov(ctx._h, C.byref(p), None, None) == rt.ERR_INVALID
        assert rt._lib.rt1w_render_aov_device(ctx._h, C.byref(p), None, None) == rt.ERR_INVALID
        for flag in (rt.OUT_SUM, rt.UNSORTED, rt.GENERIC, rt.RNG_REFERENCE, rt.OUT_FRAME, 1 << 20):
            p.flags = flag
            assert rt._lib.rt1w_render_aov(ctx._h, C.byref(p), buf.ctypes.data_as(C.c_void_p), None) == rt.ERR_INVALID
            assert rt.last_error()
        p.flags = 0
        p.precision = 1
        assert rt._lib.rt1w_render_aov(ctx._h, C.byref(p), buf.ctypes.data_as(C.c_void_p), None) == rt.ERR_UNSUPPORTED
        ctx.close()


@pytest.mark.gpu
def test_gpu_beauty_render_after_aov_is_unchanged(rt):
    """An AOV call leaves nothing behind that a beauty render on the same context would see."""
    for arm in (5, 7):
        sc = rt.Scene.reference(arm, build_seed=1)
        fresh = rt.Context(sc, 0)
        ref, _ = fresh.render(64, 48, 4, global_seed=3)
        fresh.close()
        ctx = rt.Context(sc, 0)
        ctx.render_aov(256, 256, 2)  # grows the context's framebuffer past the beauty frame's size
        img, _ = ctx.render(64, 48, 4, global_seed=3)
        ctx.close()
        assert np.array_equal(img, ref, equal_nan=True)


@pytest.mark.gpu
@pytest.mark.parametrize("arm,W,H", [(5, 600, 600), (7, 800, 800)])
def test_gpu_aov_full_frames(rt, arm, W, H):
    """Cornell 600 x 600 x 16 and final_scene 800 x 800 x 16: finite everywhere except depth where coverage is 0, coverage in [0, 1],
    |normal| <= 1."""
    sc = rt.Scene.reference(arm, build_seed=1)
    ctx = rt.Context(sc, 0)
    t0 = time.perf_counter()
    a, st = ctx.render_aov(W, H, 16, with_stats=True)
    wall = time.perf_counter() - t0
    ctx.close()
    print(f"arm {arm} {W}x{H}x16 AOV: kernel {st['kernel_ms']:.2f} ms, call {wall * 1e3:.1f} ms, variant {st['variant']}, "
          f"grid {st['grid']} x {st['block']}, {st['segments'] / st['kernel_ms'] / 1e3:.1f} Msegments/s")
    cov = a[..., 7]
    assert np.all((cov >= 0) & (cov <= 1))
    assert np.all(np.isfinite(a[..., [0, 1, 2, 3, 4, 5, 7]]))
    assert np.all(np.isfinite(a[..., 6][cov > 0])) and np.all(np.isinf(a[..., 6][cov == 0]))
    assert np.all(np.linalg.norm(a[..., 3:6], axis=-1) <= 1 + 1e-12)
