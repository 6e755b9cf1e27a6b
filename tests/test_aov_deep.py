"""Deep feature buffers (rt1w_render_aov_deep / _device, rt1w_render_denoised_deep, include/rt1w.h): the 8 channels of rt1w_render_aov at
the first vertex of each sample's path that is not a specular surface.  CPU tier: the CPU twin (librt1w_lab.so: rt1w_lab_aov_deep_host,
the kernels' own rt_aov_deep.h built for the host) on the ABI surface, against the first-hit twin where the two must coincide, against
the beauty path of the CPU core bit for bit, on a mirror whose answer follows from the geometry, and on what the buffers are for: the
denoiser's error inside glass and mirrors.  GPU tier: the kernels bit for bit against the twin, against the beauty kernels, the entry
forms against each other, and full frames."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

# mse_M(denoise(noisy, deep guides)) / mse_M(denoise(noisy, first-hit guides)) over M = the pixels whose deep buffers differ from their
# first-hit buffers, and the same ratio over the whole frame: measured with the twins and the default filter parameters (DESIGN.md
# section 14).  Keys: (arm, max_fuzz).  The noisy frame is 16 spp, global_seed 0; the converged frames are tests/golden/denoise_ref_arm*.npy
MEASURED_RATIO = {(5, 0.0): (0.2593, 0.6514), (0, 0.0): (0.4216, 0.7308), (0, 0.5): (0.4216, 0.7308)}
QUALITY_FRAME = {5: (96, 96), 0: (128, 72)}
MAX_SPECULAR = 8


def generate_reference_frame_arm0():
    """Writes tests/golden/denoise_ref_arm0.npy the way test_denoise.generate_reference_frames writes its frames: random_scene 128 x 72 at
    2048 spp, global_seed 1, by this project's own CPU build of the core.  Run by hand from tests/."""
    rt = orc.rt()
    ref, _ = orc.flat_render(rt.Scene.reference(0, build_seed=1), 128, 72, 2048, global_seed=1)
    np.save(os.path.join(GOLD, "denoise_ref_arm0.npy"), ref)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _material_kinds(scene):
    """the kinds (rt_flat.h: 1 Lambertian, 2 Metal, 3 Dielectric, 4 DiffuseLight, 5 Isotropic) of a scene's materials, 48-byte records"""
    m = scene.flat(2).tobytes()
    return {int.from_bytes(m[k * 48 + 32:k * 48 + 36], "little") & 0xFF for k in range(len(m) // 48)}


# ------------------------------------------------------------------------------------------------------------------ CPU tier --

def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rt1w.h")).read(), flags=re.S)
    return set(re.findall(r"\b(rt1w_[a-z0-9_]+)\s*\(", src))


def test_deep_abi_surface(rt):
    """The three entries are declared, exported and mirrored in INTEGRATION.md section 2; they refuse null arguments; the twin refuses
    max_specular > 64 and a negative, NaN or infinite max_fuzz as the header says the entries do; no new ABI struct."""
    names = {"rt1w_render_aov_deep", "rt1w_render_aov_deep_device", "rt1w_render_denoised_deep"}
    assert names <= _declared()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", rt.LIB_PATH]).decode()
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    block = md[md.index("## 2."):md.index("## 3.")]
    for n in names:
        assert re.search(r"\b" + n + r"\b", syms), n
        assert f"pub fn {n}(" in block, n
    assert "rt1w_internal_aov" not in syms and "rt1w_lab_aov_deep_host" not in syms
    assert rt._lib.rt1w_abi_sizeof(5) == 0 and rt._lib.rt1w_abi_sizeof(4) == 40
    p = rt.RenderParams(64, 64, 0, 0, 64, 64, 1, 0, 50, 0, 0, 0, 0, 0, 0, 0)
    buf = np.zeros(64 * 64 * 8)
    ptr = buf.ctypes.data_as(C.c_void_p)
    lib = rt._lib
    assert lib.rt1w_render_aov_deep(None, C.byref(p), 8, 0.0, ptr, None) == rt.ERR_INVALID
    assert lib.rt1w_render_aov_deep(None, None, 8, 0.0, ptr, None) == rt.ERR_INVALID
    assert lib.rt1w_render_aov_deep_device(None, C.byref(p), 8, 0.0, C.c_void_p(16), None) == rt.ERR_INVALID
    assert lib.rt1w_render_aov_deep_device(None, None, 8, 0.0, C.c_void_p(16), None) == rt.ERR_INVALID
    assert lib.rt1w_render_denoised_deep(None, C.byref(p), None, 8, 0.0, ptr, None) == rt.ERR_INVALID
    assert lib.rt1w_render_denoised_deep(None, None, None, 8, 0.0, ptr, None) == rt.ERR_INVALID
    sc = rt.Scene.reference(5, build_seed=1)
    fn = rt.load_lab().rt1w_lab_aov_deep_host
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.POINTER(rt.RenderParams), C.c_uint32, C.c_double, C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p]
    assert fn(sc._h, C.byref(p), 64, 0.0, ptr, None, None) == 0
    assert fn(sc._h, C.byref(p), 65, 0.0, ptr, None, None) == rt.ERR_INVALID
    for bad in (-1e-300, -1.0, float("nan"), float("inf"), float("-inf")):
        assert fn(sc._h, C.byref(p), 8, bad, ptr, None, None) == rt.ERR_INVALID, bad
    assert fn(None, C.byref(p), 8, 0.0, ptr, None, None) == rt.ERR_INVALID
    assert fn(sc._h, None, 8, 0.0, ptr, None, None) == rt.ERR_INVALID
    assert fn(sc._h, C.byref(p), 8, 0.0, None, None, None) == rt.ERR_INVALID
    with pytest.raises(rt.Rt1wError) as e:
        rt.aov_host(sc, 64, 64, 1, max_specular=65)
    assert e.value.code == rt.ERR_INVALID
    # the exported entries look at the two numbers before the context (one check, csrc/rt_aov_deep.h: rt_aov_deep_args_ok), so their
    # refusal shows without a GPU: the error names the arguments, a null context alone does not
    dev = C.c_void_p(16)
    for ms, mf in ((65, 0.0), (8, -1.0), (8, -1e-300), (8, float("nan")), (8, float("inf"))):
        for call in (lambda: lib.rt1w_render_aov_deep(None, C.byref(p), ms, mf, ptr, None),
                     lambda: lib.rt1w_render_aov_deep_device(None, C.byref(p), ms, mf, dev, None),
                     lambda: lib.rt1w_render_denoised_deep(None, C.byref(p), None, ms, mf, ptr, None)):
            assert call() == rt.ERR_INVALID and "max_specular" in rt.last_error() and "max_fuzz" in rt.last_error(), (ms, mf)
    assert lib.rt1w_render_aov_deep(None, C.byref(p), 64, 0.0, ptr, None) == rt.ERR_INVALID and "max_specular" not in rt.last_error()


def test_deep_kernels_use_no_scratch():
    """The deep kernels are built for two waves per SIMD so that nothing is spilled to scratch (built with scratch
    they returned wrong results on the GPU and the cause is open).  The build keeps the compiler's resource remarks of aov.hip in
    csrc/aov.resources and fails on scratch: that Makefile step is the enforcement.  This test only mirrors it, by reading the same
    file (six deep kernels, 0 bytes each, at most 256 VGPRs): it needs a library built by `make`, and it cannot see an aov.o that was
    produced some other way."""
    path = os.path.join(ROOT, "raytracing-1w_amd", "csrc", "aov.resources")
    assert os.path.exists(path), "csrc/aov.resources is written when aov.o is built"
    blocks = re.split(r"Function Name: ", open(path).read())[1:]
    deep = [b for b in blocks if b.split()[0].find("rt_aov_deep_kernel") >= 0]
    assert len(deep) == 6
    for b in deep:
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        vgprs = int(re.search(r" VGPRs: (\d+)", b).group(1))
        spilled = int(re.search(r"VGPRs Spill: (\d+)", b).group(1))
        print(b.split()[0][:60], "VGPRs", vgprs, "scratch", scratch, "VGPR spill", spilled)
        assert scratch == 0 and spilled == 0 and vgprs <= 256


def test_bench_tool_row_arithmetic(tmp_path):
    """tools/aov_bench.py --deep: a hand-made kernel_stats.csv and hand-made child reports through kernel_stats() and make_row().  The
    figures are chosen so that every quotient is exact; a first-hit or deep kernel count other than reps + 1 is refused (the one-call
    forms, which launch both kernels too, are timed in a child of their own)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("aov_bench", os.path.join(ROOT, "tools", "aov_bench.py"))
    ab = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ab)
    d = tmp_path / "host" / "123"
    d.mkdir(parents=True)
    (d / "123_kernel_stats.csv").write_text(
        '"Name","Calls","TotalDurationNs","AverageNs","Percentage","MinNs","MaxNs","StdDev"\n'
        '"void rtaov::rt_aov_kernel<V0>(RtSceneView, RtFrame, double*)",4,2000000,500000.0,10,1,2,0\n'
        '"void rtaovdeep::rt_aov_deep_kernel<V0>(RtSceneView, RtFrame, unsigned int, double, double*, unsigned long long*)",4,4000000,1000000.0,20,1,2,0\n'
        '"rt_jit_sorted",2,8000000,4000000.0,70,1,2,0\n')
    ks = ab.kernel_stats(str(tmp_path))
    assert len(ks) == 3
    res = {"aov_event_ms": [0.5] * 3, "aov_variant": 0, "aov_grid": 10, "aov_block": 256, "paths": 1000000,
           "beauty_kernel_ms": 4.0, "beauty_segments": 8000000, "beauty_sorted": 5, "beauty_segments_per_s": 2e9,
           "deep_event_ms": [1.0] * 3, "deep_segments": 1250000}
    calls = {"denoised_total_ms": [5.0, 6.0, 5.5], "denoised_deep_total_ms": [6.0, 7.5, 6.0]}
    row = ab.make_row(("c3", 5, 250, 250, 16), res, ks, 3, False, 8, calls)
    assert row["aov_calls"] == 4 and row["aov_kernel_ms_rocprof"] == 0.5 and row["aov_segments_per_s"] == 2e9 and row["aov_over_beauty"] == 1.0
    assert row["deep_kernel_ms_rocprof"] == 1.0 and row["deep_segments_per_sample"] == 1.25 and row["deep_segments_per_s"] == 1.25e9
    assert row["deep_over_beauty"] == 0.625 and row["max_specular"] == 8
    assert row["denoised_total_ms_median"] == 5.5 and row["denoised_deep_total_ms_median"] == 6.0
    assert row["denoised_total_ms_range"] == [5.0, 6.0] and row["denoised_deep_total_ms_range"] == [6.0, 7.5]
    assert row["deep_extra_beauty_samples_per_pixel"] == 2.0  # 0.5 ms over 4 ms / 16 samples
    first_only = ab.make_row(("c3", 5, 250, 250, 16), res, ks, 3)
    assert "deep_segments_per_s" not in first_only and first_only["aov_over_beauty"] == 1.0
    with pytest.raises(AssertionError):
        ab.make_row(("c3", 5, 250, 250, 16), res, ks, 4, False, 8, calls)  # 4 calls are not reps + 1 = 5


def test_reduces_to_first_hit(rt):
    """max_specular = 0 is the first-hit twin bit for bit on all eight arms, one ray per sample; on the arms whose material tables hold
    neither a Dielectric nor a Metal (read from rt1w_scene_copy_flat(what = 2)) so are the deep buffers at max_specular = 8."""
    W, H, spp = 96, 64, 3
    plain = []
    for arm in range(8):
        sc = rt.Scene.reference(arm, build_seed=1)
        kw = dict(tile=(7, 5, 61, 43), sample_offset=2, global_seed=5)
        first = rt.aov_host(sc, W, H, spp, **kw)
        zero, st = rt.aov_host(sc, W, H, spp, max_specular=0, max_fuzz=1.0, with_stats=True, **kw)
        assert _same(first, zero), arm
        assert st["segments"] == 61 * 43 * spp and np.all(st["lengths"] == 1)
        if not (_material_kinds(sc) & {2, 3}):
            plain.append(arm)
            deep, st = rt.aov_host(sc, W, H, spp, max_specular=8, max_fuzz=1.0, with_stats=True, **kw)
            assert _same(first, deep), arm
            assert st["segments"] == 61 * 43 * spp
    print("arms without Dielectric and Metal:", plain)
    assert plain, "no arm without specular materials: the second half of this test checked nothing"


WALLS = {"left": (0.9, 0.2, 0.1), "right": (0.15, 0.7, 0.25), "floor": (0.6, 0.6, 0.65), "ceiling": (2.5, 2.25, 2.0), "back": (0.3, 0.35, 1.7)}
BACKGROUND = (0.55, 0.7, 0.95)
TINT_SPHERE, TINT_BOX = (0.85, 0.8, 0.7), (0.75, 0.9, 0.6)


def _emitter_box_scene(rt, walls=WALLS, background=BACKGROUND, tints=(TINT_SPHERE, TINT_BOX)):
    """A box 0 .. 10 on every axis, open towards the camera (z = 0); its five walls are DiffuseLights of solid colours whose front faces
    look inwards (FlipFace where the rect's own normal looks outwards).  Inside: a Dielectric sphere, a Metal sphere of fuzz 0 and a Metal
    box of fuzz 0.3, which floats behind the spheres.  Camera and spheres lie in front of its front face, inside its extent in x and y,
    and nearer to its normal than acos(0.3): a fuzzy reflection at grazing incidence could point into the box, and a ray inside a
    mirror box stays there for many bounces.  No surface scatters diffusely, so the radiance of every sample is beta (.) emitted or beta (.) background."""
    s = rt.Scene(build_seed=1)
    light = {k: s.diffuse_light(s.solid_color(v)) for k, v in walls.items()}
    ids = [s.yz_rect(0, 10, 0, 10, 0, light["left"]),
           s.flip_face(s.yz_rect(0, 10, 0, 10, 10, light["right"])),
           s.xz_rect(0, 10, 0, 10, 0, light["floor"]),
           s.flip_face(s.xz_rect(0, 10, 0, 10, 10, light["ceiling"])),
           s.flip_face(s.xy_rect(0, 10, 0, 10, 10, light["back"])),
           s.sphere((3.5, 3.5, 3.0), 1.3, s.dielectric(1.5)),
           s.sphere((6.3, 6.3, 4.0), 1.4, s.metal(tints[0], 0.0)),
           s.aabox((2.0, 2.0, 7.0), (8.0, 8.0, 9.0), s.metal(tints[1], 0.3))]
    s.set_world(s.bvh_node(ids))
    s.set_lights([])
    s.set_background(background)
    s.set_camera((5.0, 5.0, -14.0), (5.0, 5.0, 5.0), (0, 1, 0), 50.0, 1.0, 0.0, 10.0, 0.0, 1.0)
    s.commit()
    return s


PATH_FRAME = dict(W=72, H=72, spp=16, max_specular=49, max_fuzz=1.0, max_depth=50)


def _path_agreement(rt, deep_of, sums_of):
    """deep albedo x spp against the raw sums of a beauty render, bit for bit on every pixel; the same for coverage.  deep_of(scene) ->
    the deep buffers, sums_of(scene) -> the RT1W_OUT_SUM frame with chunk = spp (one sequential sum per pixel)."""
    spp = PATH_FRAME["spp"]
    sc = _emitter_box_scene(rt)
    assert _material_kinds(sc) == {2, 3, 4}
    deep = deep_of(sc)
    sums = sums_of(sc)
    alb = deep[..., 0:3] * spp  # spp is a power of two: the product undoes the division exactly
    diff = alb.view(np.uint64) != sums.view(np.uint64)
    print("pixels", diff.shape[0] * diff.shape[1], "differing", int(diff.any(-1).sum()), "max |diff|", float(np.abs(alb - sums).max()))
    assert not diff.any()
    # everything that emits set to 1: the sum is the sum of the throughputs, again the deep albedo of that scene
    ones = {k: (1.0, 1.0, 1.0) for k in WALLS}
    sc1 = _emitter_box_scene(rt, walls=ones, background=(1.0, 1.0, 1.0))
    d1 = deep_of(sc1)
    assert _same(np.ascontiguousarray(d1[..., 0:3] * spp), sums_of(sc1))
    assert _same(np.ascontiguousarray(d1[..., 3:8]), np.ascontiguousarray(deep[..., 3:8]))  # the chains do not depend on the colours
    # coverage: with the emitters at 1, white mirrors (beta stays 1) and a black background a sample's radiance is 1 if its chain ends
    # on a wall (every wall shows its front face to the inside) and 0 if it leaves through the open side: the sum is the hit count
    sc2 = _emitter_box_scene(rt, walls=ones, background=(0.0, 0.0, 0.0), tints=((1.0, 1.0, 1.0), (1.0, 1.0, 1.0)))
    count = sums_of(sc2)
    assert np.all(count == np.round(count)) and np.all(count[..., 0] == count[..., 1]) and np.all(count[..., 0] == count[..., 2])
    assert np.array_equal(deep[..., 7] * spp, count[..., 0])
    assert (count[..., 0] == spp).any() and (count[..., 0] < spp).any()  # both walls and sky are seen


def test_chain_agrees_with_the_beauty_path(rt):
    """Pins the restated scatter code and its draws: in a scene where nothing scatters diffusely every sample's radiance is beta (.)
    emitted or beta (.) background, which is the deep albedo.  72 x 72 x 16 spp, max_fuzz 1, max_specular 49, max_depth 50, against
    the CPU build of the core (orc.flat_render, out_sum, chunk = spp).  No sample of the frame is still between specular surfaces
    after 49 bounces (checked here from the twin's per-sample ray counts), so no path is cut by max_depth either."""
    F = PATH_FRAME
    sc = _emitter_box_scene(rt)
    _, st = rt.aov_host(sc, F["W"], F["H"], F["spp"], max_specular=F["max_specular"], max_fuzz=F["max_fuzz"], with_stats=True)
    L = st["lengths"]
    print("rays per sample: max", int(L.max()), "mean", float(L.mean()), "histogram", np.bincount(L.ravel())[:12])
    assert L.max() < F["max_specular"] + 1, "a chain used all its bounces: change the geometry"
    assert L.max() >= 4 and st["segments"] == int(L.sum(dtype=np.uint64))
    _path_agreement(
        rt,
        lambda s: rt.aov_host(s, F["W"], F["H"], F["spp"], max_specular=F["max_specular"], max_fuzz=F["max_fuzz"]),
        lambda s: orc.flat_render(s, F["W"], F["H"], F["spp"], max_depth=F["max_depth"], chunk=F["spp"], out_sum=True)[0])


MIRROR_TINT, WALL_COLOUR = (0.8, 0.6, 0.9), (0.3, 0.55, 0.7)


def _mirror_scene(rt, fuzz):
    """Camera at the origin looking along +z at a mirror x, y in -1 .. 1 at z = 5; behind the camera a Lambertian wall at z = -3"""
    s = rt.Scene(build_seed=1)
    ids = [s.xy_rect(-1, 1, -1, 1, 5, s.metal(MIRROR_TINT, fuzz)),
           s.xy_rect(-50, 50, -50, 50, -3, s.lambertian(s.solid_color(WALL_COLOUR)))]
    s.set_world(s.bvh_node(ids))
    s.set_lights([])
    s.set_background((0.1, 0.2, 0.3))
    s.set_camera((0, 0, 0), (0, 0, 5), (0, 1, 0), 40.0, 1.0, 0.0, 5.0, 0.0, 1.0)
    s.commit()
    return s


def test_mirror_in_front_of_a_wall(rt):
    """An axis-aligned perfect mirror facing a wall of one colour, aperture 0, one sample per pixel.  Wherever the sample's camera ray
    meets the mirror (the first-hit albedo is the mirror's tint; every pixel whose whole jitter square projects into the mirror is
    among them) the deep albedo is tint (.) wall colour exactly, the normal the wall's (0, 0, 1), and the depth the camera-to-mirror
    distance plus the mirror-to-wall distance: with the unit direction's z = 5 / (camera-to-mirror distance), the reflected segment
    spans 8 in z, so it is 8 / z long.  This departs from taking the camera-to-mirror distance of the pixel's centre ray: the sample's
    ray is jittered inside the pixel, so the centre ray is not the sample's, and the first-hit buffer (code this feature does not
    touch) is what knows the sample's ray to 1e-12.  The depth is also inside the bounds the pixel's four corner rays give, computed from the camera
    alone.  A mirror of fuzz 0.1 is not followed at the default max_fuzz = 0."""
    W = H = 64
    sc = _mirror_scene(rt, 0.0)
    cb = np.frombuffer(sc.flat(6).tobytes()[:27 * 8], dtype=np.float64)
    origin, llc, hor, ver, lens = cb[0:3], cb[3:6], cb[6:9], cb[9:12], cb[21]
    assert lens == 0.0 and np.all(origin == 0.0)
    first = rt.aov_host(sc, W, H, 1)
    deep, st = rt.aov_host(sc, W, H, 1, max_specular=8, with_stats=True)
    on_mirror = np.all(first[..., 0:3] == np.array(MIRROR_TINT), axis=-1)
    inside = np.zeros((H, W), dtype=bool)
    lo, hi = np.full((H, W), np.inf), np.zeros((H, W))
    for j in range(H):
        for i in range(W):
            # slopes x / z, y / z of the four corner rays; the folded-out path is 13 * sqrt(1 + sx^2 + sy^2) long, largest at a
            # corner, smallest where |sx| and |sy| are (0 where the square straddles an axis)
            c = [llc + (i + a) / (W - 1) * hor + (j + b) / (H - 1) * ver - origin for a in (0.0, 1.0) for b in (0.0, 1.0)]
            sx, sy = np.array([d[0] / d[2] for d in c]), np.array([d[1] / d[2] for d in c])
            inside[j, i] = np.all(np.abs(5.0 * sx) < 1.0) and np.all(np.abs(5.0 * sy) < 1.0)
            nx = 0.0 if sx.min() < 0.0 < sx.max() else np.abs(sx).min()
            ny = 0.0 if sy.min() < 0.0 < sy.max() else np.abs(sy).min()
            lo[j, i] = (5.0 + 8.0) * np.sqrt(1.0 + nx * nx + ny * ny)
            hi[j, i] = (5.0 + 8.0) * np.sqrt(1.0 + (sx * sx + sy * sy).max())
    print("pixels on the mirror", int(on_mirror.sum()), "wholly inside", int(inside.sum()))
    assert inside.sum() >= 100 and np.all(on_mirror[inside])
    m = deep[on_mirror]
    assert np.all(m[:, 0:3] == np.array(MIRROR_TINT) * np.array(WALL_COLOUR))
    assert np.all(np.abs(m[:, 3:6] - np.array([0.0, 0.0, 1.0])) <= 1e-12)
    assert np.all(m[:, 7] == 1.0)
    l1 = first[on_mirror][:, 6]
    want = l1 + 8.0 / (5.0 / l1)
    rel = np.abs(m[:, 6] - want) / want
    print("depth: max relative difference", float(rel.max()))
    assert np.all(rel <= 1e-12)
    assert np.all(deep[inside][:, 6] >= lo[inside] * (1 - 1e-12)) and np.all(deep[inside][:, 6] <= hi[inside] * (1 + 1e-12))
    assert np.all(st["lengths"][on_mirror] == 2) and np.all(st["lengths"][~on_mirror] == 1)
    assert _same(np.ascontiguousarray(deep[~on_mirror]), np.ascontiguousarray(first[~on_mirror]))
    # fuzz 0.1: not specular at the default max_fuzz, followed at max_fuzz = 0.1
    rough = _mirror_scene(rt, 0.1)
    f2 = rt.aov_host(rough, W, H, 1)
    assert _same(rt.aov_host(rough, W, H, 1, max_specular=8), f2)
    assert not _same(rt.aov_host(rough, W, H, 1, max_specular=8, max_fuzz=0.1), f2)


def _disp(c):
    return np.sqrt(np.clip(c, 0.0, 0.999))  # the displayed value, src/color.rs:56-65 (as test_denoise.py)


def _mse(a, b, mask=None):
    d = (_disp(a) - _disp(b)) ** 2
    return float(np.mean(d if mask is None else d[mask]))


@pytest.mark.parametrize("arm,max_fuzz", sorted(MEASURED_RATIO))
def test_quality_inside_glass_and_mirrors(rt, arm, max_fuzz):
    """The reason for the feature.  A 16 spp frame filtered with the deep guides against the same frame filtered with the first-hit
    guides (the behaviour before this feature), both against a converged frame of another seed, in the mean squared error of the
    displayed values: over M, the pixels whose deep buffers differ from their first-hit buffers, and over the whole frame.  Measured
    when written (twins, default parameters; M / all): Cornell 96 x 96 0.2593 / 0.6514; random_scene 128 x 72 0.4216 / 0.7308 at max_fuzz 0
    and at max_fuzz 0.5 alike: the reference draws the fuzz of that scene's small metal spheres from 0.5 .. 1 (main.rs:245), so 0.5
    admits no sphere that 0 does not; the big metal sphere has fuzz 0."""
    w, h = QUALITY_FRAME[arm]
    sc = rt.Scene.reference(arm, build_seed=1)
    noisy, _ = orc.flat_render(sc, w, h, 16)
    ref = np.load(os.path.join(GOLD, f"denoise_ref_arm{arm}.npy"))
    assert ref.shape == noisy.shape
    first = rt.aov_host(sc, w, h, 16)
    deep = rt.aov_host(sc, w, h, 16, max_specular=MAX_SPECULAR, max_fuzz=max_fuzz)
    M = np.any(first.view(np.uint64) != deep.view(np.uint64), axis=-1)
    assert M.sum() >= 100
    d_first, d_deep = rt.denoise_host(noisy, first), rt.denoise_host(noisy, deep)
    r_m = _mse(d_deep, ref, M) / _mse(d_first, ref, M)
    r_all = _mse(d_deep, ref) / _mse(d_first, ref)
    print(f"arm {arm} max_fuzz {max_fuzz}: |M| {int(M.sum())} of {w * h}; on M: noisy {_mse(noisy, ref, M):.6g} first-hit {_mse(d_first, ref, M):.6g} "
          f"deep {_mse(d_deep, ref, M):.6g} ratio {r_m:.4f}; whole frame ratio {r_all:.4f}")
    assert r_m < 1.0
    assert r_m <= (MEASURED_RATIO[(arm, max_fuzz)][0] + 1.0) / 2.0
    assert r_all <= 1.0


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


DEEP_CASES = [(ms, mf) for ms in (1, 4, 16) for mf in (0.0, 0.5)]


@pytest.mark.gpu
def test_gpu_deep_bit_identical_to_the_twin(rt, gpu_ctx_factory):
    """All eight arms, max_specular in {1, 4, 16} x max_fuzz in {0, 0.5}; small crops at several spp, non-zero sample_offset and
    global_seed; every variant valid for the scene; arms 0 and 7 under the SAH tree and the near-far order.  stats.segments is the
    twin's count of rays."""
    W, H = 96, 64
    for arm in range(8):
        sc = rt.Scene.reference(arm, build_seed=1)
        ctx = gpu_ctx_factory(sc)
        for n, (spp, tile, so, gs) in enumerate(((1, (0, 0, W, H), 0, 0), (3, (13, 7, 41, 29), 5, 11), (8, (40, 20, 17, 9), 1000, 3))):
            for ms, mf in DEEP_CASES:
                kw = dict(max_specular=ms, max_fuzz=mf, tile=tile, sample_offset=so, global_seed=gs)
                a, st = ctx.render_aov_deep(W, H, spp, with_stats=True, **kw)
                b, sb = rt.aov_host(sc, W, H, spp, with_stats=True, **kw)
                assert _same(a, b), (arm, spp, tile, ms, mf)
                assert st["segments"] == sb["segments"] and st["paths"] == tile[2] * tile[3] * spp, (arm, spp, tile, ms, mf)
        for v in _valid_variants(sc.info()):
            for ms, mf in DEEP_CASES:
                kw = dict(max_specular=ms, max_fuzz=mf, tile=(5, 3, 37, 21), sample_offset=7, global_seed=2, variant=v)
                a, st = ctx.render_aov_deep(W, H, 2, with_stats=True, **kw)
                b, sb = rt.aov_host(sc, W, H, 2, with_stats=True, **kw)
                assert st["variant"] == v and st["segments"] == sb["segments"]
                assert _same(a, b), (arm, v, ms, mf)
        ctx.close()
    for arm in (0, 7):
        for mode in ("sah", "near_far"):
            sc = rt.Scene.reference(arm, build_seed=1)
            sc = sc.set_bvh_build("sah") if mode == "sah" else sc.set_walk_order(True)
            ctx = gpu_ctx_factory(sc)
            for ms, mf in DEEP_CASES:
                kw = dict(max_specular=ms, max_fuzz=mf, tile=(8, 8, 48, 40), sample_offset=3, global_seed=9)
                a, st = ctx.render_aov_deep(W, H, 4, with_stats=True, **kw)
                b, sb = rt.aov_host(sc, W, H, 4, with_stats=True, **kw)
                assert st["variant"] == sc.info()["variant"] and st["segments"] == sb["segments"]
                assert _same(a, b), (arm, mode, ms, mf)
            ctx.close()


@pytest.mark.gpu
def test_gpu_chain_agrees_with_the_beauty_kernels(rt, gpu_ctx_factory):
    """test_chain_agrees_with_the_beauty_path on the device: rt1w_render_aov_deep against the RT1W_OUT_SUM frame of rt1w_render with
    chunk = spp, bit for bit on every pixel."""
    F = PATH_FRAME
    ctxs = {}

    def ctx_of(s):
        if id(s) not in ctxs:
            ctxs[id(s)] = (gpu_ctx_factory(s), s)
        return ctxs[id(s)][0]
    _path_agreement(
        rt,
        lambda s: ctx_of(s).render_aov_deep(F["W"], F["H"], F["spp"], max_specular=F["max_specular"], max_fuzz=F["max_fuzz"]),
        lambda s: ctx_of(s).render(F["W"], F["H"], F["spp"], max_depth=F["max_depth"], chunk=F["spp"], out_sum=True)[0])


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
def test_gpu_deep_entry_forms_agree(rt, gpu_ctx_factory):
    """Tile, strip-interleaved tile and full frame agree; the device entry equals the host entry; rt1w_render_denoised_deep equals
    rt1w_render_device + rt1w_render_aov_deep_device + rt1w_denoise_device; a render and a first-hit AOV call before and after the deep
    calls are unchanged; the argument errors that need a context."""
    W, H, spp = 80, 60, 3
    for arm in (0, 5, 7):
        sc = rt.Scene.reference(arm, build_seed=1, aspect_ratio=W / H)
        ctx = gpu_ctx_factory(sc)
        img0, s0 = ctx.render(W, H, spp, global_seed=4)
        first0 = ctx.render_aov(W, H, spp, sample_offset=2, global_seed=4)
        kw = dict(max_specular=6, max_fuzz=0.5, sample_offset=2, global_seed=4)
        full, sf = ctx.render_aov_deep(W, H, spp, with_stats=True, **kw)
        assert not _same(full, first0)
        tile = ctx.render_aov_deep(W, H, spp, tile=(10, 20, 30, 25), **kw)
        assert _same(tile, np.ascontiguousarray(full[20:45, 10:40]))
        rows = [4 + (r // 4) * 12 + r % 4 for r in range(20)]  # rank 1 of 3 with strips of 4 rows
        strip = ctx.render_aov_deep(W, H, spp, tile=(0, 4, W, 20), strips=(4, 12), **kw)
        assert _same(strip, np.ascontiguousarray(full[rows]))
        dev = _DeviceBuffer(H * W * 8 * 8)
        st = ctx.render_aov_deep_device(dev.ptr, W, H, spp, **kw)
        assert st["paths"] == W * H * spp and st["segments"] == sf["segments"] > st["paths"] and st["kernel_ms"] > 0
        assert _same(dev.to_host((H, W, 8)), full)
        dev.free()
        # the one-call form against the three device entries composed
        npix = W * H
        d_frame, d_aov, d_out = _DeviceBuffer(npix * 3 * 8), _DeviceBuffer(npix * 8 * 8), _DeviceBuffer(npix * 3 * 8)
        ctx.render_device(d_frame.ptr, W, H, spp, global_seed=4)
        ctx.render_aov_deep_device(d_aov.ptr, W, H, spp, max_specular=6, max_fuzz=0.5, global_seed=4)
        ctx.denoise_device(d_frame.ptr, d_aov.ptr, d_out.ptr, W, H)
        composed = d_out.to_host((H, W, 3))
        for b in (d_frame, d_aov, d_out):
            b.free()
        one, s1 = ctx.render_denoised_deep(W, H, spp, max_specular=6, max_fuzz=0.5, global_seed=4, with_stats=True)
        assert _same(one, composed)
        assert s1["paths"] == W * H * spp and s1["block"] == 256
        assert not _same(one, ctx.render_denoised(W, H, spp, global_seed=4))
        assert _same(ctx.render_denoised_deep(W, H, spp, max_specular=0, global_seed=4), ctx.render_denoised(W, H, spp, global_seed=4))
        dn = dict(iterations=3, keep_albedo=True, sigma_colour=2.0)
        deep_gs4 = ctx.render_aov_deep(W, H, spp, max_specular=6, max_fuzz=0.5, global_seed=4)
        assert _same(ctx.render_denoised_deep(W, H, spp, max_specular=6, max_fuzz=0.5, global_seed=4, denoise=dn), ctx.denoise(img0, deep_gs4, **dn))
        # nothing is left behind
        img1, s1b = ctx.render(W, H, spp, global_seed=4)
        assert _same(img0, img1) and s0["segments"] == s1b["segments"]
        assert _same(ctx.render_aov(W, H, spp, sample_offset=2, global_seed=4), first0)
        # refusals
        for ms, mf in ((65, 0.0), (8, -0.5), (8, float("nan")), (8, float("inf"))):
            with pytest.raises(rt.Rt1wError) as e:
                ctx.render_aov_deep(W, H, spp, max_specular=ms, max_fuzz=mf)
            assert e.value.code == rt.ERR_INVALID and ("max_specular" in str(e.value) or "max_fuzz" in str(e.value))
            with pytest.raises(rt.Rt1wError) as e:
                ctx.render_denoised_deep(W, H, spp, max_specular=ms, max_fuzz=mf)
            assert e.value.code == rt.ERR_INVALID
        buf = np.zeros((H, W, 8))
        p = ctx._params(W, H, spp, 50, None, 0, 0, 0, False)
        assert rt._lib.rt1w_render_aov_deep(ctx._h, C.byref(p), 8, 0.0, None, None) == rt.ERR_INVALID
        assert rt._lib.rt1w_render_aov_deep_device(ctx._h, C.byref(p), 8, 0.0, None, None) == rt.ERR_INVALID
        for flag in (rt.OUT_SUM, rt.UNSORTED, rt.GENERIC, rt.RNG_REFERENCE, rt.OUT_FRAME, 1 << 20):
            p.flags = flag
            assert rt._lib.rt1w_render_aov_deep(ctx._h, C.byref(p), 8, 0.0, buf.ctypes.data_as(C.c_void_p), None) == rt.ERR_INVALID
        p.flags = 0
        p.precision = 1
        assert rt._lib.rt1w_render_aov_deep(ctx._h, C.byref(p), 8, 0.0, buf.ctypes.data_as(C.c_void_p), None) == rt.ERR_UNSUPPORTED
        for flags, name in ((rt.OUT_SUM, "RT1W_OUT_SUM"), (rt.OUT_FRAME, "RT1W_OUT_FRAME"), (rt.RNG_REFERENCE, "RT1W_RNG_REFERENCE"),
                            (rt.PROBE_COHERENT, "RT1W_PROBE_COHERENT")):
            with pytest.raises(rt.Rt1wError) as e:
                ctx.render_denoised_deep(W, H, spp, flags=flags)
            assert e.value.code == rt.ERR_INVALID and name in str(e.value)
        with pytest.raises(rt.Rt1wError) as e:
            ctx.render_denoised_deep(W, H, spp, tile=(0, 0, W, 30), strips=(10, 20))
        assert e.value.code == rt.ERR_INVALID and "strip_rows" in str(e.value)
        with pytest.raises(rt.Rt1wError) as e:
            ctx.render_denoised_deep(W, H, spp, precision=1)
        assert e.value.code == rt.ERR_INVALID and "RT1W_PRECISION_F32" in str(e.value)
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("arm,size", [(5, 600), (7, 800)])
def test_gpu_deep_full_frames(rt, gpu_ctx_factory, arm, size):
    """C3 (Cornell 600 x 600) and C4 (final_scene 800 x 800) at 16 spp, max_specular = 8: the sanity bounds of the first-hit full frames,
    and equal to the twin's frame on 4096 seeded pixels plus the four corners, with the twin's count of rays."""
    sc = rt.Scene.reference(arm, build_seed=1)
    ctx = gpu_ctx_factory(sc)
    a, st = ctx.render_aov_deep(size, size, 16, max_specular=8, with_stats=True)
    ctx.close()
    print(f"arm {arm} {size}x{size}x16 deep AOV: kernel {st['kernel_ms']:.2f} ms, variant {st['variant']}, grid {st['grid']} x {st['block']}, "
          f"{st['segments']} rays ({st['segments'] / st['paths']:.3f} per sample), {st['segments'] / st['kernel_ms'] / 1e3:.1f} Msegments/s")
    cov = a[..., 7]
    assert np.all((cov >= 0) & (cov <= 1))
    assert np.all(np.isfinite(a[..., [0, 1, 2, 3, 4, 5, 7]]))
    assert np.all(np.isfinite(a[..., 6][cov > 0])) and np.all(np.isinf(a[..., 6][cov == 0]))
    assert np.all(np.linalg.norm(a[..., 3:6], axis=-1) <= 1 + 1e-12)
    assert st["paths"] == size * size * 16 < st["segments"] <= 9 * st["paths"]
    rng = np.random.default_rng(2010)
    ys = np.concatenate([rng.integers(0, size, 4096), [0, 0, size - 1, size - 1]])
    xs = np.concatenate([rng.integers(0, size, 4096), [0, size - 1, 0, size - 1]])
    twin, sb = rt.aov_host(sc, size, size, 16, max_specular=8, with_stats=True)
    assert st["segments"] == sb["segments"]
    assert _same(np.ascontiguousarray(a[ys, xs]), np.ascontiguousarray(twin[ys, xs]))
