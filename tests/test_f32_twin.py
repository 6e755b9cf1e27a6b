"""The single-precision kernels (RT1W_PRECISION_F32) against their CPU twin, bit for bit.

Three builds of one text (csrc/rt_core.h and the kernels' work decomposition, compiled with `double` redefined to `float`):

  twin     oracle/oracle_flat_f32.cpp -> liborc_flat_f32.so: the host build.  sin, cos, atan2, acos and ln of a float are the 64-bit
           functions of include/rt1w_num.h, rounded once.  It walks the records of the product's own f64 -> f32 conversion
           (csrc/rt_f32_scene.h) and keeps the pixel sums in 64 bits as the kernels do.
  exact    csrc/f32_exact.hip in librt1w_lab.so: the ten f32 kernels compiled for the GPU with -DRT_F32_ELEMENTARY_F64 -- the same five
           functions in 64 bits -- and otherwise the product's options.  rt.f32_exact() makes f32 renders run them through the
           product's own plan, launch, resolve and stats.
  product  csrc/context_f32.hip: the same kernels with the device's single-precision sinf, cosf, atan2f, acosf, logf.

exact == twin is asserted bit for bit with equal segment counts, on every one of the ten kernel instantiations.  product differs from
exact in the five functions only; they are bounded on their own (test_the_five_elementary_functions_on_the_device), product == exact
is asserted bit for bit where a frame calls none of them (max_depth 1, arms without media), and statistically at full depth.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import orc
from test_kernel_choice import SIZES

HERE = os.path.dirname(os.path.abspath(__file__))
ULPS = os.path.join(HERE, "golden", "f32_elementary_ulps.json")
_P = C.c_void_p

# the shapes of test_render_passes.py: 128 x 96 pixels are 294 912 B of partial sums per chunk, so 10 samples at chunk 1 and a 1 MiB
# budget run as 3 + 3 + 3 + 1
W, H, SPP = 128, 96, 10

_SCENES = {}
_CPU = {}


def scene(rt, arm):
    assert arm in SIZES
    if arm not in _SCENES:
        _SCENES[arm] = rt.Scene.reference(arm, build_seed=1)
    return _SCENES[arm]


def cpu(rt, arm, width=W, height=H, spp=SPP, chunk=1, **kw):
    """orc.flat_f32_render of one key, computed once for the module"""
    key = (arm, width, height, spp, chunk, tuple(sorted(kw.items())))
    if key not in _CPU:
        _CPU[key] = orc.flat_f32_render(scene(rt, arm), width, height, spp, chunk=chunk, **kw)
    return _CPU[key]


def same(img, st, ref):
    """bit for bit, equal segment counts"""
    want, sw = ref
    return st["segments"] == sw["segments"] and np.array_equal(img, want, equal_nan=True)


def first_difference(img, want):
    d = np.argwhere(~((img == want) | (np.isnan(img) & np.isnan(want))))
    return None if not len(d) else (len(d), tuple(int(v) for v in d[0]), float(img[tuple(d[0])]), float(want[tuple(d[0])]))


# ------------------------------------------------------------------------------------------------------------------- CPU tier

F32_BIT, SORTED_BIT, PW_BIT, SS_BIT = 32, 1, 128, 512   # rt1w_stats.sorted (include/rt1w.h)
BVH_KINDS = (0, 1)                                      # rt_flat.h: RT_BVH2, RT_BVH1 (`kind(i) <= RT_BVH1` is a BVH node)
NODE64 = np.dtype([("kind", "<u4"), ("skip", "<u4"), ("d", "<f8", 6), ("b", "<u4"), ("mat", "<u4"), ("e", "<f8", 3), ("a", "<u4"), ("pad", "<u4")])
NODE32 = np.dtype([("kind", "<u4"), ("skip", "<u4"), ("d", "<f4", 6), ("b", "<u4"), ("mat", "<u4"), ("e", "<f4", 3), ("a", "<u4"), ("pad", "<u4")])


def _layouts_are_the_headers():
    lib = orc.flat_f32_lib()
    assert orc.B.orcflat_sizeof(0) == NODE64.itemsize and lib.orcflat_f32_sizeof(0) == NODE32.itemsize
    assert orc.B.orcflat_sizeof(1) == 48 and lib.orcflat_f32_sizeof(1) == 32


def check_conversion(sc, label):
    """The properties of csrc/rt_f32_scene.h on one committed scene; expected values from numpy float64 and np.nextafter."""
    n = sc.info()["n_nodes"]
    for what in (0, 1):
        a = sc.flat(what)
        src = np.frombuffer(a.tobytes(), dtype=NODE64)[:n if what == 0 else None]
        dst = np.frombuffer(orc.flat_f32_records(sc, what).tobytes(), dtype=NODE32)
        assert len(src) == len(dst), (label, what)
        for f in ("kind", "skip", "b", "mat", "a", "pad"):
            assert np.array_equal(src[f], dst[f]), (label, what, f)                      # integer fields are untouched
        assert np.array_equal(dst["e"], src["e"].astype(np.float32), equal_nan=True), (label, what, "e")
        box = np.isin(src["kind"] & 0xFF, BVH_KINDS)
        plain = ~box
        assert np.array_equal(dst["d"][plain], src["d"][plain].astype(np.float32), equal_nan=True), (label, what, "d")
        lo, hi = src["d"][box][:, :3], src["d"][box][:, 3:]
        mag = np.maximum(1.0, np.maximum(np.abs(lo), np.abs(hi)))
        wlo, whi = lo - 1e-5 * mag, hi + 1e-5 * mag                                       # the widened f64 box
        glo, ghi = dst["d"][box][:, :3], dst["d"][box][:, 3:]
        assert (glo.astype(np.float64) <= wlo).all() and (ghi.astype(np.float64) >= whi).all(), (label, what, "box does not contain")
        # the nearest floats outward: the bound is the largest float <= wlo (smallest >= whi): one float further in would be inside
        assert (np.nextafter(glo, np.float32(np.inf)).astype(np.float64) > wlo).all(), (label, what, "lower bound not tight")
        assert (np.nextafter(ghi, np.float32(-np.inf)).astype(np.float64) < whi).all(), (label, what, "upper bound not tight")
    info = sc.info()
    mats = np.frombuffer(sc.flat(2).tobytes(), dtype=np.dtype([("d", "<f8", 4), ("kind", "<u4"), ("tex", "<u4"), ("pad", "<u4", 2)]))
    m32 = np.frombuffer(orc.flat_f32_records(sc, 2).tobytes(), dtype=np.dtype([("d", "<f4", 4), ("kind", "<u4"), ("tex", "<u4"), ("pad", "<u4", 2)]))
    assert len(mats) == len(m32) == info["n_materials"], label
    assert np.array_equal(m32["d"], mats["d"].astype(np.float32)) and np.array_equal(m32["kind"], mats["kind"]) and np.array_equal(m32["tex"], mats["tex"]), label
    t64 = np.dtype([("d", "<f8", 3), ("kind", "<u4"), ("a", "<u4"), ("b", "<u4"), ("c", "<u4"), ("pad", "<u4", 2)])
    t32 = np.dtype([("d", "<f4", 3), ("kind", "<u4"), ("a", "<u4"), ("b", "<u4"), ("c", "<u4"), ("pad", "<u4", 2)])
    assert orc.B.orcflat_sizeof(2) == t64.itemsize and orc.flat_f32_lib().orcflat_f32_sizeof(2) == t32.itemsize
    a, b = np.frombuffer(sc.flat(3).tobytes(), dtype=t64), np.frombuffer(orc.flat_f32_records(sc, 3).tobytes(), dtype=t32)
    assert len(a) == len(b) == info["n_textures"], label
    assert np.array_equal(b["d"], a["d"].astype(np.float32)), label
    for f in ("kind", "a", "b", "c"):
        assert np.array_equal(a[f], b[f]), (label, f)
    # camera (7 vectors, lens radius, shutter) and background: 24 + 3 numbers, each the plain rounding
    cam = np.frombuffer(sc.flat(6).tobytes()[:27 * 8], dtype="<f8")
    c32 = np.frombuffer(orc.flat_f32_records(sc, 5).tobytes(), dtype="<f4")
    assert len(c32) == 27 and np.array_equal(c32, cam.astype(np.float32)), label
    # Perlin records: 768 vectors' components rounded, permutation tables copied
    p64, p32 = sc.flat(4), orc.flat_f32_records(sc, 4)
    if len(p64):
        rec64, rec32 = orc.B.orcflat_sizeof(3), orc.flat_f32_lib().orcflat_f32_sizeof(3)
        assert len(p64) % rec64 == 0 and len(p32) // rec32 == len(p64) // rec64, label
        for i in range(len(p64) // rec64):
            v64 = np.frombuffer(p64[i * rec64:i * rec64 + 768 * 8].tobytes(), dtype="<f8")
            v32 = np.frombuffer(p32[i * rec32:i * rec32 + 768 * 4].tobytes(), dtype="<f4")
            assert np.array_equal(v32, v64.astype(np.float32)), label
            assert np.array_equal(p64[i * rec64 + 768 * 8:(i + 1) * rec64], p32[i * rec32 + 768 * 4:(i + 1) * rec32]), label


@pytest.mark.parametrize("arm", range(8))
def test_conversion_properties_on_the_reference_arms(rt, arm):
    """csrc/rt_f32_scene.h on every reference arm: every f32 BVH box contains its f64 box widened by 1e-5 * max(1, |lo|, |hi|) per axis and
    is the tightest float box that does (no bound is tighter, none is a float further out than needed); every other number is the plain
    rounding of its f64 value; integer fields are untouched."""
    _layouts_are_the_headers()
    check_conversion(rt.Scene.reference(arm, build_seed=1), arm)


@pytest.mark.parametrize("seed", (1000, 1003, 1011, 1020, 1042))
def test_conversion_properties_on_random_scene_graphs(rt, seed):
    from dual import random_scene_pair
    prod, _ = random_scene_pair(seed)
    check_conversion(prod, seed)


VALID = {5: (0, 1, 2, 3), 0: (1, 2, 3, 5), 6: (1, 3), 7: (1, 3), 3: (1, 2, 3), 2: (1, 2, 3)}


@pytest.mark.parametrize("arm", sorted(VALID))
def test_twin_every_valid_variant_gives_identical_bits(rt, arm):
    """As test_flat_vs_literal.py for the f64 core: the feature-specialised variants differ in the code they leave out, not in a result."""
    sc = rt.Scene.reference(arm, build_seed=1)
    ref = None
    for v in VALID[arm]:
        img, st = orc.flat_f32_render(sc, 48, 32, 4, chunk=1, variant=v)
        ref = ref or (img, st)
        assert same(img, st, ref), (arm, v, first_difference(img, ref[0]))


@pytest.mark.parametrize("build", ("best_axis", "sah"))
def test_twin_pair_walk_equals_the_classic_walk(rt, build):
    """random_scene in f32: the pair walk over the widened f32 boxes gates the same spheres as the one-entry-per-step walk -- same frame,
    same segments, on the best-axis tree and the SAH tree; stack (the kernel's 12 entries) and queue are bound-checked."""
    sc = rt.Scene.reference(0, build_seed=1, aspect_ratio=1.5)
    if build == "sah":
        sc = sc.set_bvh_build("sah")
    a = orc.flat_f32_render(sc, 48, 32, 8, chunk=1)
    b, sb = orc.flat_f32_render(sc, 48, 32, 8, chunk=1, pair_walk=True)
    assert same(b, sb, a), first_difference(b, a[0])


def test_twin_tile_with_sample_offset_equals_the_full_render(rt):
    """raw sums (out_sum), chunk 1: samples 3..7 of a tile are the difference-free continuation of samples 0..2 -- the tile's pixels of
    the 8-sample frame are the 3-sample sums plus the 5-sample sums at offset 3, added in the same order (64-bit sums: exact here only if
    the twin adds chunk sums in sample order)."""
    for arm in (5, 7):
        sc = rt.Scene.reference(arm, build_seed=1)
        tile = (8, 4, 24, 16)
        full, _ = orc.flat_f32_render(sc, 48, 32, 8, chunk=1, out_sum=True)
        t, _ = orc.flat_f32_render(sc, 48, 32, 8, chunk=1, out_sum=True, tile=tile)
        assert np.array_equal(t, full[4:20, 8:32], equal_nan=True), arm
        lo, _ = orc.flat_f32_render(sc, 48, 32, 1, chunk=1, out_sum=True, tile=tile)
        hi, _ = orc.flat_f32_render(sc, 48, 32, 1, chunk=1, out_sum=True, tile=tile, sample_offset=1)
        two, _ = orc.flat_f32_render(sc, 48, 32, 2, chunk=1, out_sum=True, tile=tile)
        assert np.array_equal(lo + hi, two, equal_nan=True), arm


def test_twin_against_the_f32_literal_oracle(rt):
    """The twin against orc.OracleScene(f32=True), the literal recursive oracle with `type Float = f32`: the CPU tier's first check of the
    f32 core.  The twin may differ from it in three ways only -- the widened boxes, the 64-bit sums, iterative against recursive evaluation
    order -- so it meets the bounds the project sets for the GPU in test_f32_mode_against_the_f32_oracle: segments per path and frame mean
    within 0.5 %, every block's mean within 2.5 % (+ 0.002 for the near-black blocks).  The committed cases random_scene_300x200x64 and
    final_scene_200x200x64 of tests/golden/oracle_f32_blocks.json take seconds through the twin; cornell_600x600x256 (92 M paths) does
    not fit a CPU test, so Cornell is rendered live by both at 120 x 120 x 256 with 20-pixel blocks: 102 400 paths per block against
    the golden case's 2 560 000, a noisier block under the same bound, not a wider bound.
    Worst values measured (worst block, segments, mean): random_scene 0.0002, -0.00014, -0.00000; final_scene 0.0068, -0.00004,
    -0.00005; Cornell live 0.0002, -0.00018, -0.00000."""
    gold = json.load(open(os.path.join(HERE, "golden", "oracle_f32_blocks.json")))["cases"]
    cases = []
    for name in ("random_scene_300x200x64", "final_scene_200x200x64"):
        g = gold[name]
        cases.append((name, g["arm"], g["aspect"], g["W"], g["H"], g["spp"], g["block"], np.array(g["block_means_bottom_up"]), g["segments"], g["mean"]))
    lit, sl = orc.OracleScene(5, build_seed=1, f32=True).render(120, 120, 256)
    cases.append(("cornell_120x120x256_live", 5, None, 120, 120, 256, 20, lit.reshape(6, 20, 6, 20, 3).mean(axis=(1, 3)), sl["segments"], float(lit.mean())))
    for name, arm, aspect, w, h, spp, blk, want, segments, mean in cases:
        img, st = orc.flat_f32_render(rt.Scene.reference(arm, build_seed=1, aspect_ratio=aspect), w, h, spp, pair_walk=(arm == 0))
        assert np.isfinite(img).all(), name
        got = img.reshape(h // blk, blk, w // blk, blk, 3).mean(axis=(1, 3))
        rel = np.abs(got - want) / (np.abs(want) + 0.08)
        print(name, "worst block %.4f  segments %+.5f  mean %+.5f" % (float(rel.max()), st["segments"] / segments - 1.0, float(img.mean() / mean - 1.0)))
        assert abs(st["segments"] / segments - 1.0) < 0.005, (name, st["segments"], segments)
        assert abs(img.mean() / mean - 1.0) < 0.005, (name, img.mean(), mean)
        assert rel.max() < 0.025, (name, float(rel.max()))


def draw_probe(lib, bits):
    out = np.empty(12, dtype=np.float64)
    lib.orcflat_draw_probe.argtypes = [C.c_uint64, _P]
    lib.orcflat_draw_probe(bits, out.ctypes.data_as(_P))
    return out


def test_draws_that_round_to_one_stay_in_range(rt):
    """A 53-bit draw r < 1 of the generator would round to 1.0f where the f32 core assigns it (r >= 1 - 2^-25), which rand's own
    `gen::<f32>()` never returns; the draw contract of the f32 builds (include/rt1w_num.h, tests/test_f32_draws.py) makes it 1 - 2^-24
    instead, and a range draw that rounds onto `high` is drawn again.  The smallest draw is 0 in both precisions.  Every consumer of a
    uniform draw -- the cosine direction, random_to_sphere, the light rectangle's point, the free flight -ln(r) / density, the Schlick
    comparison, the lens disk and the shutter time -- is fed the largest draw (all mantissa bits set) and 0 through the f32 twin
    (orcflat_draw_probe).  Each result must be finite wherever the f64 core's is, and lie inside what the f64 core returns for the
    64-bit draws the f32 draw may stand for -- the contract keeps it within 2^-24 of the 64-bit draw, so for the largest: that draw, its
    three neighbours, 1 - 2^-24 and 1 - 2^-23; for 0: the draw and its three neighbours -- widened by 4 f32 roundings (4 * 2^-24 *
    max(1, |value|): 2 pi r and the function's).  The free flight of the draw 0 is +inf in both cores, as the reference's ln(0) makes
    it: the medium is left without scattering.  The lens disk and the shutter time reject the largest draw and draw on from the
    stream: finite, inside the disk, and in [0, 1) as floats."""
    f32, f64 = orc.flat_f32_lib(), orc.B
    names = ("cos.x", "cos.y", "cos.z", "sph.x", "sph.y", "sph.z", "light", "flight", "draw", "lens.x", "lens.y", "time")
    top = (1 << 64) - 1
    step = 1 << 11
    stands_for = [top - k * step for k in range(4)] + [((1 << 53) - (1 << 29)) << 11, ((1 << 53) - (1 << 30)) << 11]
    for label, around in (("largest", stands_for), ("smallest", [k * step for k in range(4)])):
        got = draw_probe(f32, around[0])
        ref = np.array([draw_probe(f64, b) for b in around])
        for i, name in enumerate(names):
            if name.startswith("lens") or (name == "time" and label == "largest"):   # the rejection draws on from the stream
                assert np.isfinite(got[i]) and abs(got[i]) < 1.0, (label, name, got[i])
                continue
            if not np.isfinite(ref[0, i]):
                assert got[i] == ref[0, i], (label, name, got[i], ref[0, i])
                continue
            assert np.isfinite(got[i]), (label, name, got[i])
            fin = ref[:, i][np.isfinite(ref[:, i])]
            tol = 4 * 2.0 ** -24 * max(1.0, float(np.abs(fin).max()))
            assert fin.min() - tol <= got[i] <= fin.max() + tol, (label, name, got[i], fin.min(), fin.max())
        # the unit draw and the shutter time are half-open as floats; the light's coordinate is shown before its caller's retry (rt_core.h)
        assert 0.0 <= got[8] < 1.0 and 0.0 <= got[11] < 1.0 and 213.0 <= got[6] <= 343.0, (label, got)
        assert got[8] == np.float32(got[8]) and got[11] == np.float32(got[11])
    assert draw_probe(f32, top)[8] == 1.0 - 2.0 ** -24 and draw_probe(f32, top)[2] == 2.0 ** -12   # the cosine lobe leaves the surface: z = sqrt(1 - r2)


# ------------------------------------------------------------------------------------------------------------------- GPU tier

# the ten f32 instantiations (csrc/rt_f32_kernels.h): (arm, render flags, pair walk on the twin) -> (variant, stats.sorted)
FORMS = [
    ("plain V0", 5, {"unsorted": True}, (0, F32_BIT)),
    ("plain V1", 2, {"unsorted": True}, (1, F32_BIT)),
    ("plain V2", 2, {"unsorted": True, "variant": 2}, (2, F32_BIT)),
    ("plain V3", 7, {"unsorted": True}, (3, F32_BIT)),
    ("plain V5", 0, {"unsorted": True}, (5, F32_BIT)),
    ("reordering V0", 5, {}, (0, F32_BIT | SORTED_BIT)),
    ("reordering V1", 2, {}, (1, F32_BIT | SORTED_BIT)),
    ("slice-sorted V2", 2, {"variant": 2}, (2, F32_BIT | SS_BIT)),
    ("slice-sorted V3", 7, {}, (3, F32_BIT | SS_BIT)),
    ("slice-sorted V5", 0, {"classic_walk": True}, (5, F32_BIT | SS_BIT)),
    ("pair walk V5", 0, {}, (5, F32_BIT | SS_BIT | PW_BIT)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS, ids=[f[0].replace(" ", "_") for f in FORMS])
def test_exact_build_equals_the_twin_bit_for_bit(rt, gpu_ctx_factory, form):
    """Every f32 kernel instantiation, built with 64-bit elementary functions, against the CPU twin at 128 x 96 x 10, chunk 1: the same
    frame bit for bit and the same segment count.  stats.variant and stats.sorted say the intended form ran.  Eleven rows for ten
    kernels: the slice-sorted V5 kernel serves random_scene with classic_walk and would serve a sphere scene without pair-walk records."""
    name, arm, kw, (variant, bits) = form
    ctx = gpu_ctx_factory(scene(rt, arm))
    with rt.f32_exact():
        img, st = ctx.render(W, H, SPP, chunk=1, f32=True, generic=True, **kw)
    assert (st["variant"], st["sorted"]) == (variant, bits), (name, st["variant"], st["sorted"])
    ref = cpu(rt, arm, variant=variant, pair_walk=bool(bits & PW_BIT))
    print(f"\n{name}: arm {arm}, {st['segments']} segments (twin {ref[1]['segments']}), first difference {first_difference(img, ref[0])}")
    assert same(img, st, ref), (name, st["segments"], ref[1]["segments"], first_difference(img, ref[0]))
    # and the product's kernel of the same form is another kernel: the switch is off again
    _, sp = ctx.render(W, H, 1, chunk=1, f32=True, generic=True, **kw)
    assert (sp["variant"], sp["sorted"]) == (variant, bits)


@pytest.mark.gpu
@pytest.mark.parametrize("arm", (5, 7, 0))
def test_exact_build_default_form_entries_and_passes(rt, gpu_ctx_factory, arm):
    """The default f32 form of Cornell, final_scene and random_scene through the product's other paths: a tile with a sample offset, raw
    sums, a 1 MiB partial budget (4 passes), render_rows with a ragged last strip, render_device -- each equal to the twin."""
    from test_render_passes import DeviceBuffer
    ctx = gpu_ctx_factory(scene(rt, arm))
    variant = {5: 0, 7: 3, 0: 5}[arm]
    pw = arm == 0
    with rt.f32_exact():
        tile = (16, 8, 96, 80)
        img, st = ctx.render(W, H, SPP, tile=tile, sample_offset=7, chunk=1, f32=True, generic=True)
        assert same(img, st, cpu(rt, arm, variant=variant, pair_walk=pw, tile=tile, sample_offset=7)), (arm, "tile")
        raw, sr = ctx.render(W, H, SPP, out_sum=True, chunk=1, f32=True, generic=True)
        assert same(raw, sr, cpu(rt, arm, variant=variant, pair_walk=pw, out_sum=True)), (arm, "raw sums")
        full = cpu(rt, arm, variant=variant, pair_walk=pw)
        img, st = ctx.render(W, H, SPP, chunk=1, partial_mib=1, f32=True, generic=True)
        assert st["passes"] == 4 and same(img, st, full), (arm, "passes", st["passes"])
        img, st = ctx.render_rows(W, H, SPP, strip_rows=40, chunk=1, f32=True, generic=True)    # 40 + 40 + 16 rows
        assert st["sorted"] & F32_BIT and same(img, st, full), (arm, "render_rows")
        dev = DeviceBuffer(H * W * 3 * 8)
        try:
            sd = ctx.render_device(dev.ptr, W, H, SPP, chunk=1, f32=True, generic=True)
            got = dev.to_host((H, W, 3))
        finally:
            dev.free()
        assert same(got, sd, full), (arm, "render_device")


def elementary_arguments():
    """The arguments the f32 core feeds the five functions (csrc/rt_core.h call sites), ~1e5 each plus the edges.
    sin / cos: phi = 2 pi r of rt_random_cosine_direction, rt_random_to_sphere and the sphere-light sample, r a 53-bit draw rounded to
    float (so r = 1.0f occurs); sin also of the checker and marble textures' 10 * p, |p| up to ~1000.  acos(-p.y) and
    atan2(-p.z, p.x) + pi of sphere_uv, p a unit vector up to rounding.  ln(r) of the free flight, r in [0, 1] as above."""
    rng = np.random.default_rng(20261017)
    n = 100_000
    f = np.float32
    r = rng.random(n).astype(f)
    edges_r = np.array([0.0, 2.0 ** -53, 2.0 ** -24, np.nextafter(f(1), f(0)), 1.0, 0.25, 0.5, 0.75], dtype=f)
    phi = (f(2.0) * f(np.pi)) * np.concatenate([r, edges_r])
    tex = np.concatenate([rng.uniform(-1e4, 1e4, n).astype(f), np.array([0.0, -0.0, 1e4, -1e4], dtype=f)])
    v = rng.normal(size=(n, 3))
    v = (v / np.linalg.norm(v, axis=1)[:, None]).astype(f)
    one = f(1)
    ac = np.concatenate([rng.uniform(-1, 1, n).astype(f), -v[:, 1], np.array([-1, 1, 0, -0.0, np.nextafter(one, f(0)), -np.nextafter(one, f(0)), 2.0 ** -30], dtype=f)])
    ax = np.array([[0, 1], [0, -1], [1, 0], [-1, 0], [-0.0, 1], [-0.0, -1], [1, -0.0], [-1, -0.0], [0, 0], [-0.0, 0], [0, -0.0], [-0.0, -0.0],
                   [2.0 ** -40, 1], [2.0 ** -40, -1], [-(2.0 ** -40), -1], [1, 2.0 ** -40], [1, 1], [-1, 1], [1, -1], [-1, -1]], dtype=f)
    at_x = np.concatenate([-v[:, 2], ax[:, 0]])
    at_y = np.concatenate([v[:, 0], ax[:, 1]])
    ln = np.concatenate([r[r > 0], rng.uniform(0, 1e-3, n // 10).astype(f) + f(2.0 ** -53), np.array([2.0 ** -53, 2.0 ** -24, np.nextafter(one, f(0)), 1.0, 0.5], dtype=f)])
    return {"sin": (np.concatenate([phi, tex]), None), "cos": (phi, None), "atan2": (at_x, at_y), "acos": (ac, None), "log": (ln, None)}


def ulp_distance(got, want):
    """distance in f32 ulps by the integer order of the floats (+0 and -0 are one apart: a wrong sign of zero counts)"""
    def key(a):
        i = a.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF) - 1, i)
    return np.abs(key(got) - key(want))


def measure_elementary(rt):
    lib = orc.flat_f32_lib()
    out = {}
    for name, (x, y) in elementary_arguments().items():
        y = y if y is not None else np.zeros_like(x)
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        want = np.empty_like(x)
        lib.orcflat_f32_elementary(rt.F32_ELEMENTARY.index(name), x.ctypes.data_as(_P), y.ctypes.data_as(_P), x.size, want.ctypes.data_as(_P))
        got = rt.f32_elementary(name, x, y)
        d = ulp_distance(got, want)
        worst = int(np.argmax(d))
        out[name] = {"n": int(x.size), "max_ulp": int(d.max()), "at": [float(x[worst]), float(y[worst])],
                     "nan": int(np.isnan(got).sum()), "want_nan": int(np.isnan(want).sum()),
                     "sign_mismatch": int((np.signbit(got) != np.signbit(want))[(want != 0) | (got != 0)].sum()),
                     "zero_sign_mismatch": int((np.signbit(got) != np.signbit(want))[(want == 0) & (got == 0)].sum())}
    return out


@pytest.mark.gpu
def test_the_five_elementary_functions_on_the_device(rt):
    """::sinf, ::cosf, ::atan2f, ::acosf, ::logf on the device -- all that separates the product's f32 kernels from the exact build --
    against the 64-bit function of include/rt1w_num.h rounded once (the twin's), over the arguments the core feeds them.  The maximum
    distance per function was measured on the MI355X and is recorded in tests/golden/f32_elementary_ulps.json with the ROCm version;
    asserted: the recorded maximum + 1 ulp (room for a point release of the math library), no NaN, no wrong sign at any argument."""
    rec = json.load(open(ULPS))
    got = measure_elementary(rt)
    print("\nf32 elementary functions, max ulp distance (device single precision against 64-bit rounded once):")
    for name, g in got.items():
        print(f"  {name:6s} n={g['n']:7d} max {g['max_ulp']} ulp at {g['at']}  (recorded {rec['max_ulp'][name]})  nan {g['nan']} sign {g['sign_mismatch']}")
    for name, g in got.items():
        assert g["nan"] == 0 and g["want_nan"] == 0, (name, g)
        assert g["sign_mismatch"] == 0, (name, g)
        assert g["max_ulp"] <= rec["max_ulp"][name] + 1, (name, g, rec["max_ulp"][name])


# arms whose max_depth = 1 frame calls none of the five functions in a way that reaches the frame
DEPTH1_ARMS = (5, 0, 2, 4)


@pytest.mark.gpu
@pytest.mark.parametrize("arm", DEPTH1_ARMS)
def test_product_equals_exact_at_depth_1(rt, gpu_ctx_factory, arm):
    """max_depth = 1: a sample is the background (miss) or the emitted radiance of the first hit; the scattered ray's segment ends at
    once at depth 0 and adds beta * 0.  The first segment of a scene without media is camera ray (lens and shutter draws: rejection
    sampling and a range, no elementary function), BVH walk and primitive tests: + - * / sqrt.  The five functions are called in the
    scatter half (cosine direction, light sample) and in sphere_uv for a textured albedo, and feed only the next ray and beta, which
    the frame sees multiplied by zero (a finite beta in both builds: the pdf is a product of the same cosines up to an ulp).  Emitters
    of these arms are solid colours: no sphere_uv in `emitted`.  So the product's frame and the exact build's are the same bits with
    the same segment count on Cornell (5), random_scene (0: defocus, moving spheres, pair walk), two_perlin_spheres (2) and
    simple_light (4).  cornell_smoke (6) and final_scene (7) are left out: a ConstantMedium on the first segment draws its free flight
    with ln.  (That call passes the 64-bit draw, so overload resolution picks the 64-bit rt_log in every build and the two builds may
    well agree there too; it is not asserted.)"""
    ctx = gpu_ctx_factory(scene(rt, arm))
    a, sa = ctx.render(W, H, SPP, max_depth=1, chunk=1, f32=True, generic=True)
    with rt.f32_exact():
        b, sb = ctx.render(W, H, SPP, max_depth=1, chunk=1, f32=True, generic=True)
    assert sa["sorted"] == sb["sorted"] and sa["variant"] == sb["variant"]
    assert same(a, sa, (b, sb)), (arm, sa["segments"], sb["segments"], first_difference(a, b))
    assert same(b, sb, cpu(rt, arm, max_depth=1, pair_walk=(arm == 0))), arm


@pytest.mark.gpu
def test_product_against_exact_at_full_depth(rt, gpu_ctx_factory):
    """The product's f32 frame against the exact build's at the shapes of test_f32_mode_matches_the_f64_frame_statistically: frame mean
    and segments per path within the 3 % asserted there between f32 and f64.  Observed values are printed; they are far smaller."""
    for arm, aspect, (w, h, spp) in ((0, 1.5, (240, 160, 32)), (6, None, (128, 128, 32)), (7, None, (128, 128, 32)), (2, None, (128, 72, 16))):
        ctx = gpu_ctx_factory(rt.Scene.reference(arm, build_seed=1, aspect_ratio=aspect))
        a, sa = ctx.render(w, h, spp, f32=True, generic=True)
        with rt.f32_exact():
            b, sb = ctx.render(w, h, spp, f32=True, generic=True)
        assert np.isfinite(a).all() and np.isfinite(b).all(), arm
        dm, ds = a.mean() / b.mean() - 1.0, sa["segments"] / sb["segments"] - 1.0
        print(f"\narm {arm} {w}x{h}x{spp}: product/exact mean {dm:+.6f}, segments {ds:+.6f}, differing pixels {int((a != b).any(axis=2).sum())} of {w * h}")
        assert abs(dm) < 0.03 and abs(ds) < 0.03, (arm, dm, ds)
