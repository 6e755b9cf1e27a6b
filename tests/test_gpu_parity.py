"""GPU parity tests: everything goes through the C ABI (librt1w.so -> HIP kernel on gfx950).

Bars:
  * GPU == CPU build of the same core (oracle_flat): BIT-EXACT f64 framebuffers (np.array_equal).
  * GPU vs the literal recursive oracle: |diff| <= 1e-12 * |value| per channel (the recursion and the
    iteration associate the colour products differently), equal segment counts, identical PPM text.
  * at BASELINE's full sizes: crops against the oracle + size-independent properties
    (tile == full, sample ranges add up, determinism, statistics vs the reference's PNG).
"""
import json
import os

import numpy as np
import pytest

import orc
from dual import random_scene_pair

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
RTOL = 1e-12


def close(a, b):
    both_nan = np.isnan(a) & np.isnan(b)
    return bool((both_nan | (np.abs(a - b) <= RTOL * np.abs(a)) | (a == b)).all())


def literal_crop_check(arm, aspect, W, H, spp, tile, gpu_crop, flat_segments=None):
    """A crop of a FULL-SIZE job against oracle A (oracle/oracle.cpp, the literal recursive restatement) rendering the same pixels of
    the same W x H x spp job: <= 1e-12 relative (the chunked sum and the recursion associate differently), and the oracle's segment
    count on the crop's paths equals the CPU core build's on the same crop (which the GPU frame equals bit for bit)."""
    lit, sl = orc.OracleScene(arm, build_seed=1, aspect_ratio=aspect).render(W, H, spp, tile=tile)
    assert close(lit, gpu_crop), (arm, tile)
    if flat_segments is not None:
        assert sl["segments"] == flat_segments, (arm, tile, sl["segments"], flat_segments)


SMALL = {0: (96, 64, 8), 1: (64, 36, 8), 2: (64, 36, 8), 3: (64, 36, 8), 4: (64, 36, 16), 5: (64, 64, 16), 6: (64, 64, 16),
         7: (64, 64, 16)}


def test_native_library_is_loaded(rt):
    maps = open("/proc/self/maps").read()
    assert "librt1w.so" in maps


def test_numerical_contract_bit_identical_on_device(rt, gpu_ctx_factory):
    import ctypes as C
    ctx = gpu_ctx_factory(rt.Scene.reference(5))
    rng = np.random.default_rng(11)
    n = 1 << 18
    a = rng.uniform(-1, 1, n) * 10.0 ** rng.integers(-3, 6, n)
    b = rng.uniform(-1, 1, n) * 10.0 ** rng.integers(-6, 4, n)
    a[:8] = [0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 2.0 ** 31]
    for fn in range(9):
        host = np.empty(n)
        orc.A.orc_num_eval(fn, a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), host.ctypes.data_as(C.c_void_p), n)
        dev = ctx.debug_eval(fn, a, b)
        assert np.array_equal(host.view(np.uint64)[~np.isnan(host)], dev.view(np.uint64)[~np.isnan(host)]), f"fn {fn}"
        assert np.array_equal(np.isnan(host), np.isnan(dev)), f"fn {fn}"


def test_device_aabb_forms_match_host_literal(rt, gpu_ctx_factory):
    """The slab test as the kernels run it (max/min instructions, taken when no bound is NaN) and the literal
    compare/select form, both on the device, against the oracle's AABB::hit on the host -- on random boxes and rays
    plus the nasty ones: zero / negative-zero / infinite / NaN direction and origin components, origins on a slab
    plane (0 * inf = NaN), empty and inverted intervals, infinite bounds."""
    import ctypes as C
    ctx = gpu_ctx_factory(rt.Scene.reference(5))
    rng = np.random.default_rng(7)
    n = 200_000
    c = np.empty((n, 14))
    lo = rng.uniform(-10, 10, (n, 3)); ext = rng.uniform(0, 8, (n, 3))
    c[:, 0:3] = lo; c[:, 3:6] = lo + ext
    c[:, 6:9] = rng.uniform(-15, 15, (n, 3))
    c[:, 9:12] = rng.normal(size=(n, 3))
    aim = rng.random(n) < 0.6                                                # most rays are aimed at their box
    c[aim, 9:12] = (lo + ext * rng.random((n, 3)) - c[:, 6:9])[aim] * rng.uniform(0.05, 3.0, (n, 1))[aim]
    c[:, 12] = rng.choice([0.001, -np.inf, 0.0, 1.0], n)
    c[:, 13] = rng.choice([np.inf, 5.0, 50.0, 0.5], n)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 1e-300, 1e300])
    k = n // 2
    idx = rng.integers(0, 3, k)
    c[np.arange(k), 9 + idx] = rng.choice(special, k)                       # special direction components
    k2 = n // 4
    ax = rng.integers(0, 3, k2)
    c[np.arange(k2), 6 + ax] = c[np.arange(k2), 0 + ax]                     # origin exactly on a slab plane
    c[np.arange(0, n, 97), 6 + rng.integers(0, 3)] = np.nan                 # NaN origin component
    lit, fast = ctx.debug_aabb(c)
    host = np.array([orc.A.orc_aabb_hit(r[0:3].ctypes.data_as(C.c_void_p), r[3:6].ctypes.data_as(C.c_void_p),
                                        r[6:9].ctypes.data_as(C.c_void_p), r[9:12].ctypes.data_as(C.c_void_p), r[12], r[13])
                     for r in np.ascontiguousarray(c[:20000])], dtype=np.int32)
    assert np.array_equal(lit[:20000], host)
    assert np.array_equal(lit, fast)          # t_min / t_max are never NaN here: the regime in which the kernels use `fast`
    assert 0.1 < lit.mean() < 0.9


@pytest.mark.parametrize("arm", sorted(SMALL))
def test_gpu_bit_exact_vs_core_and_close_to_literal(rt, gpu_ctx_factory, arm):
    W, H, spp = SMALL[arm]
    sc = rt.Scene.reference(arm, build_seed=1)
    ctx = gpu_ctx_factory(sc)
    g, sg = ctx.render(W, H, spp)
    b, sb = orc.flat_render(sc, W, H, spp, chunk=sg["chunk"])
    assert sg["segments"] == sb["segments"]
    assert np.array_equal(g, b, equal_nan=True)
    a, sa = orc.OracleScene(arm, build_seed=1).render(W, H, spp)
    assert sa["segments"] == sg["segments"]
    assert close(a, g)
    assert rt.format_ppm(g) == rt.format_ppm(a)          # integer pixel output bit-identical


def test_gpu_kernel_variants_agree(rt, gpu_ctx_factory):
    """Forced variants on the GPU (sweep vs stack, pruned vs full) == the CPU build, bit for bit."""
    for arm, variants in ((5, (0, 1, 2, 3)), (6, (1, 3)), (0, (1, 2, 3, 5)), (7, (3,))):
        W, H, spp = SMALL[arm]
        sc = rt.Scene.reference(arm, build_seed=1)
        ctx = gpu_ctx_factory(sc)
        ref, sref = orc.flat_render(sc, W, H, spp, chunk=8)
        for v in variants:
            g, sg = ctx.render(W, H, spp, chunk=8, variant=v)
            assert sg["variant"] == v and sg["segments"] == sref["segments"], (arm, v)
            assert np.array_equal(g, ref, equal_nan=True), (arm, v)
    with pytest.raises(rt.Rt1wError):                    # V0 cannot render a scene with media/textures
        gpu_ctx_factory(rt.Scene.reference(6)).render(16, 16, 1, variant=0)


def test_sorted_and_unsorted_kernels_are_bit_identical(rt, gpu_ctx_factory):
    """The workgroup-level reordering only changes which lane runs which path: same bits, same segment count,
    on ragged tiles, tiny images (fewer paths than one workgroup), depth limits and sample offsets."""
    sc = rt.Scene.reference(5, build_seed=1)
    ctx = gpu_ctx_factory(sc)
    for (W, H, spp, tile, kw) in ((96, 96, 16, None, {}), (200, 200, 3, (0, 0, 37, 23), {}), (200, 200, 40, (5, 7, 100, 9), {}),
                                  (2, 2, 5, None, {}), (64, 64, 8, None, dict(max_depth=2)), (64, 64, 8, None, dict(sample_offset=100, out_sum=True)),
                                  (600, 600, 20, None, dict(chunk=7))):
        a, sa = ctx.render(W, H, spp, tile=tile, unsorted=True, **kw)
        b, sb = ctx.render(W, H, spp, tile=tile, **kw)
        assert sa["sorted"] == 0 and (sb["sorted"] & 1) == 1
        assert sa["segments"] == sb["segments"] and np.array_equal(a, b, equal_nan=True), (W, H, spp, tile, kw)


def test_lds_node_cache_is_bit_identical(rt, gpu_ctx_factory):
    """Opt-in experiment: stack variants on scenes of <= 1024 nodes reading node records from an LDS copy (16-bit stack
    entries): same bits as the default."""
    for arm, (W, H, spp) in ((0, (96, 64, 8)),):
        sc = rt.Scene.reference(arm, build_seed=1)
        ctx = gpu_ctx_factory(sc)
        a, sa = ctx.render(W, H, spp)
        b, sb = ctx.render(W, H, spp, lds_nodes=True)
        assert (sa["sorted"] & 2) == 0 and (sb["sorted"] & 2) == 2
        assert sa["segments"] == sb["segments"] and np.array_equal(a, b, equal_nan=True)
    # a user scene with media + wrappers forced onto the stack variant V3 (cached, 16-bit stack with wrapper-exit markers)
    sc = rt.Scene.reference(6, build_seed=1)
    ctx = gpu_ctx_factory(sc)
    a, sa = ctx.render(64, 64, 8, variant=3)
    b, sb = ctx.render(64, 64, 8, variant=3, lds_nodes=True)
    c, sc_ = ctx.render(64, 64, 8)
    assert (sb["sorted"] & 2) == 2 and np.array_equal(a, b, equal_nan=True) and np.array_equal(a, c, equal_nan=True)


def test_gpu_matches_committed_golden_frames(rt, gpu_ctx_factory):
    meta = json.load(open(os.path.join(HERE, "golden", "oracle_frames.json")))
    gold = np.load(os.path.join(HERE, "golden", "oracle_frames.npz"))
    for name, m in meta["cases"].items():
        sc = rt.Scene.reference(m["arm"], build_seed=meta["build_seed"])
        ctx = gpu_ctx_factory(sc)
        g, sg = ctx.render(m["W"], m["H"], m["spp"], max_depth=m["depth"], global_seed=meta["global_seed"])
        assert sg["segments"] == m["segments"], name
        if name in gold:
            assert close(gold[name], g), name
        else:                                            # C1: crop + block means
            x0, y0, w, h = m["crop"]
            assert close(gold[name + "__crop"], g[y0:y0 + h, x0:x0 + w]), name
            bm = g.reshape(m["H"] // 20, 20, m["W"] // 20, 20, 3).mean(axis=(1, 3))
            assert np.allclose(bm, gold[name + "__block20"], rtol=1e-11, atol=0), name


def test_edge_cases(rt, gpu_ctx_factory):
    sc = rt.Scene.reference(5, build_seed=1)
    ctx = gpu_ctx_factory(sc)
    # ragged tile (not a multiple of the 8x8 work-item block), 1 spp, odd sizes, explicit chunk > spp
    for (W, H, spp, tile, chunk) in ((37, 23, 1, None, 0), (50, 50, 3, (7, 9, 13, 5), 0), (33, 33, 5, (32, 32, 1, 1), 64),
                                     (2, 2, 9, None, 2)):
        g, sg = ctx.render(W, H, spp, tile=tile, chunk=chunk)
        b, sb = orc.flat_render(sc, W, H, spp, tile=tile, chunk=sg["chunk"])
        assert np.array_equal(g, b) and sg["segments"] == sb["segments"]
    # depth 0 and 1 (main.rs:59-61)
    g0, s0 = ctx.render(16, 16, 2, max_depth=0)
    assert not g0.any() and s0["segments"] == 0
    g1, _ = ctx.render(32, 32, 4, max_depth=1)
    assert np.array_equal(g1, orc.flat_render(sc, 32, 32, 4, max_depth=1)[0])
    # invalid parameters are refused, not rendered
    for bad in (dict(width=1, height=10, spp=1), dict(width=10, height=10, spp=0), dict(width=10, height=10, spp=1, tile=(5, 5, 6, 6))):
        with pytest.raises(rt.Rt1wError):
            ctx.render(bad["width"], bad["height"], bad["spp"], tile=bad.get("tile"))
    # global seed changes the image, same seed reproduces it
    ga, _ = ctx.render(24, 24, 4, global_seed=3)
    gb, _ = ctx.render(24, 24, 4, global_seed=3)
    gc, _ = ctx.render(24, 24, 4, global_seed=4)
    assert np.array_equal(ga, gb) and not np.array_equal(ga, gc)


def test_user_built_scene_through_the_constructors(rt, gpu_ctx_factory):
    """A scene assembled call by call through the ABI (not the built-in table): nested wrappers,
    a medium whose boundary is a rotated box, checker + noise textures, moving sphere, no lights."""
    def build(mod):
        s = mod.Scene(build_seed=5)
        chk = s.checker_texture(s.solid_color((0.9, 0.9, 0.9)), s.solid_color((0.1, 0.3, 0.1)))
        ground = s.lambertian(chk)
        noise = s.lambertian(s.noise_texture(2.0))
        objs = [s.sphere((0, -100.5, -1), 100.0, ground),
                s.moving_sphere((0, 0, -1), (0, 0.3, -1), 0.0, 1.0, 0.5, noise),
                s.sphere((1.1, 0, -1), 0.5, s.metal((0.8, 0.6, 0.2), 0.3)),
                s.sphere((-1.1, 0, -1), 0.5, s.dielectric(1.5)),
                s.flip_face(s.xz_rect(-1, 1, -2, 0, 2.0, s.diffuse_light(s.solid_color((4, 4, 4)))))]
        box = s.translate(s.rotate_y(s.aabox((0, 0, 0), (0.6, 0.6, 0.6), ground), 30.0), (-0.3, 0.6, -1.3))
        objs.append(s.constant_medium(box, 2.0, s.solid_color((0.8, 0.8, 1.0))))
        s.set_world(s.bvh_node(objs))
        s.set_lights([])
        s.set_background((0.5, 0.7, 1.0))
        s.set_camera((0, 1, 2), (0, 0.2, -1), (0, 1, 0), 50.0, 1.5, 0.05, 3.0, 0.0, 1.0)
        s.commit()
        return s
    sc = build(rt)
    ctx = gpu_ctx_factory(sc)
    g, sg = ctx.render(60, 40, 8)
    b, sb = orc.flat_render(sc, 60, 40, 8, chunk=sg["chunk"])
    assert sg["segments"] == sb["segments"] and np.array_equal(g, b)
    assert np.isfinite(g).all() and g.mean() > 0.05


# ---------------------------------------------------------------- full BASELINE sizes

def test_c3_cornell_600x600_1000spp_properties(rt, gpu_ctx_factory):
    sc = rt.Scene.reference(5, build_seed=1)
    ctx = gpu_ctx_factory(sc)
    W = H = 600
    full, st = ctx.render(W, H, 1000, chunk=125)
    assert st["paths"] == 360_000_000 and 4.5 < st["segments"] / st["paths"] < 5.6
    # (a) crops of the full-size job against the CPU core build (same W,H,spp) -- bit exact
    for tile in ((0, 0, 8, 8), (296, 300, 8, 8), (592, 592, 8, 8)):
        b, sb = orc.flat_render(sc, W, H, 1000, tile=tile, chunk=125)
        x0, y0, w, h = tile
        assert np.array_equal(full[y0:y0 + h, x0:x0 + w], b)
        literal_crop_check(5, None, W, H, 1000, tile, full[y0:y0 + h, x0:x0 + w], sb["segments"])
    # (b) tile renders equal the same region of the full render (image tiling across GPUs)
    strip, _ = ctx.render(W, H, 1000, tile=(0, 160, 600, 16), chunk=125)
    assert np.array_equal(strip, full[160:176])
    # (c) sample-range sharding: 8 ranges of 125 as raw sums, added in order, == the full render
    total = np.zeros_like(full)
    for r in range(8):
        s, _ = ctx.render(W, H, 125, sample_offset=125 * r, out_sum=True, chunk=125)
        total = total + s
    assert np.array_equal(rt.resolve(total, 1000), full)
    # (d) determinism
    again, _ = ctx.render(W, H, 1000, chunk=125)
    assert np.array_equal(again, full)
    # (e) no NaN pixels survive into_sampled; energy is bounded by the light's radiance
    assert np.isfinite(full).all() and 0.0 <= full.min() and full.max() <= 15.0 * 1.0001 * 50


def test_cornell_600x600_100spp_matches_reference_png(rt, gpu_ctx_factory):
    """The reference's shipped default (main.rs:868-870) on the GPU vs the reference's own render
    rest_of_your_life.png: 8-bit 100x100-block means within 4/255, channel means within 0.5/255."""
    from test_golden import png_block_check
    ctx = gpu_ctx_factory(rt.Scene.reference(5, build_seed=1))
    img, _ = ctx.render(600, 600, 100)
    png_block_check(rt, img, 4.0, 0.5)


def test_final_scene_800x800_matches_reference_png(rt, gpu_ctx_factory):
    """C4 geometry (800x800, main.rs:917-919) at 200 spp vs the reference's own next_week.png on its 21 comparable blocks
    (tests/golden/make_golden.py says which and why): every block's linear mean within 12 %, the mean ratio within 3 %.
    (Measured at 1500 spp: 0.91..1.07, means 0.993/1.000/0.998.)"""
    from test_golden import final_png_block_check
    ctx = gpu_ctx_factory(rt.Scene.reference(7, build_seed=1))
    img, _ = ctx.render(800, 800, 200)
    final_png_block_check(img, 0.12, 0.03)


def test_c2_random_scene_1200x800_500spp_crops(rt, gpu_ctx_factory):
    sc = rt.Scene.reference(0, build_seed=1, aspect_ratio=1.5)
    ctx = gpu_ctx_factory(sc)
    W, H, spp = 1200, 800, 500
    full, st = ctx.render(W, H, spp)
    assert st["paths"] == W * H * spp and np.isfinite(full).all()
    assert st["chunk"] == 1 and st["passes"] == 2        # 500 chunks of 23.04 MB partial sums, 372 of them per 8 GiB pass
    for tile in ((600, 400, 8, 8), (100, 60, 8, 4)):
        b, sb = orc.flat_render(sc, W, H, spp, tile=tile, chunk=st["chunk"])
        x0, y0, w, h = tile
        assert np.array_equal(full[y0:y0 + h, x0:x0 + w], b)
        literal_crop_check(0, 1.5, W, H, spp, tile, full[y0:y0 + h, x0:x0 + w], sb["segments"])
    # sky: top-left pixel sees only background (0.7,0.8,1.0) -- or geometry; mean stays in gamut
    assert 0.0 < full.mean() < 1.0


def test_c4_final_scene_800x800_tile_at_10000spp(rt, gpu_ctx_factory):
    """C4 is an 8-GPU job (6.4e9 paths); one 16x16 tile of it at the full 10000 spp, against the CPU core build."""
    sc = rt.Scene.reference(7, build_seed=1)
    ctx = gpu_ctx_factory(sc)
    tile = (392, 300, 16, 16)
    g, sg = ctx.render(800, 800, 10000, tile=tile)
    b, sb = orc.flat_render(sc, 800, 800, 10000, tile=tile, chunk=sg["chunk"])
    assert sg["segments"] == sb["segments"] and np.array_equal(g, b, equal_nan=True)
    literal_crop_check(7, None, 800, 800, 10000, (392, 300, 8, 8), g[:8, :8])   # an 8x8 corner of the tile at the full 10 000 spp


def test_c5_4k_cornell_tiles(rt, gpu_ctx_factory):
    """C5 (3840x2160, 16:9, 10000 spp, 8.3e10 paths) is the 8-GPU scaling job: row strips dealt to ranks.
    Here: one 16-row strip at 200 spp on the GPU == the CPU core build on a crop; strip owners partition the image."""
    import importlib
    sh = importlib.import_module("raytracing-1w_amd.sharding")
    sc = rt.Scene.reference(5, build_seed=1, aspect_ratio=16.0 / 9.0)
    W, H = 3840, 2160
    ctx = gpu_ctx_factory(sc)
    y0, rows = sh.row_strips(H, 8, 3)[10]
    strip, st = ctx.render(W, H, 200, tile=(0, y0, W, rows))
    crop = (1900, y0 + 4, 8, 4)
    b, sb = orc.flat_render(sc, W, H, 200, tile=crop, chunk=st["chunk"])
    assert np.array_equal(strip[4:8, 1900:1908], b)
    literal_crop_check(5, 16.0 / 9.0, W, H, 200, crop, strip[4:8, 1900:1908], sb["segments"])


def test_two_contexts_render_concurrently_from_two_threads(rt, gpu_ctx_factory):
    """include/rt1w.h: calls on distinct contexts are thread-safe (one host thread per context / GPU)."""
    import threading
    sc5 = rt.Scene.reference(5, build_seed=1)
    sc0 = rt.Scene.reference(0, build_seed=1)
    c5, c0 = gpu_ctx_factory(sc5), gpu_ctx_factory(sc0)
    ref5, _ = c5.render(128, 128, 16)
    ref0, _ = c0.render(96, 64, 8)
    out = {}

    def work(name, ctx, args, n):
        res = []
        for _ in range(n):
            img, _ = ctx.render(*args)
            res.append(img)
        out[name] = res

    th = [threading.Thread(target=work, args=("a", c5, (128, 128, 16), 6)), threading.Thread(target=work, args=("b", c0, (96, 64, 8), 6))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert all(np.array_equal(i, ref5) for i in out["a"]) and all(np.array_equal(i, ref0) for i in out["b"])


def test_cli_writes_the_reference_ppm_layout(rt, tmp_path):
    """raytracing-1w_amd/rt1w: the `main` of the reference with the pixel loop on the GPU; its P3 text must equal
    what the library/oracle produce for the same parameters."""
    import subprocess
    exe = os.path.join(orc.ROOT, "raytracing-1w_amd", "rt1w")
    assert os.path.exists(exe)
    out = tmp_path / "o.ppm"
    subprocess.check_call([exe, "--scene", "5", "--width", "48", "--height", "48", "--spp", "8", "--out", str(out)], stderr=subprocess.DEVNULL)
    lit, _ = orc.OracleScene(5, build_seed=1).render(48, 48, 8)
    assert out.read_text() == rt.format_ppm(lit)


def test_device_side_quantiser_matches_host(rt, gpu_ctx_factory):
    """rt1w_render_u8: bytes == host rt1w_quantize of the f64 render, rows top-down; also on a
    framebuffer with NaN-scrubbed / over-bright / zero pixels (depth 1: only the light, saturating at 255)."""
    ctx = gpu_ctx_factory(rt.Scene.reference(5, build_seed=1))
    for (W, H, spp, tile, depth) in ((96, 64, 8, None, 50), (50, 50, 3, (7, 9, 13, 5), 50), (64, 64, 4, None, 1)):
        img, _ = ctx.render(W, H, spp, tile=tile, max_depth=depth)
        u8, _ = ctx.render_u8(W, H, spp, tile=tile, max_depth=depth)
        assert u8.dtype == np.uint8 and np.array_equal(u8, rt.quantize(img)[::-1])
    # and the P3 text assembled from the device bytes equals the reference layout
    img, _ = ctx.render(40, 30, 4)
    u8, _ = ctx.render_u8(40, 30, 4)
    txt = "P3\n40 30\n255\n" + "".join("%d %d %d\n" % tuple(px) for row in u8 for px in row)
    assert txt == rt.format_ppm(img)


def test_strip_render_with_progress_is_bit_identical(rt, gpu_ctx_factory):
    """rt1w_render_rows (main.rs:957-960 row order, :995-998 progress): strips from the top row down,
    D2H overlapped; same bits as the one-shot entries for every strip size, on a whole frame, a ragged last strip and a
    sub-tile; progress is monotonic and ends at tile_h; a true return cancels with the rows reported so far intact."""
    ctx = gpu_ctx_factory(rt.Scene.reference(5, build_seed=1))
    for (W, H, spp, tile, strip) in ((96, 80, 24, None, 0), (96, 80, 24, None, 7), (96, 80, 24, None, 80), (96, 80, 24, None, 500),
                                     (64, 64, 5, (3, 11, 40, 33), 8), (32, 24, 70, None, 1)):
        ref, s0 = ctx.render(W, H, spp, tile=tile)
        ref8, _ = ctx.render_u8(W, H, spp, tile=tile)
        seen = []
        img, s1 = ctx.render_rows(W, H, spp, strip_rows=strip, tile=tile, progress=lambda d, t: seen.append((d, t)) or 0)
        th = ref.shape[0]
        assert np.array_equal(img, ref, equal_nan=True)
        assert s1["paths"] == s0["paths"] and s1["segments"] == s0["segments"]
        assert seen and seen[-1] == (th, th) and all(t == th for _, t in seen)
        assert [d for d, _ in seen] == sorted(set(d for d, _ in seen))
        if strip not in (0,) and strip < th:
            assert [d for d, _ in seen][0] == strip
        u8, _ = ctx.render_rows(W, H, spp, strip_rows=strip, tile=tile, u8=True)
        assert u8.dtype == np.uint8 and np.array_equal(u8, ref8)
    # raw sums (multi-rank sample ranges) come through as well
    a, _ = ctx.render(48, 40, 6, out_sum=True, sample_offset=3)
    b, _ = ctx.render_rows(48, 40, 6, strip_rows=16, out_sum=True, sample_offset=3)
    assert np.array_equal(a, b, equal_nan=True)
    # cancel after the second strip: rows reported so far are final, the call says so
    ref8, _ = ctx.render_u8(64, 64, 8)
    calls = []
    out = np.full((64, 64, 3), 7, dtype=np.uint8)
    with pytest.raises(rt.Rt1wError) as e:
        ctx.render_rows(64, 64, 8, strip_rows=8, u8=True, progress=lambda d, t: calls.append(d) or d >= 16, out=out)
    assert e.value.code == rt.ERR_CANCELLED and calls == [8, 16]
    assert np.array_equal(out[:16], ref8[:16]) and np.all(out[16:] == 7)
    # the context is still usable
    again, _ = ctx.render_rows(64, 64, 8, strip_rows=8, u8=True)
    assert np.array_equal(again, ref8)
    with pytest.raises(rt.Rt1wError):
        ctx.render_rows(64, 64, 8, u8=True, out_sum=True)


def test_scene_specialised_kernels_are_bit_identical(rt, gpu_ctx_factory, tmp_path, monkeypatch):
    """rt1w_context_specialise: the sweep unrolled along the scene's own tree (compile-time node kinds), from the
    in-tree kernel cache for the reference arms at build_seed 1, from hiprtc otherwise.  Same arithmetic, so the frames
    must equal the generic kernels' bit for bit -- Cornell, the media arm, the textured arms, random graphs."""
    monkeypatch.setenv("RT1W_KERNEL_CACHE", str(tmp_path / "kcache"))
    # (1) the reference arms built into <package>/kernels: active from context creation on
    for arm, (W, H, spp) in {5: (96, 96, 16), 6: (64, 64, 12), 1: (64, 36, 8), 2: (64, 36, 8), 3: (64, 36, 8), 4: (64, 36, 16)}.items():
        sc = rt.Scene.reference(arm, build_seed=1)
        ctx = gpu_ctx_factory(sc)
        assert ctx.specialised(), f"arm {arm}: no precompiled kernel found next to the library"
        a, sa = ctx.render(W, H, spp)
        b, sb = ctx.render(W, H, spp, generic=True)
        assert (sa["sorted"] & 4) and not (sb["sorted"] & 4)
        assert sa["segments"] == sb["segments"] and np.array_equal(a, b, equal_nan=True), arm
        f, _ = orc.flat_render(sc, W, H, spp, chunk=sa["chunk"])
        assert np.array_equal(a, f, equal_nan=True), arm
    # (2) another tree (the axes of bvh.rs:84 drawn from another build seed, RT1W_BVH_REFERENCE): cache miss, compile, then a hit from the user cache
    sc = rt.Scene.reference(5, build_seed=7).set_bvh_build("reference")
    ctx = gpu_ctx_factory(sc)
    assert not ctx.specialised()
    with pytest.raises(rt.Rt1wError) as e:
        ctx.specialise(cached_only=True)
    assert e.value.code == rt.ERR_STATE
    g, sg = ctx.render(200, 200, 20)
    assert not (sg["sorted"] & 4)
    info = ctx.specialise()
    assert info["active"] and not info["from_cache"] and info["compile_ms"] > 0 and len(info["key"]) == 16
    s, ss = ctx.render(200, 200, 20)
    assert (ss["sorted"] & 4) and np.array_equal(g, s, equal_nan=True) and ss["segments"] == sg["segments"]
    ctx2 = gpu_ctx_factory(sc)
    assert ctx2.specialised() and ctx2.specialise()["from_cache"]
    # tiles, sample offsets, raw sums, strips go through the same launch path
    t1, _ = ctx.render(200, 200, 9, tile=(13, 7, 50, 31), sample_offset=5, out_sum=True)
    t2, _ = ctx.render(200, 200, 9, tile=(13, 7, 50, 31), sample_offset=5, out_sum=True, generic=True)
    assert np.array_equal(t1, t2, equal_nan=True)
    r, sr = ctx.render_rows(200, 200, 20, strip_rows=64)
    assert (sr["sorted"] & 4) and np.array_equal(r, s, equal_nan=True)
    # (3) random small graphs: wrappers nested up to 3, media with wrapped boundaries, every texture and primitive kind
    from dual import random_scene_pair
    done = 0
    for seed in range(2000, 2040):
        prod, _ = random_scene_pair(seed)
        info = prod.info()
        if info["n_nodes"] > 64:
            continue
        c = gpu_ctx_factory(prod)
        c.specialise()
        a, sa = c.render(28, 20, 4)
        b, sb = c.render(28, 20, 4, generic=True)
        assert (sa["sorted"] & 4) and sa["segments"] == sb["segments"] and np.array_equal(a, b, equal_nan=True), (seed, info)
        done += 1
        if done == 6:
            break
    assert done == 6
    # (3b) a mid-size scene (Cornell walls + 8 rotated boxes = 141 nodes): the generic code is the stack walk, the specialised
    #      kernel the unrolled sweep -- two different traversal implementations, same bits
    s8 = rt.Scene(build_seed=1)
    white = s8.lambertian(s8.solid_color((0.73, 0.73, 0.73))); lightm = s8.diffuse_light(s8.solid_color((15, 15, 15)))
    objs = [s8.yz_rect(0, 555, 0, 555, 555, s8.lambertian(s8.solid_color((0.12, 0.45, 0.15)))),
            s8.yz_rect(0, 555, 0, 555, 0, s8.lambertian(s8.solid_color((0.65, 0.05, 0.05)))),
            s8.flip_face(s8.xz_rect(213, 343, 227, 332, 554, lightm)), s8.xz_rect(0, 555, 0, 555, 0, white),
            s8.xz_rect(0, 555, 0, 555, 555, white), s8.xy_rect(0, 555, 0, 555, 555, white)]
    g8 = np.random.default_rng(3)
    for _ in range(8):
        b = s8.aabox((0, 0, 0), (60, float(g8.uniform(60, 250)), 60), s8.metal((0.8, 0.85, 0.88), 0.1) if _ % 3 == 0 else white)
        objs.append(s8.translate(s8.rotate_y(b, float(g8.uniform(-40, 40))), (float(g8.uniform(30, 460)), 0.0, float(g8.uniform(30, 460)))))
    objs.append(s8.sphere((190, 90, 190), 40, s8.dielectric(1.5)))
    s8.set_world(s8.bvh_node(objs))
    s8.set_lights([s8.xz_rect(213, 343, 227, 332, 554, s8.null_material())])
    s8.set_background((0, 0, 0))
    s8.set_camera((278, 278, -800), (278, 278, 0), (0, 1, 0), 40.0, 1.0, 0.0, 10.0, 0.0, 1.0)
    s8.commit()
    assert 64 < s8.info()["n_nodes"] <= 256
    c8 = gpu_ctx_factory(s8)
    gen8, sg8 = c8.render(120, 120, 12)
    assert sg8["variant"] == 2 and not (sg8["sorted"] & 4)
    c8.specialise()
    spe8, ss8 = c8.render(120, 120, 12)
    assert (ss8["sorted"] & 4) and ss8["segments"] == sg8["segments"] and np.array_equal(gen8, spe8, equal_nan=True)
    # (4) big scenes keep the generic kernels
    big = gpu_ctx_factory(rt.Scene.reference(0, build_seed=1, aspect_ratio=1.5))
    with pytest.raises(rt.Rt1wError) as e:
        big.specialise()
    assert e.value.code == rt.ERR_UNSUPPORTED and not big.specialised()


def test_wavefront_form_is_bit_identical(rt, gpu_ctx_factory):
    """RT1W_WAVEFRONT (rt_wavefront.h): the big scenes with the path state queued in HBM and one trace + one shade kernel per
    bounce (lanes refill from the queue as their walks end).  Same per-path function, samples still summed in order per chunk:
    bits and segment counts equal the persistent kernel's -- several chunks, several passes per chunk, a tile, raw sums."""
    for arm, aspect in ((0, 1.5), (7, None)):
        ctx = gpu_ctx_factory(rt.Scene.reference(arm, build_seed=1, aspect_ratio=aspect))
        for (W, H, spp, kw) in ((96, 64, 20, dict(chunk=8)), (64, 48, 5, dict(tile=(5, 7, 40, 30), sample_offset=3, out_sum=True))):
            a, sa = ctx.render(W, H, spp, **kw)
            b, sb = ctx.render(W, H, spp, wavefront=True, **kw)
            assert (sb["sorted"] & 8) and sa["segments"] == sb["segments"] and np.array_equal(a, b, equal_nan=True), (arm, W, H)
    small = gpu_ctx_factory(rt.Scene.reference(5, build_seed=1))
    c, sc_ = small.render(32, 32, 4, wavefront=True)      # sweep scenes keep their own kernels: the flag is ignored
    assert not (sc_["sorted"] & 8)


def test_interleaved_strips_and_shared_host_frame(rt, gpu_ctx_factory):
    """Image tiling over GPUs as ONE launch per GPU (rt1w_render_params.strip_rows / strip_period) and the host gather
    as device->host copies into one pinned whole-image frame (RT1W_OUT_FRAME): for 1, 2, 3 and 8 ranks the ranks'
    tiles, written by the library to their image positions, rebuild the single-render frame bit for bit; the packed form
    equals the rows it names; a narrow tile lands through the 2-D copy; bad parameters are refused."""
    import importlib
    sh = importlib.import_module("raytracing-1w_amd.sharding")
    sc = rt.Scene.reference(5, build_seed=1)
    ctx = gpu_ctx_factory(sc)
    W, H, spp = 96, 88, 8                      # 88 rows: five full 16-row strips and a ragged one
    chunk = sc.default_chunk(W, H, spp)
    full, _ = ctx.render(W, H, spp, chunk=chunk)
    for world in (1, 2, 3, 8):
        frame = rt.pinned_empty((H, W, 3))
        frame[:] = -1.0
        for rank in range(world):
            y0, rows, srows, period = sh.interleaved_tile(H, world, rank)
            if rows == 0:
                continue
            ctx.render(W, H, spp, tile=(0, y0, W, rows), strips=(srows, period), frame=frame, chunk=chunk)
            packed, _ = ctx.render(W, H, spp, tile=(0, y0, W, rows), strips=(srows, period), chunk=chunk)
            mine = [y for (sy, n) in sh.row_strips(H, world, rank) for y in range(sy, sy + n)]
            assert np.array_equal(packed, full[mine])
        assert np.array_equal(frame, full), world
    # contiguous narrow tile into a frame (2-D copy) + untouched remainder
    frame = rt.pinned_empty((H, W, 3))
    frame[:] = -1.0
    ctx.render(W, H, spp, tile=(10, 20, 30, 7), frame=frame, chunk=chunk)
    assert np.array_equal(frame[20:27, 10:40], full[20:27, 10:40])
    frame[20:27, 10:40] = -1.0
    assert (frame == -1.0).all()
    # pageable frames work too (slower copy, same bytes)
    plain = np.full((H, W, 3), -1.0)
    ctx.render(W, H, spp, tile=(0, 16, W, 16), frame=plain, chunk=chunk)
    assert np.array_equal(plain[16:32], full[16:32]) and (plain[:16] == -1.0).all()
    for bad in ((16, 0), (0, 16), (16, 8)):
        with pytest.raises(rt.Rt1wError):
            ctx.render(W, H, spp, tile=(0, 0, W, 16), strips=bad)
    with pytest.raises(rt.Rt1wError):          # the last strip would lie outside the image
        ctx.render(W, H, spp, tile=(0, 80, W, 32), strips=(16, 32))


def test_device_u8_equals_the_oracles_own_quantiser(rt, gpu_ctx_factory):
    """The integer pixel output of the product (quantised on the device) against the LITERAL oracle's frame pushed
    through the oracle's own quantiser (color.rs:56-65 restated in oracle.cpp) -- no product code on the expected side."""
    for arm, (W, H, spp) in ((5, (64, 64, 16)), (0, (96, 64, 8)), (7, (64, 64, 16))):
        ctx = gpu_ctx_factory(rt.Scene.reference(arm, build_seed=1))
        u8, _ = ctx.render_u8(W, H, spp)
        o = orc.OracleScene(arm, build_seed=1)
        lit, _ = o.render(W, H, spp)
        assert np.array_equal(u8, o.quantize(lit)[::-1]), arm


def test_c5_full_size_3840x2160_10000spp(rt, gpu_ctx_factory):
    """BASELINE C5 at FULL size on one GPU (8.29e10 paths, ~22 s) through rt1w_render_rows (strips, f64 means): crops
    against the CPU core build, NaN-free, the strip-wise frame's rows equal a one-shot tile render of the same rows."""
    sc = rt.Scene.reference(5, build_seed=1, aspect_ratio=16.0 / 9.0)
    ctx = gpu_ctx_factory(sc)
    W, H, spp = 3840, 2160, 10000
    seen = []
    full, st = ctx.render_rows(W, H, spp, progress=lambda d, t: seen.append((d, t)) and False)
    assert st["paths"] == W * H * spp and seen and seen[-1] == (H, H)
    assert np.isfinite(full).all() and 3.0 < st["segments"] / st["paths"] < 3.6
    chunk = sc.default_chunk(W, H, spp)
    for tile in ((1916, 1080, 4, 2), (8, 8, 2, 2)):
        b, sb = orc.flat_render(sc, W, H, spp, tile=tile, chunk=chunk)
        x0, y0, w, h = tile
        assert np.array_equal(full[y0:y0 + h, x0:x0 + w], b)
        literal_crop_check(5, 16.0 / 9.0, W, H, spp, tile, full[y0:y0 + h, x0:x0 + w], sb["segments"])
    one, _ = ctx.render(W, H, spp, tile=(0, 1072, W, 16), chunk=chunk)
    assert np.array_equal(one, full[1072:1088])
    # the ONE-SHOT entry on the same job: 20 chunks x 8.3 M pixels x 24 B = 4 GB of chunk partial sums in one launch
    whole, sw = ctx.render(W, H, spp)
    assert sw["n_chunks"] * W * H * 24 > 3.9e9 and sw["segments"] == st["segments"] and np.array_equal(whole, full)
    print(f"C5 full size: {st['total_ms'] / 1e3:.1f} s, {st['paths'] / st['total_ms'] / 1e3:.0f} Mpaths/s incl. D2H, "
          f"{st['segments'] / st['paths']:.3f} segments/path")


def test_c4_full_size_800x800_10000spp(rt, gpu_ctx_factory):
    """BASELINE C4 at FULL size on one GPU (6.4e9 paths): the whole frame at the reference's own 10 000 spp
    (main.rs:917-919) against next_week.png on its comparable blocks, tighter than the 200-spp test, + a crop against
    the CPU core build."""
    from test_golden import final_png_block_check, final_png_disc_check
    sc = rt.Scene.reference(7, build_seed=1)
    ctx = gpu_ctx_factory(sc)
    W = H = 800
    spp = 10000
    full, st = ctx.render_rows(W, H, spp)
    assert st["paths"] == W * H * spp
    final_png_block_check(full, 0.11, 0.02)
    final_png_disc_check(full, 0.08, "C4 full size: ")     # the literal objects (earth, moving sphere, blue ball): tighter than the blocks
    tile = (392, 300, 4, 2)
    b, sb = orc.flat_render(sc, W, H, spp, tile=tile, chunk=sc.default_chunk(W, H, spp))
    assert np.array_equal(full[300:302, 392:396], b, equal_nan=True)
    literal_crop_check(7, None, W, H, spp, tile, full[300:302, 392:396], sb["segments"])
    print(f"C4 full size: {st['total_ms'] / 1e3:.1f} s, {st['paths'] / st['total_ms'] / 1e3:.0f} Mpaths/s incl. D2H")


def test_gpu_reference_stream_reproduces_the_reference_png(rt, gpu_ctx_factory):
    """RT1W_RNG_REFERENCE: the HIP kernels drawing from the reference's own `StdRng::seed_from_u64(j*W+i)` (main.rs:964)
    render the reference's shipped default (Cornell 600x600, 100 spp, depth 50, main.rs:868-870) and the quantised frame
    is rest_of_your_life.png -- the Rust program's own output -- on every one of its 360 000 pixels (sha256 of the RGB
    bytes + per-row crc32 from tests/golden/cornell_png_pixels.json).  Also: equal to the CPU build of the same core on a
    crop, deterministic, and the default (Philox) frame is a different frame."""
    import hashlib, zlib
    pix = json.load(open(os.path.join(HERE, "golden", "cornell_png_pixels.json")))
    sc = rt.Scene.reference(5, build_seed=1)
    ctx = gpu_ctx_factory(sc)
    u8, st = ctx.render_u8(600, 600, 100, reference_stream=True)
    assert st["sorted"] & 16 and st["n_chunks"] == 1
    assert st["sorted"] & 1, "the reference stream did not go through the reordering kernel"   # round 4: the generator state travels with the path
    bad = [r for r in range(600) if zlib.crc32(np.ascontiguousarray(u8[r]).tobytes()) != pix["row_crc32_top_down"][r]]
    assert not bad, f"{len(bad)} rows differ from the reference PNG, first: {bad[:5]}"
    assert hashlib.sha256(np.ascontiguousarray(u8).tobytes()).hexdigest() == pix["sha256_rgb_top_down"]
    f64, _ = ctx.render(600, 600, 100, tile=(200, 300, 16, 8), reference_stream=True)
    cpu, _ = orc.flat_render(sc, 600, 600, 100, tile=(200, 300, 16, 8), chunk=100, lib=orc.flat_ref_lib())
    assert np.array_equal(f64, cpu)
    again, _ = ctx.render_u8(600, 600, 100, reference_stream=True)
    assert np.array_equal(again, u8)
    philox, _ = ctx.render_u8(600, 600, 100)
    assert (philox != u8).any()
    full, sf = ctx.render(600, 600, 100, reference_stream=True)
    plain, sp = ctx.render(600, 600, 100, reference_stream=True, unsorted=True)      # one lane per pixel for all samples: round 2's form
    assert (sf["sorted"] & 17) == 17 and sp["sorted"] & 16 and not (sp["sorted"] & 1)
    assert sp["segments"] == sf["segments"] == st["segments"] and np.array_equal(plain, full)
    with pytest.raises(rt.Rt1wError):
        ctx.render(64, 64, 4, sample_offset=2, reference_stream=True)
    # a big scene goes through the stack-walk build of the same kernel: equal to the CPU build of the core
    big = rt.Scene.reference(0, build_seed=1, aspect_ratio=1.5)
    g, sg = gpu_ctx_factory(big).render(96, 64, 6, reference_stream=True)
    c, sc_ = orc.flat_render(big, 96, 64, 6, chunk=6, lib=orc.flat_ref_lib(), variant=3)
    assert sg["segments"] == sc_["segments"] and np.array_equal(g, c)


def test_f32_mode_matches_the_f64_frame_statistically(rt, gpu_ctx_factory):
    """RT1W_PRECISION_F32 (the reference's `type Float = f32`, main.rs:1): same scene, same streams, f32
    arithmetic.  Parity is statistical: at 600x600x256 spp the 8-bit 100x100-block means of the f32 and f64 frames agree
    within 1/255 (measured 0.65) and the global channel means within 0.1/255 (the two frames share their random numbers, so most paths
    are the same paths and the difference is far below the Monte-Carlo noise of either); no NaN pixel, and no more pixels that are black in f32 only than
    twice the literal f32 oracle's own count for this frame (5, so 10: tests/golden/f32_nonfinite_census.json, which accounts for each -- a
    diffuse hit at the very height of the light's plane, the reference's own 0 / 0, and one pixel on a mirror's edge that no NaN touches;
    measured on the MI355X: 7 -- the twin's 6 and [417, 254], where the product's path leaves the twin's at its first sinf / cosf and goes
    non-finite a bounce later; 10 before the draw contract of include/rt1w_num.h); and explicitly at the reference's thin spots: the k = 555 walls, whose BVH boxes are
    0.0001 thick (aarect.rs:74-79) = 1.6 f32 ulps -- the rows and columns next to the walls show no holes (their means
    stay within 2 % of the f64 frame's) -- and t_min = 0.001 (main.rs:62): no acne, i.e. the floor's mean is unchanged."""
    ctx = gpu_ctx_factory(rt.Scene.reference(5, build_seed=1))
    W = H = 600
    a, sa = ctx.render(W, H, 256)
    b, sb = ctx.render(W, H, 256, f32=True)
    assert sb["sorted"] & 32 and np.isfinite(b).all()
    if sb["sorted"] & 4:   # the scene-specialised f32 kernel (kernel cache / hiprtc) does the generic f32 kernel's arithmetic
        g32, sg32 = ctx.render(W, H, 256, f32=True, generic=True)
        assert not (sg32["sorted"] & 4) and sg32["segments"] == sb["segments"] and np.array_equal(b, g32)
    assert abs(sb["segments"] / sa["segments"] - 1.0) < 0.03          # f32 paths run 1.5 % longer (measured)
    qa, qb = rt.quantize(a).astype(np.float64), rt.quantize(b).astype(np.float64)
    assert np.abs(qa.mean(axis=(0, 1)) - qb.mean(axis=(0, 1))).max() < 0.1
    blocks = (qa - qb).reshape(6, 100, 6, 100, 3).mean(axis=(1, 3))
    assert np.abs(blocks).max() < 1.0, np.abs(blocks).max()          # measured 0.65
    # pixels that are black in f32 only (color.rs:16-18 scrubs a NaN sum to zero): the literal f32 oracle's own count for this frame,
    # computed on the CPU and stored with the census, allowed twice (paths the five single-precision functions send elsewhere), 2 at the least
    census = json.load(open(os.path.join(HERE, "golden", "f32_nonfinite_census.json")))
    allowed = max(2, 2 * census["cornell_literal_zero_pixel_count"])
    black = np.argwhere((b == 0).all(axis=2) & ~(a == 0).all(axis=2))
    print(f"\nf32-only black pixels: {len(black)} (allowed {allowed}): {black.tolist()}")
    assert len(black) <= allowed, black.tolist()
    for sl in (np.s_[:, 5:25], np.s_[:, -25:-5], np.s_[5:25, :], np.s_[-25:-5, :]):      # next to the four walls in the picture
        ra, rb = a[sl].mean(), b[sl].mean()
        assert abs(rb / ra - 1.0) < 0.03, (ra, rb)
    # every arm renders in f32 and stays close to its f64 frame
    for arm, aspect, (w, h, spp) in ((0, 1.5, (240, 160, 32)), (6, None, (128, 128, 32)), (7, None, (128, 128, 32)), (2, None, (128, 72, 16))):
        c = gpu_ctx_factory(rt.Scene.reference(arm, build_seed=1, aspect_ratio=aspect))
        x, _ = c.render(w, h, spp)
        y, sy = c.render(w, h, spp, f32=True)
        assert sy["sorted"] & 32 and np.isfinite(y).all()
        assert abs(y.mean() / x.mean() - 1.0) < 0.03, (arm, x.mean(), y.mean())
    with pytest.raises(rt.Rt1wError):
        ctx.render(64, 64, 4, f32=True, reference_stream=True)


def test_f32_mode_against_the_f32_oracle(rt, gpu_ctx_factory):
    """The expected side of RT1W_PRECISION_F32 that is NOT the product: the literal oracle built with the reference's own precision switch
    thrown, `type Float = f32` (main.rs:1; oracle/oracle_f32.cpp -> liborc_f32.so), whose block means are committed under
    tests/golden/oracle_f32_blocks.json (make_golden.py f32).  Same scene, same Philox streams, so most paths are the same paths; what
    differs is the last f32 ulp here and there (the device evaluates sin / cos / acos / atan2 / ln of a float in single precision, the
    oracle in 64 bits rounded once; the device's BVH boxes are widened by 1e-5, context_f32.hip) and the paths that ulp sends elsewhere.
    Bounds: segments per path within 0.5 %, the frame mean within 0.5 %, every block's linear mean within 2.5 % of the oracle's
    (+ 0.002 absolute for the near-black blocks), no NaN.  random_scene runs the pair walk in this precision too."""
    gold = json.load(open(os.path.join(HERE, "golden", "oracle_f32_blocks.json")))["cases"]
    worst = {}
    for name, g in gold.items():
        W, H, spp, blk = g["W"], g["H"], g["spp"], g["block"]
        ctx = gpu_ctx_factory(rt.Scene.reference(g["arm"], build_seed=1, aspect_ratio=g["aspect"]))
        img, st = ctx.render(W, H, spp, f32=True)
        assert st["sorted"] & 32 and np.isfinite(img).all(), name
        if g["arm"] == 0:
            assert st["sorted"] & 128, "random_scene in f32 did not run the pair-walk kernel"
            classic, sc_ = ctx.render(W, H, spp, f32=True, classic_walk=True)
            assert not (sc_["sorted"] & 128)
            # f32 pair walk against the f32 one-entry-per-step walk: the same boxes gate the same spheres -- the same frame
            assert sc_["segments"] == st["segments"] and np.array_equal(classic, img), "f32 pair walk differs from the f32 stack walk"
        want = np.array(g["block_means_bottom_up"])
        got = img.reshape(H // blk, blk, W // blk, blk, 3).mean(axis=(1, 3))
        rel = np.abs(got - want) / (np.abs(want) + 0.08)
        worst[name] = (float(rel.max()), st["segments"] / g["segments"] - 1.0, float(img.mean() / g["mean"] - 1.0))
        print(name, "worst block %.4f  segments %+.4f  mean %+.4f" % worst[name])
        assert abs(st["segments"] / g["segments"] - 1.0) < 0.005, (name, st["segments"], g["segments"])
        assert abs(img.mean() / g["mean"] - 1.0) < 0.005, (name, img.mean(), g["mean"])
        assert rel.max() < 0.025, (name, float(rel.max()))
        ctx.close()


def test_cli_with_the_reference_stream_prints_the_reference_programs_output(rt, tmp_path):
    """`rt1w --reference-stream` with no other option is the reference's `main` as shipped (match 5 -> Cornell, 600x600,
    100 spp, depth 50; main.rs:815,868-870): its P3 text, parsed back, is rest_of_your_life.png on every pixel -- i.e. the
    bytes `cargo run` of the reference prints.  Wavefront edge cases ride along: depths below / at the number of
    wavefront bounces and depth 0 equal the megakernel."""
    import hashlib, subprocess
    pix = json.load(open(os.path.join(HERE, "golden", "cornell_png_pixels.json")))
    exe = os.path.join(orc.ROOT, "raytracing-1w_amd", "rt1w")
    out = tmp_path / "ref.ppm"
    subprocess.check_call([exe, "--reference-stream", "--out", str(out)], stderr=subprocess.DEVNULL)
    tok = out.read_text().split()
    assert tok[:4] == ["P3", "600", "600", "255"]
    img = np.array(tok[4:], dtype=np.uint8).reshape(600, 600, 3)
    assert hashlib.sha256(img.tobytes()).hexdigest() == pix["sha256_rgb_top_down"]


def test_wavefront_depth_edge_cases(rt, gpu_ctx_factory):
    ctx = gpu_ctx_factory(rt.Scene.reference(0, build_seed=1, aspect_ratio=1.5))
    for depth in (0, 1, 3, 6, 7):
        a, sa = ctx.render(72, 48, 6, max_depth=depth)
        b, sb = ctx.render(72, 48, 6, max_depth=depth, wavefront=True)
        assert (sb["sorted"] & 8) and sa["segments"] == sb["segments"] and np.array_equal(a, b, equal_nan=True), depth
    with pytest.raises(rt.Rt1wError):
        ctx.render(72, 48, 2, max_depth=65, wavefront=True)          # beyond WF_MAX_BOUNCES: refused, not silently different


def test_pair_walk_of_sphere_scenes_is_bit_identical(rt, gpu_ctx_factory):
    """Sphere scenes (random_scene, BASELINE C2) walk their BVH with the pair walk of csrc/rt_walk_pair.h by default: box work and
    leaf work in separate wave phases, inner boxes in f32 rounded outward, every sphere gated by its group's own f64 box at the
    reference's moment.  The frame must equal the one-entry-per-step walk's (RT1W_CLASSIC_WALK) and the CPU build of the core,
    bit for bit, with equal segment counts -- on the reference's tree and on the SAH tree, at sizes where lanes suspend and
    resume their walks (slices) and take new work items."""
    for sah in (False, True):
        sc = rt.Scene.reference(0, build_seed=1, aspect_ratio=1.5)
        if sah:
            sc.set_bvh_build(True)
        ctx = gpu_ctx_factory(sc)
        for W, H, spp in ((96, 64, 8), (600, 400, 3)):
            a, sa = ctx.render(W, H, spp)
            b, sb = ctx.render(W, H, spp, classic_walk=True)
            assert sa["sorted"] & 128 and not (sb["sorted"] & 128), (sa["sorted"], sb["sorted"])
            assert sa["segments"] == sb["segments"] and np.array_equal(a, b, equal_nan=True), (sah, W, H, spp)
        cpu, sc_ = orc.flat_render(sc, 96, 64, 8, chunk=sc.default_chunk(96, 64, 8))
        a, sa = ctx.render(96, 64, 8)
        assert sa["segments"] == sc_["segments"] and np.array_equal(a, cpu, equal_nan=True), sah
        ctx.close()
    # other build seeds (other trees, other sphere placements), a tile, a sample offset
    for seed in (2, 3):
        sc = rt.Scene.reference(0, build_seed=seed, aspect_ratio=1.5)
        ctx = gpu_ctx_factory(sc)
        a, sa = ctx.render(300, 200, 4, tile=(16, 8, 200, 120), sample_offset=3)
        b, sb = ctx.render(300, 200, 4, tile=(16, 8, 200, 120), sample_offset=3, classic_walk=True)
        assert sa["sorted"] & 128 and sa["segments"] == sb["segments"] and np.array_equal(a, b, equal_nan=True), seed
        ctx.close()
    # a scene the pair walk does not cover keeps the one-entry-per-step walk
    ctx = gpu_ctx_factory(rt.Scene.reference(7, build_seed=1))
    _, st = ctx.render(32, 32, 2)
    assert not (st["sorted"] & 128)


def test_sphere_media_kernels_are_bit_identical(rt, gpu_ctx_factory):
    """Scenes whose every ConstantMedium is bounded by a bare Sphere (final_scene, main.rs:730-752) run stack-walk kernels built
    without the general boundary walks (rt_flat.h: RtCfgSphereMedia; stats.sorted bit 8).  Same frame as the general kernel
    (RT1W_CLASSIC_WALK) and as the CPU build of the core, on the reference's tree, the SAH tree and with the near-far order (V4);
    a scene with a medium inside a box (not a bare sphere) must keep the general kernel."""
    for sah, near_far in ((False, False), (True, False), (True, True)):
        sc = rt.Scene.reference(7, build_seed=1)
        if sah:
            sc.set_bvh_build(True)
        if near_far:
            sc.set_walk_order(True)
        ctx = gpu_ctx_factory(sc)
        for W, H, spp in ((64, 64, 6), (320, 320, 3)):
            a, sa = ctx.render(W, H, spp)
            b, sb = ctx.render(W, H, spp, classic_walk=True)
            assert sa["sorted"] & 256 and not (sb["sorted"] & 256), (sa["sorted"], sb["sorted"])
            assert sa["variant"] == sb["variant"] == (4 if near_far else 3)
            assert sa["segments"] == sb["segments"] and np.array_equal(a, b, equal_nan=True), (sah, near_far, W, H, spp)
        cpu, sc_ = orc.flat_render(sc, 64, 64, 6, chunk=sc.default_chunk(64, 64, 6))
        a, sa = ctx.render(64, 64, 6)
        assert sa["segments"] == sc_["segments"] and np.array_equal(a, cpu, equal_nan=True), (sah, near_far)
        ctx.close()
    # media bounded by boxes under wrappers (cornel_smoke, main.rs:528-546) keep the general kernel, also when the stack walk is forced
    sc = rt.Scene.reference(6, build_seed=1)
    ctx = gpu_ctx_factory(sc)
    a, sa = ctx.render(48, 48, 4, variant=3)
    assert sa["variant"] == 3 and not (sa["sorted"] & 256)
    cpu, sc_ = orc.flat_render(sc, 48, 48, 4, chunk=sc.default_chunk(48, 48, 4))
    assert sa["segments"] == sc_["segments"] and np.array_equal(a, cpu, equal_nan=True)
    ctx.close()


def test_specialised_kernels_are_built_for_the_waves_their_shading_allows(rt, gpu_ctx_factory):
    """jit.cpp builds a scene's specialised f64 kernel for four waves per SIMD (128 VGPRs, the exchange in two rounds, four workgroups per
    CU) unless the scene has a noise or checker texture, whose shading code would spill at 128 and which keep three waves (168 VGPRs,
    one round).  What a render computes does not depend on it: both forms against the CPU build of the core."""
    grids = {}
    for arm, four in ((5, True), (6, True), (3, True), (2, False), (1, False), (4, False)):
        sc = rt.Scene.reference(arm, build_seed=1)
        ctx = gpu_ctx_factory(sc)
        info = ctx.specialise()
        assert info["active"]
        assert (info["vgprs"] <= 128) == four, (arm, info)
        grids[arm] = info["grid"]
        W, H, spp = (48, 48, 8) if arm != 3 else (48, 27, 8)
        g, sg = ctx.render(W, H, spp)
        assert sg["sorted"] & 4
        b, sb = orc.flat_render(sc, W, H, spp, chunk=sg["chunk"])
        assert sg["segments"] == sb["segments"] and np.array_equal(g, b, equal_nan=True), arm
        ctx.close()
    assert grids[5] * 3 == grids[2] * 4, grids  # four workgroups per CU against three


def test_node_cache_kernels_are_bit_identical(rt, gpu_ctx_factory):
    """Big scenes' stack-walk kernels read their node records through the scene's WALK TABLE (csrc/rt_walk_table.h) and keep its first 256
    records -- the most visited nodes, ranked by a visit count the context takes at creation -- in LDS (stats.sorted bit 10 = 1024).
    Where a record is read from changes nothing: same frame and segment count as the same kernels without the cache
    (RT1W_NO_NODE_CACHE) and as the CPU build of the core walking the node array -- final_scene on the three trees and the near-far
    order (sphere-media builds of V3 / V4), its general-media build (RT1W_CLASSIC_WALK), random_scene's one-entry-per-step renders
    (V5, V2), tiles, sample offsets, tiny frames, several samples per work item."""
    for build, near_far in (("best_axis", False), ("reference", False), ("sah", True)):
        sc = rt.Scene.reference(7, build_seed=1).set_bvh_build(build)
        if near_far:
            sc.set_walk_order(True)
        ctx = gpu_ctx_factory(sc)
        for W, H, spp, kw in ((64, 64, 6, {}), (320, 320, 3, {}), (13, 9, 5, {}), (96, 80, 8, dict(tile=(16, 8, 50, 37), sample_offset=3)),
                              (48, 48, 24, dict(chunk=8)), (64, 64, 6, dict(classic_walk=True))):
            if near_far and "classic_walk" in kw:
                continue  # the near-far order's general-media build has no reordering form: the plain kernel runs, with or without the flag
            a, sa = ctx.render(W, H, spp, **kw)
            b, sb = ctx.render(W, H, spp, no_node_cache=True, **kw)
            assert sa["sorted"] & 1024 and sa["sorted"] & 512 and not (sb["sorted"] & 1024) and sb["sorted"] & 512, (sa["sorted"], sb["sorted"])
            assert bool(sa["sorted"] & 256) == ("classic_walk" not in kw)
            assert sa["variant"] == sb["variant"] == (4 if near_far else 3)
            assert sa["segments"] == sb["segments"] and np.array_equal(a, b, equal_nan=True), (build, near_far, W, H, spp, kw)
        cpu, sc_ = orc.flat_render(sc, 64, 64, 6, chunk=sc.default_chunk(64, 64, 6))
        a, sa = ctx.render(64, 64, 6)
        assert sa["sorted"] & 1024 and sa["segments"] == sc_["segments"] and np.array_equal(a, cpu, equal_nan=True), (build, near_far)
        ctx.close()
    sc = rt.Scene.reference(0, build_seed=1, aspect_ratio=1.5)
    ctx = gpu_ctx_factory(sc)
    base, sb = ctx.render(96, 64, 6)
    assert sb["sorted"] & 128 and not (sb["sorted"] & 1024)       # the pair walk has its own records
    for kw in (dict(classic_walk=True), dict(variant=2)):
        a, sa = ctx.render(96, 64, 6, **kw)
        b, sb2 = ctx.render(96, 64, 6, no_node_cache=True, **kw)
        assert sa["sorted"] & 1024 and not (sb2["sorted"] & 1024) and not (sa["sorted"] & 128), (kw, sa["sorted"], sb2["sorted"])
        assert sa["segments"] == sb2["segments"] == sb["segments"] and np.array_equal(a, b, equal_nan=True) and np.array_equal(a, base, equal_nan=True), kw
    ctx.close()


def test_slice_sorted_kernels_are_bit_identical(rt, gpu_ctx_factory):
    """The default kernels of sphere-media scenes (final_scene) reorder the paths whose walk has ended across the workgroup at the
    end of every slice of the stack walk (rt_kernel_plain.h: rt_render_ss_body; stats.sorted bit 9 = 512): which lane shades a
    path changes, nothing else.  Same frame and segment count as the plain sliced kernel (RT1W_UNSORTED) and as the CPU build of
    the core -- reference tree, SAH tree, near-far order (V4), tiles, sample offsets, frames smaller than one workgroup's lanes
    (retired lanes take part in the exchange) and several samples per work item."""
    for sah, near_far in ((False, False), (True, True)):
        sc = rt.Scene.reference(7, build_seed=1)
        if sah:
            sc.set_bvh_build(True)
        if near_far:
            sc.set_walk_order(True)
        ctx = gpu_ctx_factory(sc)
        for W, H, spp, kw in ((64, 64, 6, {}), (320, 320, 3, {}), (13, 9, 5, {}), (96, 80, 8, dict(tile=(16, 8, 50, 37), sample_offset=3)),
                              (48, 48, 24, dict(chunk=8))):
            a, sa = ctx.render(W, H, spp, **kw)
            b, sb = ctx.render(W, H, spp, unsorted=True, **kw)
            assert sa["sorted"] & 512 and sa["sorted"] & 256 and not (sb["sorted"] & 512) and sb["sorted"] & 256, (sa["sorted"], sb["sorted"])
            assert sa["variant"] == sb["variant"] == (4 if near_far else 3)
            assert sa["segments"] == sb["segments"] and np.array_equal(a, b, equal_nan=True), (sah, near_far, W, H, spp, kw)
        cpu, sc_ = orc.flat_render(sc, 64, 64, 6, chunk=sc.default_chunk(64, 64, 6))
        a, sa = ctx.render(64, 64, 6)
        assert sa["sorted"] & 512 and sa["segments"] == sc_["segments"] and np.array_equal(a, cpu, equal_nan=True), (sah, near_far)
        ctx.close()
    # sphere scenes: the pair walk in slices + the same reordering (bits 7 and 9); with the one-entry-per-step walk (V5, V2) as well
    for sah in (False, True):
        sc = rt.Scene.reference(0, build_seed=1, aspect_ratio=1.5)
        if sah:
            sc.set_bvh_build(True)
        ctx = gpu_ctx_factory(sc)
        for W, H, spp, kw in ((96, 64, 6, {}), (300, 200, 3, {}), (17, 11, 5, {}), (96, 64, 24, dict(chunk=8, tile=(8, 8, 60, 40)))):
            a, sa = ctx.render(W, H, spp, **kw)
            b, sb = ctx.render(W, H, spp, unsorted=True, **kw)
            assert sa["sorted"] & 512 and sa["sorted"] & 128 and not (sb["sorted"] & 512) and sb["sorted"] & 128, (sa["sorted"], sb["sorted"])
            assert sa["segments"] == sb["segments"] and np.array_equal(a, b, equal_nan=True), (sah, W, H, spp, kw)
            for kw2 in (dict(classic_walk=True), dict(variant=2)):
                c_, sc2 = ctx.render(W, H, spp, **kw, **kw2)
                assert sc2["sorted"] & 512 and not (sc2["sorted"] & 128), (kw2, sc2["sorted"])
                assert sc2["segments"] == sb["segments"] and np.array_equal(c_, b, equal_nan=True), (sah, W, H, spp, kw, kw2)
        cpu, sc_ = orc.flat_render(sc, 96, 64, 6, chunk=sc.default_chunk(96, 64, 6))
        a, sa = ctx.render(96, 64, 6)
        assert sa["segments"] == sc_["segments"] and np.array_equal(a, cpu, equal_nan=True), sah
        ctx.close()
    # the f32 builds of the stack-walk kernels reorder the same way: within f32 mode the frame does not depend on it, bit for bit
    for arm, aspect, W, H, spp in ((7, 1.0, 96, 96, 4), (0, 1.5, 96, 64, 4)):
        ctx = gpu_ctx_factory(rt.Scene.reference(arm, build_seed=1, aspect_ratio=aspect))
        a, sa = ctx.render(W, H, spp, f32=True)
        b, sb = ctx.render(W, H, spp, f32=True, unsorted=True)
        assert sa["sorted"] & 32 and sa["sorted"] & 512 and sb["sorted"] & 32 and not (sb["sorted"] & 512), (sa["sorted"], sb["sorted"])
        assert sa["segments"] == sb["segments"] and np.array_equal(a, b, equal_nan=True), arm
        ctx.close()
    # media with general boundaries (cornel_smoke's boxes under wrappers) through the forced stack walk, and random graphs: every
    # stack variant a graph admits, reordered against plain against the CPU build of the core
    cases = [(rt.Scene.reference(6, build_seed=1), 48, 48, 4)] + [(random_scene_pair(4100 + s_)[0], 56, 40, 3) for s_ in range(8)]
    n_media = 0
    for sc, W, H, spp in cases:
        info = sc.info()
        ctx = gpu_ctx_factory(sc)
        cpu, sc_ = orc.flat_render(sc, W, H, spp, chunk=sc.default_chunk(W, H, spp))
        for v in [3] + ([2] if not info["has_media"] else []) + ([5] if (not info["has_media"] and info["scope_depth"] == 0) else []):
            a, sa = ctx.render(W, H, spp, variant=v)
            b, sb = ctx.render(W, H, spp, variant=v, unsorted=True)
            assert sa["variant"] == sb["variant"] == v and sa["sorted"] & 512 and not (sb["sorted"] & 512), (v, sa["sorted"], sb["sorted"])
            assert sa["segments"] == sb["segments"] == sc_["segments"], (v, info)
            assert np.array_equal(a, b, equal_nan=True) and np.array_equal(a, cpu, equal_nan=True), (v, info)
        n_media += info["has_media"]
        ctx.close()
    assert n_media >= 2


def test_precompiled_kernels_load_on_a_host_without_the_runtime_compiler(rt):
    """A host that cannot compile (no libhiprtc: RT1W_NO_HIPRTC hides it) still runs the scene-specialised kernels the build
    precompiled under <package>/kernels -- their key no longer contains the host's compiler id (round-2 advice)."""
    import subprocess
    import sys
    code = ("import importlib, sys; sys.path.insert(0, %r); rt = importlib.import_module('raytracing-1w_amd'); "
            "ctx = rt.Context(rt.Scene.reference(5, build_seed=1), 0); i = ctx.specialise(cached_only=True); "
            "g, st = ctx.render(32, 32, 2); print(int(i['active']), int(i['from_cache']), st['sorted'] & 4)" % orc.ROOT)
    env = dict(os.environ, RT1W_NO_HIPRTC="1", RT1W_KERNEL_CACHE="/nonexistent-rt1w-cache")
    out = subprocess.check_output([sys.executable, "-c", code], env=env).decode().split()
    assert out == ["1", "1", "4"], out


def test_one_sample_per_work_item_and_sample_passes(rt, gpu_ctx_factory):
    """Scenes on the stack-walk kernels render with ONE sample per work item by default (rt1w_scene_default_chunk: free lanes of a wave restart
    together on neighbouring pixels; the pixel sum is the reference's own sequential sum, main.rs:966-992), and a render whose chunk partial
    sums would not fit the budget (default 8 GiB; here `partial_mib` makes it 1-2 MiB) runs as several passes over sample ranges.  What
    must hold: the default chunk is 1 and the frame equals the CPU build of the core with chunk 1 bit for bit; the same frame whatever the
    budget (1 pass, 3 or more passes with a ragged last one, a pass per sample), raw sums (RT1W_OUT_SUM), a sample offset and a tile,
    chunks of 3 samples with a ragged last chunk split over passes; the small scenes keep the scene-independent rule; equal segment
    counts throughout; stats.passes as chunks_per_pass (context.hip) counts them.  The frames are large enough (589 824 and 614 400 B
    of partial sums per chunk) that one chunk fills a 1 MiB pass and three fill 2 MiB."""
    def passes(W, H, spp, chunk, mib):
        n_chunks = -(-spp // chunk)
        per_pass = min(max(1, (mib << 20) // (W * H * 24)), n_chunks)
        return -(-n_chunks // per_pass)
    for arm, aspect, W, H, spp in ((0, 1.5, 192, 128, 10), (7, None, 160, 160, 7)):
        sc = rt.Scene.reference(arm, build_seed=1, aspect_ratio=aspect)
        assert sc.default_chunk(W, H, spp) == 1 and sc.default_chunk(1200, 800, 500) == 1
        ctx = gpu_ctx_factory(sc)
        full, st = ctx.render(W, H, spp)
        assert st["chunk"] == 1 and st["n_chunks"] == spp and st["passes"] == 1
        cpu, sc_ = orc.flat_render(sc, W, H, spp, chunk=1)
        assert st["segments"] == sc_["segments"] and np.array_equal(full, cpu, equal_nan=True), arm
        assert passes(W, H, spp, 1, 2) >= 3 and spp % 3 != 0 and passes(W, H, spp, 1, 1) == spp and passes(W, H, spp, 3, 1) >= 3
        for mib in (2, 1):                                                                          # 3 chunks per pass (ragged), one pass per sample
            got, sg = ctx.render(W, H, spp, partial_mib=mib)
            assert sg["passes"] == passes(W, H, spp, 1, mib), (arm, mib, sg["passes"])
            assert sg["segments"] == st["segments"] and sg["n_chunks"] == spp and np.array_equal(got, full, equal_nan=True), (arm, mib)
        raw, sr = ctx.render(W, H, spp, out_sum=True, partial_mib=1)
        assert sr["passes"] == spp and np.array_equal(rt.resolve(raw, spp), full, equal_nan=True), arm
        off, so = ctx.render(W, H, 4, sample_offset=3, tile=(8, 16, 32, 24), partial_mib=1)
        cpu_off, _ = orc.flat_render(sc, W, H, 4, sample_offset=3, tile=(8, 16, 32, 24), chunk=1)
        assert np.array_equal(off, cpu_off, equal_nan=True), arm
        cpu3, s3c = orc.flat_render(sc, W, H, spp, chunk=3)
        for mib in (1, 2):                                                                          # explicit chunks also run in passes
            three, s3 = ctx.render(W, H, spp, chunk=3, partial_mib=mib)
            assert s3["chunk"] == 3 and s3["passes"] == passes(W, H, spp, 3, mib), (arm, mib, s3["passes"])
            assert s3["segments"] == s3c["segments"] and np.array_equal(three, cpu3, equal_nan=True), (arm, mib)
        ctx.close()
    small = rt.Scene.reference(5, build_seed=1)
    assert small.default_chunk(600, 600, 1000) == rt.default_chunk(600, 600, 1000) > 1
