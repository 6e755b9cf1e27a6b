"""Pixel seeds at and above 2^32, and the top of the sample range.

The per-pixel seed is (uint64_t)j * width + i (rt_core.h: rt_path_begin_cam).  Its high word is the second Philox key word
(rt1w_num.h: rt_rng_pixel_sample) and, in reference-stream mode, the high half of the PCG state that seed_from_u64 expands.  Below
2^32 that word is always 0, so every smaller frame would pass with it dropped or mangled.  The image here is W x H = 100 003 x 50 021
(5.0e9 pixels): the tiles straddle the pixel whose seed is exactly 2^32, lie in the image's far corner (where the Cornell box's camera
sees only the void around the box) and inside the box's top wall, with seeds of about 4.8e9.

CPU tier: the CPU build of the kernel core against the literal oracle (Philox) and against oracle/refstream.h's independent ChaCha
restatement (reference stream).  GPU tier: the same tiles through the render entries, against the CPU core.
"""
import numpy as np
import pytest

import orc

W, H = 100_003, 50_021
J0 = 2 ** 32 // W
I0 = 2 ** 32 - J0 * W
STRADDLE = (I0 - 16, J0 - 8, 32, 16)          # seeds from 2^32 - 8 W - 16 to 2^32 + 7 W + 15
CORNER = (W - 32, H - 16, 32, 16)             # the largest seeds of the image, about 5.0e9
HIGH = (W - 10_032, H - 2_016, 32, 16)         # seeds of about 4.8e9 where both scenes have geometry
TILES = (STRADDLE, CORNER, HIGH)
IDS = ("straddle", "corner", "high")
TOP = 0xFFFFFFFF                               # validate: sample_offset + spp <= 0xFFFFFFFF
RTOL = 1e-12


def close(a, b):
    both_nan = np.isnan(a) & np.isnan(b)
    return bool((both_nan | (np.abs(a - b) <= RTOL * np.abs(a)) | (a == b)).all())


def seeds(tile):
    x0, y0, tw, th = tile
    j = np.arange(y0, y0 + th, dtype=np.uint64)[:, None]
    i = np.arange(x0, x0 + tw, dtype=np.uint64)[None, :]
    return j * np.uint64(W) + i


def test_the_tiles_cover_seeds_with_a_high_word():
    s = seeds(STRADDLE)
    assert s.min() < 2 ** 32 <= s.max() and (s == 2 ** 32).sum() == 1
    assert seeds(CORNER).max() == W * H - 1 and seeds(CORNER).min() >> 32 == 1 and seeds(HIGH).min() >> 32 == 1


@pytest.mark.parametrize("arm", (5, 7))
@pytest.mark.parametrize("tile", TILES, ids=IDS)
def test_core_matches_the_literal_oracle_at_64_bit_seeds(rt, arm, tile):
    sc = rt.Scene.reference(arm, build_seed=1)
    lit = orc.OracleScene(arm, build_seed=1)
    a, sa = orc.flat_render(sc, W, H, 4, tile=tile)
    b, sb = lit.render(W, H, 4, tile=tile)
    assert sa["segments"] == sb["segments"] and close(b, a), (arm, tile)
    if tile != CORNER or arm == 7:
        assert sa["segments"] > 1.5 * sa["paths"] and a.mean() > 0, "the tile must see geometry, or the streams hardly matter"


@pytest.mark.parametrize("tile", TILES, ids=IDS)
def test_core_reference_stream_matches_refstream_h_at_64_bit_seeds(rt, tile):
    """The product's ChaCha12 / seed_from_u64 restatement (rt1w_num.h) against oracle/refstream.h's, with the seed's high word set."""
    sc = rt.Scene.reference(5, build_seed=1)
    a, sa = orc.flat_render(sc, W, H, 6, tile=tile, chunk=6, lib=orc.flat_ref_lib())
    b, sb = orc.OracleScene(5, build_seed=1, refstream=True).render(W, H, 6, tile=tile)
    assert sa["segments"] == sb["segments"] and close(b, a), tile


@pytest.mark.parametrize("arm", (5, 7))
def test_core_matches_the_literal_oracle_at_the_top_of_the_sample_range(rt, arm):
    """The last samples validate accepts (sample_offset + spp == 0xFFFFFFFF) and the largest global seed."""
    sc = rt.Scene.reference(arm, build_seed=1)
    lit = orc.OracleScene(arm, build_seed=1)
    spp = 5
    for kw in ({"sample_offset": TOP - spp}, {"global_seed": TOP}, {"sample_offset": TOP - spp, "global_seed": TOP}):
        a, sa = orc.flat_render(sc, W, H, spp, tile=STRADDLE, **kw)
        b, sb = lit.render(W, H, spp, tile=STRADDLE, **kw)
        assert sa["segments"] == sb["segments"] and close(b, a), (arm, kw)
    low, _ = orc.flat_render(sc, W, H, spp, tile=STRADDLE)
    assert not np.array_equal(low, a), "the sample offset and global seed did not reach the stream"


# ---- GPU tier ----

@pytest.mark.gpu
@pytest.mark.parametrize("arm", (5, 7))
def test_gpu_entries_at_64_bit_seeds(rt, gpu_ctx_factory, arm):
    """Default, reference-stream, render_rows and AOV entries equal the CPU core (or the AOV twin) bit for bit on both tiles; the
    f32 frame is finite and equal to the f64 frame in the mean, within its noise."""
    sc = rt.Scene.reference(arm, build_seed=1)
    ctx = gpu_ctx_factory(sc)
    for tile in TILES:
        img, st = ctx.render(W, H, 8, tile=tile)
        cpu, sc_ = orc.flat_render(sc, W, H, 8, tile=tile, chunk=st["chunk"])
        assert st["segments"] == sc_["segments"] and np.array_equal(img, cpu, equal_nan=True), (arm, tile)
        rows, sr = ctx.render_rows(W, H, 8, strip_rows=8, tile=tile, chunk=st["chunk"])
        assert sr["segments"] == st["segments"] and np.array_equal(rows, img, equal_nan=True), (arm, tile)
        ref, sref = ctx.render(W, H, 6, tile=tile, reference_stream=True)
        cref, scref = orc.flat_render(sc, W, H, 6, tile=tile, chunk=6, lib=orc.flat_ref_lib(), variant=sref["variant"])
        assert sref["segments"] == scref["segments"] and np.array_equal(ref, cref, equal_nan=True), (arm, tile)
        aov = ctx.render_aov(W, H, 4, tile=tile, sample_offset=3, global_seed=2)
        assert np.array_equal(aov, rt.aov_host(sc, W, H, 4, tile=tile, sample_offset=3, global_seed=2), equal_nan=True), (arm, tile)
        f64, _ = ctx.render(W, H, 64, tile=tile)
        f32, s32 = ctx.render(W, H, 64, tile=tile, f32=True)
        assert s32["sorted"] & 32 and np.isfinite(f32).all(), (arm, tile)
        # the two frames share their random numbers, but paths that branch differently in f32 (a medium's free-flight distance, an
        # edge-on hit) are new paths: their per-pixel difference is Monte-Carlo noise, and its mean must be within 5 standard errors
        d = (f32 - f64).mean(axis=2).ravel()
        if not f64.any():                        # the Cornell box's far corner: every camera ray misses
            assert not f32.any(), (arm, tile)
            continue
        assert f32.mean() > 0 and abs(d.mean()) <= 5 * d.std(ddof=1) / np.sqrt(d.size), (arm, tile, f32.mean(), f64.mean(), d.std())


@pytest.mark.gpu
@pytest.mark.parametrize("arm", (5, 7))
def test_gpu_top_of_the_sample_range(rt, gpu_ctx_factory, arm):
    """sample_offset = 0xFFFFFFFF - spp renders and equals the CPU core and the literal oracle, in one pass and split over sample
    passes; one sample more is refused; global_seed = 0xFFFFFFFF equals the CPU core."""
    sc = rt.Scene.reference(arm, build_seed=1)
    ctx = gpu_ctx_factory(sc)
    spp = 10
    img, st = ctx.render(W, H, spp, tile=STRADDLE, sample_offset=TOP - spp)
    cpu, sc_ = orc.flat_render(sc, W, H, spp, tile=STRADDLE, sample_offset=TOP - spp, chunk=st["chunk"])
    assert st["segments"] == sc_["segments"] and np.array_equal(img, cpu, equal_nan=True)
    lit, sl = orc.OracleScene(arm, build_seed=1).render(W, H, spp, tile=STRADDLE, sample_offset=TOP - spp)
    assert sl["segments"] == st["segments"] and close(lit, img)
    big = (I0 - 64, J0 - 48, 128, 96)         # 294 912 B per chunk: 3 chunks per MiB, passes of 3 + 3 + 3 + 1 samples
    split, ss = ctx.render(W, H, spp, tile=big, sample_offset=TOP - spp, chunk=1, partial_mib=1)
    cpu_split, scs = orc.flat_render(sc, W, H, spp, tile=big, sample_offset=TOP - spp, chunk=1)
    assert ss["passes"] == 4 and ss["segments"] == scs["segments"] and np.array_equal(split, cpu_split, equal_nan=True)
    with pytest.raises(rt.Rt1wError) as e:
        ctx.render(W, H, spp, tile=STRADDLE, sample_offset=0x100000000 - spp)
    assert e.value.code == rt.ERR_INVALID
    gs, sg = ctx.render(W, H, spp, tile=STRADDLE, global_seed=TOP)
    cgs, scg = orc.flat_render(sc, W, H, spp, tile=STRADDLE, global_seed=TOP, chunk=sg["chunk"])
    assert sg["segments"] == scg["segments"] and np.array_equal(gs, cgs, equal_nan=True)
