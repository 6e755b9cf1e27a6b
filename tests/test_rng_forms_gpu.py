"""The shorter forms of the random generator on the GPU (include/rt1w_num.h): the Philox round with gfx950's three-input XOR against the
two-XOR round the host compiles, word for word, and the loop-free (-1, 1) draw of the unit-sphere and unit-disk samplers (rt_take_pm1)
in the kernels that run them, against the CPU build of the core (bits) and the literal oracle, which keeps rand 0.8's retry loops."""
import ctypes as C

import numpy as np
import pytest

import orc

pytestmark = pytest.mark.gpu

RTOL = 1e-12
DOMAIN_RENDER = 0x52454E44
N = 65536
SAMPLES = (0, 1, 1 << 31, (1 << 32) - 1)


def close(a, b):
    both_nan = np.isnan(a) & np.isnan(b)
    return bool((both_nan | (np.abs(a - b) <= RTOL * np.abs(a)) | (a == b)).all())


def as_bits(u):
    """doubles that carry the given 64-bit words (the device entry reads its integer arguments from the bits of its inputs)"""
    return np.ascontiguousarray(u, dtype=np.uint64).view(np.float64)


@pytest.fixture(scope="module")
def pairs():
    g = np.random.default_rng(5)
    sample = g.integers(0, 1 << 32, N, dtype=np.uint64)
    sample[: N // 2] = np.resize(np.array(SAMPLES, dtype=np.uint64), N // 2)
    seed = g.integers(0, 1 << 64, N, dtype=np.uint64)
    seed[:8] = [0, 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 63), (1 << 64) - 2, (1 << 64) - 1]
    seed[8:4096] = np.arange(8, 4096, dtype=np.uint64)
    assert (seed >= np.uint64(1 << 32)).sum() > N // 2 and seed[7] == np.uint64((1 << 64) - 1)
    return seed, sample


def host_block0(seed, sample):
    """block 0 of the streams, from the oracle's own Philox (g++: the two-XOR round)"""
    out = np.empty((seed.size, 4), dtype=np.uint32)
    ctr, key, o = np.zeros(4, dtype=np.uint32), np.zeros(2, dtype=np.uint32), np.zeros(4, dtype=np.uint32)
    pc, pk, po = (x.ctypes.data_as(C.c_void_p) for x in (ctr, key, o))
    for i in range(seed.size):
        ctr[:] = (0, int(sample[i]) & 0xFFFFFFFF, 0, DOMAIN_RENDER)
        key[:] = (int(seed[i]) & 0xFFFFFFFF, int(seed[i]) >> 32)
        orc.A.orc_philox(pc, pk, po)
        out[i] = o
    return out.astype(np.uint64)


def test_device_words_equal_host_words(rt, gpu_ctx_factory, pairs):
    seed, sample = pairs
    ctx = gpu_ctx_factory(rt.Scene.reference(5))
    a = as_bits(sample)
    # selectors 7 and 8: the stream of (pixel = index, sample), against the oracle's same selectors
    zeros = np.zeros(N)
    for fn in (7, 8):
        host = np.empty(N)
        orc.A.orc_num_eval(fn, a.ctypes.data_as(C.c_void_p), zeros.ctypes.data_as(C.c_void_p), host.ctypes.data_as(C.c_void_p), N)
        dev = ctx.debug_eval(fn, a, zeros)
        assert np.array_equal(host.view(np.uint64), dev.view(np.uint64)), fn
    # selectors 11-13: any 64-bit pixel seed; the host side is the oracle's Philox block and rand 0.8's two conversions
    w = host_block0(seed, sample)
    q0, q1 = (w[:, 1] << np.uint64(32)) | w[:, 0], (w[:, 3] << np.uint64(32)) | w[:, 2]
    f64 = (q0 >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
    v12 = ((q1 >> np.uint64(12)) | np.uint64(0x3FF0000000000000)).view(np.float64)
    rng = (v12 - 1.0) * 2.0 + -1.0
    assert np.all(rng < 1.0)                                  # so the oracle's retry loop would not have drawn again
    b = as_bits(seed)
    assert np.array_equal(ctx.debug_eval(11, a, b).view(np.uint64), f64.view(np.uint64))
    assert np.array_equal(ctx.debug_eval(12, a, b).view(np.uint64), rng.view(np.uint64))
    assert np.array_equal(ctx.debug_eval(13, a, b).view(np.uint64), rng.view(np.uint64))
    # the two entries agree where they overlap (pixel = index)
    idx = as_bits(np.arange(N, dtype=np.uint64))
    assert np.array_equal(ctx.debug_eval(12, a, idx).view(np.uint64), ctx.debug_eval(8, a, zeros).view(np.uint64))


FRAMES = [(5, None, 64, 64, 8, 4), (5, None, 8, 8, 4, 4), (6, None, 48, 48, 6, 4), (0, 1.5, 96, 64, 4, 128), (7, None, 64, 64, 2, 512 | 1024)]


@pytest.mark.parametrize("arm,aspect,W,H,spp,flags", FRAMES, ids=lambda v: str(v))
def test_frames_equal_cpu_core_and_literal_oracle(rt, gpu_ctx_factory, arm, aspect, W, H, spp, flags):
    """arm 5: the metal box draws in the unit sphere (8x8: a frame smaller than a workgroup); arm 6: isotropic scatter inside the media;
    arm 0: aperture 0.1, the unit disk accepts and rejects, fuzzy metal, the pair-walk kernel; arm 7: the ss_hc kernel"""
    sc = rt.Scene.reference(arm, build_seed=1, aspect_ratio=aspect)
    ctx = gpu_ctx_factory(sc)
    g, sg = ctx.render(W, H, spp)
    assert sg["sorted"] & flags == flags, sg["sorted"]
    f, sf = orc.flat_render(sc, W, H, spp, chunk=sg["chunk"])
    assert sg["segments"] == sf["segments"]
    assert np.array_equal(g, f, equal_nan=True)
    lit, sl = orc.OracleScene(arm, build_seed=1, aspect_ratio=aspect).render(W, H, spp)
    assert sl["segments"] == sg["segments"]
    assert close(lit, g)
    assert np.any(g > 0.0)
    if arm in (5, 6):
        b, sb = ctx.render(W, H, spp, generic=True)
        assert not (sb["sorted"] & 4) and sb["segments"] == sg["segments"] and np.array_equal(g, b, equal_nan=True)
        a32, s32 = ctx.render(W, H, spp, f32=True)
        b32, t32 = ctx.render(W, H, spp, f32=True, generic=True)
        assert (s32["sorted"] & 4) and not (t32["sorted"] & 4)
        assert s32["segments"] == t32["segments"] and np.array_equal(a32, b32, equal_nan=True)


def fuzzy_room(rt):
    """a Cornell-like room whose only scatterers are a fuzzy metal sphere (fuzz 0.7) and a Lambertian floor: the walls and the ceiling
    are dim emitters, so every bounce but the floor's draws in the unit sphere"""
    s = rt.Scene(build_seed=1)

    def glow(rgb):
        return s.diffuse_light(s.solid_color(rgb))

    def lamp():
        return s.flip_face(s.xz_rect(1.2, 2.8, 1.2, 2.8, 3.9, glow((9.0, 9.0, 9.0))))

    objs = [s.xz_rect(0.0, 4.0, 0.0, 4.0, 0.0, s.lambertian(s.solid_color((0.73, 0.73, 0.73)))),
            s.yz_rect(0.0, 4.0, 0.0, 4.0, 0.0, glow((0.30, 0.03, 0.03))), s.yz_rect(0.0, 4.0, 0.0, 4.0, 4.0, glow((0.04, 0.25, 0.05))),
            s.xy_rect(0.0, 4.0, 0.0, 4.0, 0.0, glow((0.12, 0.12, 0.14))), s.xz_rect(0.0, 4.0, 0.0, 4.0, 4.0, glow((0.10, 0.10, 0.10))),
            s.sphere((2.0, 1.1, 2.0), 1.1, s.metal((0.8, 0.85, 0.88), 0.7)), lamp()]
    s.set_world(s.bvh_node(objs))
    s.set_lights([lamp()])
    s.set_background((0.0, 0.0, 0.0))
    s.set_camera((2.0, 2.0, 7.5), (2.0, 1.4, 0.0), (0, 1, 0), 45.0, 1.0, 0.0, 6.0, 0.0, 1.0)
    s.commit()
    return s


def test_hand_built_fuzzy_metal_room_compiled_at_run_time(rt, gpu_ctx_factory, tmp_path, monkeypatch):
    monkeypatch.setenv("RT1W_KERNEL_CACHE", str(tmp_path / "kcache"))
    sc = fuzzy_room(rt)
    ctx = gpu_ctx_factory(sc)
    b, sb = ctx.render(32, 32, 8)
    assert not (sb["sorted"] & 4)
    info = ctx.specialise()
    assert info["active"] and not info["from_cache"]
    a, sa = ctx.render(32, 32, 8)
    f, sf = orc.flat_render(sc, 32, 32, 8, chunk=sa["chunk"])
    assert (sa["sorted"] & 4) and sa["segments"] == sb["segments"] == sf["segments"]
    assert np.array_equal(a, b, equal_nan=True) and np.array_equal(a, f, equal_nan=True)
    assert np.any(a > 0.0) and sa["segments"] > 32 * 32 * 8 * 5 // 4     # paths do bounce off the sphere and the floor
