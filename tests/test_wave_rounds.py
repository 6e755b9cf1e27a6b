"""Rounds of the unit-sphere and unit-disk rejection samplers as functions of the stream position (include/rt1w_num.h: rt_rng_pos_even,
rt_sphere_round, rt_disk_round, rt_rng_after_round) against the looped samplers they restate, and the assignment of rounds to the lanes of
a wave (rt_wave_rounds_log2, rt_wave_slot, rt_wave_first) in an emulation of 64 lanes that runs the very functions the kernels run.
The header is built with g++ as the CPU twins build it; the two loops are the text of csrc/rt_core.h's samplers."""
import ctypes as C

import numpy as np
import pytest

import core_builds as CB

SHIM = r"""
#include "rt1w_num.h"
/* csrc/rt_core.h: rt_random_in_unit_sphere / rt_random_in_unit_disk, with a count of the rounds */
static RtV3 loop_sphere(RtRng& rng, uint32_t& rounds) {
    for (rounds = 1u;; ++rounds) {
        rt_rng_reserve(rng, rt_rng_need_2u64(rng));
        double x = rt_take_pm1(rng);
        double y = rt_take_pm1(rng);
        rt_rng_reserve(rng, rt_rng_need_u64(rng));
        double z = rt_take_pm1(rng);
        RtV3 v = rt_v3(x, y, z);
        if (rt_mag2(v) < RT_R(1.0)) return v;
    }
}
static RtV3 loop_disk(RtRng& rng, uint32_t& rounds) {
    for (rounds = 1u;; ++rounds) {
        rt_rng_reserve(rng, rt_rng_need_2u64(rng));
        double x = rt_take_pm1(rng);
        double y = rt_take_pm1(rng);
        RtV3 p = rt_v3(x, y, RT_R(0.0));
        if (rt_mag2(p) < RT_R(1.0)) return p;
    }
}
static RtV3 loop_of(bool sphere, RtRng& rng, uint32_t& rounds) { return sphere ? loop_sphere(rng, rounds) : loop_disk(rng, rounds); }
static RtRound round_of(bool sphere, const RtRng& r, RtRngPos start, uint32_t round) {
    return sphere ? rt_sphere_round(r.k0, r.k1, r.c1, r.c2, r.c3, start, round) : rt_disk_round(r.k0, r.k1, r.c1, r.c2, r.c3, start, round);
}
/* an entry state: mode 0 draws `pre` 32-bit words (and tops B up when `fill`); mode 1 stands at (blk, left, bv) by rt_rng_rewind */
static RtRng enter(uint64_t seed, uint32_t sample, uint32_t mode, uint32_t pre, uint32_t fill, uint32_t blk, uint32_t left, uint32_t bv) {
    RtRng r = rt_rng_pixel_sample(seed, sample, 0x5EEDu);
    if (mode == 0u) {
        for (uint32_t i = 0; i < pre; ++i) (void)rt_next_u32(r);
        if (fill) rt_rng_fill(r);
    } else {
        RtRngMark m; m.blk = blk; m.left = left; m.bv = bv;
        rt_rng_rewind(r, m);
    }
    return r;
}
static bool same3(RtV3 a, RtV3 b) { return rt_d2u(a.x) == rt_d2u(b.x) && rt_d2u(a.y) == rt_d2u(b.y) && rt_d2u(a.z) == rt_d2u(b.z); }
static bool same_words(RtRng a, RtRng b, uint32_t n) {
    bool same = true;
    for (uint32_t i = 0; i < n; ++i) same = same && rt_next_u32(a) == rt_next_u32(b);
    return same;
}
extern "C" {
/* per stream: the loop from the entry state, and rounds 0, 1, ... of the candidate function from the same state.  ok bit 0: same vector
 * bits, 1: same number of rounds, 2: the next 16 words agree, 3: the state left is the documented one (left 0 or 2, bv 0) */
void wr_walk(uint32_t sphere, uint64_t n, const uint64_t* seed, const uint32_t* sample, const uint32_t* mode, const uint32_t* pre,
             const uint32_t* fill, const uint32_t* blk, const uint32_t* left, const uint32_t* bv,
             uint8_t* ok, uint32_t* rounds, uint32_t* entry_left, uint32_t* entry_bv, double* vec) {
    for (uint64_t i = 0; i < n; ++i) {
        RtRng a = enter(seed[i], sample[i], mode[i], pre[i], fill[i], blk[i], left[i], bv[i]), b = a;
        entry_left[i] = a.left; entry_bv[i] = a.bv;
        uint32_t ra;
        const RtV3 va = loop_of(sphere != 0u, a, ra);
        const RtRngPos start = rt_rng_pos_even(b);
        uint32_t r = 0u;
        RtRound o = round_of(sphere != 0u, b, start, r);
        while (!o.accept) o = round_of(sphere != 0u, b, start, ++r);
        rt_rng_after_round(b, o);
        ok[i] = (uint8_t)((same3(va, o.v) ? 1 : 0) | (ra == r + 1u ? 2 : 0) | (same_words(a, b, 16u) ? 4 : 0) |
                          ((b.left == 0u || b.left == 2u) && b.bv == 0u ? 8 : 0));
        rounds[i] = ra;
        vec[3 * i] = va.x; vec[3 * i + 1] = va.y; vec[3 * i + 2] = va.z;
    }
}
/* A wave of 64 lanes, `want` of them sampling, as the kernels' rt_wave_rounds runs it (csrc/rt_core.h) with the shared slot functions:
 * per pass K rounds of every loop on the lanes' ranks; with K = 1 every lane takes its own loop's round.  ok[lane]: a lane that wants gets its own
 * loop's vector and stream (bits 0, 2 as above); one that does not keeps its state.  Returns the number of passes. */
uint32_t wr_wave(uint32_t sphere, uint32_t cap, const uint64_t* seed, const uint32_t* sample, const uint32_t* pre, const uint8_t* want_in,
                 uint8_t* ok, uint32_t* k_seen /* [4]: passes with K = 1, 2, 4, 8 */) {
    RtRng rng[64], entry[64];
    bool want[64];
    RtV3 out[64];
    for (uint32_t l = 0; l < 64u; ++l) { rng[l] = entry[l] = enter(seed[l], sample[l], 0u, pre[l], l & 1u, 0u, 0u, 0u); want[l] = want_in[l] != 0; out[l] = rt_v3(0.0, 0.0, 0.0); }
    RtRngPos start[64];
    for (uint32_t l = 0; l < 64u; ++l) start[l] = rt_rng_pos_even(rng[l]);
    uint32_t base = 0u, passes = 0u, kl_before = 0u;
    for (;; ++passes) {
        uint32_t nw = 0u, lane_of[64], wr[64];
        for (uint32_t l = 0; l < 64u; ++l) if (want[l]) { wr[l] = nw; lane_of[nw++] = l; }
        if (nw == 0u) break;
        const uint32_t kl = rt_wave_rounds_log2(64u, nw, cap);
        k_seen[kl] += 1u;
        if (kl < kl_before) return 0xFFFFFFFFu; /* the lanes that want only become fewer: K only grows */
        kl_before = kl;
        RtRound o[64];
        uint64_t accepted = 0u;
        for (uint32_t j = 0; j < 64u; ++j) {
            if (kl == 0u) { /* every lane that wants takes its own loop's round */
                if (want[j]) o[j] = round_of(sphere != 0u, rng[j], start[j], base);
                continue;
            }
            const RtWaveSlot s = rt_wave_slot(j, kl, nw, base);
            const uint32_t src = lane_of[s.valid ? s.loop : 0u];
            o[j] = round_of(sphere != 0u, rng[src], start[src], s.round);
            if (s.valid && o[j].accept) accepted |= 1ull << j;
        }
        for (uint32_t l = 0; l < 64u; ++l) if (want[l]) {
            const uint32_t first = kl == 0u ? (o[l].accept ? l : 64u) : rt_wave_first(accepted, wr[l], kl);
            if (first < 64u) { out[l] = o[first].v; rt_rng_after_round(rng[l], o[first]); want[l] = false; }
        }
        base += 1u << kl;
    }
    for (uint32_t l = 0; l < 64u; ++l) {
        if (want_in[l]) {
            RtRng a = entry[l];
            uint32_t ra;
            const RtV3 va = loop_of(sphere != 0u, a, ra);
            ok[l] = (uint8_t)((same3(va, out[l]) ? 1 : 0) | (same_words(a, rng[l], 16u) ? 4 : 0));
        } else {
            const RtRng &a = entry[l], &b = rng[l];
            ok[l] = (a.blk == b.blk && a.left == b.left && a.bv == b.bv && a.a0 == b.a0 && a.a1 == b.a1 && a.a2 == b.a2 && a.a3 == b.a3 &&
                     a.b0 == b.b0 && a.b1 == b.b1 && a.b2 == b.b2 && a.b3 == b.b3) ? 5 : 0;
        }
    }
    return passes;
}
uint32_t wr_k_log2(uint32_t helpers, uint32_t wanting, uint32_t cap) { return rt_wave_rounds_log2(helpers, wanting, cap); }
}
"""


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    lib = CB.shim_lib(tmp_path_factory.mktemp("wave_rounds"), "wave_rounds", SHIM)
    lib.wr_wave.restype = C.c_uint32
    lib.wr_k_log2.restype = C.c_uint32
    return lib


N = 100_000


def _walk(lib, sphere, seed, sample, mode, pre, fill, blk, left, bv):
    n = seed.size
    u32 = lambda a: np.ascontiguousarray(a, dtype=np.uint32)
    seed = np.ascontiguousarray(seed, dtype=np.uint64)
    args = [u32(a) for a in (sample, mode, pre, fill, blk, left, bv)]
    ok, rounds = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint32)
    el, eb, vec = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32), np.zeros(3 * n)
    lib.wr_walk(C.c_uint32(sphere), C.c_uint64(n), _p(seed), *[_p(a) for a in args], _p(ok), _p(rounds), _p(el), _p(eb), _p(vec))
    return ok, rounds, el, eb, vec.reshape(n, 3)


@pytest.fixture(scope="module")
def streams():
    g = np.random.default_rng(20261019)
    seed = g.integers(0, 1 << 64, N, dtype=np.uint64)
    seed[:4096] = np.arange(4096, dtype=np.uint64)            # the seeds of a small frame: j * W + i
    sample = g.integers(0, 1 << 32, N, dtype=np.uint32)
    sample[:4096:2] = np.arange(2048, dtype=np.uint32) % 64
    return g, seed, sample


@pytest.mark.parametrize("sphere", [1, 0], ids=["sphere", "disk"])
def test_rounds_by_position_equal_the_loop_from_drawn_entry_states(lib, streams, sphere):
    """entry states reached by drawing: 0-7 words, with and without rt_rng_fill behind them"""
    g, seed, sample = streams
    pre = np.arange(N, dtype=np.uint32) % 8
    fill = (np.arange(N, dtype=np.uint32) // 8) % 2
    z = np.zeros(N, dtype=np.uint32)
    ok, rounds, el, eb, vec = _walk(lib, sphere, seed, sample, z, pre, fill, z, z, z)
    assert np.all(ok == 15), np.unique(ok, return_counts=True)
    assert {(int(a), int(b)) for a, b in zip(el, eb)} >= {(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1), (3, 0), (3, 1)}
    # the loops do reject: the mean number of rounds is 1 / (the volume, or area, inside), and some streams need many
    inside = np.pi / 6.0 if sphere else np.pi / 4.0
    assert abs(rounds.mean() - 1.0 / inside) < 5.0 * np.sqrt((1.0 - inside) / inside ** 2 / N)
    assert rounds.max() >= 8
    assert np.all((vec * vec).sum(axis=1) < 1.0) and (np.all(vec[:, 2] == 0.0) if not sphere else np.any(vec[:, 2] != 0.0))


@pytest.mark.parametrize("sphere", [1, 0], ids=["sphere", "disk"])
def test_rounds_by_position_equal_the_loop_from_every_buffer_state(lib, streams, sphere):
    """every (left 0..4, bv 0/1), stood at by rt_rng_rewind, at block indices that include the 32-bit wrap"""
    g, seed, sample = streams
    left = np.arange(N, dtype=np.uint32) % 5
    bv = (np.arange(N, dtype=np.uint32) // 5) % 2
    blk = g.integers(2, 1 << 32, N, dtype=np.uint64).astype(np.uint32)
    blk[:2000] = np.uint32(0xFFFFFFFF) - (np.arange(2000, dtype=np.uint32) % 8)          # the loop runs across block 2^32 - 1 -> 0
    blk[2000:4000] = 2 + (np.arange(2000, dtype=np.uint32) % 8)
    blk[4000:6000] = np.uint32(1 << 30) - 4 + (np.arange(2000, dtype=np.uint32) % 8)    # where a flat word index would wrap
    one = np.ones(N, dtype=np.uint32)
    z = np.zeros(N, dtype=np.uint32)
    ok, rounds, el, eb, vec = _walk(lib, sphere, seed, sample, one, z, z, blk, left, bv)
    assert np.all(ok == 15), np.unique(ok, return_counts=True)
    assert {(int(a), int(b)) for a, b in zip(el, eb)} == {(a, b) for a in range(5) for b in range(2)}
    assert rounds.max() >= 8


def _wave(lib, sphere, cap, seed, sample, pre, want):
    ok, k_seen = np.zeros(64, dtype=np.uint8), np.zeros(4, dtype=np.uint32)
    passes = lib.wr_wave(C.c_uint32(sphere), C.c_uint32(cap), _p(seed), _p(sample), _p(pre), _p(want), _p(ok), _p(k_seen))
    return passes, ok, k_seen


@pytest.fixture(scope="module")
def long_loops(lib):
    """(seed, sample) of streams, entered after 0 words, whose loop runs 9 rounds or more -- more than any K.  For the disk that is
    one stream in 220 000, so the search is wide"""
    out = {}
    for sphere, n in ((1, 100_000), (0, 4_000_000)):
        seed, z = np.arange(n, dtype=np.uint64), np.zeros(n, dtype=np.uint32)
        ok, rounds, *_ = _walk(lib, sphere, seed, z, z, z, z, z, z, z)
        idx = np.flatnonzero(rounds >= 9)
        assert idx.size >= 3 and np.all(ok == 15)
        out[sphere] = seed[idx]
    return out


@pytest.mark.parametrize("cap", [1, 4, 8])
@pytest.mark.parametrize("wanting", [1, 2, 3, 21, 22, 32, 33, 64])
@pytest.mark.parametrize("sphere", [1, 0], ids=["sphere", "disk"])
def test_wave_emulation_gives_every_lane_its_own_loop(lib, streams, long_loops, sphere, wanting, cap):
    g, seed, sample = streams
    r = np.random.default_rng(1000 * wanting + 10 * cap + sphere)
    k_total = np.zeros(4, dtype=np.uint32)
    for trial in range(24):
        pick = r.integers(0, N, 64)
        want = np.zeros(64, dtype=np.uint8)
        lanes = r.permutation(64)[:wanting] if trial % 3 else np.arange(wanting) + (trial % (65 - wanting))   # scattered, or one run as behind the sort
        want[lanes] = 1
        pre = r.integers(0, 8, 64).astype(np.uint32)
        if trial % 2 == 0:   # a lane whose loop outlasts K rounds: several passes
            pre[lanes[0]] = 0
        sd, sm = np.ascontiguousarray(seed[pick]), np.ascontiguousarray(sample[pick])
        if trial % 2 == 0:
            sd[lanes[0]], sm[lanes[0]] = r.choice(long_loops[sphere]), 0
        passes, ok, k_seen = _wave(lib, sphere, cap, sd, sm, pre, want)
        assert passes != 0xFFFFFFFF
        assert np.all(ok == 5), (trial, np.flatnonzero(ok != 5), ok)
        if trial % 2 == 0:
            assert passes >= 2
        k_total += k_seen
    # the first pass's K is the one the formula gives for this many wanting lanes
    k0 = 1
    while 2 * k0 <= cap and 2 * k0 * wanting <= 64:
        k0 *= 2
    assert lib.wr_k_log2(C.c_uint32(64), C.c_uint32(wanting), C.c_uint32(cap)) == int(np.log2(k0))
    assert k_total[int(np.log2(k0))] >= 24
    assert np.all(k_total[int(np.log2(max(cap, 1))) + 1:] == 0)
    if wanting > 32 or cap == 1:
        assert k0 == 1   # most of the wave wants a sample: the loop as it is
