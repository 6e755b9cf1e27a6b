"""The two shorter forms of the random generator (include/rt1w_num.h): rt_take_pm1, the (-1, 1) draw of the unit-sphere and unit-disk
samplers without rand 0.8's retry loop, against rt_take_range(r, -1.0, 1.0), which keeps the loop -- bits and generator state; and
rt_xor3's plain form, the one every target but gfx950 compiles.  The header is built with g++ as the CPU twins build it."""
import ctypes as C

import numpy as np
import pytest

import core_builds as CB

SHIM = r"""
#include "rt1w_num.h"
static bool same_state(const RtRng& a, const RtRng& b) {
    return a.left == b.left && a.blk == b.blk && a.bv == b.bv && a.a0 == b.a0 && a.a1 == b.a1 && a.a2 == b.a2 && a.a3 == b.a3;
}
extern "C" {
/* one draw from an A buffer loaded with the chosen word (a0 low, a1 high; a2, a3 a second word), left = 4, bv = 0 */
void forms_words(const uint64_t* w, uint64_t n, double* pm1, double* range, uint8_t* state_equal) {
    for (uint64_t i = 0; i < n; ++i) {
        RtRng a = rt_rng_make(7u, 9u, 3u, 0u, RT_DOMAIN_RENDER);
        a.blk = 5u; a.left = 4u; a.bv = 0u;
        a.a0 = (uint32_t)w[i]; a.a1 = (uint32_t)(w[i] >> 32); a.a2 = 0x12345678u; a.a3 = 0x9ABCDEF0u;
        RtRng b = a;
        pm1[i] = rt_take_pm1(a);
        range[i] = rt_take_range(b, -1.0, 1.0);
        state_equal[i] = same_state(a, b) && a.left == 2u && a.blk == 5u;
    }
}
/* `draws` (-1, 1) draws of the stream of (seed, sample), a 32-bit draw before every third so that odd alignments occur */
void forms_streams(const uint64_t* seed, const uint32_t* sample, uint64_t n, uint32_t draws, double* pm1, double* range,
                   uint8_t* state_equal, uint32_t* odd_seen) {
    for (uint64_t i = 0; i < n; ++i) {
        RtRng a = rt_rng_pixel_sample(seed[i], sample[i], 0u), b = a;
        uint32_t odd = 0u;
        bool same = true;
        for (uint32_t d = 0; d < draws; ++d) {
            if (d % 3u == 1u) same = same && rt_next_u32(a) == rt_next_u32(b);
            odd += a.left & 1u;
            rt_rng_reserve(a, rt_rng_need_u64(a));
            rt_rng_reserve(b, rt_rng_need_u64(b));
            pm1[i * draws + d] = rt_take_pm1(a);
            range[i * draws + d] = rt_take_range(b, -1.0, 1.0);
            same = same && same_state(a, b);
        }
        state_equal[i] = same && a.b0 == b.b0 && a.b1 == b.b1 && a.b2 == b.b2 && a.b3 == b.b3;
        odd_seen[i] = odd;
    }
}
void forms_xor3(const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t* out, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i) out[i] = rt_xor3(a[i], b[i], c[i]);
}
}
"""

TOP = 1.0 - 2.0 ** -51   # the largest value a (-1, 1) draw can take


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return CB.shim_lib(tmp_path_factory.mktemp("rng_forms"), "rng_forms", SHIM)


def _words(lib, w):
    w = np.ascontiguousarray(w, dtype=np.uint64)
    pm1, rng, same = np.empty(w.size), np.empty(w.size), np.empty(w.size, dtype=np.uint8)
    lib.forms_words(_p(w), C.c_uint64(w.size), _p(pm1), _p(rng), _p(same))
    return pm1, rng, same


def chosen_words():
    full = (1 << 64) - 1
    w = [0, full, 0xFFFFFFFFFFFFF000, 0x0000000000000FFF, 1 << 12, (1 << 12) - 1]
    for k in range(52):   # the draw keeps bits 12..63 of the word: its 52 mantissa bits
        bit = 1 << (12 + k)
        w += [bit, bit | 0xFFF, full ^ bit, (full ^ bit) & ~0xFFF]
    return np.array(w, dtype=np.uint64)


def test_take_pm1_equals_take_range_on_chosen_words(lib):
    w = chosen_words()
    pm1, rng, same = _words(lib, w)
    assert np.array_equal(pm1.view(np.uint64), rng.view(np.uint64))
    assert same.all()
    assert np.all((pm1 >= -1.0) & (pm1 < 1.0))
    assert pm1.max() == TOP and pm1[1] == TOP and pm1[2] == TOP   # all mantissa bits set: the top, whatever the low 12 bits are
    assert pm1[0] == -1.0 and pm1[3] == -1.0 and pm1[5] == -1.0   # no mantissa bit set: the bottom
    assert pm1[4] == -1.0 + 2.0 ** -51                            # one step of the grid
    # every value is a multiple of 2^-51: the three operations were exact
    assert np.array_equal(np.ldexp(pm1, 51), np.rint(np.ldexp(pm1, 51)))


def test_take_pm1_equals_take_range_on_random_words(lib):
    g = np.random.default_rng(20240611)
    w = g.integers(0, 1 << 64, 1_000_000, dtype=np.uint64)
    pm1, rng, same = _words(lib, w)
    assert np.array_equal(pm1.view(np.uint64), rng.view(np.uint64))
    assert same.all()
    assert np.all((pm1 >= -1.0) & (pm1 < 1.0)) and pm1.max() <= TOP
    # the value is the word's top 52 bits on the grid of 2^-51, exactly
    assert np.array_equal(pm1, (w >> np.uint64(12)).astype(np.float64) * 2.0 ** -51 - 1.0)


def test_take_pm1_equals_take_range_on_real_streams(lib):
    g = np.random.default_rng(7)
    n, draws = 4096, 64
    seed = g.integers(0, 1 << 64, n, dtype=np.uint64)
    seed[:6] = [0, 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 12345, (1 << 64) - 1]
    seed[6:1024] = np.arange(6, 1024, dtype=np.uint64)                   # the seeds of a small frame: j * W + i
    sample = g.integers(0, 1 << 32, n, dtype=np.uint32)
    sample[:2048:4] = 0xFFFFFFFF
    sample[1:2048:4] = 0
    sample[2:2048:4] = np.arange(512, dtype=np.uint32)
    assert (seed >= np.uint64(1 << 32)).sum() > 1000
    pm1, rng = np.empty(n * draws), np.empty(n * draws)
    same, odd = np.empty(n, dtype=np.uint8), np.empty(n, dtype=np.uint32)
    lib.forms_streams(_p(seed), _p(sample), C.c_uint64(n), C.c_uint32(draws), _p(pm1), _p(rng), _p(same), _p(odd))
    assert np.array_equal(pm1.view(np.uint64), rng.view(np.uint64))
    assert same.all()
    assert np.all(odd > 0)                                               # every stream met draws that had to skip a word
    assert np.all((pm1 >= -1.0) & (pm1 < 1.0))
    assert abs(pm1.mean()) < 5.0 / np.sqrt(3.0 * pm1.size)               # uniform on (-1, 1): sd 1/sqrt(3); five sigma of the mean


def test_xor3_host_form_is_two_xors(lib):
    g = np.random.default_rng(3)
    a, b, c = (g.integers(0, 1 << 32, 100_000, dtype=np.uint32) for _ in range(3))
    a[:4], b[:4], c[:4] = [0, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF], [0, 0, 0xFFFFFFFF, 0xFFFFFFFF], [0, 0, 0, 0xFFFFFFFF]
    out = np.empty_like(a)
    lib.forms_xor3(_p(a), _p(b), _p(c), _p(out), C.c_uint64(a.size))
    assert np.array_equal(out, a ^ b ^ c)
