"""The class bases of the reordering kernels' sort from one wave scan (include/rt1w_num.h: rt_sort_slot, rt_sort_scan) against the double
loop they replace (csrc/rt_kernel_sorted.h, RT_SORT_SCAN 0: every lane sums every count below its own), in an emulation of a workgroup of
NW waves of 64 lanes that runs the very functions the kernels run.  The emulation supplies the moves between lanes as the header states
them (what the DPP row shifts and row broadcasts of the device do) and follows the kernel's statements: counts by ballot, one count to a
lane, the scan, the fetch from the lane that holds the base, the idle total from the scan's last class.  The header is built with g++ as
the CPU twins build it."""
import ctypes as C

import numpy as np
import pytest

import core_builds as CB

N_CLS, IDLE = 6, 5   # csrc/rt_core.h: RT_N_CLS, RT_CLS_IDLE

SHIM = r"""
#include "rt1w_num.h"
#define N_CLS 6u
#define CLS_IDLE 5u
struct Lanes {
    uint32_t v[64];
    Lanes operator+(const Lanes& o) const { Lanes r; for (int l = 0; l < 64; ++l) r.v[l] = v[l] + o.v[l]; return r; }
    Lanes operator-(const Lanes& o) const { Lanes r; for (int l = 0; l < 64; ++l) r.v[l] = v[l] - o.v[l]; return r; }
};
/* the moves of rt_sort_scan as the header states them */
struct Wave {
    template <uint32_t S> Lanes row_shr(const Lanes& x) const {
        Lanes r;
        for (uint32_t l = 0; l < 64u; ++l) r.v[l] = (l & 15u) >= S ? x.v[l - S] : 0u;
        return r;
    }
    Lanes row_bcast15(const Lanes& x) const {
        Lanes r;
        for (uint32_t l = 0; l < 64u; ++l) r.v[l] = ((l >> 4) & 1u) ? x.v[(l & ~15u) - 1u] : 0u;
        return r;
    }
    Lanes row_bcast31(const Lanes& x) const {
        Lanes r;
        for (uint32_t l = 0; l < 64u; ++l) r.v[l] = l >= 32u ? x.v[31] : 0u;
        return r;
    }
};
/* one iteration's sort of a workgroup of NW waves: cls[wave * 64 + lane].  The lanes behind the last slot hold the last slot's count, as
 * in the kernel (junk 0), or `junk` + their lane number (nothing may look at their sums).  Returns bit 0: the two dest differ on some
 * lane, bit 1: the idle totals differ (on some wave: every wave computes its own), bit 2: dest is no permutation of 0 .. 64 NW - 1,
 * bit 3: a path of a higher class stands before one of a lower class */
template <uint32_t NW>
static uint32_t sort_once(const uint8_t* cls, uint32_t junk, uint32_t* dest_out, uint32_t* idle_out) {
    constexpr uint32_t NV = NW * N_CLS, BLOCK = NW * 64u;
    uint32_t rank[BLOCK], cnt_wc[NW][N_CLS], cnt_slot[NV];
    for (uint32_t w = 0; w < NW; ++w)
        for (uint32_t c = 0; c < N_CLS; ++c) {
            uint32_t n = 0u;
            for (uint32_t l = 0; l < 64u; ++l) if (cls[w * 64u + l] == c) rank[w * 64u + l] = n++; /* lane_prefix(ballot) */
            cnt_wc[w][c] = n;
            cnt_slot[rt_sort_slot(c, w, NW)] = n;
        }
    uint32_t bad = 0u;
    bool seen[BLOCK];
    uint8_t at[BLOCK];
    for (uint32_t i = 0; i < BLOCK; ++i) seen[i] = false;
    for (uint32_t wave = 0; wave < NW; ++wave) {
        /* RT_SORT_SCAN 1 */
        Lanes held, index;
        for (uint32_t l = 0; l < 64u; ++l) held.v[l] = l < NV ? cnt_slot[l] : (junk ? junk + l : cnt_slot[NV - 1u]);
        const Lanes below = rt_sort_scan<NV>(Wave(), held);
        const uint32_t idle_scan = (below.v[NV - 1u] + held.v[NV - 1u]) - below.v[rt_sort_slot(CLS_IDLE, 0u, NW)];
        for (uint32_t l = 0; l < 64u; ++l) index.v[l] = rt_sort_slot(cls[wave * 64u + l], wave, NW);
        for (uint32_t l = 0; l < 64u; ++l) {
            const uint32_t i = wave * 64u + l;
            const uint32_t dest_scan = rank[i] + below.v[index.v[l] & 63u]; /* the fetch: lane l reads lane index[l] */
            /* RT_SORT_SCAN 0: the kernel's double loop */
            uint32_t dest = rank[i], idle_total = 0u;
            for (uint32_t c = 0; c < N_CLS; ++c)
                for (uint32_t w = 0; w < NW; ++w) {
                    const uint32_t v = cnt_wc[w][c];
                    if (c < cls[i] || (c == cls[i] && w < wave)) dest += v;
                    if (c == CLS_IDLE) idle_total += v;
                }
            if (dest_scan != dest) bad |= 1u;
            if (idle_scan != idle_total) bad |= 2u;
            if (dest_scan >= BLOCK || seen[dest_scan]) bad |= 4u;
            else { seen[dest_scan] = true; at[dest_scan] = cls[i]; }
            dest_out[i] = dest_scan;
            idle_out[wave] = idle_scan;
        }
    }
    if (!(bad & 4u))
        for (uint32_t i = 1; i < BLOCK; ++i) if (at[i - 1u] > at[i]) bad |= 8u;
    return bad;
}
extern "C" uint32_t sort_many(uint32_t nw, uint64_t n, const uint8_t* cls, uint32_t junk, uint32_t* dest, uint32_t* idle) {
    uint32_t bad = 0u;
    for (uint64_t k = 0; k < n; ++k) {
        const uint8_t* c = cls + k * nw * 64u;
        uint32_t* d = dest + k * nw * 64u;
        bad |= nw == 4u ? sort_once<4u>(c, junk, d, idle + k * nw) : sort_once<8u>(c, junk, d, idle + k * nw);
    }
    return bad;
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    lib = CB.shim_lib(tmp_path_factory.mktemp("sort_scan"), "sort_scan", SHIM)
    lib.sort_many.restype = C.c_uint32
    return lib


def _sort(lib, nw, cls, junk=0):
    cls = np.ascontiguousarray(cls, dtype=np.uint8).reshape(-1, nw * 64)
    n = cls.shape[0]
    dest, idle = np.zeros((n, nw * 64), dtype=np.uint32), np.zeros((n, nw), dtype=np.uint32)
    bad = lib.sort_many(C.c_uint32(nw), C.c_uint64(n), cls.ctypes.data_as(C.c_void_p), C.c_uint32(junk),
                        dest.ctypes.data_as(C.c_void_p), idle.ctypes.data_as(C.c_void_p))
    return bad, dest, idle


def _check(lib, nw, cls):
    """both forms agree on every lane, in the kernel's form and with junk behind the last slot; returns dest and the idle totals"""
    cls = np.asarray(cls, dtype=np.uint8).reshape(-1, nw * 64)
    bad, dest, idle = _sort(lib, nw, cls)
    assert bad == 0, bad
    bad_j, dest_j, idle_j = _sort(lib, nw, cls, junk=0x9E3779B9)
    assert bad_j == 0 and np.array_equal(dest, dest_j) and np.array_equal(idle, idle_j)
    assert np.array_equal(np.sort(dest, axis=1), np.broadcast_to(np.arange(nw * 64, dtype=np.uint32), dest.shape))
    assert np.array_equal(idle, np.broadcast_to((cls == IDLE).sum(axis=1, dtype=np.uint32)[:, None], idle.shape))
    return dest, idle


NWS = [4, 8]   # RT_SORT_BLOCK 256 and 512


@pytest.mark.parametrize("nw", NWS)
def test_every_path_in_one_class(lib, nw):
    for c in range(N_CLS):
        dest, idle = _check(lib, nw, np.full(nw * 64, c))
        assert np.array_equal(dest[0], np.arange(nw * 64))   # nobody moves
        assert np.all(idle == (nw * 64 if c == IDLE else 0))   # IDLE: the workgroup is done


@pytest.mark.parametrize("nw", NWS)
def test_one_path_per_class(lib, nw):
    """one path of every class but IDLE, each in a wave and lane of its own, the rest idle: they come to stand in slots 0 .. 4"""
    cls = np.full(nw * 64, IDLE)
    where = [(c * 3 + 1) % nw * 64 + (17 * c + 5) % 64 for c in range(N_CLS - 1)]
    for c, i in enumerate(where):
        cls[i] = N_CLS - 2 - c   # (the higher class in the lower wave)
    dest, idle = _check(lib, nw, cls)
    assert [int(dest[0][i]) for i in where] == [N_CLS - 2 - c for c in range(N_CLS - 1)]
    assert np.all(idle == nw * 64 - (N_CLS - 1))


@pytest.mark.parametrize("nw", NWS)
def test_a_class_absent_from_some_waves(lib, nw):
    g = np.random.default_rng(77 + nw)
    cases = []
    for c in range(N_CLS):
        for keep in range(1, nw):   # class c lives in `keep` of the waves only; the others draw from the rest
            cls = g.integers(0, N_CLS - 1, (nw, 64))
            cls[cls >= c] += 1
            waves = g.permutation(nw)[:keep]
            cls[waves] = g.integers(0, N_CLS, (keep, 64))
            cls[waves[0], 0] = c
            cases.append(cls.reshape(-1))
    # and whole waves of one class each, so that most counts of the table are zero
    cases.append(np.repeat(np.arange(nw) % N_CLS, 64))
    cases.append(np.repeat((np.arange(nw)[::-1] * 5) % N_CLS, 64))
    _check(lib, nw, np.stack(cases))


@pytest.mark.parametrize("nw", NWS)
def test_random_fills(lib, nw):
    """10^4 workgroups: uniform classes, skewed ones (mostly Lambertian and idle, as a Cornell workgroup is), and runs as the previous
    iteration's sort leaves them"""
    g = np.random.default_rng(20261019 + nw)
    n = 10_000
    cls = g.integers(0, N_CLS, (n, nw * 64))
    skew = g.choice(N_CLS, size=(n // 4, nw * 64), p=[0.55, 0.02, 0.08, 0.0, 0.15, 0.2])
    cls[: n // 4] = skew
    cls[n // 4: n // 2] = np.sort(cls[n // 4: n // 2], axis=1)
    dest, idle = _check(lib, nw, cls)
    assert np.unique(idle).size > 20   # the fills do differ
