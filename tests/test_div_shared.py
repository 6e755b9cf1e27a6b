"""Quotients of one divisor (include/rt1w_num.h: rt_div_refine, rt_div_q, rt_div_inv and their guards): the second half of the f64
division the GPU compiler emits, run on a `y` that several quotients share.  The header is built with g++ as the CPU twins build it;
the one thing the CPU does not have is the seed, the value v_rcp_f64 returns, so the model takes it as a parameter.

ASSUMPTION about the seed (no ISA manual is at hand here): v_rcp_f64 returns 1/d with a relative error of at most 2^-24.  That is
on the safe side of every figure quoted for it (the division the compiler builds on it needs far better than 2^-24 to be correctly
rounded after two Newton steps and one correction), and the test perturbs the correctly rounded reciprocal by relative errors up
to that size, both signs.  The real seed is tested on the GPU (test_div_shared_gpu.py).

Condition, not a statistic: for every pair whose guards pass, the model's quotient is `n / d` bit for bit and the model's 1/d is
`1.0 / d` bit for bit; every pair with a zero, infinite, NaN, denormal or out-of-range operand or result raises a guard."""
import ctypes as C

import numpy as np
import pytest

import core_builds as CB

SHIM = r"""
#include "rt1w_num.h"
extern "C" {
/* verdict: 1 the divisor is out of range | 2 the quotient is bad if it is used | 4 the quotient is too large (bad whether used or not) */
void ds_quot(const double* n, const double* d, const double* y0, uint64_t cnt, double* q_fast, double* q_div, double* inv_fast,
             double* inv_div, uint8_t* verdict) {
    for (uint64_t i = 0; i < cnt; ++i) {
        const double y = rt_div_refine(d[i], y0[i]);
        const double t = rt_div_q(n[i], d[i], y);
        q_fast[i] = t;
        q_div[i] = n[i] / d[i];
        inv_fast[i] = rt_div_inv(d[i], y);
        inv_div[i] = 1.0 / d[i];
        verdict[i] = (uint8_t)((rt_div_d_ok(d[i]) ? 0 : 1) | (rt_div_q_bad(t, true) ? 2 : 0) | (rt_div_q_big(t) ? 4 : 0));
    }
}
/* a rect's use of a quotient: `use` is its t_min / t_max test (rt_core.h: rt_rect_hot_t) */
void ds_use(const double* t, const double* t_min, const double* t_max, uint64_t cnt, uint8_t* tmin_ok, uint8_t* bad, uint8_t* big) {
    for (uint64_t i = 0; i < cnt; ++i) {
        const bool use = !((t[i] < t_min[i]) | (t[i] > t_max[i]));
        tmin_ok[i] = rt_div_tmin_ok(t_min[i]);
        bad[i] = rt_div_q_bad(t[i], use);
        big[i] = rt_div_q_big(t[i]);
    }
}
double ds_lo() { return RT_DIV_LO; }
double ds_hi() { return RT_DIV_HI; }
}
"""

SEED_ERR = 2.0 ** -24


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    L = CB.shim_lib(tmp_path_factory.mktemp("div_shared"), "div_shared", SHIM)
    L.ds_lo.restype = L.ds_hi.restype = C.c_double
    return L


def seeds_of(d, g):
    """RN(1/d) x (1 + e), |e| <= 2^-24: random e, and the two ends for the first quarter"""
    with np.errstate(all="ignore"):
        y = 1.0 / d
    e = g.uniform(-SEED_ERR, SEED_ERR, d.size)
    k = d.size // 4
    e[0:k:2] = SEED_ERR
    e[1:k:2] = -SEED_ERR
    with np.errstate(all="ignore"):
        return y * (1.0 + e)


def run(lib, n, d, y0):
    n, d, y0 = (np.ascontiguousarray(a, dtype=np.float64) for a in (n, d, y0))
    qf, qd, vf, vd = (np.empty(n.size) for _ in range(4))
    v = np.empty(n.size, dtype=np.uint8)
    lib.ds_quot(_p(n), _p(d), _p(y0), C.c_uint64(n.size), _p(qf), _p(qd), _p(vf), _p(vd), _p(v))
    return qf, qd, vf, vd, v


def check(lib, n, d, g, expect_all_bad=False):
    """the condition; returns how many pairs passed their guards"""
    qf, qd, vf, vd, v = run(lib, n, d, seeds_of(d, g))
    good = (v & 3) == 0
    assert np.array_equal(qf[good].view(np.uint64), qd[good].view(np.uint64)), "an in-range quotient differs from n / d"
    dok = (v & 1) == 0
    assert np.array_equal(vf[dok].view(np.uint64), vd[dok].view(np.uint64)), "1/d from an in-range divisor differs from 1.0 / d"
    # what the guards must catch, from the division's own operands and result
    lo, hi = lib.ds_lo(), lib.ds_hi()
    with np.errstate(all="ignore"):
        special = ~(np.abs(d) > lo) | ~(np.abs(d) < hi) | ~(np.abs(qd) > lo) | ~(np.abs(qd) < hi)
    assert not np.any(special & good), "a zero, infinity, NaN, denormal or out-of-range value passed the guards"
    if expect_all_bad:
        assert not good.any()
    return int(good.sum())


def rand_pairs(g, count, emin, emax):
    m = lambda: g.uniform(1.0, 2.0, count) * g.choice([-1.0, 1.0], count)
    return (np.ldexp(m(), g.integers(emin, emax, count).astype(np.int32)), np.ldexp(m(), g.integers(emin, emax, count).astype(np.int32)))


def test_bounds_are_the_powers_of_two(lib):
    assert lib.ds_lo() == 2.0 ** -300 and lib.ds_hi() == 2.0 ** 300


def test_random_pairs_over_the_exponent_range(lib):
    g = np.random.default_rng(20241019)
    n, d = rand_pairs(g, 1_000_000, -1070, 1023)           # everything a double can be: most of it must raise a guard
    check(lib, n, d, g)
    n, d = rand_pairs(g, 1_000_000, -140, 140)            # the range the sweep lives in: |n / d| < 2^281, every pair in range
    assert check(lib, n, d, g) == n.size
    n, d = rand_pairs(g, 200_000, -10, 10)                # a ray's numbers
    assert check(lib, n, d, g) == n.size


def test_quotients_next_to_rounding_midpoints(lib):
    """n = d x (q + half an ulp) rounded: the exact quotient lies within about 2^-53 relative of the midpoint between q and its
    neighbour -- the cases where a division that is not correctly rounded shows; and n = d x q rounded (next to q itself)"""
    g = np.random.default_rng(5)
    count = 300_000
    q = np.ldexp(g.uniform(1.0, 2.0, count), g.integers(-60, 60, count).astype(np.int32))
    d = np.ldexp(g.uniform(1.0, 2.0, count), g.integers(-60, 60, count).astype(np.int32)) * g.choice([-1.0, 1.0], count)
    ulp = np.spacing(q)
    # (q + ulp / 2) x d in two pieces so that the product keeps the half ulp: q x d + (ulp / 2) x d (the second is exact up to rounding)
    for frac in (0.5, -0.5, 0.0):
        n = q * d + (frac * ulp) * d
        assert check(lib, n, d, g) == count
    # small integers: exact quotients, and thirds and sevenths
    a = np.arange(1.0, 2049.0)
    n, d = (x.ravel() for x in np.meshgrid(a[:512], a[:512]))
    assert check(lib, n, d, g) == n.size
    assert check(lib, -n, d * 2.0 ** -40, g) == n.size


def test_zeros_infinities_nans_and_denormals(lib):
    g = np.random.default_rng(6)
    sp = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, -5e-324, 2.2250738585072014e-308, 1e-310, -1e-310, 1.7976931348623157e308])
    ordinary = np.array([1.0, -3.0, 0.001, 555.0, 2.0 ** 200, 2.0 ** -200])
    # a special divisor: the divisor guard, whatever the numerator is
    n, d = (x.ravel() for x in np.meshgrid(np.concatenate([sp, ordinary]), sp))
    qf, qd, vf, vd, v = run(lib, n, d, seeds_of(d, g))
    assert np.all(v & 1)
    # a special numerator over an ordinary divisor: the quotient guard (zero and tiny: because it is used; inf and NaN: always)
    n, d = (x.ravel() for x in np.meshgrid(sp, ordinary))
    check(lib, n, d, g, expect_all_bad=True)
    qf, qd, vf, vd, v = run(lib, n, d, seeds_of(d, g))
    big = ~np.isfinite(n) | (np.abs(n) > 1e308)
    assert np.all((v[big] & 4) != 0)
    # the zero's sign is what the guard is for: -0 / d differs from the division's somewhere
    z = np.array([0.0, -0.0, 0.0, -0.0])
    dd = np.array([3.0, 3.0, -3.0, -3.0])
    qf, qd, *_ = run(lib, z, dd, 1.0 / dd)
    assert np.all(qf == 0.0) and np.all(qd == 0.0)
    assert not np.array_equal(np.signbit(qf), np.signbit(qd))


def test_both_sides_of_each_bound(lib):
    g = np.random.default_rng(7)
    lo, hi = 2.0 ** -300, 2.0 ** 300
    up, dn = lambda x: np.nextafter(x, np.inf), lambda x: np.nextafter(x, 0.0)
    # the divisor: strictly inside passes, the bound itself and beyond do not
    d = np.array([up(lo), lo, dn(lo), dn(hi), hi, up(hi)])
    for s in (1.0, -1.0):
        qf, qd, vf, vd, v = run(lib, s * d, s * d, seeds_of(s * d, g))      # n = d: the quotient is 1
        assert list(v & 1) == [0, 1, 1, 0, 1, 1]
        assert np.all(qf[(v & 1) == 0] == 1.0)
    # the quotient: the neighbours of each bound over a power of two (exact), and values 2^-40 away over 1.5 (1.5 t is exact for them)
    near = np.array([up(lo), lo, dn(lo), dn(hi), hi, up(hi)])
    away = np.array([lo * (1 + 2.0 ** -40), lo, lo * (1 - 2.0 ** -40), hi * (1 - 2.0 ** -40), hi, hi * (1 + 2.0 ** -40)])
    for t, div in ((near, 1.0), (near, -4.0), (near, 0.5), (away, 1.5), (away, -1.5), (away, 3.0)):
        for s in (1.0, -1.0):
            n, d = s * t * div, np.full(t.size, div)
            qf, qd, vf, vd, v = run(lib, n, d, seeds_of(d, g))
            assert np.array_equal(qd, s * t)
            assert list((v & 2) != 0) == [False, True, True, False, True, True]
            assert list((v & 4) != 0) == [False, False, False, False, True, True]
            good = (v & 3) == 0
            assert np.array_equal(qf[good].view(np.uint64), qd[good].view(np.uint64))


def test_a_rect_need_not_look_at_the_lower_bound(lib):
    """with a t_min that rt_div_tmin_ok accepts, `bad if used` is `too large`: a quotient at or below the lower bound fails t_min.
    And such a quotient's division, which is below twice the bound, fails it too: the two forms reject alike.  Without such a t_min
    (zero, negative, -inf, NaN, tiny) the general guard does fire on zero and tiny quotients."""
    g = np.random.default_rng(8)
    lo, hi = 2.0 ** -300, 2.0 ** 300
    t = np.concatenate([[0.0, -0.0, lo, -lo, np.nextafter(lo, 1.0), 2 * lo, 5e-324, 1e-310, np.inf, -np.inf, np.nan, hi, np.nextafter(hi, 0.0), 0.001, 1.0, -1.0],
                        np.ldexp(g.uniform(1.0, 2.0, 4000), g.integers(-1070, 1023, 4000).astype(np.int32)) * g.choice([-1.0, 1.0], 4000)])
    t_mins = [0.001, np.nextafter(2 * lo, 1.0), 1.0, 1e300]
    t_maxs = [np.inf, 555.0, 0.0005, np.nan]
    for t_min in t_mins:
        for t_max in t_maxs:
            ok, bad, big = (np.empty(t.size, dtype=np.uint8) for _ in range(3))
            lib.ds_use(_p(t), _p(np.full(t.size, t_min)), _p(np.full(t.size, t_max)), C.c_uint64(t.size), _p(ok), _p(bad), _p(big))
            assert ok.all() and np.array_equal(bad, big)
            with np.errstate(invalid="ignore"):
                assert not np.any((np.abs(t) <= 2 * lo) & ~(t < t_min))      # whatever is down there fails t_min, so does anything within a factor 2
    for t_min in (0.0, -1.0, -np.inf, np.nan, lo, 2 * lo, 5e-324):
        ok, bad, big = (np.empty(t.size, dtype=np.uint8) for _ in range(3))
        lib.ds_use(_p(t), _p(np.full(t.size, t_min)), _p(np.full(t.size, np.inf)), C.c_uint64(t.size), _p(ok), _p(bad), _p(big))
        assert not ok.any()
    ok, bad, big = (np.empty(t.size, dtype=np.uint8) for _ in range(3))
    lib.ds_use(_p(t), _p(np.full(t.size, -np.inf)), _p(np.full(t.size, np.inf)), C.c_uint64(t.size), _p(ok), _p(bad), _p(big))
    assert bad[0] and bad[1] and bad[2] and bad[6] and not big[0] and not bad[13]
