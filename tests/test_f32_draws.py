"""The draw contract of the single-precision builds (include/rt1w_num.h under RT_F32), on the host build of the f32 core.

rand's floats are half-open: a unit draw is in [0, 1) and a range draw in [low, high) as FLOATS.  The f32 builds take the 64-bit draw
(k 2^-53 with k = word >> 11; low + (m 2^-52) (high - low) with m = word >> 12) and round it to float where it is assigned, so the open
end has to survive that rounding.  The expected side here is Python integers and numpy float64 / float32 only; the code under test is
rt1w_lab_f32_draws (csrc/rt_f32_draws.h over rt1w_num.h), device 0 = its host build.  tests/test_f32_draws_gpu.py runs the same words on
the device and holds it to this build bit for bit."""
import numpy as np
import pytest

ONE_BELOW = np.float32(1.0) - np.float32(2.0 ** -24)      # 1 - 2^-24: the largest float below 1
FIRST_TO_ONE = (1 << 53) - (1 << 28)                      # the first k whose k 2^-53 rounds to 1.0f (the tie at 1 - 2^-25 goes to even)
RANGES = ((213.0, 343.0), (227.0, 332.0), (0.0, 1.0), (-1.0, 1.0))   # Cornell's light in x and z, the shutter, the samplers' cube


def unit_words():
    """64-bit generator words for the unit draw: the ends, the last 4096 values of k, the first k that rounds to 1.0f +- 8, bits set
    and clear under the shift (they must not matter), random words."""
    w = [0, (1 << 64) - 1]
    w += [((1 << 53) - j) << 11 for j in range(1, 4097)]
    w += [(FIRST_TO_ONE + d) << 11 for d in range(-8, 9)]
    for k in (1, 3, (1 << 52) + 1, FIRST_TO_ONE - 1, FIRST_TO_ONE, (1 << 53) - 1):
        w += [k << 11, (k << 11) | 0x7FF, (k << 11) | 0x400, (k << 11) | 1]
    w += [int(x) for x in np.random.default_rng(20251).integers(0, 1 << 64, 65536, dtype=np.uint64)]
    return np.array(w, dtype=np.uint64)


def range_single64(m, lo, hi):
    """rand 0.8's UniformFloat::sample_single on 52 mantissa bits m, in float64: ((1 + m 2^-52) - 1) * (hi - lo) + lo.  m 2^-52 and
    hi - lo are exact for these bounds; the product and the sum round once each, as IEEE doubles do here and there."""
    return (m.astype(np.float64) * 2.0 ** -52) * np.float64(hi - lo) + np.float64(lo)


def first_rounding_onto_high(lo, hi):
    """the smallest m whose single take rounds to a float >= hi (the take is monotone in m), by bisection"""
    a, b = 0, (1 << 52) - 1
    top = np.float32(range_single64(np.array([b], dtype=np.uint64), lo, hi))[0]
    assert top >= np.float32(hi), "the last value rounds onto `high` for every one of these ranges"
    while a < b:
        mid = (a + b) // 2
        if np.float32(range_single64(np.array([mid], dtype=np.uint64), lo, hi))[0] >= np.float32(hi):
            b = mid
        else:
            a = mid + 1
    return a


def range_words(lo, hi):
    m0 = first_rounding_onto_high(lo, hi)
    w = [0, (1 << 64) - 1]
    w += [((1 << 52) - j) << 12 for j in range(1, 4097)]
    w += [(m0 + d) << 12 for d in range(-8, 9)]
    w += [(m0 << 12) | 0xFFF, ((m0 - 1) << 12) | 0xFFF, 1 << 12, 0xFFF]
    w += [int(x) for x in np.random.default_rng(20252).integers(0, 1 << 64, 65536, dtype=np.uint64)]
    return np.array(w, dtype=np.uint64)


def check_unit(out, words):
    k = words >> np.uint64(11)
    x = k.astype(np.float64) * 2.0 ** -53          # exact: k < 2^53
    assert out.dtype == np.float32
    assert (out < np.float32(1.0)).all(), f"{int((out >= 1).sum())} unit draws reach 1.0f"
    assert (out >= 0).all()
    assert (np.abs(out.astype(np.float64) - x) <= 2.0 ** -24).all()
    nearest = x.astype(np.float32)                 # round to nearest even
    below = nearest < np.float32(1.0)
    assert np.array_equal(out[below], nearest[below])
    assert (out[~below] == ONE_BELOW).all() and (~below).sum() >= 4096
    assert np.array_equal(below, k < np.uint64(FIRST_TO_ONE))
    order = np.argsort(k, kind="stable")
    assert (np.diff(out[order].astype(np.float64)) >= 0).all(), "the unit draw is not monotone in k"


def check_range(single, retried, words, lo, hi):
    m = words >> np.uint64(12)
    want = range_single64(m, lo, hi).astype(np.float32)
    assert np.array_equal(single, want)
    assert (single >= np.float32(lo)).all() and (retried >= np.float32(lo)).all()
    onto_high = want >= np.float32(hi)
    assert onto_high.sum() >= 4096 and (~onto_high).sum() >= 60000
    # the stream behind the word holds the word 0, whose draw is `lo`: that is what a rejected word comes back as
    assert (retried < np.float32(hi)).all(), f"{int((retried >= np.float32(hi)).sum())} range draws reach `high` as floats"
    assert np.array_equal(retried[~onto_high], want[~onto_high])
    assert (retried[onto_high] == np.float32(lo)).all()


def test_unit_draw_is_half_open(rt):
    """A unit draw of the f32 builds is the float nearest k 2^-53, except that 1.0f becomes 1 - 2^-24: in [0, 1), within 2^-24 of the
    64-bit draw, monotone in k, and the bits under the shift do not matter.  All three spellings (rt_f64_from_bits, rt_take_f64,
    rt_gen_f64).  With the rounding alone -- the rule before this contract -- these assertions fail for every k >= 2^53 - 2^28, that
    is 2^28 of the 2^53 values of k: 2^-25 of the draws were 1.0f (a few in a 600x600x256 frame, each a NaN pixel through the cosine
    lobe's 0 / 0)."""
    words = unit_words()
    out = rt.f32_draws("unit", words)
    check_unit(out, words)
    assert np.array_equal(rt.f32_draws("take_unit", words), out)
    assert np.array_equal(rt.f32_draws("gen_unit", words), out)


@pytest.mark.parametrize("lo,hi", RANGES)
def test_range_draw_is_half_open(rt, lo, hi):
    """A range draw of the f32 builds: the single take is rand's 64-bit statement rounded to float (so it can equal `high`: shown by
    "range_single", which does not retry), never below `low`; and every word whose single take is >= high as a float is one that the
    retrying draws rt_take_range and rt_gen_range reject -- they return the draw of the next word instead (here `low`).  Before this
    contract the retry compared in 64 bits and rounded afterwards: the camera's shutter time could equal time1."""
    words = range_words(lo, hi)
    single = rt.f32_draws("range_single", words, lo, hi)
    check_range(single, rt.f32_draws("take_range", words, lo, hi), words, lo, hi)
    check_range(single, rt.f32_draws("gen_range", words, lo, hi), words, lo, hi)


def test_the_samplers_cube_draw(rt):
    """rt_take_pm1 / rt_pm1_from_bits (the unit sphere's and disk's gen_range(-1.0..1.0), which has no retry of its own) is the single
    take of (-1, 1) bit for bit.  It can therefore be 1.0f; a candidate with such a coordinate has squared length >= 1 in float
    arithmetic (1 * 1 is exact and the other squares are not negative), so the samplers' own `< 1` rejects it."""
    words = range_words(-1.0, 1.0)
    pm1 = rt.f32_draws("pm1", words)
    assert np.array_equal(pm1, rt.f32_draws("range_single", words, -1.0, 1.0))
    one = pm1 == np.float32(1.0)
    assert one.sum() >= 4096 and (pm1[~one] < np.float32(1.0)).all() and (pm1 >= np.float32(-1.0)).all()
    other = np.float32(np.random.default_rng(3).uniform(-1, 1, (int(one.sum()), 2)))
    assert ((pm1[one] * pm1[one] + other[:, 0] * other[:, 0]) + other[:, 1] * other[:, 1] >= np.float32(1.0)).all()


def test_refusals(rt):
    w = np.zeros(4, dtype=np.uint64)
    for bad in (dict(lo=1.0, hi=1.0), dict(lo=2.0, hi=1.0), dict(lo=0.0, hi=float("inf")), dict(lo=float("nan"), hi=1.0),
                dict(lo=-3e38, hi=3e38)):
        for name in ("range_single", "take_range", "gen_range"):
            with pytest.raises(rt.Rt1wError):
                rt.f32_draws(name, w, **bad)
    with pytest.raises(rt.Rt1wError):
        rt.f32_draws("unit", w, device=2)
