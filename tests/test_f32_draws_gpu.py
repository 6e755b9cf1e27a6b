"""The draw contract of the single-precision builds on the GPU: rt1w_lab_f32_draws with device 1 runs csrc/rt_f32_draws.h over the f32
build of include/rt1w_num.h, one lane per word, in the translation unit of the f32 kernels' exact build.  The device must meet the
assertions of tests/test_f32_draws.py on its own (the expected side there is Python integers and numpy) and equal the host build bit for
bit: every step is an integer operation, a correctly rounded f64 multiply, add or compare, or a conversion."""
import numpy as np
import pytest

from test_f32_draws import RANGES, check_range, check_unit, range_words, unit_words

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    return a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_unit_draw_on_the_device(rt):
    assert rt.device_count() >= 1, "no HIP device visible: GPU tests must run on the GPU box"
    words = unit_words()
    out = rt.f32_draws("unit", words, device=1)
    check_unit(out, words)
    for name in ("unit", "take_unit", "gen_unit"):
        assert same_bits(rt.f32_draws(name, words, device=1), rt.f32_draws(name, words, device=0)), name
        assert same_bits(rt.f32_draws(name, words, device=1), out), name


@pytest.mark.parametrize("lo,hi", RANGES)
def test_range_draw_on_the_device(rt, lo, hi):
    assert rt.device_count() >= 1, "no HIP device visible: GPU tests must run on the GPU box"
    words = range_words(lo, hi)
    single = rt.f32_draws("range_single", words, lo, hi, device=1)
    assert same_bits(single, rt.f32_draws("range_single", words, lo, hi, device=0))
    for name in ("take_range", "gen_range"):
        got = rt.f32_draws(name, words, lo, hi, device=1)
        check_range(single, got, words, lo, hi)
        assert same_bits(got, rt.f32_draws(name, words, lo, hi, device=0)), name
    if (lo, hi) == (-1.0, 1.0):
        assert same_bits(rt.f32_draws("pm1", words, device=1), single)
