"""Both denoisers and the batch variance against an independent statement of include/rt1w.h (tests/dn_reference.py: numpy longdouble,
np.exp and ** for the weights, written from the header's prose).  The other denoise tests compare one build of csrc/rt_denoise.h /
rt_denoise_var.h with another build of the same text, or check invariances; a slip in the definition itself -- a wrong B3 weight, a
sigma not halved, min for max, a shortened polynomial -- passes them all.  Here it does not: the twin and the kernels must agree with
the reference within 1e-12 on a synthetic image that has every edge the definition names.

CPU tier: the twins (librt1w_lab.so) against the reference; rt_dn_falloff and rt_dn_powi on their own against longdouble exp and pow.
GPU tier: the kernels against the twins bit for bit AND against the reference, so that a failure tells which side moved."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import dn_reference as ref
import orc

LD = np.longdouble
HERE = os.path.dirname(os.path.abspath(__file__))
ULPS = os.path.join(HERE, "golden", "denoise_elementary_ulps.json")

SHAPES = [(1, 1), (1, 40), (40, 1), (15, 17), (16, 16), (17, 33), (37, 53)]   # h x w
ITERATIONS = [1, 2, 3, 5, 8]
# the non-default parameter sets, at 37 x 53: (filter, keywords)
PARAMETER_SETS = [("denoise", (("sigma_colour", 0.3),)), ("denoise", (("sigma_depth", 0.9),)), ("denoise_var", (("sigma_depth", 0.9),)),
                  ("denoise", (("sigma_normal", 0.5),)), ("denoise", (("sigma_normal", 7.9),)), ("denoise", (("sigma_normal", 33.0),)),
                  ("denoise", (("sigma_normal", 1e9),)), ("denoise_var", (("sigma_normal", 0.5),)), ("denoise_var", (("sigma_normal", 7.9),)),
                  ("denoise_var", (("sigma_normal", 33.0),)), ("denoise_var", (("sigma_normal", 1e9),)), ("denoise_var", (("sigma_variance", 0.7),))]
MAX_UNDECIDABLE = 0.005   # of a case's pixels


# ------------------------------------------------------------------------------------------------------------------- inputs --

def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def synthetic(h, w, variant=""):
    """(frame [h, w, 3], aov [h, w, 8], var [h, w]), seeded, read-only.  Three interleaved regions of 9 rows x 11 columns with base
    normals x, y (perpendicular: weight exactly 0 were they not perturbed) and an oblique one; normals perturbed and of length
    0.3 .. 1; depth a ramp with noise and exact ties; a tenth of the pixels with coverage 0.5 .. 1; a corner block of misses; albedo
    0.005 .. 1 (the floor is 0.01) with a few 0, NaN and inf pixels; frame = albedo x region radiance x |1 + N(0, 0.3)|; var of the size of
    that noise with a rectangle of exact 0 and a few negative, NaN and inf entries.
    variant "corner" (for 33 x 37): frame pixels that are not finite on the corner where four 16 x 16 tiles meet."""
    rng = np.random.default_rng([2010, h, w])
    yy, xx = np.mgrid[0:h, 0:w]
    region = ((yy // 9) + (xx // 11)) % 3
    base = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.48, 0.6, 0.64]])
    radiance = np.array([[1.0, 0.8, 0.6], [0.2, 0.5, 0.9], [3.0, 2.5, 2.0]])
    aov = np.empty((h, w, 8))
    aov[..., 0:3] = rng.uniform(0.005, 1.0, (h, w, 3))
    aov[..., 3:6] = (base[region] + rng.normal(0.0, 0.05, (h, w, 3))) * rng.uniform(0.3, 1.0, (h, w, 1))
    depth = 2.0 + 0.05 * xx + 0.03 * yy + rng.normal(0.0, 0.01, (h, w))
    ties = rng.random((h, w)) < 0.15
    depth[ties] = np.round(depth[ties] * 4.0) / 4.0   # exact ties among neighbours: the ramp moves a quarter in 5 columns
    aov[..., 6] = depth
    aov[..., 7] = np.where(rng.random((h, w)) < 0.1, rng.uniform(0.5, 1.0, (h, w)), 1.0)
    mh, mw = (h + 3) // 4, (w + 3) // 4
    if h * w > 1:   # the miss block: the top right corner
        aov[:mh, w - mw:, 3:6] = 0.0
        aov[:mh, w - mw:, 6] = np.inf
        aov[:mh, w - mw:, 7] = 0.0
    n_special = min(3, (h * w) // 12)
    special = rng.choice(h * w, 3 * n_special, replace=False)
    for k, value in enumerate((0.0, np.nan, np.inf)):
        ys, xs = np.unravel_index(special[k * n_special:(k + 1) * n_special], (h, w))
        aov[ys, xs, 0:3] = value
    with np.errstate(invalid="ignore"):
        frame = aov[..., 0:3] * radiance[region] * np.abs(1.0 + rng.normal(0.0, 0.3, (h, w, 3)))
    lum = radiance[region] @ np.array([0.2126, 0.7152, 0.0722])
    var = (0.3 * lum) ** 2 * rng.uniform(0.5, 1.5, (h, w))
    var[h // 3:h // 3 + 7, w // 3:w // 3 + 9] = 0.0
    odd = rng.choice(h * w, 3 * n_special, replace=False)
    for k, value in enumerate((-1.0, np.nan, np.inf)):
        var.flat[odd[k * n_special:(k + 1) * n_special]] = value
    if variant == "corner":
        frame[16, 16] = np.nan
        frame[16, 17] = np.inf
        frame[17, 16, 0] = np.nan
        frame[17, 17, 1] = np.inf
    else:
        assert variant == ""
    return _frozen(frame, aov, var)


@functools.lru_cache(maxsize=None)
def reference(which, h, w, iterations, keep, params=(), variant=""):
    """(out longdouble [h, w, 3], undecidable [h, w], the integer normal power) of one case, computed once for both tiers"""
    frame, aov, var = synthetic(h, w, variant)
    kw = dict(params, iterations=iterations, keep_albedo=keep)
    out, mask = ref.denoise(frame, aov, **kw) if which == "denoise" else ref.denoise_var(frame, aov, var, **kw)
    return _frozen(out, mask) + (ref.normal_power(kw.get("sigma_normal", 0.0)),)


def twin(rt, which, h, w, iterations, keep, params=(), variant=""):
    frame, aov, var = synthetic(h, w, variant)
    kw = dict(params, iterations=iterations, keep_albedo=keep)
    return rt.denoise_host(frame, aov, **kw) if which == "denoise" else rt.denoise_var_host(frame, aov, var, **kw)


def against_reference(got, case, label):
    """Every finite channel within 1e-12 * max(1, P / 32) relative of the reference, P the integer normal power: the weight's rounding
    error is led by the P - 1 multiplications of the power (test_powi_against_pow), the whole filter measured 2.0e-14 at P = 32
    and 7.7e-13 at P = 4096, and 8 levels did not grow it.  What is not finite matches in kind and place.  Undecidable pixels (dn_reference.py) are left out; they
    may be at most 0.5 % of the case.  Returns (largest relative error, pixels left out)."""
    want, mask, power = reference(*case)
    tol = 1e-12 * max(1.0, power / 32.0)
    excluded = int(mask.sum())
    g = got.astype(LD)
    use = np.broadcast_to(~mask[..., None], want.shape)
    for kind in (np.isnan, np.isposinf, np.isneginf):
        assert np.array_equal(kind(g)[use], kind(want)[use]), (label, case, kind.__name__)
    fin = use & np.isfinite(want)
    with np.errstate(all="ignore"):
        err = np.where(want == 0, np.where(g == 0, LD(0), LD(np.inf)), np.abs(g - want) / np.abs(want))
    worst = float(err[fin].max()) if fin.any() else 0.0
    print(f"{label} {case[0]} {case[1]}x{case[2]} levels {case[3]} keep {int(case[4])} {dict(case[5])} {case[6]}: "
          f"max rel err {worst:.3e} (tol {tol:.1e}), excluded {excluded}")
    assert excluded <= MAX_UNDECIDABLE * mask.size, (label, case, excluded)
    assert worst <= tol, (label, case, worst, tol)
    return worst, excluded


# ------------------------------------------------------------------------------------------------------------------ CPU tier --

def test_the_reference_loads_no_library():
    """dn_reference.py stands on numpy alone: it must not import the package, ctypes or the oracle loader."""
    text = open(os.path.join(HERE, "dn_reference.py")).read()
    imports = [line.split()[1] for line in text.splitlines() if line.startswith(("import ", "from "))]
    assert imports == ["numpy"], imports
    assert np.finfo(ref.LD).nmant >= 63


@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("iterations", ITERATIONS)
@pytest.mark.parametrize("h,w", SHAPES)
@pytest.mark.parametrize("which", ["denoise", "denoise_var"])
def test_twin_against_reference(rt, which, h, w, iterations, keep):
    """rt1w_lab_denoise_host and rt1w_lab_denoise_var_host against the reference on the synthetic image: shapes from one pixel, one
    row and one column to 37 x 53 (the step exceeds the image from level 1, 4 or 6 on), every level count that matters, both flags."""
    case = (which, h, w, iterations, keep, (), "")
    against_reference(twin(rt, *case), case, "twin")


@pytest.mark.parametrize("which,params", PARAMETER_SETS)
@pytest.mark.parametrize("keep", [False, True])
def test_twin_against_reference_other_parameters(rt, which, params, keep):
    """The parameters off their defaults, 37 x 53, 5 levels: sigma_colour 0.3, sigma_depth 0.9, sigma_variance 0.7, and sigma_normal
    0.5 (clamped to power 1), 7.9 (truncated to 7), 33 and 1e9 (clamped to 4096)."""
    case = (which, 37, 53, 5, keep, params, "")
    against_reference(twin(rt, *case), case, "twin")
    assert ref.normal_power(0.5) == 1 and ref.normal_power(7.9) == 7 and ref.normal_power(33.0) == 33 and ref.normal_power(1e9) == 4096
    assert ref.normal_power() == 32


def test_the_synthetic_image_has_what_it_promises():
    """The edges the comparison is there for are in the input: all three regions, sub-floor albedo next to ordinary albedo, fractional
    coverage, depth ties between neighbours, misses, albedo and variance entries that are not finite, a variance-0 rectangle."""
    frame, aov, var = synthetic(37, 53)
    alb = aov[..., 0:3]
    assert (alb[np.isfinite(alb)] < 0.01).sum() > 10 and np.isnan(alb).any() and np.isposinf(alb).any() and (alb == 0).any()
    assert ((aov[..., 7] > 0) & (aov[..., 7] < 1)).sum() > 100 and (aov[..., 7] == 0).sum() > 50
    z = aov[..., 6]
    assert (np.isfinite(z[:, 1:]) & (z[:, 1:] == z[:, :-1])).sum() > 5 and np.isposinf(z).sum() > 50
    m = np.sqrt((aov[..., 3:6] ** 2).sum(-1))
    assert (m == 0).sum() > 50 and ((m > 0) & (m < 0.9)).sum() > 1000
    assert (var[12:19, 17:26] == 0).all() and (var < 0).any() and np.isnan(var).any() and np.isposinf(var).any()
    assert np.isnan(frame).any() and np.isposinf(frame).any() and frame[np.isfinite(frame)].min() >= 0.0


@functools.lru_cache(maxsize=None)
def batch_sums(K, n):
    """K batch sums on the 17 x 33 synthetic image, built so that the 1e-12 bound on the variance can be decided in 64 bits.  A batch
    luminance l_k reaches l_k - lbar with up to 6 roundings of its own (the product by 1 / n, the division by the albedo, three
    products and two sums): 6 * 2^-53 l_k.  An error common to all K, lbar's, drops out to first order (the deviations sum to 0).  So
    var carries about 12 * 2^-53 lbar / d relative, d the rms deviation: 1e-12 needs d > 1.3e-3 lbar, whoever computes it.  Per-channel
    noise alone does not give that: two batches whose luminances agree to 1e-5 of their mean turn up about once in a thousand pixels
    (measured on such sums: 5.7e-12 at a pixel with 1.4e-5, 1.2e-12 at 7.5e-5, below 7e-13 elsewhere).  So batch k of a pixel is its
    frame value times n (1 + 0.3 t_k), the t_k a per-pixel shuffle of K points spread evenly over -1 .. 1, times a per-channel
    |1 + N(0, 0.02)|: d is near 0.3 lbar for K = 2 and 0.18 lbar for K = 16, and check_batch_variance asserts d > 0.05 lbar.
    One pixel has a NaN sample and one an inf sample, next to the image's own albedo pixels that are not finite."""
    frame, aov, _ = synthetic(17, 33)
    rng = np.random.default_rng([2017, K, n])
    t = rng.permuted(np.broadcast_to(np.linspace(-1.0, 1.0, K)[:, None, None], (K, 17, 33)), axis=0)
    with np.errstate(invalid="ignore"):
        sums = n * frame[None] * (1.0 + 0.3 * t[..., None]) * np.abs(1.0 + rng.normal(0.0, 0.02, (K, 17, 33, 3)))
    sums[K - 1, 5, 7, 1] = np.nan
    sums[0, 9, 20, 2] = np.inf
    return _frozen(sums)[0]


@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("n", [1, 4, 1000])
@pytest.mark.parametrize("K", [2, 3, 4, 16])
def test_batch_variance_twin_against_reference(rt, K, n, keep):
    """rt1w_lab_batch_variance_host against the reference: var within 1e-12 relative where the reference's var exceeds 1e-20 times the
    squared mean luminance, within that threshold of it otherwise; frame within 4 ulp; a NaN or inf sample gives var == 0 exactly.
    batch_sums says why its batches are spread as they are."""
    check_batch_variance(rt.batch_variance_host(batch_sums(K, n), synthetic(17, 33)[1], n, keep_albedo=keep), K, n, keep, "twin")


@functools.lru_cache(maxsize=None)
def batch_reference(K, n, keep):
    return _frozen(*ref.batch_variance(batch_sums(K, n), synthetic(17, 33)[1], n, keep_albedo=keep))


def check_batch_variance(got, K, n, keep, label):
    frame, var = got
    sums = batch_sums(K, n)
    want_frame, want_var, lbar = batch_reference(K, n, keep)
    bad = ~np.isfinite(sums).all(axis=(0, 3))
    assert bad[5, 7] and bad[9, 20] and bad.sum() >= 4
    assert np.all(var[bad] == 0.0) and np.all(want_var[bad] == 0)
    assert np.all(np.isfinite(var)) and var.min() >= 0.0
    v = var.astype(LD)
    floor = LD(1e-20) * lbar * lbar
    with np.errstate(all="ignore"):
        big = np.isfinite(floor) & (want_var > floor)
        rel = np.abs(v - want_var) / want_var
        small_ok = np.abs(v - want_var) <= np.where(np.isfinite(floor), floor, LD(0))
        spread = np.sqrt(want_var * (K - 1)) / lbar   # rms deviation of the batch luminances over their mean
    assert spread[big].min() > 0.05, (label, K, n, keep, float(spread[big].min()))   # what batch_sums promises: the bound is decidable
    worst = float(rel[big].max())
    f = frame.astype(LD)
    for kind in (np.isnan, np.isposinf, np.isneginf):
        assert np.array_equal(kind(f), kind(want_frame)), (label, kind.__name__)
    fin = np.isfinite(want_frame)
    with np.errstate(all="ignore"):
        ulps = np.abs(f - want_frame) / np.spacing(np.abs(frame))
    frame_worst = float(ulps[fin].max())
    print(f"{label} batch variance K {K} n {n} keep {int(keep)}: var max rel err {worst:.3e} over {int(big.sum())} pixels, "
          f"{int((~big).sum())} at or under the floor; frame max {frame_worst:.3f} ulp")
    assert worst <= 1e-12, (label, K, n, keep, worst)
    assert small_ok[~big].all(), (label, K, n, keep)
    assert frame_worst <= 4.0, (label, K, n, keep, frame_worst)


# ------------------------------------------------------------------------------------------------ the elementary functions --

LN2 = 0.6931471805599453


@functools.lru_cache(maxsize=None)
def falloff_arguments():
    """2 M uniform points in (0, 40), 0.5 M log-uniform down to 1e-300, the range-reduction boundaries (n - 1/2) ln 2 below 40 with two
    neighbours on either side, the last double under 40, the smallest denormal and the smallest normal"""
    rng = np.random.default_rng(382)
    uni = rng.uniform(0.0, 40.0, 2_000_000)
    uni = uni[uni > 0.0]
    logu = 10.0 ** rng.uniform(-300.0, np.log10(40.0), 500_000)
    logu = logu[logu < 40.0]
    b = (np.arange(1, 59) - 0.5) * LN2
    assert 57 <= (b < 40.0).sum() <= 58
    near = [b]
    for direction in (0.0, 50.0):
        s = np.nextafter(b, direction)
        near += [s, np.nextafter(s, direction)]
    edges = np.array([np.nextafter(40.0, 0.0), 5e-324, np.finfo(np.float64).tiny])
    return _frozen(np.concatenate([uni, logu] + near + [edges]))[0]


POWERS = (1, 2, 7, 32, 33, 255, 4096)


@functools.lru_cache(maxsize=None)
def powi_arguments():
    """per power: 200 000 uniform points of (0, 1] and 1 - 10^-k, k = 1 .. 16"""
    rng = np.random.default_rng(4096)
    x = np.concatenate([1.0 - rng.uniform(0.0, 1.0, 200_000), 1.0 - 10.0 ** -np.arange(1.0, 17.0)])
    assert x.min() > 0.0 and x.max() <= 1.0
    return _frozen(np.tile(x, len(POWERS)), np.repeat(np.array(POWERS, dtype=np.uint32), x.size))


def _ulp_of(want):
    """the unit in the last place of a double at the true value `want` (longdouble): 2^(e - 53) for want in [2^(e-1), 2^e), and the
    denormal spacing below the normal range"""
    _, e = np.frexp(want)
    return np.ldexp(LD(1), np.maximum(e.astype(np.int64) - 53, -1074).astype(np.int32))


def measure_falloff(rt, device=0):
    x = falloff_arguments()
    got = rt.denoise_elementary("falloff", x, device=device)
    want = np.exp(-x.astype(LD))
    d = np.abs(got.astype(LD) - want) / _ulp_of(want)
    i = int(np.argmax(d))
    return got, {"n": int(x.size), "max_ulp": round(float(d[i]), 4), "at": float(x[i])}


def measure_powi(rt, device=0):
    x, e = powi_arguments()
    got = rt.denoise_elementary("powi", x, e, device=device)
    want = x.astype(LD) ** e.astype(LD)
    d = np.abs(got.astype(LD) - want) / _ulp_of(want)
    out = {}
    for p in POWERS:
        sel = np.flatnonzero(e == p)
        i = sel[int(np.argmax(d[sel]))]
        out[str(p)] = {"n": int(sel.size), "max_ulp": round(float(d[i]), 4), "at": float(x[i])}
    return got, out


def test_falloff_against_exp(rt):
    """rt_dn_falloff on its own: within 2 ulp of longdouble exp(-x) over (0, 40) (1.13 measured on a restatement; the header claims a
    truncation error below 5e-18, the rest is the rounding of 14 Horner steps and of the reduction), and the exact cases."""
    rec = json.load(open(ULPS))
    _, m = measure_falloff(rt)
    print(f"falloff: n {m['n']} max {m['max_ulp']} ulp at x = {m['at']!r} (recorded {rec['falloff']['max_ulp']})")
    assert m["max_ulp"] <= 2.0
    assert m["max_ulp"] <= rec["falloff"]["max_ulp"] + 0.01, "worse than the recorded maximum: tests/golden/denoise_elementary_ulps.json"
    exact = np.array([-0.0, 0.0, -1.0, -5e-324, -np.inf, 40.0, np.nextafter(40.0, 50.0), 1e300, np.inf, np.nan])
    assert np.array_equal(rt.denoise_elementary("falloff", exact), np.array([1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0]))
    edge = rt.denoise_elementary("falloff", np.array([np.nextafter(40.0, 0.0), 5e-324, np.finfo(np.float64).tiny]))
    assert 4.2e-18 < edge[0] < 4.3e-18 and edge[1] == 1.0 and edge[2] == 1.0


def test_powi_against_pow(rt):
    """rt_dn_powi on its own: within P ulp of longdouble x ** P for P = 1, 2, 7, 32, 33, 255, 4096 over (0, 1].  Binary exponentiation
    brackets the P factors in some order; whatever the order, the rounding errors of at most P - 1 multiplications reach the result,
    each 2^-53 relative at most, so (P - 1) 2^-53 relative: between (P - 1) / 2 and P - 1 ulp, by where in its binade the result
    lies.  Measured: 0.60 P at 4096, at most 0.81 P below (tests/golden/denoise_elementary_ulps.json).  0 and 1 are exact."""
    rec = json.load(open(ULPS))
    _, m = measure_powi(rt)
    for p in POWERS:
        g = m[str(p)]
        print(f"powi P = {p}: n {g['n']} max {g['max_ulp']} ulp at x = {g['at']!r} (recorded {rec['powi'][str(p)]['max_ulp']})")
    for p in POWERS:
        assert m[str(p)]["max_ulp"] <= p, (p, m[str(p)])
        assert m[str(p)]["max_ulp"] <= rec["powi"][str(p)]["max_ulp"] + 0.01, p
    for p in POWERS:
        assert np.array_equal(rt.denoise_elementary("powi", np.array([0.0, 1.0]), p), np.array([0.0, 1.0])), p
    with pytest.raises(rt.Rt1wError):
        rt.denoise_elementary("falloff", np.ones(4), device=2)


# ------------------------------------------------------------------------------------------------------------------ GPU tier --

def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.fixture(scope="module")
def cornell(rt, gpu_ctx_factory):
    return gpu_ctx_factory(rt.Scene.reference(5, build_seed=1))


def _gpu(ctx, which, h, w, iterations, keep, params=(), variant=""):
    frame, aov, var = synthetic(h, w, variant)
    kw = dict(params, iterations=iterations, keep_albedo=keep)
    return ctx.denoise(frame, aov, **kw) if which == "denoise" else ctx.denoise_var(frame, aov, var, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", SHAPES)
@pytest.mark.parametrize("which", ["denoise", "denoise_var"])
def test_gpu_against_twin_and_reference(rt, cornell, which, h, w):
    """rt1w_denoise and rt1w_denoise_var on the synthetic image, 1, 2, 3, 5 and 8 levels, both flags: the bits of the twin, and the
    reference within the tolerance.  The shapes put the image edge inside the staged halo on every side, leave a partial 16 x 16 tile
    in both axes and make the step exceed the image."""
    for iterations in ITERATIONS:
        for keep in (False, True):
            case = (which, h, w, iterations, keep, (), "")
            got = _gpu(cornell, *case)
            assert _same(got, twin(rt, *case)), case
            against_reference(got, case, "gpu")


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["denoise", "denoise_var"])
def test_gpu_values_that_are_not_finite_on_a_tile_corner(rt, cornell, which):
    """33 x 37 with NaN and inf frame pixels at rows and columns 16 and 17, where four 16 x 16 tiles meet: each is staged into the
    halo of its three neighbours."""
    for iterations in (1, 2, 5):
        for keep in (False, True):
            case = (which, 33, 37, iterations, keep, (), "corner")
            got = _gpu(cornell, *case)
            assert _same(got, twin(rt, *case)), case
            against_reference(got, case, "gpu")
            assert np.isnan(got[16, 16]).all() and np.isposinf(got[16, 17]).all() and np.isnan(got[17, 16, 0]) and np.isposinf(got[17, 17, 1])


class _DeviceBuffers:
    """plain device memory of the HIP runtime this process already uses"""

    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")
        self.made = []

    def upload(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), C.c_size_t(a.nbytes)) == 0
        self.made.append(p)
        assert self.hip.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0  # HostToDevice
        return p.value

    def fetch(self, p, shape):
        out = np.empty(shape)
        assert self.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(p), C.c_size_t(out.nbytes), 2) == 0  # DeviceToHost
        return out

    def free(self):
        for p in self.made:
            self.hip.hipFree(p)


@pytest.mark.gpu
def test_gpu_in_place_device_forms(rt, cornell):
    """rt1w_denoise_device and rt1w_denoise_var_device with d_out == d_frame on 17 x 33, through plain hipMalloc buffers: twin and
    reference as above, and the guides and the variance come back untouched."""
    h, w = 17, 33
    frame, aov, var = synthetic(h, w)
    dev = _DeviceBuffers()
    try:
        for which in ("denoise", "denoise_var"):
            for iterations in (2, 5):
                case = (which, h, w, iterations, False, (), "")
                d_frame, d_aov, d_var = dev.upload(frame), dev.upload(aov), dev.upload(var)
                if which == "denoise":
                    cornell.denoise_device(d_frame, d_aov, d_frame, w, h, iterations=iterations)
                else:
                    cornell.denoise_var_device(d_frame, d_aov, d_var, d_frame, w, h, iterations=iterations)
                got = dev.fetch(d_frame, (h, w, 3))
                assert _same(got, twin(rt, *case)), case
                against_reference(got, case, "gpu in place")
                assert _same(dev.fetch(d_aov, (h, w, 8)), aov) and _same(dev.fetch(d_var, (h, w)), var)
    finally:
        dev.free()


@pytest.mark.gpu
@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("n", [1, 4, 1000])
@pytest.mark.parametrize("K", [2, 3, 4, 16])
def test_gpu_batch_variance_against_twin_and_reference(rt, cornell, K, n, keep):
    """rt1w_batch_variance on the synthetic sums: the bits of the twin, and the reference within the bounds of the CPU tier."""
    aov = synthetic(17, 33)[1]
    frame, var = cornell.batch_variance(batch_sums(K, n), aov, n, keep_albedo=keep)
    tf, tv = rt.batch_variance_host(batch_sums(K, n), aov, n, keep_albedo=keep)
    assert _same(frame, tf) and _same(var, tv), (K, n, keep)
    check_batch_variance((frame, var), K, n, keep, "gpu")


@pytest.mark.gpu
def test_gpu_elementary_functions_equal_the_host_build(rt):
    """rt_dn_falloff and rt_dn_powi, one lane per element on the GPU, over the sweeps of the CPU tier: the bits of the host build."""
    host, _ = measure_falloff(rt, device=0)
    dev, m = measure_falloff(rt, device=1)
    print(f"falloff on the device: n {m['n']} max {m['max_ulp']} ulp")
    assert _same(host, dev)
    host, _ = measure_powi(rt, device=0)
    dev, _ = measure_powi(rt, device=1)
    assert _same(host, dev)
    exact = np.array([-0.0, 0.0, -1.0, 40.0, np.inf, np.nan])
    assert _same(rt.denoise_elementary("falloff", exact, device=1), rt.denoise_elementary("falloff", exact, device=0))
