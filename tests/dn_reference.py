"""An independent statement of the two denoisers and the batch variance, written from the prose of include/rt1w.h (the comment blocks
"feature-guided denoiser" and "variance-guided denoiser") and from nothing else: no library is loaded, nothing of csrc/rt_denoise.h or
csrc/rt_denoise_var.h is shared.  Everything is numpy longdouble (64 bits of mantissa or more: asserted), whole images at a time, one
shifted slice per tap; the falloff is np.exp and the normal weight is `**`, where the kernels have a polynomial and binary exponentiation.
So the two sides differ in precision, in order of evaluation and in how exp and pow are computed: what they share is the definition.

tests/test_denoise_reference.py holds the kernels and their CPU twins to this, within 1e-12.

The definition is continuous in its inputs but for one place: the variance-guided colour term with v_p + v_q == 0 is 0 (weight kept)
where l_p == l_q and +inf (weight 0) where they differ, however little.  Two evaluations that round l differently may fall on either
side.  denoise_var therefore returns, next to the image, a mask of the pixels that saw such a tap with l_p, l_q unequal and within 1e-9
relative, or whose later levels read a pixel that did.  (The cut-off k(x) = 0 at x >= 40 is no such place: it drops at most e^-40.)"""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "numpy longdouble is no wider than double here: the reference would prove nothing"

EPS = LD(0.01)                    # albedo floor
DEFAULT_LEVELS = 5
SIGMA_COLOUR, SIGMA_NORMAL, SIGMA_DEPTH, SIGMA_VARIANCE = 1.0, 32.0, 0.1, 3.0
INV_SIGMA_COVERAGE2 = LD(16)      # sigma_coverage = 1/4
CUTOFF = LD(40)
B3 = (LD(3) / 8, LD(1) / 4, LD(1) / 16)
LUM = (LD(0.2126), LD(0.7152), LD(0.0722))
NEAR = LD(1e-9)                   # "within 1e-9 relative": the undecidable band of the variance form


def normal_power(sigma_normal=0.0):
    """`sigma_normal` (0 = 32) truncated to an integer and clamped to 1 .. 4096"""
    sn = SIGMA_NORMAL if sigma_normal == 0 else sigma_normal
    return int(min(max(np.trunc(sn), 1.0), 4096.0))


def luminance(c):
    return (LUM[0] * c[..., 0] + LUM[1] * c[..., 1]) + LUM[2] * c[..., 2]


def albedo_floor(aov, keep_albedo):
    a = np.asarray(aov, dtype=np.float64)[..., 0:3].astype(LD)
    if keep_albedo:
        return np.ones_like(a)
    return np.where(np.isfinite(a) & (a > EPS), a, EPS)


def prepare(frame, aov, keep_albedo=False):
    """The prepare pass: (A, c, l, u, z, coverage) of every pixel"""
    frame = np.asarray(frame, dtype=np.float64)
    aov = np.asarray(aov, dtype=np.float64)
    assert frame.ndim == 3 and frame.shape[2] == 3 and aov.shape == frame.shape[:2] + (8,)
    A = albedo_floor(aov, keep_albedo)
    with np.errstate(all="ignore"):
        c = frame.astype(LD) / A
        n = aov[..., 3:6].astype(LD)
        m2 = (n * n).sum(axis=-1)
        m2_double = (aov[..., 3:6] ** 2).sum(axis=-1)   # "is 0, underflows or is not finite" speaks of the 64-bit square
        unit = (m2_double > 0) & np.isfinite(m2_double)
        u = np.where(unit[..., None], n / np.sqrt(np.where(unit, m2, 1))[..., None], LD(0))
    return A, c, luminance(c), u, aov[..., 6].astype(LD), aov[..., 7].astype(LD)


def falloff(x):
    """k(x): 1 for x <= 0; exp(-x) for 0 < x < 40; 0 for x >= 40, +inf and NaN"""
    with np.errstate(all="ignore"):
        inside = (x > 0) & (x < CUTOFF)
        return np.where(x <= 0, LD(1), np.where(inside, np.exp(-np.where(inside, x, LD(1))), LD(0)))


def _taps(h, w, step):
    """(dy, dx, slices of p, slices of q) of the taps q = p + step (dx, dy) that lie inside the image, in row order"""
    for dy in range(-2, 3):
        oy = dy * step
        if abs(oy) >= h:
            continue
        for dx in range(-2, 3):
            ox = dx * step
            if abs(ox) >= w:
                continue
            p = (slice(max(0, -oy), h - max(0, oy)), slice(max(0, -ox), w - max(0, ox)))
            q = (slice(max(0, oy), h - max(0, -oy)), slice(max(0, ox), w - max(0, -ox)))
            yield dy, dx, p, q


def _filter(frame, aov, var, iterations, keep_albedo, sigma_colour, sigma_normal, sigma_depth, sigma_variance):
    levels = DEFAULT_LEVELS if iterations == 0 else int(iterations)
    assert 1 <= levels <= 8
    power = normal_power(sigma_normal)
    s_colour = LD(SIGMA_COLOUR if sigma_colour == 0 else sigma_colour)
    s_depth = LD(SIGMA_DEPTH if sigma_depth == 0 else sigma_depth)
    A, c, l, u, z, cov = prepare(frame, aov, keep_albedo)
    h, w = l.shape
    variance_form = var is not None
    if variance_form:
        var = np.asarray(var, dtype=np.float64)
        assert var.shape == (h, w)
        s_var = LD(SIGMA_VARIANCE if sigma_variance == 0 else sigma_variance)
        v = np.where(np.isfinite(var) & (var >= 0), var, 0.0).astype(LD)
    undecidable = np.zeros((h, w), dtype=bool)
    with np.errstate(all="ignore"):
        for i in range(levels):
            step = 2 ** i
            num = np.zeros((h, w, 3), dtype=LD)
            den = np.zeros((h, w), dtype=LD)
            vnum = np.zeros((h, w), dtype=LD)
            marked = undecidable.copy()
            for dy, dx, p, q in _taps(h, w, step):
                hw = B3[abs(dx)] * B3[abs(dy)]
                if dx == 0 and dy == 0:
                    wt = np.full((h, w), hw)   # the centre tap: h(0, 0) whatever the guides say
                else:
                    up, uq = u[p], u[q]
                    both_zero = np.all(up == 0, axis=-1) & np.all(uq == 0, axis=-1)
                    wn = np.where(both_zero, LD(1), np.clip((up * uq).sum(axis=-1), LD(0), LD(1)) ** power)
                    zp, zq = z[p], z[q]
                    one_inf = np.isposinf(zp) != np.isposinf(zq)
                    x_depth = np.where(zp == zq, LD(0), np.where(one_inf, LD(np.inf), np.abs(zp - zq) / (np.maximum(zp, zq) * s_depth)))
                    dv = cov[p] - cov[q]
                    x_coverage = (dv * dv) * INV_SIGMA_COVERAGE2
                    lp, lq = l[p], l[q]
                    dl2 = (lp - lq) ** 2
                    if variance_form:
                        vsum = v[p] + v[q]
                        x_colour = np.where(lp == lq, LD(0), dl2 / (s_var * s_var * vsum))   # a zero denominator: +inf
                        knife = (vsum == 0) & (lp != lq) & (np.abs(lp - lq) <= NEAR * np.maximum(np.abs(lp), np.abs(lq)))
                        knife &= np.isfinite(lp) & np.isfinite(lq)   # a value that is not finite is rejected, near or far
                        knife &= (hw * wn) * falloff(x_depth + x_coverage) > 0    # a tap the guides reject is 0 on either side
                        marked[p] |= knife
                    elif i == 0:
                        x_colour = LD(0) * dl2   # no colour term on level 0; a value that is not finite still gives NaN
                    else:
                        sigma_i = s_colour / LD(2) ** i
                        x_colour = dl2 / (sigma_i * sigma_i)
                    wt = (hw * wn) * falloff((x_depth + x_colour) + x_coverage)
                    marked[p] |= undecidable[q]   # later levels: whoever reads a marked pixel is marked
                take = wt > 0   # not 0, not NaN
                wt = np.where(take, wt, LD(0))
                num[p] += wt[..., None] * np.where(take[..., None], c[q], LD(0))
                den[p] += wt
                if variance_form:
                    vnum[p] += wt * wt * v[q]
            through = ~np.isfinite(l)   # a centre pixel whose luminance is not finite is passed through unchanged
            c = np.where(through[..., None], c, num / np.where(through, LD(1), den)[..., None])
            l = np.where(through, l, luminance(c))
            if variance_form:
                v = np.where(through, v, vnum / np.where(through, LD(1), den * den))
            undecidable = marked
        out = c * A
    return out, undecidable


def denoise(frame, aov, iterations=0, keep_albedo=False, sigma_colour=0.0, sigma_normal=0.0, sigma_depth=0.0):
    """rt1w_denoise: (out longdouble [h, w, 3], undecidable bool [h, w] -- all False: this form has no discontinuity)"""
    return _filter(frame, aov, None, iterations, keep_albedo, sigma_colour, sigma_normal, sigma_depth, 0.0)


def denoise_var(frame, aov, var, sigma_variance=0.0, iterations=0, keep_albedo=False, sigma_normal=0.0, sigma_depth=0.0):
    """rt1w_denoise_var: (out longdouble [h, w, 3], undecidable bool [h, w])"""
    return _filter(frame, aov, var, iterations, keep_albedo, 0.0, sigma_normal, sigma_depth, sigma_variance)


def batch_variance(sums, aov, n, keep_albedo=False):
    """rt1w_batch_variance: (frame, var, lbar), longdouble [h, w, 3], [h, w], [h, w]"""
    sums = np.asarray(sums, dtype=np.float64)
    K = sums.shape[0]
    assert 2 <= K <= 16 and n >= 1 and sums.ndim == 4 and sums.shape[3] == 3
    S = sums.astype(LD)
    A = albedo_floor(aov, keep_albedo)
    with np.errstate(all="ignore"):
        total = S.sum(axis=0)
        frame = np.where(np.isnan(total), LD(0), total) / LD(K * n)
        lk = luminance((S / LD(n)) / A)
        lbar = lk.sum(axis=0) / LD(K)
        var = ((lk - lbar) ** 2).sum(axis=0) / LD(K * (K - 1))
        var = np.where(np.isfinite(var) & (var >= 0), var, LD(0))
    return frame, var, lbar
