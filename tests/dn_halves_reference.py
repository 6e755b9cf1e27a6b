"""An independent statement of rt1w_halves_resolve's variance and of rt1w_denoise_var_halves, written from the prose of include/rt1w.h (the
comment block "adaptive sampling steered by the error that remains AFTER the filter") in numpy longdouble, beside tests/dn_reference.py, whose
prepare pass, falloff, tap walk and constants it takes: no library is loaded, nothing of csrc/rt_denoise_halves.h is shared.

tests/test_adaptive_filtered.py holds the CPU twins to this, within 1e-12 where the quantity is well conditioned."""
import numpy as np

import dn_reference as R

LD = R.LD
ERR_FLOOR = LD(0.01)


def halves_variance(batches_a, batches_b, aov, n, keep_albedo=False):
    """var of rt1w_halves_resolve by its meaning: the variance of the mean demodulated luminance over ALL batches of both halves.
    batches_x: [m_x, h, w, 3] raw sums.  longdouble [h, w]"""
    S = np.concatenate([np.asarray(batches_a, dtype=np.float64), np.asarray(batches_b, dtype=np.float64)]).astype(LD)
    m = S.shape[0]
    A = R.albedo_floor(aov, keep_albedo)
    lk = R.luminance((S / LD(n)) / A)
    lbar = lk.sum(axis=0) / LD(m)
    return ((lk - lbar) ** 2).sum(axis=0) / LD(m * (m - 1))


def denoise_var_halves(frame, aov, var, half_a, half_b, sigma_variance=0.0, iterations=0, keep_albedo=False, sigma_normal=0.0, sigma_depth=0.0):
    """rt1w_denoise_var_halves: (out, a', b', err_px, undecidable), longdouble; a', b' are the filtered halves with the albedo back.
    `undecidable` as tests/dn_reference.py defines it."""
    levels = R.DEFAULT_LEVELS if iterations == 0 else int(iterations)
    power = R.normal_power(sigma_normal)
    s_depth = LD(R.SIGMA_DEPTH if sigma_depth == 0 else sigma_depth)
    s_var = LD(R.SIGMA_VARIANCE if sigma_variance == 0 else sigma_variance)
    A, c, l, u, z, cov = R.prepare(frame, aov, keep_albedo)
    h, w = l.shape
    var = np.asarray(var, dtype=np.float64)
    v = np.where(np.isfinite(var) & (var >= 0), var, 0.0).astype(LD)
    with np.errstate(all="ignore"):
        ha = np.asarray(half_a, dtype=np.float64).astype(LD) / A
        hb = np.asarray(half_b, dtype=np.float64).astype(LD) / A
        undecidable = np.zeros((h, w), dtype=bool)
        for i in range(levels):
            num = np.zeros((h, w, 3), dtype=LD)
            na = np.zeros((h, w, 3), dtype=LD)
            nb = np.zeros((h, w, 3), dtype=LD)
            den = np.zeros((h, w), dtype=LD)
            vnum = np.zeros((h, w), dtype=LD)
            marked = undecidable.copy()
            for dy, dx, p, q in R._taps(h, w, 2 ** i):
                hw = R.B3[abs(dx)] * R.B3[abs(dy)]
                if dx == 0 and dy == 0:
                    wt = np.full((h, w), hw)
                else:
                    up, uq = u[p], u[q]
                    both_zero = np.all(up == 0, axis=-1) & np.all(uq == 0, axis=-1)
                    wn = np.where(both_zero, LD(1), np.clip((up * uq).sum(axis=-1), LD(0), LD(1)) ** power)
                    zp, zq = z[p], z[q]
                    one_inf = np.isposinf(zp) != np.isposinf(zq)
                    x_depth = np.where(zp == zq, LD(0), np.where(one_inf, LD(np.inf), np.abs(zp - zq) / (np.maximum(zp, zq) * s_depth)))
                    dv = cov[p] - cov[q]
                    x_coverage = (dv * dv) * R.INV_SIGMA_COVERAGE2
                    lp, lq = l[p], l[q]
                    vsum = v[p] + v[q]
                    x_colour = np.where(lp == lq, LD(0), (lp - lq) ** 2 / (s_var * s_var * vsum))
                    knife = (vsum == 0) & (lp != lq) & (np.abs(lp - lq) <= R.NEAR * np.maximum(np.abs(lp), np.abs(lq)))
                    knife &= np.isfinite(lp) & np.isfinite(lq)
                    knife &= (hw * wn) * R.falloff(x_depth + x_coverage) > 0
                    marked[p] |= knife
                    wt = (hw * wn) * R.falloff((x_depth + x_colour) + x_coverage)   # the halves never enter a weight
                    marked[p] |= undecidable[q]
                take = wt > 0
                wt = np.where(take, wt, LD(0))
                for acc, src in ((num, c), (na, ha), (nb, hb)):
                    acc[p] += wt[..., None] * np.where(take[..., None], src[q], LD(0))
                den[p] += wt
                vnum[p] += wt * wt * v[q]
            through = ~np.isfinite(l)   # all three values pass through unchanged
            d1 = np.where(through, LD(1), den)
            c = np.where(through[..., None], c, num / d1[..., None])
            ha = np.where(through[..., None], ha, na / d1[..., None])
            hb = np.where(through[..., None], hb, nb / d1[..., None])
            l = np.where(through, l, R.luminance(c))
            v = np.where(through, v, vnum / (d1 * d1))
            undecidable = marked
        out, fa, fb = c * A, ha * A, hb * A
        d = R.luminance(fa) - R.luminance(fb)
        e = ((d * d) * LD(0.25)) / (np.maximum(R.luminance(out), LD(0)) + ERR_FLOOR)
        e = np.where(np.isfinite(e), e, LD(0))
    return out, fa, fb, e, undecidable
