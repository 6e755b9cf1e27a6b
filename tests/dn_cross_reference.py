"""An independent statement of rt1w_denoise_cross, written from the prose of include/rt1w.h (the comment block "cross-filtered half
buffers") in numpy longdouble, beside tests/dn_reference.py, whose prepare pass, falloff, tap walk and constants it takes: no library is
loaded, nothing of csrc/rt_denoise_cross.h is shared.  The falloff is np.exp and the normal weight `**`.

tests/test_denoise_cross.py holds the CPU twin to this, within 1e-12 where the quantity is well conditioned."""
import numpy as np

import dn_reference as R

LD = R.LD
ERR_FLOOR = LD(0.01)


def denoise_cross(frame, aov, var, half_a, half_b, sigma_variance=0.0, iterations=0, keep_albedo=False, sigma_normal=0.0, sigma_depth=0.0):
    """rt1w_denoise_cross: (out, a', b', err_px, undecidable), longdouble; a', b' are the two filtered halves with the albedo back.
    `undecidable` as tests/dn_reference.py defines it, here for either of the two colour terms."""
    levels = R.DEFAULT_LEVELS if iterations == 0 else int(iterations)
    power = R.normal_power(sigma_normal)
    s_depth = LD(R.SIGMA_DEPTH if sigma_depth == 0 else sigma_depth)
    s_var = LD(R.SIGMA_VARIANCE if sigma_variance == 0 else sigma_variance)
    A, cf, lf, u, z, cov = R.prepare(frame, aov, keep_albedo)
    h, w = lf.shape
    var = np.asarray(var, dtype=np.float64)
    v0 = np.where(np.isfinite(var) & (var >= 0), var, 0.0).astype(LD)
    with np.errstate(all="ignore"):
        col = [np.asarray(x, dtype=np.float64).astype(LD) / A for x in (half_a, half_b)]
        # the frame gives no value, only its finiteness: the first of (frame's luminance, la, lb) that is not finite stands for la and lb
        la, lb = R.luminance(col[0]), R.luminance(col[1])
        bad = np.where(~np.isfinite(lf), lf, np.where(~np.isfinite(la), la, lb))
        ok = np.isfinite(lf) & np.isfinite(la) & np.isfinite(lb)
        lum = [np.where(ok, la, bad), np.where(ok, lb, bad)]
        vv = [LD(2) * v0, LD(2) * v0]
        undecidable = np.zeros((h, w), dtype=bool)
        for i in range(levels):
            num = [np.zeros((h, w, 3), dtype=LD) for _ in range(2)]
            den = [np.zeros((h, w), dtype=LD) for _ in range(2)]
            vnum = [np.zeros((h, w), dtype=LD) for _ in range(2)]
            marked = undecidable.copy()
            for dy, dx, p, q in R._taps(h, w, 2 ** i):
                hw = R.B3[abs(dx)] * R.B3[abs(dy)]
                centre = dx == 0 and dy == 0
                if not centre:
                    up, uq = u[p], u[q]
                    both_zero = np.all(up == 0, axis=-1) & np.all(uq == 0, axis=-1)
                    wn = np.where(both_zero, LD(1), np.clip((up * uq).sum(axis=-1), LD(0), LD(1)) ** power)
                    zp, zq = z[p], z[q]
                    one_inf = np.isposinf(zp) != np.isposinf(zq)
                    x_depth = np.where(zp == zq, LD(0), np.where(one_inf, LD(np.inf), np.abs(zp - zq) / (np.maximum(zp, zq) * s_depth)))
                    dv = cov[p] - cov[q]
                    x_coverage = (dv * dv) * R.INV_SIGMA_COVERAGE2
                    marked[p] |= undecidable[q]
                for k in (0, 1):                                   # half k is filtered with the colour term of the OTHER half
                    o = 1 - k
                    if centre:
                        wt = np.full((h, w), hw)
                    else:
                        lp, lq = lum[o][p], lum[o][q]
                        vsum = vv[o][p] + vv[o][q]
                        x_colour = np.where(lp == lq, LD(0), (lp - lq) ** 2 / (s_var * s_var * vsum))
                        knife = (vsum == 0) & (lp != lq) & (np.abs(lp - lq) <= R.NEAR * np.maximum(np.abs(lp), np.abs(lq)))
                        knife &= np.isfinite(lp) & np.isfinite(lq)
                        knife &= (hw * wn) * R.falloff(x_depth + x_coverage) > 0
                        marked[p] |= knife
                        wt = (hw * wn) * R.falloff((x_depth + x_colour) + x_coverage)
                    take = wt > 0
                    wt = np.where(take, wt, LD(0))
                    num[k][p] += wt[..., None] * np.where(take[..., None], col[k][q], LD(0))
                    den[k][p] += wt
                    vnum[k][p] += wt * wt * np.where(take, vv[k][q], LD(0))
            through = ~(np.isfinite(lum[0]) & np.isfinite(lum[1]))   # the whole record passes through unchanged
            for k in (0, 1):
                d1 = np.where(through, LD(1), den[k])
                col[k] = np.where(through[..., None], col[k], num[k] / d1[..., None])
                lum[k] = np.where(through, lum[k], R.luminance(col[k]))
                vv[k] = np.where(through, vv[k], vnum[k] / (d1 * d1))
            undecidable = marked
        out = ((col[0] + col[1]) * LD(0.5)) * A
        fa, fb = col[0] * A, col[1] * A
        d = R.luminance(fa) - R.luminance(fb)
        e = ((d * d) * LD(0.25)) / (np.maximum(R.luminance(out), LD(0)) + ERR_FLOOR)
        e = np.where(np.isfinite(e), e, LD(0))
    return out, fa, fb, e, undecidable
