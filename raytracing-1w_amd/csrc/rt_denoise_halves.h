/* rt_denoise_halves.h -- the half-buffer error estimate of the variance-guided denoiser (include/rt1w.h: rt1w_halves_resolve,
 * rt1w_denoise_var_halves, rt1w_tile_error_map): a frame whose samples are kept in two independent halves A and B, the filter of
 * rt_denoise_var.h carrying both halves through the weights it computes for the whole frame, and the squared difference of the two
 * filtered halves as the error that remains after filtering (Rousselle et al. 2012).  Compiled by the kernels (denoise_halves.hip,
 * adaptive.hip) and by the CPU twins of the diagnostics library (denoise_host.cpp, adaptive_host.cpp), from this one text.
 *
 * The rules of rt_denoise.h hold: + - * /, rt_sqrt, comparisons, selects, integer conversions in one fixed order, -ffp-contract=off,
 * no libm, no intrinsic.  The weight is rt_denoise_var.h's rt_dv_tap_weight and the colour's additions are rt_dv_level_pixel's in its
 * order, so the colour, luminance and variance of a level here are the bits of rt_dv_level_pixel: the halves never enter a weight. */
#ifndef RT_DENOISE_HALVES_H
#define RT_DENOISE_HALVES_H

#include "rt_denoise_var.h"
#include "rt_adaptive.h"

/* what the levels read and write for a pixel: RtDvCol, then the two demodulated halves.  88 bytes */
struct RtDhCol { double r, g, b, l, v, ar, ag, ab, br, bg, bb; };

/* one pixel of rt1w_halves_resolve.  a, b: the pixel's records in the two accumulators (rt_adaptive.h), merged with the same batch_spp */
RT_HD void rt_dh_resolve_pixel(uint32_t batch_spp, const double* a, const double* b, double* frame, double* var, double* half_a, double* half_b,
                               double* spp) {
    double va, vb, sa, sb;
    rt_ad_resolve_pixel(batch_spp, a, half_a, &va, &sa); /* rt1w_resolve's rule on S_x with count m_x n; (0, 0, 0) where m_x = 0 */
    rt_ad_resolve_pixel(batch_spp, b, half_b, &vb, &sb);
    const double ma = a[3], mb = b[3];
    const double m = ma + mb;
    const double count = m * (double)batch_spp;
    if (m >= 1.0) {
        const double tr = a[0] + b[0], tg = a[1] + b[1], tb = a[2] + b[2];
        const double scale = 1.0 / count;
        frame[0] = (tr != tr ? 0.0 : tr) * scale;
        frame[1] = (tg != tg ? 0.0 : tg) * scale;
        frame[2] = (tb != tb ? 0.0 : tb) * scale;
    } else { /* an empty pixel */
        frame[0] = 0.0; frame[1] = 0.0; frame[2] = 0.0;
    }
    /* the two Welford states of the demodulated luminance as one (Chan et al.'s pairwise update), in this order */
    double v = 0.0;
    if (m >= 2.0 && a[5] >= 0.0 && b[5] >= 0.0) {
        const double delta = b[4] - a[4];
        const double m2 = (a[5] + b[5]) + ((delta * delta) * (ma * mb)) / m;
        v = m2 / (m * (m - 1.0));
        v = (v >= 0.0 && rt_dn_finite(v)) ? v : 0.0;
    }
    *var = v;
    *spp = m >= 1.0 ? count : 0.0;
}

/* the prepare pass of one pixel: rt_dv_prepare_pixel, and the two halves demodulated with the same albedo A_p */
RT_HD void rt_dh_prepare_pixel(const RtDnParams& P, const double* frame, const double* aov, double var, const double* half_a, const double* half_b,
                               RtDhCol& c, RtDnGuide& g) {
    RtDvCol c5;
    rt_dv_prepare_pixel(P, frame, aov, var, c5, g);
    c.r = c5.r; c.g = c5.g; c.b = c5.b; c.l = c5.l; c.v = c5.v;
    c.ar = P.keep_albedo ? half_a[0] : half_a[0] / g.ar;
    c.ag = P.keep_albedo ? half_a[1] : half_a[1] / g.ag;
    c.ab = P.keep_albedo ? half_a[2] : half_a[2] / g.ab;
    c.br = P.keep_albedo ? half_b[0] : half_b[0] / g.ar;
    c.bg = P.keep_albedo ? half_b[1] : half_b[1] / g.ag;
    c.bb = P.keep_albedo ? half_b[2] : half_b[2] / g.ab;
}

/* level `level` of pixel (x, y): rt_dv_level_pixel -- the same weight, the same taps, the same additions for r, g, b, l, v -- and
 * a' = sum w a_q / sum w, b' likewise, over exactly the taps the colour takes, in the colour's order */
template <class Src>
RT_HD RtDhCol rt_dh_level_pixel(const RtDnParams& P, double sv2, const Src& src, uint32_t x, uint32_t y, uint32_t level) {
    const RtDhCol cp = src.col(x, y);
    if (!rt_dn_finite(cp.l)) return cp; /* a centre value that is not finite is passed through: all three values */
    double gp[5];
    src.guide(x, y, gp);
    const bool pz = gp[0] == 0.0 && gp[1] == 0.0 && gp[2] == 0.0;
    const long long step = 1ll << level;
    double sr = 0.0, sg = 0.0, sb = 0.0, sw = 0.0, svar = 0.0;
    double sar = 0.0, sag = 0.0, sab = 0.0, sbr = 0.0, sbg = 0.0, sbb = 0.0;
    for (int dy = -2; dy <= 2; ++dy) {
        const long long yy = (long long)y + dy * step;
        if (yy < 0 || yy >= (long long)P.h) continue;
        for (int dx = -2; dx <= 2; ++dx) {
            const long long xx = (long long)x + dx * step;
            if (xx < 0 || xx >= (long long)P.w) continue;
            const double hw = rt_dn_b3(dy) * rt_dn_b3(dx);
            double w = hw;
            RtDhCol cq = cp;
            if (dx != 0 || dy != 0) {
                cq = src.col((uint32_t)xx, (uint32_t)yy);
                double gq[5];
                src.guide((uint32_t)xx, (uint32_t)yy, gq);
                w = rt_dv_tap_weight(P, sv2, hw, gp, pz, cp.l, cp.v, gq, cq.l, cq.v);
            }
            if (w > 0.0) { /* not for 0 and not for NaN: such a tap contributes nothing, whatever its value */
                sr += w * cq.r; sg += w * cq.g; sb += w * cq.b; sw += w;
                svar += (w * w) * cq.v;
                sar += w * cq.ar; sag += w * cq.ag; sab += w * cq.ab;
                sbr += w * cq.br; sbg += w * cq.bg; sbb += w * cq.bb;
            }
        }
    }
    RtDhCol o;
    o.r = sr / sw; o.g = sg / sw; o.b = sb / sw;
    o.l = rt_dn_lum(o.r, o.g, o.b);
    o.v = svar / (sw * sw);
    o.ar = sar / sw; o.ag = sag / sw; o.ab = sab / sw;
    o.br = sbr / sw; o.bg = sbg / sw; o.bb = sbb / sw;
    return o;
}

/* after the last level: the albedo back on all three, out as rt_dv_finish_pixel, and the error of the filtered pixel:
 * d = lum(a' A) - lum(b' A);  err = ((d d) 0.25) / (max(lum(out), 0) + 0.01), 0 where that is not finite.  1/4: Var((A + B) / 2) =
 * Var(A - B) / 4 for two independent halves of equal count; the denominator is rt_ad_pixel_error's */
RT_HD void rt_dh_finish_pixel(const RtDhCol& c, const RtDnGuide& g, double* out, double* err) {
    const double o0 = c.r * g.ar, o1 = c.g * g.ag, o2 = c.b * g.ab;
    out[0] = o0; out[1] = o1; out[2] = o2;
    const double d = rt_dn_lum(c.ar * g.ar, c.ag * g.ag, c.ab * g.ab) - rt_dn_lum(c.br * g.ar, c.bg * g.ag, c.bb * g.ab);
    const double lo = rt_dn_lum(o0, o1, o2);
    const double e = ((d * d) * 0.25) / ((lo > 0.0 ? lo : 0.0) + RT_AD_ERR_FLOOR);
    *err = rt_dn_finite(e) ? e : 0.0;
}

/* a value of rt1w_tile_error_map's per-pixel map as the tile sum takes it: negative or not finite counts as 0 */
RT_HD double rt_dh_map_value(double e) { return (e >= 0.0 && rt_dn_finite(e)) ? e : 0.0; }

/* the filter as the skeletons see it (rt_denoise.h: RtDnFilter) */
struct RtDhFilter {
    typedef RtDhCol Col;
    static RT_HD void prepare(const RtDnParams& P, unsigned long long i, Col& c, RtDnGuide& g, const double* frame, const double* aov, const double* var,
                              const double* half_a, const double* half_b) {
        rt_dh_prepare_pixel(P, frame + i * 3u, aov + i * 8u, var[i], half_a + i * 3u, half_b + i * 3u, c, g);
    }
    template <class Src>
    static RT_HD Col level(const RtDnParams& P, double sv2, const Src& src, uint32_t x, uint32_t y, uint32_t level) { return rt_dh_level_pixel(P, sv2, src, x, y, level); }
    static RT_HD void finish(const Col& c, const RtDnGuide& g, unsigned long long i, double* out, double* err_px) { rt_dh_finish_pixel(c, g, out + i * 3u, err_px + i); }
};

#endif
