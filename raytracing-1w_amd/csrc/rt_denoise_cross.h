/* rt_denoise_cross.h -- the cross-filtered half buffers (include/rt1w.h: rt1w_denoise_cross): the two halves A and B of a frame, each
 * filtered by the a-trous filter of rt_denoise_var.h with the colour term taken from the OTHER half, so that no weight is computed from
 * the value it multiplies and no error of a weight is common to the two filtered halves; their mean is the filtered frame and their
 * squared difference the error that remains (Rousselle et al. 2012).  Compiled by the kernels (denoise_cross.hip) and by the CPU twin
 * of the diagnostics library (denoise_host.cpp), from this one text.
 *
 * The rules of rt_denoise.h hold: + - * /, rt_sqrt, comparisons, selects, integer conversions in one fixed order, -ffp-contract=off,
 * no libm, no intrinsic.  The weight is rt_denoise_var.h's rt_dv_tap_weight, called once with B's luminance and variance (the weight
 * that filters A) and once with A's; a half's additions are rt_dv_level_pixel's in its order, so with half_a == half_b each half's
 * (colour, luminance) is the bits of rt_dv_level_pixel on that buffer with the variance 2 v. */
#ifndef RT_DENOISE_CROSS_H
#define RT_DENOISE_CROSS_H

#include "rt_denoise_var.h"
#include "rt_adaptive.h"

/* what the levels read and write for a pixel: the demodulated half A, its luminance and the variance of that luminance, then B.  80 bytes */
struct RtDcCol { double ar, ag, ab, la, va, br, bg, bb, lb, vb; };

/* the prepare pass of one pixel: guides, A_p and v_p of rt_dv_prepare_pixel; the halves demodulated with A_p; va = vb = 2 v_p (a half of
 * equal count has twice the variance of the whole mean).  The frame gives no value, only its finiteness.  A weight never sees the value
 * it multiplies, so a value that is not finite has to be kept out here: where the luminance of frame / A_p, la or lb is not finite, the
 * first of the three that is not stands for la AND lb -- the pixel is passed through every level and taken by no other, in either half */
RT_HD void rt_dc_prepare_pixel(const RtDnParams& P, const double* frame, const double* aov, double var, const double* half_a, const double* half_b,
                               RtDcCol& c, RtDnGuide& g) {
    RtDvCol c5;
    rt_dv_prepare_pixel(P, frame, aov, var, c5, g);
    c.ar = P.keep_albedo ? half_a[0] : half_a[0] / g.ar;
    c.ag = P.keep_albedo ? half_a[1] : half_a[1] / g.ag;
    c.ab = P.keep_albedo ? half_a[2] : half_a[2] / g.ab;
    c.br = P.keep_albedo ? half_b[0] : half_b[0] / g.ar;
    c.bg = P.keep_albedo ? half_b[1] : half_b[1] / g.ag;
    c.bb = P.keep_albedo ? half_b[2] : half_b[2] / g.ab;
    const double la = rt_dn_lum(c.ar, c.ag, c.ab), lb = rt_dn_lum(c.br, c.bg, c.bb);
    const bool ok = rt_dn_finite(c5.l) && rt_dn_finite(la) && rt_dn_finite(lb);
    const double bad = !rt_dn_finite(c5.l) ? c5.l : (!rt_dn_finite(la) ? la : lb);
    c.la = ok ? la : bad;
    c.lb = ok ? lb : bad;
    c.va = 2.0 * c5.v;
    c.vb = c.va;
}

/* level `level` of pixel (x, y): rt_dv_level_pixel's taps and order, two weights per tap -- wa from (lb, vb), which filters A, and wb
 * from (la, va), which filters B -- and each half's sums over the taps its own weight takes (w > 0) */
template <class Src>
RT_HD RtDcCol rt_dc_level_pixel(const RtDnParams& P, double sv2, const Src& src, uint32_t x, uint32_t y, uint32_t level) {
    const RtDcCol cp = src.col(x, y);
    if (!rt_dn_finite(cp.la) || !rt_dn_finite(cp.lb)) return cp; /* a centre value that is not finite is passed through: the whole record */
    double gp[5];
    src.guide(x, y, gp);
    const bool pz = gp[0] == 0.0 && gp[1] == 0.0 && gp[2] == 0.0;
    const long long step = 1ll << level;
    double sar = 0.0, sag = 0.0, sab = 0.0, swa = 0.0, sva = 0.0;
    double sbr = 0.0, sbg = 0.0, sbb = 0.0, swb = 0.0, svb = 0.0;
    for (int dy = -2; dy <= 2; ++dy) {
        const long long yy = (long long)y + dy * step;
        if (yy < 0 || yy >= (long long)P.h) continue;
        for (int dx = -2; dx <= 2; ++dx) {
            const long long xx = (long long)x + dx * step;
            if (xx < 0 || xx >= (long long)P.w) continue;
            const double hw = rt_dn_b3(dy) * rt_dn_b3(dx);
            double wa = hw, wb = hw;
            RtDcCol cq = cp;
            if (dx != 0 || dy != 0) {
                cq = src.col((uint32_t)xx, (uint32_t)yy);
                double gq[5];
                src.guide((uint32_t)xx, (uint32_t)yy, gq);
                wa = rt_dv_tap_weight(P, sv2, hw, gp, pz, cp.lb, cp.vb, gq, cq.lb, cq.vb);
                wb = rt_dv_tap_weight(P, sv2, hw, gp, pz, cp.la, cp.va, gq, cq.la, cq.va);
            }
            if (wa > 0.0) { /* not for 0 and not for NaN: such a tap contributes nothing, whatever its value */
                sar += wa * cq.ar; sag += wa * cq.ag; sab += wa * cq.ab; swa += wa;
                sva += (wa * wa) * cq.va;
            }
            if (wb > 0.0) {
                sbr += wb * cq.br; sbg += wb * cq.bg; sbb += wb * cq.bb; swb += wb;
                svb += (wb * wb) * cq.vb;
            }
        }
    }
    RtDcCol o;
    o.ar = sar / swa; o.ag = sag / swa; o.ab = sab / swa;
    o.la = rt_dn_lum(o.ar, o.ag, o.ab);
    o.va = sva / (swa * swa);
    o.br = sbr / swb; o.bg = sbg / swb; o.bb = sbb / swb;
    o.lb = rt_dn_lum(o.br, o.bg, o.bb);
    o.vb = svb / (swb * swb);
    return o;
}

/* after the last level: out = ((a' + b') 0.5) A, the plain mean of the two filtered halves (equal counts: m_A == m_B), and the error of
 * rt_dh_finish_pixel: d = lum(a' A) - lum(b' A);  err = ((d d) 0.25) / (max(lum(out), 0) + 0.01), 0 where that is not finite */
RT_HD void rt_dc_finish_pixel(const RtDcCol& c, const RtDnGuide& g, double* out, double* err) {
    const double o0 = ((c.ar + c.br) * 0.5) * g.ar, o1 = ((c.ag + c.bg) * 0.5) * g.ag, o2 = ((c.ab + c.bb) * 0.5) * g.ab;
    out[0] = o0; out[1] = o1; out[2] = o2;
    const double d = rt_dn_lum(c.ar * g.ar, c.ag * g.ag, c.ab * g.ab) - rt_dn_lum(c.br * g.ar, c.bg * g.ag, c.bb * g.ab);
    const double lo = rt_dn_lum(o0, o1, o2);
    const double e = ((d * d) * 0.25) / ((lo > 0.0 ? lo : 0.0) + RT_AD_ERR_FLOOR);
    *err = rt_dn_finite(e) ? e : 0.0;
}

/* the filter as the skeletons see it (rt_denoise.h: RtDnFilter) */
struct RtDcFilter {
    typedef RtDcCol Col;
    static RT_HD void prepare(const RtDnParams& P, unsigned long long i, Col& c, RtDnGuide& g, const double* frame, const double* aov, const double* var,
                              const double* half_a, const double* half_b) {
        rt_dc_prepare_pixel(P, frame + i * 3u, aov + i * 8u, var[i], half_a + i * 3u, half_b + i * 3u, c, g);
    }
    template <class Src>
    static RT_HD Col level(const RtDnParams& P, double sv2, const Src& src, uint32_t x, uint32_t y, uint32_t level) { return rt_dc_level_pixel(P, sv2, src, x, y, level); }
    static RT_HD void finish(const Col& c, const RtDnGuide& g, unsigned long long i, double* out, double* err_px) { rt_dc_finish_pixel(c, g, out + i * 3u, err_px + i); }
};

#endif
