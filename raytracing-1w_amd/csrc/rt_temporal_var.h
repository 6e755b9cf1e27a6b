/* rt_temporal_var.h -- the variance of a temporal history (include/rt1w.h: rt1w_temporal_moments, rt1w_temporal_variance): next to the
 * history of rt_temporal.h a running mean of the squared demodulated luminance is kept, and the spread of a pixel's values from frame to
 * frame becomes the variance buffer rt1w_denoise_var takes (Schied et al. 2017, SVGF).  Compiled by the kernels (temporal_var.hip) and by
 * the CPU twin of the diagnostics library (denoise_host.cpp), from this one text.
 *
 * The moments pixel is rt_tm_pixel itself, called with the two m2 pointers.  What is here is the variance pixel.  The rules of
 * rt_temporal.h hold: + - * /, comparisons and selects in one fixed order, -ffp-contract=off, no libm, no intrinsic. */
#ifndef RT_TEMPORAL_VAR_H
#define RT_TEMPORAL_VAR_H

#include "rt_temporal.h"
#include "rt_denoise_var.h" /* rt_dv_tap_weight: the guide-only weight of the spatial estimate */

#define RT_TV_MIN_LEN 4.0 /* == RT1W_TEMPORAL_MIN_LEN: shorter histories take the spatial estimate */
#define RT_TV_RADIUS 3    /* of its window: 7 x 7 taps */

/* the guide weights' parameters: rt1w_denoise's defaults (normal power 32, sigma_depth 0.1).  false: w x h refused */
RT_HD bool rt_tv_make_params(uint32_t w, uint32_t h, RtDnParams& P) { return rt_dn_make_params(w, h, 0u, 0u, 0.0, 0.0, 0.0, P); }

/* var of pixel (x, y) of a P.w x P.h image: hist[h][w][3], m2[h][w], len[h][w] as rt1w_temporal_moments wrote them, aov the current frame's */
RT_HD double rt_tv_pixel(const RtDnParams& P, const double* hist, const double* m2, const double* len, const double* aov, uint32_t x, uint32_t y) {
    const unsigned long long i = (unsigned long long)y * P.w + x;
    RtDnCol cp;
    RtDnGuide g;
    rt_tm_prepare(1u, hist + i * 3u, aov + i * 8u, cp, g); /* the history is demodulated: taken as it is; cp.l is its luminance */
    const double l1 = cp.l, mp = m2[i], n = len[i];
    if (!rt_dn_finite(l1) || !rt_dn_finite(mp) || !rt_dn_finite(n) || !(n >= 1.0)) return 0.0; /* no usable estimate */
    double v;
    if (n >= RT_TV_MIN_LEN) { /* temporal: the spread of this pixel's own frames */
        const double d = mp - l1 * l1;
        v = (d > 0.0 ? d : 0.0) / (n - 1.0);
    } else { /* spatial: the spread of both moments over the taps the guides let in */
        const double gp[5] = {g.nx, g.ny, g.nz, g.z, g.v};
        const bool pz = gp[0] == 0.0 && gp[1] == 0.0 && gp[2] == 0.0;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        for (int dy = -RT_TV_RADIUS; dy <= RT_TV_RADIUS; ++dy) {
            const long long yy = (long long)y + dy;
            if (yy < 0 || yy >= (long long)P.h) continue;
            for (int dx = -RT_TV_RADIUS; dx <= RT_TV_RADIUS; ++dx) {
                const long long xx = (long long)x + dx;
                if (xx < 0 || xx >= (long long)P.w) continue;
                double w = 1.0, lq = l1, mq = mp;
                if (dx != 0 || dy != 0) {
                    const unsigned long long j = (unsigned long long)yy * P.w + (unsigned long long)xx;
                    RtDnCol cq;
                    RtDnGuide q;
                    rt_tm_prepare(1u, hist + j * 3u, aov + j * 8u, cq, q);
                    const double gq[5] = {q.nx, q.ny, q.nz, q.z, q.v};
                    w = rt_dv_tap_weight(P, 1.0, 1.0, gp, pz, 0.0, 0.0, gq, 0.0, 0.0);
                    lq = cq.l; mq = m2[j];
                }
                if (w > 0.0 && rt_dn_finite(lq) && rt_dn_finite(mq)) { s0 += w; s1 += w * lq; s2 += w * mq; }
            }
        }
        const double M1 = s1 / s0, M2 = s2 / s0;
        const double d = M2 - M1 * M1;
        v = (d > 0.0 ? d : 0.0) / n;
    }
    return (v >= 0.0 && rt_dn_finite(v)) ? v : 0.0;
}

#endif
