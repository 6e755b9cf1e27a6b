/* rt_denoise_var.h -- the variance-guided form of the feature-guided denoiser (include/rt1w.h: rt1w_batch_variance, rt1w_denoise_var):
 * the variance of the mean of K sample batches, and the a-trous filter of rt_denoise.h with a colour term scaled by that variance, which
 * it propagates from level to level (Dammertz et al. 2010 with the variance guidance of Schied et al. 2017, SVGF).  Compiled by the
 * kernels (denoise_var.hip) and by the CPU twin of the diagnostics library (denoise_host.cpp), from this one text.
 *
 * The rules of rt_denoise.h hold: + - * /, rt_sqrt, comparisons, selects, integer conversions in one fixed order, -ffp-contract=off,
 * no libm, no intrinsic.  rt_dn_falloff, rt_dn_powi, rt_dn_b3, the guide record and the prepare pass are that header's. */
#ifndef RT_DENOISE_VAR_H
#define RT_DENOISE_VAR_H

#include "rt_denoise.h"

#define RT_DV_MIN_BATCHES 2u
#define RT_DV_MAX_BATCHES 16u
/* the defaults, chosen with the CPU twin on the three scenes of tests/test_denoise_var.py */
#define RT_DV_DEFAULT_BATCHES 4u
#define RT_DV_SIGMA_VARIANCE 3.0

/* what the levels read and write for a pixel: the (demodulated) colour, its luminance and the variance of that luminance */
struct RtDvCol { double r, g, b, l, v; };

/* K batches of n samples each: K = 2 .. 16, n >= 1, K n a sample count (false: RT1W_ERR_INVALID) */
RT_HD bool rt_dv_batches_ok(uint32_t batches, uint32_t batch_spp) {
    return batches >= RT_DV_MIN_BATCHES && batches <= RT_DV_MAX_BATCHES && batch_spp >= 1u &&
           (unsigned long long)batches * batch_spp <= 0xFFFFFFFFull;
}
/* sigma_variance with the default filled in; false: negative or not finite (RT1W_ERR_INVALID) */
RT_HD bool rt_dv_sigma(double sigma_variance, double& sv) {
    if (!(sigma_variance >= 0.0) || !rt_dn_finite(sigma_variance)) return false;
    sv = sigma_variance == 0.0 ? RT_DV_SIGMA_VARIANCE : sigma_variance;
    return true;
}
/* how rt1w_render_denoised_var splits `spp` samples: batches 0 = the default; false where the count is out of range or does not divide spp */
RT_HD bool rt_dv_split(uint32_t spp, uint32_t batches, uint32_t& k, uint32_t& n) {
    k = batches ? batches : RT_DV_DEFAULT_BATCHES;
    if (k < RT_DV_MIN_BATCHES || k > RT_DV_MAX_BATCHES || spp == 0u || spp % k != 0u) return false;
    n = spp / k;
    return rt_dv_batches_ok(k, n);
}

/* one pixel of rt1w_batch_variance.  s: the pixel's three sums in batch 0, `stride` doubles from one batch to the next; aov: its 8
 * channels.  frame[3]: Color::into_sampled (rt_into_sampled: NaN of the sum to 0, times 1 / spp) of the batch sums added in batch order;
 * *var: the variance of the mean of the batches' demodulated luminances, 0 where that is negative or not finite.  The luminances are
 * computed twice (mean, then deviations) rather than kept: K is a run-time count, and an indexed array would live in scratch. */
RT_HD void rt_dv_variance_pixel(uint32_t batches, uint32_t batch_spp, bool keep_albedo, const double* s, unsigned long long stride,
                                const double* aov, double* frame, double* var) {
    const double a0 = aov[0], a1 = aov[1], a2 = aov[2];
    const double ar = keep_albedo ? 1.0 : ((a0 > RT_DN_EPS && rt_dn_finite(a0)) ? a0 : RT_DN_EPS);
    const double ag = keep_albedo ? 1.0 : ((a1 > RT_DN_EPS && rt_dn_finite(a1)) ? a1 : RT_DN_EPS);
    const double ab = keep_albedo ? 1.0 : ((a2 > RT_DN_EPS && rt_dn_finite(a2)) ? a2 : RT_DN_EPS);
    const double inv_n = 1.0 / (double)batch_spp;
    double tr = s[0], tg = s[1], tb = s[2];
    double lsum = 0.0;
    for (uint32_t k = 0; k < batches; ++k) {
        const double* q = s + k * stride;
        if (k) { tr = tr + q[0]; tg = tg + q[1]; tb = tb + q[2]; }
        const double mr = q[0] * inv_n, mg = q[1] * inv_n, mb = q[2] * inv_n;
        lsum = lsum + rt_dn_lum(keep_albedo ? mr : mr / ar, keep_albedo ? mg : mg / ag, keep_albedo ? mb : mb / ab);
    }
    const double scale = 1.0 / (double)(batches * batch_spp);
    frame[0] = (tr != tr ? 0.0 : tr) * scale;
    frame[1] = (tg != tg ? 0.0 : tg) * scale;
    frame[2] = (tb != tb ? 0.0 : tb) * scale;
    const double lbar = lsum / (double)batches;
    double dsum = 0.0;
    for (uint32_t k = 0; k < batches; ++k) {
        const double* q = s + k * stride;
        const double mr = q[0] * inv_n, mg = q[1] * inv_n, mb = q[2] * inv_n;
        const double d = rt_dn_lum(keep_albedo ? mr : mr / ar, keep_albedo ? mg : mg / ag, keep_albedo ? mb : mb / ab) - lbar;
        dsum = dsum + d * d;
    }
    const double v = dsum / (double)(batches * (batches - 1u));
    *var = (v >= 0.0 && rt_dn_finite(v)) ? v : 0.0;
}

/* the prepare pass of one pixel: rt_dn_prepare_pixel, and the variance as given -- 0 where it is negative or not finite (no estimate) */
RT_HD void rt_dv_prepare_pixel(const RtDnParams& P, const double* frame, const double* aov, double var, RtDvCol& c, RtDnGuide& g) {
    RtDnCol c4;
    rt_dn_prepare_pixel(P, frame, aov, c4, g);
    c.r = c4.r; c.g = c4.g; c.b = c4.b; c.l = c4.l;
    c.v = (var >= 0.0 && rt_dn_finite(var)) ? var : 0.0;
}

/* the weight of a tap q that is not the centre p: rt_dn_level_pixel's but for the colour term -- x_colour = 0 where l_p == l_q, else
 * (l_p - l_q)^2 / (sigma_variance^2 (v_p + v_q)), +inf where both variances are 0.  hw = h(dx, dy); gp, gq: the two guides; pz: u_p is
 * (0, 0, 0); sv2 = sigma_variance^2.  Shared by the level below and the level of rt_denoise_halves.h: one text for the weight. */
RT_HD double rt_dv_tap_weight(const RtDnParams& P, double sv2, double hw, const double gp[5], bool pz, double lp, double vp, const double gq[5],
                              double lq, double vq) {
    const bool qz = gq[0] == 0.0 && gq[1] == 0.0 && gq[2] == 0.0;
    double cosv = (gp[0] * gq[0] + gp[1] * gq[1]) + gp[2] * gq[2];
    cosv = cosv > 0.0 ? (cosv < 1.0 ? cosv : 1.0) : 0.0; /* NaN: 0 */
    const double wn = (pz && qz) ? 1.0 : rt_dn_powi(cosv, P.normal_power);
    const bool pinf = gp[3] == RT_INF, qinf = gq[3] == RT_INF;
    const double zmax = gp[3] > gq[3] ? gp[3] : gq[3];
    const double xd = (gp[3] == gq[3]) ? 0.0 : ((pinf || qinf) ? RT_INF : rt_abs(gp[3] - gq[3]) / (zmax * P.sigma_depth));
    const double dl = lp - lq;
    const double xc = (lp == lq) ? 0.0 : (dl * dl) / (sv2 * (vp + vq)); /* x / 0 = +inf: a converged pixel keeps its value */
    const double dv = gp[4] - gq[4];
    const double xv = (dv * dv) * RT_DN_INV_SIGMA_COV2;
    return (hw * wn) * rt_dn_falloff((xd + xc) + xv);
}

/* level `level` (step 2^level) of pixel (x, y): rt_dn_level_pixel but for the colour term, which every level has (rt_dv_tap_weight), and
 * for the variance it hands on: v' = sum w^2 v_q / (sum w)^2 over the taps the colour takes, in their order.  sv2 = sigma_variance^2. */
template <class Src>
RT_HD RtDvCol rt_dv_level_pixel(const RtDnParams& P, double sv2, const Src& src, uint32_t x, uint32_t y, uint32_t level) {
    const RtDvCol cp = src.col(x, y);
    if (!rt_dn_finite(cp.l)) return cp; /* a centre value that is not finite is passed through */
    double gp[5];
    src.guide(x, y, gp);
    const bool pz = gp[0] == 0.0 && gp[1] == 0.0 && gp[2] == 0.0;
    const long long step = 1ll << level;
    double sr = 0.0, sg = 0.0, sb = 0.0, sw = 0.0, svar = 0.0;
    for (int dy = -2; dy <= 2; ++dy) {
        const long long yy = (long long)y + dy * step;
        if (yy < 0 || yy >= (long long)P.h) continue;
        for (int dx = -2; dx <= 2; ++dx) {
            const long long xx = (long long)x + dx * step;
            if (xx < 0 || xx >= (long long)P.w) continue;
            const double hw = rt_dn_b3(dy) * rt_dn_b3(dx);
            double w = hw;
            RtDvCol cq = cp;
            if (dx != 0 || dy != 0) {
                cq = src.col((uint32_t)xx, (uint32_t)yy);
                double gq[5];
                src.guide((uint32_t)xx, (uint32_t)yy, gq);
                w = rt_dv_tap_weight(P, sv2, hw, gp, pz, cp.l, cp.v, gq, cq.l, cq.v);
            }
            if (w > 0.0) { /* not for 0 and not for NaN: such a tap contributes nothing, whatever its value */
                sr += w * cq.r; sg += w * cq.g; sb += w * cq.b; sw += w;
                svar += (w * w) * cq.v;
            }
        }
    }
    RtDvCol o;
    o.r = sr / sw; o.g = sg / sw; o.b = sb / sw;
    o.l = rt_dn_lum(o.r, o.g, o.b);
    o.v = svar / (sw * sw);
    return o;
}

/* after the last level: the albedo back (times 1 with RT_DN_KEEP_ALBEDO) */
RT_HD void rt_dv_finish_pixel(const RtDvCol& c, const RtDnGuide& g, double* out) {
    out[0] = c.r * g.ar; out[1] = c.g * g.ag; out[2] = c.b * g.ab;
}

/* the filter as the skeletons see it (rt_denoise.h: RtDnFilter) */
struct RtDvFilter {
    typedef RtDvCol Col;
    static RT_HD void prepare(const RtDnParams& P, unsigned long long i, Col& c, RtDnGuide& g, const double* frame, const double* aov, const double* var) {
        rt_dv_prepare_pixel(P, frame + i * 3u, aov + i * 8u, var[i], c, g);
    }
    template <class Src>
    static RT_HD Col level(const RtDnParams& P, double sv2, const Src& src, uint32_t x, uint32_t y, uint32_t level) { return rt_dv_level_pixel(P, sv2, src, x, y, level); }
    static RT_HD void finish(const Col& c, const RtDnGuide& g, unsigned long long i, double* out, double*) { rt_dv_finish_pixel(c, g, out + i * 3u); }
};

#endif
