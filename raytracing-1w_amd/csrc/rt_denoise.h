/* rt_denoise.h -- the feature-guided denoiser of rt1w_denoise (include/rt1w.h has the definitions): an edge-avoiding a-trous wavelet
 * filter (Dammertz, Sewtz, Hanika, Lensch 2010) over a frame and its first-hit feature buffers.  Compiled by the filter kernels
 * (denoise.hip) and by the CPU twin of the diagnostics library (denoise_host.cpp), from this one text.
 *
 * Everything is + - * /, rt_sqrt, comparisons, selects, integer <-> double conversions and integer bit operations in one fixed
 * order (built with -ffp-contract=off like every build of the core): the two builds give the same bits.  No libm, no intrinsic.
 * Nothing here is reached by the render kernels or by the run-time compiler. */
#ifndef RT_DENOISE_H
#define RT_DENOISE_H

#include "rt1w_num.h"

#define RT_DN_MAX_LEVELS 8u
#define RT_DN_DEFAULT_LEVELS 5u
#define RT_DN_KEEP_ALBEDO 1u /* == RT1W_DENOISE_KEEP_ALBEDO */
/* the defaults, chosen with the CPU twin on the three scenes of tests/test_denoise.py */
#define RT_DN_SIGMA_COLOUR 1.0
#define RT_DN_SIGMA_NORMAL 32.0 /* the exponent of the clamped cosine */
#define RT_DN_SIGMA_DEPTH 0.1
#define RT_DN_EPS 0.01          /* floor of the albedo a frame is divided by */
#define RT_DN_INV_SIGMA_COV2 16.0 /* 1 / sigma_coverage^2, sigma_coverage = 1/4: not a parameter */
#define RT_DN_CUTOFF 40.0       /* k(x) = 0 for x >= 40 (exp(-40) = 4.2e-18 would be the value) */
#define RT_DN_MAX_POWER 4096u

/* a call's parameters with the defaults filled in */
struct RtDnParams {
    uint32_t w, h, levels, keep_albedo, normal_power, pad;
    double sigma_colour, sigma_depth, eps;
};

/* what the levels read and write for a pixel: the (demodulated) colour and its luminance */
struct RtDnCol { double r, g, b, l; };
/* the guide record of a pixel: unit normal (0 where the mean normal is 0, not finite, or too short to square), depth, coverage, and
 * the albedo the result is multiplied by after the last level (1 with RT_DN_KEEP_ALBEDO) */
struct RtDnGuide { double nx, ny, nz, z, v, ar, ag, ab; };

RT_HD bool rt_dn_finite(double x) { return (rt_d2u(x) & 0x7FF0000000000000ull) != 0x7FF0000000000000ull; }
RT_HD double rt_dn_lum(double r, double g, double b) { return (0.2126 * r + 0.7152 * g) + 0.0722 * b; }

/* false: the parameters are refused (RT1W_ERR_INVALID) */
RT_HD bool rt_dn_make_params(uint32_t w, uint32_t h, uint32_t iterations, uint32_t flags, double sigma_colour, double sigma_normal,
                             double sigma_depth, RtDnParams& P) {
    if (w == 0u || h == 0u || w > 0x40000000u || h > 0x40000000u || iterations > RT_DN_MAX_LEVELS || (flags & ~RT_DN_KEEP_ALBEDO) != 0u) return false;
    if (!(sigma_colour >= 0.0) || !(sigma_normal >= 0.0) || !(sigma_depth >= 0.0)) return false;
    if (!rt_dn_finite(sigma_colour) || !rt_dn_finite(sigma_normal) || !rt_dn_finite(sigma_depth)) return false;
    if ((((unsigned long long)w + 15u) >> 4) * (((unsigned long long)h + 15u) >> 4) > 0x7FFFFFFFull) return false;
    P.w = w; P.h = h;
    P.levels = iterations ? iterations : RT_DN_DEFAULT_LEVELS;
    P.keep_albedo = flags & RT_DN_KEEP_ALBEDO;
    const double sn = sigma_normal == 0.0 ? RT_DN_SIGMA_NORMAL : sigma_normal;
    P.normal_power = sn < 1.0 ? 1u : (sn > (double)RT_DN_MAX_POWER ? RT_DN_MAX_POWER : (uint32_t)sn);
    P.pad = 0u;
    P.sigma_colour = sigma_colour == 0.0 ? RT_DN_SIGMA_COLOUR : sigma_colour;
    P.sigma_depth = sigma_depth == 0.0 ? RT_DN_SIGMA_DEPTH : sigma_depth;
    P.eps = RT_DN_EPS;
    return true;
}

/* the falloff k(x): 1 for x <= 0, exp(-x) for 0 < x < 40, exactly 0 for x >= 40, +inf and NaN.
 * exp(-x) = 2^-n * exp(r), n = trunc(x / ln 2 + 1/2), r = n ln 2 - x in [-0.35, 0.35] (ln 2 in two parts, as rt_log has it);
 * exp(r) by its Taylor polynomial of degree 13 in Horner form (truncation < 5e-18); 2^-n built from its exponent bits (n <= 58) */
RT_HD double rt_dn_falloff(double x) {
    if (!(x < RT_DN_CUTOFF)) return 0.0;
    if (!(x > 0.0)) return 1.0;
    const double INV_LN2 = 1.44269504088896338700e+00, LN2_HI = 6.93147180369123816490e-01, LN2_LO = 1.90821492927058770002e-10;
    const int n = (int)(x * INV_LN2 + 0.5);
    const double dn = (double)n;
    const double r = (dn * LN2_HI - x) + dn * LN2_LO;
    double p = 1.0 / 6227020800.0;
    p = p * r + 1.0 / 479001600.0;
    p = p * r + 1.0 / 39916800.0;
    p = p * r + 1.0 / 3628800.0;
    p = p * r + 1.0 / 362880.0;
    p = p * r + 1.0 / 40320.0;
    p = p * r + 1.0 / 5040.0;
    p = p * r + 1.0 / 720.0;
    p = p * r + 1.0 / 120.0;
    p = p * r + 1.0 / 24.0;
    p = p * r + 1.0 / 6.0;
    p = p * r + 0.5;
    p = p * r + 1.0;
    p = p * r + 1.0;
    return p * rt_u2d((uint64_t)(1023 - n) << 52);
}

/* c^e for an integer e >= 1 by binary exponentiation, lowest bit first */
RT_HD double rt_dn_powi(double c, uint32_t e) {
    double r = 1.0, b = c;
    while (e) {
        if (e & 1u) r = r * b;
        b = b * b;
        e >>= 1;
    }
    return r;
}

/* the prepare pass of one pixel: frame[3] and aov[8] (the layouts of rt1w_render and rt1w_render_aov) to colour and guide record */
RT_HD void rt_dn_prepare_pixel(const RtDnParams& P, const double* frame, const double* aov, RtDnCol& c, RtDnGuide& g) {
    const double nx = aov[3], ny = aov[4], nz = aov[5];
    const double m2 = (nx * nx + ny * ny) + nz * nz;
    const double inv = (m2 > 0.0) ? 1.0 / rt_sqrt(m2) : 0.0; /* m2 = +inf gives 0, NaN gives 0 */
    const bool unit = inv > 0.0 && rt_dn_finite(inv);
    g.nx = unit ? nx * inv : 0.0; g.ny = unit ? ny * inv : 0.0; g.nz = unit ? nz * inv : 0.0;
    g.z = aov[6]; g.v = aov[7];
    const double a0 = aov[0], a1 = aov[1], a2 = aov[2];
    g.ar = P.keep_albedo ? 1.0 : ((a0 > P.eps && rt_dn_finite(a0)) ? a0 : P.eps);
    g.ag = P.keep_albedo ? 1.0 : ((a1 > P.eps && rt_dn_finite(a1)) ? a1 : P.eps);
    g.ab = P.keep_albedo ? 1.0 : ((a2 > P.eps && rt_dn_finite(a2)) ? a2 : P.eps);
    c.r = P.keep_albedo ? frame[0] : frame[0] / g.ar;
    c.g = P.keep_albedo ? frame[1] : frame[1] / g.ag;
    c.b = P.keep_albedo ? frame[2] : frame[2] / g.ab;
    c.l = rt_dn_lum(c.r, c.g, c.b);
}

/* the B3-spline tap weights h(dy, dx) = k1(|dy|) * k1(|dx|), k1 = 3/8, 1/4, 1/16: all products are exact */
RT_HD double rt_dn_b3(int d) { return d == 0 ? 0.375 : ((d == 1 || d == -1) ? 0.25 : 0.0625); }

/* images as a level reads them: plain arrays in memory (the twin, and the kernel's direct form), for the colour record of any of the
 * four filters (this one, rt_denoise_var.h, rt_denoise_halves.h, rt_denoise_cross.h) */
template <class Col>
struct RtDnGlobalSrc {
    const Col* c;
    const RtDnGuide* g;
    uint32_t w;
    RT_HD Col col(uint32_t x, uint32_t y) const { return c[(unsigned long long)y * w + x]; }
    RT_HD void guide(uint32_t x, uint32_t y, double o[5]) const {
        const RtDnGuide* q = g + ((unsigned long long)y * w + x);
        o[0] = q->nx; o[1] = q->ny; o[2] = q->nz; o[3] = q->z; o[4] = q->v;
    }
};

/* level `level` (step 2^level) of pixel (x, y): the weighted mean of the 5 x 5 taps inside the image, in row order */
template <class Src>
RT_HD RtDnCol rt_dn_level_pixel(const RtDnParams& P, const Src& src, uint32_t x, uint32_t y, uint32_t level) {
    const RtDnCol cp = src.col(x, y);
    if (!rt_dn_finite(cp.l)) return cp; /* a centre value that is not finite is passed through */
    double gp[5];
    src.guide(x, y, gp);
    const bool pz = gp[0] == 0.0 && gp[1] == 0.0 && gp[2] == 0.0;
    const long long step = 1ll << level;
    const double sc = P.sigma_colour / (double)(1u << level); /* halved at every level */
    const double inv_sc2 = level == 0u ? 0.0 : 1.0 / (sc * sc); /* the first level has no colour term: a firefly does not reject its neighbours there */
    double sr = 0.0, sg = 0.0, sb = 0.0, sw = 0.0;
    for (int dy = -2; dy <= 2; ++dy) {
        const long long yy = (long long)y + dy * step;
        if (yy < 0 || yy >= (long long)P.h) continue;
        for (int dx = -2; dx <= 2; ++dx) {
            const long long xx = (long long)x + dx * step;
            if (xx < 0 || xx >= (long long)P.w) continue;
            const double hw = rt_dn_b3(dy) * rt_dn_b3(dx);
            double w = hw;
            RtDnCol cq = cp;
            if (dx != 0 || dy != 0) {
                cq = src.col((uint32_t)xx, (uint32_t)yy);
                double gq[5];
                src.guide((uint32_t)xx, (uint32_t)yy, gq);
                const bool qz = gq[0] == 0.0 && gq[1] == 0.0 && gq[2] == 0.0;
                double cosv = (gp[0] * gq[0] + gp[1] * gq[1]) + gp[2] * gq[2];
                cosv = cosv > 0.0 ? (cosv < 1.0 ? cosv : 1.0) : 0.0; /* NaN: 0 */
                const double wn = (pz && qz) ? 1.0 : rt_dn_powi(cosv, P.normal_power);
                const bool pinf = gp[3] == RT_INF, qinf = gq[3] == RT_INF;
                const double zmax = gp[3] > gq[3] ? gp[3] : gq[3];
                const double xd = (gp[3] == gq[3]) ? 0.0 : ((pinf || qinf) ? RT_INF : rt_abs(gp[3] - gq[3]) / (zmax * P.sigma_depth));
                const double dl = cp.l - cq.l;
                const double xc = (dl * dl) * inv_sc2;
                const double dv = gp[4] - gq[4];
                const double xv = (dv * dv) * RT_DN_INV_SIGMA_COV2;
                /* k(xd) k(xc) k(xv) evaluated as one k of the sum; the cut-off applies to the sum */
                w = (hw * wn) * rt_dn_falloff((xd + xc) + xv);
            }
            if (w > 0.0) { /* not for 0 and not for NaN: such a tap contributes nothing, whatever its value */
                sr += w * cq.r; sg += w * cq.g; sb += w * cq.b; sw += w;
            }
        }
    }
    RtDnCol o;
    o.r = sr / sw; o.g = sg / sw; o.b = sb / sw;
    o.l = rt_dn_lum(o.r, o.g, o.b);
    return o;
}

/* after the last level: the albedo back (times 1 with RT_DN_KEEP_ALBEDO) */
RT_HD void rt_dn_finish_pixel(const RtDnCol& c, const RtDnGuide& g, double* out) {
    out[0] = c.r * g.ar; out[1] = c.g * g.ag; out[2] = c.b * g.ab;
}

/* A filter as the two skeletons see it (the kernels' in rt_atrous_kernels.h, the twin's in denoise_host.cpp): Col, the record a level
 * reads and writes, a whole number of doubles; prepare, pixel i of the caller's input buffers to its records; level, with Src a reader
 * like RtDnGlobalSrc<Col> and sv2 the filter's extra argument (this filter has none); finish, the last level's record of pixel i to the
 * caller's output buffers (err_px: only the filters that have one).  Every filter header ends in its own */
struct RtDnFilter {
    typedef RtDnCol Col;
    static RT_HD void prepare(const RtDnParams& P, unsigned long long i, Col& c, RtDnGuide& g, const double* frame, const double* aov) {
        rt_dn_prepare_pixel(P, frame + i * 3u, aov + i * 8u, c, g);
    }
    template <class Src>
    static RT_HD Col level(const RtDnParams& P, double, const Src& src, uint32_t x, uint32_t y, uint32_t level) { return rt_dn_level_pixel(P, src, x, y, level); }
    static RT_HD void finish(const Col& c, const RtDnGuide& g, unsigned long long i, double* out, double*) { rt_dn_finish_pixel(c, g, out + i * 3u); }
};

#endif
