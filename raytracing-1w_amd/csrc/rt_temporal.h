/* rt_temporal.h -- temporal accumulation (rt1w_temporal_accumulate, include/rt1w.h has the definition): the current frame's pixel is
 * reprojected through its first-hit depth into the previous frame, whose demodulated history is gathered with four bilinear taps that
 * pass a depth and a normal test, and blended with the current value.  Compiled by the kernels (temporal.hip, and temporal_var.hip for
 * rt1w_temporal_moments) and by the CPU twin of the diagnostics library (denoise_host.cpp), from this one text.
 *
 * Everything is + - * /, rt_sqrt, comparisons, selects and integer <-> double conversions in one fixed order (built with
 * -ffp-contract=off like every build of the core): the two builds give the same bits.  No libm, no intrinsic.  Nothing here is reached
 * by the render kernels or by the run-time compiler. */
#ifndef RT_TEMPORAL_H
#define RT_TEMPORAL_H

#include "rt_flat.h"    /* RtCamera, RtV3 */
#include "rt_denoise.h" /* the prepare pass: albedo floor, unit normal */

#define RT_TM_KEEP_ALBEDO RT_DN_KEEP_ALBEDO
#define RT_TM_MAX_HISTORY 32u
#define RT_TM_DEPTH_TOL 0.05
#define RT_TM_NORMAL_MIN 0.9
#define RT_TM_REC 8 /* doubles of the twin's optional record of a pixel: fx, fy, the four taps' weights (0: not valid), their sum, history (1 / 0) */

/* a call's parameters with the defaults filled in */
struct RtTmParams {
    uint32_t w, h, keep_albedo, max_history;
    double depth_tol, normal_min;
};

/* false: the parameters are refused (RT1W_ERR_INVALID) */
RT_HD bool rt_tm_make_params(uint32_t w, uint32_t h, uint32_t flags, uint32_t max_history, double depth_tol, double normal_min, RtTmParams& P) {
    if (w == 0u || h == 0u || w > 0x40000000u || h > 0x40000000u || (flags & ~RT_TM_KEEP_ALBEDO) != 0u) return false;
    if (!(depth_tol >= 0.0) || !(normal_min >= 0.0) || !rt_dn_finite(depth_tol) || normal_min > 1.0) return false;
    if ((((unsigned long long)w + 15u) >> 4) * (((unsigned long long)h + 15u) >> 4) > 0x7FFFFFFFull) return false;
    P.w = w; P.h = h;
    P.keep_albedo = flags & RT_TM_KEEP_ALBEDO;
    P.max_history = max_history ? max_history : RT_TM_MAX_HISTORY;
    P.depth_tol = depth_tol == 0.0 ? RT_TM_DEPTH_TOL : depth_tol;
    P.normal_min = normal_min == 0.0 ? RT_TM_NORMAL_MIN : normal_min;
    return true;
}

/* the prepare pass of rt_denoise.h with this call's albedo switch */
RT_HD void rt_tm_prepare(uint32_t keep_albedo, const double* frame, const double* aov, RtDnCol& c, RtDnGuide& g) {
    RtDnParams D;
    D.w = D.h = D.levels = D.normal_power = D.pad = 0u;
    D.sigma_colour = D.sigma_depth = 0.0;
    D.keep_albedo = keep_albedo; D.eps = RT_DN_EPS;
    rt_dn_prepare_pixel(D, frame, aov, c, g);
}

/* pixel (x, y) of a w x h image: hist[3], len[1] and frame_out[3] of that pixel; rec: RT_TM_REC doubles, or null.
 * prev_m2, m2: null for rt1w_temporal_accumulate (its kernel passes null constants: the branches fold away).  For rt1w_temporal_moments
 * the whole previous image of second moments and this pixel's m2[1]: the running mean of the squared demodulated luminance, gathered
 * over the very taps of the history, read only where a tap is valid */
RT_HD void rt_tm_pixel(const RtTmParams& P, const RtCamera& cc, const RtCamera& pc, const double* cur_frame, const double* cur_aov,
                       const double* prev_hist, const double* prev_len, const double* prev_aov, const double* prev_m2, uint32_t x, uint32_t y,
                       double* hist, double* len, double* frame_out, double* m2, double* rec) {
    const unsigned long long i = (unsigned long long)y * P.w + x;
    RtDnCol c;
    RtDnGuide g;
    rt_tm_prepare(P.keep_albedo, cur_frame + i * 3u, cur_aov + i * 8u, c, g);
    /* the divisors of main.rs:968-969; an image of one column or row (which no render makes) has its centre at 1/2 */
    const double w1 = (double)(P.w > 1u ? P.w - 1u : 1u), h1 = (double)(P.h > 1u ? P.h - 1u : 1u);
    double hr = 0.0, hg = 0.0, hb = 0.0, hn = 0.0, hm = 0.0, sw = 0.0, fx = 0.0, fy = 0.0;
    double tw[4] = {0.0, 0.0, 0.0, 0.0};
    bool history = false;
    if (g.v > 0.0 && rt_dn_finite(g.z)) { /* a hit with a depth: NaN coverage is no hit */
        /* the point seen: along the ray from the lens centre through the pixel centre, at the first-hit distance */
        const double s = ((double)x + 0.5) / w1, t = ((double)y + 0.5) / h1;
        const RtV3 dir = ((cc.lower_left_corner + s * cc.horizontal) + t * cc.vertical) - cc.origin;
        const RtV3 X = cc.origin + dir * (g.z / rt_mag(dir));
        /* through the previous camera's pinhole onto its focus plane */
        const RtV3 p = X - pc.origin;
        const double pw = rt_dot(p, pc.w);
        if (pw < 0.0) { /* in front of the previous camera, which looks along -w */
            const double dist = rt_mag(p);
            const RtV3 D = pc.origin - pc.lower_left_corner;
            const double k = rt_dot(D, pc.w) / (0.0 - pw); /* focus distance over the point's distance along the axis */
            const RtV3 q = D + p * k;                     /* the point on the focus plane, from its lower left corner */
            const double ps = rt_dot(q, pc.horizontal) / rt_dot(pc.horizontal, pc.horizontal);
            const double pt = rt_dot(q, pc.vertical) / rt_dot(pc.vertical, pc.vertical);
            fx = ps * w1 - 0.5;
            fy = pt * h1 - 0.5;
            if (fx > -1.0 && fx < (double)P.w && fy > -1.0 && fy < (double)P.h) { /* NaN: no tap in the image */
                long long ix = (long long)fx, iy = (long long)fy; /* floor: truncation, one less where that rounded up */
                if ((double)ix > fx) ix -= 1;
                if ((double)iy > fy) iy -= 1;
                const double wx = fx - (double)ix, wy = fy - (double)iy;
                for (int k4 = 0; k4 < 4; ++k4) { /* (0,0), (1,0), (0,1), (1,1) */
                    const long long qx = ix + (k4 & 1), qy = iy + (k4 >> 1);
                    if (qx < 0 || qy < 0 || qx >= (long long)P.w || qy >= (long long)P.h) continue;
                    const unsigned long long j = (unsigned long long)qy * P.w + (unsigned long long)qx;
                    const double n = prev_len[j];
                    RtDnCol cq;
                    RtDnGuide gq;
                    rt_tm_prepare(1u, prev_hist + j * 3u, prev_aov + j * 8u, cq, gq); /* the history is kept demodulated: taken as it is */
                    const double cosv = (gq.nx * g.nx + gq.ny * g.ny) + gq.nz * g.nz;
                    const bool valid = n > 0.0 && rt_dn_finite(n) && gq.v > 0.0 && rt_dn_finite(gq.z) && rt_abs(gq.z - dist) <= P.depth_tol * dist &&
                                       cosv >= P.normal_min && rt_dn_finite(cq.r) && rt_dn_finite(cq.g) && rt_dn_finite(cq.b);
                    if (!valid) continue;
                    const double w = ((k4 & 1) ? wx : 1.0 - wx) * ((k4 >> 1) ? wy : 1.0 - wy);
                    tw[k4] = w;
                    hr += w * cq.r; hg += w * cq.g; hb += w * cq.b; hn += w * n; sw += w;
                    if (prev_m2) hm += w * prev_m2[j];
                }
                history = sw > 0.0;
            }
        }
    }
    double o0 = c.r, o1 = c.g, o2 = c.b, on = 1.0;
    if (history) {
        const double cap = (double)(P.max_history - 1u);
        const double N = hn / sw;
        const double Nc = N < cap ? N : cap;
        o0 = (Nc * (hr / sw) + c.r) / (Nc + 1.0);
        o1 = (Nc * (hg / sw) + c.g) / (Nc + 1.0);
        o2 = (Nc * (hb / sw) + c.b) / (Nc + 1.0);
        on = Nc + 1.0;
        if (m2) m2[0] = (Nc * (hm / sw) + c.l * c.l) / (Nc + 1.0);
    } else if (m2) {
        m2[0] = c.l * c.l;
    }
    hist[0] = o0; hist[1] = o1; hist[2] = o2;
    len[0] = on;
    frame_out[0] = o0 * g.ar; frame_out[1] = o1 * g.ag; frame_out[2] = o2 * g.ab;
    if (rec) {
        rec[0] = fx; rec[1] = fy; rec[2] = tw[0]; rec[3] = tw[1]; rec[4] = tw[2]; rec[5] = tw[3]; rec[6] = sw; rec[7] = history ? 1.0 : 0.0;
    }
}

#endif
