/* rt_adaptive.h -- the per-pixel accumulator of adaptive sampling (include/rt1w.h: rt1w_accum_merge, rt1w_accum_resolve,
 * rt1w_accum_tile_error): the running sum of sample batches with Welford's mean and sum of squared deviations of their luminances, what
 * a frame, a variance buffer and a sample-count map are read from it, and the error of a tile.  Compiled by the kernels (adaptive.hip)
 * and by the CPU twin of the diagnostics library (adaptive_host.cpp), from this one text.
 *
 * The rules of rt_denoise.h hold: + - * /, comparisons, selects and integer conversions in one fixed order, -ffp-contract=off, no libm, no
 * intrinsic.  The albedo floor and the luminance are that header's (RT_DN_EPS, rt_dn_lum), so l_k is rt1w_batch_variance's l_k. */
#ifndef RT_ADAPTIVE_H
#define RT_ADAPTIVE_H

#include "rt_denoise.h"

/* the record of a pixel, 8 doubles: S_r, S_g, S_b, m, mean_d, M2_d, mean_p, M2_p */
#define RT_AD_RECORD 8u
#define RT_AD_NO_ESTIMATE (-1.0) /* == RT1W_ACCUM_NO_ESTIMATE, kept in M2_d and M2_p */
#define RT_AD_ERR_FLOOR 0.01     /* added to the mean plain luminance a pixel's variance is divided by */
#define RT_AD_BLOCK 16u          /* the summation blocks of a tile are 16 x 16 pixels */
#define RT_AD_MIN_TILE 16u
#define RT_AD_MAX_TILE 256u

/* frame and rectangle of rt1w_accum_merge (false: RT1W_ERR_INVALID) */
RT_HD bool rt_ad_rect_ok(uint32_t w, uint32_t h, uint32_t x0, uint32_t y0, uint32_t tw, uint32_t th, uint32_t batch_spp, uint32_t flags) {
    RtDnParams P;
    if (!rt_dn_make_params(w, h, 0u, flags, 0.0, 0.0, 0.0, P)) return false;
    return batch_spp >= 1u && tw >= 1u && th >= 1u && x0 < w && y0 < h && tw <= w - x0 && th <= h - y0;
}
RT_HD bool rt_ad_frame_ok(uint32_t w, uint32_t h) {
    RtDnParams P;
    return rt_dn_make_params(w, h, 0u, 0u, 0.0, 0.0, 0.0, P);
}
RT_HD bool rt_ad_tile_ok(uint32_t tile) { return tile >= RT_AD_MIN_TILE && tile <= RT_AD_MAX_TILE && tile % RT_AD_BLOCK == 0u; }

/* Welford, in this order: the count is the caller's (m already raised) */
RT_HD void rt_ad_welford(double m, double l, double& mean, double& m2) {
    const double d = l - mean;
    mean = mean + d / m;
    m2 = m2 + d * (l - mean);
}

/* one pixel of rt1w_accum_merge.  q: the pixel's three raw sums of the batch; aov: its 8 channels; acc: its record */
RT_HD void rt_ad_merge_pixel(uint32_t batch_spp, bool keep_albedo, const double* q, const double* aov, double* acc) {
    const double a0 = aov[0], a1 = aov[1], a2 = aov[2];
    const double ar = keep_albedo ? 1.0 : ((a0 > RT_DN_EPS && rt_dn_finite(a0)) ? a0 : RT_DN_EPS);
    const double ag = keep_albedo ? 1.0 : ((a1 > RT_DN_EPS && rt_dn_finite(a1)) ? a1 : RT_DN_EPS);
    const double ab = keep_albedo ? 1.0 : ((a2 > RT_DN_EPS && rt_dn_finite(a2)) ? a2 : RT_DN_EPS);
    const double inv_n = 1.0 / (double)batch_spp;
    const double q0 = q[0], q1 = q[1], q2 = q[2];
    const double m0 = acc[3];
    const bool first = m0 == 0.0; /* the first batch is taken as it is: 0 + q would lose the sign of a zero */
    acc[0] = first ? q0 : acc[0] + q0;
    acc[1] = first ? q1 : acc[1] + q1;
    acc[2] = first ? q2 : acc[2] + q2;
    const double m = m0 + 1.0;
    acc[3] = m;
    const double mr = q0 * inv_n, mg = q1 * inv_n, mb = q2 * inv_n;
    const double ld = rt_dn_lum(keep_albedo ? mr : mr / ar, keep_albedo ? mg : mg / ag, keep_albedo ? mb : mb / ab);
    const double lp = rt_dn_lum(mr, mg, mb);
    double mean_d = acc[4], m2_d = acc[5], mean_p = acc[6], m2_p = acc[7];
    const bool marked = m2_d < 0.0 || m2_p < 0.0;
    if (!marked) {
        if (rt_dn_finite(ld) && rt_dn_finite(lp)) {
            rt_ad_welford(m, ld, mean_d, m2_d);
            rt_ad_welford(m, lp, mean_p, m2_p);
        } else {
            m2_d = RT_AD_NO_ESTIMATE; m2_p = RT_AD_NO_ESTIMATE;
        }
    }
    acc[4] = mean_d; acc[5] = m2_d; acc[6] = mean_p; acc[7] = m2_p;
}

/* one pixel of rt1w_accum_merge_tiles: pixel (lx, ly) of tile k of the list, whose corner is (x0, y0); sums[n][tile][tile][3].  A pixel
 * beyond the frame's edge is skipped.  The same rt_ad_merge_pixel on the same operands as rt1w_accum_merge of the clipped rectangle. */
RT_HD void rt_ad_merge_tiles_pixel(uint32_t w, uint32_t h, uint32_t tile, uint32_t x0, uint32_t y0, uint32_t k, uint32_t lx, uint32_t ly, uint32_t batch_spp,
                                   bool keep_albedo, const double* sums, const double* aov, double* acc) {
    const uint32_t x = x0 + lx, y = y0 + ly;
    if (x >= w || y >= h) return;
    const unsigned long long i = (unsigned long long)y * w + x;
    const unsigned long long t = ((unsigned long long)k * tile + ly) * tile + lx;
    rt_ad_merge_pixel(batch_spp, keep_albedo, sums + t * 3u, aov + i * 8u, acc + i * RT_AD_RECORD);
}
#define RT_AD_TILES_MAX (1u << 20) /* tiles of one list (rt1w_render_tiles' bound) */

/* one pixel of rt1w_accum_resolve: frame[3], *var, *spp */
RT_HD void rt_ad_resolve_pixel(uint32_t batch_spp, const double* acc, double* frame, double* var, double* spp) {
    const double m = acc[3];
    const double count = m * (double)batch_spp;
    const double tr = acc[0], tg = acc[1], tb = acc[2];
    if (m >= 1.0) {
        const double scale = 1.0 / count;
        frame[0] = (tr != tr ? 0.0 : tr) * scale;
        frame[1] = (tg != tg ? 0.0 : tg) * scale;
        frame[2] = (tb != tb ? 0.0 : tb) * scale;
    } else { /* an empty pixel */
        frame[0] = 0.0; frame[1] = 0.0; frame[2] = 0.0;
    }
    const double m2 = acc[5];
    double v = 0.0;
    if (m >= 2.0 && m2 >= 0.0) {
        v = m2 / (m * (m - 1.0));
        v = (v >= 0.0 && rt_dn_finite(v)) ? v : 0.0;
    }
    *var = v;
    *spp = m >= 1.0 ? count : 0.0;
}

/* e_p of rt1w_accum_tile_error */
RT_HD double rt_ad_pixel_error(const double* acc) {
    const double m = acc[3], mean = acc[6], m2 = acc[7];
    if (!(m >= 2.0) || !(m2 >= 0.0)) return 0.0;
    const double v = m2 / (m * (m - 1.0));
    const double e = v / ((mean > 0.0 ? mean : 0.0) + RT_AD_ERR_FLOOR);
    return (e >= 0.0 && rt_dn_finite(e)) ? e : 0.0;
}

/* the binary tree over the 256 values of a block, stride 128 down to 1: the twin's form (the kernel runs the same additions, one
 * lane per i, between barriers) */
RT_HD double rt_ad_block_tree(double* v) {
    for (uint32_t stride = 128u; stride >= 1u; stride >>= 1)
        for (uint32_t i = 0; i < stride; ++i) v[i] = v[i] + v[i + stride];
    return v[0];
}

/* pixels of tile (tx, ty) that lie inside the frame */
RT_HD unsigned long long rt_ad_tile_pixels(uint32_t w, uint32_t h, uint32_t tile, uint32_t tx, uint32_t ty) {
    const unsigned long long x0 = (unsigned long long)tx * tile, y0 = (unsigned long long)ty * tile;
    const unsigned long long x1 = x0 + tile < w ? x0 + tile : w, y1 = y0 + tile < h ? y0 + tile : h;
    return (x1 - x0) * (y1 - y0);
}

#endif
