/* rt_guides.h -- the guide accumulator (include/rt1w.h: rt1w_guides_merge_tiles, rt1w_guides_resolve): per pixel the eight first-hit feature
 * sums rt1w_render_aov_tiles writes, added up over calls, and the number of samples they hold; feature buffers in rt1w_render_aov's layout
 * are read from it.  Compiled by the kernels (guides.hip) and by the CPU twin of the diagnostics library (adaptive_host.cpp), from this one
 * text.  The rules of rt_denoise.h hold: + and /, comparisons and selects in one fixed order, -ffp-contract=off, no libm, no intrinsic. */
#ifndef RT_GUIDES_H
#define RT_GUIDES_H

#include "rt_adaptive.h"

/* the record of a pixel, 9 doubles: the sums of albedo rgb, normal xyz, t |d| over the hits and the hit count, then N, the samples merged */
#define RT_GD_RECORD 9u
#define RT_GD_SUMS 8u

/* one pixel of a merge.  s: its eight sums over `spp` samples; g: its record.  An empty record takes the sums as they are (0 + s would
 * lose the sign of a zero), so one merge into an empty accumulator keeps rt1w_render_aov_tiles's bits */
RT_HD void rt_gd_merge_pixel(uint32_t spp, const double* s, double* g) {
    const double n0 = g[8];
    const bool first = n0 == 0.0;
    for (uint32_t c = 0; c < RT_GD_SUMS; ++c) {
        const double v = s[c];
        g[c] = first ? v : g[c] + v;
    }
    g[8] = first ? (double)spp : n0 + (double)spp;
}

/* one pixel of rt1w_guides_merge_tiles: pixel (lx, ly) of tile k of the list, whose corner is (x0, y0); sums[n][tile][tile][8].  A pixel
 * beyond the frame's edge is skipped */
RT_HD void rt_gd_merge_tiles_pixel(uint32_t w, uint32_t h, uint32_t tile, uint32_t x0, uint32_t y0, uint32_t k, uint32_t lx, uint32_t ly, uint32_t spp,
                                   const double* sums, double* gacc) {
    const uint32_t x = x0 + lx, y = y0 + ly;
    if (x >= w || y >= h) return;
    const unsigned long long i = (unsigned long long)y * w + x;
    const unsigned long long t = ((unsigned long long)k * tile + ly) * tile + lx;
    rt_gd_merge_pixel(spp, sums + t * RT_GD_SUMS, gacc + i * RT_GD_RECORD);
}

/* one pixel of rt1w_guides_resolve: the 8 channels of rt1w_render_aov.  rt_aov_pixel's divisions: 0-5 and 7 by the sample count, 6 by the
 * hit count, +inf without a hit; an empty record is a pixel nobody has looked at: black, no normal, no hit */
RT_HD void rt_gd_resolve_pixel(const double* g, double* aov) {
    const double n = g[8], hits = g[7];
    if (n == 0.0) {
        for (uint32_t c = 0; c < RT_GD_SUMS; ++c) aov[c] = 0.0;
        aov[6] = RT_INF;
        return;
    }
    aov[0] = g[0] / n; aov[1] = g[1] / n; aov[2] = g[2] / n;
    aov[3] = g[3] / n; aov[4] = g[4] / n; aov[5] = g[5] / n;
    aov[6] = hits > 0.0 ? g[6] / hits : RT_INF;
    aov[7] = hits / n;
}

#endif
