/* rt_aov_tiles.h -- the first-hit feature SUMS of a list of square tiles (rt1w_render_aov_tiles, include/rt1w.h): what rt_aov_pixel adds up,
 * before its divisions, for a pixel named by its image position.  Compiled by the tile-list AOV kernels (aov_tiles.hip) and by the CPU twin
 * of the diagnostics library (aov_host.cpp), from this one text.  The per-sample code is rt_aov_sample of rt_aov.h, as it stands; nothing
 * here is reached by rt_aov_kernel or by the render kernels. */
#ifndef RT_AOV_TILES_H
#define RT_AOV_TILES_H

#include "rt_aov.h"

/* the 8 raw sums of image pixel (i, j): samples first .. first + f.spp - 1 added in order, exactly the additions of rt_aov_pixel.  0-2 the
 * albedo, 3-5 the normal, 6 t |d| over the samples that hit (+0.0 if none did), 7 the number of samples that hit.  From f: width, height,
 * spp, global_seed */
template <class Cfg, class Stack, class NS>
RT_HD void rt_aov_pixel_sums(const RtSceneView& sc, const NS& ns, const RtFrame& f, uint32_t i, uint32_t j, uint32_t first, Stack& stk, double* out) {
    RtV3 alb = rt_v3(RT_R(0.0), RT_R(0.0), RT_R(0.0)), nrm = alb;
    double dist = RT_R(0.0), cov = RT_R(0.0);
    for (uint32_t s = 0; s < f.spp; ++s) {
        const RtAovSample a = rt_aov_sample<Cfg>(sc, ns, f, i, j, first + s, stk);
        alb = alb + a.albedo;
        nrm = nrm + a.normal;
        if (a.hit) { dist += a.dist; cov += RT_R(1.0); }
    }
    out[0] = alb.x; out[1] = alb.y; out[2] = alb.z;
    out[3] = nrm.x; out[4] = nrm.y; out[5] = nrm.z;
    out[6] = dist;
    out[7] = cov;
}

/* pixel (lx, ly) of tile k of the list, whose corner is (x0, y0) and whose own sample offset is `so`: out[n][tile][tile][8].  A pixel beyond
 * the frame's edge is not traced: +0.0 in all eight.  false: such a pixel */
template <class Cfg, class Stack, class NS>
RT_HD bool rt_aov_tiles_pixel(const RtSceneView& sc, const NS& ns, const RtFrame& f, uint32_t tile, uint32_t k, uint32_t x0, uint32_t y0, uint32_t so,
                              uint32_t lx, uint32_t ly, Stack& stk, double* out) {
    double* o = out + (((unsigned long long)k * tile + ly) * tile + lx) * RT_AOV_CHANNELS;
    const uint32_t i = x0 + lx, j = y0 + ly;
    if (i >= f.width || j >= f.height) {
        for (int c = 0; c < RT_AOV_CHANNELS; ++c) o[c] = RT_R(0.0);
        return false;
    }
    rt_aov_pixel_sums<Cfg>(sc, ns, f, i, j, f.sample_offset + so, stk, o);
    return true;
}

#endif
