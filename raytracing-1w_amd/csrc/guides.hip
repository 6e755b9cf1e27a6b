/* guides.hip -- the kernels of rt1w_guides_merge_tiles and rt1w_guides_resolve (include/rt1w.h) over rt_guides.h.
 *
 * A unit of its own, inside its own namespace (the pattern of adaptive.hip), so that no other code object moves with it.  The host half
 * is in features.hip, which calls the two launchers below.
 *
 * Work mapping: that of rt_pixel_kernels.h -- one lane per pixel, an 8 x 8 pixel block per wave, 2 x 2 blocks (16 x 16 pixels) per workgroup
 * of 256 lanes; every pixel is computed whole by one lane, no atomics.  The resolve runs its workgroups in row order over the frame, the
 * merge (tile / 16)^2 workgroups per tile of the list, tile after tile.  The record is 72 bytes per pixel, read and written by its lane
 * as 9 doubles. */
#include <hip/hip_runtime.h>
#include "rt_feature_launch.h" /* this unit's functions as features.hip calls them: the definitions below are held to it */
#include <stdint.h>
#include <string.h>

namespace rtgd {
#include "rt1w_num.h"
#include "rt_guides.h"

#include "rt_pixel_kernels.h"

/* sums[n][tile][tile][8] -> gacc[h][w][9] */
__global__ __launch_bounds__(RT_PX_WG) void rt_gd_merge_tiles_kernel(uint32_t w, uint32_t h, uint32_t tile, const uint32_t* __restrict__ rec, uint32_t spp,
                                                                      const double* __restrict__ sums, double* __restrict__ gacc) {
    const RtPxListLane l = rt_px_list_lane(tile, rec);
    rt_gd_merge_tiles_pixel(w, h, tile, l.x0, l.y0, l.k, l.lx, l.ly, spp, sums, gacc);
}

/* gacc[h][w][9] -> aov[h][w][8] */
__global__ __launch_bounds__(RT_PX_WG) void rt_gd_resolve_kernel(uint32_t w, uint32_t h, const double* __restrict__ gacc, double* __restrict__ aov) {
    uint32_t x, y;
    rt_px_lane_pixel(w, x, y);
    if (x >= w || y >= h) return;
    const unsigned long long i = (unsigned long long)y * w + x;
    rt_gd_resolve_pixel(gacc + i * RT_GD_RECORD, aov + i * RT_GD_SUMS);
}
} // namespace rtgd

/* called by features.hip.  Each enqueues one kernel on `stream`; launch[0..1] = grid, block.  0, -1 (launch failure) or -2 (parameters
 * refused).  The list itself (alignment, frame, no tile twice) is the caller's to check (rt_adaptive_plan.h: rt_gd_tiles_check); rec is
 * device memory */
extern "C" int rt1w_internal_guides_merge_tiles_launch(uint32_t w, uint32_t h, uint32_t tile, const uint32_t* rec, uint32_t n, uint32_t spp, const double* sums,
                                                       double* gacc, hipStream_t stream, unsigned launch[2]) {
    using namespace rtgd;
    if (!rt_ad_frame_ok(w, h) || !rt_ad_tile_ok(tile) || spp < 1u || n < 1u || n > RT_AD_TILES_MAX) return -2;
    return rt_px_launch(rt_gd_merge_tiles_kernel, rt_px_list_grid(tile, n), stream, launch, w, h, tile, rec, spp, sums, gacc);
}
extern "C" int rt1w_internal_guides_resolve_launch(uint32_t w, uint32_t h, const double* gacc, double* aov, hipStream_t stream, unsigned launch[2]) {
    using namespace rtgd;
    if (!rt_ad_frame_ok(w, h)) return -2;
    return rt_px_launch(rt_gd_resolve_kernel, rt_px_frame_grid(w, h), stream, launch, w, h, gacc, aov);
}
