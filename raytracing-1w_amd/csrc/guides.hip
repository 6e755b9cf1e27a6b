/* guides.hip -- the kernels of rt1w_guides_merge_tiles and rt1w_guides_resolve (include/rt1w.h) over rt_guides.h.
 *
 * A unit of its own, inside its own namespace (the pattern of adaptive.hip), so that no other code object moves with it.  The host half
 * is in features.hip, which calls the two launchers below.
 *
 * Work mapping: that of adaptive.hip -- one lane per pixel, an 8 x 8 pixel block per wave, 2 x 2 blocks (16 x 16 pixels) per workgroup of
 * 256 lanes; every pixel is computed whole by one lane, no atomics.  The merge runs (tile / 16)^2 workgroups per tile of the list, tile
 * after tile: a workgroup's tile follows from blockIdx alone, so its record {x0, y0, -, -} is read wave-uniformly.  The record is 72 bytes
 * per pixel, read and written by its lane as 9 doubles. */
#include <hip/hip_runtime.h>
#include "rt_feature_launch.h" /* this unit's functions as features.hip calls them: the definitions below are held to it */
#include <stdint.h>
#include <string.h>

namespace rtgd {
#include "rt1w_num.h"
#include "rt_guides.h"

#define RT_GD_WG 256

/* pixel of this lane inside its workgroup's 16 x 16 block: 8 x 8 per wave, 2 x 2 waves */
__device__ __forceinline__ void rt_gd_lane_xy(uint32_t& lx, uint32_t& ly) {
    const uint32_t wv = threadIdx.x >> 6, in = threadIdx.x & 63u;
    lx = (wv & 1u) * 8u + (in & 7u);
    ly = (wv >> 1) * 8u + (in >> 3);
}

/* sums[n][tile][tile][8] -> gacc[h][w][9] */
__global__ __launch_bounds__(RT_GD_WG) void rt_gd_merge_tiles_kernel(uint32_t w, uint32_t h, uint32_t tile, const uint32_t* __restrict__ rec, uint32_t spp,
                                                                      const double* __restrict__ sums, double* __restrict__ gacc) {
    const uint32_t bw = tile / RT_AD_BLOCK;
    const uint32_t k = blockIdx.x / (bw * bw), b = blockIdx.x % (bw * bw);
    const uint32_t x0 = rec[(size_t)k * 4u], y0 = rec[(size_t)k * 4u + 1u];
    uint32_t lx, ly;
    rt_gd_lane_xy(lx, ly);
    rt_gd_merge_tiles_pixel(w, h, tile, x0, y0, k, (b % bw) * RT_AD_BLOCK + lx, (b / bw) * RT_AD_BLOCK + ly, spp, sums, gacc);
}

/* gacc[h][w][9] -> aov[h][w][8] */
__global__ __launch_bounds__(RT_GD_WG) void rt_gd_resolve_kernel(uint32_t w, uint32_t h, const double* __restrict__ gacc, double* __restrict__ aov) {
    const uint32_t blocks_x = (w + RT_AD_BLOCK - 1u) / RT_AD_BLOCK;
    uint32_t lx, ly;
    rt_gd_lane_xy(lx, ly);
    const uint32_t x = (blockIdx.x % blocks_x) * RT_AD_BLOCK + lx, y = (blockIdx.x / blocks_x) * RT_AD_BLOCK + ly;
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
    const unsigned bw = tile / RT_AD_BLOCK, grid = n * bw * bw; /* <= 2^20 x 256 */
    launch[0] = grid; launch[1] = RT_GD_WG;
    hipLaunchKernelGGL(rt_gd_merge_tiles_kernel, dim3(grid), dim3(RT_GD_WG), 0, stream, w, h, tile, rec, spp, sums, gacc);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
extern "C" int rt1w_internal_guides_resolve_launch(uint32_t w, uint32_t h, const double* gacc, double* aov, hipStream_t stream, unsigned launch[2]) {
    using namespace rtgd;
    if (!rt_ad_frame_ok(w, h)) return -2;
    const unsigned grid = ((w + RT_AD_BLOCK - 1u) / RT_AD_BLOCK) * ((h + RT_AD_BLOCK - 1u) / RT_AD_BLOCK);
    launch[0] = grid; launch[1] = RT_GD_WG;
    hipLaunchKernelGGL(rt_gd_resolve_kernel, dim3(grid), dim3(RT_GD_WG), 0, stream, w, h, gacc, aov);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
