/* adaptive.hip -- the kernels of rt1w_accum_merge, rt1w_accum_resolve and rt1w_accum_tile_error (include/rt1w.h) over rt_adaptive.h, and
 * of rt1w_halves_resolve and rt1w_tile_error_map over rt_denoise_halves.h.
 *
 * rt1w_accum_merge_tiles is the merge over a list of square tiles in one launch.  rt1w_halves_resolve is the resolve of two accumulators
 * as the halves of one frame; rt1w_tile_error_map is the tile error's sum over a per-pixel map instead of the accumulator's e_p: the
 * same kernel text with another source of the pixel's value.
 * A unit of its own, inside its own namespace (the pattern of denoise_var.hip), so that no other code object moves with it.  The host
 * half is in features.hip, which calls the three launchers below.
 *
 * Work mapping: that of rt_pixel_kernels.h -- one lane per pixel, an 8 x 8 pixel block per wave, 2 x 2 blocks (16 x 16 pixels) per
 * workgroup of 256 lanes.  Merge and resolve compute every pixel whole by one lane.  The tile error runs one workgroup per tile: for
 * each 16 x 16 block of the tile in row-major order every lane writes its pixel's e_p (0 outside the frame) into 2 KiB of LDS at the
 * pixel's row-major index, the workgroup adds them by the binary tree of the header (stride 128 .. 1, a barrier per step), and lane 0
 * adds the block's sum to the tile's: no atomics, one fixed order, the same bits as the CPU twin (adaptive_host.cpp).  The accumulator
 * record is 64 bytes per pixel, read and written by its lane as 8 doubles. */
#include <hip/hip_runtime.h>
#include "rt_feature_launch.h" /* this unit's functions as features.hip calls them: the definitions below are held to it */
#include <stdint.h>
#include <string.h>

namespace rtad {
#include "rt1w_num.h"
#include "rt_adaptive.h"
#include "rt_denoise_halves.h"

#include "rt_pixel_kernels.h"
static_assert(RT_AD_BLOCK == RT_PX_BLOCK, "a summation block of the tile error is a workgroup's block of pixels");

/* tile_sums[th][tw][3], aov[h][w][8] -> acc[h][w][8]; workgroups in row order over the rectangle */
__global__ __launch_bounds__(RT_PX_WG) void rt_ad_merge_kernel(uint32_t w, uint32_t x0, uint32_t y0, uint32_t tw, uint32_t th, uint32_t batch_spp,
                                                                uint32_t keep_albedo, const double* __restrict__ sums, const double* __restrict__ aov,
                                                                double* __restrict__ acc) {
    uint32_t rx, ry;
    rt_px_lane_pixel(tw, rx, ry);
    if (rx >= tw || ry >= th) return;
    const unsigned long long i = (unsigned long long)(y0 + ry) * w + (x0 + rx);
    const unsigned long long t = (unsigned long long)ry * tw + rx;
    rt_ad_merge_pixel(batch_spp, keep_albedo != 0u, sums + t * 3u, aov + i * 8u, acc + i * RT_AD_RECORD);
}

/* rt1w_accum_merge_tiles: sums[n][tile][tile][3], aov[h][w][8] -> acc[h][w][8]; (tile / 16)^2 workgroups per tile of the list, tile after
 * tile (rt_px_list_lane). */
__global__ __launch_bounds__(RT_PX_WG) void rt_ad_merge_tiles_kernel(uint32_t w, uint32_t h, uint32_t tile, const uint32_t* __restrict__ rec, uint32_t batch_spp,
                                                                      uint32_t keep_albedo, const double* __restrict__ sums, const double* __restrict__ aov,
                                                                      double* __restrict__ acc) {
    const RtPxListLane l = rt_px_list_lane(tile, rec);
    rt_ad_merge_tiles_pixel(w, h, tile, l.x0, l.y0, l.k, l.lx, l.ly, batch_spp, keep_albedo != 0u, sums, aov, acc);
}

/* acc[h][w][8] -> frame[h][w][3], var[h][w], spp[h][w] */
__global__ __launch_bounds__(RT_PX_WG) void rt_ad_resolve_kernel(uint32_t w, uint32_t h, uint32_t batch_spp, const double* __restrict__ acc,
                                                                  double* __restrict__ frame, double* __restrict__ var, double* __restrict__ spp) {
    uint32_t x, y;
    rt_px_lane_pixel(w, x, y);
    if (x >= w || y >= h) return;
    const unsigned long long i = (unsigned long long)y * w + x;
    double f[3], v, s;
    rt_ad_resolve_pixel(batch_spp, acc + i * RT_AD_RECORD, f, &v, &s);
    frame[i * 3u] = f[0]; frame[i * 3u + 1u] = f[1]; frame[i * 3u + 2u] = f[2];
    var[i] = v;
    spp[i] = s;
}

/* acc_a[h][w][8], acc_b[h][w][8] -> frame[h][w][3], var[h][w], half_a[h][w][3], half_b[h][w][3], spp[h][w] */
__global__ __launch_bounds__(RT_PX_WG) void rt_ad_halves_resolve_kernel(uint32_t w, uint32_t h, uint32_t batch_spp, const double* __restrict__ acc_a,
                                                                         const double* __restrict__ acc_b, double* __restrict__ frame, double* __restrict__ var,
                                                                         double* __restrict__ half_a, double* __restrict__ half_b, double* __restrict__ spp) {
    uint32_t x, y;
    rt_px_lane_pixel(w, x, y);
    if (x >= w || y >= h) return;
    const unsigned long long i = (unsigned long long)y * w + x;
    double f[3], a[3], b[3], v, s;
    rt_dh_resolve_pixel(batch_spp, acc_a + i * RT_AD_RECORD, acc_b + i * RT_AD_RECORD, f, &v, a, b, &s);
    frame[i * 3u] = f[0]; frame[i * 3u + 1u] = f[1]; frame[i * 3u + 2u] = f[2];
    half_a[i * 3u] = a[0]; half_a[i * 3u + 1u] = a[1]; half_a[i * 3u + 2u] = a[2];
    half_b[i * 3u] = b[0]; half_b[i * 3u + 1u] = b[1]; half_b[i * 3u + 2u] = b[2];
    var[i] = v;
    spp[i] = s;
}

/* MAP false: in = acc[h][w][8], a pixel's value its e_p; MAP true: in = err_px[h][w], the value as rt_dh_map_value takes it
 * -> err[tiles_y][tiles_x]; one workgroup per tile */
template <bool MAP>
__global__ __launch_bounds__(RT_PX_WG) void rt_ad_tile_error_kernel(uint32_t w, uint32_t h, uint32_t tile, const double* __restrict__ in,
                                                                     double* __restrict__ err) {
    __shared__ double v[RT_PX_WG];
    const uint32_t tiles_x = (w + tile - 1u) / tile;
    const uint32_t tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
    const uint32_t px0 = tx * tile, py0 = ty * tile; /* inside the frame: tile <= 256 and tx < tiles_x */
    const uint32_t bw = tile / RT_AD_BLOCK;
    uint32_t lx, ly;
    rt_px_lane_xy(lx, ly);
    double total = 0.0;
    for (uint32_t by = 0; by < bw; ++by) {
        if (py0 + by * RT_AD_BLOCK >= h) break; /* uniform over the workgroup: blocks without a pixel of the frame are not added */
        for (uint32_t bx = 0; bx < bw; ++bx) {
            if (px0 + bx * RT_AD_BLOCK >= w) break;
            const uint32_t x = px0 + bx * RT_AD_BLOCK + lx, y = py0 + by * RT_AD_BLOCK + ly;
            double e = 0.0;
            if (x < w && y < h) {
                const unsigned long long i = (unsigned long long)y * w + x;
                if constexpr (MAP) e = rt_dh_map_value(in[i]);
                else e = rt_ad_pixel_error(in + i * RT_AD_RECORD);
            }
            v[ly * RT_AD_BLOCK + lx] = e;
            __syncthreads();
            for (uint32_t stride = 128u; stride >= 1u; stride >>= 1) {
                if (threadIdx.x < stride) v[threadIdx.x] = v[threadIdx.x] + v[threadIdx.x + stride];
                __syncthreads();
            }
            if (threadIdx.x == 0u) total = total + v[0];
            __syncthreads(); /* v[0] is read before the next block's values are written */
        }
    }
    if (threadIdx.x == 0u) err[blockIdx.x] = total / (double)rt_ad_tile_pixels(w, h, tile, tx, ty);
}
} // namespace rtad

/* called by features.hip.  Each enqueues one kernel on `stream`; launch[0..1] = grid, block.  0, -1 (launch failure) or -2 (parameters
 * refused). */
extern "C" int rt1w_internal_accum_merge_launch(uint32_t w, uint32_t h, uint32_t x0, uint32_t y0, uint32_t tw, uint32_t th, uint32_t batch_spp,
                                                uint32_t flags, const double* sums, const double* aov, double* acc, hipStream_t stream,
                                                unsigned launch[2]) {
    using namespace rtad;
    if (!rt_ad_rect_ok(w, h, x0, y0, tw, th, batch_spp, flags)) return -2;
    return rt_px_launch(rt_ad_merge_kernel, rt_px_frame_grid(tw, th), stream, launch, w, x0, y0, tw, th, batch_spp, flags & RT_DN_KEEP_ALBEDO, sums, aov, acc);
}
/* the list itself (alignment, frame, no tile twice) is the caller's to check (rt_adaptive_plan.h: rt_ad_tiles_check); rec is device memory */
extern "C" int rt1w_internal_accum_merge_tiles_launch(uint32_t w, uint32_t h, uint32_t tile, const uint32_t* rec, uint32_t n, uint32_t batch_spp, uint32_t flags,
                                                      const double* sums, const double* aov, double* acc, hipStream_t stream, unsigned launch[2]) {
    using namespace rtad;
    if (!rt_ad_rect_ok(w, h, 0u, 0u, 1u, 1u, batch_spp, flags) || !rt_ad_tile_ok(tile) || n < 1u || n > RT_AD_TILES_MAX) return -2;
    return rt_px_launch(rt_ad_merge_tiles_kernel, rt_px_list_grid(tile, n), stream, launch, w, h, tile, rec, batch_spp, flags & RT_DN_KEEP_ALBEDO, sums, aov, acc);
}
extern "C" int rt1w_internal_accum_resolve_launch(uint32_t w, uint32_t h, uint32_t batch_spp, const double* acc, double* frame, double* var,
                                                  double* spp, hipStream_t stream, unsigned launch[2]) {
    using namespace rtad;
    if (!rt_ad_frame_ok(w, h) || batch_spp == 0u) return -2;
    return rt_px_launch(rt_ad_resolve_kernel, rt_px_frame_grid(w, h), stream, launch, w, h, batch_spp, acc, frame, var, spp);
}
extern "C" int rt1w_internal_halves_resolve_launch(uint32_t w, uint32_t h, uint32_t batch_spp, const double* acc_a, const double* acc_b, double* frame,
                                                   double* var, double* half_a, double* half_b, double* spp, hipStream_t stream, unsigned launch[2]) {
    using namespace rtad;
    if (!rt_ad_frame_ok(w, h) || batch_spp == 0u) return -2;
    return rt_px_launch(rt_ad_halves_resolve_kernel, rt_px_frame_grid(w, h), stream, launch, w, h, batch_spp, acc_a, acc_b, frame, var, half_a, half_b, spp);
}
/* from_map 0: in = the accumulator (rt1w_accum_tile_error); 1: in = a per-pixel map (rt1w_tile_error_map) */
static int rt_ad_tile_error_launch(uint32_t w, uint32_t h, uint32_t tile, bool from_map, const double* in, double* err, hipStream_t stream, unsigned launch[2]) {
    using namespace rtad;
    if (!rt_ad_frame_ok(w, h) || !rt_ad_tile_ok(tile)) return -2;
    const unsigned grid = ((w + tile - 1u) / tile) * ((h + tile - 1u) / tile); /* one workgroup per tile */
    return rt_px_launch(from_map ? rt_ad_tile_error_kernel<true> : rt_ad_tile_error_kernel<false>, grid, stream, launch, w, h, tile, in, err);
}
extern "C" int rt1w_internal_accum_tile_error_launch(uint32_t w, uint32_t h, uint32_t tile, const double* acc, double* err, hipStream_t stream,
                                                     unsigned launch[2]) {
    return rt_ad_tile_error_launch(w, h, tile, false, acc, err, stream, launch);
}
extern "C" int rt1w_internal_tile_error_map_launch(uint32_t w, uint32_t h, uint32_t tile, const double* err_px, double* err, hipStream_t stream,
                                                   unsigned launch[2]) {
    return rt_ad_tile_error_launch(w, h, tile, true, err_px, err, stream, launch);
}
