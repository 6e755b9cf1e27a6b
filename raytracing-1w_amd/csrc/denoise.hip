/* denoise.hip -- the filter kernels of rt1w_denoise (include/rt1w.h): a prepare pass and one launch per a-trous level over rt_denoise.h.
 *
 * Kept out of context.hip, inside its own namespace (the pattern of aov.hip), so that none of the render kernels' code objects and none
 * of the run-time compiler's inputs moves with it.  The host half (validation, buffers, timing, copies) is in features.hip, which calls
 * the launcher below.
 *
 * Work mapping: one lane per pixel, an 8 x 8 pixel block per wave, 2 x 2 blocks (16 x 16 pixels) per workgroup of 256 lanes.  Every
 * output pixel is computed whole by one lane in the fixed tap order of rt_dn_level_pixel: no atomics, the same bits as the CPU twin
 * (denoise_host.cpp).  The prepare pass turns frame and feature buffers into what the levels read: a 32-byte colour record
 * (demodulated rgb and its luminance) and a 64-byte guide record (unit normal, depth, coverage, albedo), both f64.  A level reads
 * the colour records of the previous one and writes its own (two buffers, ping-pong); the last level multiplies the albedo back and
 * writes the caller's rgb.
 *
 * Two forms of the level kernel.  Staged (steps 1 and 2): the workgroup copies its tile plus the 2-step halo, (16 + 4 step)^2 pixels x 9
 * doubles as struct-of-arrays (28.8 / 41.5 KB of LDS), then every tap is an LDS read.  Direct (any step): the 25 taps of a wave are 25
 * 8 x 8 blocks, read from memory through L2.  RT_DENOISE_LDS_MASK, bit `level`, says which levels run staged; DESIGN.md section 13 has
 * the measurement behind the default. */
#include <hip/hip_runtime.h>
#include "rt_feature_launch.h" /* this unit's functions as features.hip calls them: the definitions below are held to it */
#include <stdint.h>
#include <string.h>

namespace rtdn {
#include "rt1w_num.h"
#include "rt_denoise.h"

#ifndef RT_DENOISE_LDS_MASK
#define RT_DENOISE_LDS_MASK 3u /* levels 0 and 1 (steps 1 and 2) staged in LDS; only bits 0 and 1 are honoured */
#endif
#define RT_DN_BLOCK 256
#define RT_DN_TILE 16u

/* pixel of this lane: 8 x 8 block per wave, 2 x 2 waves per workgroup, workgroups in row order over the image */
__device__ __forceinline__ void rt_dn_lane_pixel(const RtDnParams& P, uint32_t& tx, uint32_t& ty, uint32_t& x, uint32_t& y) {
    const uint32_t tiles_x = (P.w + RT_DN_TILE - 1u) / RT_DN_TILE;
    tx = blockIdx.x % tiles_x; ty = blockIdx.x / tiles_x;
    const uint32_t wv = threadIdx.x >> 6, in = threadIdx.x & 63u;
    x = tx * RT_DN_TILE + (wv & 1u) * 8u + (in & 7u);
    y = ty * RT_DN_TILE + (wv >> 1) * 8u + (in >> 3);
}

__global__ __launch_bounds__(RT_DN_BLOCK) void rt_dn_prepare_kernel(RtDnParams P, const double* __restrict__ frame, const double* __restrict__ aov,
                                                                     RtDnCol* __restrict__ col, RtDnGuide* __restrict__ guide) {
    uint32_t tx, ty, x, y;
    rt_dn_lane_pixel(P, tx, ty, x, y);
    if (x >= P.w || y >= P.h) return;
    const unsigned long long i = (unsigned long long)y * P.w + x;
    RtDnCol c;
    RtDnGuide g;
    rt_dn_prepare_pixel(P, frame + i * 3u, aov + i * 8u, c, g);
    col[i] = c;
    guide[i] = g;
}

/* the staged tile: 9 planes of T x T doubles, origin (ox, oy) in the image; only pixels inside the image are filled and only those are read */
template <int T>
struct RtDnLdsSrc {
    const double* t;
    long long ox, oy;
    __device__ __forceinline__ int at(uint32_t x, uint32_t y) const { return (int)((long long)y - oy) * T + (int)((long long)x - ox); }
    __device__ __forceinline__ RtDnCol col(uint32_t x, uint32_t y) const {
        const int i = at(x, y);
        RtDnCol c;
        c.r = t[i]; c.g = t[T * T + i]; c.b = t[2 * T * T + i]; c.l = t[3 * T * T + i];
        return c;
    }
    __device__ __forceinline__ void guide(uint32_t x, uint32_t y, double o[5]) const {
        const int i = at(x, y);
        for (int k = 0; k < 5; ++k) o[k] = t[(4 + k) * T * T + i];
    }
};

/* STEP 0: direct form, any level.  STEP 1, 2: staged form of the level whose step it is.  out != nullptr: the last level */
template <int STEP>
__global__ __launch_bounds__(RT_DN_BLOCK) void rt_dn_level_kernel(RtDnParams P, uint32_t level, const RtDnCol* __restrict__ src,
                                                                   const RtDnGuide* __restrict__ guide, RtDnCol* __restrict__ dst, double* __restrict__ out) {
    uint32_t tx, ty, x, y;
    rt_dn_lane_pixel(P, tx, ty, x, y);
    const bool inside = x < P.w && y < P.h;
    RtDnCol c;
    if constexpr (STEP > 0) {
        constexpr int T = (int)RT_DN_TILE + 4 * STEP;
        __shared__ double tile[9 * T * T];
        const long long ox = (long long)tx * RT_DN_TILE - 2 * STEP, oy = (long long)ty * RT_DN_TILE - 2 * STEP;
        for (int i = (int)threadIdx.x; i < T * T; i += RT_DN_BLOCK) {
            const long long gx = ox + i % T, gy = oy + i / T;
            if (gx < 0 || gy < 0 || gx >= (long long)P.w || gy >= (long long)P.h) continue;
            const unsigned long long q = (unsigned long long)gy * P.w + (unsigned long long)gx;
            const RtDnCol cq = src[q];
            const RtDnGuide* gq = guide + q;
            tile[i] = cq.r; tile[T * T + i] = cq.g; tile[2 * T * T + i] = cq.b; tile[3 * T * T + i] = cq.l;
            tile[4 * T * T + i] = gq->nx; tile[5 * T * T + i] = gq->ny; tile[6 * T * T + i] = gq->nz;
            tile[7 * T * T + i] = gq->z; tile[8 * T * T + i] = gq->v;
        }
        __syncthreads();
        if (!inside) return;
        const RtDnLdsSrc<T> s{tile, ox, oy};
        c = rt_dn_level_pixel(P, s, x, y, level);
    } else {
        if (!inside) return;
        const RtDnGlobalSrc s{src, guide, P.w};
        c = rt_dn_level_pixel(P, s, x, y, level);
    }
    const unsigned long long i = (unsigned long long)y * P.w + x;
    if (out) rt_dn_finish_pixel(c, guide[i], out + i * 3u);
    else dst[i] = c;
}
} // namespace rtdn

/* called by context.hip.  Enqueues the prepare pass and the levels on `stream`, one after another: frame + aov -> col_a, guide; the levels
 * ping-pong col_a / col_b; the last one writes `out` (which may be `frame`: the prepare pass has consumed it).  col_a, col_b hold
 * w * h records of rt1w_internal_denoise_sizeof(0) bytes, guide of rt1w_internal_denoise_sizeof(1).  launch[0..1] = grid, block of the
 * level kernel.  0, -1 (launch failure) or -2 (parameters refused). */
extern "C" int rt1w_internal_denoise_launch(uint32_t w, uint32_t h, uint32_t iterations, uint32_t flags, double sigma_colour, double sigma_normal,
                                            double sigma_depth, const double* frame, const double* aov, double* out, void* col_a, void* col_b,
                                            void* guide, hipStream_t stream, unsigned launch[2]) {
    using namespace rtdn;
    RtDnParams P;
    if (!rt_dn_make_params(w, h, iterations, flags, sigma_colour, sigma_normal, sigma_depth, P)) return -2;
    const unsigned grid = ((P.w + RT_DN_TILE - 1u) / RT_DN_TILE) * ((P.h + RT_DN_TILE - 1u) / RT_DN_TILE);
    launch[0] = grid; launch[1] = RT_DN_BLOCK;
    RtDnCol* src = (RtDnCol*)col_a;
    RtDnCol* dst = (RtDnCol*)col_b;
    const RtDnGuide* g = (const RtDnGuide*)guide;
    hipLaunchKernelGGL(rt_dn_prepare_kernel, dim3(grid), dim3(RT_DN_BLOCK), 0, stream, P, frame, aov, src, (RtDnGuide*)guide);
    for (uint32_t level = 0; level < P.levels; ++level) {
        double* o = level + 1u == P.levels ? out : nullptr;
        const bool staged = level < 2u && ((RT_DENOISE_LDS_MASK >> level) & 1u);
        if (staged && level == 0u) hipLaunchKernelGGL(rt_dn_level_kernel<1>, dim3(grid), dim3(RT_DN_BLOCK), 0, stream, P, level, src, g, dst, o);
        else if (staged) hipLaunchKernelGGL(rt_dn_level_kernel<2>, dim3(grid), dim3(RT_DN_BLOCK), 0, stream, P, level, src, g, dst, o);
        else hipLaunchKernelGGL(rt_dn_level_kernel<0>, dim3(grid), dim3(RT_DN_BLOCK), 0, stream, P, level, src, g, dst, o);
        RtDnCol* t = src; src = dst; dst = t;
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
extern "C" unsigned rt1w_internal_denoise_sizeof(int what) { return what == 0 ? (unsigned)sizeof(rtdn::RtDnCol) : (unsigned)sizeof(rtdn::RtDnGuide); }
