/* denoise_var.hip -- the kernels of rt1w_batch_variance and rt1w_denoise_var (include/rt1w.h) over rt_denoise_var.h: the batch-variance
 * pass, a prepare pass and one launch per a-trous level.
 *
 * A unit of its own, inside its own namespace (the pattern of denoise.hip), so that neither the render kernels' nor the fixed-sigma
 * filter's code objects move with it.  The host half is in features.hip, which calls the two launchers below.
 *
 * Work mapping: that of denoise.hip -- one lane per pixel, an 8 x 8 pixel block per wave, 2 x 2 blocks (16 x 16 pixels) per workgroup of
 * 256 lanes, every output pixel computed whole by one lane in the fixed order of rt_denoise_var.h: no atomics, the same bits as the CPU
 * twin (denoise_host.cpp).  The colour record is 40 bytes (demodulated rgb, luminance, variance), the guide record denoise.hip's 64.
 *
 * Two forms of the level kernel.  Staged (steps 1 and 2): the workgroup copies its tile plus the 2-step halo, (16 + 4 step)^2 pixels x 10
 * doubles as struct-of-arrays (32 000 / 46 080 B of LDS), then every tap is an LDS read.  Direct (any step): the 25 taps of a wave are
 * 25 8 x 8 blocks, read from memory through L2.  The choice by level is denoise.hip's (DESIGN.md section 13 has its measurement). */
#include <hip/hip_runtime.h>
#include "rt_feature_launch.h" /* this unit's functions as features.hip calls them: the definitions below are held to it */
#include <stdint.h>
#include <string.h>

namespace rtdv {
#include "rt1w_num.h"
#include "rt_denoise_var.h"

#define RT_DV_BLOCK 256
#define RT_DV_TILE 16u

/* pixel of this lane: 8 x 8 block per wave, 2 x 2 waves per workgroup, workgroups in row order over the image */
__device__ __forceinline__ void rt_dv_lane_pixel(uint32_t w, uint32_t& tx, uint32_t& ty, uint32_t& x, uint32_t& y) {
    const uint32_t tiles_x = (w + RT_DV_TILE - 1u) / RT_DV_TILE;
    tx = blockIdx.x % tiles_x; ty = blockIdx.x / tiles_x;
    const uint32_t wv = threadIdx.x >> 6, in = threadIdx.x & 63u;
    x = tx * RT_DV_TILE + (wv & 1u) * 8u + (in & 7u);
    y = ty * RT_DV_TILE + (wv >> 1) * 8u + (in >> 3);
}

/* sums[K][h][w][3], aov[h][w][8] -> frame[h][w][3], var[h][w] */
__global__ __launch_bounds__(RT_DV_BLOCK) void rt_dv_variance_kernel(uint32_t w, uint32_t h, uint32_t batches, uint32_t batch_spp, uint32_t keep_albedo,
                                                                      const double* __restrict__ sums, const double* __restrict__ aov,
                                                                      double* __restrict__ frame, double* __restrict__ var) {
    uint32_t tx, ty, x, y;
    rt_dv_lane_pixel(w, tx, ty, x, y);
    if (x >= w || y >= h) return;
    const unsigned long long i = (unsigned long long)y * w + x;
    double f[3], v;
    rt_dv_variance_pixel(batches, batch_spp, keep_albedo != 0u, sums + i * 3u, (unsigned long long)w * h * 3u, aov + i * 8u, f, &v);
    frame[i * 3u] = f[0]; frame[i * 3u + 1u] = f[1]; frame[i * 3u + 2u] = f[2];
    var[i] = v;
}

__global__ __launch_bounds__(RT_DV_BLOCK) void rt_dv_prepare_kernel(RtDnParams P, const double* __restrict__ frame, const double* __restrict__ aov,
                                                                     const double* __restrict__ var, RtDvCol* __restrict__ col,
                                                                     RtDnGuide* __restrict__ guide) {
    uint32_t tx, ty, x, y;
    rt_dv_lane_pixel(P.w, tx, ty, x, y);
    if (x >= P.w || y >= P.h) return;
    const unsigned long long i = (unsigned long long)y * P.w + x;
    RtDvCol c;
    RtDnGuide g;
    rt_dv_prepare_pixel(P, frame + i * 3u, aov + i * 8u, var[i], c, g);
    col[i] = c;
    guide[i] = g;
}

/* the staged tile: 10 planes of T x T doubles, origin (ox, oy) in the image; only pixels inside the image are filled and only those are read */
template <int T>
struct RtDvLdsSrc {
    const double* t;
    long long ox, oy;
    __device__ __forceinline__ int at(uint32_t x, uint32_t y) const { return (int)((long long)y - oy) * T + (int)((long long)x - ox); }
    __device__ __forceinline__ RtDvCol col(uint32_t x, uint32_t y) const {
        const int i = at(x, y);
        RtDvCol c;
        c.r = t[i]; c.g = t[T * T + i]; c.b = t[2 * T * T + i]; c.l = t[3 * T * T + i]; c.v = t[4 * T * T + i];
        return c;
    }
    __device__ __forceinline__ void guide(uint32_t x, uint32_t y, double o[5]) const {
        const int i = at(x, y);
        for (int k = 0; k < 5; ++k) o[k] = t[(5 + k) * T * T + i];
    }
};

/* STEP 0: direct form, any level.  STEP 1, 2: staged form of the level whose step it is.  out != nullptr: the last level */
template <int STEP>
__global__ __launch_bounds__(RT_DV_BLOCK) void rt_dv_level_kernel(RtDnParams P, double sv2, uint32_t level, const RtDvCol* __restrict__ src,
                                                                   const RtDnGuide* __restrict__ guide, RtDvCol* __restrict__ dst, double* __restrict__ out) {
    uint32_t tx, ty, x, y;
    rt_dv_lane_pixel(P.w, tx, ty, x, y);
    const bool inside = x < P.w && y < P.h;
    RtDvCol c;
    if constexpr (STEP > 0) {
        constexpr int T = (int)RT_DV_TILE + 4 * STEP;
        __shared__ double tile[10 * T * T];
        const long long ox = (long long)tx * RT_DV_TILE - 2 * STEP, oy = (long long)ty * RT_DV_TILE - 2 * STEP;
        for (int i = (int)threadIdx.x; i < T * T; i += RT_DV_BLOCK) {
            const long long gx = ox + i % T, gy = oy + i / T;
            if (gx < 0 || gy < 0 || gx >= (long long)P.w || gy >= (long long)P.h) continue;
            const unsigned long long q = (unsigned long long)gy * P.w + (unsigned long long)gx;
            const RtDvCol cq = src[q];
            const RtDnGuide* gq = guide + q;
            tile[i] = cq.r; tile[T * T + i] = cq.g; tile[2 * T * T + i] = cq.b; tile[3 * T * T + i] = cq.l; tile[4 * T * T + i] = cq.v;
            tile[5 * T * T + i] = gq->nx; tile[6 * T * T + i] = gq->ny; tile[7 * T * T + i] = gq->nz;
            tile[8 * T * T + i] = gq->z; tile[9 * T * T + i] = gq->v;
        }
        __syncthreads();
        if (!inside) return;
        const RtDvLdsSrc<T> s{tile, ox, oy};
        c = rt_dv_level_pixel(P, sv2, s, x, y, level);
    } else {
        if (!inside) return;
        const RtDvGlobalSrc s{src, guide, P.w};
        c = rt_dv_level_pixel(P, sv2, s, x, y, level);
    }
    const unsigned long long i = (unsigned long long)y * P.w + x;
    if (out) rt_dv_finish_pixel(c, guide[i], out + i * 3u);
    else dst[i] = c;
}

__host__ unsigned rt_dv_grid(uint32_t w, uint32_t h) { return ((w + RT_DV_TILE - 1u) / RT_DV_TILE) * ((h + RT_DV_TILE - 1u) / RT_DV_TILE); }
} // namespace rtdv

/* called by features.hip.  Enqueues the batch-variance pass on `stream`: sums[batches][h][w][3] + aov -> frame, var.  launch[0..1] = grid,
 * block.  0, -1 (launch failure) or -2 (parameters refused). */
extern "C" int rt1w_internal_batch_variance_launch(uint32_t w, uint32_t h, uint32_t batches, uint32_t batch_spp, uint32_t flags, const double* sums,
                                                   const double* aov, double* frame, double* var, hipStream_t stream, unsigned launch[2]) {
    using namespace rtdv;
    RtDnParams P;
    if (!rt_dn_make_params(w, h, 0u, flags, 0.0, 0.0, 0.0, P) || !rt_dv_batches_ok(batches, batch_spp)) return -2;
    const unsigned grid = rt_dv_grid(w, h);
    launch[0] = grid; launch[1] = RT_DV_BLOCK;
    hipLaunchKernelGGL(rt_dv_variance_kernel, dim3(grid), dim3(RT_DV_BLOCK), 0, stream, w, h, batches, batch_spp, P.keep_albedo, sums, aov, frame, var);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

/* called by features.hip.  Enqueues the prepare pass and the levels on `stream`, one after another: frame + aov + var -> col_a, guide; the
 * levels ping-pong col_a / col_b; the last one writes `out` (which may be `frame`: the prepare pass has consumed it).  col_a, col_b hold
 * w * h records of rt1w_internal_denoise_var_sizeof() bytes, guide of rt1w_internal_denoise_sizeof(1).  Same returns. */
extern "C" int rt1w_internal_denoise_var_launch(uint32_t w, uint32_t h, uint32_t iterations, uint32_t flags, double sigma_normal, double sigma_depth,
                                                double sigma_variance, const double* frame, const double* aov, const double* var, double* out,
                                                void* col_a, void* col_b, void* guide, hipStream_t stream, unsigned launch[2]) {
    using namespace rtdv;
    RtDnParams P;
    double sv;
    if (!rt_dn_make_params(w, h, iterations, flags, 0.0, sigma_normal, sigma_depth, P) || !rt_dv_sigma(sigma_variance, sv)) return -2;
    const double sv2 = sv * sv;
    const unsigned grid = rt_dv_grid(P.w, P.h);
    launch[0] = grid; launch[1] = RT_DV_BLOCK;
    RtDvCol* src = (RtDvCol*)col_a;
    RtDvCol* dst = (RtDvCol*)col_b;
    const RtDnGuide* g = (const RtDnGuide*)guide;
    hipLaunchKernelGGL(rt_dv_prepare_kernel, dim3(grid), dim3(RT_DV_BLOCK), 0, stream, P, frame, aov, var, src, (RtDnGuide*)guide);
    for (uint32_t level = 0; level < P.levels; ++level) {
        double* o = level + 1u == P.levels ? out : nullptr;
        if (level == 0u) hipLaunchKernelGGL(rt_dv_level_kernel<1>, dim3(grid), dim3(RT_DV_BLOCK), 0, stream, P, sv2, level, src, g, dst, o);
        else if (level == 1u) hipLaunchKernelGGL(rt_dv_level_kernel<2>, dim3(grid), dim3(RT_DV_BLOCK), 0, stream, P, sv2, level, src, g, dst, o);
        else hipLaunchKernelGGL(rt_dv_level_kernel<0>, dim3(grid), dim3(RT_DV_BLOCK), 0, stream, P, sv2, level, src, g, dst, o);
        RtDvCol* t = src; src = dst; dst = t;
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
extern "C" unsigned rt1w_internal_denoise_var_sizeof(void) { return (unsigned)sizeof(rtdv::RtDvCol); }
