/* denoise_cross.hip -- the kernels of rt1w_denoise_cross (include/rt1w.h) over rt_denoise_cross.h: the two half buffers of a frame, each
 * filtered with the colour term of the other, a prepare pass and one launch per a-trous level; the last level writes the mean of the two
 * filtered halves and the per-pixel error of that frame.
 *
 * A unit of its own, inside its own namespace (the pattern of denoise_halves.hip), so that no other code object moves with it: the kernels
 * of rt1w_denoise_var and rt1w_denoise_var_halves stay the build they were.  The host half is in features.hip, which calls the launcher
 * below.
 *
 * Work mapping: that of denoise_halves.hip -- one lane per pixel, an 8 x 8 pixel block per wave, 2 x 2 blocks (16 x 16 pixels) per
 * workgroup of 256 lanes, every output pixel computed whole by one lane in the fixed order of rt_denoise_cross.h: no atomics, the same bits
 * as the CPU twin (denoise_host.cpp).  The colour record is 80 bytes (a half's colour, luminance and variance, twice), the guide record
 * denoise.hip's 64.
 *
 * Two forms of the level kernel, as there.  Staged: the workgroup copies its tile plus the 2-step halo, (16 + 4 step)^2 pixels x 15
 * doubles as struct-of-arrays (step 1: 48 000 B, step 2: 69 120 B of LDS; 160 KiB per CU hold 3 / 2 such workgroups), then every tap is
 * an LDS read.  Direct (any step): the taps are read from memory through L2.  RT_DC_STAGED_LEVELS is how many leading levels run staged
 * (0 .. 2; DESIGN.md section 18 has the measurement behind the default). */
#include <hip/hip_runtime.h>
#include "rt_feature_launch.h" /* this unit's functions as features.hip calls them: the definitions below are held to it */
#include <stdint.h>
#include <string.h>

#ifndef RT_DC_STAGED_LEVELS
#define RT_DC_STAGED_LEVELS 2
#endif

namespace rtdc {
#include "rt1w_num.h"
#include "rt_denoise_cross.h"

#define RT_DC_BLOCK 256
#define RT_DC_TILE 16u
#define RT_DC_PLANES 15

/* pixel of this lane: 8 x 8 block per wave, 2 x 2 waves per workgroup, workgroups in row order over the image */
__device__ __forceinline__ void rt_dc_lane_pixel(uint32_t w, uint32_t& tx, uint32_t& ty, uint32_t& x, uint32_t& y) {
    const uint32_t tiles_x = (w + RT_DC_TILE - 1u) / RT_DC_TILE;
    tx = blockIdx.x % tiles_x; ty = blockIdx.x / tiles_x;
    const uint32_t wv = threadIdx.x >> 6, in = threadIdx.x & 63u;
    x = tx * RT_DC_TILE + (wv & 1u) * 8u + (in & 7u);
    y = ty * RT_DC_TILE + (wv >> 1) * 8u + (in >> 3);
}

__global__ __launch_bounds__(RT_DC_BLOCK) void rt_dc_prepare_kernel(RtDnParams P, const double* __restrict__ frame, const double* __restrict__ aov,
                                                                     const double* __restrict__ var, const double* __restrict__ half_a,
                                                                     const double* __restrict__ half_b, RtDcCol* __restrict__ col,
                                                                     RtDnGuide* __restrict__ guide) {
    uint32_t tx, ty, x, y;
    rt_dc_lane_pixel(P.w, tx, ty, x, y);
    if (x >= P.w || y >= P.h) return;
    const unsigned long long i = (unsigned long long)y * P.w + x;
    RtDcCol c;
    RtDnGuide g;
    rt_dc_prepare_pixel(P, frame + i * 3u, aov + i * 8u, var[i], half_a + i * 3u, half_b + i * 3u, c, g);
    col[i] = c;
    guide[i] = g;
}

/* the staged tile: 15 planes of T x T doubles -- colour record 0 .. 9, guide 10 .. 14 -- origin (ox, oy) in the image; only pixels inside
 * the image are filled and only those are read */
template <int T>
struct RtDcLdsSrc {
    const double* t;
    long long ox, oy;
    __device__ __forceinline__ int at(uint32_t x, uint32_t y) const { return (int)((long long)y - oy) * T + (int)((long long)x - ox); }
    __device__ __forceinline__ RtDcCol col(uint32_t x, uint32_t y) const {
        const int i = at(x, y);
        RtDcCol c;
        c.ar = t[i]; c.ag = t[T * T + i]; c.ab = t[2 * T * T + i]; c.la = t[3 * T * T + i]; c.va = t[4 * T * T + i];
        c.br = t[5 * T * T + i]; c.bg = t[6 * T * T + i]; c.bb = t[7 * T * T + i]; c.lb = t[8 * T * T + i]; c.vb = t[9 * T * T + i];
        return c;
    }
    __device__ __forceinline__ void guide(uint32_t x, uint32_t y, double o[5]) const {
        const int i = at(x, y);
        for (int k = 0; k < 5; ++k) o[k] = t[(10 + k) * T * T + i];
    }
};

/* STEP 0: direct form, any level.  STEP 1, 2: staged form of the level whose step it is.  out != nullptr: the last level */
template <int STEP>
__global__ __launch_bounds__(RT_DC_BLOCK) void rt_dc_level_kernel(RtDnParams P, double sv2, uint32_t level, const RtDcCol* __restrict__ src,
                                                                   const RtDnGuide* __restrict__ guide, RtDcCol* __restrict__ dst, double* __restrict__ out,
                                                                   double* __restrict__ err_px) {
    uint32_t tx, ty, x, y;
    rt_dc_lane_pixel(P.w, tx, ty, x, y);
    const bool inside = x < P.w && y < P.h;
    RtDcCol c;
    if constexpr (STEP > 0) {
        constexpr int T = (int)RT_DC_TILE + 4 * STEP;
        __shared__ double tile[RT_DC_PLANES * T * T];
        const long long ox = (long long)tx * RT_DC_TILE - 2 * STEP, oy = (long long)ty * RT_DC_TILE - 2 * STEP;
        for (int i = (int)threadIdx.x; i < T * T; i += RT_DC_BLOCK) {
            const long long gx = ox + i % T, gy = oy + i / T;
            if (gx < 0 || gy < 0 || gx >= (long long)P.w || gy >= (long long)P.h) continue;
            const unsigned long long q = (unsigned long long)gy * P.w + (unsigned long long)gx;
            const RtDcCol cq = src[q];
            const RtDnGuide* gq = guide + q;
            tile[i] = cq.ar; tile[T * T + i] = cq.ag; tile[2 * T * T + i] = cq.ab; tile[3 * T * T + i] = cq.la; tile[4 * T * T + i] = cq.va;
            tile[5 * T * T + i] = cq.br; tile[6 * T * T + i] = cq.bg; tile[7 * T * T + i] = cq.bb; tile[8 * T * T + i] = cq.lb; tile[9 * T * T + i] = cq.vb;
            tile[10 * T * T + i] = gq->nx; tile[11 * T * T + i] = gq->ny; tile[12 * T * T + i] = gq->nz;
            tile[13 * T * T + i] = gq->z; tile[14 * T * T + i] = gq->v;
        }
        __syncthreads();
        if (!inside) return;
        const RtDcLdsSrc<T> s{tile, ox, oy};
        c = rt_dc_level_pixel(P, sv2, s, x, y, level);
    } else {
        if (!inside) return;
        const RtDcGlobalSrc s{src, guide, P.w};
        c = rt_dc_level_pixel(P, sv2, s, x, y, level);
    }
    const unsigned long long i = (unsigned long long)y * P.w + x;
    if (out) rt_dc_finish_pixel(c, guide[i], out + i * 3u, err_px + i);
    else dst[i] = c;
}

__host__ unsigned rt_dc_grid(uint32_t w, uint32_t h) { return ((w + RT_DC_TILE - 1u) / RT_DC_TILE) * ((h + RT_DC_TILE - 1u) / RT_DC_TILE); }
} // namespace rtdc

/* called by features.hip.  Enqueues the prepare pass and the levels on `stream`, one after another: frame + aov + var + half_a + half_b
 * -> col_a, guide; the levels ping-pong col_a / col_b; the last one writes `out` (which may be `frame`: the prepare pass has consumed
 * it) and err_px.  col_a, col_b hold w * h records of rt1w_internal_denoise_cross_sizeof() bytes, guide of
 * rt1w_internal_denoise_sizeof(1).  0, -1 (launch failure) or -2 (parameters refused). */
extern "C" int rt1w_internal_denoise_cross_launch(uint32_t w, uint32_t h, uint32_t iterations, uint32_t flags, double sigma_normal, double sigma_depth,
                                                  double sigma_variance, const double* frame, const double* aov, const double* var,
                                                  const double* half_a, const double* half_b, double* out, double* err_px, void* col_a, void* col_b,
                                                  void* guide, hipStream_t stream, unsigned launch[2]) {
    using namespace rtdc;
    RtDnParams P;
    double sv;
    if (!rt_dn_make_params(w, h, iterations, flags, 0.0, sigma_normal, sigma_depth, P) || !rt_dv_sigma(sigma_variance, sv)) return -2;
    const double sv2 = sv * sv;
    const unsigned grid = rt_dc_grid(P.w, P.h);
    launch[0] = grid; launch[1] = RT_DC_BLOCK;
    RtDcCol* src = (RtDcCol*)col_a;
    RtDcCol* dst = (RtDcCol*)col_b;
    const RtDnGuide* g = (const RtDnGuide*)guide;
    hipLaunchKernelGGL(rt_dc_prepare_kernel, dim3(grid), dim3(RT_DC_BLOCK), 0, stream, P, frame, aov, var, half_a, half_b, src, (RtDnGuide*)guide);
    for (uint32_t level = 0; level < P.levels; ++level) {
        double* o = level + 1u == P.levels ? out : nullptr;
        if (level == 0u && RT_DC_STAGED_LEVELS >= 1) hipLaunchKernelGGL(rt_dc_level_kernel<1>, dim3(grid), dim3(RT_DC_BLOCK), 0, stream, P, sv2, level, src, g, dst, o, err_px);
        else if (level == 1u && RT_DC_STAGED_LEVELS >= 2) hipLaunchKernelGGL(rt_dc_level_kernel<2>, dim3(grid), dim3(RT_DC_BLOCK), 0, stream, P, sv2, level, src, g, dst, o, err_px);
        else hipLaunchKernelGGL(rt_dc_level_kernel<0>, dim3(grid), dim3(RT_DC_BLOCK), 0, stream, P, sv2, level, src, g, dst, o, err_px);
        RtDcCol* t = src; src = dst; dst = t;
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
extern "C" unsigned rt1w_internal_denoise_cross_sizeof(void) { return (unsigned)sizeof(rtdc::RtDcCol); }
