/* denoise_var.hip -- the kernels of rt1w_batch_variance and rt1w_denoise_var (include/rt1w.h) over rt_denoise_var.h: the batch-variance
 * pass, a prepare pass and one launch per a-trous level.
 *
 * A unit of its own, inside its own namespace (the pattern of denoise.hip), so that neither the render kernels' nor the fixed-sigma
 * filter's code objects move with it.  The host half is in features.hip, which calls the two launchers below.
 *
 * The filter's kernels are the skeleton of rt_atrous_kernels.h over RtDvFilter: a 40-byte colour record (demodulated rgb, luminance,
 * variance), so 10 planes in the staged tile (32 000 / 46 080 B of LDS); levels 0 and 1 run staged, denoise.hip's choice (DESIGN.md
 * section 13 has its measurement).  The batch-variance pass has the skeleton's work mapping: one lane per pixel. */
#include <hip/hip_runtime.h>
#include "rt_feature_launch.h" /* this unit's functions as features.hip calls them: the definitions below are held to it */
#include <stdint.h>
#include <string.h>

namespace rtdv {
#include "rt1w_num.h"
#include "rt_denoise_var.h"
#include "rt_atrous_kernels.h"

/* sums[K][h][w][3], aov[h][w][8] -> frame[h][w][3], var[h][w] */
__global__ __launch_bounds__(RT_PX_WG) void rt_dv_variance_kernel(uint32_t w, uint32_t h, uint32_t batches, uint32_t batch_spp, uint32_t keep_albedo,
                                                                      const double* __restrict__ sums, const double* __restrict__ aov,
                                                                      double* __restrict__ frame, double* __restrict__ var) {
    uint32_t x, y;
    rt_px_lane_pixel(w, x, y);
    if (x >= w || y >= h) return;
    const unsigned long long i = (unsigned long long)y * w + x;
    double f[3], v;
    rt_dv_variance_pixel(batches, batch_spp, keep_albedo != 0u, sums + i * 3u, (unsigned long long)w * h * 3u, aov + i * 8u, f, &v);
    frame[i * 3u] = f[0]; frame[i * 3u + 1u] = f[1]; frame[i * 3u + 2u] = f[2];
    var[i] = v;
}

__global__ __launch_bounds__(RT_PX_WG) void rt_dv_prepare_kernel(RtDnParams P, const double* __restrict__ frame, const double* __restrict__ aov,
                                                                     const double* __restrict__ var, RtDvCol* __restrict__ col,
                                                                     RtDnGuide* __restrict__ guide) {
    rt_at_prepare<RtDvFilter>(P, col, guide, frame, aov, var);
}
template <int STEP>
__global__ __launch_bounds__(RT_PX_WG) void rt_dv_level_kernel(RtDnParams P, double sv2, uint32_t level, const RtDvCol* __restrict__ src,
                                                                   const RtDnGuide* __restrict__ guide, RtDvCol* __restrict__ dst, double* __restrict__ out) {
    rt_at_level<RtDvFilter, STEP>(P, sv2, level, src, guide, dst, out, nullptr);
}
} // namespace rtdv

/* called by features.hip.  Enqueues the batch-variance pass on `stream`: sums[batches][h][w][3] + aov -> frame, var.  launch[0..1] = grid,
 * block.  0, -1 (launch failure) or -2 (parameters refused). */
extern "C" int rt1w_internal_batch_variance_launch(uint32_t w, uint32_t h, uint32_t batches, uint32_t batch_spp, uint32_t flags, const double* sums,
                                                   const double* aov, double* frame, double* var, hipStream_t stream, unsigned launch[2]) {
    using namespace rtdv;
    RtDnParams P;
    if (!rt_dn_make_params(w, h, 0u, flags, 0.0, 0.0, 0.0, P) || !rt_dv_batches_ok(batches, batch_spp)) return -2;
    return rt_px_launch(rt_dv_variance_kernel, rt_px_frame_grid(w, h), stream, launch, w, h, batches, batch_spp, P.keep_albedo, sums, aov, frame, var);
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
    RtDnGuide* g = (RtDnGuide*)guide;
    return rt_at_enqueue<RtDvCol>(
        P, 3u, col_a, col_b, launch,
        [&](dim3 grid, dim3 block, RtDvCol* col) { hipLaunchKernelGGL(rt_dv_prepare_kernel, grid, block, 0, stream, P, frame, aov, var, col, g); },
        [&](int step, dim3 grid, dim3 block, uint32_t level, const RtDvCol* src, RtDvCol* dst, bool last) {
            hipLaunchKernelGGL(step == 1 ? rt_dv_level_kernel<1> : (step == 2 ? rt_dv_level_kernel<2> : rt_dv_level_kernel<0>), grid, block, 0, stream, P,
                               sv2, level, src, (const RtDnGuide*)g, dst, last ? out : nullptr);
        });
}
extern "C" unsigned rt1w_internal_denoise_var_sizeof(void) { return (unsigned)sizeof(rtdv::RtDvCol); }
