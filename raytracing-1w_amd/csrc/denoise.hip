/* denoise.hip -- the filter kernels of rt1w_denoise (include/rt1w.h): a prepare pass and one launch per a-trous level over rt_denoise.h.
 *
 * Kept out of context.hip, inside its own namespace (the pattern of aov.hip), so that none of the render kernels' code objects and none
 * of the run-time compiler's inputs moves with it.  The host half (validation, buffers, timing, copies) is in features.hip, which calls
 * the launcher below.
 *
 * The kernels are the skeleton of rt_atrous_kernels.h (work mapping, staged and direct form of the level kernel, enqueue loop) over
 * RtDnFilter: a 32-byte colour record (demodulated rgb and its luminance), so 9 planes in the staged tile (28 800 / 41 472 B of LDS).
 * RT_DENOISE_LDS_MASK, bit `level`, says which levels run staged; DESIGN.md section 13 has the measurement behind the default. */
#include <hip/hip_runtime.h>
#include "rt_feature_launch.h" /* this unit's functions as features.hip calls them: the definitions below are held to it */
#include <stdint.h>
#include <string.h>

#ifndef RT_DENOISE_LDS_MASK
#define RT_DENOISE_LDS_MASK 3u /* levels 0 and 1 (steps 1 and 2) staged in LDS; only bits 0 and 1 are honoured */
#endif

namespace rtdn {
#include "rt1w_num.h"
#include "rt_denoise.h"
#include "rt_atrous_kernels.h"

__global__ __launch_bounds__(RT_PX_WG) void rt_dn_prepare_kernel(RtDnParams P, const double* __restrict__ frame, const double* __restrict__ aov,
                                                                     RtDnCol* __restrict__ col, RtDnGuide* __restrict__ guide) {
    rt_at_prepare<RtDnFilter>(P, col, guide, frame, aov);
}
template <int STEP>
__global__ __launch_bounds__(RT_PX_WG) void rt_dn_level_kernel(RtDnParams P, uint32_t level, const RtDnCol* __restrict__ src,
                                                                   const RtDnGuide* __restrict__ guide, RtDnCol* __restrict__ dst, double* __restrict__ out) {
    rt_at_level<RtDnFilter, STEP>(P, 0.0, level, src, guide, dst, out, nullptr);
}
} // namespace rtdn

/* called by features.hip.  Enqueues the prepare pass and the levels on `stream`, one after another: frame + aov -> col_a, guide; the levels
 * ping-pong col_a / col_b; the last one writes `out` (which may be `frame`: the prepare pass has consumed it).  col_a, col_b hold
 * w * h records of rt1w_internal_denoise_sizeof(0) bytes, guide of rt1w_internal_denoise_sizeof(1).  launch[0..1] = grid, block of the
 * level kernel.  0, -1 (launch failure) or -2 (parameters refused). */
extern "C" int rt1w_internal_denoise_launch(uint32_t w, uint32_t h, uint32_t iterations, uint32_t flags, double sigma_colour, double sigma_normal,
                                            double sigma_depth, const double* frame, const double* aov, double* out, void* col_a, void* col_b,
                                            void* guide, hipStream_t stream, unsigned launch[2]) {
    using namespace rtdn;
    RtDnParams P;
    if (!rt_dn_make_params(w, h, iterations, flags, sigma_colour, sigma_normal, sigma_depth, P)) return -2;
    RtDnGuide* g = (RtDnGuide*)guide;
    return rt_at_enqueue<RtDnCol>(
        P, RT_DENOISE_LDS_MASK, col_a, col_b, launch,
        [&](dim3 grid, dim3 block, RtDnCol* col) { hipLaunchKernelGGL(rt_dn_prepare_kernel, grid, block, 0, stream, P, frame, aov, col, g); },
        [&](int step, dim3 grid, dim3 block, uint32_t level, const RtDnCol* src, RtDnCol* dst, bool last) {
            hipLaunchKernelGGL(step == 1 ? rt_dn_level_kernel<1> : (step == 2 ? rt_dn_level_kernel<2> : rt_dn_level_kernel<0>), grid, block, 0, stream, P,
                               level, src, (const RtDnGuide*)g, dst, last ? out : nullptr);
        });
}
extern "C" unsigned rt1w_internal_denoise_sizeof(int what) { return what == 0 ? (unsigned)sizeof(rtdn::RtDnCol) : (unsigned)sizeof(rtdn::RtDnGuide); }
