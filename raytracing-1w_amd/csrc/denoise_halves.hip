/* denoise_halves.hip -- the kernels of rt1w_denoise_var_halves (include/rt1w.h) over rt_denoise_halves.h: the variance-guided filter of
 * denoise_var.hip carrying the two half buffers of the frame through its weights, a prepare pass and one launch per a-trous level; the
 * last level writes the filtered frame and the per-pixel error of the filtered frame.
 *
 * A unit of its own, inside its own namespace (the pattern of denoise_var.hip), so that no other code object moves with it: the kernels
 * of rt1w_denoise_var stay the build they were.  The host half is in features.hip, which calls the launcher below.
 *
 * The kernels are the skeleton of rt_atrous_kernels.h over RtDhFilter: an 88-byte colour record (RtDvCol's five doubles, then the two
 * demodulated halves), so 16 planes in the staged tile -- the record's eleven in its field order, then the guide's five (step 1:
 * 51 200 B, step 2: 73 728 B of LDS; 160 KiB per CU hold 3 / 2 such workgroups).  RT_DH_STAGED_LEVELS is how many leading levels run
 * staged (0 .. 2; DESIGN.md section 17 has the measurement behind the default). */
#include <hip/hip_runtime.h>
#include "rt_feature_launch.h" /* this unit's functions as features.hip calls them: the definitions below are held to it */
#include <stdint.h>
#include <string.h>

#ifndef RT_DH_STAGED_LEVELS
#define RT_DH_STAGED_LEVELS 2
#endif

namespace rtdh {
#include "rt1w_num.h"
#include "rt_denoise_halves.h"
#include "rt_atrous_kernels.h"

__global__ __launch_bounds__(RT_PX_WG) void rt_dh_prepare_kernel(RtDnParams P, const double* __restrict__ frame, const double* __restrict__ aov,
                                                                     const double* __restrict__ var, const double* __restrict__ half_a,
                                                                     const double* __restrict__ half_b, RtDhCol* __restrict__ col,
                                                                     RtDnGuide* __restrict__ guide) {
    rt_at_prepare<RtDhFilter>(P, col, guide, frame, aov, var, half_a, half_b);
}
template <int STEP>
__global__ __launch_bounds__(RT_PX_WG) void rt_dh_level_kernel(RtDnParams P, double sv2, uint32_t level, const RtDhCol* __restrict__ src,
                                                                   const RtDnGuide* __restrict__ guide, RtDhCol* __restrict__ dst, double* __restrict__ out,
                                                                   double* __restrict__ err_px) {
    rt_at_level<RtDhFilter, STEP>(P, sv2, level, src, guide, dst, out, err_px);
}
} // namespace rtdh

/* called by features.hip.  Enqueues the prepare pass and the levels on `stream`, one after another: frame + aov + var + half_a + half_b
 * -> col_a, guide; the levels ping-pong col_a / col_b; the last one writes `out` (which may be `frame`: the prepare pass has consumed
 * it) and err_px.  col_a, col_b hold w * h records of rt1w_internal_denoise_var_halves_sizeof() bytes, guide of
 * rt1w_internal_denoise_sizeof(1).  0, -1 (launch failure) or -2 (parameters refused). */
extern "C" int rt1w_internal_denoise_var_halves_launch(uint32_t w, uint32_t h, uint32_t iterations, uint32_t flags, double sigma_normal, double sigma_depth,
                                                       double sigma_variance, const double* frame, const double* aov, const double* var,
                                                       const double* half_a, const double* half_b, double* out, double* err_px, void* col_a,
                                                       void* col_b, void* guide, hipStream_t stream, unsigned launch[2]) {
    using namespace rtdh;
    RtDnParams P;
    double sv;
    if (!rt_dn_make_params(w, h, iterations, flags, 0.0, sigma_normal, sigma_depth, P) || !rt_dv_sigma(sigma_variance, sv)) return -2;
    const double sv2 = sv * sv;
    RtDnGuide* g = (RtDnGuide*)guide;
    return rt_at_enqueue<RtDhCol>(
        P, (1u << RT_DH_STAGED_LEVELS) - 1u, col_a, col_b, launch, /* the leading RT_DH_STAGED_LEVELS levels staged */
        [&](dim3 grid, dim3 block, RtDhCol* col) { hipLaunchKernelGGL(rt_dh_prepare_kernel, grid, block, 0, stream, P, frame, aov, var, half_a, half_b, col, g); },
        [&](int step, dim3 grid, dim3 block, uint32_t level, const RtDhCol* src, RtDhCol* dst, bool last) {
            hipLaunchKernelGGL(step == 1 ? rt_dh_level_kernel<1> : (step == 2 ? rt_dh_level_kernel<2> : rt_dh_level_kernel<0>), grid, block, 0, stream, P,
                               sv2, level, src, (const RtDnGuide*)g, dst, last ? out : nullptr, err_px);
        });
}
extern "C" unsigned rt1w_internal_denoise_var_halves_sizeof(void) { return (unsigned)sizeof(rtdh::RtDhCol); }
