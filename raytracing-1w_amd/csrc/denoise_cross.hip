/* denoise_cross.hip -- the kernels of rt1w_denoise_cross (include/rt1w.h) over rt_denoise_cross.h: the two half buffers of a frame, each
 * filtered with the colour term of the other, a prepare pass and one launch per a-trous level; the last level writes the mean of the two
 * filtered halves and the per-pixel error of that frame.
 *
 * A unit of its own, inside its own namespace (the pattern of denoise_halves.hip), so that no other code object moves with it: the kernels
 * of rt1w_denoise_var and rt1w_denoise_var_halves stay the build they were.  The host half is in features.hip, which calls the launcher
 * below.
 *
 * The kernels are the skeleton of rt_atrous_kernels.h over RtDcFilter: an 80-byte colour record (a half's colour, luminance and
 * variance, twice), so 15 planes in the staged tile (step 1: 48 000 B, step 2: 69 120 B of LDS; 160 KiB per CU hold 3 / 2 such
 * workgroups).  RT_DC_STAGED_LEVELS is how many leading levels run staged (0 .. 2; DESIGN.md section 18 has the measurement behind the
 * default). */
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
#include "rt_atrous_kernels.h"

__global__ __launch_bounds__(RT_PX_WG) void rt_dc_prepare_kernel(RtDnParams P, const double* __restrict__ frame, const double* __restrict__ aov,
                                                                     const double* __restrict__ var, const double* __restrict__ half_a,
                                                                     const double* __restrict__ half_b, RtDcCol* __restrict__ col,
                                                                     RtDnGuide* __restrict__ guide) {
    rt_at_prepare<RtDcFilter>(P, col, guide, frame, aov, var, half_a, half_b);
}
template <int STEP>
__global__ __launch_bounds__(RT_PX_WG) void rt_dc_level_kernel(RtDnParams P, double sv2, uint32_t level, const RtDcCol* __restrict__ src,
                                                                   const RtDnGuide* __restrict__ guide, RtDcCol* __restrict__ dst, double* __restrict__ out,
                                                                   double* __restrict__ err_px) {
    rt_at_level<RtDcFilter, STEP>(P, sv2, level, src, guide, dst, out, err_px);
}
} // namespace rtdc

/* called by features.hip.  Enqueues the prepare pass and the levels on `stream`, one after another: frame + aov + var + half_a + half_b
 * -> col_a, guide; the levels ping-pong col_a / col_b; the last one writes `out` (which may be `frame`: the prepare pass has consumed
 * it) and err_px.  col_a, col_b hold w * h records of rt1w_internal_denoise_cross_sizeof() bytes, guide of
 * rt1w_internal_denoise_sizeof(1).  0, -1 (launch failure) or -2 (parameters refused). */
extern "C" int rt1w_internal_denoise_cross_launch(uint32_t w, uint32_t h, uint32_t iterations, uint32_t flags, double sigma_normal, double sigma_depth,
                                                  double sigma_variance, const double* frame, const double* aov, const double* var,
                                                  const double* half_a, const double* half_b, double* out, double* err_px, void* col_a,
                                                  void* col_b, void* guide, hipStream_t stream, unsigned launch[2]) {
    using namespace rtdc;
    RtDnParams P;
    double sv;
    if (!rt_dn_make_params(w, h, iterations, flags, 0.0, sigma_normal, sigma_depth, P) || !rt_dv_sigma(sigma_variance, sv)) return -2;
    const double sv2 = sv * sv;
    RtDnGuide* g = (RtDnGuide*)guide;
    return rt_at_enqueue<RtDcCol>(
        P, (1u << RT_DC_STAGED_LEVELS) - 1u, col_a, col_b, launch, /* the leading RT_DC_STAGED_LEVELS levels staged */
        [&](dim3 grid, dim3 block, RtDcCol* col) { hipLaunchKernelGGL(rt_dc_prepare_kernel, grid, block, 0, stream, P, frame, aov, var, half_a, half_b, col, g); },
        [&](int step, dim3 grid, dim3 block, uint32_t level, const RtDcCol* src, RtDcCol* dst, bool last) {
            hipLaunchKernelGGL(step == 1 ? rt_dc_level_kernel<1> : (step == 2 ? rt_dc_level_kernel<2> : rt_dc_level_kernel<0>), grid, block, 0, stream, P,
                               sv2, level, src, (const RtDnGuide*)g, dst, last ? out : nullptr, err_px);
        });
}
extern "C" unsigned rt1w_internal_denoise_cross_sizeof(void) { return (unsigned)sizeof(rtdc::RtDcCol); }
