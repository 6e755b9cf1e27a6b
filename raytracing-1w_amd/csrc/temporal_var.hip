/* temporal_var.hip -- the kernels of rt1w_temporal_moments and rt1w_temporal_variance (include/rt1w.h): one launch each, over
 * rt_temporal.h and rt_temporal_var.h.
 *
 * A unit and a namespace of its own (the pattern of temporal.hip), so that no other code object moves with it.  The host half
 * (validation, buffers, timing, copies, the state of rt1w_render_temporal_var) is in features.hip, which calls the launchers below.
 *
 * Work mapping: that of rt_pixel_kernels.h, workgroups in row order over the image -- one lane per pixel, an 8 x 8 pixel block per wave,
 * 16 x 16 pixels per workgroup of 256 lanes.  Every output pixel is computed whole by one lane in a fixed order: no atomics, no LDS, the
 * same bits as the CPU twin (denoise_host.cpp).
 *   rt_tv_moments_kernel   rt_tm_pixel with the two m2 pointers: the accumulate kernel's gather plus one tap value, 256 B per pixel.
 *   rt_tv_variance_kernel  the direct form: a lane whose history is shorter than RT_TV_MIN_LEN walks the 7 x 7 window through global
 *                          memory (88 B per tap, neighbours' windows overlap in cache); every other lane reads its own 104 B and
 *                          leaves.  In a steady animation only disoccluded lanes enter the loop; on a first frame every lane does.
 * The build fails if a kernel uses scratch (Makefile: no_scratch_unit). */
#include <hip/hip_runtime.h>
#include "rt_feature_launch.h" /* this unit's functions as features.hip calls them: the definitions below are held to it */
#include <stdint.h>
#include <string.h>

namespace rttv {
#include "rt1w_num.h"
#include "rt_temporal_var.h"

#include "rt_pixel_kernels.h"

__global__ __launch_bounds__(RT_PX_WG) void rt_tv_moments_kernel(RtTmParams P, RtCamera cc, RtCamera pc, const double* __restrict__ cur_frame,
                                                                     const double* __restrict__ cur_aov, const double* __restrict__ prev_hist,
                                                                     const double* __restrict__ prev_m2, const double* __restrict__ prev_len,
                                                                     const double* __restrict__ prev_aov, double* __restrict__ hist,
                                                                     double* __restrict__ m2, double* __restrict__ len, double* __restrict__ frame_out) {
    uint32_t x, y;
    rt_px_lane_pixel(P.w, x, y);
    if (x >= P.w || y >= P.h) return;
    const unsigned long long i = (unsigned long long)y * P.w + x;
    rt_tm_pixel(P, cc, pc, cur_frame, cur_aov, prev_hist, prev_len, prev_aov, prev_m2, x, y, hist + i * 3u, len + i, frame_out + i * 3u, m2 + i, nullptr);
}

__global__ __launch_bounds__(RT_PX_WG) void rt_tv_variance_kernel(RtDnParams P, const double* __restrict__ hist, const double* __restrict__ m2,
                                                                      const double* __restrict__ len, const double* __restrict__ aov,
                                                                      double* __restrict__ var) {
    uint32_t x, y;
    rt_px_lane_pixel(P.w, x, y);
    if (x >= P.w || y >= P.h) return;
    var[(unsigned long long)y * P.w + x] = rt_tv_pixel(P, hist, m2, len, aov, x, y);
}
} // namespace rttv

/* called by features.hip.  One launch on `stream` each; the cameras as for rt1w_internal_temporal_launch, rt1w_internal_temporal_var_sizeof()
 * bytes each.  launch[0..1] = grid, block.  0, -1 (launch failure) or -2 (parameters refused). */
extern "C" int rt1w_internal_temporal_moments_launch(uint32_t w, uint32_t h, uint32_t flags, uint32_t max_history, double depth_tol, double normal_min,
                                                     const double* cur_frame, const double* cur_aov, const void* cur_cam, const double* prev_hist,
                                                     const double* prev_m2, const double* prev_len, const double* prev_aov, const void* prev_cam,
                                                     double* hist, double* m2, double* len, double* frame_out, hipStream_t stream, unsigned launch[2]) {
    using namespace rttv;
    RtTmParams P;
    if (!rt_tm_make_params(w, h, flags, max_history, depth_tol, normal_min, P)) return -2;
    RtCamera cc, pc;
    memcpy(&cc, cur_cam, sizeof cc);
    memcpy(&pc, prev_cam, sizeof pc);
    return rt_px_launch(rt_tv_moments_kernel, rt_px_frame_grid(P.w, P.h), stream, launch, P, cc, pc, cur_frame, cur_aov, prev_hist, prev_m2, prev_len,
                        prev_aov, hist, m2, len, frame_out);
}
extern "C" int rt1w_internal_temporal_variance_launch(uint32_t w, uint32_t h, const double* hist, const double* m2, const double* len, const double* aov,
                                                      double* var, hipStream_t stream, unsigned launch[2]) {
    using namespace rttv;
    RtDnParams P;
    if (!rt_tv_make_params(w, h, P)) return -2;
    return rt_px_launch(rt_tv_variance_kernel, rt_px_frame_grid(P.w, P.h), stream, launch, P, hist, m2, len, aov, var);
}
extern "C" unsigned rt1w_internal_temporal_var_sizeof(void) { return (unsigned)sizeof(rttv::RtCamera); }
