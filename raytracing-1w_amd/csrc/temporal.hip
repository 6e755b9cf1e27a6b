/* temporal.hip -- the kernel of rt1w_temporal_accumulate (include/rt1w.h): one launch over rt_temporal.h.
 *
 * Kept out of context.hip, inside its own namespace (the pattern of denoise.hip), so that none of the render kernels' code objects and
 * none of the run-time compiler's inputs moves with it.  The host half (validation, buffers, timing, copies, the state of
 * rt1w_render_temporal) is in features.hip, which calls the launcher below.
 *
 * Work mapping: that of rt_pixel_kernels.h, workgroups in row order over the image -- one lane per pixel, an 8 x 8 pixel block per wave,
 * 2 x 2 blocks (16 x 16 pixels) per workgroup of 256 lanes, as the denoiser has it: the reprojection of a block is a block of about the same size, so a wave's four gathers fall into few cache lines.
 * Every output pixel is computed whole by one lane in the fixed tap order of rt_tm_pixel: no atomics, no LDS, the same bits as the CPU
 * twin (denoise_host.cpp).  Both cameras are kernel arguments by value (2 x 192 bytes of the kernel-argument segment, read by scalar
 * loads).  The build fails if the kernel uses scratch (Makefile: no_scratch_unit). */
#include <hip/hip_runtime.h>
#include "rt_feature_launch.h" /* this unit's functions as features.hip calls them: the definitions below are held to it */
#include <stdint.h>
#include <string.h>

namespace rttm {
#include "rt1w_num.h"
#include "rt_temporal.h"

#include "rt_pixel_kernels.h"

__global__ __launch_bounds__(RT_PX_WG) void rt_tm_accumulate_kernel(RtTmParams P, RtCamera cc, RtCamera pc, const double* __restrict__ cur_frame,
                                                                        const double* __restrict__ cur_aov, const double* __restrict__ prev_hist,
                                                                        const double* __restrict__ prev_len, const double* __restrict__ prev_aov,
                                                                        double* __restrict__ hist, double* __restrict__ len, double* __restrict__ frame_out) {
    uint32_t x, y;
    rt_px_lane_pixel(P.w, x, y);
    if (x >= P.w || y >= P.h) return;
    const unsigned long long i = (unsigned long long)y * P.w + x;
    rt_tm_pixel(P, cc, pc, cur_frame, cur_aov, prev_hist, prev_len, prev_aov, nullptr, x, y, hist + i * 3u, len + i, frame_out + i * 3u, nullptr, nullptr);
}
} // namespace rttm

/* called by features.hip.  One launch on `stream`; cur_cam and prev_cam point to rt1w_internal_temporal_sizeof() bytes each (RtCamera, the
 * layout of rt1w_camera).  launch[0..1] = grid, block.  0, -1 (launch failure) or -2 (parameters refused). */
extern "C" int rt1w_internal_temporal_launch(uint32_t w, uint32_t h, uint32_t flags, uint32_t max_history, double depth_tol, double normal_min,
                                             const double* cur_frame, const double* cur_aov, const void* cur_cam, const double* prev_hist,
                                             const double* prev_len, const double* prev_aov, const void* prev_cam, double* hist, double* len,
                                             double* frame_out, hipStream_t stream, unsigned launch[2]) {
    using namespace rttm;
    RtTmParams P;
    if (!rt_tm_make_params(w, h, flags, max_history, depth_tol, normal_min, P)) return -2;
    RtCamera cc, pc;
    memcpy(&cc, cur_cam, sizeof cc);
    memcpy(&pc, prev_cam, sizeof pc);
    return rt_px_launch(rt_tm_accumulate_kernel, rt_px_frame_grid(P.w, P.h), stream, launch, P, cc, pc, cur_frame, cur_aov, prev_hist, prev_len, prev_aov,
                        hist, len, frame_out);
}
extern "C" unsigned rt1w_internal_temporal_sizeof(void) { return (unsigned)sizeof(rttm::RtCamera); }
