/* aov_tiles.hip -- the first-hit feature buffers once more, in their TILE-LIST FORM (rt1w_render_aov_tiles, include/rt1w.h): the raw sums of
 * a list of square tiles of the image by one launch, one kernel per scene variant V0..V5 over rt_aov_tiles.h.
 *
 * The pattern of aov.hip and context_tiles.hip: a unit of its own, inside its own namespace, so that the code objects of rt_aov_kernel and
 * of every other unit stay where they are.  The host half (validation, the list's upload, buffers, timing) is in features.hip,
 * which calls the launcher below.
 *
 * Work mapping: that of rt_aov_kernel -- one lane per pixel, looping over the pixel's samples in order, an 8 x 8 pixel block per wave --
 * with 2 x 2 such blocks (16 x 16 pixels) per workgroup of RT_BLOCK lanes and (tile / 16)^2 workgroups per tile of the list, tile after
 * tile (rt_pixel_kernels.h: rt_px_list_lane).  A lane whose
 * pixel lies beyond the frame's right or top edge writes its eight +0.0 and leaves before any walk; the walks' wave votes count active
 * lanes only.  Sweep variants walk with scalar node loads (RtGlobalNodes); stack variants keep their stacks in LDS columns
 * (RT_STACK_CAP x RT_BLOCK entries).  Built for four waves per SIMD (128 VGPRs) like rt_aov_kernel; the figures are in DESIGN.md. */
#include <hip/hip_runtime.h>
#include "rt_feature_launch.h" /* this unit's functions as features.hip calls them: the definitions below are held to it */
#include <stdint.h>
#include <string.h>
#include <type_traits>

namespace rtaovt {
#include "rt1w_num.h"
#include "rt_flat.h"
#include "rt_kernel_sorted.h"
#include "rt_aov_tiles.h"
#include "rt_pixel_kernels.h"
static_assert(RT_BLOCK == RT_PX_WG, "a workgroup covers 16 x 16 pixels: 2 x 2 waves of 8 x 8");

#ifndef RT_AOV_TILES_WAVES
#define RT_AOV_TILES_WAVES 4 /* waves per SIMD the kernels are built for */
#endif

/* rec[n][4] = rt1w_tile records (device memory); out[n][tile][tile][8] */
template <class Cfg>
__global__ __launch_bounds__(RT_BLOCK, RT_AOV_TILES_WAVES) void rt_aov_tiles_kernel(RtSceneView sc, RtFrame f, uint32_t tile, const uint32_t* __restrict__ rec,
                                                                                   double* __restrict__ out) {
    __shared__ uint32_t stack_mem[Cfg::sweep ? 1 : RT_STACK_CAP * RT_BLOCK];
    const RtPxListLane l = rt_px_list_lane(tile, rec);
    LdsStack stk;
    stk.base = stack_mem + threadIdx.x;
    stk.sp = 0;
    RtGlobalNodes ns;
    ns.p = sc.nodes;
    rt_aov_tiles_pixel<Cfg>(sc, ns, f, tile, l.k, l.x0, l.y0, l.sample_offset, l.lx, l.ly, stk, out);
}

typedef void (*kernel_t)(RtSceneView, RtFrame, uint32_t, const uint32_t*, double*);
static kernel_t const g_aov_tiles[RT_N_VARIANTS] = {rt_aov_tiles_kernel<RtCfgV0>, rt_aov_tiles_kernel<RtCfgV1>, rt_aov_tiles_kernel<RtCfgV2>,
                                                    rt_aov_tiles_kernel<RtCfgV3>, rt_aov_tiles_kernel<RtCfgV4>, rt_aov_tiles_kernel<RtCfgV5>};
} // namespace rtaovt

/* called by features.hip.  Enqueues the kernel of `variant` on `stream` over the n tiles of `rec` (device memory; the list is the caller's to
 * check: rt_adaptive_plan.h, rt_aov_tiles_check); `view` and `frame` point to the bytes of an RtSceneView and an RtFrame (same headers, same
 * layout: features.hip checks rt1w_internal_aov_tiles_sizeof), copied into the kernel's arguments.  launch[0..1] = grid, block.  0, -1
 * (launch failure) or -2 (parameters refused) */
extern "C" int rt1w_internal_aov_tiles_launch(const void* view, const void* frame, int variant, uint32_t tile, const uint32_t* rec, uint32_t n, double* out,
                                              hipStream_t stream, unsigned launch[2]) {
    using namespace rtaovt;
    if (variant < 0 || variant >= RT_N_VARIANTS || tile < RT_PX_BLOCK || tile % RT_PX_BLOCK || n < 1u) return -2;
    RtSceneView sc;
    RtFrame f;
    memcpy(&sc, view, sizeof sc);
    memcpy(&f, frame, sizeof f);
    return rt_px_launch(g_aov_tiles[variant], rt_px_list_grid(tile, n), stream, launch, sc, f, tile, rec, out);
}
extern "C" unsigned rt1w_internal_aov_tiles_sizeof(int what) { return what == 0 ? (unsigned)sizeof(rtaovt::RtSceneView) : (unsigned)sizeof(rtaovt::RtFrame); }
