/* aov_tiles.hip -- the first-hit feature buffers once more, in their TILE-LIST FORM (rt1w_render_aov_tiles, include/rt1w.h): the raw sums of
 * a list of square tiles of the image by one launch, one kernel per scene variant V0..V5 over rt_aov_tiles.h.
 *
 * The pattern of aov.hip and context_tiles.hip: a unit of its own, inside its own namespace, so that the code objects of rt_aov_kernel and
 * of every other unit stay where they are.  The host half (validation, the list's upload, buffers, launch, timing) is in features.hip,
 * which gets the kernel's host handle from the exports below.
 *
 * Work mapping: that of rt_aov_kernel -- one lane per pixel, looping over the pixel's samples in order, an 8 x 8 pixel block per wave --
 * with 2 x 2 such blocks (16 x 16 pixels) per workgroup of RT_BLOCK lanes and (tile / 16)^2 workgroups per tile of the list, tile after
 * tile.  A workgroup's tile follows from blockIdx alone, so its record {x0, y0, sample_offset, -} is read wave-uniformly.  A lane whose
 * pixel lies beyond the frame's right or top edge writes its eight +0.0 and leaves before any walk; the walks' wave votes count active
 * lanes only.  Sweep variants walk with scalar node loads (RtGlobalNodes); stack variants keep their stacks in LDS columns
 * (RT_STACK_CAP x RT_BLOCK entries).  Built for four waves per SIMD (128 VGPRs) like rt_aov_kernel; the figures are in DESIGN.md. */
#include <hip/hip_runtime.h>
#include "rt_feature_launch.h" /* this unit's functions as features.hip calls them: the definitions below are held to it */
#include <stdint.h>
#include <type_traits>

namespace rtaovt {
#include "rt1w_num.h"
#include "rt_flat.h"
#include "rt_kernel_sorted.h"
#include "rt_aov_tiles.h"

#ifndef RT_AOV_TILES_WAVES
#define RT_AOV_TILES_WAVES 4 /* waves per SIMD the kernels are built for */
#endif

/* rec[n][4] = rt1w_tile records (device memory); out[n][tile][tile][8] */
template <class Cfg>
__global__ __launch_bounds__(RT_BLOCK, RT_AOV_TILES_WAVES) void rt_aov_tiles_kernel(RtSceneView sc, RtFrame f, uint32_t tile, const uint32_t* __restrict__ rec,
                                                                                   double* __restrict__ out) {
    __shared__ uint32_t stack_mem[Cfg::sweep ? 1 : RT_STACK_CAP * RT_BLOCK];
    const uint32_t bw = tile >> 4;
    const uint32_t k = blockIdx.x / (bw * bw), b = blockIdx.x % (bw * bw);
    const uint32_t x0 = rec[(size_t)k * 4u], y0 = rec[(size_t)k * 4u + 1u], so = rec[(size_t)k * 4u + 2u];
    const uint32_t wv = threadIdx.x >> 6, in = threadIdx.x & 63u;
    const uint32_t lx = (b % bw) * 16u + (wv & 1u) * 8u + (in & 7u), ly = (b / bw) * 16u + (wv >> 1) * 8u + (in >> 3);
    LdsStack stk;
    stk.base = stack_mem + threadIdx.x;
    stk.sp = 0;
    RtGlobalNodes ns;
    ns.p = sc.nodes;
    rt_aov_tiles_pixel<Cfg>(sc, ns, f, tile, k, x0, y0, so, lx, ly, stk, out);
}

typedef void (*kernel_t)(RtSceneView, RtFrame, uint32_t, const uint32_t*, double*);
static kernel_t const g_aov_tiles[RT_N_VARIANTS] = {rt_aov_tiles_kernel<RtCfgV0>, rt_aov_tiles_kernel<RtCfgV1>, rt_aov_tiles_kernel<RtCfgV2>,
                                                    rt_aov_tiles_kernel<RtCfgV3>, rt_aov_tiles_kernel<RtCfgV4>, rt_aov_tiles_kernel<RtCfgV5>};
static_assert(RT_BLOCK == 256, "a workgroup covers 16 x 16 pixels: 2 x 2 waves of 8 x 8");
} // namespace rtaovt

/* the kernel of a variant for features.hip, which launches it with RT_BLOCK work-items and n_tiles x (tile / 16)^2 workgroups on (its
 * RtSceneView, its RtFrame, tile, the uploaded list, out): same headers, same layout, checked through rt1w_internal_aov_tiles_sizeof.
 * nullptr: no such variant */
extern "C" const void* rt1w_internal_aov_tiles_kernel(int variant) {
    return variant >= 0 && variant < RT_N_VARIANTS ? reinterpret_cast<const void*>(rtaovt::g_aov_tiles[variant]) : nullptr;
}
extern "C" unsigned rt1w_internal_aov_tiles_sizeof(int what) { return what == 0 ? (unsigned)sizeof(rtaovt::RtSceneView) : (unsigned)sizeof(rtaovt::RtFrame); }
