/* aov.hip -- the first-hit feature buffers of rt1w_render_aov (include/rt1w.h): one kernel per scene variant V0..V5 over rt_aov.h;
 * below them the deep feature buffers of rt1w_render_aov_deep over rt_aov_deep.h, in a namespace of their own.
 *
 * Kept out of context.hip, inside its own namespace (the pattern of context_ref.hip), so that none of the render kernels' code objects
 * and none of the run-time compiler's inputs moves with it.  The host half (validation, buffers, launch, timing) is in features.hip, which
 * gets the kernel's host handle and its grid from the two exports below.
 *
 * Work mapping: one lane per pixel, looping over the pixel's samples in order -- the sums have one fixed order, the same as the CPU
 * twin's (aov_host.cpp), and no partial-sum buffer is needed.  A wave covers an 8 x 8 block of the tile, so its 64 camera rays are
 * neighbours (the wave-uniform sweep of the small scenes and the stack walk of the big ones see coherent rays).  Lanes outside the
 * tile leave before any walk; the walks' wave votes (__ballot) count active lanes only, so a partly filled wave is well defined.
 * Sweep variants walk with scalar node loads (RtGlobalNodes); stack variants keep their stacks in LDS columns as rt_kernel_plain.h
 * does (RT_STACK_CAP x RT_BLOCK entries).  Built for four waves per SIMD (128 VGPRs); the figures are in DESIGN.md. */
#include <hip/hip_runtime.h>
#include "rt_feature_launch.h" /* this unit's functions as features.hip calls them: the definitions below are held to it */
#include <stdint.h>
#include <type_traits>

namespace rtaov {
#include "rt1w_num.h"
#include "rt_flat.h"
#include "rt_kernel_sorted.h"
#include "rt_aov_deep.h"

#ifndef RT_AOV_WAVES
#define RT_AOV_WAVES 4 /* waves per SIMD the kernels are built for */
#endif
#ifndef RT_AOV_ROW_MAJOR
#define RT_AOV_ROW_MAJOR 0 /* 1: consecutive lanes take consecutive pixels of a tile row (the measured alternative) */
#endif

template <class Cfg>
__global__ __launch_bounds__(RT_BLOCK, RT_AOV_WAVES) void rt_aov_kernel(RtSceneView sc, RtFrame f, double* __restrict__ out) {
    __shared__ uint32_t stack_mem[Cfg::sweep ? 1 : RT_STACK_CAP * RT_BLOCK];
#if RT_AOV_ROW_MAJOR
    const unsigned long long idx = (unsigned long long)blockIdx.x * RT_BLOCK + threadIdx.x;
    const uint32_t px = (uint32_t)(idx % f.tile_w), py = (uint32_t)(idx / f.tile_w);
    if (idx >= (unsigned long long)f.tile_w * f.tile_h) return;
#else
    const uint32_t bw = (f.tile_w + 7u) >> 3;
    const uint32_t wave = blockIdx.x * (RT_BLOCK / 64u) + (threadIdx.x >> 6), in = threadIdx.x & 63u;
    const uint32_t px = (wave % bw) * 8u + (in & 7u), py = (wave / bw) * 8u + (in >> 3);
    if (px >= f.tile_w || py >= f.tile_h) return;
#endif
    LdsStack stk;
    stk.base = stack_mem + threadIdx.x;
    stk.sp = 0;
    RtGlobalNodes ns;
    ns.p = sc.nodes;
    rt_aov_pixel<Cfg>(sc, ns, f, px, py, stk, out + ((unsigned long long)py * f.tile_w + px) * RT_AOV_CHANNELS);
}

/* workgroups that cover the tile */
inline unsigned aov_grid(const RtFrame& f) {
#if RT_AOV_ROW_MAJOR
    return (unsigned)(((unsigned long long)f.tile_w * f.tile_h + RT_BLOCK - 1u) / RT_BLOCK);
#else
    const unsigned long long blocks8 = (unsigned long long)((f.tile_w + 7u) >> 3) * ((f.tile_h + 7u) >> 3);
    return (unsigned)((blocks8 + RT_BLOCK / 64u - 1u) / (RT_BLOCK / 64u));
#endif
}
typedef void (*kernel_t)(RtSceneView, RtFrame, double*);
static kernel_t const g_aov[RT_N_VARIANTS] = {rt_aov_kernel<RtCfgV0>, rt_aov_kernel<RtCfgV1>, rt_aov_kernel<RtCfgV2>,
                                              rt_aov_kernel<RtCfgV3>, rt_aov_kernel<RtCfgV4>, rt_aov_kernel<RtCfgV5>};
} // namespace rtaov

/* The deep feature buffers of rt1w_render_aov_deep over rt_aov_deep.h: the same mapping, grid and stacks.  A lane whose chain has
 * ended walks along with an empty interval while lanes of its wave are still between specular surfaces (rt_aov_deep.h; the share of
 * such lane-slots is in DESIGN.md).  `segments` receives the rays traced: counted per lane, summed over the wave by shuffles, added by one vector atomic
 * per wave -- so no lane leaves before the sum, and lanes outside the tile bring 0.
 *
 * Built for TWO waves per SIMD, where nothing is spilled to scratch, and the build fails if a deep kernel has scratch (Makefile).
 * Built for four waves like the kernels above, one instantiation per build returned wrong, run-to-run varying results on the GPU; the
 * cause is open. */
namespace rtaovdeep {
using namespace rtaov;

#ifndef RT_AOV_DEEP_WAVES
#define RT_AOV_DEEP_WAVES 2 /* waves per SIMD the deep kernels are built for: 256 VGPRs */
#endif

template <class Cfg>
__global__ __launch_bounds__(RT_BLOCK, RT_AOV_DEEP_WAVES) void rt_aov_deep_kernel(RtSceneView sc, RtFrame f, uint32_t max_specular, double max_fuzz,
                                                                             double* __restrict__ out, unsigned long long* __restrict__ segments) {
    __shared__ uint32_t stack_mem[Cfg::sweep ? 1 : RT_STACK_CAP * RT_BLOCK];
#if RT_AOV_ROW_MAJOR
    const unsigned long long idx = (unsigned long long)blockIdx.x * RT_BLOCK + threadIdx.x;
    const uint32_t px = (uint32_t)(idx % f.tile_w), py = (uint32_t)(idx / f.tile_w);
    const bool inside = idx < (unsigned long long)f.tile_w * f.tile_h;
#else
    const uint32_t bw = (f.tile_w + 7u) >> 3;
    const uint32_t wave = blockIdx.x * (RT_BLOCK / 64u) + (threadIdx.x >> 6), in = threadIdx.x & 63u;
    const uint32_t px = (wave % bw) * 8u + (in & 7u), py = (wave / bw) * 8u + (in >> 3);
    const bool inside = px < f.tile_w && py < f.tile_h;
#endif
    unsigned long long rays = 0ull;
    if (inside) {
        LdsStack stk;
        stk.base = stack_mem + threadIdx.x;
        stk.sp = 0;
        RtGlobalNodes ns;
        ns.p = sc.nodes;
        rays = rt_aov_deep_pixel<Cfg>(sc, ns, f, px, py, max_specular, max_fuzz, stk,
                                      out + ((unsigned long long)py * f.tile_w + px) * RT_AOV_CHANNELS, nullptr);
    }
    for (int off = 32; off > 0; off >>= 1) rays += __shfl_down(rays, off, 64);
    if ((threadIdx.x & 63u) == 0u && rays) atomicAdd(segments, rays);
}

typedef void (*deep_kernel_t)(RtSceneView, RtFrame, uint32_t, double, double*, unsigned long long*);
static deep_kernel_t const g_aov_deep[RT_N_VARIANTS] = {rt_aov_deep_kernel<RtCfgV0>, rt_aov_deep_kernel<RtCfgV1>, rt_aov_deep_kernel<RtCfgV2>,
                                                        rt_aov_deep_kernel<RtCfgV3>, rt_aov_deep_kernel<RtCfgV4>, rt_aov_deep_kernel<RtCfgV5>};
} // namespace rtaovdeep

/* the kernel of a variant for context.hip, which launches it with RT_BLOCK work-items on (its RtSceneView, its RtFrame, out): same
 * headers, same layout, checked through rt1w_internal_aov_sizeof.  nullptr: no such variant */
extern "C" const void* rt1w_internal_aov_kernel(int variant) {
    return variant >= 0 && variant < RT_N_VARIANTS ? reinterpret_cast<const void*>(rtaov::g_aov[variant]) : nullptr;
}
/* the deep kernel of a variant: launched the same way on (view, frame, max_specular, max_fuzz, out, segments counter), same grid */
extern "C" const void* rt1w_internal_aov_deep_kernel(int variant) {
    return variant >= 0 && variant < RT_N_VARIANTS ? reinterpret_cast<const void*>(rtaovdeep::g_aov_deep[variant]) : nullptr;
}
/* the workgroups of that launch; `frame` = the bytes of the RtFrame */
extern "C" unsigned rt1w_internal_aov_grid(const void* frame) { return rtaov::aov_grid(*static_cast<const rtaov::RtFrame*>(frame)); }
extern "C" unsigned rt1w_internal_aov_sizeof(int what) { return what == 0 ? (unsigned)sizeof(rtaov::RtSceneView) : (unsigned)sizeof(rtaov::RtFrame); }
