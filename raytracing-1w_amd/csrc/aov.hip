/* aov.hip -- the first-hit feature buffers of rt1w_render_aov (include/rt1w.h): one kernel per scene variant V0..V5 over rt_aov.h;
 * below them the deep feature buffers of rt1w_render_aov_deep over rt_aov_deep.h, in a namespace of their own.
 *
 * Kept out of context.hip, inside its own namespace (the pattern of context_ref.hip), so that none of the render kernels' code objects
 * and none of the run-time compiler's inputs moves with it.  The host half (validation, buffers, timing) is in features.hip, which
 * calls the two launchers below.
 *
 * Work mapping: one lane per pixel, looping over the pixel's samples in order -- the sums have one fixed order, the same as the CPU
 * twin's (aov_host.cpp), and no partial-sum buffer is needed.  A wave covers an 8 x 8 block of the tile (aov_lane_pixel: the blocks are
 * numbered wave by wave in row order over the tile, four to a workgroup -- not the 16 x 16 mapping of rt_pixel_kernels.h, of which this
 * unit takes the launch tail only), so its 64 camera rays are neighbours (the wave-uniform sweep of the small scenes and the stack
 * walk of the big ones see coherent rays).  Lanes outside the tile leave before any walk; the walks' wave votes (__ballot) count active lanes only, so a partly filled wave is well defined.
 * Sweep variants walk with scalar node loads (RtGlobalNodes); stack variants keep their stacks in LDS columns as rt_kernel_plain.h
 * does (RT_STACK_CAP x RT_BLOCK entries).  Built for four waves per SIMD (128 VGPRs); the figures are in DESIGN.md. */
#include <hip/hip_runtime.h>
#include "rt_feature_launch.h" /* this unit's functions as features.hip calls them: the definitions below are held to it */
#include <stdint.h>
#include <string.h>
#include <type_traits>

namespace rtaov {
#include "rt1w_num.h"
#include "rt_flat.h"
#include "rt_kernel_sorted.h"
#include "rt_aov_deep.h"
#include "rt_pixel_kernels.h"
static_assert(RT_BLOCK == RT_PX_WG, "rt_px_launch launches workgroups of RT_BLOCK lanes");

#ifndef RT_AOV_WAVES
#define RT_AOV_WAVES 4 /* waves per SIMD the kernels are built for */
#endif
#ifndef RT_AOV_ROW_MAJOR
#define RT_AOV_ROW_MAJOR 0 /* 1: consecutive lanes take consecutive pixels of a tile row (the measured alternative) */
#endif

/* this lane's pixel of the tile; false: the lane has none.  aov_grid() workgroups cover the tile */
__device__ __forceinline__ bool aov_lane_pixel(const RtFrame& f, uint32_t& px, uint32_t& py) {
#if RT_AOV_ROW_MAJOR
    const unsigned long long idx = (unsigned long long)blockIdx.x * RT_BLOCK + threadIdx.x;
    px = (uint32_t)(idx % f.tile_w); py = (uint32_t)(idx / f.tile_w);
    return idx < (unsigned long long)f.tile_w * f.tile_h;
#else
    const uint32_t bw = (f.tile_w + 7u) >> 3;
    const uint32_t wave = blockIdx.x * (RT_BLOCK / 64u) + (threadIdx.x >> 6), in = threadIdx.x & 63u;
    px = (wave % bw) * 8u + (in & 7u); py = (wave / bw) * 8u + (in >> 3);
    return px < f.tile_w && py < f.tile_h;
#endif
}
__host__ inline unsigned aov_grid(const RtFrame& f) {
#if RT_AOV_ROW_MAJOR
    return (unsigned)(((unsigned long long)f.tile_w * f.tile_h + RT_BLOCK - 1u) / RT_BLOCK);
#else
    const unsigned long long blocks8 = (unsigned long long)((f.tile_w + 7u) >> 3) * ((f.tile_h + 7u) >> 3);
    return (unsigned)((blocks8 + RT_BLOCK / 64u - 1u) / (RT_BLOCK / 64u));
#endif
}

template <class Cfg>
__global__ __launch_bounds__(RT_BLOCK, RT_AOV_WAVES) void rt_aov_kernel(RtSceneView sc, RtFrame f, double* __restrict__ out) {
    __shared__ uint32_t stack_mem[Cfg::sweep ? 1 : RT_STACK_CAP * RT_BLOCK];
    uint32_t px, py;
    if (!aov_lane_pixel(f, px, py)) return;
    LdsStack stk;
    stk.base = stack_mem + threadIdx.x;
    stk.sp = 0;
    RtGlobalNodes ns;
    ns.p = sc.nodes;
    rt_aov_pixel<Cfg>(sc, ns, f, px, py, stk, out + ((unsigned long long)py * f.tile_w + px) * RT_AOV_CHANNELS);
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
    uint32_t px, py;
    const bool inside = aov_lane_pixel(f, px, py);
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

/* called by features.hip.  Each enqueues the kernel of `variant` on `stream` over the tile of `frame`; `view` and `frame` point to the
 * bytes of an RtSceneView and an RtFrame (same headers, same layout: features.hip checks rt1w_internal_aov_sizeof), copied into the kernel's
 * arguments.  launch[0..1] = grid, block.  0, -1 (launch failure) or -2 (no such variant) */
extern "C" int rt1w_internal_aov_launch(const void* view, const void* frame, int variant, double* out, hipStream_t stream, unsigned launch[2]) {
    using namespace rtaov;
    if (variant < 0 || variant >= RT_N_VARIANTS) return -2;
    RtSceneView sc;
    RtFrame f;
    memcpy(&sc, view, sizeof sc);
    memcpy(&f, frame, sizeof f);
    return rt_px_launch(g_aov[variant], aov_grid(f), stream, launch, sc, f, out);
}
/* `segments` (device memory, zeroed by the caller on `stream`) receives the rays traced */
extern "C" int rt1w_internal_aov_deep_launch(const void* view, const void* frame, int variant, uint32_t max_specular, double max_fuzz, double* out,
                                             unsigned long long* segments, hipStream_t stream, unsigned launch[2]) {
    using namespace rtaovdeep;
    if (variant < 0 || variant >= RT_N_VARIANTS) return -2;
    RtSceneView sc;
    RtFrame f;
    memcpy(&sc, view, sizeof sc);
    memcpy(&f, frame, sizeof f);
    return rt_px_launch(g_aov_deep[variant], aov_grid(f), stream, launch, sc, f, max_specular, max_fuzz, out, segments);
}
extern "C" unsigned rt1w_internal_aov_sizeof(int what) { return what == 0 ? (unsigned)sizeof(rtaov::RtSceneView) : (unsigned)sizeof(rtaov::RtFrame); }
