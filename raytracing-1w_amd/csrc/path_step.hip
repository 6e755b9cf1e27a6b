/* path_step.hip -- the path states of rt1w_path_step and rt1w_path_begin (include/rt1w.h): one step kernel per scene variant V0..V5 over
 * rt_path_state.h, and the begin kernel.
 *
 * Kept out of context.hip, inside its own namespace (the pattern of hit.hip), so that none of the render kernels' code objects and none
 * of the run-time compiler's inputs moves with it.  The host half (validation, buffers, timing) is in features.hip, which calls the
 * launchers below.  rt_pixel_kernels.h gives the launch tail only.
 *
 * Work mapping: one lane per state, state r = blockIdx.x * RT_BLOCK + threadIdx.x, so a wave takes 64 consecutive states of the caller's
 * list; the list is never reordered (the event bits of a state are there so that the caller can sort).  Lanes past n bring nothing and
 * take no part in any walk; the walks' wave votes (__ballot) count active lanes only, and so do the level loops of lanes whose paths end
 * at different levels.  Sweep variants walk with scalar node loads (RtGlobalNodes); stack variants keep their stacks in LDS columns
 * (RT_STACK_CAP x RT_BLOCK entries).  All state offsets are 64-bit.
 *
 * State I/O: a state is one 128-byte line, moved as eight 16-byte accesses of its lane (features.hip refuses device pointers that are
 * not 16-byte aligned).  A lane has read its whole record before it writes any of it, and no lane touches another's, so `in` and `out`
 * may be one buffer.  No LDS staging: for rt1w_hit's records it measured as a wash.  The levels that traced a ray
 * are summed over the wave and added to the caller's counter by one lane.  Built for RT_PATH_WAVES waves per SIMD; the figures of 3 and 4
 * are in profiles/path_step_resources.txt and DESIGN.md section 24. */
#include <hip/hip_runtime.h>
#include "rt_feature_launch.h" /* this unit's functions as features.hip calls them: the definitions below are held to it */
#include <stdint.h>
#include <string.h>
#include <type_traits>

namespace rtpath {
#include "rt1w_num.h"
#include "rt_flat.h"
#include "rt_kernel_sorted.h"
#include "rt_path_state.h"
#include "rt_pixel_kernels.h"
static_assert(RT_BLOCK == RT_PX_WG, "rt_px_launch launches workgroups of RT_BLOCK lanes");

#ifndef RT_PATH_WAVES
#define RT_PATH_WAVES 4 /* waves per SIMD the step kernels are built for (hit.hip: RT_HIT_WAVES) */
#endif

/* a state between memory and registers: eight 16-byte accesses, their words put together in registers */
__device__ __forceinline__ double words_f64(uint32_t lo, uint32_t hi) { return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo)); }
__device__ __forceinline__ void f64_words(double x, uint32_t& lo, uint32_t& hi) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(x);
    lo = (uint32_t)u; hi = (uint32_t)(u >> 32);
}
__device__ __forceinline__ void state_load(RtPathState& s, const RtPathState* at) {
    const uint4* src = reinterpret_cast<const uint4*>(at);
    uint4 q[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) q[k] = src[k];
    double d[13]; /* ray 7, beta 3, radiance 3 */
#pragma unroll
    for (int k = 0; k < 13; ++k) d[k] = (k & 1) ? words_f64(q[k >> 1].z, q[k >> 1].w) : words_f64(q[k >> 1].x, q[k >> 1].y);
#pragma unroll
    for (int k = 0; k < 7; ++k) s.ray[k] = d[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) { s.beta[k] = d[7 + k]; s.radiance[k] = d[10 + k]; }
    s.stream = ((uint64_t)q[6].w << 32) | q[6].z;
    s.sample = q[7].x; s.word = q[7].y; s.depth_left = q[7].z; s.status = q[7].w;
}
__device__ __forceinline__ void state_store(const RtPathState& s, RtPathState* at) {
    double d[13];
#pragma unroll
    for (int k = 0; k < 7; ++k) d[k] = s.ray[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) { d[7 + k] = s.beta[k]; d[10 + k] = s.radiance[k]; }
    uint4 q[8];
#pragma unroll
    for (int k = 0; k < 13; ++k) {
        if (k & 1) f64_words(d[k], q[k >> 1].z, q[k >> 1].w);
        else f64_words(d[k], q[k >> 1].x, q[k >> 1].y);
    }
    q[6].z = (uint32_t)s.stream; q[6].w = (uint32_t)(s.stream >> 32);
    q[7].x = s.sample; q[7].y = s.word; q[7].z = s.depth_left; q[7].w = s.status;
    uint4* dst = reinterpret_cast<uint4*>(at);
#pragma unroll
    for (int k = 0; k < 8; ++k) dst[k] = q[k];
}

/* LDS of a workgroup in 32-bit words: the stacks of a stack variant */
template <class Cfg>
constexpr unsigned path_lds_words() { return !Cfg::sweep ? RT_STACK_CAP * RT_BLOCK : 1u; }

/* in and out may be the same buffer: neither is __restrict__ */
template <class Cfg>
__global__ __launch_bounds__(RT_BLOCK, RT_PATH_WAVES) void rt_path_step_kernel(RtSceneView sc, RtPathParams pp, const RtPathState* in, RtPathState* out,
                                                                               uint32_t* out_node, unsigned long long* segments) {
    __shared__ __attribute__((aligned(16))) uint32_t lds_mem[path_lds_words<Cfg>()];
    const unsigned long long r = (unsigned long long)blockIdx.x * RT_BLOCK + threadIdx.x;
    uint32_t traced = 0u;
    if (r < pp.n) {
        RtPathState s;
        state_load(s, in + r);
        LdsStack stk;
        stk.base = lds_mem + threadIdx.x;
        stk.sp = 0;
        RtGlobalNodes ns;
        ns.p = sc.nodes;
        uint32_t node;
        traced = rt_state_advance<Cfg>(sc, ns, (uint32_t)pp.global_seed, pp.steps, s, stk, node);
        state_store(s, out + r);
        if (out_node) out_node[r] = node;
    }
    /* every lane of the wave is here again: the wave's sum, one atomic per wave that traced anything */
    for (int off = 32; off > 0; off >>= 1) traced += __shfl_down(traced, off);
    if ((threadIdx.x & 63u) == 0u && traced != 0u) atomicAdd(segments, (unsigned long long)traced);
}

/* one lane per entry of the list; *outside counts the entries whose pixel is not in the frame (their states are zeros) */
__global__ __launch_bounds__(RT_BLOCK) void rt_path_begin_kernel(RtCamera cam, RtPathBeginParams bp, const uint32_t* __restrict__ pixels,
                                                                 RtPathState* __restrict__ out, unsigned long long* outside) {
    const unsigned long long r = (unsigned long long)blockIdx.x * RT_BLOCK + threadIdx.x;
    if (r >= bp.n) return;
    const uint32_t pix[3] = {pixels[r * 3u], pixels[r * 3u + 1u], pixels[r * 3u + 2u]};
    RtPathState s;
    if (!rt_state_begin(cam, bp, pix, s)) atomicAdd(outside, 1ull);
    state_store(s, out + r);
}

typedef void (*kernel_t)(RtSceneView, RtPathParams, const RtPathState*, RtPathState*, uint32_t*, unsigned long long*);
static kernel_t const g_step[RT_N_VARIANTS] = {rt_path_step_kernel<RtCfgV0>, rt_path_step_kernel<RtCfgV1>, rt_path_step_kernel<RtCfgV2>,
                                               rt_path_step_kernel<RtCfgV3>, rt_path_step_kernel<RtCfgV4>, rt_path_step_kernel<RtCfgV5>};
} // namespace rtpath

/* called by features.hip.  Enqueues the step kernel of `variant` on `stream` over the params->n states at `in` into `out` (device memory,
 * 16-byte aligned, the same buffer or apart); `view` and `params` point to the bytes of an RtSceneView and of an rt1w_path_params (same
 * layouts: features.hip checks rt1w_internal_path_sizeof), copied into the kernel's arguments; out_node may be null; *segments (device,
 * zeroed by the caller) receives the levels that traced a ray.  launch[0..1] = grid, block.  0, -1 (launch failure) or -2 (no such
 * variant, n outside 1 .. 2^32 - 1, steps outside 1 .. 65536) */
extern "C" int rt1w_internal_path_step_launch(const void* view, const void* params, int variant, const void* in, void* out, uint32_t* out_node,
                                              unsigned long long* segments, hipStream_t stream, unsigned launch[2]) {
    using namespace rtpath;
    if (variant < 0 || variant >= RT_N_VARIANTS) return -2;
    RtSceneView sc;
    RtPathParams pp;
    memcpy(&sc, view, sizeof sc);
    memcpy(&pp, params, sizeof pp);
    if (pp.n == 0u || pp.n > 0xFFFFFFFFull || pp.steps == 0u || pp.steps > RT_PATH_MAX_STEPS) return -2;
    return rt_px_launch(g_step[variant], (unsigned)((pp.n + RT_BLOCK - 1u) / RT_BLOCK), stream, launch, sc, pp, static_cast<const RtPathState*>(in),
                        static_cast<RtPathState*>(out), out_node, segments);
}
/* ... and the begin kernel over the n entries {i, j, sample} at `pixels` into `out`, with the camera of `view`; *outside (device, zeroed
 * by the caller) receives the number of entries outside the frame.  0, -1 or -2 (n outside 1 .. 2^32 - 1) */
extern "C" int rt1w_internal_path_begin_launch(const void* view, uint32_t width, uint32_t height, uint32_t global_seed, uint32_t max_depth,
                                               const uint32_t* pixels, uint64_t n, void* out, unsigned long long* outside, hipStream_t stream,
                                               unsigned launch[2]) {
    using namespace rtpath;
    if (n == 0u || n > 0xFFFFFFFFull) return -2;
    RtSceneView sc;
    memcpy(&sc, view, sizeof sc);
    RtPathBeginParams bp;
    bp.n = n; bp.width = width; bp.height = height; bp.global_seed = global_seed; bp.max_depth = max_depth;
    return rt_px_launch(rt_path_begin_kernel, (unsigned)((n + RT_BLOCK - 1u) / RT_BLOCK), stream, launch, sc.camera, bp, pixels,
                        static_cast<RtPathState*>(out), outside);
}
/* 0, 1, 2: bytes of RtSceneView, RtPathParams and RtPathState as this unit sees them; 3: the waves per SIMD it was built for */
extern "C" unsigned rt1w_internal_path_sizeof(int what) {
    return what == 0 ? (unsigned)sizeof(rtpath::RtSceneView) : what == 1 ? (unsigned)sizeof(rtpath::RtPathParams)
         : what == 2 ? (unsigned)sizeof(rtpath::RtPathState) : (unsigned)RT_PATH_WAVES;
}
