/* hit.hip -- the ray queries of rt1w_hit (include/rt1w.h): one kernel per scene variant V0..V5 over rt_hit.h.
 *
 * Kept out of context.hip, inside its own namespace (the pattern of aov.hip), so that none of the render kernels' code objects and
 * none of the run-time compiler's inputs moves with it.  The host half (validation, buffers, timing) is in features.hip, which calls
 * the launcher below.  rt_pixel_kernels.h gives the launch tail only.
 *
 * Work mapping: one lane per ray, ray r = blockIdx.x * RT_BLOCK + threadIdx.x, so a wave takes 64 consecutive rays of the caller's list
 * (what is coherent in the list is coherent in the wave; the list is not reordered).  Lanes past n bring nothing and take no part in
 * any walk; the walks' wave votes (__ballot) count active lanes only, so a partly filled wave is well defined.  Sweep variants walk
 * with scalar node loads (RtGlobalNodes); stack variants keep their stacks in LDS columns as aov.hip does (RT_STACK_CAP x RT_BLOCK
 * entries).  All ray and record offsets are 64-bit.
 *
 * Ray I/O, the part no other unit has: a lane's ray record is 72 bytes and its hit record 96, so a wave's 64 records are 4608 and 6144
 * contiguous bytes which one lane per record touches at a 72- and a 96-byte stride.  Two forms, chosen when the unit is built:
 *   RT_HIT_STAGED 0  direct: each lane loads its 9 doubles and stores its 12;
 *   RT_HIT_STAGED 1  staged: the workgroup copies its RT_BLOCK ray records (18432 bytes) into LDS with 16-byte accesses from
 *                    consecutive lanes (8-byte ones where the caller's buffer is not 16-byte aligned, and for an odd last double),
 *                    each lane takes its record from LDS, and the hit records (24576 bytes) go back the same way.  The stack
 *                    variants' stack memory (32 KB) is free before and after the walk and holds the records; the sweep variants get
 *                    24 KB of LDS for them.  Barriers separate the three uses; lanes past n take part in the copies and barriers.
 * Both forms run rt_hit_ray on the same nine doubles in registers, so they give the same bits (and the twin's).  out_node is 4 bytes
 * per lane at consecutive addresses in either form.  Built for four waves per SIMD (128 VGPRs), the budget of the first-hit AOV
 * kernels; the figures are in DESIGN.md section 22. */
#include <hip/hip_runtime.h>
#include "rt_feature_launch.h" /* this unit's functions as features.hip calls them: the definitions below are held to it */
#include <stdint.h>
#include <string.h>
#include <type_traits>

namespace rthit {
#include "rt1w_num.h"
#include "rt_flat.h"
#include "rt_kernel_sorted.h"
#include "rt_hit.h"
#include "rt_pixel_kernels.h"
static_assert(RT_BLOCK == RT_PX_WG, "rt_px_launch launches workgroups of RT_BLOCK lanes");

#ifndef RT_HIT_WAVES
#define RT_HIT_WAVES 4 /* waves per SIMD the kernels are built for (aov.hip: RT_AOV_WAVES) */
#endif
#ifndef RT_HIT_STAGED
#define RT_HIT_STAGED 0 /* 1: ray and hit records pass through LDS (the measured alternative) */
#endif

/* LDS of a workgroup in 32-bit words: the stacks of a stack variant (which also hold the staged records), the staged records of a sweep variant */
template <class Cfg>
constexpr unsigned hit_lds_words() {
    return !Cfg::sweep ? RT_STACK_CAP * RT_BLOCK : (RT_HIT_STAGED ? RT_HIT_RECORD * RT_BLOCK * 2u : 1u);
}
static_assert(RT_STACK_CAP * RT_BLOCK >= RT_HIT_RECORD * RT_BLOCK * 2u, "the stack memory holds a workgroup's hit records");

#if RT_HIT_STAGED
/* `count` doubles (<= RT_BLOCK * RT_HIT_RECORD) between global memory at g and LDS at l, by the whole workgroup: 16-byte accesses from
 * consecutive lanes where g is 16-byte aligned, an odd last double and an unaligned buffer by 8-byte ones.  TO_LDS: g -> l */
template <bool TO_LDS>
__device__ __forceinline__ void hit_stage(double* g, double* l, uint32_t count) {
    if ((reinterpret_cast<uintptr_t>(g) & 15u) == 0u) {
        const uint32_t pairs = count >> 1;
        double2* g2 = reinterpret_cast<double2*>(g);
        double2* l2 = reinterpret_cast<double2*>(l);
        for (uint32_t i = threadIdx.x; i < pairs; i += RT_BLOCK) {
            if (TO_LDS) l2[i] = g2[i]; else g2[i] = l2[i];
        }
        if ((count & 1u) && threadIdx.x == 0u) {
            if (TO_LDS) l[count - 1u] = g[count - 1u]; else g[count - 1u] = l[count - 1u];
        }
    } else {
        for (uint32_t i = threadIdx.x; i < count; i += RT_BLOCK) {
            if (TO_LDS) l[i] = g[i]; else g[i] = l[i];
        }
    }
}
#endif

template <class Cfg>
__global__ __launch_bounds__(RT_BLOCK, RT_HIT_WAVES) void rt_hit_kernel(RtSceneView sc, RtHitParams hp, const double* __restrict__ rays,
                                                                        double* __restrict__ out, uint32_t* __restrict__ out_node) {
    __shared__ __attribute__((aligned(16))) uint32_t lds_mem[hit_lds_words<Cfg>()];
    const unsigned long long first = (unsigned long long)blockIdx.x * RT_BLOCK; /* the workgroup's first ray */
    const unsigned long long r = first + threadIdx.x;
    const bool live = r < hp.n;
    double ray[RT_HIT_RAY], rec[RT_HIT_RECORD];
    uint32_t node = RT_NONE;
#if RT_HIT_STAGED
    const uint32_t here = (uint32_t)(hp.n - first < RT_BLOCK ? hp.n - first : RT_BLOCK); /* rays of this workgroup: >= 1 (the grid covers n) */
    double* staged = reinterpret_cast<double*>(lds_mem);
    hit_stage<true>(const_cast<double*>(rays) + first * RT_HIT_RAY, staged, here * RT_HIT_RAY);
    __syncthreads();
    if (live)
        for (int k = 0; k < RT_HIT_RAY; ++k) ray[k] = staged[threadIdx.x * RT_HIT_RAY + k];
    __syncthreads(); /* every record is in registers: the memory becomes the stacks */
#else
    if (!live) return;
    for (int k = 0; k < RT_HIT_RAY; ++k) ray[k] = rays[r * RT_HIT_RAY + k];
#endif
    if (live) {
        LdsStack stk;
        stk.base = lds_mem + threadIdx.x;
        stk.sp = 0;
        RtGlobalNodes ns;
        ns.p = sc.nodes;
        rt_hit_ray<Cfg>(sc, ns, ray, r, hp, stk, rec, node);
        if (out_node) out_node[r] = node;
    }
#if RT_HIT_STAGED
    __syncthreads(); /* every walk of the workgroup has ended: the memory becomes the hit records */
    if (live)
        for (int k = 0; k < RT_HIT_RECORD; ++k) staged[threadIdx.x * RT_HIT_RECORD + k] = rec[k];
    __syncthreads();
    hit_stage<false>(out + first * RT_HIT_RECORD, staged, here * RT_HIT_RECORD);
#else
    for (int k = 0; k < RT_HIT_RECORD; ++k) out[r * RT_HIT_RECORD + k] = rec[k];
#endif
}

typedef void (*kernel_t)(RtSceneView, RtHitParams, const double*, double*, uint32_t*);
static kernel_t const g_hit[RT_N_VARIANTS] = {rt_hit_kernel<RtCfgV0>, rt_hit_kernel<RtCfgV1>, rt_hit_kernel<RtCfgV2>,
                                              rt_hit_kernel<RtCfgV3>, rt_hit_kernel<RtCfgV4>, rt_hit_kernel<RtCfgV5>};
} // namespace rthit

/* called by features.hip.  Enqueues the kernel of `variant` on `stream` over the params->n rays at `rays` (device memory); `view` and
 * `params` point to the bytes of an RtSceneView and of an rt1w_hit_params (same layouts: features.hip checks rt1w_internal_hit_sizeof),
 * copied into the kernel's arguments; out_node may be null.  launch[0..1] = grid, block.  0, -1 (launch failure) or -2 (no such
 * variant, or n outside 1 .. 2^32 - 1) */
extern "C" int rt1w_internal_hit_launch(const void* view, const void* params, int variant, const double* rays, double* out, uint32_t* out_node,
                                        hipStream_t stream, unsigned launch[2]) {
    using namespace rthit;
    if (variant < 0 || variant >= RT_N_VARIANTS) return -2;
    RtSceneView sc;
    RtHitParams hp;
    memcpy(&sc, view, sizeof sc);
    memcpy(&hp, params, sizeof hp);
    if (hp.n == 0u || hp.n > 0xFFFFFFFFull) return -2;
    return rt_px_launch(g_hit[variant], (unsigned)((hp.n + RT_BLOCK - 1u) / RT_BLOCK), stream, launch, sc, hp, rays, out, out_node);
}
/* 0, 1: bytes of the two structs above; 2: the I/O form this build runs (RT_HIT_STAGED) */
extern "C" unsigned rt1w_internal_hit_sizeof(int what) {
    return what == 0 ? (unsigned)sizeof(rthit::RtSceneView) : what == 1 ? (unsigned)sizeof(rthit::RtHitParams) : (unsigned)RT_HIT_STAGED;
}
