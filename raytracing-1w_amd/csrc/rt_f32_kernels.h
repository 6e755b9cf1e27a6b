/* rt_f32_kernels.h -- the render kernels in single precision: the ten __global__ instantiations of RT1W_PRECISION_F32, as text.
 *
 * Two translation units compile this text: context_f32.hip, the product's kernels (namespace rtf32), and f32_exact.hip of the
 * diagnostics library librt1w_lab.so, with -DRT_F32_ELEMENTARY_F64 and nothing else changed (namespace rtf32x) -- the build whose
 * frames equal the CPU build of the same core bit for bit (oracle/oracle_flat_f32.cpp).  Include it once, first, in a .hip file;
 * afterwards `double` is double again, the f64 record layouts are in the global namespace and the f32 ones in RT_F32_NS. */
#ifndef RT_F32_KERNELS_H
#define RT_F32_KERNELS_H
#ifndef RT_F32_NS
#define RT_F32_NS rtf32
#endif
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <string.h>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "rt_kernel_plain.h" /* the f64 record layouts, for the converters (global namespace) */

#undef RT1W_NUM_H
#undef RT1W_FLAT_H
#undef RT1W_CORE_H
#undef RT_KERNEL_SORTED_H
#undef RT_KERNEL_PLAIN_H
#undef RT1W_WALK_PAIR_H
#define RT_F32 1
#define double float

namespace RT_F32_NS {
#include "rt1w_num.h"
#include "rt_flat.h"
#include "rt_core.h"
#include "rt_kernel_sorted.h"
#include "rt_kernel_plain.h"

/* waves per SIMD the f32 kernels are built for.  The Cornell variant V0 fits 4 (127 VGPRs, no spill).  The feature-rich variants do
 * not: held to 128 registers they spill 140-200 of them (and the reordering kernels missed the bound anyway: 3 and 2 waves), so
 * they are built for 3 like their f64 forms (static figures: hipcc -Rpass-analysis=kernel-resource-usage, tools/kernel_resources.py). */
#define RT_F32_WAVES(Cfg) ((Cfg::sweep && !Cfg::media && !Cfg::tex && !Cfg::msphere) ? 4 : 3)
template <class Cfg>
__global__ __launch_bounds__(RT_BLOCK, RT_F32_WAVES(Cfg)) void rt_render_kernel_f32(RtSceneView sc, RtFrame f, rt_f64* __restrict__ partial, unsigned long long* __restrict__ counters) {
    rt_render_plain_body<Cfg, false>(sc, f, partial, counters);
}
/* the reordering kernels: 3 for both variants.  The feature-rich one needs a register or two around the 168 of that step (167 with the
 * two-XOR Philox round, 169 with the three-input one when left to the f64 form's bound of 2 waves); held to 168 it spills nothing */
#define RT_F32_SORT_WAVES 3
template <class Cfg>
__global__ __launch_bounds__(RT_SORT_BLOCK, RT_F32_SORT_WAVES) void rt_render_kernel_sorted_f32(RtSceneView sc, RtFrame f, rt_f64* __restrict__ partial, unsigned long long* __restrict__ counters) {
    rt_render_sorted_body<Cfg>(sc, f, partial, counters);
}
/* the stack-walk variants with the finished paths reordered at the end of every slice (rt_kernel_plain.h: rt_render_ss_body) */
template <class Cfg>
__global__ __launch_bounds__(RT_BLOCK, RT_F32_WAVES(Cfg)) void rt_render_kernel_ss_f32(RtSceneView sc, RtFrame f, rt_f64* __restrict__ partial, unsigned long long* __restrict__ counters) {
    rt_render_ss_body<Cfg, RT_STACK_CAP, 3>(sc, f, partial, counters);
}
/* sphere scenes: the pair walk (rt_walk_pair.h: inner boxes and group boxes are both this build's f32 boxes, widened like every BVH box of
 * this mode) in slices + the reordering of the finished paths */
__global__ __launch_bounds__(RT_BLOCK, 3) void rt_render_kernel_pw_ss_f32(RtSceneView sc, RtPwView pw, RtFrame f, rt_f64* __restrict__ partial, unsigned long long* __restrict__ counters) {
    rt_render_ss_body<RtCfgV5, RT_PW_SS_STACK, RT_PW_SS_PARTS, true>(sc, f, partial, counters, &pw);
}
typedef void (*kernel_t)(RtSceneView, RtFrame, rt_f64*, unsigned long long*);
static kernel_t const g_plain[RT_N_VARIANTS] = {rt_render_kernel_f32<RtCfgV0>, rt_render_kernel_f32<RtCfgV1>, rt_render_kernel_f32<RtCfgV2>, rt_render_kernel_f32<RtCfgV3>,
                                                nullptr, rt_render_kernel_f32<RtCfgV5>};
static kernel_t const g_sorted[RT_N_VARIANTS] = {rt_render_kernel_sorted_f32<RtCfgV0>, rt_render_kernel_sorted_f32<RtCfgV1>, rt_render_kernel_ss_f32<RtCfgV2>,
                                                 rt_render_kernel_ss_f32<RtCfgV3>, nullptr, rt_render_kernel_ss_f32<RtCfgV5>};
} // namespace RT_F32_NS

#undef double

#endif
