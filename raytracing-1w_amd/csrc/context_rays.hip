/* context_rays.hip -- the f64 render kernels a third time, in their RAY-LIST FORM (rt1w_ray_color: ray_color, main.rs:51-116 and :118-190,
 * for a list of the caller's own rays).
 *
 * The pattern of context_tiles.hip: this unit compiles the SAME bodies (rt_kernel_sorted.h, rt_kernel_plain.h, rt_walk_pair.h) behind the
 * same entry points with the same launch bounds (rt_kernels.h), with RT_RAY_LIST defined, inside a namespace of its own so that nothing of
 * it can meet the other builds at link time.  With the switch a kernel takes the ray list as one more argument; a work item is a chunk of
 * samples of one RAY, item = chunk * roundup(n, 64) + r, and a sample begins on the ray's record and at the ray's stream position instead
 * of the camera's (rt_kernel_sorted.h: the RT_ITEM_* macros; rt_ray_list.h).  Traversal, shading, draw order, slices, reordering, segment
 * counting and the order of every sum are the text the default kernels are built from, so the camera's own rays give the bits of
 * rt1w_render_device.  context.hip gets the kernels as host handles and launches them like its own (render_launch).
 *
 * Built: the set of context_tiles.hip -- what render_plan reaches with RT1W_GENERIC.  A scene-specialised (hiprtc) kernel has no
 * ray-list form: a context that holds one runs these. */
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#define RT_RAY_LIST 1
#define RT_NO_PROBE 1 /* RT1W_PROBE_COHERENT does not exist in this form */

namespace rtrays {
#include "rt1w_num.h"
#include "rt_flat.h"
#include "rt_core.h"
#include "rt_kernel_plain.h"
#include "rt_kernels.h"

typedef void (*kernel_t)(RtSceneView, RtFrame, double*, unsigned long long*, RtRayList);
typedef void (*pw_kernel_t)(RtSceneView, RtPwView, RtFrame, double*, unsigned long long*, RtRayList);
/* by walk form (context.h: RtWalkForm) and variant, as context.hip's g_kernels; nullptr: no ray-list form */
static kernel_t const g_rays[8][RT_N_VARIANTS] = {
    {nullptr, nullptr, nullptr, nullptr, rt_render_kernel<RtCfgV4>, nullptr},
    {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr},
    {nullptr, nullptr, rt_render_kernel_ss<RtCfgV2, RT_SS_CAP, 3>, rt_render_kernel_ss<RtCfgV3, RT_SS_CAP, 3>, nullptr, rt_render_kernel_ss<RtCfgV5, RT_SS_CAP, 3>},
    {nullptr, nullptr, nullptr, rt_render_kernel_ss<RtCfgSphereMedia<RtCfgV3>, RT_SS_CAP, 3>, rt_render_kernel_ss<RtCfgSphereMedia<RtCfgV4>, RT_SS_CAP, 3>, nullptr},
    {nullptr, nullptr, rt_render_kernel_ss_hc<RtCfgV2>, rt_render_kernel_ss_hc<RtCfgV3>, nullptr, rt_render_kernel_ss_hc<RtCfgV5>},
    {nullptr, nullptr, nullptr, rt_render_kernel_ss_hc<RtCfgSphereMedia<RtCfgV3>>, rt_render_kernel_ss_hc<RtCfgSphereMedia<RtCfgV4>>, nullptr},
    {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr},
    {rt_render_kernel_sorted<RtCfgV0>, rt_render_kernel_sorted<RtCfgV1>, nullptr, nullptr, nullptr, nullptr}};
static pw_kernel_t const g_rays_pw[2] = {rt_render_kernel_pw<RtCfgV5>, rt_render_kernel_pw_ss<RtCfgV5>};
} // namespace rtrays

/* the kernels' host handles for context.hip: their arguments are the bytes of its RtSceneView / RtPwView / RtFrame (same headers, same
 * layout: checked through rt1w_internal_ray_sizeof) and, last, an RtRayList.  nullptr: no such kernel */
extern "C" const void* rt1w_internal_ray_kernel(int walk, int variant) {
    return walk >= 0 && walk < 8 && variant >= 0 && variant < RT_N_VARIANTS ? reinterpret_cast<const void*>(rtrays::g_rays[walk][variant]) : nullptr;
}
extern "C" const void* rt1w_internal_ray_pw_kernel(int which) { return which == 0 || which == 1 ? reinterpret_cast<const void*>(rtrays::g_rays_pw[which]) : nullptr; }
/* bytes of its 0 RtSceneView, 1 RtFrame, 2 RtPwView, 3 RtRayList */
extern "C" unsigned rt1w_internal_ray_sizeof(int what) {
    return what == 0 ? (unsigned)sizeof(rtrays::RtSceneView) : what == 1 ? (unsigned)sizeof(rtrays::RtFrame)
         : what == 2 ? (unsigned)sizeof(rtrays::RtPwView) : (unsigned)sizeof(rtrays::RtRayList);
}
