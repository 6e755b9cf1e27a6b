/* context_tiles.hip -- the f64 render kernels once more, in their TILE-LIST FORM (rt1w_render_tiles: a list of square tiles of the image
 * rendered by one launch).
 *
 * The pattern of context_ref.hip: this unit compiles the SAME bodies (rt_kernel_sorted.h, rt_kernel_plain.h, rt_walk_pair.h) behind the
 * same entry points with the same launch bounds (rt_kernels.h) a second time, with RT_TILE_LIST defined, inside a namespace of its own so
 * that nothing of it can meet the default build at link time.  With the switch a kernel takes the tile table as one more argument and
 * maps a pixel of its (virtual) tile to the image through it (rt_kernel_sorted.h: rt_tile_item); traversal, shading, draw order and the
 * order of every sum are the text the default kernels are built from, so a tile's pixels are the bits of rt1w_render_device on its
 * rectangle.  context.hip gets the kernels as host handles and launches them like its own (render_launch).
 *
 * Built: the kernels render_plan reaches with flags 0 on a context without a scene-specialised kernel -- the reordering kernels of V0 and
 * V1, the stack walks that reorder the finished paths (with and without the node cache, with and without the sphere-media build), the
 * pair walks of sphere scenes, and the plain kernel V4 falls back to.  The tile-list form of a scene-specialised kernel is generated and
 * compiled like its rectangle form (jit.cpp: jit_source with `tiles`, the two switches below ahead of its includes) and is no part of
 * this unit. */
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#define RT_TILE_LIST 1
#define RT_NO_PROBE 1 /* RT1W_PROBE_COHERENT does not exist in this form */

namespace rttile {
#include "rt1w_num.h"
#include "rt_flat.h"
#include "rt_core.h"
#include "rt_kernel_plain.h"
#include "rt_kernels.h"

typedef void (*kernel_t)(RtSceneView, RtFrame, double*, unsigned long long*, RtTileList);
typedef void (*pw_kernel_t)(RtSceneView, RtPwView, RtFrame, double*, unsigned long long*, RtTileList);
/* by walk form (context.h: RtWalkForm) and variant, as context.hip's g_kernels; nullptr: no tile form */
static kernel_t const g_tile[8][RT_N_VARIANTS] = {
    {nullptr, nullptr, nullptr, nullptr, rt_render_kernel<RtCfgV4>, nullptr},
    {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr},
    {nullptr, nullptr, rt_render_kernel_ss<RtCfgV2, RT_SS_CAP, 3>, rt_render_kernel_ss<RtCfgV3, RT_SS_CAP, 3>, nullptr, rt_render_kernel_ss<RtCfgV5, RT_SS_CAP, 3>},
    {nullptr, nullptr, nullptr, rt_render_kernel_ss<RtCfgSphereMedia<RtCfgV3>, RT_SS_CAP, 3>, rt_render_kernel_ss<RtCfgSphereMedia<RtCfgV4>, RT_SS_CAP, 3>, nullptr},
    {nullptr, nullptr, rt_render_kernel_ss_hc<RtCfgV2>, rt_render_kernel_ss_hc<RtCfgV3>, nullptr, rt_render_kernel_ss_hc<RtCfgV5>},
    {nullptr, nullptr, nullptr, rt_render_kernel_ss_hc<RtCfgSphereMedia<RtCfgV3>>, rt_render_kernel_ss_hc<RtCfgSphereMedia<RtCfgV4>>, nullptr},
    {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr},
    {rt_render_kernel_sorted<RtCfgV0>, rt_render_kernel_sorted<RtCfgV1>, nullptr, nullptr, nullptr, nullptr}};
static pw_kernel_t const g_tile_pw[2] = {rt_render_kernel_pw<RtCfgV5>, rt_render_kernel_pw_ss<RtCfgV5>};
} // namespace rttile

/* the kernels' host handles for context.hip: their arguments are the bytes of its RtSceneView / RtPwView / RtFrame (same headers, same
 * layout: checked through rt1w_internal_tile_sizeof) and, last, an RtTileList.  nullptr: no such kernel */
extern "C" const void* rt1w_internal_tile_kernel(int walk, int variant) {
    return walk >= 0 && walk < 8 && variant >= 0 && variant < RT_N_VARIANTS ? reinterpret_cast<const void*>(rttile::g_tile[walk][variant]) : nullptr;
}
extern "C" const void* rt1w_internal_tile_pw_kernel(int which) { return which == 0 || which == 1 ? reinterpret_cast<const void*>(rttile::g_tile_pw[which]) : nullptr; }
/* bytes of its 0 RtSceneView, 1 RtFrame, 2 RtPwView, 3 RtTileList */
extern "C" unsigned rt1w_internal_tile_sizeof(int what) {
    return what == 0 ? (unsigned)sizeof(rttile::RtSceneView) : what == 1 ? (unsigned)sizeof(rttile::RtFrame)
         : what == 2 ? (unsigned)sizeof(rttile::RtPwView) : (unsigned)sizeof(rttile::RtTileList);
}
