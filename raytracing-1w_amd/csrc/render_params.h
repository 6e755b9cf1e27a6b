/* render_params.h -- what every entry refuses in an rt1w_render_params, the kernels' frame of one and their view of a committed scene:
 * one text for the entries of librt1w.so (context.hip, features.hip) and for the AOV kernels' CPU twin (aov_host.cpp), which is the
 * expected side of the GPU tests and so refuses exactly what the entries refuse.  Host code only. */
#ifndef RT1W_RENDER_PARAMS_H
#define RT1W_RENDER_PARAMS_H

#include "scene.h"

namespace rt1w {
/* RT1W_OK, or the error code with its text in *why (optional) */
inline int params_check(const rt1w_render_params* p, const char** why) {
    const auto refuse = [why](int rc, const char* text) { if (why) *why = text; return rc; };
    if (p->width < 2 || p->height < 2) return refuse(RT1W_ERR_INVALID, "width and height must be >= 2 (u,v divide by W-1, H-1; main.rs:968-969)");
    if (p->tile_w == 0 || p->tile_h == 0 || (uint64_t)p->x0 + p->tile_w > p->width || (uint64_t)p->y0 + p->tile_h > p->height)
        return refuse(RT1W_ERR_INVALID, "tile outside the image");
    if (p->spp == 0) return refuse(RT1W_ERR_INVALID, "spp must be > 0");
    if ((p->strip_rows == 0) != (p->strip_period == 0) || p->strip_period < p->strip_rows)
        return refuse(RT1W_ERR_INVALID, "strip_rows / strip_period: both 0, or 0 < strip_rows <= strip_period");
    if (p->precision != RT1W_PRECISION_F64 && p->precision != RT1W_PRECISION_F32) return refuse(RT1W_ERR_UNSUPPORTED, "unknown precision");
    if (p->strip_rows) {
        const uint64_t last = (uint64_t)p->tile_h - 1u;
        const uint64_t j = (uint64_t)p->y0 + (last / p->strip_rows) * p->strip_period + last % p->strip_rows;
        if (j >= p->height) return refuse(RT1W_ERR_INVALID, "interleaved tile: last strip outside the image");
    }
    if ((uint64_t)p->sample_offset + p->spp > 0xFFFFFFFFull) return refuse(RT1W_ERR_INVALID, "sample index overflow");
    return RT1W_OK;
}

/* the frame of a render of `p`, but for its chunking (chunk, n_chunks: the caller's) */
inline RtFrame frame_of(const rt1w_render_params* p) {
    RtFrame f{};
    f.width = p->width; f.height = p->height;
    f.x0 = p->x0; f.y0 = p->y0; f.tile_w = p->tile_w; f.tile_h = p->tile_h;
    f.spp = p->spp; f.sample_offset = p->sample_offset; f.max_depth = p->max_depth; f.global_seed = p->global_seed;
    f.strip_rows = p->strip_rows; f.strip_period = p->strip_period;
    f.probe = (p->flags & RT1W_PROBE_COHERENT) ? 1u : 0u;
    return f;
}

/* the view of a committed scene, but for its six arrays (the caller's: device copies, or the scene's own vectors) */
inline RtSceneView view_of(const rt1w_scene& s) {
    RtSceneView v{};
    v.root = s.flat_root; v.n_nodes = (uint32_t)s.flat_nodes.size(); v.n_lights = (uint32_t)s.flat_lights.size();
    v.n_materials = (uint32_t)s.materials.size(); v.n_textures = (uint32_t)s.textures.size();
    v.camera = s.camera; v.background = s.background;
    return v;
}
} // namespace rt1w

#endif
