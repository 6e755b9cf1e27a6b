/* aov_host.cpp -- the CPU twin of the AOV kernels (aov.hip, aov_tiles.hip) and of the ray-query kernels (hit.hip) and the ray-list form of the render kernels (context_rays.hip) and of the path-state kernels (path_step.hip): rt_aov.h, rt_aov_deep.h, rt_aov_tiles.h, rt_hit.h and rt_path_state.h compiled for the host (g++, -ffp-contract=off
 * like every build of the core) and run over a committed scene's flat arrays.  Diagnostics library only (librt1w_lab.so): the expected side of the GPU
 * tests' bit-equality checks and of the CPU tier's checks against the literal oracle.  librt1w.so keeps no CPU render path. */
#include <algorithm>
#include <cstring>
#include <thread>
#include <vector>

#include "render_params.h"
#include "rt1w_internal.h" /* rt1w_internal_set_error: the twin of rt1w_ray_color says why it refuses, as the entries do */
#include "rt_adaptive_plan.h" /* rt_aov_tiles_check */
#include "rt_aov_deep.h"
#include "rt_aov_tiles.h"
#include "rt_hit.h"
#include "rt_ray_list.h"
#include "rt_path_state.h"
#include "walk_lab.h"

namespace {
struct AovHostStack {
    uint32_t e[RT_STACK_CAP];
    int sp = 0;
    bool overflow = false;
    void push(uint32_t v) { if (sp >= RT_STACK_CAP) { overflow = true; return; } e[sp++] = v; }
    void poke(int above, uint32_t v) { if (sp + above >= RT_STACK_CAP) { overflow = true; return; } e[sp + above] = v; }
    uint32_t pop() { return e[--sp]; }
};

/* what the deep entry adds to a call; max_specular < 0: the first-hit buffers of rt_aov.h */
struct AovDeep {
    long max_specular = -1;
    double max_fuzz = 0.0;
    uint8_t* lengths = nullptr; /* [tile_h][tile_w][spp] rays per sample, optional */
};

template <class Cfg>
bool aov_rows(const RtSceneView& sc, const RtFrame& f, const AovDeep& d, uint32_t row0, uint32_t row_step, double* out, uint64_t* rays) {
    AovHostStack stk;
    RtGlobalNodes ns{sc.nodes};
    for (uint32_t py = row0; py < f.tile_h; py += row_step)
        for (uint32_t px = 0; px < f.tile_w; ++px) {
            const size_t pix = (size_t)py * f.tile_w + px;
            if (d.max_specular < 0) {
                rt_aov_pixel<Cfg>(sc, ns, f, px, py, stk, out + pix * RT_AOV_CHANNELS);
                *rays += f.spp;
            } else {
                *rays += rt_aov_deep_pixel<Cfg>(sc, ns, f, px, py, (uint32_t)d.max_specular, d.max_fuzz, stk, out + pix * RT_AOV_CHANNELS,
                                                d.lengths ? d.lengths + pix * f.spp : nullptr);
            }
            if (stk.overflow) return false;
        }
    return true;
}
/* run(Cfg{}) for the Cfg of variant v: the variants the kernels are built for */
template <class Run>
bool with_variant(int v, Run run) {
    switch (v) {
        case 0: return run(RtCfgV0{});
        case 1: return run(RtCfgV1{});
        case 2: return run(RtCfgV2{});
        case 4: return run(RtCfgV4{});
        case 5: return run(RtCfgV5{});
        default: return run(RtCfgV3{});
    }
}

/* the kernels' view of a committed scene over its own vectors (`nodes`: with the spare record the context's node array carries) and the
 * variant the entries run: the scene's, or the one p's RT1W_FORCE_VARIANT names.  false: that variant does not cover the scene */
bool host_view(const rt1w_scene* s, uint32_t flags, std::vector<RtNode>& nodes, RtSceneView& sc, int& v) {
    const uint32_t n_nodes = (uint32_t)s->flat_nodes.size();
    v = rt_pick_variant(n_nodes, s->has_media, s->has_tex, s->has_msphere, s->scope_depth, s->walk_annotated != 0u);
    if ((flags >> 8) & 0xFFu) {
        v = (int)((flags >> 8) & 0xFFu) - 1;
        if (!rt_variant_valid(v, n_nodes, s->has_media, s->has_tex, s->has_msphere, s->scope_depth)) return false;
    }
    nodes = s->flat_nodes;
    nodes.push_back(RtNode{});
    sc = rt1w::view_of(*s);
    sc.nodes = nodes.data(); sc.lights = s->flat_lights.data(); sc.materials = s->materials.data(); sc.textures = s->textures.data();
    sc.perlin = s->perlin.data(); sc.images = s->images.data();
    return true;
}
constexpr uint32_t MAX_THREADS = 16u;
/* `work` items dealt round-robin over at most MAX_THREADS threads: part(t, n_threads) does items t, t + n_threads, ..  Every pixel is computed whole
 * by one thread, so the result does not depend on their number.  false: a part returned false (a traversal stack overflowed) */
template <class Part>
bool round_robin(uint32_t work, Part part) {
    const unsigned hw = std::thread::hardware_concurrency();
    const uint32_t n_threads = std::max(1u, std::min({(uint32_t)hw, MAX_THREADS, work}));
    std::vector<char> ok(n_threads, 1);
    std::vector<std::thread> pool;
    for (uint32_t t = 1; t < n_threads; ++t) pool.emplace_back([&, t]() { ok[t] = part(t, n_threads) ? 1 : 0; });
    ok[0] = part(0u, n_threads) ? 1 : 0;
    for (auto& th : pool) th.join();
    for (char k : ok) if (!k) return false;
    return true;
}

int aov_host_run(const rt1w_scene* s, const rt1w_render_params* p, const AovDeep& deep, double* out, uint64_t* segments) {
    if (!s || !p || !out || !s->committed) return RT1W_ERR_INVALID;
    if (const int rc = rt1w::params_check(p, nullptr); rc < 0) return rc; /* the entries' own check: the twin refuses what they refuse */
    if ((p->flags & ~(0xFFu << 8)) != 0u) return RT1W_ERR_INVALID;
    if (p->precision != RT1W_PRECISION_F64) return RT1W_ERR_UNSUPPORTED;
    std::vector<RtNode> nodes;
    RtSceneView sc;
    int v;
    if (!host_view(s, p->flags, nodes, sc, v)) return RT1W_ERR_INVALID;
    RtFrame f = rt1w::frame_of(p);
    f.max_depth = 1u; f.chunk = p->spp; f.n_chunks = 1u;
    uint64_t rays[MAX_THREADS] = {}; /* per thread */
    const bool ok = round_robin(f.tile_h, [&](uint32_t t, uint32_t n_threads) { /* the tile's rows */
        return with_variant(v, [&](auto cfg) { return aov_rows<decltype(cfg)>(sc, f, deep, t, n_threads, out, &rays[t]); });
    });
    if (!ok) return RT1W_ERR_STATE;
    if (segments) { *segments = 0u; for (uint64_t r : rays) *segments += r; }
    return RT1W_OK;
}

/* the tiles of a list k0, k0 + step, ..: every pixel of a tile by rt_aov_tiles_pixel, as the kernel's lanes run it */
template <class Cfg>
bool aov_tiles(const RtSceneView& sc, const RtFrame& f, uint32_t tile, const rt1w_tile* tiles, uint32_t n, uint32_t k0, uint32_t step, double* out) {
    AovHostStack stk;
    RtGlobalNodes ns{sc.nodes};
    for (uint32_t k = k0; k < n; k += step)
        for (uint32_t ly = 0; ly < tile; ++ly)
            for (uint32_t lx = 0; lx < tile; ++lx) {
                rt_aov_tiles_pixel<Cfg>(sc, ns, f, tile, k, tiles[k].x0, tiles[k].y0, tiles[k].sample_offset, lx, ly, stk, out);
                if (stk.overflow) return false;
            }
    return true;
}

/* rays k0, k0 + step, .. of a query list by rt_hit_ray, as the kernel's lanes run them */
template <class Cfg>
bool hit_rays(const RtSceneView& sc, const RtHitParams& hp, uint64_t k0, uint64_t step, const double* rays, double* out, uint32_t* out_node) {
    AovHostStack stk;
    RtGlobalNodes ns{sc.nodes};
    for (uint64_t r = k0; r < hp.n; r += step) {
        uint32_t node;
        rt_hit_ray<Cfg>(sc, ns, rays + r * RT_HIT_RAY, r, hp, stk, out + r * RT_HIT_RECORD, node);
        if (stk.overflow) return false;
        if (out_node) out_node[r] = node;
    }
    return true;
}

/* rays k0, k0 + step, .. of a radiance list, as the ray-list kernels run them (rt_kernel_sorted.h with RT_RAY_LIST): per ray, per work item
 * of f.chunk samples, per sample rt_ray_begin and rt_path_step until the path ends; the items' sums added in order (rt_resolve_kernel) */
template <class Cfg>
bool ray_color_rays(const RtSceneView& sc, const RtFrame& f, const RtRayList& rl, bool out_sum, uint64_t k0, uint64_t step, double* out, uint64_t* segments,
                    uint32_t* ray_segments) {
    AovHostStack stk;
    RtGlobalNodes ns{sc.nodes};
    for (uint64_t r = k0; r < rl.n; r += step) {
        const bool traced = rt_ray_traced(rl.rays + r * (uint64_t)rl.stride);
        const uint64_t before = *segments;
        RtV3 total = rt_v3(0.0, 0.0, 0.0);
        for (uint32_t chunk = 0; chunk < f.n_chunks; ++chunk) {
            const uint32_t s0 = chunk * f.chunk, s_end = s0 + f.chunk < f.spp ? s0 + f.chunk : f.spp;
            RtV3d sum = rt_v3d(0.0, 0.0, 0.0);
            if (!traced) sum = rt_ray_untraced_sum(sc, f.max_depth, s_end - s0);
            else
                for (uint32_t s = s0; s < s_end; ++s) {
                    RtPath path;
                    rt_ray_begin(rl, f.global_seed, f.max_depth, r, f.sample_offset + s, path);
                    while (path.alive) {
                        *segments += path.depth_left != 0u ? 1u : 0u;
                        rt_path_step<Cfg>(sc, ns, path, stk);
                        if (stk.overflow) return false;
                    }
                    sum = rt_v3d_add(sum, path.radiance);
                }
            total = total + rt_v3(sum.x, sum.y, sum.z);
        }
        if (!out_sum) total = rt_into_sampled(total, f.spp);
        out[r * 3u] = total.x; out[r * 3u + 1u] = total.y; out[r * 3u + 2u] = total.z;
        if (ray_segments) ray_segments[r] = (uint32_t)(*segments - before);
    }
    return true;
}

/* states k0, k0 + step, .. of a list by rt_state_advance, as the step kernel's lanes run them; a state is copied whole before it is
 * written, so `in` may be `out` */
template <class Cfg>
bool path_states(const RtSceneView& sc, const RtPathParams& pp, uint64_t k0, uint64_t step, const RtPathState* in, RtPathState* out, uint32_t* out_node,
                 uint64_t* segments) {
    AovHostStack stk;
    RtGlobalNodes ns{sc.nodes};
    for (uint64_t r = k0; r < pp.n; r += step) {
        RtPathState s;
        memcpy(&s, (const char*)in + r * sizeof s, sizeof s); /* the caller's states may have any alignment */
        uint32_t node;
        *segments += rt_state_advance<Cfg>(sc, ns, (uint32_t)pp.global_seed, pp.steps, s, stk, node);
        if (stk.overflow) return false;
        memcpy((char*)out + r * sizeof s, &s, sizeof s);
        if (out_node) out_node[r] = node;
    }
    return true;
}
} // namespace

extern "C" int rt1w_lab_path_step_host(const rt1w_scene* s, const rt1w_path_params* p, const rt1w_path_state* in, rt1w_path_state* out, uint32_t* out_node,
                                       uint64_t* segments) {
    static_assert(sizeof(rt1w_path_params) == sizeof(RtPathParams) && sizeof(rt1w_path_state) == sizeof(RtPathState), "the path blocks are the kernels' layouts");
    if (!s || !s->committed) { rt1w_internal_set_error("null or uncommitted scene"); return RT1W_ERR_INVALID; }
    if (const char* why = rt_path_step_refusal((const RtPathParams*)p, in, out, out_node, false)) { /* the entries' own check */
        rt1w_internal_set_error(why); return RT1W_ERR_INVALID;
    }
    RtPathParams pp;
    memcpy(&pp, p, sizeof pp);
    std::vector<RtNode> nodes;
    RtSceneView sc;
    int v;
    if (!host_view(s, p->flags, nodes, sc, v)) { rt1w_internal_set_error("path_step: the forced variant does not cover the scene"); return RT1W_ERR_INVALID; }
    uint64_t segs[MAX_THREADS] = {}; /* per thread */
    const bool ok = round_robin((uint32_t)pp.n, [&](uint32_t t, uint32_t n_threads) { /* the list's states */
        return with_variant(v, [&](auto cfg) {
            return path_states<decltype(cfg)>(sc, pp, t, n_threads, (const RtPathState*)in, (RtPathState*)out, out_node, &segs[t]);
        });
    });
    if (!ok) return RT1W_ERR_STATE;
    if (segments) { *segments = 0u; for (uint64_t k : segs) *segments += k; }
    return RT1W_OK;
}

extern "C" int rt1w_lab_path_begin_host(const rt1w_scene* s, uint32_t width, uint32_t height, uint64_t global_seed, uint32_t max_depth, const uint32_t* pixels,
                                        uint64_t n, rt1w_path_state* out) {
    if (!s || !s->committed) { rt1w_internal_set_error("null or uncommitted scene"); return RT1W_ERR_INVALID; }
    if (const char* why = rt_path_begin_refusal(width, height, global_seed, pixels, n, out, false)) { rt1w_internal_set_error(why); return RT1W_ERR_INVALID; }
    RtPathBeginParams bp;
    bp.n = n; bp.width = width; bp.height = height; bp.global_seed = (uint32_t)global_seed; bp.max_depth = max_depth;
    bool inside = true;
    for (uint64_t r = 0; r < n; ++r) {
        RtPathState st;
        inside &= rt_state_begin(s->camera, bp, pixels + r * 3u, st);
        memcpy((char*)out + r * sizeof st, &st, sizeof st);
    }
    if (!inside) { rt1w_internal_set_error("path_begin: a pixel of the list lies outside the frame (i >= width or j >= height)"); return RT1W_ERR_INVALID; }
    return RT1W_OK;
}

extern "C" int rt1w_lab_ray_color_counts_host(const rt1w_scene* s, const rt1w_ray_color_params* p, const double* rays, const uint32_t* start_word, double* out,
                                              uint64_t* segments, uint32_t* ray_segments) {
    static_assert(sizeof(rt1w_ray_color_params) == sizeof(RtRayColorParams), "rt1w_ray_color_params is RtRayColorParams' layout");
    if (!s || !s->committed) { rt1w_internal_set_error("null or uncommitted scene"); return RT1W_ERR_INVALID; }
    if (const char* why = rt_ray_color_refusal((const RtRayColorParams*)p, rays, start_word, out, RT1W_OUT_SUM, RT1W_GENERIC)) { /* the entries' own check */
        rt1w_internal_set_error(why); return RT1W_ERR_INVALID;
    }
    std::vector<RtNode> nodes;
    RtSceneView sc;
    int v;
    if (!host_view(s, 0u, nodes, sc, v)) return RT1W_ERR_INVALID;
    RtFrame f{};
    f.width = f.tile_w = (uint32_t)p->n; f.height = f.tile_h = 1u;
    f.spp = p->spp; f.sample_offset = p->sample_offset; f.max_depth = p->max_depth; f.global_seed = (uint32_t)p->global_seed;
    f.chunk = p->chunk ? p->chunk : rt1w_scene_default_chunk(s, (uint32_t)p->n, 1u, p->spp);
    if (f.chunk > f.spp) f.chunk = f.spp;
    f.n_chunks = (f.spp + f.chunk - 1u) / f.chunk;
    RtRayList rl;
    rl.rays = rays; rl.start_word = start_word; rl.n = p->n; rl.first_stream = p->first_stream;
    rl.stride = p->stride ? p->stride : (uint32_t)RT_RAY_RECORD; rl.pad = 0u;
    uint64_t segs[MAX_THREADS] = {}; /* per thread */
    const bool ok = round_robin((uint32_t)p->n, [&](uint32_t t, uint32_t n_threads) { /* the list's rays */
        return with_variant(v, [&](auto cfg) { return ray_color_rays<decltype(cfg)>(sc, f, rl, (p->flags & RT1W_OUT_SUM) != 0u, t, n_threads, out, &segs[t], ray_segments); });
    });
    if (!ok) return RT1W_ERR_STATE;
    if (segments) { *segments = 0u; for (uint64_t k : segs) *segments += k; }
    return RT1W_OK;
}

extern "C" int rt1w_lab_ray_color_host(const rt1w_scene* s, const rt1w_ray_color_params* p, const double* rays, const uint32_t* start_word, double* out,
                                       uint64_t* segments) {
    return rt1w_lab_ray_color_counts_host(s, p, rays, start_word, out, segments, nullptr);
}

extern "C" int rt1w_lab_hit_host(const rt1w_scene* s, const rt1w_hit_params* p, const double* rays, double* out, uint32_t* out_node) {
    static_assert(sizeof(rt1w_hit_params) == sizeof(RtHitParams), "rt1w_hit_params is RtHitParams' layout");
    if (!s || !p || !rays || !out || !s->committed) return RT1W_ERR_INVALID;
    RtHitParams hp;
    memcpy(&hp, p, sizeof hp);
    if (rt_hit_refusal(hp, rays, out, out_node)) return RT1W_ERR_INVALID; /* the entries' own check */
    std::vector<RtNode> nodes;
    RtSceneView sc;
    int v;
    if (!host_view(s, p->flags, nodes, sc, v)) return RT1W_ERR_INVALID;
    const bool ok = round_robin((uint32_t)hp.n, [&](uint32_t t, uint32_t n_threads) { /* the list's rays */
        return with_variant(v, [&](auto cfg) { return hit_rays<decltype(cfg)>(sc, hp, t, n_threads, rays, out, out_node); });
    });
    return ok ? RT1W_OK : RT1W_ERR_STATE;
}

/* what rt_debug_texture_kernel (context.hip) does per input, over the scene's host arrays */
extern "C" int rt1w_lab_texture_host(const rt1w_scene* s, int mode, uint32_t tex, const double* in, double* out, uint64_t n) {
    if (!s || !s->committed) { rt1w_internal_set_error("null or uncommitted scene"); return RT1W_ERR_INVALID; }
    if (!in || !out) { rt1w_internal_set_error("null argument"); return RT1W_ERR_INVALID; }
    if (n == 0) return RT1W_OK;
    if (const char* why = rt1w::debug_texture_refusal(mode, tex, in, out, s->textures.size(), s->perlin.size())) { /* the probe's own check */
        rt1w_internal_set_error(why); return RT1W_ERR_INVALID;
    }
    std::vector<RtNode> nodes;
    RtSceneView sc;
    int v;
    if (!host_view(s, 0u, nodes, sc, v)) return RT1W_ERR_INVALID;
    for (uint64_t i = 0; i < n; ++i) {
        const double u = in[i * 5], vv = in[i * 5 + 1];
        const RtV3 p = rt_v3(in[i * 5 + 2], in[i * 5 + 3], in[i * 5 + 4]);
        RtV3 r = rt_v3(0.0, 0.0, 0.0);
        if (mode == 0) r = rt_texture<RtCfgV1>(sc, tex, u, vv, p);
        else if (mode == 1) { r.x = rt_perlin_noise(sc.perlin[tex], p); r.y = rt_perlin_turb(sc.perlin[tex], p, 7); }
        else { double su, sv; rt_sphere_uv(p, su, sv); r.x = su; r.y = sv; }
        out[i * 3] = r.x; out[i * 3 + 1] = r.y; out[i * 3 + 2] = r.z;
    }
    return RT1W_OK;
}

extern "C" int rt1w_lab_camera_rays_pos_host(const rt1w_scene* s, const rt1w_render_params* p, double* out, uint32_t* out_word);
extern "C" int rt1w_lab_camera_rays_host(const rt1w_scene* s, const rt1w_render_params* p, double* out) { return rt1w_lab_camera_rays_pos_host(s, p, out, nullptr); }

extern "C" int rt1w_lab_camera_rays_pos_host(const rt1w_scene* s, const rt1w_render_params* p, double* out, uint32_t* out_word) {
    if (!s || !p || !out || !s->committed) return RT1W_ERR_INVALID;
    if (const int rc = rt1w::params_check(p, nullptr); rc < 0) return rc;
    if (p->precision != RT1W_PRECISION_F64) return RT1W_ERR_UNSUPPORTED;
    std::vector<RtNode> nodes;
    RtSceneView sc;
    int v;
    if (!host_view(s, 0u, nodes, sc, v)) return RT1W_ERR_INVALID;
    RtFrame f = rt1w::frame_of(p);
    f.max_depth = 1u; f.chunk = p->spp; f.n_chunks = 1u;
    double* o = out;
    for (uint32_t py = 0; py < f.tile_h; ++py)
        for (uint32_t px = 0; px < f.tile_w; ++px)
            for (uint32_t k = 0; k < f.spp; ++k, o += 8) {
                RtPath path;
                rt_path_begin(sc, f, f.x0 + px, rt_frame_row(f, py), f.sample_offset + k, path); /* what rt_aov_sample and the render kernels begin with */
                o[0] = path.ray.o.x; o[1] = path.ray.o.y; o[2] = path.ray.o.z;
                o[3] = path.ray.d.x; o[4] = path.ray.d.y; o[5] = path.ray.d.z;
                o[6] = path.ray.time; o[7] = 1.0; /* valid, as in rt1w_lab_dump_rays */
                if (out_word) *out_word++ = rt_rng_word(path.rng); /* where the sample's stream stands behind Camera::get_ray */
            }
    return RT1W_OK;
}

extern "C" int rt1w_lab_aov_tiles_host(const rt1w_scene* s, const rt1w_render_params* p, uint32_t tile, const rt1w_tile* tiles, uint32_t n_tiles, double* out) {
    if (!s || !p || !tiles || !out || !s->committed) return RT1W_ERR_INVALID;
    const char* why = nullptr;
    if (const int rc = rt_aov_tiles_check(p, tile, tiles, n_tiles, &why); rc < 0) return rc; /* the entries' own check */
    std::vector<RtNode> nodes;
    RtSceneView sc;
    int v;
    if (!host_view(s, p->flags, nodes, sc, v)) return RT1W_ERR_INVALID;
    RtFrame f = rt1w::frame_of(p);
    f.x0 = 0u; f.y0 = 0u; f.tile_w = tile; f.tile_h = n_tiles * tile;
    f.max_depth = 1u; f.chunk = p->spp; f.n_chunks = 1u;
    const bool ok = round_robin(n_tiles, [&](uint32_t t, uint32_t n_threads) { /* the list's tiles */
        return with_variant(v, [&](auto cfg) { return aov_tiles<decltype(cfg)>(sc, f, tile, tiles, n_tiles, t, n_threads, out); });
    });
    return ok ? RT1W_OK : RT1W_ERR_STATE;
}

extern "C" int rt1w_lab_aov_host(const rt1w_scene* s, const rt1w_render_params* p, double* out) { return aov_host_run(s, p, AovDeep{}, out, nullptr); }

extern "C" int rt1w_lab_aov_deep_host(const rt1w_scene* s, const rt1w_render_params* p, uint32_t max_specular, double max_fuzz, double* out,
                                      uint64_t* segments, uint8_t* lengths) {
    if (!rt_aov_deep_args_ok(max_specular, max_fuzz)) return RT1W_ERR_INVALID;
    AovDeep deep;
    deep.max_specular = (long)max_specular; deep.max_fuzz = max_fuzz; deep.lengths = lengths;
    return aov_host_run(s, p, deep, out, segments);
}

extern "C" int rt1w_lab_scene_set_camera(rt1w_scene* s, const double look_from[3], const double look_at[3], const double vup[3], double vfov_deg,
                                         double aspect_ratio, double aperture, double focus_dist, double time0, double time1) {
    if (!s || !s->committed) return RT1W_ERR_INVALID;
    RtCamera cam;
    const char* why = nullptr;
    if (const int rc = rt1w::camera_make(look_from, look_at, vup, vfov_deg, aspect_ratio, aperture, focus_dist, time0, time1, &cam, &why); rc < 0) return rc;
    s->camera = cam;
    return RT1W_OK;
}
extern "C" int rt1w_lab_scene_get_camera(const rt1w_scene* s, rt1w_camera* out) {
    if (!s || !out || !s->has_camera) return RT1W_ERR_INVALID;
    static_assert(sizeof(rt1w_camera) == sizeof(RtCamera), "rt1w_camera is RtCamera's layout");
    memcpy(out, &s->camera, sizeof *out);
    return RT1W_OK;
}
