/* rt_path_state.h -- path states (rt1w_path_step, rt1w_path_begin, include/rt1w.h): ray_color(ray, background, world, lights, depth, rng)
 * (main.rs:51-116, and :118-190 without lights) one level at a time, on a self-contained 128-byte record the caller keeps between calls.
 * Compiled by the kernels of path_step.hip and by the CPU twin of the diagnostics library (aov_host.cpp) from this one text.
 *
 * A level is rt_path_trace and rt_path_shade, the text of every render, between two conversions: the record's stream position becomes a
 * stream (rt_rng_at of rt_rng_pixel_sample) before it and a position again (rt_rng_word) behind it.  The blocks of a stream are a pure
 * function of key and counter, so a path taken level by level, in any split, order or company, draws what the same path draws inside a
 * render kernel.  Nothing here is reached by the render kernels. */
#ifndef RT_PATH_STATE_H
#define RT_PATH_STATE_H

#include "rt_ray_list.h" /* rt_ray_traced: the one deviation, shared with rt1w_ray_color */

/* rt1w_path_state (include/rt1w.h), the same 128 bytes */
struct RtPathState {
    double ray[RT_RAY_RECORD]; /* origin 3, direction 3, time: the NEXT ray to trace */
    double beta[3], radiance[3];
    uint64_t stream;
    uint32_t sample, word, depth_left, status;
};
static_assert(sizeof(RtPathState) == 128, "a path state is one 128-byte line");
/* rt1w_path_params (include/rt1w.h), the same 32 bytes */
struct RtPathParams {
    uint64_t n, global_seed;
    uint32_t steps, flags, reserved[2];
};
/* what the begin kernel takes: the frame's three numbers of rt_path_begin and the list's length */
struct RtPathBeginParams {
    uint64_t n;
    uint32_t width, height, global_seed, max_depth;
};

#define RT_PATH_ALIVE 1u       /* RT1W_PATH_ALIVE */
#define RT_PATH_TRACED 2u      /* RT1W_PATH_TRACED: a level of the entry produced this ray */
#define RT_PATH_EVENT_SHIFT 8  /* bits 8-15: the event of the last level taken */
#define RT_PATH_MAX_STEPS 65536u
enum {
    RT_PE_NONE = 0, RT_PE_MISS = 1, RT_PE_DEPTH = 2, RT_PE_LIGHT = 3, RT_PE_ABSORBED = 4, RT_PE_LAMBERTIAN = 5, RT_PE_METAL = 6,
    RT_PE_DIELECTRIC = 7, RT_PE_ISOTROPIC = 8, RT_PE_UNTRACED = 9
};

#if !defined(__HIP_DEVICE_COMPILE__)
/* What rt1w_path_step, rt1w_path_step_device and the twin refuse of a call, in the order they look; null = nothing (all RT1W_ERR_INVALID).
 * The buffers: in and out n * 128 bytes, the same pointer or apart; out_node (may be null) n * 4.  `device`: the kernels move a state as
 * eight 16-byte accesses, so device pointers are 16-byte aligned; the host entries copy and take any alignment */
inline const char* rt_path_step_refusal(const RtPathParams* p, const void* in, const void* out, const void* out_node, bool device) {
    if (!p || !in || !out) return "null argument";
    if (p->n == 0u || p->n > 0xFFFFFFFFull) return "path_step: n must be 1 .. 2^32 - 1";
    if (p->steps == 0u || p->steps > RT_PATH_MAX_STEPS) return "path_step: steps must be 1 .. 65536";
    if (p->global_seed > 0xFFFFFFFFull) return "path_step: global_seed must be below 2^32";
    if (p->flags & ~(0xFFu << 8)) return "path_step: unknown flag (flags: 0 or RT1W_FORCE_VARIANT)";
    if (p->reserved[0] != 0u || p->reserved[1] != 0u) return "path_step: reserved must be 0";
    if (device && ((((uintptr_t)in) | ((uintptr_t)out)) & 15u)) return "path_step: device states must be 16-byte aligned";
    const auto overlap = [](const void* a, uint64_t na, const void* b, uint64_t nb) {
        const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
        return x < y + nb && y < x + na;
    };
    const uint64_t bytes = p->n * sizeof(RtPathState), node_bytes = p->n * sizeof(uint32_t);
    if (in != out && overlap(in, bytes, out, bytes)) return "path_step: in and out must be the same buffer or apart";
    if (out_node && (overlap(in, bytes, out_node, node_bytes) || overlap(out, bytes, out_node, node_bytes))) return "path_step: out_node must not overlap the states";
    return nullptr;
}
/* ... and rt1w_path_begin, rt1w_path_begin_device and its twin, but for the pixels of the list, which the lanes look at (rt_state_begin).
 * Width and height as a render takes them (render_params.h: params_check).  The buffers: pixels n * 12 bytes, out n * 128 */
inline const char* rt_path_begin_refusal(uint32_t width, uint32_t height, uint64_t global_seed, const void* pixels, uint64_t n, const void* out, bool device) {
    if (!pixels || !out) return "null argument";
    if (width < 2u || height < 2u) return "width and height must be >= 2 (u,v divide by W-1, H-1; main.rs:968-969)";
    if (n == 0u || n > 0xFFFFFFFFull) return "path_begin: n must be 1 .. 2^32 - 1";
    if (global_seed > 0xFFFFFFFFull) return "path_begin: global_seed must be below 2^32";
    if (device && ((((uintptr_t)out) & 15u) || (((uintptr_t)pixels) & 3u))) return "path_begin: device states must be 16-byte aligned, pixels 4-byte";
    const uintptr_t x = (uintptr_t)pixels, y = (uintptr_t)out;
    if (x < y + n * sizeof(RtPathState) && y < x + n * 3u * sizeof(uint32_t)) return "path_begin: out must not overlap pixels";
    return nullptr;
}
#endif

/* the event of a level from what rt_path_trace found, before rt_path_shade runs: the hit leaf's material kind from the node's own
 * material word (rt_flat.h: RT_MAT_KINDF), the word rt_path_trace takes the path class from */
template <class NS>
RT_HD uint32_t rt_state_event(const NS& ns, uint32_t depth_left, const RtTrace& tr) {
    if (depth_left == 0u) return RT_PE_DEPTH;
    if (tr.prim == RT_NONE) return RT_PE_MISS;
    const uint32_t mk = RT_MAT_KINDF(ns.hot(tr.prim).mat) & 0xFFu;
    return mk == RT_MAT_DIFFUSE_LIGHT ? RT_PE_LIGHT : mk == RT_MAT_LAMBERTIAN ? RT_PE_LAMBERTIAN : mk == RT_MAT_METAL ? RT_PE_METAL
         : mk == RT_MAT_DIELECTRIC ? RT_PE_DIELECTRIC : mk == RT_MAT_ISOTROPIC ? RT_PE_ISOTROPIC : RT_PE_ABSORBED;
}

/* State `s` advanced by up to `steps` levels while it is alive; a dead state is left as it is, every bit.  node: the hit leaf of the last
 * level taken (RT_NONE: a miss, no level, a ray not traced); returns the levels that traced a ray, as rt1w_ray_color counts segments */
template <class Cfg, class Stack, class NS>
RT_HD uint32_t rt_state_advance(const RtSceneView& sc, const NS& ns, uint32_t global_seed, uint32_t steps, RtPathState& s, Stack& stk, uint32_t& node) {
    node = RT_NONE;
    uint32_t segments = 0u;
    if (!(s.status & RT_PATH_ALIVE)) return segments;
    bool traced = (s.status & RT_PATH_TRACED) != 0u;
    uint32_t event = RT_PE_NONE;
    RtPath p;
    p.ray.o = rt_v3(s.ray[0], s.ray[1], s.ray[2]);
    p.ray.d = rt_v3(s.ray[3], s.ray[4], s.ray[5]);
    p.ray.time = s.ray[6];
    p.beta = rt_v3(s.beta[0], s.beta[1], s.beta[2]);
    p.radiance = rt_v3(s.radiance[0], s.radiance[1], s.radiance[2]);
    p.depth_left = s.depth_left;
    p.alive = true;
    uint32_t word = s.word;
    if (!traced && !rt_ray_traced(s.ray)) {
        /* the caller's ray is not finite: a miss that is not traced, what rt1w_ray_color makes of such a ray (rt_ray_untraced_sum) */
        const RtV3 zero = rt_v3(RT_R(0.0), RT_R(0.0), RT_R(0.0));
        p.radiance = p.radiance + rt_mul(p.beta, p.depth_left == 0u ? zero : sc.background);
        p.alive = false;
        event = RT_PE_UNTRACED;
    }
    for (uint32_t k = 0; k < steps && p.alive; ++k) {
        p.rng = rt_rng_at(rt_rng_pixel_sample(s.stream, s.sample, global_seed), word);
        segments += p.depth_left != 0u ? 1u : 0u;
        const RtTrace tr = rt_path_trace<Cfg>(sc, ns, p, stk);
        event = rt_state_event(ns, p.depth_left, tr);
        node = p.depth_left == 0u ? (uint32_t)RT_NONE : tr.prim;
        rt_path_shade<Cfg>(sc, p, tr);
        word = rt_rng_word(p.rng);
        traced = true;
    }
    s.ray[0] = p.ray.o.x; s.ray[1] = p.ray.o.y; s.ray[2] = p.ray.o.z;
    s.ray[3] = p.ray.d.x; s.ray[4] = p.ray.d.y; s.ray[5] = p.ray.d.z;
    s.ray[6] = p.ray.time;
    s.beta[0] = p.beta.x; s.beta[1] = p.beta.y; s.beta[2] = p.beta.z;
    s.radiance[0] = p.radiance.x; s.radiance[1] = p.radiance.y; s.radiance[2] = p.radiance.z;
    s.word = word;
    s.depth_left = p.depth_left;
    s.status = (p.alive ? RT_PATH_ALIVE : 0u) | (traced ? RT_PATH_TRACED : 0u) | (event << RT_PATH_EVENT_SHIFT);
    return segments;
}

/* entry `pix` = {i, j, sample} of a begin list into a fresh state: Camera::get_ray (camera.rs:61-73, with the jitter of main.rs:964-971)
 * through rt_path_begin_cam.  false, and a state of zeros (dead), where the pixel lies outside the frame */
RT_HD bool rt_state_begin(const RtCamera& cam, const RtPathBeginParams& bp, const uint32_t* pix, RtPathState& s) {
    const uint32_t i = pix[0], j = pix[1], sample = pix[2];
    if (i >= bp.width || j >= bp.height) {
        for (int k = 0; k < RT_RAY_RECORD; ++k) s.ray[k] = RT_R(0.0);
        for (int k = 0; k < 3; ++k) { s.beta[k] = RT_R(0.0); s.radiance[k] = RT_R(0.0); }
        s.stream = 0u; s.sample = 0u; s.word = 0u; s.depth_left = 0u; s.status = 0u;
        return false;
    }
    RtFrame f{};
    f.width = bp.width; f.height = bp.height; f.global_seed = bp.global_seed; f.max_depth = bp.max_depth;
    RtPath p;
    rt_path_begin_cam(cam, f, i, j, sample, p);
    s.ray[0] = p.ray.o.x; s.ray[1] = p.ray.o.y; s.ray[2] = p.ray.o.z;
    s.ray[3] = p.ray.d.x; s.ray[4] = p.ray.d.y; s.ray[5] = p.ray.d.z;
    s.ray[6] = p.ray.time;
    s.beta[0] = p.beta.x; s.beta[1] = p.beta.y; s.beta[2] = p.beta.z;
    s.radiance[0] = p.radiance.x; s.radiance[1] = p.radiance.y; s.radiance[2] = p.radiance.z;
    s.stream = (uint64_t)j * bp.width + i;
    s.sample = sample;
    s.word = rt_rng_word(p.rng);
    s.depth_left = p.depth_left;
    s.status = RT_PATH_ALIVE;
    return true;
}

#endif
