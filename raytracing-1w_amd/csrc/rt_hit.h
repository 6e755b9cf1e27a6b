/* rt_hit.h -- ray queries (rt1w_hit, include/rt1w.h): Hittable::hit(ray, t_min, t_max, rng) -> Option<HitRecord> (hittable.rs:63-64,
 * HitRecord hittable.rs:10-18) of the scene's world for one caller-given ray.  Compiled by the query kernels (hit.hip) and by the CPU
 * twin of the diagnostics library (aov_host.cpp) from this one text.
 *
 * Made of rt_closest_hit and rt_finish_hit only: the walk is the scene variant's own, in the reference's order (bvh.rs:25-50), with the
 * caller's t_min / t_max where the first segment of a beauty path has 0.001 / inf (main.rs:62); ties and the MovingSphere time are
 * rt_closest_hit's.  The direction is used as given: t is in units of it.  A ConstantMedium draws (constant_medium.rs:58-113) from the
 * stream rt_rng_pixel_sample(first_stream + r, sample, global_seed) of ray r, starting at its first word: nothing else draws, so the
 * records of a ray do not depend on the call it is part of.  Nothing here is reached by the render kernels. */
#ifndef RT_HIT_H
#define RT_HIT_H

#include "rt_core.h"

#define RT_HIT_RAY 9      /* doubles of a ray record: origin 3, direction 3, time, t_min, t_max */
#define RT_HIT_RECORD 12  /* doubles of a hit record: hit, t, p 3, normal 3, u, v, front_face, material */

/* rt1w_hit_params (include/rt1w.h), the same 32 bytes */
struct RtHitParams {
    uint64_t n, first_stream, global_seed;
    uint32_t sample, flags;
};

/* What rt1w_hit, rt1w_hit_device and the twin refuse of a call once its pointers are there, in the order they look; null = nothing.
 * The buffers: rays n * 72 bytes, out n * 96, out_node (may be null) n * 4 */
inline const char* rt_hit_refusal(const RtHitParams& p, const void* rays, const void* out, const void* out_node) {
    if (p.n == 0u || p.n > 0xFFFFFFFFull) return "ray query: n must be 1 .. 2^32 - 1";
    if (p.global_seed > 0xFFFFFFFFull) return "ray query: global_seed must be below 2^32";
    if (p.flags & ~(0xFFu << 8)) return "ray query: unknown flag (flags: 0 or RT1W_FORCE_VARIANT)";
    const auto overlap = [](const void* a, uint64_t na, const void* b, uint64_t nb) {
        const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
        return x < y + nb && y < x + na;
    };
    const uint64_t ray_bytes = p.n * RT_HIT_RAY * sizeof(double), out_bytes = p.n * RT_HIT_RECORD * sizeof(double), node_bytes = p.n * sizeof(uint32_t);
    if (overlap(rays, ray_bytes, out, out_bytes) || (out_node && (overlap(rays, ray_bytes, out_node, node_bytes) || overlap(out, out_bytes, out_node, node_bytes))))
        return "ray query: out and out_node must not overlap rays or each other";
    return nullptr;
}

/* finite: neither an infinity nor a NaN (the exponent field is not all ones) */
RT_HD bool rt_hit_finite(double x) { return (rt_d2u(x) & 0x7FF0000000000000ull) != 0x7FF0000000000000ull; }

/* Ray `r` of a call (ray = its RT_HIT_RAY doubles) into out[RT_HIT_RECORD] and `node`.
 * THE ONE DEVIATION from the literal hit(): a ray with a non-finite origin, direction or time, or with a NaN for t_min or t_max, is
 * answered as a miss without a walk of its own.  Its lane still calls the walk -- the walks vote wave-wide (RT_WAVE_ANY) -- on a fixed
 * finite ray with the empty interval (0.001, 0), in which no box and no primitive is hit and no medium draws.  Everything else is
 * literal: a zero direction, t_min > t_max, a t_max of +inf. */
template <class Cfg, class Stack, class NS>
RT_HD void rt_hit_ray(const RtSceneView& sc, const NS& ns, const double* ray, uint64_t r, const RtHitParams& hp, Stack& stk, double* out,
                      uint32_t& node) {
    RtRay q;
    q.o = rt_v3(ray[0], ray[1], ray[2]); q.d = rt_v3(ray[3], ray[4], ray[5]); q.time = ray[6];
    double t_min = ray[7], t_max = ray[8];
    bool refused = rt_isnan(t_min) | rt_isnan(t_max);
    for (int k = 0; k < 7; ++k) refused |= !rt_hit_finite(ray[k]);
    if (refused) {
        q.o = rt_v3(RT_R(0.0), RT_R(0.0), RT_R(0.0)); q.d = rt_v3(RT_R(0.0), RT_R(0.0), RT_R(1.0)); q.time = RT_R(0.0);
        t_min = RT_R(0.001); t_max = RT_R(0.0);
    }
    RtRng rng = rt_rng_pixel_sample(hp.first_stream + r, hp.sample, (uint32_t)hp.global_seed);
    double t;
    uint32_t prim, scope;
    const bool found = rt_closest_hit<Cfg>(sc, ns, q, t_min, t_max, rng, stk, t, prim, scope) & !refused;
    if (!found) {
        for (int k = 0; k < RT_HIT_RECORD; ++k) out[k] = RT_R(0.0);
        node = RT_NONE;
        return;
    }
    RtHit h;
    rt_finish_hit<Cfg>(sc, q, prim, scope, t, h);
    out[0] = RT_R(1.0); out[1] = t;
    out[2] = h.p.x; out[3] = h.p.y; out[4] = h.p.z;
    out[5] = h.n.x; out[6] = h.n.y; out[7] = h.n.z;
    out[8] = h.u; out[9] = h.v;
    out[10] = h.front ? RT_R(1.0) : RT_R(0.0);
    out[11] = (double)RT_MAT_INDEX(h.mat);
    node = prim;
}

#endif
