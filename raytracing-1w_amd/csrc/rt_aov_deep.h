/* rt_aov_deep.h -- deep feature buffers (rt1w_render_aov_deep, include/rt1w.h): the 8 channels of rt_aov.h taken at the first vertex of
 * the sample's path that is not a specular surface.  Compiled by the deep AOV kernel (aov.hip) and by the CPU twin of the diagnostics
 * library (aov_host.cpp), from this one text.
 *
 * The sample starts as rt_aov_sample does and then steps the prefix of the beauty path through Dielectrics and through Metals whose
 * fuzz is at most max_fuzz, at most max_specular times.  The two scatter arms below restate the Metal and Dielectric arms of
 * rt_path_shade (rt_core.h) in the same order of operations and with the same draws, so the stream stays in step and the chain
 * followed is the chain beauty sample k follows; rt_path_shade itself is not called, so that its Lambertian and light-sampling code
 * stays out of a kernel that never runs it.  Nothing here is reached by the render kernels or by the first-hit entries. */
#ifndef RT_AOV_DEEP_H
#define RT_AOV_DEEP_H

#include "rt_aov.h"

#define RT_AOV_DEEP_MAX_SPECULAR 64u /* rt1w_render_aov_deep refuses more */

/* what the deep entries and the twin refuse (include/rt1w.h): more than RT_AOV_DEEP_MAX_SPECULAR bounces, a max_fuzz that is negative
 * or not finite */
inline bool rt_aov_deep_args_ok(uint32_t max_specular, double max_fuzz) {
    return max_specular <= RT_AOV_DEEP_MAX_SPECULAR && max_fuzz >= 0.0 && max_fuzz <= 1.7976931348623157e308;
}

/* sample `sample` (absolute index) of image pixel (i, j): begin -> [closest hit -> finish hit -> specular scatter]* -> material colour.
 * `rays` counts the rays traced (1 .. max_specular + 1).
 *
 * The wave stays together across the walk: the bounce loop runs while ANY lane of the wave is still on its chain, and a lane whose
 * chain has ended walks along with an empty interval (t_max 0: a box at the root fails at once; any other root is walked and may
 * draw from the finished lane's stream, which nobody reads again) and ignores the answer.  It would wait for the others anyway.
 * This is the form that has been verified on the GPU in every variant; it is NOT known to be necessary: a four-wave build of it was
 * wrong in one variant like the four-wave builds of the plain loop (cause open).  On the CPU build a wave is
 * one lane and this is the plain loop. */
template <class Cfg, class Stack, class NS>
RT_HD RtAovSample rt_aov_deep_sample(const RtSceneView& sc, const NS& ns, const RtFrame& f, uint32_t i, uint32_t j, uint32_t sample,
                                     uint32_t max_specular, double max_fuzz, Stack& stk, uint32_t& rays) {
    RtPath p;
    rt_path_begin(sc, f, i, j, sample, p); /* p.beta = 1 */
    RtAovSample a;
    a.albedo = a.normal = rt_v3(RT_R(0.0), RT_R(0.0), RT_R(0.0));
    a.dist = RT_R(0.0);
    a.hit = false;
    bool done = false;
    for (uint32_t bounce = 0u; RT_WAVE_ANY(!done); ++bounce) {
        double t;
        uint32_t prim, scope;
        const bool found = rt_closest_hit<Cfg>(sc, ns, p.ray, RT_R(0.001), done ? RT_R(0.0) : RT_INF, p.rng, stk, t, prim, scope);
        if (done) continue;
        rays += 1u;
        a.hit = found;
        if (!found) {
            a.albedo = rt_mul(p.beta, sc.background);
            done = true;
            continue;
        }
        RtHit h;
        rt_finish_hit<Cfg>(sc, p.ray, prim, scope, t, h);
        a.dist += t * rt_mag(p.ray.d);
        const RtMaterial& m = sc.materials[RT_MAT_INDEX(h.mat)];
        const uint32_t mk = RT_MAT_KINDF(h.mat) & 0xFFu;
        const bool specular = mk == RT_MAT_DIELECTRIC || (mk == RT_MAT_METAL && m.d[3] <= max_fuzz);
        if (!specular || bounce >= max_specular) {
            a.albedo = rt_mul(p.beta, rt_aov_albedo<Cfg>(sc, h));
            a.normal = h.n;
            done = true;
            continue;
        }
        if (mk == RT_MAT_METAL) {
            /* Metal::scatter material.rs:99-111: the draw is taken at fuzz 0 too */
            RtV3 reflected = rt_reflect(rt_normalize(p.ray.d), h.n);
            RtV3 dir = reflected + m.d[3] * rt_random_in_unit_sphere(p.rng);
            p.beta = rt_mul(p.beta, rt_v3(m.d[0], m.d[1], m.d[2]));
            p.ray.o = h.p; p.ray.d = dir;
        } else {
            /* Dielectric::scatter material.rs:133-160 */
            double refraction_ratio = h.front ? RT_R(1.0) / m.d[0] : m.d[0];
            RtV3 unit_direction = rt_normalize(p.ray.d);
            double cos_theta = rt_min(rt_dot(-unit_direction, h.n), RT_R(1.0));
            double sin_theta = rt_sqrt(RT_R(1.0) - cos_theta * cos_theta);
            bool cannot_refract = refraction_ratio * sin_theta > RT_R(1.0);
            RtV3 dir;
            if (cannot_refract || rt_reflectance(cos_theta, refraction_ratio) > rt_gen_f64(p.rng))
                dir = rt_reflect(unit_direction, h.n);
            else
                dir = rt_refract(unit_direction, h.n, refraction_ratio);
            p.beta = rt_mul(p.beta, rt_v3(RT_R(1.0), RT_R(1.0), RT_R(1.0)));
            p.ray.o = h.p; p.ray.d = dir;
        }
        /* the ray keeps its time: neither arm sets it (main.rs:86 does so on the Lambertian arm only) */
    }
    return a;
}

/* the 8 channels of tile pixel (px, py), summed and divided as rt_aov_pixel does; returns the rays traced.  The seven running sums
 * live in the pixel's own `out` (one lane owns it; the volatile accesses keep the compiler from promoting them back to registers):
 * held in registers across the chain loop they push the V2 and V5 kernels past 256 VGPRs (44 B of scratch per lane), which the
 * build refuses (Makefile).  Same additions in the same order as rt_aov_pixel; coverage is the exact count of hits.  `lengths` (twin
 * only, may be null): the rays of each of the pixel's spp samples */
template <class Cfg, class Stack, class NS>
RT_HD unsigned long long rt_aov_deep_pixel(const RtSceneView& sc, const NS& ns, const RtFrame& f, uint32_t px, uint32_t py,
                                           uint32_t max_specular, double max_fuzz, Stack& stk, double* out, uint8_t* lengths) {
    const uint32_t i = f.x0 + px, j = rt_frame_row(f, py);
    volatile double* sum = out;
    for (int c = 0; c < 7; ++c) sum[c] = RT_R(0.0);
    uint32_t hits = 0u;
    unsigned long long total = 0ull;
    for (uint32_t s = 0; s < f.spp; ++s) {
        uint32_t rays = 0u;
        const RtAovSample a = rt_aov_deep_sample<Cfg>(sc, ns, f, i, j, f.sample_offset + s, max_specular, max_fuzz, stk, rays);
        sum[0] = sum[0] + a.albedo.x; sum[1] = sum[1] + a.albedo.y; sum[2] = sum[2] + a.albedo.z;
        sum[3] = sum[3] + a.normal.x; sum[4] = sum[4] + a.normal.y; sum[5] = sum[5] + a.normal.z;
        if (a.hit) { sum[6] = sum[6] + a.dist; hits += 1u; }
        total += rays;
        if (lengths) lengths[s] = (uint8_t)rays;
    }
    const double n = (double)f.spp;
    for (int c = 0; c < 6; ++c) sum[c] = sum[c] / n;
    sum[6] = hits ? sum[6] / (double)hits : RT_INF;
    sum[7] = (double)hits / n;
    return total;
}

#endif
