/* rt_aov.h -- first-hit feature buffers (rt1w_render_aov, include/rt1w.h): albedo, shading normal, hit distance and coverage of the
 * camera ray of one (pixel, sample).  Compiled by the AOV kernel (aov.hip) and by the CPU twin of the diagnostics library
 * (aov_host.cpp), from this one text.
 *
 * The ray is the one rt1w_render's sample starts with (rt_path_begin: main.rs:964-971, camera.rs:61-73), traced once with
 * world.hit(ray, 0.001, inf) (main.rs:62) by the scene variant's own walk; a ConstantMedium draws its free flight from the sample's
 * stream exactly as the first segment of the beauty path does.  Nothing here is reached by the render kernels. */
#ifndef RT_AOV_H
#define RT_AOV_H

#include "rt_core.h"

#define RT_AOV_CHANNELS 8 /* == RT1W_AOV_CHANNELS */

/* what one sample contributes */
struct RtAovSample {
    RtV3 albedo, normal;
    double dist;
    bool hit;
};

/* "albedo" of the hit's material: Lambertian / Isotropic the texture's value at (u, v, p) (material.rs:71-80, constant_medium.rs:37-50),
 * Metal its albedo (material.rs:99-111), Dielectric 1 (material.rs:133-160), DiffuseLight emitted(u, v, p) -- front face only
 * (material.rs:163-178) --, impl Material for () 0 (material.rs:68) */
template <class Cfg>
RT_HD RtV3 rt_aov_albedo(const RtSceneView& sc, const RtHit& h) {
    const RtMaterial& m = sc.materials[RT_MAT_INDEX(h.mat)];
    const uint32_t mk = RT_MAT_KINDF(h.mat) & 0xFFu;
    if (mk == RT_MAT_LAMBERTIAN || (Cfg::media && mk == RT_MAT_ISOTROPIC)) return rt_mat_colour<Cfg>(sc, m, h.u, h.v, h.p);
    if (mk == RT_MAT_METAL) return rt_v3(m.d[0], m.d[1], m.d[2]);
    if (mk == RT_MAT_DIELECTRIC) return rt_v3(RT_R(1.0), RT_R(1.0), RT_R(1.0));
    if (mk == RT_MAT_DIFFUSE_LIGHT && h.front) return rt_mat_colour<Cfg>(sc, m, h.u, h.v, h.p);
    return rt_v3(RT_R(0.0), RT_R(0.0), RT_R(0.0));
}

/* sample `sample` (absolute index) of image pixel (i, j): begin -> closest hit -> finish hit -> material colour */
template <class Cfg, class Stack, class NS>
RT_HD RtAovSample rt_aov_sample(const RtSceneView& sc, const NS& ns, const RtFrame& f, uint32_t i, uint32_t j, uint32_t sample, Stack& stk) {
    RtPath p;
    rt_path_begin(sc, f, i, j, sample, p);
    RtAovSample a;
    double t;
    uint32_t prim, scope;
    a.hit = rt_closest_hit<Cfg>(sc, ns, p.ray, RT_R(0.001), RT_INF, p.rng, stk, t, prim, scope);
    if (!a.hit) {
        a.albedo = sc.background;
        a.normal = rt_v3(RT_R(0.0), RT_R(0.0), RT_R(0.0));
        a.dist = RT_R(0.0);
        return a;
    }
    RtHit h;
    rt_finish_hit<Cfg>(sc, p.ray, prim, scope, t, h);
    a.albedo = rt_aov_albedo<Cfg>(sc, h);
    a.normal = h.n; /* world space, against the ray (hittable.rs:30-35, :206-270); FlipFace flips the flag only; a medium's (1, 0, 0) */
    a.dist = t * rt_mag(p.ray.d);
    return a;
}

/* the 8 channels of tile pixel (px, py): samples sample_offset .. sample_offset + spp - 1 summed in order.  0-5 and 7 (coverage) are
 * divided by spp; 6 (distance) is the mean over the samples that hit, +inf if none did */
template <class Cfg, class Stack, class NS>
RT_HD void rt_aov_pixel(const RtSceneView& sc, const NS& ns, const RtFrame& f, uint32_t px, uint32_t py, Stack& stk, double* out) {
    const uint32_t i = f.x0 + px, j = rt_frame_row(f, py);
    RtV3 alb = rt_v3(RT_R(0.0), RT_R(0.0), RT_R(0.0)), nrm = alb;
    double dist = RT_R(0.0), cov = RT_R(0.0);
    uint32_t hits = 0u;
    for (uint32_t s = 0; s < f.spp; ++s) {
        const RtAovSample a = rt_aov_sample<Cfg>(sc, ns, f, i, j, f.sample_offset + s, stk);
        alb = alb + a.albedo;
        nrm = nrm + a.normal;
        if (a.hit) { dist += a.dist; cov += RT_R(1.0); hits += 1u; }
    }
    const double n = (double)f.spp;
    out[0] = alb.x / n; out[1] = alb.y / n; out[2] = alb.z / n;
    out[3] = nrm.x / n; out[4] = nrm.y / n; out[5] = nrm.z / n;
    out[6] = hits ? dist / (double)hits : RT_INF;
    out[7] = cov / n;
}

#endif
