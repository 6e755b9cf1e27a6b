/* rt_ray_list.h -- radiance queries (rt1w_ray_color, include/rt1w.h): ray_color(ray, background, world, lights, depth, rng) (main.rs:51-116,
 * and :118-190 without lights) for a list of the caller's own rays.  What the ray-list form of the render kernels (context_rays.hip:
 * rt_kernel_sorted.h with RT_RAY_LIST) and the CPU twin of the diagnostics library (aov_host.cpp) share: the parameter block, the
 * refusals of a call, the test for a ray that is not traced, what such a ray's samples sum to, and the begin of a sample.
 *
 * A sample of ray r is a path that starts on the caller's ray instead of Camera::get_ray's (camera.rs:61-73): stream
 * rt_rng_pixel_sample(first_stream + r, sample, global_seed) standing at word start_word[r] (rt1w_num.h: rt_rng_at), beta 1, radiance 0,
 * depth_left = max_depth.  From there on it is rt_path_trace / rt_path_shade, the text of every render. */
#ifndef RT_RAY_LIST_H
#define RT_RAY_LIST_H

#include "rt_core.h"

#define RT_RAY_RECORD 7 /* doubles of a ray record the entry reads: origin 3, direction 3, time (Ray, ray.rs:5) */

/* rt1w_ray_color_params (include/rt1w.h), the same 56 bytes */
struct RtRayColorParams {
    uint64_t n, first_stream, global_seed;
    uint32_t spp, sample_offset, max_depth, chunk, stride, flags, partial_mib, reserved;
};

/* the list as the kernels take it, in last place (context.h: RtRayArg, the same bytes) */
struct RtRayList {
    const double* rays;         /* [n][stride] */
    const uint32_t* start_word; /* [n] or null */
    uint64_t n, first_stream;
    uint32_t stride, pad;
};

#if !defined(__HIP_DEVICE_COMPILE__)
/* What rt1w_ray_color, rt1w_ray_color_device and the twin refuse of a call, in the order they look; null = nothing (all RT1W_ERR_INVALID;
 * the parameter block has no precision member: single precision cannot be asked for, the bindings answer it RT1W_ERR_UNSUPPORTED).
 * `flag_out_sum`, `flag_generic`: RT1W_OUT_SUM, RT1W_GENERIC (this header does not see rt1w.h).  The buffers: rays ((n - 1) * stride + 7)
 * doubles, start_word (may be null) n words, out n * 24 bytes */
inline const char* rt_ray_color_refusal(const RtRayColorParams* p, const void* rays, const void* start_word, const void* out,
                                        uint32_t flag_out_sum, uint32_t flag_generic) {
    if (!p || !rays || !out) return "null argument";
    if (p->n == 0u || p->n > 0xFFFFFFFFull) return "ray_color: n must be 1 .. 2^32 - 1";
    if (p->spp == 0u) return "ray_color: spp must be > 0";
    if ((uint64_t)p->sample_offset + p->spp > 0xFFFFFFFFull) return "ray_color: sample index overflow";
    if (p->global_seed > 0xFFFFFFFFull) return "ray_color: global_seed must be below 2^32";
    if (p->stride != 0u && p->stride < (uint32_t)RT_RAY_RECORD) return "ray_color: stride must be 0 or >= 7";
    if (p->flags & ~(flag_out_sum | flag_generic)) return "ray_color: flags 0, RT1W_OUT_SUM or RT1W_GENERIC only";
    if (p->reserved != 0u) return "ray_color: reserved must be 0";
    const auto overlap = [](const void* a, uint64_t na, const void* b, uint64_t nb) {
        const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
        return x < y + nb && y < x + na;
    };
    const uint64_t stride = p->stride ? p->stride : (uint64_t)RT_RAY_RECORD;
    const uint64_t ray_bytes = ((p->n - 1u) * stride + RT_RAY_RECORD) * sizeof(double), out_bytes = p->n * 3u * sizeof(double);
    if (overlap(rays, ray_bytes, out, out_bytes) || (start_word && overlap(start_word, p->n * sizeof(uint32_t), out, out_bytes)))
        return "ray_color: out must not overlap rays or start_word";
    return nullptr;
}
#endif

/* finite: neither an infinity nor a NaN (the exponent field is not all ones) */
RT_HD bool rt_ray_finite(double x) { return (rt_d2u(x) & 0x7FF0000000000000ull) != 0x7FF0000000000000ull; }
/* THE ONE DEVIATION from the literal ray_color: a ray with a non-finite origin, direction or time is not traced */
RT_HD bool rt_ray_traced(const double* ray) {
    bool ok = true;
    for (int k = 0; k < RT_RAY_RECORD; ++k) ok &= rt_ray_finite(ray[k]);
    return ok;
}
/* ... each of its samples is a miss: what rt_path_shade leaves of a fresh path that hit nothing (the background, main.rs:64-66), or of
 * one with no depth left (main.rs:59-61), summed over the `count` samples of a work item as the kernels sum a traced ray's */
RT_HD RtV3d rt_ray_untraced_sum(const RtSceneView& sc, uint32_t max_depth, uint32_t count) {
    const RtV3 beta = rt_v3(RT_R(1.0), RT_R(1.0), RT_R(1.0)), zero = rt_v3(RT_R(0.0), RT_R(0.0), RT_R(0.0));
    const RtV3 radiance = zero + rt_mul(beta, max_depth == 0u ? zero : sc.background);
    RtV3d sum = rt_v3d(RT_R(0.0), RT_R(0.0), RT_R(0.0));
    for (uint32_t k = 0; k < count; ++k) sum = rt_v3d_add(sum, radiance);
    return sum;
}
/* the begin of sample `sample` of ray r: what rt_path_begin is to a pixel's sample */
RT_HD void rt_ray_begin(const RtRayList& rl, uint32_t global_seed, uint32_t max_depth, uint64_t r, uint32_t sample, RtPath& p) {
    const double* ray = rl.rays + r * (uint64_t)rl.stride;
    p.rng = rt_rng_at(rt_rng_pixel_sample(rl.first_stream + r, sample, global_seed), rl.start_word ? rl.start_word[r] : 0u);
    p.ray.o = rt_v3(ray[0], ray[1], ray[2]);
    p.ray.d = rt_v3(ray[3], ray[4], ray[5]);
    p.ray.time = ray[6];
    p.beta = rt_v3(RT_R(1.0), RT_R(1.0), RT_R(1.0));
    p.radiance = rt_v3(RT_R(0.0), RT_R(0.0), RT_R(0.0));
    p.depth_left = max_depth;
    p.alive = true;
}

#endif
