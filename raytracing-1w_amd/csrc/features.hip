/* features.hip -- the entries of the feature buffers and the denoiser (include/rt1w.h: rt1w_render_aov*, rt1w_hit*, rt1w_ray_color*, rt1w_denoise*,
 * rt1w_render_denoised*, rt1w_batch_variance*, rt1w_accum_*, rt1w_guides_*, rt1w_render_adaptive*, rt1w_temporal_*, rt1w_render_temporal*) and a live context's camera (rt1w_context_set_camera).  Host code only, built without a device pass: the kernels
 * belong to aov.hip, hit.hip, aov_tiles.hip, guides.hip, denoise.hip, denoise_var.hip, denoise_halves.hip, denoise_cross.hip, adaptive.hip, temporal.hip and temporal_var.hip and are reached through rt_feature_launch.h, the context and its render
 * path belong to context.hip (context.h), so a change here rebuilds none of the code objects.
 * Every entry is its checks, in the order its callers know, then one table of its buffers (Staged) handed to staged_entry(), which does what
 * the host and the device form of an entry differ in -- growing the context's buffers, laying the call's buffers out in them, the copies
 * in and out -- and the clock.  Every kernel launch of this file goes through lane_run() over a typed *_launch of rt_feature_launch.h: no
 * kernel handle, no argument array and no launch call of its own is left here.  The AOV entries add to lane_run's stats the fields it does
 * not fill (segments, chunk, n_chunks, variant). */
#include <cstdio>
#include <cstring>

#include "context.h"
#include "rt_feature_launch.h"
#include "rt_aov_deep.h" /* rt_aov_deep_args_ok only */
#include "rt_hit.h" /* RtHitParams, rt_hit_refusal only */
#include "rt_ray_list.h" /* RtRayColorParams, rt_ray_color_refusal only */
#include "rt_path_state.h" /* RtPathParams, RtPathState, rt_path_step_refusal, rt_path_begin_refusal only */
#include "rt_denoise_var.h" /* rt_dv_batches_ok, rt_dv_sigma, rt_dv_split only */
#include "rt_adaptive_plan.h" /* the plan of rt1w_render_adaptive and rt1w_adaptive_select; rt_ad_*_ok of rt_adaptive.h; the tile lists' checks */
#include "rt_guides.h" /* RT_GD_RECORD only */
#include "rt_temporal.h" /* rt_tm_make_params only */

/* context_f32.hip: the f32 scene's copy of the camera, rounded anew from the f64 view */
extern "C" void rt1w_internal_f32_set_camera(void* h, const void* view64);

using namespace rt1w;
namespace {

/* ---- what the entries share: one run on the lane, one description of an entry's buffers ---- */
/* A unit's launches on lane 0, between the lane's two events.  `enqueue(stream, launch)` is one *_launch of rt_feature_launch.h behind a
 * lambda; then wait.  *stats but for total_ms: `paths`, the HIP-event time, grid / block as the launcher reports them */
template <class Enqueue>
int lane_run(rt1w_context* c, uint64_t paths, const char* what, rt1w_stats* stats, Enqueue enqueue) {
    RtLane& l = c->lane[0];
    unsigned launch[2] = {0u, 0u};
    (void)hipEventRecord(l.ev0, l.stream);
    const int rc = enqueue(l.stream, launch);
    if (rc == -2) { set_error(std::string(what) + ": parameters refused"); return RT1W_ERR_INVALID; }
    if (rc != 0) { set_error(std::string(what) + " kernel launch failed"); return RT1W_ERR_DEVICE; }
    (void)hipEventRecord(l.ev1, l.stream);
    if (!hip_ok(hipStreamSynchronize(l.stream), what)) return RT1W_ERR_DEVICE;
    memset(stats, 0, sizeof *stats);
    stats->paths = paths; stats->kernel_ms = lane_ms(l);
    stats->grid = launch[0]; stats->block = launch[1]; stats->passes = 1u;
    return RT1W_OK;
}

/* One buffer of an entry.  The host forms stage it in one of the context's three grow-on-demand buffers, where the buffers of a call lie
 * one behind the other in the order of the entry's table; the device forms hand the caller's pointers through. */
enum Pool { FRAMEBUFFER, BATCH_BUFFER, ACCUM_BUFFER, N_POOLS };
struct Staged {
    const double* in;  /* the caller's buffer copied in before the run, or null */
    double* out;       /* the caller's buffer copied out after it, or null.  Both: ONE staged place -- an update, or a filter in place */
    size_t count;      /* doubles */
    Pool pool;
    const char* in_text; const char* out_text; /* the error texts of the two copies */
    const double* d_in = nullptr; double* d_out = nullptr; /* where the kernels find it; staged: the same place */
};
/* What every entry does once its checks have passed: device, clock, (host) grow the context's buffers to the table and copy the inputs in,
 * run(&st), (host) copy the outputs back, *stats = st with total_ms.  A row without `in` and `out` is room the run itself fills and reads. */
template <size_t N, class Run>
int staged_entry(rt1w_context* c, bool host, Staged (&s)[N], rt1w_stats* stats, Run run) {
    if (!hip_ok(hipSetDevice(c->device), "hipSetDevice")) return RT1W_ERR_DEVICE;
    const RtTimer timer;
    int rc;
    if (host) {
        size_t need[N_POOLS] = {0, 0, 0};
        for (const Staged& b : s) need[b.pool] += b.count * sizeof(double);
        if ((rc = reserve_out(c, need[FRAMEBUFFER])) < 0) return rc;
        if ((rc = dev_grow((void**)&c->d_batches, &c->batches_bytes, need[BATCH_BUFFER], "hipMalloc(batch sums)")) < 0) return rc;
        if ((rc = dev_grow((void**)&c->d_accum, &c->accum_bytes, need[ACCUM_BUFFER], "hipMalloc(accumulator)")) < 0) return rc;
        double* at[N_POOLS] = {c->d_out, c->d_batches, c->d_accum};
        for (Staged& b : s) {
            b.d_in = b.d_out = at[b.pool];
            at[b.pool] += b.count;
            if (b.in && !hip_ok(hipMemcpy(b.d_out, b.in, b.count * sizeof(double), hipMemcpyHostToDevice), b.in_text)) return RT1W_ERR_DEVICE;
        }
    } else
        for (Staged& b : s) { b.d_in = b.in; b.d_out = b.out; }
    rt1w_stats st;
    if ((rc = run(&st)) < 0) return rc;
    if (host)
        for (const Staged& b : s)
            if (b.out && !hip_ok(hipMemcpy(b.out, b.d_out, b.count * sizeof(double), hipMemcpyDeviceToHost), b.out_text)) return RT1W_ERR_DEVICE;
    if (stats) { *stats = st; stats->total_ms = timer.ms(); }
    return RT1W_OK;
}
/* one more render into the sum of a composite entry's renders (the first render gives the fields that are no sums) */
void stats_add(rt1w_stats* total, const rt1w_stats& one) {
    total->paths += one.paths; total->segments += one.segments; total->kernel_ms += one.kernel_ms; total->passes += one.passes;
}

/* ---- first-hit and deep feature buffers (include/rt1w.h: rt1w_render_aov, rt1w_render_aov_deep) ---- */
/* the render flags by name, in the order the refusals look for them; `denoised`: one rt1w_render_denoised refuses too */
const struct { uint32_t bit; const char* name; bool denoised; } g_flags[] = {
    {RT1W_OUT_SUM, "RT1W_OUT_SUM", true}, {RT1W_UNSORTED, "RT1W_UNSORTED", false}, {RT1W_LDS_NODES, "RT1W_LDS_NODES", false},
    {RT1W_GENERIC, "RT1W_GENERIC", false}, {RT1W_WAVEFRONT, "RT1W_WAVEFRONT", false}, {RT1W_OUT_FRAME, "RT1W_OUT_FRAME", true},
    {RT1W_RNG_REFERENCE, "RT1W_RNG_REFERENCE", true}, {RT1W_CLASSIC_WALK, "RT1W_CLASSIC_WALK", false},
    {RT1W_NO_NODE_CACHE, "RT1W_NO_NODE_CACHE", false}, {RT1W_PROBE_COHERENT, "RT1W_PROBE_COHERENT", true},
    {RT1W_TILES_SPECIALISED, "RT1W_TILES_SPECIALISED", false}};
/* refuses the first flag of `flags` that has a name (denoised_only: and that rt1w_render_denoised refuses), as "<name><tail>" */
int refuse_named_flag(uint32_t flags, bool denoised_only, const char* tail) {
    for (const auto& k : g_flags)
        if ((flags & k.bit) && (k.denoised || !denoised_only)) { set_error(std::string(k.name) + tail); return RT1W_ERR_INVALID; }
    return RT1W_OK;
}
/* the p->flags of an adaptive entry whose rounds go through the tile entries: 0, RT1W_GENERIC, or RT1W_TILES_SPECIALISED (the rounds on
 * the tile-list form of the scene-specialised kernel; the pilot's rectangle renders ignore the bit) */
bool tile_round_flags_ok(uint32_t flags) { return flags == 0u || flags == RT1W_GENERIC || flags == RT1W_TILES_SPECIALISED; }
/* the one flag the AOV entries take besides RT1W_FORCE_VARIANT: everything else is named and refused */
int aov_check_flags(uint32_t flags) {
    const uint32_t bad = flags & ~(0xFFu << 8);
    if (!bad) return RT1W_OK;
    if (refuse_named_flag(bad, false, " does not apply to the AOV entries (flags: 0 or RT1W_FORCE_VARIANT)") < 0) return RT1W_ERR_INVALID;
    char buf[96];
    snprintf(buf, sizeof buf, "unknown flag 0x%x for the AOV entries (flags: 0 or RT1W_FORCE_VARIANT)", bad & (0u - bad));
    set_error(buf);
    return RT1W_ERR_INVALID;
}
/* the deep entries' two extra arguments (include/rt1w.h: rt1w_render_aov_deep); null = the first-hit buffers */
struct AovDeep { uint32_t max_specular; double max_fuzz; };
int aov_deep_validate(const AovDeep* deep) {
    if (!deep || rt_aov_deep_args_ok(deep->max_specular, deep->max_fuzz)) return RT1W_OK;
    set_error("max_specular must be 0 .. 64 and max_fuzz finite and >= 0");
    return RT1W_ERR_INVALID;
}
/* the AOV kernel of the context's (or the forced) variant into d_out through lane_run; of the stats what that leaves open */
int render_aov_common(rt1w_context* c, const rt1w_render_params* p, const AovDeep* deep, double* d_out, rt1w_stats* stats) {
    int variant = c->variant;
    const int rc = forced_variant(c, p->flags, true, &variant);
    if (rc < 0) return rc;
    RtFrame f = frame_of(p);
    f.max_depth = 1u; f.chunk = p->spp; f.n_chunks = 1u; /* not read by the AOV kernels */
    RtLane& l = c->lane[0];
    if (rt1w_internal_aov_sizeof(0) != sizeof(RtSceneView) || rt1w_internal_aov_sizeof(1) != sizeof(RtFrame)) {
        set_error("AOV kernels built against another scene layout"); return RT1W_ERR_DEVICE;
    }
    /* the deep kernel counts the rays it traces in the lane's second counter, the one the render kernels count their segments in: zeroed
     * before the lane's two events, read after them */
    unsigned long long* d_rays = l.d_counters + 1;
    if (deep && !hip_ok(hipMemsetAsync(d_rays, 0, sizeof *d_rays, l.stream), "AOV counter")) return RT1W_ERR_DEVICE;
    rt1w_stats st;
    const int r = lane_run(c, (uint64_t)p->tile_w * p->tile_h * p->spp, "AOV", &st, [&](hipStream_t stream, unsigned* launch) {
        return deep ? rt1w_internal_aov_deep_launch(&c->view, &f, variant, deep->max_specular, deep->max_fuzz, d_out, d_rays, stream, launch)
                    : rt1w_internal_aov_launch(&c->view, &f, variant, d_out, stream, launch);
    });
    if (r < 0) return r;
    if (deep && !(hip_ok(hipMemcpyAsync(l.h_counters + 1, d_rays, sizeof *d_rays, hipMemcpyDeviceToHost, l.stream), "AOV counter copy") &&
                  hip_ok(hipStreamSynchronize(l.stream), "AOV counter copy")))
        return RT1W_ERR_DEVICE; /* on the lane's own stream: no other stream of the device is waited for */
    st.segments = deep ? l.h_counters[1] : st.paths; /* first hit: one camera ray per sample */
    st.chunk = p->spp; st.n_chunks = 1u;
    st.variant = (uint32_t)variant;
    if (stats) *stats = st;
    return RT1W_OK;
}
/* the four AOV entries.  `out` is device memory, or (host) host memory, filled through the context's framebuffer */
int render_aov(rt1w_context* c, const rt1w_render_params* p, const AovDeep* deep, void* out, bool host, rt1w_stats* stats) {
    int rc = aov_deep_validate(deep); /* first: needs no context */
    if (rc < 0) return rc;
    if ((rc = validate(c, p)) < 0) return rc;
    if (!out) { set_error("null output"); return RT1W_ERR_INVALID; }
    if ((rc = aov_check_flags(p->flags)) < 0) return rc;
    if (p->precision != RT1W_PRECISION_F64) { set_error("the AOV entries are f64 only (RT1W_PRECISION_F64)"); return RT1W_ERR_UNSUPPORTED; }
    Staged s[] = {{nullptr, (double*)out, (size_t)p->tile_w * p->tile_h * RT1W_AOV_CHANNELS, FRAMEBUFFER, nullptr, "AOV copy"}};
    return staged_entry(c, host, s, stats, [&](rt1w_stats* st) { return render_aov_common(c, p, deep, s[0].d_out, st); });
}

/* ---- ray queries (include/rt1w.h: rt1w_hit) ---- */
static_assert(sizeof(rt1w_hit_params) == sizeof(RtHitParams), "rt1w_hit_params is RtHitParams' layout");
/* the query kernel of the context's (or the forced) variant over device buffers through lane_run; of the stats what that leaves open */
int hit_common(rt1w_context* c, const rt1w_hit_params* p, int variant, const double* d_rays, double* d_out, uint32_t* d_node, rt1w_stats* stats) {
    if (rt1w_internal_hit_sizeof(0) != sizeof(RtSceneView) || rt1w_internal_hit_sizeof(1) != sizeof(rt1w_hit_params)) {
        set_error("ray-query kernels built against another scene layout"); return RT1W_ERR_DEVICE;
    }
    rt1w_stats st;
    const int r = lane_run(c, p->n, "ray query", &st, [&](hipStream_t stream, unsigned* launch) {
        return rt1w_internal_hit_launch(&c->view, p, variant, d_rays, d_out, d_node, stream, launch);
    });
    if (r < 0) return r;
    st.segments = st.paths; /* one ray each */
    st.chunk = 1u; st.n_chunks = 1u;
    st.variant = (uint32_t)variant;
    if (stats) *stats = st;
    return RT1W_OK;
}
/* the two query entries.  The buffers are device memory, or (host) host memory, passed through the context's framebuffer */
int hit(rt1w_context* c, const rt1w_hit_params* p, const void* rays, void* out, void* out_node, bool host, rt1w_stats* stats) {
    if (!c || !p || !rays || !out) { set_error("null argument"); return RT1W_ERR_INVALID; }
    RtHitParams hp;
    memcpy(&hp, p, sizeof hp);
    if (const char* why = rt_hit_refusal(hp, rays, out, out_node)) { set_error(why); return RT1W_ERR_INVALID; }
    int variant = c->variant;
    const int rc = forced_variant(c, p->flags, true, &variant);
    if (rc < 0) return rc;
    const uint64_t node_bytes = p->n * sizeof(uint32_t);
    /* the node indices are 4 bytes each: staged as room of whole doubles, copied out here in their own size */
    Staged s[] = {{(const double*)rays, nullptr, (size_t)p->n * 9u, FRAMEBUFFER, "ray copy", nullptr},
                  {nullptr, (double*)out, (size_t)p->n * 12u, FRAMEBUFFER, nullptr, "hit record copy"},
                  {nullptr, nullptr, host && out_node ? (size_t)((p->n + 1u) / 2u) : 0u, FRAMEBUFFER, nullptr, nullptr}};
    return staged_entry(c, host, s, stats, [&](rt1w_stats* st) {
        uint32_t* d_node = host ? (out_node ? (uint32_t*)s[2].d_out : nullptr) : (uint32_t*)out_node;
        const int r = hit_common(c, p, variant, s[0].d_in, s[1].d_out, d_node, st);
        if (r < 0) return r;
        if (host && out_node && !hip_ok(hipMemcpy(out_node, d_node, node_bytes, hipMemcpyDeviceToHost), "node index copy")) return (int)RT1W_ERR_DEVICE;
        return (int)RT1W_OK;
    });
}

/* ---- radiance queries (include/rt1w.h: rt1w_ray_color) ---- */
static_assert(sizeof(rt1w_ray_color_params) == sizeof(RtRayColorParams) && sizeof(RtRayColorParams) == 56, "rt1w_ray_color_params is RtRayColorParams' layout");
/* the two radiance entries.  The buffers are device memory, or (host) host memory, passed through the context's framebuffer.  The rays go
 * through the render kernels' ray-list form (context.hip: ray_color_common) as a render of n x 1 pixels with RT1W_GENERIC */
int ray_color(rt1w_context* c, const rt1w_ray_color_params* p, const void* rays, const void* start_word, void* out, bool host, rt1w_stats* stats) {
    if (!c) { set_error("null argument"); return RT1W_ERR_INVALID; }
    if (const char* why = rt_ray_color_refusal((const RtRayColorParams*)p, rays, start_word, out, RT1W_OUT_SUM, RT1W_GENERIC)) { set_error(why); return RT1W_ERR_INVALID; }
    const uint32_t stride = p->stride ? p->stride : (uint32_t)RT_RAY_RECORD;
    rt1w_render_params q;
    memset(&q, 0, sizeof q);
    q.width = q.tile_w = (uint32_t)p->n; q.height = q.tile_h = 1u;
    q.spp = p->spp; q.sample_offset = p->sample_offset; q.max_depth = p->max_depth; q.global_seed = (uint32_t)p->global_seed;
    q.chunk = p->chunk; q.partial_mib = p->partial_mib; q.precision = RT1W_PRECISION_F64;
    q.flags = (p->flags & RT1W_OUT_SUM) | RT1W_GENERIC;
    const uint64_t word_bytes = p->n * sizeof(uint32_t);
    /* the start words are 4 bytes each: staged as room of whole doubles, copied in here in their own size */
    Staged s[] = {{(const double*)rays, nullptr, (size_t)((p->n - 1u) * stride + RT_RAY_RECORD), FRAMEBUFFER, "ray copy", nullptr},
                  {nullptr, (double*)out, (size_t)p->n * 3u, FRAMEBUFFER, nullptr, "radiance copy"},
                  {nullptr, nullptr, host && start_word ? (size_t)((p->n + 1u) / 2u) : 0u, FRAMEBUFFER, nullptr, nullptr}};
    return staged_entry(c, host, s, stats, [&](rt1w_stats* st) {
        RtRayArg rl;
        rl.rays = s[0].d_in; rl.n = p->n; rl.first_stream = p->first_stream; rl.stride = stride;
        rl.start_word = host ? (start_word ? (const uint32_t*)s[2].d_out : nullptr) : (const uint32_t*)start_word;
        if (host && start_word && !hip_ok(hipMemcpy(s[2].d_out, start_word, word_bytes, hipMemcpyHostToDevice), "start word copy")) return (int)RT1W_ERR_DEVICE;
        return ray_color_common(c, &q, rl, s[1].d_out, st);
    });
}

/* ---- path states (include/rt1w.h: rt1w_path_step, rt1w_path_begin) ---- */
static_assert(sizeof(rt1w_path_params) == sizeof(RtPathParams) && sizeof(RtPathParams) == 32, "rt1w_path_params is RtPathParams' layout");
static_assert(sizeof(rt1w_path_state) == sizeof(RtPathState), "rt1w_path_state is RtPathState's layout");
constexpr size_t PATH_STATE_DOUBLES = sizeof(RtPathState) / sizeof(double);
/* One launch of path_step.hip through lane_run with the lane's second counter -- the one the render kernels count their segments in --
 * zeroed in front of the lane's two events and read behind them (render_aov_common does the same for the deep kernel): *count = what
 * the kernel added to it */
template <class Enqueue>
int path_counted_run(rt1w_context* c, uint64_t n, const char* what, rt1w_stats* st, unsigned long long* count, Enqueue enqueue) {
    if (rt1w_internal_path_sizeof(0) != sizeof(RtSceneView) || rt1w_internal_path_sizeof(1) != sizeof(rt1w_path_params) ||
        rt1w_internal_path_sizeof(2) != sizeof(rt1w_path_state)) {
        set_error("path-state kernels built against another scene layout"); return RT1W_ERR_DEVICE;
    }
    RtLane& l = c->lane[0];
    unsigned long long* d_count = l.d_counters + 1;
    if (!hip_ok(hipMemsetAsync(d_count, 0, sizeof *d_count, l.stream), "path-state counter")) return RT1W_ERR_DEVICE;
    const int r = lane_run(c, n, what, st, [&](hipStream_t stream, unsigned* launch) { return enqueue(d_count, stream, launch); });
    if (r < 0) return r;
    if (!(hip_ok(hipMemcpyAsync(l.h_counters + 1, d_count, sizeof *d_count, hipMemcpyDeviceToHost, l.stream), "path-state counter copy") &&
          hip_ok(hipStreamSynchronize(l.stream), "path-state counter copy")))
        return RT1W_ERR_DEVICE; /* on the lane's own stream: no other stream of the device is waited for */
    *count = l.h_counters[1];
    st->chunk = 1u; st->n_chunks = 1u;
    return RT1W_OK;
}
/* the two step entries.  The buffers are device memory, or (host) host memory, passed through the context's framebuffer, where the states
 * have one place: the kernel advances them where they lie */
int path_step(rt1w_context* c, const rt1w_path_params* p, const void* in, void* out, void* out_node, bool host, rt1w_stats* stats) {
    if (!c) { set_error("null argument"); return RT1W_ERR_INVALID; }
    if (const char* why = rt_path_step_refusal((const RtPathParams*)p, in, out, out_node, !host)) { set_error(why); return RT1W_ERR_INVALID; }
    int variant = c->variant;
    const int rc = forced_variant(c, p->flags, true, &variant);
    if (rc < 0) return rc;
    const uint64_t node_bytes = p->n * sizeof(uint32_t);
    /* host: the caller's states may have any alignment, they are copied as bytes; the node indices are 4 bytes each, staged as room of
     * whole doubles and copied out here in their own size */
    Staged s[] = {{(const double*)in, (double*)out, (size_t)p->n * PATH_STATE_DOUBLES, FRAMEBUFFER, "path state copy", "path state copy"},
                  {nullptr, nullptr, host && out_node ? (size_t)((p->n + 1u) / 2u) : 0u, FRAMEBUFFER, nullptr, nullptr}};
    return staged_entry(c, host, s, stats, [&](rt1w_stats* st) {
        uint32_t* d_node = host ? (out_node ? (uint32_t*)s[1].d_out : nullptr) : (uint32_t*)out_node;
        unsigned long long segments = 0u;
        const int r = path_counted_run(c, p->n, "path step", st, &segments, [&](unsigned long long* d_count, hipStream_t stream, unsigned* launch) {
            return rt1w_internal_path_step_launch(&c->view, p, variant, s[0].d_in, s[0].d_out, d_node, d_count, stream, launch);
        });
        if (r < 0) return r;
        st->segments = segments;
        st->variant = (uint32_t)variant;
        if (host && out_node && !hip_ok(hipMemcpy(out_node, d_node, node_bytes, hipMemcpyDeviceToHost), "node index copy")) return (int)RT1W_ERR_DEVICE;
        return (int)RT1W_OK;
    });
}
/* the two begin entries: the states first in the framebuffer (16-byte aligned there), the list behind them in its own size */
int path_begin(rt1w_context* c, uint32_t width, uint32_t height, uint64_t global_seed, uint32_t max_depth, const void* pixels, uint64_t n, void* out,
               bool host, rt1w_stats* stats) {
    if (!c) { set_error("null argument"); return RT1W_ERR_INVALID; }
    if (const char* why = rt_path_begin_refusal(width, height, global_seed, pixels, n, out, !host)) { set_error(why); return RT1W_ERR_INVALID; }
    const uint64_t pixel_bytes = n * 3u * sizeof(uint32_t);
    Staged s[] = {{nullptr, (double*)out, (size_t)n * PATH_STATE_DOUBLES, FRAMEBUFFER, nullptr, "path state copy"},
                  {nullptr, nullptr, host ? (size_t)((n * 3u + 1u) / 2u) : 0u, FRAMEBUFFER, nullptr, nullptr}};
    bool outside_frame = false;
    const int rc = staged_entry(c, host, s, stats, [&](rt1w_stats* st) {
        const uint32_t* d_pixels = host ? (const uint32_t*)s[1].d_out : (const uint32_t*)pixels;
        if (host && !hip_ok(hipMemcpy(s[1].d_out, pixels, pixel_bytes, hipMemcpyHostToDevice), "pixel list copy")) return (int)RT1W_ERR_DEVICE;
        unsigned long long outside = 0u;
        const int r = path_counted_run(c, n, "path begin", st, &outside, [&](unsigned long long* d_count, hipStream_t stream, unsigned* launch) {
            return rt1w_internal_path_begin_launch(&c->view, width, height, (uint32_t)global_seed, max_depth, d_pixels, n, s[0].d_out, d_count, stream, launch);
        });
        if (r < 0) return r;
        outside_frame = outside != 0u;
        st->variant = (uint32_t)c->variant;
        return (int)RT1W_OK;
    });
    if (rc < 0) return rc;
    if (outside_frame) { set_error("path_begin: a pixel of the list lies outside the frame (i >= width or j >= height)"); return RT1W_ERR_INVALID; }
    return RT1W_OK;
}

/* ---- feature-guided denoiser (include/rt1w.h: rt1w_denoise) ---- */
int denoise_validate(const rt1w_context* c, const rt1w_denoise_params* p) {
    if (!c || !p) { set_error("null argument"); return RT1W_ERR_INVALID; }
    if (p->width == 0 || p->height == 0 || p->width > 0x40000000u || p->height > 0x40000000u) { set_error("denoise: width and height must be 1 .. 2^30"); return RT1W_ERR_INVALID; }
    if (p->iterations > 8u) { set_error("denoise: at most 8 iterations"); return RT1W_ERR_INVALID; }
    if (p->flags & ~RT1W_DENOISE_KEEP_ALBEDO) { set_error("denoise: unknown flag (flags: 0 or RT1W_DENOISE_KEEP_ALBEDO)"); return RT1W_ERR_INVALID; }
    const double sig[3] = {p->sigma_colour, p->sigma_normal, p->sigma_depth};
    for (double v : sig)
        if (!(v >= 0.0) || v > 1.7976931348623157e308) { set_error("denoise: a sigma must be finite and >= 0 (0 = default)"); return RT1W_ERR_INVALID; }
    return RT1W_OK;
}
/* the context's two colour buffers (col_bytes per pixel) and guide buffer, grown to the image */
int denoise_reserve(rt1w_context* c, size_t npix, size_t col_bytes) {
    for (int k = 0; k < 3; ++k) {
        const int rc = dev_grow(&c->dn_buf[k], &c->dn_bytes[k], npix * (k == 2 ? rt1w_internal_denoise_sizeof(1) : col_bytes), "hipMalloc(denoise buffers)");
        if (rc < 0) return rc;
    }
    return RT1W_OK;
}
/* prepare pass and levels; grid / block of the level kernel */
int denoise_common(rt1w_context* c, const rt1w_denoise_params* p, const double* d_frame, const double* d_aov, double* d_out, rt1w_stats* stats) {
    const int rc = denoise_reserve(c, (size_t)p->width * p->height, rt1w_internal_denoise_sizeof(0));
    if (rc < 0) return rc;
    return lane_run(c, (uint64_t)p->width * p->height, "denoise", stats, [&](hipStream_t stream, unsigned* launch) {
        return rt1w_internal_denoise_launch(p->width, p->height, p->iterations, p->flags, p->sigma_colour, p->sigma_normal, p->sigma_depth, d_frame, d_aov,
                                            d_out, c->dn_buf[0], c->dn_buf[1], c->dn_buf[2], stream, launch);
    });
}
/* the two denoise entries.  Host form: the frame is filtered in place, the feature buffers lie behind it */
int denoise(rt1w_context* c, const rt1w_denoise_params* p, const double* frame, const double* aov, double* out, bool host, rt1w_stats* stats) {
    const int rc = denoise_validate(c, p);
    if (rc < 0) return rc;
    if (!frame || !aov || !out) { set_error("null buffer"); return RT1W_ERR_INVALID; }
    const size_t npix = (size_t)p->width * p->height;
    Staged s[] = {{frame, out, npix * 3, FRAMEBUFFER, "denoise: frame copy", "denoise: result copy"},
                  {aov, nullptr, npix * RT1W_AOV_CHANNELS, FRAMEBUFFER, "denoise: feature buffer copy", nullptr}};
    return staged_entry(c, host, s, stats, [&](rt1w_stats* st) { return denoise_common(c, p, s[0].d_in, s[1].d_in, s[0].d_out, st); });
}

/* ---- render, then filter (include/rt1w.h: rt1w_render_denoised*, rt1w_render_adaptive): what their preambles share ---- */
/* the render parameters, in this order: validate, the output, the flags rt1w_render_denoised refuses by name, strips, precision */
int denoised_render_validate(const rt1w_context* c, const rt1w_render_params* p, const void* out_rgb) {
    int rc = validate(c, p);
    if (rc < 0) return rc;
    if (!out_rgb) { set_error("null output"); return RT1W_ERR_INVALID; }
    if ((rc = refuse_named_flag(p->flags, true, " does not apply to rt1w_render_denoised")) < 0) return rc;
    if (p->strip_rows) { set_error("rt1w_render_denoised takes a contiguous tile (strip_rows must be 0): denoise the gathered frame with rt1w_denoise"); return RT1W_ERR_INVALID; }
    if (p->precision != RT1W_PRECISION_F64) { set_error("RT1W_PRECISION_F32 does not apply to rt1w_render_denoised (the filter is f64 only)"); return RT1W_ERR_INVALID; }
    return RT1W_OK;
}
/* *dp: the filter's parameters for the w x h pixels rendered -- the caller's (null: every default), whose width / height are 0 or those */
int denoised_filter_params(const rt1w_context* c, const rt1w_denoise_params* d, uint32_t w, uint32_t h, rt1w_denoise_params* dp) {
    memset(dp, 0, sizeof *dp);
    if (d) *dp = *d;
    if ((dp->width && dp->width != w) || (dp->height && dp->height != h)) { set_error("denoise: width / height must be 0 or the tile's"); return RT1W_ERR_INVALID; }
    dp->width = w; dp->height = h;
    return denoise_validate(c, dp);
}
/* rt1w_render_denoised and, with `deep`, rt1w_render_denoised_deep: the frame in the framebuffer, the feature buffers behind it */
int render_denoised(rt1w_context* c, const rt1w_render_params* p, const rt1w_denoise_params* d, const AovDeep* deep, double* out_rgb, rt1w_stats* stats) {
    int rc = aov_deep_validate(deep);
    if (rc < 0) return rc;
    if ((rc = denoised_render_validate(c, p, out_rgb)) < 0) return rc;
    rt1w_denoise_params dp;
    if ((rc = denoised_filter_params(c, d, p->tile_w, p->tile_h, &dp)) < 0) return rc;
    const size_t npix = (size_t)p->tile_w * p->tile_h;
    Staged s[] = {{nullptr, out_rgb, npix * 3, FRAMEBUFFER, nullptr, "denoised frame copy"}, {nullptr, nullptr, npix * RT1W_AOV_CHANNELS, FRAMEBUFFER, nullptr, nullptr}};
    return staged_entry(c, true, s, stats, [&](rt1w_stats* st) {
        double *d_frame = s[0].d_out, *d_aov = s[1].d_out;
        memset(st, 0, sizeof *st);
        int r = render_common(c, p, d_frame, st);
        if (r < 0) return r;
        rt1w_render_params ap = *p; /* the feature buffers of the same tile, samples and seed, by the scene's own variant */
        ap.flags = 0u;
        rt1w_stats sa, sd;
        if ((r = render_aov_common(c, &ap, deep, d_aov, &sa)) < 0) return r;
        if ((r = denoise_common(c, &dp, d_frame, d_aov, d_frame, &sd)) < 0) return r;
        st->kernel_ms = st->kernel_ms + sa.kernel_ms + sd.kernel_ms;
        st->grid = sd.grid; st->block = sd.block;
        return RT1W_OK;
    });
}

/* ---- variance-guided denoiser (include/rt1w.h: rt1w_batch_variance, rt1w_denoise_var, rt1w_render_denoised_var) ---- */
int batches_validate(uint32_t batches, uint32_t batch_spp) {
    if (rt_dv_batches_ok(batches, batch_spp)) return RT1W_OK;
    set_error("batch variance: 2 .. 16 batches of >= 1 samples each, at most 2^32 - 1 samples in all");
    return RT1W_ERR_INVALID;
}
int sigma_variance_validate(double sigma_variance) {
    double sv;
    if (rt_dv_sigma(sigma_variance, sv)) return RT1W_OK;
    set_error("denoise: sigma_variance must be finite and >= 0 (0 = default)");
    return RT1W_ERR_INVALID;
}
int batch_variance_common(rt1w_context* c, uint32_t w, uint32_t h, uint32_t batches, uint32_t batch_spp, uint32_t flags, const double* d_sums,
                          const double* d_aov, double* d_frame, double* d_var, rt1w_stats* stats) {
    return lane_run(c, (uint64_t)w * h, "batch variance", stats, [&](hipStream_t stream, unsigned* launch) {
        return rt1w_internal_batch_variance_launch(w, h, batches, batch_spp, flags, d_sums, d_aov, d_frame, d_var, stream, launch);
    });
}
int denoise_var_common(rt1w_context* c, const rt1w_denoise_params* p, double sigma_variance, const double* d_frame, const double* d_aov,
                       const double* d_var, double* d_out, rt1w_stats* stats) {
    const int rc = denoise_reserve(c, (size_t)p->width * p->height, rt1w_internal_denoise_var_sizeof());
    if (rc < 0) return rc;
    return lane_run(c, (uint64_t)p->width * p->height, "denoise", stats, [&](hipStream_t stream, unsigned* launch) {
        return rt1w_internal_denoise_var_launch(p->width, p->height, p->iterations, p->flags, p->sigma_normal, p->sigma_depth, sigma_variance, d_frame, d_aov,
                                                d_var, d_out, c->dn_buf[0], c->dn_buf[1], c->dn_buf[2], stream, launch);
    });
}
/* the two batch-variance entries.  Host form: frame, var and the feature buffers in the framebuffer, the batch sums in the batch buffer */
int batch_variance(rt1w_context* c, uint32_t w, uint32_t h, uint32_t batches, uint32_t batch_spp, uint32_t flags, const double* sums, const double* aov,
                   double* frame, double* var, bool host, rt1w_stats* stats) {
    if (!c) { set_error("null argument"); return RT1W_ERR_INVALID; }
    rt1w_denoise_params dp;
    memset(&dp, 0, sizeof dp);
    dp.width = w; dp.height = h; dp.flags = flags;
    int rc = denoise_validate(c, &dp);
    if (rc < 0) return rc;
    if ((rc = batches_validate(batches, batch_spp)) < 0) return rc;
    if (!sums || !aov || !frame || !var) { set_error("null buffer"); return RT1W_ERR_INVALID; }
    const size_t npix = (size_t)w * h;
    Staged s[] = {{sums, nullptr, npix * 3 * batches, BATCH_BUFFER, "batch variance: sums copy", nullptr},
                  {nullptr, frame, npix * 3, FRAMEBUFFER, nullptr, "batch variance: frame copy"},
                  {nullptr, var, npix, FRAMEBUFFER, nullptr, "batch variance: variance copy"},
                  {aov, nullptr, npix * RT1W_AOV_CHANNELS, FRAMEBUFFER, "batch variance: feature buffer copy", nullptr}};
    return staged_entry(c, host, s, stats, [&](rt1w_stats* st) {
        return batch_variance_common(c, w, h, batches, batch_spp, flags, s[0].d_in, s[3].d_in, s[1].d_out, s[2].d_out, st);
    });
}
/* the two rt1w_denoise_var entries: as denoise(), with the variance buffer between the frame and the feature buffers */
int denoise_var(rt1w_context* c, const rt1w_denoise_params* p, const double* frame, const double* aov, const double* var, double sigma_variance,
                double* out, bool host, rt1w_stats* stats) {
    int rc = denoise_validate(c, p);
    if (rc < 0) return rc;
    if ((rc = sigma_variance_validate(sigma_variance)) < 0) return rc;
    if (!frame || !aov || !var || !out) { set_error("null buffer"); return RT1W_ERR_INVALID; }
    const size_t npix = (size_t)p->width * p->height;
    Staged s[] = {{frame, out, npix * 3, FRAMEBUFFER, "denoise: frame copy", "denoise: result copy"},
                  {var, nullptr, npix, FRAMEBUFFER, "denoise: variance copy", nullptr},
                  {aov, nullptr, npix * RT1W_AOV_CHANNELS, FRAMEBUFFER, "denoise: feature buffer copy", nullptr}};
    return staged_entry(c, host, s, stats, [&](rt1w_stats* st) {
        return denoise_var_common(c, p, sigma_variance, s[0].d_in, s[2].d_in, s[1].d_in, s[0].d_out, st);
    });
}
/* rt1w_render_denoised_var: the batches' sums in the context's batch buffer; frame, var and the deep feature buffers in the framebuffer */
int render_denoised_var(rt1w_context* c, const rt1w_render_params* p, const rt1w_denoise_params* d, uint32_t batches, double sigma_variance,
                        const AovDeep& deep, double* out_rgb, rt1w_stats* stats) {
    int rc = aov_deep_validate(&deep);
    if (rc < 0) return rc;
    if ((rc = sigma_variance_validate(sigma_variance)) < 0) return rc;
    if ((rc = denoised_render_validate(c, p, out_rgb)) < 0) return rc;
    uint32_t k = 0u, n = 0u;
    if (!rt_dv_split(p->spp, batches, k, n)) { set_error("rt1w_render_denoised_var: 2 .. 16 batches (0 = 4), and spp a multiple of their number"); return RT1W_ERR_INVALID; }
    rt1w_denoise_params dp;
    if ((rc = denoised_filter_params(c, d, p->tile_w, p->tile_h, &dp)) < 0) return rc;
    const size_t npix = (size_t)p->tile_w * p->tile_h;
    Staged s[] = {{nullptr, out_rgb, npix * 3, FRAMEBUFFER, nullptr, "denoised frame copy"}, {nullptr, nullptr, npix, FRAMEBUFFER, nullptr, nullptr},
                  {nullptr, nullptr, npix * RT1W_AOV_CHANNELS, FRAMEBUFFER, nullptr, nullptr}, {nullptr, nullptr, npix * 3 * k, BATCH_BUFFER, nullptr, nullptr}};
    return staged_entry(c, true, s, stats, [&](rt1w_stats* st) {
        double *d_frame = s[0].d_out, *d_var = s[1].d_out, *d_aov = s[2].d_out, *d_sums = s[3].d_out;
        int r;
        rt1w_render_params bp = *p; /* batch b: samples sample_offset + b n .. + n - 1 as raw sums; one chunk size for all, the default of n samples */
        bp.flags |= RT1W_OUT_SUM;
        bp.spp = n;
        for (uint32_t b = 0; b < k; ++b) {
            bp.sample_offset = p->sample_offset + b * n;
            rt1w_stats sb;
            memset(&sb, 0, sizeof sb);
            if ((r = render_common(c, &bp, d_sums + npix * 3 * b, &sb)) < 0) return r;
            if (b == 0u) *st = sb;
            else stats_add(st, sb);
        }
        rt1w_render_params ap = *p; /* the feature buffers of the same tile, all k n samples and seed, by the scene's own variant */
        ap.flags = 0u;
        rt1w_stats sa, sv, sd;
        if ((r = render_aov_common(c, &ap, &deep, d_aov, &sa)) < 0) return r;
        if ((r = batch_variance_common(c, dp.width, dp.height, k, n, dp.flags, d_sums, d_aov, d_frame, d_var, &sv)) < 0) return r;
        if ((r = denoise_var_common(c, &dp, sigma_variance, d_frame, d_aov, d_var, d_frame, &sd)) < 0) return r;
        st->kernel_ms = st->kernel_ms + sa.kernel_ms + sv.kernel_ms + sd.kernel_ms;
        st->grid = sd.grid; st->block = sd.block;
        return RT1W_OK;
    });
}

/* ---- adaptive sampling (include/rt1w.h: rt1w_accum_merge, rt1w_accum_resolve, rt1w_accum_tile_error, rt1w_render_adaptive) ---- */
int accum_frame_validate(const rt1w_context* c, uint32_t w, uint32_t h) {
    if (!c) { set_error("null argument"); return RT1W_ERR_INVALID; }
    if (rt_ad_frame_ok(w, h)) return RT1W_OK;
    set_error("accumulator: width and height must be 1 .. 2^30");
    return RT1W_ERR_INVALID;
}
int accum_merge_common(rt1w_context* c, uint32_t w, uint32_t h, uint32_t x0, uint32_t y0, uint32_t tw, uint32_t th, uint32_t batch_spp, uint32_t flags,
                       const double* d_sums, const double* d_aov, double* d_acc, rt1w_stats* stats) {
    return lane_run(c, (uint64_t)tw * th, "accumulator merge", stats, [&](hipStream_t stream, unsigned* launch) {
        return rt1w_internal_accum_merge_launch(w, h, x0, y0, tw, th, batch_spp, flags, d_sums, d_aov, d_acc, stream, launch);
    });
}
/* the list is checked by the caller (rt_ad_tiles_check) */
int accum_merge_tiles_common(rt1w_context* c, uint32_t w, uint32_t h, uint32_t tile, const rt1w_tile* tiles, uint32_t n, uint32_t batch_spp, uint32_t flags,
                             const double* d_sums, const double* d_aov, double* d_acc, rt1w_stats* stats) {
    const uint32_t* d_rec = nullptr;
    const int rc = tiles_upload(c, tiles, n, &d_rec);
    if (rc < 0) return rc;
    return lane_run(c, rt_ad_list_pixels(w, h, tile, tiles, n), "accumulator merge (tile list)", stats, [&](hipStream_t stream, unsigned* launch) {
        return rt1w_internal_accum_merge_tiles_launch(w, h, tile, d_rec, n, batch_spp, flags, d_sums, d_aov, d_acc, stream, launch);
    });
}
int accum_resolve_common(rt1w_context* c, uint32_t w, uint32_t h, uint32_t batch_spp, const double* d_acc, double* d_frame, double* d_var, double* d_spp,
                         rt1w_stats* stats) {
    return lane_run(c, (uint64_t)w * h, "accumulator resolve", stats, [&](hipStream_t stream, unsigned* launch) {
        return rt1w_internal_accum_resolve_launch(w, h, batch_spp, d_acc, d_frame, d_var, d_spp, stream, launch);
    });
}
int accum_tile_error_common(rt1w_context* c, uint32_t w, uint32_t h, uint32_t tile, const double* d_acc, double* d_err, rt1w_stats* stats) {
    return lane_run(c, (uint64_t)w * h, "tile error", stats, [&](hipStream_t stream, unsigned* launch) {
        return rt1w_internal_accum_tile_error_launch(w, h, tile, d_acc, d_err, stream, launch);
    });
}
/* the four rt1w_accum_merge entries once their own check has passed; run(d_sums, d_aov, d_acc, st).  Host form: the feature buffers and,
 * behind them, the batch (`tpix` pixels) in the framebuffer, the accumulator in the accumulator buffer */
template <class Run>
int accum_merge_entry(rt1w_context* c, size_t npix, size_t tpix, const double* sums, const double* aov, double* acc, bool host, rt1w_stats* stats, Run run) {
    if (!sums || !aov || !acc) { set_error("null buffer"); return RT1W_ERR_INVALID; }
    Staged s[] = {{aov, nullptr, npix * RT1W_AOV_CHANNELS, FRAMEBUFFER, "accumulator merge: feature buffer copy", nullptr},
                  {sums, nullptr, tpix * 3, FRAMEBUFFER, "accumulator merge: sums copy", nullptr},
                  {acc, acc, npix * RT_AD_RECORD, ACCUM_BUFFER, "accumulator merge: accumulator copy", "accumulator merge: result copy"}};
    return staged_entry(c, host, s, stats, [&](rt1w_stats* st) { return run(s[1].d_in, s[0].d_in, s[2].d_out, st); });
}
int accum_merge(rt1w_context* c, uint32_t w, uint32_t h, uint32_t x0, uint32_t y0, uint32_t tw, uint32_t th, uint32_t batch_spp, uint32_t flags,
                const double* sums, const double* aov, double* acc, bool host, rt1w_stats* stats) {
    const int rc = accum_frame_validate(c, w, h);
    if (rc < 0) return rc;
    if (!rt_ad_rect_ok(w, h, x0, y0, tw, th, batch_spp, flags)) {
        set_error("accumulator merge: the rectangle must lie inside the frame, batch_spp >= 1, flags 0 or RT1W_DENOISE_KEEP_ALBEDO");
        return RT1W_ERR_INVALID;
    }
    return accum_merge_entry(c, (size_t)w * h, (size_t)tw * th, sums, aov, acc, host, stats, [&](const double* d_sums, const double* d_aov, double* d_acc, rt1w_stats* st) {
        return accum_merge_common(c, w, h, x0, y0, tw, th, batch_spp, flags, d_sums, d_aov, d_acc, st);
    });
}
int accum_merge_tiles(rt1w_context* c, uint32_t w, uint32_t h, uint32_t tile, const rt1w_tile* tiles, uint32_t n, uint32_t batch_spp, uint32_t flags,
                      const double* sums, const double* aov, double* acc, bool host, rt1w_stats* stats) {
    if (!c) { set_error("null argument"); return RT1W_ERR_INVALID; }
    if (const char* why = rt_ad_tiles_check(w, h, tile, tiles, n, batch_spp, flags)) { set_error(why); return RT1W_ERR_INVALID; }
    return accum_merge_entry(c, (size_t)w * h, (size_t)n * tile * tile, sums, aov, acc, host, stats, [&](const double* d_sums, const double* d_aov, double* d_acc, rt1w_stats* st) {
        return accum_merge_tiles_common(c, w, h, tile, tiles, n, batch_spp, flags, d_sums, d_aov, d_acc, st);
    });
}
int accum_resolve(rt1w_context* c, uint32_t w, uint32_t h, uint32_t batch_spp, const double* acc, double* frame, double* var, double* spp, bool host,
                  rt1w_stats* stats) {
    const int rc = accum_frame_validate(c, w, h);
    if (rc < 0) return rc;
    if (batch_spp == 0u) { set_error("accumulator resolve: batch_spp must be >= 1"); return RT1W_ERR_INVALID; }
    if (!acc || !frame || !var || !spp) { set_error("null buffer"); return RT1W_ERR_INVALID; }
    const size_t npix = (size_t)w * h;
    Staged s[] = {{acc, nullptr, npix * RT_AD_RECORD, ACCUM_BUFFER, "accumulator resolve: accumulator copy", nullptr},
                  {nullptr, frame, npix * 3, FRAMEBUFFER, nullptr, "accumulator resolve: frame copy"},
                  {nullptr, var, npix, FRAMEBUFFER, nullptr, "accumulator resolve: variance copy"},
                  {nullptr, spp, npix, FRAMEBUFFER, nullptr, "accumulator resolve: count copy"}};
    return staged_entry(c, host, s, stats, [&](rt1w_stats* st) {
        return accum_resolve_common(c, w, h, batch_spp, s[0].d_in, s[1].d_out, s[2].d_out, s[3].d_out, st);
    });
}
int accum_tile_error(rt1w_context* c, uint32_t w, uint32_t h, uint32_t tile, const double* acc, double* err, bool host, rt1w_stats* stats) {
    const int rc = accum_frame_validate(c, w, h);
    if (rc < 0) return rc;
    if (!rt_ad_tile_ok(tile)) { set_error("tile error: tile must be a multiple of 16 in 16 .. 256"); return RT1W_ERR_INVALID; }
    if (!acc || !err) { set_error("null buffer"); return RT1W_ERR_INVALID; }
    const size_t npix = (size_t)w * h, ntiles = (size_t)((w + tile - 1u) / tile) * ((h + tile - 1u) / tile);
    Staged s[] = {{acc, nullptr, npix * RT_AD_RECORD, ACCUM_BUFFER, "tile error: accumulator copy", nullptr},
                  {nullptr, err, ntiles, ACCUM_BUFFER, nullptr, "tile error: result copy"}};
    return staged_entry(c, host, s, stats, [&](rt1w_stats* st) { return accum_tile_error_common(c, w, h, tile, s[0].d_in, s[1].d_out, st); });
}
/* rt1w_render_aov_device, then per batch rt1w_render_device + rt1w_accum_merge_device, per round rt1w_accum_tile_error_device and the plan,
 * rt1w_accum_resolve_device and (d) rt1w_denoise_var_device: frame, var, spp and the feature buffers in the framebuffer, a batch's sums in
 * the batch buffer, the accumulator and the tile errors in the accumulator buffer */
int render_adaptive(rt1w_context* c, const rt1w_render_params* p, const rt1w_adaptive_params* a, const rt1w_denoise_params* d, double sigma_variance,
                    double* out_rgb, double* out_spp, rt1w_stats* stats) {
    int rc = sigma_variance_validate(sigma_variance);
    if (rc < 0) return rc;
    RtAdPlan plan;
    if (const char* why = rt_ad_make_plan(a, &plan)) { set_error(why); return RT1W_ERR_INVALID; }
    rt1w_render_params q;
    if (p) { q = *p; q.spp = plan.batch_spp; } /* p->spp is ignored: validated as one batch */
    if ((rc = denoised_render_validate(c, p ? &q : nullptr, out_rgb)) < 0) return rc;
    if (p->x0 || p->y0 || p->tile_w != p->width || p->tile_h != p->height) { set_error("rt1w_render_adaptive takes the whole frame (x0 = y0 = 0, tile_w = width, tile_h = height)"); return RT1W_ERR_INVALID; }
    if (plan.one_launch && !tile_round_flags_ok(p->flags)) { set_error("adaptive: with RT1W_ADAPTIVE_ONE_LAUNCH p->flags must be 0 or RT1W_GENERIC (rt1w_render_tiles runs the generic kernels)"); return RT1W_ERR_INVALID; }
    if ((unsigned long long)p->sample_offset + plan.max_spp > 0xFFFFFFFFull) { set_error("adaptive: sample_offset + max_spp exceeds 2^32 - 1"); return RT1W_ERR_INVALID; }
    const uint32_t W = p->width, H = p->height;
    rt1w_denoise_params dp;
    if ((rc = denoised_filter_params(c, d, W, H, &dp)) < 0) return rc;
    const size_t npix = (size_t)W * H;
    const uint32_t tiles_x = (W + plan.tile - 1u) / plan.tile, tiles_y = (H + plan.tile - 1u) / plan.tile;
    const size_t ntiles = (size_t)tiles_x * tiles_y;
    /* one launch per round: a round's batch is whole tiles, the edge tiles' pixels beyond the frame included */
    const size_t batch_px = plan.one_launch ? std::max(npix, ntiles * plan.tile * plan.tile) : npix;
    Staged s[] = {{nullptr, out_rgb, npix * 3, FRAMEBUFFER, nullptr, "adaptive frame copy"}, {nullptr, nullptr, npix, FRAMEBUFFER, nullptr, nullptr},
                  {nullptr, out_spp, npix, FRAMEBUFFER, nullptr, "adaptive count copy"}, {nullptr, nullptr, npix * RT1W_AOV_CHANNELS, FRAMEBUFFER, nullptr, nullptr},
                  {nullptr, nullptr, batch_px * 3, BATCH_BUFFER, nullptr, nullptr},
                  {nullptr, nullptr, npix * RT_AD_RECORD, ACCUM_BUFFER, nullptr, nullptr}, {nullptr, nullptr, ntiles, ACCUM_BUFFER, nullptr, nullptr}};
    return staged_entry(c, true, s, stats, [&](rt1w_stats* st) {
        double *d_frame = s[0].d_out, *d_var = s[1].d_out, *d_spp = s[2].d_out, *d_aov = s[3].d_out, *d_sums = s[4].d_out, *d_acc = s[5].d_out, *d_err = s[6].d_out;
        int r;
        if (!hip_ok(hipMemsetAsync(d_acc, 0, npix * RT_AD_RECORD * sizeof(double), c->lane[0].stream), "accumulator clear")) return RT1W_ERR_DEVICE;
        rt1w_stats sk; /* the last kernel that is no render: its grid and block are reported; other_ms: the time of them all */
        memset(st, 0, sizeof *st);
        rt1w_render_params ap = *p; /* the feature buffers of the pilot's samples, by the scene's own variant */
        ap.flags = 0u; ap.spp = plan.pilot * plan.batch_spp;
        if ((r = render_aov_common(c, &ap, nullptr, d_aov, &sk)) < 0) return r;
        double other_ms = sk.kernel_ms;
        rt1w_render_params bp = *p;
        bp.flags |= RT1W_OUT_SUM;
        bp.spp = plan.batch_spp;
        bp.chunk = p->chunk ? p->chunk : (c->variant >= 2 ? 1u : rt1w_default_chunk(W, H, plan.batch_spp)); /* rt1w_scene_default_chunk of the whole frame */
        bool first = true;
        /* one batch of a rectangle whose pixels all hold m batches: render, merge */
        auto batch = [&](uint32_t x0, uint32_t y0, uint32_t tw, uint32_t th, uint32_t m) -> int {
            bp.x0 = x0; bp.y0 = y0; bp.tile_w = tw; bp.tile_h = th;
            bp.sample_offset = p->sample_offset + m * plan.batch_spp;
            rt1w_stats sb;
            memset(&sb, 0, sizeof sb);
            int e = render_common(c, &bp, d_sums, &sb);
            if (e < 0) return e;
            if (first) { *st = sb; first = false; }
            else stats_add(st, sb);
            if ((e = accum_merge_common(c, W, H, x0, y0, tw, th, plan.batch_spp, plan.flags, d_sums, d_aov, d_acc, &sk)) < 0) return e;
            other_ms += sk.kernel_ms;
            return RT1W_OK;
        };
        for (uint32_t b = 0; b < plan.pilot; ++b)
            if ((r = batch(0u, 0u, W, H, b)) < 0) return r;
        std::vector<uint32_t> m(ntiles, plan.pilot);
        std::vector<double> err(ntiles);
        std::vector<rt1w_tile> list;
        uint32_t rounds = 0;
        for (;;) {
            if ((r = accum_tile_error_common(c, W, H, plan.tile, d_acc, d_err, &sk)) < 0) return r;
            other_ms += sk.kernel_ms;
            if (!hip_ok(hipMemcpy(err.data(), d_err, ntiles * sizeof(double), hipMemcpyDeviceToHost), "tile error copy")) return RT1W_ERR_DEVICE;
            const std::vector<uint32_t> taken = rt_ad_select(plan, tiles_x, tiles_y, W, H, err.data(), m.data());
            if (taken.empty()) break;
            ++rounds;
            if (plan.one_launch) {
                /* RT1W_ADAPTIVE_ONE_LAUNCH: the round's tiles as one list -- one render launch, one merge */
                list.clear();
                for (uint32_t t : taken) list.push_back(rt1w_tile{(t % tiles_x) * plan.tile, (t / tiles_x) * plan.tile, m[t] * plan.batch_spp, 0u});
                bp.sample_offset = p->sample_offset;
                rt1w_stats sb;
                memset(&sb, 0, sizeof sb);
                if ((r = render_tiles_common(c, &bp, plan.tile, list.data(), (uint32_t)list.size(), d_sums, &sb)) < 0) return r;
                stats_add(st, sb);
                if ((r = accum_merge_tiles_common(c, W, H, plan.tile, list.data(), (uint32_t)list.size(), plan.batch_spp, plan.flags, d_sums, d_aov, d_acc, &sk)) < 0) return r;
                other_ms += sk.kernel_ms;
            } else
                for (const RtAdRun& run : rt_ad_group(plan, tiles_x, W, H, taken, m.data()))
                    if ((r = batch(run.x0, run.y0, run.w, run.h, run.m)) < 0) return r;
            for (uint32_t t : taken) ++m[t];
        }
        if ((r = accum_resolve_common(c, W, H, plan.batch_spp, d_acc, d_frame, d_var, d_spp, &sk)) < 0) return r;
        other_ms += sk.kernel_ms;
        if (d) {
            if ((r = denoise_var_common(c, &dp, sigma_variance, d_frame, d_aov, d_var, d_frame, &sk)) < 0) return r;
            other_ms += sk.kernel_ms;
        }
        st->kernel_ms += other_ms;
        st->chunk = bp.chunk; st->n_chunks = rounds;
        st->grid = sk.grid; st->block = sk.block;
        return RT1W_OK;
    });
}

/* ---- adaptive sampling steered by the filtered frame's half-buffer error (include/rt1w.h: rt1w_halves_resolve, rt1w_denoise_var_halves,
 * rt1w_tile_error_map, rt1w_render_adaptive_filtered; rt1w_denoise_cross, rt1w_render_adaptive_cross) ---- */
int halves_resolve_common(rt1w_context* c, uint32_t w, uint32_t h, uint32_t batch_spp, const double* d_acc_a, const double* d_acc_b, double* d_frame,
                          double* d_var, double* d_half_a, double* d_half_b, double* d_spp, rt1w_stats* stats) {
    return lane_run(c, (uint64_t)w * h, "halves resolve", stats, [&](hipStream_t stream, unsigned* launch) {
        return rt1w_internal_halves_resolve_launch(w, h, batch_spp, d_acc_a, d_acc_b, d_frame, d_var, d_half_a, d_half_b, d_spp, stream, launch);
    });
}
/* the filter of a frame's two halves: the launcher of its unit and the bytes per pixel of one of that unit's colour buffers */
struct HalvesFilter {
    decltype(&rt1w_internal_denoise_var_halves_launch) launch;
    unsigned (*col_sizeof)(void);
};
const HalvesFilter halves_filter = {rt1w_internal_denoise_var_halves_launch, rt1w_internal_denoise_var_halves_sizeof};
const HalvesFilter cross_filter = {rt1w_internal_denoise_cross_launch, rt1w_internal_denoise_cross_sizeof};
int denoise_halves_common(rt1w_context* c, const HalvesFilter& f, const rt1w_denoise_params* p, double sigma_variance, const double* d_frame,
                          const double* d_aov, const double* d_var, const double* d_half_a, const double* d_half_b, double* d_out, double* d_err_px,
                          rt1w_stats* stats) {
    const int rc = denoise_reserve(c, (size_t)p->width * p->height, f.col_sizeof());
    if (rc < 0) return rc;
    return lane_run(c, (uint64_t)p->width * p->height, "denoise", stats, [&](hipStream_t stream, unsigned* launch) {
        return f.launch(p->width, p->height, p->iterations, p->flags, p->sigma_normal, p->sigma_depth, sigma_variance, d_frame, d_aov, d_var, d_half_a,
                        d_half_b, d_out, d_err_px, c->dn_buf[0], c->dn_buf[1], c->dn_buf[2], stream, launch);
    });
}
int tile_error_map_common(rt1w_context* c, uint32_t w, uint32_t h, uint32_t tile, const double* d_err_px, double* d_err, rt1w_stats* stats) {
    return lane_run(c, (uint64_t)w * h, "tile error", stats, [&](hipStream_t stream, unsigned* launch) {
        return rt1w_internal_tile_error_map_launch(w, h, tile, d_err_px, d_err, stream, launch);
    });
}
/* the two rt1w_halves_resolve entries.  Host form: the two accumulators in the accumulator buffer, the five results in the framebuffer */
int halves_resolve(rt1w_context* c, uint32_t w, uint32_t h, uint32_t batch_spp, const double* acc_a, const double* acc_b, double* frame, double* var,
                   double* half_a, double* half_b, double* spp, bool host, rt1w_stats* stats) {
    const int rc = accum_frame_validate(c, w, h);
    if (rc < 0) return rc;
    if (batch_spp == 0u) { set_error("halves resolve: batch_spp must be >= 1"); return RT1W_ERR_INVALID; }
    if (!acc_a || !acc_b || !frame || !var || !half_a || !half_b || !spp) { set_error("null buffer"); return RT1W_ERR_INVALID; }
    const size_t npix = (size_t)w * h;
    Staged s[] = {{acc_a, nullptr, npix * RT_AD_RECORD, ACCUM_BUFFER, "halves resolve: accumulator copy", nullptr},
                  {acc_b, nullptr, npix * RT_AD_RECORD, ACCUM_BUFFER, "halves resolve: accumulator copy", nullptr},
                  {nullptr, frame, npix * 3, FRAMEBUFFER, nullptr, "halves resolve: frame copy"},
                  {nullptr, var, npix, FRAMEBUFFER, nullptr, "halves resolve: variance copy"},
                  {nullptr, half_a, npix * 3, FRAMEBUFFER, nullptr, "halves resolve: half copy"},
                  {nullptr, half_b, npix * 3, FRAMEBUFFER, nullptr, "halves resolve: half copy"},
                  {nullptr, spp, npix, FRAMEBUFFER, nullptr, "halves resolve: count copy"}};
    return staged_entry(c, host, s, stats, [&](rt1w_stats* st) {
        return halves_resolve_common(c, w, h, batch_spp, s[0].d_in, s[1].d_in, s[2].d_out, s[3].d_out, s[4].d_out, s[5].d_out, s[6].d_out, st);
    });
}
/* the two rt1w_denoise_var_halves entries and the two rt1w_denoise_cross entries, by `filter`: as denoise_var(), with the two halves behind
 * the variance and the error map behind the frame */
int denoise_var_halves(rt1w_context* c, const rt1w_denoise_params* p, const double* frame, const double* aov, const double* var, const double* half_a,
                       const double* half_b, double sigma_variance, double* out, double* err_px, const HalvesFilter& filter, bool host, rt1w_stats* stats) {
    int rc = denoise_validate(c, p);
    if (rc < 0) return rc;
    if ((rc = sigma_variance_validate(sigma_variance)) < 0) return rc;
    if (!frame || !aov || !var || !half_a || !half_b || !out || !err_px) { set_error("null buffer"); return RT1W_ERR_INVALID; }
    const size_t npix = (size_t)p->width * p->height;
    Staged s[] = {{frame, out, npix * 3, FRAMEBUFFER, "denoise: frame copy", "denoise: result copy"},
                  {nullptr, err_px, npix, FRAMEBUFFER, nullptr, "denoise: error map copy"},
                  {var, nullptr, npix, FRAMEBUFFER, "denoise: variance copy", nullptr},
                  {half_a, nullptr, npix * 3, FRAMEBUFFER, "denoise: half copy", nullptr},
                  {half_b, nullptr, npix * 3, FRAMEBUFFER, "denoise: half copy", nullptr},
                  {aov, nullptr, npix * RT1W_AOV_CHANNELS, FRAMEBUFFER, "denoise: feature buffer copy", nullptr}};
    return staged_entry(c, host, s, stats, [&](rt1w_stats* st) {
        return denoise_halves_common(c, filter, p, sigma_variance, s[0].d_in, s[5].d_in, s[2].d_in, s[3].d_in, s[4].d_in, s[0].d_out, s[1].d_out, st);
    });
}
int tile_error_map(rt1w_context* c, uint32_t w, uint32_t h, uint32_t tile, const double* err_px, double* err, bool host, rt1w_stats* stats) {
    const int rc = accum_frame_validate(c, w, h);
    if (rc < 0) return rc;
    if (!rt_ad_tile_ok(tile)) { set_error("tile error: tile must be a multiple of 16 in 16 .. 256"); return RT1W_ERR_INVALID; }
    if (!err_px || !err) { set_error("null buffer"); return RT1W_ERR_INVALID; }
    const size_t npix = (size_t)w * h, ntiles = (size_t)((w + tile - 1u) / tile) * ((h + tile - 1u) / tile);
    Staged s[] = {{err_px, nullptr, npix, FRAMEBUFFER, "tile error: map copy", nullptr}, {nullptr, err, ntiles, ACCUM_BUFFER, nullptr, "tile error: result copy"}};
    return staged_entry(c, host, s, stats, [&](rt1w_stats* st) { return tile_error_map_common(c, w, h, tile, s[0].d_in, s[1].d_out, st); });
}
/* ---- first-hit feature sums of a list of tiles and the guide accumulator (include/rt1w.h: rt1w_render_aov_tiles, rt1w_guides_merge_tiles,
 * rt1w_guides_resolve) ---- */
/* upload the list, the tile-list AOV kernel of the context's (or the forced) variant into d_out through lane_run; of the stats what that
 * leaves open.  The parameters and the list are checked by the caller (rt_aov_tiles_check) */
int render_aov_tiles_common(rt1w_context* c, const rt1w_render_params* p, uint32_t tile, const rt1w_tile* tiles, uint32_t n, double* d_out, rt1w_stats* stats) {
    int variant = c->variant;
    int rc = forced_variant(c, p->flags, true, &variant);
    if (rc < 0) return rc;
    RtFrame f = frame_of(p);
    f.x0 = 0u; f.y0 = 0u; f.tile_w = tile; f.tile_h = n * tile; /* the list as one virtual tile; not read by the kernels, nor are these: */
    f.max_depth = 1u; f.chunk = p->spp; f.n_chunks = 1u;
    if (rt1w_internal_aov_tiles_sizeof(0) != sizeof(RtSceneView) || rt1w_internal_aov_tiles_sizeof(1) != sizeof(RtFrame)) {
        set_error("tile-list AOV kernels built against another scene layout"); return RT1W_ERR_DEVICE;
    }
    const uint32_t* d_rec = nullptr;
    if ((rc = tiles_upload(c, tiles, n, &d_rec)) < 0) return rc;
    /* first hit: one camera ray per sample; pixels beyond the frame are not traced */
    const uint64_t paths = rt_ad_list_pixels(p->width, p->height, tile, tiles, n) * p->spp;
    rt1w_stats st;
    if ((rc = lane_run(c, paths, "tile-list AOV", &st, [&](hipStream_t stream, unsigned* launch) {
            return rt1w_internal_aov_tiles_launch(&c->view, &f, variant, tile, d_rec, n, d_out, stream, launch);
        })) < 0)
        return rc;
    st.segments = st.paths;
    st.chunk = p->spp; st.n_chunks = 1u;
    st.variant = (uint32_t)variant;
    if (stats) *stats = st;
    return RT1W_OK;
}
/* the two rt1w_render_aov_tiles entries.  What the parameters and the list alone decide comes before the context is looked at.  Host form:
 * the sums in the framebuffer */
int render_aov_tiles(rt1w_context* c, const rt1w_render_params* p, uint32_t tile, const rt1w_tile* tiles, uint32_t n, void* out, bool host, rt1w_stats* stats) {
    if (!p || !tiles || !out) { set_error("null argument"); return RT1W_ERR_INVALID; }
    const char* why = nullptr;
    if (const int rc = rt_aov_tiles_check(p, tile, tiles, n, &why); rc < 0) { set_error(why); return rc; }
    if (!c) { set_error("null argument"); return RT1W_ERR_INVALID; }
    Staged s[] = {{nullptr, (double*)out, (size_t)n * tile * tile * RT1W_AOV_CHANNELS, FRAMEBUFFER, nullptr, "AOV tile sums copy"}};
    return staged_entry(c, host, s, stats, [&](rt1w_stats* st) { return render_aov_tiles_common(c, p, tile, tiles, n, s[0].d_out, st); });
}
/* the list is checked by the caller (rt_gd_tiles_check) */
int guides_merge_tiles_common(rt1w_context* c, uint32_t w, uint32_t h, uint32_t tile, const rt1w_tile* tiles, uint32_t n, uint32_t spp, const double* d_sums,
                              double* d_gacc, rt1w_stats* stats) {
    const uint32_t* d_rec = nullptr;
    const int rc = tiles_upload(c, tiles, n, &d_rec);
    if (rc < 0) return rc;
    return lane_run(c, rt_ad_list_pixels(w, h, tile, tiles, n), "guides merge (tile list)", stats, [&](hipStream_t stream, unsigned* launch) {
        return rt1w_internal_guides_merge_tiles_launch(w, h, tile, d_rec, n, spp, d_sums, d_gacc, stream, launch);
    });
}
int guides_resolve_common(rt1w_context* c, uint32_t w, uint32_t h, const double* d_gacc, double* d_aov, rt1w_stats* stats) {
    return lane_run(c, (uint64_t)w * h, "guides resolve", stats, [&](hipStream_t stream, unsigned* launch) {
        return rt1w_internal_guides_resolve_launch(w, h, d_gacc, d_aov, stream, launch);
    });
}
/* the two rt1w_guides_merge_tiles entries.  Host form: the sums in the framebuffer, the guide accumulator in the accumulator buffer */
int guides_merge_tiles(rt1w_context* c, uint32_t w, uint32_t h, uint32_t tile, const rt1w_tile* tiles, uint32_t n, uint32_t spp, const double* sums,
                       double* gacc, bool host, rt1w_stats* stats) {
    if (const char* why = rt_gd_tiles_check(w, h, tile, tiles, n, spp)) { set_error(why); return RT1W_ERR_INVALID; }
    if (!sums || !gacc) { set_error("null buffer"); return RT1W_ERR_INVALID; }
    if (!c) { set_error("null argument"); return RT1W_ERR_INVALID; }
    Staged s[] = {{sums, nullptr, (size_t)n * tile * tile * RT1W_AOV_CHANNELS, FRAMEBUFFER, "guides merge: sums copy", nullptr},
                  {gacc, gacc, (size_t)w * h * RT_GD_RECORD, ACCUM_BUFFER, "guides merge: accumulator copy", "guides merge: result copy"}};
    return staged_entry(c, host, s, stats, [&](rt1w_stats* st) { return guides_merge_tiles_common(c, w, h, tile, tiles, n, spp, s[0].d_in, s[1].d_out, st); });
}
/* the two rt1w_guides_resolve entries.  Host form: the guide accumulator in the accumulator buffer, the feature buffers in the framebuffer */
int guides_resolve(rt1w_context* c, uint32_t w, uint32_t h, const double* gacc, double* aov, bool host, rt1w_stats* stats) {
    if (!rt_ad_frame_ok(w, h)) { set_error("guides: width and height must be 1 .. 2^30"); return RT1W_ERR_INVALID; }
    if (!gacc || !aov) { set_error("null buffer"); return RT1W_ERR_INVALID; }
    if (!c) { set_error("null argument"); return RT1W_ERR_INVALID; }
    const size_t npix = (size_t)w * h;
    Staged s[] = {{gacc, nullptr, npix * RT_GD_RECORD, ACCUM_BUFFER, "guides resolve: accumulator copy", nullptr},
                  {nullptr, aov, npix * RT1W_AOV_CHANNELS, FRAMEBUFFER, nullptr, "guides resolve: feature buffer copy"}};
    return staged_entry(c, host, s, stats, [&](rt1w_stats* st) { return guides_resolve_common(c, w, h, s[0].d_in, s[1].d_out, st); });
}

/* rt1w_render_aov_device, the pilot's rt1w_render_device + rt1w_accum_merge_device into the halves in turn, then per round
 * rt1w_halves_resolve_device, rt1w_denoise_var_halves_device, rt1w_tile_error_map_device, the plan, one rt1w_render_tiles_device and two
 * rt1w_accum_merge_tiles_device: frame, var, spp, the error map, the feature buffers and the two halves in the framebuffer, a round's
 * sums in the batch buffer, the two accumulators and the tile errors in the accumulator buffer.  rt1w_render_adaptive_cross (`name`) is the same
 * loop with rt1w_denoise_cross_device as its `filter`.  rt1w_render_adaptive_guided is the same loop with `guided`: the feature buffers come
 * from a guide accumulator (behind the tile errors) that every round tops up with the first-hit sums of the tiles it takes (their sums
 * behind the round's in the batch buffer), and the filter is guided by its resolve (a second feature buffer, last in the framebuffer);
 * the pilot's feature buffers go on demodulating the merges */
int render_adaptive_filtered(rt1w_context* c, const rt1w_render_params* p, const rt1w_adaptive_params* a, const rt1w_denoise_params* d, double sigma_variance,
                             double* out_rgb, double* out_spp, double* out_err, const HalvesFilter& filter, bool guided, const char* name, rt1w_stats* stats) {
    int rc = sigma_variance_validate(sigma_variance);
    if (rc < 0) return rc;
    RtAdPlan plan, pair;
    if (const char* why = rt_ad_make_pair_plan(a, &plan, &pair)) { set_error(why); return RT1W_ERR_INVALID; }
    rt1w_render_params q;
    if (p) { /* what the parameters alone decide comes before anything that needs the context */
        if ((rc = refuse_named_flag(p->flags, true, " does not apply to rt1w_render_denoised")) < 0) return rc;
        if (!tile_round_flags_ok(p->flags)) { set_error(std::string(name) + ": p->flags must be 0 or RT1W_GENERIC (the rounds go through rt1w_render_tiles, which runs the generic kernels)"); return RT1W_ERR_INVALID; }
        if (p->x0 || p->y0 || p->tile_w != p->width || p->tile_h != p->height) { set_error(std::string(name) + " takes the whole frame (x0 = y0 = 0, tile_w = width, tile_h = height)"); return RT1W_ERR_INVALID; }
        q = *p; q.spp = plan.batch_spp; /* p->spp is ignored: validated as one batch */
    }
    if ((rc = denoised_render_validate(c, p ? &q : nullptr, out_rgb)) < 0) return rc;
    if ((unsigned long long)p->sample_offset + plan.max_spp > 0xFFFFFFFFull) { set_error("adaptive: sample_offset + max_spp exceeds 2^32 - 1"); return RT1W_ERR_INVALID; }
    const uint32_t W = p->width, H = p->height, n = plan.batch_spp;
    rt1w_denoise_params dp;
    if ((rc = denoised_filter_params(c, d, W, H, &dp)) < 0) return rc;
    const size_t npix = (size_t)W * H;
    const uint32_t tiles_x = (W + plan.tile - 1u) / plan.tile, tiles_y = (H + plan.tile - 1u) / plan.tile;
    const size_t ntiles = (size_t)tiles_x * tiles_y, tile_px = (size_t)plan.tile * plan.tile;
    /* a round's batch is whole tiles, every taken tile twice, the edge tiles' pixels beyond the frame included */
    const size_t batch_px = std::max(npix, 2 * ntiles * tile_px);
    Staged s[] = {{nullptr, out_rgb, npix * 3, FRAMEBUFFER, nullptr, "adaptive frame copy"}, {nullptr, nullptr, npix, FRAMEBUFFER, nullptr, nullptr},
                  {nullptr, out_spp, npix, FRAMEBUFFER, nullptr, "adaptive count copy"}, {nullptr, out_err, npix, FRAMEBUFFER, nullptr, "adaptive error map copy"},
                  {nullptr, nullptr, npix * RT1W_AOV_CHANNELS, FRAMEBUFFER, nullptr, nullptr}, {nullptr, nullptr, npix * 3, FRAMEBUFFER, nullptr, nullptr},
                  {nullptr, nullptr, npix * 3, FRAMEBUFFER, nullptr, nullptr}, {nullptr, nullptr, batch_px * 3, BATCH_BUFFER, nullptr, nullptr},
                  {nullptr, nullptr, npix * RT_AD_RECORD, ACCUM_BUFFER, nullptr, nullptr}, {nullptr, nullptr, npix * RT_AD_RECORD, ACCUM_BUFFER, nullptr, nullptr},
                  {nullptr, nullptr, ntiles, ACCUM_BUFFER, nullptr, nullptr},
                  /* guided only: the guide accumulator, the full-count feature buffers, the first-hit sums of a round's tiles (or of the pilot's: all) */
                  {nullptr, nullptr, guided ? npix * RT_GD_RECORD : 0u, ACCUM_BUFFER, nullptr, nullptr},
                  {nullptr, nullptr, guided ? npix * RT1W_AOV_CHANNELS : 0u, FRAMEBUFFER, nullptr, nullptr},
                  {nullptr, nullptr, guided ? ntiles * tile_px * RT1W_AOV_CHANNELS : 0u, BATCH_BUFFER, nullptr, nullptr}};
    return staged_entry(c, true, s, stats, [&](rt1w_stats* st) {
        double *d_frame = s[0].d_out, *d_var = s[1].d_out, *d_spp = s[2].d_out, *d_err_px = s[3].d_out, *d_aov = s[4].d_out, *d_half_a = s[5].d_out,
               *d_half_b = s[6].d_out, *d_sums = s[7].d_out, *d_acc_a = s[8].d_out, *d_acc_b = s[9].d_out, *d_err = s[10].d_out;
        double *d_gacc = s[11].d_out, *d_guides = guided ? s[12].d_out : d_aov, *d_aov_sums = s[13].d_out;
        int r;
        /* the two accumulators lie one behind the other: one clear */
        if (!hip_ok(hipMemsetAsync(d_acc_a, 0, 2 * npix * RT_AD_RECORD * sizeof(double), c->lane[0].stream), "accumulator clear")) return RT1W_ERR_DEVICE;
        rt1w_stats sk; /* the last kernel that is no render: its grid and block are reported; other_ms: the time of them all */
        memset(st, 0, sizeof *st);
        rt1w_render_params ap = *p; /* the feature buffers of the pilot's samples, by the scene's own variant */
        ap.flags = 0u; ap.spp = plan.pilot * n;
        double other_ms = 0.0;
        std::vector<rt1w_tile> list;
        /* guided: the first-hit sums of `list` (spp and offsets as set), merged into the guide accumulator */
        auto guides_add = [&]() -> int {
            int e = render_aov_tiles_common(c, &ap, plan.tile, list.data(), (uint32_t)list.size(), d_aov_sums, &sk);
            if (e < 0) return e;
            other_ms += sk.kernel_ms;
            if ((e = guides_merge_tiles_common(c, W, H, plan.tile, list.data(), (uint32_t)list.size(), ap.spp, d_aov_sums, d_gacc, &sk)) < 0) return e;
            other_ms += sk.kernel_ms;
            return RT1W_OK;
        };
        if (guided) { /* every tile of the frame in row-major order, into a zeroed guide accumulator; its resolve is rt1w_render_aov_device's bits */
            if (!hip_ok(hipMemsetAsync(d_gacc, 0, npix * RT_GD_RECORD * sizeof(double), c->lane[0].stream), "guide accumulator clear")) return RT1W_ERR_DEVICE;
            for (uint32_t t = 0; t < ntiles; ++t) list.push_back(rt1w_tile{(t % tiles_x) * plan.tile, (t / tiles_x) * plan.tile, 0u, 0u});
            if ((r = guides_add()) < 0) return r;
            if ((r = guides_resolve_common(c, W, H, d_gacc, d_aov, &sk)) < 0) return r;
        } else if ((r = render_aov_common(c, &ap, nullptr, d_aov, &sk)) < 0) return r;
        other_ms += sk.kernel_ms;
        rt1w_render_params bp = *p;
        bp.flags |= RT1W_OUT_SUM;
        bp.spp = n;
        bp.chunk = p->chunk ? p->chunk : (c->variant >= 2 ? 1u : rt1w_default_chunk(W, H, n)); /* rt1w_scene_default_chunk of the whole frame */
        for (uint32_t b = 0; b < plan.pilot; ++b) { /* the pilot: whole-frame batches, even ones into A, odd ones into B */
            bp.sample_offset = p->sample_offset + b * n;
            rt1w_stats sb;
            memset(&sb, 0, sizeof sb);
            if ((r = render_common(c, &bp, d_sums, &sb)) < 0) return r;
            if (b == 0u) *st = sb;
            else stats_add(st, sb);
            if ((r = accum_merge_common(c, W, H, 0u, 0u, W, H, n, plan.flags, d_sums, d_aov, (b & 1u) ? d_acc_b : d_acc_a, &sk)) < 0) return r;
            other_ms += sk.kernel_ms;
        }
        std::vector<uint32_t> m(ntiles, plan.pilot / 2u); /* pairs per tile */
        std::vector<double> err(ntiles);
        uint32_t rounds = 0;
        for (;;) {
            /* the estimate: every pixel holds as many batches in A as in B here; the filter runs in place on the resolved frame */
            if ((r = halves_resolve_common(c, W, H, n, d_acc_a, d_acc_b, d_frame, d_var, d_half_a, d_half_b, d_spp, &sk)) < 0) return r;
            other_ms += sk.kernel_ms;
            if (guided) { /* the guides of every sample the pixel holds */
                if ((r = guides_resolve_common(c, W, H, d_gacc, d_guides, &sk)) < 0) return r;
                other_ms += sk.kernel_ms;
            }
            if ((r = denoise_halves_common(c, filter, &dp, sigma_variance, d_frame, d_guides, d_var, d_half_a, d_half_b, d_frame, d_err_px, &sk)) < 0) return r;
            other_ms += sk.kernel_ms;
            const rt1w_stats sf = sk; /* the level kernel's grid and block are the ones reported */
            if ((r = tile_error_map_common(c, W, H, plan.tile, d_err_px, d_err, &sk)) < 0) return r;
            other_ms += sk.kernel_ms;
            sk = sf;
            if (!hip_ok(hipMemcpy(err.data(), d_err, ntiles * sizeof(double), hipMemcpyDeviceToHost), "tile error copy")) return RT1W_ERR_DEVICE;
            const std::vector<uint32_t> taken = rt_ad_select(pair, tiles_x, tiles_y, W, H, err.data(), m.data());
            if (taken.empty()) break; /* this round's filtered frame and error map are the result */
            ++rounds;
            /* one render launch: every taken tile twice, first all of them with the pair's even batch (for A), then all with the odd one */
            const uint32_t nt = (uint32_t)taken.size();
            list.clear();
            for (uint32_t half = 0; half < 2u; ++half)
                for (uint32_t t : taken) list.push_back(rt1w_tile{(t % tiles_x) * plan.tile, (t / tiles_x) * plan.tile, (2u * m[t] + half) * n, 0u});
            bp.sample_offset = p->sample_offset;
            rt1w_stats sb;
            memset(&sb, 0, sizeof sb);
            if ((r = render_tiles_common(c, &bp, plan.tile, list.data(), 2u * nt, d_sums, &sb)) < 0) return r;
            stats_add(st, sb);
            if ((r = accum_merge_tiles_common(c, W, H, plan.tile, list.data(), nt, n, plan.flags, d_sums, d_aov, d_acc_a, &sk)) < 0) return r;
            other_ms += sk.kernel_ms;
            if ((r = accum_merge_tiles_common(c, W, H, plan.tile, list.data() + nt, nt, n, plan.flags, d_sums + (size_t)nt * tile_px * 3, d_aov, d_acc_b, &sk)) < 0) return r;
            other_ms += sk.kernel_ms;
            if (guided) { /* the pair's 2 n samples are contiguous: every taken tile once, in the order taken */
                list.resize(nt);
                ap.spp = 2u * n;
                if ((r = guides_add()) < 0) return r;
            }
            sk = sf;
            for (uint32_t t : taken) ++m[t];
        }
        st->kernel_ms += other_ms;
        st->chunk = bp.chunk; st->n_chunks = rounds;
        st->grid = sk.grid; st->block = sk.block;
        return RT1W_OK;
    });
}

/* ---- temporal accumulation (include/rt1w.h: rt1w_temporal_accumulate, rt1w_render_temporal) ---- */
static_assert(sizeof(rt1w_camera) == sizeof(RtCamera), "rt1w_camera is RtCamera's layout");
int temporal_validate(const rt1w_context* c, const rt1w_temporal_params* p) {
    if (!c || !p) { set_error("null argument"); return RT1W_ERR_INVALID; }
    if (p->width == 0 || p->height == 0 || p->width > 0x40000000u || p->height > 0x40000000u) { set_error("temporal: width and height must be 1 .. 2^30"); return RT1W_ERR_INVALID; }
    if (p->flags & ~RT1W_DENOISE_KEEP_ALBEDO) { set_error("temporal: unknown flag (flags: 0 or RT1W_DENOISE_KEEP_ALBEDO)"); return RT1W_ERR_INVALID; }
    if (!(p->depth_tol >= 0.0) || p->depth_tol > 1.7976931348623157e308) { set_error("temporal: depth_tol must be finite and >= 0 (0 = default)"); return RT1W_ERR_INVALID; }
    if (!(p->normal_min >= 0.0) || p->normal_min > 1.0) { set_error("temporal: normal_min must be 0 .. 1 (0 = default)"); return RT1W_ERR_INVALID; }
    RtTmParams P;
    if (!rt_tm_make_params(p->width, p->height, p->flags, p->max_history, p->depth_tol, p->normal_min, P)) { set_error("temporal: parameters refused"); return RT1W_ERR_INVALID; }
    return RT1W_OK;
}
int temporal_common(rt1w_context* c, const rt1w_temporal_params* p, const double* d_cur_frame, const double* d_cur_aov, const void* cur_cam,
                    const double* d_prev_hist, const double* d_prev_len, const double* d_prev_aov, const void* prev_cam, double* d_hist, double* d_len,
                    double* d_frame_out, rt1w_stats* stats) {
    if (rt1w_internal_temporal_sizeof() != sizeof(rt1w_camera)) { set_error("temporal kernel built against another camera layout"); return RT1W_ERR_DEVICE; }
    return lane_run(c, (uint64_t)p->width * p->height, "temporal accumulation", stats, [&](hipStream_t stream, unsigned* launch) {
        return rt1w_internal_temporal_launch(p->width, p->height, p->flags, p->max_history, p->depth_tol, p->normal_min, d_cur_frame, d_cur_aov, cur_cam,
                                             d_prev_hist, d_prev_len, d_prev_aov, prev_cam, d_hist, d_len, d_frame_out, stream, launch);
    });
}
/* true: output row `o` of an entry's table overlaps another row of it (the caller's buffers: an input's `in`, an output's `out`) */
template <size_t N>
bool staged_output_overlaps(const Staged (&s)[N], size_t o) {
    const char* a = (const char*)s[o].out;
    for (size_t k = 0; k < N; ++k) {
        const char* b = s[k].out ? (const char*)s[k].out : (const char*)s[k].in;
        if (k != o && a < b + s[k].count * sizeof(double) && b < a + s[o].count * sizeof(double)) return true;
    }
    return false;
}
/* the two rt1w_temporal_accumulate entries.  Host form: the eight buffers one behind the other in the framebuffer */
int temporal_accumulate(rt1w_context* c, const rt1w_temporal_params* p, const double* cur_frame, const double* cur_aov, const rt1w_camera* cur_cam,
                        const double* prev_hist, const double* prev_len, const double* prev_aov, const rt1w_camera* prev_cam, double* hist, double* len,
                        double* frame_out, bool host, rt1w_stats* stats) {
    const int rc = temporal_validate(c, p);
    if (rc < 0) return rc;
    if (!cur_frame || !cur_aov || !prev_hist || !prev_len || !prev_aov || !hist || !len || !frame_out) { set_error("null buffer"); return RT1W_ERR_INVALID; }
    if (!cur_cam || !prev_cam) { set_error("null camera"); return RT1W_ERR_INVALID; }
    const size_t npix = (size_t)p->width * p->height;
    Staged s[] = {{cur_frame, nullptr, npix * 3, FRAMEBUFFER, "temporal: frame copy", nullptr},
                  {cur_aov, nullptr, npix * RT1W_AOV_CHANNELS, FRAMEBUFFER, "temporal: feature buffer copy", nullptr},
                  {prev_hist, nullptr, npix * 3, FRAMEBUFFER, "temporal: history copy", nullptr},
                  {prev_len, nullptr, npix, FRAMEBUFFER, "temporal: history length copy", nullptr},
                  {prev_aov, nullptr, npix * RT1W_AOV_CHANNELS, FRAMEBUFFER, "temporal: previous feature buffer copy", nullptr},
                  {nullptr, hist, npix * 3, FRAMEBUFFER, nullptr, "temporal: history result copy"},
                  {nullptr, len, npix, FRAMEBUFFER, nullptr, "temporal: history length result copy"},
                  {nullptr, frame_out, npix * 3, FRAMEBUFFER, nullptr, "temporal: frame result copy"}};
    for (size_t o = 5; o < 8; ++o) /* the three outputs */
        if (staged_output_overlaps(s, o)) { set_error("temporal: hist, len and frame_out must not overlap each other or an input"); return RT1W_ERR_INVALID; }
    return staged_entry(c, host, s, stats, [&](rt1w_stats* st) {
        return temporal_common(c, p, s[0].d_in, s[1].d_in, cur_cam, s[2].d_in, s[3].d_in, s[4].d_in, prev_cam, s[5].d_out, s[6].d_out, s[7].d_out, st);
    });
}
/* rt1w_render_temporal: frame_out and the frame in the framebuffer; history, its length and the feature buffers in the context's two state sets */
int render_temporal(rt1w_context* c, const rt1w_render_params* p, const rt1w_temporal_params* t, const rt1w_denoise_params* d, double* out_rgb, rt1w_stats* stats) {
    int rc = denoised_render_validate(c, p, out_rgb);
    if (rc < 0) return rc;
    if (p->x0 != 0u || p->y0 != 0u || p->tile_w != p->width || p->tile_h != p->height) {
        set_error("rt1w_render_temporal takes the whole image (the reprojection works in image coordinates)"); return RT1W_ERR_INVALID;
    }
    rt1w_temporal_params tp;
    memset(&tp, 0, sizeof tp);
    if (t) tp = *t;
    if ((tp.width && tp.width != p->width) || (tp.height && tp.height != p->height)) { set_error("temporal: width / height must be 0 or the image's"); return RT1W_ERR_INVALID; }
    tp.width = p->width; tp.height = p->height;
    if ((rc = temporal_validate(c, &tp)) < 0) return rc;
    rt1w_denoise_params dp;
    if (d && (rc = denoised_filter_params(c, d, p->width, p->height, &dp)) < 0) return rc;
    const size_t npix = (size_t)p->width * p->height;
    Staged s[] = {{nullptr, out_rgb, npix * 3, FRAMEBUFFER, nullptr, "temporal frame copy"}, {nullptr, nullptr, npix * 3, FRAMEBUFFER, nullptr, nullptr}};
    return staged_entry(c, true, s, stats, [&](rt1w_stats* st) {
        double *d_out = s[0].d_out, *d_frame = s[1].d_out;
        const size_t set_bytes = npix * (3 + 1 + RT1W_AOV_CHANNELS) * sizeof(double);
        int r;
        if (c->tm_w != p->width || c->tm_h != p->height) c->tm_valid = false;
        for (int k = 0; k < 2; ++k)
            if ((r = dev_grow(&c->tm_buf[k], &c->tm_bytes[k], set_bytes, "hipMalloc(temporal state)")) < 0) { c->tm_valid = false; return r; }
        c->tm_w = p->width; c->tm_h = p->height;
        const int prev = c->tm_prev, cur = 1 - prev;
        double *ph = (double*)c->tm_buf[prev], *pl = ph + npix * 3, *pa = pl + npix;
        double *ch = (double*)c->tm_buf[cur], *cl = ch + npix * 3, *ca = cl + npix;
        if (!c->tm_valid) { /* no history: prev_len = 0 everywhere (all of the set is zeroed), prev_cam = cur_cam */
            if (!hip_ok(hipMemsetAsync(ph, 0, set_bytes, c->lane[0].stream), "temporal state reset")) return RT1W_ERR_DEVICE;
            c->tm_cam = c->view.camera;
        }
        memset(st, 0, sizeof *st);
        if ((r = render_common(c, p, d_frame, st)) < 0) return r;
        rt1w_render_params ap = *p; /* the feature buffers of the same image, samples and seed, by the scene's own variant */
        ap.flags = 0u;
        rt1w_stats sa, sm, sd;
        memset(&sd, 0, sizeof sd);
        if ((r = render_aov_common(c, &ap, nullptr, ca, &sa)) < 0) return r;
        c->tm_valid = false; /* a failure from here on leaves no history behind */
        if ((r = temporal_common(c, &tp, d_frame, ca, &c->view.camera, ph, pl, pa, &c->tm_cam, ch, cl, d_out, &sm)) < 0) return r;
        c->tm_prev = cur; c->tm_cam = c->view.camera; c->tm_valid = true;
        if (d && (r = denoise_common(c, &dp, d_out, ca, d_out, &sd)) < 0) return r;
        st->kernel_ms = st->kernel_ms + sa.kernel_ms + sm.kernel_ms + sd.kernel_ms;
        st->grid = d ? sd.grid : sm.grid; st->block = d ? sd.block : sm.block;
        return RT1W_OK;
    });
}

/* ---- the variance of a temporal history (include/rt1w.h: rt1w_temporal_moments, rt1w_temporal_variance, rt1w_render_temporal_var) ---- */
int temporal_moments_common(rt1w_context* c, const rt1w_temporal_params* p, const double* d_cur_frame, const double* d_cur_aov, const void* cur_cam,
                            const double* d_prev_hist, const double* d_prev_m2, const double* d_prev_len, const double* d_prev_aov, const void* prev_cam,
                            double* d_hist, double* d_m2, double* d_len, double* d_frame_out, rt1w_stats* stats) {
    if (rt1w_internal_temporal_var_sizeof() != sizeof(rt1w_camera)) { set_error("temporal kernel built against another camera layout"); return RT1W_ERR_DEVICE; }
    return lane_run(c, (uint64_t)p->width * p->height, "temporal moments", stats, [&](hipStream_t stream, unsigned* launch) {
        return rt1w_internal_temporal_moments_launch(p->width, p->height, p->flags, p->max_history, p->depth_tol, p->normal_min, d_cur_frame, d_cur_aov,
                                                     cur_cam, d_prev_hist, d_prev_m2, d_prev_len, d_prev_aov, prev_cam, d_hist, d_m2, d_len, d_frame_out,
                                                     stream, launch);
    });
}
int temporal_variance_common(rt1w_context* c, uint32_t w, uint32_t h, const double* d_hist, const double* d_m2, const double* d_len, const double* d_aov,
                             double* d_var, rt1w_stats* stats) {
    return lane_run(c, (uint64_t)w * h, "temporal variance", stats, [&](hipStream_t stream, unsigned* launch) {
        return rt1w_internal_temporal_variance_launch(w, h, d_hist, d_m2, d_len, d_aov, d_var, stream, launch);
    });
}
/* the two rt1w_temporal_moments entries.  Host form: the ten buffers one behind the other in the framebuffer */
int temporal_moments(rt1w_context* c, const rt1w_temporal_params* p, const double* cur_frame, const double* cur_aov, const rt1w_camera* cur_cam,
                     const double* prev_hist, const double* prev_m2, const double* prev_len, const double* prev_aov, const rt1w_camera* prev_cam,
                     double* hist, double* m2, double* len, double* frame_out, bool host, rt1w_stats* stats) {
    const int rc = temporal_validate(c, p);
    if (rc < 0) return rc;
    if (!cur_frame || !cur_aov || !prev_hist || !prev_m2 || !prev_len || !prev_aov || !hist || !m2 || !len || !frame_out) { set_error("null buffer"); return RT1W_ERR_INVALID; }
    if (!cur_cam || !prev_cam) { set_error("null camera"); return RT1W_ERR_INVALID; }
    const size_t npix = (size_t)p->width * p->height;
    Staged s[] = {{cur_frame, nullptr, npix * 3, FRAMEBUFFER, "temporal: frame copy", nullptr},
                  {cur_aov, nullptr, npix * RT1W_AOV_CHANNELS, FRAMEBUFFER, "temporal: feature buffer copy", nullptr},
                  {prev_hist, nullptr, npix * 3, FRAMEBUFFER, "temporal: history copy", nullptr},
                  {prev_m2, nullptr, npix, FRAMEBUFFER, "temporal: second moment copy", nullptr},
                  {prev_len, nullptr, npix, FRAMEBUFFER, "temporal: history length copy", nullptr},
                  {prev_aov, nullptr, npix * RT1W_AOV_CHANNELS, FRAMEBUFFER, "temporal: previous feature buffer copy", nullptr},
                  {nullptr, hist, npix * 3, FRAMEBUFFER, nullptr, "temporal: history result copy"},
                  {nullptr, m2, npix, FRAMEBUFFER, nullptr, "temporal: second moment result copy"},
                  {nullptr, len, npix, FRAMEBUFFER, nullptr, "temporal: history length result copy"},
                  {nullptr, frame_out, npix * 3, FRAMEBUFFER, nullptr, "temporal: frame result copy"}};
    for (size_t o = 6; o < 10; ++o) /* the four outputs */
        if (staged_output_overlaps(s, o)) { set_error("temporal: hist, m2, len and frame_out must not overlap each other or an input"); return RT1W_ERR_INVALID; }
    return staged_entry(c, host, s, stats, [&](rt1w_stats* st) {
        return temporal_moments_common(c, p, s[0].d_in, s[1].d_in, cur_cam, s[2].d_in, s[3].d_in, s[4].d_in, s[5].d_in, prev_cam, s[6].d_out, s[7].d_out,
                                       s[8].d_out, s[9].d_out, st);
    });
}
/* the two rt1w_temporal_variance entries.  Host form: the five buffers one behind the other in the framebuffer */
int temporal_variance(rt1w_context* c, uint32_t w, uint32_t h, const double* hist, const double* m2, const double* len, const double* aov, double* var,
                      bool host, rt1w_stats* stats) {
    if (!c) { set_error("null argument"); return RT1W_ERR_INVALID; }
    if (w == 0 || h == 0 || w > 0x40000000u || h > 0x40000000u) { set_error("temporal variance: width and height must be 1 .. 2^30"); return RT1W_ERR_INVALID; }
    if (!hist || !m2 || !len || !aov || !var) { set_error("null buffer"); return RT1W_ERR_INVALID; }
    const size_t npix = (size_t)w * h;
    Staged s[] = {{hist, nullptr, npix * 3, FRAMEBUFFER, "temporal variance: history copy", nullptr},
                  {m2, nullptr, npix, FRAMEBUFFER, "temporal variance: second moment copy", nullptr},
                  {len, nullptr, npix, FRAMEBUFFER, "temporal variance: history length copy", nullptr},
                  {aov, nullptr, npix * RT1W_AOV_CHANNELS, FRAMEBUFFER, "temporal variance: feature buffer copy", nullptr},
                  {nullptr, var, npix, FRAMEBUFFER, nullptr, "temporal variance: result copy"}};
    if (staged_output_overlaps(s, 4)) { set_error("temporal variance: var must not overlap an input"); return RT1W_ERR_INVALID; }
    return staged_entry(c, host, s, stats, [&](rt1w_stats* st) { return temporal_variance_common(c, w, h, s[0].d_in, s[1].d_in, s[2].d_in, s[3].d_in, s[4].d_out, st); });
}
/* rt1w_render_temporal_var: frame_out, the frame and var in the framebuffer; history, second moment, length and the feature buffers in the
 * context's two state sets of this entry */
int render_temporal_var(rt1w_context* c, const rt1w_render_params* p, const rt1w_temporal_params* t, const rt1w_denoise_params* d, double sigma_variance,
                        double* out_rgb, rt1w_stats* stats) {
    /* what the parameters alone decide, before the context is looked at */
    int rc = sigma_variance_validate(sigma_variance);
    if (rc < 0) return rc;
    if (((t ? t->flags : 0u) ^ (d ? d->flags : 0u)) & RT1W_DENOISE_KEEP_ALBEDO) {
        set_error("rt1w_render_temporal_var: the temporal and the denoise parameters must agree on RT1W_DENOISE_KEEP_ALBEDO (the variance is in the units of the history's demodulation)");
        return RT1W_ERR_INVALID;
    }
    if ((rc = denoised_render_validate(c, p, out_rgb)) < 0) return rc;
    if (p->x0 != 0u || p->y0 != 0u || p->tile_w != p->width || p->tile_h != p->height) {
        set_error("rt1w_render_temporal_var takes the whole image (the reprojection works in image coordinates)"); return RT1W_ERR_INVALID;
    }
    rt1w_temporal_params tp;
    memset(&tp, 0, sizeof tp);
    if (t) tp = *t;
    if ((tp.width && tp.width != p->width) || (tp.height && tp.height != p->height)) { set_error("temporal: width / height must be 0 or the image's"); return RT1W_ERR_INVALID; }
    tp.width = p->width; tp.height = p->height;
    if ((rc = temporal_validate(c, &tp)) < 0) return rc;
    rt1w_denoise_params dp;
    if ((rc = denoised_filter_params(c, d, p->width, p->height, &dp)) < 0) return rc;
    const size_t npix = (size_t)p->width * p->height;
    Staged s[] = {{nullptr, out_rgb, npix * 3, FRAMEBUFFER, nullptr, "temporal frame copy"}, {nullptr, nullptr, npix * 3, FRAMEBUFFER, nullptr, nullptr},
                  {nullptr, nullptr, npix, FRAMEBUFFER, nullptr, nullptr}};
    return staged_entry(c, true, s, stats, [&](rt1w_stats* st) {
        double *d_out = s[0].d_out, *d_frame = s[1].d_out, *d_var = s[2].d_out;
        const size_t set_bytes = npix * (3 + 1 + 1 + RT1W_AOV_CHANNELS) * sizeof(double);
        int r;
        if (c->tv_w != p->width || c->tv_h != p->height) c->tv_valid = false;
        for (int k = 0; k < 2; ++k)
            if ((r = dev_grow(&c->tv_buf[k], &c->tv_bytes[k], set_bytes, "hipMalloc(temporal variance state)")) < 0) { c->tv_valid = false; return r; }
        c->tv_w = p->width; c->tv_h = p->height;
        const int prev = c->tv_prev, cur = 1 - prev;
        double *ph = (double*)c->tv_buf[prev], *pm = ph + npix * 3, *pl = pm + npix, *pa = pl + npix;
        double *ch = (double*)c->tv_buf[cur], *cm = ch + npix * 3, *cl = cm + npix, *ca = cl + npix;
        if (!c->tv_valid) { /* no history: prev_len = 0 everywhere (all of the set is zeroed), prev_cam = cur_cam */
            if (!hip_ok(hipMemsetAsync(ph, 0, set_bytes, c->lane[0].stream), "temporal variance state reset")) return RT1W_ERR_DEVICE;
            c->tv_cam = c->view.camera;
        }
        memset(st, 0, sizeof *st);
        if ((r = render_common(c, p, d_frame, st)) < 0) return r;
        rt1w_render_params ap = *p; /* the feature buffers of the same image, samples and seed, by the scene's own variant */
        ap.flags = 0u;
        rt1w_stats sa, sm, sv, sd;
        if ((r = render_aov_common(c, &ap, nullptr, ca, &sa)) < 0) return r;
        c->tv_valid = false; /* a failure from here on leaves no history behind */
        if ((r = temporal_moments_common(c, &tp, d_frame, ca, &c->view.camera, ph, pm, pl, pa, &c->tv_cam, ch, cm, cl, d_out, &sm)) < 0) return r;
        c->tv_prev = cur; c->tv_cam = c->view.camera; c->tv_valid = true;
        if ((r = temporal_variance_common(c, p->width, p->height, ch, cm, cl, ca, d_var, &sv)) < 0) return r;
        if ((r = denoise_var_common(c, &dp, sigma_variance, d_out, ca, d_var, d_out, &sd)) < 0) return r;
        st->kernel_ms = st->kernel_ms + sa.kernel_ms + sm.kernel_ms + sv.kernel_ms + sd.kernel_ms;
        st->grid = sd.grid; st->block = sd.block;
        return RT1W_OK;
    });
}

} // namespace

extern "C" {
int rt1w_context_set_camera(rt1w_context* c, const double look_from[3], const double look_at[3], const double vup[3], double vfov_deg,
                            double aspect_ratio, double aperture, double focus_dist, double time0, double time1) {
    if (!c) { set_error("null argument"); return RT1W_ERR_INVALID; }
    RtCamera cam;
    const char* why = nullptr;
    if (camera_make(look_from, look_at, vup, vfov_deg, aspect_ratio, aperture, focus_dist, time0, time1, &cam, &why) < 0) { set_error(why); return RT1W_ERR_INVALID; }
    /* the view every f64 kernel takes by value -- the generic, scene-specialised, reference-stream, pair-walk and tile-list kernels and the
     * AOV kernels all read this one copy -- and the f32 scene's rounded copy, if it has been built */
    c->view.camera = cam;
    rt1w_internal_f32_set_camera(c->f32_scene, &c->view);
    return RT1W_OK;
}
int rt1w_context_get_camera(const rt1w_context* c, rt1w_camera* out) {
    if (!c || !out) { set_error("null argument"); return RT1W_ERR_INVALID; }
    memcpy(out, &c->view.camera, sizeof *out);
    return RT1W_OK;
}
int rt1w_temporal_accumulate(rt1w_context* c, const rt1w_temporal_params* p, const double* cur_frame, const double* cur_aov, const rt1w_camera* cur_cam,
                             const double* prev_hist, const double* prev_len, const double* prev_aov, const rt1w_camera* prev_cam, double* hist,
                             double* len, double* frame_out, rt1w_stats* stats) {
    return temporal_accumulate(c, p, cur_frame, cur_aov, cur_cam, prev_hist, prev_len, prev_aov, prev_cam, hist, len, frame_out, true, stats);
}
int rt1w_temporal_accumulate_device(rt1w_context* c, const rt1w_temporal_params* p, const void* d_cur_frame, const void* d_cur_aov,
                                    const rt1w_camera* cur_cam, const void* d_prev_hist, const void* d_prev_len, const void* d_prev_aov,
                                    const rt1w_camera* prev_cam, void* d_hist, void* d_len, void* d_frame_out, rt1w_stats* stats) {
    return temporal_accumulate(c, p, (const double*)d_cur_frame, (const double*)d_cur_aov, cur_cam, (const double*)d_prev_hist, (const double*)d_prev_len,
                               (const double*)d_prev_aov, prev_cam, (double*)d_hist, (double*)d_len, (double*)d_frame_out, false, stats);
}
int rt1w_render_temporal(rt1w_context* c, const rt1w_render_params* p, const rt1w_temporal_params* t, const rt1w_denoise_params* d, double* out_rgb,
                         rt1w_stats* stats) {
    return render_temporal(c, p, t, d, out_rgb, stats);
}
int rt1w_temporal_reset(rt1w_context* c) {
    if (!c) { set_error("null argument"); return RT1W_ERR_INVALID; }
    c->tm_valid = false;
    c->tv_valid = false;
    return RT1W_OK;
}
int rt1w_temporal_moments(rt1w_context* c, const rt1w_temporal_params* p, const double* cur_frame, const double* cur_aov, const rt1w_camera* cur_cam,
                          const double* prev_hist, const double* prev_m2, const double* prev_len, const double* prev_aov, const rt1w_camera* prev_cam,
                          double* hist, double* m2, double* len, double* frame_out, rt1w_stats* stats) {
    return temporal_moments(c, p, cur_frame, cur_aov, cur_cam, prev_hist, prev_m2, prev_len, prev_aov, prev_cam, hist, m2, len, frame_out, true, stats);
}
int rt1w_temporal_moments_device(rt1w_context* c, const rt1w_temporal_params* p, const void* d_cur_frame, const void* d_cur_aov, const rt1w_camera* cur_cam,
                                 const void* d_prev_hist, const void* d_prev_m2, const void* d_prev_len, const void* d_prev_aov,
                                 const rt1w_camera* prev_cam, void* d_hist, void* d_m2, void* d_len, void* d_frame_out, rt1w_stats* stats) {
    return temporal_moments(c, p, (const double*)d_cur_frame, (const double*)d_cur_aov, cur_cam, (const double*)d_prev_hist, (const double*)d_prev_m2,
                            (const double*)d_prev_len, (const double*)d_prev_aov, prev_cam, (double*)d_hist, (double*)d_m2, (double*)d_len,
                            (double*)d_frame_out, false, stats);
}
int rt1w_temporal_variance(rt1w_context* c, uint32_t width, uint32_t height, const double* hist, const double* m2, const double* len, const double* aov,
                           double* var, rt1w_stats* stats) {
    return temporal_variance(c, width, height, hist, m2, len, aov, var, true, stats);
}
int rt1w_temporal_variance_device(rt1w_context* c, uint32_t width, uint32_t height, const void* d_hist, const void* d_m2, const void* d_len,
                                  const void* d_aov, void* d_var, rt1w_stats* stats) {
    return temporal_variance(c, width, height, (const double*)d_hist, (const double*)d_m2, (const double*)d_len, (const double*)d_aov, (double*)d_var, false,
                             stats);
}
int rt1w_render_temporal_var(rt1w_context* c, const rt1w_render_params* p, const rt1w_temporal_params* t, const rt1w_denoise_params* d,
                             double sigma_variance, double* out_rgb, rt1w_stats* stats) {
    return render_temporal_var(c, p, t, d, sigma_variance, out_rgb, stats);
}
int rt1w_render_aov(rt1w_context* c, const rt1w_render_params* p, double* out_aov, rt1w_stats* stats) { return render_aov(c, p, nullptr, out_aov, true, stats); }
int rt1w_render_aov_device(rt1w_context* c, const rt1w_render_params* p, void* d_out_aov, rt1w_stats* stats) { return render_aov(c, p, nullptr, d_out_aov, false, stats); }
int rt1w_render_aov_deep(rt1w_context* c, const rt1w_render_params* p, uint32_t max_specular, double max_fuzz, double* out_aov, rt1w_stats* stats) {
    const AovDeep deep{max_specular, max_fuzz};
    return render_aov(c, p, &deep, out_aov, true, stats);
}
int rt1w_render_aov_deep_device(rt1w_context* c, const rt1w_render_params* p, uint32_t max_specular, double max_fuzz, void* d_out_aov, rt1w_stats* stats) {
    const AovDeep deep{max_specular, max_fuzz};
    return render_aov(c, p, &deep, d_out_aov, false, stats);
}
int rt1w_hit(rt1w_context* c, const rt1w_hit_params* p, const double* rays, double* out, uint32_t* out_node, rt1w_stats* stats) { return hit(c, p, rays, out, out_node, true, stats); }
int rt1w_hit_device(rt1w_context* c, const rt1w_hit_params* p, const void* d_rays, void* d_out, void* d_out_node, rt1w_stats* stats) { return hit(c, p, d_rays, d_out, d_out_node, false, stats); }
int rt1w_ray_color(rt1w_context* c, const rt1w_ray_color_params* p, const double* rays, const uint32_t* start_word, double* out, rt1w_stats* stats) { return ray_color(c, p, rays, start_word, out, true, stats); }
int rt1w_ray_color_device(rt1w_context* c, const rt1w_ray_color_params* p, const void* d_rays, const void* d_start_word, void* d_out, rt1w_stats* stats) { return ray_color(c, p, d_rays, d_start_word, d_out, false, stats); }
int rt1w_path_step(rt1w_context* c, const rt1w_path_params* p, const rt1w_path_state* in, rt1w_path_state* out, uint32_t* out_node, rt1w_stats* stats) { return path_step(c, p, in, out, out_node, true, stats); }
int rt1w_path_step_device(rt1w_context* c, const rt1w_path_params* p, const void* d_in, void* d_out, void* d_out_node, rt1w_stats* stats) { return path_step(c, p, d_in, d_out, d_out_node, false, stats); }
int rt1w_path_begin(rt1w_context* c, uint32_t width, uint32_t height, uint64_t global_seed, uint32_t max_depth, const uint32_t* pixels, uint64_t n, rt1w_path_state* out, rt1w_stats* stats) {
    return path_begin(c, width, height, global_seed, max_depth, pixels, n, out, true, stats);
}
int rt1w_path_begin_device(rt1w_context* c, uint32_t width, uint32_t height, uint64_t global_seed, uint32_t max_depth, const void* d_pixels, uint64_t n, void* d_out, rt1w_stats* stats) {
    return path_begin(c, width, height, global_seed, max_depth, d_pixels, n, d_out, false, stats);
}
int rt1w_denoise(rt1w_context* c, const rt1w_denoise_params* p, const double* frame, const double* aov, double* out, rt1w_stats* stats) { return denoise(c, p, frame, aov, out, true, stats); }
int rt1w_denoise_device(rt1w_context* c, const rt1w_denoise_params* p, const void* d_frame, const void* d_aov, void* d_out, rt1w_stats* stats) {
    return denoise(c, p, (const double*)d_frame, (const double*)d_aov, (double*)d_out, false, stats);
}
int rt1w_render_denoised(rt1w_context* c, const rt1w_render_params* p, const rt1w_denoise_params* d, double* out_rgb, rt1w_stats* stats) { return render_denoised(c, p, d, nullptr, out_rgb, stats); }
int rt1w_render_denoised_deep(rt1w_context* c, const rt1w_render_params* p, const rt1w_denoise_params* d, uint32_t max_specular, double max_fuzz,
                              double* out_rgb, rt1w_stats* stats) {
    const AovDeep deep{max_specular, max_fuzz};
    return render_denoised(c, p, d, &deep, out_rgb, stats);
}
int rt1w_batch_variance(rt1w_context* c, uint32_t width, uint32_t height, uint32_t batches, uint32_t batch_spp, uint32_t flags, const double* sums,
                        const double* aov, double* frame, double* var, rt1w_stats* stats) {
    return batch_variance(c, width, height, batches, batch_spp, flags, sums, aov, frame, var, true, stats);
}
int rt1w_batch_variance_device(rt1w_context* c, uint32_t width, uint32_t height, uint32_t batches, uint32_t batch_spp, uint32_t flags, const void* d_sums,
                               const void* d_aov, void* d_frame, void* d_var, rt1w_stats* stats) {
    return batch_variance(c, width, height, batches, batch_spp, flags, (const double*)d_sums, (const double*)d_aov, (double*)d_frame, (double*)d_var, false, stats);
}
int rt1w_denoise_var(rt1w_context* c, const rt1w_denoise_params* p, const double* frame, const double* aov, const double* var, double sigma_variance,
                     double* out, rt1w_stats* stats) {
    return denoise_var(c, p, frame, aov, var, sigma_variance, out, true, stats);
}
int rt1w_denoise_var_device(rt1w_context* c, const rt1w_denoise_params* p, const void* d_frame, const void* d_aov, const void* d_var,
                            double sigma_variance, void* d_out, rt1w_stats* stats) {
    return denoise_var(c, p, (const double*)d_frame, (const double*)d_aov, (const double*)d_var, sigma_variance, (double*)d_out, false, stats);
}
int rt1w_render_denoised_var(rt1w_context* c, const rt1w_render_params* p, const rt1w_denoise_params* d, uint32_t batches, double sigma_variance,
                             uint32_t max_specular, double max_fuzz, double* out_rgb, rt1w_stats* stats) {
    const AovDeep deep{max_specular, max_fuzz};
    return render_denoised_var(c, p, d, batches, sigma_variance, deep, out_rgb, stats);
}
int rt1w_accum_merge(rt1w_context* c, uint32_t width, uint32_t height, uint32_t x0, uint32_t y0, uint32_t tile_w, uint32_t tile_h, uint32_t batch_spp,
                     uint32_t flags, const double* tile_sums, const double* aov, double* acc, rt1w_stats* stats) {
    return accum_merge(c, width, height, x0, y0, tile_w, tile_h, batch_spp, flags, tile_sums, aov, acc, true, stats);
}
int rt1w_accum_merge_device(rt1w_context* c, uint32_t width, uint32_t height, uint32_t x0, uint32_t y0, uint32_t tile_w, uint32_t tile_h,
                            uint32_t batch_spp, uint32_t flags, const void* d_tile_sums, const void* d_aov, void* d_acc, rt1w_stats* stats) {
    return accum_merge(c, width, height, x0, y0, tile_w, tile_h, batch_spp, flags, (const double*)d_tile_sums, (const double*)d_aov, (double*)d_acc, false, stats);
}
int rt1w_accum_merge_tiles(rt1w_context* c, uint32_t width, uint32_t height, uint32_t tile, const rt1w_tile* tiles, uint32_t n_tiles, uint32_t batch_spp,
                           uint32_t flags, const double* tile_sums, const double* aov, double* acc, rt1w_stats* stats) {
    return accum_merge_tiles(c, width, height, tile, tiles, n_tiles, batch_spp, flags, tile_sums, aov, acc, true, stats);
}
int rt1w_accum_merge_tiles_device(rt1w_context* c, uint32_t width, uint32_t height, uint32_t tile, const rt1w_tile* tiles, uint32_t n_tiles,
                                  uint32_t batch_spp, uint32_t flags, const void* d_tile_sums, const void* d_aov, void* d_acc, rt1w_stats* stats) {
    return accum_merge_tiles(c, width, height, tile, tiles, n_tiles, batch_spp, flags, (const double*)d_tile_sums, (const double*)d_aov, (double*)d_acc, false, stats);
}
int rt1w_accum_resolve(rt1w_context* c, uint32_t width, uint32_t height, uint32_t batch_spp, const double* acc, double* frame, double* var,
                       double* spp, rt1w_stats* stats) {
    return accum_resolve(c, width, height, batch_spp, acc, frame, var, spp, true, stats);
}
int rt1w_accum_resolve_device(rt1w_context* c, uint32_t width, uint32_t height, uint32_t batch_spp, const void* d_acc, void* d_frame, void* d_var,
                              void* d_spp, rt1w_stats* stats) {
    return accum_resolve(c, width, height, batch_spp, (const double*)d_acc, (double*)d_frame, (double*)d_var, (double*)d_spp, false, stats);
}
int rt1w_accum_tile_error(rt1w_context* c, uint32_t width, uint32_t height, uint32_t tile, const double* acc, double* err, rt1w_stats* stats) {
    return accum_tile_error(c, width, height, tile, acc, err, true, stats);
}
int rt1w_accum_tile_error_device(rt1w_context* c, uint32_t width, uint32_t height, uint32_t tile, const void* d_acc, void* d_err, rt1w_stats* stats) {
    return accum_tile_error(c, width, height, tile, (const double*)d_acc, (double*)d_err, false, stats);
}
int rt1w_adaptive_select(const rt1w_adaptive_params* params, uint32_t n_tiles_x, uint32_t n_tiles_y, uint32_t width, uint32_t height, const double* err,
                         const uint32_t* m_per_tile, uint32_t* out_tiles, uint32_t capacity) {
    RtAdPlan plan;
    if (const char* why = rt_ad_make_plan(params, &plan)) { set_error(why); return RT1W_ERR_INVALID; }
    if (!rt_ad_frame_ok(width, height) || n_tiles_x != (width + plan.tile - 1u) / plan.tile || n_tiles_y != (height + plan.tile - 1u) / plan.tile) {
        set_error("adaptive select: n_tiles_x / n_tiles_y must be ceil(width / tile), ceil(height / tile)"); return RT1W_ERR_INVALID;
    }
    if (!err || !m_per_tile || (!out_tiles && capacity)) { set_error("null buffer"); return RT1W_ERR_INVALID; }
    const std::vector<uint32_t> taken = rt_ad_select(plan, n_tiles_x, n_tiles_y, width, height, err, m_per_tile);
    for (size_t i = 0; i < taken.size() && i < capacity; ++i) out_tiles[i] = taken[i];
    return (int)taken.size();
}
int rt1w_render_adaptive(rt1w_context* c, const rt1w_render_params* p, const rt1w_adaptive_params* a, const rt1w_denoise_params* d, double sigma_variance,
                         double* out_rgb, double* out_spp, rt1w_stats* stats) {
    return render_adaptive(c, p, a, d, sigma_variance, out_rgb, out_spp, stats);
}
int rt1w_halves_resolve(rt1w_context* c, uint32_t width, uint32_t height, uint32_t batch_spp, const double* acc_a, const double* acc_b, double* frame,
                        double* var, double* half_a, double* half_b, double* spp, rt1w_stats* stats) {
    return halves_resolve(c, width, height, batch_spp, acc_a, acc_b, frame, var, half_a, half_b, spp, true, stats);
}
int rt1w_halves_resolve_device(rt1w_context* c, uint32_t width, uint32_t height, uint32_t batch_spp, const void* d_acc_a, const void* d_acc_b, void* d_frame,
                               void* d_var, void* d_half_a, void* d_half_b, void* d_spp, rt1w_stats* stats) {
    return halves_resolve(c, width, height, batch_spp, (const double*)d_acc_a, (const double*)d_acc_b, (double*)d_frame, (double*)d_var, (double*)d_half_a,
                          (double*)d_half_b, (double*)d_spp, false, stats);
}
int rt1w_denoise_var_halves(rt1w_context* c, const rt1w_denoise_params* p, const double* frame, const double* aov, const double* var, const double* half_a,
                            const double* half_b, double sigma_variance, double* out, double* err_px, rt1w_stats* stats) {
    return denoise_var_halves(c, p, frame, aov, var, half_a, half_b, sigma_variance, out, err_px, halves_filter, true, stats);
}
int rt1w_denoise_var_halves_device(rt1w_context* c, const rt1w_denoise_params* p, const void* d_frame, const void* d_aov, const void* d_var,
                                   const void* d_half_a, const void* d_half_b, double sigma_variance, void* d_out, void* d_err_px, rt1w_stats* stats) {
    return denoise_var_halves(c, p, (const double*)d_frame, (const double*)d_aov, (const double*)d_var, (const double*)d_half_a, (const double*)d_half_b,
                              sigma_variance, (double*)d_out, (double*)d_err_px, halves_filter, false, stats);
}
int rt1w_tile_error_map(rt1w_context* c, uint32_t width, uint32_t height, uint32_t tile, const double* err_px, double* err, rt1w_stats* stats) {
    return tile_error_map(c, width, height, tile, err_px, err, true, stats);
}
int rt1w_tile_error_map_device(rt1w_context* c, uint32_t width, uint32_t height, uint32_t tile, const void* d_err_px, void* d_err, rt1w_stats* stats) {
    return tile_error_map(c, width, height, tile, (const double*)d_err_px, (double*)d_err, false, stats);
}
int rt1w_render_adaptive_filtered(rt1w_context* c, const rt1w_render_params* p, const rt1w_adaptive_params* a, const rt1w_denoise_params* d,
                                  double sigma_variance, double* out_rgb, double* out_spp, double* out_err, rt1w_stats* stats) {
    return render_adaptive_filtered(c, p, a, d, sigma_variance, out_rgb, out_spp, out_err, halves_filter, false, "rt1w_render_adaptive_filtered", stats);
}
int rt1w_denoise_cross(rt1w_context* c, const rt1w_denoise_params* p, const double* frame, const double* aov, const double* var, const double* half_a,
                       const double* half_b, double sigma_variance, double* out, double* err_px, rt1w_stats* stats) {
    return denoise_var_halves(c, p, frame, aov, var, half_a, half_b, sigma_variance, out, err_px, cross_filter, true, stats);
}
int rt1w_denoise_cross_device(rt1w_context* c, const rt1w_denoise_params* p, const void* d_frame, const void* d_aov, const void* d_var, const void* d_half_a,
                              const void* d_half_b, double sigma_variance, void* d_out, void* d_err_px, rt1w_stats* stats) {
    return denoise_var_halves(c, p, (const double*)d_frame, (const double*)d_aov, (const double*)d_var, (const double*)d_half_a, (const double*)d_half_b,
                              sigma_variance, (double*)d_out, (double*)d_err_px, cross_filter, false, stats);
}
int rt1w_render_adaptive_cross(rt1w_context* c, const rt1w_render_params* p, const rt1w_adaptive_params* a, const rt1w_denoise_params* d,
                               double sigma_variance, double* out_rgb, double* out_spp, double* out_err, rt1w_stats* stats) {
    return render_adaptive_filtered(c, p, a, d, sigma_variance, out_rgb, out_spp, out_err, cross_filter, false, "rt1w_render_adaptive_cross", stats);
}
int rt1w_render_aov_tiles(rt1w_context* c, const rt1w_render_params* p, uint32_t tile, const rt1w_tile* tiles, uint32_t n_tiles, double* out, rt1w_stats* stats) {
    return render_aov_tiles(c, p, tile, tiles, n_tiles, out, true, stats);
}
int rt1w_render_aov_tiles_device(rt1w_context* c, const rt1w_render_params* p, uint32_t tile, const rt1w_tile* tiles, uint32_t n_tiles, void* d_out,
                                 rt1w_stats* stats) {
    return render_aov_tiles(c, p, tile, tiles, n_tiles, d_out, false, stats);
}
int rt1w_guides_merge_tiles(rt1w_context* c, uint32_t width, uint32_t height, uint32_t tile, const rt1w_tile* tiles, uint32_t n_tiles, uint32_t spp,
                            const double* tile_sums, double* gacc, rt1w_stats* stats) {
    return guides_merge_tiles(c, width, height, tile, tiles, n_tiles, spp, tile_sums, gacc, true, stats);
}
int rt1w_guides_merge_tiles_device(rt1w_context* c, uint32_t width, uint32_t height, uint32_t tile, const rt1w_tile* tiles, uint32_t n_tiles, uint32_t spp,
                                   const void* d_tile_sums, void* d_gacc, rt1w_stats* stats) {
    return guides_merge_tiles(c, width, height, tile, tiles, n_tiles, spp, (const double*)d_tile_sums, (double*)d_gacc, false, stats);
}
int rt1w_guides_resolve(rt1w_context* c, uint32_t width, uint32_t height, const double* gacc, double* aov, rt1w_stats* stats) {
    return guides_resolve(c, width, height, gacc, aov, true, stats);
}
int rt1w_guides_resolve_device(rt1w_context* c, uint32_t width, uint32_t height, const void* d_gacc, void* d_aov, rt1w_stats* stats) {
    return guides_resolve(c, width, height, (const double*)d_gacc, (double*)d_aov, false, stats);
}
int rt1w_render_adaptive_guided(rt1w_context* c, const rt1w_render_params* p, const rt1w_adaptive_params* a, const rt1w_denoise_params* d,
                                double sigma_variance, double* out_rgb, double* out_spp, double* out_err, rt1w_stats* stats) {
    return render_adaptive_filtered(c, p, a, d, sigma_variance, out_rgb, out_spp, out_err, halves_filter, true, "rt1w_render_adaptive_guided", stats);
}
} /* extern "C" */
