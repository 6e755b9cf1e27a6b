/* features.hip -- the entries of the feature buffers and the denoiser (include/rt1w.h: rt1w_render_aov*, rt1w_denoise*,
 * rt1w_render_denoised*, rt1w_batch_variance*, rt1w_accum_*, rt1w_render_adaptive): validation, buffers, launch, timing, copies.  Host code only, built without a device pass: the
 * kernels belong to aov.hip, denoise.hip, denoise_var.hip and adaptive.hip and are launched through their host handles, the context and its render path to context.hip (context.h), so a
 * change here rebuilds none of the code objects. */
#include <cstdio>
#include <cstring>

#include "context.h"
#include "rt_aov_deep.h" /* rt_aov_deep_args_ok only */
#include "rt_denoise_var.h" /* rt_dv_batches_ok, rt_dv_sigma, rt_dv_split only */
#include "rt_adaptive_plan.h" /* the plan of rt1w_render_adaptive and rt1w_adaptive_select; rt_ad_*_ok of rt_adaptive.h */

/* aov.hip: the first-hit feature buffers (rt1w_render_aov), by variant; workgroups of RT_BLOCK work-items that cover the frame's tile */
extern "C" const void* rt1w_internal_aov_kernel(int variant);
extern "C" const void* rt1w_internal_aov_deep_kernel(int variant); /* rt1w_render_aov_deep: + (max_specular, max_fuzz) before out, a segment counter after */
extern "C" unsigned rt1w_internal_aov_grid(const void* frame);
extern "C" unsigned rt1w_internal_aov_sizeof(int what);
/* denoise.hip: the filter of rt1w_denoise; enqueues the prepare pass and the levels; 0, -1 launch failure, -2 parameters refused */
extern "C" int rt1w_internal_denoise_launch(uint32_t w, uint32_t h, uint32_t iterations, uint32_t flags, double sigma_colour, double sigma_normal,
                                            double sigma_depth, const double* frame, const double* aov, double* out, void* col_a, void* col_b,
                                            void* guide, hipStream_t stream, unsigned launch[2]);
extern "C" unsigned rt1w_internal_denoise_sizeof(int what); /* bytes per pixel of 0 a colour buffer, 1 the guide buffer */
/* denoise_var.hip: the batch-variance pass and the variance-guided filter; returns as rt1w_internal_denoise_launch */
extern "C" int rt1w_internal_batch_variance_launch(uint32_t w, uint32_t h, uint32_t batches, uint32_t batch_spp, uint32_t flags, const double* sums,
                                                   const double* aov, double* frame, double* var, hipStream_t stream, unsigned launch[2]);
extern "C" int rt1w_internal_denoise_var_launch(uint32_t w, uint32_t h, uint32_t iterations, uint32_t flags, double sigma_normal, double sigma_depth,
                                                double sigma_variance, const double* frame, const double* aov, const double* var, double* out,
                                                void* col_a, void* col_b, void* guide, hipStream_t stream, unsigned launch[2]);
extern "C" unsigned rt1w_internal_denoise_var_sizeof(void); /* bytes per pixel of one of its colour buffers */
/* adaptive.hip: the accumulator kernels; returns as rt1w_internal_denoise_launch */
extern "C" int rt1w_internal_accum_merge_launch(uint32_t w, uint32_t h, uint32_t x0, uint32_t y0, uint32_t tw, uint32_t th, uint32_t batch_spp,
                                                uint32_t flags, const double* sums, const double* aov, double* acc, hipStream_t stream,
                                                unsigned launch[2]);
extern "C" int rt1w_internal_accum_merge_tiles_launch(uint32_t w, uint32_t h, uint32_t tile, const uint32_t* rec, uint32_t n, uint32_t batch_spp, uint32_t flags,
                                                      const double* sums, const double* aov, double* acc, hipStream_t stream, unsigned launch[2]);
extern "C" int rt1w_internal_accum_resolve_launch(uint32_t w, uint32_t h, uint32_t batch_spp, const double* acc, double* frame, double* var,
                                                  double* spp, hipStream_t stream, unsigned launch[2]);
extern "C" int rt1w_internal_accum_tile_error_launch(uint32_t w, uint32_t h, uint32_t tile, const double* acc, double* err, hipStream_t stream,
                                                     unsigned launch[2]);

using namespace rt1w;
namespace {

/* ---- first-hit and deep feature buffers (include/rt1w.h: rt1w_render_aov, rt1w_render_aov_deep) ---- */
/* the render flags by name, in the order the refusals look for them; `denoised`: one rt1w_render_denoised refuses too */
const struct { uint32_t bit; const char* name; bool denoised; } g_flags[] = {
    {RT1W_OUT_SUM, "RT1W_OUT_SUM", true}, {RT1W_UNSORTED, "RT1W_UNSORTED", false}, {RT1W_LDS_NODES, "RT1W_LDS_NODES", false},
    {RT1W_GENERIC, "RT1W_GENERIC", false}, {RT1W_WAVEFRONT, "RT1W_WAVEFRONT", false}, {RT1W_OUT_FRAME, "RT1W_OUT_FRAME", true},
    {RT1W_RNG_REFERENCE, "RT1W_RNG_REFERENCE", true}, {RT1W_CLASSIC_WALK, "RT1W_CLASSIC_WALK", false},
    {RT1W_NO_NODE_CACHE, "RT1W_NO_NODE_CACHE", false}, {RT1W_PROBE_COHERENT, "RT1W_PROBE_COHERENT", true}};
/* refuses the first flag of `flags` that has a name (denoised_only: and that rt1w_render_denoised refuses), as "<name><tail>" */
int refuse_named_flag(uint32_t flags, bool denoised_only, const char* tail) {
    for (const auto& k : g_flags)
        if ((flags & k.bit) && (k.denoised || !denoised_only)) { set_error(std::string(k.name) + tail); return RT1W_ERR_INVALID; }
    return RT1W_OK;
}
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
/* launch the AOV kernel of the context's (or the forced) variant into d_out, wait, fill stats */
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
    const void* fn = deep ? rt1w_internal_aov_deep_kernel(variant) : rt1w_internal_aov_kernel(variant);
    if (!fn) { set_error("no AOV kernel of this variant"); return RT1W_ERR_DEVICE; }
    const unsigned grid = rt1w_internal_aov_grid(&f);
    /* (view, frame, out), the deep kernel's (view, frame, max_specular, max_fuzz, out, rays traced): the lane's second counter, the
     * one the render kernels count their segments in */
    AovDeep dv = deep ? *deep : AovDeep{0u, 0.0};
    unsigned long long* d_rays = l.d_counters + 1;
    void* args_first[] = {&c->view, &f, &d_out};
    void* args_deep[] = {&c->view, &f, &dv.max_specular, &dv.max_fuzz, &d_out, &d_rays};
    if (deep && !hip_ok(hipMemsetAsync(d_rays, 0, sizeof *d_rays, l.stream), "AOV counter")) return RT1W_ERR_DEVICE;
    (void)hipEventRecord(l.ev0, l.stream);
    if (!hip_ok(hipLaunchKernel(fn, dim3(grid), dim3(RT_BLOCK), deep ? args_deep : args_first, 0, l.stream), "AOV kernel launch")) return RT1W_ERR_DEVICE;
    (void)hipEventRecord(l.ev1, l.stream);
    if (deep && !hip_ok(hipMemcpyAsync(l.h_counters + 1, d_rays, sizeof *d_rays, hipMemcpyDeviceToHost, l.stream), "AOV counter copy")) return RT1W_ERR_DEVICE;
    if (!hip_ok(hipStreamSynchronize(l.stream), "AOV kernel")) return RT1W_ERR_DEVICE;
    if (stats) {
        memset(stats, 0, sizeof *stats);
        stats->paths = (uint64_t)p->tile_w * p->tile_h * p->spp;
        stats->segments = deep ? l.h_counters[1] : stats->paths; /* first hit: one camera ray per sample */
        stats->kernel_ms = lane_ms(l);
        stats->chunk = p->spp; stats->n_chunks = 1u;
        stats->grid = grid; stats->block = RT_BLOCK;
        stats->variant = (uint32_t)variant; stats->passes = 1u;
    }
    return RT1W_OK;
}
/* the four AOV entries.  `out` is device memory, or (host) host memory, filled through the context's framebuffer as rt1w_render grows it */
int render_aov(rt1w_context* c, const rt1w_render_params* p, const AovDeep* deep, void* out, bool host, rt1w_stats* stats) {
    int rc = aov_deep_validate(deep); /* first: needs no context */
    if (rc < 0) return rc;
    if ((rc = validate(c, p)) < 0) return rc;
    if (!out) { set_error("null output"); return RT1W_ERR_INVALID; }
    if ((rc = aov_check_flags(p->flags)) < 0) return rc;
    if (p->precision != RT1W_PRECISION_F64) { set_error("the AOV entries are f64 only (RT1W_PRECISION_F64)"); return RT1W_ERR_UNSUPPORTED; }
    if (!hip_ok(hipSetDevice(c->device), "hipSetDevice")) return RT1W_ERR_DEVICE;
    const RtTimer timer;
    const size_t bytes = (size_t)p->tile_w * p->tile_h * RT1W_AOV_CHANNELS * sizeof(double);
    if (host && (rc = reserve_out(c, bytes)) < 0) return rc;
    double* d_out = host ? c->d_out : (double*)out;
    if ((rc = render_aov_common(c, p, deep, d_out, stats)) < 0) return rc;
    if (host && !hip_ok(hipMemcpy(out, d_out, bytes, hipMemcpyDeviceToHost), "AOV copy")) return RT1W_ERR_DEVICE;
    if (stats) stats->total_ms = timer.ms();
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
        const size_t bytes = npix * (k == 2 ? rt1w_internal_denoise_sizeof(1) : col_bytes);
        if (bytes <= c->dn_bytes[k]) continue;
        if (c->dn_buf[k]) (void)hipFree(c->dn_buf[k]);
        c->dn_buf[k] = nullptr; c->dn_bytes[k] = 0;
        if (!hip_ok(hipMalloc(&c->dn_buf[k], bytes), "hipMalloc(denoise buffers)")) return RT1W_ERR_NOMEM;
        c->dn_bytes[k] = bytes;
    }
    return RT1W_OK;
}
/* prepare pass and levels on lane 0's stream, wait; *stats but for total_ms: their HIP-event time, grid / block of the level kernel */
int denoise_common(rt1w_context* c, const rt1w_denoise_params* p, const double* d_frame, const double* d_aov, double* d_out, rt1w_stats* stats) {
    int rc = denoise_reserve(c, (size_t)p->width * p->height, rt1w_internal_denoise_sizeof(0));
    if (rc < 0) return rc;
    RtLane& l = c->lane[0];
    unsigned launch[2] = {0u, 0u};
    (void)hipEventRecord(l.ev0, l.stream);
    rc = rt1w_internal_denoise_launch(p->width, p->height, p->iterations, p->flags, p->sigma_colour, p->sigma_normal, p->sigma_depth, d_frame, d_aov,
                                      d_out, c->dn_buf[0], c->dn_buf[1], c->dn_buf[2], l.stream, launch);
    if (rc == -2) { set_error("denoise: parameters refused"); return RT1W_ERR_INVALID; }
    if (rc != 0) { set_error("denoise kernel launch failed"); return RT1W_ERR_DEVICE; }
    (void)hipEventRecord(l.ev1, l.stream);
    if (!hip_ok(hipStreamSynchronize(l.stream), "denoise kernels")) return RT1W_ERR_DEVICE;
    memset(stats, 0, sizeof *stats);
    stats->paths = (uint64_t)p->width * p->height; stats->kernel_ms = lane_ms(l);
    stats->grid = launch[0]; stats->block = launch[1]; stats->passes = 1u;
    return RT1W_OK;
}
/* the two denoise entries.  The buffers are device memory, or (host) host memory: the context's framebuffer then holds the frame
 * (filtered in place) and, behind it, the feature buffers */
int denoise(rt1w_context* c, const rt1w_denoise_params* p, const double* frame, const double* aov, double* out, bool host, rt1w_stats* stats) {
    int rc = denoise_validate(c, p);
    if (rc < 0) return rc;
    if (!frame || !aov || !out) { set_error("null buffer"); return RT1W_ERR_INVALID; }
    if (!hip_ok(hipSetDevice(c->device), "hipSetDevice")) return RT1W_ERR_DEVICE;
    const RtTimer timer;
    const size_t npix = (size_t)p->width * p->height;
    const double *d_frame = frame, *d_aov = aov;
    double* d_out = out;
    if (host) {
        if ((rc = reserve_out(c, npix * (3 + RT1W_AOV_CHANNELS) * sizeof(double))) < 0) return rc;
        d_frame = d_out = c->d_out;
        d_aov = c->d_out + npix * 3;
        if (!hip_ok(hipMemcpy(d_out, frame, npix * 3 * sizeof(double), hipMemcpyHostToDevice), "denoise: frame copy")) return RT1W_ERR_DEVICE;
        if (!hip_ok(hipMemcpy(d_out + npix * 3, aov, npix * RT1W_AOV_CHANNELS * sizeof(double), hipMemcpyHostToDevice), "denoise: feature buffer copy")) return RT1W_ERR_DEVICE;
    }
    rt1w_stats st;
    if ((rc = denoise_common(c, p, d_frame, d_aov, d_out, &st)) < 0) return rc;
    if (host && !hip_ok(hipMemcpy(out, d_out, npix * 3 * sizeof(double), hipMemcpyDeviceToHost), "denoise: result copy")) return RT1W_ERR_DEVICE;
    if (stats) { *stats = st; stats->total_ms = timer.ms(); }
    return RT1W_OK;
}
/* rt1w_render_denoised and, with `deep`, rt1w_render_denoised_deep */
int render_denoised(rt1w_context* c, const rt1w_render_params* p, const rt1w_denoise_params* d, const AovDeep* deep, double* out_rgb, rt1w_stats* stats) {
    int rc = aov_deep_validate(deep);
    if (rc < 0) return rc;
    if ((rc = validate(c, p)) < 0) return rc;
    if (!out_rgb) { set_error("null output"); return RT1W_ERR_INVALID; }
    if ((rc = refuse_named_flag(p->flags, true, " does not apply to rt1w_render_denoised")) < 0) return rc;
    if (p->strip_rows) { set_error("rt1w_render_denoised takes a contiguous tile (strip_rows must be 0): denoise the gathered frame with rt1w_denoise"); return RT1W_ERR_INVALID; }
    if (p->precision != RT1W_PRECISION_F64) { set_error("RT1W_PRECISION_F32 does not apply to rt1w_render_denoised (the filter is f64 only)"); return RT1W_ERR_INVALID; }
    rt1w_denoise_params dp;
    memset(&dp, 0, sizeof dp);
    if (d) dp = *d;
    if ((dp.width && dp.width != p->tile_w) || (dp.height && dp.height != p->tile_h)) { set_error("denoise: width / height must be 0 or the tile's"); return RT1W_ERR_INVALID; }
    dp.width = p->tile_w; dp.height = p->tile_h;
    if ((rc = denoise_validate(c, &dp)) < 0) return rc;
    if (!hip_ok(hipSetDevice(c->device), "hipSetDevice")) return RT1W_ERR_DEVICE;
    const RtTimer timer;
    const size_t npix = (size_t)p->tile_w * p->tile_h;
    if ((rc = reserve_out(c, npix * (3 + RT1W_AOV_CHANNELS) * sizeof(double))) < 0) return rc;
    double* d_frame = c->d_out;
    double* d_aov = c->d_out + npix * 3;
    rt1w_stats st;
    memset(&st, 0, sizeof st);
    if ((rc = render_common(c, p, d_frame, &st)) < 0) return rc;
    rt1w_render_params ap = *p; /* the feature buffers of the same tile, samples and seed, by the scene's own variant */
    ap.flags = 0u;
    rt1w_stats sa, sd;
    if ((rc = render_aov_common(c, &ap, deep, d_aov, &sa)) < 0) return rc;
    if ((rc = denoise_common(c, &dp, d_frame, d_aov, d_frame, &sd)) < 0) return rc;
    if (!hip_ok(hipMemcpy(out_rgb, d_frame, npix * 3 * sizeof(double), hipMemcpyDeviceToHost), "denoised frame copy")) return RT1W_ERR_DEVICE;
    if (stats) {
        *stats = st;
        stats->kernel_ms = st.kernel_ms + sa.kernel_ms + sd.kernel_ms;
        stats->grid = sd.grid; stats->block = sd.block;
        stats->total_ms = timer.ms();
    }
    return RT1W_OK;
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
/* the context's buffer of batch sums, grown to `bytes` */
int batches_reserve(rt1w_context* c, size_t bytes) {
    if (bytes <= c->batches_bytes) return RT1W_OK;
    if (c->d_batches) (void)hipFree(c->d_batches);
    c->d_batches = nullptr; c->batches_bytes = 0;
    if (!hip_ok(hipMalloc((void**)&c->d_batches, bytes), "hipMalloc(batch sums)")) return RT1W_ERR_NOMEM;
    c->batches_bytes = bytes;
    return RT1W_OK;
}
/* the two passes on lane 0's stream, wait; *stats as denoise_common fills them */
int lane_finish(rt1w_context* c, int rc, const unsigned launch[2], uint64_t npix, const char* what, rt1w_stats* stats) {
    RtLane& l = c->lane[0];
    if (rc == -2) { set_error(std::string(what) + ": parameters refused"); return RT1W_ERR_INVALID; }
    if (rc != 0) { set_error(std::string(what) + " kernel launch failed"); return RT1W_ERR_DEVICE; }
    (void)hipEventRecord(l.ev1, l.stream);
    if (!hip_ok(hipStreamSynchronize(l.stream), what)) return RT1W_ERR_DEVICE;
    memset(stats, 0, sizeof *stats);
    stats->paths = npix; stats->kernel_ms = lane_ms(l);
    stats->grid = launch[0]; stats->block = launch[1]; stats->passes = 1u;
    return RT1W_OK;
}
int batch_variance_common(rt1w_context* c, uint32_t w, uint32_t h, uint32_t batches, uint32_t batch_spp, uint32_t flags, const double* d_sums,
                          const double* d_aov, double* d_frame, double* d_var, rt1w_stats* stats) {
    RtLane& l = c->lane[0];
    unsigned launch[2] = {0u, 0u};
    (void)hipEventRecord(l.ev0, l.stream);
    const int rc = rt1w_internal_batch_variance_launch(w, h, batches, batch_spp, flags, d_sums, d_aov, d_frame, d_var, l.stream, launch);
    return lane_finish(c, rc, launch, (uint64_t)w * h, "batch variance", stats);
}
int denoise_var_common(rt1w_context* c, const rt1w_denoise_params* p, double sigma_variance, const double* d_frame, const double* d_aov,
                       const double* d_var, double* d_out, rt1w_stats* stats) {
    int rc = denoise_reserve(c, (size_t)p->width * p->height, rt1w_internal_denoise_var_sizeof());
    if (rc < 0) return rc;
    RtLane& l = c->lane[0];
    unsigned launch[2] = {0u, 0u};
    (void)hipEventRecord(l.ev0, l.stream);
    rc = rt1w_internal_denoise_var_launch(p->width, p->height, p->iterations, p->flags, p->sigma_normal, p->sigma_depth, sigma_variance, d_frame, d_aov,
                                          d_var, d_out, c->dn_buf[0], c->dn_buf[1], c->dn_buf[2], l.stream, launch);
    return lane_finish(c, rc, launch, (uint64_t)p->width * p->height, "denoise", stats);
}
/* the two batch-variance entries.  Device memory, or (host) host memory: the batch sums then go through the context's batch buffer and
 * the framebuffer holds frame, var and, behind them, the feature buffers */
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
    if (!hip_ok(hipSetDevice(c->device), "hipSetDevice")) return RT1W_ERR_DEVICE;
    const RtTimer timer;
    const size_t npix = (size_t)w * h;
    const double *d_sums = sums, *d_aov = aov;
    double *d_frame = frame, *d_var = var;
    if (host) {
        if ((rc = reserve_out(c, npix * (4 + RT1W_AOV_CHANNELS) * sizeof(double))) < 0) return rc;
        if ((rc = batches_reserve(c, npix * 3 * batches * sizeof(double))) < 0) return rc;
        d_frame = c->d_out; d_var = c->d_out + npix * 3;
        double* d_a = c->d_out + npix * 4;
        if (!hip_ok(hipMemcpy(c->d_batches, sums, npix * 3 * batches * sizeof(double), hipMemcpyHostToDevice), "batch variance: sums copy")) return RT1W_ERR_DEVICE;
        if (!hip_ok(hipMemcpy(d_a, aov, npix * RT1W_AOV_CHANNELS * sizeof(double), hipMemcpyHostToDevice), "batch variance: feature buffer copy")) return RT1W_ERR_DEVICE;
        d_sums = c->d_batches; d_aov = d_a;
    }
    rt1w_stats st;
    if ((rc = batch_variance_common(c, w, h, batches, batch_spp, flags, d_sums, d_aov, d_frame, d_var, &st)) < 0) return rc;
    if (host && !hip_ok(hipMemcpy(frame, d_frame, npix * 3 * sizeof(double), hipMemcpyDeviceToHost), "batch variance: frame copy")) return RT1W_ERR_DEVICE;
    if (host && !hip_ok(hipMemcpy(var, d_var, npix * sizeof(double), hipMemcpyDeviceToHost), "batch variance: variance copy")) return RT1W_ERR_DEVICE;
    if (stats) { *stats = st; stats->total_ms = timer.ms(); }
    return RT1W_OK;
}
/* the two rt1w_denoise_var entries: as denoise(), with the variance buffer behind the feature buffers */
int denoise_var(rt1w_context* c, const rt1w_denoise_params* p, const double* frame, const double* aov, const double* var, double sigma_variance,
                double* out, bool host, rt1w_stats* stats) {
    int rc = denoise_validate(c, p);
    if (rc < 0) return rc;
    if ((rc = sigma_variance_validate(sigma_variance)) < 0) return rc;
    if (!frame || !aov || !var || !out) { set_error("null buffer"); return RT1W_ERR_INVALID; }
    if (!hip_ok(hipSetDevice(c->device), "hipSetDevice")) return RT1W_ERR_DEVICE;
    const RtTimer timer;
    const size_t npix = (size_t)p->width * p->height;
    const double *d_frame = frame, *d_aov = aov, *d_var = var;
    double* d_out = out;
    if (host) {
        if ((rc = reserve_out(c, npix * (4 + RT1W_AOV_CHANNELS) * sizeof(double))) < 0) return rc;
        d_frame = d_out = c->d_out;
        d_var = c->d_out + npix * 3;
        d_aov = c->d_out + npix * 4;
        if (!hip_ok(hipMemcpy(d_out, frame, npix * 3 * sizeof(double), hipMemcpyHostToDevice), "denoise: frame copy")) return RT1W_ERR_DEVICE;
        if (!hip_ok(hipMemcpy(d_out + npix * 3, var, npix * sizeof(double), hipMemcpyHostToDevice), "denoise: variance copy")) return RT1W_ERR_DEVICE;
        if (!hip_ok(hipMemcpy(d_out + npix * 4, aov, npix * RT1W_AOV_CHANNELS * sizeof(double), hipMemcpyHostToDevice), "denoise: feature buffer copy")) return RT1W_ERR_DEVICE;
    }
    rt1w_stats st;
    if ((rc = denoise_var_common(c, p, sigma_variance, d_frame, d_aov, d_var, d_out, &st)) < 0) return rc;
    if (host && !hip_ok(hipMemcpy(out, d_out, npix * 3 * sizeof(double), hipMemcpyDeviceToHost), "denoise: result copy")) return RT1W_ERR_DEVICE;
    if (stats) { *stats = st; stats->total_ms = timer.ms(); }
    return RT1W_OK;
}
/* rt1w_render_denoised_var: the batches' sums into the context's batch buffer; frame, var and the deep feature buffers in the framebuffer */
int render_denoised_var(rt1w_context* c, const rt1w_render_params* p, const rt1w_denoise_params* d, uint32_t batches, double sigma_variance,
                        const AovDeep& deep, double* out_rgb, rt1w_stats* stats) {
    int rc = aov_deep_validate(&deep);
    if (rc < 0) return rc;
    if ((rc = sigma_variance_validate(sigma_variance)) < 0) return rc;
    if ((rc = validate(c, p)) < 0) return rc;
    if (!out_rgb) { set_error("null output"); return RT1W_ERR_INVALID; }
    if ((rc = refuse_named_flag(p->flags, true, " does not apply to rt1w_render_denoised")) < 0) return rc;
    if (p->strip_rows) { set_error("rt1w_render_denoised takes a contiguous tile (strip_rows must be 0): denoise the gathered frame with rt1w_denoise"); return RT1W_ERR_INVALID; }
    if (p->precision != RT1W_PRECISION_F64) { set_error("RT1W_PRECISION_F32 does not apply to rt1w_render_denoised (the filter is f64 only)"); return RT1W_ERR_INVALID; }
    uint32_t k = 0u, n = 0u;
    if (!rt_dv_split(p->spp, batches, k, n)) { set_error("rt1w_render_denoised_var: 2 .. 16 batches (0 = 4), and spp a multiple of their number"); return RT1W_ERR_INVALID; }
    rt1w_denoise_params dp;
    memset(&dp, 0, sizeof dp);
    if (d) dp = *d;
    if ((dp.width && dp.width != p->tile_w) || (dp.height && dp.height != p->tile_h)) { set_error("denoise: width / height must be 0 or the tile's"); return RT1W_ERR_INVALID; }
    dp.width = p->tile_w; dp.height = p->tile_h;
    if ((rc = denoise_validate(c, &dp)) < 0) return rc;
    if (!hip_ok(hipSetDevice(c->device), "hipSetDevice")) return RT1W_ERR_DEVICE;
    const RtTimer timer;
    const size_t npix = (size_t)p->tile_w * p->tile_h;
    if ((rc = reserve_out(c, npix * (4 + RT1W_AOV_CHANNELS) * sizeof(double))) < 0) return rc;
    if ((rc = batches_reserve(c, npix * 3 * k * sizeof(double))) < 0) return rc;
    double* d_frame = c->d_out;
    double* d_var = c->d_out + npix * 3;
    double* d_aov = c->d_out + npix * 4;
    rt1w_stats st;
    memset(&st, 0, sizeof st);
    rt1w_render_params bp = *p; /* batch b: samples sample_offset + b n .. + n - 1 as raw sums; one chunk size for all, the default of n samples */
    bp.flags |= RT1W_OUT_SUM;
    bp.spp = n;
    for (uint32_t b = 0; b < k; ++b) {
        bp.sample_offset = p->sample_offset + b * n;
        rt1w_stats sb;
        memset(&sb, 0, sizeof sb);
        if ((rc = render_common(c, &bp, c->d_batches + npix * 3 * b, &sb)) < 0) return rc;
        if (b == 0u) st = sb;
        else { st.paths += sb.paths; st.segments += sb.segments; st.kernel_ms += sb.kernel_ms; st.passes += sb.passes; }
    }
    rt1w_render_params ap = *p; /* the feature buffers of the same tile, all k n samples and seed, by the scene's own variant */
    ap.flags = 0u;
    rt1w_stats sa, sv, sd;
    if ((rc = render_aov_common(c, &ap, &deep, d_aov, &sa)) < 0) return rc;
    if ((rc = batch_variance_common(c, dp.width, dp.height, k, n, dp.flags, c->d_batches, d_aov, d_frame, d_var, &sv)) < 0) return rc;
    if ((rc = denoise_var_common(c, &dp, sigma_variance, d_frame, d_aov, d_var, d_frame, &sd)) < 0) return rc;
    if (!hip_ok(hipMemcpy(out_rgb, d_frame, npix * 3 * sizeof(double), hipMemcpyDeviceToHost), "denoised frame copy")) return RT1W_ERR_DEVICE;
    if (stats) {
        *stats = st;
        stats->kernel_ms = st.kernel_ms + sa.kernel_ms + sv.kernel_ms + sd.kernel_ms;
        stats->grid = sd.grid; stats->block = sd.block;
        stats->total_ms = timer.ms();
    }
    return RT1W_OK;
}

/* ---- adaptive sampling (include/rt1w.h: rt1w_accum_merge, rt1w_accum_resolve, rt1w_accum_tile_error, rt1w_render_adaptive) ---- */
/* the context's accumulator buffer (the accumulator and, behind it, the tile errors), grown to `bytes` */
int accum_reserve(rt1w_context* c, size_t bytes) {
    if (bytes <= c->accum_bytes) return RT1W_OK;
    if (c->d_accum) (void)hipFree(c->d_accum);
    c->d_accum = nullptr; c->accum_bytes = 0;
    if (!hip_ok(hipMalloc((void**)&c->d_accum, bytes), "hipMalloc(accumulator)")) return RT1W_ERR_NOMEM;
    c->accum_bytes = bytes;
    return RT1W_OK;
}
int accum_frame_validate(const rt1w_context* c, uint32_t w, uint32_t h) {
    if (!c) { set_error("null argument"); return RT1W_ERR_INVALID; }
    if (rt_ad_frame_ok(w, h)) return RT1W_OK;
    set_error("accumulator: width and height must be 1 .. 2^30");
    return RT1W_ERR_INVALID;
}
int accum_merge_common(rt1w_context* c, uint32_t w, uint32_t h, uint32_t x0, uint32_t y0, uint32_t tw, uint32_t th, uint32_t batch_spp, uint32_t flags,
                       const double* d_sums, const double* d_aov, double* d_acc, rt1w_stats* stats) {
    RtLane& l = c->lane[0];
    unsigned launch[2] = {0u, 0u};
    (void)hipEventRecord(l.ev0, l.stream);
    const int rc = rt1w_internal_accum_merge_launch(w, h, x0, y0, tw, th, batch_spp, flags, d_sums, d_aov, d_acc, l.stream, launch);
    return lane_finish(c, rc, launch, (uint64_t)tw * th, "accumulator merge", stats);
}
/* the list is checked by the caller (rt_ad_tiles_check) */
int accum_merge_tiles_common(rt1w_context* c, uint32_t w, uint32_t h, uint32_t tile, const rt1w_tile* tiles, uint32_t n, uint32_t batch_spp, uint32_t flags,
                             const double* d_sums, const double* d_aov, double* d_acc, rt1w_stats* stats) {
    RtLane& l = c->lane[0];
    const uint32_t* d_rec = nullptr;
    int rc = tiles_upload(c, tiles, n, &d_rec);
    if (rc < 0) return rc;
    unsigned launch[2] = {0u, 0u};
    (void)hipEventRecord(l.ev0, l.stream);
    rc = rt1w_internal_accum_merge_tiles_launch(w, h, tile, d_rec, n, batch_spp, flags, d_sums, d_aov, d_acc, l.stream, launch);
    uint64_t inside = 0;
    for (uint32_t k = 0; k < n; ++k) inside += (uint64_t)std::min(tile, w - tiles[k].x0) * std::min(tile, h - tiles[k].y0);
    return lane_finish(c, rc, launch, inside, "accumulator merge (tile list)", stats);
}
int accum_resolve_common(rt1w_context* c, uint32_t w, uint32_t h, uint32_t batch_spp, const double* d_acc, double* d_frame, double* d_var, double* d_spp,
                         rt1w_stats* stats) {
    RtLane& l = c->lane[0];
    unsigned launch[2] = {0u, 0u};
    (void)hipEventRecord(l.ev0, l.stream);
    const int rc = rt1w_internal_accum_resolve_launch(w, h, batch_spp, d_acc, d_frame, d_var, d_spp, l.stream, launch);
    return lane_finish(c, rc, launch, (uint64_t)w * h, "accumulator resolve", stats);
}
int accum_tile_error_common(rt1w_context* c, uint32_t w, uint32_t h, uint32_t tile, const double* d_acc, double* d_err, rt1w_stats* stats) {
    RtLane& l = c->lane[0];
    unsigned launch[2] = {0u, 0u};
    (void)hipEventRecord(l.ev0, l.stream);
    const int rc = rt1w_internal_accum_tile_error_launch(w, h, tile, d_acc, d_err, l.stream, launch);
    return lane_finish(c, rc, launch, (uint64_t)w * h, "tile error", stats);
}
/* the two rt1w_accum_merge entries.  Device memory, or (host) host memory: the accumulator then goes through the context's accumulator
 * buffer, the feature buffers and the batch through the framebuffer */
int accum_merge(rt1w_context* c, uint32_t w, uint32_t h, uint32_t x0, uint32_t y0, uint32_t tw, uint32_t th, uint32_t batch_spp, uint32_t flags,
                const double* sums, const double* aov, double* acc, bool host, rt1w_stats* stats) {
    int rc = accum_frame_validate(c, w, h);
    if (rc < 0) return rc;
    if (!rt_ad_rect_ok(w, h, x0, y0, tw, th, batch_spp, flags)) {
        set_error("accumulator merge: the rectangle must lie inside the frame, batch_spp >= 1, flags 0 or RT1W_DENOISE_KEEP_ALBEDO");
        return RT1W_ERR_INVALID;
    }
    if (!sums || !aov || !acc) { set_error("null buffer"); return RT1W_ERR_INVALID; }
    if (!hip_ok(hipSetDevice(c->device), "hipSetDevice")) return RT1W_ERR_DEVICE;
    const RtTimer timer;
    const size_t npix = (size_t)w * h, tpix = (size_t)tw * th;
    const double *d_sums = sums, *d_aov = aov;
    double* d_acc = acc;
    if (host) {
        if ((rc = reserve_out(c, (npix * RT1W_AOV_CHANNELS + tpix * 3) * sizeof(double))) < 0) return rc;
        if ((rc = accum_reserve(c, npix * RT_AD_RECORD * sizeof(double))) < 0) return rc;
        double* d_s = c->d_out + npix * RT1W_AOV_CHANNELS;
        if (!hip_ok(hipMemcpy(c->d_out, aov, npix * RT1W_AOV_CHANNELS * sizeof(double), hipMemcpyHostToDevice), "accumulator merge: feature buffer copy")) return RT1W_ERR_DEVICE;
        if (!hip_ok(hipMemcpy(d_s, sums, tpix * 3 * sizeof(double), hipMemcpyHostToDevice), "accumulator merge: sums copy")) return RT1W_ERR_DEVICE;
        if (!hip_ok(hipMemcpy(c->d_accum, acc, npix * RT_AD_RECORD * sizeof(double), hipMemcpyHostToDevice), "accumulator merge: accumulator copy")) return RT1W_ERR_DEVICE;
        d_aov = c->d_out; d_sums = d_s; d_acc = c->d_accum;
    }
    rt1w_stats st;
    if ((rc = accum_merge_common(c, w, h, x0, y0, tw, th, batch_spp, flags, d_sums, d_aov, d_acc, &st)) < 0) return rc;
    if (host && !hip_ok(hipMemcpy(acc, d_acc, npix * RT_AD_RECORD * sizeof(double), hipMemcpyDeviceToHost), "accumulator merge: result copy")) return RT1W_ERR_DEVICE;
    if (stats) { *stats = st; stats->total_ms = timer.ms(); }
    return RT1W_OK;
}
int accum_merge_tiles(rt1w_context* c, uint32_t w, uint32_t h, uint32_t tile, const rt1w_tile* tiles, uint32_t n, uint32_t batch_spp, uint32_t flags,
                      const double* sums, const double* aov, double* acc, bool host, rt1w_stats* stats) {
    if (!c) { set_error("null argument"); return RT1W_ERR_INVALID; }
    if (const char* why = rt_ad_tiles_check(w, h, tile, tiles, n, batch_spp, flags)) { set_error(why); return RT1W_ERR_INVALID; }
    if (!sums || !aov || !acc) { set_error("null buffer"); return RT1W_ERR_INVALID; }
    if (!hip_ok(hipSetDevice(c->device), "hipSetDevice")) return RT1W_ERR_DEVICE;
    const RtTimer timer;
    const size_t npix = (size_t)w * h, tpix = (size_t)n * tile * tile;
    const double *d_sums = sums, *d_aov = aov;
    double* d_acc = acc;
    int rc;
    if (host) {
        if ((rc = reserve_out(c, (npix * RT1W_AOV_CHANNELS + tpix * 3) * sizeof(double))) < 0) return rc;
        if ((rc = accum_reserve(c, npix * RT_AD_RECORD * sizeof(double))) < 0) return rc;
        double* d_s = c->d_out + npix * RT1W_AOV_CHANNELS;
        if (!hip_ok(hipMemcpy(c->d_out, aov, npix * RT1W_AOV_CHANNELS * sizeof(double), hipMemcpyHostToDevice), "accumulator merge: feature buffer copy")) return RT1W_ERR_DEVICE;
        if (!hip_ok(hipMemcpy(d_s, sums, tpix * 3 * sizeof(double), hipMemcpyHostToDevice), "accumulator merge: sums copy")) return RT1W_ERR_DEVICE;
        if (!hip_ok(hipMemcpy(c->d_accum, acc, npix * RT_AD_RECORD * sizeof(double), hipMemcpyHostToDevice), "accumulator merge: accumulator copy")) return RT1W_ERR_DEVICE;
        d_aov = c->d_out; d_sums = d_s; d_acc = c->d_accum;
    }
    rt1w_stats st;
    if ((rc = accum_merge_tiles_common(c, w, h, tile, tiles, n, batch_spp, flags, d_sums, d_aov, d_acc, &st)) < 0) return rc;
    if (host && !hip_ok(hipMemcpy(acc, d_acc, npix * RT_AD_RECORD * sizeof(double), hipMemcpyDeviceToHost), "accumulator merge: result copy")) return RT1W_ERR_DEVICE;
    if (stats) { *stats = st; stats->total_ms = timer.ms(); }
    return RT1W_OK;
}
int accum_resolve(rt1w_context* c, uint32_t w, uint32_t h, uint32_t batch_spp, const double* acc, double* frame, double* var, double* spp, bool host,
                  rt1w_stats* stats) {
    int rc = accum_frame_validate(c, w, h);
    if (rc < 0) return rc;
    if (batch_spp == 0u) { set_error("accumulator resolve: batch_spp must be >= 1"); return RT1W_ERR_INVALID; }
    if (!acc || !frame || !var || !spp) { set_error("null buffer"); return RT1W_ERR_INVALID; }
    if (!hip_ok(hipSetDevice(c->device), "hipSetDevice")) return RT1W_ERR_DEVICE;
    const RtTimer timer;
    const size_t npix = (size_t)w * h;
    const double* d_acc = acc;
    double *d_frame = frame, *d_var = var, *d_spp = spp;
    if (host) {
        if ((rc = reserve_out(c, npix * 5 * sizeof(double))) < 0) return rc;
        if ((rc = accum_reserve(c, npix * RT_AD_RECORD * sizeof(double))) < 0) return rc;
        if (!hip_ok(hipMemcpy(c->d_accum, acc, npix * RT_AD_RECORD * sizeof(double), hipMemcpyHostToDevice), "accumulator resolve: accumulator copy")) return RT1W_ERR_DEVICE;
        d_acc = c->d_accum; d_frame = c->d_out; d_var = c->d_out + npix * 3; d_spp = c->d_out + npix * 4;
    }
    rt1w_stats st;
    if ((rc = accum_resolve_common(c, w, h, batch_spp, d_acc, d_frame, d_var, d_spp, &st)) < 0) return rc;
    if (host) {
        if (!hip_ok(hipMemcpy(frame, d_frame, npix * 3 * sizeof(double), hipMemcpyDeviceToHost), "accumulator resolve: frame copy")) return RT1W_ERR_DEVICE;
        if (!hip_ok(hipMemcpy(var, d_var, npix * sizeof(double), hipMemcpyDeviceToHost), "accumulator resolve: variance copy")) return RT1W_ERR_DEVICE;
        if (!hip_ok(hipMemcpy(spp, d_spp, npix * sizeof(double), hipMemcpyDeviceToHost), "accumulator resolve: count copy")) return RT1W_ERR_DEVICE;
    }
    if (stats) { *stats = st; stats->total_ms = timer.ms(); }
    return RT1W_OK;
}
int accum_tile_error(rt1w_context* c, uint32_t w, uint32_t h, uint32_t tile, const double* acc, double* err, bool host, rt1w_stats* stats) {
    int rc = accum_frame_validate(c, w, h);
    if (rc < 0) return rc;
    if (!rt_ad_tile_ok(tile)) { set_error("tile error: tile must be a multiple of 16 in 16 .. 256"); return RT1W_ERR_INVALID; }
    if (!acc || !err) { set_error("null buffer"); return RT1W_ERR_INVALID; }
    if (!hip_ok(hipSetDevice(c->device), "hipSetDevice")) return RT1W_ERR_DEVICE;
    const RtTimer timer;
    const size_t npix = (size_t)w * h, ntiles = (size_t)((w + tile - 1u) / tile) * ((h + tile - 1u) / tile);
    const double* d_acc = acc;
    double* d_err = err;
    if (host) {
        if ((rc = accum_reserve(c, (npix * RT_AD_RECORD + ntiles) * sizeof(double))) < 0) return rc;
        if (!hip_ok(hipMemcpy(c->d_accum, acc, npix * RT_AD_RECORD * sizeof(double), hipMemcpyHostToDevice), "tile error: accumulator copy")) return RT1W_ERR_DEVICE;
        d_acc = c->d_accum; d_err = c->d_accum + npix * RT_AD_RECORD;
    }
    rt1w_stats st;
    if ((rc = accum_tile_error_common(c, w, h, tile, d_acc, d_err, &st)) < 0) return rc;
    if (host && !hip_ok(hipMemcpy(err, d_err, ntiles * sizeof(double), hipMemcpyDeviceToHost), "tile error: result copy")) return RT1W_ERR_DEVICE;
    if (stats) { *stats = st; stats->total_ms = timer.ms(); }
    return RT1W_OK;
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
    if ((rc = validate(c, p ? &q : nullptr)) < 0) return rc;
    if (!out_rgb) { set_error("null output"); return RT1W_ERR_INVALID; }
    if ((rc = refuse_named_flag(p->flags, true, " does not apply to rt1w_render_denoised")) < 0) return rc;
    if (p->strip_rows) { set_error("rt1w_render_denoised takes a contiguous tile (strip_rows must be 0): denoise the gathered frame with rt1w_denoise"); return RT1W_ERR_INVALID; }
    if (p->precision != RT1W_PRECISION_F64) { set_error("RT1W_PRECISION_F32 does not apply to rt1w_render_denoised (the filter is f64 only)"); return RT1W_ERR_INVALID; }
    if (p->x0 || p->y0 || p->tile_w != p->width || p->tile_h != p->height) { set_error("rt1w_render_adaptive takes the whole frame (x0 = y0 = 0, tile_w = width, tile_h = height)"); return RT1W_ERR_INVALID; }
    if (plan.one_launch && (p->flags & ~RT1W_GENERIC)) { set_error("adaptive: with RT1W_ADAPTIVE_ONE_LAUNCH p->flags must be 0 or RT1W_GENERIC (rt1w_render_tiles runs the generic kernels)"); return RT1W_ERR_INVALID; }
    if ((unsigned long long)p->sample_offset + plan.max_spp > 0xFFFFFFFFull) { set_error("adaptive: sample_offset + max_spp exceeds 2^32 - 1"); return RT1W_ERR_INVALID; }
    const uint32_t W = p->width, H = p->height;
    rt1w_denoise_params dp;
    memset(&dp, 0, sizeof dp);
    if (d) dp = *d;
    if ((dp.width && dp.width != W) || (dp.height && dp.height != H)) { set_error("denoise: width / height must be 0 or the tile's"); return RT1W_ERR_INVALID; }
    dp.width = W; dp.height = H;
    if ((rc = denoise_validate(c, &dp)) < 0) return rc;
    if (!hip_ok(hipSetDevice(c->device), "hipSetDevice")) return RT1W_ERR_DEVICE;
    const RtTimer timer;
    const size_t npix = (size_t)W * H;
    const uint32_t tiles_x = (W + plan.tile - 1u) / plan.tile, tiles_y = (H + plan.tile - 1u) / plan.tile;
    const size_t ntiles = (size_t)tiles_x * tiles_y;
    if ((rc = reserve_out(c, npix * (5 + RT1W_AOV_CHANNELS) * sizeof(double))) < 0) return rc;
    /* one launch per round: a round's batch is whole tiles, the edge tiles' pixels beyond the frame included */
    const size_t batch_px = plan.one_launch ? std::max(npix, ntiles * plan.tile * plan.tile) : npix;
    if ((rc = batches_reserve(c, batch_px * 3 * sizeof(double))) < 0) return rc;
    if ((rc = accum_reserve(c, (npix * RT_AD_RECORD + ntiles) * sizeof(double))) < 0) return rc;
    double* d_frame = c->d_out;
    double* d_var = c->d_out + npix * 3;
    double* d_spp = c->d_out + npix * 4;
    double* d_aov = c->d_out + npix * 5;
    double* d_acc = c->d_accum;
    double* d_err = c->d_accum + npix * RT_AD_RECORD;
    RtLane& l = c->lane[0];
    if (!hip_ok(hipMemsetAsync(d_acc, 0, npix * RT_AD_RECORD * sizeof(double), l.stream), "accumulator clear")) return RT1W_ERR_DEVICE;
    rt1w_stats st, sk;
    memset(&st, 0, sizeof st);
    rt1w_render_params ap = *p; /* the feature buffers of the pilot's samples, by the scene's own variant */
    ap.flags = 0u; ap.spp = plan.pilot * plan.batch_spp;
    if ((rc = render_aov_common(c, &ap, nullptr, d_aov, &sk)) < 0) return rc;
    double kernel_ms = sk.kernel_ms;
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
        int r = render_common(c, &bp, c->d_batches, &sb);
        if (r < 0) return r;
        if (first) { st = sb; first = false; }
        else { st.paths += sb.paths; st.segments += sb.segments; st.passes += sb.passes; }
        kernel_ms += sb.kernel_ms;
        if ((r = accum_merge_common(c, W, H, x0, y0, tw, th, plan.batch_spp, plan.flags, c->d_batches, d_aov, d_acc, &sk)) < 0) return r;
        kernel_ms += sk.kernel_ms;
        return RT1W_OK;
    };
    for (uint32_t b = 0; b < plan.pilot; ++b)
        if ((rc = batch(0u, 0u, W, H, b)) < 0) return rc;
    std::vector<uint32_t> m(ntiles, plan.pilot);
    std::vector<double> err(ntiles);
    std::vector<rt1w_tile> list;
    uint32_t rounds = 0;
    for (;;) {
        if ((rc = accum_tile_error_common(c, W, H, plan.tile, d_acc, d_err, &sk)) < 0) return rc;
        kernel_ms += sk.kernel_ms;
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
            if ((rc = render_tiles_common(c, &bp, plan.tile, list.data(), (uint32_t)list.size(), c->d_batches, &sb)) < 0) return rc;
            st.paths += sb.paths; st.segments += sb.segments; st.passes += sb.passes;
            kernel_ms += sb.kernel_ms;
            if ((rc = accum_merge_tiles_common(c, W, H, plan.tile, list.data(), (uint32_t)list.size(), plan.batch_spp, plan.flags, c->d_batches, d_aov, d_acc, &sk)) < 0) return rc;
            kernel_ms += sk.kernel_ms;
        } else
        for (const RtAdRun& r : rt_ad_group(plan, tiles_x, W, H, taken, m.data()))
            if ((rc = batch(r.x0, r.y0, r.w, r.h, r.m)) < 0) return rc;
        for (uint32_t t : taken) ++m[t];
    }
    if ((rc = accum_resolve_common(c, W, H, plan.batch_spp, d_acc, d_frame, d_var, d_spp, &sk)) < 0) return rc;
    kernel_ms += sk.kernel_ms;
    if (d) {
        if ((rc = denoise_var_common(c, &dp, sigma_variance, d_frame, d_aov, d_var, d_frame, &sk)) < 0) return rc;
        kernel_ms += sk.kernel_ms;
    }
    if (!hip_ok(hipMemcpy(out_rgb, d_frame, npix * 3 * sizeof(double), hipMemcpyDeviceToHost), "adaptive frame copy")) return RT1W_ERR_DEVICE;
    if (out_spp && !hip_ok(hipMemcpy(out_spp, d_spp, npix * sizeof(double), hipMemcpyDeviceToHost), "adaptive count copy")) return RT1W_ERR_DEVICE;
    if (stats) {
        *stats = st;
        stats->kernel_ms = kernel_ms;
        stats->chunk = bp.chunk; stats->n_chunks = rounds;
        stats->grid = sk.grid; stats->block = sk.block;
        stats->total_ms = timer.ms();
    }
    return RT1W_OK;
}

} // namespace

extern "C" {
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
} /* extern "C" */
