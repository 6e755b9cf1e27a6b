/* features.hip -- the entries of the feature buffers and the denoiser (include/rt1w.h: rt1w_render_aov*, rt1w_denoise*,
 * rt1w_render_denoised*, rt1w_batch_variance*): validation, buffers, launch, timing, copies.  Host code only, built without a device pass: the
 * kernels belong to aov.hip, denoise.hip and denoise_var.hip and are launched through their host handles, the context and its render path to context.hip (context.h), so a
 * change here rebuilds none of the code objects. */
#include <cstdio>
#include <cstring>

#include "context.h"
#include "rt_aov_deep.h" /* rt_aov_deep_args_ok only */
#include "rt_denoise_var.h" /* rt_dv_batches_ok, rt_dv_sigma, rt_dv_split only */

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
} /* extern "C" */
