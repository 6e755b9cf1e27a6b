/* denoise_host.cpp -- the CPU twin of the filter kernels (denoise.hip, denoise_var.hip, denoise_halves.hip, denoise_cross.hip) and of temporal accumulation and its variance (temporal.hip, temporal_var.hip): rt_denoise.h, rt_denoise_var.h, rt_denoise_halves.h, rt_denoise_cross.h, rt_temporal.h and rt_temporal_var.h compiled for the host (g++, -ffp-contract=off
 * like every build of the core).  Diagnostics library only (librt1w_lab.so): the expected side of the GPU tests' bit-equality checks
 * and what the CPU tier's property and quality tests run.  librt1w.so keeps no CPU path. */
#include <cstring>
#include <thread>
#include <vector>

#include "rt1w.h"
#include "rt_denoise.h"
#include "rt_denoise_var.h"
#include "rt_denoise_halves.h"
#include "rt_denoise_cross.h"
#include "rt_temporal.h"
#include "rt_temporal_var.h"
#include "walk_lab.h"

namespace {
/* rows dealt round-robin over at most 16 threads: every pixel is computed whole by one thread, so the result does not depend on it */
template <class F>
void for_rows(uint32_t h, F f) {
    unsigned hw = std::thread::hardware_concurrency();
    uint32_t n_threads = hw == 0u ? 1u : (hw > 16u ? 16u : hw);
    if (n_threads > h) n_threads = h;
    std::vector<std::thread> pool;
    for (uint32_t t = 1; t < n_threads; ++t) pool.emplace_back([=]() { for (uint32_t y = t; y < h; y += n_threads) f(y); });
    for (uint32_t y = 0; y < h; y += n_threads) f(y);
    for (auto& th : pool) th.join();
}
/* the twin of an a-trous filter F (the policies at the end of rt_denoise*.h; the kernels' skeleton over them is rt_atrous_kernels.h):
 * prepare every pixel from the buffers `in`, run the levels with ping-pong, finish on the last, where hook(i, c, g) sees pixel i's
 * record and guide as well.  sv2, err_px: as F takes them */
template <class F, class Hook, class... In>
void atrous_host(const RtDnParams& P, double sv2, double* out, double* err_px, Hook hook, In... in) {
    typedef typename F::Col Col;
    const size_t n = (size_t)P.w * P.h;
    std::vector<Col> a(n), b(n);
    std::vector<RtDnGuide> g(n);
    for_rows(P.h, [&](uint32_t y) {
        for (uint32_t x = 0; x < P.w; ++x) {
            const size_t i = (size_t)y * P.w + x;
            F::prepare(P, i, a[i], g[i], in...);
        }
    });
    Col* src = a.data();
    Col* dst = b.data();
    for (uint32_t level = 0; level < P.levels; ++level) {
        const RtDnGlobalSrc<Col> s{src, g.data(), P.w};
        const bool last = level + 1u == P.levels;
        for_rows(P.h, [&](uint32_t y) {
            for (uint32_t x = 0; x < P.w; ++x) {
                const size_t i = (size_t)y * P.w + x;
                const Col c = F::level(P, sv2, s, x, y, level);
                if (last) {
                    F::finish(c, g[i], i, out, err_px);
                    hook(i, c, g[i]);
                } else
                    dst[i] = c;
            }
        });
        Col* t = src; src = dst; dst = t;
    }
}
const auto no_hook = [](size_t, const auto&, const RtDnGuide&) {};
} // namespace

extern "C" int rt1w_lab_denoise_host(const rt1w_denoise_params* p, const double* frame, const double* aov, double* out) {
    if (!p || !frame || !aov || !out) return RT1W_ERR_INVALID;
    RtDnParams P;
    if (!rt_dn_make_params(p->width, p->height, p->iterations, p->flags, p->sigma_colour, p->sigma_normal, p->sigma_depth, P)) return RT1W_ERR_INVALID;
    atrous_host<RtDnFilter>(P, 0.0, out, nullptr, no_hook, frame, aov);
    return RT1W_OK;
}

extern "C" int rt1w_lab_batch_variance_host(uint32_t width, uint32_t height, uint32_t batches, uint32_t batch_spp, uint32_t flags, const double* sums,
                                            const double* aov, double* frame, double* var) {
    if (!sums || !aov || !frame || !var) return RT1W_ERR_INVALID;
    RtDnParams P;
    if (!rt_dn_make_params(width, height, 0u, flags, 0.0, 0.0, 0.0, P) || !rt_dv_batches_ok(batches, batch_spp)) return RT1W_ERR_INVALID;
    const unsigned long long stride = (unsigned long long)P.w * P.h * 3u;
    for_rows(P.h, [&](uint32_t y) {
        for (uint32_t x = 0; x < P.w; ++x) {
            const size_t i = (size_t)y * P.w + x;
            rt_dv_variance_pixel(batches, batch_spp, P.keep_albedo != 0u, sums + i * 3, stride, aov + i * 8, frame + i * 3, var + i);
        }
    });
    return RT1W_OK;
}

extern "C" int rt1w_lab_denoise_var_host(const rt1w_denoise_params* p, const double* frame, const double* aov, const double* var, double sigma_variance,
                                         double* out) {
    if (!p || !frame || !aov || !var || !out) return RT1W_ERR_INVALID;
    RtDnParams P;
    double sv;
    if (!rt_dn_make_params(p->width, p->height, p->iterations, p->flags, 0.0, p->sigma_normal, p->sigma_depth, P) || !rt_dv_sigma(sigma_variance, sv)) return RT1W_ERR_INVALID;
    atrous_host<RtDvFilter>(P, sv * sv, out, nullptr, no_hook, frame, aov, var);
    return RT1W_OK;
}

extern "C" int rt1w_lab_denoise_var_halves_host(const rt1w_denoise_params* p, const double* frame, const double* aov, const double* var,
                                                const double* half_a, const double* half_b, double sigma_variance, double* out, double* err_px,
                                                double* filtered_a, double* filtered_b) {
    if (!p || !frame || !aov || !var || !half_a || !half_b || !out || !err_px) return RT1W_ERR_INVALID;
    RtDnParams P;
    double sv;
    if (!rt_dn_make_params(p->width, p->height, p->iterations, p->flags, 0.0, p->sigma_normal, p->sigma_depth, P) || !rt_dv_sigma(sigma_variance, sv)) return RT1W_ERR_INVALID;
    /* for the tests: the two filtered halves with the albedo back, the products rt_dh_finish_pixel takes the luminances of */
    atrous_host<RtDhFilter>(P, sv * sv, out, err_px, [&](size_t i, const RtDhCol& c, const RtDnGuide& g) {
        if (filtered_a) { filtered_a[i * 3] = c.ar * g.ar; filtered_a[i * 3 + 1] = c.ag * g.ag; filtered_a[i * 3 + 2] = c.ab * g.ab; }
        if (filtered_b) { filtered_b[i * 3] = c.br * g.ar; filtered_b[i * 3 + 1] = c.bg * g.ag; filtered_b[i * 3 + 2] = c.bb * g.ab; }
    }, frame, aov, var, half_a, half_b);
    return RT1W_OK;
}

extern "C" int rt1w_lab_denoise_cross_host(const rt1w_denoise_params* p, const double* frame, const double* aov, const double* var, const double* half_a,
                                           const double* half_b, double sigma_variance, double* out, double* err_px, double* rec) {
    if (!p || !frame || !aov || !var || !half_a || !half_b || !out || !err_px) return RT1W_ERR_INVALID;
    RtDnParams P;
    double sv;
    /* sigma_colour is not used by this filter, but the entries refuse a bad one (denoise_validate): so does the twin */
    if (!rt_dn_make_params(p->width, p->height, p->iterations, p->flags, p->sigma_colour, p->sigma_normal, p->sigma_depth, P) || !rt_dv_sigma(sigma_variance, sv)) return RT1W_ERR_INVALID;
    atrous_host<RtDcFilter>(P, sv * sv, out, err_px, [&](size_t i, const RtDcCol& c, const RtDnGuide&) {
        if (rec) memcpy(rec + i * 10, &c, sizeof c);
    }, frame, aov, var, half_a, half_b);
    return RT1W_OK;
}

extern "C" int rt1w_lab_temporal_host(const rt1w_temporal_params* p, const double* cur_frame, const double* cur_aov, const rt1w_camera* cur_cam,
                                      const double* prev_hist, const double* prev_len, const double* prev_aov, const rt1w_camera* prev_cam, double* hist,
                                      double* len, double* frame_out, double* rec) {
    if (!p || !cur_frame || !cur_aov || !cur_cam || !prev_hist || !prev_len || !prev_aov || !prev_cam || !hist || !len || !frame_out) return RT1W_ERR_INVALID;
    RtTmParams P;
    if (!rt_tm_make_params(p->width, p->height, p->flags, p->max_history, p->depth_tol, p->normal_min, P)) return RT1W_ERR_INVALID;
    const size_t n = (size_t)P.w * P.h;
    /* the entries' own check: an output that overlaps another buffer of the call */
    const struct { const double* p; size_t count; } b[8] = {{cur_frame, n * 3}, {cur_aov, n * 8}, {prev_hist, n * 3}, {prev_len, n}, {prev_aov, n * 8},
                                                            {hist, n * 3}, {len, n}, {frame_out, n * 3}};
    for (int o = 5; o < 8; ++o)
        for (int k = 0; k < 8; ++k)
            if (k != o && (const char*)b[o].p < (const char*)(b[k].p + b[k].count) && (const char*)b[k].p < (const char*)(b[o].p + b[o].count)) return RT1W_ERR_INVALID;
    static_assert(sizeof(rt1w_camera) == sizeof(RtCamera), "rt1w_camera is RtCamera's layout");
    RtCamera cc, pc;
    memcpy(&cc, cur_cam, sizeof cc);
    memcpy(&pc, prev_cam, sizeof pc);
    for_rows(P.h, [&](uint32_t y) {
        for (uint32_t x = 0; x < P.w; ++x) {
            const size_t i = (size_t)y * P.w + x;
            rt_tm_pixel(P, cc, pc, cur_frame, cur_aov, prev_hist, prev_len, prev_aov, nullptr, x, y, hist + i * 3, len + i, frame_out + i * 3,
                        nullptr, rec ? rec + i * RT_TM_REC : nullptr);
        }
    });
    return RT1W_OK;
}

extern "C" int rt1w_lab_temporal_moments_host(const rt1w_temporal_params* p, const double* cur_frame, const double* cur_aov, const rt1w_camera* cur_cam,
                                              const double* prev_hist, const double* prev_m2, const double* prev_len, const double* prev_aov,
                                              const rt1w_camera* prev_cam, double* hist, double* m2, double* len, double* frame_out, double* rec) {
    if (!p || !cur_frame || !cur_aov || !cur_cam || !prev_hist || !prev_m2 || !prev_len || !prev_aov || !prev_cam || !hist || !m2 || !len || !frame_out)
        return RT1W_ERR_INVALID;
    RtTmParams P;
    if (!rt_tm_make_params(p->width, p->height, p->flags, p->max_history, p->depth_tol, p->normal_min, P)) return RT1W_ERR_INVALID;
    const size_t n = (size_t)P.w * P.h;
    /* the entries' own check: an output that overlaps another buffer of the call */
    const struct { const double* p; size_t count; } b[10] = {{cur_frame, n * 3}, {cur_aov, n * 8}, {prev_hist, n * 3}, {prev_m2, n}, {prev_len, n},
                                                             {prev_aov, n * 8}, {hist, n * 3}, {m2, n}, {len, n}, {frame_out, n * 3}};
    for (int o = 6; o < 10; ++o)
        for (int k = 0; k < 10; ++k)
            if (k != o && (const char*)b[o].p < (const char*)(b[k].p + b[k].count) && (const char*)b[k].p < (const char*)(b[o].p + b[o].count)) return RT1W_ERR_INVALID;
    RtCamera cc, pc;
    memcpy(&cc, cur_cam, sizeof cc);
    memcpy(&pc, prev_cam, sizeof pc);
    for_rows(P.h, [&](uint32_t y) {
        for (uint32_t x = 0; x < P.w; ++x) {
            const size_t i = (size_t)y * P.w + x;
            rt_tm_pixel(P, cc, pc, cur_frame, cur_aov, prev_hist, prev_len, prev_aov, prev_m2, x, y, hist + i * 3, len + i, frame_out + i * 3, m2 + i,
                        rec ? rec + i * RT_TM_REC : nullptr);
        }
    });
    return RT1W_OK;
}

extern "C" int rt1w_lab_temporal_variance_host(uint32_t width, uint32_t height, const double* hist, const double* m2, const double* len, const double* aov,
                                               double* var) {
    RtDnParams P;
    if (!hist || !m2 || !len || !aov || !var || !rt_tv_make_params(width, height, P)) return RT1W_ERR_INVALID;
    const size_t n = (size_t)P.w * P.h;
    const struct { const double* p; size_t count; } b[4] = {{hist, n * 3}, {m2, n}, {len, n}, {aov, n * 8}};
    for (int k = 0; k < 4; ++k)
        if ((const char*)var < (const char*)(b[k].p + b[k].count) && (const char*)b[k].p < (const char*)(var + n)) return RT1W_ERR_INVALID;
    for_rows(P.h, [&](uint32_t y) {
        for (uint32_t x = 0; x < P.w; ++x) var[(size_t)y * P.w + x] = rt_tv_pixel(P, hist, m2, len, aov, x, y);
    });
    return RT1W_OK;
}

/* f32_exact.hip: the same two functions of rt_denoise.h, one lane per element, on GPU 0 */
int rt_lab_denoise_elementary_device(int fn, const double* x, const uint32_t* e, uint64_t n, double* out);

extern "C" int rt1w_lab_denoise_elementary(int device, int fn, const double* x, const uint32_t* e, uint64_t n, double* out) {
    if ((device != 0 && device != 1) || (fn != 0 && fn != 1) || !x || !out || (fn == 1 && !e) || n == 0u) return RT1W_ERR_INVALID;
    if (device == 1) return rt_lab_denoise_elementary_device(fn, x, e, n, out);
    for (uint64_t i = 0; i < n; ++i) out[i] = fn == 0 ? rt_dn_falloff(x[i]) : rt_dn_powi(x[i], e[i]);
    return RT1W_OK;
}

extern "C" int rt1w_lab_denoised_var_split(uint32_t spp, uint32_t batches, double sigma_variance, uint32_t out[2]) {
    double sv;
    uint32_t k = 0u, n = 0u;
    if (!rt_dv_sigma(sigma_variance, sv) || !rt_dv_split(spp, batches, k, n)) return RT1W_ERR_INVALID;
    if (out) { out[0] = k; out[1] = n; }
    return RT1W_OK;
}
