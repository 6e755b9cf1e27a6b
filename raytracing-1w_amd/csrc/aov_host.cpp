/* aov_host.cpp -- the CPU twin of the AOV kernels (aov.hip): rt_aov.h and rt_aov_deep.h compiled for the host (g++, -ffp-contract=off
 * like every build of the core) and run over a committed scene's flat arrays.  Diagnostics library only (librt1w_lab.so): the expected side of the GPU
 * tests' bit-equality checks and of the CPU tier's checks against the literal oracle.  librt1w.so keeps no CPU render path. */
#include <thread>
#include <vector>

#include "render_params.h"
#include "rt_aov_deep.h"
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
bool aov_rows_variant(int v, const RtSceneView& sc, const RtFrame& f, const AovDeep& d, uint32_t row0, uint32_t row_step, double* out, uint64_t* rays) {
    switch (v) { /* the variants the kernels are built for */
        case 0: return aov_rows<RtCfgV0>(sc, f, d, row0, row_step, out, rays);
        case 1: return aov_rows<RtCfgV1>(sc, f, d, row0, row_step, out, rays);
        case 2: return aov_rows<RtCfgV2>(sc, f, d, row0, row_step, out, rays);
        case 4: return aov_rows<RtCfgV4>(sc, f, d, row0, row_step, out, rays);
        case 5: return aov_rows<RtCfgV5>(sc, f, d, row0, row_step, out, rays);
        default: return aov_rows<RtCfgV3>(sc, f, d, row0, row_step, out, rays);
    }
}

int aov_host_run(const rt1w_scene* s, const rt1w_render_params* p, const AovDeep& deep, double* out, uint64_t* segments) {
    if (!s || !p || !out || !s->committed) return RT1W_ERR_INVALID;
    if (const int rc = rt1w::params_check(p, nullptr); rc < 0) return rc; /* the entries' own check: the twin refuses what they refuse */
    if ((p->flags & ~(0xFFu << 8)) != 0u) return RT1W_ERR_INVALID;
    if (p->precision != RT1W_PRECISION_F64) return RT1W_ERR_UNSUPPORTED;
    const uint32_t n_nodes = (uint32_t)s->flat_nodes.size();
    int v = rt_pick_variant(n_nodes, s->has_media, s->has_tex, s->has_msphere, s->scope_depth, s->walk_annotated != 0u);
    if ((p->flags >> 8) & 0xFFu) {
        v = (int)((p->flags >> 8) & 0xFFu) - 1;
        if (!rt_variant_valid(v, n_nodes, s->has_media, s->has_tex, s->has_msphere, s->scope_depth)) return RT1W_ERR_INVALID;
    }
    std::vector<RtNode> nodes(s->flat_nodes);
    nodes.push_back(RtNode{}); /* the spare record the context's node array carries */
    RtSceneView sc = rt1w::view_of(*s);
    sc.nodes = nodes.data(); sc.lights = s->flat_lights.data(); sc.materials = s->materials.data(); sc.textures = s->textures.data();
    sc.perlin = s->perlin.data(); sc.images = s->images.data();
    RtFrame f = rt1w::frame_of(p);
    f.max_depth = 1u; f.chunk = p->spp; f.n_chunks = 1u;
    /* rows dealt round-robin over at most 16 threads: every pixel is computed whole by one thread, so the result does not depend on it */
    unsigned hw = std::thread::hardware_concurrency();
    uint32_t n_threads = hw == 0u ? 1u : (hw > 16u ? 16u : hw);
    if (n_threads > f.tile_h) n_threads = f.tile_h;
    std::vector<char> ok(n_threads, 1);
    std::vector<uint64_t> rays(n_threads, 0u);
    std::vector<std::thread> pool;
    for (uint32_t t = 1; t < n_threads; ++t) pool.emplace_back([&, t]() { ok[t] = aov_rows_variant(v, sc, f, deep, t, n_threads, out, &rays[t]) ? 1 : 0; });
    ok[0] = aov_rows_variant(v, sc, f, deep, 0u, n_threads, out, &rays[0]) ? 1 : 0;
    for (auto& th : pool) th.join();
    for (char k : ok) if (!k) return RT1W_ERR_STATE; /* a traversal stack overflowed */
    if (segments) { *segments = 0u; for (uint64_t r : rays) *segments += r; }
    return RT1W_OK;
}
} // namespace

extern "C" int rt1w_lab_aov_host(const rt1w_scene* s, const rt1w_render_params* p, double* out) { return aov_host_run(s, p, AovDeep{}, out, nullptr); }

extern "C" int rt1w_lab_aov_deep_host(const rt1w_scene* s, const rt1w_render_params* p, uint32_t max_specular, double max_fuzz, double* out,
                                      uint64_t* segments, uint8_t* lengths) {
    if (!rt_aov_deep_args_ok(max_specular, max_fuzz)) return RT1W_ERR_INVALID;
    AovDeep deep;
    deep.max_specular = (long)max_specular; deep.max_fuzz = max_fuzz; deep.lengths = lengths;
    return aov_host_run(s, p, deep, out, segments);
}
