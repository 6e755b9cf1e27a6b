/* oracle_flat.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT.
 *
 * The device kernel's core (raytracing-1w_amd/csrc/rt_core.h) compiled for the
 * host with g++, driven by the same work decomposition as the HIP kernel
 * (context.hip: chunk partial sums, then resolve).  Purpose:
 *   - lets the CPU-only test tier check the flattener + iterative integrator
 *     against the literal recursive oracle (oracle.cpp) without a GPU;
 *   - is what the GPU result must equal BIT FOR BIT (same text, same
 *     arithmetic, -ffp-contract=off on both sides);
 *   - can be built with -fsanitize=address,undefined (GPU sanitizers are not
 *     available on the pool).
 * librt1w.so does not contain or call this; it has no CPU render path.
 */
#include <atomic>
#include <thread>
#include <vector>
#include <cstring>

#include "rt_core.h"
#include "rt_walk_table.h" /* the walk table of the kernels that keep the most visited nodes in LDS: built and walked here on the CPU */
#if !defined(RT_RNG_REFSTREAM)
#include "rt_walk_pair.h" /* the pair walk of sphere scenes: its lane functions are built here with bound-checked stacks and queues */
#endif

/* tests/test_static_sweep.py compiles this file a second time with a generated header that defines scene topologies
 * as compile-time arrays (what the library's run-time compiler does for the GPU, jit.cpp) and adds them as variants
 * 100, 101, ...: the unrolled sweep (rt_sweep_static) against the generic one, on the CPU. */
#ifdef ORC_STATIC_TOPO_H
#include ORC_STATIC_TOPO_H
#endif

namespace {
struct HostStack {
    uint32_t e[RT_STACK_CAP + 8];
    int sp = 0;
    int max_sp = 0;
    bool overflow = false;
    void push(uint32_t v) {
        if (sp >= RT_STACK_CAP) { overflow = true; return; }
        e[sp++] = v;
        if (sp > max_sp) max_sp = sp;
    }
    /* write without moving the top (rt_walk_box's branchless push): the touched slot counts towards the high-water mark and
     * must lie inside the stack like a push */
    void poke(int above, uint32_t v) {
        if (sp + above >= RT_STACK_CAP) { overflow = true; return; }
        e[sp + above] = v;
        if (sp + above + 1 > max_sp) max_sp = sp + above + 1;
    }
    uint32_t pop() { return e[--sp]; }
};
}

/* the pixel sums exactly as the kernels keep them (rt_kernel_plain.h; rt_kernels.h: rt_resolve_kernel): a chunk's samples are added
 * in 64 bits (RtV3d, rt_v3d_add), the chunk sums are added in order in 64 bits, the mean is taken in 64 bits -- in the f32 build of this
 * file too, where RtV3 is three floats */
static RtV3d into_sampled64(RtV3d sum, uint32_t samples_per_pixel) { /* rt_into_sampled (color.rs:14-21) of the f64 build */
    const rt_f64 scale = 1.0 / (rt_f64)samples_per_pixel;
    const rt_f64 r = rt_isnan64(sum.x) ? 0.0 : sum.x, g = rt_isnan64(sum.y) ? 0.0 : sum.y, b = rt_isnan64(sum.z) ? 0.0 : sum.z;
    return rt_v3d(r * scale, g * scale, b * scale);
}

template <class Cfg>
static void run_path(const RtSceneView& sc, const RtFrame& f, uint32_t px, uint32_t py, uint32_t s, HostStack& stk,
                     RtV3d& sum, uint64_t& segs, RtPath& path) { /* `path` lives as long as the pixel: the reference-stream build
                                                                   (-DRT_RNG_REFSTREAM) draws all samples of a pixel from one stream */
    rt_path_begin(sc, f, f.x0 + px, rt_frame_row(f, py), f.sample_offset + s, path);
    while (path.alive) {
        segs += path.depth_left != 0u ? 1u : 0u;
        RtGlobalNodes ns{sc.nodes};
        rt_path_step<Cfg>(sc, ns, path, stk);
    }
    sum = rt_v3d_add(sum, path.radiance);
}

#if !defined(RT_RNG_REFSTREAM)
namespace {
/* an array the pair walk's lane functions index like their LDS columns, bounds checked: a write or read outside is recorded, not done */
template <class T>
struct Checked {
    std::vector<T> v;
    bool* fault;
    T dummy{};
    T& operator[](long i) {
        if (i < 0 || (size_t)i >= v.size()) { *fault = true; return dummy; }
        return v[(size_t)i];
    }
};
}
namespace {
/* one lane's pair-walk stack and queue (the kernels' LDS columns), bound-checked */
struct PwMem {
    bool fault = false;
    RtPwLds<1, Checked<uint32_t>, Checked<float>, Checked<uint32_t>> m;
    explicit PwMem(uint32_t stack_cap)
        : m{{std::vector<uint32_t>(stack_cap), &fault}, {std::vector<float>(stack_cap), &fault}, {std::vector<uint32_t>(RT_PW_QCAP), &fault}} {}
};
}
/* A path of a sphere scene as the pair-walk kernels run it (rt_kernel_plain.h: the PW arm of rt_render_ss_body / rt_render_plain_body):
 * every segment's closest hit by the pair walk -- the root's box, then box work and leaf work in the order a lane alone in its wave
 * takes them (box steps while it can, a pending group when it cannot), the NaN hand-overs to the one-entry-per-step walk -- and the
 * second half of the step, rt_path_shade, on that hit.  Stack (`m`: the kernel's entries per lane) and queue are bound-checked. */
static void run_path_pw(const RtSceneView& sc, const RtPwView& pw, const RtFrame& f, uint32_t px, uint32_t py, uint32_t s, HostStack& stk, PwMem& mem,
                        RtV3d& sum, uint64_t& segs, RtPath& path) {
    typedef RtCfgV5 Cfg;
    RtGlobalNodes ns{sc.nodes};
    rt_path_begin(sc, f, f.x0 + px, rt_frame_row(f, py), f.sample_offset + s, path);
    while (path.alive) {
        segs += path.depth_left != 0u ? 1u : 0u;
        RtTrace tr;
        tr.t = RT_R(0.0); tr.prim = RT_NONE; tr.scope = RT_NONE; tr.cls = RT_CLS_TERMINAL;
        if (path.depth_left != 0u) {
            RtPwLane L; L.cur = RT_PW_NONE; L.qh = 0u; L.qn = 0u; L.sp = 0;
            double best_t = RT_INF; uint32_t best_prim = RT_NONE;
            const RtV3 o = path.ray.o, d = path.ray.d, inv = rt_inv3(d);
            const double frac = (path.ray.time - pw.ms_time0) / (pw.ms_time1 - pw.ms_time0);
            bool bad = rt_isnan(frac), walking = bad;
            if (!bad) walking = rt_pw_begin(pw, L, mem.m, o, inv, RT_R(0.001));
            if (walking) {
                while (!bad && !rt_pw_done(L) && !mem.fault) {
                    if (rt_pw_can_box(L)) {
                        rt_pw_box_step(pw, L, mem.m, o, inv, RT_R(0.001), best_t);
                    } else if (L.qn > 0u) {
                        rt_pw_group_step(pw, L, mem.m, o, d, inv, frac, RT_R(0.001), best_t, best_prim);
                        if (rt_isnan(best_t)) bad = true;
                    } else { mem.fault = true; } /* neither kind of work and not done: the state machine is stuck */
                }
                if (bad) { /* the hand-over of the kernels: the segment is redone by the one-entry-per-step walk */
                    uint32_t scope_;
                    best_t = RT_INF; best_prim = RT_NONE;
                    rt_traverse_stack<Cfg, true>(sc, ns, sc.root, path.ray, RT_R(0.001), RT_INF, path.rng, stk, best_t, best_prim, scope_);
                }
                tr.t = best_t; tr.prim = best_prim; tr.scope = RT_NONE;
                if (tr.prim != RT_NONE) {
                    const uint32_t mk = RT_MAT_KINDF(ns.hot(tr.prim).mat) & 0xFFu;
                    tr.cls = mk == RT_MAT_LAMBERTIAN ? RT_CLS_LAMBERT : mk == RT_MAT_DIELECTRIC ? RT_CLS_DIELECTRIC
                           : mk == RT_MAT_METAL ? RT_CLS_METAL : mk == RT_MAT_ISOTROPIC ? RT_CLS_OTHER : RT_CLS_TERMINAL;
                }
            }
        }
        path.radiance = rt_v3(RT_R(0.0), RT_R(0.0), RT_R(0.0)); /* written by the terminal only: not carried across the walk */
        rt_path_shade<Cfg>(sc, path, tr);
    }
    sum = rt_v3d_add(sum, path.radiance);
}
#else
struct RtPwView;
#endif

extern "C" {

struct orcflat_cam_bg { RtCamera cam; RtV3 bg; uint32_t root, pad; };

} /* extern "C" */

/* the kernels' work decomposition over a scene view: chunk partial sums, then resolve.  `pw` (with variant 5): the pair-walk form,
 * `pw_stack` stack entries per lane; nullptr: the one-entry-per-step walk.  0, -2 a traversal stack overflowed, -3 an index of the
 * pair walk left its stack or queue */
static int render_view(const RtSceneView& sc, const RtPwView* pw, uint32_t pw_stack, const RtFrame* frame, int variant, int out_sum, int threads,
                       rt_f64* out, uint64_t* segments_out, uint32_t* max_stack_out) {
#if defined(RT_RNG_REFSTREAM)
    if (pw) return -1;
#endif
    RtFrame f = *frame;
    if (f.chunk == 0 || f.chunk > f.spp) f.chunk = f.spp;
    f.n_chunks = (f.spp + f.chunk - 1u) / f.chunk;
    const uint64_t npix = (uint64_t)f.tile_w * f.tile_h;
    std::atomic<uint64_t> next(0), seg_total(0);
    std::atomic<uint32_t> max_stack(0);
    std::atomic<int> bad(0);
    auto worker = [&]() {
        HostStack stk;
#if !defined(RT_RNG_REFSTREAM)
        PwMem pwmem(pw ? pw_stack : 1u);
#endif
        uint64_t segs = 0;
        for (;;) {
            uint64_t p = next.fetch_add(1);
            if (p >= npix) break;
            uint32_t px = (uint32_t)(p % f.tile_w), py = (uint32_t)(p / f.tile_w);
            RtV3d total = rt_v3d(0.0, 0.0, 0.0);
            RtPath path;
            for (uint32_t c = 0; c < f.n_chunks; ++c) {
                uint32_t s = c * f.chunk;
                uint32_t s_end = s + f.chunk < f.spp ? s + f.chunk : f.spp;
                RtV3d sum = rt_v3d(0.0, 0.0, 0.0);
                for (; s < s_end; ++s) {
#if !defined(RT_RNG_REFSTREAM)
                    if (pw && variant == 5) { run_path_pw(sc, *pw, f, px, py, s, stk, pwmem, sum, segs, path); continue; }
#endif
                    switch (variant) { /* the same feature-specialised variants the GPU library builds */
                        case 0: run_path<RtCfgV0>(sc, f, px, py, s, stk, sum, segs, path); break;
                        case 1: run_path<RtCfgV1>(sc, f, px, py, s, stk, sum, segs, path); break;
                        case 2: run_path<RtCfgV2>(sc, f, px, py, s, stk, sum, segs, path); break;
                        case 4: run_path<RtCfgV4>(sc, f, px, py, s, stk, sum, segs, path); break;
                        case 5: run_path<RtCfgV5>(sc, f, px, py, s, stk, sum, segs, path); break;
#ifdef ORC_STATIC_CASES
                        ORC_STATIC_CASES
#endif
                        default: run_path<RtCfgV3>(sc, f, px, py, s, stk, sum, segs, path); break;
                    }
                }
                total = rt_v3d(total.x + sum.x, total.y + sum.y, total.z + sum.z);
            }
            if (!out_sum) total = into_sampled64(total, f.spp);
            out[p * 3 + 0] = total.x; out[p * 3 + 1] = total.y; out[p * 3 + 2] = total.z;
        }
        seg_total += segs;
        uint32_t m = (uint32_t)stk.max_sp, cur = max_stack.load();
        while (m > cur && !max_stack.compare_exchange_weak(cur, m)) {}
        if (stk.overflow) bad = 1;
#if !defined(RT_RNG_REFSTREAM)
        if (pwmem.fault) bad = 2;
#endif
    };
    if (threads < 1) threads = 1;
    std::vector<std::thread> pool;
    for (int t = 1; t < threads; ++t) pool.emplace_back(worker);
    worker();
    for (auto& t : pool) t.join();
    if (segments_out) *segments_out = seg_total.load();
    if (max_stack_out) *max_stack_out = max_stack.load();
    return bad.load() == 2 ? -3 : bad.load() ? -2 : 0;
}

extern "C" {

/* arrays are the bytes of rt1w_scene_copy_flat selectors 0..6 */
int orcflat_render(const void* nodes, uint32_t n_nodes, const void* lights, uint32_t n_lights, const void* materials,
                   uint32_t n_materials, const void* textures, uint32_t n_textures, const void* perlin, const void* images,
                   const void* cam_bg, const RtFrame* frame, int variant, int out_sum, int threads, rt_f64* out,
                   uint64_t* segments_out, uint32_t* max_stack_out) {
    RtSceneView sc;
    std::memset(&sc, 0, sizeof sc);
    const orcflat_cam_bg* cb = (const orcflat_cam_bg*)cam_bg;
    sc.nodes = (const RtNode*)nodes; sc.lights = (const RtNode*)lights;
    sc.materials = (const RtMaterial*)materials; sc.textures = (const RtTexture*)textures;
    sc.perlin = (const RtPerlin*)perlin; sc.images = (const uint8_t*)images;
    sc.root = cb->root; sc.n_nodes = n_nodes; sc.n_lights = n_lights; sc.n_materials = n_materials; sc.n_textures = n_textures;
    sc.camera = cb->cam; sc.background = cb->bg;
    return render_view(sc, nullptr, 0u, frame, variant, out_sum, threads, out, segments_out, max_stack_out);
}

/* 1: built with -DRT_RNG_REFSTREAM (the reference's ChaCha12 stream per pixel; include/rt1w_num.h) */
int orcflat_is_refstream(void) {
#ifdef RT_RNG_REFSTREAM
    return 1;
#else
    return 0;
#endif
}
/* number of compile-time topologies built in as variants 100.. (0 in the ordinary build) */
int orcflat_n_static(void) {
#ifdef ORC_N_STATIC
    return ORC_N_STATIC;
#else
    return 0;
#endif
}
uint64_t orcflat_item_count(const RtFrame* f) { return rt_item_count(*f); }
void orcflat_item_decode(const RtFrame* f, uint64_t item, uint32_t out[3]) { rt_item_decode(*f, item, out[0], out[1], out[2]); }
uint32_t orcflat_sizeof(int what) {
    switch (what) { case 0: return sizeof(RtNode); case 1: return sizeof(RtMaterial); case 2: return sizeof(RtTexture);
                    case 3: return sizeof(RtPerlin); case 4: return sizeof(RtCamera); case 5: return sizeof(RtFrame); default: return 0; }
}

/* rt_rng_mark / rt_rng_rewind (include/rt1w_num.h): after `before` mixed draws the stream is marked, `n` words are drawn into
 * out_a, the stream is rewound to the mark and the same `n` words drawn into out_b: they must be equal.  Bit i of `pattern`
 * picks a 32-bit (0) or 64-bit (1) draw for draw i (mod 32).  Built for the Philox streams and, in liborc_flat_ref.so, for
 * the reference's ChaCha12 stream. */
void orcflat_rng_rewind_check(uint64_t seed, uint32_t pattern, uint32_t before, uint32_t n, uint64_t* out_a, uint64_t* out_b) {
    RtRng r = rt_rng_pixel_sample(seed, 3u, 7u);
    for (uint32_t i = 0; i < before; ++i) { if ((pattern >> (i & 31u)) & 1u) (void)rt_next_u64(r); else (void)rt_next_u32(r); }
    const RtRngMark m = rt_rng_mark(r);
    for (uint32_t i = 0; i < n; ++i) out_a[i] = ((pattern >> ((i + before) & 31u)) & 1u) ? rt_next_u64(r) : (uint64_t)rt_next_u32(r);
    rt_rng_rewind(r, m);
    for (uint32_t i = 0; i < n; ++i) out_b[i] = ((pattern >> ((i + before) & 31u)) & 1u) ? rt_next_u64(r) : (uint64_t)rt_next_u32(r);
}

} /* extern "C" */

/* The walk over the WALK TABLE (rt_walk_table.h; rt_core.h: RtWalkNodes) on the CPU, ray by ray, against the walk over the node array.
 * `rays[n][8]` = origin, direction, time, unused; `visits` (n_nodes counts, may be NULL) ranks the table as the context's visit count
 * does -- tests hand in arbitrary counts: whatever the ranking, every ray must report the same t, primitive and scope and leave the
 * random stream (media draw inside the walk) in the same state.  `nc` = how many records the "cache" holds (the walk reads record v from
 * one array below nc and from the other above: any value must do).  variant 3 = the general media walk, 103 = the sphere-media build.
 * out_flags per ray: bit 0 the two walks differ, bit 1 a stack overflowed.  Returns 0, -1 if the table cannot be built. */
extern "C" int orcflat_walk_table_check(const void* nodes_, uint32_t n_nodes, uint32_t root, const uint32_t* visits, uint32_t nc, int variant,
                                        const double* rays, uint64_t n, double* out_t, uint32_t* out_prim, uint32_t* out_scope, uint32_t* out_flags,
                                        uint32_t* id_of_out) {
    const RtNode* nodes = (const RtNode*)nodes_;
    std::vector<RtNode> N(nodes, nodes + n_nodes);
    RtWalkTable T;
    std::string why;
    if (!rt_walk_table_build(N, root, visits, T, why)) return -1;
    if (id_of_out) std::memcpy(id_of_out, T.id_of.data(), (size_t)n_nodes * 4u);
    RtSceneView sc;
    std::memset(&sc, 0, sizeof sc);
    sc.nodes = nodes; sc.root = root; sc.n_nodes = n_nodes;
    std::vector<RtNodeHot> head(T.rec.begin(), T.rec.begin() + (nc < n_nodes ? nc : n_nodes)); /* a separate copy, as the LDS is */
    RtWalkNodes wn; wn.lds = head.data(); wn.glob = T.rec.data(); wn.nc = (uint32_t)head.size();
    RtGlobalNodes gn{nodes};
    for (uint64_t i = 0; i < n; ++i) {
        RtRay r;
        r.o = rt_v3(rays[i * 8 + 0], rays[i * 8 + 1], rays[i * 8 + 2]); r.d = rt_v3(rays[i * 8 + 3], rays[i * 8 + 4], rays[i * 8 + 5]); r.time = rays[i * 8 + 6];
        HostStack sa, sb;
        RtRng ra = rt_rng_pixel_sample(i, 5u, 9u), rb = ra;
        double ta = 0, tb = 0; uint32_t pa = RT_NONE, pb = RT_NONE, ca = RT_NONE, cb = RT_NONE;
        bool ha, hb;
        if (variant == 103) {
            ha = rt_traverse_stack<RtCfgSphereMedia<RtCfgV3>, true>(sc, gn, root, r, RT_R(0.001), RT_INF, ra, sa, ta, pa, ca);
            hb = rt_traverse_stack<RtCfgSphereMedia<RtCfgV3>, true>(sc, wn, 0u, r, RT_R(0.001), RT_INF, rb, sb, tb, pb, cb);
        } else {
            ha = rt_traverse_stack<RtCfgV3, true>(sc, gn, root, r, RT_R(0.001), RT_INF, ra, sa, ta, pa, ca);
            hb = rt_traverse_stack<RtCfgV3, true>(sc, wn, 0u, r, RT_R(0.001), RT_INF, rb, sb, tb, pb, cb);
        }
        uint32_t fl = 0;
        if (ha != hb || pa != pb || (ha && (std::memcmp(&ta, &tb, sizeof ta) != 0 || ca != cb)) || rt_next_u64(ra) != rt_next_u64(rb)) fl |= 1u;
        if (sa.overflow || sb.overflow || sb.max_sp > sa.max_sp) fl |= 2u; /* the table's walk needs no more stack than the node array's */
        out_t[i] = tb; out_prim[i] = hb ? pb : RT_NONE; out_scope[i] = hb ? cb : RT_NONE; out_flags[i] = fl;
    }
    return 0;
}

#if !defined(RT_RNG_REFSTREAM)
/* Every consumer of a uniform draw in the core, fed ONE chosen draw: the generator's buffer is loaded so that each 64-bit take returns
 * `bits` (all ones: the largest draw, 1 - 2^-53, which would round to 1.0f -- a value rand's own f32 shapes never return -- and which
 * the f32 build's draw contract, include/rt1w_num.h, makes 1 - 2^-24; 0: the smallest).  out[12], in 64 bits whatever the build: 0-2 rt_random_cosine_direction, 3-5 rt_random_to_sphere(0.5, 4),
 * 6 the light rectangle's coordinate in [213, 343), 7 the free flight -100 ln(r), 8 the draw as the Schlick test compares it,
 * 9-10 rt_random_in_unit_disk (first try from `bits`, further tries from the stream), 11 the shutter time in [0, 1) */
extern "C" void orcflat_draw_probe(uint64_t bits, rt_f64* out) {
    auto loaded = [bits]() {
        RtRng r = rt_rng_pixel_sample(1u, 2u, 3u);
        r.left = 4u; r.a0 = r.a2 = (uint32_t)bits; r.a1 = r.a3 = (uint32_t)(bits >> 32);
        return r;
    };
    RtRng r = loaded();
    RtV3 v = rt_random_cosine_direction(r);
    out[0] = v.x; out[1] = v.y; out[2] = v.z;
    r = loaded();
    v = rt_random_to_sphere(RT_R(0.5), RT_R(4.0), r);
    out[3] = v.x; out[4] = v.y; out[5] = v.z;
    const double x = rt_range_from_bits(bits, RT_R(213.0), RT_R(343.0));
    out[6] = x;
    r = loaded();
    const double flight = RT_R(-100.0) * rt_log(rt_take_f64(r));
    out[7] = flight;
    r = loaded();
    const double draw = rt_take_f64(r);
    out[8] = draw;
    r = loaded();
    v = rt_random_in_unit_disk(r);
    out[9] = v.x; out[10] = v.y;
    r = loaded();
    const double time = rt_take_range(r, RT_R(0.0), RT_R(1.0));
    out[11] = time;
}

/* The pair walk (rt_walk_pair.h) on the CPU, ray by ray, against the one-entry-per-step walk.  `rays[n][8]` = origin, direction, time, unused.
 * Each ray is walked as ONE lane would be by rt_render_ss_body / rt_render_plain_body -- the root's box, then box work and leaf work,
 * the NaN hand-overs (a NaN shutter fraction; a closest hit that turns NaN) -- under a RANDOM schedule (seeded): whether the lane does
 * box work or leaf work next, and how many inner records it takes on a box vote, is drawn; the exactness argument says the result may
 * not depend on it.  Stack (`stack_cap` entries) and queue (RT_PW_QCAP) are bound-checked.  out_flags per ray: bit 0 the segment was
 * handed to the classic walk, bit 1 an index left its array (a defect), bit 2 the ray missed the root box.  Returns 0, or -1 when the
 * scene is outside the pair walk's scope. */
extern "C" int orcflat_pair_walk(const void* nodes_, uint32_t n_nodes, uint32_t root, const double* rays, uint64_t n, uint32_t stack_cap,
                                 uint64_t schedule_seed, double* out_t, uint32_t* out_prim, double* ref_t, uint32_t* ref_prim, uint32_t* out_flags) {
    const RtNode* nodes = (const RtNode*)nodes_;
    std::vector<RtNode> N(nodes, nodes + n_nodes);
    std::vector<RtPwInner> inner;
    std::vector<RtPwGroup> groups;
    RtPwView pw;
    std::memset(&pw, 0, sizeof pw);
    std::string why;
    if (!rt_pw_build(N, root, inner, groups, pw, why)) return -1;
    pw.inner = inner.data(); pw.groups = groups.data();
    RtSceneView sc;
    std::memset(&sc, 0, sizeof sc);
    sc.nodes = nodes; sc.root = root; sc.n_nodes = n_nodes;
    RtGlobalNodes ns{nodes};
    uint64_t lcg = schedule_seed * 6364136223846793005ull + 1442695040888963407ull;
    auto draw = [&lcg]() { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(lcg >> 33); };
    for (uint64_t i = 0; i < n; ++i) {
        RtRay ray;
        ray.o = rt_v3(rays[i * 8], rays[i * 8 + 1], rays[i * 8 + 2]);
        ray.d = rt_v3(rays[i * 8 + 3], rays[i * 8 + 4], rays[i * 8 + 5]);
        ray.time = rays[i * 8 + 6];
        RtRng rng = rt_rng_pixel_sample(i, 0u, 0u); /* such a scene's walk draws nothing */
        uint32_t scope_;
        {   /* the reference answer: the one-entry-per-step walk */
            HostStack cs;
            double t = RT_INF; uint32_t prim = RT_NONE;
            rt_traverse_stack<RtCfgV5, true>(sc, ns, root, ray, RT_R(0.001), RT_INF, rng, cs, t, prim, scope_);
            ref_t[i] = t; ref_prim[i] = prim;
        }
        bool fault = false;
        RtPwLds<1, Checked<uint32_t>, Checked<float>, Checked<uint32_t>> m{{std::vector<uint32_t>(stack_cap), &fault}, {std::vector<float>(stack_cap), &fault},
                                                                             {std::vector<uint32_t>(RT_PW_QCAP), &fault}};
        RtPwLane L; L.cur = RT_PW_NONE; L.qh = 0u; L.qn = 0u; L.sp = 0;
        uint32_t flags = 0u;
        double best_t = RT_INF; uint32_t best_prim = RT_NONE;
        const double frac0 = (ray.time - pw.ms_time0) / (pw.ms_time1 - pw.ms_time0);
        bool bad = rt_isnan(frac0), walking = bad;
        const RtV3 inv = rt_inv3(ray.d);
        if (!bad) walking = rt_pw_begin(pw, L, m, ray.o, inv, RT_R(0.001));
        if (!walking) flags |= 4u;
        while (walking && !bad && !rt_pw_done(L) && !fault) {
            const bool can_box = rt_pw_can_box(L), can_leaf = L.qn > 0u;
            if (can_leaf && (!can_box || (draw() & 1u))) {
                rt_pw_group_step(pw, L, m, ray.o, ray.d, inv, frac0, RT_R(0.001), best_t, best_prim);
                if (rt_isnan(best_t)) bad = true;
            } else if (can_box) {
                const uint32_t steps = 1u + draw() % 6u;
                for (uint32_t k = 0; k < steps && rt_pw_can_box(L); ++k) rt_pw_box_step(pw, L, m, ray.o, inv, RT_R(0.001), best_t);
            } else { fault = true; } /* neither kind of work and not done: the state machine is stuck */
        }
        if (bad) { /* the hand-over of the kernels: the segment is redone by the one-entry-per-step walk */
            HostStack cs;
            best_t = RT_INF; best_prim = RT_NONE;
            rt_traverse_stack<RtCfgV5, true>(sc, ns, root, ray, RT_R(0.001), RT_INF, rng, cs, best_t, best_prim, scope_);
            flags |= 1u;
        }
        if (fault) flags |= 2u;
        out_t[i] = best_t; out_prim[i] = best_prim; out_flags[i] = flags;
    }
    return 0;
}
#endif

