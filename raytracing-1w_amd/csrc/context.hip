/* context.hip -- execution half of the C ABI: device context, the persistent-thread
 * render kernel and the resolve kernel.  gfx950 only.
 *
 * Kernel shape (replaces the rayon loop of src/main.rs:957-1001):
 *   - one lane owns one path at a time; a lane whose path ended regenerates in
 *     place (next sample of its work item, or a new work item), so lanes of a
 *     wave stay busy although path lengths differ (1..50 segments);
 *   - a work item = (pixel, chunk of `chunk` consecutive samples).  Items are
 *     handed out by one global counter; the first grid-size items are assigned
 *     statically, later ones by a wave-aggregated atomic (one atomic per wave per
 *     refill round: ballot + mbcnt prefix);
 *   - the pixel sum of a chunk lives in registers and is stored once
 *     (24 B per item, `partial[chunk][pixel]`); no floating-point atomics, so the
 *     summation order -- and therefore every bit of the result -- is fixed:
 *     sum over chunks in order of (sum over the chunk's samples in order);
 *   - the BVH traversal stack is per-lane in LDS, laid out [entry][lane] so that a
 *     wave's pushes/pops are bank-conflict free whatever depth each lane is at;
 *   - Philox4x32-10 state is 11 VGPRs (rt1w_num.h), nothing RNG-related in memory.
 */
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <new>

#include "context.h"
#include "jit.h"
#include "rt1w_internal.h"

/* The companion units' kernels come here as host handles (nullptr: no such kernel) and are launched like this unit's own.
 * context_ref.hip: the kernels built with the reference's own random stream (RT1W_RNG_REFERENCE), by mode (render_plan) */
extern "C" const void* rt1w_internal_ref_kernel(int mode);
extern "C" unsigned rt1w_internal_ref_sizeof(int what); /* bytes of its 0 RtSceneView, 1 RtFrame */
/* context_f32.hip: the kernels in single precision (RT1W_PRECISION_F32) and the f32 copies of the scene arrays */
extern "C" int rt1w_internal_f32_create(const void* nodes, uint32_t n_nodes, const void* lights, uint32_t n_lights, const void* materials,
                                        uint32_t n_materials, const void* textures, uint32_t n_textures, const void* perlin, uint32_t n_perlin,
                                        const void* view64, void** out);
extern "C" void rt1w_internal_f32_destroy(void* h);
extern "C" const void* rt1w_internal_f32_kernel(int variant, int mode); /* mode: 0 plain, 1 reordering, 2 pair walk (render_plan) */
extern "C" int rt1w_internal_f32_pw(void* h, unsigned stack_cap); /* 1: the scene has f32 pair-walk records and fits `stack_cap` entries */
extern "C" const void* rt1w_internal_f32_view(void* h, int what); /* the kernels' 0 f32 RtSceneView, 1 f32 RtPwView (nullptr: none) */
/* context_tiles.hip: the tile-list forms of the f64 kernels (rt1w_render_tiles), by walk form and variant as g_kernels below */
extern "C" const void* rt1w_internal_tile_kernel(int walk, int variant);
extern "C" const void* rt1w_internal_tile_pw_kernel(int which);  /* 0 pair walk, 1 pair walk + reordering */
extern "C" unsigned rt1w_internal_tile_sizeof(int what);         /* bytes of its 0 RtSceneView, 1 RtFrame, 2 RtPwView, 3 RtTileList */

/* context_rays.hip: the ray-list forms of the f64 kernels (rt1w_ray_color), indexed like the tile-list forms */
extern "C" const void* rt1w_internal_ray_kernel(int walk, int variant);
extern "C" const void* rt1w_internal_ray_pw_kernel(int which);
extern "C" unsigned rt1w_internal_ray_sizeof(int what);          /* bytes of its 0 RtSceneView, 1 RtFrame, 2 RtPwView, 3 RtRayList */

#include "rt_kernels.h"
#include "rt_walk_table.h"

namespace {

/* AABB slab test on the device, both forms, for tests: in[i] = {bb[6], o[3], d[3], t_min, t_max} */
__global__ void rt_debug_aabb_kernel(const double* in, int* out_literal, int* out_fast, unsigned long long n) {
    unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* p = in + i * 14;
    RtV3 o = rt_v3(p[6], p[7], p[8]);
    RtV3 inv = rt_inv3(rt_v3(p[9], p[10], p[11]));
    out_literal[i] = rt_aabb_hit(p, o, inv, p[12], p[13]) ? 1 : 0;
    const bool fe = rt_aabb_hit_fast<true>(p, o, inv, p[12], p[13]), fn = rt_aabb_hit_fast<false>(p, o, inv, p[12], p[13]);
    out_fast[i] = (fe == fn) ? (fe ? 1 : 0) : 2; /* 2: the two max/min forms disagree -- never equal to the literal's 0/1 */
}

__global__ void rt_debug_eval_kernel(int fn, const double* a, const double* b, double* out, unsigned long long n) {
    unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double x = a[i], y = b[i], r = 0.0;
    switch (fn) {
        case 0: r = x / y; break;
        case 1: r = rt_sqrt(rt_abs(x)); break;
        case 2: r = rt_sin(x); break;
        case 3: r = rt_cos(x); break;
        case 4: r = rt_acos(x / (rt_abs(x) + 1.0)); break;
        case 5: r = rt_atan2(x, y); break;
        case 6: r = rt_log(rt_abs(y)); break;
        case 7: { RtRng g = rt_rng_pixel_sample(i, (uint32_t)rt_d2u(x), 0u); r = rt_gen_f64(g); } break;
        case 8: { RtRng g = rt_rng_pixel_sample(i, (uint32_t)rt_d2u(x), 0u); (void)rt_gen_f64(g); r = rt_gen_range(g, -1.0, 1.0); } break;
        /* the same three draws on the stream of any 64-bit pixel seed (b's bits), and the loop-free (-1, 1) form the samplers use */
        case 11: { RtRng g = rt_rng_pixel_sample(rt_d2u(y), (uint32_t)rt_d2u(x), 0u); r = rt_gen_f64(g); } break;
        case 12: { RtRng g = rt_rng_pixel_sample(rt_d2u(y), (uint32_t)rt_d2u(x), 0u); (void)rt_gen_f64(g); r = rt_gen_range(g, -1.0, 1.0); } break;
        case 13: { RtRng g = rt_rng_pixel_sample(rt_d2u(y), (uint32_t)rt_d2u(x), 0u); (void)rt_gen_f64(g);
                   rt_rng_reserve(g, rt_rng_need_u64(g)); r = rt_take_pm1(g); } break;
#if defined(__HIP_DEVICE_COMPILE__)
        /* quotients of one divisor (rt1w_num.h): 14 the quotient x / y from the prepared divisor, 15 what the guards say of it (1 the
         * divisor is out of range, 2 the quotient is if it were used, 4 it is too large to be trusted at all), 16 the slab tests' 1 / y */
        case 14: r = rt_div_q(x, y, rt_div_prep(y)); break;
        case 15: { const double t = rt_div_q(x, y, rt_div_prep(y));
                   r = (double)((rt_div_d_ok(y) ? 0 : 1) | (rt_div_q_bad(t, true) ? 2 : 0) | (rt_div_q_big(t) ? 4 : 0)); } break;
        case 16: r = rt_div_inv(y, rt_div_prep(y)); break;
#endif
        default: break;
    }
    out[i] = r;
}

} // namespace

namespace rt1w {
bool hip_ok(hipError_t e, const char* what) {
    if (e == hipSuccess) return true;
    rt1w::set_error(std::string(what) + ": " + hipGetErrorString(e));
    return false;
}
int validate(const rt1w_context* c, const rt1w_render_params* p) {
    const char* why = "null argument";
    const int rc = (c && p) ? params_check(p, &why) : RT1W_ERR_INVALID;
    if (rc < 0) set_error(why);
    return rc;
}
int dev_grow(void** p, size_t* have, size_t need, const char* what) {
    if (need <= *have) return RT1W_OK;
    if (*p) (void)hipFree(*p);
    *p = nullptr; *have = 0;
    if (!hip_ok(hipMalloc(p, need), what)) return RT1W_ERR_NOMEM;
    *have = need;
    return RT1W_OK;
}
double lane_ms(const RtLane& l) {
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, l.ev0, l.ev1);
    return ms;
}
int forced_variant(const rt1w_context* c, uint32_t flags, bool allow_v4, int* v) {
    if (!((flags >> 8) & 0xFFu)) return RT1W_OK;
    *v = (int)((flags >> 8) & 0xFFu) - 1;
    if ((*v == 4 && !allow_v4) || !rt_variant_valid(*v, c->n_nodes, c->has_media, c->has_tex, c->has_msphere, c->scope_depth)) {
        rt1w::set_error("forced kernel variant does not cover this scene's features"); return RT1W_ERR_INVALID;
    }
    return RT1W_OK;
}
} // namespace rt1w
using namespace rt1w;

/* the rt1w_stats.sorted bits (include/rt1w.h) a kernel reports; bit 3, the wavefront form, is filled by wavefront.hip */
enum : uint32_t {
    RT_BIT_SORTED = 1u, RT_BIT_LDS_NODES = 2u, RT_BIT_JIT = 4u, RT_BIT_REF = 16u, RT_BIT_F32 = 32u, RT_BIT_PW = 128u, RT_BIT_SPHERE_MEDIA = 256u,
    RT_BIT_SS = 512u, RT_BIT_HC = 1024u
};

/* The f64 render kernels by walk form (context.h: RtWalkForm) and variant; nullptr: not built for that variant. */
typedef void (*render_kernel_t)(RtSceneView, RtFrame, double*, unsigned long long*);
static render_kernel_t const g_kernels[RT_N_WALKS][RT_N_VARIANTS] = {
    {rt_render_kernel<RtCfgV0>, rt_render_kernel<RtCfgV1>, rt_render_kernel<RtCfgV2>, rt_render_kernel<RtCfgV3>, rt_render_kernel<RtCfgV4>,
     rt_render_kernel<RtCfgV5>},
    /* the stack variants with media */
    {nullptr, nullptr, nullptr, rt_render_kernel<RtCfgSphereMedia<RtCfgV3>>, rt_render_kernel<RtCfgSphereMedia<RtCfgV4>>, nullptr},
    /* the default of the stack-walk scenes they cover */
    {nullptr, nullptr, rt_render_kernel_ss<RtCfgV2, RT_SS_CAP, 3>, rt_render_kernel_ss<RtCfgV3, RT_SS_CAP, 3>, nullptr, rt_render_kernel_ss<RtCfgV5, RT_SS_CAP, 3>},
    {nullptr, nullptr, nullptr, rt_render_kernel_ss<RtCfgSphereMedia<RtCfgV3>, RT_SS_CAP, 3>, rt_render_kernel_ss<RtCfgSphereMedia<RtCfgV4>, RT_SS_CAP, 3>, nullptr},
    {nullptr, nullptr, rt_render_kernel_ss_hc<RtCfgV2>, rt_render_kernel_ss_hc<RtCfgV3>, nullptr, rt_render_kernel_ss_hc<RtCfgV5>},
    {nullptr, nullptr, nullptr, rt_render_kernel_ss_hc<RtCfgSphereMedia<RtCfgV3>>, rt_render_kernel_ss_hc<RtCfgSphereMedia<RtCfgV4>>, nullptr},
    /* measured on random_scene: 464 Mpaths/s (80 KB LDS -> 2 waves/SIMD) against 486 for the plain variant at 3 waves/SIMD */
    {nullptr, nullptr, rt_render_kernel<RtCfgV2, true>, rt_render_kernel<RtCfgV3, true>, nullptr, rt_render_kernel<RtCfgV5, true>},
    /* where it pays (measured): the sweep variants.  Stack variants: 0.55x (LDS for stack + exchange halves occupancy) */
    {rt_render_kernel_sorted<RtCfgV0>, rt_render_kernel_sorted<RtCfgV1>, nullptr, nullptr, nullptr, nullptr}};
static const struct { int block; uint32_t bits; } g_walks[RT_N_WALKS] = {
    {RT_BLOCK, 0u}, {RT_BLOCK, RT_BIT_SPHERE_MEDIA}, {RT_BLOCK, RT_BIT_SS}, {RT_BLOCK, RT_BIT_SS | RT_BIT_SPHERE_MEDIA},
    {RT_BLOCK, RT_BIT_SS | RT_BIT_HC}, {RT_BLOCK, RT_BIT_SS | RT_BIT_HC | RT_BIT_SPHERE_MEDIA}, {RT_BLOCK, RT_BIT_LDS_NODES}, {RT_SORT_BLOCK, RT_BIT_SORTED}};

namespace {

bool upload(void** dst, const void* src, size_t bytes) {
    *dst = nullptr;
    size_t alloc = bytes ? bytes : 16;
    if (!hip_ok(hipMalloc(dst, alloc), "hipMalloc(scene)")) return false;
    if (bytes && !hip_ok(hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice), "hipMemcpy(scene)")) return false;
    return true;
}

/* the node array with one spare (zeroed) record behind it (the fused walk requests record e + 1 together with record e), and behind
 * that, at RT_WT_OFFSET, room for the scene's walk table (rt_walk_table.h; written by build_walk_table once the visits are counted) */
bool upload_nodes(void** dst, const std::vector<RtNode>& nodes) {
    const size_t n = nodes.size();
    std::vector<unsigned char> buf(RT_WT_OFFSET(n) + n * sizeof(RtNodeHot), 0);
    if (n) memcpy(buf.data(), nodes.data(), n * sizeof(RtNode));
    return upload(dst, buf.data(), buf.size());
}

/* The walk table of a stack-walk scene (rt_walk_table.h), ranked by MEASURED visits: a 128 x 128 x 1 render of the scene's own camera
 * with a kernel that counts the node fetches (rt_visit_count_kernel: a few ms, once per context).  Which nodes the kernels keep in LDS
 * changes where a record is read from and nothing else -- a scene whose table cannot be built, or whose walk needs more stack than the
 * cached kernels have, simply keeps the kernels without the cache. */
static_assert(RT_SS_HC_RECORDS == (int)RT_WT_CACHE_MAX, "the kernels cache exactly the records the table ranks");
bool build_walk_table(rt1w_context* c, const std::vector<RtNode>& nodes, uint32_t root, uint32_t stack_need, std::string& why) {
    const uint32_t n = (uint32_t)nodes.size();
    if (n == 0u) { why = "no nodes"; return false; }
    if (stack_need > (uint32_t)RT_SS_HC_CAP) { why = "the walk needs more than RT_SS_HC_CAP stack entries"; return false; }
    uint32_t* d_visits = nullptr;
    std::vector<uint32_t> visits(n, 0u);
    if (!hip_ok(hipMalloc((void**)&d_visits, (size_t)n * 4u), "hipMalloc(visits)")) return false;
    bool ok = hip_ok(hipMemset(d_visits, 0, (size_t)n * 4u), "hipMemset(visits)");
    if (ok) {
        RtFrame f;
        memset(&f, 0, sizeof f);
        f.width = f.tile_w = 128u; f.height = f.tile_h = 128u; f.spp = 1u; f.max_depth = 50u; f.chunk = 1u; f.n_chunks = 1u;
        hipLaunchKernelGGL(rt_visit_count_kernel, dim3(64), dim3(256), 0, c->lane[0].stream, c->view, f, d_visits);
        ok = hip_ok(hipGetLastError(), "rt_visit_count_kernel") &&
             hip_ok(hipMemcpyAsync(visits.data(), d_visits, (size_t)n * 4u, hipMemcpyDeviceToHost, c->lane[0].stream), "hipMemcpy(visits)") &&
             hip_ok(hipStreamSynchronize(c->lane[0].stream), "hipStreamSynchronize(visits)");
    }
    (void)hipFree(d_visits);
    if (!ok) { why = "the visit count failed"; return false; }
    RtWalkTable T;
    if (!rt_walk_table_build(nodes, root, visits.data(), T, why)) return false;
    if (!hip_ok(hipMemcpy((unsigned char*)c->d_nodes + RT_WT_OFFSET(n), T.rec.data(), (size_t)n * sizeof(RtNodeHot), hipMemcpyHostToDevice), "hipMemcpy(walk table)")) {
        why = "upload failed"; return false;
    }
    c->walk_table_first = T.n_first;
    return true;
}

/* RT1W_PRECISION_F32: the f32 copies of the scene arrays, at the first f32 render */
int ensure_f32_scene(rt1w_context* c) {
    if (c->f32_scene) return RT1W_OK;
    if (c->tried_f32_scene) { rt1w::set_error("could not build the single-precision scene arrays"); return RT1W_ERR_DEVICE; }
    c->tried_f32_scene = true;
    if (rt1w_internal_f32_create(c->h_nodes.data(), (uint32_t)c->h_nodes.size(), c->h_lights.data(), (uint32_t)c->h_lights.size(),
                                 c->h_materials.data(), (uint32_t)c->h_materials.size(), c->h_textures.data(), (uint32_t)c->h_textures.size(),
                                 c->h_perlin.data(), (uint32_t)c->h_perlin.size(), &c->view, &c->f32_scene) != 0) {
        c->f32_scene = nullptr;
        rt1w::set_error("could not build the single-precision scene arrays"); return RT1W_ERR_DEVICE;
    }
    return RT1W_OK;
}

/* the shading-side leaf functions ON THE DEVICE, for known-answer tests of what no artefact of the reference pins:
 * mode 0 Texture::value(u, v, p) of texture `tex` (texture.rs:40-89); mode 1 Perlin::noise(p) and Perlin::turb(p, 7) of
 * Perlin table `tex` (perlin.rs:46-86); mode 2 sphere_uv(p) (math.rs:67-71).  in[i] = {u, v, p.x, p.y, p.z}. */
__global__ void rt_debug_texture_kernel(RtSceneView sc, int mode, uint32_t tex, const double* __restrict__ in, double* __restrict__ out, unsigned long long n) {
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double u = in[i * 5], v = in[i * 5 + 1];
    const RtV3 p = rt_v3(in[i * 5 + 2], in[i * 5 + 3], in[i * 5 + 4]);
    RtV3 r = rt_v3(0.0, 0.0, 0.0);
    if (mode == 0) r = rt_texture<RtCfgV1>(sc, tex, u, v, p);
    else if (mode == 1) { r.x = rt_perlin_noise(sc.perlin[tex], p); r.y = rt_perlin_turb(sc.perlin[tex], p, 7); }
    else { double uu, vv; rt_sphere_uv(p, uu, vv); r.x = uu; r.y = vv; }
    out[i * 3] = r.x; out[i * 3 + 1] = r.y; out[i * 3 + 2] = r.z;
}

__global__ void rt_init_counters_kernel(unsigned long long* ctr, unsigned long long next_item, uint32_t keep_segments) { ctr[0] = next_item; if (!keep_segments) ctr[1] = 0ull; }

bool lane_init(RtLane& l) {
    if (l.stream) return true;
    /* ordinary (blocking) streams: ordered after work the caller queued on the null stream, e.g. on the tensor handed to
     * rt1w_render_device; the two lanes still run concurrently with each other */
    return hip_ok(hipStreamCreate(&l.stream), "hipStreamCreate") &&
           hip_ok(hipEventCreate(&l.ev0), "hipEventCreate") && hip_ok(hipEventCreate(&l.ev1), "hipEventCreate") &&
           hip_ok(hipMalloc((void**)&l.d_counters, 2 * sizeof(unsigned long long)), "hipMalloc(counters)") &&
           hip_ok(hipHostMalloc((void**)&l.h_counters, 2 * sizeof(unsigned long long), hipHostMallocDefault), "hipHostMalloc(counters)");
}
void lane_destroy(RtLane& l) {
    if (l.d_partial) (void)hipFree(l.d_partial);
    if (l.d_counters) (void)hipFree(l.d_counters);
    if (l.h_counters) (void)hipHostFree(l.h_counters);
    if (l.d_strip) (void)hipFree(l.d_strip);
    if (l.h_strip) (void)hipHostFree(l.h_strip);
    if (l.ev0) (void)hipEventDestroy(l.ev0);
    if (l.ev1) (void)hipEventDestroy(l.ev1);
    if (l.stream) (void)hipStreamDestroy(l.stream);
    l = RtLane();
}

#define RT_TILES_MAX (1u << 20) /* tiles of one rt1w_render_tiles list: the kernels carry a tile's index in 29 bits, the virtual tile's height is a uint32 */
#ifndef RT_PARTIAL_BUDGET
#define RT_PARTIAL_BUDGET (8ull << 30)
#endif
/* where a plan's kernel sits in the context: k64[i][v], pw_k[i], or neither; its tile-list form has the same index (tile_kernel_of) */
struct RtKernelAt { enum Table { NOWHERE, K64, PW } table = NOWHERE; int i = 0, v = 0; };
struct RtLaunch { RtFrame f; unsigned long long npix; unsigned long long partial_budget = RT_PARTIAL_BUDGET; int variant; RtKernel k; RtKernelAt at; RtTileArg tl; RtRayArg rl; };

/* the persistent grid of a kernel: as many workgroups as are resident at once, at least one per CU; 0, with the error set, if the
 * occupancy query failed */
int kernel_grid(const rt1w_context* c, const RtKernel& k) {
    int per_cu = 0;
    if (!hip_ok(k.jit ? hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k.jit, k.block, 0)
                      : hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k.fn, k.block, 0), "occupancy query")) return 0;
    return c->n_cu * (per_cu < 1 ? 1 : per_cu);
}

/* the kernels that are resolved at their first use (reference stream, f32): `slot` becomes `k` with its grid */
int first_use(const rt1w_context* c, RtKernel& slot, const RtKernel& k) {
    if (slot.grid) return RT1W_OK;
    if (!k.fn) { rt1w::set_error("no kernel of this mode for the scene's variant"); return RT1W_ERR_DEVICE; }
    const int grid = kernel_grid(c, k);
    if (!grid) return RT1W_ERR_DEVICE;
    slot = k; slot.grid = grid;
    return RT1W_OK;
}

/* the work-item size of a render with chunk 0 (include/rt1w.h: rt1w_scene_default_chunk): one sample per item on the stack-walk scenes,
 * except for the wavefront form, whose passes are per chunk */
uint32_t default_chunk(const rt1w_context* c, const rt1w_render_params* p) {
    return (c->variant >= 2 && !(p->flags & RT1W_WAVEFRONT)) ? 1u : rt1w_default_chunk(p->tile_w, p->tile_h, p->spp);
}

const RtKernel* specialised_lookup(rt1w_context* c, JitForm form);

/* the f32 kernel of (variant, mode): the product's own (context_f32.hip), unless librt1w_lab.so has registered a function that hands
 * out another build of the same kernel (rt1w_internal.h: rt1w_f32_kernel_fn; f32_exact.hip).  While that function answers, the
 * scene-specialised f32 kernel stands back too (mode 1 exists for every variant: the plan asks with it) */
static rt1w_f32_kernel_fn g_f32_kernel_of = nullptr;
const void* f32_kernel_of(int variant, int mode, bool& own) {
    const void* fn = g_f32_kernel_of ? g_f32_kernel_of(variant, mode) : nullptr;
    own = fn == nullptr;
    return own ? rt1w_internal_f32_kernel(variant, mode) : fn;
}

/* what the launch will need, without launching: frame, variant, kernel */
int render_plan(rt1w_context* c, const rt1w_render_params* p, RtLaunch& L) {
    RtFrame& f = L.f = frame_of(p);
    f.chunk = p->chunk ? p->chunk : default_chunk(c, p); /* the reference stream sets its own below */
    if (f.chunk > f.spp) f.chunk = f.spp;
    f.n_chunks = (f.spp + f.chunk - 1u) / f.chunk;
    L.npix = (unsigned long long)f.tile_w * f.tile_h;
    L.partial_budget = p->partial_mib ? ((unsigned long long)p->partial_mib << 20) : RT_PARTIAL_BUDGET;
    L.at = RtKernelAt();
    const uint32_t fl = p->flags;
    const bool forced = ((fl >> 8) & 0xFFu) != 0u;
    int rc;
    if (p->precision == RT1W_PRECISION_F32) {
        if (fl & (RT1W_RNG_REFERENCE | RT1W_WAVEFRONT | RT1W_LDS_NODES)) { rt1w::set_error("RT1W_PRECISION_F32 has the default kernels only"); return RT1W_ERR_INVALID; }
        if ((rc = ensure_f32_scene(c)) < 0) return rc;
        bool own = true;
        L.variant = c->variant == 4 ? 3 : c->variant; /* the order-aware variant exists in f64 only */
        if ((rc = forced_variant(c, fl, false, &L.variant)) < 0) return rc;
        (void)f32_kernel_of(L.variant, 1, own); /* own: the product's kernels serve, the scene-specialised one among them */
        /* a context that runs a scene-specialised kernel in f64 uses the f32 build of that kernel too -- from the kernel
         * caches only: renders never compile (rt1w_context_specialise does, for both precisions) */
        if (!(fl & (RT1W_GENERIC | RT1W_UNSORTED)) && !forced && c->jit[JIT_F64].k.jit && own)
            if (const RtKernel* k = specialised_lookup(c, JIT_F32)) { L.k = *k; return RT1W_OK; }
        /* mode 1: the reordering kernel of the sweep variants, the slice-end reordering of the stack walks; 2: sphere scenes' pair walk
         * (rt_walk_pair.h) in this precision too -- in the kernel that reorders the finished paths */
        const int v = L.variant;
        const int mode = (fl & RT1W_UNSORTED) ? 0
                       : (v == 5 && !(fl & RT1W_CLASSIC_WALK) && rt1w_internal_f32_pw(c->f32_scene, (unsigned)RT_PW_SS_STACK) == 1) ? 2 : 1;
        const uint32_t bits = RT_BIT_F32 | (mode == 2 ? RT_BIT_PW | RT_BIT_SS : mode == 1 ? (v >= 2 ? RT_BIT_SS : RT_BIT_SORTED) : 0u);
        const void* fn = f32_kernel_of(v, mode, own);
        RtKernel& slot = own ? c->k32[v][mode] : c->k32x[v][mode];
        if ((rc = first_use(c, slot, RtKernel::of(mode ? RT_SORT_BLOCK : RT_BLOCK, bits, fn).with_f32().with_pw(mode == 2))) < 0) return rc;
        L.k = slot;
        return RT1W_OK;
    }
    if (fl & RT1W_RNG_REFERENCE) {
        /* the reference's own stream: one lane owns a pixel for all its samples (main.rs:964-989) */
        if (p->sample_offset != 0u) { rt1w::set_error("RT1W_RNG_REFERENCE: one stream per pixel, sample_offset must be 0"); return RT1W_ERR_INVALID; }
        f.chunk = f.spp; f.n_chunks = 1u; f.global_seed = 0u;
        const bool stack_walk = c->n_nodes > RT_SWEEP_MAX_NODES;
        /* small scenes: through the workgroup-level path reordering (the stream's state travels with the path) unless RT1W_UNSORTED */
        const int mode = stack_walk ? 1 : ((fl & RT1W_UNSORTED) ? 0 : (c->variant == 0 ? 2 : 3));
        L.variant = stack_walk ? 3 : (mode == 2 ? 0 : 1);
        if (!c->ref[mode].grid && (rt1w_internal_ref_sizeof(0) != sizeof(RtSceneView) || rt1w_internal_ref_sizeof(1) != sizeof(RtFrame))) {
            rt1w::set_error("reference-stream kernels built against another scene layout"); return RT1W_ERR_DEVICE;
        }
        if ((rc = first_use(c, c->ref[mode], RtKernel::of(mode >= 2 ? RT_SORT_BLOCK : RT_BLOCK, RT_BIT_REF | (mode >= 2 ? RT_BIT_SORTED : 0u), rt1w_internal_ref_kernel(mode)))) < 0) return rc;
        L.k = c->ref[mode];
        return RT1W_OK;
    }
    L.variant = c->variant;
    if ((rc = forced_variant(c, fl, true, &L.variant)) < 0) return rc;
    const int v = L.variant;
    if (c->jit[JIT_F64].k.jit && !(fl & (RT1W_GENERIC | RT1W_UNSORTED | RT1W_LDS_NODES)) && !forced) { L.k = c->jit[JIT_F64].k; return RT1W_OK; }
    /* sphere scenes: the pair walk (same frames, bit for bit), unless the caller asks for the one-entry-per-step walk */
    if (c->pw_k[0].grid && v == 5 && !(fl & (RT1W_CLASSIC_WALK | RT1W_LDS_NODES | RT1W_WAVEFRONT))) {
        L.at.table = RtKernelAt::PW; L.at.i = c->pw_k[1].grid && !(fl & RT1W_UNSORTED) ? 1 : 0;
        L.k = c->pw_k[L.at.i];
        return RT1W_OK;
    }
    auto built = [&](int w) { return c->k64[w][v].grid > 0; };
    int w;
    if (built(RT_WALK_SORTED) && !(fl & RT1W_UNSORTED)) w = RT_WALK_SORTED;
    else if (built(RT_WALK_LDS_NODES) && c->n_nodes <= RT_LDS_NODE_CAP && (fl & RT1W_LDS_NODES)) w = RT_WALK_LDS_NODES;
    else {
        const int sm = (c->sphere_media && built(RT_WALK_SPHERE_MEDIA) && !(fl & RT1W_CLASSIC_WALK)) ? 1 : 0;
        w = RT_WALK_PLAIN + sm;
        if (built(RT_WALK_SS + sm) && !(fl & RT1W_UNSORTED))
            w = (built(RT_WALK_SS_HC + sm) && !(fl & RT1W_NO_NODE_CACHE)) ? RT_WALK_SS_HC + sm : RT_WALK_SS + sm;
    }
    L.at.table = RtKernelAt::K64; L.at.i = w; L.at.v = v;
    L.k = c->k64[w][v];
    return RT1W_OK;
}

/* chunk partial sums: [chunk][pixel][3] f64.  A render whose partial sums would exceed this budget runs as several PASSES over
 * consecutive chunk ranges (= sample ranges): every pass is one launch of the persistent kernel into the same buffer, and the resolve
 * kernel adds the pass's chunks to the running pixel sums in order -- the same additions in the same order as one pass, so the same
 * bits whatever the budget (one sample per work item on a big frame at 10 000 spp would otherwise need 150 GB) */
uint32_t chunks_per_pass(const RtLaunch& L, unsigned long long bytes = RT_PARTIAL_BUDGET) {
    const unsigned long long per_chunk = L.npix * 3ull * sizeof(double);
    unsigned long long n = per_chunk ? bytes / per_chunk : 1ull;
    if (n < 1ull) n = 1ull;
    return n >= L.f.n_chunks ? L.f.n_chunks : (uint32_t)n;
}

int lane_reserve_partial(RtLane& l, const RtLaunch& L) {
    return dev_grow((void**)&l.d_partial, &l.partial_bytes, (size_t)L.npix * chunks_per_pass(L, L.partial_budget) * 3 * sizeof(double), "hipMalloc(partial sums)");
}

/* the chunk sums of `n_chunks` chunks into the pixels of `out` (rt_resolve_kernel: carry bit 0 adds to earlier passes, bit 1 keeps raw sums) */
void launch_resolve(hipStream_t stream, const double* partial, double* out, unsigned long long npix, uint32_t n_chunks, uint32_t spp,
                    const rt1w_render_params* p, uint32_t carry) {
    const unsigned int rb = 256;
    hipLaunchKernelGGL(rt_resolve_kernel, dim3((unsigned int)((npix + rb - 1) / rb)), dim3(rb), 0, stream, partial, out, npix, n_chunks, spp,
                       (p->flags & RT1W_OUT_SUM) ? 1u : 0u, carry);
}

/* enqueue on the lane's stream: counters, trace kernel, resolve into d_out, counters back to pinned memory.  No host wait. */
int render_launch(rt1w_context* c, RtLane& l, const rt1w_render_params* p, const RtLaunch& L, double* d_out) {
    const RtKernel& k = L.k;
    /* the kernel's arguments: its scene view, the pair-walk view of the same precision where it takes one, frame, partial sums, counters */
    const void* view = k.f32 ? rt1w_internal_f32_view(c->f32_scene, 0) : &c->view;
    const void* pw = k.f32 ? rt1w_internal_f32_view(c->f32_scene, 1) : &c->pw;
    if (!view || (k.pw && !pw)) { rt1w::set_error("single-precision scene missing"); return RT1W_ERR_DEVICE; }
    (void)hipEventRecord(l.ev0, l.stream);
    const uint32_t cpp = chunks_per_pass(L, l.partial_bytes < L.partial_budget ? l.partial_bytes : L.partial_budget); /* what the lane's buffer holds (lane_reserve_partial), within the caller's bound */
    const uint32_t n_pass = (L.f.n_chunks + cpp - 1u) / cpp;
    l.passes = n_pass;
    for (uint32_t pass = 0; pass < n_pass; ++pass) {
    /* this pass's chunks as a frame of their own: samples [c0 * chunk, ...) of the call, absolute sample indices through sample_offset */
    RtFrame PF = L.f;
    const uint32_t c0 = pass * cpp;
    PF.n_chunks = L.f.n_chunks - c0 < cpp ? L.f.n_chunks - c0 : cpp;
    PF.sample_offset = L.f.sample_offset + c0 * L.f.chunk;
    PF.spp = (L.f.spp - c0 * L.f.chunk < PF.n_chunks * L.f.chunk) ? L.f.spp - c0 * L.f.chunk : PF.n_chunks * L.f.chunk;
    hipLaunchKernelGGL(rt_init_counters_kernel, dim3(1), dim3(1), 0, l.stream, l.d_counters, (unsigned long long)k.grid * k.block, pass ? 1u : 0u);
    double* partial = l.d_partial;
    unsigned long long* counters = l.d_counters;
    RtTileArg tl = L.tl;
    RtRayArg rl = L.rl;
    void* args[6];
    int n = 0;
    args[n++] = const_cast<void*>(view);
    if (k.pw) args[n++] = const_cast<void*>(pw);
    args[n++] = &PF; args[n++] = &partial; args[n++] = &counters;
    if (k.rays) args[n++] = &rl;
    if (k.tiles) args[n++] = &tl; /* a pass's sample delta reaches every tile through PF.sample_offset, which the kernel adds to the tile's own */
    if (!hip_ok(k.jit ? hipModuleLaunchKernel(k.jit, (unsigned)k.grid, 1, 1, (unsigned)k.block, 1, 1, 0, l.stream, args, nullptr)
                      : hipLaunchKernel(k.fn, dim3(k.grid), dim3(k.block), args, 0, l.stream), "render kernel launch")) return RT1W_ERR_DEVICE;
    launch_resolve(l.stream, l.d_partial, d_out, L.npix, PF.n_chunks, L.f.spp, p, (pass ? 1u : 0u) | (pass + 1u < n_pass ? 2u : 0u));
    } /* passes */
    (void)hipEventRecord(l.ev1, l.stream);
    if (!hip_ok(hipGetLastError(), "kernel launch")) return RT1W_ERR_DEVICE;
    if (!hip_ok(hipMemcpyAsync(l.h_counters, l.d_counters, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, l.stream), "counter copy")) return RT1W_ERR_DEVICE;
    return RT1W_OK;
}

/* wait for everything enqueued on the lane and fill the stats of its last launch */
int render_finish(RtLane& l, const RtLaunch& L, rt1w_stats* stats) {
    if (!hip_ok(hipStreamSynchronize(l.stream), "render kernel")) return RT1W_ERR_DEVICE;
    if (stats) {
        stats->paths = L.npix * L.f.spp;
        stats->segments = l.h_counters[1];
        stats->kernel_ms = lane_ms(l);
        stats->chunk = L.f.chunk; stats->n_chunks = L.f.n_chunks;
        stats->grid = (uint32_t)L.k.grid; stats->block = (uint32_t)L.k.block;
        stats->variant = (uint32_t)L.variant; stats->sorted = L.k.bits;
        stats->passes = l.passes; stats->reserved = 0u;
    }
    return RT1W_OK;
}

/* How loading the scene-specialised kernel differs between its forms (jit.h: JitForm); load_specialised is the only reader.  There is
 * no column for "a cached object the driver refuses is compiled once more": that is `!optional`, since compiling again repeats a failure */
struct RtJitPolicy {
    const char* what;        /* the prefix of the form's error texts */
    bool views_f32;          /* takes the f32 scene's views: the RT_F32 build reads the f32 copies of the scene arrays */
    bool tile_list;          /* takes the tile list in last place: only this form's text has an RtTileList, whose sizeof is checked */
    bool block_from_bounds;  /* workgroup size = launch bound = sort domain: experiments build the f64 text for 512 or 128; f32 runs at RT_SORT_BLOCK like its twins */
    bool optional;           /* a by-product of the f64 form nobody asks for by name: honours RT1W_NO_JIT, a failed compile or load is remembered, not repeated */
};
static_assert(sizeof(rt1w_context::jit) / sizeof(RtJitSlot) == JIT_N_FORMS, "one slot per form");
static constexpr RtJitPolicy g_jit_forms[JIT_N_FORMS] = {
    /*              what                            views_f32 tile_list block_from_bounds optional */
    /* JIT_F64   */ {"specialised kernel",           false,    false,    true,             false},
    /* JIT_F32   */ {"f32 specialised kernel",       true,     false,    false,            true},
    /* JIT_TILES */ {"tile-list specialised kernel", false,    true,     true,             false},
};

/* load one form of the specialised kernel of this context's scene: from the caches, or (allow_compile) from the compiler */
int load_specialised(rt1w_context* c, JitForm form, bool allow_compile, rt1w::JitInfo& info) {
    const RtJitPolicy& P = g_jit_forms[form];
    RtJitSlot& s = c->jit[form];
    if (s.k.jit) { info = rt1w::JitInfo(); info.key = s.key; info.from_cache = true; return RT1W_OK; }
    if (s.src.empty()) { rt1w::set_error("scene has more than RT_JIT_MAX_NODES nodes: no specialised kernel"); return RT1W_ERR_UNSUPPORTED; }
    const std::string what = P.what;
    if (P.optional && s.failed) { rt1w::set_error(what + ": " + s.error); return RT1W_ERR_DEVICE; }
    std::vector<char> code;
    int rc = rt1w::jit_get_code(s.src, allow_compile && !(P.optional && getenv("RT1W_NO_JIT")), code, info);
    s.key = info.key;
    if (rc < 0) {
        rt1w::set_error(what + ": " + info.message);
        if (P.optional && allow_compile) { s.failed = true; s.error = info.message; }
        return rc;
    }
    bool ok = hip_ok(hipModuleLoadData(&s.mod, code.data()), ("hipModuleLoadData(" + what + ")").c_str());
    if (!ok) s.mod = nullptr;
    if (!ok && info.from_cache && !P.optional) {
        /* a cached object the driver refuses (truncated, foreign toolchain): forget it and, if allowed, compile afresh */
        rt1w::jit_invalidate(info);
        if (!allow_compile) return RT1W_ERR_DEVICE;
        if ((rc = rt1w::jit_get_code(s.src, true, code, info, true)) < 0) { rt1w::set_error(what + ": " + info.message); return rc; }
        if (!(ok = hip_ok(hipModuleLoadData(&s.mod, code.data()), ("hipModuleLoadData(" + what + ")").c_str()))) s.mod = nullptr;
    }
    RtKernel k = RtKernel::of(RT_SORT_BLOCK, RT_BIT_SORTED | RT_BIT_JIT | (P.views_f32 ? RT_BIT_F32 : 0u)).with_f32(P.views_f32).with_tiles(P.tile_list);
    int max_threads = 0;
    ok = ok && hip_ok(hipModuleGetFunction(&k.jit, s.mod, "rt_jit_sorted"), ("hipModuleGetFunction(" + what + ")").c_str());
    if (ok && P.tile_list) {
        /* the unit's own RtTileList against the bytes render_launch will pass, as tile_kernel_of checks the built-in forms */
        hipDeviceptr_t dptr = nullptr;
        size_t bytes = 0;
        unsigned int theirs = 0u;
        ok = hip_ok(hipModuleGetGlobal(&dptr, &bytes, s.mod, "rt_jit_tile_list_bytes"), ("hipModuleGetGlobal(" + what + ")").c_str()) &&
             bytes == sizeof theirs && hip_ok(hipMemcpy(&theirs, dptr, sizeof theirs, hipMemcpyDeviceToHost), ("hipMemcpy(" + what + ")").c_str());
        if (ok && theirs != (unsigned int)sizeof(RtTileArg)) { rt1w::set_error(what + " built against another tile-list layout"); ok = false; }
    }
    if (ok && P.block_from_bounds && hipFuncGetAttribute(&max_threads, HIP_FUNC_ATTRIBUTE_MAX_THREADS_PER_BLOCK, k.jit) == hipSuccess &&
        (max_threads == 512 || max_threads == 128)) k.block = max_threads;
    if (ok) ok = (k.grid = kernel_grid(c, k)) > 0;
    if (!ok) {
        if (s.mod) (void)hipModuleUnload(s.mod);
        s.mod = nullptr;
        if (P.optional) {
            if (info.from_cache) rt1w::jit_invalidate(info);
            s.failed = true; s.error = rt1w_last_error();
        }
        return RT1W_ERR_DEVICE;
    }
    int vg = 0;
    if (hipFuncGetAttribute(&vg, HIP_FUNC_ATTRIBUTE_NUM_REGS, k.jit) == hipSuccess) s.vgprs = (uint32_t)vg;
    s.k = k;
    return RT1W_OK;
}

/* What a render may do about a form: the loaded kernel, or one look into the kernel caches per context and form, never the compiler.  A miss
 * is remembered and is no error: nullptr, a generic kernel runs, no HIP error of a refused object is left for the next launch check */
const RtKernel* specialised_lookup(rt1w_context* c, JitForm form) {
    RtJitSlot& s = c->jit[form];
    if (s.k.jit) return &s.k;
    if (s.consulted || s.src.empty()) return nullptr;
    s.consulted = true;
    rt1w::JitInfo info;
    if (load_specialised(c, form, false, info) == RT1W_OK) return &s.k;
    (void)hipGetLastError();
    return nullptr;
}

/* ---- wavefront form: lives in librt1w_lab.so (wavefront.hip), which registers itself here when it is loaded ---- */
static rt1w_wf_render_fn g_wf_render = nullptr;
static rt1w_wf_destroy_fn g_wf_destroy = nullptr;

int render_wavefront(rt1w_context* c, const rt1w_render_params* p, const RtLaunch& L, double* d_out, rt1w_stats* stats) {
    if (!g_wf_render) {
        rt1w::set_error("RT1W_WAVEFRONT: the wavefront form (a measured, slower opt-in) is part of librt1w_lab.so -- load that library, it registers itself");
        return RT1W_ERR_UNSUPPORTED;
    }
    RtLane& l = c->lane[0];
    rt1w_wf_call k;
    memset(&k, 0, sizeof k);
    k.device = c->device; k.view = &c->view; k.frame = &L.f; k.npix = L.npix; k.variant = L.variant;
    k.n_nodes = c->n_nodes; k.scope_depth = c->scope_depth; k.stack_need = c->stack_need;
    k.h_nodes = c->h_nodes.data(); k.n_h_nodes = (uint32_t)c->h_nodes.size();
    k.stream = (void*)l.stream; k.d_partial = l.d_partial; k.state = &c->wf_state; k.stats = stats;
    (void)hipEventRecord(l.ev0, l.stream);
    const int rc = g_wf_render(&k);                /* enqueues generate / trace / shade / finish / chunk sums on the lane's stream */
    if (rc < 0) return rc;
    launch_resolve(l.stream, l.d_partial, d_out, L.npix, L.f.n_chunks, L.f.spp, p, 0u);
    (void)hipEventRecord(l.ev1, l.stream);
    if (!hip_ok(hipGetLastError(), "kernel launch") || !hip_ok(hipStreamSynchronize(l.stream), "wavefront render")) return RT1W_ERR_DEVICE;
    if (stats) {
        stats->paths = L.npix * L.f.spp; stats->segments = k.h_segments ? *k.h_segments : 0ull; stats->kernel_ms = lane_ms(l);
        stats->chunk = L.f.chunk; stats->n_chunks = L.f.n_chunks;
        stats->passes = 1u; stats->reserved = 0u;
    }
    return RT1W_OK;
}

/* the tile-list form of the kernel a plan holds (from k64 / pw_k: the plan was made with RT1W_GENERIC), resolved at its first use */
int tile_kernel_of(rt1w_context* c, RtLaunch& L) {
    if (rt1w_internal_tile_sizeof(0) != sizeof(RtSceneView) || rt1w_internal_tile_sizeof(1) != sizeof(RtFrame) ||
        rt1w_internal_tile_sizeof(2) != sizeof(RtPwView) || rt1w_internal_tile_sizeof(3) != sizeof(RtTileArg)) {
        rt1w::set_error("tile-list kernels built against another scene layout"); return RT1W_ERR_DEVICE;
    }
    const RtKernelAt& at = L.at;
    RtKernel* const slot = at.table == RtKernelAt::PW ? &c->pw_kt[at.i] : at.table == RtKernelAt::K64 ? &c->kt[at.i][at.v] : nullptr;
    RtKernel want = L.k.with_tiles(); want.grid = 0;
    want.fn = at.table == RtKernelAt::PW ? rt1w_internal_tile_pw_kernel(at.i) : at.table == RtKernelAt::K64 ? rt1w_internal_tile_kernel(at.i, at.v) : nullptr;
    if (!slot || !want.fn) { rt1w::set_error("rt1w_render_tiles: the kernel this scene renders with has no tile-list form"); return RT1W_ERR_DEVICE; }
    const int rc = first_use(c, *slot, want);
    if (rc < 0) return rc;
    L.k = *slot;
    return RT1W_OK;
}

/* the ray-list form of the kernel a plan holds (from k64 / pw_k: the plan was made with RT1W_GENERIC), resolved at its first use */
int ray_kernel_of(rt1w_context* c, RtLaunch& L) {
    if (rt1w_internal_ray_sizeof(0) != sizeof(RtSceneView) || rt1w_internal_ray_sizeof(1) != sizeof(RtFrame) ||
        rt1w_internal_ray_sizeof(2) != sizeof(RtPwView) || rt1w_internal_ray_sizeof(3) != sizeof(RtRayArg)) {
        rt1w::set_error("ray-list kernels built against another scene layout"); return RT1W_ERR_DEVICE;
    }
    const RtKernelAt& at = L.at;
    RtKernel* const slot = at.table == RtKernelAt::PW ? &c->pw_kr[at.i] : at.table == RtKernelAt::K64 ? &c->kr[at.i][at.v] : nullptr;
    RtKernel want = L.k.with_rays(); want.grid = 0;
    want.fn = at.table == RtKernelAt::PW ? rt1w_internal_ray_pw_kernel(at.i) : at.table == RtKernelAt::K64 ? rt1w_internal_ray_kernel(at.i, at.v) : nullptr;
    if (!slot || !want.fn) { rt1w::set_error("rt1w_ray_color: the kernel this scene renders with has no ray-list form"); return RT1W_ERR_DEVICE; }
    const int rc = first_use(c, *slot, want);
    if (rc < 0) return rc;
    L.k = *slot;
    return RT1W_OK;
}

} // namespace

namespace rt1w {
int ray_color_common(rt1w_context* c, const rt1w_render_params* q, const RtRayArg& rays, double* d_out, rt1w_stats* stats) {
    RtLaunch L;
    int rc = render_plan(c, q, L); /* q: n x 1 pixels, RT1W_GENERIC: a kernel of k64 / pw_k, never the scene-specialised one */
    if (rc < 0) return rc;
    if ((rc = ray_kernel_of(c, L)) < 0) return rc;
    L.rl = rays;
    RtLane& l = c->lane[0];
    if ((rc = lane_reserve_partial(l, L)) < 0) return rc;
    if ((rc = render_launch(c, l, q, L, d_out)) < 0) return rc;
    return render_finish(l, L, stats);
}

int tiles_upload(rt1w_context* c, const rt1w_tile* tiles, uint32_t n_tiles, const uint32_t** d_rec) {
    static_assert(sizeof(rt1w_tile) == 16, "the kernels read a tile's record as four 32-bit words");
    const size_t bytes = (size_t)n_tiles * sizeof(rt1w_tile);
    /* a list that outgrows the buffer gets room to spare: 4096 bytes at least, otherwise twice its size */
    if (bytes > c->tiles_bytes && dev_grow(&c->d_tiles, &c->tiles_bytes, bytes < 4096 ? 4096 : bytes * 2, "hipMalloc(tile list)") < 0) return RT1W_ERR_NOMEM;
    /* nothing of an earlier call is in flight (every entry waits for the lane), so the list may be replaced now */
    if (!hip_ok(hipMemcpy(c->d_tiles, tiles, bytes, hipMemcpyHostToDevice), "tile list copy")) return RT1W_ERR_DEVICE;
    *d_rec = (const uint32_t*)c->d_tiles;
    return RT1W_OK;
}

int render_tiles_common(rt1w_context* c, const rt1w_render_params* p, uint32_t tile, const rt1w_tile* tiles, uint32_t n_tiles, double* d_out, rt1w_stats* stats) {
    if (!c || !p || !tiles || !d_out) { set_error("null argument"); return RT1W_ERR_INVALID; }
    if (p->width < 2 || p->height < 2) { set_error("width and height must be >= 2 (u,v divide by W-1, H-1; main.rs:968-969)"); return RT1W_ERR_INVALID; }
    if (p->spp == 0) { set_error("spp must be > 0"); return RT1W_ERR_INVALID; }
    if (p->precision == RT1W_PRECISION_F32) { set_error("rt1w_render_tiles: the tile-list kernels are f64 only"); return RT1W_ERR_UNSUPPORTED; }
    if (p->precision != RT1W_PRECISION_F64) { set_error("unknown precision"); return RT1W_ERR_UNSUPPORTED; }
    if (p->flags & ~(RT1W_OUT_SUM | RT1W_GENERIC | RT1W_TILES_SPECIALISED)) { set_error("rt1w_render_tiles: flags 0, RT1W_OUT_SUM or RT1W_GENERIC only"); return RT1W_ERR_INVALID; }
    if ((p->flags & RT1W_TILES_SPECIALISED) && (p->flags & RT1W_GENERIC)) { set_error("rt1w_render_tiles: RT1W_TILES_SPECIALISED and RT1W_GENERIC exclude each other"); return RT1W_ERR_INVALID; }
    if (p->strip_rows || p->strip_period) { set_error("rt1w_render_tiles takes no interleaved strips"); return RT1W_ERR_INVALID; }
    if (tile < 16u || tile > 256u || tile % 16u) { set_error("rt1w_render_tiles: tile must be a multiple of 16 in 16 .. 256"); return RT1W_ERR_INVALID; }
    if (n_tiles < 1u || n_tiles > RT_TILES_MAX) { set_error("rt1w_render_tiles: n_tiles must be 1 .. 2^20"); return RT1W_ERR_INVALID; }
    unsigned long long inside = 0ull;
    for (uint32_t k = 0; k < n_tiles; ++k) {
        const rt1w_tile& t = tiles[k];
        if (t.reserved != 0u || t.x0 % tile || t.y0 % tile || t.x0 >= p->width || t.y0 >= p->height) {
            set_error("rt1w_render_tiles: a tile's x0 and y0 must be multiples of `tile` inside the frame, its reserved member 0"); return RT1W_ERR_INVALID;
        }
        if ((unsigned long long)p->sample_offset + t.sample_offset + p->spp > 0xFFFFFFFFull) { set_error("sample index overflow"); return RT1W_ERR_INVALID; }
        inside += (unsigned long long)(p->width - t.x0 < tile ? p->width - t.x0 : tile) * (p->height - t.y0 < tile ? p->height - t.y0 : tile);
    }
    /* the list as ONE virtual tile of width `tile` and height n_tiles x tile, chunked as the WHOLE frame is.  The plan is the one of a
     * render with RT1W_GENERIC, whose kernel has a tile-list form in context_tiles.hip; with RT1W_TILES_SPECIALISED the tile-list form
     * of the scene-specialised kernel takes its place where a kernel cache has one (the same bits; never compiled here) */
    rt1w_render_params q = *p;
    q.x0 = 0u; q.y0 = 0u; q.tile_w = tile; q.tile_h = n_tiles * tile;
    q.flags = (q.flags & ~RT1W_TILES_SPECIALISED) | RT1W_GENERIC;
    if (!q.chunk) q.chunk = c->variant >= 2 ? 1u : rt1w_default_chunk(p->width, p->height, p->spp);
    RtLaunch L;
    int rc = render_plan(c, &q, L);
    if (rc < 0) return rc;
    const RtKernel* spec = (p->flags & RT1W_TILES_SPECIALISED) ? specialised_lookup(c, JIT_TILES) : nullptr;
    if (spec) L.k = *spec;
    else if ((rc = tile_kernel_of(c, L)) < 0) return rc;
    RtLane& l = c->lane[0];
    if ((rc = tiles_upload(c, tiles, n_tiles, &L.tl.rec)) < 0) return rc;
    L.tl.side = tile; L.tl.n = n_tiles;
    if ((rc = lane_reserve_partial(l, L)) < 0) return rc;
    if ((rc = render_launch(c, l, &q, L, d_out)) < 0) return rc;
    if ((rc = render_finish(l, L, stats)) < 0) return rc;
    if (stats) stats->paths = inside * p->spp; /* the pixels inside the frame: the others are not traced */
    return RT1W_OK;
}

int render_common(rt1w_context* c, const rt1w_render_params* p, double* d_out, rt1w_stats* stats) {
    /* a render this long repays the 1-8 s of the compiler: 2^35 paths where the gain is ~1.3x (scenes the generic sweep
     * handles), 2^32 where it is 1.5-2.3x (scenes the generic code hands to the stack walk).  RT1W_NO_JIT: never compile
     * behind the caller's back */
    if (!c->jit[JIT_F64].k.jit && !c->jit[JIT_F64].failed && !c->jit[JIT_F64].src.empty() && !(p->flags & (RT1W_GENERIC | RT1W_UNSORTED)) &&
        (unsigned long long)p->tile_w * p->tile_h * p->spp >= (c->n_nodes <= RT_SWEEP_MAX_NODES ? (1ull << 35) : (1ull << 32)) &&
        !getenv("RT1W_NO_JIT")) {
        rt1w::JitInfo info;
        if (load_specialised(c, JIT_F64, true, info) < 0) c->jit[JIT_F64].failed = true;
    }
    RtLaunch L;
    int rc = render_plan(c, p, L);
    if (rc < 0) return rc;
    RtLane& l = c->lane[0];
    if ((rc = lane_reserve_partial(l, L)) < 0) return rc;
    /* the wavefront form stands in for the generic f64 kernels other than the reordering kernel: with the flag the plan holds one of those,
     * the scene-specialised kernel (a reordering kernel too) or a reference-stream kernel */
    if ((p->flags & RT1W_WAVEFRONT) && !(L.k.bits & (RT_BIT_SORTED | RT_BIT_REF))) {
        if (chunks_per_pass(L, L.partial_budget) < L.f.n_chunks) { rt1w::set_error("RT1W_WAVEFRONT renders in one pass: its chunk partial sums must fit the budget (rt1w_render_params.partial_mib)"); return RT1W_ERR_UNSUPPORTED; }
        return render_wavefront(c, p, L, d_out, stats);
    }
    if ((rc = render_launch(c, l, p, L, d_out)) < 0) return rc;
    return render_finish(l, L, stats);
}

int reserve_out(rt1w_context* c, size_t bytes) { return dev_grow((void**)&c->d_out, &c->out_bytes, bytes, "hipMalloc(framebuffer)"); }
} // namespace rt1w

extern "C" {

int rt1w_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int rt1w_context_create(int device_id, const rt1w_scene* s, rt1w_context** out) {
    if (!s || !out) { rt1w::set_error("null argument"); return RT1W_ERR_INVALID; }
    if (!s->committed) { rt1w::set_error("scene not committed"); return RT1W_ERR_STATE; }
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        rt1w::set_error("no HIP device: librt1w has no CPU render path"); return RT1W_ERR_DEVICE;
    }
    if (device_id < 0 || device_id >= n) { rt1w::set_error("bad device id"); return RT1W_ERR_INVALID; }
    if (!hip_ok(hipSetDevice(device_id), "hipSetDevice")) return RT1W_ERR_DEVICE;
    rt1w_context* c = new (std::nothrow) rt1w_context();
    if (!c) { rt1w::set_error("out of memory"); return RT1W_ERR_NOMEM; }
    c->device = device_id;
    bool ok = lane_init(c->lane[0]) &&
              upload_nodes(&c->d_nodes, s->flat_nodes) &&
              upload(&c->d_lights, s->flat_lights.data(), s->flat_lights.size() * sizeof(RtNode)) &&
              upload(&c->d_materials, s->materials.data(), s->materials.size() * sizeof(RtMaterial)) &&
              upload(&c->d_textures, s->textures.data(), s->textures.size() * sizeof(RtTexture)) &&
              upload(&c->d_perlin, s->perlin.data(), s->perlin.size() * sizeof(RtPerlin)) &&
              upload(&c->d_images, s->images.data(), s->images.size());
    if (!ok) { rt1w_context_destroy(c); return RT1W_ERR_DEVICE; }
    RtSceneView& v = c->view = view_of(*s);
    v.nodes = (const RtNode*)c->d_nodes; v.lights = (const RtNode*)c->d_lights;
    v.materials = (const RtMaterial*)c->d_materials; v.textures = (const RtTexture*)c->d_textures;
    v.perlin = (const RtPerlin*)c->d_perlin; v.images = (const uint8_t*)c->d_images;
    hipDeviceProp_t prop;
    if (!hip_ok(hipGetDeviceProperties(&prop, device_id), "hipGetDeviceProperties")) { rt1w_context_destroy(c); return RT1W_ERR_DEVICE; }
    c->n_cu = prop.multiProcessorCount;
    c->has_media = s->has_media; c->has_tex = s->has_tex; c->has_msphere = s->has_msphere;
    c->sphere_media = s->has_media && s->media_bare_spheres;
    c->n_nodes = (uint32_t)s->flat_nodes.size();
    c->scope_depth = s->scope_depth;
    c->stack_need = s->stack_need;
    c->variant = rt_pick_variant(c->n_nodes, c->has_media, c->has_tex, c->has_msphere, c->scope_depth, s->walk_annotated != 0u);
    /* the walk table and the kernels that keep its head in LDS: what a stack-walk scene's renders run (sphere scenes run the pair
     * walk by default; the table serves their one-entry-per-step renders, RT1W_CLASSIC_WALK).  Built for every scene: a small
     * scene's renders with a forced stack-walk variant (tests) go through it as well */
    {
        std::string why;
        c->walk_table = build_walk_table(c, s->flat_nodes, s->flat_root, s->stack_need, why);
    }
    /* persistent grids of the f64 kernels: as many workgroups as are resident at once */
    for (int w = 0; w < RT_N_WALKS; ++w)
        for (int v = 0; v < RT_N_VARIANTS; ++v) {
            if (!g_kernels[w][v] || ((w == RT_WALK_SS_HC || w == RT_WALK_SS_HC_SPHERE_MEDIA) && !c->walk_table)) continue;
            RtKernel& k = c->k64[w][v];
            k = RtKernel::of(g_walks[w].block, g_walks[w].bits, reinterpret_cast<const void*>(g_kernels[w][v]));
            if (!(k.grid = kernel_grid(c, k))) { rt1w_context_destroy(c); return RT1W_ERR_DEVICE; }
        }
    if (c->variant == 5 && s->stack_need + 1u <= (uint32_t)RT_PW_STACK) {
        /* a sphere scene: records of the pair walk (rt_walk_pair.h); a scene outside its scope keeps the one-entry-per-step walk.  The
         * kernel that also reorders the finished paths needs a shallower tree */
        std::vector<RtPwInner> pin; std::vector<RtPwGroup> pgr;
        if (rt_pw_build(s->flat_nodes, s->flat_root, pin, pgr, c->pw, c->pw_why)) {
            const int n_pw = s->stack_need + 1u <= (uint32_t)RT_PW_SS_STACK ? 2 : 1;
            c->pw_k[0] = RtKernel::of(RT_BLOCK, RT_BIT_PW, reinterpret_cast<const void*>(rt_render_kernel_pw<RtCfgV5>)).with_pw();
            c->pw_k[1] = RtKernel::of(RT_BLOCK, RT_BIT_PW | RT_BIT_SS, reinterpret_cast<const void*>(rt_render_kernel_pw_ss<RtCfgV5>)).with_pw();
            if (!upload(&c->d_pw_inner, pin.data(), pin.size() * sizeof(RtPwInner)) || !upload(&c->d_pw_groups, pgr.data(), pgr.size() * sizeof(RtPwGroup))) {
                rt1w_context_destroy(c); return RT1W_ERR_DEVICE;
            }
            c->pw.inner = (const RtPwInner*)c->d_pw_inner; c->pw.groups = (const RtPwGroup*)c->d_pw_groups;
            for (int i = 0; i < n_pw; ++i)
                if (!(c->pw_k[i].grid = kernel_grid(c, c->pw_k[i]))) { rt1w_context_destroy(c); return RT1W_ERR_DEVICE; }
        }
    } else c->pw_why = "not a wrapper-free, media-free scene of more than 64 nodes, or its tree is deeper than the pair walk's stack";
    /* the opt-in modes' own data (f32 scene arrays, the wavefront form's walk records) are built at their first use:
     * ensure_f32_scene; the wavefront form's in librt1w_lab.so */
    c->h_nodes = s->flat_nodes; c->h_lights = s->flat_lights; c->h_materials = s->materials; c->h_textures = s->textures; c->h_perlin = s->perlin;
    if (rt1w::jit_eligible(*s)) {
        for (int form = 0; form < JIT_N_FORMS; ++form) c->jit[form].src = rt1w::jit_source(*s, (JitForm)form);
        rt1w::JitInfo info;
        (void)load_specialised(c, JIT_F64, false, info); /* a cache hit is used from the first render on, a miss costs nothing; the other forms: specialised_lookup */
    }
    *out = c;
    return RT1W_OK;
}

void rt1w_context_destroy(rt1w_context* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    void* bufs[] = {c->d_nodes, c->d_lights, c->d_materials, c->d_textures, c->d_perlin, c->d_images, c->d_out, c->dn_buf[0], c->dn_buf[1], c->dn_buf[2], c->d_batches, c->d_accum, c->d_tiles, c->tm_buf[0], c->tm_buf[1], c->tv_buf[0], c->tv_buf[1]};
    if (c->wf_state && g_wf_destroy) g_wf_destroy(c->wf_state);
    for (void* b : bufs) if (b) (void)hipFree(b);
    rt1w_internal_f32_destroy(c->f32_scene);
    if (c->d_pw_inner) (void)hipFree(c->d_pw_inner);
    if (c->d_pw_groups) (void)hipFree(c->d_pw_groups);
    lane_destroy(c->lane[0]);
    lane_destroy(c->lane[1]);
    for (RtJitSlot& j : c->jit) if (j.mod) (void)hipModuleUnload(j.mod);
    if (c->ev_first) (void)hipEventDestroy(c->ev_first);
    delete c;
}

int rt1w_context_specialise(rt1w_context* c, uint32_t flags, rt1w_specialise_info* out) {
    if (!c) { rt1w::set_error("null argument"); return RT1W_ERR_INVALID; }
    if (!hip_ok(hipSetDevice(c->device), "hipSetDevice")) return RT1W_ERR_DEVICE;
    const RtJitSlot& j64 = c->jit[JIT_F64];
    const bool had = j64.k.jit != nullptr;
    rt1w::JitInfo info; /* the f64 form's, with the compile time of the tile-list form */
    int rc = RT1W_OK;
    for (int form = 0; form < JIT_N_FORMS && rc == RT1W_OK; ++form) {
        /* f64: required.  f32: only beside a loaded f64 kernel, its failure is not the call's.  Tiles: when asked for, its failure is the call's */
        if (form == JIT_F32 ? !j64.k.jit : form == JIT_TILES && !(flags & RT1W_SPECIALISE_TILES)) continue;
        rt1w::JitInfo fi;
        const int r = load_specialised(c, (JitForm)form, !(flags & RT1W_SPECIALISE_CACHED_ONLY), fi);
        if (form == JIT_F32) continue;
        rc = r;
        if (form == JIT_F64) info = fi; else info.compile_ms += fi.compile_ms;
    }
    if (out) {
        memset(out, 0, sizeof *out);
        snprintf(out->key, sizeof out->key, "%s", j64.key.c_str());
        out->active = j64.k.jit ? 1u : 0u;
        out->from_cache = (had || info.from_cache) ? 1u : 0u;
        out->compile_ms = info.compile_ms;
        out->grid = (uint32_t)j64.k.grid; out->vgprs = j64.vgprs;
    }
    return rc;
}

int rt1w_render_device(rt1w_context* c, const rt1w_render_params* p, void* d_out_rgb, rt1w_stats* stats) {
    int rc = validate(c, p);
    if (rc < 0) return rc;
    if (!d_out_rgb) { rt1w::set_error("null output"); return RT1W_ERR_INVALID; }
    if (p->flags & RT1W_OUT_FRAME) { rt1w::set_error("RT1W_OUT_FRAME is a host-output mode (rt1w_render)"); return RT1W_ERR_INVALID; }
    if (!hip_ok(hipSetDevice(c->device), "hipSetDevice")) return RT1W_ERR_DEVICE;
    const RtTimer timer;
    rc = render_common(c, p, (double*)d_out_rgb, stats);
    if (rc == RT1W_OK && stats) stats->total_ms = timer.ms();
    return rc;
}

int rt1w_render_tiles_device(rt1w_context* c, const rt1w_render_params* p, uint32_t tile, const rt1w_tile* tiles, uint32_t n_tiles, void* d_out, rt1w_stats* stats) {
    if (c && !hip_ok(hipSetDevice(c->device), "hipSetDevice")) return RT1W_ERR_DEVICE;
    const RtTimer timer;
    const int rc = render_tiles_common(c, p, tile, tiles, n_tiles, (double*)d_out, stats);
    if (rc == RT1W_OK && stats) stats->total_ms = timer.ms();
    return rc;
}

int rt1w_render_tiles(rt1w_context* c, const rt1w_render_params* p, uint32_t tile, const rt1w_tile* tiles, uint32_t n_tiles, double* out, rt1w_stats* stats) {
    if (!c || !out) { rt1w::set_error("null argument"); return RT1W_ERR_INVALID; }
    if (tile > 256u || n_tiles > RT_TILES_MAX) { rt1w::set_error("rt1w_render_tiles: tile must be a multiple of 16 in 16 .. 256, n_tiles 1 .. 2^20"); return RT1W_ERR_INVALID; }
    if (!hip_ok(hipSetDevice(c->device), "hipSetDevice")) return RT1W_ERR_DEVICE;
    const RtTimer timer;
    const size_t bytes = (size_t)n_tiles * tile * tile * 3 * sizeof(double);
    int rc = reserve_out(c, bytes ? bytes : 16);
    if (rc < 0) return rc;
    if ((rc = render_tiles_common(c, p, tile, tiles, n_tiles, c->d_out, stats)) < 0) return rc;
    if (!hip_ok(hipMemcpy(out, c->d_out, bytes, hipMemcpyDeviceToHost), "tile copy")) return RT1W_ERR_DEVICE;
    if (stats) stats->total_ms = timer.ms();
    return RT1W_OK;
}

int rt1w_render_u8(rt1w_context* c, const rt1w_render_params* p, uint8_t* out_rgb8, rt1w_stats* stats) {
    int rc = validate(c, p);
    if (rc < 0) return rc;
    if (!out_rgb8) { rt1w::set_error("null output"); return RT1W_ERR_INVALID; }
    if (p->flags & RT1W_OUT_SUM) { rt1w::set_error("RT1W_OUT_SUM has no 8-bit form"); return RT1W_ERR_INVALID; }
    if ((p->flags & RT1W_OUT_FRAME) || p->strip_rows) { rt1w::set_error("rt1w_render_u8 takes contiguous tiles only"); return RT1W_ERR_INVALID; }
    if (!hip_ok(hipSetDevice(c->device), "hipSetDevice")) return RT1W_ERR_DEVICE;
    const RtTimer timer;
    size_t npix = (size_t)p->tile_w * p->tile_h;
    size_t bytes = npix * 3 * sizeof(double) + npix * 3; /* framebuffer + quantised image behind it */
    if ((rc = reserve_out(c, bytes)) < 0) return rc;
    rc = render_common(c, p, c->d_out, stats);
    if (rc < 0) return rc;
    uint8_t* d_u8 = reinterpret_cast<uint8_t*>(c->d_out + npix * 3);
    hipLaunchKernelGGL(rt_quantize_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, c->lane[0].stream, c->d_out, d_u8, p->tile_w, p->tile_h);
    if (!hip_ok(hipMemcpyAsync(out_rgb8, d_u8, npix * 3, hipMemcpyDeviceToHost, c->lane[0].stream), "quantised image copy") ||
        !hip_ok(hipStreamSynchronize(c->lane[0].stream), "quantise kernel")) return RT1W_ERR_DEVICE;
    if (stats) stats->total_ms = timer.ms();
    return RT1W_OK;
}

int rt1w_render_rows(rt1w_context* c, const rt1w_render_params* p, uint32_t strip_rows, int format, void* out,
                     rt1w_progress_fn progress, void* user, rt1w_stats* stats) {
    int rc = validate(c, p);
    if (rc < 0) return rc;
    if (!out) { rt1w::set_error("null output"); return RT1W_ERR_INVALID; }
    if (format != RT1W_ROWS_F64 && format != RT1W_ROWS_U8) { rt1w::set_error("unknown output format"); return RT1W_ERR_INVALID; }
    if (format == RT1W_ROWS_U8 && (p->flags & RT1W_OUT_SUM)) { rt1w::set_error("RT1W_OUT_SUM has no 8-bit form"); return RT1W_ERR_INVALID; }
    if ((p->flags & RT1W_OUT_FRAME) || p->strip_rows) { rt1w::set_error("rt1w_render_rows takes contiguous tiles only"); return RT1W_ERR_INVALID; }
    if (p->flags & RT1W_WAVEFRONT) { rt1w::set_error("rt1w_render_rows runs the persistent kernels only (RT1W_WAVEFRONT is a one-shot form)"); return RT1W_ERR_UNSUPPORTED; }
    if (!hip_ok(hipSetDevice(c->device), "hipSetDevice")) return RT1W_ERR_DEVICE;
    const RtTimer timer;
    const uint32_t H = p->tile_h, W = p->tile_w;
    const uint32_t tile_chunk = p->chunk ? p->chunk : default_chunk(c, p); /* the whole tile's chunking */
    if (strip_rows == 0) {
        /* about 16 strips, but never so thin that a strip has fewer than ~4M work items (pixel x sample chunk): the
         * persistent kernel needs that many to keep its tail short, and the chunking is the whole tile's by contract */
        const uint64_t n_chunks = (p->spp + (uint64_t)(tile_chunk < p->spp ? tile_chunk : p->spp) - 1u) / (tile_chunk < p->spp ? tile_chunk : p->spp);
        const uint64_t min_rows = ((4ull << 20) + (uint64_t)W * n_chunks - 1u) / ((uint64_t)W * n_chunks);
        uint64_t rows = (H + 15u) / 16u;
        if (rows < min_rows) rows = min_rows;
        rows = (rows + 7u) & ~7ull;
        strip_rows = rows > H ? H : (uint32_t)rows;
    }
    if (strip_rows > H) strip_rows = H;
    /* one strip: f64 means, and behind them the quantised bytes when asked for */
    const size_t strip_px = (size_t)strip_rows * W;
    const size_t f64_bytes = strip_px * 3 * sizeof(double);
    const size_t dev_bytes = f64_bytes + (format == RT1W_ROWS_U8 ? strip_px * 3 : 0);
    rt1w_render_params sp = *p;
    sp.chunk = tile_chunk; /* same sums, same bits */
    sp.tile_h = strip_rows;
    RtLaunch plan;
    if ((rc = render_plan(c, &sp, plan)) < 0) return rc;
    /* all allocation up front: hipMalloc/hipFree in the loop would serialise the two lanes */
    if (!c->ev_first && !hip_ok(hipEventCreate(&c->ev_first), "hipEventCreate")) return RT1W_ERR_DEVICE;
    for (int k = 0; k < 2; ++k) {
        RtLane& l = c->lane[k];
        if (!lane_init(l)) return RT1W_ERR_DEVICE;
        if ((rc = lane_reserve_partial(l, plan)) < 0) return rc;
        if (dev_bytes > l.strip_bytes) {
            if (l.d_strip) (void)hipFree(l.d_strip);
            if (l.h_strip) (void)hipHostFree(l.h_strip);
            l.d_strip = l.h_strip = nullptr; l.strip_bytes = 0;
            if (!hip_ok(hipMalloc(&l.d_strip, dev_bytes), "hipMalloc(strip)") ||
                !hip_ok(hipHostMalloc(&l.h_strip, dev_bytes, hipHostMallocDefault), "hipHostMalloc(strip)")) return RT1W_ERR_NOMEM;
            l.strip_bytes = dev_bytes;
        }
    }
    const uint32_t n_strips = (H + strip_rows - 1u) / strip_rows;
    struct Flight { RtLaunch L; uint32_t top, rows; } fl[2];
    rt1w_stats total; memset(&total, 0, sizeof total);
    uint32_t rows_done = 0;
    /* strip i goes to lane i & 1: trace, resolve, (quantise,) copy to the lane's pinned strip -- all on the lane's stream */
    auto launch = [&](uint32_t i) -> int {
        RtLane& l = c->lane[i & 1u];
        Flight& F = fl[i & 1u];
        F.top = i * strip_rows;
        F.rows = (H - F.top < strip_rows) ? H - F.top : strip_rows;
        sp.tile_h = F.rows;
        sp.y0 = p->y0 + (H - F.top - F.rows);
        int r = render_plan(c, &sp, F.L);
        if (r < 0) return r;
        if (i == 0) (void)hipEventRecord(c->ev_first, l.stream);
        if ((r = render_launch(c, l, &sp, F.L, (double*)l.d_strip)) < 0) return r;
        const uint8_t* src = (const uint8_t*)l.d_strip;
        const size_t npix = (size_t)F.rows * W;
        if (format == RT1W_ROWS_U8) {
            uint8_t* d_u8 = (uint8_t*)l.d_strip + f64_bytes;
            hipLaunchKernelGGL(rt_quantize_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, l.stream,
                               (const double*)l.d_strip, d_u8, W, F.rows);
            src = d_u8;
        }
        const size_t nbytes = format == RT1W_ROWS_U8 ? npix * 3 : npix * 3 * sizeof(double);
        if (!hip_ok(hipMemcpyAsync(l.h_strip, src, nbytes, hipMemcpyDeviceToHost, l.stream), "strip copy")) return RT1W_ERR_DEVICE;
        return RT1W_OK;
    };
    /* waits for strip i, lands it in the caller's buffer and reports it; > 0 = the callback asked to stop */
    auto land = [&](uint32_t i) -> int {
        RtLane& l = c->lane[i & 1u];
        Flight& F = fl[i & 1u];
        rt1w_stats st;
        int r = render_finish(l, F.L, &st);
        if (r < 0) return r;
        total.paths += st.paths; total.segments += st.segments;
        total.chunk = st.chunk; total.n_chunks = st.n_chunks; total.grid = st.grid; total.block = st.block;
        total.variant = st.variant; total.sorted = st.sorted; total.passes += st.passes;
        if (i + 1u == n_strips) { float ms = 0.f; (void)hipEventElapsedTime(&ms, c->ev_first, l.ev1); total.kernel_ms = ms; }
        if (format == RT1W_ROWS_U8) memcpy((uint8_t*)out + (size_t)F.top * W * 3, l.h_strip, (size_t)F.rows * W * 3);
        else memcpy((double*)out + (size_t)(H - F.top - F.rows) * W * 3, l.h_strip, (size_t)F.rows * W * 3 * sizeof(double));
        rows_done += F.rows;
        return (progress && progress(user, rows_done, H) != 0) ? 1 : 0;
    };
    if ((rc = launch(0)) < 0) return rc;
    for (uint32_t i = 0; i < n_strips; ++i) {
        if (i + 1u < n_strips && (rc = launch(i + 1u)) < 0) { (void)hipStreamSynchronize(c->lane[i & 1u].stream); return rc; }
        rc = land(i);
        if (rc != 0) {
            /* error or cancel: the strip already in flight on the other lane is left to finish, unreported */
            if (i + 1u < n_strips) (void)hipStreamSynchronize(c->lane[(i + 1u) & 1u].stream);
            if (rc < 0) return rc;
            if (i + 1u == n_strips) break; /* asked to stop after the last strip: nothing left to stop */
            rt1w::set_error("cancelled by the progress callback");
            return RT1W_ERR_CANCELLED;
        }
    }
    if (stats) {
        *stats = total; /* kernel_ms: first strip's start to last strip's end on the device (the strips overlap) */
        stats->total_ms = timer.ms();
    }
    return RT1W_OK;
}

int rt1w_render(rt1w_context* c, const rt1w_render_params* p, double* out_rgb, rt1w_stats* stats) {
    int rc = validate(c, p);
    if (rc < 0) return rc;
    if (!out_rgb) { rt1w::set_error("null output"); return RT1W_ERR_INVALID; }
    if (!hip_ok(hipSetDevice(c->device), "hipSetDevice")) return RT1W_ERR_DEVICE;
    const RtTimer timer;
    size_t bytes = (size_t)p->tile_w * p->tile_h * 3 * sizeof(double);
    if ((rc = reserve_out(c, bytes)) < 0) return rc;
    rc = render_common(c, p, c->d_out, stats);
    if (rc < 0) return rc;
    if (p->flags & RT1W_OUT_FRAME) {
        /* the tile's rows to their places in the caller's whole-image buffer: one copy per strip (a strip of full-width rows
         * is contiguous in both), queued on the stream, one wait */
        hipStream_t st = c->lane[0].stream;
        const size_t px = 3 * sizeof(double);
        const uint32_t srows = p->strip_rows ? p->strip_rows : p->tile_h;
        for (uint32_t r = 0; r < p->tile_h; r += srows) {
            const uint32_t rows = p->tile_h - r < srows ? p->tile_h - r : srows;
            const uint64_t j = p->strip_rows ? (uint64_t)p->y0 + (uint64_t)(r / srows) * p->strip_period : (uint64_t)p->y0 + r;
            double* dst = out_rgb + (j * p->width + p->x0) * 3u;
            const double* src = c->d_out + (size_t)r * p->tile_w * 3u;
            hipError_t e = (p->tile_w == p->width)
                ? hipMemcpyAsync(dst, src, (size_t)rows * p->tile_w * px, hipMemcpyDeviceToHost, st)
                : hipMemcpy2DAsync(dst, (size_t)p->width * px, src, (size_t)p->tile_w * px, (size_t)p->tile_w * px, rows, hipMemcpyDeviceToHost, st);
            if (!hip_ok(e, "framebuffer copy")) return RT1W_ERR_DEVICE;
        }
        if (!hip_ok(hipStreamSynchronize(st), "framebuffer copy")) return RT1W_ERR_DEVICE;
    } else if (!hip_ok(hipMemcpy(out_rgb, c->d_out, bytes, hipMemcpyDeviceToHost), "framebuffer copy")) return RT1W_ERR_DEVICE;
    if (stats) stats->total_ms = timer.ms();
    return RT1W_OK;
}

uint32_t rt1w_abi_sizeof(int what) {
    switch (what) {
        case 0: return (uint32_t)sizeof(rt1w_render_params);
        case 1: return (uint32_t)sizeof(rt1w_stats);
        case 2: return (uint32_t)sizeof(rt1w_scene_info);
        case 3: return (uint32_t)sizeof(rt1w_specialise_info);
        case 4: return (uint32_t)sizeof(rt1w_denoise_params);
        case 6: return (uint32_t)sizeof(rt1w_camera);
        case 8: return (uint32_t)sizeof(rt1w_ray_color_params);
        case 10: return (uint32_t)sizeof(rt1w_path_params);
        case 11: return (uint32_t)sizeof(rt1w_path_state);
        default: return 0u;
    }
}

int rt1w_host_alloc(uint64_t bytes, void** out) {
    if (!out || bytes == 0) { rt1w::set_error("null argument"); return RT1W_ERR_INVALID; }
    *out = nullptr;
    if (!hip_ok(hipHostMalloc(out, (size_t)bytes, hipHostMallocPortable), "hipHostMalloc")) return RT1W_ERR_NOMEM;
    return RT1W_OK;
}
int rt1w_host_free(void* p) { if (p && !hip_ok(hipHostFree(p), "hipHostFree")) return RT1W_ERR_DEVICE; return RT1W_OK; }
int rt1w_host_register(void* p, uint64_t bytes) {
    if (!p || bytes == 0) { rt1w::set_error("null argument"); return RT1W_ERR_INVALID; }
    if (!hip_ok(hipHostRegister(p, (size_t)bytes, hipHostRegisterPortable), "hipHostRegister")) return RT1W_ERR_DEVICE;
    return RT1W_OK;
}
int rt1w_host_unregister(void* p) { if (p && !hip_ok(hipHostUnregister(p), "hipHostUnregister")) return RT1W_ERR_DEVICE; return RT1W_OK; }

/* for walk_lab.hip (diagnostics): the scene view the kernels get, and the device */
void rt1w_internal_register_wavefront(rt1w_wf_render_fn render, rt1w_wf_destroy_fn destroy) { g_wf_render = render; g_wf_destroy = destroy; }
void rt1w_internal_register_f32_kernels(rt1w_f32_kernel_fn kernel_of) { g_f32_kernel_of = kernel_of; }
const void* rt1w_internal_view(const rt1w_context* c) { return &c->view; }
int rt1w_internal_device(const rt1w_context* c) { return c->device; }

int rt1w_debug_aabb(rt1w_context* c, const double* in, int* out_literal, int* out_fast, uint64_t n) {
    if (!c || !in || !out_literal || !out_fast) { rt1w::set_error("null argument"); return RT1W_ERR_INVALID; }
    if (n == 0) return RT1W_OK;
    if (!hip_ok(hipSetDevice(c->device), "hipSetDevice")) return RT1W_ERR_DEVICE;
    double* din = nullptr; int *d0 = nullptr, *d1 = nullptr;
    int rc = RT1W_OK;
    if (!hip_ok(hipMalloc((void**)&din, n * 14 * sizeof(double)), "hipMalloc") || !hip_ok(hipMalloc((void**)&d0, n * sizeof(int)), "hipMalloc") ||
        !hip_ok(hipMalloc((void**)&d1, n * sizeof(int)), "hipMalloc")) rc = RT1W_ERR_NOMEM;
    if (rc == RT1W_OK) {
        (void)hipMemcpy(din, in, n * 14 * sizeof(double), hipMemcpyHostToDevice);
        hipLaunchKernelGGL(rt_debug_aabb_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->lane[0].stream, din, d0, d1, (unsigned long long)n);
        if (!hip_ok(hipStreamSynchronize(c->lane[0].stream), "debug kernel")) rc = RT1W_ERR_DEVICE;
        else { (void)hipMemcpy(out_literal, d0, n * sizeof(int), hipMemcpyDeviceToHost); (void)hipMemcpy(out_fast, d1, n * sizeof(int), hipMemcpyDeviceToHost); }
    }
    if (din) (void)hipFree(din);
    if (d0) (void)hipFree(d0);
    if (d1) (void)hipFree(d1);
    return rc;
}

int rt1w_debug_texture(rt1w_context* c, int mode, uint32_t tex, const double* in, double* out, uint64_t n) {
    if (!c || !in || !out) { rt1w::set_error("null argument"); return RT1W_ERR_INVALID; }
    if (n == 0) return RT1W_OK;
    RtSceneView view;
    memcpy(&view, &c->view, sizeof view);
    /* h_perlin is the scene's table list as uploaded: mode 1 indexes it, so `tex` is held to its count before anything is launched */
    if (const char* why = rt1w::debug_texture_refusal(mode, tex, in, out, view.n_textures, view.perlin ? c->h_perlin.size() : 0u)) {
        rt1w::set_error(why); return RT1W_ERR_INVALID;
    }
    if (!hip_ok(hipSetDevice(c->device), "hipSetDevice")) return RT1W_ERR_DEVICE;
    double *din = nullptr, *dout = nullptr;
    int rc = RT1W_OK;
    if (!hip_ok(hipMalloc((void**)&din, n * 5 * sizeof(double)), "hipMalloc") || !hip_ok(hipMalloc((void**)&dout, n * 3 * sizeof(double)), "hipMalloc")) rc = RT1W_ERR_NOMEM;
    if (rc == RT1W_OK) {
        (void)hipMemcpy(din, in, n * 5 * sizeof(double), hipMemcpyHostToDevice);
        hipLaunchKernelGGL(rt_debug_texture_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, view, mode, tex, din, dout, (unsigned long long)n);
        if (!hip_ok(hipGetLastError(), "launch") || !hip_ok(hipDeviceSynchronize(), "texture probe kernel")) rc = RT1W_ERR_DEVICE;
        else (void)hipMemcpy(out, dout, n * 3 * sizeof(double), hipMemcpyDeviceToHost);
    }
    if (din) (void)hipFree(din);
    if (dout) (void)hipFree(dout);
    return rc;
}


int rt1w_debug_stamps(rt1w_context* c, uint64_t out[16], int reset) {
    if (!c || !out) { rt1w::set_error("null argument"); return RT1W_ERR_INVALID; }
    for (int i = 0; i < 16; ++i) out[i] = 0;
    int valid = 0;
    (void)hipSetDevice(c->device);
#ifdef RT_STAMPS
    {
        unsigned long long h[16];
        (void)hipMemcpyFromSymbol(h, HIP_SYMBOL(g_stamp_total), sizeof h);
        for (int i = 0; i < 16; ++i) out[i] += h[i];
        if (reset) { unsigned long long z[16] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_stamp_total), z, sizeof z); }
        valid = 1;
    }
#endif
    /* a scene-specialised kernel compiled with RT1W_JIT_STAMPS=1 in the environment carries its own counters */
    if (c->jit[JIT_F64].mod) {
        hipDeviceptr_t dptr = nullptr;
        size_t bytes = 0;
        if (hipModuleGetGlobal(&dptr, &bytes, c->jit[JIT_F64].mod, "g_stamp_total") == hipSuccess && bytes == 16 * sizeof(unsigned long long)) {
            unsigned long long h[16];
            (void)hipMemcpy(h, dptr, sizeof h, hipMemcpyDeviceToHost);
            for (int i = 0; i < 16; ++i) out[i] += h[i];
            if (reset) (void)hipMemset(dptr, 0, sizeof h);
            valid = 1;
        }
    }
    (void)hipGetLastError(); /* a kernel without the counters is not an error: do not leave "named symbol not found" for the next launch check */
    return valid;
}

int rt1w_debug_eval(rt1w_context* c, int fn, const double* a, const double* b, double* out, uint64_t n) {
    if (!c || !a || !b || !out) { rt1w::set_error("null argument"); return RT1W_ERR_INVALID; }
    if (n == 0) return RT1W_OK;
    if (!hip_ok(hipSetDevice(c->device), "hipSetDevice")) return RT1W_ERR_DEVICE;
    double *da = nullptr, *db = nullptr, *dout = nullptr;
    size_t bytes = (size_t)n * sizeof(double);
    int rc = RT1W_OK;
    if (!hip_ok(hipMalloc((void**)&da, bytes), "hipMalloc") || !hip_ok(hipMalloc((void**)&db, bytes), "hipMalloc") ||
        !hip_ok(hipMalloc((void**)&dout, bytes), "hipMalloc")) rc = RT1W_ERR_NOMEM;
    if (rc == RT1W_OK) {
        (void)hipMemcpy(da, a, bytes, hipMemcpyHostToDevice);
        (void)hipMemcpy(db, b, bytes, hipMemcpyHostToDevice);
        hipLaunchKernelGGL(rt_debug_eval_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->lane[0].stream, fn, da, db, dout, (unsigned long long)n);
        if (!hip_ok(hipStreamSynchronize(c->lane[0].stream), "debug kernel")) rc = RT1W_ERR_DEVICE;
        else (void)hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost);
    }
    if (da) (void)hipFree(da);
    if (db) (void)hipFree(db);
    if (dout) (void)hipFree(dout);
    return rc;
}

} /* extern "C" */
