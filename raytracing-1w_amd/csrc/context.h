/* context.h -- the device context as the library's own units see it: context.hip (the context, the render kernels' plan and launch, the
 * render entries) and features.hip (the entries of the feature buffers and the denoiser), with the helpers of the first that the second
 * calls: the checks of an rt1w_render_params, the render path without an entry's clock, and dev_grow, through which every grow-on-demand
 * device buffer of the context and its lanes grows.  The scene-specialised kernel is kept by form (jit.h: JitForm) in RtJitSlot jit[], state
 * only: loader, policy table and render-time lookup are context.hip's.  Private: nothing here is exported (-fvisibility=hidden, librt1w.map). */
#ifndef RT1W_CONTEXT_H
#define RT1W_CONTEXT_H

#include <hip/hip_runtime.h>

#include <chrono>
#include <string>
#include <vector>

#include "rt_kernel_plain.h"
#include "render_params.h"

/* Everything one in-flight render needs.  Lane 0 serves the one-shot entries; rt1w_render_rows keeps two strips in
 * flight, one per lane, so that the next strip's workgroups fill the CUs as the previous strip's persistent kernel tails off
 * and its device->host copy runs under the other lane's tracing. */
struct RtLane {
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    double* d_partial = nullptr; size_t partial_bytes = 0;
    unsigned long long* d_counters = nullptr;
    unsigned long long* h_counters = nullptr; /* pinned */
    void* d_strip = nullptr; void* h_strip = nullptr; size_t strip_bytes = 0; /* rt1w_render_rows: device strip + pinned host strip */
    uint32_t passes = 0; /* sample passes of the launch in flight (render_launch), reported by render_finish */
};

/* one runnable kernel: what to call, with which scene arguments in front of (frame, partial sums, counters), its workgroup size and
 * stats bits, and its persistent grid (0: not built for this context, or not resolved yet) */
struct RtKernel {
    int block;
    uint32_t bits;
    const void* fn = nullptr;     /* a __global__ of this library (context.hip, context_ref.hip, context_f32.hip) ... */
    hipFunction_t jit = nullptr;  /* ... or the scene-specialised kernel (jit.cpp), from its module */
    bool pw = false,              /* takes the pair-walk view (rt_walk_pair.h) in second place */
         f32 = false,             /* takes the f32 scene's views (context_f32.hip) instead of the context's */
         tiles = false,           /* tile-list form (context_tiles.hip): takes the tile list (RtTileArg) in last place */
         rays = false;            /* ray-list form (context_rays.hip): takes the ray list (RtRayArg) in last place */
    int grid = 0;
    /* the makers: RtKernel::of(block, bits, fn).with_pw() -- a call site names the arguments its kernel takes */
    static RtKernel of(int block, uint32_t bits, const void* fn = nullptr) { RtKernel k; k.block = block; k.bits = bits; k.fn = fn; return k; }
    RtKernel with_pw(bool on = true) const { RtKernel k = *this; k.pw = on; return k; }
    RtKernel with_f32(bool on = true) const { RtKernel k = *this; k.f32 = on; return k; }
    RtKernel with_tiles(bool on = true) const { RtKernel k = *this; k.tiles = on; return k; }
    RtKernel with_rays(bool on = true) const { RtKernel k = *this; k.rays = on; return k; }
};

/* the tile list as the kernels of context_tiles.hip take it (rt_kernel_sorted.h: RtTileList; the same bytes, checked at first use) */
struct RtTileArg {
    const uint32_t* rec = nullptr; /* device: [n][4] = rt1w_tile records */
    uint32_t side = 0, n = 0;
};

/* the ray list as the kernels of context_rays.hip take it (rt_ray_list.h: RtRayList; the same bytes, checked at first use) */
struct RtRayArg {
    const double* rays = nullptr;         /* device: [n][stride] */
    const uint32_t* start_word = nullptr; /* device: [n], or null */
    uint64_t n = 0, first_stream = 0;
    uint32_t stride = 0, pad = 0;
};

/* The f64 render kernels by walk form and variant (context.hip: g_kernels).  Every walk form is followed by its build for
 * scenes whose media are all bounded by a bare Sphere (rt_flat.h: RtCfgSphereMedia): form + 1. */
enum RtWalkForm {
    RT_WALK_PLAIN, RT_WALK_SPHERE_MEDIA,
    RT_WALK_SS, RT_WALK_SS_SPHERE_MEDIA,       /* finished paths reordered across the workgroup at the end of every slice (rt_render_ss_body) */
    RT_WALK_SS_HC, RT_WALK_SS_HC_SPHERE_MEDIA, /* ... and the scene's most visited nodes in LDS (rt_walk_table.h): a context with a walk table */
    RT_WALK_LDS_NODES,                         /* all nodes in LDS (scenes of <= RT_LDS_NODE_CAP nodes; opt-in: RT1W_LDS_NODES) */
    RT_WALK_SORTED,                            /* the reordering kernel (rt_kernel_sorted.h) */
    RT_N_WALKS
};

/* a scene-specialised kernel (jit.cpp) in one of its forms (jit.h: JitForm): what the context knows of it.  State only -- how loading
 * differs between the forms is one table beside the loader (context.hip: g_jit_forms, load_specialised) */
struct RtJitSlot {
    std::string src, key;      /* generated source (empty: scene not eligible), cache key */
    hipModule_t mod = nullptr;
    RtKernel k{};              /* k.jit != nullptr once loaded */
    uint32_t vgprs = 0;
    bool consulted = false;    /* a render has looked in the kernel caches for it (specialised_lookup: once per context and form) */
    bool failed = false;       /* a compile or load failed and is not repeated: by a long render (render_common), of an optional form (load_specialised) */
    std::string error;         /* ... and why */
};

struct rt1w_context {
    int device = 0;
    int n_cu = 0; /* compute units: a persistent grid is n_cu x the workgroups resident per CU (kernel_grid) */
    RtLane lane[2];
    hipEvent_t ev_first = nullptr;
    void* d_nodes = nullptr; void* d_lights = nullptr; void* d_materials = nullptr;
    void* d_textures = nullptr; void* d_perlin = nullptr; void* d_images = nullptr;
    RtSceneView view{};
    double* d_out = nullptr; size_t out_bytes = 0;
    void* dn_buf[3] = {nullptr, nullptr, nullptr}; size_t dn_bytes[3] = {0, 0, 0}; /* rt1w_denoise, rt1w_denoise_var: two colour buffers and the guide buffer */
    double* d_batches = nullptr; size_t batches_bytes = 0; /* rt1w_batch_variance, rt1w_render_denoised_var: the sums of the sample batches */
    double* d_accum = nullptr; size_t accum_bytes = 0; /* rt1w_accum_*, rt1w_render_adaptive: the accumulator and, behind it, the tile errors */
    /* rt1w_render_temporal: the two sets of (hist[3], len[1], aov[8]) per pixel that swap -- tm_buf[tm_prev] is the previous frame's --,
     * the image they hold, the camera of the previous frame; tm_valid false: no history (first call, rt1w_temporal_reset, another size) */
    void* tm_buf[2] = {nullptr, nullptr}; size_t tm_bytes[2] = {0, 0};
    uint32_t tm_w = 0, tm_h = 0; int tm_prev = 0; bool tm_valid = false;
    RtCamera tm_cam{};
    /* rt1w_render_temporal_var: a state of its own, the same scheme -- two sets of (hist[3], m2[1], len[1], aov[8]) per pixel that swap */
    void* tv_buf[2] = {nullptr, nullptr}; size_t tv_bytes[2] = {0, 0};
    uint32_t tv_w = 0, tv_h = 0; int tv_prev = 0; bool tv_valid = false;
    RtCamera tv_cam{};
    RtKernel k64[RT_N_WALKS][RT_N_VARIANTS] = {}; /* g_kernels, queried at creation; the node-cache walks only with a walk table */
    bool walk_table = false; uint32_t walk_table_first = 0;
    bool sphere_media = false; /* every medium of the scene is bounded by a bare Sphere: the sphere-media walks serve */
    int variant = 0;
    bool has_media = false, has_tex = false, has_msphere = false;
    uint32_t n_nodes = 0, scope_depth = 0;
    void* wf_state = nullptr; /* the wavefront form's own state (librt1w_lab.so: wavefront.hip), freed through its destroy hook */
    uint32_t stack_need = 0;
    RtKernel ref[4] = {}; /* reference-stream kernels by rt1w_internal_ref_kernel mode: sweep, stack walk, reordering V0, reordering every-feature */
    void* f32_scene = nullptr;   /* context_f32.hip: f32 copies of the scene arrays, built at the first f32 render */
    bool tried_f32_scene = false;
    /* pair walk (rt_walk_pair.h): records of an eligible scene (sphere-only, variant 5); its kernels, plain and reordering (grid 0: the
     * scene is not eligible) */
    void* d_pw_inner = nullptr; void* d_pw_groups = nullptr;
    RtPwView pw{};
    std::string pw_why;
    RtKernel pw_k[2] = {};
    /* rt1w_render_tiles: the tile-list forms of k64 and pw_k (context_tiles.hip), resolved at their first use, and the uploaded list */
    RtKernel kt[RT_N_WALKS][RT_N_VARIANTS] = {};
    RtKernel pw_kt[2] = {};
    void* d_tiles = nullptr; size_t tiles_bytes = 0;
    /* rt1w_ray_color: the ray-list forms of k64 and pw_k (context_rays.hip), resolved at their first use */
    RtKernel kr[RT_N_WALKS][RT_N_VARIANTS] = {};
    RtKernel pw_kr[2] = {};
    /* host copies of the flat arrays the two opt-in modes convert on first use (a scene may be destroyed before its contexts) */
    std::vector<RtNode> h_nodes, h_lights; std::vector<RtMaterial> h_materials; std::vector<RtTexture> h_textures; std::vector<RtPerlin> h_perlin;
    RtKernel k32[RT_N_VARIANTS][3] = {}; /* f32 kernels by variant and rt1w_internal_f32_kernel mode: plain, reordering, pair walk */
    RtKernel k32x[RT_N_VARIANTS][3] = {}; /* the same slots for the kernels a registered rt1w_f32_kernel_fn hands out (rt1w_internal.h) */
    /* the scene-specialised kernel by form: JIT_F64 from the caches at creation, the other two at the first render that asks for them
     * (specialised_lookup: JIT_F32 only beside JIT_F64, JIT_TILES with RT1W_TILES_SPECIALISED); from the compiler in rt1w_context_specialise */
    RtJitSlot jit[3]; /* JIT_N_FORMS: context.hip checks it (features.hip, which never looks at a slot, does not see jit.h) */
};

namespace rt1w {
bool hip_ok(hipError_t e, const char* what); /* false with the error set */
int validate(const rt1w_context* c, const rt1w_render_params* p); /* null arguments and params_check (render_params.h), with the error set */
/* RT1W_FORCE_VARIANT: `*v` becomes the variant the flags name, if they name one (allow_v4: the order-aware V4, which exists in f64 only) */
int forced_variant(const rt1w_context* c, uint32_t flags, bool allow_v4, int* v);
double lane_ms(const RtLane& l); /* ms between the two events of the lane, once its stream has drained */
/* The one way a grow-on-demand device buffer grows: (*p, *have bytes) to at least `need` bytes -- freed and allocated anew, its contents
 * are not kept, nothing happens while it is large enough.  `what` is the text of a failed allocation ("hipMalloc(framebuffer)"), which
 * returns RT1W_ERR_NOMEM and leaves the buffer empty.  Serves the framebuffer, a lane's partial sums, the tile list, the denoisers' buffers,
 * the batch buffer, the accumulator buffer and the temporal state; the strips of rt1w_render_rows pair a device and a pinned host allocation and stay apart. */
int dev_grow(void** p, size_t* have, size_t need, const char* what);
int reserve_out(rt1w_context* c, size_t bytes); /* the context's framebuffer, grown to at least `bytes` */
/* plan, launch on lane 0, wait, stats: what every one-shot render entry runs */
int render_common(rt1w_context* c, const rt1w_render_params* p, double* d_out, rt1w_stats* stats);
/* rt1w_render_tiles_device without the entry's own clock: validate, upload the list, plan, launch on lane 0, wait, stats */
/* the context's copy of a tile list (HOST memory in, device memory out: valid until the next upload), grown on demand */
int tiles_upload(rt1w_context* c, const rt1w_tile* tiles, uint32_t n_tiles, const uint32_t** d_rec);
int render_tiles_common(rt1w_context* c, const rt1w_render_params* p, uint32_t tile, const rt1w_tile* tiles, uint32_t n_tiles, double* d_out, rt1w_stats* stats);
/* rt1w_ray_color_device without the entry's checks and clock (features.hip): the plan of a render of n x 1 pixels with RT1W_GENERIC, its
 * kernel's ray-list form over the device buffers, launch on lane 0 (sample passes included), wait, stats */
int ray_color_common(rt1w_context* c, const rt1w_render_params* frame, const RtRayArg& rays, double* d_out, rt1w_stats* stats);
/* the host clock of an entry, for rt1w_stats.total_ms */
struct RtTimer {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    double ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};
} // namespace rt1w

#endif
