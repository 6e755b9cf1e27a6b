/* context_f32.hip -- the render kernels in single precision (RT1W_PRECISION_F32).
 *
 * The reference chooses its arithmetic with one alias, `type Float = f64;` (src/main.rs:1); setting it to f32 turns every
 * vector, ray, hit record, bounding box, camera and colour of the program into f32.  This translation unit does the same to
 * the device core: it compiles rt_core.h / rt_kernel_*.h a second time, inside its own namespace, with `double` redefined
 * to `float` (RT_F32).  What stays 64-bit is spelled rt_f64 in the headers: the generator's word -> number conversions,
 * the internals of sin/cos/atan2/acos/log (evaluated in 64 bits, rounded once), the bit tricks, and the per-pixel sums
 * ("f32 traversal and shading, f64 accumulation").  The scene arrays are converted to the f32 record layouts once per
 * context; BVH boxes are rounded OUTWARD and widened by 1e-5 of their magnitude, because the reference's 0.0001 pad of a
 * rect's box (src/aarect.rs:74-79) is 1.6 f32 ulps at k = 555 and nothing at the final scene's coordinates.
 * The kernels themselves are rt_f32_kernels.h; the record conversion is rt_f32_scene.h, shared with the CPU build of this core.
 *
 * What is bitwise and what is statistical (tests/test_f32_twin.py).  The same kernels built with -DRT_F32_ELEMENTARY_F64
 * (f32_exact.hip, diagnostics library) equal the CPU twin oracle/oracle_flat_f32.cpp bit for bit on all ten instantiations.  This
 * translation unit differs from that build in five functions only -- the device's sinf, cosf, atan2f, acosf, logf instead of the 64-bit
 * ones rounded once (include/rt1w_num.h) -- each bounded on its own (tests/golden/f32_elementary_ulps.json: 1-2 ulp).  The frame of
 * THIS build against the f32 literal oracle and against the f64 frame stays statistical (tests/test_gpu_parity.py::test_f32_mode_*):
 * block means within Monte-Carlo noise, no NaN pixels beyond the f64 frame's, no light leaks at the k = 555 walls.
 */
#include "rt_f32_kernels.h" /* the kernels; leaves the f64 layouts in the global namespace and the f32 ones in rtf32 */
#include "rt_f32_scene.h"   /* the f64 -> f32 record conversion, shared with the CPU build of this core */

namespace {

struct F32Scene {
    void* nodes = nullptr; void* lights = nullptr; void* materials = nullptr; void* textures = nullptr; void* perlin = nullptr;
    void* pw_inner = nullptr; void* pw_groups = nullptr;
    rtf32::RtSceneView view;
    rtf32::RtPwView pw;
    bool pw_ok = false;
    uint32_t pw_stack = 0; /* pushed right children a walk can hold at once: the depth of the inner-record tree */
};

template <class T>
bool upload_vec(void** dst, const std::vector<T>& v) {
    *dst = nullptr;
    const size_t bytes = v.size() * sizeof(T);
    if (hipMalloc(dst, bytes ? bytes : 16) != hipSuccess) return false;
    return !bytes || hipMemcpy(*dst, v.data(), bytes, hipMemcpyHostToDevice) == hipSuccess;
}

} // namespace

extern "C" void rt1w_internal_f32_destroy(void* h) {
    F32Scene* s = static_cast<F32Scene*>(h);
    if (!s) return;
    void* bufs[] = {s->nodes, s->lights, s->materials, s->textures, s->perlin, s->pw_inner, s->pw_groups};
    for (void* b : bufs) if (b) (void)hipFree(b);
    delete s;
}

/* builds the f32 copies of the scene arrays on the current device; `images` is the context's own device copy (bytes) */
extern "C" int rt1w_internal_f32_create(const void* nodes_, uint32_t n_nodes, const void* lights_, uint32_t n_lights, const void* materials_,
                                        uint32_t n_materials, const void* textures_, uint32_t n_textures, const void* perlin_, uint32_t n_perlin,
                                        const void* view64_, void** out) {
    const ::RtNode* nodes = static_cast<const ::RtNode*>(nodes_);
    const ::RtNode* lights = static_cast<const ::RtNode*>(lights_);
    const ::RtMaterial* materials = static_cast<const ::RtMaterial*>(materials_);
    const ::RtTexture* textures = static_cast<const ::RtTexture*>(textures_);
    const ::RtPerlin* perlin = static_cast<const ::RtPerlin*>(perlin_);
    const ::RtSceneView& v64 = *static_cast<const ::RtSceneView*>(view64_);
    F32Scene* s = new (std::nothrow) F32Scene();
    if (!s) return -1;
    rt_f32_scene::Arrays a; /* the conversion itself: rt_f32_scene.h */
    rt_f32_scene::rt_f32_convert(nodes, n_nodes, lights, n_lights, materials, n_materials, textures, n_textures, perlin, n_perlin, v64, a);
    if (!upload_vec(&s->nodes, a.nodes) || !upload_vec(&s->lights, a.lights) || !upload_vec(&s->materials, a.materials) ||
        !upload_vec(&s->textures, a.textures) || !upload_vec(&s->perlin, a.perlin)) { rt1w_internal_f32_destroy(s); return -1; }
    rtf32::RtSceneView& v = s->view;
    v = a.view;
    v.nodes = (const rtf32::RtNode*)s->nodes; v.lights = (const rtf32::RtNode*)s->lights;
    v.materials = (const rtf32::RtMaterial*)s->materials; v.textures = (const rtf32::RtTexture*)s->textures;
    v.perlin = (const rtf32::RtPerlin*)s->perlin;
    /* pair-walk records of a sphere scene, from THIS build's node array (boxes already widened by the conversion) */
    memset(&s->pw, 0, sizeof s->pw);
    if (a.pw_ok && upload_vec(&s->pw_inner, a.pw_inner) && upload_vec(&s->pw_groups, a.pw_groups)) {
        s->pw = a.pw;
        s->pw.inner = (const rtf32::RtPwInner*)s->pw_inner; s->pw.groups = (const rtf32::RtPwGroup*)s->pw_groups;
        s->pw_stack = a.pw_stack;
        s->pw_ok = true;
    }
    *out = s;
    return 0;
}

/* rt1w_context_set_camera: the camera of the f64 view `view64_`, rounded as the conversion rounds it */
extern "C" void rt1w_internal_f32_set_camera(void* h, const void* view64_) {
    F32Scene* s = static_cast<F32Scene*>(h);
    if (s) rt_f32_scene::rt_f32_camera(static_cast<const ::RtSceneView*>(view64_)->camera, s->view.camera);
}

extern "C" int rt1w_internal_f32_pw(void* h, unsigned stack_cap) {
    F32Scene* s = static_cast<F32Scene*>(h);
    return (s && s->pw_ok && s->pw_stack <= stack_cap) ? 1 : 0;
}

/* the kernels' scene arguments, which context.hip passes by address: what 0 the f32 RtSceneView, 1 the f32 RtPwView (nullptr: the
 * scene has no pair-walk records).  They live as long as the scene */
extern "C" const void* rt1w_internal_f32_view(void* h, int what) {
    F32Scene* s = static_cast<F32Scene*>(h);
    if (!s) return nullptr;
    return what == 0 ? static_cast<const void*>(&s->view) : (what == 1 && s->pw_ok) ? static_cast<const void*>(&s->pw) : nullptr;
}

/* The kernels' host handles for context.hip, which launches them like its own; nullptr: no such kernel.  mode 0: the plain kernel;
 * 1: the reordering kernel of the sweep variants, the slice-end reordering of the stack walks (g_sorted); 2: the pair-walk kernel of
 * sphere scenes (variant 5 only; takes the RtPwView in second place, the caller asked rt1w_internal_f32_pw first).  After the view(s)
 * the kernels take the caller's RtFrame as it is: */
static_assert(sizeof(rtf32::RtFrame) == sizeof(::RtFrame), "RtFrame has no floating-point fields: same layout in both builds");
extern "C" const void* rt1w_internal_f32_kernel(int variant, int mode) {
    if (variant < 0 || variant >= RT_N_VARIANTS) return nullptr;
    if (mode == 2) return variant == 5 ? reinterpret_cast<const void*>(rtf32::rt_render_kernel_pw_ss_f32) : nullptr;
    return reinterpret_cast<const void*>(mode ? rtf32::g_sorted[variant] : rtf32::g_plain[variant]);
}
