/* oracle_flat_f32.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT: the CPU twin of the single-precision kernels (RT1W_PRECISION_F32).
 *
 * oracle_flat.cpp -- the device core driven by the kernels' work decomposition -- compiled a second time with `double` redefined to
 * `float` (RT_F32), inside namespace rtf32: the switch raytracing-1w_amd/csrc/rt_f32_kernels.h throws for the device.  On the host the
 * elementary functions of a float (sin, cos, atan2, acos, ln) are the 64-bit ones of include/rt1w_num.h rounded once; the device build
 * with -DRT_F32_ELEMENTARY_F64 (csrc/f32_exact.hip) does the same, and everything else in the f32 core is + - * /, sqrtf, comparisons
 * and conversions under -ffp-contract=off.  So the frame of that device build must equal this library's bit for bit, with equal segment
 * counts (tests/test_f32_twin.py); the product's kernels differ from it in those five functions only.
 *
 * orcflat_f32_render takes the f64 flat arrays of a scene, as orcflat_render does, converts them with the product's own conversion
 * (csrc/rt_f32_scene.h: outward-rounded, widened BVH boxes; the f32 pair-walk records) and walks those records.  Pixel sums are 64-bit
 * as in the kernels (oracle_flat.cpp: RtV3d), frames come back as f64.  The standard headers come first: their text must not see the
 * redefined keyword. */
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <queue>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "rt_flat.h" /* the f64 record layouts (global namespace): what the conversion reads */

#undef RT1W_NUM_H
#undef RT1W_FLAT_H
#define RT_F32 1
#define double float

namespace rtf32 {
#include "oracle_flat.cpp"
} // namespace rtf32

#undef double
#include "rt_f32_scene.h"

extern "C" {

struct orcflat_cam_bg64 { ::RtCamera cam; ::RtV3 bg; uint32_t root, pad; };

static void convert(const void* nodes, uint32_t n_nodes, const void* lights, uint32_t n_lights, const void* materials, uint32_t n_materials,
                    const void* textures, uint32_t n_textures, const void* perlin, uint32_t n_perlin, const void* images, const void* cam_bg,
                    rt_f32_scene::Arrays& a) {
    const orcflat_cam_bg64* cb = (const orcflat_cam_bg64*)cam_bg;
    ::RtSceneView v64;
    memset(&v64, 0, sizeof v64);
    v64.images = (const uint8_t*)images;
    v64.root = cb->root; v64.n_nodes = n_nodes; v64.n_lights = n_lights; v64.n_materials = n_materials; v64.n_textures = n_textures;
    v64.camera = cb->cam; v64.background = cb->bg;
    rt_f32_scene::rt_f32_convert((const ::RtNode*)nodes, n_nodes, (const ::RtNode*)lights, n_lights, (const ::RtMaterial*)materials, n_materials,
                                 (const ::RtTexture*)textures, n_textures, (const ::RtPerlin*)perlin, n_perlin, v64, a);
    a.view.nodes = a.nodes.data(); a.view.lights = a.lights.data(); a.view.materials = a.materials.data();
    a.view.textures = a.textures.data(); a.view.perlin = a.perlin.data();
    a.pw.inner = a.pw_inner.data(); a.pw.groups = a.pw_groups.data();
}

/* The f64 arrays of orcflat_render (+ the number of Perlin records).  walk 0: the one-entry-per-step walk; 1: the pair walk of sphere
 * scenes with `pw_stack` stack entries per lane (variant 5; -4 if the scene has no pair-walk records or they need a deeper stack: the
 * product then keeps the other walk).  Otherwise orcflat_render's results. */
int orcflat_f32_render(const void* nodes, uint32_t n_nodes, const void* lights, uint32_t n_lights, const void* materials, uint32_t n_materials,
                       const void* textures, uint32_t n_textures, const void* perlin, uint32_t n_perlin, const void* images, const void* cam_bg,
                       const ::RtFrame* frame, int variant, int walk, uint32_t pw_stack, int out_sum, int threads, double* out,
                       uint64_t* segments_out, uint32_t* max_stack_out) {
    static_assert(sizeof(rtf32::RtFrame) == sizeof(::RtFrame), "RtFrame has no floating-point fields: same layout in both builds");
    rt_f32_scene::Arrays a;
    convert(nodes, n_nodes, lights, n_lights, materials, n_materials, textures, n_textures, perlin, n_perlin, images, cam_bg, a);
    if (walk == 1 && (variant != 5 || !a.pw_ok || a.pw_stack > pw_stack)) return -4;
    return rtf32::render_view(a.view, walk == 1 ? &a.pw : nullptr, pw_stack, (const rtf32::RtFrame*)frame, variant, out_sum, threads, out,
                              segments_out, max_stack_out);
}

/* the converted records, for the conversion's own tests: what 0 nodes (n_nodes records), 1 lights, 2 materials,
 * 3 textures, 4 Perlin records, 5 {camera, background} as floats, 6 pair-walk inner records, 7 pair-walk groups, 8 the pair-walk view's
 * root box (6 floats).  Returns the bytes of the selection; copies them when `out` is not null and `cap` suffices. */
uint64_t orcflat_f32_records(const void* nodes, uint32_t n_nodes, const void* lights, uint32_t n_lights, const void* materials, uint32_t n_materials,
                             const void* textures, uint32_t n_textures, const void* perlin, uint32_t n_perlin, const void* cam_bg, int what,
                             void* out, uint64_t cap) {
    rt_f32_scene::Arrays a;
    convert(nodes, n_nodes, lights, n_lights, materials, n_materials, textures, n_textures, perlin, n_perlin, nullptr, cam_bg, a);
    struct { rtf32::RtCamera cam; rtf32::RtV3 bg; } cb = {a.view.camera, a.view.background};
    const void* p = nullptr; uint64_t bytes = 0;
    switch (what) {
        case 0: p = a.nodes.data(); bytes = (uint64_t)n_nodes * sizeof(rtf32::RtNode); break;
        case 1: p = a.lights.data(); bytes = a.lights.size() * sizeof(rtf32::RtNode); break;
        case 2: p = a.materials.data(); bytes = a.materials.size() * sizeof(rtf32::RtMaterial); break;
        case 3: p = a.textures.data(); bytes = a.textures.size() * sizeof(rtf32::RtTexture); break;
        case 4: p = a.perlin.data(); bytes = a.perlin.size() * sizeof(rtf32::RtPerlin); break;
        case 5: p = &cb; bytes = sizeof cb; break;
        case 6: p = a.pw_inner.data(); bytes = a.pw_inner.size() * sizeof(rtf32::RtPwInner); break;
        case 7: p = a.pw_groups.data(); bytes = a.pw_groups.size() * sizeof(rtf32::RtPwGroup); break;
        case 8: p = a.pw.root_box; bytes = a.pw_ok ? sizeof a.pw.root_box : 0u; break;
        default: return 0;
    }
    if (out && bytes <= cap && bytes) memcpy(out, p, bytes);
    return bytes;
}

/* The shading-side leaf functions of the f32 core over the converted records, for the known-answer tests (tests/test_texture_kats.py):
 * in[i] = {u, v, p.x, p.y, p.z}, each rounded to float once; out[i] = 3 results widened to double.  mode 0 rt_texture of texture `tex`,
 * mode 1 rt_perlin_noise and rt_perlin_turb(.., 7) of Perlin table `tex`.  0, or -1: another mode, or `tex` beyond the records. */
int orcflat_f32_texture(const void* nodes, uint32_t n_nodes, const void* lights, uint32_t n_lights, const void* materials, uint32_t n_materials,
                        const void* textures, uint32_t n_textures, const void* perlin, uint32_t n_perlin, const void* images, const void* cam_bg,
                        int mode, uint32_t tex, const double* in, double* out, uint64_t n) {
    if (!in || !out || mode < 0 || mode > 1 || (mode == 0 && tex >= n_textures) || (mode == 1 && tex >= n_perlin)) return -1;
    rt_f32_scene::Arrays a;
    convert(nodes, n_nodes, lights, n_lights, materials, n_materials, textures, n_textures, perlin, n_perlin, images, cam_bg, a);
    for (uint64_t i = 0; i < n; ++i) {
        const float u = (float)in[i * 5], v = (float)in[i * 5 + 1];
        const rtf32::RtV3 p = rtf32::rt_v3((float)in[i * 5 + 2], (float)in[i * 5 + 3], (float)in[i * 5 + 4]);
        rtf32::RtV3 r = rtf32::rt_v3(0.0f, 0.0f, 0.0f);
        if (mode == 0) r = rtf32::rt_texture<rtf32::RtCfgV1>(a.view, tex, u, v, p);
        else { r.x = rtf32::rt_perlin_noise(a.view.perlin[tex], p); r.y = rtf32::rt_perlin_turb(a.view.perlin[tex], p, 7); }
        out[i * 3] = (double)r.x; out[i * 3 + 1] = (double)r.y; out[i * 3 + 2] = (double)r.z;
    }
    return 0;
}

/* the five elementary functions as the f32 core calls them on the host: the 64-bit function of include/rt1w_num.h, rounded once.
 * fn 0 sin(x), 1 cos(x), 2 atan2(x, y), 3 acos(x), 4 ln(x) */
void orcflat_f32_elementary(int fn, const float* x, const float* y, uint64_t n, float* out) {
    for (uint64_t i = 0; i < n; ++i) {
        switch (fn) {
            case 0: out[i] = (float)rtf32::rt_sin((rt_f64)x[i]); break;
            case 1: out[i] = (float)rtf32::rt_cos((rt_f64)x[i]); break;
            case 2: out[i] = (float)rtf32::rt_atan2((rt_f64)x[i], (rt_f64)y[i]); break;
            case 3: out[i] = (float)rtf32::rt_acos((rt_f64)x[i]); break;
            default: out[i] = (float)rtf32::rt_log((rt_f64)x[i]); break;
        }
    }
}

uint32_t orcflat_f32_sizeof(int what) {
    switch (what) { case 0: return sizeof(rtf32::RtNode); case 1: return sizeof(rtf32::RtMaterial); case 2: return sizeof(rtf32::RtTexture);
                    case 3: return sizeof(rtf32::RtPerlin); case 4: return sizeof(rtf32::RtCamera); default: return 0; }
}

} /* extern "C" */
