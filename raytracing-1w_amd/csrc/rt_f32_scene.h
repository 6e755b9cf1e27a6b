/* rt_f32_scene.h -- the f64 -> f32 conversion of a flattened scene (RT1W_PRECISION_F32), host code, header-only.
 *
 * One statement of it for the two places that walk f32 records: context_f32.hip uploads what rt_f32_convert returns, and the CPU
 * build of the f32 core (oracle/oracle_flat_f32.cpp) walks the same records on the host -- so a frame of that build is compared with
 * the kernels' frame over the records the device walks, not over a restatement of them.
 *
 * Include it where `double` is double, after the record layouts exist twice: the f64 ones in the global namespace (rt_flat.h) and the
 * f32 ones, with rt_walk_pair.h, in namespace RT_F32_NS (the same headers compiled with `double` redefined to `float`).
 *
 * The rules.  BVH boxes (RT_BVH2 / RT_BVH1 records) are widened by 1e-5 of max(1, |lo|, |hi|) per axis and then rounded OUTWARD:
 * the reference's 0.0001 pad of a rect's box (src/aarect.rs:74-79) is 1.6 f32 ulps at k = 555 and nothing at the final scene's
 * coordinates.  Every other number -- primitives, wrappers, materials, textures, Perlin vectors, camera, background -- is its f64
 * value rounded to nearest.  Integer fields are copied.  The pair-walk records of a sphere scene (rt_walk_pair.h) are built by
 * rt_pw_build of the f32 build from the CONVERTED node array, so their inner boxes and group boxes are the widened f32 boxes. */
#ifndef RT_F32_SCENE_H
#define RT_F32_SCENE_H
#ifdef double
#error "rt_f32_scene.h: include after `#undef double`"
#endif
#ifndef RT_F32_NS
#define RT_F32_NS rtf32
#endif

#include <math.h>
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>

namespace rt_f32_scene {

inline float down(double x) { float f = (float)x; return ((double)f > x) ? nextafterf(f, -INFINITY) : f; }
inline float up(double x) { float f = (float)x; return ((double)f < x) ? nextafterf(f, INFINITY) : f; }

inline RT_F32_NS::RtNode conv_node(const ::RtNode& n) {
    RT_F32_NS::RtNode o;
    memset(&o, 0, sizeof o);
    o.kind = n.kind; o.skip = n.skip; o.b = n.b; o.mat = n.mat; o.a = n.a; o.pad = n.pad;
    const uint32_t k = n.kind & RT_KIND_MASK;
    if (k == RT_BVH2 || k == RT_BVH1) {
        for (int i = 0; i < 3; ++i) {
            const double mag = fmax(1.0, fmax(fabs(n.d[i]), fabs(n.d[i + 3])));
            o.d[i] = down(n.d[i] - 1e-5 * mag);
            o.d[i + 3] = up(n.d[i + 3] + 1e-5 * mag);
        }
    } else {
        for (int i = 0; i < 6; ++i) o.d[i] = (float)n.d[i];
    }
    for (int i = 0; i < 3; ++i) o.e[i] = (float)n.e[i];
    return o;
}

inline RT_F32_NS::RtV3 v3f(const ::RtV3& v) { RT_F32_NS::RtV3 o; o.x = (float)v.x; o.y = (float)v.y; o.z = (float)v.z; return o; }

/* the f32 records of one scene, on the host.  `view` and `pw` carry the counts, root, camera, background and the pair walk's root box
 * and shutter; their array pointers are left null for the owner to set (device copies, or these vectors) */
struct Arrays {
    std::vector<RT_F32_NS::RtNode> nodes; /* n_nodes + one spare record: the fused walk reads record e + 1 with record e */
    std::vector<RT_F32_NS::RtNode> lights;
    std::vector<RT_F32_NS::RtMaterial> materials;
    std::vector<RT_F32_NS::RtTexture> textures;
    std::vector<RT_F32_NS::RtPerlin> perlin;
    RT_F32_NS::RtSceneView view;
    std::vector<RT_F32_NS::RtPwInner> pw_inner;
    std::vector<RT_F32_NS::RtPwGroup> pw_groups;
    RT_F32_NS::RtPwView pw;
    bool pw_ok = false;    /* a sphere scene: pw_inner / pw_groups / pw are filled */
    uint32_t pw_stack = 0; /* pushed right children a walk can hold at once: the depth of the inner-record tree */
};

/* the camera, every quantity rounded once: at the conversion, and again when a live context's camera is set (rt1w_context_set_camera) */
inline void rt_f32_camera(const ::RtCamera& c, RT_F32_NS::RtCamera& o) {
    o.origin = v3f(c.origin); o.lower_left_corner = v3f(c.lower_left_corner); o.horizontal = v3f(c.horizontal);
    o.vertical = v3f(c.vertical); o.u = v3f(c.u); o.v = v3f(c.v); o.w = v3f(c.w);
    o.lens_radius = (float)c.lens_radius; o.time0 = (float)c.time0; o.time1 = (float)c.time1;
}

/* `v64`: the f64 view of the scene (counts, root, camera, background; its array pointers are not read, `images` is copied as it is) */
inline void rt_f32_convert(const ::RtNode* nodes, uint32_t n_nodes, const ::RtNode* lights, uint32_t n_lights, const ::RtMaterial* materials,
                           uint32_t n_materials, const ::RtTexture* textures, uint32_t n_textures, const ::RtPerlin* perlin, uint32_t n_perlin,
                           const ::RtSceneView& v64, Arrays& s) {
    s.nodes.resize(n_nodes + 1u); s.lights.resize(n_lights);
    memset(&s.nodes[n_nodes], 0, sizeof s.nodes[n_nodes]);
    for (uint32_t i = 0; i < n_nodes; ++i) s.nodes[i] = conv_node(nodes[i]);
    for (uint32_t i = 0; i < n_lights; ++i) s.lights[i] = conv_node(lights[i]);
    s.materials.resize(n_materials);
    for (uint32_t i = 0; i < n_materials; ++i) {
        memset(&s.materials[i], 0, sizeof s.materials[i]);
        for (int k = 0; k < 4; ++k) s.materials[i].d[k] = (float)materials[i].d[k];
        s.materials[i].kind = materials[i].kind; s.materials[i].tex = materials[i].tex;
    }
    s.textures.resize(n_textures);
    for (uint32_t i = 0; i < n_textures; ++i) {
        memset(&s.textures[i], 0, sizeof s.textures[i]);
        for (int k = 0; k < 3; ++k) s.textures[i].d[k] = (float)textures[i].d[k];
        s.textures[i].kind = textures[i].kind; s.textures[i].a = textures[i].a; s.textures[i].b = textures[i].b; s.textures[i].c = textures[i].c;
    }
    s.perlin.resize(n_perlin);
    for (uint32_t i = 0; i < n_perlin; ++i) {
        for (int k = 0; k < 256 * 3; ++k) s.perlin[i].ranvec[k] = (float)perlin[i].ranvec[k];
        memcpy(s.perlin[i].perm_x, perlin[i].perm_x, sizeof s.perlin[i].perm_x);
        memcpy(s.perlin[i].perm_y, perlin[i].perm_y, sizeof s.perlin[i].perm_y);
        memcpy(s.perlin[i].perm_z, perlin[i].perm_z, sizeof s.perlin[i].perm_z);
    }
    RT_F32_NS::RtSceneView& v = s.view;
    memset(&v, 0, sizeof v);
    v.images = v64.images;
    v.root = v64.root; v.n_nodes = v64.n_nodes; v.n_lights = v64.n_lights; v.n_materials = v64.n_materials; v.n_textures = v64.n_textures;
    rt_f32_camera(v64.camera, v.camera);
    v.background = v3f(v64.background);
    /* pair-walk records of a sphere scene, from THIS build's node array (boxes already widened by conv_node) */
    memset(&s.pw, 0, sizeof s.pw);
    s.pw_ok = false; s.pw_stack = 0; s.pw_inner.clear(); s.pw_groups.clear();
    std::vector<RT_F32_NS::RtNode> only(s.nodes.begin(), s.nodes.begin() + n_nodes);
    std::string why;
    if (n_nodes > 0 && RT_F32_NS::rt_pw_build(only, v64.root, s.pw_inner, s.pw_groups, s.pw, why)) {
        /* deepest chain of inner records: a walk pushes at most one right child per level */
        struct D { static uint32_t of(const std::vector<RT_F32_NS::RtPwInner>& v, uint32_t i) {
            if (i & RT_PW_LEAF) return 0u;
            const uint32_t a = of(v, v[i].l), b = of(v, v[i].r);
            return 1u + (a > b ? a : b);
        } };
        s.pw_stack = (s.pw.root & RT_PW_LEAF) ? 0u : D::of(s.pw_inner, s.pw.root);
        s.pw_ok = true;
    }
}

} // namespace rt_f32_scene

#endif
