/* scene.h -- host-side scene graph of librt1w: the constructors of the
 * reference's Hittable / Material / Texture implementors, BVHNode::new, and the
 * flattener that turns the graph into the record arrays of rt_flat.h.
 *
 * Host code here only BUILDS (bounding boxes, BVH, camera frame).  It has no
 * `hit`/`scatter`: intersection and shading exist only in the device kernel
 * (rt_core.h compiled by hipcc) -- there is no CPU render path in the library.
 */
#ifndef RT1W_SCENE_H
#define RT1W_SCENE_H

#include <map>
#include <string>
#include <vector>

#include "rt1w.h"
#include "rt_flat.h"

namespace rt1w {

struct AABB { RtV3 minimum, maximum; }; /* aabb.rs:7-10 */

/* host-only kinds on top of RT_* */
enum { H_AABOX = 100, H_BVH = 101 };

struct HostHittable {
    uint32_t kind = RT_DEFAULT;
    double d[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    int mat = -1;
    int child = -1;          /* wrapper child / medium boundary / AABox side BVH */
    int left = -1, right = -1; /* H_BVH: BVHChild::One -> left only */
    AABB box{};              /* H_BVH aabb, RotateY cached aabb, AABox (box_min, box_max) */
    bool has_box = false;
    bool used = false;       /* already owned by a parent (Box ownership) */
};

void set_error(const std::string& msg);

/* Camera::new (camera.rs:22-59) from the arguments of rt1w_scene_set_camera: the one text behind the scene's camera
 * (rt1w_scene_set_camera), a live context's (rt1w_context_set_camera) and the diagnostics library's.  RT1W_OK, or RT1W_ERR_INVALID
 * with the refusal's text in *why */
inline int camera_make(const double look_from[3], const double look_at[3], const double vup[3], double vfov_deg, double aspect_ratio,
                       double aperture, double focus_dist, double time0, double time1, RtCamera* out, const char** why) {
    if (!look_from || !look_at || !vup) { *why = "null camera vector"; return RT1W_ERR_INVALID; }
    if (!(time0 < time1)) { *why = "camera needs time0 < time1 (gen_range panics otherwise, camera.rs:71)"; return RT1W_ERR_INVALID; }
    RtV3 lf = rt_v3(look_from[0], look_from[1], look_from[2]);
    RtV3 la = rt_v3(look_at[0], look_at[1], look_at[2]);
    RtV3 up = rt_v3(vup[0], vup[1], vup[2]);
    double theta = vfov_deg * (RT_PI / 180.0);
    double h = rt_tan(theta / 2.0);
    double viewport_height = 2.0 * h;
    double viewport_width = aspect_ratio * viewport_height;
    RtCamera c;
    c.w = rt_normalize(lf - la);
    c.u = rt_normalize(rt_cross(up, c.w));
    c.v = rt_cross(c.w, c.u);
    c.origin = lf;
    c.horizontal = focus_dist * viewport_width * c.u;
    c.vertical = focus_dist * viewport_height * c.v;
    c.lower_left_corner = c.origin - c.horizontal / 2.0 - c.vertical / 2.0 - focus_dist * c.w;
    c.lens_radius = aperture / 2.0;
    c.time0 = time0; c.time1 = time1;
    *out = c;
    return RT1W_OK;
}

/* What rt1w_debug_texture and its CPU twin (rt1w_lab_texture_host) refuse, before anything is launched or read: the refusal's text,
 * or null.  Mode 0 reads texture `tex`, mode 1 Perlin table `tex`, mode 2 (sphere_uv) no record at all: it ignores `tex` */
inline const char* debug_texture_refusal(int mode, uint32_t tex, const double* in, const double* out, size_t n_textures, size_t n_perlin) {
    if (!in || !out) return "null argument";
    if (mode < 0 || mode > 2) return "unknown mode";
    if (mode == 0 && tex >= n_textures) return "bad texture id";
    if (mode == 1 && n_perlin == 0u) return "the scene has no Perlin table";
    if (mode == 1 && tex >= n_perlin) return "bad Perlin table index";
    return nullptr;
}

} // namespace rt1w

struct rt1w_scene {
    RtRng rng;
    bool committed = false;
    std::vector<RtTexture> textures;
    std::vector<RtPerlin> perlin;
    std::vector<uint8_t> images;
    std::vector<RtMaterial> materials;
    std::vector<rt1w::HostHittable> hittables;
    int world = -1;
    std::vector<int> lights;
    RtV3 background{0, 0, 0};
    RtCamera camera{};
    bool has_camera = false;
    /* flat form, valid after commit */
    std::vector<RtNode> flat_nodes, flat_lights;
    uint32_t flat_root = RT_NONE;
    uint32_t stack_need = 0, scope_depth = 0;
    bool has_media = false, has_tex = false, has_msphere = false;
    bool media_bare_spheres = false; /* every ConstantMedium's boundary is a bare Sphere node (the kernels of RtCfgSphereMedia) */
    uint32_t walk_order = 0; /* RT1W_WALK_* */
    uint32_t walk_annotated = 0; /* BVH nodes that carry an order annotation (0: the plain kernels serve) */
    uint32_t bvh_build = RT1W_BVH_BEST_AXIS;  /* RT1W_BVH_*: what rt1w_scene_commit flattens with (include/rt1w.h says why) */
    std::vector<int32_t> bvh_topology; /* RT1W_BVH_SAH / RT1W_BVH_BEST_AXIS: the rebuilt trees, see rt1w_scene_get_bvh_topology */
    /* every `BVHNode::new` call of the host (rt1w_hittable_bvh, an AABox's sides): root hittable id -> the objects in the order they
     * were handed over (what RT1W_BVH_BEST_AXIS re-runs the reference's build rule on, bvh.rs:84-87) */
    std::map<int, std::vector<int>> bvh_calls;
};

#endif
