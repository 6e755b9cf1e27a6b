/* rt1w.h -- C ABI of the MI355X path tracer (librt1w.so).
 *
 * The reference (hatoo/raytracing-1w, /root/reference) has NO FFI or plugin
 * interface: the hot path is a closure inlined in `main`
 * (src/main.rs:957-1001) over `camera`, `world: BVHNode`,
 * `lights: Option<Vec<Box<dyn Hittable>>>`, `background`, image size, spp and
 * MAX_DEPTH.  This header is the seam a Rust host would bind with
 * `extern "C"`: the scene is described through constructors that mirror the
 * reference's own (same names, same argument order and meaning), flattened
 * once, uploaded once, and `rt1w_render` replaces the closure.
 * INTEGRATION.md shows the Rust-side binding.
 *
 * Conventions
 *   - every function returns an `int`: >= 0 success (an id where the function
 *     creates something), < 0 one of RT1W_ERR_*; `rt1w_last_error()` returns a
 *     thread-local message.  Nothing aborts or throws across the ABI; the
 *     reference's panics (src/bvh.rs:61,67, src/hittable.rs:153) become
 *     RT1W_ERR_INVALID.
 *   - caller owns every buffer it passes; the library copies what it keeps.
 *   - a scene is immutable after rt1w_scene_commit and may back many contexts;
 *     one context = one GPU + one HIP stream; calls on distinct contexts are
 *     thread-safe, calls on one context are serialised by the caller.
 *   - there is no CPU render path: without a usable GPU rt1w_context_create
 *     fails with RT1W_ERR_DEVICE.
 *   - all geometry/colour arithmetic is f64 (`type Float = f64`, src/main.rs:1).
 */
#ifndef RT1W_H
#define RT1W_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* librt1w.so is built with -fvisibility=hidden: what this header declares is everything it exports (plus three rt1w_internal_* hooks
 * of its own diagnostics library, csrc/rt1w_internal.h) */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define RT1W_OK 0
#define RT1W_ERR_INVALID (-1)     /* bad argument / bad id / empty BVH (src/bvh.rs:61) */
#define RT1W_ERR_UNSUPPORTED (-2) /* graph shape the device format cannot express */
#define RT1W_ERR_DEVICE (-3)      /* no GPU, HIP error */
#define RT1W_ERR_NOMEM (-4)
#define RT1W_ERR_STATE (-5)       /* e.g. mutate after commit, render before commit */
#define RT1W_ERR_CANCELLED (-6)   /* the progress callback of rt1w_render_rows asked to stop */

typedef struct rt1w_scene rt1w_scene;
typedef struct rt1w_context rt1w_context;

const char* rt1w_last_error(void);
const char* rt1w_version(void);

/* ---- scene construction: one-shot host work (src/main.rs:192-795, 807-951) ---- */

/* `build_seed` seeds the scene-build random stream that replaces the
 * reference's entropy-seeded `MyRng::from_entropy()` (src/main.rs:803).  Every
 * constructor below that takes `rng` in the reference (AABox::new, BVHNode::new,
 * NoiseTexture::new) draws from it at call time, in call order, exactly like
 * the Rust constructors do. */
int rt1w_scene_create(uint64_t build_seed, rt1w_scene** out);
void rt1w_scene_destroy(rt1w_scene* s);

/* draws for the host's own scene code (`rng.gen()`, `rng.gen_range(a..b)` in
 * random_scene / final_scene, src/main.rs:212-245,653,777-779) from the same
 * build stream; value returned through *out */
int rt1w_scene_rng_f64(rt1w_scene* s, double* out);
int rt1w_scene_rng_range(rt1w_scene* s, double low, double high, double* out);

/* Texture implementors (src/texture.rs).  Return a texture id. */
int rt1w_texture_solid(rt1w_scene* s, const double rgb[3]);                 /* SolidColor   texture.rs:13-16 */
int rt1w_texture_checker(rt1w_scene* s, int odd, int even);                 /* CheckerTexture texture.rs:18-22 */
int rt1w_texture_noise(rt1w_scene* s, double scale);                        /* NoiseTexture256::new(scale, rng) texture.rs:32-38, perlin.rs:25-43 */
int rt1w_texture_noise_tables(rt1w_scene* s, double scale, const double ranvec[768],
                              const uint32_t perm_x[256], const uint32_t perm_y[256],
                              const uint32_t perm_z[256]);                  /* same, caller-supplied tables */
int rt1w_texture_image(rt1w_scene* s, const uint8_t* rgb8, uint32_t width, uint32_t height); /* DynamicImage texture.rs:67-89 (decoded RGB8, row 0 = top) */

/* Material implementors (src/material.rs).  Return a material id. */
int rt1w_material_lambertian(rt1w_scene* s, int albedo_texture);            /* material.rs:52-55 */
int rt1w_material_metal(rt1w_scene* s, const double albedo[3], double fuzz);/* material.rs:57-61 */
int rt1w_material_dielectric(rt1w_scene* s, double ir);                     /* material.rs:127-130 */
int rt1w_material_diffuse_light(rt1w_scene* s, int emit_texture);           /* material.rs:63-66 */
int rt1w_material_null(rt1w_scene* s);                                      /* impl Material for () material.rs:68 */

/* Hittable implementors.  Return a hittable id.  A hittable id may be used as
 * a child exactly once (the reference owns children by Box). */
int rt1w_hittable_sphere(rt1w_scene* s, const double center[3], double radius, int material);  /* sphere.rs:16-20 */
int rt1w_hittable_moving_sphere(rt1w_scene* s, const double center0[3], const double center1[3],
                                double time0, double time1, double radius, int material);      /* moving_sphere.rs:13-20 */
int rt1w_hittable_xy_rect(rt1w_scene* s, double x0, double x1, double y0, double y1, double k, int material); /* aarect.rs:15-22 */
int rt1w_hittable_xz_rect(rt1w_scene* s, double x0, double x1, double z0, double z1, double k, int material); /* aarect.rs:25-32 */
int rt1w_hittable_yz_rect(rt1w_scene* s, double y0, double y1, double z0, double z1, double k, int material); /* aarect.rs:35-42 */
int rt1w_hittable_aabox(rt1w_scene* s, const double p0[3], const double p1[3], int material);  /* AABox::new aabox.rs:22-84 (draws rng) */
int rt1w_hittable_translate(rt1w_scene* s, int child, const double offset[3]);                 /* hittable.rs:49-52 */
int rt1w_hittable_rotate_y(rt1w_scene* s, int child, double time0, double time1, double angle_deg); /* RotateY::new hittable.rs:158-202 */
int rt1w_hittable_flip_face(rt1w_scene* s, int child);                                         /* hittable.rs:61 */
int rt1w_hittable_constant_medium(rt1w_scene* s, int boundary, double density, int texture);   /* ConstantMedium::new constant_medium.rs:22-28 */
int rt1w_hittable_bvh(rt1w_scene* s, const int* children, uint32_t n, double time0, double time1); /* BVHNode::new bvh.rs:54-103 (draws rng) */

/* what `main` hands to the pixel loop (src/main.rs:807-951) */
int rt1w_scene_set_world(rt1w_scene* s, int hittable);
int rt1w_scene_set_lights(rt1w_scene* s, const int* hittables, uint32_t n); /* n = 0: `lights = None` -> ray_color_without_light_objects */
int rt1w_scene_set_background(rt1w_scene* s, const double rgb[3]);
int rt1w_scene_set_camera(rt1w_scene* s, const double look_from[3], const double look_at[3],
                          const double vup[3], double vfov_deg, double aspect_ratio,
                          double aperture, double focus_dist, double time0, double time1); /* Camera::new camera.rs:22-59 */
/* BVH is already built by the constructors; commit flattens the graph into the
 * device record arrays and freezes the scene. */
int rt1w_scene_commit(rt1w_scene* s);

/* the scene table of `main` (src/main.rs:815-937): arm 0 random_scene, 1 two_spheres,
 * 2 two_perlin_spheres, 3 earth, 4 simple_light, 5 cornel_box, 6 cornel_smoke,
 * any other final_scene; built through the constructors above.  `aspect_ratio`
 * is what `main` passes to Camera::new (1.0 for arms 5,6,7; 16/9 otherwise, or
 * the caller's override).  `earth_rgb8` (1024x512 decoded assets/earthmap.jpg or
 * any RGB8 image) is needed by arms 3 and 7, else may be NULL.
 * `defaults[3]` receives the arm's image_width, image_height, samples_per_pixel. */
int rt1w_scene_build_reference(int arm, uint64_t build_seed, double aspect_ratio,
                               const uint8_t* earth_rgb8, uint32_t earth_w, uint32_t earth_h,
                               rt1w_scene** out, uint32_t defaults[3]);
/* The arguments rt1w_scene_build_reference hands to rt1w_scene_set_camera for `arm` (main.rs:798-800, the arms' overrides :816-936,
 * Camera::new :941-951) besides the caller's aspect_ratio and the times 0, 1: what a host that moves a reference arm's camera
 * (rt1w_context_set_camera) starts from.  No scene is built. */
int rt1w_reference_camera(int arm, double look_from[3], double look_at[3], double vup[3], double* vfov_deg, double* aperture, double* focus_dist);

/* OPT-IN traversal order of the BVHs.  Default RT1W_WALK_REFERENCE: every BVH node's children are visited
 * left then right exactly as `BVHNode::hit` does (src/bvh.rs:38-47) -- the walk then tests the very primitives the reference
 * tests, in its order, which is what makes the default results provably the reference's.  RT1W_WALK_NEAR_FAR visits the
 * child on the ray's near side first (fewer node visits: the closest hit is found earlier and prunes the rest).  The
 * closest hit does not depend on the order; what does is (a) which of two primitives hit at exactly the same t wins -- kept
 * the reference's by preferring the larger pre-order index -- (b) the random numbers a ConstantMedium draws while being
 * visited -- kept by leaving every node with a medium below it in the reference's order -- and (c) primitive tests the
 * reference never runs because a box test with a fresher t_max pruned them: equal "almost surely" (a primitive hit outside
 * its own bounding box by rounding would be needed) -- except for MovingSphere: the reference gives a scattered ray
 * time = hit t (src/main.rs:86,145), which moves such a sphere far outside the box the BVH holds for it, so whether it is
 * tested depends on the order.  RT1W_WALK_NEAR_FAR therefore also leaves subtrees with moving spheres in the reference's
 * order: with it the FRAMES were identical on every scene tested (all eight arms, random graphs), but that is a measurement, not
 * a proof -- on axis-aligned geometry a box's entry distance can equal a neighbouring face's hit distance, so which of two
 * edge-on hits survives a prune can depend on the order -- and path lengths (rt1w_stats.segments) may differ for a few rays.
 * RT1W_WALK_NEAR_FAR_ALL reorders the moving-sphere subtrees too and does change frames (measured on random_scene: 2 of
 * 9600 pixels differ at 4 spp).  Call on a committed scene, before creating contexts. */
#define RT1W_WALK_REFERENCE 0u
#define RT1W_WALK_NEAR_FAR 1u
#define RT1W_WALK_NEAR_FAR_ALL 2u
int rt1w_scene_set_walk_order(rt1w_scene* s, uint32_t mode);

/* OPT-IN build of the BVHs.  Default RT1W_BVH_REFERENCE: `BVHNode::new` as written -- a random axis per
 * node, objects sorted by their box minimum on it, split at the median (src/bvh.rs:84-100).  RT1W_BVH_SAH rebuilds the tree
 * over every BVH's leaf set by the surface-area heuristic (each split minimises area(L)*|L| + area(R)*|R| over the three axes
 * and every position of the centroid order; boxes are still `surrounding_box` of the children, src/aabb.rs:42-55): fewer
 * node visits per ray.  The closest hit of a ray does not depend on the tree, but everything that depends on the ORDER of the
 * walk does -- ties in t, the random numbers a ConstantMedium draws while visited, MovingSphere tests of scattered rays
 * (see rt1w_scene_set_walk_order) -- so frames are the reference's only statistically, never bit for bit in general
 * (measured: DESIGN.md section 5).  Combine with RT1W_WALK_NEAR_FAR* freely.  Call on a committed scene, before creating
 * contexts; RT1W_ERR_UNSUPPORTED (scene unchanged) if the rebuilt trees need a deeper traversal stack than the kernels have. */
#define RT1W_BVH_REFERENCE 0u
#define RT1W_BVH_SAH 1u
/* RT1W_BVH_BEST_AXIS: `BVHNode::new` as written -- the reference's sort key, stable order, median split and one- / two-object shapes
 * (src/bvh.rs:60-100) -- with the axis of src/bvh.rs:84 CHOSEN (the one whose median split has the lowest area(L)*|L| + area(R)*|R|)
 * instead of drawn from the entropy-seeded generator of src/main.rs:803.  Every axis sequence is a tree some run of the reference
 * builds, so unlike RT1W_BVH_SAH this is a tree the reference itself can produce; nested `BVHNode::new` calls stay separate BVHs.
 * In its topology stream (rt1w_scene_get_bvh_topology) a leaf's number is the object's position in the list its `BVHNode::new` call
 * received (src/bvh.rs:55), and a BVHNode that is an object of another BVH is a leaf whose own tree follows its number. */
#define RT1W_BVH_BEST_AXIS 2u
int rt1w_scene_set_bvh_build(rt1w_scene* s, uint32_t mode);
/* The trees RT1W_BVH_SAH built in place of `BVHNode::new` (src/bvh.rs:54-103), written down so that they can be checked from
 * outside (tests feed them to the literal oracle, which then runs `BVHNode::hit` src/bvh.rs:25-50 over the same trees).
 * One stream of int32 for the whole scene, the rebuilt BVHs in the order the flattener meets them (depth first): each tree in
 * pre-order, -1 = an inner node (`BVHChild::Two`, its two subtrees follow), -2 = a `BVHChild::One` (its one object follows: an
 * object whose sibling is a subtree keeps a node of its own with its own box, as in the reference's trees, src/bvh.rs:63-70),
 * k >= 0 = the k-th leaf of that BVH counted left to
 * right through the tree `BVHNode::new` had built (nested BVHNodes are merged into their parent's leaf set); what a leaf holds
 * inside (an AABox's side BVH, a wrapped BVH, a medium's boundary) follows right after the leaf's number.  Returns the number
 * of entries (0 under RT1W_BVH_REFERENCE); `out` may be NULL to ask for the size. */
int64_t rt1w_scene_get_bvh_topology(const rt1w_scene* s, int32_t* out, uint64_t capacity);

/* introspection of the committed flat scene (tests, DESIGN.md numbers) */
typedef struct rt1w_scene_info {
    uint32_t n_nodes, n_lights, n_materials, n_textures, n_perlin;
    uint32_t stack_need;   /* traversal stack entries the scene needs */
    uint32_t scope_depth;  /* deepest wrapper nesting */
    uint32_t has_media;
    uint32_t has_textures; /* any non-solid texture */
    uint32_t has_moving;   /* any MovingSphere */
    uint32_t variant;      /* kernel variant rt1w_render picks (V0..V5) */
    uint64_t bytes;        /* bytes uploaded per context */
} rt1w_scene_info;
int rt1w_scene_get_info(const rt1w_scene* s, rt1w_scene_info* out);
/* copy of the flat arrays (the exact bytes a context uploads); `what`: 0 nodes,
 * 1 lights, 2 materials, 3 textures, 4 perlin, 5 images, 6 camera+background.
 * Returns bytes written, or needed size if buf==NULL. */
int64_t rt1w_scene_copy_flat(const rt1w_scene* s, int what, void* buf, uint64_t cap);

/* ---- execution (replaces src/main.rs:957-1001) ---- */

int rt1w_device_count(void);
/* uploads the committed scene's flat arrays once (they are immutable afterwards); loads the scene-specialised kernel if the kernel
 * cache has it; counts node visits in a 128 x 128 x 1 render of the scene's own camera (5-15 ms) to rank the records the stack-walk
 * kernels keep in LDS (csrc/rt_walk_table.h) */
int rt1w_context_create(int device_id, const rt1w_scene* s, rt1w_context** out);
void rt1w_context_destroy(rt1w_context* c);

#define RT1W_OUT_SUM 1u   /* write raw per-pixel sums (for sample-range sharding) instead of into_sampled means */
#define RT1W_LDS_NODES 4u /* experiment: stack variants read node records from an LDS copy (scenes <= 1024 nodes); measured slower than the default */
#define RT1W_GENERIC 8u   /* do not use a scene-specialised kernel even if the context has one (rt1w_context_specialise) */
#define RT1W_WAVEFRONT 16u /* opt-in, big scenes (stack-walk variants) and the one-shot entries only: path state queued in HBM as SoA records, a trace kernel + a shade kernel per bounce, a finish kernel for the tail; bit-identical to the default, measured 0.4-0.9x its speed (docs/LAB_NOTES.md).  Since round 4 the form lives in the diagnostics library librt1w_lab.so (csrc/wavefront.hip), which registers itself with librt1w.so when it is loaded: without it the flag answers RT1W_ERR_UNSUPPORTED.  Scenes that run a sweep kernel ignore the flag (stats.sorted bit 3 says what ran); rt1w_render_rows refuses it */
#define RT1W_OUT_FRAME 32u /* rt1w_render only: `out_rgb` is the WHOLE image [height][width][3] (row 0 = j = 0) and the call writes just its tile's pixels at their image positions -- several contexts / processes fill one (shared, pinned) host frame: the host gather of the image-tiled multi-GPU job */
#define RT1W_RNG_REFERENCE 64u /* PARITY MODE: draw from the reference's own generator instead of the Philox streams -- `StdRng::seed_from_u64(j * image_width + i)` (src/main.rs:964; ChaCha12, rand 0.8.4), one stream per pixel drawn on through all its samples in order (sample_offset must be 0, global_seed is ignored).  The frame is then the Rust program's own, pixel for pixel: the GPU reproduces rest_of_your_life.png.  Slower than the default (a lane owns a pixel for all its samples) */
#define RT1W_CLASSIC_WALK 128u /* tests/ablation: sphere scenes (random_scene) walk their BVH with the pair walk of csrc/rt_walk_pair.h by default (box work and leaf work in separate phases, inner boxes in f32 rounded outward, every sphere gated by its group's own f64 box at the reference's moment: the same frames bit for bit, stats.sorted bit 7 says it ran); this flag keeps the one-entry-per-step walk.  Likewise scenes whose every ConstantMedium is bounded by a bare Sphere (final_scene) run stack-walk kernels built without the general boundary walks (rt_flat.h: RtCfgSphereMedia; stats.sorted bit 8); this flag keeps the general kernels */
#define RT1W_PROBE_COHERENT 0x40000000u /* MEASUREMENT ONLY -- the frame written is NOT the image: every wave's 64 lanes trace the SAME path (one pixel of every 8x8 block, each 64 times), so the kernel runs without divergence and its instruction count per traced segment (rocprofv3 SQ_INSTS_VALU x 64 / stats.segments) is what ONE path needs in this kernel's code: the `necessary` side of bench.py's `roofline.valu` (tools/bench_pmc.sh).  Replaces nothing of the reference: a property of this implementation's measurement */
#define RT1W_NO_NODE_CACHE 0x10000u /* tests/ablation: big scenes' stack-walk kernels keep the most visited node records in LDS (csrc/rt_walk_table.h: ranked by a visit count at context creation; stats.sorted bit 10 says the cache ran; same frames bit for bit); this flag keeps the kernels that read every record from memory */
#define RT1W_TILES_SPECIALISED 0x40000u /* rt1w_render_tiles[_device] and the adaptive entries whose rounds go through them: run the tile-list form of the scene-specialised kernel where the context can load one from a kernel cache (the build's, or the user's after rt1w_context_specialise with RT1W_SPECIALISE_TILES), the generic tile-list kernel otherwise -- the same bits either way, a tile render never compiles, stats.sorted bit 2 says which ran.  Excludes RT1W_GENERIC.  The rectangle entries ignore the bit */
#define RT1W_UNSORTED 2u  /* tests/ablation: use the plain persistent kernel (no workgroup-level path reordering: neither the reordering kernel of the small scenes nor, for sphere-media scenes such as final_scene, the reordering of the finished paths at the end of every slice of the stack walk, stats.sorted bit 9) */
#define RT1W_FORCE_VARIANT(v) ((((uint32_t)(v)) + 1u) << 8) /* tests: force kernel variant v (must be valid for the scene) */

typedef struct rt1w_render_params {
    uint32_t width, height;         /* image_width, image_height (src/main.rs:799,939) */
    uint32_t x0, y0, tile_w, tile_h;/* tile to render; y is the reference's row index j (j = height-1 is the TOP row of the PPM) */
    uint32_t spp;                   /* samples_per_pixel rendered by this call */
    uint32_t sample_offset;         /* first absolute sample index; 0 unless sharding samples */
    uint32_t max_depth;             /* MAX_DEPTH = 50 (src/main.rs:801) */
    uint32_t global_seed;
    uint32_t chunk;                 /* samples per work item, 0 = library default (rt1w_scene_default_chunk) */
    uint32_t flags;                 /* RT1W_OUT_* */
    /* Row-interleaved tile, for tiling ONE image over several GPUs with balanced load (the reference hands rows to rayon
     * workers, src/main.rs:957-963; Cornell rows differ in cost by region): the tile's rows are strips of `strip_rows`
     * image rows taken every `strip_period` rows, i.e. tile row r is image row y0 + (r / strip_rows) * strip_period +
     * r % strip_rows.  Rank k of n passes y0 = k * strip_rows, strip_period = n * strip_rows, tile_h = the rows it owns.
     * Both 0: an ordinary contiguous tile.  One launch renders all of the rank's strips. */
    uint32_t strip_rows, strip_period;
    uint32_t precision;             /* RT1W_PRECISION_*: 0 = f64, the reference's `type Float = f64` (src/main.rs:1) */
    uint32_t partial_mib;           /* memory-constrained hosts / tests: upper bound, in MiB, of the buffer of chunk partial sums (24 B per work item); 0 = 8192.
                                       A render that needs more runs as several passes over sample ranges -- the same bits (rt1w_scene_default_chunk) */
} rt1w_render_params;
#define RT1W_PRECISION_F64 0u
/* the reference's switch set the other way, `type Float = f32`: rays, hit records, boxes, camera and colours in f32 (the
 * random draws are still made in 64 bits and rounded, the elementary functions are evaluated in 64 bits and rounded once, a
 * pixel's samples are summed in f64).  Statistically equal to the f64 frame, not bitwise.  Runs the generic kernels, or the
 * f32 build of the scene-specialised kernel where rt1w_context_specialise made one (renders themselves never compile). */
#define RT1W_PRECISION_F32 1u

typedef struct rt1w_stats {
    uint64_t paths;        /* pixels * spp */
    uint64_t segments;     /* traced rays (camera + bounces) */
    double kernel_ms;      /* HIP-event time of the render kernel(s) on the context's stream */
    double total_ms;       /* host wall time of the call incl. device->host copy */
    uint32_t chunk, n_chunks;
    uint32_t grid, block;
    uint32_t variant;      /* feature variant of the kernel (V0..V5: rt_flat.h).  With bit 2 of `sorted` set the kernel that ran is the
                              scene-specialised SWEEP kernel whatever walk this number names (scenes of 65-256 nodes report a stack
                              variant here because that is what the generic code would have used) */
    uint32_t sorted;       /* bit 0: the reordering kernel ran; bit 1: node records in LDS; bit 2: scene-specialised kernel; bit 3:
                              wavefront form; bit 4: reference-stream kernel (RT1W_RNG_REFERENCE); bit 5: f32 kernel; bit 7: pair walk
                              (sphere scenes); bit 8: sphere-media build of the stack walk; bit 9: finished paths reordered across the
                              workgroup at the end of every slice of the stack walk; bit 10: most visited node records in LDS (walk table) */
    uint32_t passes;       /* launches of the trace kernel the call made: a render whose chunk partial sums exceed the budget
                              (rt1w_render_params.partial_mib) runs as several sample passes; rt1w_render_rows sums them over its
                              strips; 1 for the wavefront form and the AOV entries */
    uint32_t reserved;     /* 0 */
} rt1w_stats;

/* ---- a list of tiles in one launch ----
 * One record of the list, 16 bytes (not one of rt1w_abi_sizeof's: bindings assert the 16 themselves). */
typedef struct rt1w_tile { uint32_t x0, y0, sample_offset, reserved; } rt1w_tile;   /* 16 bytes, reserved = 0 */
/* Renders n_tiles square tiles of side `tile` (a multiple of 16 in 16 .. 256; x0 and y0 multiples of it, inside the p->width x p->height
 * frame; n_tiles 1 .. 2^20) by ONE launch of the trace kernel per sample pass.  `tiles` is HOST memory in both forms (uploaded into a
 * context buffer that grows on demand).  From p: width, height, spp (the same for every tile), max_depth, global_seed, chunk, partial_mib,
 * flags; p->x0, y0, tile_w, tile_h are ignored; p->sample_offset is added to every tile's own (a sum + spp beyond 2^32 - 1:
 * RT1W_ERR_INVALID).  chunk 0 means rt1w_scene_default_chunk(scene, width, height, spp) of the WHOLE frame.
 * out: double[n_tiles][tile][tile][3], tile k's row 0 = image row y0_k; raw sums with RT1W_OUT_SUM, else into_sampled means.  A pixel of
 * a tile beyond the frame's right or top edge is never traced and comes back as +0.0.
 * CONTRACT: tile k's pixels inside the frame are bit-identical to rt1w_render_device of the rectangle (x0_k, y0_k, min(tile, width - x0_k),
 * min(tile, height - y0_k)) with the same spp and seed, the tile's absolute sample offset and the same chunk passed explicitly.  The order
 * of the list, repeats of a tile with other offsets and partial_mib do not change a bit.
 * Flags: 0, RT1W_OUT_SUM, RT1W_GENERIC (a no-op: without RT1W_TILES_SPECIALISED the tile entries run the generic kernels, which render
 * the same bits as the scene-specialised ones), RT1W_TILES_SPECIALISED (alongside RT1W_OUT_SUM or alone: the tile-list form of the
 * scene-specialised kernel if the context can load one from a kernel cache -- looked up at the first such call, never compiled here --
 * and the generic tile-list kernel otherwise, without an error; the contract above holds unchanged; with RT1W_GENERIC:
 * RT1W_ERR_INVALID); any other flag, interleaved strips or a non-zero `reserved`: RT1W_ERR_INVALID; RT1W_PRECISION_F32:
 * RT1W_ERR_UNSUPPORTED.
 * stats: paths = pixels inside the frame x spp; segments = rays traced (the sum over the per-rectangle renders); passes = launches of the
 * trace kernel; variant / sorted / grid / block / chunk / n_chunks as rt1w_render with RT1W_GENERIC, or, where the specialised tile-list
 * kernel ran (sorted bit 2), that kernel's sorted bits, grid and block. */
int rt1w_render_tiles(rt1w_context* c, const rt1w_render_params* p, uint32_t tile, const rt1w_tile* tiles, uint32_t n_tiles, double* out, rt1w_stats* stats);
int rt1w_render_tiles_device(rt1w_context* c, const rt1w_render_params* p, uint32_t tile, const rt1w_tile* tiles, uint32_t n_tiles, void* d_out, rt1w_stats* stats);

/* default work-item size for a (tile, spp): deterministic, documented in DESIGN.md.  This is the scene-independent rule (what the
 * small scenes' reordering kernels run with); see rt1w_scene_default_chunk for what a render of a given scene uses */
uint32_t rt1w_default_chunk(uint32_t tile_w, uint32_t tile_h, uint32_t spp);
/* The work-item size rt1w_render* use for THIS scene when rt1w_render_params.chunk is 0 (the samples of a pixel are summed per work
 * item, then the items in order: src/main.rs:966-992 sums them all in order, which is the case chunk = 1).  Scenes that run a
 * stack-walk kernel (more than 64 nodes) take ONE sample per item: a lane whose path ended fetches its next item with the other free
 * lanes of its wave, so they restart on neighbouring pixels (coherent camera rays; measured +8-15 % on final_scene / random_scene),
 * and the pixel sum is the reference's own sequential sum; scenes on the sweep kernels keep rt1w_default_chunk.  Renders whose
 * partial sums would not fit 8 GiB run as several passes over sample ranges with the same bits.  A host that tiles one image over
 * several GPUs passes this value (for the WHOLE frame) as `chunk` to every tile.  Committed scenes only (0 otherwise). */
uint32_t rt1w_scene_default_chunk(const rt1w_scene* s, uint32_t tile_w, uint32_t tile_h, uint32_t spp);

/* Renders the tile into caller memory: out_rgb[(y - y0) * tile_w + (x - x0)][3],
 * row 0 = j = y0.  Values are the reference's `pixel_color.into_sampled(spp)`
 * (src/main.rs:992, color.rs:14-21), i.e. linear f64 means before gamma, or raw
 * sums with RT1W_OUT_SUM. */
int rt1w_render(rt1w_context* c, const rt1w_render_params* p, double* out_rgb, rt1w_stats* stats);
/* same, but `d_out_rgb` is a device pointer on the context's GPU (e.g. a torch
 * tensor); no host copy.  Synchronises the context's stream before returning. */
int rt1w_render_device(rt1w_context* c, const rt1w_render_params* p, void* d_out_rgb, rt1w_stats* stats);

/* same render, but the tile comes back already quantised ON THE DEVICE exactly as the reference prints it
 * (Display for SampledColor src/color.rs:56-65: (256 * sqrt(c).clamp(0, 0.999)) as usize) and in the reference's row
 * order (top row = j = y0 + tile_h - 1 first, src/main.rs:957-960,1003-1007): out_rgb8[tile_h][tile_w][3].  No host
 * post-pass, 1/8 of the device->host bytes.   */
int rt1w_render_u8(rt1w_context* c, const rt1w_render_params* p, uint8_t* out_rgb8, rt1w_stats* stats);

/* Strip-wise render with progress, for big frames (C5 is 199 MB of f64 means).  The reference renders the rows top-down
 * and reports progress as rows finish (src/main.rs:957-960 row order, :995-998 the stderr progress line).  This entry
 * traces the tile in strips of `strip_rows` image rows from the top row (j = y0 + tile_h - 1) downwards; the finished strip
 * is copied to the host on a second stream while the next one is traced, and `progress(user, rows_done, rows_total)` is
 * called on the calling thread each time a strip has landed in `out` (rows_done counts from the top).  A non-zero return
 * from the callback stops the render: strips already reported are valid, the call returns RT1W_ERR_CANCELLED.
 *   format RT1W_ROWS_F64: out = double[tile_h][tile_w][3], the layout of rt1w_render (row 0 = j = y0);
 *   format RT1W_ROWS_U8 : out = uint8_t[tile_h][tile_w][3], the layout of rt1w_render_u8 (top row first), so a PPM writer can
 *                         stream rows out as they are reported.
 * Every strip uses the sample-chunk size of the whole tile, so the result is bit-identical to rt1w_render / rt1w_render_u8.
 * strip_rows = 0 picks about 16 strips, fewer when a strip would hold less than ~4M (pixel, sample-chunk) work items.  `progress` may be NULL.  stats (optional) are totals over the strips. */
#define RT1W_ROWS_F64 0
#define RT1W_ROWS_U8 1
typedef int (*rt1w_progress_fn)(void* user, uint32_t rows_done, uint32_t rows_total);
int rt1w_render_rows(rt1w_context* c, const rt1w_render_params* p, uint32_t strip_rows, int format, void* out,
                     rt1w_progress_fn progress, void* user, rt1w_stats* stats);

/* ---- first-hit feature buffers (AOVs): what a denoiser or a learning / compositing host takes next to the frame ----
 * For every pixel of the tile, samples sample_offset .. sample_offset + spp - 1.  Each sample's camera ray is EXACTLY the camera ray of
 * that sample in rt1w_render: the same stream, the same u, v jitter, lens draw and time (src/main.rs:964-971, camera.rs:61-73).  Only
 * that ray is traced, with world.hit(ray, 0.001, inf) (main.rs:62); a ConstantMedium draws its free flight from the same stream, as the
 * first segment of the beauty path does.  So the first hit of AOV sample k is the first hit of beauty sample k.
 * Every pixel gets RT1W_AOV_CHANNELS doubles; channels 0-5 and 7 are sums over the samples, in sample order, divided by spp; channel 6
 * is the sum over the samples that hit divided by their count:
 *   0-2 albedo   hit: Lambertian / Isotropic the albedo texture's value at (u, v, p) (material.rs:71-80, constant_medium.rs:37-50);
 *                Metal its `albedo` (material.rs:99-111); Dielectric (1, 1, 1); DiffuseLight emitted(u, v, p) at the hit -- front face:
 *                the emit texture, else 0 (material.rs:163-178); `()` 0.   miss: the scene's background.
 *   3-5 normal   hit: HitRecord.normal in world space -- it faces against the ray, FlipFace does not flip it, a medium's is (1, 0, 0)
 *                (hittable.rs:30-35, :206-270, constant_medium.rs:101); the mean is not renormalised.   miss: (0, 0, 0).
 *   6 depth      distance from the ray origin to the hit, t * |d|, averaged over the samples that hit; +inf if no sample hits.
 *   7 coverage   hit 1, miss 0.
 * Layout double[tile_h][tile_w][8], row 0 = j = y0, as rt1w_render; an interleaved tile (strip_rows / strip_period) maps its rows as
 * rt1w_render does.  max_depth, chunk and partial_mib are ignored; flags may be 0 or RT1W_FORCE_VARIANT(v) (tests), anything else is
 * RT1W_ERR_INVALID; precision must be RT1W_PRECISION_F64 (RT1W_ERR_UNSUPPORTED otherwise).  stats: paths = segments = pixels * spp,
 * kernel_ms (HIP events), total_ms, grid, block, variant.  One lane per pixel runs its samples in order: deterministic sums, bit-identical
 * to the CPU build of the same code (librt1w_lab.so: rt1w_lab_aov_host).  None of the render kernels is involved. */
#define RT1W_AOV_CHANNELS 8
/* into caller host memory: out_aov[tile_h][tile_w][8] (through the context's device framebuffer) */
int rt1w_render_aov(rt1w_context* c, const rt1w_render_params* p, double* out_aov, rt1w_stats* stats);
/* same, into device memory on the context's GPU (e.g. a torch tensor); no host copy.  Synchronises the context's stream before returning. */
int rt1w_render_aov_device(rt1w_context* c, const rt1w_render_params* p, void* d_out_aov, rt1w_stats* stats);

/* ---- deep feature buffers: the same 8 channels at the first vertex of the sample's path that is not a specular surface ----
 * What is seen through glass or in a mirror gets the guides of what is seen, not of the glass or the mirror.  For every pixel of the
 * tile and every sample k of sample_offset .. sample_offset + spp - 1:
 *   1. start as rt1w_render_aov does: the camera ray of beauty sample k, world.hit(ray, 0.001, inf) (main.rs:62);
 *   2. continue while the ray hits, the hit material is SPECULAR -- a Dielectric, or a Metal whose fuzz <= max_fuzz -- and fewer than
 *      max_specular bounces have been followed;
 *   3. to continue, scatter exactly as the beauty path does: Dielectric::scatter (material.rs:133-160) with its one draw,
 *      Metal::scatter (material.rs:99-111) with its random_in_unit_sphere even at fuzz 0; a throughput beta (1 at the start) is
 *      multiplied by the attenuation, the scattered ray keeps the ray's time.  The stream stays in step with rt1w_render's, so the
 *      chain followed is the chain beauty sample k follows (as long as that path is alive: max_depth is not looked at here);
 *   4. at the vertex where it stops:
 *        0-2 albedo   beta (.) the albedo rule of rt1w_render_aov at that vertex; beta (.) background if the last ray missed;
 *        3-5 normal   that vertex's HitRecord.normal; (0, 0, 0) if the last ray missed;
 *        6 depth      the sum of t * |d| over all segments of the chain that hit (the length of the folded-out path);
 *        7 coverage   1 if the last ray hit, 0 if it missed;
 *   5. a chain still on a specular surface after max_specular bounces stops there and takes that surface as its vertex.
 * Sums, divisions (depth: over the samples whose last ray hit, +inf if none), layout, tiles, strips, flags, precision and argument
 * checks are those of rt1w_render_aov.  max_specular = 0 is rt1w_render_aov, bit for bit; with max_fuzz = 0 only Dielectrics and
 * perfect mirrors are followed.  max_specular > 64, or a max_fuzz that is negative or not finite: RT1W_ERR_INVALID.
 * stats: paths = pixels * spp; segments = the rays actually traced (counted per lane, summed per wave, one atomic add per wave);
 * kernel_ms, total_ms, grid, block, variant as rt1w_render_aov.  One lane per pixel runs its samples in order: bit-identical to the CPU
 * build of the same code (librt1w_lab.so: rt1w_lab_aov_deep_host).  None of the render kernels is involved. */
int rt1w_render_aov_deep(rt1w_context* c, const rt1w_render_params* p, uint32_t max_specular, double max_fuzz, double* out_aov, rt1w_stats* stats);
/* same, into device memory on the context's GPU; no host copy.  Synchronises the context's stream before returning. */
int rt1w_render_aov_deep_device(rt1w_context* c, const rt1w_render_params* p, uint32_t max_specular, double max_fuzz, void* d_out_aov,
                                rt1w_stats* stats);

/* ---- ray queries: Hittable::hit of the scene's world for a list of the caller's own rays ----
 * For every ray r of 0 .. n - 1: world.hit(ray, t_min, t_max, rng) -> Option<HitRecord> (hittable.rs:63-64, HitRecord hittable.rs:10-18),
 * exactly as the first segment of a beauty path does it (main.rs:62, bvh.rs:25-50) but with the caller's ray and bounds: the walk is
 * the scene variant's own, in the reference's order; ties between equal t and the time a MovingSphere is evaluated at are those of the
 * render kernels.  The direction is NOT normalised: t is in units of it, p = origin + t * direction (ray.rs:12-14).
 *   rays  double[n][9] = origin xyz, direction xyz, time (Ray, ray.rs:5), t_min, t_max (the two bounds of `hit`).
 *   out   double[n][12]:
 *           0     hit 1, miss 0
 *           1     t
 *           2-4   p: the hit point in world space (a Translate / RotateY above the leaf moves it back as hittable.rs:215-225, :255-278 do)
 *           5-7   normal in world space, against the ray (hittable.rs:30-35); a ConstantMedium's is (1, 0, 0) (constant_medium.rs:101)
 *           8, 9  u, v of the leaf (sphere.rs:50-62, aarect.rs:58-71) WHERE THE HIT MATERIAL'S TEXTURE READS THEM -- an image texture
 *                 (texture.rs:67-89) somewhere in its texture tree --, else 0: the kernels do not compute what no texture looks at
 *           10    front_face 1 or 0; a FlipFace flips this flag only, not the normal (hittable.rs:288-291)
 *           11    index of the hit material in the scene's material table: the id the rt1w_material_* constructor returned.  The
 *                 Isotropic of a ConstantMedium (constant_medium.rs:22-28) has no constructor of its own: it takes the next free id at
 *                 the moment rt1w_hittable_constant_medium is called, so ids handed out later skip it
 *   out_node  (may be NULL) uint32[n]: the pre-order index of the hit leaf's record in the flattened node array, the array
 *             rt1w_scene_copy_flat(.., 0, ..) exports (a ConstantMedium's own record for a hit inside it).
 *   A miss writes 0 into all 12 slots and 0xFFFFFFFF as the node.
 * Media: ConstantMedium::hit draws (constant_medium.rs:58-113, the free flight of :85).  Ray r draws from the Philox stream of
 * (pixel seed first_stream + r, sample `sample`, `global_seed`) -- the stream a render gives that pixel's sample -- starting at the
 * stream's FIRST word (a render's sample has drawn its camera ray before).  A list split into two calls, the second with first_stream
 * advanced by the rays of the first, therefore gives the same records, bit for bit.  A scene without media draws nothing.
 * ONE DEVIATION from the literal hit(): a ray with a non-finite value (an infinity or a NaN) among origin, direction and time, or with
 * a NaN for t_min or t_max, is answered as a miss before any walk.  A t_max of +inf is allowed, and everything finite is literal: a
 * zero direction, denormals, t_min > t_max.
 * RT1W_ERR_INVALID: a null context, params, rays or out; n = 0 or n > 2^32 - 1; global_seed >= 2^32 (the streams take 32 bits of it);
 * flags other than 0 or RT1W_FORCE_VARIANT(v) with a v that covers the scene (tests); out or out_node overlapping rays or each other.
 * stats: paths = segments = n, kernel_ms (HIP events), total_ms, grid, block, variant.  One lane per ray, 64 consecutive rays per wave;
 * the list is not reordered.  Bit-identical to the CPU build of the same code (librt1w_lab.so: rt1w_lab_hit_host).  None of the render
 * kernels is involved. */
typedef struct rt1w_hit_params {
    uint64_t n;            /* rays */
    uint64_t first_stream; /* ray r draws from the stream of pixel seed first_stream + r */
    uint64_t global_seed;  /* as rt1w_render_params.global_seed; below 2^32 */
    uint32_t sample;       /* the stream's sample index */
    uint32_t flags;        /* 0 or RT1W_FORCE_VARIANT(v) */
} rt1w_hit_params; /* 32 bytes */
/* host memory in and out (through the context's device framebuffer, grown on demand and freed with the context) */
int rt1w_hit(rt1w_context* c, const rt1w_hit_params* params, const double* rays, double* out, uint32_t* out_node /* may be NULL */, rt1w_stats* stats);
/* same, on device memory of the context's GPU (e.g. torch tensors): d_rays double[n][9], d_out double[n][12], d_out_node uint32[n] or
 * NULL; no host copy.  Synchronises the context's stream before returning. */
int rt1w_hit_device(rt1w_context* c, const rt1w_hit_params* params, const void* d_rays, void* d_out, void* d_out_node /* may be NULL */,
                    rt1w_stats* stats);

/* ---- radiance queries: ray_color for a list of the caller's own rays ----
 * For every ray r of 0 .. n - 1 and every sample k of 0 .. spp - 1: ray_color(ray, background, world, lights, max_depth, rng) (main.rs:51-116;
 * a scene without lights :118-190) -- the other half of the reference's sample loop (main.rs:964-989), which rt1w_render reaches through
 * Camera::get_ray (camera.rs:61-73) alone.  The rays run through the kernels rt1w_render runs with RT1W_GENERIC -- the reordering
 * kernel of small scenes, the sliced stack walk with the node cache and slice-end reordering, the pair walk of sphere scenes -- built
 * once more with the ray's record where the camera was: traversal, shading, draw order and sums are the render's text.
 *   rays  double[n][stride] = origin xyz, direction xyz, time (Ray, ray.rs:5); the record's other doubles are not read (stride 9 takes
 *         rt1w_hit's records as they are).  The direction is used as given; the bounds are ray_color's own, 0.001 and +inf (main.rs:62).
 *   start_word  (may be NULL: all 0) uint32[n], see below.
 *   out   double[n][3]: with RT1W_OUT_SUM the raw sum over the ray's samples, else Color::into_sampled(sum, spp) (color.rs:14-21, the NaN
 *         scrub included).  The sums are made exactly as rt1w_render makes a pixel's: per work item of `chunk` samples in sample order,
 *         then the items in order.
 * Streams.  Sample k of ray r draws from the Philox stream of (pixel seed first_stream + r, sample sample_offset + k, global_seed) -- the
 * stream a render gives that pixel's sample (main.rs:964) -- starting at word start_word[r] of it: word index = 4 * block + word in block,
 * the RtRngPos of include/rt1w_num.h as one number (rt_rng_at puts a stream there).  The same start_word[r] serves each of the ray's
 * samples.  Two consequences:
 *   - a list split into two calls, the second with first_stream advanced by the first call's ray count, gives the same values bit for bit;
 *   - given the camera ray of pixel (i, j), sample s, and the position that ray's stream has after Camera::get_ray (camera.rs:61-73), with
 *     first_stream + r = j * width + i and sample_offset = s, the entry returns that sample of rt1w_render, bit for bit.
 * ONE DEVIATION from the literal ray_color, the one rt1w_hit has: a ray with a non-finite value (an infinity or a NaN) among origin,
 * direction and time is not traced; each of its samples is a miss -- the background (main.rs:64-66), or 0 at max_depth 0 (main.rs:59-61).
 * Everything finite is literal: a zero direction, denormals, huge values.
 * RT1W_ERR_INVALID: a null context, params, rays or out; n = 0 or n > 2^32 - 1; spp = 0; sample_offset + spp > 2^32 - 1; global_seed >=
 * 2^32; stride 1 .. 6; any flag but RT1W_OUT_SUM and RT1W_GENERIC (RT1W_RNG_REFERENCE included: the reference stream has no positions);
 * reserved != 0; out overlapping rays or start_word.  f64 only: the block has no precision member.
 * stats: paths = n * spp; segments = rays traced (a ray that is not traced counts none); passes, variant, sorted, grid, block, chunk and
 * n_chunks as rt1w_render's with RT1W_GENERIC on a frame of n x 1 pixels.  A context that holds a scene-specialised kernel runs the
 * generic ray-list kernel: the same bits, `sorted` says what ran.  Bit-identical to the CPU build of the same code (librt1w_lab.so:
 * rt1w_lab_ray_color_host). */
typedef struct rt1w_ray_color_params {
    uint64_t n;             /* rays, 1 .. 2^32 - 1 */
    uint64_t first_stream;  /* ray r draws from the streams of pixel seed first_stream + r */
    uint64_t global_seed;   /* as rt1w_render_params.global_seed; below 2^32 */
    uint32_t spp;           /* samples per ray: streams (first_stream + r, sample_offset + k), k = 0 .. spp - 1 */
    uint32_t sample_offset;
    uint32_t max_depth;     /* the `depth` argument of ray_color; 0 gives 0 (main.rs:59-61) */
    uint32_t chunk;         /* samples per work item, 0 = rt1w_scene_default_chunk(scene, (uint32_t)n, 1, spp) */
    uint32_t stride;        /* doubles from one ray record to the next, >= 7; 0 = 7 */
    uint32_t flags;         /* 0, RT1W_OUT_SUM, RT1W_GENERIC (a no-op: the generic kernels run anyway) */
    uint32_t partial_mib;   /* as rt1w_render_params.partial_mib: the budget of the chunk partial sums, 0 = default */
    uint32_t reserved;      /* 0 */
} rt1w_ray_color_params; /* 56 bytes; rt1w_abi_sizeof(8) */
/* host memory in and out (through the context's device buffers, grown on demand and freed with the context); ray_color, main.rs:51-116 */
int rt1w_ray_color(rt1w_context* c, const rt1w_ray_color_params* params, const double* rays, const uint32_t* start_word /* may be NULL */,
                   double* out, rt1w_stats* stats);
/* same, on device memory of the context's GPU (e.g. torch tensors): d_rays double[n][stride], d_start_word uint32[n] or NULL, d_out
 * double[n][3]; no host copy.  Synchronises the context's stream before returning.  ray_color, main.rs:51-116 */
int rt1w_ray_color_device(rt1w_context* c, const rt1w_ray_color_params* params, const void* d_rays, const void* d_start_word /* may be NULL */,
                          void* d_out, rt1w_stats* stats);

/* ---- path states: ray_color one level at a time ----
 * What lies between one world.hit (rt1w_hit) and the whole recursion (rt1w_ray_color): a path as a VALUE, a self-contained 128-byte record
 * that the library advances by a chosen number of levels of ray_color (main.rs:51-116; a scene without lights :118-190).  Between calls the
 * caller may inspect, reorder, compact or split the list, or stop: an integrator of its own, per-bounce contributions, path vertices.
 * Carried to its end a record holds the bits of rt1w_ray_color, and begun at the camera (rt1w_path_begin) the bits of rt1w_render.
 *   bytes    field               meaning
 *   0-55     double ray[7]       origin xyz, direction xyz, time (Ray, ray.rs:5): the NEXT ray to trace
 *   56-79    double beta[3]      product of attenuation * scattering_pdf / pdf so far (main.rs:96-115)
 *   80-103   double radiance[3]  sum of beta (.) terminal values so far
 *   104-111  uint64_t stream     pixel seed of the Philox stream: j * width + i in a render, first_stream + r in the queries
 *   112-115  uint32_t sample     the stream's sample index
 *   116-119  uint32_t word       position in that stream, 4 * block + word in block (rt1w_ray_color's start_word)
 *   120-123  uint32_t depth_left the `depth` argument of ray_color still to spend
 *   124-127  uint32_t status     RT1W_PATH_ALIVE | RT1W_PATH_TRACED | event << 8; all other bits are ignored on input and written as 0
 * RT1W_PATH_TRACED: a level of the entry produced this ray; a caller's fresh state leaves it clear.  The event of the last level taken
 * (RT1W_PATH_EVENT(status)): 0 none yet, 1 miss (the background, main.rs:64-66), 2 depth exhausted (main.rs:59-61), 3 DiffuseLight
 * (emitted, no scatter: material.rs:168-181, main.rs:110-112), 4 `()` (material.rs:68: absorbed), 5 Lambertian, 6 Metal, 7 Dielectric,
 * 8 Isotropic -- the material of the leaf hit, whether or not it scattered --, 9 not traced (a caller's ray that is not finite).
 * Everything a level needs travels in the record; only global_seed is per call.
 *
 * rt1w_path_step advances each of n states by up to `steps` levels while it is alive:
 *   - RT1W_PATH_TRACED clear and one of the seven ray doubles an infinity or a NaN (the ONE DEVIATION rt1w_ray_color has): the level is a
 *     miss that is not traced, radiance += beta (.) (depth_left == 0 ? 0 : background), the state is dead with event 9;
 *   - else one level: the stream of (stream, sample, global_seed) placed at `word`; depth check and world.hit (main.rs:59-62), emitted,
 *     scatter, the next ray (main.rs:63-115); `word` = where the stream stands afterwards, RT1W_PATH_TRACED set, the event written.  A ray
 *     a level produced is traced as it is, finite or not, as the render kernels trace it;
 *   - a dead state is copied unchanged, every bit of it.
 * Split, order and company change no bit: 64 levels in one call, in 64 calls, with the list shuffled or compacted in between.
 *   out_node  (may be NULL) uint32[n]: the hit leaf of the last level the state took, in rt1w_hit's convention; 0xFFFFFFFF for a miss, a
 *             level without depth, a dead state or a ray that is not traced.
 * `in` and `out` may be the same pointer (a state is read whole before it is written); any other overlap is refused.
 * RT1W_ERR_INVALID: a null context, params, in or out; n = 0 or n > 2^32 - 1; steps = 0 or steps > 65536; global_seed >= 2^32; flags other
 * than 0 or RT1W_FORCE_VARIANT(v) with a v that covers the scene; reserved != 0; overlapping buffers; in the device form a state pointer
 * that is not 16-byte aligned (the host form copies and takes any alignment).  f64 and Philox only: the block has no precision member.
 * stats: paths = n; segments = levels that traced a ray, counted as rt1w_ray_color counts them; kernel_ms, total_ms, grid, block, variant
 * as rt1w_hit's.  One lane per state, 64 consecutive states per wave; the list is not reordered.  Bit-identical to the CPU build of the
 * same code (librt1w_lab.so: rt1w_lab_path_step_host). */
#define RT1W_PATH_ALIVE 1u
#define RT1W_PATH_TRACED 2u
#define RT1W_PATH_EVENT(status) (((status) >> 8) & 0xFFu)
typedef struct rt1w_path_state {
    double ray[7];
    double beta[3];
    double radiance[3];
    uint64_t stream;
    uint32_t sample;
    uint32_t word;
    uint32_t depth_left;
    uint32_t status;
} rt1w_path_state; /* 128 bytes; rt1w_abi_sizeof(11) */
typedef struct rt1w_path_params {
    uint64_t n;           /* states, 1 .. 2^32 - 1 */
    uint64_t global_seed; /* as rt1w_render_params.global_seed; below 2^32 */
    uint32_t steps;       /* levels per state at most, 1 .. 65536 */
    uint32_t flags;       /* 0 or RT1W_FORCE_VARIANT(v) */
    uint32_t reserved[2]; /* 0 */
} rt1w_path_params; /* 32 bytes; rt1w_abi_sizeof(10) */
/* host memory in and out (through the context's device buffers, grown on demand and freed with the context); ray_color, main.rs:51-116 */
int rt1w_path_step(rt1w_context* c, const rt1w_path_params* params, const rt1w_path_state* in, rt1w_path_state* out,
                   uint32_t* out_node /* may be NULL */, rt1w_stats* stats);
/* same, on device memory of the context's GPU (e.g. torch tensors): d_in and d_out n states, 16-byte aligned, d_out_node uint32[n] or
 * NULL; no host copy.  Synchronises the context's stream before returning.  ray_color, main.rs:51-116 */
int rt1w_path_step_device(rt1w_context* c, const rt1w_path_params* params, const void* d_in, void* d_out, void* d_out_node /* may be NULL */,
                          rt1w_stats* stats);
/* Fresh states from the context's live camera (rt1w_context_set_camera included): for entry r of pixels = {i, j, sample}, Camera::get_ray
 * (camera.rs:61-73) with the jitter of main.rs:964-971 for that sample of pixel (i, j) of a width x height frame -- the ray rt1w_render
 * begins that sample with --, beta 1, radiance 0, stream = j * width + i, the sample, word = the stream's position behind get_ray,
 * depth_left = max_depth, status RT1W_PATH_ALIVE.  begin -> step* -> radiance is that sample of rt1w_render, bit for bit.
 * RT1W_ERR_INVALID: a null context, pixels or out; width or height below 2 (as a render); n = 0 or n > 2^32 - 1; global_seed >= 2^32; an
 * entry with i >= width or j >= height (its state, and only its, is written as zeros); out overlapping pixels; in the device form an out
 * that is not 16-byte aligned.  stats: paths = n, segments = 0.  Bit-identical to librt1w_lab.so's rt1w_lab_path_begin_host */
int rt1w_path_begin(rt1w_context* c, uint32_t width, uint32_t height, uint64_t global_seed, uint32_t max_depth, const uint32_t* pixels /* [n][3] */,
                    uint64_t n, rt1w_path_state* out, rt1w_stats* stats);
/* same, on device memory: d_pixels uint32[n][3], d_out n states, 16-byte aligned.  camera.rs:61-73 */
int rt1w_path_begin_device(rt1w_context* c, uint32_t width, uint32_t height, uint64_t global_seed, uint32_t max_depth, const void* d_pixels,
                           uint64_t n, void* d_out, rt1w_stats* stats);

/* ---- feature-guided denoiser: the consumer of the feature buffers above ----
 * An edge-avoiding a-trous wavelet filter (Dammertz, Sewtz, Hanika, Lensch 2010) over an image and its first-hit feature buffers.
 * Replaces nothing of the reference, which reaches a clean image by sample count alone (10 000 spp for final_scene, src/main.rs:939).
 *   frame double[h][w][3], the layout of rt1w_render: means, not sums.   aov double[h][w][8], the layout of rt1w_render_aov.
 *   out   double[h][w][3].   A tile is filtered as an image of its own: taps outside the three buffers are skipped, nothing is known of
 *   the pixels around it.  A host that tiles one image over several GPUs denoises the gathered frame.
 * Prepare, per pixel p.  Albedo A_p = max(albedo, eps) per channel, eps = 0.01 (also where the albedo is not finite); with
 *   RT1W_DENOISE_KEEP_ALBEDO A_p = 1.  Value c_p = frame / A_p per channel (demodulation: texture detail stays out of the blur; the
 *   albedo channel holds the emission on lights and the background on misses, so those come through clean).  Luminance
 *   l_p = (0.2126 r + 0.7152 g) + 0.0722 b of c_p.  Unit normal u_p = n_p / |n_p| of the mean normal, (0, 0, 0) where |n_p|^2 is 0,
 *   underflows or is not finite (a miss).  Depth z_p and coverage v_p as they are.
 * Levels i = 0 .. iterations - 1, step s = 2^i.  c'_p = sum_q w(p, q) c_q / sum_q w(p, q) over the taps q = p + s (dx, dy),
 *   dx, dy = -2 .. 2, that lie inside the image, in row order (dy outer, dx inner); l' is the luminance of c'.  The centre tap has
 *   w = h(0, 0) whatever the guides say, so the denominator is never 0.  For the others
 *     w = (h(dx, dy) * w_normal) * k((x_depth + x_colour) + x_coverage),
 *   which is h * w_normal * w_depth * w_colour * w_coverage with each falloff w_x = k(x) and the three multiplied as one k of the sum:
 *     h          = b(|dx|) * b(|dy|), b = 3/8, 1/4, 1/16 (B3 spline);
 *     w_normal   = 1 if u_p and u_q are both (0, 0, 0); else clamp(u_p . u_q, 0, 1) ^ P by binary exponentiation, where P is
 *                  `sigma_normal` truncated to an integer and clamped to 1 .. 4096 (default 32): exactly 0 for perpendicular or
 *                  opposed normals and where exactly one normal is (0, 0, 0);
 *     x_depth    = 0 if z_p == z_q (two misses: both +inf); +inf if exactly one is +inf; else |z_p - z_q| / (max(z_p, z_q) *
 *                  sigma_depth) (default 0.1);
 *     x_colour   = (l_p - l_q)^2 / sigma_i^2 of the current level's values, sigma_i = sigma_colour / 2^i (default 1, halved at every
 *                  level as in the paper); level 0 has NO colour term (x_colour = 0 * (l_p - l_q)^2): the paper's remedy for fireflies
 *                  -- a firefly in the centre pixel would otherwise reject all its neighbours and survive;
 *     x_coverage = (v_p - v_q)^2 * 16 (sigma_coverage = 1/4, not a parameter);
 *     k(x)       = 1 for x <= 0; exp(-x) for 0 < x < 40, evaluated as 2^-n * T13(n ln 2 - x), n = trunc(x / ln 2 + 1/2), T13 the
 *                  Taylor polynomial of exp of degree 13 (csrc/rt_denoise.h: rt_dn_falloff); exactly 0 for x >= 40, +inf and NaN.
 *   A tap is added only if w > 0: a tap whose value or weight is not finite contributes nothing (a value that is not finite has a
 *   luminance that is not finite, so x_colour and with it w is 0 or NaN).  A centre pixel whose luminance is not finite is passed through
 *   every level unchanged.
 * After the last level out = c * A_p per channel.
 * Arithmetic: + - * /, sqrt, comparisons, selects and integer operations in one fixed order, without FMA contraction, each output pixel
 * whole by one lane: bit-identical to the CPU build of the same code (librt1w_lab.so: rt1w_lab_denoise_host).
 * Known limit: with the first-hit buffers the guides describe the first hit: what is seen through a glass sphere or reflected in a
 * metal one is filtered with the glass or metal surface's guides.  The deep buffers (rt1w_render_aov_deep, rt1w_render_denoised_deep)
 * lift it for Dielectrics and for Metals up to a chosen fuzz. */
#define RT1W_DENOISE_KEEP_ALBEDO 1u      /* no demodulation */
typedef struct rt1w_denoise_params {
    uint32_t width, height;              /* of the three buffers */
    uint32_t iterations;                 /* 0 = 5, at most 8 (RT1W_ERR_INVALID beyond) */
    uint32_t flags;                      /* 0 or RT1W_DENOISE_KEEP_ALBEDO */
    double sigma_colour, sigma_normal, sigma_depth;   /* 0 = default; negative or not finite: RT1W_ERR_INVALID */
} rt1w_denoise_params;
/* host buffers, through the context's device buffers (two colour buffers of 32 B per pixel and a guide buffer of 64 B per pixel, which
 * grow on demand and are freed with the context).  `out` may be `frame`.  stats: kernel_ms = HIP-event time of the prepare pass and
 * the level launches, total_ms the whole call, passes 1, grid / block of the level kernel, paths = pixels. */
int rt1w_denoise(rt1w_context* c, const rt1w_denoise_params* p, const double* frame, const double* aov, double* out, rt1w_stats* stats);
/* same on device memory of the context's GPU (e.g. torch tensors); d_out may equal d_frame.  Synchronises the context's stream before returning. */
int rt1w_denoise_device(rt1w_context* c, const rt1w_denoise_params* p, const void* d_frame, const void* d_aov, void* d_out, rt1w_stats* stats);
/* One call: rt1w_render_device of the tile into a context buffer, rt1w_render_aov_device of the same tile, spp, sample_offset and
 * global_seed, the filter, one device->host copy into out_rgb[tile_h][tile_w][3].  Bit-identical to composing the three public calls.
 * `d` may be NULL (all defaults); its width / height must be 0 or the tile's.  Takes the flags rt1w_render takes except RT1W_OUT_SUM,
 * RT1W_OUT_FRAME, RT1W_RNG_REFERENCE (the AOV entries have no reference-stream form) and RT1W_PROBE_COHERENT; interleaved strips
 * (strip_rows != 0) and RT1W_PRECISION_F32 are refused too: all RT1W_ERR_INVALID.  stats are the render's, with the AOV and filter kernel
 * times added to kernel_ms; total_ms is the whole call; grid / block are the level kernel's. */
int rt1w_render_denoised(rt1w_context* c, const rt1w_render_params* p, const rt1w_denoise_params* d, double* out_rgb, rt1w_stats* stats);
/* rt1w_render_denoised with the deep feature buffers (rt1w_render_aov_deep_device with max_specular, max_fuzz) in place of the first-hit
 * ones: bit-identical to composing rt1w_render_device, rt1w_render_aov_deep_device and rt1w_denoise_device.  Refuses what
 * rt1w_render_denoised refuses, and max_specular / max_fuzz as rt1w_render_aov_deep does. */
int rt1w_render_denoised_deep(rt1w_context* c, const rt1w_render_params* p, const rt1w_denoise_params* d, uint32_t max_specular, double max_fuzz,
                              double* out_rgb, rt1w_stats* stats);

/* ---- variance-guided denoiser: the filter above with a colour term that follows the frame's own noise ----
 * rt1w_denoise's colour falloff has a fixed width (sigma_colour), so it blurs a converged frame as hard as a noisy one and its error has a
 * floor that more samples do not lower.  Here the width is each pixel's estimated variance (Schied et al. 2017, SVGF; the estimate from
 * sample batches as Rousselle et al. 2012 take theirs from two half buffers): the filter fades out as the frame converges.  Like
 * rt1w_denoise it replaces nothing of the reference, which has sample count alone (src/main.rs:939).
 *
 * Batch variance.  sums double[K][h][w][3]: the raw sums S_0 .. S_(K-1) of K disjoint batches of n samples each, as K renders with
 *   RT1W_OUT_SUM, spp = n and sample_offset = k n return them.  aov double[h][w][8].  flags 0 or RT1W_DENOISE_KEEP_ALBEDO.  Per pixel:
 *     frame = Color::into_sampled (color.rs:14-21, rt1w_resolve) of ((S_0 + S_1) + ...) with spp = K n: NaN of the sum to 0, times 1 / (K n).
 *             This is the sum of the BATCH sums: not bit-equal to rt1w_render of K n samples in general, which adds its chunks in another
 *             association (equal where every batch is one chunk and the render's chunk is n);
 *     A     = the albedo floor of rt1w_denoise's prepare pass (max(albedo, 0.01), 0.01 where not finite; 1 with KEEP_ALBEDO);
 *     l_k   = luminance of (S_k * (1 / n)) / A per channel, (0.2126 r + 0.7152 g) + 0.0722 b;
 *     lbar  = (((0 + l_0) + l_1) + ...) / K;     var = (((0 + (l_0 - lbar)^2) + (l_1 - lbar)^2) + ...) / (K (K - 1)):
 *             the variance of the mean demodulated luminance.  Where that is negative or not finite (a NaN or inf sample) var = 0: no
 *             usable estimate, and the filter's handling of values that are not finite covers the pixel.
 *   K = 2 .. 16, n >= 1, K n <= 2^32 - 1, width / height as rt1w_denoise: RT1W_ERR_INVALID otherwise.  One lane per pixel, bit-identical
 *   to the CPU build (librt1w_lab.so: rt1w_lab_batch_variance_host).
 * Filter.  rt1w_denoise with a variance buffer var double[h][w] and `sigma_variance` (0 = the default 3; negative or not finite:
 *   RT1W_ERR_INVALID); p->sigma_colour is ignored.  The prepare pass takes v_p = var, 0 where var is negative or not finite.  Every
 *   definition of rt1w_denoise holds but for these:
 *     x_colour   = 0 where l_p == l_q; else (l_p - l_q)^2 / (sigma_variance^2 * (v_p + v_q)) of the current level's values.  A zero
 *                  denominator gives +inf, so weight 0: a converged pixel (v = 0 all around) keeps its value.  The term applies on EVERY
 *                  level, level 0 included, and sigma_variance is not halved: the variance itself shrinks from level to level.  A
 *                  firefly has a large variance of its own and so accepts its neighbours, which replaces the level-0 exemption;
 *     variance   v'_p = sum_q w(p, q)^2 v_q / (sum_q w(p, q))^2 over the taps that the colour takes, in the same order;
 *   the variance is not prefiltered in space.  Bit-identical to the CPU build (librt1w_lab.so: rt1w_lab_denoise_var_host).
 * Buffers of the host forms: two colour buffers of 40 B per pixel, the guide buffer of 64 B per pixel and a buffer for the batch sums,
 * owned by the context, grown on demand, freed with it.  stats as rt1w_denoise. */
int rt1w_batch_variance(rt1w_context* c, uint32_t width, uint32_t height, uint32_t batches, uint32_t batch_spp, uint32_t flags, const double* sums,
                        const double* aov, double* frame, double* var, rt1w_stats* stats);
/* same on device memory of the context's GPU; the four buffers are distinct.  Synchronises the context's stream before returning. */
int rt1w_batch_variance_device(rt1w_context* c, uint32_t width, uint32_t height, uint32_t batches, uint32_t batch_spp, uint32_t flags, const void* d_sums,
                               const void* d_aov, void* d_frame, void* d_var, rt1w_stats* stats);
/* `out` may be `frame` */
int rt1w_denoise_var(rt1w_context* c, const rt1w_denoise_params* p, const double* frame, const double* aov, const double* var, double sigma_variance,
                     double* out, rt1w_stats* stats);
/* same on device memory of the context's GPU; d_out may equal d_frame.  Synchronises the context's stream before returning. */
int rt1w_denoise_var_device(rt1w_context* c, const rt1w_denoise_params* p, const void* d_frame, const void* d_aov, const void* d_var,
                            double sigma_variance, void* d_out, rt1w_stats* stats);
/* One call.  K = `batches` (0 = 4; p->spp must be a multiple of K, n = spp / K): K rt1w_render_device calls with RT1W_OUT_SUM, spp = n,
 * sample_offset = p->sample_offset + k n and p->chunk (0: every batch gets the default of a render of n samples,
 * rt1w_scene_default_chunk(scene, tile_w, tile_h, n)) into the context's batch buffer; rt1w_render_aov_deep_device over all K n samples
 * (max_specular = 0: the first-hit buffers); rt1w_batch_variance_device; rt1w_denoise_var_device; one device->host copy into
 * out_rgb[tile_h][tile_w][3].  Bit-identical to composing those public calls.  The frame that is filtered is the batch sum defined above,
 * NOT in general the bits of rt1w_render at K n samples.  Refuses what rt1w_render_denoised_deep refuses, a K outside 2 .. 16 or that does
 * not divide spp, and sigma_variance as rt1w_denoise_var does.  stats: the renders' sums (paths, segments, passes), all kernel times added
 * in kernel_ms; total_ms the whole call; grid / block the level kernel's; chunk / n_chunks of one batch. */
int rt1w_render_denoised_var(rt1w_context* c, const rt1w_render_params* p, const rt1w_denoise_params* d, uint32_t batches, double sigma_variance,
                             uint32_t max_specular, double max_fuzz, double* out_rgb, rt1w_stats* stats);

/* ---- adaptive sampling: a sample budget spent where the frame is noisy ----
 * The consumer of the batch variance that the entries above lack: instead of giving every pixel the same count, render a short pilot,
 * estimate the error of every tile from the spread of its sample batches, and give further batches to the tiles that need them, until a
 * budget is spent.  Replaces nothing of the reference, which reaches a clean image by sample count alone (src/main.rs:939).  No render
 * kernel is involved beyond being called: a batch of a rectangle is rt1w_render_device with RT1W_OUT_SUM, whose bits depend on (pixel,
 * sample index, chunk) only, not on the rectangle.
 * KNOWN PROPERTY: a pixel's sample count depends on its earlier samples, so the estimator is slightly biased (a pixel that looks converged
 * by chance stops early).  This is adaptive sampling's known bias; the pilot, which every pixel gets whatever it shows, bounds it.
 *
 * Accumulator.  acc double[h][w][8], caller-owned, 64 B per pixel; all zero = empty.  Per pixel:
 *     0-2 S        the sum of the batch sums, added in merge order (the first batch is taken as it is);
 *     3   m        the number of batches merged.  Every merge into one accumulator uses the same batch_spp = n: the count is m n;
 *     4,5 mean_d, M2_d   Welford's mean and sum of squared deviations of the DEMODULATED batch luminance l_k, exactly
 *                  rt1w_batch_variance's l_k: luminance of (S_k * (1 / n)) / A, A the albedo floor (1 with RT1W_DENOISE_KEEP_ALBEDO);
 *     6,7 mean_p, M2_p   the same of the PLAIN luminance, of S_k * (1 / n).
 *   Welford, in this order, without FMA contraction:  m += 1;  d = l - mean;  mean = mean + d / m;  M2 = M2 + d * (l - mean).
 *   A batch whose demodulated or plain luminance is not finite is still added to S and m, but updates neither pair and writes
 *   RT1W_ACCUM_NO_ESTIMATE into M2_d and M2_p; a pixel so marked stays marked (later batches add to S and m only).  A Welford M2 is
 *   never negative, so the marker cannot be met otherwise.
 * rt1w_accum_merge: one rendered batch of the rectangle (x0, y0, tile_w, tile_h) of a width x height frame into acc.
 *   tile_sums double[tile_h][tile_w][3] as rt1w_render with RT1W_OUT_SUM and spp = batch_spp returns it; aov double[height][width][8] of
 *   the WHOLE frame; flags 0 or RT1W_DENOISE_KEEP_ALBEDO.  One lane per pixel of the rectangle, 8 x 8 per wave, 16 x 16 per workgroup:
 *   stats grid = ceil(tile_w / 16) * ceil(tile_h / 16), block 256.  A rectangle outside the frame, batch_spp 0: RT1W_ERR_INVALID.
 * rt1w_accum_resolve: acc -> frame double[h][w][3], var double[h][w], spp double[h][w].
 *     frame = rt1w_resolve's rule on S with the pixel's own count: NaN of S to 0, times 1 / (m n); (0, 0, 0) for an empty pixel;
 *     var   = M2_d / (m (m - 1)), the variance of the mean demodulated luminance that rt1w_denoise_var takes; 0 where m < 2, where the
 *             value is negative or not finite, and where the pixel has no estimate;
 *     spp   = m n as a double.
 *   grid = ceil(w / 16) * ceil(h / 16), block 256.
 * rt1w_accum_tile_error: acc -> err double[ceil(h / tile)][ceil(w / tile)]; tile a multiple of 16 in 16 .. 256.
 *     e_p   = (M2_p / (m (m - 1))) / (max(mean_p, 0) + 0.01): the estimated variance of the pixel's mean over its brightness, which is
 *             the squared error of the DISPLAYED value sqrt(c) (color.rs:56-65) up to a factor 4 -- d sqrt(c) = dc / (2 sqrt(c)); the
 *             0.01 keeps dark pixels from dividing by 0.  0 where m < 2, where the pixel has no estimate or the value is not finite;
 *     err   = (sum of the tile's e_p) / (pixels of the tile inside the frame), summed in this order: within each 16 x 16 block of the
 *             tile, 256 values at the pixels' row-major index in the block (0 for a pixel outside the frame), added by the binary tree
 *             v[i] += v[i + stride] for i < stride, stride = 128, 64 .. 1; then the blocks of the tile that hold a pixel of the frame in
 *             row-major order, 0 + b_0 + b_1 ..., by one lane.  No atomics.
 *   grid = the number of tiles (one workgroup each), block 256.
 * All three are bit-identical to the CPU build (librt1w_lab.so: rt1w_lab_accum_merge_host, rt1w_lab_accum_resolve_host,
 * rt1w_lab_tile_error_host).  The host forms go through context buffers (grown on demand, freed with the context); stats as
 * rt1w_batch_variance (paths = pixels touched, passes 1, kernel_ms, total_ms). */
#define RT1W_ACCUM_NO_ESTIMATE (-1.0)
int rt1w_accum_merge(rt1w_context* c, uint32_t width, uint32_t height, uint32_t x0, uint32_t y0, uint32_t tile_w, uint32_t tile_h, uint32_t batch_spp,
                     uint32_t flags, const double* tile_sums, const double* aov, double* acc, rt1w_stats* stats);
/* same on device memory of the context's GPU; the three buffers are distinct.  Synchronises the context's stream before returning. */
int rt1w_accum_merge_device(rt1w_context* c, uint32_t width, uint32_t height, uint32_t x0, uint32_t y0, uint32_t tile_w, uint32_t tile_h,
                            uint32_t batch_spp, uint32_t flags, const void* d_tile_sums, const void* d_aov, void* d_acc, rt1w_stats* stats);
int rt1w_accum_resolve(rt1w_context* c, uint32_t width, uint32_t height, uint32_t batch_spp, const double* acc, double* frame, double* var,
                       double* spp, rt1w_stats* stats);
int rt1w_accum_resolve_device(rt1w_context* c, uint32_t width, uint32_t height, uint32_t batch_spp, const void* d_acc, void* d_frame, void* d_var,
                              void* d_spp, rt1w_stats* stats);
int rt1w_accum_tile_error(rt1w_context* c, uint32_t width, uint32_t height, uint32_t tile, const double* acc, double* err, rt1w_stats* stats);
int rt1w_accum_tile_error_device(rt1w_context* c, uint32_t width, uint32_t height, uint32_t tile, const void* d_acc, void* d_err, rt1w_stats* stats);

/* rt1w_accum_merge for a LIST of square tiles in one launch (the tiles of rt1w_render_tiles: `tile` a multiple of 16 in 16 .. 256, x0 and y0
 * multiples of it inside the frame, reserved 0, n_tiles 1 .. 2^20; sample_offset is ignored here).  tile_sums double[n_tiles][tile][tile][3]
 * as rt1w_render_tiles writes them with RT1W_OUT_SUM; a pixel of a tile beyond the frame's edge is skipped.  The tiles of one call are
 * disjoint -- a tile named twice is RT1W_ERR_INVALID (two lanes would update one record) -- so the result is bit-identical to n_tiles calls
 * of rt1w_accum_merge on the clipped rectangles, in any order.  One lane per pixel, 16 x 16 pixels per workgroup, grid = n_tiles x
 * (tile / 16)^2; the list is HOST memory in both forms.  CPU twin: rt1w_lab_accum_merge_tiles_host (librt1w_lab.so). */
int rt1w_accum_merge_tiles(rt1w_context* c, uint32_t width, uint32_t height, uint32_t tile, const rt1w_tile* tiles, uint32_t n_tiles, uint32_t batch_spp,
                           uint32_t flags, const double* tile_sums, const double* aov, double* acc, rt1w_stats* stats);
int rt1w_accum_merge_tiles_device(rt1w_context* c, uint32_t width, uint32_t height, uint32_t tile, const rt1w_tile* tiles, uint32_t n_tiles,
                                  uint32_t batch_spp, uint32_t flags, const void* d_tile_sums, const void* d_aov, void* d_acc, rt1w_stats* stats);

/* The plan.  Zero means the default for every member but `size`, which is sizeof(rt1w_adaptive_params) as the caller compiled it (anything
 * else: RT1W_ERR_INVALID; the struct is not one of rt1w_abi_sizeof's).
 *   Pilot.   pilot_batches batches of batch_spp samples on the whole frame.
 *   Rounds.  While budget remains: (1) rt1w_accum_tile_error; (2) the candidates are the tiles with err > target_error and
 *            (m + 1) * batch_spp <= max_spp; (3) ordered by err descending, ties by tile index (row-major) ascending; (4) taken in that
 *            order WHILE both hold -- the pixels taken this round stay <= round_share * width * height (the first candidate is taken
 *            whatever its size), and the pixel-samples spent in all, the candidate's included, stay <= budget_spp * width * height: the
 *            first candidate that breaks either ends the round; (5) a round that takes nothing ends the loop.
 *   Batch.   Every taken tile gets one more batch: rt1w_render_device of its rectangle with RT1W_OUT_SUM, spp = batch_spp,
 *            sample_offset = p->sample_offset + m * batch_spp, and chunk = p->chunk or, if that is 0,
 *            rt1w_scene_default_chunk(scene, width, height, batch_spp) of the WHOLE frame, passed explicitly: with that the bits do not
 *            depend on how tiles are grouped into launches.
 *   Launches. Taken tiles that are adjacent in one tile row and have equal m are rendered as one rectangle and merged by one
 *            rt1w_accum_merge (bits-neutral by the above).
 *   One launch per round.  With RT1W_ADAPTIVE_ONE_LAUNCH in `flags` every ROUND is instead one rt1w_render_tiles_device of all its taken
 *            tiles (each with sample_offset = m * batch_spp, RT1W_OUT_SUM, the same spp and chunk) and one rt1w_accum_merge_tiles_device;
 *            the pilot stays whole-frame.  Frame, spp map, paths, segments and n_chunks are the bits of the call without the flag;
 *            passes falls to the pilot's launches + one per round (times its sample passes).  p->flags must then be 0, RT1W_GENERIC
 *            or RT1W_TILES_SPECIALISED: the flags go to the renders as they are, the pilot's rectangle renders ignore the last and the
 *            rounds' tile lists run the tile-list form of the scene-specialised kernel with it (the generic kernels without: the same
 *            bits).  rt1w_adaptive_select accepts the flag and ignores it. */
#define RT1W_ADAPTIVE_ONE_LAUNCH 0x100u
typedef struct rt1w_adaptive_params {
    uint32_t size;           /* sizeof(rt1w_adaptive_params) */
    uint32_t tile;           /* side of the square tiles, a multiple of 16 in 16 .. 256; 0 = 16 */
    uint32_t batch_spp;      /* samples per batch n; 0 = max(1, budget_spp / 8): the default pilot is half of the budget */
    uint32_t pilot_batches;  /* 2 .. 16; 0 = 4 */
    uint32_t budget_spp;     /* mean samples per pixel to spend, at least the pilot's pilot_batches * batch_spp; 0 = 64 */
    uint32_t max_spp;        /* most samples of one pixel, at least the pilot's; 0 = 8 * budget_spp */
    double target_error;     /* tiles at or below it get no more samples; finite, >= 0; 0 (default): the budget alone decides */
    double round_share;      /* share of the frame's pixels one round may take, in (0, 1]; 0 = 1/4 */
    uint32_t flags;          /* RT1W_DENOISE_KEEP_ALBEDO: how the merges demodulate; RT1W_ADAPTIVE_ONE_LAUNCH: one render launch per round */
} rt1w_adaptive_params;
/* One round of the plan, on the host, without a GPU or a context: err and m_per_tile are [n_tiles_y][n_tiles_x] of a width x height frame
 * (n_tiles_x = ceil(width / tile), likewise y: RT1W_ERR_INVALID otherwise); the pixel-samples spent so far are those m_per_tile says.
 * Returns the number of tiles taken (0 ends the loop) and writes their row-major indices, in the order taken, to out_tiles -- as many as
 * `capacity` holds (out_tiles may be NULL with capacity 0, to ask for the number). */
int rt1w_adaptive_select(const rt1w_adaptive_params* params, uint32_t n_tiles_x, uint32_t n_tiles_y, uint32_t width, uint32_t height, const double* err,
                         const uint32_t* m_per_tile, uint32_t* out_tiles, uint32_t capacity);
/* One call.  p is the frame: its tile must be the whole image (x0 = y0 = 0, tile_w = width, tile_h = height), p->spp is ignored (the budget
 * decides).  In this order: rt1w_render_aov_device over the PILOT's samples only (spp = pilot_batches * batch_spp at p->sample_offset) --
 * these feature buffers demodulate every merge and guide the filter, a stated limit: the guides have the pilot's sample count; the pilot
 * and the rounds as above, every batch merged by rt1w_accum_merge_device, one device->host copy of err per round; rt1w_accum_resolve_device;
 * if `d` is not NULL rt1w_denoise_var_device with `d` and sigma_variance (d's width / height must be 0 or the frame's; with d NULL
 * sigma_variance is still validated); one device->host copy into out_rgb[height][width][3] and, if not NULL, out_spp[height][width] (the
 * per-pixel sample counts as doubles).  Bit-identical to composing these public entries.  Refuses what rt1w_render_denoised_var refuses
 * (RT1W_OUT_SUM, RT1W_OUT_FRAME, RT1W_RNG_REFERENCE, RT1W_PROBE_COHERENT, interleaved strips, RT1W_PRECISION_F32), a tile that is not the
 * frame, the plan's refusals above and a p->sample_offset + max_spp beyond 2^32 - 1: all RT1W_ERR_INVALID.
 * stats: the renders' sums -- paths = the samples actually spent (= the sum of the spp map), segments, passes; kernel_ms every kernel of
 * the call; total_ms the whole call; chunk the batches' chunk; n_chunks = the number of ROUNDS after the pilot (not a chunk count here);
 * grid / block of the last kernel (the filter's level kernel, or the resolve kernel).  Buffers are the context's, grown on demand. */
int rt1w_render_adaptive(rt1w_context* c, const rt1w_render_params* p, const rt1w_adaptive_params* a, const rt1w_denoise_params* d /* NULL: no filter */,
                         double sigma_variance, double* out_rgb, double* out_spp /* may be NULL */, rt1w_stats* stats);

/* ---- adaptive sampling steered by the error that remains AFTER the filter ----
 * rt1w_render_adaptive chooses its tiles by the variance of the unfiltered pixel mean and then, if asked, filters: the filter removes the
 * very noise the plan spent its samples on.  Here the plan is steered by an estimate of the filtered frame's own error, the half-buffer
 * one (Rousselle et al. 2012): the samples of every pixel are kept in two independent halves A and B, both halves go through the weights
 * the filter computes for the whole frame, and the squared difference of the two filtered halves measures the noise that is still there.
 * The estimate is empirical -- it does not rest on the independence assumptions of the variance v' the levels hand on -- and it is a
 * per-pixel error map of the denoised frame, so target_error means "stop when the picture that will be looked at is this good".
 * No render kernel is involved beyond being called, and no entry above changes.
 *
 * Halves.  Two accumulators acc_a, acc_b, each double[h][w][8] exactly as rt1w_accum_merge keeps it, merged with the same batch_spp = n.
 *   Batch number b of a pixel (0-based: its samples b n .. b n + n - 1) goes into A when b is even and into B when b is odd.
 * rt1w_halves_resolve: (acc_a, acc_b) -> frame double[h][w][3], var double[h][w], half_a, half_b double[h][w][3], spp double[h][w].
 *   Per pixel, with m = m_A + m_B:
 *     frame  = rt1w_resolve's rule on S_A + S_B (per channel, that one addition) with count m n; (0, 0, 0) for an empty pixel;
 *     half_x = the same rule on S_x with count m_x n; (0, 0, 0) where m_x = 0;
 *     spp    = m n as a double;
 *     var    = the variance of the mean demodulated luminance over all m batches, from the two Welford states combined in this order:
 *              delta = mean_dB - mean_dA;  M2 = (M2_dA + M2_dB) + ((delta * delta) * (double)(m_A * m_B)) / m;  var = M2 / (m (m - 1));
 *              0 where m < 2, where either half carries RT1W_ACCUM_NO_ESTIMATE, and where the value is negative or not finite.
 *   var is NOT bit-equal to rt1w_accum_resolve of one accumulator that received the same batches (another order of the same sums); the
 *   two agree to 1e-12 relative where the batches' rms deviation is above 0.05 of their mean.  m_A != m_B is handled as defined.
 *   grid = ceil(w / 16) * ceil(h / 16), block 256; batch_spp 0: RT1W_ERR_INVALID.
 * rt1w_denoise_var_halves: rt1w_denoise_var, definition for definition, on frame, aov and var -- `out` is BIT-IDENTICAL to
 *   rt1w_denoise_var of the same three buffers -- and in addition:
 *     prepare   a_p = half_a / A_p and b_p = half_b / A_p per channel, with the A_p the frame is demodulated with;
 *     levels    a'_p = sum_q w(p, q) a_q / sum_q w(p, q) over exactly the taps the colour takes (w > 0), in the colour's order, with the
 *               weight the level computed for the frame; b likewise.  The halves never enter a weight.  A centre pixel whose luminance
 *               is not finite passes all three values through unchanged;
 *     finish    d = lum(a' * A_p) - lum(b' * A_p), lum = (0.2126 r + 0.7152 g) + 0.0722 b;
 *               err_px = ((d * d) * 0.25) / (max(lum(out_p), 0) + 0.01), 0 where that is not finite.  1/4: Var((A + B) / 2) =
 *               Var(A - B) / 4 for two independent halves of equal count.  The denominator is rt1w_accum_tile_error's: err_px is in the
 *               units of that entry's e_p.  One squared difference is a one-degree-of-freedom estimate: read it through a tile mean.
 *   out double[h][w][3] (may be `frame`), err_px double[h][w]; the other buffers are distinct.  The colour record of a level is 88 B per
 *   pixel (two context buffers, grown on demand), the guide record 64 B.  stats as rt1w_denoise_var.
 * rt1w_tile_error_map: err_px double[h][w] -> err double[ceil(h / tile)][ceil(w / tile)], the tile mean of a per-pixel map in the
 *   summation order of rt1w_accum_tile_error (the block tree over the row-major index, then the tile's blocks in row-major order by one
 *   lane; one workgroup per tile, no atomics).  A value that is negative or not finite counts as 0.  tile as there.
 * All three are bit-identical to the CPU build (librt1w_lab.so: rt1w_lab_halves_resolve_host, rt1w_lab_denoise_var_halves_host,
 * rt1w_lab_tile_error_map_host). */
int rt1w_halves_resolve(rt1w_context* c, uint32_t width, uint32_t height, uint32_t batch_spp, const double* acc_a, const double* acc_b, double* frame,
                        double* var, double* half_a, double* half_b, double* spp, rt1w_stats* stats);
/* same on device memory of the context's GPU; the seven buffers are distinct.  Synchronises the context's stream before returning. */
int rt1w_halves_resolve_device(rt1w_context* c, uint32_t width, uint32_t height, uint32_t batch_spp, const void* d_acc_a, const void* d_acc_b, void* d_frame,
                               void* d_var, void* d_half_a, void* d_half_b, void* d_spp, rt1w_stats* stats);
int rt1w_denoise_var_halves(rt1w_context* c, const rt1w_denoise_params* p, const double* frame, const double* aov, const double* var, const double* half_a,
                            const double* half_b, double sigma_variance, double* out, double* err_px, rt1w_stats* stats);
/* same on device memory of the context's GPU; d_out may equal d_frame, the other buffers are distinct */
int rt1w_denoise_var_halves_device(rt1w_context* c, const rt1w_denoise_params* p, const void* d_frame, const void* d_aov, const void* d_var,
                                   const void* d_half_a, const void* d_half_b, double sigma_variance, void* d_out, void* d_err_px, rt1w_stats* stats);
int rt1w_tile_error_map(rt1w_context* c, uint32_t width, uint32_t height, uint32_t tile, const double* err_px, double* err, rt1w_stats* stats);
int rt1w_tile_error_map_device(rt1w_context* c, uint32_t width, uint32_t height, uint32_t tile, const void* d_err_px, void* d_err, rt1w_stats* stats);
/* One call.  The unit of the plan is a PAIR of batches, one for each half: pilot_batches must be even (RT1W_ERR_INVALID otherwise) and the
 * pilot is pilot_batches / 2 pairs.  One round's choice is rt1w_adaptive_select, unchanged, with batch_spp = 2 n, pilot_batches =
 * max(2, pilot_batches / 2) and m = the tile's PAIR count, so its budget, max_spp, round_share and ordering rules hold as written (and
 * what it refuses of those parameters is refused here).  RT1W_ADAPTIVE_ONE_LAUNCH is accepted and changes nothing: every round is one launch.
 * In this order:
 *   1. rt1w_render_aov_device over the PILOT's samples only (spp = pilot_batches * n at p->sample_offset): as in rt1w_render_adaptive these
 *      feature buffers demodulate every merge and guide the filter -- the same stated limit: the guides have the pilot's sample count;
 *   2. the pilot: pilot_batches whole-frame rt1w_render_device with RT1W_OUT_SUM, spp = n, sample_offset = p->sample_offset + b n, each
 *      merged by rt1w_accum_merge_device into A (b even) or B (b odd);
 *   3. rounds, each of: rt1w_halves_resolve_device; rt1w_denoise_var_halves_device with `d` (NULL: every default) and sigma_variance,
 *      in place on the resolved frame; rt1w_tile_error_map_device; one device->host copy of err; the select; ONE rt1w_render_tiles_device
 *      whose list names every taken tile twice -- first all taken tiles, in the order taken, with sample_offset = p->sample_offset +
 *      2 j n, then all of them again with + (2 j + 1) n, j the tile's pair count -- with RT1W_OUT_SUM, spp = n; two
 *      rt1w_accum_merge_tiles_device, the first half of the list and of the sums into A, the second into B.  chunk = p->chunk or, if that
 *      is 0, rt1w_scene_default_chunk(scene, width, height, n) of the WHOLE frame, passed explicitly;
 *   4. the round that takes nothing ends the loop: ITS filtered frame and error map are the result -- no further filter pass is made;
 *   5. one device->host copy each into out_rgb[height][width][3] and, if not NULL, out_spp[height][width] and out_err[height][width].
 * Every pixel's count is a multiple of 2 n and m_A == m_B at every estimate.  Bit-identical to composing these public entries.
 * Because the rounds go through the tile entries, p->flags must be 0, RT1W_GENERIC or RT1W_TILES_SPECIALISED (the rounds on the tile-list
 * form of the scene-specialised kernel: the same bits); everything rt1w_render_adaptive refuses is refused
 * here too: all RT1W_ERR_INVALID.  stats as there: the renders' sums (paths = the samples spent, segments, passes = the pilot's launches +
 * one per round, times its sample passes); kernel_ms every kernel of the call, every filter pass included; total_ms the whole call;
 * n_chunks = the number of ROUNDS; grid / block of the filter's level kernel.  Buffers are the context's, grown on demand. */
int rt1w_render_adaptive_filtered(rt1w_context* c, const rt1w_render_params* p, const rt1w_adaptive_params* a, const rt1w_denoise_params* d /* NULL: defaults */,
                                  double sigma_variance, double* out_rgb, double* out_spp /* may be NULL */, double* out_err /* may be NULL */,
                                  rt1w_stats* stats);

/* ---- cross-filtered half buffers: an error map that is not blind to the weights' own error ----
 * rt1w_denoise_var_halves sends both halves through ONE set of weights, computed from the whole noisy frame: whatever error enters through
 * the weights is common to a' and b' and cancels in their difference, so its map orders tiles but understates the filtered frame's
 * seed-to-seed variance.  Here each half is filtered with weights whose colour term comes from the OTHER half
 * (Rousselle et al. 2012): the two filtered halves share no weight, and no weight is computed from the value it multiplies, so a pixel
 * no longer prefers the neighbours that share its own noise.  Like every filter here it replaces nothing of the reference, which has
 * sample count alone (src/main.rs:939).  No entry above changes.
 * rt1w_denoise_cross: the buffers of rt1w_denoise_var_halves.  `frame` gives no value, only its finiteness (below).
 *   Prepare.  A_p, the guides and v_p (var, 0 where negative or not finite) as rt1w_denoise_var.  a_p = half_a / A_p, b_p = half_b / A_p per
 *     channel; la_p, lb_p their luminances (0.2126 r + 0.7152 g) + 0.0722 b; va_p = vb_p = 2 v_p: a half of equal count has twice the
 *     variance of the whole mean (var is the buffer rt1w_halves_resolve writes).  A weight here never sees the value it multiplies, so
 *     what is not finite is kept out at this point: where the luminance of frame / A_p, la_p or lb_p is not finite, the first of these three
 *     that is not stands for BOTH la_p and lb_p -- the pixel is passed through every level and no other pixel takes it, in either half.
 *   Level i.  Step, taps, order, h, w_normal, x_depth, x_coverage and k as rt1w_denoise_var.  Two weights per tap that is not the centre:
 *     wA(p, q), which filters A, has x_colour = 0 where lb_p == lb_q, else (lb_p - lb_q)^2 / (sigma_variance^2 * (vb_p + vb_q));
 *     wB(p, q), which filters B, the same of la, va.  The centre tap has wA = wB = h(0, 0).
 *       a'_p  = sum wA a_q / sum wA over the taps with wA > 0, in tap order;  la'_p = the luminance of a'_p;
 *       va'_p = sum wA^2 va_q / (sum wA)^2 over the same taps;                 b', lb', vb' likewise with wB.
 *     A centre whose la or lb is not finite passes its whole record through unchanged.  Every level has the colour term and
 *     sigma_variance is not halved, as in rt1w_denoise_var.
 *   Finish.  out = ((a' + b') * 0.5) * A_p per channel: the plain mean, which assumes m_A == m_B (rt1w_render_adaptive_cross guarantees it).
 *     d = lum(a' * A_p) - lum(b' * A_p);  err_px = ((d * d) * 0.25) / (max(lum(out_p), 0) + 0.01), 0 where that is not finite: the units of
 *     rt1w_denoise_var_halves's map, so rt1w_tile_error_map and the plan run on it unchanged.
 *   `out` is NOT the bits of rt1w_denoise_var.  With half_a == half_b == frame each half's (a', la') is the bits of rt1w_denoise_var's
 *   (c', l') of that frame with the variance 2 var, and err_px is 0.
 *   out double[h][w][3] (may be `frame`), err_px double[h][w]; the other buffers are distinct.  The colour record of a level is 80 B per
 *   pixel (two context buffers, grown on demand), the guide record 64 B.  Refuses what rt1w_denoise_var_halves refuses; stats as there.
 *   Bit-identical to the CPU build (librt1w_lab.so: rt1w_lab_denoise_cross_host). */
int rt1w_denoise_cross(rt1w_context* c, const rt1w_denoise_params* p, const double* frame, const double* aov, const double* var, const double* half_a,
                       const double* half_b, double sigma_variance, double* out, double* err_px, rt1w_stats* stats);
/* same on device memory of the context's GPU; d_out may equal d_frame, the other buffers are distinct */
int rt1w_denoise_cross_device(rt1w_context* c, const rt1w_denoise_params* p, const void* d_frame, const void* d_aov, const void* d_var,
                              const void* d_half_a, const void* d_half_b, double sigma_variance, void* d_out, void* d_err_px, rt1w_stats* stats);
/* One call: rt1w_render_adaptive_filtered, step for step, with rt1w_denoise_cross_device in place of rt1w_denoise_var_halves_device in
 * step 3.  The same parameters, refusals (under this entry's name), buffers and stats; bit-identical to composing the public entries.
 * An entry of its own rather than a bit of rt1w_adaptive_params.flags. */
int rt1w_render_adaptive_cross(rt1w_context* c, const rt1w_render_params* p, const rt1w_adaptive_params* a, const rt1w_denoise_params* d /* NULL: defaults */,
                               double sigma_variance, double* out_rgb, double* out_spp /* may be NULL */, double* out_err /* may be NULL */,
                               rt1w_stats* stats);

/* ---- full-count guides: first-hit feature SUMS of a list of tiles, and an accumulator of them ----
 * The adaptive entries above render their feature buffers once, over the pilot's samples, and filter with them to the end: where the plan
 * spends its samples -- geometric edges, defocus, motion blur -- a first-hit albedo, normal or depth is itself a noisy mean, and those pixels
 * keep the pilot's guides.  What follows lets a round top up the guides of the tiles it takes in ONE launch, so that at every estimate a
 * pixel's guides hold as many samples as its colour.  Each sample's camera ray is the one rt1w_render_aov traces (src/main.rs:964-971); like
 * every buffer here it replaces nothing of the reference, which has sample count alone (src/main.rs:939, :957-1001).  No entry above changes.
 * rt1w_render_aov_tiles: rt1w_render_aov for a LIST of square tiles, with the list rules of rt1w_render_tiles: `tile` a multiple of 16 in
 *   16 .. 256, x0 and y0 multiples of it inside the p->width x p->height frame, reserved 0, n_tiles 1 .. 2^20; `tiles` is HOST memory in both
 *   forms (uploaded into the context's tile-list buffer).  From p: width, height, spp (the same for every tile), global_seed, flags;
 *   p->sample_offset is added to every tile's own (a sum + spp beyond 2^32 - 1: RT1W_ERR_INVALID); x0, y0, tile_w, tile_h, max_depth, chunk
 *   and partial_mib are ignored.  Flags: 0 or RT1W_FORCE_VARIANT(v) (tests); anything else, interleaved strips or a non-zero `reserved`:
 *   RT1W_ERR_INVALID; RT1W_PRECISION_F32: RT1W_ERR_UNSUPPORTED.  What the parameters and the list alone decide is refused before the
 *   context is looked at.
 *   out: double[n_tiles][tile][tile][8] of RAW SUMS in sample order, tile k's row 0 = image row y0_k:
 *     0-2 the sum of the albedo, 3-5 of the normal, 6 of t * |d| over the samples that hit (+0.0 if none did), 7 the number of samples that hit.
 *   A pixel beyond the frame's right or top edge is never traced and is +0.0 in all eight.
 *   CONTRACT: for every pixel of tile k inside the frame the sums, finished as s / (double)spp in channels 0-5 and 7 and as
 *   s7 > 0 ? s6 / s7 : +inf in channel 6, are bit-identical to rt1w_render_aov_device of the rectangle (x0_k, y0_k, min(tile, width - x0_k),
 *   min(tile, height - y0_k)) with the same spp and seed and the tile's absolute sample offset.  The order of the list and repeats of a
 *   tile with other offsets do not change a bit.
 *   One lane per pixel runs its samples in order, 8 x 8 pixels per wave, 16 x 16 per workgroup, grid = n_tiles x (tile / 16)^2.
 *   stats: paths = segments = pixels inside the frame x spp; passes 1; grid, block, variant, kernel_ms, total_ms.
 * The guide accumulator gacc: double[h][w][9], caller-owned, 72 bytes per pixel, all zero = empty.  Values 0-7 are the sums above, value 8 is
 *   N, the samples merged, exact as a double.
 * rt1w_guides_merge_tiles: tile_sums double[n_tiles][tile][tile][8] as rt1w_render_aov_tiles writes them for `spp` samples, into gacc.  The
 *   list as above, but the tiles of one call are disjoint -- a tile named twice is RT1W_ERR_INVALID, as in rt1w_accum_merge_tiles;
 *   sample_offset is ignored; spp 0 is RT1W_ERR_INVALID.  Per pixel inside the frame: where N == 0 the eight sums are taken as they are and
 *   N = spp; otherwise g_c = g_c + s_c for c = 0 .. 7 and N = N + spp.  One lane per pixel, 16 x 16 pixels per workgroup, grid = n_tiles x
 *   (tile / 16)^2, no atomics.
 * rt1w_guides_resolve: gacc -> aov double[h][w][8] in the layout of rt1w_render_aov.  N == 0 gives (0, 0, 0, 0, 0, 0, +inf, 0); otherwise
 *   channel c of 0-5 and 7 is g_c / N and channel 6 is g7 > 0 ? g6 / g7 : +inf.  grid = ceil(w / 16) * ceil(h / 16), block 256.
 *   After ONE merge of spp samples into an empty accumulator the resolved buffer is the bits of rt1w_render_aov_device.  After several merges
 *   it is NOT (another association of the same sums, as rt1w_halves_resolve's var is not rt1w_accum_resolve's): the hit count and so the
 *   coverage's numerator stay exact; the sums of a + b samples agree within (a + b) * 2^-52, relative for the non-negative ones (albedo,
 *   distance), absolute for the normal's.
 * All three are bit-identical to the CPU build (librt1w_lab.so: rt1w_lab_aov_tiles_host, rt1w_lab_guides_merge_tiles_host,
 * rt1w_lab_guides_resolve_host). */
int rt1w_render_aov_tiles(rt1w_context* c, const rt1w_render_params* p, uint32_t tile, const rt1w_tile* tiles, uint32_t n_tiles, double* out, rt1w_stats* stats);
/* same, into device memory on the context's GPU; the list itself is host memory.  Synchronises the context's stream before returning. */
int rt1w_render_aov_tiles_device(rt1w_context* c, const rt1w_render_params* p, uint32_t tile, const rt1w_tile* tiles, uint32_t n_tiles, void* d_out,
                                 rt1w_stats* stats);
int rt1w_guides_merge_tiles(rt1w_context* c, uint32_t width, uint32_t height, uint32_t tile, const rt1w_tile* tiles, uint32_t n_tiles, uint32_t spp,
                            const double* tile_sums, double* gacc, rt1w_stats* stats);
int rt1w_guides_merge_tiles_device(rt1w_context* c, uint32_t width, uint32_t height, uint32_t tile, const rt1w_tile* tiles, uint32_t n_tiles, uint32_t spp,
                                   const void* d_tile_sums, void* d_gacc, rt1w_stats* stats);
int rt1w_guides_resolve(rt1w_context* c, uint32_t width, uint32_t height, const double* gacc, double* aov, rt1w_stats* stats);
int rt1w_guides_resolve_device(rt1w_context* c, uint32_t width, uint32_t height, const void* d_gacc, void* d_aov, rt1w_stats* stats);
/* One call: rt1w_render_adaptive_filtered, step for step, with the same parameters, refusals (under this entry's name), buffers and stats.
 * It differs only here:
 *   1. in place of rt1w_render_aov_device: rt1w_render_aov_tiles_device of EVERY tile of the frame in row-major order (spp = pilot_batches * n
 *      at p->sample_offset, every tile's own offset 0), rt1w_guides_merge_tiles_device into a zeroed gacc, rt1w_guides_resolve_device into the
 *      pilot feature buffer -- by the contracts above the bits rt1w_render_adaptive_filtered renders.  That buffer stays fixed and
 *      demodulates every rt1w_accum_merge*, exactly as there, so the Welford states keep one albedo;
 *   3. each round, after rt1w_halves_resolve_device: rt1w_guides_resolve_device into a SECOND feature buffer, which the filter and its
 *      error map take as `aov`; after the round's rt1w_render_tiles_device: one rt1w_render_aov_tiles_device over the taken tiles, in the
 *      order taken, once each, with sample_offset = p->sample_offset + 2 j n and spp = 2 n (the pair's samples are contiguous), then one
 *      rt1w_guides_merge_tiles_device.
 * At every estimate each pixel's N equals its entry in the spp map.  A stated limit: `var` is the variance of the luminance demodulated with
 * the PILOT's albedo, while the filter demodulates the frame with the full-count albedo.  stats.passes counts trace-kernel launches only, as
 * there; the AOV and guide kernels add to kernel_ms.  Bit-identical to composing these public entries; with budget_spp equal to the pilot's
 * samples (no round takes a tile) out_rgb, out_spp and out_err are the bits of rt1w_render_adaptive_filtered.  An entry of its own rather
 * than a bit of rt1w_adaptive_params.flags. */
int rt1w_render_adaptive_guided(rt1w_context* c, const rt1w_render_params* p, const rt1w_adaptive_params* a, const rt1w_denoise_params* d /* NULL: defaults */,
                                double sigma_variance, double* out_rgb, double* out_spp /* may be NULL */, double* out_err /* may be NULL */,
                                rt1w_stats* stats);

/* ---- a live context's camera ----
 * The camera is frozen into a scene at rt1w_scene_set_camera; a context copies it at creation and hands it to every kernel by value.
 * rt1w_context_set_camera replaces that copy: the arguments, their meaning and the arithmetic (Camera::new, camera.rs:22-59: one function
 * behind both entries) are rt1w_scene_set_camera's, and so are the refusals (a null vector, time0 >= time1: RT1W_ERR_INVALID).  Every
 * later call on the context -- rt1w_render*, rt1w_render_aov*, the tile lists, f32 mode (its f32 copy is rounded anew), the
 * reference-stream mode -- traces the new camera and gives, bit for bit, what a fresh context of a scene committed with these arguments
 * gives.  Host work only: the scene object is not touched, so other contexts of the scene keep their camera; the kernel choice, the key
 * of the scene-specialised kernel (the camera is no part of the generated source), the walk table (ranked once, by the scene's own
 * camera) and the partial-sum buffers are unaffected.  Not to be called while a call on the context is in flight on another thread. */
typedef struct rt1w_camera {
    double origin[3], lower_left_corner[3], horizontal[3], vertical[3], u[3], v[3], w[3];   /* camera.rs:7-18 */
    double lens_radius, time0, time1;
} rt1w_camera;                          /* 192 bytes */
int rt1w_context_set_camera(rt1w_context* c, const double look_from[3], const double look_at[3], const double vup[3], double vfov_deg,
                            double aspect_ratio, double aperture, double focus_dist, double time0, double time1);
/* the ten quantities the context's kernels are handed now */
int rt1w_context_get_camera(const rt1w_context* c, rt1w_camera* out);

/* ---- temporal accumulation: the previous frame's samples, reprojected ----
 * A frame of an animation is blended with the history of the frames before it, fetched where the surface point seen in a pixel was seen
 * in the previous frame.  Replaces nothing of the reference, which renders stills.
 *   cur_frame double[h][w][3] means, the layout of rt1w_render;  cur_aov, prev_aov double[h][w][8], the layout of rt1w_render_aov
 *   (first-hit buffers: the depth is t |d|, the distance along the camera ray);  cur_cam, prev_cam the cameras the two frames were
 *   rendered with;  prev_hist double[h][w][3] and prev_len double[h][w] the outputs `hist` and `len` of the previous frame's call
 *   (prev_len = 0 everywhere: no history, the first frame);  out: hist[h][w][3], len[h][w], frame_out[h][w][3].  The buffers are whole
 *   images: pixel (x, y) of the buffers is pixel i = x, j = y of both cameras.  The three outputs must not overlap each other or an input:
 *   RT1W_ERR_INVALID.
 * Per pixel p = (x, y):
 *   1. Demodulation.  Albedo A, value c = cur_frame / A and unit normal n_cur exactly as the prepare pass of rt1w_denoise forms them
 *      (A = max(albedo, 0.01) per channel, 1 with RT1W_DENOISE_KEEP_ALBEDO; n_cur = (0, 0, 0) for a degenerate mean normal).  The
 *      history is kept demodulated, so textures are not blurred by the resampling.
 *   2. No reuse on a miss.  If the coverage of p is not > 0 or its depth z is not finite: hist = c, len = 1.
 *   3. Reprojection point.  X = cur_cam.origin + (z / |dir|) dir,  dir = lower_left_corner + s horizontal + t vertical - origin,
 *      s = (x + 1/2) / (w - 1), t = (y + 1/2) / (h - 1): the pixel CENTRE, the mean of the reference's jittered (i + r) / (width - 1),
 *      r in [0, 1) (main.rs:964-971) (a buffer of one column or row, which no render makes, divides by 1).  With lens_radius > 0 this is
 *      the ray from the lens CENTRE -- a stated approximation: the depth is a mean over rays from all over the lens, and what is out of
 *      focus is reprojected as if it were sharp.
 *   4. Projection.  P = X - prev_cam.origin.  If P . w_prev >= 0 (X behind the previous camera, which looks along -w) or the product is
 *      NaN: no history.  Else X goes through prev_cam's pinhole onto its focus plane: q = D + P (D . w_prev) / (-(P . w_prev)),
 *      D = origin - lower_left_corner, s' = q . horizontal / |horizontal|^2, t' = q . vertical / |vertical|^2, and the continuous pixel
 *      position is fx = s' (w - 1) - 1/2, fy = t' (h - 1) - 1/2 (a pixel's centre has integer fx, fy).  Unless -1 < fx < w and
 *      -1 < fy < h no tap lies in the image: no history.
 *   5. Taps.  (ix, iy) = floor(fx, fy), the taps are (ix + dx, iy + dy) in the order (0,0), (1,0), (0,1), (1,1) with the bilinear
 *      weights (dx ? fx - ix : 1 - (fx - ix)) * (dy ? fy - iy : 1 - (fy - iy)).  A tap q is VALID if it lies in the image,
 *      prev_len_q > 0, its previous coverage > 0, |z_q - |P|| <= depth_tol |P| with z_q its previous depth,
 *      n_q . n_cur >= normal_min with n_q the unit normal of its previous mean normal, and prev_len_q, z_q and the three values of
 *      prev_hist_q are finite.
 *   6. History.  h = (sum of weight * prev_hist over the valid taps, in that order) / (sum of their weights), N the same of prev_len.  If
 *      the sum of weights is not > 0: no history.
 *   7. Update.  With history N' = min(N, max_history - 1), hist = (N' h + c) / (N' + 1), len = N' + 1: the running mean of all frames up
 *      to max_history, an exponential average from there on.  With no history hist = c, len = 1.
 *   8. Output.  frame_out = hist * A per channel.
 * Arithmetic: + - * /, sqrt, comparisons and selects in one fixed order, without FMA contraction, each output pixel whole by one lane
 * (an 8 x 8 pixel block per wave, 2 x 2 blocks per workgroup, the cameras by value, no atomics, one launch on the context's stream):
 * bit-identical to the CPU build of the same code (librt1w_lab.so: rt1w_lab_temporal_host).
 * Stated limits.  The scene is taken as static: a MovingSphere's surface fails the depth test or smears.  What is seen through glass
 * or in a mirror is reprojected with the first surface's motion.  Light that depends on the view (a Metal's reflection) lags by up to
 * max_history frames. */
typedef struct rt1w_temporal_params {
    uint32_t width, height;              /* of all buffers: 1 .. 2^30 */
    uint32_t flags;                      /* 0 or RT1W_DENOISE_KEEP_ALBEDO */
    uint32_t max_history;                /* 0 = 32 */
    double depth_tol;                    /* 0 = 0.05; negative or not finite: RT1W_ERR_INVALID */
    double normal_min;                   /* 0 = 0.9; negative, NaN or > 1: RT1W_ERR_INVALID */
} rt1w_temporal_params;                 /* 32 bytes; not one of rt1w_abi_sizeof's: bindings assert the 32 themselves */
/* host buffers, through the context's device buffers.  stats: kernel_ms = HIP-event time of the launch, total_ms the whole call, passes 1,
 * grid / block of the kernel, paths = pixels. */
int rt1w_temporal_accumulate(rt1w_context* c, const rt1w_temporal_params* p, const double* cur_frame, const double* cur_aov, const rt1w_camera* cur_cam,
                             const double* prev_hist, const double* prev_len, const double* prev_aov, const rt1w_camera* prev_cam, double* hist,
                             double* len, double* frame_out, rt1w_stats* stats);
/* same on device memory of the context's GPU (e.g. torch tensors); the cameras are host memory.  Synchronises the context's stream before returning. */
int rt1w_temporal_accumulate_device(rt1w_context* c, const rt1w_temporal_params* p, const void* d_cur_frame, const void* d_cur_aov,
                                    const rt1w_camera* cur_cam, const void* d_prev_hist, const void* d_prev_len, const void* d_prev_aov,
                                    const rt1w_camera* prev_cam, void* d_hist, void* d_len, void* d_frame_out, rt1w_stats* stats);
/* One frame of an animation in one call: rt1w_render_device of the tile, rt1w_render_aov_device of the same tile, spp, sample_offset and
 * global_seed, rt1w_temporal_accumulate_device against the state the context keeps from the previous call (prev_hist, prev_len, prev_aov
 * and the camera of that call: two sets of device buffers that swap, grown on demand and freed with the context) with the context's
 * camera at the time of the call as cur_cam, then, if `d` is given, rt1w_denoise_device of frame_out with the current feature buffers,
 * one device->host copy into out_rgb[height][width][3].  On the first call, after rt1w_temporal_reset and after a change of width or
 * height prev_len is 0 everywhere (and prev_cam is cur_cam).  Bit-identical to composing these public entries.  `t` may be NULL (all
 * defaults), its width / height must be 0 or the image's; `d` NULL: no filter.  Refuses what rt1w_render_denoised refuses, and a tile
 * that is not the whole image (the reprojection works in image coordinates): RT1W_ERR_INVALID.  stats are the render's, with the AOV,
 * accumulation and filter kernel times added to kernel_ms; total_ms is the whole call; grid / block are the last kernel's.  The state is
 * read and written by this entry alone: no other entry's result depends on it. */
int rt1w_render_temporal(rt1w_context* c, const rt1w_render_params* p, const rt1w_temporal_params* t /* NULL: defaults */,
                         const rt1w_denoise_params* d /* NULL: no filter */, double* out_rgb, rt1w_stats* stats);
/* forget the history: the next rt1w_render_temporal -- and the next rt1w_render_temporal_var, whose state is its own -- is a first frame.
 * The buffers stay allocated. */
int rt1w_temporal_reset(rt1w_context* c);

/* ---- temporal second moments: a variance for the filter from the history ----
 * An animation carries a variance estimate for free: the spread of a pixel's values from frame to frame is the variance of its
 * accumulated mean (Schied et al. 2017, SVGF).  One more history channel, the running mean of the squared demodulated luminance, and one
 * small pass turn the history into the `var` buffer rt1w_denoise_var takes -- one render launch per frame instead of rt1w_batch_variance's
 * K.  Replaces nothing of the reference, which renders stills.  No entry above changes; the parameters are rt1w_temporal_params and
 * rt1w_denoise_params.
 * rt1w_temporal_moments: the arguments of rt1w_temporal_accumulate, with prev_m2 double[h][w] after prev_hist (the output `m2` of the
 *   previous frame's call) and the output m2 double[h][w] after hist.  Steps 1-8 are rt1w_temporal_accumulate's, word for word: hist, len
 *   and frame_out are ITS BITS on the same inputs.  In addition, with l = the luminance (0.2126 r + 0.7152 g) + 0.0722 b of the
 *   demodulated current value c of step 1:
 *     no history:    m2 = l * l;
 *     with history:  m2 = (N' * (sum of weight * prev_m2 over the valid taps of step 5, in that order, / the sum of their weights) + l * l)
 *                         / (N' + 1), with the N' of step 7.
 *   prev_m2 is no part of a tap's validity (the tap set stays the accumulate entry's) and an invalid tap's prev_m2 is never read into a
 *   product: with prev_len = 0 everywhere prev_m2 may hold anything.  A valid tap whose prev_m2 is not finite gives an m2 that is not
 *   finite, which rt1w_temporal_variance answers with "no estimate".  The four outputs must not overlap each other or an input:
 *   RT1W_ERR_INVALID.  Refusals, stats and work mapping as rt1w_temporal_accumulate; 256 bytes per pixel against its 240.
 * rt1w_temporal_variance: hist double[h][w][3], m2 and len double[h][w] as rt1w_temporal_moments wrote them, aov double[h][w][8] the
 *   CURRENT frame's feature buffers -> var double[h][w], the buffer rt1w_denoise_var takes: the variance of the mean demodulated
 *   luminance.  Per pixel p, with l1 = lum(hist_p) -- the luminance is linear, so this is the running mean of l up to rounding, and no
 *   first-moment channel is kept:
 *     Temporal estimate, where len_p >= RT1W_TEMPORAL_MIN_LEN (4: a constant as in SVGF, not a parameter):
 *       var = max(m2_p - l1 * l1, 0) / (len_p - 1).
 *     Spatial estimate, where len_p < 4.  The taps are q = p + (dx, dy), dx, dy = -3 .. 3, inside the image, in row order (dy outer).  The
 *       guides are the prepare pass's of rt1w_denoise: unit normal, depth, coverage.  The centre tap has weight 1; every other tap has the
 *       guide-only weight of the variance filter, w_normal * k(x_depth + x_coverage) with rt1w_denoise's defaults (normal power 32,
 *       sigma_depth 0.1).  A tap is taken if w > 0 and lum(hist_q) and m2_q are finite.  S0 = sum w, S1 = sum w * lum(hist_q),
 *       S2 = sum w * m2_q;  M1 = S1 / S0, M2 = S2 / S0;  var = max(M2 - M1 * M1, 0) / len_p.
 *     var = 0 ("no usable estimate", rt1w_batch_variance's rule) where l1, m2_p or len_p is not finite, where len_p < 1, and where the
 *       result is negative or not finite.
 *   var must not overlap an input, width and height are 1 .. 2^30: RT1W_ERR_INVALID.  One lane per pixel in the work mapping of
 *   rt1w_temporal_accumulate, no atomics, no LDS: a lane of a short history walks the 49 taps through global memory, every other lane
 *   reads its own 104 bytes.  stats as rt1w_temporal_accumulate.
 *   A stated limit: the first frame of an animation has no history, so its variance is the spatial estimate alone, which takes the
 *   frame's own texture under the window for noise (DESIGN.md section 21 has the measurement).
 * Both are bit-identical to the CPU build of the same code (librt1w_lab.so: rt1w_lab_temporal_moments_host,
 * rt1w_lab_temporal_variance_host). */
#define RT1W_TEMPORAL_MIN_LEN 4
int rt1w_temporal_moments(rt1w_context* c, const rt1w_temporal_params* p, const double* cur_frame, const double* cur_aov, const rt1w_camera* cur_cam,
                          const double* prev_hist, const double* prev_m2, const double* prev_len, const double* prev_aov, const rt1w_camera* prev_cam,
                          double* hist, double* m2, double* len, double* frame_out, rt1w_stats* stats);
/* same on device memory of the context's GPU; the cameras are host memory.  Synchronises the context's stream before returning. */
int rt1w_temporal_moments_device(rt1w_context* c, const rt1w_temporal_params* p, const void* d_cur_frame, const void* d_cur_aov, const rt1w_camera* cur_cam,
                                 const void* d_prev_hist, const void* d_prev_m2, const void* d_prev_len, const void* d_prev_aov,
                                 const rt1w_camera* prev_cam, void* d_hist, void* d_m2, void* d_len, void* d_frame_out, rt1w_stats* stats);
int rt1w_temporal_variance(rt1w_context* c, uint32_t width, uint32_t height, const double* hist, const double* m2, const double* len, const double* aov,
                           double* var, rt1w_stats* stats);
int rt1w_temporal_variance_device(rt1w_context* c, uint32_t width, uint32_t height, const void* d_hist, const void* d_m2, const void* d_len,
                                  const void* d_aov, void* d_var, rt1w_stats* stats);
/* One frame of an animation, filtered with the history's own variance, in one call.  In this order: rt1w_render_device of the whole image,
 * rt1w_render_aov_device of the same spp, sample_offset and global_seed, rt1w_temporal_moments_device against a state of this entry's
 * own (two swapping sets of hist, m2, len and feature buffers, grown on demand and freed with the context; zeroed on the first call,
 * after rt1w_temporal_reset and after a change of size -- never rt1w_render_temporal's state, so the two entries may be interleaved),
 * rt1w_temporal_variance_device of the new history with the current feature buffers, rt1w_denoise_var_device of frame_out with the
 * current feature buffers, that var, `d` (NULL: every default) and sigma_variance, one device->host copy into
 * out_rgb[height][width][3].  Bit-identical to composing these public entries.  The filter is always on: without it the call would be
 * rt1w_render_temporal.  Refuses what rt1w_render_temporal refuses, sigma_variance as rt1w_denoise_var does, and a `t` and a `d` that
 * disagree on RT1W_DENOISE_KEEP_ALBEDO (var is in the units of t's demodulation): RT1W_ERR_INVALID; sigma_variance and that disagreement
 * are decided before the context is looked at.  stats as rt1w_render_temporal, every kernel of the call in kernel_ms, grid / block of the
 * filter's level kernel. */
int rt1w_render_temporal_var(rt1w_context* c, const rt1w_render_params* p, const rt1w_temporal_params* t /* NULL: defaults */,
                             const rt1w_denoise_params* d /* NULL: defaults */, double sigma_variance, double* out_rgb, rt1w_stats* stats);

/* Page-locked host memory for output frames (hipHostMalloc / hipHostRegister): device->host copies into it run at full
 * PCIe rate and asynchronously.  rt1w_host_register pins memory the caller already owns, e.g. a POSIX shared-memory
 * mapping that several single-GPU processes fill with RT1W_OUT_FRAME. */
int rt1w_host_alloc(uint64_t bytes, void** out);
int rt1w_host_free(void* p);
int rt1w_host_register(void* p, uint64_t bytes);
int rt1w_host_unregister(void* p);

/* ---- scene-specialised kernels ----
 * Small scenes are traversed by a stackless pre-order sweep.  When the node kinds and subtree ends are compile-time
 * constants that sweep unrolls into straight-line code along the scene's own tree (same arithmetic, bit-identical
 * frames; Cornell box, 29 nodes: 1.3x the generic sweep; scenes of 65-256 nodes: 1.5-2.3x the stack walk).  The constants
 * are only known once a scene is committed, so such a kernel is generated per scene topology and compiled with hiprtc
 * (1-8 s), then kept in a kernel cache: <directory of librt1w.so>/kernels (filled by the build for the reference's own
 * scene arms) and $RT1W_KERNEL_CACHE or ~/.cache/rt1w.  rt1w_context_create looks the scene up in the cache and uses a
 * hit silently; rt1w_context_specialise compiles on a miss.  A render of >= 2^35 paths (2^32 for scenes of more than 64 nodes) compiles on
 * its own -- the compile then costs less than it saves -- unless RT1W_NO_JIT is set in the environment.  Scenes of more than 256 nodes keep the
 * generic kernels: RT1W_ERR_UNSUPPORTED.  RT1W_GENERIC in rt1w_render_params.flags selects the generic kernel for one
 * render. */
#define RT1W_SPECIALISE_CACHED_ONLY 1u /* do not run the compiler: RT1W_ERR_STATE on a cache miss */
#define RT1W_SPECIALISE_TILES 2u /* after the f64 kernel (and the optional f32 one) load the kernel's tile-list form too (RT1W_TILES_SPECIALISED), compiling it unless RT1W_SPECIALISE_CACHED_ONLY is set; its failure is the call's error.  The info describes the rectangle kernel as without the flag; compile_ms includes the tile form's compile */
typedef struct rt1w_specialise_info {
    char key[24];        /* cache key: hash of the generated source, the library's embedded headers and the compiler options */
    uint32_t active;     /* 1: renders on this context now use the specialised kernel */
    uint32_t from_cache; /* 1: the code object came from a cache, 0: it was compiled by this call */
    double compile_ms;   /* time spent in hiprtc by this call */
    uint32_t grid, vgprs;/* persistent grid of the kernel; 0 if unknown */
} rt1w_specialise_info;
int rt1w_context_specialise(rt1w_context* c, uint32_t flags, rt1w_specialise_info* info /* may be NULL */);
/* cache key of the specialised kernel of a committed scene (16 hex digits + NUL): the code object is
 * `sweep_<key>.hsaco` in the kernel cache.  No GPU needed.  RT1W_ERR_UNSUPPORTED for scenes of more than 256 nodes. */
int rt1w_scene_kernel_key(const rt1w_scene* s, char out[24]);
/* copy of the translation unit that is generated for a committed scene (f32 != 0: its single-precision build): the topology tables the
 * specialised kernel is compiled around, as text.  No GPU needed.  Returns bytes written (no NUL), or the needed size if buf==NULL;
 * RT1W_ERR_UNSUPPORTED for scenes of more than 256 nodes. */
int64_t rt1w_scene_kernel_source(const rt1w_scene* s, int f32, char* buf, uint64_t cap);
/* the same two for the kernel's TILE-LIST FORM (f64 only; RT1W_TILES_SPECIALISED): the same tables around a kernel that takes the tile
 * table of rt1w_render_tiles as its last argument -- the list stands in for the row hand-out of src/main.rs:957-963, a tile's record
 * saying where its pixels lie in the image.  Another text, so another key and another `sweep_<key>.hsaco`.  No GPU needed; the
 * refusals of the two above. */
int rt1w_scene_kernel_key_tiles(const rt1w_scene* s, char out[24]);
int64_t rt1w_scene_kernel_source_tiles(const rt1w_scene* s, char* buf, uint64_t cap);

/* ---- output side (src/color.rs) ---- */

/* Color::into_sampled (color.rs:14-21) over n pixels: NaN scrub of the SUM, then * 1/spp */
int rt1w_resolve(const double* sums, uint64_t n_pixels, uint32_t spp, double* means);
/* Display for SampledColor (color.rs:56-65): gamma-2, clamp, *256, truncate; n values -> n bytes */
int rt1w_quantize(const double* means, uint64_t n_values, uint8_t* out);
/* the whole P3 text of src/main.rs:953,1003-1007 for an image whose row 0 is j = 0
 * (rows are emitted top-down, j = height-1 first).  Returns bytes written
 * (excluding NUL) or needed size if buf==NULL. */
int64_t rt1w_format_ppm(const double* means, uint32_t width, uint32_t height, char* buf, uint64_t cap);

/* sizeof of the ABI structs as this library was compiled (bindings check their own layout against it):
 * 0 rt1w_render_params, 1 rt1w_stats, 2 rt1w_scene_info, 3 rt1w_specialise_info, 4 rt1w_denoise_params, 6 rt1w_camera,
 * 8 rt1w_ray_color_params, 10 rt1w_path_params, 11 rt1w_path_state; 0 for anything else (5, 7 and 9 are not given out: they stay codes
 * that answer 0) */
uint32_t rt1w_abi_sizeof(int what);

/* ---- diagnostics ---- */
/* evaluates the numerical contract (include/rt1w_num.h) ON THE DEVICE for n inputs:
 * fn 0 a/b, 1 sqrt|a|, 2 sin a, 3 cos a, 4 acos(a/(|a|+1)), 5 atan2(a,b), 6 log|b|,
 * 7 first gen_f64 of stream (pixel=i, sample=(uint32)a_bits), 8 gen_range(-1,1) of same;
 * 11, 12 the same two of stream (pixel=b_bits, sample=(uint32)a_bits), 13 that gen_range as reserve + rt_take_pm1.
 * 14 a/b from b's prepared divisor (rt_div_q), 15 its guards (1 divisor out of range | 2 quotient bad if used | 4 quotient too large),
 * 16 1/b from the prepared divisor (rt_div_inv).
 * Used by the GPU tests to prove host/device bit equality. */
int rt1w_debug_eval(rt1w_context* c, int fn, const double* a, const double* b, double* out, uint64_t n);
/* AABB::hit (src/aabb.rs:13-32) ON THE DEVICE for n cases, in[i] = {min[3], max[3], origin[3], direction[3], t_min, t_max}:
 * `out_literal` from the compare/select form, `out_fast` from the max/min-instruction form the kernels use when no
 * bound is NaN.  Tests compare both with the host's literal form. */
int rt1w_debug_aabb(rt1w_context* c, const double* in, int* out_literal, int* out_fast, uint64_t n);
/* The shading-side leaf functions ON THE DEVICE for n inputs in[i] = {u, v, p.x, p.y, p.z}, out[i] = 3 doubles:
 * mode 0 `Texture::value(u, v, p)` of texture `tex` of the context's scene (src/texture.rs:40-89) -> rgb;
 * mode 1 `Perlin::noise(p)` and `Perlin::turb(p, 7)` of Perlin table `tex` (src/perlin.rs:46-86) -> out[0], out[1];
 * mode 2 `sphere_uv(p)` (src/math.rs:67-71) -> out[0] = u, out[1] = v; it reads no record of the scene and ignores `tex`.
 * RT1W_ERR_INVALID, before anything is launched: a null pointer, an unknown mode, mode 0 with `tex` not a texture of the scene,
 * mode 1 with `tex` not one of its Perlin tables (a scene has one per noise texture, in the order they were made).
 * Known-answer tests of what no artefact of the reference reaches (lattice points of the noise, checker parity, poles and
 * seam of sphere_uv). */
int rt1w_debug_texture(rt1w_context* c, int mode, uint32_t tex, const double* in, double* out, uint64_t n);
/* per-phase wave-cycle totals of the render kernel since the last reset.  Only the diagnostic build
 * (make stamps -> librt1w_stamps.so, -DRT_STAMPS) fills them (returns 1); the shipped library executes no
 * stamp and returns 0 with zeros.  Buckets: see context.hip. */
int rt1w_debug_stamps(rt1w_context* c, uint64_t out[16], int reset);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
