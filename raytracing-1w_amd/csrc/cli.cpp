/* rt1w -- command-line front end over the C ABI: what the reference's `main` does
 * (src/main.rs:797-1010: pick a scene arm, render, print the P3 image on stdout, progress on
 * stderr), with the pixel loop running on the GPU.  The reference has no flags (the arm is
 * the literal `match 5`, main.rs:815); here the literals are options with the reference's
 * values as defaults.
 *   rt1w [--scene N] [--width W] [--height H] [--spp S] [--depth D] [--seed G] [--build-seed B]
 *        [--device I] [--earth file.rgb8 W H] [--out file.ppm] [--specialise | --generic]
 *        [--reference-stream] [--f32] [--near-far] [--sah] [--denoise [--denoise-iterations N] [--deep-guides [N]] [--variance [K]]]
 *        [--adaptive BUDGET [--max-spp N] [--target-error E] [--one-launch] [--filtered-error [--full-guides] | --cross-filter [--err-out FILE]] [--specialised-tiles]]
 *        [--frames N --orbit DEG [--denoise [--temporal-variance [SIGMA]]]]
 *        [--pick I J] [--panorama W H] [--trace-path I J [S]]
 * --trace-path I J [S] renders nothing: it follows sample S (default 0) of pixel (I, J), J counting the reference's rows j, one level of
 * ray_color at a time (main.rs:51-116) -- rt1w_path_begin for the one state, then rt1w_path_step with n = 1, steps = 1 until the state is
 * dead -- and prints per level the event, the hit leaf's node, the next ray, beta, radiance and the stream word.  The last radiance is
 * that pixel sample of rt1w_render (spp 1, sample_offset S, RT1W_OUT_SUM).  --depth and --seed as for a render.
 * --panorama W H renders an equirectangular 360 x 180 degree image of W x H pixels from the arm's look_from through rt1w_ray_color: the
 * camera is a few lines of host code.  Pixel (i, j), j counting rows from the bottom, looks along longitude phi = 2 pi (i + 1/2) / W - pi
 * + phi0 and latitude theta = pi (j + 1/2) / H - pi / 2: direction (cos theta sin phi, sin theta, -cos theta cos phi), time 0.  phi0 =
 * atan2(dx, -dz) of d = look_at - look_from (0 if d is vertical) puts what the arm's own camera looks at into the middle column.  Ray r = j W + i
 * draws from the streams of pixel seed r (first_stream 0), --spp samples each (default: the arm's), --depth and --seed as for a render;
 * the means go through the quantiser and the PPM writer of every other mode.
 * --pick I J renders nothing: it prints the hit record (rt1w_hit) of the ray through the CENTRE of pixel (I, J), J counting the
 * reference's rows j (0 = bottom row, main.rs:957): origin = the camera's lens centre, direction = lower_left_corner + s horizontal +
 * t vertical - origin with s = (I + 1/2) / (width - 1), t = (J + 1/2) / (height - 1) (rt1w_context_get_camera; the s, t of
 * rt1w_temporal_accumulate step 3), time = the shutter's opening, bounds 0.001 and inf (main.rs:62).
 * --frames N --orbit DEG renders an animation of N frames through rt1w_render_temporal: before frame k look_from is turned about the
 * vertical axis through look_at by k * DEG degrees (rt1w_context_set_camera; the scene, its upload and its kernel are frame 0's), the
 * frame's seed is --seed + k, and the previous frames' samples are reused where their surface points are seen again; with --denoise
 * the feature-guided filter follows; with --denoise --temporal-variance [SIGMA] the frames go through rt1w_render_temporal_var instead: the
 * variance-guided filter, steered by the variance the history itself carries (SIGMA: sigma_variance, default 3).  Frame k is written to NAME_%04d.ppm, NAME being --out without its ".ppm" (default "frame").
 * --adaptive BUDGET spends a budget of BUDGET mean samples per pixel where the frame is noisy (rt1w_render_adaptive; --spp is ignored),
 * at most --max-spp samples on one pixel, none on tiles whose error is at or below --target-error; with --denoise --variance the
 * variance-guided filter follows (first-hit guides of the pilot's samples; K and --deep-guides do not apply).
 * --filtered-error steers the plan by the half-buffer error of the FILTERED frame instead (rt1w_render_adaptive_filtered: the variance-guided
 * filter runs in every round and its last frame is the image; --target-error then means the error of the picture that is printed);
 * --full-guides (with --filtered-error) tops up the first-hit feature buffers of the tiles every round takes, so that the filter's guides hold
 * every sample a pixel has received (rt1w_render_adaptive_guided) instead of the pilot's.
 * --cross-filter is the same plan with the cross-filtered half buffers in every round (rt1w_render_adaptive_cross: each half is filtered with
 * the other's colour term, the image is the mean of the two); it excludes --filtered-error.
 * --specialised-tiles (with --adaptive B and one of --one-launch, --filtered-error, --cross-filter) runs the rounds' tile lists on the
 * tile-list form of the scene-specialised kernel where the kernel cache has one (RT1W_TILES_SPECIALISED; the same frame, bit for bit).
 * --err-out FILE writes the per-pixel error map of that frame as text, "width height" and then one value per pixel, top row first.
 * --denoise renders through rt1w_render_denoised: the frame, its first-hit feature buffers and the feature-guided filter in one call
 * (default 5 levels), then the PPM of the filtered frame.  --deep-guides [N] (implies --denoise) takes the guides through glass and
 * perfect mirrors instead, up to N specular bounces (default 8, at most 64): rt1w_render_denoised_deep with max_fuzz 0.
 * --variance [K] (implies --denoise) renders the samples as K batches (default 4; --spp must be a multiple of K) and filters with the
 * variance-guided filter, which fades out as the frame converges: rt1w_render_denoised_var, with the guides --deep-guides asks for.
 * --reference-stream draws from the reference's own StdRng per pixel (RT1W_RNG_REFERENCE): `rt1w --reference-stream` prints
 * what `cargo run` of the reference prints, byte for byte (Cornell arm, 600x600, 100 spp).  --f32: RT1W_PRECISION_F32.
 * --near-far: rt1w_scene_set_walk_order(RT1W_WALK_NEAR_FAR).  --sah: rt1w_scene_set_bvh_build(RT1W_BVH_SAH).
 * --specialise compiles the kernel for this scene's topology now if the kernel cache has none (rt1w_context_specialise;
 * by default only a cached kernel is used, and renders of >= 2^35 paths compile on their own); --generic forbids it.
 */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rt1w.h"

static int fail(const char* what) {
    std::fprintf(stderr, "rt1w: %s: %s\n", what, rt1w_last_error());
    return 1;
}

int main(int argc, char** argv) {
    int arm = 5, device = 0;
    bool specialise = false, generic = false, reference_stream = false, f32 = false, near_far = false, sah = false, denoise = false;
    long denoise_iterations = 0, deep_guides = -1, variance = -1; /* -1: first-hit guides; -1: the fixed-sigma filter */
    long adaptive = -1, max_spp = 0; /* -1: every pixel gets --spp samples */
    bool one_launch = false;         /* --adaptive: every round as one launch of all its tiles (RT1W_ADAPTIVE_ONE_LAUNCH) */
    bool filtered_error = false;     /* --adaptive: rt1w_render_adaptive_filtered */
    bool cross_filter = false;       /* --adaptive: rt1w_render_adaptive_cross */
    bool full_guides = false;        /* --adaptive --filtered-error: rt1w_render_adaptive_guided */
    bool specialised_tiles = false;  /* --adaptive with rounds through the tile entries: RT1W_TILES_SPECIALISED */
    std::string err_path;
    long pick_i = -1, pick_j = -1;   /* >= 0: --pick, the record under a pixel instead of a render */
    long pano_w = 0, pano_h = 0;     /* > 0: --panorama, an equirectangular image through rt1w_ray_color */
    long trace_i = -1, trace_j = -1, trace_s = 0; /* >= 0: --trace-path, one path level by level instead of a render */
    long frames = 0;                 /* > 0: an animation through rt1w_render_temporal */
    double orbit = 0.0;
    double temporal_variance = -1.0; /* >= 0: the frames through rt1w_render_temporal_var with this sigma_variance (0 = default) */
    double target_error = 0.0;
    long width = -1, height = -1, spp = -1, depth = 50; /* MAX_DEPTH main.rs:801 */
    unsigned long long build_seed = 1, seed = 0;
    std::string out_path, earth_path;
    unsigned earth_w = 0, earth_h = 0;
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        auto next = [&](const char* name) -> const char* {
            if (i + 1 >= argc) { std::fprintf(stderr, "rt1w: %s needs a value\n", name); std::exit(2); }
            return argv[++i];
        };
        if (a == "--scene") arm = std::atoi(next("--scene"));
        else if (a == "--width") width = std::atol(next("--width"));
        else if (a == "--height") height = std::atol(next("--height"));
        else if (a == "--spp") spp = std::atol(next("--spp"));
        else if (a == "--depth") depth = std::atol(next("--depth"));
        else if (a == "--seed") seed = std::strtoull(next("--seed"), nullptr, 10);
        else if (a == "--build-seed") build_seed = std::strtoull(next("--build-seed"), nullptr, 10);
        else if (a == "--device") device = std::atoi(next("--device"));
        else if (a == "--out") out_path = next("--out");
        else if (a == "--specialise") specialise = true;
        else if (a == "--generic") generic = true;
        else if (a == "--reference-stream") reference_stream = true;
        else if (a == "--f32") f32 = true;
        else if (a == "--near-far") near_far = true;
        else if (a == "--sah") sah = true;
        else if (a == "--denoise") denoise = true;
        else if (a == "--denoise-iterations") { denoise = true; denoise_iterations = std::atol(next("--denoise-iterations")); }
        else if (a == "--deep-guides") {
            denoise = true; deep_guides = 8;
            if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') deep_guides = std::atol(argv[++i]);
        }
        else if (a == "--variance") {
            denoise = true; variance = 0;
            if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') variance = std::atol(argv[++i]);
        }
        else if (a == "--adaptive") adaptive = std::atol(next("--adaptive"));
        else if (a == "--one-launch") one_launch = true;
        else if (a == "--filtered-error") filtered_error = true;
        else if (a == "--cross-filter") cross_filter = true;
        else if (a == "--full-guides") full_guides = true;
        else if (a == "--specialised-tiles") specialised_tiles = true;
        else if (a == "--err-out") err_path = next("--err-out");
        else if (a == "--frames") frames = std::atol(next("--frames"));
        else if (a == "--pick") { pick_i = std::atol(next("--pick I")); pick_j = std::atol(next("--pick J")); }
        else if (a == "--panorama") { pano_w = std::atol(next("--panorama W")); pano_h = std::atol(next("--panorama H")); }
        else if (a == "--trace-path") {
            trace_i = std::atol(next("--trace-path I")); trace_j = std::atol(next("--trace-path J"));
            if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') trace_s = std::atol(argv[++i]);
        }
        else if (a == "--temporal-variance") {
            temporal_variance = 0.0;
            if (i + 1 < argc && ((argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') || argv[i + 1][0] == '.')) temporal_variance = std::atof(argv[++i]);
        }
        else if (a == "--orbit") orbit = std::atof(next("--orbit"));
        else if (a == "--max-spp") max_spp = std::atol(next("--max-spp"));
        else if (a == "--target-error") target_error = std::atof(next("--target-error"));
        else if (a == "--earth") { earth_path = next("--earth"); earth_w = (unsigned)std::atoi(next("--earth W")); earth_h = (unsigned)std::atoi(next("--earth H")); }
        else { std::fprintf(stderr, "usage: rt1w [--scene N] [--width W] [--height H] [--spp S] [--depth D] [--seed G] [--build-seed B] [--device I] [--earth file.rgb8 W H] [--out file.ppm] [--specialise | --generic] [--reference-stream] [--f32] [--near-far] [--sah] [--denoise [--denoise-iterations N] [--deep-guides [N]] [--variance [K]]] [--adaptive BUDGET [--max-spp N] [--target-error E] [--one-launch] [--filtered-error [--full-guides] | --cross-filter [--err-out FILE]] [--specialised-tiles]] [--frames N --orbit DEG [--denoise [--temporal-variance [SIGMA]]]] [--pick I J] [--panorama W H] [--trace-path I J [S]]\n"); return 2; }
    }
    std::vector<unsigned char> earth;
    if (!earth_path.empty()) {
        FILE* f = std::fopen(earth_path.c_str(), "rb");
        if (!f) { std::perror("rt1w: --earth"); return 1; }
        earth.resize((size_t)earth_w * earth_h * 3);
        size_t got = std::fread(earth.data(), 1, earth.size(), f);
        std::fclose(f);
        if (got != earth.size()) { std::fprintf(stderr, "rt1w: --earth: short file\n"); return 1; }
    }
    /* aspect_ratio: 16/9 by default, 1.0 for arms 5, 6 and the final scene (main.rs:798,868,896,917);
     * an explicit --width/--height pair overrides it */
    bool square = (arm == 5 || arm == 6 || arm < 0 || arm > 6);
    double aspect = square ? 1.0 : 16.0 / 9.0;
    if (width > 0 && height > 0) aspect = (double)width / (double)height;
    rt1w_scene* scene = nullptr;
    uint32_t defaults[3];
    if (rt1w_scene_build_reference(arm, build_seed, aspect, earth.empty() ? nullptr : earth.data(), earth_w, earth_h, &scene, defaults) < 0)
        return fail("scene");
    if (width <= 0) width = defaults[0];
    if (height <= 0) height = (long)((double)width / aspect); /* main.rs:939 */
    if (spp <= 0) spp = defaults[2];
    if (sah && rt1w_scene_set_bvh_build(scene, RT1W_BVH_SAH) < 0) return fail("BVH build");
    if (near_far && rt1w_scene_set_walk_order(scene, RT1W_WALK_NEAR_FAR) < 0) return fail("walk order");
    rt1w_context* ctx = nullptr;
    if (rt1w_context_create(device, scene, &ctx) < 0) return fail("context");
    if (specialise && !generic) {
        rt1w_specialise_info si;
        if (rt1w_context_specialise(ctx, 0, &si) < 0) std::fprintf(stderr, "rt1w: not specialised: %s\n", rt1w_last_error());
        else std::fprintf(stderr, "rt1w: kernel %s (%s, %.1f s in the compiler)\n", si.key, si.from_cache ? "from the kernel cache" : "compiled", si.compile_ms / 1e3);
    }
    if (pick_i >= 0 || pick_j >= 0) {
        if (pick_i < 0 || pick_j < 0 || pick_i >= width || pick_j >= height) { std::fprintf(stderr, "rt1w: --pick I J: a pixel of the %ldx%ld frame\n", width, height); return 2; }
        rt1w_camera cam;
        if (rt1w_context_get_camera(ctx, &cam) < 0) return fail("camera");
        const double s = ((double)pick_i + 0.5) / (double)(width > 1 ? width - 1 : 1), t = ((double)pick_j + 0.5) / (double)(height > 1 ? height - 1 : 1);
        double ray[9], rec[12];
        for (int k = 0; k < 3; ++k) {
            ray[k] = cam.origin[k];
            ray[3 + k] = cam.lower_left_corner[k] + s * cam.horizontal[k] + t * cam.vertical[k] - cam.origin[k];
        }
        ray[6] = cam.time0; ray[7] = 0.001; ray[8] = HUGE_VAL;
        rt1w_hit_params hp;
        std::memset(&hp, 0, sizeof hp);
        hp.n = 1u; hp.first_stream = (uint64_t)pick_j * (uint64_t)width + (uint64_t)pick_i; hp.global_seed = (uint32_t)seed;
        uint32_t node;
        rt1w_stats hs;
        if (rt1w_hit(ctx, &hp, ray, rec, &node, &hs) < 0) return fail("pick");
        std::printf("pixel %ld %ld\norigin %.17g %.17g %.17g\ndirection %.17g %.17g %.17g\n", pick_i, pick_j, ray[0], ray[1], ray[2], ray[3], ray[4], ray[5]);
        if (rec[0] == 0.0) std::printf("miss\n");
        else
            std::printf("hit\nt %.17g\np %.17g %.17g %.17g\nnormal %.17g %.17g %.17g\nu %.17g\nv %.17g\nfront_face %d\nmaterial %u\nnode %u\n", rec[1], rec[2],
                        rec[3], rec[4], rec[5], rec[6], rec[7], rec[8], rec[9], (int)rec[10], (unsigned)rec[11], node);
        rt1w_context_destroy(ctx);
        rt1w_scene_destroy(scene);
        return 0;
    }
    if (trace_i >= 0 || trace_j >= 0) {
        if (trace_i < 0 || trace_j < 0 || trace_i >= width || trace_j >= height || trace_s > 0xFFFFFFFEl) { std::fprintf(stderr, "rt1w: --trace-path I J [S]: a pixel of the %ldx%ld frame\n", width, height); return 2; }
        static const char* const events[] = {"none", "miss", "depth exhausted", "DiffuseLight", "() absorbed", "Lambertian", "Metal", "Dielectric", "Isotropic", "not traced"};
        const uint32_t pixel[3] = {(uint32_t)trace_i, (uint32_t)trace_j, (uint32_t)trace_s};
        rt1w_path_state st;
        rt1w_stats ps;
        if (rt1w_path_begin(ctx, (uint32_t)width, (uint32_t)height, (uint64_t)(uint32_t)seed, (uint32_t)depth, pixel, 1u, &st, &ps) < 0) return fail("trace-path");
        rt1w_path_params pp;
        std::memset(&pp, 0, sizeof pp);
        pp.n = 1u; pp.global_seed = (uint32_t)seed; pp.steps = 1u;
        const auto print_state = [&st]() {
            std::printf("  ray %.17g %.17g %.17g  %.17g %.17g %.17g  time %.17g\n  beta %.17g %.17g %.17g\n  radiance %.17g %.17g %.17g\n  word %u  depth_left %u\n",
                        st.ray[0], st.ray[1], st.ray[2], st.ray[3], st.ray[4], st.ray[5], st.ray[6], st.beta[0], st.beta[1], st.beta[2], st.radiance[0],
                        st.radiance[1], st.radiance[2], st.word, st.depth_left);
        };
        std::printf("pixel %ld %ld sample %ld stream %llu\nlevel 0: camera\n", trace_i, trace_j, trace_s, (unsigned long long)st.stream);
        print_state();
        for (long level = 1; st.status & RT1W_PATH_ALIVE; ++level) {
            uint32_t node;
            if (rt1w_path_step(ctx, &pp, &st, &st, &node, &ps) < 0) return fail("trace-path");
            const uint32_t ev = RT1W_PATH_EVENT(st.status);
            std::printf("level %ld: %s", level, ev < 10u ? events[ev] : "?");
            if (node != 0xFFFFFFFFu) std::printf(", node %u", node);
            std::printf("%s\n", (st.status & RT1W_PATH_ALIVE) ? "" : ", the path ends");
            print_state();
        }
        rt1w_context_destroy(ctx);
        rt1w_scene_destroy(scene);
        return 0;
    }
    if (pano_w != 0 || pano_h != 0) {
        if (pano_w < 1 || pano_h < 1 || (unsigned long long)pano_w * (unsigned long long)pano_h > 0xFFFFFFFFull) { std::fprintf(stderr, "rt1w: --panorama W H: at least 1 x 1, at most 2^32 - 1 pixels\n"); return 2; }
        if (reference_stream || f32 || denoise || adaptive >= 0 || frames > 0) { std::fprintf(stderr, "rt1w: --panorama goes with --scene, --spp, --depth, --seed and --out only\n"); return 2; }
        double lf[3], la[3], up[3], vfov, aperture, focus;
        if (rt1w_reference_camera(arm, lf, la, up, &vfov, &aperture, &focus) < 0) return fail("camera");
        const size_t n = (size_t)pano_w * (size_t)pano_h;
        const double pi = 3.14159265358979323846;
        const double dx = la[0] - lf[0], dz = la[2] - lf[2];
        const double phi0 = (dx == 0.0 && dz == 0.0) ? 0.0 : std::atan2(dx, -dz); /* the middle column looks towards look_at */
        std::vector<double> rays(n * 7), means(n * 3);
        for (long j = 0; j < pano_h; ++j)
            for (long i = 0; i < pano_w; ++i) {
                const double phi = 2.0 * pi * (((double)i + 0.5) / (double)pano_w) - pi + phi0, theta = pi * (((double)j + 0.5) / (double)pano_h) - 0.5 * pi;
                double* r = rays.data() + ((size_t)j * pano_w + i) * 7;
                r[0] = lf[0]; r[1] = lf[1]; r[2] = lf[2];
                r[3] = std::cos(theta) * std::sin(phi); r[4] = std::sin(theta); r[5] = -(std::cos(theta) * std::cos(phi));
                r[6] = 0.0;
            }
        rt1w_ray_color_params rp;
        std::memset(&rp, 0, sizeof rp);
        rp.n = n; rp.spp = (uint32_t)spp; rp.max_depth = (uint32_t)depth; rp.global_seed = (uint32_t)seed;
        rt1w_stats rs;
        std::fprintf(stderr, "rt1w: scene arm %d, panorama %ldx%ld, %ld spp, depth %ld\n", arm, pano_w, pano_h, spp, depth);
        if (rt1w_ray_color(ctx, &rp, rays.data(), nullptr, means.data(), &rs) < 0) return fail("panorama");
        const int64_t len = rt1w_format_ppm(means.data(), (uint32_t)pano_w, (uint32_t)pano_h, nullptr, 0);
        if (len < 0) return fail("format");
        std::vector<char> text((size_t)len + 1);
        if (rt1w_format_ppm(means.data(), (uint32_t)pano_w, (uint32_t)pano_h, text.data(), (uint64_t)len + 1) < 0) return fail("format");
        FILE* f = out_path.empty() ? stdout : std::fopen(out_path.c_str(), "w");
        if (!f) { std::perror("rt1w: --out"); return 1; }
        std::fwrite(text.data(), 1, (size_t)len, f);
        if (f != stdout) std::fclose(f);
        std::fprintf(stderr, "Done\nrt1w: %.1f ms kernels, %.1f Mpaths/s, %.2f segments/path, kernel variant V%u\n", rs.kernel_ms,
                     (double)rs.paths / rs.kernel_ms / 1e3, (double)rs.segments / (double)rs.paths, rs.variant);
        rt1w_context_destroy(ctx);
        rt1w_scene_destroy(scene);
        return 0;
    }
    rt1w_render_params p;
    std::memset(&p, 0, sizeof p);
    p.width = (uint32_t)width; p.height = (uint32_t)height; p.tile_w = p.width; p.tile_h = p.height;
    p.spp = (uint32_t)spp; p.max_depth = (uint32_t)depth; p.global_seed = (uint32_t)seed;
    if (generic) p.flags |= RT1W_GENERIC;
    if (specialised_tiles) {
        if (adaptive < 0 || !(one_launch || filtered_error || cross_filter) || generic) {
            std::fprintf(stderr, "rt1w: --specialised-tiles goes with --adaptive B and --one-launch, --filtered-error or --cross-filter, without --generic\n"); return 2;
        }
        p.flags |= RT1W_TILES_SPECIALISED;
    }
    if (reference_stream) p.flags |= RT1W_RNG_REFERENCE;
    if (f32) p.precision = RT1W_PRECISION_F32;
    rt1w_stats st;
    if (temporal_variance >= 0.0 && (frames <= 0 || !denoise)) { std::fprintf(stderr, "rt1w: --temporal-variance goes with --frames N --denoise\n"); return 2; }
    if (frames > 0) {
        if (adaptive >= 0 || variance >= 0 || deep_guides >= 0 || reference_stream || f32) { std::fprintf(stderr, "rt1w: --frames goes with --denoise only\n"); return 2; }
        double lf[3], la[3], up[3], vfov, aperture, focus;
        if (rt1w_reference_camera(arm, lf, la, up, &vfov, &aperture, &focus) < 0) return fail("camera");
        std::string name = out_path.empty() ? "frame" : out_path;
        if (name.size() > 4 && name.compare(name.size() - 4, 4, ".ppm") == 0) name.resize(name.size() - 4);
        rt1w_denoise_params d;
        std::memset(&d, 0, sizeof d);
        d.iterations = denoise_iterations > 0 ? (uint32_t)denoise_iterations : 0u;
        std::vector<double> means((size_t)width * height * 3);
        std::fprintf(stderr, "rt1w: scene arm %d, %ld frames of %ldx%ld, %ld spp, %g degrees per frame\n", arm, frames, width, height, spp, orbit);
        double kernel_ms = 0.0;
        for (long k = 0; k < frames; ++k) {
            /* look_from about the vertical axis through look_at */
            const double t = orbit * (double)k * 3.14159265358979323846 / 180.0, c = std::cos(t), sn = std::sin(t);
            const double dx = lf[0] - la[0], dz = lf[2] - la[2];
            const double from[3] = {la[0] + c * dx + sn * dz, lf[1], la[2] - sn * dx + c * dz};
            if (rt1w_context_set_camera(ctx, from, la, up, vfov, aspect, aperture, focus, 0.0, 1.0) < 0) return fail("camera");
            p.global_seed = (uint32_t)seed + (uint32_t)k;
            if ((temporal_variance >= 0.0 ? rt1w_render_temporal_var(ctx, &p, nullptr, &d, temporal_variance, means.data(), &st)
                                          : rt1w_render_temporal(ctx, &p, nullptr, denoise ? &d : nullptr, means.data(), &st)) < 0) return fail("render");
            kernel_ms += st.kernel_ms;
            const int64_t n = rt1w_format_ppm(means.data(), p.width, p.height, nullptr, 0);
            if (n < 0) return fail("format");
            std::vector<char> text((size_t)n + 1);
            if (rt1w_format_ppm(means.data(), p.width, p.height, text.data(), (uint64_t)n + 1) < 0) return fail("format");
            char file[32];
            std::snprintf(file, sizeof file, "_%04ld.ppm", k);
            FILE* f = std::fopen((name + file).c_str(), "w");
            if (!f) { std::perror("rt1w: --out"); return 1; }
            std::fwrite(text.data(), 1, (size_t)n, f);
            std::fclose(f);
            std::fprintf(stderr, "\rFrames remaining: %ld ", frames - 1 - k);
        }
        std::fprintf(stderr, "\nDone\nrt1w: %.1f ms kernels in %ld frames\n", kernel_ms, frames);
        rt1w_context_destroy(ctx);
        rt1w_scene_destroy(scene);
        return 0;
    }
    /* the reference collects the rows top-down, counting them down on stderr (main.rs:957-960,995-998), then prints them
     * (main.rs:1003-1007); here the rows are quantised on the device and written as their strips land */
    std::vector<unsigned char> img((size_t)width * height * 3);
    FILE* o = out_path.empty() ? stdout : std::fopen(out_path.c_str(), "w");
    if (!o) { std::perror("rt1w: --out"); return 1; }
    std::fprintf(o, "P3\n%u %u\n255\n", p.width, p.height);
    struct Sink { FILE* o; const unsigned char* img; uint32_t w, written; std::string line; } sink{o, img.data(), p.width, 0, {}};
    auto on_rows = [](void* user, uint32_t rows_done, uint32_t rows_total) -> int {
        Sink& k = *static_cast<Sink*>(user);
        for (; k.written < rows_done; ++k.written) {
            const unsigned char* row = k.img + (size_t)k.written * k.w * 3;
            k.line.clear();
            char buf[16];
            for (uint32_t i = 0; i < k.w; ++i) {
                int n = std::snprintf(buf, sizeof buf, "%u %u %u\n", row[3 * i], row[3 * i + 1], row[3 * i + 2]); /* color.rs:59-64 */
                k.line.append(buf, (size_t)n);
            }
            std::fwrite(k.line.data(), 1, k.line.size(), k.o);
        }
        std::fprintf(stderr, "\rScanlines remaining: %u ", rows_total - rows_done);
        return 0;
    };
    std::fprintf(stderr, "rt1w: scene arm %d, %ldx%ld, %ld spp, depth %ld\n", arm, width, height, spp, depth);
    if (adaptive < 0 && (filtered_error || !err_path.empty())) { std::fprintf(stderr, "rt1w: --filtered-error and --err-out go with --adaptive\n"); return 2; }
    if (cross_filter && filtered_error) { std::fprintf(stderr, "rt1w: --cross-filter and --filtered-error exclude each other\n"); return 2; }
    if (full_guides && !filtered_error) { std::fprintf(stderr, "rt1w: --full-guides goes with --adaptive B --filtered-error\n"); return 2; }
    if (adaptive < 0 && cross_filter) { std::fprintf(stderr, "rt1w: --cross-filter goes with --adaptive\n"); return 2; }
    if (!err_path.empty() && !filtered_error && !cross_filter) { std::fprintf(stderr, "rt1w: --err-out goes with --filtered-error\n"); return 2; }
    if (adaptive >= 0) {
        if (denoise && variance < 0 && !filtered_error && !cross_filter) { std::fprintf(stderr, "rt1w: --adaptive filters with --denoise --variance only\n"); return 2; }
        rt1w_adaptive_params ap;
        std::memset(&ap, 0, sizeof ap);
        ap.size = (uint32_t)sizeof ap; ap.budget_spp = (uint32_t)adaptive; ap.max_spp = (uint32_t)max_spp; ap.target_error = target_error;
        if (one_launch) ap.flags |= RT1W_ADAPTIVE_ONE_LAUNCH;
        rt1w_denoise_params d;
        std::memset(&d, 0, sizeof d);
        d.iterations = denoise_iterations > 0 ? (uint32_t)denoise_iterations : 0u;
        std::vector<double> means((size_t)width * height * 3);
        if (filtered_error || cross_filter) {
            std::vector<double> err(err_path.empty() ? 0 : (size_t)width * height);
            if ((cross_filter ? rt1w_render_adaptive_cross : full_guides ? rt1w_render_adaptive_guided : rt1w_render_adaptive_filtered)(ctx, &p, &ap, &d, 0.0, means.data(), nullptr, err.empty() ? nullptr : err.data(), &st) < 0) return fail("render");
            if (!err.empty()) {
                FILE* e = std::fopen(err_path.c_str(), "w");
                if (!e) { std::perror("rt1w: --err-out"); return 1; }
                std::fprintf(e, "%u %u\n", p.width, p.height);
                for (uint32_t r = 0; r < p.height; ++r)
                    for (uint32_t i = 0; i < p.width; ++i) std::fprintf(e, "%.17g\n", err[(size_t)(p.height - 1u - r) * p.width + i]);
                std::fclose(e);
            }
        } else if (rt1w_render_adaptive(ctx, &p, &ap, denoise ? &d : nullptr, 0.0, means.data(), nullptr, &st) < 0) return fail("render");
        std::fprintf(stderr, "rt1w: adaptive: %.2f samples per pixel in %u rounds, %u render launches\n", (double)st.paths / ((double)width * height), st.n_chunks, st.passes);
        for (uint32_t r = 0; r < p.height; ++r)
            if (rt1w_quantize(means.data() + (size_t)(p.height - 1u - r) * p.width * 3, (uint64_t)p.width * 3, img.data() + (size_t)r * p.width * 3) < 0) return fail("quantize");
        on_rows(&sink, p.height, p.height);
    } else if (denoise) {
        rt1w_denoise_params d;
        std::memset(&d, 0, sizeof d);
        d.iterations = denoise_iterations > 0 ? (uint32_t)denoise_iterations : 0u;
        std::vector<double> means((size_t)width * height * 3);
        if ((variance >= 0 ? rt1w_render_denoised_var(ctx, &p, &d, (uint32_t)variance, 0.0, deep_guides >= 0 ? (uint32_t)deep_guides : 0u, 0.0, means.data(), &st)
             : deep_guides >= 0 ? rt1w_render_denoised_deep(ctx, &p, &d, (uint32_t)deep_guides, 0.0, means.data(), &st)
             : rt1w_render_denoised(ctx, &p, &d, means.data(), &st)) < 0) return fail("render");
        /* quantised as the reference prints it (color.rs:56-65), top row (j = height - 1) first (main.rs:957-960) */
        for (uint32_t r = 0; r < p.height; ++r)
            if (rt1w_quantize(means.data() + (size_t)(p.height - 1u - r) * p.width * 3, (uint64_t)p.width * 3, img.data() + (size_t)r * p.width * 3) < 0) return fail("quantize");
        on_rows(&sink, p.height, p.height);
    } else if (rt1w_render_rows(ctx, &p, 0, RT1W_ROWS_U8, img.data(), on_rows, &sink, &st) < 0) return fail("render");
    std::fprintf(stderr, "\nDone\nrt1w: %.1f ms kernels, %.1f Mpaths/s, %.2f segments/path, kernel variant V%u%s\n", st.kernel_ms,
                 (double)st.paths / st.kernel_ms / 1e3, (double)st.segments / (double)st.paths, st.variant, (st.sorted & 4u) ? " (scene-specialised)" : "");
    if (o != stdout) std::fclose(o);
    rt1w_context_destroy(ctx);
    rt1w_scene_destroy(scene);
    return 0;
}
