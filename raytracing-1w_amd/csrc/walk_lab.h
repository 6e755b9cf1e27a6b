/* walk_lab.h -- entry points of the trace-only harness (walk_lab.hip).  Diagnostics: a library of their own (librt1w_lab.so, linked
 * against librt1w.so), not part of include/rt1w.h; tools/walk_lab.py and the GPU tests bind them with ctypes. */
#ifndef RT1W_WALK_LAB_H
#define RT1W_WALK_LAB_H

#include <stdint.h>

#include "rt1w.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

typedef struct rt1w_lab rt1w_lab;

int rt1w_lab_create(rt1w_context* c, const rt1w_scene* s, rt1w_lab** out);
void rt1w_lab_destroy(rt1w_lab* l);
/* out = {W1 available, inner pair records, leaf groups, kernel variant of the product's walk} */
int rt1w_lab_info(const rt1w_lab* l, uint32_t out[4]);
/* rays traced at bounces 0 .. n_bounces-1 by the paths of the tile (spp samples per pixel): out[b][path][8] =
 * {origin, direction, time, valid}; path = (row * tile_w + column) * spp + sample */
int rt1w_lab_dump_rays(rt1w_lab* l, const rt1w_render_params* p, uint32_t n_bounces, double* out_host);
/* L1 gather probe: records (64 B of the node array at pseudo-random indices) per launch and the kernel ms of
 * {own record, quad-shared} x {independent, dependent} index streams */
int rt1w_lab_gather_probe(rt1w_lab* l, uint32_t iters, uint32_t blocks_per_cu, double out_ms[4], uint64_t* records_per_launch);
/* rays[n][8] (slot 7 ignored) */
int rt1w_lab_set_rays(rt1w_lab* l, const double* rays, uint64_t n);
/* closest hit (t_min 0.001, t_max inf: main.rs:62) of every ray with walk `mode`; kernel time = best of `repeats` */
int rt1w_lab_trace(rt1w_lab* l, int mode, const uint32_t params[4], int repeats, double* out_t, uint32_t* out_prim, uint32_t* out_flags,
                   double* ms_best, uint64_t stats_out[8]);

/* CPU twin of rt1w_render_aov (aov_host.cpp: rt_aov.h built for the host): the same double[tile_h][tile_w][8] for a committed scene,
 * same variant choice (or p->flags' RT1W_FORCE_VARIANT), no GPU.  RT1W_OK, RT1W_ERR_INVALID / _UNSUPPORTED as the device entry,
 * RT1W_ERR_STATE if a traversal stack overflowed */
int rt1w_lab_aov_host(const rt1w_scene* s, const rt1w_render_params* p, double* out);
/* CPU twin of rt1w_render_aov_deep (aov_host.cpp: rt_aov_deep.h built for the host), same returns; max_specular / max_fuzz refused as
 * the device entry refuses them.  Optional: *segments = the rays traced (rt1w_stats.segments of the device entry),
 * lengths[tile_h][tile_w][spp] = the rays of every sample, 1 .. max_specular + 1 */
int rt1w_lab_aov_deep_host(const rt1w_scene* s, const rt1w_render_params* p, uint32_t max_specular, double max_fuzz, double* out,
                           uint64_t* segments, uint8_t* lengths);

/* CPU twin of rt1w_hit (aov_host.cpp: rt_hit.h built for the host): the same out[n][12] and out_node[n] (may be null) for a committed
 * scene, same variant choice (or p->flags' RT1W_FORCE_VARIANT), no GPU.  RT1W_OK, RT1W_ERR_INVALID as the device entry (null pointers,
 * n, global_seed, flags, overlapping buffers), RT1W_ERR_STATE if a traversal stack overflowed */
int rt1w_lab_hit_host(const rt1w_scene* s, const rt1w_hit_params* p, const double* rays, double* out, uint32_t* out_node);
/* CPU twin of rt1w_debug_texture (aov_host.cpp: rt_texture, rt_perlin_noise, rt_perlin_turb and rt_sphere_uv of rt_core.h built for the
 * host, called as rt_debug_texture_kernel calls them): the same modes, in[n][5] = {u, v, p.x, p.y, p.z} and out[n][3], over a committed
 * scene's own arrays, no GPU.  RT1W_OK, RT1W_ERR_INVALID with the probe's own text (null pointers, an unknown mode, mode 0 with tex
 * beyond the textures, mode 1 with tex beyond the Perlin tables) */
int rt1w_lab_texture_host(const rt1w_scene* s, int mode, uint32_t tex, const double* in, double* out, uint64_t n);
/* the camera rays of a tile: out[tile_h][tile_w][spp][8] = {origin, direction, time, 1} of the ray rt_path_begin gives sample
 * sample_offset + k of the pixel -- the ray rt1w_render and rt1w_render_aov trace first (main.rs:964-971, camera.rs:61-73).  No GPU;
 * refusals of rt1w_lab_aov_host */
int rt1w_lab_camera_rays_host(const rt1w_scene* s, const rt1w_render_params* p, double* out);
/* the same rays and, per ray, out_word[tile_h][tile_w][spp] (may be null) = the word its sample's stream stands at behind rt_path_begin
 * (rt1w_num.h: rt_rng_pos as one number, 4 * block + word): what rt1w_ray_color takes as start_word to continue that sample */
int rt1w_lab_camera_rays_pos_host(const rt1w_scene* s, const rt1w_render_params* p, double* out, uint32_t* out_word);
/* CPU twin of rt1w_ray_color (aov_host.cpp: rt_ray_list.h and rt_core.h built for the host): the same out[n][3] for a committed scene, the
 * scene's own variant, no GPU; per ray, per work item of `chunk` samples, per sample rt_rng_at and rt_path_step until the path ends, summed
 * as the kernels sum.  *segments (may be null) = the rays traced (rt1w_stats.segments of the entries).  RT1W_OK, RT1W_ERR_INVALID with the
 * entries' own text (rt_ray_color_refusal), RT1W_ERR_STATE if a traversal stack overflowed */
int rt1w_lab_ray_color_host(const rt1w_scene* s, const rt1w_ray_color_params* p, const double* rays, const uint32_t* start_word, double* out,
                            uint64_t* segments);
/* the same call; ray_segments (may be null) uint32[n]: the rays traced for ray r, over all of its samples -- they add up to *segments */
int rt1w_lab_ray_color_counts_host(const rt1w_scene* s, const rt1w_ray_color_params* p, const double* rays, const uint32_t* start_word, double* out,
                                   uint64_t* segments, uint32_t* ray_segments);

/* CPU twin of rt1w_path_step (aov_host.cpp: rt_path_state.h and rt_core.h built for the host): the same out[n] and out_node[n] (may be
 * null) for a committed scene, same variant choice (or p->flags' RT1W_FORCE_VARIANT), no GPU; `in` may be `out`, and neither needs an
 * alignment.  *segments (may be null) = the levels that traced a ray (rt1w_stats.segments of the entries).  RT1W_OK, RT1W_ERR_INVALID with
 * the entries' own text (rt_path_step_refusal), RT1W_ERR_STATE if a traversal stack overflowed */
int rt1w_lab_path_step_host(const rt1w_scene* s, const rt1w_path_params* p, const rt1w_path_state* in, rt1w_path_state* out, uint32_t* out_node,
                            uint64_t* segments);
/* CPU twin of rt1w_path_begin (aov_host.cpp: rt_state_begin of rt_path_state.h built for the host) over the scene's own camera, which
 * rt1w_lab_scene_set_camera moves as rt1w_context_set_camera moves a context's; refusals and texts of the entries */
int rt1w_lab_path_begin_host(const rt1w_scene* s, uint32_t width, uint32_t height, uint64_t global_seed, uint32_t max_depth, const uint32_t* pixels,
                             uint64_t n, rt1w_path_state* out);

/* CPU twin of rt1w_denoise (denoise_host.cpp: rt_denoise.h built for the host): the same double[h][w][3] from host buffers, no GPU.
 * RT1W_OK, or RT1W_ERR_INVALID as the device entry (null pointers, zero sizes, iterations > 8, unknown flags, bad sigmas) */
int rt1w_lab_denoise_host(const rt1w_denoise_params* p, const double* frame, const double* aov, double* out);
/* CPU twins of rt1w_batch_variance and rt1w_denoise_var (denoise_host.cpp: rt_denoise_var.h built for the host): the same frame[h][w][3] and
 * var[h][w], the same out[h][w][3], from host buffers, no GPU; RT1W_ERR_INVALID as the device entries */
int rt1w_lab_batch_variance_host(uint32_t width, uint32_t height, uint32_t batches, uint32_t batch_spp, uint32_t flags, const double* sums,
                                 const double* aov, double* frame, double* var);
int rt1w_lab_denoise_var_host(const rt1w_denoise_params* p, const double* frame, const double* aov, const double* var, double sigma_variance,
                              double* out);
/* how rt1w_render_denoised_var takes its `batches` and `sigma_variance` for a render of `spp` samples: out = {batches K, samples per batch n},
 * or RT1W_ERR_INVALID exactly where that entry refuses them (K outside 2 .. 16, spp not a multiple of K, sigma negative or not finite) */
int rt1w_lab_denoised_var_split(uint32_t spp, uint32_t batches, double sigma_variance, uint32_t out[2]);
/* CPU twins of rt1w_accum_merge, rt1w_accum_resolve and rt1w_accum_tile_error (adaptive_host.cpp: rt_adaptive.h built for the host): the
 * same accumulator, the same frame / var / spp and the same tile errors from host buffers, no GPU; RT1W_ERR_INVALID as the device entries */
int rt1w_lab_accum_merge_host(uint32_t width, uint32_t height, uint32_t x0, uint32_t y0, uint32_t tile_w, uint32_t tile_h, uint32_t batch_spp,
                              uint32_t flags, const double* tile_sums, const double* aov, double* acc);
int rt1w_lab_accum_merge_tiles_host(uint32_t width, uint32_t height, uint32_t tile, const rt1w_tile* tiles, uint32_t n_tiles, uint32_t batch_spp,
                                    uint32_t flags, const double* tile_sums, const double* aov, double* acc);
int rt1w_lab_accum_resolve_host(uint32_t width, uint32_t height, uint32_t batch_spp, const double* acc, double* frame, double* var, double* spp);
int rt1w_lab_tile_error_host(uint32_t width, uint32_t height, uint32_t tile, const double* acc, double* err);
/* CPU twins of rt1w_halves_resolve, rt1w_denoise_var_halves and rt1w_tile_error_map (adaptive_host.cpp, denoise_host.cpp:
 * rt_denoise_halves.h built for the host): the same buffers from host buffers, no GPU; RT1W_ERR_INVALID as the device entries.  In the
 * filter twin `out` may be `frame` */
int rt1w_lab_halves_resolve_host(uint32_t width, uint32_t height, uint32_t batch_spp, const double* acc_a, const double* acc_b, double* frame,
                                 double* var, double* half_a, double* half_b, double* spp);
int rt1w_lab_denoise_var_halves_host(const rt1w_denoise_params* p, const double* frame, const double* aov, const double* var, const double* half_a,
                                     const double* half_b, double sigma_variance, double* out, double* err_px,
                                     double* filtered_a /* [h][w][3], may be null: a' * A_p */, double* filtered_b /* likewise */);
int rt1w_lab_tile_error_map_host(uint32_t width, uint32_t height, uint32_t tile, const double* err_px, double* err);
/* CPU twin of rt1w_denoise_cross (denoise_host.cpp: rt_denoise_cross.h built for the host); `out` may be `frame`.  rec, for the tests: the
 * record of the last level before the finish, still demodulated -- a' rgb, la', va', b' rgb, lb', vb' */
int rt1w_lab_denoise_cross_host(const rt1w_denoise_params* p, const double* frame, const double* aov, const double* var, const double* half_a,
                                const double* half_b, double sigma_variance, double* out, double* err_px, double* rec /* [h][w][10], may be null */);
/* CPU twins of rt1w_render_aov_tiles (aov_host.cpp: rt_aov_tiles.h built for the host), rt1w_guides_merge_tiles and rt1w_guides_resolve
 * (adaptive_host.cpp: rt_guides.h built for the host): the same sums[n_tiles][tile][tile][8], the same gacc[h][w][9] and aov[h][w][8], no
 * GPU; refusals and returns as the device entries, RT1W_ERR_STATE if a traversal stack overflowed */
int rt1w_lab_aov_tiles_host(const rt1w_scene* s, const rt1w_render_params* p, uint32_t tile, const rt1w_tile* tiles, uint32_t n_tiles, double* out);
int rt1w_lab_guides_merge_tiles_host(uint32_t width, uint32_t height, uint32_t tile, const rt1w_tile* tiles, uint32_t n_tiles, uint32_t spp,
                                     const double* tile_sums, double* gacc);
int rt1w_lab_guides_resolve_host(uint32_t width, uint32_t height, const double* gacc, double* aov);
/* CPU twin of rt1w_temporal_accumulate (denoise_host.cpp: rt_temporal.h built for the host): the same hist[h][w][3], len[h][w] and
 * frame_out[h][w][3] from host buffers, no GPU; RT1W_ERR_INVALID as the device entry (null pointers, overlapping outputs, zero sizes,
 * unknown flags, bad tolerances).  rec, for the tests: per pixel fx, fy, the four taps' weights (0 where a tap is not valid), their sum,
 * 1 / 0 history */
int rt1w_lab_temporal_host(const rt1w_temporal_params* p, const double* cur_frame, const double* cur_aov, const rt1w_camera* cur_cam,
                           const double* prev_hist, const double* prev_len, const double* prev_aov, const rt1w_camera* prev_cam, double* hist,
                           double* len, double* frame_out, double* rec /* [h][w][8], may be null */);
/* CPU twins of rt1w_temporal_moments and rt1w_temporal_variance (denoise_host.cpp: rt_temporal.h and rt_temporal_var.h built for the host),
 * no GPU; RT1W_ERR_INVALID as the device entries.  rec as above */
int rt1w_lab_temporal_moments_host(const rt1w_temporal_params* p, const double* cur_frame, const double* cur_aov, const rt1w_camera* cur_cam,
                                   const double* prev_hist, const double* prev_m2, const double* prev_len, const double* prev_aov,
                                   const rt1w_camera* prev_cam, double* hist, double* m2, double* len, double* frame_out,
                                   double* rec /* [h][w][8], may be null */);
int rt1w_lab_temporal_variance_host(uint32_t width, uint32_t height, const double* hist, const double* m2, const double* len, const double* aov, double* var);
/* The camera of a COMMITTED scene as the twins and rt1w_scene_copy_flat see it (aov_host.cpp).  set: what rt1w_context_set_camera does to
 * a context's view, done to the scene's own record through the same function (csrc/scene.h: camera_make) with the same refusals -- the
 * twins, which build their view from the scene, then render the camera a live context would.  A diagnostic: it breaks the rule that a
 * committed scene is immutable.  Everything made from the scene afterwards -- a context too -- sees a scene committed with these
 * arguments; contexts made before keep the camera they copied.  get: the ten quantities of the scene's record */
int rt1w_lab_scene_set_camera(rt1w_scene* s, const double look_from[3], const double look_at[3], const double vup[3], double vfov_deg,
                              double aspect_ratio, double aperture, double focus_dist, double time0, double time1);
int rt1w_lab_scene_get_camera(const rt1w_scene* s, rt1w_camera* out);
/* the two functions the filters build their weights from (rt_denoise.h), on their own: out[i] = rt_dn_falloff(x[i]) (fn 0; e may be
 * null) or rt_dn_powi(x[i], e[i]) (fn 1).  device 0: the host build of denoise_host.cpp, no GPU; device 1: one lane per element on
 * GPU 0 (f32_exact.hip).  RT1W_ERR_INVALID for anything else, null pointers or n = 0 */
int rt1w_lab_denoise_elementary(int device, int fn, const double* x, const uint32_t* e, uint64_t n, double* out);

/* f32_exact.hip.  rt1w_lab_f32_exact: on != 0 makes every RT1W_PRECISION_F32 render of the process run the f32 kernels built with 64-bit
 * elementary functions (generic kernels only; the build the CPU twin oracle/oracle_flat_f32.cpp equals bit for bit) instead of the
 * product's; returns the previous setting.  rt1w_lab_f32_elementary: out[i] = the device's single-precision fn of (x[i], y[i]) as the
 * product's f32 kernels call it -- fn 0 sinf(x), 1 cosf(x), 2 atan2f(x, y), 3 acosf(x), 4 logf(x) */
int rt1w_lab_f32_exact(int on);
int rt1w_lab_f32_elementary(int device, int fn, const float* x, const float* y, uint64_t n, float* out);
/* the draw layer of the f32 builds (include/rt1w_num.h under RT_F32) on given 64-bit words: out[i] = what the f32 core holds after
 * assigning the draw of words[i] to its float.  fn (rt_f32_draws.h): 0 the unit draw rt_f64_from_bits, 1 the range draw
 * rt_range_from_bits(lo, hi) with one take and no retry, 2 rt_take_range(lo, hi) over a stream of words[i] then the word 0 (= the
 * single take where the retry accepts it, lo where it rejects), 3 rt_take_f64, 4 rt_gen_f64, 5 rt_gen_range as 2, 6 rt_pm1_from_bits.
 * device 0: the host build, no GPU; device 1: one lane per word on GPU 0.  RT1W_ERR_INVALID for anything else, null pointers, n = 0 or,
 * for the range selectors, bounds that are not finite with lo < hi */
int rt1w_lab_f32_draws(int device, int fn, const uint64_t* words, float lo, float hi, uint64_t n, float* out);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
