/* rt_feature_launch.h -- what features.hip calls in the kernel units aov.hip, aov_tiles.hip, guides.hip, denoise.hip, denoise_var.hip, denoise_halves.hip, denoise_cross.hip, adaptive.hip, temporal.hip, temporal_var.hip, hit.hip and path_step.hip, declared once.
 * The functions are extern "C": nothing in their names says what they take, so caller and definition both include this header and the
 * compiler holds each definition to the declaration the caller sees.  Private (librt1w.map exports none of them).
 * Every kernel is reached through a typed *_launch: no kernel handle leaves its unit, and no argument array is built by hand.  The
 * *_launch functions enqueue on `stream`, put grid and block of the launch (of the level kernel, for the filters) into launch[0..1]
 * and return 0, -1 launch failure, -2 parameters refused.  What a unit's kernels take by value in a layout of the caller's (the AOV
 * kernels' view and frame, the temporal kernel's cameras) is passed by address and copied into the unit's own type; the *_sizeof
 * functions let the caller check that the two layouts have one size. */
#ifndef RT1W_FEATURE_LAUNCH_H
#define RT1W_FEATURE_LAUNCH_H

#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {
/* aov.hip: the first-hit feature buffers (rt1w_render_aov) and the deep ones (rt1w_render_aov_deep: + max_specular, max_fuzz and a counter
 * in device memory, zeroed by the caller, that receives the rays traced), by the kernel of `variant` over the tile of `frame`.  `view` and
 * `frame` by address: the bytes of an RtSceneView and an RtFrame, rt1w_internal_aov_sizeof(0) and (1) of them, copied into the kernel's
 * arguments */
int rt1w_internal_aov_launch(const void* view, const void* frame, int variant, double* out, hipStream_t stream, unsigned launch[2]);
int rt1w_internal_aov_deep_launch(const void* view, const void* frame, int variant, uint32_t max_specular, double max_fuzz, double* out,
                                  unsigned long long* segments, hipStream_t stream, unsigned launch[2]);
unsigned rt1w_internal_aov_sizeof(int what);
/* denoise.hip: the filter of rt1w_denoise; enqueues the prepare pass and the levels */
int rt1w_internal_denoise_launch(uint32_t w, uint32_t h, uint32_t iterations, uint32_t flags, double sigma_colour, double sigma_normal,
                                 double sigma_depth, const double* frame, const double* aov, double* out, void* col_a, void* col_b, void* guide,
                                 hipStream_t stream, unsigned launch[2]);
unsigned rt1w_internal_denoise_sizeof(int what); /* bytes per pixel of 0 a colour buffer, 1 the guide buffer */
/* denoise_var.hip: the batch-variance pass and the variance-guided filter */
int rt1w_internal_batch_variance_launch(uint32_t w, uint32_t h, uint32_t batches, uint32_t batch_spp, uint32_t flags, const double* sums,
                                        const double* aov, double* frame, double* var, hipStream_t stream, unsigned launch[2]);
int rt1w_internal_denoise_var_launch(uint32_t w, uint32_t h, uint32_t iterations, uint32_t flags, double sigma_normal, double sigma_depth,
                                     double sigma_variance, const double* frame, const double* aov, const double* var, double* out, void* col_a,
                                     void* col_b, void* guide, hipStream_t stream, unsigned launch[2]);
unsigned rt1w_internal_denoise_var_sizeof(void); /* bytes per pixel of one of its colour buffers */
/* adaptive.hip: the accumulator kernels */
int rt1w_internal_accum_merge_launch(uint32_t w, uint32_t h, uint32_t x0, uint32_t y0, uint32_t tw, uint32_t th, uint32_t batch_spp, uint32_t flags,
                                     const double* sums, const double* aov, double* acc, hipStream_t stream, unsigned launch[2]);
int rt1w_internal_accum_merge_tiles_launch(uint32_t w, uint32_t h, uint32_t tile, const uint32_t* rec, uint32_t n, uint32_t batch_spp, uint32_t flags,
                                           const double* sums, const double* aov, double* acc, hipStream_t stream, unsigned launch[2]);
int rt1w_internal_accum_resolve_launch(uint32_t w, uint32_t h, uint32_t batch_spp, const double* acc, double* frame, double* var, double* spp,
                                       hipStream_t stream, unsigned launch[2]);
int rt1w_internal_accum_tile_error_launch(uint32_t w, uint32_t h, uint32_t tile, const double* acc, double* err, hipStream_t stream,
                                          unsigned launch[2]);
/* adaptive.hip: two accumulators as the halves of one frame, and the tile error's sum over a per-pixel map */
int rt1w_internal_halves_resolve_launch(uint32_t w, uint32_t h, uint32_t batch_spp, const double* acc_a, const double* acc_b, double* frame,
                                        double* var, double* half_a, double* half_b, double* spp, hipStream_t stream, unsigned launch[2]);
int rt1w_internal_tile_error_map_launch(uint32_t w, uint32_t h, uint32_t tile, const double* err_px, double* err, hipStream_t stream,
                                        unsigned launch[2]);
/* denoise_halves.hip: the variance-guided filter carrying the two halves; out and err_px of the last level */
int rt1w_internal_denoise_var_halves_launch(uint32_t w, uint32_t h, uint32_t iterations, uint32_t flags, double sigma_normal, double sigma_depth,
                                            double sigma_variance, const double* frame, const double* aov, const double* var, const double* half_a,
                                            const double* half_b, double* out, double* err_px, void* col_a, void* col_b, void* guide,
                                            hipStream_t stream, unsigned launch[2]);
unsigned rt1w_internal_denoise_var_halves_sizeof(void); /* bytes per pixel of one of its colour buffers */
/* denoise_cross.hip: the two halves, each filtered with the other's colour term; out and err_px of the last level */
int rt1w_internal_denoise_cross_launch(uint32_t w, uint32_t h, uint32_t iterations, uint32_t flags, double sigma_normal, double sigma_depth,
                                       double sigma_variance, const double* frame, const double* aov, const double* var, const double* half_a,
                                       const double* half_b, double* out, double* err_px, void* col_a, void* col_b, void* guide,
                                       hipStream_t stream, unsigned launch[2]);
unsigned rt1w_internal_denoise_cross_sizeof(void); /* bytes per pixel of one of its colour buffers */
/* aov_tiles.hip: the first-hit feature sums of a list of tiles (rt1w_render_aov_tiles), by the kernel of `variant`; view and frame as for
 * aov.hip, rt1w_internal_aov_tiles_sizeof(0) and (1) bytes; rec the uploaded list */
int rt1w_internal_aov_tiles_launch(const void* view, const void* frame, int variant, uint32_t tile, const uint32_t* rec, uint32_t n, double* out,
                                   hipStream_t stream, unsigned launch[2]);
unsigned rt1w_internal_aov_tiles_sizeof(int what);
/* guides.hip: the guide accumulator (rt1w_guides_merge_tiles, rt1w_guides_resolve) */
int rt1w_internal_guides_merge_tiles_launch(uint32_t w, uint32_t h, uint32_t tile, const uint32_t* rec, uint32_t n, uint32_t spp, const double* sums,
                                            double* gacc, hipStream_t stream, unsigned launch[2]);
int rt1w_internal_guides_resolve_launch(uint32_t w, uint32_t h, const double* gacc, double* aov, hipStream_t stream, unsigned launch[2]);
/* temporal.hip: the reprojection and accumulation of rt1w_temporal_accumulate, one launch; the two cameras by address, each
 * rt1w_internal_temporal_sizeof() bytes in the layout of rt1w_camera, copied into the kernel's arguments */
int rt1w_internal_temporal_launch(uint32_t w, uint32_t h, uint32_t flags, uint32_t max_history, double depth_tol, double normal_min,
                                  const double* cur_frame, const double* cur_aov, const void* cur_cam, const double* prev_hist, const double* prev_len,
                                  const double* prev_aov, const void* prev_cam, double* hist, double* len, double* frame_out, hipStream_t stream,
                                  unsigned launch[2]);
unsigned rt1w_internal_temporal_sizeof(void);
/* temporal_var.hip: that launch with the second-moment channel beside the history (rt1w_temporal_moments), and the pass that turns
 * history, second moment and length into the variance buffer of rt1w_denoise_var (rt1w_temporal_variance); the cameras as above,
 * rt1w_internal_temporal_var_sizeof() bytes each */
int rt1w_internal_temporal_moments_launch(uint32_t w, uint32_t h, uint32_t flags, uint32_t max_history, double depth_tol, double normal_min,
                                          const double* cur_frame, const double* cur_aov, const void* cur_cam, const double* prev_hist,
                                          const double* prev_m2, const double* prev_len, const double* prev_aov, const void* prev_cam, double* hist,
                                          double* m2, double* len, double* frame_out, hipStream_t stream, unsigned launch[2]);
int rt1w_internal_temporal_variance_launch(uint32_t w, uint32_t h, const double* hist, const double* m2, const double* len, const double* aov,
                                           double* var, hipStream_t stream, unsigned launch[2]);
unsigned rt1w_internal_temporal_var_sizeof(void);
/* hit.hip: the ray queries (rt1w_hit): the kernel of `variant` over the params->n rays of `rays` into out (and out_node unless null), all device
 * memory.  `view` and `params` by address: the bytes of an RtSceneView and an rt1w_hit_params, rt1w_internal_hit_sizeof(0) and (1) of
 * them, copied into the kernel's arguments; rt1w_internal_hit_sizeof(2): 1 if the unit was built with the staged ray I/O */
int rt1w_internal_hit_launch(const void* view, const void* params, int variant, const double* rays, double* out, uint32_t* out_node,
                             hipStream_t stream, unsigned launch[2]);
unsigned rt1w_internal_hit_sizeof(int what);
/* path_step.hip: the path states (rt1w_path_step, rt1w_path_begin).  The step kernel of `variant` over the params->n states of `in` into `out`
 * (the same buffer or apart; out_node unless null), all device memory, the states 16-byte aligned; `view` and `params` by address: the bytes
 * of an RtSceneView and an rt1w_path_params, rt1w_internal_path_sizeof(0) and (1) of them; *segments, zeroed by the caller, receives the
 * levels that traced a ray.  The begin kernel over n entries {i, j, sample} with the camera of `view`; *outside, zeroed by the caller,
 * receives the entries whose pixel is outside the frame.  rt1w_internal_path_sizeof(2): bytes of a state, (3): waves per SIMD of the build */
int rt1w_internal_path_step_launch(const void* view, const void* params, int variant, const void* in, void* out, uint32_t* out_node,
                                   unsigned long long* segments, hipStream_t stream, unsigned launch[2]);
int rt1w_internal_path_begin_launch(const void* view, uint32_t width, uint32_t height, uint32_t global_seed, uint32_t max_depth, const uint32_t* pixels,
                                    uint64_t n, void* out, unsigned long long* outside, hipStream_t stream, unsigned launch[2]);
unsigned rt1w_internal_path_sizeof(int what);
}

#endif
