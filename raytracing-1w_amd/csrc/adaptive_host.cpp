/* adaptive_host.cpp -- the CPU twin of the accumulator kernels (adaptive.hip, guides.hip): rt_adaptive.h, rt_denoise_halves.h and rt_guides.h compiled for the host (g++,
 * -ffp-contract=off like every build of the core).  Diagnostics library only (librt1w_lab.so): the expected side of the GPU tests'
 * bit-equality checks and what the CPU tier's known-answer, plan and quality tests run.  librt1w.so keeps no CPU path. */
#include <cstring>

#include "rt1w.h"
#include "rt_adaptive_plan.h"
#include "rt_denoise_halves.h"
#include "rt_guides.h"
#include "walk_lab.h"

extern "C" int rt1w_lab_accum_merge_host(uint32_t width, uint32_t height, uint32_t x0, uint32_t y0, uint32_t tile_w, uint32_t tile_h, uint32_t batch_spp,
                                         uint32_t flags, const double* tile_sums, const double* aov, double* acc) {
    if (!tile_sums || !aov || !acc || !rt_ad_rect_ok(width, height, x0, y0, tile_w, tile_h, batch_spp, flags)) return RT1W_ERR_INVALID;
    const bool keep = (flags & RT_DN_KEEP_ALBEDO) != 0u;
    for (uint32_t ry = 0; ry < tile_h; ++ry)
        for (uint32_t rx = 0; rx < tile_w; ++rx) {
            const size_t i = (size_t)(y0 + ry) * width + (x0 + rx), t = (size_t)ry * tile_w + rx;
            rt_ad_merge_pixel(batch_spp, keep, tile_sums + t * 3, aov + i * 8, acc + i * RT_AD_RECORD);
        }
    return RT1W_OK;
}

extern "C" int rt1w_lab_accum_merge_tiles_host(uint32_t width, uint32_t height, uint32_t tile, const rt1w_tile* tiles, uint32_t n_tiles, uint32_t batch_spp,
                                               uint32_t flags, const double* tile_sums, const double* aov, double* acc) {
    if (!tile_sums || !aov || !acc || rt_ad_tiles_check(width, height, tile, tiles, n_tiles, batch_spp, flags)) return RT1W_ERR_INVALID;
    const bool keep = (flags & RT_DN_KEEP_ALBEDO) != 0u;
    for (uint32_t k = 0; k < n_tiles; ++k)
        for (uint32_t ly = 0; ly < tile; ++ly)
            for (uint32_t lx = 0; lx < tile; ++lx)
                rt_ad_merge_tiles_pixel(width, height, tile, tiles[k].x0, tiles[k].y0, k, lx, ly, batch_spp, keep, tile_sums, aov, acc);
    return RT1W_OK;
}

extern "C" int rt1w_lab_accum_resolve_host(uint32_t width, uint32_t height, uint32_t batch_spp, const double* acc, double* frame, double* var,
                                           double* spp) {
    if (!acc || !frame || !var || !spp || !rt_ad_frame_ok(width, height) || batch_spp == 0u) return RT1W_ERR_INVALID;
    const size_t n = (size_t)width * height;
    for (size_t i = 0; i < n; ++i) rt_ad_resolve_pixel(batch_spp, acc + i * RT_AD_RECORD, frame + i * 3, var + i, spp + i);
    return RT1W_OK;
}

namespace {
/* the tile sum of the kernel: value(x, y) of every pixel inside the frame, the block tree, the blocks in row-major order */
template <class Value>
void tile_sums(uint32_t width, uint32_t height, uint32_t tile, double* err, Value value) {
    const uint32_t tiles_x = (width + tile - 1u) / tile, tiles_y = (height + tile - 1u) / tile, bw = tile / RT_AD_BLOCK;
    for (uint32_t ty = 0; ty < tiles_y; ++ty)
        for (uint32_t tx = 0; tx < tiles_x; ++tx) {
            const uint32_t px0 = tx * tile, py0 = ty * tile;
            double total = 0.0;
            for (uint32_t by = 0; by < bw && py0 + by * RT_AD_BLOCK < height; ++by)
                for (uint32_t bx = 0; bx < bw && px0 + bx * RT_AD_BLOCK < width; ++bx) {
                    double v[RT_AD_BLOCK * RT_AD_BLOCK];
                    for (uint32_t ly = 0; ly < RT_AD_BLOCK; ++ly)
                        for (uint32_t lx = 0; lx < RT_AD_BLOCK; ++lx) {
                            const uint32_t x = px0 + bx * RT_AD_BLOCK + lx, y = py0 + by * RT_AD_BLOCK + ly;
                            v[ly * RT_AD_BLOCK + lx] = (x < width && y < height) ? value((size_t)y * width + x) : 0.0;
                        }
                    total = total + rt_ad_block_tree(v);
                }
            err[(size_t)ty * tiles_x + tx] = total / (double)rt_ad_tile_pixels(width, height, tile, tx, ty);
        }
}
} // namespace

extern "C" int rt1w_lab_tile_error_host(uint32_t width, uint32_t height, uint32_t tile, const double* acc, double* err) {
    if (!acc || !err || !rt_ad_frame_ok(width, height) || !rt_ad_tile_ok(tile)) return RT1W_ERR_INVALID;
    tile_sums(width, height, tile, err, [&](size_t i) { return rt_ad_pixel_error(acc + i * RT_AD_RECORD); });
    return RT1W_OK;
}

extern "C" int rt1w_lab_tile_error_map_host(uint32_t width, uint32_t height, uint32_t tile, const double* err_px, double* err) {
    if (!err_px || !err || !rt_ad_frame_ok(width, height) || !rt_ad_tile_ok(tile)) return RT1W_ERR_INVALID;
    tile_sums(width, height, tile, err, [&](size_t i) { return rt_dh_map_value(err_px[i]); });
    return RT1W_OK;
}

extern "C" int rt1w_lab_halves_resolve_host(uint32_t width, uint32_t height, uint32_t batch_spp, const double* acc_a, const double* acc_b, double* frame,
                                            double* var, double* half_a, double* half_b, double* spp) {
    if (!acc_a || !acc_b || !frame || !var || !half_a || !half_b || !spp || !rt_ad_frame_ok(width, height) || batch_spp == 0u) return RT1W_ERR_INVALID;
    const size_t n = (size_t)width * height;
    for (size_t i = 0; i < n; ++i)
        rt_dh_resolve_pixel(batch_spp, acc_a + i * RT_AD_RECORD, acc_b + i * RT_AD_RECORD, frame + i * 3, var + i, half_a + i * 3, half_b + i * 3, spp + i);
    return RT1W_OK;
}

extern "C" int rt1w_lab_guides_merge_tiles_host(uint32_t width, uint32_t height, uint32_t tile, const rt1w_tile* tiles, uint32_t n_tiles, uint32_t spp,
                                                const double* tile_sums, double* gacc) {
    if (!tile_sums || !gacc || rt_gd_tiles_check(width, height, tile, tiles, n_tiles, spp)) return RT1W_ERR_INVALID;
    for (uint32_t k = 0; k < n_tiles; ++k)
        for (uint32_t ly = 0; ly < tile; ++ly)
            for (uint32_t lx = 0; lx < tile; ++lx) rt_gd_merge_tiles_pixel(width, height, tile, tiles[k].x0, tiles[k].y0, k, lx, ly, spp, tile_sums, gacc);
    return RT1W_OK;
}

extern "C" int rt1w_lab_guides_resolve_host(uint32_t width, uint32_t height, const double* gacc, double* aov) {
    if (!gacc || !aov || !rt_ad_frame_ok(width, height)) return RT1W_ERR_INVALID;
    const size_t n = (size_t)width * height;
    for (size_t i = 0; i < n; ++i) rt_gd_resolve_pixel(gacc + i * RT_GD_RECORD, aov + i * RT_GD_SUMS);
    return RT1W_OK;
}
