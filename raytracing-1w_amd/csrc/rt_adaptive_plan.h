/* rt_adaptive_plan.h -- the plan of adaptive sampling (include/rt1w.h: rt1w_adaptive_params, rt1w_adaptive_select,
 * rt1w_render_adaptive): the parameters with their defaults, one round's choice of tiles, and the grouping of the chosen tiles into
 * rectangles.  Host code; rt1w_render_adaptive and rt1w_adaptive_select (features.hip) both run exactly this, so a host that composes
 * the public entries itself makes the one call's choices. */
#ifndef RT_ADAPTIVE_PLAN_H
#define RT_ADAPTIVE_PLAN_H

#include <algorithm>
#include <vector>

#include "rt1w.h"
#include "rt_adaptive.h"

/* the defaults, chosen with the CPU twins on the three scenes of tests/test_adaptive.py */
#define RT_AD_DEFAULT_TILE 16u
#define RT_AD_DEFAULT_BATCH_DIV 8u /* batch_spp = max(1, budget_spp / 8): with 4 pilot batches the pilot is half of the budget at any budget */
#define RT_AD_DEFAULT_PILOT 4u
#define RT_AD_DEFAULT_BUDGET 64u
#define RT_AD_DEFAULT_MAX_FACTOR 8u /* max_spp = 8 x budget_spp */
#define RT_AD_DEFAULT_ROUND_SHARE 0.25

/* rt1w_adaptive_params with the defaults filled in */
struct RtAdPlan {
    uint32_t tile, batch_spp, pilot, budget_spp, max_spp, flags; /* flags: how the merges demodulate (RT1W_DENOISE_KEEP_ALBEDO or 0) */
    bool one_launch;                                             /* RT1W_ADAPTIVE_ONE_LAUNCH */
    double target_error, round_share;
};

/* nullptr: accepted, *out filled; else why not (RT1W_ERR_INVALID) */
inline const char* rt_ad_make_plan(const rt1w_adaptive_params* a, RtAdPlan* out) {
    if (!a) return "adaptive: null parameters";
    if (a->size != (uint32_t)sizeof(rt1w_adaptive_params)) return "adaptive: rt1w_adaptive_params.size is not this library's sizeof(rt1w_adaptive_params)";
    RtAdPlan p;
    p.tile = a->tile ? a->tile : RT_AD_DEFAULT_TILE;
    p.budget_spp = a->budget_spp ? a->budget_spp : RT_AD_DEFAULT_BUDGET;
    p.batch_spp = a->batch_spp ? a->batch_spp : std::max(1u, p.budget_spp / RT_AD_DEFAULT_BATCH_DIV);
    p.pilot = a->pilot_batches ? a->pilot_batches : RT_AD_DEFAULT_PILOT;
    p.flags = a->flags;
    p.target_error = a->target_error;
    p.round_share = a->round_share == 0.0 ? RT_AD_DEFAULT_ROUND_SHARE : a->round_share;
    if (!rt_ad_tile_ok(p.tile)) return "adaptive: tile must be a multiple of 16 in 16 .. 256";
    if (p.pilot < 2u || p.pilot > 16u) return "adaptive: pilot_batches must be 2 .. 16";
    const unsigned long long pilot_spp = (unsigned long long)p.pilot * p.batch_spp;
    const unsigned long long mx = a->max_spp ? a->max_spp : std::min<unsigned long long>((unsigned long long)p.budget_spp * RT_AD_DEFAULT_MAX_FACTOR, 0xFFFFFFFFull);
    if (pilot_spp > 0xFFFFFFFFull || mx < pilot_spp) return "adaptive: max_spp is less than the pilot's pilot_batches * batch_spp samples";
    if (p.budget_spp < pilot_spp) return "adaptive: budget_spp is less than the pilot's pilot_batches * batch_spp samples";
    p.max_spp = (uint32_t)mx;
    if (!(p.target_error >= 0.0) || !rt_dn_finite(p.target_error)) return "adaptive: target_error must be finite and >= 0";
    if (!(p.round_share > 0.0) || !(p.round_share <= 1.0)) return "adaptive: round_share must be in (0, 1] (0 = default)";
    if (p.flags & ~(RT1W_DENOISE_KEEP_ALBEDO | RT1W_ADAPTIVE_ONE_LAUNCH)) return "adaptive: unknown flag (flags: RT1W_DENOISE_KEEP_ALBEDO, RT1W_ADAPTIVE_ONE_LAUNCH)";
    p.one_launch = (p.flags & RT1W_ADAPTIVE_ONE_LAUNCH) != 0u;
    p.flags &= ~RT1W_ADAPTIVE_ONE_LAUNCH;
    *out = p;
    return nullptr;
}

/* The plan of rt1w_render_adaptive_filtered, whose unit is a PAIR of batches, one for each half: *out the plan as given (its pilot even:
 * pilot / 2 pairs), *pair what one round's choice runs on -- the same plan with batch_spp = 2 n, exactly what rt1w_adaptive_select makes
 * of the parameters with batch_spp = 2 n and pilot_batches = max(2, pilot / 2), so that a host composing the public entries makes the one
 * call's choices.  nullptr, or why not (RT1W_ERR_INVALID) */
inline const char* rt_ad_make_pair_plan(const rt1w_adaptive_params* a, RtAdPlan* out, RtAdPlan* pair) {
    if (const char* why = rt_ad_make_plan(a, out)) return why;
    if (out->pilot % 2u) return "adaptive (filtered error): pilot_batches must be even (a pixel receives its batches in pairs, one for each half)";
    if (out->batch_spp > 0x7FFFFFFFu) return "adaptive (filtered error): batch_spp must be below 2^31 (a pair is 2 batch_spp samples)";
    rt1w_adaptive_params b = *a;
    b.tile = out->tile; b.budget_spp = out->budget_spp; b.max_spp = out->max_spp;
    b.batch_spp = 2u * out->batch_spp;
    b.pilot_batches = std::max(2u, out->pilot / 2u);
    return rt_ad_make_plan(&b, pair);
}

/* the records of a tile list: 0 accepted, 1 a record off the grid, outside the frame or with a non-zero reserved member, 2 (disjoint
 * lists only) a tile named twice */
inline int rt_ad_tile_records_check(uint32_t w, uint32_t h, uint32_t tile, const rt1w_tile* tiles, uint32_t n, bool disjoint) {
    const uint32_t tiles_x = (w + tile - 1u) / tile, tiles_y = (h + tile - 1u) / tile;
    std::vector<bool> seen(disjoint ? (size_t)tiles_x * tiles_y : 0u, false);
    for (uint32_t k = 0; k < n; ++k) {
        const rt1w_tile& t = tiles[k];
        if (t.reserved != 0u || t.x0 % tile || t.y0 % tile || t.x0 >= w || t.y0 >= h) return 1;
        if (!disjoint) continue;
        const size_t id = (size_t)(t.y0 / tile) * tiles_x + t.x0 / tile;
        if (seen[id]) return 2;
        seen[id] = true;
    }
    return 0;
}

/* pixels of a list's tiles that lie inside the frame (the records checked: rt_ad_tile_records_check).  Each tile's rt_ad_tile_pixels, clipped
 * with two comparisons instead of that function's divisions: lists run to 2^20 tiles */
inline unsigned long long rt_ad_list_pixels(uint32_t w, uint32_t h, uint32_t tile, const rt1w_tile* tiles, uint32_t n) {
    unsigned long long inside = 0ull;
    for (uint32_t k = 0; k < n; ++k) inside += (unsigned long long)std::min(tile, w - tiles[k].x0) * std::min(tile, h - tiles[k].y0);
    return inside;
}

/* the list of rt1w_accum_merge_tiles: nullptr, or why it is refused (RT1W_ERR_INVALID) */
inline const char* rt_ad_tiles_check(uint32_t w, uint32_t h, uint32_t tile, const rt1w_tile* tiles, uint32_t n, uint32_t batch_spp, uint32_t flags) {
    if (!rt_ad_frame_ok(w, h)) return "accumulator: width and height must be 1 .. 2^30";
    if (!rt_ad_tile_ok(tile)) return "accumulator merge: tile must be a multiple of 16 in 16 .. 256";
    if (batch_spp < 1u || (flags & ~RT1W_DENOISE_KEEP_ALBEDO)) return "accumulator merge: batch_spp >= 1, flags 0 or RT1W_DENOISE_KEEP_ALBEDO";
    if (!tiles || n < 1u || n > RT_AD_TILES_MAX) return "accumulator merge: a list of 1 .. 2^20 tiles";
    switch (rt_ad_tile_records_check(w, h, tile, tiles, n, true)) {
        case 1: return "accumulator merge: a tile's x0 and y0 must be multiples of `tile` inside the frame, its reserved member 0";
        case 2: return "accumulator merge: a tile is named twice (the tiles of one call are disjoint)";
    }
    return nullptr;
}

/* the list of rt1w_guides_merge_tiles: nullptr, or why it is refused (RT1W_ERR_INVALID) */
inline const char* rt_gd_tiles_check(uint32_t w, uint32_t h, uint32_t tile, const rt1w_tile* tiles, uint32_t n, uint32_t spp) {
    if (!rt_ad_frame_ok(w, h)) return "guides: width and height must be 1 .. 2^30";
    if (!rt_ad_tile_ok(tile)) return "guides merge: tile must be a multiple of 16 in 16 .. 256";
    if (spp < 1u) return "guides merge: spp must be >= 1";
    if (!tiles || n < 1u || n > RT_AD_TILES_MAX) return "guides merge: a list of 1 .. 2^20 tiles";
    switch (rt_ad_tile_records_check(w, h, tile, tiles, n, true)) {
        case 1: return "guides merge: a tile's x0 and y0 must be multiples of `tile` inside the frame, its reserved member 0";
        case 2: return "guides merge: a tile is named twice (the tiles of one call are disjoint)";
    }
    return nullptr;
}

/* what rt1w_render_aov_tiles refuses in its parameters and its list, in the order its callers know: RT1W_OK, or the code with *why set.
 * A tile may be named more than once (with other offsets) */
inline int rt_aov_tiles_check(const rt1w_render_params* p, uint32_t tile, const rt1w_tile* tiles, uint32_t n, const char** why) {
    const auto refuse = [why](int rc, const char* text) { *why = text; return rc; };
    if (p->width < 2 || p->height < 2) return refuse(RT1W_ERR_INVALID, "width and height must be >= 2 (u,v divide by W-1, H-1; main.rs:968-969)");
    if (p->spp == 0) return refuse(RT1W_ERR_INVALID, "spp must be > 0");
    if (p->flags & ~(0xFFu << 8)) return refuse(RT1W_ERR_INVALID, "rt1w_render_aov_tiles: flags 0 or RT1W_FORCE_VARIANT only");
    if (p->precision == RT1W_PRECISION_F32) return refuse(RT1W_ERR_UNSUPPORTED, "rt1w_render_aov_tiles: the AOV entries are f64 only (RT1W_PRECISION_F64)");
    if (p->precision != RT1W_PRECISION_F64) return refuse(RT1W_ERR_UNSUPPORTED, "unknown precision");
    if (p->strip_rows || p->strip_period) return refuse(RT1W_ERR_INVALID, "rt1w_render_aov_tiles takes no interleaved strips");
    if (!rt_ad_tile_ok(tile)) return refuse(RT1W_ERR_INVALID, "rt1w_render_aov_tiles: tile must be a multiple of 16 in 16 .. 256");
    if (n < 1u || n > RT_AD_TILES_MAX) return refuse(RT1W_ERR_INVALID, "rt1w_render_aov_tiles: n_tiles must be 1 .. 2^20");
    if (rt_ad_tile_records_check(p->width, p->height, tile, tiles, n, false))
        return refuse(RT1W_ERR_INVALID, "rt1w_render_aov_tiles: a tile's x0 and y0 must be multiples of `tile` inside the frame, its reserved member 0");
    for (uint32_t k = 0; k < n; ++k)
        if ((unsigned long long)p->sample_offset + tiles[k].sample_offset + p->spp > 0xFFFFFFFFull) return refuse(RT1W_ERR_INVALID, "sample index overflow");
    return RT1W_OK;
}

/* One round.  err and m by tile, row-major over tiles_x x tiles_y tiles of a w x h frame; the tiles taken, in the order taken */
inline std::vector<uint32_t> rt_ad_select(const RtAdPlan& p, uint32_t tiles_x, uint32_t tiles_y, uint32_t w, uint32_t h, const double* err,
                                          const uint32_t* m) {
    const uint32_t n = tiles_x * tiles_y;
    const double frame_px = (double)w * (double)h;
    const double budget = (double)p.budget_spp * frame_px, share = p.round_share * frame_px;
    double spent = 0.0; /* pixel-samples so far: whole numbers below 2^53, exact */
    for (uint32_t t = 0; t < n; ++t) spent += (double)m[t] * (double)p.batch_spp * (double)rt_ad_tile_pixels(w, h, p.tile, t % tiles_x, t / tiles_x);
    std::vector<uint32_t> cand;
    for (uint32_t t = 0; t < n; ++t)
        if (err[t] > p.target_error && ((unsigned long long)m[t] + 1u) * p.batch_spp <= p.max_spp) cand.push_back(t);
    std::stable_sort(cand.begin(), cand.end(), [&](uint32_t a, uint32_t b) { return err[a] > err[b]; }); /* ties: tile index ascending */
    std::vector<uint32_t> taken;
    double round_px = 0.0;
    for (uint32_t t : cand) {
        const double px = (double)rt_ad_tile_pixels(w, h, p.tile, t % tiles_x, t / tiles_x);
        if (!taken.empty() && round_px + px > share) break;
        if (spent + px * (double)p.batch_spp > budget) break;
        taken.push_back(t);
        round_px += px;
        spent += px * (double)p.batch_spp;
    }
    return taken;
}

/* a run of taken tiles that are adjacent in one tile row and have equal m: rendered as one rectangle, merged by one rt1w_accum_merge */
struct RtAdRun { uint32_t x0, y0, w, h, m; };
inline std::vector<RtAdRun> rt_ad_group(const RtAdPlan& p, uint32_t tiles_x, uint32_t w, uint32_t h, std::vector<uint32_t> taken, const uint32_t* m) {
    std::sort(taken.begin(), taken.end());
    std::vector<RtAdRun> runs;
    uint32_t prev = 0;
    for (size_t i = 0; i < taken.size(); ++i) {
        const uint32_t t = taken[i], tx = t % tiles_x, ty = t / tiles_x;
        const uint32_t x0 = tx * p.tile, y0 = ty * p.tile;
        const uint32_t tw = std::min(p.tile, w - x0), th = std::min(p.tile, h - y0);
        if (i > 0 && t == prev + 1u && tx != 0u && m[t] == runs.back().m) runs.back().w += tw;
        else runs.push_back(RtAdRun{x0, y0, tw, th, m[t]});
        prev = t;
    }
    return runs;
}

#endif
