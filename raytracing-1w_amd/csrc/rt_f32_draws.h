/* rt_f32_draws.h -- DIAGNOSTICS: the draw layer of the single-precision builds (include/rt1w_num.h under RT_F32) on a given 64-bit word.
 *
 * Include it inside the namespace that holds an RT_F32 build of rt1w_num.h, with `double` defined to float as that build had it
 * (f32_exact.hip: host and device; oracle/oracle_flat_f32.cpp: the CPU twin).  Every selector returns what a caller of the f32 core
 * holds after assigning the draw to its `double`:
 *   0  rt_f64_from_bits(w)                                  the unit draw
 *   1  rt_range_from_bits(w, lo, hi)                        the range draw, one take, no retry: a value the retry would reject shows
 *   2  rt_take_range(r, lo, hi)                             over a stream that holds w and then the word 0 (whose draw is `lo`):
 *                                                           the single take where the retry accepts it, `lo` where it rejects
 *   3  rt_take_f64(r), 4 rt_gen_f64(r)                      the unit draw's two other spellings, over the same stream
 *   5  rt_gen_range(r, lo, hi)                              as 2, the checked spelling
 *   6  rt_pm1_from_bits(w)                                  the samplers' gen_range(-1.0..1.0) (no retry; lo and hi unused) */
#ifndef RT_F32_DRAWS_H
#define RT_F32_DRAWS_H

#define RT_F32_DRAW_FNS 7

/* a stream whose next 64-bit draw is w and whose draw after that is the word 0: both blocks are in the buffer, nothing is generated */
RT_HD RtRng rt_f32_draw_stream(uint64_t w) {
    RtRng r = rt_rng_make(0u, 0u, 0u, 0u, 0u);
    r.left = 2u; r.a0 = (uint32_t)w; r.a1 = (uint32_t)(w >> 32);
    r.bv = 1u; r.blk = 2u;
    return r;
}
RT_HD float rt_f32_draw(int fn, uint64_t w, float lo, float hi) {
    RtRng r = rt_f32_draw_stream(w);
    double x;
    switch (fn) {
        case 0: x = rt_f64_from_bits(w); break;
        case 1: x = rt_range_from_bits(w, lo, hi); break;
        case 2: x = rt_take_range(r, lo, hi); break;
        case 3: x = rt_take_f64(r); break;
        case 4: x = rt_gen_f64(r); break;
        case 5: x = rt_gen_range(r, lo, hi); break;
        default: x = rt_pm1_from_bits(w); break;
    }
    return x;
}

#endif
