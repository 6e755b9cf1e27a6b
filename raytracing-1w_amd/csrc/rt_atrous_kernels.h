/* rt_atrous_kernels.h -- the one skeleton of the four a-trous filter units (denoise.hip, denoise_var.hip, denoise_halves.hip,
 * denoise_cross.hip): the staged tile, the bodies of the prepare and the level kernel, and the enqueue loop.  A unit
 * includes it inside its own namespace, after its rt_denoise*.h (<hip/hip_runtime.h> and <stdint.h> before the namespace), and adds the
 * named __global__ shells over the bodies and its extern "C" launcher: the four code objects stay separate.
 *
 * What a filter is comes from its policy F in rt_denoise*.h (RtDnFilter, RtDvFilter, RtDhFilter, RtDcFilter; denoise_host.cpp runs the
 * CPU twin over the same four): F::Col, the colour record, sizeof(Col) / 8 doubles; F::prepare, F::level, F::finish over the per-pixel
 * functions of that header.
 *
 * Work mapping: that of rt_pixel_kernels.h, workgroups in row order over the image -- one lane per pixel, an 8 x 8 pixel block per wave,
 * 2 x 2 blocks (16 x 16 pixels) per workgroup of 256 lanes.  Every output
 * pixel is computed whole by one lane in the fixed tap order of the filter's level_pixel: no atomics, the same bits as the twin.  The
 * prepare pass turns the caller's buffers into what the levels read: a colour record and the 64-byte guide record (RtDnGuide), both f64.
 * A level reads the colour records of the previous one and writes its own (two buffers, ping-pong); the last level writes the caller's
 * buffers through F::finish.
 *
 * Two forms of the level kernel.  Staged (STEP 1 and 2, the levels of those steps): the workgroup copies its tile plus the 2-step halo,
 * T^2 = (16 + 4 step)^2 pixels, into LDS as struct-of-arrays -- planes 0 .. NC-1 the colour record in its field order, NC .. NC+4 the
 * guide's normal, depth and coverage; (NC + 5) T^2 doubles -- then every tap is an LDS read.  Direct (STEP 0, any level): the 25 taps of a
 * wave are 25 8 x 8 blocks, read from memory through L2.  Which of levels 0 and 1 run staged is the launcher's mask, bit = level
 * (DESIGN.md sections 13, 17, 18 have the measurements behind the units' defaults). */
#include "rt_pixel_kernels.h" /* the work mapping (rt_px_lane_pixel), its grid, RT_PX_WG, RT_PX_BLOCK */

/* the body of a prepare kernel; in: the caller's buffers as F::prepare takes them */
template <class F, class... In>
__device__ __forceinline__ void rt_at_prepare(const RtDnParams& P, typename F::Col* col, RtDnGuide* guide, In... in) {
    uint32_t tx, ty, x, y;
    rt_px_lane_pixel(P.w, tx, ty, x, y);
    if (x >= P.w || y >= P.h) return;
    const unsigned long long i = (unsigned long long)y * P.w + x;
    typename F::Col c;
    RtDnGuide g;
    F::prepare(P, i, c, g, in...);
    col[i] = c;
    guide[i] = g;
}

/* the staged tile: NC + 5 planes of T x T doubles, origin (ox, oy) in the image; only pixels inside the image are filled and only those are read */
template <class Col, int T>
struct RtAtLdsSrc {
    static constexpr int NC = (int)(sizeof(Col) / 8);
    const double* t;
    long long ox, oy;
    __device__ __forceinline__ int at(uint32_t x, uint32_t y) const { return (int)((long long)y - oy) * T + (int)((long long)x - ox); }
    __device__ __forceinline__ Col col(uint32_t x, uint32_t y) const {
        const int i = at(x, y);
        double v[NC];
#pragma unroll
        for (int k = 0; k < NC; ++k) v[k] = t[k * T * T + i];
        Col c;
        __builtin_memcpy(&c, v, sizeof c);
        return c;
    }
    __device__ __forceinline__ void guide(uint32_t x, uint32_t y, double o[5]) const {
        const int i = at(x, y);
        for (int k = 0; k < 5; ++k) o[k] = t[(NC + k) * T * T + i];
    }
};

/* the body of a level kernel.  STEP 0: direct form, any level.  STEP 1, 2: staged form of the level whose step it is.  out != nullptr: the
 * last level.  Every lane of the workgroup reaches the barrier: a lane outside the image fills its share of the halo and returns after it */
template <class F, int STEP>
__device__ __forceinline__ void rt_at_level(const RtDnParams& P, double sv2, uint32_t level, const typename F::Col* src, const RtDnGuide* guide,
                                            typename F::Col* dst, double* out, double* err_px) {
    typedef typename F::Col Col;
    uint32_t tx, ty, x, y;
    rt_px_lane_pixel(P.w, tx, ty, x, y);
    const bool inside = x < P.w && y < P.h;
    Col c;
    if constexpr (STEP > 0) {
        constexpr int T = (int)RT_PX_BLOCK + 4 * STEP, NC = (int)(sizeof(Col) / 8);
        __shared__ double tile[(NC + 5) * T * T];
        const long long ox = (long long)tx * RT_PX_BLOCK - 2 * STEP, oy = (long long)ty * RT_PX_BLOCK - 2 * STEP;
        for (int i = (int)threadIdx.x; i < T * T; i += RT_PX_WG) {
            const long long gx = ox + i % T, gy = oy + i / T;
            if (gx < 0 || gy < 0 || gx >= (long long)P.w || gy >= (long long)P.h) continue;
            const unsigned long long q = (unsigned long long)gy * P.w + (unsigned long long)gx;
            const Col cq = src[q];
            const RtDnGuide* gq = guide + q;
            double v[NC];
            __builtin_memcpy(v, &cq, sizeof cq);
#pragma unroll
            for (int k = 0; k < NC; ++k) tile[k * T * T + i] = v[k];
            tile[NC * T * T + i] = gq->nx; tile[(NC + 1) * T * T + i] = gq->ny; tile[(NC + 2) * T * T + i] = gq->nz;
            tile[(NC + 3) * T * T + i] = gq->z; tile[(NC + 4) * T * T + i] = gq->v;
        }
        __syncthreads();
        if (!inside) return;
        const RtAtLdsSrc<Col, T> s{tile, ox, oy};
        c = F::level(P, sv2, s, x, y, level);
    } else {
        if (!inside) return;
        const RtDnGlobalSrc<Col> s{src, guide, P.w};
        c = F::level(P, sv2, s, x, y, level);
    }
    const unsigned long long i = (unsigned long long)y * P.w + x;
    if (out) F::finish(c, guide[i], i, out, err_px);
    else dst[i] = c;
}

/* what a launcher ends in.  Enqueues the prepare pass and the levels, one after another: prepare(grid, block, col_a); then per level
 * level(step, grid, block, level, src, dst, last), step = the STEP of the kernel to launch (staged: bits 0 and 1 of `staged`, bit = level),
 * src / dst the ping-pong of col_a / col_b (w * h records of Col each), last: this level writes the caller's buffers.  launch[0..1] =
 * grid, block of the level kernel.  0 or -1 (launch failure) */
template <class Col, class Prepare, class Level>
__host__ int rt_at_enqueue(const RtDnParams& P, unsigned staged, void* col_a, void* col_b, unsigned launch[2], Prepare prepare, Level level_launch) {
    const dim3 grid(rt_px_frame_grid(P.w, P.h)), block(RT_PX_WG);
    launch[0] = grid.x; launch[1] = RT_PX_WG;
    Col* src = (Col*)col_a;
    Col* dst = (Col*)col_b;
    prepare(grid, block, src);
    for (uint32_t level = 0; level < P.levels; ++level) {
        const int step = (level < 2u && ((staged >> level) & 1u)) ? (int)level + 1 : 0;
        level_launch(step, grid, block, level, (const Col*)src, dst, level + 1u == P.levels);
        Col* t = src; src = dst; dst = t;
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
