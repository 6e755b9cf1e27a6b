/* rt_pixel_kernels.h -- the one work mapping of the per-pixel kernel units (the four a-trous filters through rt_atrous_kernels.h,
 * denoise_var.hip's variance pass, adaptive.hip, guides.hip, temporal.hip, aov_tiles.hip), the grids that go with it and the one launch
 * tail.  A unit includes it inside its own namespace, as rt_atrous_kernels.h is (<hip/hip_runtime.h> and <stdint.h> before the namespace).
 *
 * The mapping: one lane per pixel, an 8 x 8 pixel block per wave, 2 x 2 such blocks (16 x 16 pixels) per workgroup of 256 lanes.  Three
 * ways to place a workgroup's block: in row order over a width (a frame, or the rectangle of a merge); inside a tile of a tile list,
 * (tile / 16)^2 workgroups per tile, tile after tile; or by the kernel's own loop over the lane's position (the tile error). */
#define RT_PX_WG 256     /* lanes of a workgroup */
#define RT_PX_BLOCK 16u  /* its block is 16 x 16 pixels */

/* this lane's pixel of the 16 x 16 block (bx, by): 8 x 8 per wave, 2 x 2 waves */
__device__ __forceinline__ void rt_px_block_pixel(uint32_t bx, uint32_t by, uint32_t& x, uint32_t& y) {
    const uint32_t wv = threadIdx.x >> 6, in = threadIdx.x & 63u;
    x = bx * RT_PX_BLOCK + (wv & 1u) * 8u + (in & 7u);
    y = by * RT_PX_BLOCK + (wv >> 1) * 8u + (in >> 3);
}
/* this lane's position inside its workgroup's block, for a kernel that places the block itself */
__device__ __forceinline__ void rt_px_lane_xy(uint32_t& lx, uint32_t& ly) { rt_px_block_pixel(0u, 0u, lx, ly); }
/* this lane's pixel (x, y) with the workgroups in row order over `w` pixels, (bx, by) its workgroup's block.  The caller leaves or masks
 * where x >= w or y is beyond its rows */
__device__ __forceinline__ void rt_px_lane_pixel(uint32_t w, uint32_t& bx, uint32_t& by, uint32_t& x, uint32_t& y) {
    const uint32_t blocks_x = (w + RT_PX_BLOCK - 1u) / RT_PX_BLOCK;
    bx = blockIdx.x % blocks_x; by = blockIdx.x / blocks_x;
    rt_px_block_pixel(bx, by, x, y);
}
__device__ __forceinline__ void rt_px_lane_pixel(uint32_t w, uint32_t& x, uint32_t& y) {
    uint32_t bx, by;
    rt_px_lane_pixel(w, bx, by, x, y);
}
/* this lane in a tile list: tile k of the list, pixel (lx, ly) of that tile, and the tile's record rec[k] = {x0, y0, sample_offset, -}
 * (rt1w_tile).  k follows from blockIdx alone, so the record is read wave-uniformly */
struct RtPxListLane { uint32_t k, lx, ly, x0, y0, sample_offset; };
__device__ __forceinline__ RtPxListLane rt_px_list_lane(uint32_t tile, const uint32_t* __restrict__ rec) {
    const uint32_t bw = tile / RT_PX_BLOCK;
    RtPxListLane l;
    l.k = blockIdx.x / (bw * bw);
    const uint32_t b = blockIdx.x % (bw * bw);
    l.x0 = rec[(size_t)l.k * 4u]; l.y0 = rec[(size_t)l.k * 4u + 1u]; l.sample_offset = rec[(size_t)l.k * 4u + 2u];
    rt_px_block_pixel(b % bw, b / bw, l.lx, l.ly);
    return l;
}

/* workgroups of rt_px_lane_pixel over w x h pixels, and of rt_px_list_lane over n tiles (<= 2^20 x 256) */
__host__ inline unsigned rt_px_frame_grid(uint32_t w, uint32_t h) { return ((w + RT_PX_BLOCK - 1u) / RT_PX_BLOCK) * ((h + RT_PX_BLOCK - 1u) / RT_PX_BLOCK); }
__host__ inline unsigned rt_px_list_grid(uint32_t tile, uint32_t n) { return n * (tile / RT_PX_BLOCK) * (tile / RT_PX_BLOCK); }

/* what a launcher ends in: `grid` workgroups of RT_PX_WG lanes of `kernel` on `stream`, launch[0..1] = grid, block.  0 or -1 (launch
 * failure).  The arguments are converted to the kernel's own parameter types */
template <class... Params, class... Args>
__host__ int rt_px_launch(void (*kernel)(Params...), unsigned grid, hipStream_t stream, unsigned launch[2], const Args&... args) {
    launch[0] = grid; launch[1] = RT_PX_WG;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(RT_PX_WG), 0, stream, static_cast<Params>(args)...);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
