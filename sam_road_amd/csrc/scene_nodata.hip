// The validity mask of a scene from a nodata VALUE, on the device (config key SCENE_NODATA): the two steps that
// srh_mask_clean does not already provide.  The rule is stated on the host (sam_road_amd/nodata.py) and the result must equal nodata_ref
// byte for byte.  The reference has no such step.
//
// scene_nodata_match: out u8 [n], 0 / 1 per pixel of a raw scene u8 / u16 [n, C] — does every (any) band lie within [lo_c, hi_c]?  The
//   kernel sees n pixels and knows nothing of H or W, so one launch serves a scene and the ragged buffer of a scene group alike.
//   Bandwidth-bound: a thread takes four pixels, reads their 4 C elements in the 16-byte chunks of the ADDRESS (one 16-byte load each;
//   element loads only where a chunk reaches outside the buffer, at its head and tail) and stores its four results as one word.  With
//   `invert` and `and_with` the same launch writes the finished validity mask, !hit & (caller's mask != 0).  No atomics, no LDS.
// scene_nodata_grow: the Chebyshev dilation by r of n images described by a table, src -> dst (no overlap).  Separable and output-
//   stationary: a workgroup owns a 64 x 64 block of outputs, stages the window block + r on each side in the LDS (0 outside the image),
//   runs a row pass (any of 2 r + 1 neighbours in the row) over every window row, then a column pass over the row pass for its own
//   outputs, and stores them, four per thread.  Every index is bounded by the image's H and W where it is used.  15 KiB of LDS, no
//   atomics, no scratch, no inline assembly.
// scene_nodata_piece.hpp has the per-item code of both.
#include "common.hpp"
#include "kernels.hpp"

namespace srh {

template <class T>
__global__ __launch_bounds__(ND_THREADS) void scene_nodata_match_kernel(SceneNodataParams p, long n_items) {
    for (long i = (long)blockIdx.x * ND_THREADS + threadIdx.x; i < n_items; i += (long)gridDim.x * ND_THREADS) nodata_match_item<T>(p, i);
}

__global__ __launch_bounds__(ND_THREADS) void scene_nodata_grow_kernel(SceneGrowParams p) {
    __shared__ alignas(16) uint8_t win[NG_WIN_BYTES];
    __shared__ alignas(16) uint8_t row[NG_ROW_BYTES];
    const int k = blockIdx.y;                                          // the image: uniform over the workgroup
    const long n_blocks = grow_blocks((long)p.table[(long)k * NG_COLS + NG_H], (long)p.table[(long)k * NG_COLS + NG_W]);
    const int n_stage = (NG_BH + 2 * p.r) * (NG_BW + 2 * p.r), n_row = (NG_BH + 2 * p.r) * NG_BW;
    for (long b = blockIdx.x; b < n_blocks; b += gridDim.x) {
        const NgBlock g = grow_locate(p, k, b);
        for (int t = threadIdx.x; t < n_stage; t += ND_THREADS) grow_stage_item(p, g, win, t);
        __syncthreads();
        for (int t = threadIdx.x; t < n_row; t += ND_THREADS) grow_row_item(p, win, row, t);
        __syncthreads();
        for (int t = threadIdx.x; t < NG_BH * NG_BW / 4; t += ND_THREADS) grow_col_item(p, g, row, t);
        __syncthreads();                                               // the next block's staging overwrites what this one still reads
    }
}

int launch_scene_nodata_match(const SceneNodataParams& p, hipStream_t s) {
    if (!nodata_params_ok(p)) return -2;
    const long n_items = nodata_items(p);
    const long groups = (n_items + ND_THREADS - 1) / ND_THREADS;
    const unsigned grid = (unsigned)(groups < (1L << 20) ? groups : (1L << 20));
    if (p.wide) hipLaunchKernelGGL(scene_nodata_match_kernel<uint16_t>, dim3(grid), dim3(ND_THREADS), 0, s, p, n_items);
    else hipLaunchKernelGGL(scene_nodata_match_kernel<uint8_t>, dim3(grid), dim3(ND_THREADS), 0, s, p, n_items);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

// The table has been checked on the host (grow_table_ok); max_blocks = grow_max_blocks of it.  -2 for bad parameters.
int launch_scene_nodata_grow(const SceneGrowParams& p, long max_blocks, hipStream_t s) {
    if (!p.src || !p.dst || !p.table || p.n < 1 || p.n > NG_MAX_IMAGES || p.r < 1 || p.r > NG_MAX_R || (p.invert != 0 && p.invert != 1) || max_blocks < 1)
        return -2;
    const dim3 grid((unsigned)(max_blocks < (1L << 16) ? max_blocks : (1L << 16)), (unsigned)p.n);
    hipLaunchKernelGGL(scene_nodata_grow_kernel, grid, dim3(ND_THREADS), 0, s, p);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace srh
