// The validity mask of a scene from the POLYGONS of an area of interest, on the device (config key SCENE_AOI).  The rule is
// stated on the host (sam_road_amd/aoi.py) in integers, and the result must equal aoi_ref byte for byte.  The reference has no such step.
//
// scene_aoi_fill: out u8 [H, W], 0 / 1 per pixel — is the pixel's centre inside (include polygons, or everywhere without any) and outside
//   every exclude polygon?  One launch whatever the polygons hold.  A workgroup of 256 threads owns a row (grid-stride over the rows) and
//   walks it in segments of 4096 columns, one bit per pixel in the LDS: per polygon its threads stride over the polygon's edges (one
//   16-byte load each), a crossing edge costs one 64-bit division and one LDS XOR, a prefix XOR (shifts inside a word, a population count
//   over the words' parities across words) turns toggles into inside bits, and the bits are ORed into an include or exclude row.  The
//   finished bits are expanded to bytes with 16-byte stores in the chunks of the ADDRESS, bytes at the ragged ends; `invert` and `and_with`
//   let the same launch write the finished validity mask.  1552 bytes of LDS whatever W is, LDS atomics only, no scratch, no workspace,
//   nothing read back.  XOR and OR commute: the result is independent of scheduling.
// scene_aoi_piece.hpp has the per-item code of every phase.
#include "common.hpp"
#include "kernels.hpp"

namespace srh {

__global__ __launch_bounds__(AOI_THREADS) void scene_aoi_fill_kernel(SceneAoiParams p) {
    __shared__ AoiLds lds;
    const int t = threadIdx.x;
    const int n_polys = p.n_include + p.n_exclude;
    for (long y = blockIdx.x; y < p.H; y += gridDim.x) {              // the row: uniform over the workgroup, and so is every loop bound below
        for (long x0 = 0; x0 < p.W; x0 += AOI_SEG) {
            aoi_begin_item(lds, t);
            for (int k = 0; k < n_polys; ++k) {
                aoi_clear_item(lds, t);
                __syncthreads();
                const int e1 = p.polys[k + 1];
                for (int e = p.polys[k] + t; e < e1; e += AOI_THREADS) aoi_edge_item(p, lds, y, x0, e);
                __syncthreads();
                aoi_scan_item(lds, t);
                __syncthreads();
                aoi_fold_item(lds, t, k < p.n_include);
                __syncthreads();                                       // the next polygon clears what this one still reads
            }
            aoi_final_item(p, lds, t);
            __syncthreads();
            const int chunks = aoi_store_chunks(p, y, x0);
            for (int c = t; c < chunks; c += AOI_THREADS) aoi_store_item(p, lds, y, x0, c);
            __syncthreads();                                           // the next segment's toggles overwrite the bits this one still reads
        }
    }
}

// The tables have been checked on the host (aoi_table_ok).  -2 for bad parameters.
int launch_scene_aoi_fill(const SceneAoiParams& p, hipStream_t s) {
    if (!aoi_params_ok(p)) return -2;
    const unsigned grid = (unsigned)(p.H < (1 << 16) ? p.H : (1 << 16));
    hipLaunchKernelGGL(scene_aoi_fill_kernel, dim3(grid), dim3(AOI_THREADS), 0, s, p);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace srh
