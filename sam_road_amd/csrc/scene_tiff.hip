// A GeoTIFF's decompressed strips or tiles -> the scene raster [H, W, C] on the device (config key GEOTIFF): the predictor
// undo, the byte swap of big-endian files, planar -> interleaved and tile -> raster placement in ONE launch, whatever the file holds.  The
// rule is stated on the host (sam_road_amd/geotiff.py); the raster must equal tiff_read_ref bit for bit.  geotiff_piece.hpp has the layout
// of the table, the phases and every address; this file adds what needs a GPU: the barriers and the scan across the threads.
//
// A workgroup owns a row of a segment (grid-stride over the items, every lane of a workgroup takes the same trips).  Per chunk of at most
// TIF_CHUNK elements: stage (lane l loads elements l, l + 256, ...: consecutive over the lanes), barrier, and unless the predictor is 1:
// for each of the S samples of a pixel the lane's own sum (padded LDS: the lanes' words lie S * PP + a pad apart, no two of a wave's on
// one bank for the common S), an inclusive shuffle scan of the 64 sums in the wave, the wave's total into LDS, barrier, the running sums
// in place from (carry of the earlier chunks + the earlier waves' totals + the earlier lanes' sums), barrier; store, barrier.  The loops
// over the samples are unrolled to TIF_MAX_BANDS with a guard, so the S exclusive sums and carries of a lane are registers, not scratch.
// Wrapping 32-bit adds, of which the store keeps the low bits: exact.  Plain loads and stores, no atomics, nothing read back, LDS
// 16.5 KiB + 256 B whatever W is.
#include "common.hpp"
#include "kernels.hpp"

namespace srh {

__global__ __launch_bounds__(TIF_THREADS) void tiff_assemble_kernel(TiffParams p) {
    __shared__ uint32_t buf[TIF_LDS_WORDS];
    __shared__ uint32_t wtot[TIF_MAX_BANDS * TIF_WAVES];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long items = (long)p.n_seg * p.max_rows;
    for (long it = blockIdx.x; it < items; it += gridDim.x) {
        const TifRow row = tif_row(p, it);
        if (!row.live) continue;                                       // the same for every lane of the workgroup
        const int E = tif_chunk_elems(row.S);
        uint32_t carry[TIF_MAX_BANDS];
#pragma unroll
        for (int c = 0; c < TIF_MAX_BANDS; ++c) carry[c] = 0u;
        for (long k0 = 0; k0 < row.n; k0 += E) {
            const int ne = (int)(row.n - k0 < E ? row.n - k0 : E);
            for (int i = t; i < ne; i += TIF_THREADS) buf[tif_pad(i)] = tif_load(p, row, k0 + i);
            __syncthreads();
            if (p.predictor != 1) {
                const int npix = ne / row.S;
                uint32_t ex[TIF_MAX_BANDS];
#pragma unroll
                for (int c = 0; c < TIF_MAX_BANDS; ++c) {
                    ex[c] = 0u;
                    if (c < row.S) {
                        const uint32_t acc = tif_local_sum(buf, row.S, t, c, npix);
                        uint32_t inc = acc;
#pragma unroll
                        for (int off = 1; off < 64; off <<= 1) {       // whole waves get here: row.S is the workgroup's
                            const uint32_t v = __shfl_up(inc, off);
                            if (lane >= off) inc += v;
                        }
                        ex[c] = inc - acc;
                        if (lane == 63) wtot[c * TIF_WAVES + wave] = inc;
                    }
                }
                __syncthreads();
#pragma unroll
                for (int c = 0; c < TIF_MAX_BANDS; ++c) {
                    if (c < row.S) {
                        uint32_t base = carry[c] + ex[c], all = 0u;
#pragma unroll
                        for (int w = 0; w < TIF_WAVES; ++w) {
                            const uint32_t v = wtot[c * TIF_WAVES + w];
                            if (w < wave) base += v;
                            all += v;
                        }
                        tif_local_apply(buf, row.S, t, c, npix, base);
                        carry[c] += all;
                    }
                }
                __syncthreads();                                       // the store reads the other lanes' words
            }
            tif_store(p, row, k0, ne, t, buf);
            __syncthreads();                                           // buf and wtot are overwritten by the next chunk
        }
    }
}

// The table has been checked on the host (tif_table_ok).  -2 for bad parameters.
int launch_tiff_assemble(const TiffParams& p, hipStream_t s) {
    if (!tif_params_ok(p)) return -2;
    const long items = (long)p.n_seg * p.max_rows;
    hipLaunchKernelGGL(tiff_assemble_kernel, dim3((unsigned)(items < TIF_MAX_BLOCKS ? items : TIF_MAX_BLOCKS)), dim3(TIF_THREADS), 0, s, p);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace srh
