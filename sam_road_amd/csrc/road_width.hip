// The road width under every edge of a graph, on the device (config key ROAD_WIDTH): an exact, capped, squared Euclidean
// distance map of the thresholded road mask in two separable passes, and a per-edge gather of it along the edge's centre line.  The rule
// is stated on the host (sam_road_amd/road_width.py) in integers; the map must equal road_dist_ref and the statistics road_width_ref
// exactly.  Three launches, their count and their grids fixed by H, W and E alone; no workgroup waits for another, no atomics, nothing is
// read back.  road_width_piece.hpp has the per-item code.
//
// road_dist_cols: a workgroup owns RW_COL_THREADS columns by RW_COL_ROWS rows.  A lane owns a column: the 64 lanes of a wave read 64
//   consecutive bytes of a row of the mask.  It sweeps down from R rows above the chunk, keeps the chunk's distances in its own column of
//   8 KiB of LDS (lane l writes byte l of a row of 256: the four lanes of a dword share a bank and no two dwords of a wave do), sweeps up
//   from R rows below the chunk and stores the smaller of the two.  Rows outside the image hold no background.
// road_dist_rows: a workgroup owns a segment of RW_ROW_SEG pixels of one row, counted in quads of the FLAT pixel index so that a lane's
//   four u16 are one aligned 8-byte store in every row whatever W is.  The segment and R columns of G on either side are staged in LDS
//   (at most 1532 bytes); a lane reads bytes l + dx, consecutive over the lanes: 16 dwords of 16 banks per wave, no conflict.  A pixel
//   with G = 0 stores 0 without a search; the search stops where dx^2 reaches the minimum so far.
// graph_edge_widths: EDGE_SUPPORT's lane dealing at t = 1, RW_LANES = 16 lanes per edge, four edges per wave, grid-stride over the edges;
//   six values in registers, four shuffle sums, a shuffle minimum and a shuffle maximum, two 16-byte stores per edge.
#include "common.hpp"
#include "kernels.hpp"

namespace srh {

constexpr long RW_MAX_BLOCKS = 1L << 20;

__global__ __launch_bounds__(RW_COL_THREADS) void road_dist_cols_kernel(RoadDistParams p) {
    __shared__ uint8_t down[RW_COL_ROWS * RW_COL_THREADS];
    const long strips = rw_col_strips(p), items = strips * rw_col_chunks(p);
    for (long it = blockIdx.x; it < items; it += gridDim.x) {          // a lane's LDS column is its own: no barrier between items
        const long x = (it % strips) * RW_COL_THREADS + threadIdx.x;
        if (x < p.W) rw_col_item(p, (int)x, (int)(it / strips) * RW_COL_ROWS, down + threadIdx.x, RW_COL_THREADS);
    }
}

__global__ __launch_bounds__(RW_ROW_THREADS) void road_dist_rows_kernel(RoadDistParams p) {
    __shared__ __attribute__((aligned(16))) uint8_t win[RW_ROW_LDS];
    const long segs = rw_row_segs(p), items = segs * p.H;
    for (long it = blockIdx.x; it < items; it += gridDim.x) {          // the same trip count for every lane of a workgroup
        const int y = (int)(it / segs);
        const long seg = it % segs;
        int lo, hi;
        rw_row_window(p, y, seg, lo, hi);
        for (int k = threadIdx.x; k < hi - lo; k += RW_ROW_THREADS) win[k] = rw_row_stage(p, y, lo, k);
        __syncthreads();
        rw_row_item(p, y, seg, threadIdx.x, win, lo, hi);
        __syncthreads();                                               // the window is overwritten by the next item
    }
}

__global__ __launch_bounds__(GR_THREADS) void graph_edge_widths_kernel(EdgeWidthParams p) {
    constexpr int PER_BLOCK = GR_THREADS / RW_LANES;
    const int lane = threadIdx.x & (RW_LANES - 1);
    // every lane of a wave runs the same number of rounds (an edge index past E loads nothing and stores nothing), so the shuffles below
    // are executed by whole waves
    const long rounds = (p.g.E + (long)gridDim.x * PER_BLOCK - 1) / ((long)gridDim.x * PER_BLOCK);
    long e = (long)blockIdx.x * PER_BLOCK + threadIdx.x / RW_LANES;
    for (long k = 0; k < rounds; ++k, e += (long)gridDim.x * PER_BLOCK) {
        RwAcc a;
        if (e < p.g.E) {
            const GrEdge ed = gr_edge_load(p.g, e);
            if (ed.x0 <= ed.x1)
                for (int y = ed.y0; y <= ed.y1; ++y) {
                    int xlo, xhi;
                    gr_edge_row(ed, y, xlo, xhi);
                    for (int x = xlo + lane; x <= xhi; x += RW_LANES) rw_edge_pixel(p, ed, y, x, a);
                }
        }
        for (int off = RW_LANES / 2; off > 0; off >>= 1) {             // n < 46343 and s_q < 2^31: no carry out of 32 bits
            a.n += __shfl_down(a.n, off, RW_LANES); a.n_in += __shfl_down(a.n_in, off, RW_LANES);
            a.s_q += __shfl_down(a.s_q, off, RW_LANES); a.n_cap += __shfl_down(a.n_cap, off, RW_LANES);
            const uint32_t mn = __shfl_down(a.d2_min, off, RW_LANES), mx = __shfl_down(a.d2_max, off, RW_LANES);
            a.d2_min = mn < a.d2_min ? mn : a.d2_min; a.d2_max = mx > a.d2_max ? mx : a.d2_max;
        }
        if (lane == 0 && e < p.g.E) rw_edge_store(p, e, a);
    }
}

// Which of the two passes: 0 the column pass (mask -> g), 1 the row pass (g -> d2).  -2 for bad parameters.
int launch_road_dist(const RoadDistParams& p, int pass, hipStream_t s) {
    if (!rw_dist_ok(p) || pass < 0 || pass > 1) return -2;
    // a workgroup per item up to RW_MAX_BLOCKS, a stride over the items above it: the grid is a function of H and W alone
    if (pass == 0) {
        const long items = rw_col_strips(p) * rw_col_chunks(p);
        hipLaunchKernelGGL(road_dist_cols_kernel, dim3((unsigned)(items < RW_MAX_BLOCKS ? items : RW_MAX_BLOCKS)), dim3(RW_COL_THREADS), 0, s, p);
    } else {
        const long items = rw_row_segs(p) * p.H;
        hipLaunchKernelGGL(road_dist_rows_kernel, dim3((unsigned)(items < RW_MAX_BLOCKS ? items : RW_MAX_BLOCKS)), dim3(RW_ROW_THREADS), 0, s, p);
    }
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

// The tables have been checked on the host (gr_tables_ok).  -2 for bad parameters.
int launch_graph_edge_widths(const EdgeWidthParams& p, hipStream_t s) {
    if (!rw_edges_ok(p)) return -2;
    constexpr int PER_BLOCK = GR_THREADS / RW_LANES;
    const long blocks = ((long)p.g.E + PER_BLOCK - 1) / PER_BLOCK;
    hipLaunchKernelGGL(graph_edge_widths_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(GR_THREADS), 0, s, p);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace srh
