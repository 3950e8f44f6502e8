// The road graph as a raster, on the device (config key GRAPH_RASTER): the class map of a graph (0 background, 1 edge, 2
// node mark), its composition over the scene, and the comparison of a predicted graph with a ground-truth one.  The rule is stated on the
// host (sam_road_amd/graph_raster.py) in integers; the class map must equal graph_raster_ref byte for byte.  The reference draws with
// cv2.line / cv2.circle on the host (triage.py:8-71); those bytes are not reproduced.
//
// graph_clear: the map to 0, one 16-byte store per chunk of the ADDRESS, bytes at the ragged ends.
// graph_edges: a wave per edge (grid-stride over the edges).  It walks the rows of the edge's bounding box, grown by ceil(t / 2) and
//   clipped to the image, lanes across the columns the segment can reach in that row, and stores the edge byte where the pixel lies
//   within t / 2 of the segment.  Concurrent writers of a pixel store the same byte.
// graph_nodes: a wave per node, lanes across the pixels of the mark's clipped box; it runs behind graph_edges on the stream, so a node
//   mark wins over an edge.
// graph_composite: four pixels per thread, the scene (or a background colour) with the two classes in their colours.
// graph_compare: four pixels per thread; the four counts are summed per thread, per wave by shuffles, per workgroup in the LDS, and one
//   workgroup adds four 64-bit integers to the result with device-scope vector atomics (graph_counts_zero clears it in front).  Integer
//   sums: any order gives the same numbers.
// No workspace, nothing read back.  graph_raster_piece.hpp has the per-item code of every launch.
#include "common.hpp"
#include "kernels.hpp"

namespace srh {

__global__ __launch_bounds__(GR_THREADS) void graph_clear_kernel(GraphRasterParams p) {
    const long chunks = gr_clear_chunks(p);
    for (long c = (long)blockIdx.x * GR_THREADS + threadIdx.x; c < chunks; c += (long)gridDim.x * GR_THREADS) gr_clear_item(p, c);
}

__global__ __launch_bounds__(GR_THREADS) void graph_edges_kernel(GraphRasterParams p) {
    const int lane = threadIdx.x & (GR_WAVE - 1);
    for (long e = (long)blockIdx.x * GR_WAVES + threadIdx.x / GR_WAVE; e < p.E; e += (long)gridDim.x * GR_WAVES) {
        const GrEdge ed = gr_edge_load(p, e);
        if (ed.x0 > ed.x1) continue;
        for (int y = ed.y0; y <= ed.y1; ++y) {
            int xlo, xhi;
            gr_edge_row(ed, y, xlo, xhi);
            for (int x = xlo + lane; x <= xhi; x += GR_WAVE) gr_edge_item(p, ed, y, x);
        }
    }
}

__global__ __launch_bounds__(GR_THREADS) void graph_nodes_kernel(GraphRasterParams p) {
    const int lane = threadIdx.x & (GR_WAVE - 1);
    for (long n = (long)blockIdx.x * GR_WAVES + threadIdx.x / GR_WAVE; n < p.N; n += (long)gridDim.x * GR_WAVES) {
        const GrNode nd = gr_node_load(p, n);
        const int px = nd.bh * nd.bw;                                  // at most 255 x 255
        for (int k = lane; k < px; k += GR_WAVE) gr_node_item(p, nd, k);
    }
}

__global__ __launch_bounds__(GR_THREADS) void graph_composite_kernel(GraphCompositeParams p) {
    const long quads = gr_quads(p.n);
    for (long q = (long)blockIdx.x * GR_THREADS + threadIdx.x; q < quads; q += (long)gridDim.x * GR_THREADS) gr_composite_item(p, q);
}

__global__ void graph_counts_zero_kernel(unsigned long long* counts) {
    if (threadIdx.x < 4) counts[threadIdx.x] = 0ull;
}

__global__ __launch_bounds__(GR_THREADS) void graph_compare_kernel(GraphCompareParams p) {
    __shared__ uint32_t part[GR_WAVES][4];
    uint32_t acc[4] = {0u, 0u, 0u, 0u};                                // a thread sees at most 2^31 / GR_THREADS pixels
    const long quads = gr_quads(p.n);
    for (long q = (long)blockIdx.x * GR_THREADS + threadIdx.x; q < quads; q += (long)gridDim.x * GR_THREADS) gr_compare_item(p, q, acc);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t v = acc[k];                                           // a wave sees at most 2^31 pixels: no carry out of 32 bits
        for (int off = GR_WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off, GR_WAVE);
        if ((threadIdx.x & (GR_WAVE - 1)) == 0) part[threadIdx.x / GR_WAVE][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        unsigned long long sum = 0ull;
        for (int w = 0; w < GR_WAVES; ++w) sum += part[w][threadIdx.x];
        if (sum) atomicAdd(&p.counts[threadIdx.x], sum);
    }
}

static unsigned gr_grid(long items, long per_block, long cap) {
    const long blocks = (items + per_block - 1) / per_block;
    return (unsigned)(blocks < 1 ? 1 : blocks < cap ? blocks : cap);
}

// The tables have been checked on the host (gr_tables_ok).  -2 for bad parameters.  The caller issues clear, edges (E > 0), nodes (N > 0 and a
// mark) in this order on one stream; the clear always runs, so out is fully defined.
int launch_graph_clear(const GraphRasterParams& p, hipStream_t s) {
    if (!gr_params_ok(p)) return -2;
    hipLaunchKernelGGL(graph_clear_kernel, dim3(gr_grid(gr_clear_chunks(p), GR_THREADS, 2048)), dim3(GR_THREADS), 0, s, p);
    if (hipGetLastError() != hipSuccess) return -3;
    return 0;
}

int launch_graph_edges(const GraphRasterParams& p, hipStream_t s) {
    if (!gr_params_ok(p) || p.E < 1) return -2;
    hipLaunchKernelGGL(graph_edges_kernel, dim3(gr_grid(p.E, GR_WAVES, 8192)), dim3(GR_THREADS), 0, s, p);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_graph_nodes(const GraphRasterParams& p, hipStream_t s) {
    if (!gr_params_ok(p) || p.N < 1 || p.mark == GR_MARK_NONE) return -2;
    hipLaunchKernelGGL(graph_nodes_kernel, dim3(gr_grid(p.N, GR_WAVES, 8192)), dim3(GR_THREADS), 0, s, p);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_graph_composite(const GraphCompositeParams& p, hipStream_t s) {
    if (!gr_composite_ok(p)) return -2;
    hipLaunchKernelGGL(graph_composite_kernel, dim3(gr_grid(gr_quads(p.n), GR_THREADS, 2048)), dim3(GR_THREADS), 0, s, p);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_graph_counts_zero(const GraphCompareParams& p, hipStream_t s) {
    if (!gr_compare_ok(p)) return -2;
    hipLaunchKernelGGL(graph_counts_zero_kernel, dim3(1), dim3(GR_WAVE), 0, s, p.counts);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_graph_compare(const GraphCompareParams& p, hipStream_t s) {
    if (!gr_compare_ok(p)) return -2;
    hipLaunchKernelGGL(graph_compare_kernel, dim3(gr_grid(gr_quads(p.n), GR_THREADS, 1024)), dim3(GR_THREADS), 0, s, p);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace srh
