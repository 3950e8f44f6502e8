// The road-mask evidence under every edge of a graph, on the device (config key EDGE_SUPPORT): for every edge the number
// of pixels GRAPH_RASTER's rule covers for it at width t, the sum of the mask over them, the number of them above a level and the number
// of them outside a validity mask.  The rule is stated on the host (sam_road_amd/edge_support.py) in integers; the four counters must
// equal edge_support_ref exactly.
//
// graph_edge_stats: LANES lanes per edge (64: a wave per edge; 16: four edges per wave), grid-stride over the edges.  The lanes walk the rows of the edge's bounding
//   box, grown by ceil(t / 2) and clipped to the image, across the columns the segment can reach in that row (gr_edge_row), and add one
//   byte of the mask and one of valid per covered pixel to four 32-bit counters in registers.  The counters are summed over the lanes by
//   shuffles and lane 0 stores the edge's 16 bytes as one vector store.  No atomics, no LDS, no scratch; an edge with an empty box stores
//   four zeros, so every element of out is defined and nothing else is written.
// Lane use is a measured choice: at t = 1 a row's span is about 5 columns, so a wave per edge leaves nine lanes in ten
//   idle.  Where the span fits, 2 ceil(t / 2) + 3 <= ES_GROUP (t <= 12), an edge gets a group of 16 lanes, four edges per wave, and the
//   sums are taken inside the group: 0.114 ms against 0.258 ms for the 35 771 edges of the 2048^2 bench scene at t = 1 (the kernel time
//   varies by 0.006 ms from run to run).  Wider lines keep the wave per edge.  -DSRH_ES_GROUP_LANES=64 builds the wave-per-edge form alone.
// No workspace, nothing read back.  edge_support_piece.hpp has the per-item code.
#include "common.hpp"
#include "kernels.hpp"

#ifndef SRH_ES_GROUP_LANES
#define SRH_ES_GROUP_LANES 16
#endif

namespace srh {

template <int LANES>
__global__ __launch_bounds__(GR_THREADS) void graph_edge_stats_kernel(EdgeStatsParams p) {
    constexpr int PER_BLOCK = GR_THREADS / LANES;
    const int lane = threadIdx.x & (LANES - 1);
    // every lane of a wave runs the same number of rounds (an edge index past E loads nothing and stores nothing), so the shuffles below
    // are executed by whole waves
    const long rounds = (p.g.E + (long)gridDim.x * PER_BLOCK - 1) / ((long)gridDim.x * PER_BLOCK);
    long e = (long)blockIdx.x * PER_BLOCK + threadIdx.x / LANES;
    for (long k = 0; k < rounds; ++k, e += (long)gridDim.x * PER_BLOCK) {
        uint32_t acc[4] = {0u, 0u, 0u, 0u};
        if (e < p.g.E) {
            const GrEdge ed = gr_edge_load(p.g, e);
            if (ed.x0 <= ed.x1)
                for (int y = ed.y0; y <= ed.y1; ++y) {
                    int xlo, xhi;
                    gr_edge_row(ed, y, xlo, xhi);
                    for (int x = xlo + lane; x <= xhi; x += LANES) es_pixel(p, ed, y, x, acc);
                }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c)                                    // an edge covers fewer than 6.0e6 pixels: no carry out of 32 bits
            for (int off = LANES / 2; off > 0; off >>= 1) acc[c] += __shfl_down(acc[c], off, LANES);
        if (lane == 0 && e < p.g.E) es_store(p, e, acc);
    }
}

// The tables have been checked on the host (gr_tables_ok).  -2 for bad parameters.
int launch_graph_edge_stats(const EdgeStatsParams& p, hipStream_t s) {
    if (!es_params_ok(p)) return -2;
    constexpr int G = SRH_ES_GROUP_LANES;
    static_assert(G == 64 || G == 32 || G == 16, "a group is a power-of-two part of a wave");
    if (G < GR_WAVE && 2 * ((p.g.t + 1) >> 1) + 3 <= G) {
        const long blocks = ((long)p.g.E + GR_THREADS / G - 1) / (GR_THREADS / G);
        hipLaunchKernelGGL(graph_edge_stats_kernel<G>, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(GR_THREADS), 0, s, p);
    } else {
        const long blocks = ((long)p.g.E + GR_WAVES - 1) / GR_WAVES;
        hipLaunchKernelGGL(graph_edge_stats_kernel<GR_WAVE>, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(GR_THREADS), 0, s, p);
    }
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace srh
