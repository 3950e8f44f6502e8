// The road-mask evidence under every edge of a graph (edge_support.hip, config key EDGE_SUPPORT): the parameters and the
// work of ONE item of the launch, free of HIP so that a CPU program can run the kernel's own addressing and arithmetic over every item
// of a launch (tests/edge_support_check.cpp, under the host sanitizers) before a GPU does.  The rule is stated on the host
// (sam_road_amd/edge_support.py) in integers, and the four counters must equal edge_support_ref exactly.
//
// Which pixels belong to an edge is GRAPH_RASTER's rule, unchanged: gr_edge_load, gr_edge_row and gr_covered of graph_raster_piece.hpp.  A
// wave owns an edge and walks the rows of its grown, clipped bounding box, lanes across the columns of the part of the row the segment can
// reach; a lane adds, for every covered pixel, one byte of the mask (and one of valid) to four 32-bit counters of its own.  The counters
// are summed over the wave and the edge's 16 bytes are stored once.  Integer sums: any order gives the same numbers.
//
// The 32-bit bound.  The covered set of an edge is the set of lattice points of a stadium: a convex region of length l <= sqrt(2) S
// (S = GR_MAX_SPAN = 16383), width t <= GR_MAX_WIDTH = 255, area A = l t + pi t^2 / 4 and perimeter P = 2 l + pi t.  A convex region holds
// at most A + P / 2 + 1 lattice points: n <= 23170 * 255 + 51071 + 23170 + 401 + 1 = 5 982 993 < 6.0e6, and 255 n <= 1 525 663 215 < 2^31.
#pragma once
#include "graph_raster_piece.hpp"

namespace srh {

constexpr long ES_MAX_COVERED = 5982993L;                          // the bound above, in whole pixels
static_assert(255L * ES_MAX_COVERED < 2147483648L, "the sum of an edge's mask bytes fits 32 bits");

// out[4 e .. 4 e + 3] = {n, s, n_on, n_invalid} of edge e over its covered pixels: their number, the sum of mask, the number with
// mask > on_level, the number with valid == 0 (0 without valid).
struct EdgeStatsParams {
    GraphRasterParams g;                 // nodes, edges, N, E, H, W and t as the rasteriser takes them; g.out is not used
    const uint8_t* mask = nullptr;       // u8 [H, W]
    const uint8_t* valid = nullptr;      // u8 [H, W] or nullptr
    int on_level = 0;                    // 0 .. 255
    int32_t* out = nullptr;              // [E, 4], 16-byte aligned
};

inline bool es_params_ok(const EdgeStatsParams& p) {
    const GraphRasterParams& g = p.g;
    if (g.N < 0 || g.E < 1 || g.N == 0 || !g.nodes || !g.edges || !p.mask || !p.out) return false;
    if ((reinterpret_cast<uintptr_t>(g.nodes) | reinterpret_cast<uintptr_t>(g.edges)) & 3) return false;
    if (reinterpret_cast<uintptr_t>(p.out) & 15) return false;
    if (g.H < 1 || g.W < 1 || (long)g.H * g.W > GR_MAX_PIXELS) return false;
    return g.t >= 1 && g.t <= GR_MAX_WIDTH && p.on_level >= 0 && p.on_level <= 255;
}

// Pixel (y, x) of the edge's row span, inside the clipped box: the ONLY reads of the launch besides the tables.  acc: the lane's counters.
SRH_GR_HD void es_pixel(const EdgeStatsParams& p, const GrEdge& ed, int y, int x, uint32_t* acc) {
    if (!gr_covered(ed, y, x)) return;
    const long i = (long)y * p.g.W + x;
    const uint32_t m = p.mask[i];
    acc[0] += 1u; acc[1] += m; acc[2] += m > (uint32_t)p.on_level;
    if (p.valid) acc[3] += p.valid[i] == 0;
}

// The edge's 16 bytes: the ONLY write of the launch, one 16-byte store.
SRH_GR_HD void es_store(const EdgeStatsParams& p, long e, const uint32_t* acc) {
    *reinterpret_cast<GrWords*>(p.out + 4 * e) = GrWords{{acc[0], acc[1], acc[2], acc[3]}};
}

}  // namespace srh
