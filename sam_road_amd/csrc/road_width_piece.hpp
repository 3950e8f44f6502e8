// The road width under every edge of a graph (road_width.hip, config key ROAD_WIDTH): the parameters and the work of ONE
// item of each of the three launches, free of HIP so that a CPU program can run the kernels' own addressing and arithmetic over every item
// of a launch (tests/road_width_check.cpp, under the host sanitizers) before a GPU does.  The rule is stated on the host
// (sam_road_amd/road_width.py) in integers; the distance map must equal road_dist_ref and the six statistics road_width_ref exactly.
//
// The distance map is the capped squared Euclidean distance of every road pixel (mask > on_level) to the nearest pixel OF THE IMAGE that
// is not road, in its separable form:
//   column pass  G[y, x]  = min(R + 1, vertical distance in column x to the nearest background pixel)          u8, 0 on background
//   row pass     D2[y, x] = min(R^2, min over |dx| <= R, 0 <= x + dx < W of dx^2 + G[y, x + dx]^2)              u16, 0 on background
// Rows and columns outside the image hold no background.  The capped search is exact: a background pixel nearer than R lies within R in
// both axes, so its column is searched and its row is within the R rows the column pass looked at; a candidate that the caps distort
// (G = R + 1) is at least (R + 1)^2 > R^2 and is cut by the cap.
//
// The edge gather walks the 8-connected centre line of an edge — EDGE_SUPPORT's covered set at t = 1, by gr_edge_load, gr_edge_row and
// gr_covered, unchanged — and keeps six values per lane: n, n_in = #(D2 > 0), s_q = sum of floor(16 sqrt(D2)), n_cap = #(D2 = R^2), the
// minimum of D2 over the pixels with D2 > 0 and the maximum of D2.
//
// The 32-bit bound.  At t = 1 the covered set lies in a stadium of length l <= sqrt(2) GR_MAX_SPAN < 23170 and width 1: by the
// lattice-point bound of edge_support_piece.hpp, n <= 23170 + 0.79 + 23170 + 1.58 + 1 < 46343 (RW_MAX_COVERED), floor(16 sqrt(D2)) <=
// floor(16 * 254) = 4064, so s_q <= 4064 * 46343 = 188 337 952 < 2^31.
#pragma once
#include "edge_support_piece.hpp"

#define RW_UNROLL8 _Pragma("unroll 8")

namespace srh {

constexpr int RW_MAX_R = 254;                                      // (R + 1) fits a byte, R^2 = 64516 fits 16 bits
constexpr int RW_COL_THREADS = 256;                                // columns of a strip of the column pass, one per lane
constexpr int RW_COL_ROWS = 32;                                    // rows of a chunk of the column pass
constexpr int RW_ROW_THREADS = 256;
constexpr int RW_QUAD = 4;                                         // pixels of a lane of the row pass: four u16, one 8-byte store
constexpr int RW_ROW_SEG = RW_ROW_THREADS * RW_QUAD;               // pixels of a segment of the row pass
constexpr int RW_ROW_LDS = RW_ROW_SEG + 2 * RW_MAX_R;              // bytes of G a segment stages at most
constexpr int RW_LANES = 16;                                       // lanes of an edge of the gather
constexpr long RW_MAX_COVERED = 46343L;
constexpr uint32_t RW_MAX_Q = 4064u;
static_assert((long)RW_MAX_Q * RW_MAX_COVERED < 2147483648L, "the sum of an edge's floor(16 sqrt(D2)) fits 32 bits");
static_assert(RW_MAX_R * RW_MAX_R <= 65535 && RW_MAX_R + 1 <= 255, "D2 fits 16 bits and G a byte");

struct alignas(8) RwQuad { uint16_t v[RW_QUAD]; };

struct RoadDistParams {
    const uint8_t* mask = nullptr;       // u8 [H, W]
    uint8_t* g = nullptr;                // u8 [H, W]: written by the column pass, read by the row pass
    uint16_t* d2 = nullptr;              // u16 [H, W], 8-byte aligned: pixel i of the flat image lies at d2 + i, so the quads of pixels
                                         // 4 q .. 4 q + 3 OF THE FLAT INDEX are whole aligned 8-byte words in every row, whatever W is
    int H = 0, W = 0;
    int on_level = 0;                    // 0 .. 255
    int R = 1;                           // 1 .. 254
};

inline bool rw_dist_ok(const RoadDistParams& p) {
    if (!p.mask || !p.g || !p.d2 || (reinterpret_cast<uintptr_t>(p.d2) & 7)) return false;
    if (p.H < 1 || p.W < 1 || (long)p.H * p.W > GR_MAX_PIXELS) return false;
    return p.R >= 1 && p.R <= RW_MAX_R && p.on_level >= 0 && p.on_level <= 255;
}

// ---- column pass -----------------------------------------------------------------------------------------------------------------------
SRH_GR_HD long rw_col_strips(const RoadDistParams& p) { return ((long)p.W + RW_COL_THREADS - 1) / RW_COL_THREADS; }
SRH_GR_HD long rw_col_chunks(const RoadDistParams& p) { return ((long)p.H + RW_COL_ROWS - 1) / RW_COL_ROWS; }

// Column x (0 <= x < W), rows y0 .. y0 + RW_COL_ROWS - 1 (those below H).  down[k * stride], 0 <= k < RW_COL_ROWS, is the lane's own
// scratch (a column of the workgroup's LDS).  The sweep down starts R rows above the chunk, the sweep up R rows below it, both clipped to
// the image: the ONLY reads of mask and the ONLY writes of g of the launch.
SRH_GR_HD void rw_col_item(const RoadDistParams& p, int x, int y0, uint8_t* down, int stride) {
    const int y1 = gr_min(y0 + RW_COL_ROWS, p.H);                  // one past the chunk's last row
    const int cap = p.R + 1;
    int d = cap;                                                   // no background seen; the rows above the image hold none
    RW_UNROLL8                                                     // the loads do not depend on d: eight of them are in flight at a time
    for (int y = gr_max(y0 - p.R, 0); y < y1; ++y) {
        d = p.mask[(long)y * p.W + x] > p.on_level ? gr_min(d + 1, cap) : 0;
        if (y >= y0) down[(y - y0) * stride] = (uint8_t)d;
    }
    d = cap;
    RW_UNROLL8
    for (int y = gr_min(y1 - 1 + p.R, p.H - 1); y >= y0; --y) {
        d = p.mask[(long)y * p.W + x] > p.on_level ? gr_min(d + 1, cap) : 0;
        if (y < y1) p.g[(long)y * p.W + x] = (uint8_t)gr_min(d, (int)down[(y - y0) * stride]);
    }
}

// ---- row pass --------------------------------------------------------------------------------------------------------------------------
// A row is cut into quads of the FLAT index: quad j of row y holds x = 4 j - mis .. 4 j - mis + 3 with mis = (y W) mod 4, so the first and
// the last quad of a row may be ragged.  A segment is RW_ROW_THREADS quads of one row.
SRH_GR_HD int rw_row_mis(const RoadDistParams& p, int y) { return (int)(((long)y * p.W) & 3); }
SRH_GR_HD long rw_row_quads(const RoadDistParams& p) { return ((long)p.W + 3 + RW_QUAD - 1) / RW_QUAD; }          // enough for every mis
SRH_GR_HD long rw_row_segs(const RoadDistParams& p) { return (rw_row_quads(p) + RW_ROW_THREADS - 1) / RW_ROW_THREADS; }

// The columns segment `seg` of row y stages: [lo, hi), its pixels and R columns on either side, clipped to the image (hi <= lo: none).
SRH_GR_HD void rw_row_window(const RoadDistParams& p, int y, long seg, int& lo, int& hi) {
    const long first = seg * RW_ROW_SEG - rw_row_mis(p, y);
    lo = (int)(first - p.R > 0 ? first - p.R : 0);
    const long end = first + RW_ROW_SEG + p.R;
    hi = (int)(end < p.W ? end : p.W);
}

// Byte k of the window, lo + k < hi: the ONLY read of g of the launch.
SRH_GR_HD uint8_t rw_row_stage(const RoadDistParams& p, int y, int lo, int k) { return p.g[(long)y * p.W + lo + k]; }

// D2 of pixel x of the row whose window [lo, hi) is staged at win.  The search stops where dx^2 reaches the minimum so far: no later
// candidate can be smaller, so the result is that of the full search.
SRH_GR_HD uint32_t rw_row_pixel(const uint8_t* win, int lo, int hi, int x, int R) {
    const uint32_t g0 = win[x - lo];
    if (g0 == 0) return 0u;
    const uint32_t rr = (uint32_t)(R * R);
    uint32_t best = g0 * g0 < rr ? g0 * g0 : rr;
    for (int d = 1; d <= R; ++d) {
        const uint32_t dd = (uint32_t)(d * d);
        if (dd >= best) break;
        if (x - d >= lo) { const uint32_t g = win[x - d - lo]; const uint32_t v = dd + g * g; best = v < best ? v : best; }
        if (x + d < hi) { const uint32_t g = win[x + d - lo]; const uint32_t v = dd + g * g; best = v < best ? v : best; }
    }
    return best;
}

// Quad `quad` of segment `seg` of row y: the ONLY writes of d2 of the launch, one 8-byte store for a whole quad, its own pixels one at
// a time at the ragged ends of a row.
SRH_GR_HD void rw_row_item(const RoadDistParams& p, int y, long seg, int quad, const uint8_t* win, int lo, int hi) {
    const long x0 = seg * RW_ROW_SEG - rw_row_mis(p, y) + (long)quad * RW_QUAD;
    if (x0 >= p.W || x0 + RW_QUAD <= 0) return;
    uint16_t* row = p.d2 + (long)y * p.W;
    if (x0 >= 0 && x0 + RW_QUAD <= p.W) {
        RwQuad q;
        GR_UNROLL
        for (int k = 0; k < RW_QUAD; ++k) q.v[k] = (uint16_t)rw_row_pixel(win, lo, hi, (int)x0 + k, p.R);
        *reinterpret_cast<RwQuad*>(row + x0) = q;
    } else {
        for (int k = 0; k < RW_QUAD; ++k)
            if (x0 + k >= 0 && x0 + k < p.W) row[x0 + k] = (uint16_t)rw_row_pixel(win, lo, hi, (int)(x0 + k), p.R);
    }
}

// ---- edge gather -----------------------------------------------------------------------------------------------------------------------
// out[8 e .. 8 e + 7] = {n, n_in, s_q, n_cap, d2_min, d2_max, 0, 0} of edge e over its centre line.
struct EdgeWidthParams {
    GraphRasterParams g;                 // nodes, edges, N, E, H, W as the rasteriser takes them; g.t is 1; g.out is not used
    const uint16_t* d2 = nullptr;        // u16 [H, W], 2-byte aligned
    int R = 1;                           // 1 .. 254: the cap of d2 is R^2
    int32_t* out = nullptr;              // [E, 8], 16-byte aligned
};

inline bool rw_edges_ok(const EdgeWidthParams& p) {
    const GraphRasterParams& g = p.g;
    if (g.N < 1 || g.E < 1 || !g.nodes || !g.edges || !p.d2 || !p.out) return false;
    if ((reinterpret_cast<uintptr_t>(g.nodes) | reinterpret_cast<uintptr_t>(g.edges)) & 3) return false;
    if ((reinterpret_cast<uintptr_t>(p.d2) & 1) || (reinterpret_cast<uintptr_t>(p.out) & 15)) return false;
    if (g.H < 1 || g.W < 1 || (long)g.H * g.W > GR_MAX_PIXELS) return false;
    return g.t == 1 && p.R >= 1 && p.R <= RW_MAX_R;
}

// floor(sqrt(v)) for v < 2^24: v is exact as a float and its correctly rounded root is off by at most one, which the two loops mend.
SRH_GR_HD uint32_t rw_isqrt(uint32_t v) {
    uint32_t q = (uint32_t)__builtin_sqrtf((float)v);
    while (q * q > v) --q;
    while ((q + 1u) * (q + 1u) <= v) ++q;
    return q;
}

struct RwAcc { uint32_t n = 0u, n_in = 0u, s_q = 0u, n_cap = 0u, d2_min = 0xFFFFFFFFu, d2_max = 0u; };

// Pixel (y, x) of the edge's row span, inside the clipped box: the ONLY read of d2 of the launch.
SRH_GR_HD void rw_edge_pixel(const EdgeWidthParams& p, const GrEdge& ed, int y, int x, RwAcc& a) {
    if (!gr_covered(ed, y, x)) return;
    const uint32_t d = p.d2[(long)y * p.g.W + x];
    a.n += 1u; a.n_in += d > 0u; a.s_q += rw_isqrt(d << 8); a.n_cap += d == (uint32_t)(p.R * p.R);
    if (d > 0u && d < a.d2_min) a.d2_min = d;
    if (d > a.d2_max) a.d2_max = d;
}

// The edge's 32 bytes: the ONLY writes of the launch, two 16-byte stores.
SRH_GR_HD void rw_edge_store(const EdgeWidthParams& p, long e, const RwAcc& a) {
    *reinterpret_cast<GrWords*>(p.out + 8 * e) = GrWords{{a.n, a.n_in, a.s_q, a.n_cap}};
    *reinterpret_cast<GrWords*>(p.out + 8 * e + 4) = GrWords{{a.n_in ? a.d2_min : 0u, a.d2_max, 0u, 0u}};
}

}  // namespace srh
