// The graph as a raster (graph_raster.hip, config key GRAPH_RASTER): the parameters and the work of ONE item of every launch,
// free of HIP so that a CPU program can run the kernels' own addressing and arithmetic over every item of a launch
// (tests/graph_raster_check.cpp, under the host sanitizers) before a GPU does.  The rule is stated on the host
// (sam_road_amd/graph_raster.py) in integers, and the class map must equal graph_raster_ref byte for byte.
//
// Three launches make the class map: the map is cleared in 16-byte chunks of the ADDRESS; a wave owns an edge and walks the rows of its
// grown, clipped bounding box, lanes across the columns of the part of the row the segment can reach, and stores the edge byte where the
// rule holds; a wave owns a node and stores the node byte over its mark.  Every writer of a launch stores the same byte and the launches
// are ordered by the stream, so the result does not depend on scheduling.
//
// The 64-bit bound.  An edge's span is at most S = GR_MAX_SPAN = 16383 per axis, a pixel of its box grown by g = ceil(t / 2) <= 128 has
// |p| <= S + g = 16511 per axis.  Then |u| = |p . d| and |p x d| are at most 2 S (S + g) = 540 999 426 < 2^30, L = d . d <= 2 S^2 < 2^29,
// p . p <= 2 (S + g)^2 < 2^30, and the largest products of the rule are 4 (p x d)^2 < 2^62 and t^2 L < 2^45: inside a signed 64-bit
// integer.  Coordinates lie within +-2^28, so every sum of two of them and g fits an int.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define SRH_GR_HD __host__ __device__ __forceinline__
#else
#define SRH_GR_HD inline
#endif
#define GR_UNROLL _Pragma("unroll")                               // constant trip counts: the quads' bytes stay in registers

namespace srh {

constexpr int GR_THREADS = 256, GR_WAVE = 64;
constexpr int GR_WAVES = GR_THREADS / GR_WAVE;                     // edges (nodes) a workgroup works on at a time
constexpr int GR_MAX_SPAN = 16383;                                 // |b - a| per axis
constexpr int GR_MAX_COORD = 1 << 28;
constexpr int GR_MAX_WIDTH = 255, GR_MAX_RADIUS = 127;
constexpr long GR_MAX_PIXELS = 2147483647L;
constexpr int GR_MARK_NONE = 0, GR_MARK_SQUARE = 1, GR_MARK_DISC = 2;

struct alignas(16) GrWords { uint32_t w[4]; };

// out[y W + x] = node_value on a node mark, else edge_value on an edge, else 0.
struct GraphRasterParams {
    const int32_t* nodes = nullptr;      // [N, 2] (row, col), 4-byte aligned
    const int32_t* edges = nullptr;      // [E, 2] indices into nodes
    uint8_t* out = nullptr;              // u8 [H, W], any byte address
    int N = 0, E = 0, H = 0, W = 0;
    int t = 1;                           // the width of an edge, 1 .. 255
    int mark = GR_MARK_NONE, r = 0;      // the node mark and its radius, 0 .. 127
    int edge_value = 1, node_value = 2;  // 1 .. 255
};

inline bool gr_params_ok(const GraphRasterParams& p) {
    if (!p.out || p.N < 0 || p.E < 0 || (p.N > 0 && !p.nodes) || (p.E > 0 && (!p.edges || p.N == 0))) return false;
    if ((reinterpret_cast<uintptr_t>(p.nodes) | reinterpret_cast<uintptr_t>(p.edges)) & 3) return false;
    if (p.H < 1 || p.W < 1 || (long)p.H * p.W > GR_MAX_PIXELS) return false;
    if (p.t < 1 || p.t > GR_MAX_WIDTH || p.mark < GR_MARK_NONE || p.mark > GR_MARK_DISC || p.r < 0 || p.r > GR_MAX_RADIUS) return false;
    return p.edge_value >= 1 && p.edge_value <= 255 && p.node_value >= 1 && p.node_value <= 255;
}

// The tables on the HOST, checked before a launch: coordinates within +-2^28, edge indices in [0, N), spans of at most GR_MAX_SPAN per axis.
inline bool gr_tables_ok(const int32_t* nodes, int N, const int32_t* edges, int E) {
    if (N < 0 || E < 0 || (N > 0 && !nodes) || (E > 0 && !edges)) return false;
    for (long k = 0; k < 2L * N; ++k)
        if (nodes[k] < -GR_MAX_COORD || nodes[k] > GR_MAX_COORD) return false;
    for (long e = 0; e < E; ++e) {
        const int32_t a = edges[2 * e], b = edges[2 * e + 1];
        if (a < 0 || a >= N || b < 0 || b >= N) return false;
        for (int k = 0; k < 2; ++k) {
            const long d = (long)nodes[2L * b + k] - nodes[2L * a + k];
            if (d < -GR_MAX_SPAN || d > GR_MAX_SPAN) return false;
        }
    }
    return true;
}

// ---- clear -------------------------------------------------------------------------------------------------------------------------------
// The 16-byte chunks OF THE ADDRESS that hold the map's bytes, the first of them starting `mis` bytes in front of it.
SRH_GR_HD long gr_clear_chunks(const GraphRasterParams& p) {
    const long mis = (long)(reinterpret_cast<uintptr_t>(p.out) & 15);
    return (mis + (long)p.H * p.W + 15) >> 4;
}

// Chunk c: one 16-byte store if it lies inside the map, its own bytes one at a time at the ragged ends.
SRH_GR_HD void gr_clear_item(const GraphRasterParams& p, long c) {
    const long n = (long)p.H * p.W;
    const long first = c * 16 - (long)(reinterpret_cast<uintptr_t>(p.out) & 15);
    if (first >= 0 && first + 16 <= n) {
        *reinterpret_cast<GrWords*>(p.out + first) = GrWords{{0u, 0u, 0u, 0u}};
    } else {
        for (int k = 0; k < 16; ++k)
            if (first + k >= 0 && first + k < n) p.out[first + k] = 0;
    }
}

// ---- edges -------------------------------------------------------------------------------------------------------------------------------
struct GrEdge {
    int ar, ac, dr, dc;                  // a and d = b - a
    int g;                               // ceil(t / 2)
    int y0, y1, x0, x1;                  // the bounding box grown by g, clipped to the image; empty iff y0 > y1 or x0 > x1
    long L, tt;                          // d . d and t^2
};

SRH_GR_HD int gr_min(int a, int b) { return a < b ? a : b; }
SRH_GR_HD int gr_max(int a, int b) { return a > b ? a : b; }

SRH_GR_HD GrEdge gr_edge_load(const GraphRasterParams& p, long e) {
    const int32_t ia = p.edges[2 * e], ib = p.edges[2 * e + 1];
    GrEdge ed;
    ed.ar = p.nodes[2L * ia]; ed.ac = p.nodes[2L * ia + 1];
    const int br = p.nodes[2L * ib], bc = p.nodes[2L * ib + 1];
    ed.dr = br - ed.ar; ed.dc = bc - ed.ac;
    ed.g = (p.t + 1) >> 1;
    ed.y0 = gr_max(gr_min(ed.ar, br) - ed.g, 0); ed.y1 = gr_min(gr_max(ed.ar, br) + ed.g, p.H - 1);
    ed.x0 = gr_max(gr_min(ed.ac, bc) - ed.g, 0); ed.x1 = gr_min(gr_max(ed.ac, bc) + ed.g, p.W - 1);
    ed.L = (long)ed.dr * ed.dr + (long)ed.dc * ed.dc;
    ed.tt = (long)p.t * p.t;
    return ed;
}

// The columns of row y (y0 <= y <= y1) that the edge can cover: a covered pixel is within g of a point of the segment whose row lies
// within g of y, and the segment's column is monotone in its row, so it lies between the columns at the two ends of that row range; the
// truncating divisions are off by less than 1 each, hence the margin of 1.  A horizontal edge keeps the box.
SRH_GR_HD void gr_edge_row(const GrEdge& ed, int y, int& xlo, int& xhi) {
    xlo = ed.x0; xhi = ed.x1;
    if (ed.dr == 0) return;
    const int br = ed.ar + ed.dr;
    const int r1 = gr_max(y - ed.g, gr_min(ed.ar, br)), r2 = gr_min(y + ed.g, gr_max(ed.ar, br));
    const int c1 = ed.ac + ed.dc * (r1 - ed.ar) / ed.dr, c2 = ed.ac + ed.dc * (r2 - ed.ar) / ed.dr;      // |dc (r - ar)| <= S^2 < 2^31
    xlo = gr_max(xlo, gr_min(c1, c2) - 1 - ed.g);
    xhi = gr_min(xhi, gr_max(c1, c2) + 1 + ed.g);
}

// The rule: is the pixel at (y, x) within t / 2 of the segment?  (y, x) lies in the edge's grown box.
SRH_GR_HD bool gr_covered(const GrEdge& ed, int y, int x) {
    const long pr = y - ed.ar, pc = x - ed.ac;
    const long u = pr * ed.dr + pc * ed.dc;
    if (ed.L == 0 || u <= 0) return 4 * (pr * pr + pc * pc) <= ed.tt;
    if (u >= ed.L) {
        const long qr = pr - ed.dr, qc = pc - ed.dc;
        return 4 * (qr * qr + qc * qc) <= ed.tt;
    }
    const long cr = pr * ed.dc - pc * ed.dr;
    return 4 * cr * cr <= ed.tt * ed.L;
}

// Pixel (y, x) of the edge's row span: the ONLY write of the edge launch, inside the clipped box.
SRH_GR_HD void gr_edge_item(const GraphRasterParams& p, const GrEdge& ed, int y, int x) {
    if (gr_covered(ed, y, x)) p.out[(long)y * p.W + x] = (uint8_t)p.edge_value;
}

// ---- node marks --------------------------------------------------------------------------------------------------------------------------
struct GrNode { int ar, ac, y0, x0, bh, bw; };                     // the mark's box clipped to the image: bh x bw pixels from (y0, x0); bh or bw <= 0: empty

SRH_GR_HD GrNode gr_node_load(const GraphRasterParams& p, long n) {
    GrNode nd;
    nd.ar = p.nodes[2 * n]; nd.ac = p.nodes[2 * n + 1];
    nd.y0 = gr_max(nd.ar - p.r, 0); nd.x0 = gr_max(nd.ac - p.r, 0);
    nd.bh = gr_min(nd.ar + p.r, p.H - 1) - nd.y0 + 1;
    nd.bw = gr_min(nd.ac + p.r, p.W - 1) - nd.x0 + 1;
    if (nd.bh <= 0 || nd.bw <= 0) nd.bh = nd.bw = 0;
    return nd;
}

// Pixel k (0 <= k < bh bw) of the node's clipped box, row-major: the ONLY write of the node launch.
SRH_GR_HD void gr_node_item(const GraphRasterParams& p, const GrNode& nd, int k) {
    const int y = nd.y0 + k / nd.bw, x = nd.x0 + k % nd.bw;
    if (p.mark == GR_MARK_DISC) {
        const int pr = y - nd.ar, pc = x - nd.ac;
        if (pr * pr + pc * pc > p.r * p.r) return;
    }
    p.out[(long)y * p.W + x] = (uint8_t)p.node_value;
}

// ---- composite ---------------------------------------------------------------------------------------------------------------------------
// out[i] = colour[2] where cls[i] >= 2, colour[1] where cls[i] == 1, else img[i] (colour[0] without an image).  A colour is r | g << 8 | b << 16.
struct GraphCompositeParams {
    const uint8_t* cls = nullptr;        // u8 [n]
    const uint8_t* img = nullptr;        // u8 [n, 3] or nullptr
    uint8_t* out = nullptr;              // u8 [n, 3]
    long n = 0;
    uint32_t colour[3] = {0u, 0u, 0u};
};

inline bool gr_composite_ok(const GraphCompositeParams& p) {
    return p.cls && p.out && p.n >= 1 && p.n <= GR_MAX_PIXELS && !((p.colour[0] | p.colour[1] | p.colour[2]) >> 24);
}

SRH_GR_HD long gr_quads(long n) { return (n + 3) >> 2; }
// are four pixels of these pointers whole aligned words (1 word of classes, 3 of colours)?
SRH_GR_HD bool gr_words_ok(const void* a, const void* b, const void* c, const void* d, const void* e, const void* f) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) | reinterpret_cast<uintptr_t>(d) |
             reinterpret_cast<uintptr_t>(e) | reinterpret_cast<uintptr_t>(f)) & 3) == 0;
}

SRH_GR_HD void gr_put_rgb(uint8_t* px, uint32_t colour) {
    px[0] = (uint8_t)colour; px[1] = (uint8_t)(colour >> 8); px[2] = (uint8_t)(colour >> 16);
}

// Quad q: pixels 4 q .. 4 q + 3 (those below n).  A whole quad of word-aligned arrays moves as words, anything else as bytes.
SRH_GR_HD void gr_composite_item(const GraphCompositeParams& p, long q) {
    const long i0 = 4 * q;
    const int m = p.n - i0 < 4 ? (int)(p.n - i0) : 4;
    const bool words = m == 4 && gr_words_ok(p.cls, p.img, p.out, nullptr, nullptr, nullptr);
    union { uint32_t w; uint8_t b[4]; } c;
    union { uint32_t w[3]; uint8_t b[12]; } px;
    c.w = 0u;
    px.w[0] = px.w[1] = px.w[2] = 0u;
    if (words) {
        c.w = *reinterpret_cast<const uint32_t*>(p.cls + i0);
        if (p.img)
            for (int k = 0; k < 3; ++k) px.w[k] = reinterpret_cast<const uint32_t*>(p.img + 3 * i0)[k];
    } else {
        GR_UNROLL
        for (int k = 0; k < 4; ++k)
            if (k < m) c.b[k] = p.cls[i0 + k];
        if (p.img) {
            GR_UNROLL
            for (int k = 0; k < 12; ++k)
                if (k < 3 * m) px.b[k] = p.img[3 * i0 + k];
        }
    }
    GR_UNROLL
    for (int k = 0; k < 4; ++k) {
        if (k >= m) continue;
        if (c.b[k] >= 2) gr_put_rgb(px.b + 3 * k, p.colour[2]);
        else if (c.b[k] == 1) gr_put_rgb(px.b + 3 * k, p.colour[1]);
        else if (!p.img) gr_put_rgb(px.b + 3 * k, p.colour[0]);
    }
    if (words) {
        for (int k = 0; k < 3; ++k) reinterpret_cast<uint32_t*>(p.out + 3 * i0)[k] = px.w[k];
    } else {
        GR_UNROLL
        for (int k = 0; k < 12; ++k)
            if (k < 3 * m) p.out[3 * i0 + k] = px.b[k];
    }
}

// ---- compare -----------------------------------------------------------------------------------------------------------------------------
// Four class maps of one shape, compared over the pixels with valid != 0 (all of them without valid):
//   counts[0] n_pred   = #(pred_thin != 0)               counts[1] n_fp     = #(pred_thin != 0 & gt_wide == 0)
//   counts[2] n_gt     = #(gt_thin != 0)                 counts[3] n_missed = #(gt_thin != 0 & pred_wide == 0)
// diff (optional): img (black without one), red on a missed pixel, else blue on a false positive; pixels with valid == 0 are not painted.
constexpr uint32_t GR_RED = 255u, GR_BLUE = 255u << 16;

struct GraphCompareParams {
    const uint8_t* pred_thin = nullptr; const uint8_t* pred_wide = nullptr;
    const uint8_t* gt_thin = nullptr; const uint8_t* gt_wide = nullptr;      // u8 [n] each
    const uint8_t* valid = nullptr;      // u8 [n] or nullptr
    const uint8_t* img = nullptr;        // u8 [n, 3] or nullptr
    uint8_t* diff = nullptr;             // u8 [n, 3] or nullptr
    unsigned long long* counts = nullptr;  // [4], 8-byte aligned; zeroed by a launch of its own in front
    long n = 0;
};

inline bool gr_compare_ok(const GraphCompareParams& p) {
    if (!p.pred_thin || !p.pred_wide || !p.gt_thin || !p.gt_wide || !p.counts || (reinterpret_cast<uintptr_t>(p.counts) & 7)) return false;
    return p.n >= 1 && p.n <= GR_MAX_PIXELS;
}

// Quad q: adds its pixels to acc[4] (the thread's own counters) and writes its pixels of diff.
SRH_GR_HD void gr_compare_item(const GraphCompareParams& p, long q, uint32_t* acc) {
    const long i0 = 4 * q;
    const int m = p.n - i0 < 4 ? (int)(p.n - i0) : 4;
    const bool words = m == 4 && gr_words_ok(p.pred_thin, p.pred_wide, p.gt_thin, p.gt_wide, p.valid, nullptr) && gr_words_ok(p.img, p.diff, nullptr, nullptr, nullptr, nullptr);
    union Q { uint32_t w; uint8_t b[4]; } pt, pw, gt, gw, va;
    union { uint32_t w[3]; uint8_t b[12]; } px;
    pt.w = pw.w = gt.w = gw.w = 0u;
    va.w = 0x01010101u;
    px.w[0] = px.w[1] = px.w[2] = 0u;
    if (words) {
        pt.w = *reinterpret_cast<const uint32_t*>(p.pred_thin + i0); pw.w = *reinterpret_cast<const uint32_t*>(p.pred_wide + i0);
        gt.w = *reinterpret_cast<const uint32_t*>(p.gt_thin + i0); gw.w = *reinterpret_cast<const uint32_t*>(p.gt_wide + i0);
        if (p.valid) va.w = *reinterpret_cast<const uint32_t*>(p.valid + i0);
        if (p.img && p.diff)
            for (int k = 0; k < 3; ++k) px.w[k] = reinterpret_cast<const uint32_t*>(p.img + 3 * i0)[k];
    } else {
        GR_UNROLL
        for (int k = 0; k < 4; ++k) {
            if (k >= m) continue;
            pt.b[k] = p.pred_thin[i0 + k]; pw.b[k] = p.pred_wide[i0 + k]; gt.b[k] = p.gt_thin[i0 + k]; gw.b[k] = p.gt_wide[i0 + k];
            if (p.valid) va.b[k] = p.valid[i0 + k];
        }
        if (p.img && p.diff) {
            GR_UNROLL
            for (int k = 0; k < 12; ++k)
                if (k < 3 * m) px.b[k] = p.img[3 * i0 + k];
        }
    }
    GR_UNROLL
    for (int k = 0; k < 4; ++k) {
        if (k >= m || !va.b[k]) continue;
        const bool pred = pt.b[k] != 0, truth = gt.b[k] != 0;
        const bool fp = pred && gw.b[k] == 0, missed = truth && pw.b[k] == 0;
        acc[0] += pred; acc[1] += fp; acc[2] += truth; acc[3] += missed;
        if (missed) gr_put_rgb(px.b + 3 * k, GR_RED);
        else if (fp) gr_put_rgb(px.b + 3 * k, GR_BLUE);
    }
    if (!p.diff) return;
    if (words) {
        for (int k = 0; k < 3; ++k) reinterpret_cast<uint32_t*>(p.diff + 3 * i0)[k] = px.w[k];
    } else {
        GR_UNROLL
        for (int k = 0; k < 12; ++k)
            if (k < 3 * m) p.diff[3 * i0 + k] = px.b[k];
    }
}

}  // namespace srh
