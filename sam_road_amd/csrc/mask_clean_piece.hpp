// Connected-component filter of the scene masks (mask_clean.hip, config key MASK_CLEAN): the parameters and the work of
// ONE item of each of the five launches, free of HIP so that a CPU program can run the kernels' own code over every item, in any order
// (tests/mask_clean_check.cpp, under the host sanitizers), before a GPU does.  The atomic operations are a template parameter `A`:
//   A::load(p) / store    an atomic load / store: every access to the three workspaces goes through A, in every launch.  Inside the merge
//                         launch a load may return a value that another workgroup has replaced since; mc_find and mc_union are written
//                         for that.  Behind it nothing that is loaded changes any more
//   A::min / add / max    atomicMin / atomicAdd / atomicMax on an int32, returning the old value
// mask_clean.hip supplies the device's, the CPU program serial ones.
//
// The work is cut into SEGMENTS: 64 consecutive pixels of one image row, columns 64 j .. 64 j + 63 (fewer at the row's end).  A segment is
// one wave; lane l owns pixel x0 + l.  What the lanes of a segment share is the 64-bit foreground word of the segment (bit l: pixel
// x0 + l is foreground) — a ballot on the device, a loop on the CPU — so the per-lane code below takes such words and never talks to
// another lane.  A pixel's workspace index is BASE + y W + x; parents only ever point at a smaller or equal index of the same image.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define SRH_MC_HD __host__ __device__ __forceinline__
#else
#define SRH_MC_HD inline
#endif

namespace srh {

// One row of the table per image, eight int64.  OFF: byte offset of the image's dense H x W block in the buffer.  T_ON (0 .. 256): a
// pixel is foreground iff its level is >= T_ON.  MIN_AREA (>= 1), T_PEAK (0 .. 256): a component stays iff its area is >= MIN_AREA and
// its highest level is >= T_PEAK.  BASE: workspace index of the image's first pixel = the sum of H W over the rows before it.  SEG0:
// number of the image's first segment = the sum of H ceil(W / 64) over the rows before it.
constexpr int MC_COLS = 8;
constexpr int MC_OFF = 0, MC_H = 1, MC_W = 2, MC_T_ON = 3, MC_MIN_AREA = 4, MC_T_PEAK = 5, MC_BASE = 6, MC_SEG0 = 7;
constexpr int MC_SEG = 64;                  // pixels per segment = lanes per wave
constexpr int MC_THREADS = 256;             // a workgroup takes four consecutive segments
constexpr int MC_MAX_IMAGES = 4096;           // the host check compares every pair of blocks

struct MaskCleanParams {
    uint8_t* buf = nullptr;                 // the images, filtered in place
    const int64_t* table = nullptr;         // [n, MC_COLS]
    int n = 0;
    int conn = 8;                           // 8 or 4
    int32_t* parent = nullptr;              // [sum H W]: -1 on background; parent, then (from the third launch on) the root = the label
    int32_t* area = nullptr;                // [sum H W]: at a root, the pixels of its component
    int32_t* peak = nullptr;                // [sum H W]: at a root, the highest level of its component
    long n_segs = 0;                        // the sum of H ceil(W / 64)
};

SRH_MC_HD long mc_segs_per_row(long W) { return (W + MC_SEG - 1) / MC_SEG; }

// What the 64 lanes of one segment share.
struct McSeg {
    uint8_t* img;                           // the image's first byte
    int H, W, y, x0;                        // the segment: pixels (y, x0 .. x0 + lanes - 1)
    int lanes;                              // min(64, W - x0)
    int g0;                                 // workspace index of pixel (y, x0)
    int t_on, t_peak;
    int64_t min_area;
};

// Segment s (0 <= s < n_segs): its image is the last one whose SEG0 is <= s.
SRH_MC_HD McSeg mc_locate(const MaskCleanParams& p, long s) {
    int lo = 0, hi = p.n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (p.table[(long)mid * MC_COLS + MC_SEG0] <= s) lo = mid; else hi = mid - 1;
    }
    const int64_t* t = p.table + (long)lo * MC_COLS;
    McSeg g;
    g.img = p.buf + t[MC_OFF];
    g.H = (int)t[MC_H]; g.W = (int)t[MC_W];
    const long spr = mc_segs_per_row(g.W), local = s - t[MC_SEG0];
    g.y = (int)(local / spr);
    g.x0 = (int)(local - (long)g.y * spr) * MC_SEG;
    g.lanes = g.W - g.x0 < MC_SEG ? g.W - g.x0 : MC_SEG;
    g.g0 = (int)(t[MC_BASE] + (long)g.y * g.W + g.x0);
    g.t_on = (int)t[MC_T_ON]; g.t_peak = (int)t[MC_T_PEAK]; g.min_area = t[MC_MIN_AREA];
    return g;
}

// Is pixel (y, x) of the segment's image foreground?  Outside the image: no.  The ONLY way a neighbour is read: bounded by H and W.
SRH_MC_HD bool mc_fg(const McSeg& g, int y, int x) {
    if (y < 0 || y >= g.H || x < 0 || x >= g.W) return false;
    return (int)g.img[(long)y * g.W + x] >= g.t_on;
}

// ---- the union-find in global memory ------------------------------------------------------------------------------------------------
// Invariant: every value ever stored at parent[i] of a foreground pixel i is a foreground pixel of the same image with index <= i, and it
// only ever decreases (the stores are the initialisation and atomicMin).  So a walk along parents strictly descends and ends at an i
// with parent[i] == i, whatever other workgroups do meanwhile, and no value read — however old — leads outside the image.
template <class A>
SRH_MC_HD int mc_find(int32_t* parent, int i) {
    while (true) {
        const int q = A::load(parent + i);
        if ((unsigned)q >= (unsigned)i) return i;       // a root (q == i); q > i or q < 0 cannot be stored and only end the walk
        i = q;
    }
}

// a and b end up in one tree.  Find both roots, hang the larger below the smaller with atomicMin; if the larger was no root any more
// (old != a: somebody linked it meanwhile, and the atomicMin may have replaced that link) go on with what it pointed at, so that no
// equivalence is lost.  The larger of the pair strictly decreases with every retry: at most `max(a, b) - BASE` of them.
// There is NO path compression: a version that, after a union, pointed the nodes of both chains at the new root (atomicMin) lost, rarely,
// the link of a small fragment on the device (what was seen and how it was separated); the textbook form below did not.
template <class A>
SRH_MC_HD void mc_union(int32_t* parent, int a, int b) {
    while (true) {
        a = mc_find<A>(parent, a);
        b = mc_find<A>(parent, b);
        if (a == b) break;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = A::min(parent + a, b);
        if (old == a) break;
        a = old;
    }
}

// ---- launch 1, init: a foreground pixel's parent is the first pixel of its run inside the segment; statistics zeroed ---------------------
template <class A>
SRH_MC_HD void mc_init_lane(const MaskCleanParams& p, const McSeg& g, int lane, uint64_t cur) {
    if (lane >= g.lanes) return;
    const int i = g.g0 + lane;
    int q = -1;
    if ((cur >> lane) & 1) {
        const uint64_t gaps = ~cur & ((1ull << lane) - 1);             // background below the lane
        q = g.g0 + (gaps ? 64 - __builtin_clzll(gaps) : 0);            // one past the highest of them
    }
    A::store(p.parent + i, q);
    A::store(p.area + i, 0);
    A::store(p.peak + i, 0);
}

// ---- launch 2, merge ------------------------------------------------------------------------------------------------------------------------
// cur / up: the foreground words of the segment and of the same columns one row up (0 for row 0).  up_l, up_r, left: pixels
// (y - 1, x0 - 1), (y - 1, x0 + 64), (y, x0 - 1).  A pixel is united with the pixel above it only where that is not already implied: at
// the start of its run inside the segment, or where the pixel above-left is background (otherwise its left neighbour, in the same run,
// is united with the pixel above-left by the same rule, and that one touches the pixel above).  With 8-connectivity and background
// above, it is united with the foreground pixels above-left and above-right.  Lane 0 is united with a foreground left neighbour.
template <class A>
SRH_MC_HD void mc_merge_lane(const MaskCleanParams& p, const McSeg& g, int lane, uint64_t cur, uint64_t up, bool up_l, bool up_r, bool left) {
    if (lane >= g.lanes || !((cur >> lane) & 1)) return;
    const int i = g.g0 + lane;
    if (lane == 0 && left) mc_union<A>(p.parent, i, i - 1);
    if (g.y == 0) return;
    const int iu = i - g.W;
    const bool run_start = lane == 0 || !((cur >> (lane - 1)) & 1);
    const bool U = (up >> lane) & 1;
    const bool UL = lane ? (up >> (lane - 1)) & 1 : up_l;
    const bool UR = lane < MC_SEG - 1 ? (up >> (lane + 1)) & 1 : up_r;
    if (U) {
        if (run_start || !UL) mc_union<A>(p.parent, i, iu);
    } else if (p.conn == 8) {
        if (UL) mc_union<A>(p.parent, i, iu - 1);
        if (UR) mc_union<A>(p.parent, i, iu + 1);
    }
}

// ---- launch 3, flatten: every foreground pixel stores its root as its label (the parents of the roots no longer change) ------------------
template <class A>
SRH_MC_HD void mc_flatten_lane(const MaskCleanParams& p, const McSeg& g, int lane, uint64_t cur) {
    if (lane >= g.lanes || !((cur >> lane) & 1)) return;
    const int i = g.g0 + lane;
    A::store(p.parent + i, mc_find<A>(p.parent, i));
}

// ---- launch 4, statistics: ONE atomicAdd (area) and ONE atomicMax (peak) per label and segment.  The work is done by the first pixel of
// the first run of the segment that carries the label: it reads the labels of the segment's other run starts (stored by launch 3), adds up
// the lengths of the runs with its own label (from the foreground word) and takes the highest of their levels.  With one atomic pair per
// RUN, a component that spans the mask serialised a million atomics on one address (DESIGN.md §6k has the measurement) -------------------
template <class A>
SRH_MC_HD void mc_stats_lane(const MaskCleanParams& p, const McSeg& g, int lane, uint64_t cur) {
    if (lane >= g.lanes || !((cur >> lane) & 1) || (lane && ((cur >> (lane - 1)) & 1))) return;      // run starts only
    const int r = A::load(p.parent + g.g0 + lane);
    const uint64_t starts = cur & ~(cur << 1);
    for (uint64_t lower = starts & ((1ull << lane) - 1); lower; lower &= lower - 1)
        if (A::load(p.parent + g.g0 + __builtin_ctzll(lower)) == r) return;                                  // an earlier run has this label: its work
    const uint8_t* row = g.img + (long)g.y * g.W + g.x0;
    int area = 0, top = 0;
    for (uint64_t rest = starts >> lane << lane; rest; rest &= rest - 1) {
        const int j = __builtin_ctzll(rest);
        if (j != lane && A::load(p.parent + g.g0 + j) != r) continue;
        const uint64_t gap = ~(cur >> j);
        const int len = gap ? __builtin_ctzll(gap) : MC_SEG - j;
        for (int k = j; k < j + len; ++k) top = row[k] > top ? row[k] : top;
        area += len;
    }
    A::add(p.area + r, area);
    A::max(p.peak + r, top);
}

// ---- launch 5, apply: the runs of a label that fails the test become 0.  As in launch 4 the first run of the segment that carries the
// label does the work for the segment, so area and peak of a root are read once per segment and label, not once per pixel ----------------
template <class A>
SRH_MC_HD void mc_apply_lane(const MaskCleanParams& p, const McSeg& g, int lane, uint64_t cur) {
    if (lane >= g.lanes || !((cur >> lane) & 1) || (lane && ((cur >> (lane - 1)) & 1))) return;      // run starts only
    const int r = A::load(p.parent + g.g0 + lane);
    const uint64_t starts = cur & ~(cur << 1);
    for (uint64_t lower = starts & ((1ull << lane) - 1); lower; lower &= lower - 1)
        if (A::load(p.parent + g.g0 + __builtin_ctzll(lower)) == r) return;
    if ((int64_t)A::load(p.area + r) >= g.min_area && A::load(p.peak + r) >= g.t_peak) return;
    uint8_t* row = g.img + (long)g.y * g.W + g.x0;
    for (uint64_t rest = starts >> lane << lane; rest; rest &= rest - 1) {
        const int j = __builtin_ctzll(rest);
        if (j != lane && A::load(p.parent + g.g0 + j) != r) continue;
        const uint64_t gap = ~(cur >> j);
        const int len = gap ? __builtin_ctzll(gap) : MC_SEG - j;
        for (int k = j; k < j + len; ++k) row[k] = 0;
    }
}

// The table on the HOST, checked before a launch: every block inside the buffer, no two blocks overlapping, BASE and SEG0 the running
// sums, the thresholds in range, and at most 2^31 - 1 pixels in all (workspace indices are int32).
inline bool mask_clean_table_ok(const int64_t* t, int n, long long bytes, long long ws_pixels) {
    if (!t || n < 1 || n > MC_MAX_IMAGES || bytes < 1) return false;
    long long base = 0, seg0 = 0;
    for (int k = 0; k < n; ++k) {
        const int64_t* r = t + (long)k * MC_COLS;
        const long long H = r[MC_H], W = r[MC_W];
        if (H < 1 || W < 1 || H > 2147483647LL || W > 2147483647LL || H * W > 2147483647LL) return false;
        if (r[MC_OFF] < 0 || r[MC_OFF] > bytes - H * W) return false;
        if (r[MC_T_ON] < 0 || r[MC_T_ON] > 256 || r[MC_T_PEAK] < 0 || r[MC_T_PEAK] > 256 || r[MC_MIN_AREA] < 1) return false;
        if (r[MC_BASE] != base || r[MC_SEG0] != seg0) return false;
        base += H * W;
        seg0 += H * mc_segs_per_row(W);
        if (base > 2147483647LL) return false;
        for (int j = 0; j < k; ++j) {                            // n is small: the two masks of a scene, or of the scenes of a group
            const int64_t* q = t + (long)j * MC_COLS;
            if (r[MC_OFF] < q[MC_OFF] + q[MC_H] * q[MC_W] && q[MC_OFF] < r[MC_OFF] + H * W) return false;
        }
    }
    return base <= ws_pixels;
}

inline long mask_clean_segs(const int64_t* t, int n) {
    const int64_t* r = t + (long)(n - 1) * MC_COLS;
    return (long)(r[MC_SEG0] + r[MC_H] * mc_segs_per_row(r[MC_W]));
}

}  // namespace srh
