// Validity mask from the polygons of an area of interest (scene_aoi.hip, config key SCENE_AOI): the parameters and the work of
// ONE item of every phase of a workgroup of the fill launch, free of HIP so that a CPU program can run the kernel's own addressing and
// arithmetic over every item of a launch (tests/scene_aoi_check.cpp, under the host sanitizers) before a GPU does.
//
// A workgroup owns a row y and walks it in column segments of AOI_SEG pixels; a segment is AOI_WORDS 32-bit words of one bit per pixel in
// the LDS.  Per polygon: the toggle row is cleared, the threads stride over the polygon's edges and XOR one bit per crossing edge at the
// column its toggling starts (an edge that starts left of the segment toggles the segment's first bit: that IS the parity carried in from
// the left, so a segment needs nothing from the one before it), a prefix XOR turns toggles into inside bits — five shift-XORs inside a
// word, then the words' parities, collected as AOI_WORDS bits, give every word its carry by a population count —, and the row is ORed into
// the include or the exclude accumulator.  At the end (include | none) & ~exclude is expanded to bytes.  XOR and OR commute, so the result
// does not depend on the order in which threads or edges arrive.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define SRH_AOI_HD __host__ __device__ __forceinline__
#else
#define SRH_AOI_HD inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define SRH_AOI_XOR(ptr, v) atomicXor((ptr), (v))          // LDS atomics: several edges may toggle bits of one word
#define SRH_AOI_OR(ptr, v) atomicOr((ptr), (v))
#else
#define SRH_AOI_XOR(ptr, v) (*(ptr) ^= (v))
#define SRH_AOI_OR(ptr, v) (*(ptr) |= (v))
#endif

namespace srh {

constexpr int AOI_THREADS = 256;
constexpr int AOI_SEG = 4096;                                      // pixels of a column segment
constexpr int AOI_WORDS = AOI_SEG / 32;                            // 128 words of one bit per pixel
constexpr int AOI_PAR_WORDS = AOI_WORDS / 32;                      // the words' parities, one bit each
constexpr int AOI_MAX_POLYGONS = 64;
constexpr int AOI_MAX_EDGES = 16384;
constexpr int AOI_MAX_COORD = 1 << 28;                             // 2^20 px in 1/256 px
constexpr long AOI_MAX_PIXELS = 2147483647L;
constexpr int AOI_FRAC = 256, AOI_HALF = 128;
static_assert(AOI_WORDS <= AOI_THREADS && AOI_WORDS % 32 == 0, "one word per thread, whole parity words");

struct alignas(16) AoiEdge { int32_t y0, x0, y1, x1; };            // 1/256 px, y0 < y1: a row of the table, one 16-byte load
struct alignas(16) AoiWords { uint32_t w[4]; };

struct AoiLds {                                                    // 1552 bytes, whatever W is
    uint32_t tog[AOI_WORDS];                                       // toggles -> inside bits of the current polygon; at the end the result
    uint32_t inc[AOI_WORDS];                                       // OR over the include polygons
    uint32_t exc[AOI_WORDS];                                       // OR over the exclude polygons
    uint32_t par[AOI_PAR_WORDS];                                   // bit t: the parity of word t
};
constexpr int AOI_LDS_BYTES = (3 * AOI_WORDS + AOI_PAR_WORDS) * 4;
static_assert(sizeof(AoiLds) == AOI_LDS_BYTES, "the stated LDS size");

// out[y W + x] = (invert ? !aoi : aoi) & (and_with ? and_with[y W + x] != 0 : 1), a u8 0 / 1.
struct SceneAoiParams {
    const int32_t* edges = nullptr;      // [E, 4] {y0, x0, y1, x1}, 16-byte aligned
    const int32_t* polys = nullptr;      // [n_include + n_exclude + 1]: polygon k owns edges polys[k] .. polys[k + 1]
    const uint8_t* and_with = nullptr;   // u8 [H, W], or nullptr
    uint8_t* out = nullptr;              // u8 [H, W], any byte address
    int n_include = 0, n_exclude = 0;    // 0 include polygons: the whole scene is inside
    int H = 0, W = 0;
    int invert = 0;
};

inline bool aoi_params_ok(const SceneAoiParams& p) {
    if (!p.edges || !p.polys || !p.out || (reinterpret_cast<uintptr_t>(p.edges) & 15)) return false;
    if (p.H < 1 || p.W < 1 || (long)p.H * p.W > AOI_MAX_PIXELS) return false;
    if (p.n_include < 0 || p.n_exclude < 0 || p.n_include + p.n_exclude > AOI_MAX_POLYGONS) return false;
    return p.invert == 0 || p.invert == 1;
}

// The tables on the HOST, checked before a launch: the offsets are a running sum from 0 to at most AOI_MAX_EDGES, every edge has y0 < y1
// and coordinates within +- 2^28.
inline bool aoi_table_ok(const int32_t* edges, const int32_t* polys, int n_include, int n_exclude) {
    if (!edges || !polys || n_include < 0 || n_exclude < 0 || n_include > AOI_MAX_POLYGONS || n_exclude > AOI_MAX_POLYGONS) return false;
    const int n = n_include + n_exclude;
    if (n > AOI_MAX_POLYGONS || polys[0] != 0) return false;
    for (int k = 0; k < n; ++k)
        if (polys[k + 1] < polys[k] || polys[k + 1] > AOI_MAX_EDGES) return false;
    for (int e = 0; e < polys[n]; ++e) {
        const int32_t* r = edges + 4L * e;
        if (r[0] >= r[2]) return false;
        for (int k = 0; k < 4; ++k)
            if (r[k] < -AOI_MAX_COORD || r[k] > AOI_MAX_COORD) return false;
    }
    return true;
}

SRH_AOI_HD int aoi_seg_pixels(const SceneAoiParams& p, long x0) { return p.W - x0 < AOI_SEG ? (int)(p.W - x0) : AOI_SEG; }

// Start of a segment, item t (0 <= t < AOI_THREADS): both accumulators empty.
SRH_AOI_HD void aoi_begin_item(AoiLds& l, int t) {
    if (t < AOI_WORDS) l.inc[t] = l.exc[t] = 0u;
}

// Start of a polygon, item t: no toggles, no parities.
SRH_AOI_HD void aoi_clear_item(AoiLds& l, int t) {
    if (t < AOI_WORDS) l.tog[t] = 0u;
    if (t < AOI_PAR_WORDS) l.par[t] = 0u;
}

// Edge e of the table against row y in the segment that starts at column x0.  The row test comes first, so the products stay below 2^59:
// |x0 - 128| <= 2^28 + 128, dy <= 2^29, 0 <= yc - y0 < dy, |dx| <= 2^29.  j = ceil(num / den), den > 0, from one truncating division.
SRH_AOI_HD void aoi_edge_item(const SceneAoiParams& p, AoiLds& l, long y, long x0, int e) {
    const AoiEdge ed = *reinterpret_cast<const AoiEdge*>(p.edges + 4L * e);
    const long yc = AOI_FRAC * y + AOI_HALF;
    if (yc < ed.y0 || yc >= ed.y1) return;
    const long dy = (long)ed.y1 - ed.y0, dx = (long)ed.x1 - ed.x0;
    const long num = ((long)ed.x0 - AOI_HALF) * dy + (yc - ed.y0) * dx, den = AOI_FRAC * dy;
    long j = num / den;
    if (num - j * den > 0) ++j;
    if (j >= x0 + aoi_seg_pixels(p, x0)) return;                   // the toggling starts right of the segment (or of the scene)
    const int jj = j <= x0 ? 0 : (int)(j - x0);                    // left of it: the whole segment is toggled
    SRH_AOI_XOR(&l.tog[jj >> 5], 1u << (jj & 31));
}

// Prefix XOR inside word t, and its parity (the word's last bit) into the parity bits.
SRH_AOI_HD void aoi_scan_item(AoiLds& l, int t) {
    if (t >= AOI_WORDS) return;
    uint32_t w = l.tog[t];
    w ^= w << 1; w ^= w << 2; w ^= w << 4; w ^= w << 8; w ^= w << 16;
    l.tog[t] = w;
    if (w >> 31) SRH_AOI_OR(&l.par[t >> 5], 1u << (t & 31));
}

// Word t with the parity of all words in front of it carried in, ORed into the include (or exclude) accumulator.
SRH_AOI_HD void aoi_fold_item(AoiLds& l, int t, bool include) {
    if (t >= AOI_WORDS) return;
    int carry = __builtin_popcount(l.par[t >> 5] & ((1u << (t & 31)) - 1u));
    for (int k = 0; k < (t >> 5); ++k) carry += __builtin_popcount(l.par[k]);
    const uint32_t w = (carry & 1) ? ~l.tog[t] : l.tog[t];
    if (include) l.inc[t] |= w;
    else l.exc[t] |= w;
}

// The result bits of word t, into tog: (include, or everything without include polygons) & ~exclude, inverted if asked.
SRH_AOI_HD void aoi_final_item(const SceneAoiParams& p, AoiLds& l, int t) {
    if (t >= AOI_WORDS) return;
    const uint32_t f = (p.n_include ? l.inc[t] : ~0u) & ~l.exc[t];
    l.tog[t] = p.invert ? ~f : f;
}

// The 16-byte chunks OF THE ADDRESS that hold the segment's n output bytes, the first of them starting `mis` bytes in front of it.
SRH_AOI_HD int aoi_store_chunks(const SceneAoiParams& p, long y, long x0) {
    const int mis = (int)(reinterpret_cast<uintptr_t>(p.out + y * p.W + x0) & 15);
    return (mis + aoi_seg_pixels(p, x0) + 15) >> 4;
}

// Chunk c (0 <= c < aoi_store_chunks): a chunk that lies inside the segment's bytes is one 16-byte store, of a chunk that reaches outside
// (the ragged ends) only the segment's own bytes are stored, one at a time.  The ONLY write, and the only read of and_with: bounded by W.
SRH_AOI_HD void aoi_store_item(const SceneAoiParams& p, const AoiLds& l, long y, long x0, int c) {
    const long at = y * p.W + x0;
    uint8_t* base = p.out + at;
    const int n = aoi_seg_pixels(p, x0);
    const int first = c * 16 - (int)(reinterpret_cast<uintptr_t>(base) & 15);
    if (first >= 0 && first + 16 <= n) {
        uint32_t bits = l.tog[first >> 5] >> (first & 31);
        if ((first & 31) > 16) bits |= l.tog[(first >> 5) + 1] << (32 - (first & 31));      // first + 15 lies in the next word: it exists
        AoiWords v;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t nib = (bits >> (4 * q)) & 15u;
            v.w[q] = (nib & 1u) | ((nib & 2u) << 7) | ((nib & 4u) << 14) | ((nib & 8u) << 21);
        }
        if (p.and_with) {
            const uint8_t* a = p.and_with + at + first;
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if (a[k] == 0) v.w[k >> 2] &= ~(0xffu << (8 * (k & 3)));
        }
        *reinterpret_cast<AoiWords*>(base + first) = v;
    } else {
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int col = first + k;
            if (col < 0 || col >= n) continue;
            uint8_t b = (uint8_t)((l.tog[col >> 5] >> (col & 31)) & 1u);
            if (p.and_with && p.and_with[at + col] == 0) b = 0;
            base[col] = b;
        }
    }
}

}  // namespace srh
