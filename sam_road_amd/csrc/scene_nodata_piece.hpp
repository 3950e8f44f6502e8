// Validity mask from a nodata value (scene_nodata.hip, config key SCENE_NODATA): the parameters and the work of ONE item of
// the match launch and of the three phases of a workgroup of the grow launch, free of HIP so that a CPU program can run the kernels' own
// addressing over every item of a launch (tests/scene_nodata_check.cpp, under the host sanitizers) before a GPU does.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define SRH_ND_HD __host__ __device__ __forceinline__
#else
#define SRH_ND_HD inline
#endif

namespace srh {

constexpr int ND_THREADS = 256;
constexpr int ND_MAX_C = 16;
constexpr long ND_MAX_PIXELS = 2147483647L;
constexpr int ND_ALL = 0, ND_ANY = 1;                              // = SRH_NODATA_ALL / SRH_NODATA_ANY of include/samroad_hip.h

// ---- match ---------------------------------------------------------------------------------------------------------------------------------
// hit[i] = all / any over c of lo[c] <= src[i * C + c] <= hi[c], src u8 or u16 [n, C]; out[i] = (invert ? !hit : hit) & (and_with ?
// and_with[i] != 0 : 1), a u8 0 / 1.  The kernel knows nothing of H or W.  Offsets are 64-bit from the first product on: 16 bands *
// (2^31 - 1) pixels * 2 bytes does not fit 32 bits.
struct SceneNodataParams {
    const void* src = nullptr;
    const uint8_t* and_with = nullptr;   // u8 [n], or nullptr
    uint8_t* out = nullptr;              // u8 [n]
    long n = 0;                          // pixels
    int C = 3;                           // bands per source pixel, 1 .. ND_MAX_C
    int wide = 0;                        // 0: u8 source, 1: u16 source
    int any = 0;                         // ND_ALL / ND_ANY
    int invert = 0;
    uint32_t lohi[ND_MAX_C] = {};        // band c: lo in bits 0..15, hi in bits 16..31 (lo > hi: the band never hits)
};

struct alignas(16) NdWords { uint32_t w[4]; };

inline bool nodata_params_ok(const SceneNodataParams& p) {
    if (!p.src || !p.out || p.n < 1 || p.n > ND_MAX_PIXELS || p.C < 1 || p.C > ND_MAX_C) return false;
    if ((p.wide != 0 && p.wide != 1) || (p.any != ND_ALL && p.any != ND_ANY) || (p.invert != 0 && p.invert != 1)) return false;
    return !p.wide || (reinterpret_cast<uintptr_t>(p.src) & 1) == 0;
}

SRH_ND_HD long nodata_items(const SceneNodataParams& p) { return (p.n + 3) >> 2; }

// Item i (0 <= i < nodata_items): pixels 4 i .. 4 i + 3 (fewer at the end).  Their 4 C elements are one contiguous byte range of the
// source; it is read in the 16-byte chunks of the ADDRESS that hold it.  A chunk that lies between the first and the last 16-byte boundary
// inside the source is one 16-byte load; of a chunk that reaches outside (the head and the tail of the buffer) only the item's own
// elements are loaded, one at a time.  Neighbouring items share the chunk their border falls into: it comes from memory once and from the
// cache after that.  The four results are stored as one word where out + 4 i is word-aligned and the item is whole, else as bytes.
template <class T>
SRH_ND_HD void nodata_match_item(const SceneNodataParams& p, long i) {
    constexpr int E = (int)sizeof(T);                                  // bytes per element
    constexpr int PER = 16 / E;                                        // elements per chunk
    const uint8_t* s8 = static_cast<const uint8_t*>(p.src);            // everything below is an offset from it: the loads stay global
    const long mis = (long)(reinterpret_cast<uintptr_t>(p.src) & 15);  // the source starts `mis` bytes into its first chunk
    const long total = p.n * (long)p.C * E;                            // bytes of the source
    const long first16 = mis ? 16 - mis : 0, last16 = ((mis + total) & ~15L) - mis;      // the first and last 16-byte boundary inside it
    const long px0 = i * 4;
    const int npx = p.n - px0 < 4 ? (int)(p.n - px0) : 4;
    const long a0 = px0 * (long)p.C * E, a1 = a0 + (long)npx * p.C * E;                 // the item's bytes of the source
    uint32_t acc = 0u;                                                 // byte j: the number of bands of pixel j that hit (<= 16)
    int c = 0, j = 0;
    for (long ch = ((a0 + mis) & ~15L) - mis; ch < a1; ch += 16) {     // chunk offsets: ch + mis is a multiple of 16 (the first may be < 0)
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        if (ch >= first16 && ch + 16 <= last16) {
            const NdWords v = *reinterpret_cast<const NdWords*>(s8 + ch);
            w[0] = v.w[0]; w[1] = v.w[1]; w[2] = v.w[2]; w[3] = v.w[3];
        } else {
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                const long ea = ch + k * E;
                if (ea >= a0 && ea < a1) w[(k * E) >> 2] |= (uint32_t)*reinterpret_cast<const T*>(s8 + ea) << (8 * ((k * E) & 3));
            }
        }
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const long ea = ch + k * E;
            if (ea < a0 || ea >= a1) continue;
            const uint32_t v = (w[(k * E) >> 2] >> (8 * ((k * E) & 3))) & (E == 1 ? 0xffu : 0xffffu);
            const uint32_t lh = p.lohi[c];
            if (v >= (lh & 0xffffu) && v <= (lh >> 16)) acc += 1u << (8 * j);
            if (++c == p.C) { c = 0; ++j; }
        }
    }
    uint32_t word = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t cnt = (acc >> (8 * k)) & 0xffu;
        const uint32_t hit = p.any ? (cnt != 0u) : (cnt == (uint32_t)p.C);
        word |= (p.invert ? hit ^ 1u : hit) << (8 * k);
    }
    uint8_t* o = p.out + px0;
    const bool whole = npx == 4 && (reinterpret_cast<uintptr_t>(o) & 3) == 0;
    if (p.and_with) {
        const uint8_t* a = p.and_with + px0;
        uint32_t m = 0u;
        if (npx == 4 && (reinterpret_cast<uintptr_t>(a) & 3) == 0) {
            const uint32_t v = *reinterpret_cast<const uint32_t*>(a);
#pragma unroll
            for (int k = 0; k < 4; ++k) m |= (uint32_t)(((v >> (8 * k)) & 0xffu) != 0u) << (8 * k);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < npx) m |= (uint32_t)(a[k] != 0) << (8 * k);
        }
        word &= m;
    }
    if (whole) {
        *reinterpret_cast<uint32_t*>(o) = word;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < npx) o[k] = (uint8_t)(word >> (8 * k));
    }
}

// ---- grow ----------------------------------------------------------------------------------------------------------------------------------
// n images, dense H x W u8 blocks of src at byte offsets OFF and of dst at the SAME offsets: g[y, x] = any src != 0 within Chebyshev
// distance r INSIDE the image; dst = (invert ? !g : g) & (and_with ? and_with != 0 : 1), and_with laid out like src.  One table row per
// image, eight int64 of which the first three are read: {OFF, H, W, ...} — the rows of a srh_mask_clean table serve as they are.
constexpr int NG_COLS = 8;
constexpr int NG_OFF = 0, NG_H = 1, NG_W = 2;
constexpr int NG_MAX_R = 16;
constexpr int NG_MAX_IMAGES = 4096;                                // the host check compares every pair of blocks
constexpr int NG_BW = 64, NG_BH = 64;                              // outputs of one workgroup
constexpr int NG_WS = NG_BW + 2 * NG_MAX_R;                        // row stride of the staged window (bytes)
constexpr int NG_WIN_BYTES = (NG_BH + 2 * NG_MAX_R) * NG_WS;       // 9216: the window, block + r on each side
constexpr int NG_ROW_BYTES = (NG_BH + 2 * NG_MAX_R) * NG_BW;       // 6144: the row pass, every window row, the block's columns
constexpr int NG_LDS_BYTES = NG_WIN_BYTES + NG_ROW_BYTES;          // 15 KiB of the 160 KiB of a CU

struct SceneGrowParams {
    const uint8_t* src = nullptr;
    const uint8_t* and_with = nullptr;   // laid out like src, or nullptr
    uint8_t* dst = nullptr;
    const int64_t* table = nullptr;      // [n, NG_COLS]
    int n = 0;
    int r = 1;                           // 1 .. NG_MAX_R
    int invert = 0;
};

// What the threads of a workgroup share: block b of image k.
struct NgBlock {
    long off;                            // byte offset of the image in src, dst and and_with
    int H, W, y0, x0;                    // the block's outputs: rows y0 .. y0 + NG_BH, columns x0 .. x0 + NG_BW, clipped to H and W
};

SRH_ND_HD long grow_blocks_x(long W) { return (W + NG_BW - 1) / NG_BW; }
SRH_ND_HD long grow_blocks(long H, long W) { return ((H + NG_BH - 1) / NG_BH) * grow_blocks_x(W); }

SRH_ND_HD NgBlock grow_locate(const SceneGrowParams& p, int k, long b) {
    const int64_t* t = p.table + (long)k * NG_COLS;
    NgBlock g;
    g.off = (long)t[NG_OFF]; g.H = (int)t[NG_H]; g.W = (int)t[NG_W];
    const long bx = grow_blocks_x(g.W);
    g.y0 = (int)(b / bx) * NG_BH;
    g.x0 = (int)(b - (b / bx) * bx) * NG_BW;
    return g;
}

// Phase 1, item t (0 <= t < (NG_BH + 2 r) * (NG_BW + 2 r)): one byte of the window, 1 where the source pixel is set, 0 where it is not
// or lies outside the image.  The ONLY read of src: bounded by H and W.
SRH_ND_HD void grow_stage_item(const SceneGrowParams& p, const NgBlock& g, uint8_t* win, int t) {
    const int ww = NG_BW + 2 * p.r;
    const int wy = t / ww, wx = t - wy * ww;
    const int y = g.y0 - p.r + wy, x = g.x0 - p.r + wx;
    uint8_t v = 0;
    if (y >= 0 && y < g.H && x >= 0 && x < g.W) v = p.src[g.off + (long)y * g.W + x] != 0;
    win[wy * NG_WS + wx] = v;
}

// Phase 2, item t (0 <= t < (NG_BH + 2 r) * NG_BW): the row pass, row[wy][x] = any of win[wy][x .. x + 2 r].
SRH_ND_HD void grow_row_item(const SceneGrowParams& p, const uint8_t* win, uint8_t* row, int t) {
    const int wy = t / NG_BW, x = t - wy * NG_BW;
    const uint8_t* w = win + wy * NG_WS + x;
    uint8_t v = 0;
    for (int k = 0; k <= 2 * p.r; ++k) v |= w[k];
    row[wy * NG_BW + x] = v;
}

// Phase 3, item t (0 <= t < NG_BH * NG_BW / 4): the column pass and the store of outputs (y0 + t / 16, x0 + 4 (t % 16) .. + 3), those
// inside the image: one word where the four are and their address is word-aligned, else bytes.  The ONLY write: bounded by H and W.
SRH_ND_HD void grow_col_item(const SceneGrowParams& p, const NgBlock& g, const uint8_t* row, int t) {
    const int ly = t / (NG_BW / 4), lx = (t - ly * (NG_BW / 4)) * 4;
    const int y = g.y0 + ly, x = g.x0 + lx;
    if (y >= g.H || x >= g.W) return;
    const int npx = g.W - x < 4 ? g.W - x : 4;
    uint32_t word = 0u;
    for (int k = 0; k <= 2 * p.r; ++k) word |= *reinterpret_cast<const uint32_t*>(row + (ly + k) * NG_BW + lx);     // 4-byte aligned: lx % 4 == 0
    if (p.invert) word ^= 0x01010101u;
    const long at = g.off + (long)y * g.W + x;
    if (p.and_with) {
        uint32_t m = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < npx) m |= (uint32_t)(p.and_with[at + k] != 0) << (8 * k);
        word &= m;
    }
    uint8_t* o = p.dst + at;
    if (npx == 4 && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
        *reinterpret_cast<uint32_t*>(o) = word;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < npx) o[k] = (uint8_t)(word >> (8 * k));
    }
}

// The table on the HOST, checked before a launch: every block inside the buffers (src, dst and and_with hold `bytes` bytes each), no two
// blocks overlapping, at most 2^31 - 1 pixels per image and in all.
inline bool grow_table_ok(const int64_t* t, int n, long long bytes) {
    if (!t || n < 1 || n > NG_MAX_IMAGES || bytes < 1) return false;
    long long total = 0;
    for (int k = 0; k < n; ++k) {
        const int64_t* r = t + (long)k * NG_COLS;
        const long long H = r[NG_H], W = r[NG_W];
        if (H < 1 || W < 1 || H > 2147483647LL || W > 2147483647LL || H * W > 2147483647LL) return false;
        if (r[NG_OFF] < 0 || r[NG_OFF] > bytes - H * W) return false;
        total += H * W;
        if (total > 2147483647LL) return false;
        for (int j = 0; j < k; ++j) {
            const int64_t* q = t + (long)j * NG_COLS;
            if (r[NG_OFF] < q[NG_OFF] + q[NG_H] * q[NG_W] && q[NG_OFF] < r[NG_OFF] + H * W) return false;
        }
    }
    return true;
}

inline long grow_max_blocks(const int64_t* t, int n) {
    long m = 0;
    for (int k = 0; k < n; ++k) {
        const long b = grow_blocks((long)t[(long)k * NG_COLS + NG_H], (long)t[(long)k * NG_COLS + NG_W]);
        m = b > m ? b : m;
    }
    return m;
}

}  // namespace srh
