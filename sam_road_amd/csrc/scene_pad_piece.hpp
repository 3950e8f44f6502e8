// Scene border padding (scene_pad.hip): the parameters and the work of ONE item, free of HIP so that a CPU program can run
// the kernel's own addressing over every item of a launch (tests/scene_pad_check.cpp, under the host sanitizers) before a GPU does.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define SRH_PAD_HD __host__ __device__ __forceinline__
#else
#define SRH_PAD_HD inline
#endif

namespace srh {

constexpr int PAD_REFLECT = 0, PAD_EDGE = 1, PAD_CONSTANT = 2;     // = SRH_PAD_* of include/samroad_hip.h
constexpr int PAD_THREADS = 256, PAD_PIECES = 1024;                // a workgroup takes 1024 pieces (16 KiB) of one row, four per thread

// dst u8 [Hv,Wv,C] = src u8 [H,W,C] padded: virtual pixel (Y, X) holds source pixel (fold(Y - top, H), fold(X - left, W)).
// H * W and Hv * Wv fit an int (the C ABI checks both); byte offsets are 64-bit.  src and dst must not overlap.
struct ScenePadParams {
    const uint8_t* src = nullptr; uint8_t* dst = nullptr;
    int H = 0, W = 0, Hv = 0, Wv = 0, top = 0, left = 0;
    int C = 3;                   // bytes per pixel: 3 (the scene) or 1 (the validity mask)
    int mode = PAD_REFLECT;
    uint32_t fill = 0;           // PAD_CONSTANT: channel ch of the fill colour in bits 8 ch .. 8 ch + 7
};

struct alignas(16) PadWords { uint32_t w[4]; };

// source index of virtual index i (relative to the source's first row / column) on an axis of n pixels; -1: the fill colour
SRH_PAD_HD int pad_fold(long i, int n, int mode) {
    if (mode == PAD_REFLECT) {
        if (n == 1) return 0;
        const uint32_t T = 2u * (uint32_t)(n - 1);           // the mirror image is symmetric about 0: fold |i|
        const uint32_t j = (uint32_t)(i < 0 ? -i : i) % T;
        return (int)(j < (uint32_t)n ? j : T - j);
    }
    if (mode == PAD_EDGE) return (int)(i < 0 ? 0 : (i > n - 1 ? n - 1 : i));
    return i >= 0 && i < n ? (int)i : -1;
}

// What the pieces of destination row Y share.  A piece is 16 bytes of the row cut at the 16-byte boundaries of the ADDRESS.
struct PadRow {
    const uint8_t* srow; uint8_t* drow;
    int sy;                      // the source row, -1: the whole row is the fill colour
    long mis, n_pieces;          // the row starts `mis` bytes into its first piece
};

template <int C>
SRH_PAD_HD PadRow pad_row(const ScenePadParams& p, long Y) {
    PadRow r;
    const long row_b = (long)p.Wv * C;
    r.sy = pad_fold(Y - p.top, p.H, p.mode);
    r.srow = p.src + (long)(r.sy < 0 ? 0 : r.sy) * ((long)p.W * C);
    r.drow = p.dst + Y * row_b;
    r.mis = (long)(reinterpret_cast<uintptr_t>(r.drow) & 15);
    r.n_pieces = (r.mis + row_b + 15) >> 4;
    return r;
}

// Piece pc (0 <= pc < n_pieces) of a row: writes the bytes of the piece that belong to the row, each once, and nothing else.
template <int C>
SRH_PAD_HD void pad_piece(const ScenePadParams& p, const PadRow& r, long pc) {
    const long row_b = (long)p.Wv * C, src_row_b = (long)p.W * C;     // bytes per destination / source row
    const long in0 = (long)p.left * C, in1 = in0 + src_row_b;         // the interior of a destination row, in bytes of the row
    const long r0 = pc * 16 - r.mis;                                  // byte of the row the piece starts at (negative: before the row)
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    const bool whole = r0 >= 0 && r0 + 16 <= row_b;
    if (whole && r.sy >= 0 && r0 >= in0 && r0 + 16 <= in1) {          // contiguous copy of 16 source bytes
        const uint8_t* s = r.srow + (r0 - in0);
        const uintptr_t a = reinterpret_cast<uintptr_t>(s), a4 = a & ~(uintptr_t)3;
        const uintptr_t src_lo = reinterpret_cast<uintptr_t>(p.src), src_hi = src_lo + (uintptr_t)((long)p.H * src_row_b);
        if ((a & 15) == 0) {
            const PadWords v = *reinterpret_cast<const PadWords*>(s);
            w[0] = v.w[0]; w[1] = v.w[1]; w[2] = v.w[2]; w[3] = v.w[3];
        } else if ((a & 3) == 0) {
#pragma unroll
            for (int k = 0; k < 4; ++k) w[k] = reinterpret_cast<const uint32_t*>(s)[k];
        } else if (a4 >= src_lo && a4 + 20 <= src_hi) {               // the five aligned words that hold the 16 bytes lie inside src
            const uint32_t* q = reinterpret_cast<const uint32_t*>(a4);
            const int sh = (int)(a & 3) * 8;                          // 8, 16 or 24 (little endian)
            uint32_t v[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) v[k] = q[k];
#pragma unroll
            for (int k = 0; k < 4; ++k) w[k] = (v[k] >> sh) | (v[k + 1] << (32 - sh));
        } else {                                                      // the first / last bytes of the buffer
#pragma unroll
            for (int k = 0; k < 16; ++k) w[k >> 2] |= (uint32_t)s[k] << (8 * (k & 3));
        }
        *reinterpret_cast<PadWords*>(r.drow + r0) = PadWords{{w[0], w[1], w[2], w[3]}};
        return;
    }
    // per-pixel addressing: bytes kb .. ke of the piece belong to the row
    const int kb = r0 < 0 ? (int)-r0 : 0;
    const int ke = r0 + 16 > row_b ? (int)(row_b - r0) : 16;
    long X = (r0 + kb) / C;
    int ch = (int)((r0 + kb) - X * C);
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        if (k < kb || k >= ke) continue;
        const int sx = r.sy < 0 ? -1 : pad_fold(X - p.left, p.W, p.mode);
        const uint32_t b = sx < 0 ? (p.fill >> (8 * ch)) & 0xffu : (uint32_t)r.srow[(long)sx * C + ch];
        w[k >> 2] |= b << (8 * (k & 3));
        if (++ch == C) { ch = 0; ++X; }
    }
    if (whole) {
        *reinterpret_cast<PadWords*>(r.drow + r0) = PadWords{{w[0], w[1], w[2], w[3]}};
    } else {
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (k >= kb && k < ke) r.drow[r0 + k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
    }
}

// How a launch is cut: a workgroup (a "group") takes PAD_PIECES consecutive pieces of one row.
inline long pad_groups_per_row(const ScenePadParams& p) {
    const long max_pieces = (((long)p.Wv * p.C + 15) >> 4) + 1;       // a row that does not start on a boundary may have one piece more
    return (max_pieces + PAD_PIECES - 1) / PAD_PIECES;
}
inline bool pad_params_ok(const ScenePadParams& p) {
    return (p.C == 1 || p.C == 3) && p.src && p.dst && p.H > 0 && p.W > 0 && p.Hv >= p.H && p.Wv >= p.W && p.top >= 0 && p.left >= 0 &&
           p.top <= p.Hv - p.H && p.left <= p.Wv - p.W && p.mode >= PAD_REFLECT && p.mode <= PAD_CONSTANT;
}

}  // namespace srh
