// Scene resampling (scene_scale.hip): the parameters, how a launch is cut into blocks, and the work of ONE item of each of
// a block's three phases, free of HIP so that a CPU program can run the kernel's own addressing over every item of a launch
// (tests/scene_scale_check.cpp, under the host sanitizers) before a GPU does.  The rule itself is stated once, on the host
// (sam_road_amd/resample.py): the kernel only reads the tables built there.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define SRH_SCALE_HD __host__ __device__ __forceinline__
#else
#define SRH_SCALE_HD inline
#endif

namespace srh {

constexpr int SCALE_THREADS = 256;
constexpr int SCALE_MAX_T = 32, SCALE_MAX_D = 32, SCALE_MAX_BLOCK = 256;
constexpr long SCALE_MAX_LDS = 64 * 1024;
constexpr int SCALE_SUM = 0, SCALE_VALID = 1;                        // = the mode of srh_scene_resample

// dst u8 [Ho,Wo,C] from src u8 [H,W,C]: output (Y, X) reads rows clamp(sy[Y] + t, 0, H - 1) with weights wy[Y Ty + t] (sum Dy) and columns
// clamp(sx[X] + t, 0, W - 1) with weights wx[X Tx + t] (sum Dx).  H * W and Ho * Wo fit an int (the C ABI checks both); byte offsets are
// 64-bit.  Every tap index is clamped where it is used, so no table content can take an access outside src.
struct SceneScaleParams {
    const uint8_t* src = nullptr; uint8_t* dst = nullptr;
    const uint8_t* zero_where = nullptr;                             // u8 [Ho,Wo] or null: dst is 0 where it is 0
    const int32_t* sy = nullptr; const uint8_t* wy = nullptr;        // int32 [Ho], u8 [Ho,Ty]
    const int32_t* sx = nullptr; const uint8_t* wx = nullptr;        // int32 [Wo], u8 [Wo,Tx]
    int H = 0, W = 0, Ho = 0, Wo = 0, C = 3, Ty = 0, Tx = 0, Dy = 0, Dx = 0;
    int mode = SCALE_SUM;
    int bh = 0, bw = 0;          // a workgroup's output block
    int win_h = 0, win_w = 0;    // the source window LDS holds (rows, pixels); 0 x 0: the direct form, every output gathers its own taps
    uint64_t magic = 0;          // floor(2^32 / (Dy Dx)) + 1: n / (Dy Dx) == (n * magic) >> 32 for every n the rule produces
};

struct alignas(16) ScaleWords { uint32_t w[4]; };

SRH_SCALE_HD int scale_tap(int start, int t, int n) {                // clamp(start + t, 0, n - 1)
    const long i = (long)start + t;
    return (int)(i < 0 ? 0 : (i > n - 1 ? n - 1 : i));
}
SRH_SCALE_HD uint64_t scale_magic(int DD) { return (1ull << 32) / (uint32_t)DD + 1u; }
SRH_SCALE_HD uint32_t scale_round_div(uint32_t acc, int DD, uint64_t magic) {      // (acc + DD / 2) / DD
    return (uint32_t)(((acc + (uint32_t)(DD >> 1)) * magic) >> 32);
}

// LDS of a workgroup: win_h window rows of `pitch` bytes — a row is staged from the 16-byte boundary at or below its first byte, so that
// aligned 16-byte pieces of src land on aligned 16-byte pieces of LDS — then win_h rows of bw * C u16 row sums.
SRH_SCALE_HD int scale_pitch(int win_w, int C) { return (win_w * C + 15 + 15) / 16 * 16; }
inline long scale_lds_bytes(const SceneScaleParams& p) {
    return p.win_h > 0 ? (long)p.win_h * (scale_pitch(p.win_w, p.C) + 2L * p.bw * p.C) : 0;
}
inline long scale_blocks_x(const SceneScaleParams& p) { return ((long)p.Wo + p.bw - 1) / p.bw; }
inline long scale_blocks(const SceneScaleParams& p) { return scale_blocks_x(p) * (((long)p.Ho + p.bh - 1) / p.bh); }

inline bool scale_params_ok(const SceneScaleParams& p) {
    if (!p.src || !p.dst || !p.sy || !p.wy || !p.sx || !p.wx) return false;
    if ((p.C != 1 && p.C != 3) || (p.mode != SCALE_SUM && p.mode != SCALE_VALID)) return false;
    if (p.H < 1 || p.W < 1 || p.Ho < 1 || p.Wo < 1 || (long)p.H * p.W > 2147483647L || (long)p.Ho * p.Wo > 2147483647L) return false;
    if (p.Ty < 1 || p.Tx < 1 || p.Ty > SCALE_MAX_T || p.Tx > SCALE_MAX_T || p.Dy < 1 || p.Dx < 1 || p.Dy > SCALE_MAX_D || p.Dx > SCALE_MAX_D) return false;
    if (p.bh < 1 || p.bw < 1 || p.bh > SCALE_MAX_BLOCK || p.bw > SCALE_MAX_BLOCK) return false;
    if (p.win_h < 0 || p.win_w < 0 || (p.win_h == 0) != (p.win_w == 0) || p.win_h > 4096 || p.win_w > 4096) return false;
    return scale_lds_bytes(p) <= SCALE_MAX_LDS && p.magic == scale_magic(p.Dy * p.Dx);
}

// What the items of block b share: its outputs [y0, y0 + ny) x [x0, x0 + nx) and the source window [r0, r0 + nr) x [c0, c0 + nc) their
// taps fall into (the starts are monotone; a tap outside the window — tables that are not — is clamped into it).  lds: the window fits
// what the launch reserved and the mode is the weighted sum; else every output of the block gathers its own taps from src.
struct ScaleBlock {
    int y0, ny, x0, nx, r0, nr, c0, nc;
    bool lds;
};

SRH_SCALE_HD ScaleBlock scale_block(const SceneScaleParams& p, long b) {
    ScaleBlock k;
    const long nbx = ((long)p.Wo + p.bw - 1) / p.bw;
    const long by = b / nbx, bx = b - by * nbx;
    k.y0 = (int)(by * p.bh); k.ny = p.Ho - k.y0 < p.bh ? p.Ho - k.y0 : p.bh;
    k.x0 = (int)(bx * p.bw); k.nx = p.Wo - k.x0 < p.bw ? p.Wo - k.x0 : p.bw;
    k.r0 = scale_tap(p.sy[k.y0], 0, p.H);
    const int r1 = scale_tap(p.sy[k.y0 + k.ny - 1], p.Ty - 1, p.H);
    k.nr = r1 >= k.r0 ? r1 - k.r0 + 1 : 1;
    k.c0 = scale_tap(p.sx[k.x0], 0, p.W);
    const int c1 = scale_tap(p.sx[k.x0 + k.nx - 1], p.Tx - 1, p.W);
    k.nc = c1 >= k.c0 ? c1 - k.c0 + 1 : 1;
    k.lds = p.mode == SCALE_SUM && p.win_h > 0 && k.nr <= p.win_h && k.nc <= p.win_w;
    return k;
}

SRH_SCALE_HD int scale_in_window(int i, int lo, int n) { return i < lo ? 0 : (i > lo + n - 1 ? n - 1 : i - lo); }

// first byte of window row i in src, and how far it lies behind its 16-byte boundary
SRH_SCALE_HD const uint8_t* scale_row_src(const SceneScaleParams& p, const ScaleBlock& k, int i) {
    return p.src + ((long)(k.r0 + i) * p.W + k.c0) * p.C;
}
SRH_SCALE_HD int scale_row_mis(const SceneScaleParams& p, const ScaleBlock& k, int i) {
    return (int)(reinterpret_cast<uintptr_t>(scale_row_src(p, k, i)) & 15);
}

// ---- phase 1, staging: item = (window row i, 16-byte piece pc of the row's pitch) -------------------------------------------------------
SRH_SCALE_HD long scale_stage_items(const SceneScaleParams& p, const ScaleBlock& k) { return (long)k.nr * (scale_pitch(p.win_w, p.C) >> 4); }

SRH_SCALE_HD void scale_stage_item(const SceneScaleParams& p, const ScaleBlock& k, uint8_t* lds, long item) {
    const int pitch = scale_pitch(p.win_w, p.C), ppr = pitch >> 4;
    const int i = (int)(item / ppr), pc = (int)(item - (long)i * ppr);
    const uint8_t* a = scale_row_src(p, k, i);
    const int mis = (int)(reinterpret_cast<uintptr_t>(a) & 15);
    if (pc * 16 >= mis + k.nc * p.C) return;                          // behind the row's last byte
    const long g = (a - p.src) - mis + (long)pc * 16;                 // offset in src of the piece: its address is 16-byte aligned
    const long total = (long)p.H * p.W * p.C;
    ScaleWords v = {{0u, 0u, 0u, 0u}};
    if (g >= 0 && g + 16 <= total) {
        v = *reinterpret_cast<const ScaleWords*>(p.src + g);
    } else {                                                          // the first / last bytes of the buffer
#pragma unroll
        for (int b = 0; b < 16; ++b)
            if (g + b >= 0 && g + b < total) v.w[b >> 2] |= (uint32_t)p.src[g + b] << (8 * (b & 3));
    }
    *reinterpret_cast<ScaleWords*>(lds + (long)i * pitch + pc * 16) = v;
}

// ---- phase 2, row pass: item = (window row i, output column x of the block, channel) -> u16 row sum -------------------------------------
SRH_SCALE_HD long scale_row_items(const SceneScaleParams& p, const ScaleBlock& k) { return (long)k.nr * k.nx * p.C; }

SRH_SCALE_HD void scale_row_item(const SceneScaleParams& p, const ScaleBlock& k, uint8_t* lds, long item) {
    const int pitch = scale_pitch(p.win_w, p.C), per_row = k.nx * p.C;
    const int i = (int)(item / per_row), rem = (int)(item - (long)i * per_row);
    const int x = rem / p.C, ch = rem - x * p.C, X = k.x0 + x;
    const uint8_t* row = lds + (long)i * pitch + scale_row_mis(p, k, i) + ch;
    const uint8_t* w = p.wx + (long)X * p.Tx;
    const int s = p.sx[X];
    uint32_t acc = 0;
    for (int t = 0; t < p.Tx; ++t) acc += (uint32_t)w[t] * row[scale_in_window(scale_tap(s, t, p.W), k.c0, k.nc) * p.C];
    uint16_t* sums = reinterpret_cast<uint16_t*>(lds + (long)p.win_h * pitch);
    sums[(long)i * (p.bw * p.C) + rem] = (uint16_t)acc;               // at most 255 * 32
}

// ---- phase 3, output: item = (output row y of the block, 4-byte piece pc of its segment of the dst row, cut at the ADDRESS) -------------
SRH_SCALE_HD long scale_out_items(const SceneScaleParams& p, const ScaleBlock& k) { return (long)k.ny * ((p.bw * p.C + 3) / 4 + 1); }

// one output byte: the column pass over the row sums (lds), or the byte's own taps gathered from src
SRH_SCALE_HD uint32_t scale_value(const SceneScaleParams& p, const ScaleBlock& k, const uint8_t* lds, int y, int x, int ch) {
    const int Y = k.y0 + y, X = k.x0 + x;
    if (p.zero_where && p.zero_where[(long)Y * p.Wo + X] == 0) return 0u;
    const uint8_t* wy = p.wy + (long)Y * p.Ty;
    const int s = p.sy[Y];
    if (k.lds) {
        const uint16_t* sums = reinterpret_cast<const uint16_t*>(lds + (long)p.win_h * scale_pitch(p.win_w, p.C)) + x * p.C + ch;
        uint32_t acc = 0;
        for (int t = 0; t < p.Ty; ++t) acc += (uint32_t)wy[t] * sums[(long)scale_in_window(scale_tap(s, t, p.H), k.r0, k.nr) * (p.bw * p.C)];
        return scale_round_div(acc, p.Dy * p.Dx, p.magic);
    }
    const uint8_t* wx = p.wx + (long)X * p.Tx;
    const int sx = p.sx[X];
    uint32_t acc = 0, bad = 0;
    for (int t = 0; t < p.Ty; ++t) {
        if (!wy[t]) continue;
        const uint8_t* row = p.src + (long)scale_tap(s, t, p.H) * p.W * p.C + ch;
        uint32_t r = 0;
        for (int u = 0; u < p.Tx; ++u) {
            if (!wx[u]) continue;
            const uint32_t v = row[(long)scale_tap(sx, u, p.W) * p.C];
            r += (uint32_t)wx[u] * v;
            bad |= (uint32_t)(v == 0);
        }
        acc += (uint32_t)wy[t] * r;
    }
    return p.mode == SCALE_VALID ? 1u - bad : scale_round_div(acc, p.Dy * p.Dx, p.magic);
}

SRH_SCALE_HD void scale_out_item(const SceneScaleParams& p, const ScaleBlock& k, const uint8_t* lds, long item) {
    const int ppr = (p.bw * p.C + 3) / 4 + 1, seg = k.nx * p.C;       // bytes of the block's segment of a dst row
    const int y = (int)(item / ppr), pc = (int)(item - (long)y * ppr);
    uint8_t* a = p.dst + ((long)(k.y0 + y) * p.Wo + k.x0) * p.C;
    const int mis = (int)(reinterpret_cast<uintptr_t>(a) & 3);
    const int b0 = pc * 4 - mis;                                      // byte of the segment the piece starts at (negative: before it)
    if (b0 >= seg) return;
    const int kb = b0 < 0 ? -b0 : 0, ke = b0 + 4 > seg ? seg - b0 : 4;
    uint32_t w = 0;
    int x = (b0 + kb) / p.C, ch = (b0 + kb) - x * p.C;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (j < kb || j >= ke) continue;
        w |= scale_value(p, k, lds, y, x, ch) << (8 * j);
        if (++ch == p.C) { ch = 0; ++x; }
    }
    if (kb == 0 && ke == 4) {
        *reinterpret_cast<uint32_t*>(a + b0) = w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j >= kb && j < ke) a[b0 + j] = (uint8_t)(w >> (8 * j));
    }
}

}  // namespace srh
