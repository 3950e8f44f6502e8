// Float32 scenes (scene_float.hip): the parameters, the ordered key and the work of ONE item of the valid and the apply
// kernel, free of HIP so that a CPU program can run the kernels' own addressing over every item of a launch (tests/scene_float_check.cpp,
// under the host sanitizers) before a GPU does.  A float is only ever read as its 32-bit pattern and compared as an unsigned integer:
// there is no float compare and no float arithmetic here, so no compiler flag and no denormal mode can change a byte.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define SRH_FLOAT_HD __host__ __device__ __forceinline__
#else
#define SRH_FLOAT_HD inline
#endif

namespace srh {

constexpr int FLOAT_THREADS = 256;
constexpr int FLOAT_MAX_C = 16;
constexpr int FLOAT_MAX_NODATA = 4;
constexpr int FLOAT_MAX_TARGETS = 6;
constexpr long FLOAT_MAX_PIXELS = 2147483647L;
constexpr uint32_t FLOAT_KEY_ZERO = 0x80000000u;                   // the key of +0.0 (and of -0.0)

// src f32 [n,C] as bit patterns.  The kernels know nothing of H or W.  Offsets are 64-bit from the first product on: 16 bands *
// (2^31 - 1) pixels * 4 bytes does not fit 32 bits.
struct SceneFloatParams {
    const uint32_t* src = nullptr;
    const uint8_t* valid_in = nullptr;   // the valid kernel only: the caller's mask u8 [n], or nullptr
    uint8_t* valid_out = nullptr;        // the valid kernel only: u8 [n], 0 / 1
    const uint8_t* valid = nullptr;      // hist and apply: u8 [n], 0 = the pixel does not count / comes out as 0, 0, 0
    const uint32_t* thr = nullptr;       // the apply kernel only: keys u32 [3, 256], entry 255 = 0xffffffff
    uint8_t* dst = nullptr;              // the apply kernel only: u8 [n, 3]
    uint32_t* hist = nullptr;            // the histogram only: u32 [3, 65536] (pass 1) or [n_targets, 65536] (pass 2)
    long n = 0;                          // pixels
    int C = 3;                           // bands per source pixel, 1 .. FLOAT_MAX_C
    int sel[3] = {0, 1, 2};              // the source band of output channel b
    int n_nodata = 0;                    // the valid kernel only
    uint32_t nodata[FLOAT_MAX_NODATA] = {0u, 0u, 0u, 0u};           // keys
    int log = 0;                         // the valid kernel only: 1 = every selected band must be > 0
    int n_targets = 0;                   // the histogram only: 0 = pass 1
    int tband[FLOAT_MAX_TARGETS] = {0, 0, 0, 0, 0, 0};
    uint32_t tprefix[FLOAT_MAX_TARGETS] = {0u, 0u, 0u, 0u, 0u, 0u};
};

struct alignas(16) FloatWords { uint32_t w[4]; };

inline bool float_params_ok(const SceneFloatParams& p) {
    if (!p.src || (reinterpret_cast<uintptr_t>(p.src) & 3) || p.n < 1 || p.n > FLOAT_MAX_PIXELS || p.C < 1 || p.C > FLOAT_MAX_C) return false;
    for (int b = 0; b < 3; ++b)
        if (p.sel[b] < 0 || p.sel[b] >= p.C) return false;
    if (p.n_nodata < 0 || p.n_nodata > FLOAT_MAX_NODATA || (p.log != 0 && p.log != 1) || p.n_targets < 0 || p.n_targets > FLOAT_MAX_TARGETS) return false;
    for (int t = 0; t < p.n_targets; ++t)
        if (p.tband[t] < 0 || p.tband[t] >= p.C || p.tprefix[t] > 0xffffu) return false;
    return true;
}

// The ordered key of a bit pattern: -0.0 is +0.0; over the non-NaN values unsigned order of the keys is float order.
SRH_FLOAT_HD uint32_t float_key(uint32_t b) {
    b = b == 0x80000000u ? 0u : b;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
SRH_FLOAT_HD bool float_finite(uint32_t b) { return ((b >> 23) & 0xffu) != 0xffu; }

// Rule 1 for one selected band.
SRH_FLOAT_HD bool float_band_ok(const SceneFloatParams& p, uint32_t bits) {
    const uint32_t k = float_key(bits);
    bool ok = float_finite(bits);
#pragma unroll
    for (int j = 0; j < FLOAT_MAX_NODATA; ++j)                        // constant indices: no indexed access to the parameter block
        if (j < p.n_nodata && k == p.nodata[j]) ok = false;
    if (p.log && k <= FLOAT_KEY_ZERO) ok = false;
    return ok;
}

// Rule 1 for pixel i (0 <= i < n): reads its three selected bands and valid_in[i].
SRH_FLOAT_HD uint32_t float_valid_px(const SceneFloatParams& p, long i) {
    const uint32_t* s = p.src + i * p.C;                             // 64-bit: i * C elements
    bool ok = float_band_ok(p, s[p.sel[0]]);
    ok = float_band_ok(p, s[p.sel[1]]) && ok;
    ok = float_band_ok(p, s[p.sel[2]]) && ok;
    if (p.valid_in && !p.valid_in[i]) ok = false;
    return ok ? 1u : 0u;
}

// A piece is 16 bytes of the output cut at the 16-byte boundaries of the ADDRESS; the output starts `mis` bytes into its first piece.
SRH_FLOAT_HD long float_valid_mis(const SceneFloatParams& p) { return (long)(reinterpret_cast<uintptr_t>(p.valid_out) & 15); }
SRH_FLOAT_HD long float_valid_pieces(const SceneFloatParams& p) { return (float_valid_mis(p) + p.n + 15) >> 4; }
SRH_FLOAT_HD long float_apply_mis(const SceneFloatParams& p) { return (long)(reinterpret_cast<uintptr_t>(p.dst) & 15); }
SRH_FLOAT_HD long float_apply_pieces(const SceneFloatParams& p) { return (float_apply_mis(p) + 3 * p.n + 15) >> 4; }

// Piece pc of the valid kernel (0 <= pc < float_valid_pieces): writes the bytes of the piece that belong to valid_out, each once, and
// nothing else; one 16-byte store where the whole piece lies inside, single bytes at the head and the tail.
SRH_FLOAT_HD void float_valid_piece(const SceneFloatParams& p, long pc) {
    const long r0 = pc * 16 - float_valid_mis(p);                     // pixel the piece starts at (negative: before the output)
    const int kb = r0 < 0 ? (int)-r0 : 0;
    const int ke = r0 + 16 > p.n ? (int)(p.n - r0) : 16;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        if (k < kb || k >= ke) continue;
        w[k >> 2] |= float_valid_px(p, r0 + k) << (8 * (k & 3));
    }
    if (kb == 0 && ke == 16) {
        *reinterpret_cast<FloatWords*>(p.valid_out + r0) = FloatWords{{w[0], w[1], w[2], w[3]}};
    } else {
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (k >= kb && k < ke) p.valid_out[r0 + k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
    }
}

// #{j < 255 : tab[j] <= key} for an ascending table of 256 keys: a branch-free binary search of 8 steps; the highest entry read is 254.
SRH_FLOAT_HD uint32_t float_level(const uint32_t* tab, uint32_t key) {
    uint32_t pos = 0u;
#pragma unroll
    for (uint32_t s = 128u; s; s >>= 1) pos += tab[pos + s - 1u] <= key ? s : 0u;
    return pos;
}

// Piece pc of the apply kernel (0 <= pc < float_apply_pieces): writes the bytes of the piece that belong to dst, each once, and nothing
// else; reads the selected bands and the mask byte of the five or six pixels those bytes belong to.  tab: the three tables, u32 [3, 256]
// (the kernel passes its copy in the LDS).
SRH_FLOAT_HD void float_apply_piece(const SceneFloatParams& p, const uint32_t* tab, long pc) {
    const long total = 3 * p.n;
    const long r0 = pc * 16 - float_apply_mis(p);                     // byte of dst the piece starts at (negative: before dst)
    const int kb = r0 < 0 ? (int)-r0 : 0;
    const int ke = r0 + 16 > total ? (int)(total - r0) : 16;
    long px = (r0 + kb) / 3;
    int ch = (int)((r0 + kb) - px * 3);
    const uint32_t* s = p.src + px * p.C;                             // 64-bit: px * C elements
    const int s0 = p.sel[0], s1 = p.sel[1], s2 = p.sel[2];
    uint32_t ok = p.valid[px];
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        if (k < kb || k >= ke) continue;
        const uint32_t key = float_key(s[ch == 0 ? s0 : (ch == 1 ? s1 : s2)]);
        const uint32_t level = float_level(tab + ch * 256, key);
        w[k >> 2] |= (ok ? level : 0u) << (8 * (k & 3));
        if (++ch == 3) {
            ch = 0; s += p.C; ++px;
            if (k + 1 < ke) ok = p.valid[px];                         // only the mask bytes of pixels that have a byte in the piece
        }
    }
    if (kb == 0 && ke == 16) {
        *reinterpret_cast<FloatWords*>(p.dst + r0) = FloatWords{{w[0], w[1], w[2], w[3]}};
    } else {
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (k >= kb && k < ke) p.dst[r0 + k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
    }
}

}  // namespace srh
