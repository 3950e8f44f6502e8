// Band selection + radiometric lookup (scene_bands.hip): the parameters and the work of ONE item of the apply kernel, free
// of HIP so that a CPU program can run the kernel's own addressing over every item of a launch (tests/scene_bands_check.cpp, under the
// host sanitizers) before a GPU does.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define SRH_BANDS_HD __host__ __device__ __forceinline__
#else
#define SRH_BANDS_HD inline
#endif

namespace srh {

constexpr int BANDS_THREADS = 256;
constexpr int BANDS_MAX_C = 16;
constexpr long BANDS_MAX_PIXELS = 2147483647L;                     // a scene's (or a group's ragged buffer's) pixel count fits an int

// dst u8 [n,3]: byte 3 i + b = lut[b * levels + src[i * C + sel[b]]], src u8 (levels 256) or u16 (levels 65536) [n,C].  The kernels know
// nothing of H or W.  Offsets are 64-bit from the first product on: 16 bands * (2^31 - 1) pixels * 2 bytes does not fit 32 bits.
struct SceneBandsParams {
    const void* src = nullptr;
    const uint8_t* lut = nullptr;    // u8 [3, levels]
    const uint8_t* valid = nullptr;  // the histogram only: u8 [n], 0 = the pixel does not count; nullptr: every pixel counts
    uint8_t* dst = nullptr;          // the apply kernel only
    uint32_t* hist = nullptr;        // the histogram only: u32 [3, levels]
    long n = 0;                      // pixels
    int C = 3;                       // bands per source pixel, 1 .. BANDS_MAX_C
    int sel[3] = {0, 1, 2};          // the source band of output channel b
    int wide = 0;                    // 0: u8 source, 1: u16 source
};

struct alignas(16) BandsWords { uint32_t w[4]; };

inline bool bands_params_ok(const SceneBandsParams& p) {
    if (!p.src || p.n < 1 || p.n > BANDS_MAX_PIXELS || p.C < 1 || p.C > BANDS_MAX_C || (p.wide != 0 && p.wide != 1)) return false;
    for (int b = 0; b < 3; ++b)
        if (p.sel[b] < 0 || p.sel[b] >= p.C) return false;
    return !p.wide || (reinterpret_cast<uintptr_t>(p.src) & 1) == 0;
}

// A piece is 16 bytes of dst cut at the 16-byte boundaries of the ADDRESS; dst starts `mis` bytes into its first piece.
SRH_BANDS_HD long bands_mis(const SceneBandsParams& p) { return (long)(reinterpret_cast<uintptr_t>(p.dst) & 15); }
SRH_BANDS_HD long bands_n_pieces(const SceneBandsParams& p) { return (bands_mis(p) + 3 * p.n + 15) >> 4; }

// Piece pc (0 <= pc < bands_n_pieces): writes the bytes of the piece that belong to dst, each once, and nothing else; reads the selected
// bands of the five or six pixels those bytes belong to, one element at a time (an element is naturally aligned), and the tables.
template <class T>
SRH_BANDS_HD void bands_piece(const SceneBandsParams& p, long pc) {
    constexpr long levels = sizeof(T) == 1 ? 256 : 65536;
    const T* src = static_cast<const T*>(p.src);
    const long total = 3 * p.n;
    const long r0 = pc * 16 - bands_mis(p);                           // byte of dst the piece starts at (negative: before dst)
    const int kb = r0 < 0 ? (int)-r0 : 0;
    const int ke = r0 + 16 > total ? (int)(total - r0) : 16;
    long px = (r0 + kb) / 3;
    int ch = (int)((r0 + kb) - px * 3);
    const T* s = src + px * p.C;                                      // 64-bit: px * C elements
    const int s0 = p.sel[0], s1 = p.sel[1], s2 = p.sel[2];           // selected by compares: no indexed access to the parameter block
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        if (k < kb || k >= ke) continue;
        const uint32_t v = (uint32_t)s[ch == 0 ? s0 : (ch == 1 ? s1 : s2)];
        w[k >> 2] |= (uint32_t)p.lut[ch * levels + v] << (8 * (k & 3));
        if (++ch == 3) { ch = 0; s += p.C; }
    }
    if (kb == 0 && ke == 16) {
        *reinterpret_cast<BandsWords*>(p.dst + r0) = BandsWords{{w[0], w[1], w[2], w[3]}};
    } else {
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (k >= kb && k < ke) p.dst[r0 + k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
    }
}

}  // namespace srh
