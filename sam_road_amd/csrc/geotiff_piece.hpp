// GeoTIFF scenes (scene_tiff.hip, config key GEOTIFF): the LZW decoder of the host entry srh_tiff_lzw_decode, and the
// parameters and the work of ONE thread in each phase of the assemble launch, free of HIP so that a CPU program can run whole launches
// through the kernel's own addressing and arithmetic (tests/geotiff_check.cpp, under the host sanitizers) before a GPU does.  The rule is
// stated on the host (sam_road_amd/geotiff.py): the raster must equal tiff_read_ref bit for bit.
//
// The launch takes the file's DECOMPRESSED segments as they are, in one flat array, and a table of them, int64 [n, 7], row k =
// {offset, bytes, first row, first column, rows, columns, band or -1}.  A work item is one row of one segment, item = segment * max_rows +
// row, and a workgroup of TIF_THREADS does it: the row's ELEMENTS — samples in native byte order, or for predictor 3 the bytes of the
// row's four byte planes — go through LDS in chunks of at most TIF_CHUNK, are summed along the row with stride S (the interleaved samples
// of a pixel: C in a chunky segment, 1 in a planar one) in wrapping 32-bit words, of which the store keeps the low 8 / 16 bits (or all 32:
// predictor 1 floats), and are stored at their place of the raster [H, W, C]; the columns of a tile beyond W and its rows beyond H are
// never stored.  A thread owns TF pixels-per-thread consecutive pixels of a chunk: tif_local_sum, an exclusive scan over the threads (in
// the kernel a shuffle scan in a wave and LDS across the four waves, in the CPU program a loop), tif_local_apply with the running total of
// the earlier chunks carried per sample of the pixel.  LDS does not depend on W.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define SRH_TIF_HD __host__ __device__ inline __attribute__((always_inline))   // host_geom.hip includes this without the HIP runtime header
#else
#define SRH_TIF_HD inline
#endif

namespace srh {

constexpr int TIF_THREADS = 256, TIF_WAVES = 4;
constexpr int TIF_CHUNK = 4096;                                     // elements of a chunk at most: floor(TIF_CHUNK / S) pixels
constexpr int TIF_LDS_WORDS = TIF_CHUNK + (TIF_CHUNK >> 5);            // a pad word behind every 32: a thread's pixels lie S * PP words apart
constexpr int TIF_MAX_BANDS = 16;
constexpr int TIF_TABLE_COLS = 7;
constexpr int TIF_ALIGN = 16;                                       // every segment's offset in the flat array
constexpr long TIF_MAX_PIXELS = 2147483647L;
constexpr long TIF_MAX_BLOCKS = 1L << 20;

struct alignas(16) TifWords { uint32_t w[4]; };

struct TiffParams {
    const uint8_t* flat = nullptr;       // the decompressed segments
    const int64_t* table = nullptr;      // int64 [n_seg, 7], validated on the host (tif_table_ok)
    int n_seg = 0;
    int max_rows = 0;                    // the largest `rows` of the table: a segment owns max_rows items, those beyond its rows are idle
    uint8_t* out = nullptr;              // [H, W, C] samples of B bytes, B-byte aligned
    int H = 0, W = 0, C = 0;
    int B = 1;                           // bytes of a sample: 1, 2 (unsigned) or 4 (float, moved as bit patterns)
    int predictor = 1;                   // 1; 2 with B = 1, 2; 3 with B = 4
    int big_endian = 0;                  // the file's byte order (predictor 3 does not depend on it)
};

inline bool tif_params_ok(const TiffParams& p) {
    if (!p.flat || !p.table || !p.out || p.n_seg < 1 || p.max_rows < 1) return false;
    if (p.H < 1 || p.W < 1 || (long)p.H * p.W > TIF_MAX_PIXELS || p.C < 1 || p.C > TIF_MAX_BANDS) return false;
    if (p.B != 1 && p.B != 2 && p.B != 4) return false;
    if (reinterpret_cast<uintptr_t>(p.out) & (uintptr_t)(p.B - 1)) return false;
    if (reinterpret_cast<uintptr_t>(p.flat) & (TIF_ALIGN - 1)) return false;
    if (p.predictor == 2 ? p.B == 4 : p.predictor == 3 ? p.B != 4 : p.predictor != 1) return false;
    return (long)p.n_seg * p.max_rows <= (1L << 40);
}

// The host copy of the table against the flat array and the raster; *max_rows receives the largest `rows`.
inline bool tif_table_ok(const int64_t* t, long n_seg, long flat_bytes, int H, int W, int C, int B, long* max_rows) {
    long mr = 0;
    for (long k = 0; k < n_seg; ++k) {
        const int64_t* r = t + k * TIF_TABLE_COLS;
        const int64_t off = r[0], bytes = r[1], row0 = r[2], col0 = r[3], rows = r[4], cols = r[5], band = r[6];
        if (band < -1 || band >= C || rows < 1 || cols < 1 || rows > (1 << 24) || cols > (1 << 24)) return false;
        if (row0 < 0 || row0 >= H || col0 < 0 || col0 >= W) return false;
        const int64_t S = band < 0 ? C : 1;
        if (bytes != rows * cols * S * B || off < 0 || (off & (TIF_ALIGN - 1)) || off > flat_bytes || bytes > flat_bytes - off) return false;
        if (cols * S * 4 > 2147483647L) return false;
        mr = rows > mr ? rows : mr;
    }
    *max_rows = mr;
    return n_seg >= 1;
}

// ---- one row of one segment -----------------------------------------------------------------------------------------------------------
struct TifRow {
    const uint8_t* src;                  // the row's first byte in the flat array
    long dst;                            // the SAMPLE of out its first sample goes to; sample ch of its pixel x goes to dst + x C + ch
    int S;                               // interleaved samples of a pixel in the segment: C (chunky) or 1 (planar)
    int cols, vc;                        // the row's columns in the segment, and those of them inside the raster
    long n;                              // the elements that are scanned: vc S samples, or for predictor 3 all cols S 4 bytes
    bool live;                           // false: the item is beyond the segment's rows or the raster's
};

SRH_TIF_HD TifRow tif_row(const TiffParams& p, long item) {
    const long seg = item / p.max_rows, r = item % p.max_rows;
    const int64_t* t = p.table + seg * TIF_TABLE_COLS;
    const long off = t[0], row0 = t[2], col0 = t[3], rows = t[4], cols = t[5], band = t[6];
    TifRow w;
    w.live = r < rows && row0 + r < p.H;
    w.S = band < 0 ? p.C : 1;
    w.cols = (int)cols;
    w.vc = (int)(cols < p.W - col0 ? cols : p.W - col0);
    w.src = p.flat + off + r * cols * w.S * p.B;
    w.dst = ((row0 + r) * p.W + col0) * p.C + (band < 0 ? 0 : band);
    w.n = p.predictor == 3 ? cols * w.S * 4 : (long)w.vc * w.S;
    return w;
}

SRH_TIF_HD int tif_chunk_pixels(int S) { return TIF_CHUNK / S; }
SRH_TIF_HD int tif_chunk_elems(int S) { return tif_chunk_pixels(S) * S; }
SRH_TIF_HD int tif_thread_pixels(int S) { return (tif_chunk_pixels(S) + TIF_THREADS - 1) / TIF_THREADS; }
SRH_TIF_HD int tif_pad(int i) { return i + (i >> 5); }

// Element e of the row (0 <= e < n), as the word that is summed: the ONLY read of the flat array.
SRH_TIF_HD uint32_t tif_load(const TiffParams& p, const TifRow& w, long e) {
    if (p.predictor == 3 || p.B == 1) return w.src[e];
    if (p.B == 2) {
        const uint32_t v = *reinterpret_cast<const uint16_t*>(w.src + 2 * e);
        return p.big_endian ? ((v & 0xFFu) << 8) | (v >> 8) : v;
    }
    const uint32_t v = *reinterpret_cast<const uint32_t*>(w.src + 4 * e);
    return p.big_endian ? (v << 24) | ((v & 0xFF00u) << 8) | ((v >> 8) & 0xFF00u) | (v >> 24) : v;
}

// Thread t's pixels of a chunk of npix pixels: [t PP, min((t + 1) PP, npix)).  The sum of their sample c ...
SRH_TIF_HD uint32_t tif_local_sum(const uint32_t* buf, int S, int t, int c, int npix) {
    const int pp = tif_thread_pixels(S), lo = t * pp, hi = lo + pp < npix ? lo + pp : npix;
    uint32_t acc = 0u;
    for (int px = lo; px < hi; ++px) acc += buf[tif_pad(px * S + c)];
    return acc;
}

// ... and their running sums in place, from `base`, the total of sample c over everything in front of the thread's first pixel.
SRH_TIF_HD void tif_local_apply(uint32_t* buf, int S, int t, int c, int npix, uint32_t base) {
    const int pp = tif_thread_pixels(S), lo = t * pp, hi = lo + pp < npix ? lo + pp : npix;
    for (int px = lo; px < hi; ++px) {
        base += buf[tif_pad(px * S + c)];
        buf[tif_pad(px * S + c)] = base;
    }
}

SRH_TIF_HD void tif_store_sample(const TiffParams& p, long sample, uint32_t v) {
    if (p.B == 1) p.out[sample] = (uint8_t)v;
    else if (p.B == 2) reinterpret_cast<uint16_t*>(p.out)[sample] = (uint16_t)v;
    else reinterpret_cast<uint32_t*>(p.out)[sample] = v;
}

// Thread t's share of storing the chunk that starts at element k0 and holds ne elements: the ONLY writes of the launch.
//   predictor 3: element e is byte (3 - e / (cols S)) of the little-endian float e % (cols S) of the row: one byte store each, for the
//                floats of the columns inside the raster;
//   planar:      sample x of the row goes to dst + x C, one store of B bytes each;
//   chunky:      the chunk is ne consecutive samples of the raster from dst + k0: whole aligned 16-byte words of them are stored as such,
//                the samples in front of the first and behind the last one by one.
SRH_TIF_HD void tif_store(const TiffParams& p, const TifRow& w, long k0, int ne, int t, const uint32_t* buf) {
    if (p.predictor == 3) {
        const long n1 = (long)w.cols * w.S;
        for (int i = t; i < ne; i += TIF_THREADS) {
            const long e = k0 + i, plane = e / n1, j = e % n1, x = j / w.S, ch = j % w.S;
            if (x < w.vc) p.out[(w.dst + x * p.C + ch) * 4 + (3 - plane)] = (uint8_t)buf[tif_pad(i)];
        }
        return;
    }
    if (w.S != p.C) {                                              // planar with C > 1 (a planar segment of a one-band raster is chunky)
        for (int i = t; i < ne; i += TIF_THREADS) tif_store_sample(p, w.dst + (k0 + i) * p.C, buf[tif_pad(i)]);
        return;
    }
    const long first = w.dst + k0;
    const int per = 16 / p.B;                                      // samples of a 16-byte word
    const uintptr_t a = reinterpret_cast<uintptr_t>(p.out) + (uintptr_t)first * p.B;
    int head = (int)(((16 - (a & 15)) & 15) / p.B);
    head = head < ne ? head : ne;
    const int words = (ne - head) / per;
    for (int g = t; g < words; g += TIF_THREADS) {
        const int i0 = head + g * per;
        TifWords q;
        if (p.B == 1) {
            for (int k = 0; k < 4; ++k)
                q.w[k] = (buf[tif_pad(i0 + 4 * k)] & 0xFFu) | ((buf[tif_pad(i0 + 4 * k + 1)] & 0xFFu) << 8) | ((buf[tif_pad(i0 + 4 * k + 2)] & 0xFFu) << 16) |
                         (buf[tif_pad(i0 + 4 * k + 3)] << 24);
        } else if (p.B == 2) {
            for (int k = 0; k < 4; ++k) q.w[k] = (buf[tif_pad(i0 + 2 * k)] & 0xFFFFu) | (buf[tif_pad(i0 + 2 * k + 1)] << 16);
        } else {
            for (int k = 0; k < 4; ++k) q.w[k] = buf[tif_pad(i0 + k)];
        }
        *reinterpret_cast<TifWords*>(p.out + (first + i0) * p.B) = q;
    }
    const int tail0 = head + words * per;
    for (int i = t; i < head + (ne - tail0); i += TIF_THREADS) {
        const int k = i < head ? i : tail0 + (i - head);
        tif_store_sample(p, first + k, buf[tif_pad(k)]);
    }
}

// ---- LZW (host) -------------------------------------------------------------------------------------------------------------------------
// TIFF LZW as every current writer emits it: codes most significant bit first, 9 to 12 bits, the width grows one code EARLY (when the next
// free entry is 2^width - 1), 256 clears the table, 257 ends the stream.  Decodes exactly `expected` bytes into out or returns non-zero:
// 1 the input ends early, 2 a code that no table entry stands for, 3 more bytes than expected, 4 fewer.  It reads in[0 .. in_bytes) and
// writes out[0 .. expected) and nothing else, whatever the stream holds.
inline int tif_lzw_decode(const uint8_t* in, long in_bytes, uint8_t* out, long expected) {
    uint16_t prefix[4096], len[4096];
    uint8_t suffix[4096], first[4096];
    for (int i = 0; i < 256; ++i) { prefix[i] = 0; len[i] = 1; suffix[i] = first[i] = (uint8_t)i; }
    int next = 258, width = 9, prev = -1;
    long pos = 0, o = 0;
    const long nbits = in_bytes * 8;
    while (o < expected) {
        if (pos + width > nbits) return 1;
        const long byte = pos >> 3;
        uint32_t word = 0;
        for (int j = 0; j < 4; ++j) word = (word << 8) | (byte + j < in_bytes ? in[byte + j] : 0u);
        const int code = (int)((word >> (32 - (int)(pos & 7) - width)) & ((1u << width) - 1u));
        pos += width;
        if (code == 257) break;
        if (code == 256) { next = 258; width = 9; prev = -1; continue; }
        if (prev < 0) {
            if (code > 255) return 2;
            out[o++] = (uint8_t)code;
        } else {
            if (code > next || (code == next && next >= 4096)) return 2;
            const int chain = code < next ? code : prev;           // code == next: the previous string and its own first byte again
            const long L = code < next ? len[code] : len[prev] + 1;
            if (L > expected - o) return 3;
            uint8_t* d = out + o + len[chain];
            for (int c = chain; ; c = prefix[c]) {
                *--d = suffix[c];
                if (c < 256) break;
            }
            if (code == next) out[o + L - 1] = first[prev];
            if (next < 4096) {
                prefix[next] = (uint16_t)prev; suffix[next] = first[chain]; first[next] = first[prev]; len[next] = (uint16_t)(len[prev] + 1);
                ++next;
            }
            o += L;
        }
        prev = code;
        if (next >= (1 << width) - 1 && width < 12) ++width;
    }
    return o == expected ? 0 : 4;
}

}  // namespace srh
