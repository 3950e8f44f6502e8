// Test-time augmentation over the 8 tile orientations (config key TTA): the two permutation kernels pass 1 needs
// around the unchanged encoder and decoder.  None of them runs for the `id` orientation, and no existing kernel is touched.
//
// An orientation acts on a P x P tile T[row, col]; the oriented tile is O[ty, tx] = T[sy, sx] with
//     u  = SWAP ? tx : ty          sy = FLIP_Y ? P - 1 - u  : u             SWAP   = code >> 2
//     u' = SWAP ? ty : tx          sx = FLIP_X ? P - 1 - u' : u'            FLIP_Y = (code >> 1) & 1,  FLIP_X = code & 1
//   code  0 id   1 flip_h   2 flip_v   3 rot180   4 transpose   5 rot90   6 rot270   7 anti_transpose   (the numpy table of §6f)
// The oriented crop reads T through this map; the score un-orient writes scene[sy, sx] = oriented[ty, tx], the same map read the
// other way, so one pair of formulas serves both and the inverse orientation is never spelled out.
//
// Codes 1-3 keep rows as rows: a flip only reverses the order of the lanes inside a row (or the order of the rows), the accesses stay
// inside the same cache lines and nothing is staged.  Codes 4-7 turn a tile row into a scene column; both kernels take a block through
// the LDS so that global memory is read along scene / score rows and written along output rows: no load or store instruction has its
// lanes on 64 different rows.
#include "common.hpp"
#include "kernels.hpp"

namespace srh {

// ---- 1. oriented crop + normalise + im2col (u8 scene) ---------------------------------------------------------------------------
// The A matrix patch_im2col_kernel<true> (patch.hip) writes for the oriented tile, bit for bit: the same (v - mean) * rstd in f32, the
// same rounding to f16, the same K order k = ky*48 + kx*3 + c.
__device__ __forceinline__ f16 px_norm(uint8_t b, int c) {
    const float mean[3] = {123.675f, 116.28f, 103.53f};
    const float rstd[3] = {1.0f / 58.395f, 1.0f / 57.12f, 1.0f / 57.375f};
    return (f16)(((float)b - mean[c]) * rstd[c]);
}

// Codes 1-3.  One thread = 4 consecutive values of one oriented row, as in patch_im2col_kernel; with FLIP_X the pixels of the row are
// read from right to left (the channel order inside a pixel stays), so a thread's 4 bytes come from two neighbouring pixels.
__global__ __launch_bounds__(256) void patch_im2col_flip_kernel(PatchParams p, int flip_x, int flip_y) {
    const int S = p.P / 16, Q = p.P * 3 / 4;
    const long total = (long)p.B * p.P * Q;
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const int q = (int)(gid % Q);
    const int ty = (int)((gid / Q) % p.P);
    const int b = (int)(gid / ((long)Q * p.P));
    const int x0 = p.tile_xy[2 * b], y0 = p.tile_xy[2 * b + 1];
    const int sy = flip_y ? p.P - 1 - ty : ty;
    const uint8_t* row = reinterpret_cast<const uint8_t*>(p.src) + ((long)(y0 + sy) * p.scene_W + x0) * 3;
    const int e0 = 4 * q;
    const int px = e0 / 48, within = e0 % 48;
    f16x4 h;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int tx = (e0 + e) / 3, c = (e0 + e) % 3;
        const int sx = flip_x ? p.P - 1 - tx : tx;
        h[e] = px_norm(row[sx * 3 + c], c);
    }
    const long m = ((long)b * S + (ty >> 4)) * S + px;
    *reinterpret_cast<f16x4*>(p.out + m * 768 + (ty & 15) * 48 + within) = h;
}

// Codes 4-7.  A workgroup owns TT_TY oriented rows x 16 oriented columns of one tile = up to 4 whole rows of the A matrix (one per
// 16 oriented rows, 1536 contiguous bytes each).  Its source is 16 scene rows of TT_TY pixels (192 contiguous bytes at pitch 3 W).
//   load : the 16 row pieces as aligned dwords (a piece starts at any byte: rows of a u8 RGB scene are not 4-byte aligned, W may be odd,
//          x0 is arbitrary), consecutive lanes on consecutive dwords of one scene row; a dword that is not wholly inside the scene
//          (only the very first / last one of the allocation can be) is put together from the bytes that are.
//   store: item = (oriented row, 4-value piece) in the order of the A row, 8 bytes per lane, consecutive lanes on consecutive addresses.
// P is a multiple of 16 but need not be one of TT_TY: the last block of a tile column holds fewer oriented rows (P = 208: 16).
constexpr int TT_TY = 64;
constexpr int TT_PITCH = TT_TY * 3 / 4 + 1;              // dwords per staged row: 192 bytes + up to 3 bytes of misalignment

__global__ __launch_bounds__(256) void patch_im2col_transpose_kernel(PatchParams p, long scene_bytes, int flip_x, int flip_y) {
    __shared__ uint32_t stage[16 * TT_PITCH];
    const int P = p.P, S = P / 16;
    const int b = blockIdx.z, pxcol = blockIdx.y;       // oriented patch column: tx in [16 pxcol, 16 pxcol + 16)
    const int ty0 = blockIdx.x * TT_TY;
    const int nty = min(TT_TY, P - ty0);                // a multiple of 16
    const int x0 = p.tile_xy[2 * b], y0 = p.tile_xy[2 * b + 1];
    const int tx0 = pxcol * 16;
    // source rectangle in the tile: rows sy_lo .. + 15 (from tx), columns sx_lo .. + nty - 1 (from ty)
    const int sy_lo = flip_y ? P - tx0 - 16 : tx0;
    const int sx_lo = flip_x ? P - ty0 - nty : ty0;
    const uint8_t* base = reinterpret_cast<const uint8_t*>(p.src);
    const int ndw = TT_PITCH;                           // dwords fetched per row (the last may lie past the piece: guarded, unused)
    for (int i = threadIdx.x; i < 16 * ndw; i += 256) {
        const int r = i / ndw, j = i % ndw;
        const long a = ((long)(y0 + sy_lo + r) * p.scene_W + x0 + sx_lo) * 3;          // first byte of the piece, relative to the scene
        const long mis = (long)((reinterpret_cast<uintptr_t>(base) + (uintptr_t)a) & 3);
        const long off = a - mis + 4L * j;                                             // a dword-aligned address
        uint32_t v = 0;
        if (4 * j < nty * 3 + mis) {                                                   // this dword holds bytes of the piece
            if (off >= 0 && off + 4 <= scene_bytes) {
                v = *reinterpret_cast<const uint32_t*>(base + off);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (off + k >= 0 && off + k < scene_bytes) v |= (uint32_t)base[off + k] << (8 * k);
            }
        }
        stage[r * TT_PITCH + j] = v;
    }
    __syncthreads();
    const uint8_t* sb = reinterpret_cast<const uint8_t*>(stage);
    // every staged row has its own misalignment (odd pitch): recompute it per row when reading
    const int items = nty * 12;                          // 12 pieces of 4 values per oriented row and patch column
    for (int it = threadIdx.x; it < items; it += 256) {
        const int tyl = it / 12, q = it % 12;
        const int col = flip_x ? nty - 1 - tyl : tyl;    // pixel inside the staged piece
        f16x4 h;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int txl = (4 * q + e) / 3, c = (4 * q + e) % 3;
            const int r = flip_y ? 15 - txl : txl;
            const long a = ((long)(y0 + sy_lo + r) * p.scene_W + x0 + sx_lo) * 3;
            const int mis = (int)((reinterpret_cast<uintptr_t>(base) + (uintptr_t)a) & 3);
            h[e] = px_norm(sb[r * (TT_PITCH * 4) + mis + col * 3 + c], c);
        }
        const int ty = ty0 + tyl;
        const long m = ((long)b * S + (ty >> 4)) * S + pxcol;
        *reinterpret_cast<f16x4*>(p.out + m * 768 + (ty & 15) * 48 + 4 * q) = h;
    }
}

int launch_patch_im2col_oriented(const PatchParams& p, int scene_H, int orient, hipStream_t s) {
    if (orient < 1 || orient > 7 || !p.src_is_u8 || p.scene_W <= 0 || scene_H <= 0 || p.P < 16 || p.P % 16) return -2;
    if (p.B <= 0) return 0;
    const int fx = orient & 1, fy = (orient >> 1) & 1;
    if (orient < 4) {
        const long total = (long)p.B * p.P * (p.P * 3 / 4);
        hipLaunchKernelGGL(patch_im2col_flip_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, p, fx, fy);
    } else {
        if (p.B > 65535) return -2;
        const dim3 grid((unsigned)((p.P + TT_TY - 1) / TT_TY), (unsigned)(p.P / 16), (unsigned)p.B);
        hipLaunchKernelGGL(patch_im2col_transpose_kernel, grid, dim3(256), 0, s, p, (long)scene_H * p.scene_W * 3, fx, fy);
    }
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

// ---- 2. score un-orient: scores [B,P,P,2] f32 in the oriented frame -> the scene frame ----------------------------------------------
// A pure permutation of float2 values (bit patterns are copied, never computed with): out[b, sy, sx] = in[b, ty, tx].  in != out.
// Codes 1-3: one thread per output float2; with FLIP_X the lanes of a row read its float2s from right to left.
__global__ __launch_bounds__(256) void scores_unorient_flip_kernel(const float2* __restrict__ in, float2* __restrict__ out, int B, int P,
                                                                   int flip_x, int flip_y) {
    const long total = (long)B * P * P;
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const int sx = (int)(gid % P);
    const int sy = (int)((gid / P) % P);
    const long b = gid / ((long)P * P);
    const int ty = flip_y ? P - 1 - sy : sy, tx = flip_x ? P - 1 - sx : sx;
    out[gid] = in[(b * P + ty) * P + tx];
}

// Codes 4-7: a 32 x 32 block of float2 through the LDS.  Thread (lx, r): reads in[ty = fx(ox0 + r), tx = fy(oy0 + lx)] — the 32 lanes of
// a half wave cover 256 contiguous bytes of one input row — and writes out[oy0 + r, ox0 + lx] from the transposed position.  Pitch 33
// float2: the transposed 8-byte reads of a 32-lane group fall on 32 different bank pairs.  P need not be a multiple of 32 (208).
constexpr int UT = 32;

__global__ __launch_bounds__(256) void scores_unorient_transpose_kernel(const float2* __restrict__ in, float2* __restrict__ out, int P,
                                                                        int flip_x, int flip_y) {
    __shared__ float2 tile[UT][UT + 1];
    const int lx = threadIdx.x & 31, r0 = threadIdx.x >> 5;
    const int ox0 = blockIdx.x * UT, oy0 = blockIdx.y * UT;
    const long b = blockIdx.z;
    const float2* src = in + b * P * P;
    float2* dst = out + b * P * P;
    const int sy_in = oy0 + lx;                          // the scene row this lane's input column belongs to
#pragma unroll
    for (int r = r0; r < UT; r += 8) {
        const int sx = ox0 + r;
        if (sx < P && sy_in < P) {
            const int ty = flip_x ? P - 1 - sx : sx, tx = flip_y ? P - 1 - sy_in : sy_in;
            tile[r][lx] = src[(long)ty * P + tx];
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = r0; r < UT; r += 8) {
        const int sy = oy0 + r, sx = ox0 + lx;
        if (sy < P && sx < P) dst[(long)sy * P + sx] = tile[lx][r];
    }
}

int launch_scores_unorient(const float* in, int B, int P, int orient, float* out, hipStream_t s) {
    if (orient < 1 || orient > 7 || P <= 0) return -2;
    if (B <= 0) return 0;
    const int fx = orient & 1, fy = (orient >> 1) & 1;
    const float2* i2 = reinterpret_cast<const float2*>(in);
    float2* o2 = reinterpret_cast<float2*>(out);
    if (orient < 4) {
        const long total = (long)B * P * P;
        const long blocks = (total + 255) / 256;
        if (blocks > 2147483647L) return -2;
        hipLaunchKernelGGL(scores_unorient_flip_kernel, dim3((unsigned)blocks), dim3(256), 0, s, i2, o2, B, P, fx, fy);
    } else {
        if (B > 65535) return -2;
        const unsigned nb = (unsigned)((P + UT - 1) / UT);
        hipLaunchKernelGGL(scores_unorient_transpose_kernel, dim3(nb, nb, (unsigned)B), dim3(256), 0, s, i2, o2, P, fx, fy);
    }
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace srh
