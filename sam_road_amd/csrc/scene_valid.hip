// Per-pixel validity mask of a scene (nodata): which tiles hold data, nodata pixels neutralised before the crop, nodata kept out of
// the u8 masks.  The reference has no such notion; the behaviour is defined in DESIGN.md §6d.  valid = u8 [H,W], non-zero = valid.
// None of these kernels runs for a scene without a mask, and none of the existing scene kernels (decoder.hip) is touched.
#include "common.hpp"
#include "kernels.hpp"

namespace srh {

// Non-zero bytes of a 32-bit word: OR every byte's eight bits down into its bit 0, then count those.
__device__ __forceinline__ int nonzero_bytes(uint32_t w) {
    w |= w >> 1; w |= w >> 2; w |= w >> 4;
    return __popc(w & 0x01010101u);
}

// ---- valid pixels per tile --------------------------------------------------------------------------------------------------
// One workgroup per tile walks its P rows of P mask bytes.  256 tiles of 512^2 over a 4 MB mask are 67 M byte reads, nearly all L2
// hits (a pixel lies in ~16 tiles), so what matters is bytes per load instruction: a row is read as 16-byte loads between its first
// and last 16-byte boundary, and the up to 15 + 15 bytes before and after them one by one (tile origins are arbitrary and the rows
// of an odd W are not aligned against each other, so the split is made per row; nothing outside the row is read).  P is a multiple
// of 16, so a row is P / 16 work items: the aligned 16-byte pieces and, for a row that does not start on a boundary, one item that
// counts nothing there; the 16 head + tail bytes of unaligned rows are taken in a second, short loop, one row per thread.  Items are dealt
// lane-linear over (row, piece), consecutive lanes read consecutive pieces.  Integer counts: per-lane sum, wave shuffle reduction, one
// LDS step, one store per tile — exact, no atomics, no order.  The loop is bound by L2 latency, so what counts is loads in flight: 16
// waves on the tile's CU and a branch-free piece loop unrolled four times (14 us for the 256 tiles of a 2048-px CityScale scene,
// profiles/valid_mask_kernel_stats.csv; a 4-wave workgroup with the head / tail bytes inside the loop was several times slower).
// A tile that does not lie inside the scene is not read; its count is -1 (the caller guarantees that there is none, as for pass 1).
constexpr int TVC_THREADS = 1024;

__global__ __launch_bounds__(TVC_THREADS) void tile_valid_count_kernel(const uint8_t* __restrict__ valid, int H, int W,
                                                                       const int* __restrict__ tile_xy, int P, int* __restrict__ counts) {
    __shared__ int part[TVC_THREADS / 64];
    const int t = blockIdx.x, tid = threadIdx.x;
    const int x0 = tile_xy[2 * t], y0 = tile_xy[2 * t + 1];
    if (x0 < 0 || y0 < 0 || x0 > W - P || y0 > H - P) {          // uniform over the workgroup
        if (tid == 0) counts[t] = -1;
        return;
    }
    const uint8_t* const tile = valid + (size_t)y0 * W + x0;
    const int CH = P >> 4;                                        // items per row
    const int dr = TVC_THREADS / CH, dc = TVC_THREADS - dr * CH;  // the stride of one pass over the threads as (rows, pieces)
    int r = tid / CH, c = tid - r * CH;
    int cnt = 0;
    // the aligned pieces.  Item c of a row is its c-th aligned piece; an unaligned row has one piece less, and its last item (like an
    // item past the last row) re-reads piece 0 of a row — inside the row, P >= 32 — and counts nothing: no branch around the load
    const int passes = (P * CH + TVC_THREADS - 1) / TVC_THREADS;
#pragma unroll 4
    for (int it = 0; it < passes; ++it) {
        const bool in = r < P;
        const uint8_t* row = tile + (size_t)(in ? r : 0) * W;
        const int mis = (int)(reinterpret_cast<uintptr_t>(row) & 15);
        const int head = (16 - mis) & 15;                         // bytes before the first 16-byte boundary
        const bool body = in && c < (mis ? CH - 1 : CH);
        const uint4 v = *reinterpret_cast<const uint4*>(row + head + (body ? 16 * c : 0));
        const int k = nonzero_bytes(v.x) + nonzero_bytes(v.y) + nonzero_bytes(v.z) + nonzero_bytes(v.w);
        cnt += body ? k : 0;
        r += dr; c += dc;
        if (c >= CH) { c -= CH; ++r; }
    }
    // the 16 - mis head bytes and the mis tail bytes of every unaligned row
    for (int rr = tid; rr < P; rr += TVC_THREADS) {
        const uint8_t* row = tile + (size_t)rr * W;
        const int mis = (int)(reinterpret_cast<uintptr_t>(row) & 15);
        if (mis) {
            for (int j = 0; j < 16 - mis; ++j) cnt += row[j] != 0;
            for (int j = P - mis; j < P; ++j) cnt += row[j] != 0;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if ((tid & 63) == 0) part[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) {
        int s = 0;
#pragma unroll
        for (int i = 0; i < TVC_THREADS / 64; ++i) s += part[i];
        counts[t] = s;
    }
}

int launch_tile_valid_count(const uint8_t* valid, int H, int W, const int* tile_xy, int n_tiles, int P, int* counts, hipStream_t s) {
    if (n_tiles <= 0) return 0;
    if (P < 32 || (P & 15)) return -2;
    hipLaunchKernelGGL(tile_valid_count_kernel, dim3((unsigned)n_tiles), dim3(TVC_THREADS), 0, s, valid, H, W, tile_xy, P, counts);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

// ---- nodata -> fill colour, in place ----------------------------------------------------------------------------------------
// One pass over the mask; the scene is only touched where a pixel is invalid.  VEC: four pixels per thread — one mask word and, if
// any of its bytes is zero, the 12 scene bytes as three words (both base addresses 4-byte aligned; 4 pixels x 3 bytes keeps every
// group on a word boundary).  Otherwise (and for the last n % 4 pixels) one pixel per thread.
template <bool VEC>
__global__ __launch_bounds__(256) void scene_fill_invalid_kernel(uint8_t* __restrict__ scene, const uint8_t* __restrict__ valid, long n,
                                                                 long first, uint32_t fr, uint32_t fg, uint32_t fb) {
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (VEC) {
        if (gid >= (n >> 2)) return;
        const uint32_t m = reinterpret_cast<const uint32_t*>(valid)[gid];
        if (nonzero_bytes(m) == 4) return;
        uint32_t* px = reinterpret_cast<uint32_t*>(scene) + 3 * gid;
        uint32_t w[3] = {px[0], px[1], px[2]};
        const uint32_t f[3] = {fr, fg, fb};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if ((m >> (8 * k)) & 0xffu) continue;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const int b = 3 * k + ch;                         // byte b of the group: word b / 4, byte b % 4 (little endian)
                w[b >> 2] = (w[b >> 2] & ~(0xffu << (8 * (b & 3)))) | (f[ch] << (8 * (b & 3)));
            }
        }
        px[0] = w[0]; px[1] = w[1]; px[2] = w[2];
    } else {
        const long i = first + gid;
        if (i >= n || valid[i]) return;
        scene[3 * i] = (uint8_t)fr; scene[3 * i + 1] = (uint8_t)fg; scene[3 * i + 2] = (uint8_t)fb;
    }
}

int launch_scene_fill_invalid(uint8_t* scene, const uint8_t* valid, int H, int W, int fr, int fg, int fb, hipStream_t s) {
    const long n = (long)H * W;
    const bool vec = ((reinterpret_cast<uintptr_t>(scene) | reinterpret_cast<uintptr_t>(valid)) & 3) == 0 && n >= 4;
    const long first = vec ? (n & ~3L) : 0;                       // pixels the one-per-thread form takes: all, or the last n % 4
    if (vec)
        hipLaunchKernelGGL(scene_fill_invalid_kernel<true>, dim3((unsigned)(((n >> 2) + 255) / 256)), dim3(256), 0, s, scene, valid, n, 0L,
                           (uint32_t)fr, (uint32_t)fg, (uint32_t)fb);
    if (n > first)
        hipLaunchKernelGGL(scene_fill_invalid_kernel<false>, dim3((unsigned)((n - first + 255) / 256)), dim3(256), 0, s, scene, valid, n, first,
                           (uint32_t)fr, (uint32_t)fg, (uint32_t)fb);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

// ---- canvases -> u8 masks, 0 on nodata --------------------------------------------------------------------------------------
// scene_norm_kernel (decoder.hip) with one more condition; a kernel of its own so that the unmasked one keeps its instruction
// stream.  The arithmetic of a valid, covered pixel is the same expression: an all-true mask gives the same bytes.
__global__ __launch_bounds__(256) void scene_norm_valid_kernel(SceneNormParams p, const uint8_t* __restrict__ valid) {
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= p.n) return;
    const float c = p.counter[gid];
    const float a = (p.canvas_kp[gid] / c) * 255.f, r = (p.canvas_road[gid] / c) * 255.f;
    const bool on = c > 0.f && valid[gid] != 0;
    p.kp_u8[gid] = on ? (uint8_t)a : (uint8_t)0;
    p.road_u8[gid] = on ? (uint8_t)r : (uint8_t)0;
}

int launch_scene_normalise_valid(const SceneNormParams& p, const uint8_t* valid, hipStream_t s) {
    hipLaunchKernelGGL(scene_norm_valid_kernel, dim3((unsigned)((p.n + 255) / 256)), dim3(256), 0, s, p, valid);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace srh
