// Window-weighted fusion of overlapping tiles (config key FUSE_WINDOW): the weighted forms of the three canvas steps of a scene.  The
// reference fuses with a uniform mean (inferencer.py:79-110); the behaviour here is defined in DESIGN.md §6e.  profile = f32 [P], every
// value in [2^-20, 2^20]; the weight of tile t at scene pixel (x, y) is w = profile[x - x0_t] * profile[y - y0_t], one f32 product.
// None of these kernels runs for a scene without a window, and none of the existing scene kernels (decoder.hip, scene_valid.hip) is
// touched.
//
// Layout of both kernels: a workgroup owns 256 consecutive pixels of ONE canvas row, a wave 64 of them, so y is the same in every lane
// of a wave and the tiles that can touch the wave's pixels are found once per wave, not once per pixel: lane l reads the origin of
// tile base + l (one coalesced load for 64 tiles), tests it against the wave's row segment, and a ballot gives the covering tiles
// as a bit mask.  The wave then walks the set bits in ascending order — the tile order of the list, which is the summation order —
// with the tile origin read out of the owning lane into scalar registers.  The work per pixel follows the number of tiles that cover it
// (about 25 of the 256 tiles of a CityScale scene), where the unweighted kernels test every tile of the list in every lane; a wave that
// no tile of the call touches reads and writes nothing, so an add is confined to the rows and columns of its batch's tiles without
// the host knowing the tile list (it lives on the device).  profile[y - y0] is wave-uniform (a scalar load), profile[x - x0] one coalesced read of a
// table of at most 4 KiB that stays in L1 / L2.
#include "common.hpp"
#include "kernels.hpp"

namespace srh {

constexpr int SW_THREADS = 256;

// f(t, x0, y0) for every tile of tile_xy[0 .. n) that intersects row y in the columns [xw, xw + 64), in ascending t; t, x0 and y0 are
// wave-uniform.  Every lane of the wave must call it (ballot / readlane), whether its own pixel exists or not.
template <class F>
__device__ __forceinline__ void for_covering_tiles(const int* __restrict__ tile_xy, int n, int P, int y, int xw, F&& f) {
    const int lane = threadIdx.x & 63;
    for (int base = 0; base < n; base += 64) {
        const int t = base + lane;
        int x0 = 0, y0 = 0;
        bool hit = false;
        if (t < n) {
            x0 = tile_xy[2 * t]; y0 = tile_xy[2 * t + 1];
            hit = y >= y0 && y - y0 < P && x0 < xw + 64 && x0 + P > xw;
        }
        unsigned long long m = __ballot(hit);
        while (m) {
            const int j = __builtin_amdgcn_readfirstlane(__ffsll((long long)m) - 1);
            m &= m - 1;
            f(base + j, __builtin_amdgcn_readlane(x0, j), __builtin_amdgcn_readlane(y0, j));
        }
    }
}

// The pixel of this thread: workgroup b owns row b / chunks, columns (b % chunks) * 256 .. + 255 (chunks = ceil(W / 256)).
struct RowPixel { int x, y, xw; bool live; long gid; };
__device__ __forceinline__ RowPixel row_pixel(int W) {
    const int chunks = (W + SW_THREADS - 1) / SW_THREADS;
    RowPixel p;
    p.y = (int)(blockIdx.x / (unsigned)chunks);
    const int xb = (int)(blockIdx.x % (unsigned)chunks) * SW_THREADS;
    p.xw = xb + (int)(threadIdx.x & ~63u);
    p.x = xb + (int)threadIdx.x;
    p.live = p.x < W;
    p.gid = (long)p.y * W + p.x;
    return p;
}

// ---- canvas += w * score for one batch of tiles ------------------------------------------------------------------------------
// One fused multiply-add per term and channel, terms in tile order: the result does not depend on how the tile list is cut into calls
// (the canvas travels between calls as the same f32 the register holds).  A pixel no tile of the call covers is neither read nor written.
__global__ __launch_bounds__(SW_THREADS) void scene_add_window_kernel(const float* __restrict__ scores, int B, int P,
                                                                      const int* __restrict__ tile_xy, const float* __restrict__ profile,
                                                                      float* kp, float* road, int H, int W) {
    const RowPixel px = row_pixel(W);
    if (px.y >= H) return;                                    // (the grid is exact; wave-uniform in any case)
    float a = 0.f, r = 0.f;
    bool touched = false;
    for_covering_tiles(tile_xy, B, P, px.y, px.xw, [&](int t, int x0, int y0) {
        const int ly = px.y - y0, lx = px.x - x0;
        const float wy = profile[ly];
        if (px.live && lx >= 0 && lx < P) {
            if (!touched) { a = kp[px.gid]; r = road[px.gid]; touched = true; }
            const float w = __fmul_rn(profile[lx], wy);
            const float2 v = *reinterpret_cast<const float2*>(scores + (((size_t)t * P + ly) * P + lx) * 2);
            a = __fmaf_rn(w, v.x, a);
            r = __fmaf_rn(w, v.y, r);
        }
    });
    if (touched) { kp[px.gid] = a; road[px.gid] = r; }
}

int launch_scene_add_window(const float* scores, int B, int P, const int* tile_xy, const float* profile, float* kp, float* road, int H,
                            int W, hipStream_t s) {
    if (B <= 0) return 0;
    const long blocks = (long)H * ((W + SW_THREADS - 1) / SW_THREADS);
    if (blocks > 2147483647L) return -2;
    hipLaunchKernelGGL(scene_add_window_kernel, dim3((unsigned)blocks), dim3(SW_THREADS), 0, s, scores, B, P, tile_xy, profile, kp, road, H, W);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

// ---- weight sum + normalise: canvases -> u8 masks --------------------------------------------------------------------------
// Wsum = sum of w over ALL tiles of the list, in list order, kept in a register: no H x W counter canvas is written and read back (the
// unweighted path's scene_count + scene_normalise pair).  (canvas / Wsum) * 255 is the expression of scene_norm_kernel with Wsum in
// the place of the count: an all-ones profile sums 1.0 per covering tile, exactly the count, and gives the same bytes.  Every weight
// is positive, so Wsum > 0 exactly where a tile covers the pixel.  VALID: the masks are also 0 where valid[] is 0 (§6d point 5).
template <bool VALID>
__global__ __launch_bounds__(SW_THREADS) void scene_norm_window_kernel(const float* __restrict__ kp, const float* __restrict__ road, int H,
                                                                       int W, const int* __restrict__ tile_xy, int n, int P,
                                                                       const float* __restrict__ profile, const uint8_t* __restrict__ valid,
                                                                       uint8_t* __restrict__ kp_u8, uint8_t* __restrict__ road_u8) {
    const RowPixel px = row_pixel(W);
    if (px.y >= H) return;
    float c = 0.f;
    for_covering_tiles(tile_xy, n, P, px.y, px.xw, [&](int, int x0, int y0) {
        const int lx = px.x - x0;
        const float wy = profile[px.y - y0];
        if (px.live && lx >= 0 && lx < P) c = __fadd_rn(c, __fmul_rn(profile[lx], wy));
    });
    if (!px.live) return;
    bool on = c > 0.f;
    if (VALID) on = on && valid[px.gid] != 0;
    uint8_t a8 = 0, r8 = 0;
    if (on) {
        const float a = (kp[px.gid] / c) * 255.f, r = (road[px.gid] / c) * 255.f;
        a8 = (uint8_t)a; r8 = (uint8_t)r;
    }
    kp_u8[px.gid] = a8;
    road_u8[px.gid] = r8;
}

int launch_scene_normalise_window(const float* kp, const float* road, int H, int W, const int* tile_xy, int n_tiles, int P,
                                  const float* profile, const uint8_t* valid, uint8_t* kp_u8, uint8_t* road_u8, hipStream_t s) {
    const long blocks = (long)H * ((W + SW_THREADS - 1) / SW_THREADS);
    if (blocks > 2147483647L) return -2;
    if (valid)
        hipLaunchKernelGGL(scene_norm_window_kernel<true>, dim3((unsigned)blocks), dim3(SW_THREADS), 0, s, kp, road, H, W, tile_xy, n_tiles, P,
                           profile, valid, kp_u8, road_u8);
    else
        hipLaunchKernelGGL(scene_norm_window_kernel<false>, dim3((unsigned)blocks), dim3(SW_THREADS), 0, s, kp, road, H, W, tile_xy, n_tiles, P,
                           profile, valid, kp_u8, road_u8);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace srh
