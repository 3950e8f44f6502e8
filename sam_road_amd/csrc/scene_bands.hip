// 16-bit and multi-band scenes (config key SCENE_BANDS): the two device steps between the upload of a raw scene and the
// u8 [H,W,3] scene everything else has always seen.  Both see the scene as n pixels of C elements (u8, 256 levels, or u16, 65536 levels)
// and know nothing of H or W, so one launch serves a scene and the ragged buffer of a scene group alike.  The reference has no such step.
//
// scene_bands_hist: hist u32 [3, levels], hist[b][v] = the number of counted pixels whose band sel[b] holds v.  Integer adds only, so the
//   counts are exact and do not depend on scheduling.  256 levels: a workgroup counts into 3 KiB of LDS and adds its non-zero counters to
//   the table once.  65536 levels: three tables are 768 KiB, more than the LDS, and stay in global memory (they fit the L2 many times);
//   the adds are device-scope and return nothing.  What makes the difference between 4 M adds on one address and 64 k of them is the
//   wave: before it adds, a wave peels off up to HIST_PEEL values that several of its lanes hold — the lane count is added once — and
//   only the lanes left over add 1 each; and a wave walks a contiguous span of the pixels and keeps the first peeled value as a pending
//   run, added once when another value ends it.  A constant scene costs one add per wave and band in all (adds to ONE address are
//   serial in the L2: ~12 ns each, measured); natural imagery, whose neighbours often agree, saves what it can; uniform noise pays the
//   (cheap, uniform) peel rounds and then adds lane by lane, spread over the table.
// scene_bands_apply: dst u8 [n,3], byte 3 i + b = lut[b][src[i][sel[b]]].  Output-stationary like scene_pad: the work item is one 16-byte
//   piece of dst cut at the 16-byte boundaries of the ADDRESS (scene_bands_piece.hpp), stored once; the first and last piece are clipped
//   to dst and stored as single bytes.  Only the selected bands are read, element by element (consecutive lanes read consecutive pixels);
//   the tables are gathered through the cache — 768 B for u8, 192 KiB for u16, of which an image touches the span it occupies.
#include "common.hpp"
#include "kernels.hpp"
#include "hist_wave.hpp"

namespace srh {

template <class T>
__global__ __launch_bounds__(BANDS_THREADS) void scene_bands_apply_kernel(SceneBandsParams p, long n_pieces) {
    for (long pc = (long)blockIdx.x * BANDS_THREADS + threadIdx.x; pc < n_pieces; pc += (long)gridDim.x * BANDS_THREADS) bands_piece<T>(p, pc);
}

__global__ __launch_bounds__(BANDS_THREADS) void scene_bands_hist_u8_kernel(SceneBandsParams p) {
    __shared__ uint32_t cnt[3 * 256];
    for (int i = threadIdx.x; i < 3 * 256; i += BANDS_THREADS) cnt[i] = 0u;
    __syncthreads();
    const uint8_t* src = static_cast<const uint8_t*>(p.src);
    const int s0 = p.sel[0], s1 = p.sel[1], s2 = p.sel[2];
    for (long i = (long)blockIdx.x * BANDS_THREADS + threadIdx.x; i < p.n; i += (long)gridDim.x * BANDS_THREADS) {
        if (p.valid && !p.valid[i]) continue;
        const uint8_t* s = src + i * p.C;
        atomicAdd(&cnt[s[s0]], 1u);
        atomicAdd(&cnt[256 + s[s1]], 1u);
        atomicAdd(&cnt[512 + s[s2]], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * 256; i += BANDS_THREADS)
        if (cnt[i]) atomicAdd(&p.hist[i], cnt[i]);
}

// A wave takes a contiguous span of the pixels, 64 per round, so that consecutive rounds are neighbours in the image and a run of equal
// values (nodata, saturation, water) carries over from round to round.  Every lane makes every round: the wave stays whole for the ballots.
__global__ __launch_bounds__(BANDS_THREADS) void scene_bands_hist_u16_kernel(SceneBandsParams p) {
    const uint16_t* src = static_cast<const uint16_t*>(p.src);
    const int s0 = p.sel[0], s1 = p.sel[1], s2 = p.sel[2];
    const int lane = (int)(threadIdx.x & 63);
    const long n_waves = (long)gridDim.x * (BANDS_THREADS / 64);
    const long rounds = ((p.n + 63) / 64 + n_waves - 1) / n_waves;    // rounds per wave; the last waves may find nothing left
    const long wave = (long)blockIdx.x * (BANDS_THREADS / 64) + (threadIdx.x >> 6);
    long i = wave * rounds * 64 + lane;
    uint32_t pv0 = 0xffffffffu, pv1 = 0xffffffffu, pv2 = 0xffffffffu, pn0 = 0u, pn1 = 0u, pn2 = 0u;
    for (long r = 0; r < rounds; ++r, i += 64) {
        bool active = i < p.n;
        if (active && p.valid) active = p.valid[i] != 0;
        uint32_t a = 0u, b = 0u, c = 0u;
        if (active) {
            const uint16_t* s = src + i * p.C;
            a = s[s0]; b = s[s1]; c = s[s2];
        }
        hist_wave_add(p.hist, a, active, pv0, pn0, lane);
        hist_wave_add(p.hist + 65536, b, active, pv1, pn1, lane);
        hist_wave_add(p.hist + 131072, c, active, pv2, pn2, lane);
    }
    hist_wave_flush(p.hist, pv0, pn0, lane);
    hist_wave_flush(p.hist + 65536, pv1, pn1, lane);
    hist_wave_flush(p.hist + 131072, pv2, pn2, lane);
}

static unsigned bands_grid(long items, long cap) {
    const long g = (items + BANDS_THREADS - 1) / BANDS_THREADS;
    return (unsigned)(g < cap ? g : cap);
}

int launch_scene_bands_hist(const SceneBandsParams& p, hipStream_t s) {
    if (!bands_params_ok(p) || !p.hist) return -2;
    if (hipMemsetAsync(p.hist, 0, (size_t)3 * (p.wide ? 65536 : 256) * sizeof(uint32_t), s) != hipSuccess) return -3;
    const unsigned grid = bands_grid(p.n, 2048);                      // 8 workgroups per CU: a workgroup's flush (u8) stays small against its share
    if (p.wide) hipLaunchKernelGGL(scene_bands_hist_u16_kernel, dim3(grid), dim3(BANDS_THREADS), 0, s, p);
    else hipLaunchKernelGGL(scene_bands_hist_u8_kernel, dim3(grid), dim3(BANDS_THREADS), 0, s, p);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_scene_bands_apply(const SceneBandsParams& p, hipStream_t s) {
    if (!bands_params_ok(p) || !p.lut || !p.dst) return -2;
    const long n_pieces = bands_n_pieces(p);
    const unsigned grid = bands_grid(n_pieces, 1L << 20);
    if (p.wide) hipLaunchKernelGGL(scene_bands_apply_kernel<uint16_t>, dim3(grid), dim3(BANDS_THREADS), 0, s, p, n_pieces);
    else hipLaunchKernelGGL(scene_bands_apply_kernel<uint8_t>, dim3(grid), dim3(BANDS_THREADS), 0, s, p, n_pieces);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace srh
