// Float32 scenes (config key SCENE_FLOAT): the three device steps between the upload of a raw f32 [n,C] scene and the u8
// [n,3] scene plus validity mask everything else has always seen.  The rule is stated on the host (sam_road_amd/float_scene.py) and the
// results must equal it byte for byte and count for count.  All three see n pixels of C floats and know nothing of H or W.  A float is
// read as its bit pattern and compared through the ordered key (scene_float_piece.hpp): integer compares only, no float arithmetic.  The
// reference has no such step.
//
// scene_float_valid: valid_out u8 [n], 0 / 1 by rule 1 (the three selected bands finite, none equal to a nodata key, > 0 under log, the
//   caller's mask non-zero).  Output-stationary: the work item is one 16-byte piece of valid_out cut at the 16-byte boundaries of the
//   ADDRESS, stored once; the first and last piece are clipped and stored as single bytes.  Only the selected bands are read.
// scene_float_hist: exact counting for the percentile.  Pass 1: hist u32 [3, 65536] over key >> 16 of the selected bands of the valid
//   pixels — the walk of scene_bands_hist_u16_kernel, counted in 48 KiB of LDS slots first, the wave peel (hist_wave.hpp) for what the
//   slots do not take.  Pass 2: hist u32 [n_targets, 65536] over key & 0xffff of the values whose band and key >> 16 match one of up to 6 targets.
//   Integer adds only: the counts do not depend on scheduling.  The rank arithmetic between and after the passes is the host's.
// scene_float_apply: dst u8 [n,3], byte 3 i + b = #{j : key(src[i][sel[b]]) >= thr[b][j]} for a valid pixel, 0 for an invalid one.  A
//   workgroup copies the 3 KiB of thresholds into the LDS; every value takes a branch-free binary search of 8 steps.  Output-stationary
//   in 16-byte pieces like scene_bands_apply; every byte of dst is written once and nothing else is.
#include "common.hpp"
#include "kernels.hpp"
#include "hist_wave.hpp"

namespace srh {

__global__ __launch_bounds__(FLOAT_THREADS) void scene_float_valid_kernel(SceneFloatParams p, long n_pieces) {
    for (long pc = (long)blockIdx.x * FLOAT_THREADS + threadIdx.x; pc < n_pieces; pc += (long)gridDim.x * FLOAT_THREADS) float_valid_piece(p, pc);
}

__global__ __launch_bounds__(FLOAT_THREADS) void scene_float_apply_kernel(SceneFloatParams p, long n_pieces) {
    __shared__ uint32_t tab[3 * 256];
    for (int i = threadIdx.x; i < 3 * 256; i += FLOAT_THREADS) tab[i] = p.thr[i];
    __syncthreads();
    for (long pc = (long)blockIdx.x * FLOAT_THREADS + threadIdx.x; pc < n_pieces; pc += (long)gridDim.x * FLOAT_THREADS) float_apply_piece(p, tab, pc);
}

// Pass 1.  A wave takes a contiguous span of the pixels, 64 per round, `rounds` of them (the host's division: the last waves may find
// nothing left); every lane makes every round: the wave stays whole for the ballots.  The top halves of a scene's floats fall into few
// of the 65536 counters (a binade has 128), and adds to ONE address are serial in the L2, so a workgroup counts in the LDS first: per
// band FLOAT_HIST_SLOTS slots, slot v mod FLOAT_HIST_SLOTS, a tag word that the first value to arrive claims (compare-and-swap in the
// LDS) and a counter.  A value that finds its slot held by another goes to the global table the way scene_bands_hist's values do
// (hist_wave_add: peel and pending run).  At the end a workgroup adds its non-zero slots to the table.  Integer adds only, each value
// counted exactly once in one place or the other: the sums do not depend on who claimed what.
constexpr int FLOAT_HIST_SLOTS = 2048;
constexpr uint32_t FLOAT_SLOT_EMPTY = 0xffffffffu;                 // no key >> 16 is this

__device__ __forceinline__ bool float_slot_add(uint32_t* tag, uint32_t* cnt, uint32_t v) {
    const uint32_t slot = v & (FLOAT_HIST_SLOTS - 1);
    const uint32_t old = atomicCAS(&tag[slot], FLOAT_SLOT_EMPTY, v);
    if (old != FLOAT_SLOT_EMPTY && old != v) return false;
    atomicAdd(&cnt[slot], 1u);
    return true;
}

__global__ __launch_bounds__(FLOAT_THREADS) void scene_float_hist_kernel(SceneFloatParams p, long rounds) {
    __shared__ uint32_t tag[3 * FLOAT_HIST_SLOTS];
    __shared__ uint32_t cnt[3 * FLOAT_HIST_SLOTS];
    for (int i = threadIdx.x; i < 3 * FLOAT_HIST_SLOTS; i += FLOAT_THREADS) { tag[i] = FLOAT_SLOT_EMPTY; cnt[i] = 0u; }
    __syncthreads();
    const int s0 = p.sel[0], s1 = p.sel[1], s2 = p.sel[2];
    const int lane = (int)(threadIdx.x & 63);
    const long wave = (long)blockIdx.x * (FLOAT_THREADS / 64) + (threadIdx.x >> 6);
    long i = wave * rounds * 64 + lane;
    uint32_t pv0 = 0xffffffffu, pv1 = 0xffffffffu, pv2 = 0xffffffffu, pn0 = 0u, pn1 = 0u, pn2 = 0u;
    for (long r = 0; r < rounds; ++r, i += 64) {
        const bool active = i < p.n && p.valid[i] != 0;
        uint32_t a = 0u, b = 0u, c = 0u;
        bool ga = false, gb = false, gc = false;                      // the value goes to the global table
        if (active) {
            const uint32_t* s = p.src + i * p.C;
            a = float_key(s[s0]) >> 16; b = float_key(s[s1]) >> 16; c = float_key(s[s2]) >> 16;
            ga = !float_slot_add(tag, cnt, a);
            gb = !float_slot_add(tag + FLOAT_HIST_SLOTS, cnt + FLOAT_HIST_SLOTS, b);
            gc = !float_slot_add(tag + 2 * FLOAT_HIST_SLOTS, cnt + 2 * FLOAT_HIST_SLOTS, c);
        }
        hist_wave_add(p.hist, a, ga, pv0, pn0, lane);
        hist_wave_add(p.hist + 65536, b, gb, pv1, pn1, lane);
        hist_wave_add(p.hist + 131072, c, gc, pv2, pn2, lane);
    }
    hist_wave_flush(p.hist, pv0, pn0, lane);
    hist_wave_flush(p.hist + 65536, pv1, pn1, lane);
    hist_wave_flush(p.hist + 131072, pv2, pn2, lane);
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * FLOAT_HIST_SLOTS; i += FLOAT_THREADS)
        if (cnt[i]) atomicAdd(&p.hist[(i / FLOAT_HIST_SLOTS) * 65536 + tag[i]], cnt[i]);      // cnt != 0: the slot is claimed, tag <= 65535
}

// Pass 2: the same walk; target t counts the low halves of the keys of band tband[t] whose top half is tprefix[t].  The loop over the
// targets is unrolled with constant indices (t < n_targets is uniform), so the pending runs stay in registers.
__global__ __launch_bounds__(FLOAT_THREADS) void scene_float_hist_low_kernel(SceneFloatParams p, long rounds) {
    const int lane = (int)(threadIdx.x & 63);
    const long wave = (long)blockIdx.x * (FLOAT_THREADS / 64) + (threadIdx.x >> 6);
    long i = wave * rounds * 64 + lane;
    uint32_t pv[FLOAT_MAX_TARGETS], pn[FLOAT_MAX_TARGETS];
#pragma unroll
    for (int t = 0; t < FLOAT_MAX_TARGETS; ++t) { pv[t] = 0xffffffffu; pn[t] = 0u; }
    for (long r = 0; r < rounds; ++r, i += 64) {
        const bool counted = i < p.n && p.valid[i] != 0;
        const uint32_t* s = p.src + (counted ? i : 0) * p.C;
#pragma unroll
        for (int t = 0; t < FLOAT_MAX_TARGETS; ++t) {
            if (t >= p.n_targets) break;
            const uint32_t k = counted ? float_key(s[p.tband[t]]) : 0u;
            hist_wave_add(p.hist + (long)t * 65536, k & 0xffffu, counted && (k >> 16) == p.tprefix[t], pv[t], pn[t], lane);
        }
    }
#pragma unroll
    for (int t = 0; t < FLOAT_MAX_TARGETS; ++t)
        if (t < p.n_targets) hist_wave_flush(p.hist + (long)t * 65536, pv[t], pn[t], lane);
}

// Pass 1 keeps 48 KiB of LDS per workgroup: the workgroups one device holds at a time, CUs x (LDS per CU / 48 KiB) — 256 x 3 on an
// MI355X.  More would only queue, and every workgroup ends with a flush of its slots.  768 where the device does not say.
static long float_hist_resident() {
    int dev = 0, cus = 0, lds = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, dev) != hipSuccess || cus < 1)
        return 768;
    const long per_cu = lds / (long)(2 * 3 * FLOAT_HIST_SLOTS * sizeof(uint32_t));
    return (long)cus * (per_cu < 1 ? 1 : per_cu);
}

static unsigned float_grid(long items, long cap) {
    const long g = (items + FLOAT_THREADS - 1) / FLOAT_THREADS;
    return (unsigned)(g < cap ? g : cap);
}

int launch_scene_float_valid(const SceneFloatParams& p, hipStream_t s) {
    if (!float_params_ok(p) || !p.valid_out) return -2;
    const long n_pieces = float_valid_pieces(p);
    hipLaunchKernelGGL(scene_float_valid_kernel, dim3(float_grid(n_pieces, 1L << 20)), dim3(FLOAT_THREADS), 0, s, p, n_pieces);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_scene_float_hist(const SceneFloatParams& p, hipStream_t s) {
    if (!float_params_ok(p) || !p.valid || !p.hist) return -2;
    const int rows = p.n_targets ? p.n_targets : 3;
    if (hipMemsetAsync(p.hist, 0, (size_t)rows * 65536 * sizeof(uint32_t), s) != hipSuccess) return -3;
    const unsigned grid = float_grid(p.n, p.n_targets ? 2048 : float_hist_resident());      // pass 2: 8 workgroups per CU, as scene_bands_hist
    const long n_waves = (long)grid * (FLOAT_THREADS / 64);
    const long rounds = ((p.n + 63) / 64 + n_waves - 1) / n_waves;    // rounds per wave
    if (p.n_targets) hipLaunchKernelGGL(scene_float_hist_low_kernel, dim3(grid), dim3(FLOAT_THREADS), 0, s, p, rounds);
    else hipLaunchKernelGGL(scene_float_hist_kernel, dim3(grid), dim3(FLOAT_THREADS), 0, s, p, rounds);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_scene_float_apply(const SceneFloatParams& p, hipStream_t s) {
    if (!float_params_ok(p) || !p.valid || !p.thr || !p.dst) return -2;
    const long n_pieces = float_apply_pieces(p);
    hipLaunchKernelGGL(scene_float_apply_kernel, dim3(float_grid(n_pieces, 1L << 16)), dim3(FLOAT_THREADS), 0, s, p, n_pieces);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace srh
