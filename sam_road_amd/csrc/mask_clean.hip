// Connected-component filter of the scene masks on the device (config key MASK_CLEAN): n u8 images, dense blocks of one
// buffer described by a device table, are filtered IN PLACE — the pixels of every connected component (8- or 4-connectivity) of the
// foreground (level >= T_ON) whose area is below MIN_AREA or whose highest level is below T_PEAK become 0, every other byte stays.  The
// rule is stated on the host (sam_road_amd/mask_clean.py) and the result must equal mask_clean_ref byte for byte.  The reference has no
// such step.
//
// Label equivalence with a union-find in global memory, FIVE launches per call whatever the masks hold (mask_clean_piece.hpp has the
// per-lane code and the argument why every loop ends):
//   init    a foreground pixel's parent = the first pixel of its run inside its 64-pixel segment; background -1; statistics zeroed
//   merge   run starts and pixels under a change in the row above are united with their upper neighbours, segment starts with their
//           left neighbour: find both roots, atomicMin on the larger root's parent, retried while that one was no root any more
//   flatten every foreground pixel stores its root as its label
//   stats   per segment and label, the first run that carries the label adds the pixels of the segment's runs with that label to the
//           root's area (atomicAdd) and raises the root's peak to their highest level (atomicMax): one atomic pair per segment and label
//   apply   per segment and label, the first run that carries the label reads the root's area and peak and zeroes the segment's runs
//           with that label if the root fails the test
// A wave is one segment: its foreground word is a ballot, and the code of a lane (the piece) never talks to another lane.  No workgroup
// waits for another one: there is no lock, no flag and no grid barrier — kernel boundaries are the only global synchronisation, and
// nothing is read back.  Byte loads and stores through the vector memory path, int32 atomics, no LDS, no inline assembly.
#include "common.hpp"
#include "kernels.hpp"

namespace srh {

struct McDeviceOps {
    static __device__ __forceinline__ int load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    static __device__ __forceinline__ void store(int32_t* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    static __device__ __forceinline__ int min(int32_t* p, int v) { return atomicMin(p, v); }
    static __device__ __forceinline__ int add(int32_t* p, int v) { return atomicAdd(p, v); }
    static __device__ __forceinline__ int max(int32_t* p, int v) { return atomicMax(p, v); }
};

// the segment of this wave in round `it` of the grid-stride loop (uniform over the wave), or -1 past the end
static __device__ __forceinline__ long mc_wave_seg(const MaskCleanParams& p, long it) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long s = (it * gridDim.x + blockIdx.x) * (MC_THREADS / MC_SEG) + wave;
    return s < p.n_segs ? s : -1;
}

// every kernel: for (each segment of this wave) { the segment's foreground word by ballot; the lane's piece }
#define MC_SEGMENTS(p, s) long it_ = 0, s = mc_wave_seg(p, 0); s >= 0; s = mc_wave_seg(p, ++it_)

__global__ __launch_bounds__(MC_THREADS) void mask_clean_init_kernel(MaskCleanParams p) {
    const int lane = (int)(threadIdx.x & 63);
    for (MC_SEGMENTS(p, s)) {
        const McSeg g = mc_locate(p, s);
        const uint64_t cur = __ballot(mc_fg(g, g.y, g.x0 + lane));
        mc_init_lane<McDeviceOps>(p, g, lane, cur);
    }
}

__global__ __launch_bounds__(MC_THREADS) void mask_clean_merge_kernel(MaskCleanParams p) {
    const int lane = (int)(threadIdx.x & 63);
    for (MC_SEGMENTS(p, s)) {
        const McSeg g = mc_locate(p, s);
        const uint64_t cur = __ballot(mc_fg(g, g.y, g.x0 + lane));
        const uint64_t up = __ballot(mc_fg(g, g.y - 1, g.x0 + lane));
        // the three pixels beside the segment: the same address in every lane, one broadcast load each
        const bool up_l = mc_fg(g, g.y - 1, g.x0 - 1), up_r = mc_fg(g, g.y - 1, g.x0 + MC_SEG), left = mc_fg(g, g.y, g.x0 - 1);
        mc_merge_lane<McDeviceOps>(p, g, lane, cur, up, up_l, up_r, left);
    }
}

__global__ __launch_bounds__(MC_THREADS) void mask_clean_flatten_kernel(MaskCleanParams p) {
    const int lane = (int)(threadIdx.x & 63);
    for (MC_SEGMENTS(p, s)) {
        const McSeg g = mc_locate(p, s);
        const uint64_t cur = __ballot(mc_fg(g, g.y, g.x0 + lane));
        mc_flatten_lane<McDeviceOps>(p, g, lane, cur);
    }
}

__global__ __launch_bounds__(MC_THREADS) void mask_clean_stats_kernel(MaskCleanParams p) {
    const int lane = (int)(threadIdx.x & 63);
    for (MC_SEGMENTS(p, s)) {
        const McSeg g = mc_locate(p, s);
        const uint64_t cur = __ballot(mc_fg(g, g.y, g.x0 + lane));
        mc_stats_lane<McDeviceOps>(p, g, lane, cur);
    }
}

__global__ __launch_bounds__(MC_THREADS) void mask_clean_apply_kernel(MaskCleanParams p) {
    const int lane = (int)(threadIdx.x & 63);
    for (MC_SEGMENTS(p, s)) {
        const McSeg g = mc_locate(p, s);
        const uint64_t cur = __ballot(mc_fg(g, g.y, g.x0 + lane));       // before any lane of the wave stores: only this wave writes the segment
        mc_apply_lane<McDeviceOps>(p, g, lane, cur);
    }
}

// step 0 .. 4: init, merge, flatten, stats, apply.  The table has been checked on the host (mask_clean_table_ok); -2 for bad parameters.
int launch_mask_clean(const MaskCleanParams& p, int step, hipStream_t s) {
    if (!p.buf || !p.table || !p.parent || !p.area || !p.peak || p.n < 1 || p.n > MC_MAX_IMAGES || (p.conn != 4 && p.conn != 8) || p.n_segs < 1 ||
        step < 0 || step > 4)
        return -2;
    const long n_groups = (p.n_segs + MC_THREADS / MC_SEG - 1) / (MC_THREADS / MC_SEG);
    const dim3 grid((unsigned)(n_groups < (1L << 20) ? n_groups : (1L << 20))), block(MC_THREADS);
    if (step == 0) hipLaunchKernelGGL(mask_clean_init_kernel, grid, block, 0, s, p);
    else if (step == 1) hipLaunchKernelGGL(mask_clean_merge_kernel, grid, block, 0, s, p);
    else if (step == 2) hipLaunchKernelGGL(mask_clean_flatten_kernel, grid, block, 0, s, p);
    else if (step == 3) hipLaunchKernelGGL(mask_clean_stats_kernel, grid, block, 0, s, p);
    else hipLaunchKernelGGL(mask_clean_apply_kernel, grid, block, 0, s, p);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace srh
