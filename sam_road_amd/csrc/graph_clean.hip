// Spur and small-component pruning of the road graph on the device (config key GRAPH_CLEAN): the topology of the graph
// that leaves the TopoNet votes is decided here, in integers, in a fixed number of launches; the host only applies the keep mask.  The
// rule is stated on the host (sam_road_amd/graph_clean.py) and state / out must equal graph_clean_ref exactly.  The reference has no
// such step.
//
// A pass is FIVE launches, one work item per node or edge, grid-stride (graph_clean_piece.hpp has the per-item code, the argument why
// every loop ends and why every index stays inside):
//   init    node and edge parents = themselves; degrees, incident-edge slots and sums cleared (the first pass: live = 1, state = 0)
//   edges   per live edge: atomicAdd on the degree of both ends, atomicMin / atomicMax of the edge index into both ends' incident-edge
//           slots, mc_union of the two end nodes in the node forest
//   chains  per node of degree 2: mc_union of its two incident edges (its min and max slot) in the edge forest
//   sums    per live edge: both roots; 64-bit atomicAdd of len_q to the chain root and to the component root (equal component roots
//           summed inside the wave first), the edge's leaf and junction ends to the chain root
//   decide  per live edge: the roots' totals -> its own live byte and state; the final pass writes out instead, 16 bytes per edge
// 5 (rounds + 1) launches whatever the graph holds, nothing read back.  No workgroup waits for another one: there is no lock, no flag
// and no grid barrier — kernel boundaries are the only global synchronisation.  Plain loads and vector stores, int32 / int64 atomics, no
// LDS, no inline assembly.
#include "common.hpp"
#include "kernels.hpp"

namespace srh {

struct GcDeviceOps {
    static __device__ __forceinline__ int load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    static __device__ __forceinline__ void store(int32_t* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    static __device__ __forceinline__ int min(int32_t* p, int v) { return atomicMin(p, v); }
    static __device__ __forceinline__ int max(int32_t* p, int v) { return atomicMax(p, v); }
    static __device__ __forceinline__ int add(int32_t* p, int v) { return atomicAdd(p, v); }
    static __device__ __forceinline__ int64_t load64(const int64_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    static __device__ __forceinline__ void store64(int64_t* p, int64_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    static __device__ __forceinline__ void add64(int64_t* p, int64_t v) {
        atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);      // two's complement: the same bits
    }
};

// every kernel: for (each item of this thread) the item's piece
#define GC_ITEMS(i, n) long i = (long)blockIdx.x * GC_THREADS + threadIdx.x; i < (n); i += (long)gridDim.x * GC_THREADS

__global__ __launch_bounds__(GC_THREADS) void graph_clean_init_kernel(GraphCleanParams p) {
    const long n = p.N > p.E ? p.N : p.E;
    for (GC_ITEMS(i, n)) gc_init_item<GcDeviceOps>(p, i);
}

__global__ __launch_bounds__(GC_THREADS) void graph_clean_edges_kernel(GraphCleanParams p) {
    for (GC_ITEMS(e, p.E)) gc_edges_item<GcDeviceOps>(p, e);
}

__global__ __launch_bounds__(GC_THREADS) void graph_clean_chains_kernel(GraphCleanParams p) {
    for (GC_ITEMS(v, p.N)) gc_chains_item<GcDeviceOps>(p, v);
}

// One giant component sends every edge's 64-bit atomicAdd of the component sum to ONE address.  Measured on the 2048^2 bench scene's
// graph (35 771 edges, 33 177 of them in one component): the plain sums launch takes 1.21 ms of a call's 1.60 ms of kernel
// time, the wave-aggregated one 0.038 ms of 0.46 ms; 2.48 -> 0.061 ms on 4096^2 (68 961 edges).  The aggregated form was kept on that
// measurement; -DSRH_GC_WAVE_AGG=0 builds the plain one (gc_sums_item, which the CPU program runs).  The chain sums stay single atomics:
// chains are short and the roots of a wave's 64 edges mostly differ.
#ifndef SRH_GC_WAVE_AGG
#define SRH_GC_WAVE_AGG 1
#endif

#if SRH_GC_WAVE_AGG
// The component sums with equal roots aggregated inside a wave before the atomic (the readfirstlane loop of hist_wave.hpp): the leader's
// root is broadcast, the lanes that hold it are summed by six xor-shuffles and the leader adds once.  Two roots are peeled, the rest add
// singly.  Uniform control flow: every lane of a wave runs the same number of rounds.
constexpr int GC_PEEL = 2;
static __device__ __forceinline__ void gc_wave_add64(int64_t* table, int root, int64_t v, bool active, int lane) {
    unsigned long long todo = __ballot(active);
#pragma unroll
    for (int r = 0; r < GC_PEEL; ++r) {
        if (!todo) break;
        const int leader = __ffsll((long long)todo) - 1;
        const int r0 = __shfl(root, leader, 64);
        const bool mine = active && root == r0;
        const unsigned long long same = __ballot(mine);
        long long sum = mine ? (long long)v : 0;
        for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
        if (lane == leader) GcDeviceOps::add64(table + r0, sum);
        if (mine) active = false;
        todo &= ~same;
    }
    if (active) GcDeviceOps::add64(table + root, v);
}

__global__ __launch_bounds__(GC_THREADS) void graph_clean_sums_kernel(GraphCleanParams p) {
    const int lane = (int)(threadIdx.x & 63);
    const long stride = (long)gridDim.x * GC_THREADS;
    const long rounds = (p.E + stride - 1) / stride;
    long e = (long)blockIdx.x * GC_THREADS + threadIdx.x;
    for (long k = 0; k < rounds; ++k, e += stride) {
        GcSum s{false, 0, 0, 0, 0};
        if (e < p.E) s = gc_sums_prepare<GcDeviceOps>(p, e);
        if (s.live) {
            GcDeviceOps::add64(p.chain_len + s.chain, s.len);
            if (s.ends) GcDeviceOps::add(p.ends + s.chain, s.ends);
        }
        gc_wave_add64(p.comp_len, s.comp, s.len, s.live, lane);
    }
}
#else
__global__ __launch_bounds__(GC_THREADS) void graph_clean_sums_kernel(GraphCleanParams p) {
    for (GC_ITEMS(e, p.E)) gc_sums_item<GcDeviceOps>(p, e);
}
#endif

__global__ __launch_bounds__(GC_THREADS) void graph_clean_decide_kernel(GraphCleanParams p) {
    for (GC_ITEMS(e, p.E)) gc_decide_item<GcDeviceOps>(p, e);
}

// step 0 .. 4: init, edges, chains, sums, decide.  The tables have been checked on the host (gr_tables_ok); -2 for bad parameters.
int launch_graph_clean(const GraphCleanParams& p, int step, hipStream_t s) {
    if (!gc_params_ok(p) || step < 0 || step > 4) return -2;
    const long n = step == 0 ? (p.N > p.E ? p.N : p.E) : step == 2 ? p.N : p.E;
    const long blocks = (n + GC_THREADS - 1) / GC_THREADS;
    const dim3 grid((unsigned)(blocks < 8192 ? blocks : 8192)), block(GC_THREADS);
    if (step == 0) hipLaunchKernelGGL(graph_clean_init_kernel, grid, block, 0, s, p);
    else if (step == 1) hipLaunchKernelGGL(graph_clean_edges_kernel, grid, block, 0, s, p);
    else if (step == 2) hipLaunchKernelGGL(graph_clean_chains_kernel, grid, block, 0, s, p);
    else if (step == 3) hipLaunchKernelGGL(graph_clean_sums_kernel, grid, block, 0, s, p);
    else hipLaunchKernelGGL(graph_clean_decide_kernel, grid, block, 0, s, p);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace srh
