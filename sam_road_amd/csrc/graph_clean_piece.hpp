// Spur and small-component pruning of the road graph and its chains (graph_clean.hip, config key GRAPH_CLEAN): the
// parameters and the work of ONE item (a node or an edge) of each of the five launches of a pass, free of HIP so that a CPU program can
// run the kernels' own code over every item, in any order (tests/graph_clean_check.cpp, under the host sanitizers), before a GPU does.
// The rule is stated on the host (sam_road_amd/graph_clean.py); state and out must equal graph_clean_ref exactly.
//
// The atomic operations are a template parameter `A`, as in mask_clean_piece.hpp, whose mc_find / mc_union are used as they are:
//   A::load(p) / store     an atomic load / store of an int32: every access to the int32 workspaces goes through A, in every launch
//   A::min / max / add     atomicMin / atomicMax / atomicAdd on an int32, returning the old value
//   A::load64 / store64    the same on an int64
//   A::add64               atomicAdd on an int64
// graph_clean.hip supplies the device's, the CPU program serial ones.
//
// A PASS analyses the live graph: init, edges, chains, sums, decide.  rounds passes decide (round 1 .. rounds: a live edge whose chain
// is a spur or whose component is small writes its own live byte and its state), one more (round 0, the final pass) writes out.
//
// TWO FORESTS in global memory, one over the nodes (components) and one over the edges (chains), each with the invariant of
// mask_clean_piece.hpp: every value ever stored at parent[i] is an index of the same forest <= i, and it only ever decreases (the stores
// are the initialisation parent[i] = i and atomicMin).  So the root of a class is its smallest index — the chain id, the component id.
//
// WHY EVERY LOOP ENDS.  mc_find walks along parents, which strictly descend, and stops at the first i with parent[i] >= i: at most i
// steps, whatever other workgroups store meanwhile.  mc_union retries only when the larger root a had been linked by somebody else in
// the meantime (old != a); it goes on with old < a, so the larger of its pair strictly decreases per retry: at most max(a, b) retries.
// gc_isqrt corrects a double-precision estimate that is off by at most one: each of its loops runs at most twice.  The kernels' own
// loops are grid-stride loops over [0, n).
//
// WHY EVERY INDEX STAYS INSIDE, however stale the value read:
//   a, b       the ends of an edge are read from the device table and used only if 0 <= a, b < N (gc_edge_live): the host has checked its
//              copy of the table (gr_tables_ok), and an entry the device copy does not share is skipped in every launch alike
//   parent[]   node_parent[i] is i or the result of atomicMin(node_parent + a, b) with b a root found inside [0, N): always in [0, i];
//              the same for edge_parent inside [0, E)
//   emin, emax of a node are read only where deg == 2, i.e. after two live edge-ends have stored their own index e in [0, E) into
//              both; the values are checked against E all the same
//   eroot, nroot of edge e are written by the sums launch of the same pass for every live edge and read by decide for live edges only;
//              the live bytes do not change between the two launches
// All sums are integers, so the result does not depend on the order of the atomics.
#pragma once
#include <stdint.h>

#include "mask_clean_piece.hpp"

#ifdef __HIPCC__
#define SRH_GC_HD __host__ __device__ __forceinline__
#else
#define SRH_GC_HD inline
#endif

namespace srh {

constexpr int GC_THREADS = 256;
constexpr int GC_MAX_ITEMS = 1 << 26;           // nodes, edges: 2^26 * GC_MAX_LEN_Q < 2^45
constexpr int GC_MAX_ROUNDS = 8;
constexpr int GC_MAX_LEN_Q = 370704;            // isqrt(256 * 2 * 16383^2)
constexpr int32_t GC_CLAMP = 2147483647;
constexpr int GC_SPUR = 1, GC_SMALL = 2;        // the reason bits of state = 4 * round + reason
constexpr int32_t GC_NO_EDGE = 2147483647;

struct GraphCleanParams {
    const int32_t* nodes = nullptr;             // [N, 2] (row, col), never written
    const int32_t* edges = nullptr;             // [E, 2], never written
    int N = 0, E = 0;
    int64_t spur_q = 0, comp_q = 0;             // ceil(16 s), ceil(16 c); 0: not stated
    int round = 0;                              // 1 .. rounds: a deciding pass; 0: the final pass, which writes out
    int first = 0;                              // the call's first pass: init also sets live = 1 and state = 0
    // the workspace (gc_workspace_carve)
    int64_t* comp_len = nullptr;                // [N]: at a node root, the sum of len_q of its component
    int64_t* chain_len = nullptr;               // [E]: at an edge root, the sum of len_q of its chain
    int32_t* node_parent = nullptr;             // [N]
    int32_t* deg = nullptr;                     // [N]: ends of live edges
    int32_t* emin = nullptr;                    // [N]: the smallest and the largest live edge at the node: the two edges of a
    int32_t* emax = nullptr;                    //      node of degree 2 (equal for a self-loop)
    int32_t* edge_parent = nullptr;             // [E]
    int32_t* ends = nullptr;                    // [E]: at an edge root, n_leaf + 65536 n_junc of its chain (each at most 2)
    int32_t* eroot = nullptr;                   // [E]: the chain of a live edge, from sums to decide
    int32_t* nroot = nullptr;                   // [E]: its component
    uint8_t* live = nullptr;                    // [E]: written by the edge's own item only
    // the outputs
    uint8_t* state = nullptr;                   // [E]
    int32_t* out = nullptr;                     // [E, 4], 16-byte aligned
};

struct alignas(16) GcRow { int32_t v[4]; };

// 24 N + 25 E bytes, rounded up to 16: the int64 arrays first, then the int32 ones, then the bytes.
SRH_GC_HD size_t gc_workspace_bytes(long N, long E) { return ((size_t)24 * N + (size_t)25 * E + 15) & ~(size_t)15; }

inline void gc_workspace_carve(void* base, long N, long E, GraphCleanParams& p) {
    int64_t* w8 = reinterpret_cast<int64_t*>(base);
    p.comp_len = w8; p.chain_len = w8 + N;
    int32_t* w4 = reinterpret_cast<int32_t*>(w8 + N + E);
    p.node_parent = w4; p.deg = w4 + N; p.emin = w4 + 2 * N; p.emax = w4 + 3 * N;
    w4 += 4 * N;
    p.edge_parent = w4; p.ends = w4 + E; p.eroot = w4 + 2 * E; p.nroot = w4 + 3 * E;
    p.live = reinterpret_cast<uint8_t*>(w4 + 4 * E);
}

SRH_GC_HD bool gc_params_ok(const GraphCleanParams& p) {
    return p.nodes && p.edges && p.N >= 1 && p.E >= 1 && p.N <= GC_MAX_ITEMS && p.E <= GC_MAX_ITEMS && p.spur_q >= 0 && p.comp_q >= 0 &&
           p.round >= 0 && p.round <= GC_MAX_ROUNDS && p.comp_len && p.chain_len && p.node_parent && p.deg && p.emin && p.emax &&
           p.edge_parent && p.ends && p.eroot && p.nroot && p.live && p.state && p.out && !(reinterpret_cast<uintptr_t>(p.out) & 15);
}

// floor(sqrt(v)) for v < 2^52: the double estimate is within one of it.
SRH_GC_HD uint64_t gc_isqrt(uint64_t v) {
    uint64_t q = (uint64_t)__builtin_sqrt((double)v);
    while (q * q > v) --q;
    while ((q + 1) * (q + 1) <= v) ++q;
    return q;
}

// len_q of the edge a -> b = isqrt(256 (dr^2 + dc^2)).  Coordinates lie within +-2^28 and the host has checked a span of at most 16383
// per axis, so the argument is below 2^37; the arithmetic is unsigned, so that no table could make it undefined.
SRH_GC_HD int64_t gc_len_q(const GraphCleanParams& p, int a, int b) {
    const int64_t dr = (int64_t)p.nodes[2L * b] - p.nodes[2L * a], dc = (int64_t)p.nodes[2L * b + 1] - p.nodes[2L * a + 1];
    const uint64_t ur = (uint64_t)(dr < 0 ? -dr : dr), uc = (uint64_t)(dc < 0 ? -dc : dc);
    const uint64_t l2 = (ur * ur + uc * uc) & ((1ull << 44) - 1);      // below 2^29 for every table the host admits
    return (int64_t)gc_isqrt(l2 << 8);
}

// Is edge e live, and are its ends nodes?  The ONLY read of the edge table.
SRH_GC_HD bool gc_edge_live(const GraphCleanParams& p, long e, int& a, int& b) {
    if (!p.live[e]) return false;
    a = p.edges[2 * e]; b = p.edges[2 * e + 1];
    return (unsigned)a < (unsigned)p.N && (unsigned)b < (unsigned)p.N;
}

// ---- launch 1, init: item i is node i and edge i, 0 <= i < max(N, E) -----------------------------------------------------------------------
template <class A>
SRH_GC_HD void gc_init_item(const GraphCleanParams& p, long i) {
    if (i < p.N) {
        A::store(p.node_parent + i, (int)i);
        A::store(p.deg + i, 0);
        A::store(p.emin + i, GC_NO_EDGE);
        A::store(p.emax + i, -1);
        A::store64(p.comp_len + i, 0);
    }
    if (i < p.E) {
        A::store(p.edge_parent + i, (int)i);
        A::store(p.ends + i, 0);
        A::store64(p.chain_len + i, 0);
        if (p.first) { p.live[i] = 1; p.state[i] = 0; }
    }
}

// ---- launch 2, edges: degrees, the incident-edge slots, the node forest -----------------------------------------------------------------------
template <class A>
SRH_GC_HD void gc_edges_item(const GraphCleanParams& p, long e) {
    int a, b;
    if (!gc_edge_live(p, e, a, b)) return;
    A::add(p.deg + a, 1);
    A::add(p.deg + b, 1);                                   // a self-loop counts 2
    A::min(p.emin + a, (int)e); A::max(p.emax + a, (int)e);
    A::min(p.emin + b, (int)e); A::max(p.emax + b, (int)e);
    if (a != b) mc_union<A>(p.node_parent, a, b);
}

// ---- launch 3, chains: the two edges of a node of degree 2 are one chain ------------------------------------------------------------------------
template <class A>
SRH_GC_HD void gc_chains_item(const GraphCleanParams& p, long v) {
    if (A::load(p.deg + v) != 2) return;
    const int e0 = A::load(p.emin + v), e1 = A::load(p.emax + v);
    if ((unsigned)e0 >= (unsigned)p.E || (unsigned)e1 >= (unsigned)p.E || e0 == e1) return;      // e0 == e1: a self-loop alone
    mc_union<A>(p.edge_parent, e0, e1);
}

// ---- launch 4, sums: what a live edge adds to its chain's root and to its component's root --------------------------------------------------------
struct GcSum {
    bool live;
    int chain, comp;                                        // the roots
    int64_t len;
    int ends;                                               // its ends of degree 1, + 65536 * its ends of degree >= 3
};

template <class A>
SRH_GC_HD GcSum gc_sums_prepare(const GraphCleanParams& p, long e) {
    GcSum s{false, 0, 0, 0, 0};
    int a, b;
    if (!gc_edge_live(p, e, a, b)) return s;
    s.live = true;
    s.chain = mc_find<A>(p.edge_parent, (int)e);
    s.comp = mc_find<A>(p.node_parent, a);                  // b's root is the same: launch 2 united them
    s.len = gc_len_q(p, a, b);
    const int da = A::load(p.deg + a), db = A::load(p.deg + b);
    s.ends = (da == 1) + (db == 1) + 65536 * ((da >= 3) + (db >= 3));
    p.eroot[e] = s.chain;
    p.nroot[e] = s.comp;
    return s;
}

template <class A>
SRH_GC_HD void gc_sums_item(const GraphCleanParams& p, long e) {
    const GcSum s = gc_sums_prepare<A>(p, e);
    if (!s.live) return;
    A::add64(p.chain_len + s.chain, s.len);
    A::add64(p.comp_len + s.comp, s.len);
    if (s.ends) A::add(p.ends + s.chain, s.ends);
}

// ---- launch 5, decide: the edge's own live byte and state; in the final pass its 16 bytes of out, one vector store ------------------------------------
template <class A>
SRH_GC_HD void gc_decide_item(const GraphCleanParams& p, long e) {
    GcRow* row = reinterpret_cast<GcRow*>(p.out) + e;
    int a, b;
    if (!gc_edge_live(p, e, a, b)) {
        if (p.round == 0) *row = GcRow{{-1, -1, 0, 0}};
        return;
    }
    const int rc = p.eroot[e], rn = p.nroot[e];
    if ((unsigned)rc >= (unsigned)p.E || (unsigned)rn >= (unsigned)p.N) return;      // cannot happen: written by launch 4 of this pass
    const int64_t chain_len = A::load64(p.chain_len + rc), comp_len = A::load64(p.comp_len + rn);
    if (p.round == 0) {
        *row = GcRow{{rc, rn, chain_len < GC_CLAMP ? (int32_t)chain_len : GC_CLAMP, comp_len < GC_CLAMP ? (int32_t)comp_len : GC_CLAMP}};
        return;
    }
    const int ends = A::load(p.ends + rc);
    const bool spur = p.spur_q > 0 && (ends & 65535) == 1 && (ends >> 16) == 1 && chain_len < p.spur_q;
    const bool small = p.comp_q > 0 && comp_len < p.comp_q;
    if (spur || small) {
        p.live[e] = 0;
        p.state[e] = (uint8_t)(4 * p.round + (spur ? GC_SPUR : 0) + (small ? GC_SMALL : 0));
    }
}

}  // namespace srh
