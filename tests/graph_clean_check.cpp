// The graph-clean kernels' own per-item code on a CPU: every item of the 5 (rounds + 1) launches of a call is run through
// sam_road_amd/csrc/graph_clean_piece.hpp with serial stand-ins for the atomic operations, in four schedules — ascending, descending, a
// fixed stride permutation, and ascending once more with parent loads that may return old values — and each result is compared with a
// scalar restatement of the rule written here (breadth-first searches over nodes and over edges; sam_road_amd/graph_clean.py states the
// rule).  The four results must be identical: the outcome may not depend on the schedule.  The workspace and the two outputs are placed so
// that they END at the end of their heap block, with guard bytes in front: built with the address sanitizer a read or write one element
// past either is an error, and a write in front of them changes a guard byte, which is checked.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "graph_clean_piece.hpp"
#include "graph_raster_piece.hpp"

using namespace srh;

struct SerialOps {
    static int load(const int32_t* p) { return *p; }
    static void store(int32_t* p, int v) { *p = v; }
    static int min(int32_t* p, int v) { const int old = *p; if (v < old) *p = v; return old; }
    static int max(int32_t* p, int v) { const int old = *p; if (v > old) *p = v; return old; }
    static int add(int32_t* p, int v) { const int old = *p; *p = old + v; return old; }
    static int64_t load64(const int64_t* p) { return *p; }
    static void store64(int64_t* p, int64_t v) { *p = v; }
    static void add64(int64_t* p, int64_t v) { *p += v; }
};

// The same with PARENT loads that may be old: inside the forest that a launch unites, a quarter of the loads return what the init launch
// stored (parent[i] = i) instead of the present value, as a load on the device may return a value that another workgroup has replaced
// since.  This drives mc_union through its retry.  Every other array is read only behind a kernel boundary and is never stale.
static const int32_t* stale_lo = nullptr;
static const int32_t* stale_hi = nullptr;
static uint32_t stale_state = 99;
struct StaleOps : SerialOps {
    static int load(const int32_t* p) {
        if (p < stale_lo || p >= stale_hi) return *p;
        stale_state = stale_state * 1664525u + 1013904223u;
        return (stale_state >> 20) % 4 == 0 ? (int)(p - stale_lo) : *p;
    }
};

static uint32_t rng_state = 1;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

struct Graph { std::vector<int32_t> nodes, edges; int N() const { return (int)nodes.size() / 2; } int E() const { return (int)edges.size() / 2; } };

// ---- the rule, restated ------------------------------------------------------------------------------------------------------------------------
static int64_t len_q_ref(const Graph& g, int e) {
    const int a = g.edges[2 * e], b = g.edges[2 * e + 1];
    const __int128 dr = (__int128)g.nodes[2 * b] - g.nodes[2 * a], dc = (__int128)g.nodes[2 * b + 1] - g.nodes[2 * a + 1];
    const __int128 v = 256 * (dr * dr + dc * dc);
    __int128 q = 0;
    for (int bit = 30; bit >= 0; --bit) { const __int128 t = q | ((__int128)1 << bit); if (t * t <= v) q = t; }      // bit by bit, no float
    return (int64_t)q;
}

struct Analysis { std::vector<int> chain, comp, n_leaf, n_junc; std::vector<int64_t> chain_len, comp_len; };

static Analysis analyse_ref(const Graph& g, const std::vector<uint8_t>& live) {
    const int N = g.N(), E = g.E();
    std::vector<int> deg((size_t)N, 0);
    std::vector<std::vector<int>> inc((size_t)N);                         // edge-ends per node: a self-loop twice
    for (int e = 0; e < E; ++e)
        if (live[(size_t)e])
            for (int k = 0; k < 2; ++k) { ++deg[(size_t)g.edges[2 * e + k]]; inc[(size_t)g.edges[2 * e + k]].push_back(e); }
    Analysis a;
    a.chain.assign((size_t)E, -1); a.comp.assign((size_t)E, -1); a.n_leaf.assign((size_t)E, 0); a.n_junc.assign((size_t)E, 0);
    a.chain_len.assign((size_t)E, 0); a.comp_len.assign((size_t)E, 0);
    std::vector<int> queue, members, node_comp((size_t)N, -1);
    for (int s = 0; s < N; ++s) {                                         // components: ascending start, so the label is the smallest node
        if (node_comp[(size_t)s] >= 0 || !deg[(size_t)s]) continue;
        queue.assign(1, s); node_comp[(size_t)s] = s;
        for (size_t h = 0; h < queue.size(); ++h)
            for (int e : inc[(size_t)queue[h]])
                for (int k = 0; k < 2; ++k) {
                    const int v = g.edges[2 * e + k];
                    if (node_comp[(size_t)v] < 0) { node_comp[(size_t)v] = s; queue.push_back(v); }
                }
    }
    std::vector<int64_t> comp_total((size_t)N, 0);
    for (int e = 0; e < E; ++e)
        if (live[(size_t)e]) { a.comp[(size_t)e] = node_comp[(size_t)g.edges[2 * e]]; comp_total[(size_t)a.comp[(size_t)e]] += len_q_ref(g, e); }
    for (int s = 0; s < E; ++s) {                                         // chains: ascending start, so the label is the smallest edge
        if (!live[(size_t)s] || a.chain[(size_t)s] >= 0) continue;
        queue.assign(1, s); a.chain[(size_t)s] = s;
        for (size_t h = 0; h < queue.size(); ++h)
            for (int k = 0; k < 2; ++k) {
                const int v = g.edges[2 * queue[h] + k];
                if (deg[(size_t)v] != 2) continue;
                for (int f : inc[(size_t)v])
                    if (a.chain[(size_t)f] < 0) { a.chain[(size_t)f] = s; queue.push_back(f); }
            }
        int64_t total = 0; int leaf = 0, junc = 0;
        for (int e : queue) {
            total += len_q_ref(g, e);
            for (int k = 0; k < 2; ++k) { const int d = deg[(size_t)g.edges[2 * e + k]]; leaf += d == 1; junc += d >= 3; }
        }
        for (int e : queue) { a.chain_len[(size_t)e] = total; a.n_leaf[(size_t)e] = leaf; a.n_junc[(size_t)e] = junc; }
    }
    for (int e = 0; e < E; ++e)
        if (live[(size_t)e]) a.comp_len[(size_t)e] = comp_total[(size_t)a.comp[(size_t)e]];
    return a;
}

static void clean_ref(const Graph& g, int64_t spur_q, int64_t comp_q, int rounds, std::vector<uint8_t>& state, std::vector<int32_t>& out) {
    const int E = g.E();
    std::vector<uint8_t> live((size_t)E, 1);
    state.assign((size_t)E, 0); out.assign((size_t)4 * E, 0);
    for (int r = 1; r <= rounds; ++r) {
        const Analysis a = analyse_ref(g, live);
        for (int e = 0; e < E; ++e) {
            if (!live[(size_t)e]) continue;
            const bool spur = spur_q > 0 && a.n_leaf[(size_t)e] == 1 && a.n_junc[(size_t)e] == 1 && a.chain_len[(size_t)e] < spur_q;
            const bool small = comp_q > 0 && a.comp_len[(size_t)e] < comp_q;
            if (spur || small) state[(size_t)e] = (uint8_t)(4 * r + spur + 2 * small);
        }
        for (int e = 0; e < E; ++e) if (state[(size_t)e]) live[(size_t)e] = 0;
    }
    const Analysis a = analyse_ref(g, live);
    for (int e = 0; e < E; ++e) {
        int32_t* row = out.data() + 4 * (size_t)e;
        if (!live[(size_t)e]) { row[0] = row[1] = -1; continue; }
        row[0] = a.chain[(size_t)e]; row[1] = a.comp[(size_t)e];
        row[2] = (int32_t)(a.chain_len[(size_t)e] < 2147483647 ? a.chain_len[(size_t)e] : 2147483647);
        row[3] = (int32_t)(a.comp_len[(size_t)e] < 2147483647 ? a.comp_len[(size_t)e] : 2147483647);
    }
}

// ---- one call, emulated -----------------------------------------------------------------------------------------------------------------------
static long item_at(long k, long n, int order) {
    if (order == 0 || order == 3) return k;
    if (order == 1) return n - 1 - k;
    long stride = 7919;                                   // a prime; coprime to n unless it divides n
    while (n % stride == 0) stride += 2;
    return (long)(((__int128)k * stride) % n);
}

constexpr size_t GUARD = 64;
struct Guarded {                                          // `bytes` bytes that end at the block's end, GUARD bytes of 0xC3 in front
    uint8_t* block; uint8_t* p; size_t bytes;
    explicit Guarded(size_t n) : block((uint8_t*)malloc(GUARD + n)), p(block + GUARD), bytes(n) { memset(block, 0xC3, GUARD); memset(p, 0x5a, n); }
    bool guard_ok() const { for (size_t i = 0; i < GUARD; ++i) if (block[i] != 0xC3) return false; return true; }
    ~Guarded() { free(block); }
};

static bool emulate(const Graph& g, int64_t spur_q, int64_t comp_q, int rounds, int order, std::vector<uint8_t>& state, std::vector<int32_t>& out) {
    const long N = g.N(), E = g.E();
    // exact-size copies of the tables too: the sanitizer guards their ends
    Guarded nodes((size_t)8 * N), edges((size_t)8 * E), ws(gc_workspace_bytes(N, E)), st((size_t)E), o((size_t)16 * E);
    memcpy(nodes.p, g.nodes.data(), (size_t)8 * N); memcpy(edges.p, g.edges.data(), (size_t)8 * E);
    GraphCleanParams p;
    p.nodes = (const int32_t*)nodes.p; p.edges = (const int32_t*)edges.p; p.N = (int)N; p.E = (int)E; p.spur_q = spur_q; p.comp_q = comp_q;
    p.state = st.p; p.out = (int32_t*)o.p;
    gc_workspace_carve(ws.p, N, E, p);
    if (p.live + E != ws.p + (size_t)(24 * N + 25 * E)) { printf("FAIL: the workspace is not carved to its size\n"); return false; }
    for (int r = 1; r <= rounds + 1; ++r) {
        p.round = r <= rounds ? r : 0;
        p.first = r == 1;
        if (!gc_params_ok(p)) { printf("FAIL: the parameters were refused\n"); return false; }
        for (int step = 0; step < 5; ++step) {
            const long n = step == 0 ? (N > E ? N : E) : step == 2 ? N : E;
            if (step == 1) { stale_lo = p.node_parent; stale_hi = p.node_parent + N; }
            if (step == 2) { stale_lo = p.edge_parent; stale_hi = p.edge_parent + E; }
            const bool stale = order == 3 && (step == 1 || step == 2);
            for (long k = 0; k < n; ++k) {
                const long i = item_at(k, n, order);
                if (step == 0) gc_init_item<SerialOps>(p, i);
                else if (step == 1) { if (stale) gc_edges_item<StaleOps>(p, i); else gc_edges_item<SerialOps>(p, i); }
                else if (step == 2) { if (stale) gc_chains_item<StaleOps>(p, i); else gc_chains_item<SerialOps>(p, i); }
                else if (step == 3) gc_sums_item<SerialOps>(p, i);
                else gc_decide_item<SerialOps>(p, i);
            }
        }
    }
    state.assign(st.p, st.p + E);
    out.assign((const int32_t*)o.p, (const int32_t*)o.p + 4 * E);
    const bool inputs_same = !memcmp(nodes.p, g.nodes.data(), (size_t)8 * N) && !memcmp(edges.p, g.edges.data(), (size_t)8 * E);
    if (!inputs_same) printf("FAIL: a table was written\n");
    const bool guards = nodes.guard_ok() && edges.guard_ok() && ws.guard_ok() && st.guard_ok() && o.guard_ok();
    if (!guards) printf("FAIL: a guard byte in front of a block was written\n");
    return inputs_same && guards;
}

static int failures = 0;
static long dropped = 0, total = 0;

static void check_call(const std::string& what, const Graph& g, int64_t spur_q, int64_t comp_q, int rounds) {
    if (!gr_tables_ok(g.nodes.data(), g.N(), g.edges.data(), g.E())) { printf("FAIL %s: the tables were refused\n", what.c_str()); ++failures; return; }
    std::vector<uint8_t> want_s, got_s;
    std::vector<int32_t> want_o, got_o;
    clean_ref(g, spur_q, comp_q, rounds, want_s, want_o);
    for (uint8_t s : want_s) dropped += s != 0;
    total += g.E();
    for (int order = 0; order < 4; ++order) {
        if (!emulate(g, spur_q, comp_q, rounds, order, got_s, got_o)) { ++failures; continue; }
        if (got_s != want_s || got_o != want_o) {
            long bad = 0, first = -1;
            for (int e = 0; e < g.E(); ++e)
                if (got_s[(size_t)e] != want_s[(size_t)e] || memcmp(&got_o[4 * (size_t)e], &want_o[4 * (size_t)e], 16)) { ++bad; if (first < 0) first = e; }
            printf("FAIL %s order %d: %ld edges differ, first %ld: state %d want %d, out {%d %d %d %d} want {%d %d %d %d}\n", what.c_str(), order, bad, first,
                   got_s[(size_t)first], want_s[(size_t)first], got_o[4 * first], got_o[4 * first + 1], got_o[4 * first + 2], got_o[4 * first + 3],
                   want_o[4 * first], want_o[4 * first + 1], want_o[4 * first + 2], want_o[4 * first + 3]);
            ++failures;
        }
    }
}

// N nodes, E edges: mostly neighbours in index (paths, small tangles), some far links, self-loops and parallel edges
static Graph random_graph(int N, int E, int spread) {
    Graph g;
    for (int i = 0; i < 2 * N; ++i) g.nodes.push_back((int32_t)(rnd() % (uint32_t)spread));
    for (int e = 0; e < E; ++e) {
        int a = (int)(rnd() % (uint32_t)N), b;
        const uint32_t kind = rnd() % 20;
        if (kind == 0) b = a;                                                                   // a self-loop
        else if (kind == 1 && e > 0) { a = g.edges[2 * (e - 1) + 1]; b = g.edges[2 * (e - 1)]; } // parallel to the edge before, reversed
        else if (kind < 5) b = (int)(rnd() % (uint32_t)N);
        else { b = a + (int)(rnd() % 3) - 1; b = b < 0 ? 0 : b >= N ? N - 1 : b; }
        g.edges.push_back(a); g.edges.push_back(b);
    }
    return g;
}

int main() {
    long calls = 0;
    // gc_isqrt against the bit-by-bit root at the edges of its range and around every square nearby
    for (uint64_t v : {0ull, 1ull, 2ull, 3ull, 4ull, 255ull, 256ull, (1ull << 37) - 1, 137422176512ull /* 256 * 2 * 16383^2 */, (1ull << 52) - 1})
        for (uint64_t d = 0; d < 3; ++d) {
            const uint64_t x = v >= d ? v - d : v, q = gc_isqrt(x);
            if (q * q > x || (q + 1) * (q + 1) <= x) { printf("FAIL: gc_isqrt(%llu) = %llu\n", (unsigned long long)x, (unsigned long long)q); ++failures; }
        }
    for (uint64_t r = 370000; r < 370710; ++r)
        for (uint64_t x : {r * r - 1, r * r, r * r + 1})
            if (gc_isqrt(x) != (x == r * r - 1 ? r - 1 : r)) { printf("FAIL: gc_isqrt near %llu^2\n", (unsigned long long)r); ++failures; }
    if (gc_isqrt(137422176512ull) != (uint64_t)GC_MAX_LEN_Q) { printf("FAIL: GC_MAX_LEN_Q\n"); ++failures; }

    // the sizes at the wave and workgroup edges and some in between, thresholds near the graph's own lengths, 1 to 3 rounds
    const int sizes[] = {1, 2, 63, 64, 65, 255, 256, 257, 1000};
    for (int N : sizes)
        for (int E : sizes) {
            rng_state = 777u + (uint32_t)(N * 1009 + E);
            const Graph g = random_graph(N, E, 48);
            check_call("random " + std::to_string(N) + "/" + std::to_string(E), g, 0, 0, 1);                  // attributes only
            check_call("random spur " + std::to_string(N) + "/" + std::to_string(E), g, 200 + rnd() % 400, 0, 1 + (int)(rnd() % 3));
            check_call("random both " + std::to_string(N) + "/" + std::to_string(E), g, 100 + rnd() % 600, 300 + rnd() % 1500, 1 + (int)(rnd() % 3));
            calls += 3;
        }
    // the Y whose stem falls only in round 2; 8 rounds on a caterpillar (a spine with a leg on every third node)
    {
        Graph y{{0, 0, 0, 3, 3, 0, 0, -10, 100, -10, -100, -10}, {0, 1, 0, 2, 0, 3, 3, 4, 3, 5}};
        check_call("Y 1 round", y, 192, 0, 1); check_call("Y 2 rounds", y, 192, 0, 2); check_call("Y at the threshold", y, 160, 0, 2);
        Graph c;
        for (int i = 0; i < 40; ++i) { c.nodes.push_back(0); c.nodes.push_back(4 * i); }
        for (int i = 0; i + 1 < 40; ++i) { c.edges.push_back(i + 1); c.edges.push_back(i); }
        for (int i = 0; i < 40; i += 3) { c.nodes.push_back(3); c.nodes.push_back(4 * i); c.edges.push_back(i); c.edges.push_back(c.N() - 1); }
        check_call("caterpillar", c, 16 * 13, 0, 8); check_call("caterpillar small", c, 16 * 13, 16 * 500, 8);
        calls += 5;
    }
    // a path of 6000 full-span edges from a junction: 2 224 224 000 > 2^31 sixteenths in one chain and one component, clamped in out and
    // decided in 64 bits; coordinates up to 6000 * 16383 < 2^28
    {
        Graph g;
        for (int i = 0; i <= 6000; ++i) { g.nodes.push_back(16383 * i); g.nodes.push_back(16383 * i); }
        for (int i = 0; i < 6000; ++i) { g.edges.push_back(i); g.edges.push_back(i + 1); }
        g.nodes.insert(g.nodes.end(), {-16383, 0, 0, -16383});
        g.edges.insert(g.edges.end(), {0, 6001, 0, 6002});
        check_call("long chain", g, 1 << 24, 1 << 24, 1);
        ++calls;
    }
    // coordinates at +-2^28 and a maximum-span edge there
    {
        Graph g{{-(1 << 28), -(1 << 28), -(1 << 28) + 16383, -(1 << 28) + 16383, (1 << 28), (1 << 28), (1 << 28) - 16383, (1 << 28)}, {0, 1, 2, 3, 3, 2}};
        check_call("corners", g, 1 << 24, 300000, 2);
        ++calls;
    }
    if (failures) { printf("%d failures\n", failures); return 1; }
    if (dropped * 50 < total || dropped * 2 > total) { printf("FAIL: %ld of %ld edges dropped: the thresholds decide nothing\n", dropped, total); return 1; }
    printf("graph clean OK: %ld calls, four schedules each, %ld of %ld edges dropped\n", calls, dropped, total);
    return 0;
}
