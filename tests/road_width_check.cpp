// The addressing and the arithmetic of the three ROAD_WIDTH kernels (sam_road_amd/csrc/road_width_piece.hpp) on the CPU: every work item
// of whole launches runs through the kernels' own per-item code, in a stand-alone program built with the address and undefined-behaviour
// sanitizers (tests/test_road_width_host.py builds and runs it).  The mask, G, the staged window of a segment, the column scratch, D2, the
// tables and out are heap blocks of their exact sizes, placed so that they END at their block's end: a byte read past the mask, G, a
// window or D2, or written past G, D2 or out, ends the program; the bytes in front of G, D2 and out are guards that must come back
// unchanged, the inputs must come back unwritten, and every value must equal the rule restated here as scalar loops over ALL pixels:
// the distance map by brute force over every pair of pixels, the statistics over every pixel of the image with the covering rule in
// 128-bit integers and an integer square root by bisection.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "road_width_piece.hpp"

using namespace srh;

static uint32_t rng_state = 24680u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

static uint8_t* block(size_t off, size_t bytes) {          // data at block + off, block 16-byte aligned, the block ends where the data ends
    void* b = nullptr;
    if (posix_memalign(&b, 16, off + bytes + (off + bytes == 0))) { printf("allocation failed\n"); exit(2); }
    return static_cast<uint8_t*>(b);
}

typedef __int128 wide;

static bool rule(long ar, long ac, long br, long bc, long y, long x) {          // GRAPH_RASTER's rule at t = 1
    const wide dr = br - ar, dc = bc - ac, pr = y - ar, pc = x - ac;
    const wide u = pr * dr + pc * dc, L = dr * dr + dc * dc;
    if (L == 0 || u <= 0) return 4 * (pr * pr + pc * pc) <= 1;
    if (u >= L) return 4 * ((pr - dr) * (pr - dr) + (pc - dc) * (pc - dc)) <= 1;
    const wide cr = pr * dc - pc * dr;
    return 4 * cr * cr <= L;
}

static uint32_t isqrt_bisect(uint64_t v) {
    uint64_t lo = 0, hi = 1u << 16;                                              // lo^2 <= v < hi^2
    while (hi - lo > 1) { const uint64_t mid = (lo + hi) / 2; if (mid * mid <= v) lo = mid; else hi = mid; }
    return (uint32_t)lo;
}

// The distance map by brute force: for every road pixel the nearest background pixel of the image, over all of them.
static std::vector<uint16_t> brute_dist(const std::vector<uint8_t>& m, int H, int W, int level, int R) {
    std::vector<long> bg;
    for (long i = 0; i < (long)H * W; ++i)
        if (m[i] <= level) bg.push_back(i);
    std::vector<uint16_t> out((size_t)H * W);
    for (long y = 0; y < H; ++y)
        for (long x = 0; x < W; ++x) {
            long best = (long)R * R;
            if (m[y * W + x] <= level) best = 0;
            else
                for (long b : bg) {
                    const long dy = b / W - y, dx = b % W - x;
                    if (dy * dy + dx * dx < best) best = dy * dy + dx * dx;
                }
            out[y * W + x] = (uint16_t)best;
        }
    return out;
}

struct Counts { long cases = 0, col_items = 0, row_items = 0, edge_items = 0, capped = 0, below = 0, covered = 0, partly = 0; };

// Both launches of the distance map over `m`, the mask at byte offset mask_off of its block and D2 at 8 * d2_quads bytes of its own:
// every (strip, chunk, lane) of the column pass, then every (row, segment) of the row pass with its window staged in a block of its exact
// size and every lane of the segment.  Returns D2.
static std::vector<uint16_t> dist_case(const std::vector<uint8_t>& m, int H, int W, int level, int R, int mask_off, Counts& c) {
    const size_t n = (size_t)H * W;
    uint8_t* mblock = block(mask_off, n);
    uint8_t* gblock = block(16, n);
    uint8_t* dblock = block(16, 2 * n);
    for (int k = 0; k < mask_off; ++k) mblock[k] = (uint8_t)rnd();
    memcpy(mblock + mask_off, m.data(), n);
    std::vector<uint8_t> mcopy(mblock, mblock + mask_off + n);
    memset(gblock, 0xA5, 16 + n);
    memset(dblock, 0xA5, 16 + 2 * n);
    RoadDistParams p;
    p.mask = mblock + mask_off; p.g = gblock + 16; p.d2 = reinterpret_cast<uint16_t*>(dblock + 16); p.H = H; p.W = W; p.on_level = level; p.R = R;
    if (!rw_dist_ok(p)) { printf("parameters refused (%d x %d)\n", H, W); exit(2); }
    // the column pass, workgroups and lanes from the last down: the items of a launch are independent
    for (long chunk = rw_col_chunks(p) - 1; chunk >= 0; --chunk)
        for (long strip = rw_col_strips(p) - 1; strip >= 0; --strip)
            for (int lane = RW_COL_THREADS - 1; lane >= 0; --lane) {
                const long x = strip * RW_COL_THREADS + lane;
                if (x >= W) continue;
                uint8_t* down = block(0, RW_COL_ROWS);                            // the lane's column of the LDS, stride 1
                rw_col_item(p, (int)x, (int)chunk * RW_COL_ROWS, down, 1);
                free(down);
                ++c.col_items;
            }
    // G against its definition
    for (long y = 0; y < H; ++y)
        for (long x = 0; x < W; ++x) {
            long want = R + 1;
            for (long yy = 0; yy < H; ++yy)
                if (m[yy * W + x] <= level && labs(yy - y) < want) want = labs(yy - y);
            if (p.g[y * W + x] != want) { printf("wrong G at (%ld, %ld) of %d x %d, R %d: %d, expected %ld\n", y, x, H, W, R, p.g[y * W + x], want); exit(1); }
        }
    std::vector<uint8_t> gcopy(gblock, gblock + 16 + n);
    // the row pass
    for (long y = H - 1; y >= 0; --y)
        for (long seg = rw_row_segs(p) - 1; seg >= 0; --seg) {
            int lo, hi;
            rw_row_window(p, (int)y, seg, lo, hi);
            if (hi - lo > RW_ROW_LDS) { printf("a window is larger than the LDS array\n"); exit(1); }
            const int wn = hi > lo ? hi - lo : 0;
            uint8_t* win = block(0, (size_t)wn);
            for (int k = wn - 1; k >= 0; --k) win[k] = rw_row_stage(p, (int)y, lo, k);
            for (int lane = RW_ROW_THREADS - 1; lane >= 0; --lane, ++c.row_items) rw_row_item(p, (int)y, seg, lane, win, lo, hi);
            free(win);
        }
    const std::vector<uint16_t> want = brute_dist(m, H, W, level, R);
    std::vector<uint16_t> got(n);
    memcpy(got.data(), p.d2, 2 * n);
    for (size_t i = 0; i < n; ++i) {
        if (got[i] != want[i]) { printf("wrong D2 at (%zu, %zu) of %d x %d, R %d level %d: %d, expected %d\n", i / W, i % W, H, W, R, level, got[i], want[i]); exit(1); }
        c.capped += got[i] == R * R; c.below += got[i] > 0 && got[i] < R * R;
    }
    for (int k = 0; k < 16; ++k)
        if (gblock[k] != 0xA5 || dblock[k] != 0xA5) { printf("a guard byte in front of G or D2 was written (%d x %d)\n", H, W); exit(1); }
    if (memcmp(mblock, mcopy.data(), mask_off + n) != 0 || memcmp(gblock, gcopy.data(), 16 + n) != 0) { printf("an input was written\n"); exit(1); }
    free(mblock); free(gblock); free(dblock);
    ++c.cases;
    return got;
}

// One launch of the gather: every edge, every row of its box, every column of its row span dealt to RW_LANES lanes as the kernel deals
// them, the lanes' values folded from the last lane down, two stores per edge.
static void edges_case(int H, int W, const std::vector<int32_t>& nodes, const std::vector<int32_t>& edges, const std::vector<uint16_t>& d2, int R, Counts& c) {
    const int N = (int)nodes.size() / 2, E = (int)edges.size() / 2;
    const size_t n = (size_t)H * W;
    uint8_t* nblock = block(0, nodes.size() * 4);
    uint8_t* eblock = block(0, edges.size() * 4);
    uint8_t* dblock = block(0, 2 * n);
    uint8_t* oblock = block(16, 32 * (size_t)E);
    memcpy(nblock, nodes.data(), nodes.size() * 4);
    memcpy(eblock, edges.data(), edges.size() * 4);
    memcpy(dblock, d2.data(), 2 * n);
    memset(oblock, 0xA5, 16 + 32 * (size_t)E);
    EdgeWidthParams p;
    p.g.nodes = reinterpret_cast<const int32_t*>(nblock); p.g.edges = reinterpret_cast<const int32_t*>(eblock);
    p.g.N = N; p.g.E = E; p.g.H = H; p.g.W = W; p.g.t = 1;
    p.d2 = reinterpret_cast<const uint16_t*>(dblock); p.R = R; p.out = reinterpret_cast<int32_t*>(oblock + 16);
    if (!rw_edges_ok(p) || !gr_tables_ok(p.g.nodes, N, p.g.edges, E)) { printf("parameters refused (%d x %d)\n", H, W); exit(2); }
    for (long e = E - 1; e >= 0; --e) {
        RwAcc acc[RW_LANES];
        const GrEdge ed = gr_edge_load(p.g, e);
        if (ed.x0 <= ed.x1)
            for (int y = ed.y0; y <= ed.y1; ++y) {
                int xlo, xhi;
                gr_edge_row(ed, y, xlo, xhi);
                if (xlo < ed.x0 || xhi > ed.x1) { printf("a row span leaves the box\n"); exit(1); }
                for (int lane = RW_LANES - 1; lane >= 0; --lane)
                    for (int x = xlo + lane; x <= xhi; x += RW_LANES, ++c.edge_items) rw_edge_pixel(p, ed, y, x, acc[lane]);
            }
        RwAcc a;
        for (int lane = RW_LANES - 1; lane >= 0; --lane) {
            a.n += acc[lane].n; a.n_in += acc[lane].n_in; a.s_q += acc[lane].s_q; a.n_cap += acc[lane].n_cap;
            if (acc[lane].d2_min < a.d2_min) a.d2_min = acc[lane].d2_min;
            if (acc[lane].d2_max > a.d2_max) a.d2_max = acc[lane].d2_max;
        }
        rw_edge_store(p, e, a);
    }
    for (int e = 0; e < E; ++e) {
        const long ar = nodes[2 * edges[2 * e]], ac = nodes[2 * edges[2 * e] + 1], br = nodes[2 * edges[2 * e + 1]], bc = nodes[2 * edges[2 * e + 1] + 1];
        long want[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        long mn = -1;
        for (long y = 0; y < H; ++y)
            for (long x = 0; x < W; ++x) {
                if (!rule(ar, ac, br, bc, y, x)) continue;
                const long d = d2[y * W + x];
                want[0] += 1; want[1] += d > 0; want[2] += isqrt_bisect(256u * (uint64_t)d); want[3] += d == (long)R * R;
                if (d > 0 && (mn < 0 || d < mn)) mn = d;
                if (d > want[5]) want[5] = d;
            }
        want[4] = mn < 0 ? 0 : mn;
        for (int k = 0; k < 8; ++k)
            if (p.out[8 * e + k] != want[k]) { printf("wrong value %d of edge %d: %d x %d, R %d: %d, expected %ld\n", k, e, H, W, R, p.out[8 * e + k], want[k]); exit(1); }
        if (want[0] > RW_MAX_COVERED) { printf("an edge covers more pixels than the bound\n"); exit(1); }
        c.covered += want[0]; c.partly += want[1] > 0 && want[1] < want[0];
    }
    for (int k = 0; k < 16; ++k)
        if (oblock[k] != 0xA5) { printf("guard byte %d in front of out written (%d x %d)\n", k, H, W); exit(1); }
    if (memcmp(nblock, nodes.data(), nodes.size() * 4) != 0 || memcmp(eblock, edges.data(), edges.size() * 4) != 0 || memcmp(dblock, d2.data(), 2 * n) != 0) {
        printf("an input was written\n"); exit(1);
    }
    free(nblock); free(eblock); free(dblock); free(oblock);
    ++c.cases;
}

static void random_graph(int H, int W, int N, int E, std::vector<int32_t>& nodes, std::vector<int32_t>& edges) {
    nodes.clear(); edges.clear();
    for (int k = 0; k < N; ++k) {                                                  // some nodes outside the image
        nodes.push_back((int32_t)(rnd() % (unsigned)(H + 24)) - 12);
        nodes.push_back((int32_t)(rnd() % (unsigned)(W + 24)) - 12);
    }
    for (int e = 0; e < E; ++e) {
        const int a = (int)(rnd() % (unsigned)N);
        edges.push_back(a);
        edges.push_back(e % 5 == 0 ? a : (int)(rnd() % (unsigned)N));              // zero-length edges among them
    }
}

int main() {
    Counts c;
    std::vector<int32_t> nodes, edges;
    // shapes around the chunk of the column pass (32 rows), its strip (256 columns) and the segment of the row pass (1024 pixels less the
    // misalignment of the row), odd widths so that every row has another misalignment; every kind of mask; the mask at every alignment
    const int shapes[][2] = {{1, 1}, {1, 70}, {70, 1}, {37, 53}, {31, 255}, {33, 257}, {32, 256}, {3, 1021}, {2, 1025}, {2, 1027}, {65, 9}};
    const int radii[] = {1, 2, 5, 32, 33, 254};
    int k = 0;
    for (const auto& s : shapes)
        for (int kind = 0; kind < 4; ++kind, ++k) {
            const int H = s[0], W = s[1], R = radii[k % 6], level = (k * 37) % 256;
            std::vector<uint8_t> m((size_t)H * W);
            for (auto& v : m) {
                if (kind == 0) v = (uint8_t)(rnd() % 10 ? 255 : 0);                                     // dense: mostly uncapped
                else if (kind == 1) v = 255;                                                              // all road: every pixel R^2 (0 at level 255)
                else if (kind == 2) v = (uint8_t)level;                                                   // all background
                else v = (uint8_t)(level < 255 ? level + 1 : 255);                                        // solid, background pixels below
            }
            if (kind == 3) {                                                                              // at the corners, the centre and the boundaries
                const int ys[] = {0, H - 1, H / 2, 31 % H, 32 % H}, xs[] = {0, W - 1, W / 2, 255 % W, 256 % W, 1023 % W};
                for (int y : ys) for (int x : xs) if ((y * 7 + x) % 3 == 0 || (y == 0 && x == 0)) m[(size_t)y * W + x] = (uint8_t)(level > 0 ? level - 1 : 0);
            }
            const std::vector<uint16_t> d2 = dist_case(m, H, W, level, R, k % 16, c);
            random_graph(H, W, 9, 14, nodes, edges);
            edges_case(H, W, nodes, edges, d2, R, c);
        }
    // bars and a disc whose half-width is R - 1, R and R + 1: the cap exactly reached, just missed and exceeded
    for (int R : {2, 5}) {
        for (int half = R - 1; half <= R + 1; ++half) {
            const int H = 2 * half + 9, W = 40;
            std::vector<uint8_t> m((size_t)H * W, 0);
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x)
                    if (abs(y - H / 2) <= half || (x - 20) * (x - 20) + (y - H / 2) * (y - H / 2) <= (half + 2) * (half + 2)) m[(size_t)y * W + x] = 200;
            const std::vector<uint16_t> d2 = dist_case(m, H, W, 127, R, 3, c);
            edges_case(H, W, {H / 2, 2, H / 2, 37, 0, 0, H - 1, W - 1}, {0, 1, 2, 3, 1, 1}, d2, R, c);
        }
    }
    // the maximum span along a 1 x 16384 map and across a 16384 x 2 map (maps made here: the gather alone), both ends far outside
    const int S = GR_MAX_SPAN;
    {
        std::vector<uint16_t> d2(16384);
        for (auto& v : d2) v = (uint16_t)(rnd() % 3 ? rnd() % 64517u : 0);
        edges_case(1, 16384, {0, 0, 0, S, 0, -5000, 0, S - 5000}, {0, 1, 1, 0, 2, 3}, d2, 254, c);
        edges_case(16384, 1, {0, 0, S, 0}, {0, 1}, d2, 254, c);
        std::vector<uint16_t> d3(2 * 16384);
        for (auto& v : d3) v = (uint16_t)(rnd() % 1025u);
        edges_case(16384, 2, {0, 0, S, 1, S - 7000, 1, -7000, 0}, {0, 1, 2, 3}, d3, 32, c);
    }
    if (c.capped == 0 || c.below == 0) { printf("no pixel at the cap, or none below it\n"); return 1; }
    if (c.covered == 0 || c.partly == 0) { printf("no pixel was ever covered, or no edge lies partly on the road\n"); return 1; }
    // the integer square root over its whole domain
    for (uint32_t d = 0; d <= 64516u; ++d)
        if (rw_isqrt(d << 8) != isqrt_bisect(256u * (uint64_t)d)) { printf("rw_isqrt(256 * %u) is wrong\n", d); return 1; }
    if (rw_isqrt(254u * 254u << 8) != RW_MAX_Q) { printf("RW_MAX_Q is wrong\n"); return 1; }
    // refusals of the host checks
    alignas(16) uint16_t d2[8];
    uint8_t m[4] = {0, 0, 0, 0}, g[4];
    RoadDistParams p;
    p.mask = m; p.g = g; p.d2 = d2; p.H = 2; p.W = 2; p.on_level = 255; p.R = 254;
    bool ok = rw_dist_ok(p);
    p.R = 255; ok = ok && !rw_dist_ok(p);
    p.R = 0; ok = ok && !rw_dist_ok(p);
    p.R = 1; p.on_level = 256; ok = ok && !rw_dist_ok(p);
    p.on_level = -1; ok = ok && !rw_dist_ok(p);
    p.on_level = 0; p.d2 = d2 + 1; ok = ok && !rw_dist_ok(p);                  // d2 is 8-byte aligned
    p.d2 = d2 + 2; ok = ok && !rw_dist_ok(p);
    p.d2 = nullptr; ok = ok && !rw_dist_ok(p);
    p.d2 = d2 + 4; ok = ok && rw_dist_ok(p);
    p.g = nullptr; ok = ok && !rw_dist_ok(p);
    p.g = g; p.mask = nullptr; ok = ok && !rw_dist_ok(p);
    p.mask = m; p.H = 0; ok = ok && !rw_dist_ok(p);
    p.H = 65536; p.W = 32768; ok = ok && !rw_dist_ok(p);                        // 2^31 pixels
    int32_t nd[4] = {0, 0, 1, 1}, ed[2] = {0, 1};
    alignas(16) int32_t out[12];
    EdgeWidthParams q;
    q.g.nodes = nd; q.g.edges = ed; q.g.N = 2; q.g.E = 1; q.g.H = 2; q.g.W = 2; q.g.t = 1; q.d2 = d2; q.R = 254; q.out = out;
    ok = ok && rw_edges_ok(q);
    q.R = 255; ok = ok && !rw_edges_ok(q);
    q.R = 0; ok = ok && !rw_edges_ok(q);
    q.R = 3; q.g.t = 2; ok = ok && !rw_edges_ok(q);                             // the centre line only
    q.g.t = 1; q.out = out + 1; ok = ok && !rw_edges_ok(q);                     // out is 16-byte aligned
    q.out = out + 2; ok = ok && !rw_edges_ok(q);
    q.out = nullptr; ok = ok && !rw_edges_ok(q);
    q.out = out; q.d2 = reinterpret_cast<const uint16_t*>(reinterpret_cast<const uint8_t*>(d2) + 1); ok = ok && !rw_edges_ok(q);
    q.d2 = nullptr; ok = ok && !rw_edges_ok(q);
    q.d2 = d2 + 1; ok = ok && rw_edges_ok(q);
    q.g.E = 0; ok = ok && !rw_edges_ok(q);                                      // E = 0 launches nothing
    q.g.E = 1; q.g.N = 0; ok = ok && !rw_edges_ok(q);
    q.g.N = 2; q.g.nodes = nullptr; ok = ok && !rw_edges_ok(q);
    q.g.nodes = nd; q.g.H = 0; ok = ok && !rw_edges_ok(q);
    if (!ok) { printf("the host checks accept or refuse wrongly\n"); return 1; }
    printf("road width OK: %ld cases, %ld + %ld + %ld items, %ld pixels at the cap, %ld below it, %ld covered, %ld edges partly on the road\n", c.cases,
           c.col_items, c.row_items, c.edge_items, c.capped, c.below, c.covered, c.partly);
    return 0;
}
