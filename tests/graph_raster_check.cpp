// The addressing and the arithmetic of the GRAPH_RASTER kernels (sam_road_amd/csrc/graph_raster_piece.hpp) on the CPU: every work item of
// whole launches runs through the kernels' own per-item code, in a stand-alone program built with the address and undefined-behaviour
// sanitizers (tests/test_graph_raster_host.py builds and runs it).  The tables, the maps, the images and the outputs are heap blocks of
// their exact sizes, placed so that they END at their block's end at every alignment: a byte read past a table or written past an output
// ends the program; the bytes in front of an output are guards that must come back unchanged, the tables must come back unwritten, and
// every result must equal the rule restated here as a scalar loop over ALL pixels of the image in 128-bit integers (so neither the
// bounding box nor the per-row column span of the kernel is trusted).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "graph_raster_piece.hpp"

using namespace srh;

static uint32_t rng_state = 24680u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

static uint8_t* block(size_t off, size_t bytes) {          // data at block + off, block 16-byte aligned, the block ends where the data ends
    void* b = nullptr;
    if (posix_memalign(&b, 16, off + bytes + (off + bytes == 0))) { printf("allocation failed\n"); exit(2); }
    return static_cast<uint8_t*>(b);
}

typedef __int128 wide;

static bool rule(long ar, long ac, long br, long bc, int t, long y, long x) {
    const wide dr = br - ar, dc = bc - ac, pr = y - ar, pc = x - ac, tt = (wide)t * t;
    const wide u = pr * dr + pc * dc, L = dr * dr + dc * dc;
    if (L == 0 || u <= 0) return 4 * (pr * pr + pc * pc) <= tt;
    if (u >= L) return 4 * ((pr - dr) * (pr - dr) + (pc - dc) * (pc - dc)) <= tt;
    const wide cr = pr * dc - pc * dr;
    return 4 * cr * cr <= tt * L;
}

static long raster_case(int H, int W, const std::vector<int32_t>& nodes, const std::vector<int32_t>& edges, int t, int mark, int r, int out_off, long* covered) {
    const int N = (int)nodes.size() / 2, E = (int)edges.size() / 2;
    const size_t n = (size_t)H * W;
    uint8_t* nblock = block(0, nodes.size() * 4);
    uint8_t* eblock = block(0, edges.size() * 4);
    uint8_t* oblock = block(out_off, n);
    if (N) memcpy(nblock, nodes.data(), nodes.size() * 4);
    if (E) memcpy(eblock, edges.data(), edges.size() * 4);
    memset(oblock, 0xA5, out_off + n);
    GraphRasterParams p;
    p.nodes = N ? reinterpret_cast<const int32_t*>(nblock) : nullptr; p.edges = E ? reinterpret_cast<const int32_t*>(eblock) : nullptr;
    p.out = oblock + out_off; p.N = N; p.E = E; p.H = H; p.W = W; p.t = t; p.mark = mark; p.r = r;
    if (!gr_params_ok(p) || !gr_tables_ok(p.nodes, N, p.edges, E)) { printf("parameters refused (%d x %d)\n", H, W); exit(2); }
    long items = 0;
    // the three launches, every item, in descending order (the items of a launch are independent)
    for (long c = gr_clear_chunks(p) - 1; c >= 0; --c) gr_clear_item(p, c);
    for (long e = E - 1; e >= 0; --e) {
        const GrEdge ed = gr_edge_load(p, e);
        if (ed.x0 > ed.x1) continue;
        for (int y = ed.y1; y >= ed.y0; --y) {
            int xlo, xhi;
            gr_edge_row(ed, y, xlo, xhi);
            if (xlo < ed.x0 || xhi > ed.x1) { printf("a row span leaves the box\n"); exit(1); }
            for (int x = xhi; x >= xlo; --x, ++items) gr_edge_item(p, ed, y, x);
        }
    }
    if (mark != GR_MARK_NONE)
        for (long k = N - 1; k >= 0; --k) {
            const GrNode nd = gr_node_load(p, k);
            for (int i = nd.bh * nd.bw - 1; i >= 0; --i, ++items) gr_node_item(p, nd, i);
        }
    // the rule over all pixels
    std::vector<uint8_t> want(n, 0);
    for (int e = 0; e < E; ++e) {
        const long ar = nodes[2 * edges[2 * e]], ac = nodes[2 * edges[2 * e] + 1], br = nodes[2 * edges[2 * e + 1]], bc = nodes[2 * edges[2 * e + 1] + 1];
        for (long y = 0; y < H; ++y)
            for (long x = 0; x < W; ++x)
                if (rule(ar, ac, br, bc, t, y, x)) want[y * W + x] = 1;
    }
    if (mark != GR_MARK_NONE)
        for (int k = 0; k < N; ++k) {
            const long ar = nodes[2 * k], ac = nodes[2 * k + 1];
            for (long y = ar - r < 0 ? 0 : ar - r; y <= ar + r && y < H; ++y)
                for (long x = ac - r < 0 ? 0 : ac - r; x <= ac + r && x < W; ++x)
                    if (mark == GR_MARK_SQUARE || (y - ar) * (y - ar) + (x - ac) * (x - ac) <= (long)r * r) want[y * W + x] = 2;
        }
    for (size_t i = 0; i < n; ++i) {
        if (p.out[i] != want[i]) {
            printf("wrong byte: %d x %d at (%zu, %zu), t %d mark %d r %d out_off %d: %d, expected %d\n", H, W, i / W, i % W, t, mark, r, out_off, p.out[i], want[i]);
            exit(1);
        }
        if (covered) *covered += want[i] != 0;
    }
    for (int k = 0; k < out_off; ++k)
        if (oblock[k] != 0xA5) { printf("guard byte %d in front of out written (%d x %d)\n", k, H, W); exit(1); }
    if ((N && memcmp(nblock, nodes.data(), nodes.size() * 4) != 0) || (E && memcmp(eblock, edges.data(), edges.size() * 4) != 0)) { printf("a table was written\n"); exit(1); }
    free(nblock); free(eblock); free(oblock);
    return items;
}

static long random_case(int H, int W, int N, int E, int t, int mark, int r, int out_off, long* covered) {
    std::vector<int32_t> nodes, edges;
    for (int k = 0; k < N; ++k) {                                                  // some nodes outside the image
        nodes.push_back((int32_t)(rnd() % (unsigned)(H + 24)) - 12);
        nodes.push_back((int32_t)(rnd() % (unsigned)(W + 24)) - 12);
    }
    for (int e = 0; e < E && N; ++e) {
        const int a = (int)(rnd() % (unsigned)N);
        edges.push_back(a);
        edges.push_back(e % 5 == 0 ? a : (int)(rnd() % (unsigned)N));              // zero-length edges among them
    }
    return raster_case(H, W, nodes, edges, t, mark, r, out_off, covered);
}

// composite and compare on blocks of exact size at the offsets off (classes / maps), off3 (images)
static void pixel_case(long n, int off, int off3, bool with_img, bool with_valid, bool with_diff) {
    uint8_t* maps[5];
    for (auto& m : maps) {
        m = block(off, n);
        for (long i = 0; i < n; ++i) m[off + i] = (uint8_t)(rnd() % 3 ? 0 : 1 + rnd() % 2);
    }
    uint8_t* img = block(off3, 3 * n);
    for (long i = 0; i < 3 * n; ++i) img[off3 + i] = (uint8_t)rnd();
    uint8_t* out = block(off3 + 4, 3 * n);
    memset(out, 0xA5, off3 + 4 + 3 * n);
    GraphCompositeParams c;
    c.cls = maps[0] + off; c.img = with_img ? img + off3 : nullptr; c.out = out + off3 + 4; c.n = n;
    c.colour[0] = 0x030201u; c.colour[1] = 0x0fa0fdu; c.colour[2] = 0x00ffffu;
    if (!gr_composite_ok(c)) { printf("composite parameters refused\n"); exit(2); }
    for (long q = gr_quads(n) - 1; q >= 0; --q) gr_composite_item(c, q);
    for (long i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) {
            const uint8_t cl = c.cls[i];
            const uint8_t want = cl >= 2 ? (uint8_t)(c.colour[2] >> (8 * k)) : cl == 1 ? (uint8_t)(c.colour[1] >> (8 * k)) : with_img ? img[off3 + 3 * i + k] : (uint8_t)(c.colour[0] >> (8 * k));
            if (c.out[3 * i + k] != want) { printf("composite: wrong byte at pixel %ld channel %d (n %ld off %d off3 %d)\n", i, k, n, off, off3); exit(1); }
        }
    for (int k = 0; k < off3 + 4; ++k)
        if (out[k] != 0xA5) { printf("composite: guard byte written\n"); exit(1); }

    memset(out, 0xA5, off3 + 4 + 3 * n);
    alignas(8) unsigned long long counts[4] = {0, 0, 0, 0};
    GraphCompareParams p;
    p.pred_thin = maps[1] + off; p.pred_wide = maps[2] + off; p.gt_thin = maps[3] + off; p.gt_wide = maps[4] + off;
    p.valid = with_valid ? maps[0] + off : nullptr; p.img = with_img ? img + off3 : nullptr; p.diff = with_diff ? out + off3 + 4 : nullptr; p.counts = counts; p.n = n;
    if (!gr_compare_ok(p)) { printf("compare parameters refused\n"); exit(2); }
    for (long q = gr_quads(n) - 1; q >= 0; --q) {
        uint32_t acc[4] = {0, 0, 0, 0};
        gr_compare_item(p, q, acc);
        for (int k = 0; k < 4; ++k) counts[k] += acc[k];
    }
    unsigned long long want[4] = {0, 0, 0, 0};
    for (long i = 0; i < n; ++i) {
        const bool v = !with_valid || p.valid[i] != 0;
        const bool pred = v && p.pred_thin[i], truth = v && p.gt_thin[i], fp = pred && !p.gt_wide[i], missed = truth && !p.pred_wide[i];
        want[0] += pred; want[1] += fp; want[2] += truth; want[3] += missed;
        if (!with_diff) continue;
        for (int k = 0; k < 3; ++k) {
            const uint8_t w = missed ? (k == 0 ? 255 : 0) : fp ? (k == 2 ? 255 : 0) : with_img ? img[off3 + 3 * i + k] : 0;
            if (p.diff[3 * i + k] != w) { printf("compare: wrong diff byte at pixel %ld channel %d (n %ld off %d off3 %d)\n", i, k, n, off, off3); exit(1); }
        }
    }
    for (int k = 0; k < 4; ++k)
        if (counts[k] != want[k]) { printf("compare: count %d is %llu, expected %llu\n", k, counts[k], want[k]); exit(1); }
    for (long k = 0; k < (with_diff ? off3 + 4 : off3 + 4 + 3 * n); ++k)
        if (out[k] != 0xA5) { printf("compare: a byte outside diff written\n"); exit(1); }
    for (auto& m : maps) free(m);
    free(img); free(out);
}

int main() {
    long cases = 0, items = 0, covered = 0;
    // random graphs, every width 1 .. 12 and a few wide ones, the three marks, out at every alignment mod 16
    const int shapes[][2] = {{1, 1}, {7, 5}, {3, 33}, {37, 53}, {64, 64}};
    for (const auto& s : shapes)
        for (int k = 0; k < 16; ++k) {
            const int t = k < 12 ? k + 1 : k == 12 ? 31 : k == 13 ? 100 : k == 14 ? 254 : 255;
            items += random_case(s[0], s[1], 9, 14, t, k % 3, (k * 5) % 11, k, &covered);
            ++cases;
        }
    items += random_case(40, 40, 5, 8, 3, GR_MARK_DISC, GR_MAX_RADIUS, 3, &covered);
    items += random_case(9, 9, 0, 0, 4, GR_MARK_DISC, 4, 1, nullptr);                 // N = 0, E = 0: the clear alone
    items += random_case(9, 9, 6, 0, 4, GR_MARK_SQUARE, 2, 5, &covered);              // E = 0
    cases += 3;
    // the maximum span: along a 1 x 16384 image, across a 16384 x 2 image, a diagonal through a small image with both ends far outside
    const int S = GR_MAX_SPAN;
    for (int off : {0, 1, 7}) {
        items += raster_case(1, 16384, {0, 0, 0, S}, {0, 1}, 4, GR_MARK_DISC, 4, off, &covered);
        items += raster_case(1, 16384, {0, S, 0, 0, 5, 100}, {0, 1, 1, 2}, 255, GR_MARK_NONE, 0, off, &covered);
        items += raster_case(16384, 2, {0, 0, S, 1}, {0, 1}, 1, GR_MARK_SQUARE, 1, off, &covered);
        items += raster_case(16384, 2, {S, 0, 0, 1}, {1, 0}, 10, GR_MARK_NONE, 0, off, &covered);
        items += raster_case(33, 47, {-8000, -8000, 8383, 8383, 8383 - 20, -8000 + 31, -8000 - 20, 8383 + 31}, {0, 1, 2, 3}, 5, GR_MARK_SQUARE, 3, off, &covered);
        items += raster_case(21, 30, {-(1 << 28), -(1 << 28), -(1 << 28) + S, -(1 << 28) + S, 1 << 28, 1 << 28, (1 << 28) - S, (1 << 28) - 1}, {0, 1, 2, 3}, 255, GR_MARK_DISC, 127, off, nullptr);
        items += raster_case(25, 25, {-30, 12, 60, 13, 12, -40, 11, 70, -5, -5, 30, 30}, {0, 1, 2, 3, 4, 5}, 2, GR_MARK_NONE, 0, off, &covered);      // both ends outside, crossing
        cases += 7;
    }
    // a star: many writers on the pixels around one node
    {
        std::vector<int32_t> nodes{20, 20}, edges;
        for (int k = 0; k < 120; ++k) {
            nodes.push_back(20 + (int)(rnd() % 61) - 30); nodes.push_back(20 + (int)(rnd() % 61) - 30);
            edges.push_back(0); edges.push_back(k + 1);
        }
        items += raster_case(41, 43, nodes, edges, 4, GR_MARK_DISC, 4, 9, &covered);
        ++cases;
    }
    if (covered == 0) { printf("no pixel was ever covered\n"); return 1; }
    // composite and compare: every alignment mod 4 of the maps and the images (0 / 0 takes the word path), pixel counts that are no multiple of 4
    for (long n : {1L, 3L, 4L, 5L, 64L, 1023L})
        for (int off = 0; off < 4; ++off)
            for (int off3 = 0; off3 < 4; ++off3) {
                const int f = (int)(rnd() & 7);
                pixel_case(n, off, off3, f & 1, (f & 2) != 0, (f & 4) != 0);
                pixel_case(n, off, off3, true, true, true);
                cases += 2;
            }
    // refusals of the host checks
    int32_t nd[6] = {0, 0, 5, 5, 0, S + 1}, ed[4] = {0, 1, 0, 1};
    uint8_t out[4];
    GraphRasterParams p;
    p.nodes = nd; p.edges = ed; p.out = out; p.N = 3; p.E = 2; p.H = 2; p.W = 2; p.t = 4;
    bool ok = gr_params_ok(p) && gr_tables_ok(nd, 3, ed, 2);
    p.H = 0; ok = ok && !gr_params_ok(p);
    p.H = 65536; p.W = 32768; ok = ok && !gr_params_ok(p);                       // 2^31 pixels
    p.H = 2; p.W = 2; p.t = 0; ok = ok && !gr_params_ok(p);
    p.t = 256; ok = ok && !gr_params_ok(p);
    p.t = 4; p.mark = 3; ok = ok && !gr_params_ok(p);
    p.mark = 1; p.r = 128; ok = ok && !gr_params_ok(p);
    p.r = -1; ok = ok && !gr_params_ok(p);
    p.r = 0; p.edge_value = 0; ok = ok && !gr_params_ok(p);
    p.edge_value = 1; p.node_value = 256; ok = ok && !gr_params_ok(p);
    p.node_value = 2; p.out = nullptr; ok = ok && !gr_params_ok(p);
    p.out = out; p.nodes = nullptr; ok = ok && !gr_params_ok(p);
    p.nodes = nd; p.N = 0; ok = ok && !gr_params_ok(p);                          // edges without nodes
    p.N = -1; ok = ok && !gr_params_ok(p);
    ed[3] = 2; ok = ok && !gr_tables_ok(nd, 3, ed, 2);                           // one pixel longer than the span bound
    nd[5] = S; ok = ok && gr_tables_ok(nd, 3, ed, 2);                            // the bound itself
    ed[3] = 3; ok = ok && !gr_tables_ok(nd, 3, ed, 2);                           // an index outside [0, N)
    ed[3] = -1; ok = ok && !gr_tables_ok(nd, 3, ed, 2);
    ed[3] = 1; nd[0] = (1 << 28) + 1; ok = ok && !gr_tables_ok(nd, 3, ed, 2);
    nd[0] = -(1 << 28) - 1; ok = ok && !gr_tables_ok(nd, 3, ed, 2);
    ok = ok && !gr_tables_ok(nullptr, 3, ed, 2) && !gr_tables_ok(nd, 3, nullptr, 2) && gr_tables_ok(nullptr, 0, nullptr, 0);
    if (!ok) { printf("a host check accepts or refuses wrongly\n"); return 1; }
    printf("graph raster OK: %ld cases, %ld items, %ld pixels covered\n", cases, items, covered);
    return 0;
}
