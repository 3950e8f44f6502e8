// The addressing and the arithmetic of the EDGE_SUPPORT kernel (sam_road_amd/csrc/edge_support_piece.hpp) on the CPU: every work item of
// whole launches runs through the kernel's own per-item code, in a stand-alone program built with the address and undefined-behaviour
// sanitizers (tests/test_edge_support_host.py builds and runs it).  The tables, the mask, valid and out are heap blocks of their exact
// sizes, placed so that they END at their block's end: a byte read past a table or a mask, or written past out, ends the program; the
// bytes in front of out are guards that must come back unchanged, the inputs must come back unwritten, and every counter must equal the
// rule restated here as a scalar loop over ALL pixels of the image in 128-bit integers (so neither the bounding box nor the per-row
// column span of the kernel is trusted).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "edge_support_piece.hpp"

using namespace srh;

static uint32_t rng_state = 13579u;
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

// One launch: every edge, every row of its box, every column of its row span dealt to `lanes` lanes as the kernel deals them, the lanes'
// counters summed from the last lane down, one store per edge.  Returns the number of pixels visited; *covered gets the sum of n.
static long stats_case(int H, int W, const std::vector<int32_t>& nodes, const std::vector<int32_t>& edges, int t, int on_level, bool with_valid, int mask_off,
                       int lanes, long* covered) {
    const int N = (int)nodes.size() / 2, E = (int)edges.size() / 2;
    const size_t n = (size_t)H * W;
    uint8_t* nblock = block(0, nodes.size() * 4);
    uint8_t* eblock = block(0, edges.size() * 4);
    uint8_t* mblock = block(mask_off, n);
    uint8_t* vblock = block(mask_off, n);
    uint8_t* oblock = block(16, 16 * (size_t)E);
    memcpy(nblock, nodes.data(), nodes.size() * 4);
    memcpy(eblock, edges.data(), edges.size() * 4);
    for (size_t i = 0; i < mask_off + n; ++i) { mblock[i] = (uint8_t)rnd(); vblock[i] = (uint8_t)(rnd() % 3 ? 1 + rnd() % 255 : 0); }
    std::vector<uint8_t> mcopy(mblock, mblock + mask_off + n), vcopy(vblock, vblock + mask_off + n);
    memset(oblock, 0xA5, 16 + 16 * (size_t)E);
    EdgeStatsParams p;
    p.g.nodes = reinterpret_cast<const int32_t*>(nblock); p.g.edges = reinterpret_cast<const int32_t*>(eblock);
    p.g.N = N; p.g.E = E; p.g.H = H; p.g.W = W; p.g.t = t;
    p.mask = mblock + mask_off; p.valid = with_valid ? vblock + mask_off : nullptr; p.on_level = on_level;
    p.out = reinterpret_cast<int32_t*>(oblock + 16);
    if (!es_params_ok(p) || !gr_tables_ok(p.g.nodes, N, p.g.edges, E)) { printf("parameters refused (%d x %d)\n", H, W); exit(2); }
    long items = 0;
    std::vector<uint32_t> acc(4 * (size_t)lanes);
    for (long e = E - 1; e >= 0; --e) {                                            // the edges of a launch are independent
        std::fill(acc.begin(), acc.end(), 0u);
        const GrEdge ed = gr_edge_load(p.g, e);
        if (ed.x0 <= ed.x1)
            for (int y = ed.y0; y <= ed.y1; ++y) {
                int xlo, xhi;
                gr_edge_row(ed, y, xlo, xhi);
                if (xlo < ed.x0 || xhi > ed.x1) { printf("a row span leaves the box\n"); exit(1); }
                for (int lane = lanes - 1; lane >= 0; --lane)
                    for (int x = xlo + lane; x <= xhi; x += lanes, ++items) es_pixel(p, ed, y, x, &acc[4 * (size_t)lane]);
            }
        uint32_t sum[4] = {0u, 0u, 0u, 0u};
        for (int lane = lanes - 1; lane >= 0; --lane)
            for (int c = 0; c < 4; ++c) sum[c] += acc[4 * (size_t)lane + c];
        es_store(p, e, sum);
    }
    // the rule over all pixels
    for (int e = 0; e < E; ++e) {
        const long ar = nodes[2 * edges[2 * e]], ac = nodes[2 * edges[2 * e] + 1], br = nodes[2 * edges[2 * e + 1]], bc = nodes[2 * edges[2 * e + 1] + 1];
        wide want[4] = {0, 0, 0, 0};
        for (long y = 0; y < H; ++y)
            for (long x = 0; x < W; ++x) {
                if (!rule(ar, ac, br, bc, t, y, x)) continue;
                const uint8_t m = mcopy[mask_off + y * W + x];
                want[0] += 1; want[1] += m; want[2] += m > on_level; want[3] += with_valid && vcopy[mask_off + y * W + x] == 0;
            }
        for (int c = 0; c < 4; ++c)
            if ((wide)p.out[4 * e + c] != want[c]) {
                printf("wrong counter %d of edge %d: %d x %d, t %d level %d valid %d: %d, expected %ld\n", c, e, H, W, t, on_level, (int)with_valid, p.out[4 * e + c], (long)want[c]);
                exit(1);
            }
        if (want[0] > ES_MAX_COVERED) { printf("an edge covers more pixels than the bound\n"); exit(1); }
        if (covered) *covered += (long)want[0];
    }
    for (int k = 0; k < 16; ++k)
        if (oblock[k] != 0xA5) { printf("guard byte %d in front of out written (%d x %d)\n", k, H, W); exit(1); }
    if (memcmp(nblock, nodes.data(), nodes.size() * 4) != 0 || memcmp(eblock, edges.data(), edges.size() * 4) != 0 ||
        memcmp(mblock, mcopy.data(), mask_off + n) != 0 || memcmp(vblock, vcopy.data(), mask_off + n) != 0) { printf("an input was written\n"); exit(1); }
    free(nblock); free(eblock); free(mblock); free(vblock); free(oblock);
    return items;
}

static long random_case(int H, int W, int N, int E, int t, int on_level, bool with_valid, int mask_off, int lanes, long* covered) {
    std::vector<int32_t> nodes, edges;
    for (int k = 0; k < N; ++k) {                                                  // some nodes outside the image
        nodes.push_back((int32_t)(rnd() % (unsigned)(H + 24)) - 12);
        nodes.push_back((int32_t)(rnd() % (unsigned)(W + 24)) - 12);
    }
    for (int e = 0; e < E; ++e) {
        const int a = (int)(rnd() % (unsigned)N);
        edges.push_back(a);
        edges.push_back(e % 5 == 0 ? a : (int)(rnd() % (unsigned)N));              // zero-length edges among them
    }
    return stats_case(H, W, nodes, edges, t, on_level, with_valid, mask_off, lanes, covered);
}

int main() {
    long cases = 0, items = 0, covered = 0;
    // random graphs, every width 1 .. 12 and a few wide ones, valid present and absent, the mask at every alignment mod 16, 64 and 16 lanes
    const int shapes[][2] = {{1, 1}, {7, 5}, {3, 33}, {37, 53}, {64, 64}};
    for (const auto& s : shapes)
        for (int k = 0; k < 16; ++k) {
            const int t = k < 12 ? k + 1 : k == 12 ? 31 : k == 13 ? 100 : k == 14 ? 254 : 255;
            items += random_case(s[0], s[1], 9, 14, t, (k * 37) % 256, k & 1, k, k % 3 == 2 ? 16 : 64, &covered);
            ++cases;
        }
    // the maximum span: along a 1 x 16384 image, across a 16384 x 2 image, through a small image with both ends far outside, at +-2^28
    const int S = GR_MAX_SPAN, C = GR_MAX_COORD;
    for (int v = 0; v < 2; ++v) {
        items += stats_case(1, 1, {0, 0, S, S, -S, -S + 1, 0, 0}, {0, 1, 2, 3, 3, 3}, 1, 0, v, 1, 64, &covered);
        items += stats_case(1, 1, {-S / 2, -S / 2, S / 2 + 1, S / 2 + 1, 5, 5, 40, 5}, {0, 1, 2, 3}, 255, 255, v, 0, 64, &covered);
        items += stats_case(1, 16384, {0, 0, 0, S}, {0, 1, 1, 0}, 1, 128, v, 3, 64, &covered);
        items += stats_case(1, 16384, {0, S, 0, 0, 5, 100, -3, S - 2}, {0, 1, 1, 2, 3, 1}, 255, 127, v, 7, 64, &covered);
        items += stats_case(16384, 2, {0, 0, S, 1}, {0, 1}, 1, 200, v, 1, 64, &covered);
        items += stats_case(16384, 2, {S, 0, 0, 1, S, -40, 0, -40}, {1, 0, 2, 3}, 10, 3, v, 0, 16, &covered);
        items += stats_case(33, 47, {-8000, -8000, 8383, 8383, 8383 - 20, -8000 + 31, -8000 - 20, 8383 + 31}, {0, 1, 2, 3}, 5, 90, v, 5, 64, &covered);
        items += stats_case(21, 30, {-C, -C, -C + S, -C + S, C, C, C - S, C - 1}, {0, 1, 2, 3}, 255, 10, v, 2, 64, nullptr);
        items += stats_case(25, 25, {-30, 12, 60, 13, 12, -40, 11, 70, -5, -5, 30, 30}, {0, 1, 2, 3, 4, 5}, 2, 127, v, 9, 64, &covered);      // both ends outside, crossing
        cases += 9;
    }
    if (covered == 0) { printf("no pixel was ever covered\n"); return 1; }
    // refusals of the host check
    int32_t nd[4] = {0, 0, 1, 1}, ed[2] = {0, 1};
    uint8_t m[4] = {0, 0, 0, 0};
    alignas(16) int32_t out[8];
    EdgeStatsParams p;
    p.g.nodes = nd; p.g.edges = ed; p.g.N = 2; p.g.E = 1; p.g.H = 2; p.g.W = 2; p.g.t = 1; p.mask = m; p.out = out; p.on_level = 255;
    bool ok = es_params_ok(p);
    p.on_level = 256; ok = ok && !es_params_ok(p);
    p.on_level = -1; ok = ok && !es_params_ok(p);
    p.on_level = 0; p.out = out + 1; ok = ok && !es_params_ok(p);               // out is 16-byte aligned
    p.out = nullptr; ok = ok && !es_params_ok(p);
    p.out = out; p.mask = nullptr; ok = ok && !es_params_ok(p);
    p.mask = m; p.g.t = 0; ok = ok && !es_params_ok(p);
    p.g.t = 256; ok = ok && !es_params_ok(p);
    p.g.t = 1; p.g.H = 0; ok = ok && !es_params_ok(p);
    p.g.H = 65536; p.g.W = 32768; ok = ok && !es_params_ok(p);                  // 2^31 pixels
    p.g.H = 2; p.g.W = 2; p.g.E = 0; ok = ok && !es_params_ok(p);               // E = 0 launches nothing
    p.g.E = 1; p.g.N = 0; ok = ok && !es_params_ok(p);
    p.g.N = 2; p.g.nodes = nullptr; ok = ok && !es_params_ok(p);
    p.g.nodes = nd; ok = ok && es_params_ok(p);
    if (!ok) { printf("the host check accepts or refuses wrongly\n"); return 1; }
    printf("edge support OK: %ld cases, %ld items, %ld pixels covered\n", cases, items, covered);
    return 0;
}
