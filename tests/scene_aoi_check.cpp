// The addressing and the arithmetic of the SCENE_AOI kernel (sam_road_amd/csrc/scene_aoi_piece.hpp) on the CPU: every work item of every
// phase of whole launches runs through the kernel's own per-item code, in a stand-alone program built with the address and undefined-
// behaviour sanitizers (tests/test_scene_aoi_host.py builds and runs it).  The tables, and_with, the destination and the LDS stand-in are
// heap blocks of their exact sizes, the destination placed at every alignment mod 16 so that it ENDS at its block's end at every alignment
// too: a byte read past a table or and_with, or written past out, ends the program; the bytes in front of out are guards that must come
// back unchanged, the tables must come back unwritten, and the output must equal the rule restated here in plain loops WITHOUT a
// division: an edge that crosses row y toggles pixel x iff (x0 - 128) dy + (yc - y0) dx <= 256 x dy.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "scene_aoi_piece.hpp"

using namespace srh;

static uint32_t rng_state = 13579u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

static uint8_t* block(size_t off, size_t bytes) {          // data at block + off, block 16-byte aligned, the block ends where the data ends
    void* b = nullptr;
    if (posix_memalign(&b, 16, off + bytes + (off + bytes == 0))) { printf("allocation failed\n"); exit(2); }
    return static_cast<uint8_t*>(b);
}

struct Poly { std::vector<AoiEdge> edges; };

// Every phase of the workgroup that owns row y, item by item, in descending item order (the items of a phase are independent).
static void run_row(const SceneAoiParams& p, AoiLds& l, long y) {
    const int n_polys = p.n_include + p.n_exclude;
    for (long x0 = 0; x0 < p.W; x0 += AOI_SEG) {
        memset(&l, 0xEE, sizeof(l));                       // what a phase does not write must not be read as 0
        for (int t = AOI_THREADS - 1; t >= 0; --t) aoi_begin_item(l, t);
        for (int k = 0; k < n_polys; ++k) {
            for (int t = AOI_THREADS - 1; t >= 0; --t) aoi_clear_item(l, t);
            for (int e = p.polys[k + 1] - 1; e >= p.polys[k]; --e) aoi_edge_item(p, l, y, x0, e);
            for (int t = AOI_THREADS - 1; t >= 0; --t) aoi_scan_item(l, t);
            for (int t = AOI_THREADS - 1; t >= 0; --t) aoi_fold_item(l, t, k < p.n_include);
        }
        for (int t = AOI_THREADS - 1; t >= 0; --t) aoi_final_item(p, l, t);
        for (int c = aoi_store_chunks(p, y, x0) - 1; c >= 0; --c) aoi_store_item(p, l, y, x0, c);
    }
}

static long fill_case(int H, int W, const std::vector<Poly>& inc, const std::vector<Poly>& exc, int out_off, int invert, bool with_and, long* set) {
    std::vector<int32_t> polys{0};
    std::vector<AoiEdge> all;
    for (const auto* list : {&inc, &exc})
        for (const Poly& q : *list) {
            all.insert(all.end(), q.edges.begin(), q.edges.end());
            polys.push_back((int32_t)all.size());
        }
    const size_t E = all.size(), n = (size_t)H * W;
    uint8_t* eblock = block(0, E * sizeof(AoiEdge));       // exact size: an edge read past the table ends the program
    uint8_t* pblock = block(0, polys.size() * 4);
    uint8_t* oblock = block(out_off, n);
    uint8_t* ablock = block(3, n);
    if (E) memcpy(eblock, all.data(), E * sizeof(AoiEdge));
    memcpy(pblock, polys.data(), polys.size() * 4);
    uint8_t *out = oblock + out_off, *aw = ablock + 3;
    for (size_t i = 0; i < n; ++i) aw[i] = (uint8_t)((rnd() & 3) ? (rnd() | 1) : 0);
    memset(oblock, 0xA5, out_off + n);
    AoiLds* lds = reinterpret_cast<AoiLds*>(block(0, sizeof(AoiLds)));

    SceneAoiParams p;
    p.edges = reinterpret_cast<const int32_t*>(eblock); p.polys = reinterpret_cast<const int32_t*>(pblock); p.and_with = with_and ? aw : nullptr;
    p.out = out; p.n_include = (int)inc.size(); p.n_exclude = (int)exc.size(); p.H = H; p.W = W; p.invert = invert;
    if (!aoi_params_ok(p) || !aoi_table_ok(p.edges, p.polys, p.n_include, p.n_exclude)) { printf("parameters refused\n"); exit(2); }
    for (long y = H - 1; y >= 0; --y) run_row(p, *lds, y);

    long ones = 0;
    for (int y = 0; y < H; ++y) {
        const long yc = 256L * y + 128;
        for (int x = 0; x < W; ++x) {
            int in_inc = inc.empty(), in_exc = 0, k = 0;
            for (const auto* list : {&inc, &exc}) {
                for (const Poly& q : *list) {
                    int toggles = 0;
                    for (const AoiEdge& e : q.edges) {
                        if (yc < e.y0 || yc >= e.y1) continue;
                        const __int128 dy = (long)e.y1 - e.y0, dx = (long)e.x1 - e.x0;
                        toggles += ((__int128)e.x0 - 128) * dy + ((__int128)yc - e.y0) * dx <= (__int128)256 * x * dy;
                    }
                    if (toggles & 1) (k == 0 ? in_inc : in_exc) = 1;
                }
                ++k;
            }
            int v = in_inc && !in_exc;
            ones += v;
            if (invert) v = !v;
            if (with_and) v = v && aw[(long)y * W + x] != 0;
            if (out[(long)y * W + x] != v) {
                printf("wrong byte: %d x %d at (%d, %d), %zu + %zu polygons, out_off %d invert %d and %d: %d\n", H, W, y, x, inc.size(), exc.size(), out_off, invert,
                       (int)with_and, out[(long)y * W + x]);
                exit(1);
            }
        }
    }
    for (int k = 0; k < out_off; ++k)
        if (oblock[k] != 0xA5) { printf("guard byte %d in front of out written (%d x %d)\n", k, H, W); exit(1); }
    if ((E && memcmp(eblock, all.data(), E * sizeof(AoiEdge)) != 0) || memcmp(pblock, polys.data(), polys.size() * 4) != 0) { printf("a table was written\n"); exit(1); }
    free(eblock); free(pblock); free(oblock); free(ablock); free(lds);
    if (set) *set += ones;
    return (long)H * ((W + AOI_SEG - 1) / AOI_SEG);
}

static Poly ring(const std::vector<std::pair<long, long>>& v) {               // (y, x) in 1/256 px
    Poly q;
    for (size_t i = 0; i < v.size(); ++i) {
        const auto a = v[i], b = v[(i + 1) % v.size()];
        if (a.first == b.first) continue;
        const auto lo = a.first < b.first ? a : b, hi = a.first < b.first ? b : a;
        q.edges.push_back({(int32_t)lo.first, (int32_t)lo.second, (int32_t)hi.first, (int32_t)hi.second});
    }
    return q;
}

static Poly random_ring(int H, int W, int nv, bool on_centres) {
    std::vector<std::pair<long, long>> v;
    for (int i = 0; i < nv; ++i) {
        long y = (long)(rnd() % (unsigned)(256 * (H + 8))) - 1024, x = (long)(rnd() % (unsigned)(256 * (W + 8))) - 1024;
        if (on_centres) { y = (y / 256) * 256 + 128; x = (x / 256) * 256 + 128; }
        v.push_back({y, x});
    }
    return ring(v);
}

int main() {
    long cases = 0, segments = 0, ones = 0;
    const int shapes[][2] = {{1, 1}, {7, 5}, {3, 33}, {5, 64}, {9, 130}, {2, AOI_SEG}, {2, AOI_SEG + 1}, {1, 2 * AOI_SEG + 37}};
    for (const auto& s : shapes) {
        const int H = s[0], W = s[1];
        for (int off = 0; off < 16; ++off) {
            const int f = (int)(rnd() & 7);
            std::vector<Poly> inc, exc;
            // a triangle over the scene's corner, a random ring (every other case on pixel centres), a random exclude in half the cases
            inc.push_back(ring({{-300, -200}, {256L * H + 77, -200}, {-300, 256L * W + 900}}));
            inc.push_back(random_ring(H, W, 3 + (int)(rnd() % 9), off & 1));
            if (off & 2) exc.push_back(random_ring(H, W, 3 + (int)(rnd() % 5), off & 4));
            segments += fill_case(H, W, inc, exc, off, f & 1, (f & 2) != 0, &ones);
            // no include polygon: the whole scene, minus the exclude
            segments += fill_case(H, W, {}, exc, (off + 5) & 15, (f >> 2) & 1, (f & 1) != 0, nullptr);
            cases += 2;
        }
    }
    // more edges than threads in one polygon, many toggles in one word: a 700-vertex zigzag
    {
        std::vector<std::pair<long, long>> v;
        for (int i = 0; i < 700; ++i) v.push_back({(i & 1) ? 256L * 40 + 13 : -77, 64L + 47 * i});
        v.push_back({256L * 60, 47L * 700});
        v.push_back({256L * 60, 0});
        for (int off : {0, 1, 15}) { segments += fill_case(50, 140, {ring(v)}, {}, off, 0, off == 1, &ones); ++cases; }
    }
    // the polygon limit: 64 small squares, half of them excluded; and coordinates at the limits of the table
    {
        std::vector<Poly> inc, exc;
        for (int k = 0; k < AOI_MAX_POLYGONS; ++k) {
            const long y = 256L * (3 * (k / 8)) + 100, x = 256L * (5 * (k % 8)) + 50;
            (k & 1 ? exc : inc).push_back(ring({{y, x}, {y, x + 1000}, {y + 600, x + 1000}, {y + 600, x}}));
        }
        inc.push_back(ring({{0, 0}, {0, 256 * 45}, {256 * 30, 256 * 45}, {256 * 30, 0}}));
        inc.erase(inc.begin());
        segments += fill_case(26, 43, inc, exc, 7, 0, false, &ones);
        const long M = AOI_MAX_COORD;
        segments += fill_case(11, 9, {ring({{-M, -M}, {M, M}, {M, -M}})}, {ring({{-M, M}, {M, -M + 5}, {M, M}})}, 3, 0, true, &ones);
        cases += 2;
    }
    if (ones == 0) { printf("no pixel was ever inside\n"); return 1; }
    // refusals of the two host checks
    alignas(16) int32_t e[8] = {0, 0, 256, 0, 5, 5, 900, 5};
    int32_t o[3] = {0, 1, 2};
    uint8_t out[4];
    SceneAoiParams p;
    p.edges = e; p.polys = o; p.out = out; p.n_include = 1; p.n_exclude = 1; p.H = 2; p.W = 2;
    bool ok = aoi_params_ok(p) && aoi_table_ok(e, o, 1, 1);
    p.H = 0; ok = ok && !aoi_params_ok(p);
    p.H = 65536; p.W = 32768; ok = ok && !aoi_params_ok(p);                    // 2^31 pixels
    p.H = 2; p.W = 2; p.invert = 2; ok = ok && !aoi_params_ok(p);
    p.invert = 0; p.n_include = 33; p.n_exclude = 32; ok = ok && !aoi_params_ok(p);
    p.n_include = -1; p.n_exclude = 1; ok = ok && !aoi_params_ok(p);
    p.n_include = 1; p.edges = e + 1; ok = ok && !aoi_params_ok(p);            // a misaligned table
    p.edges = nullptr; ok = ok && !aoi_params_ok(p);
    p.edges = e; p.out = nullptr; ok = ok && !aoi_params_ok(p);
    ok = ok && !aoi_table_ok(nullptr, o, 1, 1) && !aoi_table_ok(e, nullptr, 1, 1) && !aoi_table_ok(e, o, -1, 1) && !aoi_table_ok(e, o, 65, 0);
    o[0] = 1; ok = ok && !aoi_table_ok(e, o, 1, 1);                            // does not start at 0
    o[0] = 0; o[1] = 2; o[2] = 1; ok = ok && !aoi_table_ok(e, o, 1, 1);        // not a running sum
    o[1] = 1; o[2] = 2; e[2] = 0; ok = ok && !aoi_table_ok(e, o, 1, 1);        // y0 >= y1
    e[2] = 256; e[7] = AOI_MAX_COORD + 1; ok = ok && !aoi_table_ok(e, o, 1, 1);
    e[7] = 5; o[2] = AOI_MAX_EDGES + 1; ok = ok && !aoi_table_ok(e, o, 1, 1);
    if (!ok) { printf("a host check accepts or refuses wrongly\n"); return 1; }
    printf("scene aoi OK: %ld cases, %ld row segments, %ld pixels inside\n", cases, segments, ones);
    return 0;
}
