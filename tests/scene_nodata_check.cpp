// The addressing of the two SCENE_NODATA kernels (sam_road_amd/csrc/scene_nodata_piece.hpp) on the CPU: every work item of whole match and
// grow launches runs through the kernels' own per-item code, in a stand-alone program built with the address and undefined-behaviour
// sanitizers (tests/test_scene_nodata_host.py builds and runs it).  The source, and_with, the destination and the LDS stand-ins are heap
// blocks of their exact sizes — the source placed at every 16-byte misalignment of its start, so that it ENDS at the block's end at every
// misalignment too, and the whole 8-byte granules in front of it poisoned — so a byte read past src or and_with, or written past dst, ends
// the program; the bytes in front of and between the outputs are guards that must come back unchanged, and the outputs must equal the rule
// restated here in plain loops.
#include <sanitizer/asan_interface.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "scene_nodata_piece.hpp"

using namespace srh;

static uint32_t rng_state = 2468u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

static uint8_t* block(size_t off, size_t bytes) {          // data at block + off, block 16-byte aligned, the block ends where the data ends
    void* b = nullptr;
    if (posix_memalign(&b, 16, off + bytes)) { printf("allocation failed\n"); exit(2); }
    return static_cast<uint8_t*>(b);
}

template <class T>
static long match_case(long n, int C, int src_off, int out_off, int aw_off, int any, int invert, bool with_and) {
    constexpr uint32_t levels = sizeof(T) == 1 ? 256u : 65536u;
    const size_t src_bytes = (size_t)n * C * sizeof(T);
    uint8_t* sblock = block(src_off, src_bytes);
    uint8_t* oblock = block(out_off, n);
    uint8_t* ablock = block(aw_off, n);
    T* src = reinterpret_cast<T*>(sblock + src_off);
    uint8_t *out = oblock + out_off, *aw = ablock + aw_off;
    const uint32_t top = (rnd() & 1) ? levels - 4 : 0;     // the values crowd at the bottom or at the top of the range
    for (long i = 0; i < n * C; ++i) src[i] = (T)(top + rnd() % 4);
    for (long i = 0; i < n; ++i) aw[i] = (uint8_t)((rnd() & 3) ? (rnd() | 1) : 0);
    memset(oblock, 0xA5, out_off + n);
    std::vector<uint8_t> src_before(sblock + src_off, sblock + src_off + src_bytes);
    if (src_off >= 8) __asan_poison_memory_region(sblock, 8);

    SceneNodataParams p;
    p.src = src; p.out = out; p.and_with = with_and ? aw : nullptr; p.n = n; p.C = C; p.wide = sizeof(T) == 2; p.any = any; p.invert = invert;
    uint32_t lo[ND_MAX_C], hi[ND_MAX_C];
    for (int c = 0; c < C; ++c) {
        lo[c] = top + rnd() % 3; hi[c] = lo[c] + rnd() % 3;
        if (hi[c] > levels - 1) hi[c] = levels - 1;
        if (rnd() % 7 == 0) { lo[c] = 0; hi[c] = levels - 1; }
        p.lohi[c] = lo[c] | (hi[c] << 16);
    }
    if (!nodata_params_ok(p)) { printf("parameters refused\n"); exit(2); }
    const long items = nodata_items(p);
    for (long i = items - 1; i >= 0; --i) nodata_match_item<T>(p, i);          // any order: the items are independent
    for (long i = 0; i < n; ++i) {
        int cnt = 0;
        for (int c = 0; c < C; ++c) cnt += src[i * C + c] >= lo[c] && src[i * C + c] <= hi[c];
        int v = any ? cnt > 0 : cnt == C;
        if (invert) v = !v;
        if (with_and) v = v && aw[i] != 0;
        if (out[i] != v) {
            printf("wrong byte: n %ld C %d pixel %ld src_off %d out_off %d any %d invert %d and %d\n", n, C, i, src_off, out_off, any, invert, (int)with_and);
            exit(1);
        }
    }
    for (int k = 0; k < out_off; ++k)
        if (oblock[k] != 0xA5) { printf("guard byte %d in front of out written (n %ld C %d)\n", k, n, C); exit(1); }
    if (memcmp(src_before.data(), src, src_bytes) != 0) { printf("the source was written\n"); exit(1); }
    if (src_off >= 8) __asan_unpoison_memory_region(sblock, 8);
    free(sblock); free(oblock); free(ablock);
    return items;
}

struct Img { long off; int H, W; };

static long grow_case(const std::vector<Img>& imgs, long bytes, int r, int invert, bool with_and, int dst_off, int seed_mode) {
    uint8_t* src = block(0, bytes);
    uint8_t* aw = block(0, bytes);
    uint8_t* dblock = block(dst_off, bytes);
    uint8_t* dst = dblock + dst_off;
    uint8_t* win = block(0, NG_WIN_BYTES);
    uint8_t* row = block(0, NG_ROW_BYTES);
    for (long i = 0; i < bytes; ++i) {
        // seed_mode 0: sparse, 1: none, 2: all, 3: dense; the bytes between the blocks are set: nothing connects two images
        src[i] = seed_mode == 1 ? 0 : (seed_mode == 2 ? 7 : (uint8_t)((rnd() % (seed_mode == 0 ? 257 : 5)) == 0 ? 1 + rnd() % 255 : 0));
        aw[i] = (uint8_t)((rnd() & 3) ? 1 + rnd() % 255 : 0);
    }
    std::vector<int64_t> table(imgs.size() * NG_COLS, -12345);                 // columns 3 .. 7 are not read
    std::vector<uint8_t> inside(bytes, 0);
    for (size_t k = 0; k < imgs.size(); ++k) {
        table[k * NG_COLS + NG_OFF] = imgs[k].off; table[k * NG_COLS + NG_H] = imgs[k].H; table[k * NG_COLS + NG_W] = imgs[k].W;
        for (long i = 0; i < (long)imgs[k].H * imgs[k].W; ++i) inside[imgs[k].off + i] = 1;
        if (seed_mode == 0) {                                                  // the four corners and both sides of every block boundary
            const int H = imgs[k].H, W = imgs[k].W;
            uint8_t* im = src + imgs[k].off;
            im[0] = im[W - 1] = im[(long)(H - 1) * W] = im[(long)H * W - 1] = 255;
            if (H > NG_BH && W > NG_BW) { im[(long)(NG_BH - 1) * W + NG_BW - 1] = 1; im[(long)NG_BH * W + NG_BW] = 1; }
        }
    }
    for (long i = 0; i < bytes; ++i)
        if (!inside[i]) src[i] = 255;
    memset(dblock, 0xA5, dst_off + bytes);
    std::vector<uint8_t> src_before(src, src + bytes);
    if (!grow_table_ok(table.data(), (int)imgs.size(), bytes)) { printf("table refused\n"); exit(2); }

    SceneGrowParams p;
    p.src = src; p.dst = dst; p.and_with = with_and ? aw : nullptr; p.table = table.data(); p.n = (int)imgs.size(); p.r = r; p.invert = invert;
    long blocks = 0;
    for (int k = p.n - 1; k >= 0; --k) {
        const long nb = grow_blocks(imgs[k].H, imgs[k].W);
        for (long b = nb - 1; b >= 0; --b, ++blocks) {
            const NgBlock g = grow_locate(p, k, b);
            memset(win, 0xEE, NG_WIN_BYTES); memset(row, 0xEE, NG_ROW_BYTES);   // what a phase does not write must not be read as 0
            for (int t = (NG_BH + 2 * r) * (NG_BW + 2 * r) - 1; t >= 0; --t) grow_stage_item(p, g, win, t);
            for (int t = (NG_BH + 2 * r) * NG_BW - 1; t >= 0; --t) grow_row_item(p, win, row, t);
            for (int t = NG_BH * NG_BW / 4 - 1; t >= 0; --t) grow_col_item(p, g, row, t);
        }
    }
    for (size_t k = 0; k < imgs.size(); ++k) {
        const int H = imgs[k].H, W = imgs[k].W;
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                int v = 0;
                for (int yy = y - r; yy <= y + r && !v; ++yy)
                    for (int xx = x - r; xx <= x + r && !v; ++xx)
                        if (yy >= 0 && yy < H && xx >= 0 && xx < W) v = src[imgs[k].off + (long)yy * W + xx] != 0;
                if (invert) v = !v;
                const long at = imgs[k].off + (long)y * W + x;
                if (with_and) v = v && aw[at] != 0;
                if (dst[at] != v) { printf("grow: wrong byte, image %zu (%d x %d) at (%d, %d), r %d invert %d and %d\n", k, H, W, y, x, r, invert, (int)with_and); exit(1); }
            }
    }
    for (long i = 0; i < bytes; ++i)
        if (!inside[i] && dst[i] != 0xA5) { printf("grow: byte %ld between the blocks written\n", i); exit(1); }
    for (int k = 0; k < dst_off; ++k)
        if (dblock[k] != 0xA5) { printf("grow: guard byte %d in front of dst written\n", k); exit(1); }
    if (memcmp(src_before.data(), src, bytes) != 0) { printf("grow: the source was written\n"); exit(1); }
    free(src); free(aw); free(dblock); free(win); free(row);
    return blocks;
}

int main() {
    const int Cs[] = {1, 3, 4, 5, 16};
    const long ns[] = {1, 2, 3, 4, 5, 7, 17, 100, 1961};
    long cases = 0, items = 0;
    for (int C : Cs)
        for (long n : ns)
            for (int src_off = 0; src_off < 16; ++src_off) {
                const int f = (int)(rnd() & 7), out_off = (int)(rnd() & 3) + 4 * (src_off & 1), aw_off = (int)(rnd() & 3);
                items += match_case<uint8_t>(n, C, src_off, out_off, aw_off, f & 1, (f >> 1) & 1, f >> 2);           // any byte address
                items += match_case<uint8_t>(n, C, src_off, 0, 0, ~f & 1, (~f >> 1) & 1, !(f >> 2));
                items += match_case<uint16_t>(n, C, src_off & 14, out_off, aw_off, f & 1, (f >> 1) & 1, f >> 2);    // any 2-byte-aligned address
                items += match_case<uint16_t>(n, C, (src_off + 8) & 14, 0, 0, ~f & 1, (~f >> 1) & 1, !(f >> 2));
                cases += 4;
            }
    long blocks = 0;
    const int rs[] = {1, 2, 7, 16};
    const int shapes[][2] = {{1, 1}, {7, 5}, {64, 64}, {65, 130}, {70, 3}, {3, 129}};
    for (int r : rs)
        for (int mode = 0; mode < 4; ++mode) {
            for (const auto& s : shapes) {
                blocks += grow_case({{0, s[0], s[1]}}, (long)s[0] * s[1], r, mode & 1, (mode & 2) != 0, mode, mode);
                ++cases;
            }
            // three images in one call at odd offsets, in an order of their own, with gaps in front, between and behind
            blocks += grow_case({{3 + 65 * 67 + 5, 1, 1}, {3, 65, 67}, {3 + 65 * 67 + 5 + 1 + 1, 9, 131}}, 3 + 65 * 67 + 5 + 1 + 1 + 9 * 131 + 2, r, ~mode & 1,
                                (mode & 2) == 0, 1, mode == 1 ? 0 : mode);
            ++cases;
        }
    // refusals of the two host checks
    SceneNodataParams p;
    uint16_t one[16] = {0};
    uint8_t o[4];
    p.src = one; p.out = o; p.n = 1; p.C = 3;
    bool ok = nodata_params_ok(p);
    p.C = 0; ok = ok && !nodata_params_ok(p);
    p.C = 17; ok = ok && !nodata_params_ok(p);
    p.C = 3; p.n = 0; ok = ok && !nodata_params_ok(p);
    p.n = ND_MAX_PIXELS + 1; ok = ok && !nodata_params_ok(p);
    p.n = 1; p.any = 2; ok = ok && !nodata_params_ok(p);
    p.any = 0; p.invert = 2; ok = ok && !nodata_params_ok(p);
    p.invert = 0; p.wide = 1; p.src = reinterpret_cast<const uint8_t*>(one) + 1; ok = ok && !nodata_params_ok(p);
    p.src = nullptr; ok = ok && !nodata_params_ok(p);
    p.src = one; p.wide = 0; p.out = nullptr; ok = ok && !nodata_params_ok(p);
    int64_t t[2 * NG_COLS] = {0, 4, 4, 0, 0, 0, 0, 0, 16, 2, 2, 0, 0, 0, 0, 0};
    ok = ok && grow_table_ok(t, 2, 20) && !grow_table_ok(t, 2, 19) && !grow_table_ok(t, 0, 20) && !grow_table_ok(nullptr, 1, 20);
    t[NG_COLS] = 15; ok = ok && !grow_table_ok(t, 2, 20);                      // overlaps the first block
    t[NG_COLS] = 16; t[NG_H] = 0; ok = ok && !grow_table_ok(t, 2, 20);
    t[NG_H] = 4; t[NG_OFF] = -1; ok = ok && !grow_table_ok(t, 2, 20);
    t[NG_OFF] = 0; t[NG_H] = 65536; t[NG_W] = 32768; ok = ok && !grow_table_ok(t, 1, 1LL << 40);      // 2^31 pixels
    if (!ok) { printf("a host check accepts or refuses wrongly\n"); return 1; }
    // the item count of the largest match launch, in 64-bit arithmetic
    p = SceneNodataParams(); p.n = ND_MAX_PIXELS;
    if (nodata_items(p) != 536870912L) { printf("item count of the largest launch\n"); return 1; }
    printf("scene nodata OK: %ld cases, %ld match items, %ld grow blocks\n", cases, items, blocks);
    return 0;
}
