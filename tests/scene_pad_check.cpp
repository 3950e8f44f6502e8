// The scene-pad kernel's addressing on a CPU: every (row, piece) item of a launch, cut into groups exactly as launch_scene_pad cuts it,
// is run through the kernel's own pad_row / pad_piece (sam_road_amd/csrc/scene_pad_piece.hpp) and compared with a per-pixel
// restatement of DESIGN.md §6g.  src and dst are exact-size heap blocks at every misalignment 0..15 (built with the address sanitizer
// a read or write one byte outside either is an error; without it the bytes in front of dst are a sentinel).  The launch runs twice, onto
// 0x00 and onto 0xFF, so a destination byte that no item writes shows; src must come out unchanged.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "scene_pad_piece.hpp"

using namespace srh;

#if defined(__has_feature)
#if __has_feature(address_sanitizer)
#include <sanitizer/asan_interface.h>
#define SRH_POISON(p, n) ASAN_POISON_MEMORY_REGION(p, n)
#define SRH_UNPOISON(p, n) ASAN_UNPOISON_MEMORY_REGION(p, n)
#endif
#endif
#ifndef SRH_POISON
#define SRH_POISON(p, n) ((void)0)
#define SRH_UNPOISON(p, n) ((void)0)
#endif

static int ref_fold(long i, int n, int mode) {            // DESIGN.md §6g, restated without the |i| shortcut
    if (mode == PAD_REFLECT) {
        if (n == 1) return 0;
        const long T = 2L * (n - 1);
        long j = i % T;
        if (j < 0) j += T;
        return (int)(j < n ? j : T - j);
    }
    if (mode == PAD_EDGE) return (int)(i < 0 ? 0 : (i >= n ? n - 1 : i));
    return i >= 0 && i < n ? (int)i : -1;
}

template <int C>
static void emulate_launch(const ScenePadParams& p) {
    const long gpr = pad_groups_per_row(p), n_groups = gpr * p.Hv;
    for (long g = 0; g < n_groups; ++g) {
        const long Y = g / gpr, piece0 = (g - Y * gpr) * PAD_PIECES;
        const PadRow r = pad_row<C>(p, Y);
        const long piece_end = piece0 + PAD_PIECES < r.n_pieces ? piece0 + PAD_PIECES : r.n_pieces;
        for (int tid = 0; tid < PAD_THREADS; ++tid)
            for (long pc = piece0 + tid; pc < piece_end; pc += PAD_THREADS) pad_piece<C>(p, r, pc);
    }
}

static long n_cases = 0;

static bool run_case(int H, int W, int C, int top, int bottom, int left, int right, int mode, int src_mis, int dst_mis) {
    const int Hv = H + top + bottom, Wv = W + left + right;
    const size_t ns = (size_t)H * W * C, nd = (size_t)Hv * Wv * C;
    // exact-size blocks: [raw, raw + mis) is slack in front (poisoned under the address sanitizer, a sentinel otherwise), the buffer ends
    // where the block ends, so the byte after it is the allocator's red zone
    std::vector<uint8_t*> keep;
    auto block_at = [&](size_t n, int mis) {
        uint8_t* raw = (uint8_t*)malloc(mis + n);
        if (!raw || ((uintptr_t)raw & 15)) return (uint8_t*)nullptr;
        keep.push_back(raw);
        memset(raw, 0xA5, mis);
        SRH_POISON(raw, mis);
        return raw + mis;
    };
    uint8_t* src = block_at(ns, src_mis);
    uint8_t* dst = block_at(nd, dst_mis);
    if (!src || !dst) { printf("malloc did not return a 16-byte aligned block\n"); return false; }
    uint32_t seed = 12345u + H * 131 + W * 7 + C;
    for (size_t i = 0; i < ns; ++i) { seed = seed * 1664525u + 1013904223u; src[i] = (uint8_t)(seed >> 24); }
    std::vector<uint8_t> src_before(src, src + ns);
    const uint8_t fill[3] = {124, 116, 104};
    ScenePadParams p;
    p.src = src; p.dst = dst; p.H = H; p.W = W; p.Hv = Hv; p.Wv = Wv; p.top = top; p.left = left; p.C = C; p.mode = mode;
    p.fill = fill[0] | (fill[1] << 8) | (fill[2] << 16);
    bool ok = pad_params_ok(p);
    for (int pass = 0; pass < 2 && ok; ++pass) {
        memset(dst, pass ? 0xFF : 0x00, nd);
        if (C == 3) emulate_launch<3>(p); else emulate_launch<1>(p);
        for (int Y = 0; Y < Hv && ok; ++Y)
            for (int X = 0; X < Wv && ok; ++X) {
                const int sy = ref_fold((long)Y - top, H, mode), sx = ref_fold((long)X - left, W, mode);
                for (int ch = 0; ch < C; ++ch) {
                    const uint8_t want = (sy < 0 || sx < 0) ? fill[ch] : src_before[((size_t)sy * W + sx) * C + ch];
                    const uint8_t got = dst[((size_t)Y * Wv + X) * C + ch];
                    if (want != got) {
                        printf("MISMATCH H %d W %d C %d pads %d %d %d %d mode %d mis %d/%d at (%d, %d, %d): got %d want %d\n", H, W, C, top, bottom,
                               left, right, mode, src_mis, dst_mis, Y, X, ch, got, want);
                        ok = false;
                        break;
                    }
                }
            }
    }
    ok = ok && memcmp(src, src_before.data(), ns) == 0;
    SRH_UNPOISON(keep[0], src_mis);
    SRH_UNPOISON(keep[1], dst_mis);
    for (int i = 0; i < dst_mis; ++i) ok = ok && keep[1][i] == 0xA5;          // nothing in front of dst was written
    for (uint8_t* b : keep) free(b);
    ++n_cases;
    return ok;
}

int main() {
    struct Shape { int H, W, top, bottom, left, right; };
    const Shape shapes[] = {
        {37, 53, 0, 0, 0, 0}, {37, 53, 5, 9, 3, 1}, {37, 53, 80, 3, 120, 0}, {1, 64, 2, 3, 7, 9}, {64, 1, 3, 2, 9, 7}, {1, 1, 4, 4, 4, 4},
        {2, 2, 9, 0, 0, 9}, {5, 7, 0, 11, 13, 0}, {3, 40, 1, 1, 0, 0}, {4, 16, 0, 0, 16, 16}, {7, 5, 40, 40, 40, 40}, {40, 11, 124, 124, 0, 3},
        {6, 5500, 1, 0, 2, 3},                              // a row of more than PAD_PIECES pieces: two groups per row
    };
    bool ok = true;
    for (const Shape& s : shapes)
        for (int C : {1, 3})
            for (int mode : {PAD_REFLECT, PAD_EDGE, PAD_CONSTANT}) {
                const bool big = s.W > 1000;
                for (int sm = 0; sm < 16; sm += big ? 5 : 1)
                    for (int dm = 0; dm < 16; dm += big ? 7 : 3)
                        ok = run_case(s.H, s.W, C, s.top, s.bottom, s.left, s.right, mode, sm, (dm + sm) & 15) && ok;
            }
    // pad_fold against the restatement, far outside the axis and at the largest axis an int holds
    for (int n : {1, 2, 3, 7, 2147483647})
        for (int mode : {PAD_REFLECT, PAD_EDGE, PAD_CONSTANT})
            for (long i : {-2147483647L, -1000003L, -41L, -8L, -7L, -6L, -1L, 0L, 1L, 5L, 6L, 7L, 12L, 13L, 40L, 2147483646L, 2147483647L})
                if (pad_fold(i, n, mode) != ref_fold(i, n, mode)) {
                    printf("pad_fold(%ld, %d, %d) = %d, want %d\n", i, n, mode, pad_fold(i, n, mode), ref_fold(i, n, mode));
                    ok = false;
                }
    printf("%ld cases\n", n_cases);
    if (!ok) return 1;
    printf("scene pad OK\n");
    return 0;
}
