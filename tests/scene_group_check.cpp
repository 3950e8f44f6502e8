// The scene-group kernels' addressing on a CPU: every (stack row, piece) item of whole pack and crop launches, cut into groups exactly as
// launch_scene_group_pack / _crop cut them, is run through the kernels' own per-item code (sam_road_amd/csrc/scene_group_piece.hpp) and
// compared with a per-pixel restatement of DESIGN.md §6h.  Sources and destinations are exact-size heap blocks at every misalignment
// 0..15 (built with the address sanitizer a read or write one byte outside either is an error; without it the bytes in front of a
// destination are a sentinel).  Every launch runs twice, onto 0x00 and onto 0xFF, so a destination byte that no item writes shows; the
// sources must come out unchanged.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "scene_group_piece.hpp"

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

struct Scene { int H, W, top, bottom, left, right; };

template <int C>
static void emulate_pack(const SceneGroupParams& p) {
    const long gpr = group_groups_per_row(p.Wa, C), n_groups = gpr * p.Ha;
    for (long g = 0; g < n_groups; ++g) {
        const long Y = g / gpr, piece0 = (g - Y * gpr) * PAD_PIECES;
        const GroupRow row = group_pack_row<C>(p, Y);
        const long piece_end = piece0 + PAD_PIECES < row.r.n_pieces ? piece0 + PAD_PIECES : row.r.n_pieces;
        for (int tid = 0; tid < PAD_THREADS; ++tid)
            for (long pc = piece0 + tid; pc < piece_end; pc += PAD_THREADS) group_pack_piece<C>(row, pc);
    }
}

static void emulate_crop(const SceneGroupParams& p) {
    const long gpr = group_groups_per_row(p.Wa, 1), n_groups = gpr * p.Ha;
    for (long g = 0; g < n_groups; ++g) {
        const long Y = g / gpr, piece0 = (g - Y * gpr) * PAD_PIECES;
        const GroupRow row = group_crop_row(p, Y);
        const long piece_end = piece0 + PAD_PIECES < row.r.n_pieces ? piece0 + PAD_PIECES : row.r.n_pieces;
        for (int tid = 0; tid < PAD_THREADS; ++tid)
            for (long pc = piece0 + tid; pc < piece_end; pc += PAD_THREADS) group_crop_piece(row, pc);
    }
}

static long n_cases = 0;

struct Blocks {                                            // exact-size blocks: [raw, raw + mis) is slack in front, the buffer ends where the block ends
    std::vector<uint8_t*> raw;
    std::vector<int> mis;
    uint8_t* at(size_t n, int m) {
        uint8_t* r = (uint8_t*)malloc(m + n);
        if (!r || ((uintptr_t)r & 15)) { printf("malloc did not return a 16-byte aligned block\n"); exit(2); }
        raw.push_back(r); mis.push_back(m);
        memset(r, 0xA5, m);
        SRH_POISON(r, m);
        return r + m;
    }
    bool release() {                                       // nothing in front of any block was written
        bool ok = true;
        for (size_t i = 0; i < raw.size(); ++i) {
            SRH_UNPOISON(raw[i], mis[i]);
            for (int k = 0; k < mis[i]; ++k) ok = ok && raw[i][k] == 0xA5;
            free(raw[i]);
        }
        return ok;
    }
};

// One group: pack (C channels, `mode`) against the restatement, then crop of two random masks of the stack's size against slicing.
static bool run_case(const std::vector<Scene>& sc, int Wa_extra, int C, int mode, int src_mis, int dst_mis) {
    const int n = (int)sc.size();
    std::vector<int64_t> tp(n * GROUP_COLS), tc(n * GROUP_COLS);
    long Ha = 0, Wa = 0, src_b = 0, out_b = 0;
    for (int k = 0; k < n; ++k) {
        const Scene& s = sc[k];
        const long Hv = s.H + s.top + s.bottom, Wv = s.W + s.left + s.right;
        const int64_t row[GROUP_COLS] = {src_b, s.H, s.W, s.top, s.left, Hv, Wv, Ha};
        memcpy(&tp[k * GROUP_COLS], row, sizeof row);
        memcpy(&tc[k * GROUP_COLS], row, sizeof row);
        tc[k * GROUP_COLS + GROUP_OFF] = out_b;
        src_b += (long)s.H * s.W * C;
        out_b += (long)s.H * s.W;
        Ha += Hv;
        if (Wv > Wa) Wa = Wv;
    }
    Wa += Wa_extra;
    const size_t nd = (size_t)Ha * Wa * C, nm = (size_t)Ha * Wa;
    Blocks bl;
    uint8_t* src = bl.at(src_b, src_mis);
    uint8_t* dst = bl.at(nd, dst_mis);
    uint8_t* mask = bl.at(nm, (src_mis * 7 + 3) & 15);
    uint8_t* out = bl.at(out_b, (dst_mis + 5) & 15);
    uint32_t seed = 777u + n * 131 + (uint32_t)Wa * 7 + C;
    for (long i = 0; i < src_b; ++i) { seed = seed * 1664525u + 1013904223u; src[i] = (uint8_t)(seed >> 24); }
    for (size_t i = 0; i < nm; ++i) { seed = seed * 1664525u + 1013904223u; mask[i] = (uint8_t)(seed >> 24); }
    std::vector<uint8_t> src_before(src, src + src_b), mask_before(mask, mask + nm);
    const uint8_t fill[3] = {124, 116, 104};
    bool ok = group_table_ok(tp.data(), n, C, (int)Ha, (int)Wa, src_b, false) && group_table_ok(tc.data(), n, 1, (int)Ha, (int)Wa, out_b, true);
    if (!ok) printf("the table of a case was refused\n");
    SceneGroupParams p;
    p.src = src; p.dst = dst; p.table = tp.data(); p.n = n; p.Ha = (int)Ha; p.Wa = (int)Wa; p.C = C; p.mode = mode;
    p.fill = fill[0] | (fill[1] << 8) | (fill[2] << 16);
    SceneGroupParams q;
    q.src = mask; q.dst = out; q.table = tc.data(); q.n = n; q.Ha = (int)Ha; q.Wa = (int)Wa; q.C = 1; q.mode = PAD_EDGE;
    for (int pass = 0; pass < 2 && ok; ++pass) {
        memset(dst, pass ? 0xFF : 0x00, nd);
        memset(out, pass ? 0xFF : 0x00, out_b);
        if (C == 3) emulate_pack<3>(p); else emulate_pack<1>(p);
        emulate_crop(q);
        long row0 = 0, off = 0, soff = 0;
        for (int k = 0; k < n && ok; ++k) {
            const Scene& s = sc[k];
            const int Hv = s.H + s.top + s.bottom, Wv = s.W + s.left + s.right;
            for (int Y = 0; Y < Hv && ok; ++Y)
                for (int X = 0; X < Wa && ok; ++X) {
                    const int sy = ref_fold((long)Y - s.top, s.H, mode), sx = X < Wv ? ref_fold((long)X - s.left, s.W, mode) : 0;
                    for (int ch = 0; ch < C; ++ch) {
                        uint8_t want = 0;
                        if (X < Wv) want = (sy < 0 || sx < 0) ? fill[ch] : src_before[soff + ((size_t)sy * s.W + sx) * C + ch];
                        const uint8_t got = dst[((size_t)(row0 + Y) * Wa + X) * C + ch];
                        if (want != got) {
                            printf("PACK MISMATCH n %d scene %d (%d x %d) C %d mode %d mis %d/%d at (%d, %d, %d): got %d want %d\n", n, k, s.H, s.W, C,
                                   mode, src_mis, dst_mis, Y, X, ch, got, want);
                            ok = false;
                            break;
                        }
                    }
                }
            for (int y = 0; y < s.H && ok; ++y)
                for (int x = 0; x < s.W; ++x) {
                    const uint8_t want = mask_before[(size_t)(row0 + s.top + y) * Wa + s.left + x], got = out[off + (long)y * s.W + x];
                    if (want != got) {
                        printf("CROP MISMATCH n %d scene %d (%d x %d) mis %d/%d at (%d, %d): got %d want %d\n", n, k, s.H, s.W, src_mis, dst_mis, y, x,
                               got, want);
                        ok = false;
                        break;
                    }
                }
            row0 += Hv; off += (long)s.H * s.W; soff += (long)s.H * s.W * C;
        }
    }
    ok = ok && memcmp(src, src_before.data(), src_b) == 0 && memcmp(mask, mask_before.data(), nm) == 0;
    ok = bl.release() && ok;
    ++n_cases;
    return ok;
}

int main() {
    // widths 1, 5, 16, 17 and 523 mixed (gap columns), a scene as wide as the stack, axes of length 1, pads of 0 and several times the axis
    const std::vector<Scene> seven = {{3, 1, 0, 0, 0, 0}, {4, 5, 2, 1, 3, 0}, {2, 16, 0, 0, 0, 0}, {5, 17, 1, 0, 0, 2}, {3, 523, 0, 2, 1, 0},
                                      {1, 1, 4, 4, 4, 4}, {7, 5, 40, 3, 30, 41}};
    const std::vector<std::vector<Scene>> groups = {
        seven,
        {{37, 53, 5, 9, 3, 1}},                                        // n = 1: a scene as wide as the stack
        {{6, 40, 0, 0, 0, 0}, {1, 64, 2, 3, 7, 9}, {64, 1, 3, 2, 9, 7}},
        {{2, 2, 9, 0, 0, 9}, {3, 40, 1, 1, 0, 0}},
        {{2, 5500, 1, 0, 2, 3}, {3, 17, 0, 0, 0, 0}},                  // a stack row of more than PAD_PIECES pieces: two groups per row
    };
    bool ok = true;
    for (size_t gi = 0; gi < groups.size(); ++gi)
        for (int C : {1, 3})
            for (int mode : {PAD_REFLECT, PAD_EDGE, PAD_CONSTANT}) {
                const bool big = gi == 4;
                for (int sm = 0; sm < 16; sm += big ? 5 : 1)
                    for (int dm = 0; dm < 16; dm += big ? 7 : 3)
                        ok = run_case(groups[gi], gi == 3 ? 6 : 0, C, mode, sm, (dm + sm) & 15) && ok;      // group 3: a stack wider than every scene
            }
    // group_find at the borders of every scene of the table of seven
    {
        std::vector<int64_t> t(7 * GROUP_COLS, 0);
        long row0 = 0;
        for (int k = 0; k < 7; ++k) { t[k * GROUP_COLS + GROUP_ROW0] = row0; row0 += seven[k].H + seven[k].top + seven[k].bottom; }
        for (int k = 0; k < 7; ++k) {
            const long a = t[k * GROUP_COLS + GROUP_ROW0], b = (k < 6 ? t[(k + 1) * GROUP_COLS + GROUP_ROW0] : row0) - 1;
            if (group_find(t.data(), 7, a) != k || group_find(t.data(), 7, b) != k) { printf("group_find fails at scene %d\n", k); ok = false; }
        }
        if (group_find(t.data(), 1, 5) != 0) ok = false;
    }
    // tables the entries must refuse
    {
        const int64_t good[2 * GROUP_COLS] = {0, 4, 5, 1, 2, 6, 8, 0, 60, 3, 3, 0, 0, 3, 3, 6};
        auto bad = [&](int i, int64_t v, bool contiguous = false, long long bytes = 60 + 27) {
            int64_t t[2 * GROUP_COLS];
            memcpy(t, good, sizeof t);
            if (i >= 0) t[i] = v;
            return !group_table_ok(t, 2, 3, 9, 8, bytes, contiguous);
        };
        const bool tables = !bad(-1, 0) && !bad(-1, 0, true) && bad(1, 0) && bad(3, -1) && bad(4, -1) && bad(5, 4) && bad(6, 6) && bad(6, 9) &&
                            bad(15, 5) && bad(13, 4) && bad(8, 61) && bad(0, -1) && bad(8, 59, true) && bad(-1, 0, true, 88) && bad(-1, 0, false, 86);
        if (!tables) printf("group_table_ok accepts a bad table or refuses a good one\n");
        ok = ok && tables;
    }
    printf("%ld cases\n", n_cases);
    if (!ok) return 1;
    printf("scene group OK\n");
    return 0;
}
