// The resample kernel's addressing (sam_road_amd/csrc/scene_scale_piece.hpp) on the CPU: every block of a launch runs through the
// kernel's own per-item code — the block's source window, the staging loop's index-to-address map, the clamped tap indices of the row
// and column pass, the pieces of the output rows — in a stand-alone program built with the address and undefined-behaviour sanitizers
// (tests/test_scene_scale_host.py builds and runs it).  The source, the tables, the destination and the stand-in for LDS are heap blocks
// of their exact sizes; source and destination END at their block's end and start at every misalignment 0..3, so a byte read past src
// or the tables, or written past dst, ends the program.  The bytes in front of dst are guards that must come back unchanged, and the
// output must equal the rule of DESIGN.md §6j restated here from its formulas, pixel by pixel in 64-bit integers.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "scene_scale_piece.hpp"

using namespace srh;

static uint32_t rng_state = 4321u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

static long floor_div(long a, long b) { long d = a / b; return (a % b != 0 && ((a < 0) != (b < 0))) ? d - 1 : d; }
static long ceil_div(long a, long b) { return -floor_div(-a, b); }
static long clampl(long i, long lo, long hi) { return i < lo ? lo : (i > hi ? hi : i); }

// ---- the rule, restated: start and weights of output j on one axis ------------------------------------------------------------------
struct Axis { int T, D; };
static Axis axis_of(int p, int q) { return p < q ? Axis{(int)ceil_div(q, p) + 1, q} : Axis{2, 2 * p}; }
static long rule_start(long j, int p, int q) { return p < q ? floor_div(j * q, p) : floor_div((2 * j + 1) * q - p, 2L * p); }
static long rule_weight(long j, int t, int p, int q) {
    const long s = rule_start(j, p, q);
    if (p < q) {                                         // |[j q, (j + 1) q) ∩ [(s + t) p, (s + t + 1) p)|
        const long lo = (s + t) * p > j * q ? (s + t) * p : j * q, hi = (s + t + 1) * p < (j + 1) * q ? (s + t + 1) * p : (j + 1) * q;
        return hi > lo ? hi - lo : 0;
    }
    const long f = (2 * j + 1) * q - p - s * 2L * p;     // bilinear at pixel centres
    return t == 0 ? 2L * p - f : f;
}

template <class T>
static T* exact_block(size_t n) {                        // a heap block of exactly n elements: one element further is an error
    T* b = static_cast<T*>(malloc(n ? n * sizeof(T) : 1));
    if (!b) { printf("allocation failed\n"); exit(2); }
    return b;
}

// form 0: the LDS form with the block of the host's plan; 1: the direct form; 2: a window of one pixel (every block falls back)
static long run_case(int H, int W, int C, int p, int q, int Ho, int Wo, int mode, bool zero, int form, int src_off, int dst_off) {
    const Axis ay = axis_of(p, q), ax = ay;
    const size_t src_bytes = (size_t)H * W * C, dst_bytes = (size_t)Ho * Wo * C, guard = 64;
    void *sb = nullptr, *db = nullptr;
    if (posix_memalign(&sb, 16, src_off + src_bytes) || posix_memalign(&db, 16, guard + dst_off + dst_bytes)) { printf("allocation failed\n"); exit(2); }
    uint8_t *sblock = static_cast<uint8_t*>(sb), *dblock = static_cast<uint8_t*>(db);
    uint8_t *src = sblock + src_off, *dst = dblock + guard + dst_off;
    for (size_t i = 0; i < src_bytes; ++i) src[i] = mode == SCALE_VALID ? (uint8_t)((rnd() % 8 != 0) * (1 + rnd() % 255)) : (uint8_t)rnd();
    memset(dblock, 0xA5, guard + dst_off + dst_bytes);
    std::vector<uint8_t> src_before(src, src + src_bytes);

    int32_t *sy = exact_block<int32_t>(Ho), *sx = exact_block<int32_t>(Wo);
    uint8_t *wy = exact_block<uint8_t>((size_t)Ho * ay.T), *wx = exact_block<uint8_t>((size_t)Wo * ax.T);
    uint8_t* zw = zero ? exact_block<uint8_t>((size_t)Ho * Wo) : nullptr;
    for (long j = 0; j < Ho; ++j) { sy[j] = (int32_t)rule_start(j, p, q); for (int t = 0; t < ay.T; ++t) wy[j * ay.T + t] = (uint8_t)rule_weight(j, t, p, q); }
    for (long j = 0; j < Wo; ++j) { sx[j] = (int32_t)rule_start(j, p, q); for (int t = 0; t < ax.T; ++t) wx[j * ax.T + t] = (uint8_t)rule_weight(j, t, p, q); }
    if (zw) for (long i = 0; i < (long)Ho * Wo; ++i) zw[i] = (uint8_t)((rnd() % 4 != 0) * 7);

    SceneScaleParams P;
    P.src = src; P.dst = dst; P.zero_where = zw; P.sy = sy; P.wy = wy; P.sx = sx; P.wx = wx;
    P.H = H; P.W = W; P.Ho = Ho; P.Wo = Wo; P.C = C; P.Ty = ay.T; P.Tx = ax.T; P.Dy = ay.D; P.Dx = ax.D; P.mode = mode;
    P.magic = scale_magic(ay.D * ax.D);
    const int blocks[] = {64, 48, 32, 24, 16, 12, 8, 6, 4, 3, 2, 1};
    for (int b : blocks) {                               // the host's plan (resample.block_plan): the largest block inside 32 KiB
        P.bh = P.bw = b;
        P.win_h = (int)ceil_div((long)(b - 1) * q, p) + ay.T + 1; P.win_w = (int)ceil_div((long)(b - 1) * q, p) + ax.T + 1;
        if (scale_lds_bytes(P) <= 32 * 1024) break;
    }
    if (form == 1) P.win_h = P.win_w = 0;
    if (form == 2) { P.bh = 5; P.bw = 7; P.win_h = P.win_w = 1; }
    if (!scale_params_ok(P)) { printf("parameters refused\n"); exit(2); }
    const long lds_n = scale_lds_bytes(P);
    void* lb = nullptr;
    if (posix_memalign(&lb, 16, lds_n ? lds_n : 16)) { printf("allocation failed\n"); exit(2); }
    uint8_t* lds = static_cast<uint8_t*>(lb);

    const long n_blocks = scale_blocks(P);
    long lds_blocks = 0;
    for (long b = n_blocks - 1; b >= 0; --b) {           // any order: the blocks are independent
        memset(lds, 0xEE, lds_n);
        const ScaleBlock k = scale_block(P, b);
        if (k.lds) {
            ++lds_blocks;
            for (long i = scale_stage_items(P, k) - 1; i >= 0; --i) scale_stage_item(P, k, lds, i);
            for (long i = scale_row_items(P, k) - 1; i >= 0; --i) scale_row_item(P, k, lds, i);
        }
        for (long i = scale_out_items(P, k) - 1; i >= 0; --i) scale_out_item(P, k, lds, i);
    }
    // the plan's window holds every block; the direct form and the validity rule never stage (a one-pixel window may, for a block of one tap)
    if ((form == 0 && mode == SCALE_SUM && lds_blocks != n_blocks) || ((form == 1 || mode == SCALE_VALID) && lds_blocks != 0)) {
        printf("%ld of %ld blocks took the LDS form (form %d mode %d %dx%d %d/%d)\n", lds_blocks, n_blocks, form, mode, H, W, p, q); exit(1);
    }

    const long DD = (long)ay.D * ax.D;
    for (long Y = 0; Y < Ho; ++Y)
        for (long X = 0; X < Wo; ++X)
            for (int ch = 0; ch < C; ++ch) {
                long acc = 0, bad = 0, wsum = 0;
                for (int t = 0; t < ay.T; ++t)
                    for (int u = 0; u < ax.T; ++u) {
                        const long w = rule_weight(Y, t, p, q) * rule_weight(X, u, p, q);
                        const long v = src[(clampl(rule_start(Y, p, q) + t, 0, H - 1) * W + clampl(rule_start(X, p, q) + u, 0, W - 1)) * C + ch];
                        acc += w * v; wsum += w;
                        if (w != 0 && v == 0) bad = 1;
                    }
                if (wsum != DD) { printf("weights of (%ld, %ld) sum to %ld, not %ld\n", Y, X, wsum, DD); exit(1); }
                long want = mode == SCALE_VALID ? 1 - bad : (acc + DD / 2) / DD;
                if (zw && zw[Y * Wo + X] == 0) want = 0;
                if (dst[(Y * Wo + X) * C + ch] != want) {
                    printf("wrong byte at (%ld, %ld, %d): %d, want %ld (%dx%dx%d %d/%d -> %dx%d mode %d form %d offsets %d %d)\n", Y, X, ch,
                           dst[(Y * Wo + X) * C + ch], want, H, W, C, p, q, Ho, Wo, mode, form, src_off, dst_off);
                    exit(1);
                }
            }
    for (size_t i = 0; i < guard + dst_off; ++i)
        if (dblock[i] != 0xA5) { printf("guard byte %zu in front of dst written\n", i); exit(1); }
    if (memcmp(src_before.data(), src, src_bytes) != 0) { printf("the source was written\n"); exit(1); }
    free(sblock); free(dblock); free(lds); free(sy); free(sx); free(wy); free(wx); free(zw);
    return n_blocks;
}

int main() {
    // the division by multiplication: monotone in n, so the multiples of DD and their predecessors decide every n up to 256 DD
    for (int DD = 1; DD <= SCALE_MAX_D * SCALE_MAX_D; ++DD)
        for (uint32_t k = 1; k <= 256; ++k) {
            const uint64_t m = scale_magic(DD); const uint32_t half = (uint32_t)(DD >> 1);
            if (scale_round_div(k * DD - half, DD, m) != k || scale_round_div(k * DD - 1 - half, DD, m) != k - 1) { printf("division by %d is not exact at %u\n", DD, k); return 1; }
        }
    const int scales[][2] = {{1, 8}, {2, 3}, {3, 2}, {4, 1}};
    const int shapes[][2] = {{1, 64}, {64, 1}, {37, 53}, {3, 6000}};
    long cases = 0, blocks = 0;
    for (auto& s : scales)
        for (auto& hw : shapes)
            for (int off = 0; off < 4; ++off) {
                const int p = s[0], q = s[1], H = hw[0], W = hw[1];
                const int Ho = (int)ceil_div((long)H * p, q), Wo = (int)ceil_div((long)W * p, q);
                for (int C : {3, 1})
                    for (int form = 0; form < 3; ++form) {
                        if (form != 0 && (long)Ho * Wo > 40000 && off != 1) continue;       // the gathers of a large output once
                        blocks += run_case(H, W, C, p, q, Ho, Wo, SCALE_SUM, false, form, off, (off + C) & 3); ++cases;
                    }
                blocks += run_case(H, W, 1, p, q, Ho, Wo, SCALE_VALID, false, 0, off, 3 - off); ++cases;
                // the way back: the resampled size by q/p to exactly H x W, with and without zero_where
                blocks += run_case(Ho, Wo, 1, q, p, H, W, SCALE_SUM, off & 1, 0, off, off); ++cases;
                blocks += run_case(Ho, Wo, 1, q, p, H, W, SCALE_SUM, !(off & 1), 1, 3 - off, off); ++cases;
            }
    printf("scene scale OK: %ld cases, %ld blocks\n", cases, blocks);
    return 0;
}
