// The addressing of the valid and the apply kernel of SCENE_FLOAT (sam_road_amd/csrc/scene_float_piece.hpp) on the CPU: every work item of
// a launch runs through the kernels' own per-item code, in a stand-alone program built with the address and undefined-behaviour
// sanitizers (tests/test_scene_float_host.py builds and runs it).  The source, the masks, the tables and the outputs are heap blocks that
// END where the data ends, at every misalignment of the outputs' start, so a byte read past an input or written past an output ends the
// program; the bytes in front of an output are guards that must come back unchanged, and the outputs must equal a plain loop restated
// here on floats' bit patterns — a read from a wrong element shows there.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "scene_float_piece.hpp"

using namespace srh;

static uint32_t rng_state = 2463534242u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 4; }

static const uint32_t SPECIAL[] = {0x7fc00000u, 0xffc00001u, 0x7f800000u, 0xff800000u, 0x00000000u, 0x80000000u, 0x00000001u, 0x80000001u,
                                   0x007fffffu, 0xc61c3c00u /* -9999 */, 0x3f800000u, 0xbf800000u};

static uint32_t plain_key(uint32_t b) {
    if (b == 0x80000000u) b = 0u;
    return (b >> 31) ? ~b : (b | 0x80000000u);
}

static uint8_t* block(size_t off, size_t bytes, uint8_t** base) {
    void* m = nullptr;
    if (posix_memalign(&m, 16, off + bytes)) { printf("allocation failed\n"); exit(2); }
    *base = static_cast<uint8_t*>(m);
    memset(*base, 0xA5, off + bytes);
    return *base + off;
}

static long run_case(long n, int C, const int sel[3], int src_off, int dst_off, int mask_off, bool with_in, int n_nodata, int log) {
    uint8_t *sb, *db, *vb, *ib, *ob;
    uint32_t* src = reinterpret_cast<uint32_t*>(block(src_off, (size_t)n * C * 4, &sb));
    uint8_t* dst = block(dst_off, (size_t)3 * n, &db);
    uint8_t* vout = block(mask_off, (size_t)n, &vb);
    uint8_t* vin = block((mask_off + 5) & 15, (size_t)n, &ib);
    uint8_t* vapply = block((mask_off + 9) & 15, (size_t)n, &ob);
    uint32_t* tab = static_cast<uint32_t*>(malloc(3 * 256 * 4));
    if (!tab) { printf("allocation failed\n"); exit(2); }
    if ((reinterpret_cast<uintptr_t>(dst) & 15) != (uintptr_t)dst_off || (reinterpret_cast<uintptr_t>(vout) & 15) != (uintptr_t)mask_off) { printf("bad placement\n"); exit(2); }
    for (long i = 0; i < n * C; ++i) {
        const uint32_t r = rnd();
        src[i] = (r & 7u) == 0u ? SPECIAL[(r >> 3) % (sizeof(SPECIAL) / 4)] : (r << 4) ^ rnd();
    }
    for (long i = 0; i < n; ++i) { vin[i] = (uint8_t)((rnd() & 3u) ? 1 + (rnd() & 0x7f) : 0); vapply[i] = (uint8_t)((rnd() & 3u) ? 1 + (rnd() & 0x7f) : 0); }
    for (int b = 0; b < 3; ++b) {
        uint32_t* t = tab + b * 256;
        for (int j = 0; j < 255; ++j) t[j] = (j & 7) == 0 && n > 1 ? plain_key(src[(rnd() % n) * C + sel[b]]) : (rnd() << 4) ^ rnd();   // values of the scene among them
        std::sort(t, t + 255);
        t[255] = 0xffffffffu;
    }
    std::vector<uint32_t> src_before(src, src + n * C);

    SceneFloatParams p;
    p.src = src; p.n = n; p.C = C; p.valid_in = with_in ? vin : nullptr; p.valid_out = vout; p.valid = vapply; p.thr = tab; p.dst = dst;
    p.n_nodata = n_nodata; p.log = log;
    const uint32_t nd[4] = {plain_key(0xc61c3c00u), plain_key(0u), plain_key(0x3f800000u), plain_key(0x00000001u)};
    for (int j = 0; j < n_nodata; ++j) p.nodata[j] = nd[j];
    for (int b = 0; b < 3; ++b) p.sel[b] = sel[b];
    if (!float_params_ok(p)) { printf("parameters refused\n"); exit(2); }
    const long nv = float_valid_pieces(p), na = float_apply_pieces(p);
    for (long pc = nv - 1; pc >= 0; --pc) float_valid_piece(p, pc);              // any order: the pieces are independent
    for (long pc = na - 1; pc >= 0; --pc) float_apply_piece(p, tab, pc);
    for (long i = 0; i < n; ++i) {
        bool ok = !with_in || vin[i] != 0;
        for (int b = 0; b < 3; ++b) {
            const uint32_t bits = src[i * C + sel[b]], k = plain_key(bits);
            if (((bits >> 23) & 0xffu) == 0xffu) ok = false;
            for (int j = 0; j < n_nodata; ++j) if (k == nd[j]) ok = false;
            if (log && k <= 0x80000000u) ok = false;
            int level = 0;
            for (int j = 0; j < 255; ++j) level += tab[b * 256 + j] <= k;
            if (dst[3 * i + b] != (vapply[i] ? level : 0)) {
                printf("wrong level: n %ld C %d pixel %ld channel %d dst_off %d\n", n, C, i, b, dst_off);
                exit(1);
            }
        }
        if (vout[i] != (ok ? 1 : 0)) { printf("wrong validity: n %ld C %d pixel %ld mask_off %d\n", n, C, i, mask_off); exit(1); }
    }
    for (int k = 0; k < dst_off; ++k) if (db[k] != 0xA5) { printf("guard byte %d in front of dst written (n %ld C %d)\n", k, n, C); exit(1); }
    for (int k = 0; k < mask_off; ++k) if (vb[k] != 0xA5) { printf("guard byte %d in front of valid_out written (n %ld C %d)\n", k, n, C); exit(1); }
    if (memcmp(src_before.data(), src, (size_t)n * C * 4) != 0) { printf("the source was written\n"); exit(1); }
    free(sb); free(db); free(vb); free(ib); free(ob); free(tab);
    return nv + na;
}

int main() {
    const int Cs[] = {1, 3, 16};
    const long ns[] = {1, 5, 6, 17, 6000 * 3};
    const int src_offs[] = {0, 4, 12};
    long cases = 0, pieces = 0;
    for (int C : Cs)
        for (long n : ns)
            for (int off = 0; off < 16; ++off) {
                const int perm[3] = {C - 1, 0, C / 2}, grey[3] = {C - 1, C - 1, C - 1};
                pieces += run_case(n, C, (off & 1) ? grey : perm, src_offs[off % 3], off, (off * 7 + 3) & 15, (off & 2) != 0, off & 3 ? (off % 5) : 0, (off >> 2) & 1);
                ++cases;
            }
    // the binary search against a count, at and around every table entry
    uint32_t t[256];
    for (int j = 0; j < 255; ++j) t[j] = (uint32_t)(j / 3) * 1000u + 7u;        // repeats: a collapsed table
    t[255] = 0xffffffffu;
    for (int j = 0; j < 255; ++j)
        for (int d = -1; d <= 1; ++d) {
            const uint32_t k = t[j] + (uint32_t)d;
            uint32_t want = 0;
            for (int i = 0; i < 255; ++i) want += t[i] <= k;
            if (float_level(t, k) != want) { printf("binary search\n"); return 1; }
        }
    if (float_level(t, 0u) != 0u || float_level(t, 0xffffffffu) != 255u) { printf("binary search at the ends\n"); return 1; }
    // the key: -0.0 is +0.0, order of negatives, denormals
    if (float_key(0x80000000u) != float_key(0u) || !(float_key(0x80000001u) < float_key(0u)) || !(float_key(0u) < float_key(1u)) ||
        !(float_key(0xbf800000u) < float_key(0x80000001u)) || !(float_key(0xff800000u) < float_key(0xc61c3c00u)) || float_finite(0x7f800000u) ||
        float_finite(0xffc00000u) || !float_finite(0x7f7fffffu)) { printf("the ordered key\n"); return 1; }
    // refusals of the parameter check
    SceneFloatParams p;
    uint32_t one[16] = {0};
    p.src = one; p.n = 1; p.C = 3;
    bool ok = float_params_ok(p);
    p.C = 0; ok = ok && !float_params_ok(p);
    p.C = 17; ok = ok && !float_params_ok(p);
    p.C = 3; p.sel[1] = 3; ok = ok && !float_params_ok(p);
    p.sel[1] = -1; ok = ok && !float_params_ok(p);
    p.sel[1] = 1; p.n = 0; ok = ok && !float_params_ok(p);
    p.n = FLOAT_MAX_PIXELS + 1; ok = ok && !float_params_ok(p);
    p.n = 1; p.n_nodata = 5; ok = ok && !float_params_ok(p);
    p.n_nodata = 0; p.n_targets = 7; ok = ok && !float_params_ok(p);
    p.n_targets = 1; p.tband[0] = 3; ok = ok && !float_params_ok(p);
    p.tband[0] = 0; p.tprefix[0] = 65536u; ok = ok && !float_params_ok(p);
    p.n_targets = 0; p.src = reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(one) + 2); ok = ok && !float_params_ok(p);
    p.src = nullptr; ok = ok && !float_params_ok(p);
    if (!ok) { printf("the parameter check accepts or refuses wrongly\n"); return 1; }
    // the piece counts of the largest launch, in 64-bit arithmetic
    p = SceneFloatParams(); p.n = FLOAT_MAX_PIXELS; p.dst = reinterpret_cast<uint8_t*>((uintptr_t)0x1000F); p.valid_out = p.dst;
    if (float_apply_pieces(p) != (15L + 3L * 2147483647L + 15L) / 16 || float_valid_pieces(p) != (15L + 2147483647L + 15L) / 16) { printf("piece count of the largest launch\n"); return 1; }
    printf("scene float OK: %ld cases, %ld pieces\n", cases, pieces);
    return 0;
}
