// The apply kernel's addressing (sam_road_amd/csrc/scene_bands_piece.hpp) on the CPU: every work item of a launch runs through the
// kernel's own per-item code, in a stand-alone program built with the address and undefined-behaviour sanitizers
// (tests/test_scene_bands_host.py builds and runs it).  The source, the tables and the destination are heap blocks of their exact sizes
// (the source and destination placed so that they END at the block's end, at every misalignment of their start), so a byte read past
// src or the tables, or written past dst, ends the program; the bytes in front of dst are guards that must come back unchanged, and the
// output must equal lut[b][src[i][sel[b]]] restated here — a read from a wrong element shows there.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "scene_bands_piece.hpp"

using namespace srh;

static uint32_t rng_state = 12345u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

template <class T>
static long run_case(long n, int C, const int sel[3], int src_off, int dst_off) {
    constexpr long levels = sizeof(T) == 1 ? 256 : 65536;
    const size_t src_bytes = (size_t)n * C * sizeof(T), dst_bytes = (size_t)3 * n;
    // blocks that end where the data ends and start 16-byte aligned: the data's address has exactly the wanted misalignment
    const size_t src_pad = 0, dst_pad = 0;
    void *sb = nullptr, *db = nullptr;
    if (posix_memalign(&sb, 16, src_off + src_bytes) || posix_memalign(&db, 16, dst_off + dst_bytes)) { printf("allocation failed\n"); exit(2); }
    uint8_t *sblock = static_cast<uint8_t*>(sb), *dblock = static_cast<uint8_t*>(db);
    uint8_t* lut = static_cast<uint8_t*>(malloc((size_t)3 * levels));
    if (!sblock || !dblock || !lut) { printf("allocation failed\n"); exit(2); }
    T* src = reinterpret_cast<T*>(sblock + src_pad + src_off);
    uint8_t* dst = dblock + dst_pad + dst_off;
    if ((reinterpret_cast<uintptr_t>(src) & 15) != (uintptr_t)src_off || (reinterpret_cast<uintptr_t>(dst) & 15) != (uintptr_t)dst_off) { printf("bad placement\n"); exit(2); }
    for (long i = 0; i < n * C; ++i) src[i] = (T)rnd();
    for (long i = 0; i < 3 * levels; ++i) lut[i] = (uint8_t)rnd();
    memset(dblock, 0xA5, dst_pad + dst_off + dst_bytes);
    std::vector<uint8_t> src_before(sblock + src_pad + src_off, sblock + src_pad + src_off + src_bytes);

    SceneBandsParams p;
    p.src = src; p.lut = lut; p.dst = dst; p.n = n; p.C = C; p.wide = sizeof(T) == 2;
    for (int b = 0; b < 3; ++b) p.sel[b] = sel[b];
    if (!bands_params_ok(p)) { printf("parameters refused\n"); exit(2); }
    const long n_pieces = bands_n_pieces(p);
    for (long pc = n_pieces - 1; pc >= 0; --pc) bands_piece<T>(p, pc);          // any order: the pieces are independent
    for (long i = 0; i < n; ++i)
        for (int b = 0; b < 3; ++b)
            if (dst[3 * i + b] != lut[b * levels + (long)src[i * C + sel[b]]]) {
                printf("wrong byte: n %ld C %d pixel %ld channel %d src_off %d dst_off %d\n", n, C, i, b, src_off, dst_off);
                exit(1);
            }
    for (size_t k = 0; k < dst_pad + dst_off; ++k)
        if (dblock[k] != 0xA5) { printf("guard byte %zu in front of dst written (n %ld C %d dst_off %d)\n", k, n, C, dst_off); exit(1); }
    if (memcmp(src_before.data(), src, src_bytes) != 0) { printf("the source was written\n"); exit(1); }
    free(sblock); free(dblock); free(lut);
    return n_pieces;
}

int main() {
    const int Cs[] = {1, 3, 4, 5, 16};
    const long ns[] = {1, 2, 5, 6, 7, 11, 16, 17, 100, 1961, 4099};
    long cases = 0, pieces = 0;
    for (int C : Cs)
        for (long n : ns)
            for (int dst_off = 0; dst_off < 16; ++dst_off)
                for (int so = 0; so < 4; ++so) {
                    const int perm[3] = {C - 1, 0, C / 2}, grey[3] = {C - 1, C - 1, C - 1};
                    const int* sel = (so & 1) ? grey : perm;
                    pieces += run_case<uint8_t>(n, C, sel, (so * 5 + 1) & 15, dst_off);      // any byte address
                    pieces += run_case<uint16_t>(n, C, sel, (so * 6 + 2) & 14, dst_off);     // any 2-byte-aligned address
                    cases += 2;
                }
    // refusals of the parameter check
    SceneBandsParams p;
    uint16_t one[16] = {0};
    p.src = one; p.n = 1; p.C = 3;
    bool ok = bands_params_ok(p);
    p.C = 0; ok = ok && !bands_params_ok(p);
    p.C = 17; ok = ok && !bands_params_ok(p);
    p.C = 3; p.sel[1] = 3; ok = ok && !bands_params_ok(p);
    p.sel[1] = -1; ok = ok && !bands_params_ok(p);
    p.sel[1] = 1; p.n = 0; ok = ok && !bands_params_ok(p);
    p.n = BANDS_MAX_PIXELS + 1; ok = ok && !bands_params_ok(p);
    p.n = 1; p.wide = 1; p.src = reinterpret_cast<const uint8_t*>(one) + 1; ok = ok && !bands_params_ok(p);
    p.src = nullptr; ok = ok && !bands_params_ok(p);
    if (!ok) { printf("the parameter check accepts or refuses wrongly\n"); return 1; }
    // the piece count of the largest launch: 3 (2^31 - 1) bytes at misalignment 15, in 64-bit arithmetic
    p = SceneBandsParams(); p.n = BANDS_MAX_PIXELS; p.dst = reinterpret_cast<uint8_t*>((uintptr_t)0x1000F);
    if (bands_n_pieces(p) != (15L + 3L * 2147483647L + 15L) / 16) { printf("piece count of the largest launch\n"); return 1; }
    printf("scene bands OK: %ld cases, %ld pieces\n", cases, pieces);
    return 0;
}
