// CPU check of the packed weight layout (built and run by tests/test_pack_layout.py; no HIP, no GPU).  Packs the smallest model at
// which each layout can go wrong (ViT-B width, one global block, PATCH_SIZE 128) from LCG weights and compares the arena image with
// the definitions of the layouts, written out here independently of the packer's writers.
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "pack_host.hpp"

using namespace srh;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++g_fail <= 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

struct Tensors {
    std::vector<std::pair<std::string, size_t>> asked;
    std::vector<std::vector<float>> data;
    std::vector<srh_named_tensor> list;
    const float* operator[](const std::string& name) const {
        for (size_t i = 0; i < asked.size(); ++i) if (asked[i].first == name) return data[i].data();
        printf("the packer never asked for %s\n", name.c_str()); exit(2);
    }
};

static srh_weights* new_weights(int tv, int sam) {
    srh_weights* w = new srh_weights();
    w->cfg = srh_model_cfg{768, 1, 12, 128, 1, {0}, 14, tv, sam};
    w->S = 8; w->D = 768; w->heads = 12; w->hd = 64;
    return w;
}
// every pointer of *w -> into pk's own host image
static void fix_up(Packer& pk) { for (auto& f : pk.fix) *f.first = pk.host.data() + f.second; }

// half (r, k) of a matrix stored as 16 x 32 A fragments, `frag` = index of the fragment of row tile r / 16 and k block k / 32.  Lane l =
// (row i = l & 15, k group g = l >> 4) holds halves j = 0..7: natural k = 32 kb + 8 g + j, permuted k = 32 kb + 16 (j >> 2) + 4 g + (j & 3)
static f16 frag_at(const char* frags, size_t frag, int r, int k, bool perm) {
    const int kk = k % 32;
    const int g = perm ? (kk % 16) / 4 : kk / 8, j = perm ? 4 * (kk / 16) + kk % 4 : kk % 8;
    return reinterpret_cast<const f16*>(frags + frag * 1024)[((g * 16 + r % 16) * 8) + j];
}
// ConvTranspose2d weight [cin][cout][2][2] as the GEMM weight [n = (ky * 2 + kx) * cout + co][ci]
static float convt_w(const float* src, int cout, int n, int ci) {
    const int co = n % cout, ky = n / cout / 2, kx = n / cout % 2;
    return src[((ci * cout + co) * 2 + ky) * 2 + kx];
}

static void check_config(int tv, int sam) {
    printf("toponet_version %d, use_sam_decoder %d\n", tv, sam);
    // ---- layout pass: what it asks for, how it lays the arena out
    Tensors t;
    srh_weights* wl = new_weights(tv, sam);
    Packer lay;
    lay.layout_only = true; lay.asked = &t.asked;
    pack_model(lay, wl, nullptr, 0);
    CHECK(lay.missing.empty(), "layout pass reports %s", lay.missing.c_str());
    uint32_t seed = 12345u + tv * 7 + sam;
    for (auto& a : t.asked) {
        std::vector<float> v(a.second);
        for (float& x : v) { seed = seed * 1664525u + 1013904223u; x = (float)(int)(seed >> 8 & 0xffff) / 32768.f - 1.f; }
        t.data.push_back(std::move(v));
    }
    for (size_t i = 0; i < t.asked.size(); ++i) {
        srh_named_tensor nt{t.asked[i].first.c_str(), t.data[i].data(), 0, 1, {(int64_t)t.asked[i].second}};
        t.list.push_back(nt);
    }
    // ---- real pass: same arena size, same fix-ups in the same order; aligned, distinct, inside
    srh_weights* w = new_weights(tv, sam);
    Packer pk;
    pack_model(pk, w, t.list.data(), (int)t.list.size());
    CHECK(pk.missing.empty(), "real pass reports %s", pk.missing.c_str());
    CHECK(pk.host.size() == lay.host.size(), "arena %zu vs layout-only %zu", pk.host.size(), lay.host.size());
    CHECK(pk.fix.size() == lay.fix.size(), "fix-ups %zu vs %zu", pk.fix.size(), lay.fix.size());
    std::vector<size_t> offs;
    for (size_t i = 0; i < pk.fix.size() && i < lay.fix.size(); ++i) {
        CHECK(pk.fix[i].second == lay.fix[i].second, "fix-up %zu: offset %zu vs %zu", i, pk.fix[i].second, lay.fix[i].second);
        CHECK(pk.fix[i].second % 256 == 0 && pk.fix[i].second < pk.host.size(), "fix-up %zu: offset %zu", i, pk.fix[i].second);
        offs.push_back(pk.fix[i].second);
    }
    std::sort(offs.begin(), offs.end());
    CHECK(std::adjacent_find(offs.begin(), offs.end()) == offs.end(), "two slots share an offset");
    offs.push_back(pk.host.size());
    fix_up(pk);
    auto room = [&](const void* p) { const size_t o = (const char*)p - pk.host.data(); return *std::upper_bound(offs.begin(), offs.end(), o) - o; };
    const int nl = tv != 2 ? 3 : 0;
    CHECK(w->tp_layers == nl, "tp_layers %d", w->tp_layers);
    CHECK(room(w->patch_w) >= 768 * 768 * 2 && room(w->neck2_w) >= 256 * 2304 * 2, "patch_w / neck2_w region too small");
    CHECK(room(w->tp_stream) >= (size_t)tf_nfrag(nl) * 1024 && room(w->tp_params) >= (size_t)tf_nprm(nl) * 4, "trunk regions too small");
    if (!sam) CHECK(room(w->dec_frags) >= 336 * 1024 && room(w->dec_prm) >= 768 * 4, "decoder regions too small");

    // ---- reorders
    const float* src = t["image_encoder.patch_embed.proj.weight"];            // [D][3][16][16] -> k = ky*48 + kx*3 + ch
    for (int n = 0; n < 768; ++n)
        for (int ky = 0; ky < 16; ++ky) for (int kx = 0; kx < 16; ++kx) for (int ch = 0; ch < 3; ++ch)
            CHECK(w->patch_w[n * 768 + ky * 48 + kx * 3 + ch] == (f16)src[((n * 3 + ch) * 16 + ky) * 16 + kx], "patch_w n %d ky %d kx %d ch %d", n, ky, kx, ch);
    src = t["image_encoder.neck.2.weight"];                                    // [256][256][3][3] -> k = tap*256 + ch
    for (int n = 0; n < 256; ++n)
        for (int tap = 0; tap < 9; ++tap) for (int ch = 0; ch < 256; ++ch)
            CHECK(w->neck2_w[n * 2304 + tap * 256 + ch] == (f16)src[(n * 256 + ch) * 9 + tap], "neck2_w n %d tap %d ch %d", n, tap, ch);

    // ---- fused trunk: pair_proj [kb 10][rt 8] natural k, 258 of 320 columns; layer nl - 1's linear1 [rt 8][kb 4] permuted k
    src = t["topo_net.pair_proj.weight"];
    for (int r = 0; r < 128; ++r)
        for (int k = 0; k < 320; ++k)
            CHECK(frag_at(w->tp_stream, (k / 32) * 8 + r / 16, r, k, false) == (k < 258 ? (f16)src[r * 258 + k] : (f16)0.f), "pair_proj r %d k %d", r, k);
    if (nl) {
        src = t["topo_net.transformer_encoder.layers.2.linear1.weight"];
        for (int r = 0; r < 128; ++r)
            for (int k = 0; k < 128; ++k)
                CHECK(frag_at(w->tp_stream, 80 + 192 * 2 + 128 + (r / 16) * 4 + k / 32, r, k, true) == (f16)src[r * 128 + k], "linear1 r %d k %d", r, k);
        CHECK(w->tp_params[128 + 1280 * 2 + 1024 + 5] == t["topo_net.transformer_encoder.layers.2.norm2.weight"][5], "trunk norm2.weight");
    }
    CHECK(w->tp_params[128 + 1280 * nl + 128] == t["topo_net.output_proj.bias"][0], "output_proj.bias");

    if (!sam) {
        // ---- fused map_decoder: L0 [sub1 4][kb 8][rt 8] natural | L3 [sub2 4][kb 4][rt 4] permuted | L5 [kb 2][rt 8] permuted, GEMM row n
        struct { const char* name; int cin, cout, base, per_sub, nrt; bool perm; } L[3] = {
            {"map_decoder.0.weight", 256, 128, 0, 64, 8, false}, {"map_decoder.3.weight", 128, 64, 256, 16, 4, true}, {"map_decoder.5.weight", 64, 32, 320, 0, 8, true}};
        for (auto& l : L) {
            src = t[l.name];
            for (int n = 0; n < 4 * l.cout; ++n)
                for (int ci = 0; ci < l.cin; ++ci) {
                    const int sub = l.per_sub ? n / l.cout : 0, r = l.per_sub ? n % l.cout : n;      // L5: one block of 128 rows
                    const size_t f = l.base + sub * l.per_sub + (ci / 32) * l.nrt + r / 16;
                    CHECK(frag_at(w->dec_frags, f, r, ci, l.perm) == (f16)convt_w(src, l.cout, n, ci), "%s n %d ci %d", l.name, n, ci);
                }
        }
        src = t["map_decoder.7.weight"];                                       // f32 [8][32] at parameter 480, n = (ky*2+kx)*2 + class
        for (int n = 0; n < 8; ++n)
            for (int ci = 0; ci < 32; ++ci) CHECK(w->dec_prm[480 + n * 32 + ci] == convt_w(src, 2, n, ci), "map_decoder.7 n %d ci %d", n, ci);
        CHECK(w->dec_prm[736] == t["map_decoder.7.bias"][0] && w->dec_prm[384] == t["map_decoder.3.bias"][0], "decoder biases");
        for (int i = 738; i < 768; ++i) CHECK(w->dec_prm[i] == 0.f, "decoder parameter pad %d", i);
    } else {
        src = t["mask_decoder.output_upscaling.0.weight"];                     // ConvT(256 -> 64) as GEMM weight [256][256]
        for (int n = 0; n < 256; ++n)
            for (int ci = 0; ci < 256; ++ci) CHECK(w->sd.up0_w[n * 256 + ci] == (f16)convt_w(src, 64, n, ci), "up0_w n %d ci %d", n, ci);
    }

    // ---- error reporting: the first missing / mis-shaped name, in today's words
    for (int mode = 0; mode < 2; ++mode) {
        size_t victim = 0;                                                     // a name that is asked for once
        while (t.asked[victim].first != "image_encoder.neck.1.weight") ++victim;
        std::vector<srh_named_tensor> l2 = t.list;
        if (mode == 0) l2.erase(l2.begin() + victim); else l2[victim].shape[0] += 1;
        srh_weights* w2 = new_weights(tv, sam);
        Packer p2;
        pack_model(p2, w2, l2.data(), (int)l2.size());
        const std::string want = t.asked[victim].first + (mode ? " (shape mismatch)" : "");
        CHECK(p2.missing == want, "reported '%s', expected '%s'", p2.missing.c_str(), want.c_str());
        delete w2;
    }
    delete w; delete wl;
}

int main() {
    check_config(0, 0);      // naive decoder, 3 trunk layers
    check_config(2, 1);      // SAM decoder, no trunk layer
    if (g_fail) { printf("%d check(s) failed\n", g_fail); return 1; }
    printf("pack layout OK\n");
    return 0;
}
