// GEOTIFF on the CPU: whole launches of the assemble kernel through its own per-thread code (csrc/geotiff_piece.hpp) —
// only the barriers and the scan across the threads are restated, as loops — against the raster the segments were encoded from by scalar
// loops, and the LZW decoder over valid, truncated, bit-flipped and over-long streams.  Every block is a heap block of its exact size, so
// under the address sanitizer a byte read or written outside one ends the program.  Built and run by tests/test_geotiff_host.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <utility>
#include <vector>

#include "geotiff_piece.hpp"

using namespace srh;

static std::mt19937 rng(12345);

static uint8_t* block(size_t bytes, int fill) {
    void* p = nullptr;
    if (posix_memalign(&p, 16, bytes ? bytes : 1) != 0) { std::printf("out of memory\n"); std::exit(2); }
    std::memset(p, fill, bytes ? bytes : 1);
    return static_cast<uint8_t*>(p);
}

// ---- the launch, thread by thread -------------------------------------------------------------------------------------------------------
static void run_launch(const TiffParams& p) {
    const long items = (long)p.n_seg * p.max_rows;
    std::vector<uint32_t> acc(TIF_THREADS);
    for (long it = 0; it < items; ++it) {
        const TifRow row = tif_row(p, it);
        if (!row.live) continue;
        uint32_t* buf = reinterpret_cast<uint32_t*>(block(sizeof(uint32_t) * TIF_LDS_WORDS, 0xEE));
        uint32_t carry[TIF_MAX_BANDS] = {0};
        const int E = tif_chunk_elems(row.S);
        for (long k0 = 0; k0 < row.n; k0 += E) {
            const int ne = (int)(row.n - k0 < E ? row.n - k0 : E);
            for (int t = 0; t < TIF_THREADS; ++t)
                for (int i = t; i < ne; i += TIF_THREADS) buf[tif_pad(i)] = tif_load(p, row, k0 + i);
            if (p.predictor != 1) {
                const int npix = ne / row.S;
                for (int c = 0; c < row.S; ++c) {
                    for (int t = 0; t < TIF_THREADS; ++t) acc[t] = tif_local_sum(buf, row.S, t, c, npix);
                    uint32_t run = carry[c];
                    for (int t = 0; t < TIF_THREADS; ++t) { tif_local_apply(buf, row.S, t, c, npix, run); run += acc[t]; }
                    carry[c] = run;
                }
            }
            for (int t = 0; t < TIF_THREADS; ++t) tif_store(p, row, k0, ne, t, buf);
        }
        std::free(buf);
    }
}

// ---- a raster -> the segments a TIFF would hold, by scalar loops ------------------------------------------------------------------------
struct Case { int H, W, C, B, pred, planar, be, tile_h, tile_w, rps; };

static void put(uint8_t* d, uint32_t v, int B, int be) {
    for (int k = 0; k < B; ++k) d[k] = (uint8_t)(v >> (8 * (be ? B - 1 - k : k)));
}

static long run_case(const Case& q) {
    const size_t px = (size_t)q.H * q.W * q.C;
    uint8_t* raster = block(px * q.B, 0);
    for (size_t i = 0; i < px * q.B; ++i) raster[i] = (uint8_t)rng();
    auto sample = [&](long y, long x, int ch) { uint32_t v = 0; std::memcpy(&v, raster + (((size_t)y * q.W + x) * q.C + ch) * q.B, q.B); return v; };
    std::vector<int64_t> table;
    std::vector<std::vector<uint8_t>> segs;
    const int planes = q.planar ? q.C : 1, S = q.planar ? 1 : q.C;
    for (int band = 0; band < planes; ++band) {
        const int sh = q.tile_h ? q.tile_h : q.rps, sw = q.tile_h ? q.tile_w : q.W;
        for (int r0 = 0; r0 < q.H; r0 += sh)
            for (int c0 = 0; c0 < q.W; c0 += sw) {
                const int rows = q.tile_h ? sh : (sh < q.H - r0 ? sh : q.H - r0), cols = sw;
                std::vector<uint8_t> seg((size_t)rows * cols * S * q.B);
                std::vector<uint32_t> v((size_t)cols * S);
                for (int r = 0; r < rows; ++r) {
                    for (int x = 0; x < cols; ++x)
                        for (int ch = 0; ch < S; ++ch)
                            v[(size_t)x * S + ch] = (r0 + r < q.H && c0 + x < q.W) ? sample(r0 + r, c0 + x, q.planar ? band : ch) : 0xA5A5A5A5u >> (8 * (4 - q.B));
                    uint8_t* d = seg.data() + (size_t)r * cols * S * q.B;
                    if (q.pred == 3) {
                        std::vector<uint8_t> pl((size_t)cols * S * 4);
                        for (size_t j = 0; j < v.size(); ++j)
                            for (int k = 0; k < 4; ++k) pl[(size_t)k * v.size() + j] = (uint8_t)(v[j] >> (8 * (3 - k)));
                        for (size_t i = 0; i < pl.size(); ++i) d[i] = (uint8_t)(pl[i] - (i >= (size_t)S ? pl[i - S] : 0));
                    } else {
                        for (size_t j = 0; j < v.size(); ++j) put(d + j * q.B, q.pred == 2 && j >= (size_t)S ? v[j] - v[j - S] : v[j], q.B, q.be);
                    }
                }
                table.insert(table.end(), {0, (int64_t)seg.size(), r0, c0, rows, cols, q.planar ? band : -1});
                segs.push_back(std::move(seg));
            }
    }
    size_t pos = 0;
    for (size_t k = 0; k < segs.size(); ++k) {
        pos = (pos + TIF_ALIGN - 1) / TIF_ALIGN * TIF_ALIGN;
        table[k * TIF_TABLE_COLS] = (int64_t)pos;
        pos += segs[k].size();
    }
    uint8_t* flat = block(pos, 0x33);                              // exact: the last segment ends the block
    for (size_t k = 0; k < segs.size(); ++k) std::memcpy(flat + table[k * TIF_TABLE_COLS], segs[k].data(), segs[k].size());
    int64_t* tab = reinterpret_cast<int64_t*>(block(table.size() * 8, 0));
    std::memcpy(tab, table.data(), table.size() * 8);
    uint8_t* out = block(px * q.B, 0xCD);
    long max_rows = 0;
    long bad = 0;
    if (!tif_table_ok(tab, (long)segs.size(), (long)pos, q.H, q.W, q.C, q.B, &max_rows)) bad = 1;
    TiffParams p;
    p.flat = flat; p.table = tab; p.n_seg = (int)segs.size(); p.max_rows = (int)max_rows; p.out = out;
    p.H = q.H; p.W = q.W; p.C = q.C; p.B = q.B; p.predictor = q.pred; p.big_endian = q.be;
    if (!bad && !tif_params_ok(p)) bad = 1;
    if (!bad) {
        run_launch(p);
        bad = std::memcmp(out, raster, px * q.B) != 0;
    }
    if (bad) std::printf("MISMATCH H %d W %d C %d B %d pred %d planar %d be %d tile %dx%d rps %d\n", q.H, q.W, q.C, q.B, q.pred, q.planar, q.be, q.tile_h, q.tile_w, q.rps);
    std::free(raster); std::free(flat); std::free(tab); std::free(out);
    return bad;
}

// ---- LZW ------------------------------------------------------------------------------------------------------------------------------------
static std::vector<uint8_t> lzw_encode(const std::vector<uint8_t>& data) {
    std::vector<uint8_t> out;
    uint64_t acc = 0;
    int nacc = 0, width = 9, next = 258;
    std::map<std::pair<int, int>, int> table;
    auto emit = [&](int code) {
        acc = (acc << width) | (uint64_t)code; nacc += width;
        while (nacc >= 8) { out.push_back((uint8_t)(acc >> (nacc - 8))); nacc -= 8; }
    };
    auto made = [&] {
        ++next;
        if (next == 4094) { emit(256); width = 9; next = 258; table.clear(); }
        else if (next > (1 << width) - 1) ++width;
    };
    emit(256);
    int w = -1;
    for (uint8_t b : data) {
        if (w < 0) { w = b; continue; }
        auto it = table.find({w, b});
        if (it != table.end()) { w = it->second; continue; }
        emit(w);
        table[{w, b}] = next;
        made();
        w = b;
    }
    if (w >= 0) { emit(w); made(); }
    emit(257);
    if (nacc) out.push_back((uint8_t)(acc << (8 - nacc)));
    return out;
}

// Decodes `stream` into an exact block of `expected` bytes: the status, and whether the block then equals want[0 .. expected).
static int decode(const std::vector<uint8_t>& stream, const std::vector<uint8_t>& want, long expected, bool* right) {
    uint8_t* in = block(stream.size(), 0);
    if (!stream.empty()) std::memcpy(in, stream.data(), stream.size());
    uint8_t* out = block((size_t)expected, 0xCD);
    const int rc = tif_lzw_decode(in, (long)stream.size(), out, expected);
    *right = expected <= (long)want.size() && std::memcmp(out, want.data(), (size_t)expected) == 0;
    std::free(in); std::free(out);
    return rc;
}

static long run_lzw() {
    long bad = 0;
    std::vector<std::vector<uint8_t>> datas;
    std::vector<uint8_t> d;
    for (int i = 0; i < 30000; ++i) d.push_back((uint8_t)rng());                      // incompressible: every width and several table resets
    datas.push_back(d);
    d.assign(50000, 7); datas.push_back(d);                                           // one long run: the code == next case over and over
    d.clear(); for (int i = 0; i < 20000; ++i) d.push_back((uint8_t)((i / 3) % 11 + (rng() % 2))); datas.push_back(d);
    d.assign(1, 42); datas.push_back(d);
    d.clear(); for (int i = 0; i < 700; ++i) d.push_back((uint8_t)(rng() % 4)); datas.push_back(d);
    for (const auto& data : datas) {
        const std::vector<uint8_t> s = lzw_encode(data);
        bool right = false;
        if (decode(s, data, (long)data.size(), &right) != 0 || !right) { std::printf("LZW: a valid stream of %zu bytes fails\n", data.size()); ++bad; }
        // over-long: the stream holds more than is asked for; shorter than asked: an error
        for (long cut : {1L, 2L, 17L, (long)data.size() / 2}) {
            if (cut >= (long)data.size()) continue;
            const int rc = decode(s, data, (long)data.size() - cut, &right);
            if (rc == 0 && !right) { std::printf("LZW: over-long stream accepted with wrong bytes\n"); ++bad; }
        }
        if (decode(s, data, (long)data.size() + 5, &right) == 0) { std::printf("LZW: a short stream accepted\n"); ++bad; }
        // truncated: a prefix of the stream
        const size_t step = s.size() > 400 ? s.size() / 200 : 1;
        for (size_t n = 0; n < s.size(); n += step) {
            const std::vector<uint8_t> pre(s.begin(), s.begin() + (long)n);
            const int rc = decode(pre, data, (long)data.size(), &right);
            if (rc == 0 && !right) { std::printf("LZW: truncated stream accepted with wrong bytes\n"); ++bad; }
        }
        // bit flips: no checksum guards an LZW stream, so a flipped literal decodes "successfully" to other bytes; what must hold is
        // that the call returns, with a status, having touched nothing outside its blocks
        for (int k = 0; k < 300; ++k) {
            std::vector<uint8_t> f = s;
            f[rng() % f.size()] ^= (uint8_t)(1u << (rng() % 8));
            if (k % 3 == 0) f[rng() % f.size()] = (uint8_t)rng();
            (void)decode(f, data, (long)data.size(), &right);
        }
        // garbage
        for (int k = 0; k < 50; ++k) {
            std::vector<uint8_t> f(1 + rng() % 300);
            for (auto& b : f) b = (uint8_t)rng();
            (void)decode(f, data, (long)(rng() % 2000), &right);
        }
    }
    return bad;
}

int main() {
    long bad = 0, cases = 0;
    const int small[][2] = {{1, 1}, {1, 70}, {70, 1}, {37, 53}, {16, 16}};
    const int wide[][2] = {{3, TIF_CHUNK - 1}, {2, TIF_CHUNK + 1}, {2, 2 * TIF_CHUNK + 3}};
    const int formats[][2] = {{1, 1}, {1, 2}, {2, 1}, {2, 2}, {4, 1}, {4, 3}};
    for (int C : {1, 3, 4, 16})
        for (const auto& f : formats)
            for (int planar = 0; planar < 2; ++planar)
                for (int be = 0; be < 2; ++be) {
                    for (const auto& s : small) {
                        for (int rps : {1, 5, s[0]}) { bad += run_case({s[0], s[1], C, f[0], f[1], planar, be, 0, 0, rps}); ++cases; }
                        bad += run_case({s[0], s[1], C, f[0], f[1], planar, be, 16, 16, 0});
                        bad += run_case({s[0], s[1], C, f[0], f[1], planar, be, 32, 16, 0});
                        cases += 2;
                    }
                    for (const auto& s : wide) {
                        if ((C == 4 || C == 16) && (planar || be) && s[1] > TIF_CHUNK + 1) continue;      // the widest once per band count
                        bad += run_case({s[0], s[1], C, f[0], f[1], planar, be, 0, 0, s[0]});
                        ++cases;
                    }
                }
    bad += run_case({40, 1100, 3, 1, 2, 0, 0, 32, 512, 0});                        // wide tiles, clipped on both edges
    bad += run_case({40, 1100, 4, 2, 2, 1, 1, 32, 512, 0});
    bad += run_case({33, 600, 3, 4, 3, 0, 0, 16, 512, 0});
    cases += 3;
    bad += run_lzw();
    if (bad) { std::printf("%ld FAILURES\n", bad); return 1; }
    std::printf("geotiff OK (%ld launches)\n", cases);
    return 0;
}
