// The mask-clean kernels' own per-lane code on a CPU: every (segment, lane) item of the five launches of a call is run through
// sam_road_amd/csrc/mask_clean_piece.hpp with serial stand-ins for the atomic operations, in four schedules — ascending, descending, a
// fixed stride permutation, and ascending once more with loads that may return old values — and each result is compared with a
// breadth-first flood fill written here (DESIGN.md §6k's rule).  The four results must be identical: the outcome may not depend on the schedule.  Buffer and workspaces are exact-size heap blocks, so built with
// the address sanitizer a read or write one element outside either is an error.  The foreground words that a wave gets from a ballot are
// taken per segment before the launch's items run, as on the device.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "mask_clean_piece.hpp"

using namespace srh;

struct SerialOps {
    static int load(const int32_t* p) { return *p; }
    static void store(int32_t* p, int v) { *p = v; }
    static int min(int32_t* p, int v) { const int old = *p; if (v < old) *p = v; return old; }
    static int add(int32_t* p, int v) { const int old = *p; *p = old + v; return old; }
    static int max(int32_t* p, int v) { const int old = *p; if (v > old) *p = v; return old; }
};

// The same with loads that may be OLD: a quarter of them return what the init launch stored instead of the present value, as a load on the
// device may return a value that another workgroup has replaced since.  Any value ever stored must do (mask_clean_piece.hpp's invariant);
// this drives mc_union through its retry, where the node it took for a root turns out to have been linked already.
static const int32_t* stale_now = nullptr;
static const int32_t* stale_then = nullptr;
static uint32_t stale_state = 99;
struct StaleOps : SerialOps {
    static int load(const int32_t* p) {
        stale_state = stale_state * 1664525u + 1013904223u;
        return (stale_state >> 20) % 4 == 0 ? stale_then[p - stale_now] : *p;
    }
};

struct Image { int H, W, t_on; long min_area; int t_peak; long off; };

static uint32_t rng_state = 1;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

// ---- the rule, restated: flood fill -----------------------------------------------------------------------------------------------------
static void flood_ref(uint8_t* m, const Image& im, int conn) {
    const int H = im.H, W = im.W;
    std::vector<int> label((size_t)H * W, -1), queue;
    for (int sy = 0; sy < H; ++sy)
        for (int sx = 0; sx < W; ++sx) {
            if (m[(long)sy * W + sx] < im.t_on || label[(size_t)sy * W + sx] >= 0) continue;
            queue.assign(1, sy * W + sx);
            label[(size_t)sy * W + sx] = sy * W + sx;
            int top = 0;
            for (size_t h = 0; h < queue.size(); ++h) {
                const int y = queue[h] / W, x = queue[h] % W;
                top = m[queue[h]] > top ? m[queue[h]] : top;
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx) {
                        if ((!dy && !dx) || (conn == 4 && dy && dx)) continue;
                        const int yy = y + dy, xx = x + dx;
                        if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
                        const size_t j = (size_t)yy * W + xx;
                        if (m[j] < im.t_on || label[j] >= 0) continue;
                        label[j] = sy * W + sx;
                        queue.push_back((int)j);
                    }
            }
            if ((long)queue.size() < im.min_area || top < im.t_peak)
                for (int j : queue) m[j] = 0;            // (a zeroed pixel is below t_on >= 1 or was labelled: it is not visited again)
        }
}

// ---- one call, emulated -----------------------------------------------------------------------------------------------------------------
static long item_at(long k, long n, int order) {
    if (order == 0 || order == 3) return k;
    if (order == 1) return n - 1 - k;
    long stride = 7919;                                   // a prime; coprime to n unless it divides n
    while (n % stride == 0) stride += 2;
    return (long)(((__int128)k * stride) % n);
}

static void emulate(uint8_t* buf, const std::vector<int64_t>& table, int n, int conn, long ws, int order) {
    // exact-size workspaces, filled with garbage: the init launch must define everything that is read
    int32_t* parent = (int32_t*)malloc((size_t)ws * 4), *area = (int32_t*)malloc((size_t)ws * 4), *peak = (int32_t*)malloc((size_t)ws * 4);
    memset(parent, 0x5a, (size_t)ws * 4); memset(area, 0x5a, (size_t)ws * 4); memset(peak, 0x5a, (size_t)ws * 4);
    MaskCleanParams p;
    p.buf = buf; p.table = table.data(); p.n = n; p.conn = conn; p.parent = parent; p.area = area; p.peak = peak;
    p.n_segs = mask_clean_segs(table.data(), n);
    const long items = p.n_segs * MC_SEG;
    std::vector<uint64_t> cur((size_t)p.n_segs), up((size_t)p.n_segs);
    for (int step = 0; step < 5; ++step) {
        for (long s = 0; s < p.n_segs; ++s) {             // the ballots of every wave
            const McSeg g = mc_locate(p, s);
            uint64_t c = 0, u = 0;
            for (int l = 0; l < MC_SEG; ++l) {
                c |= (uint64_t)mc_fg(g, g.y, g.x0 + l) << l;
                u |= (uint64_t)mc_fg(g, g.y - 1, g.x0 + l) << l;
            }
            cur[(size_t)s] = c; up[(size_t)s] = u;
        }
        std::vector<int32_t> then;
        if (step == 1) { then.assign(parent, parent + ws); stale_now = parent; stale_then = then.data(); }
        for (long k = 0; k < items; ++k) {
            const long it = item_at(k, items, order), s = it / MC_SEG;
            const int lane = (int)(it % MC_SEG);
            const McSeg g = mc_locate(p, s);
            if (step == 0) mc_init_lane<SerialOps>(p, g, lane, cur[(size_t)s]);
            else if (step == 1 && order == 3)
                mc_merge_lane<StaleOps>(p, g, lane, cur[(size_t)s], up[(size_t)s], mc_fg(g, g.y - 1, g.x0 - 1), mc_fg(g, g.y - 1, g.x0 + MC_SEG),
                                        mc_fg(g, g.y, g.x0 - 1));
            else if (step == 1)
                mc_merge_lane<SerialOps>(p, g, lane, cur[(size_t)s], up[(size_t)s], mc_fg(g, g.y - 1, g.x0 - 1), mc_fg(g, g.y - 1, g.x0 + MC_SEG),
                                         mc_fg(g, g.y, g.x0 - 1));
            else if (step == 2) mc_flatten_lane<SerialOps>(p, g, lane, cur[(size_t)s]);
            else if (step == 3) mc_stats_lane<SerialOps>(p, g, lane, cur[(size_t)s]);
            else mc_apply_lane<SerialOps>(p, g, lane, cur[(size_t)s]);
        }
    }
    free(parent); free(area); free(peak);
}

static std::vector<int64_t> make_table(const std::vector<Image>& ims) {
    std::vector<int64_t> t;
    long base = 0, seg0 = 0;
    for (const Image& im : ims) {
        const int64_t row[MC_COLS] = {im.off, im.H, im.W, im.t_on, im.min_area, im.t_peak, base, seg0};
        t.insert(t.end(), row, row + MC_COLS);
        base += (long)im.H * im.W;
        seg0 += (long)im.H * mc_segs_per_row(im.W);
    }
    return t;
}

static int failures = 0;

// bytes: the exact-size buffer; every image of `ims` lies in it.  Runs the four schedules and compares with the flood fill.
static void check_call(const std::string& what, const std::vector<uint8_t>& bytes, const std::vector<Image>& ims, int conn) {
    const std::vector<int64_t> table = make_table(ims);
    long ws = 0;
    for (const Image& im : ims) ws += (long)im.H * im.W;
    if (!mask_clean_table_ok(table.data(), (int)ims.size(), (long long)bytes.size(), ws)) {
        printf("FAIL %s: the table was refused\n", what.c_str());
        ++failures;
        return;
    }
    std::vector<uint8_t> want(bytes);
    for (const Image& im : ims) flood_ref(want.data() + im.off, im, conn);
    for (int order = 0; order < 4; ++order) {
        uint8_t* buf = (uint8_t*)malloc(bytes.size());    // exact size: the sanitizer guards both ends
        memcpy(buf, bytes.data(), bytes.size());
        emulate(buf, table, (int)ims.size(), conn, ws, order);
        if (memcmp(buf, want.data(), bytes.size()) != 0) {
            long bad = 0, first = -1;
            for (size_t i = 0; i < bytes.size(); ++i)
                if (buf[i] != want[i]) { ++bad; if (first < 0) first = (long)i; }
            printf("FAIL %s conn %d order %d: %ld bytes differ, first at %ld (got %d, want %d, was %d)\n", what.c_str(), conn, order, bad, first,
                   buf[first], want[first], bytes[first]);
            ++failures;
        }
        free(buf);
    }
}

// ---- patterns: 1 = foreground ----------------------------------------------------------------------------------------------------------------
static std::vector<uint8_t> pattern(const std::string& kind, int H, int W) {
    std::vector<uint8_t> f((size_t)H * W, 0);
    auto at = [&](int y, int x) -> uint8_t& { return f[(size_t)y * W + x]; };
    if (kind == "all") std::fill(f.begin(), f.end(), 1);
    else if (kind == "checker") { for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) at(y, x) = (y + x) & 1; }
    else if (kind == "spiral") {                          // a 1-pixel path wound inwards from (0, 0), one pixel of background between its turns
        const int dy[4] = {0, 1, 0, -1}, dx[4] = {1, 0, -1, 0};
        auto in = [&](int y, int x) { return y >= 0 && y < H && x >= 0 && x < W; };
        int y = 0, x = 0, d = 0, turns = 0;
        at(0, 0) = 1;
        while (turns < 2) {
            const int ny = y + dy[d], nx = x + dx[d], my = ny + dy[d], mx = nx + dx[d];
            if (in(ny, nx) && !at(ny, nx) && !(in(my, mx) && at(my, mx))) { y = ny; x = nx; at(y, x) = 1; turns = 0; }
            else { d = (d + 1) & 3; ++turns; }
        }
    } else if (kind == "comb") {                          // teeth in every second column, joined by the LAST row only
        for (int y = 0; y < H; ++y) for (int x = 0; x < W; x += 2) at(y, x) = 1;
        for (int x = 0; x < W; ++x) at(H - 1, x) = 1;
    } else if (kind == "u") {                             // two arms at the left and right edge that meet only in the last row
        for (int y = 0; y < H; ++y) { at(y, 0) = 1; at(y, W - 1) = 1; }
        for (int x = 0; x < W; ++x) at(H - 1, x) = 1;
    } else if (kind == "diag") {                          // diagonals of both directions, five columns apart
        for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) at(y, x) = (x + y) % 5 == 0 || (x - y + 5 * H) % 7 == 0;
    } else if (kind == "corner") {                        // 3 x 3 blobs left and right of every 64-column border that touch only diagonally
        for (int cx = 64; cx < W + 3; cx += 64)
            for (int k = 0; 3 * k < H; ++k)
                for (int y = 3 * k; y < 3 * k + 3 && y < H; ++y)
                    for (int x = (k & 1 ? cx : cx - 3); x < (k & 1 ? cx + 3 : cx); ++x)
                        if (x >= 0 && x < W) at(y, x) = 1;
    } else {                                              // "rNN": random at density NN %
        const unsigned pct = (unsigned)atoi(kind.c_str() + 1);
        for (auto& v : f) v = rnd() % 100 < pct;
    }
    return f;
}

int main() {
    const int shapes[][2] = {{1, 1}, {1, 64}, {64, 1}, {37, 53}, {63, 63}, {257, 300}, {3, 6000}};
    const char* kinds[] = {"all", "checker", "spiral", "comb", "u", "diag", "corner", "r02", "r05", "r10", "r20", "r30", "r41", "r50", "r60"};
    long calls = 0;
    for (const auto& hw : shapes)
        for (const char* kind : kinds) {
            const int H = hw[0], W = hw[1];
            rng_state = 12345u + (uint32_t)(H * 131 + W);
            const std::vector<uint8_t> f = pattern(kind, H, W);
            std::vector<uint8_t> bytes(f.size());
            for (size_t i = 0; i < f.size(); ++i) bytes[i] = (uint8_t)(f[i] ? 128 + rnd() % 128 : rnd() % 128);
            for (int conn : {8, 4}) {
                // area and peak both decide: levels 128 .. 255 are uniform, so a small component often stays below 230
                check_call(std::string(kind) + " " + std::to_string(H) + "x" + std::to_string(W), bytes, {{H, W, 128, 5, 230, 0}}, conn);
                check_call(std::string(kind) + " area only", bytes, {{H, W, 128, 3, 0, 0}}, conn);
                calls += 2;
            }
        }
    // a ragged call: four images of different sizes with their own parameters, back to back and out of order in the buffer, neighbouring
    // blocks ending and beginning with foreground; a gap of untouched bytes between two of them
    {
        const int dims[4][2] = {{5, 70}, {9, 64}, {1, 130}, {66, 3}};
        std::vector<Image> ims;
        long off = 0;
        for (int k = 0; k < 4; ++k) {
            ims.push_back({dims[k][0], dims[k][1], 100 + 20 * k, 2 + k, k == 2 ? 0 : 180, off});
            off += (long)dims[k][0] * dims[k][1] + (k == 1 ? 7 : 0);
        }
        std::vector<uint8_t> bytes((size_t)off);
        for (auto& v : bytes) v = (uint8_t)(rnd() % 256);
        for (const Image& im : ims) {                      // the first and last row of every block: foreground
            for (int x = 0; x < im.W; ++x) bytes[(size_t)im.off + x] = bytes[(size_t)im.off + (long)(im.H - 1) * im.W + x] = (uint8_t)(im.t_on + x % 5);
        }
        std::vector<Image> shuffled = {ims[2], ims[0], ims[3], ims[1]};
        for (int conn : {8, 4}) { check_call("ragged", bytes, ims, conn); check_call("ragged shuffled", bytes, shuffled, conn); calls += 2; }
        // t_on = 256: no foreground, nothing changes; t_on = 0: everything is foreground, one component
        check_call("t_on 256", bytes, {{5, 70, 256, 1000, 256, 0}}, 8);
        check_call("t_on 0", bytes, {{5, 70, 0, 351, 0, 0}}, 4);
        calls += 2;
        // tables that must be refused
        std::vector<int64_t> t = make_table(ims);
        const long long nb = (long long)bytes.size(), ws = 5 * 70 + 9 * 64 + 130 + 66 * 3;
        auto refused = [&](const char* what, std::vector<int64_t> bad, int n, long long b, long long w) {
            if (mask_clean_table_ok(bad.data(), n, b, w)) { printf("FAIL: accepted %s\n", what); ++failures; }
        };
        if (!mask_clean_table_ok(t.data(), 4, nb, ws)) { printf("FAIL: the good table was refused\n"); ++failures; }
        refused("n = 0", t, 0, nb, ws);
        refused("a short buffer", t, 4, nb - 1, ws);
        refused("a short workspace", t, 4, nb, ws - 1);
        { auto b = t; b[MC_COLS + MC_OFF] -= 1; refused("overlapping blocks", b, 4, nb, ws); }
        { auto b = t; b[MC_OFF] = -1; refused("a negative offset", b, 4, nb, ws); }
        { auto b = t; b[MC_H] = 0; refused("H = 0", b, 4, nb, ws); }
        { auto b = t; b[MC_T_ON] = 257; refused("t_on = 257", b, 4, nb, ws); }
        { auto b = t; b[MC_MIN_AREA] = 0; refused("min_area = 0", b, 4, nb, ws); }
        { auto b = t; b[2 * MC_COLS + MC_BASE] += 1; refused("a wrong BASE", b, 4, nb, ws); }
        { auto b = t; b[3 * MC_COLS + MC_SEG0] -= 1; refused("a wrong SEG0", b, 4, nb, ws); }
        { auto b = t; b[MC_H] = 1 << 20; b[MC_W] = 1 << 20; refused("more than 2^31 - 1 pixels", b, 1, 1LL << 41, 1LL << 41); }
    }
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("mask clean OK: %ld calls, four schedules each\n", calls);
    return 0;
}
