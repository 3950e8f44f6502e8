// Scene groups (scene_group.hip): the parameters and the work of ONE item of the pack and the crop kernel, free of HIP so
// that a CPU program can run the kernels' own addressing over every item of a launch (tests/scene_group_check.cpp, under the host
// sanitizers) before a GPU does.  Both are built on scene_pad_piece.hpp: a row of the stack inside its scene IS a row of that scene's
// padded image, and a row of a scene's window of the stack's masks is a row "padded" by minus the window's origin.
#pragma once
#include "scene_pad_piece.hpp"

namespace srh {

// One row of the table per scene, eight int64: the scenes of a group stacked vertically (row0 ascending, row0[0] = 0, row0[k + 1] =
// row0[k] + Hv[k]).  OFF is the byte offset of the scene's block in the ragged buffer of THAT launch: the H * W * C source bytes of the
// pack, the H * W destination bytes of the crop.
constexpr int GROUP_COLS = 8;
constexpr int GROUP_OFF = 0, GROUP_H = 1, GROUP_W = 2, GROUP_TOP = 3, GROUP_LEFT = 4, GROUP_HV = 5, GROUP_WV = 6, GROUP_ROW0 = 7;

// pack: dst u8 [Ha,Wa,C]; stack pixel (row0 + Y, X), X < Wv, holds virtual pixel (Y, X) of the scene (ScenePadParams' rule with the
// scene's own pads), columns X >= Wv hold 0.  crop: the window [row0 + top : .. + H, left : .. + W] of src u8 [Ha,Wa] -> dst + OFF.
struct SceneGroupParams {
    const uint8_t* src = nullptr; uint8_t* dst = nullptr;
    const int64_t* table = nullptr;      // [n, GROUP_COLS]
    int n = 0, Ha = 0, Wa = 0;
    int C = 3;
    int mode = PAD_REFLECT;
    uint32_t fill = 0;
};

// The scene that holds stack row Y (0 <= Y < Ha): the last one whose row0 is <= Y.
SRH_PAD_HD int group_find(const int64_t* table, int n, long Y) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[(long)mid * GROUP_COLS + GROUP_ROW0] <= Y) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// What the pieces of one stack row share: the scene's own pad parameters, the row as pad_piece wants it, and the bytes of the whole
// stack row (pieces are cut at the 16-byte boundaries of the ADDRESS over all Wa * C bytes).
struct GroupRow {
    ScenePadParams q;
    PadRow r;
    long row_b;                  // bytes of the stack row; q.Wv * C of them belong to the scene
    bool live;                   // crop: the stack row lies inside the scene's window
};

template <int C>
SRH_PAD_HD GroupRow group_pack_row(const SceneGroupParams& p, long Y) {
    GroupRow g;
    const int64_t* t = p.table + (long)group_find(p.table, p.n, Y) * GROUP_COLS;
    g.q.H = (int)t[GROUP_H]; g.q.W = (int)t[GROUP_W]; g.q.top = (int)t[GROUP_TOP]; g.q.left = (int)t[GROUP_LEFT];
    g.q.Hv = (int)t[GROUP_HV]; g.q.Wv = (int)t[GROUP_WV]; g.q.C = C; g.q.mode = p.mode; g.q.fill = p.fill;
    g.q.src = p.src + t[GROUP_OFF];
    g.row_b = (long)p.Wa * C;
    g.q.dst = p.dst + t[GROUP_ROW0] * g.row_b;
    g.r.sy = pad_fold(Y - t[GROUP_ROW0] - g.q.top, g.q.H, p.mode);
    g.r.srow = g.q.src + (long)(g.r.sy < 0 ? 0 : g.r.sy) * ((long)g.q.W * C);
    g.r.drow = p.dst + Y * g.row_b;
    g.r.mis = (long)(reinterpret_cast<uintptr_t>(g.r.drow) & 15);
    g.r.n_pieces = (g.r.mis + g.row_b + 15) >> 4;
    g.live = true;
    return g;
}

// Piece pc (0 <= pc < n_pieces) of a stack row: the bytes inside the scene through pad_piece (which clips to q.Wv * C), the tail zeros.
template <int C>
SRH_PAD_HD void group_pack_piece(const GroupRow& g, long pc) {
    const long in_b = (long)g.q.Wv * C;
    const long r0 = pc * 16 - g.r.mis;
    if (r0 < in_b) pad_piece<C>(g.q, g.r, pc);
    if (r0 + 16 <= in_b) return;
    if (r0 >= in_b && r0 + 16 <= g.row_b) {
        *reinterpret_cast<PadWords*>(g.r.drow + r0) = PadWords{{0u, 0u, 0u, 0u}};
        return;
    }
    const long b0 = r0 > in_b ? r0 : in_b, b1 = r0 + 16 < g.row_b ? r0 + 16 : g.row_b;
    for (long b = b0; b < b1; ++b) g.r.drow[b] = 0;
}

// crop: stack row Y of src u8 [Ha,Wa] -> row Y - row0 - top of the scene's H x W block at dst + OFF.  The block's row is the "padded"
// row of pad_piece with left = -left (the interior starts before the row and ends after it, so every whole piece is a contiguous copy).
SRH_PAD_HD GroupRow group_crop_row(const SceneGroupParams& p, long Y) {
    GroupRow g;
    const int64_t* t = p.table + (long)group_find(p.table, p.n, Y) * GROUP_COLS;
    const long y = Y - t[GROUP_ROW0] - t[GROUP_TOP];
    g.live = y >= 0 && y < t[GROUP_H];
    g.q.src = p.src; g.q.H = p.Ha; g.q.W = p.Wa; g.q.Hv = (int)t[GROUP_H]; g.q.Wv = (int)t[GROUP_W]; g.q.top = 0;
    g.q.left = -(int)t[GROUP_LEFT]; g.q.C = 1; g.q.mode = PAD_EDGE; g.q.fill = 0;
    g.q.dst = p.dst + t[GROUP_OFF];
    g.row_b = g.q.Wv;
    g.r.sy = (int)Y;
    g.r.srow = p.src + Y * (long)p.Wa;
    g.r.drow = g.q.dst + (g.live ? y : 0) * g.row_b;
    g.r.mis = (long)(reinterpret_cast<uintptr_t>(g.r.drow) & 15);
    g.r.n_pieces = g.live ? (g.r.mis + g.row_b + 15) >> 4 : 0;
    return g;
}

SRH_PAD_HD void group_crop_piece(const GroupRow& g, long pc) { pad_piece<1>(g.q, g.r, pc); }

// How a launch is cut: a workgroup takes PAD_PIECES consecutive pieces of one stack row (pack: Wa * C bytes; crop: at most Wa).
inline long group_groups_per_row(int Wa, int C) {
    const long max_pieces = (((long)Wa * C + 15) >> 4) + 1;
    return (max_pieces + PAD_PIECES - 1) / PAD_PIECES;
}

// The table on the HOST, checked before a launch: every row consistent and the stack exactly Ha x Wa.  blocks_contiguous: OFF must run
// 0, H W C, ... with no gap (the crop's destination: every byte written once); else the blocks only have to lie inside `bytes`.
inline bool group_table_ok(const int64_t* t, int n, int C, int Ha, int Wa, long long bytes, bool blocks_contiguous) {
    if (!t || n < 1 || Ha < 1 || Wa < 1 || (long long)Ha * Wa > 2147483647LL || bytes < 0) return false;
    long long row0 = 0, off = 0;
    for (int k = 0; k < n; ++k, t += GROUP_COLS) {
        const long long H = t[GROUP_H], W = t[GROUP_W], top = t[GROUP_TOP], left = t[GROUP_LEFT], Hv = t[GROUP_HV], Wv = t[GROUP_WV];
        if (H < 1 || W < 1 || top < 0 || left < 0 || Hv > Ha || Wv > Wa || Hv < H + top || Wv < W + left || H * W > 2147483647LL) return false;
        if (t[GROUP_ROW0] != row0) return false;
        const long long block = H * W * C;
        if (t[GROUP_OFF] < 0 || t[GROUP_OFF] > bytes - block || (blocks_contiguous && t[GROUP_OFF] != off)) return false;
        off += block;
        row0 += Hv;
    }
    return row0 == Ha && (!blocks_contiguous || off == bytes);
}

}  // namespace srh
