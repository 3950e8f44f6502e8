// Scene groups on the device (config key SCENE_GROUP): the tiles of several small scenes run as ONE pass 1 over a
// vertical stack of their (padded) images.  Two bandwidth-bound, output-stationary kernels build and take apart that stack; everything
// between them is the existing scene path, unedited.  The reference has no such step.
//
// scene_group_pack (C = 3: the scenes, C = 1: their validity masks): one launch writes every byte of the stack u8 [Ha,Wa,C] exactly once
// and nothing else.  The source is one ragged buffer that holds the real scenes back to back; a device table (scene_group_piece.hpp) has
// one row per scene.  A workgroup takes 1024 pieces of ONE stack row, finds the row's scene by a binary search of row0 — the same for
// every lane, so the table is read through the scalar cache — and from there on a piece inside the scene's W' columns is a piece of
// scene_pad (pad_piece: contiguous 16-byte copies in the interior, pad_fold in the margins, the scene's own pads), the columns beyond W'
// are zeros.  scene_group_crop: one launch cuts every scene's window out of both u8 masks of the stack into two ragged outputs; a row of a
// window is pad_piece with a negative left pad, so the same alignment cases serve.  Rows of the stack outside every window (SCENE_PAD's
// margins) have no pieces.  No atomics, no LDS, one store per piece, 64-bit byte offsets.
#include "common.hpp"
#include "kernels.hpp"

namespace srh {

template <int C>
__global__ __launch_bounds__(PAD_THREADS) void scene_group_pack_kernel(SceneGroupParams p, long n_groups, int groups_per_row) {
    for (long g = blockIdx.x; g < n_groups; g += gridDim.x) {         // uniform over the workgroup
        const long Y = g / groups_per_row;
        const long piece0 = (g - Y * groups_per_row) * PAD_PIECES;
        const GroupRow row = group_pack_row<C>(p, Y);
        const long piece_end = piece0 + PAD_PIECES < row.r.n_pieces ? piece0 + PAD_PIECES : row.r.n_pieces;
        for (long pc = piece0 + threadIdx.x; pc < piece_end; pc += PAD_THREADS) group_pack_piece<C>(row, pc);
    }
}

// blockIdx.y: 0 the keypoint mask, 1 the road mask (two sources, two destinations, one table)
__global__ __launch_bounds__(PAD_THREADS) void scene_group_crop_kernel(SceneGroupParams kp, SceneGroupParams road, long n_groups, int groups_per_row) {
    SceneGroupParams p = kp;
    if (blockIdx.y) { p.src = road.src; p.dst = road.dst; }
    for (long g = blockIdx.x; g < n_groups; g += gridDim.x) {
        const long Y = g / groups_per_row;
        const long piece0 = (g - Y * groups_per_row) * PAD_PIECES;
        const GroupRow row = group_crop_row(p, Y);
        const long piece_end = piece0 + PAD_PIECES < row.r.n_pieces ? piece0 + PAD_PIECES : row.r.n_pieces;
        for (long pc = piece0 + threadIdx.x; pc < piece_end; pc += PAD_THREADS) group_crop_piece(row, pc);
    }
}

static bool group_params_ok(const SceneGroupParams& p) {
    return p.src && p.dst && p.table && p.n >= 1 && p.Ha >= 1 && p.Wa >= 1 && (long)p.Ha * p.Wa <= 2147483647L && (p.C == 1 || p.C == 3) &&
           p.mode >= PAD_REFLECT && p.mode <= PAD_CONSTANT;
}

int launch_scene_group_pack(const SceneGroupParams& p, hipStream_t s) {
    if (!group_params_ok(p)) return -2;
    const long groups_per_row = group_groups_per_row(p.Wa, p.C);
    const long n_groups = groups_per_row * p.Ha;
    const unsigned grid = (unsigned)(n_groups < (1L << 20) ? n_groups : (1L << 20));
    if (p.C == 3) hipLaunchKernelGGL(scene_group_pack_kernel<3>, dim3(grid), dim3(PAD_THREADS), 0, s, p, n_groups, (int)groups_per_row);
    else hipLaunchKernelGGL(scene_group_pack_kernel<1>, dim3(grid), dim3(PAD_THREADS), 0, s, p, n_groups, (int)groups_per_row);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_scene_group_crop(const SceneGroupParams& kp, const SceneGroupParams& road, hipStream_t s) {
    if (!group_params_ok(kp) || !group_params_ok(road) || kp.C != 1 || road.C != 1 || kp.Ha != road.Ha || kp.Wa != road.Wa || kp.n != road.n ||
        kp.table != road.table)
        return -2;
    const long groups_per_row = group_groups_per_row(kp.Wa, 1);
    const long n_groups = groups_per_row * kp.Ha;
    const unsigned grid = (unsigned)(n_groups < (1L << 15) ? n_groups : (1L << 15));
    hipLaunchKernelGGL(scene_group_crop_kernel, dim3(grid, 2), dim3(PAD_THREADS), 0, s, kp, road, n_groups, (int)groups_per_row);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace srh
