// Scene border padding on the device (config key SCENE_PAD): dst u8 [H',W',C] = src u8 [H,W,C] with `top` / `bottom`
// rows and `left` / `right` columns added, C = 3 (the scene) or C = 1 (the validity mask).  Virtual pixel (Y, X) holds source pixel
// (f(Y - top, H), f(X - left, W)): reflect (np.pad "reflect": period 2 (n - 1), any pad width, n = 1 repeats the one pixel), edge
// (clamp) or constant (the fill colour outside [0, n)).  The reference has no such step.
//
// Output-stationary: the work item is one 16-byte piece of a destination row, cut at the 16-byte boundaries of the ADDRESS, clipped to
// the row (scene_pad_piece.hpp).  Every destination byte lies in exactly one (row, piece), is written once, and nothing outside dst is
// written; a piece that two rows share is written by both as single bytes, each its own.  A whole piece inside the row's interior
// (columns left .. left + W) is a contiguous copy of 16 source bytes: one 16-byte load where the source address allows, four 4-byte
// loads where it is 4-byte aligned, else the five aligned words around it shifted into place — and byte loads where those words would
// reach outside src (the first and last bytes of the buffer).  Rows of an odd W are not aligned against each other and the base
// addresses are arbitrary, so the choice is made per piece from the addresses; it is uniform over a row's interior.  Everything else —
// the mirrored margins, the pieces that straddle a margin, the clipped pieces at a row's ends — is produced byte by byte with
// per-pixel addressing.  Offsets are 64-bit from the first product on (a row of W' = 2^31 - 1 pixels is 3 W' bytes).  No atomics, no
// LDS, one store per piece; consecutive lanes take consecutive pieces.
#include "common.hpp"
#include "kernels.hpp"

namespace srh {

template <int C>
__global__ __launch_bounds__(PAD_THREADS) void scene_pad_kernel(ScenePadParams p, long n_groups, int groups_per_row) {
    for (long g = blockIdx.x; g < n_groups; g += gridDim.x) {         // uniform over the workgroup
        const long Y = g / groups_per_row;
        const long piece0 = (g - Y * groups_per_row) * PAD_PIECES;
        const PadRow r = pad_row<C>(p, Y);
        const long piece_end = piece0 + PAD_PIECES < r.n_pieces ? piece0 + PAD_PIECES : r.n_pieces;
        for (long pc = piece0 + threadIdx.x; pc < piece_end; pc += PAD_THREADS) pad_piece<C>(p, r, pc);
    }
}

int launch_scene_pad(const ScenePadParams& p, hipStream_t s) {
    if (!pad_params_ok(p)) return -2;
    const long groups_per_row = pad_groups_per_row(p);
    const long n_groups = groups_per_row * p.Hv;
    const unsigned grid = (unsigned)(n_groups < (1L << 20) ? n_groups : (1L << 20));
    if (p.C == 3) hipLaunchKernelGGL(scene_pad_kernel<3>, dim3(grid), dim3(PAD_THREADS), 0, s, p, n_groups, (int)groups_per_row);
    else hipLaunchKernelGGL(scene_pad_kernel<1>, dim3(grid), dim3(PAD_THREADS), 0, s, p, n_groups, (int)groups_per_row);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace srh
