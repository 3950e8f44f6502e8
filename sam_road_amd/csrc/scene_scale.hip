// Scene resampling on the device (config key SCENE_SCALE): dst u8 [Ho,Wo,C] = src u8 [H,W,C] resampled by two per-axis
// tables of integer taps (start index + T weights that sum to D per output pixel), C = 3 (the scene) or C = 1 (a mask).  The rule that
// builds the tables — area averaging down, bilinear up, one rounding — is stated on the host (sam_road_amd/resample.py); the kernel
// evaluates  out = (sum_y sum_x wy wx v + (Dy Dx) / 2) / (Dy Dx)  in integers, or the validity rule (1 iff every tap with a non-zero
// weight is non-zero), and must equal resample_ref byte for byte.  The reference has no such step.
//
// Separable, output-stationary: a workgroup owns a bh x bw block of outputs (sized on the host from the scale).  Phase 1 stages the
// block's source window into LDS as u8, row by row in 16-byte pieces cut at the 16-byte boundaries of the source ADDRESS (one 16-byte
// load where the piece lies inside src, byte loads at the buffer's first and last bytes: src may start at any byte).  Phase 2 is the row
// pass, window -> u16 row sums in LDS (at most 255 * 32).  Phase 3 is the column pass with the one rounding; a thread produces one
// 4-byte piece of a dst row, cut at the 4-byte boundaries of the address, and stores it as a word (single bytes where the piece is
// shared with the neighbouring block).  Nothing intermediate goes through HBM, every dst byte is written exactly once, no atomics.
// A block whose window does not fit what the launch reserved, every block of the validity rule, and a launch with no window at all (the
// direct form, kept for measurements) gather each output's taps from src instead.  The per-item code is scene_scale_piece.hpp.
#include "common.hpp"
#include "kernels.hpp"

namespace srh {

__global__ __launch_bounds__(SCALE_THREADS) void scene_scale_kernel(SceneScaleParams p, long n_blocks) {
    extern __shared__ __attribute__((aligned(16))) uint8_t scale_lds[];
    for (long b = blockIdx.x; b < n_blocks; b += gridDim.x) {         // uniform over the workgroup
        const ScaleBlock k = scale_block(p, b);
        if (k.lds) {                                                  // uniform too: every thread reads the same four starts
            const long n_stage = scale_stage_items(p, k);
            for (long i = threadIdx.x; i < n_stage; i += SCALE_THREADS) scale_stage_item(p, k, scale_lds, i);
            __syncthreads();
            const long n_row = scale_row_items(p, k);
            for (long i = threadIdx.x; i < n_row; i += SCALE_THREADS) scale_row_item(p, k, scale_lds, i);
            __syncthreads();
        }
        const long n_out = scale_out_items(p, k);
        for (long i = threadIdx.x; i < n_out; i += SCALE_THREADS) scale_out_item(p, k, scale_lds, i);
        if (k.lds) __syncthreads();                                   // the next block of this workgroup restages
    }
}

int launch_scene_resample(const SceneScaleParams& p, hipStream_t s) {
    if (!scale_params_ok(p)) return -2;
    const long n_blocks = scale_blocks(p);
    const unsigned grid = (unsigned)(n_blocks < (1L << 20) ? n_blocks : (1L << 20));
    hipLaunchKernelGGL(scene_scale_kernel, dim3(grid), dim3(SCALE_THREADS), (size_t)scale_lds_bytes(p), s, p, n_blocks);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace srh
