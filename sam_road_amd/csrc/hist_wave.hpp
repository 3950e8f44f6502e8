// The wave-level histogram add of scene_bands.hip and scene_float.hip: device code shared by the two files.
#pragma once
#include <stdint.h>

namespace srh {

constexpr int HIST_PEEL = 2;

// One band's value of every lane of a wave into the table: `active` lanes hold v.  Uniform control flow (todo is the same in every
// lane), so the cross-lane reads are made with all lanes of the wave running.  The first value peeled goes through the wave's pending
// run (pend_v, pend_n; the same in every lane): as long as round after round leads with the same value, nothing is added to memory —
// the run is added once, when another value ends it or the wave is done (hist_wave_flush).
__device__ __forceinline__ void hist_wave_add(uint32_t* table, uint32_t v, bool active, uint32_t& pend_v, uint32_t& pend_n, int lane) {
    unsigned long long todo = __ballot(active);
#pragma unroll
    for (int r = 0; r < HIST_PEEL; ++r) {
        if (!todo) break;
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t v0 = (uint32_t)__shfl((int)v, leader, 64);
        const unsigned long long same = __ballot(active && v == v0);
        const uint32_t cnt = (uint32_t)__popcll(same);
        if (r == 0) {
            if (v0 == pend_v) {
                pend_n += cnt;
            } else {
                if (pend_n && lane == 0) atomicAdd(&table[pend_v], pend_n);
                pend_v = v0; pend_n = cnt;
            }
        } else if (lane == leader) {
            atomicAdd(&table[v0], cnt);
        }
        if (v == v0) active = false;
        todo &= ~same;
    }
    if (active) atomicAdd(&table[v], 1u);
}

__device__ __forceinline__ void hist_wave_flush(uint32_t* table, uint32_t pend_v, uint32_t pend_n, int lane) {
    if (pend_n && lane == 0) atomicAdd(&table[pend_v], pend_n);
}

}  // namespace srh
