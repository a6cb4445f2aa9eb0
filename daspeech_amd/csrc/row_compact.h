// row_compact.h — ranks of the flagged elements of a row from 64-bit ballots and popcounts (wave = 64 lanes): what the kernels that compact a
// row without a sort share (embed_entry_train.hip: positions from a cumulative count, the lists of the hot keys; path_features_train.hip:
// the vertices on the path).  Included after common.h.
#pragma once

namespace dsp {

// flagged lanes below `lane` in a ballot: the rank of a flagged lane among the flagged ones
__device__ __forceinline__ int lanes_before(unsigned long long bal, int lane) { return __popcll(bal & ((1ull << lane) - 1ull)); }

// kept elements of sample row [0, t0) (`before`, the same in every thread) and the keep flags of the tile [t0, t0 + TILE) as a mask
// (bit i: position t0 + i), TILE <= 32.  All 256 threads of the workgroup call it.
template <int TILE, typename KeepFn>
__device__ __forceinline__ void tile_positions(KeepFn keep, int t0, int L, int& before, unsigned& flags)
{
    static_assert(TILE >= 1 && TILE <= 32, "the tile's flags are one 32-bit mask");
    __shared__ int wsum[4];
    int c = 0;
    for (int t = threadIdx.x; t < t0; t += 256) c += keep(t) ? 1 : 0;
    c = wave_sum(c);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    before = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    const int lane = threadIdx.x & 63, t = t0 + lane;
    const bool k = lane < TILE && t < L && keep(t);
    flags = (unsigned)__ballot(k);
}

}  // namespace dsp
