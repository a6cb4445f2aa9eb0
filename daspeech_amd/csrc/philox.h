// philox.h — the counter-based dropout mask of the training operators (residual_norm_train.hip, relpos_attention_train.hip).
// Element e of a call's index space keeps its value when word (e & 3) of Philox4x32-10(counter = (e >> 2, offset), key = seed) has its top
// 24 bits >= thr (thr = ceil(p * 2^24)); dsp_dropout_keep_mask writes the same flags as bytes.
// (seed, offset) are host integers, or — the ..._state entries, for launches recorded into a graph — come from a device-resident state
// {seed, offset} to which the host integer `offset` is the call's distance (philox_stream): a replay reads whatever the state holds then.
#pragma once
#include "common.h"

namespace dsp {

// ---- Philox4x32-10 (Salmon et al., SC'11): counter (c0..c3), key (k0, k1) -> four words
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&out)[4])
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
// The (seed, offset) a kernel uses: its arguments as they are when state is null; else seed = state[0] and offset = state[1] + offset (the
// argument is then the call's distance from the state's offset, the seed argument is not used).  Called once at kernel entry: `state` is a
// kernel argument, so this is one uniform 16-byte load per wave.  Nothing but dsp_dropout_state_advance writes a state.
__device__ __forceinline__ void philox_stream(uint64_t& seed, uint64_t& offset, const uint64_t* __restrict__ state)
{
    if (state) { seed = state[0]; offset += state[1]; }
}
// keep flags of the V elements from element e on (e a multiple of 4)
template <int V> __device__ __forceinline__ void keep_flags(uint64_t e, uint64_t seed, uint64_t offset, uint32_t thr, bool (&keep)[V])
{
#pragma unroll
    for (int j = 0; j < V / 4; ++j) {
        const uint64_t g = (e >> 2) + j;
        uint32_t w[4];
        philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), (uint32_t)offset, (uint32_t)(offset >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), w);
#pragma unroll
        for (int i = 0; i < 4; ++i) keep[4 * j + i] = (w[i] >> 8) >= thr;
    }
}
// the keep flag of ONE element e (any e): the flag keep_flags gives it
__device__ __forceinline__ bool keep_flag(uint64_t e, uint64_t seed, uint64_t offset, uint32_t thr)
{
    const uint64_t g = e >> 2;
    uint32_t w[4];
    philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), (uint32_t)offset, (uint32_t)(offset >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), w);
    const uint32_t k = (uint32_t)e & 3u;
    const uint32_t x = k == 0 ? w[0] : (k == 1 ? w[1] : (k == 2 ? w[2] : w[3]));
    return (x >> 8) >= thr;
}

}  // namespace dsp
