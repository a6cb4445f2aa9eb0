// split_operand.h — the fp32 operand of the split matrix-core kernels as two fp16 pieces,  x = hi + lo / SPLIT_LO  (exact to 2^-22 relative),
// and what those kernels share beside the fragment addresses of split_frag.h: the activation codes of their epilogues and the weight pack.
#pragma once
#include "common.h"

namespace dsp {

constexpr float SPLIT_LO = 2048.f, SPLIT_LO_INV = 1.f / 2048.f;

__device__ __forceinline__ void split_hi_lo(float v, _Float16& hi, _Float16& lo)
{
    hi = (_Float16)v;
    lo = (_Float16)((v - (float)hi) * SPLIT_LO);
}
// ... into element e of two fp16 vectors (an element of a vector type has no reference; written out, not through two scalars: the order of
// the statements decides what the vectoriser makes of an unrolled loop of these), and N values into elements 0 .. N-1
template <typename HV> __device__ __forceinline__ void split_hi_lo(float v, HV& hi, HV& lo, int e)
{
    hi[e] = (_Float16)v;
    lo[e] = (_Float16)((v - (float)hi[e]) * SPLIT_LO);
}
template <int N, typename HV> __device__ __forceinline__ void split_hi_lo(const float* x, HV& hi, HV& lo)
{
#pragma unroll
    for (int e = 0; e < N; ++e) split_hi_lo(x[e], hi, lo, e);
}

// activation codes of the split kernels' epilogues: 0 none, 1 relu, 2 SiLU, 3 GELU (erf form, torch's default)
__device__ __forceinline__ float split_act(float v, int act)
{
    if (act == 1) v = fmaxf(v, 0.f);
    else if (act == 2) v = v / (1.f + __expf(-v));
    else if (act == 3) v = 0.5f * v * (1.f + erff(v * 0.70710678118654752f));
    return v;
}
// ... of N values, the branch on the (launch-uniform) code outside the loop over the values
template <int N> __device__ __forceinline__ void split_act(float (&v)[N], int act)
{
    if (act == 1) {
#pragma unroll
        for (int e = 0; e < N; ++e) v[e] = split_act(v[e], 1);
    } else if (act == 2) {
#pragma unroll
        for (int e = 0; e < N; ++e) v[e] = split_act(v[e], 2);
    } else if (act == 3) {
#pragma unroll
        for (int e = 0; e < N; ++e) v[e] = split_act(v[e], 3);
    }
}

// fp32 weight [ntaps][M][CI] (tap-major) -> hi / lo fp16 in fragment order [ntaps][CI/32][ceil(M/16)][64][8], n elements each
// (conv1d_split.hip; the one pack kernel of dsp_conv1d_split_pack and dsp_hifigan_pack_weights_f32)
int split_pack_launch(const char* who, const float* w, _Float16* w_hi, _Float16* w_lo, long n, int ntaps, int M, int CI, hipStream_t st);

}  // namespace dsp
