// ra_frag.h — what the attention training kernels share (relpos_attention_train.hip, mha_train.hip): the 32x32x16 matrix-core product in the
// "NT" form  C[32][32] += A[32][k] . B^T[32][k]  on LDS images whose k index is contiguous, the staging of such images, the accumulator's
// row map, and the keep flags of a 32 x 32 score tile under the rule of philox.h.
//
// Operand layout (A and B alike): lane l holds row l & 31, k = 16 s + 8 (l >> 5) .. + 7 of k step s — one 16-byte read.  The result has its
// column (the B^T row) on the lane and its rows in the registers: row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)  (RA_ROW).
#pragma once
#include "common.h"
#include "philox.h"

namespace dsp {

typedef _Float16 ra_h8 __attribute__((ext_vector_type(8)));
typedef __bf16 ra_b8 __attribute__((ext_vector_type(8)));
typedef float ra_acc __attribute__((ext_vector_type(16)));
typedef unsigned short ra_u16;

constexpr int RA_P64 = 72;      // pitch (elements) of an LDS image with 64 k values: 144 bytes, 16-byte aligned rows
constexpr int RA_P32 = 40;      // with 32 k values: 80 bytes
#define RA_ROW(reg, hi) (((reg) & 3) + 8 * ((reg) >> 2) + 4 * (hi))

template <typename E> struct Ra;
template <> struct Ra<__half> {
    using V = ra_h8;
    static __device__ __forceinline__ ra_acc mma(V a, V b, ra_acc c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ float val(ra_u16 u) { return __half2float(__ushort_as_half(u)); }
    static __device__ __forceinline__ ra_u16 bits(float f) { return __half_as_ushort(__float2half(f)); }
};
template <> struct Ra<__hip_bfloat16> {
    using V = ra_b8;
    static __device__ __forceinline__ ra_acc mma(V a, V b, ra_acc c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ float val(ra_u16 u) { return __uint_as_float((uint32_t)u << 16); }
    static __device__ __forceinline__ ra_u16 bits(float f) { const __hip_bfloat16 v = __float2bfloat16(f); ra_u16 u; __builtin_memcpy(&u, &v, 2); return u; }
};

// acc += A . B^T over 16 * KS values of k: A rows at a + r * lda, B^T rows at b + r * ldb, k contiguous in both (16-byte aligned rows)
template <typename E, int KS>
__device__ __forceinline__ void ra_mma_nt(ra_acc& acc, const ra_u16* a, int lda, const ra_u16* b, int ldb, int lane)
{
    using V = typename Ra<E>::V;
    const int r = lane & 31, k0 = (lane >> 5) * 8;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const V va = *reinterpret_cast<const V*>(a + r * lda + 16 * s + k0);
        const V vb = *reinterpret_cast<const V*>(b + r * ldb + 16 * s + k0);
        acc = Ra<E>::mma(va, vb, acc);
    }
}

// rows row0 .. row0 + n - 1 (n = 32 or 64) of a matrix of R rows, 64 columns from src on, row stride ld -> an LDS image; rows outside
// [0, R) as zeros.  TR: the image is [64 columns][n rows] instead of [n rows][64 columns].  bias (fp32, 64): added in fp32 and rounded once.
// NT threads share the work (lane: the thread's index among them).
template <typename E, bool TR, int NT = 64>
__device__ __forceinline__ void ra_stage(ra_u16* dst, int pitch, const E* src, long ld, int row0, int n, int R, const float* bias, int lane)
{
    for (int ci = lane; ci < n * 8; ci += NT) {
        const int rl = ci >> 3, c8 = (ci & 7) * 8, row = row0 + rl;
        uint4 u = make_uint4(0u, 0u, 0u, 0u);
        if (row >= 0 && row < R) u = *reinterpret_cast<const uint4*>(src + (long)row * ld + c8);
        const uint32_t w[4] = {u.x, u.y, u.z, u.w};
        ra_u16 e[8];
#pragma unroll
        for (int x = 0; x < 4; ++x) { e[2 * x] = (ra_u16)(w[x] & 0xffffu); e[2 * x + 1] = (ra_u16)(w[x] >> 16); }
        if (bias) {
#pragma unroll
            for (int x = 0; x < 8; ++x) e[x] = Ra<E>::bits(Ra<E>::val(e[x]) + bias[c8 + x]);
        }
        if (!TR) {
            *reinterpret_cast<uint4*>(dst + rl * pitch + c8) =
                make_uint4((uint32_t)e[0] | ((uint32_t)e[1] << 16), (uint32_t)e[2] | ((uint32_t)e[3] << 16), (uint32_t)e[4] | ((uint32_t)e[5] << 16),
                           (uint32_t)e[6] | ((uint32_t)e[7] << 16));
        } else {
#pragma unroll
            for (int x = 0; x < 8; ++x) dst[(c8 + x) * pitch + rl] = e[x];
        }
    }
}

// element (b, h, i, j) of the mask's index space [B][H][T rows][Tp columns]
__device__ __forceinline__ uint64_t ra_elem(int b, int h, int H, int T, int Tp, int i, int j)
{
    return (((uint64_t)b * H + h) * (uint64_t)T + (uint64_t)i) * (uint64_t)Tp + (uint64_t)j;
}

// The keep flags of the tile of queries i0 .. i0+31 and keys j0 .. j0+31 of sample b, head h, as bytes kb[32][32] in LDS (1 KiB), written by ONE
// wave: j0 a multiple of 4 (a query's row of the index space starts on a counter boundary: Tp is a multiple of 4), so the tile's 32 x 8 Philox
// calls are shared out, 4 per lane.  The reader (ra_keep_read) follows a barrier of whatever scope holds the writer and the reader.
__device__ __forceinline__ void ra_keep_fill(unsigned char* kb, int b, int h, int H, int T, int Tp, int i0, int j0, uint64_t seed, uint64_t offset,
                                             uint32_t thr, int lane)
{
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int il = (lane >> 3) + 8 * t, gq = lane & 7;
        bool keep[4];
        keep_flags<4>(ra_elem(b, h, H, T, Tp, i0 + il, j0 + 4 * gq), seed, offset, thr, keep);
        *reinterpret_cast<uint32_t*>(kb + il * 32 + 4 * gq) = (keep[0] ? 1u : 0u) | (keep[1] ? 0x100u : 0u) | (keep[2] ? 0x10000u : 0u) | (keep[3] ? 0x1000000u : 0u);
    }
}
// the keep factors (keep_scale or 0) of a lane's 16 accumulator elements from those bytes
__device__ __forceinline__ void ra_keep_read(const unsigned char* kb, float keep_scale, int lane, float (&kf)[16])
{
    const int jl = lane & 31, hi = lane >> 5;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) kf[reg] = kb[RA_ROW(reg, hi) * 32 + jl] ? keep_scale : 0.f;
}

// a tile with its COLUMN index on the lane -> the image [column][row] (k = the row index contiguous): 4 registers are 4 consecutive rows
template <typename E>
__device__ __forceinline__ void ra_store_t(ra_u16* dst, const float (&x)[16], int lane)
{
    const int jl = lane & 31, hi = lane >> 5;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float q[4] = {x[4 * g], x[4 * g + 1], x[4 * g + 2], x[4 * g + 3]};
        store_f<E, 4>(reinterpret_cast<E*>(dst + jl * RA_P32 + 8 * g + 4 * hi), q);
    }
}

}  // namespace dsp
