// relpos_attention_train.hip — Conformer relative-position self-attention under autograd, gfx950, fp16 / bf16 data:
//     s(b,h,i,j) = ((q_i + u_h).k_j + (q_i + v_h).pos[T-1-i+j]) / 8      masked keys: -inf           (head width 64)
//     P = softmax_j(s)   lse = log sum_j exp s   A = keep ? P / (1-p) : 0   o_i = sum_j A_ij v_j
// and its backward (include/daspeech_decode.h: dsp_relpos_attention_train_fwd / _bwd).  No [B,H,T,T] or [B,H,T,2T-1] tensor is written to
// global memory in either direction: the forward keeps o and lse, the backward recomputes P from q, k, pos, the biases and lse.
//
// One workgroup is ONE wave and owns a block of 32 rows of one (sample, head); every product is v_mfma_f32_32x32x16_f16 / _bf16 in the
// "NT" form  C[32][32] += A[32][k] . B^T[32][k]  with BOTH operands read from LDS images whose k index is contiguous (one 16-byte read per
// lane and k step: lane l takes row l & 31, k = 16 s + 8 (l >> 5) .. + 7 of each image, the same k for A and B).  An image that a product
// needs with the other index contiguous is staged transposed from global memory.  The result has its column (the B^T row) on the lane and
// its rows in the registers: row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)  (RA_ROW).
//
// The relative shift: for queries i0 .. i0+31 and keys j0 .. j0+31 the position rows T-1-i+j are the 63 rows from rb = T-1-i0-31+j0 on;
// G[il][rl] = (q_i + v).pos[rb + rl] is formed for rl = 0 .. 63 (two tiles), written to an fp32 LDS scratch, and bd[il][jl] = G[il][31 - il + jl].
// The backward scatters dS the same way into dG.  j0 may be any integer (the position pass walks the diagonals): rows outside a matrix are
// staged as zeros and keys outside [0, T) are masked.
//
// Backward, three owners (each recomputes P and dS for the tiles it visits; D_i = dO_i . o_i is formed per query block):
//   ra_bwd_kv_kernel   owns 32 keys:            dV = (P o m)^T dO,  dK = dS^T (Q + u)
//   ra_bwd_q_kernel    owns 32 queries:         dq = dS K + dG Pos, and one fp32 partial of du / dv (column sums of the two terms)
//   ra_bwd_pos_kernel  owns 32 position rows of a sample: an fp32 partial [B][2T-1][C] of dPos = dG^T (Q + v)
// and two tails add the partials in ASCENDING order (samples; samples x query blocks).  No float atomics, no hand-off between workgroups.
//
// The dropout mask is never stored: element e = ((b H + h) T + i) Tp + j, Tp = T rounded up to a multiple of 4, of the rule in philox.h.
#include "common.h"
#include "host_gates.h"
#include "philox.h"
#include "ra_frag.h"
#include "../../include/daspeech_decode.h"

namespace dsp {

constexpr int RA_PG = 65;       // pitch (floats) of the shift scratch
// bias_u / bias_v of head h as floats: bias[0..63] = u, bias[64..127] = v
__device__ __forceinline__ void ra_load_bias(float* bias, const void* bu, const void* bv, int pdtype, int h, int lane)
{
    for (int c = lane; c < 128; c += 64) {
        const void* p = c < 64 ? bu : bv;
        const int at = h * 64 + (c & 63);
        bias[c] = param_load(p, pdtype, at);
    }
}

// the scaled, masked scores of queries i0 .. i0+31 (images Qu, Qv) and keys j0 .. j0+31 (image Ks; Ps: the 64 position rows from rb on)
template <typename E>
__device__ __forceinline__ void ra_scores(const ra_u16* Qu, const ra_u16* Qv, const ra_u16* Ks, const ra_u16* Ps, float* Gs, int j0, int T,
                                          const unsigned char* mrow, int lane, float (&s)[16])
{
    ra_acc ac = {0}, g0 = {0}, g1 = {0};
    ra_mma_nt<E, 4>(ac, Qu, RA_P64, Ks, RA_P64, lane);
    ra_mma_nt<E, 4>(g0, Qv, RA_P64, Ps, RA_P64, lane);
    ra_mma_nt<E, 4>(g1, Qv, RA_P64, Ps + 32 * RA_P64, RA_P64, lane);
    const int jl = lane & 31, hi = lane >> 5;
    __syncthreads();
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int il = RA_ROW(reg, hi);
        Gs[il * RA_PG + jl] = g0[reg];
        Gs[il * RA_PG + 32 + jl] = g1[reg];
    }
    __syncthreads();
    const int j = j0 + jl;
    const bool ok = j >= 0 && j < T && !(mrow && mrow[j]);
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int il = RA_ROW(reg, hi);
        s[reg] = ok ? (ac[reg] + Gs[il * RA_PG + 31 - il + jl]) * 0.125f : NEG_INF;
    }
    __syncthreads();
}

// The keep factors (keep_scale or 0) of a lane's 16 elements of the tile of queries i0 .. i0+31 and keys j0 .. j0+31.  j0 a multiple of 4 (a query's
// row of the index space starts on a counter boundary: Tp is a multiple of 4): the tile's 32 x 8 Philox calls are shared out, 4 per lane, and the
// flags pass through LDS as bytes (kb: 1 KiB, the shift scratch, free after ra_scores).  Any other j0 (the position pass): one call per element.
__device__ __forceinline__ void ra_keep_tile(unsigned char* kb, int b, int h, int H, int T, int i0, int j0, uint64_t seed, uint64_t offset, uint32_t thr,
                                             float keep_scale, int lane, float (&kf)[16])
{
    const int jl = lane & 31, hi = lane >> 5, Tp = (T + 3) & ~3;
    if ((j0 & 3) == 0) {                                                    // workgroup-uniform
        ra_keep_fill(kb, b, h, H, T, Tp, i0, j0, seed, offset, thr, lane);
        __syncthreads();
        ra_keep_read(kb, keep_scale, lane, kf);
        __syncthreads();
    } else {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) kf[reg] = keep_flag(ra_elem(b, h, H, T, Tp, i0 + RA_ROW(reg, hi), j0 + jl), seed, offset, thr) ? keep_scale : 0.f;
    }
}

// ---------------------------------------------------------------- forward
template <typename E>
__global__ __launch_bounds__(64) void ra_fwd_kernel(const E* __restrict__ q, const E* __restrict__ k, const E* __restrict__ v, long ld,
                                                    const E* __restrict__ pos, const void* __restrict__ bu, const void* __restrict__ bv, int pdtype,
                                                    const unsigned char* __restrict__ mask, float keep_scale, uint32_t thr, uint64_t seed,
                                                    uint64_t offset, const uint64_t* __restrict__ rng_state, E* __restrict__ out,
                                                    float* __restrict__ lse, int T_, int H)
{
    __shared__ __attribute__((aligned(16))) ra_u16 Qu[32 * RA_P64], Qv[32 * RA_P64], Ks[32 * RA_P64], Ps[64 * RA_P64], Vt[64 * RA_P32], Pp[32 * RA_P32];
    __shared__ float Gs[32 * RA_PG], bias[128];
    const int lane = threadIdx.x, jl = lane & 31, hi = lane >> 5;
    philox_stream(seed, offset, rng_state);
    const int T = T_, nI = (T + 31) / 32, C = H * 64;
    const int ib = blockIdx.x % nI, bh = blockIdx.x / nI, h = bh % H, b = bh / H, i0 = ib * 32;
    const E* qb = q + (long)b * T * ld + h * 64;
    const E* kb = k + (long)b * T * ld + h * 64;
    const E* vb = v + (long)b * T * ld + h * 64;
    const E* pb = pos + h * 64;
    const unsigned char* mrow = mask ? mask + (long)b * T : nullptr;
    ra_load_bias(bias, bu, bv, pdtype, h, lane);
    __syncthreads();
    ra_stage<E, false>(Qu, RA_P64, qb, ld, i0, 32, T, bias, lane);
    ra_stage<E, false>(Qv, RA_P64, qb, ld, i0, 32, T, bias + 64, lane);
    float m[16], l[16];
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) { m[reg] = NEG_INF; l[reg] = 0.f; }
    ra_acc o0 = {0}, o1 = {0};
#pragma unroll 1
    for (int j0 = 0; j0 < T; j0 += 32) {
        ra_stage<E, false>(Ks, RA_P64, kb, ld, j0, 32, T, nullptr, lane);
        ra_stage<E, false>(Ps, RA_P64, pb, C, T - 1 - i0 - 31 + j0, 64, 2 * T - 1, nullptr, lane);
        ra_stage<E, true>(Vt, RA_P32, vb, ld, j0, 32, T, nullptr, lane);
        __syncthreads();
        float s[16], kf[16];
        ra_scores<E>(Qu, Qv, Ks, Ps, Gs, j0, T, mrow, lane, s);
        if (thr) ra_keep_tile(reinterpret_cast<unsigned char*>(Gs), b, h, H, T, i0, j0, seed, offset, thr, keep_scale, lane, kf);
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int il = RA_ROW(reg, hi);
            const float mn = fmaxf(m[reg], lanes_max<32>(s[reg]));
            const float ms = mn == NEG_INF ? 0.f : mn;                      // nothing but masked keys so far: every weight is 0
            const float a = expf(m[reg] - ms);
            float p = expf(s[reg] - ms);
            l[reg] = fmaf(l[reg], a, lanes_sum<32>(p));
            m[reg] = mn;
            o0[reg] *= a; o1[reg] *= a;
            if (thr) p *= kf[reg];
            Pp[il * RA_P32 + jl] = Ra<E>::bits(p);
        }
        __syncthreads();
        ra_mma_nt<E, 2>(o0, Pp, RA_P32, Vt, RA_P32, lane);
        ra_mma_nt<E, 2>(o1, Pp, RA_P32, Vt + 32 * RA_P32, RA_P32, lane);
        __syncthreads();
    }
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int i = i0 + RA_ROW(reg, hi);
        if (i < T) {
            const float inv = 1.f / l[reg];                                 // every key masked: 0 * inf = NaN, as torch's soft-max
            E* orow = out + ((long)b * T + i) * C + h * 64;
            orow[jl] = from_f<E>(o0[reg] * inv);
            orow[32 + jl] = from_f<E>(o1[reg] * inv);
            if (jl == 0) lse[((long)b * H + h) * T + i] = m[reg] + logf(l[reg]);
        }
    }
}

// ---------------------------------------------------------------- backward: what the three owners share
// D_i = dO_i . o_i and lse_i of the query block (rows past T: D = 0, lse = +inf, so that P = 0 there), one value per accumulator register
template <typename E>
__device__ __forceinline__ void ra_row_consts(const ra_u16* dOs, const E* __restrict__ orow0, const float* __restrict__ lse0, int i0, int T_, int C,
                                              float* Dl, float* Ll, int lane, float (&Dr)[16], float (&Lr)[16])
{
    const int il = lane >> 1, c0 = (lane & 1) * 32, i = i0 + il;
    float d = 0.f;
    if (i < T_) {
        const uint4* orow = reinterpret_cast<const uint4*>(orow0 + (long)i * C + c0);
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            const uint4 u = orow[x];
            const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
            for (int y = 0; y < 4; ++y) {
                d = fmaf(Ra<E>::val(dOs[il * RA_P64 + c0 + 8 * x + 2 * y]), Ra<E>::val((ra_u16)(w[y] & 0xffffu)), d);
                d = fmaf(Ra<E>::val(dOs[il * RA_P64 + c0 + 8 * x + 2 * y + 1]), Ra<E>::val((ra_u16)(w[y] >> 16)), d);
            }
        }
    }
    d += __shfl_xor(d, 1, 64);
    if ((lane & 1) == 0) { Dl[il] = d; Ll[il] = i < T_ ? lse0[i] : __builtin_huge_valf(); }
    __syncthreads();
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) { Dr[reg] = Dl[RA_ROW(reg, lane >> 5)]; Lr[reg] = Ll[RA_ROW(reg, lane >> 5)]; }
    __syncthreads();
}

// P o m and dS of one 32 x 32 tile from the staged images
template <typename E>
__device__ __forceinline__ void ra_grad_tile(const ra_u16* Qu, const ra_u16* Qv, const ra_u16* Ks, const ra_u16* Ps, const ra_u16* Vs, const ra_u16* dOs,
                                             float* Gs, int i0, int j0, int T_, const unsigned char* mrow, const float (&Dr)[16], const float (&Lr)[16],
                                             float keep_scale, uint32_t thr, uint64_t seed, uint64_t offset, int b, int h, int H, int lane,
                                             float (&pm)[16], float (&ds)[16])
{
    float s[16];
    ra_scores<E>(Qu, Qv, Ks, Ps, Gs, j0, T_, mrow, lane, s);
    ra_acc dp = {0};
    ra_mma_nt<E, 4>(dp, dOs, RA_P64, Vs, RA_P64, lane);
    float kf[16];
    if (thr) ra_keep_tile(reinterpret_cast<unsigned char*>(Gs), b, h, H, T_, i0, j0, seed, offset, thr, keep_scale, lane, kf);
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const float p = expf(s[reg] - Lr[reg]);
        const float f = thr ? kf[reg] : 1.f;
        pm[reg] = p * f;
        ds[reg] = p * (dp[reg] * f - Dr[reg]) * 0.125f;
    }
}

// ---------------------------------------------------------------- backward, owner of 32 keys: dK, dV
template <typename E>
__global__ __launch_bounds__(64) void ra_bwd_kv_kernel(const E* __restrict__ dout, const E* __restrict__ q, const E* __restrict__ k,
                                                       const E* __restrict__ v, long ld, const E* __restrict__ pos, const void* __restrict__ bu,
                                                       const void* __restrict__ bv, int pdtype, const unsigned char* __restrict__ mask,
                                                       const E* __restrict__ out, const float* __restrict__ lse, float keep_scale, uint32_t thr,
                                                       uint64_t seed, uint64_t offset, const uint64_t* __restrict__ rng_state, E* __restrict__ dk,
                                                       E* __restrict__ dv, int T_, int H)
{
    __shared__ __attribute__((aligned(16))) ra_u16 Qu[32 * RA_P64], Qv[32 * RA_P64], Ks[32 * RA_P64], Vs[32 * RA_P64], dOs[32 * RA_P64], Ps[64 * RA_P64],
        QuT[64 * RA_P32], dOT[64 * RA_P32];
    __shared__ __attribute__((aligned(16))) float Gs[32 * RA_PG];
    __shared__ float bias[128], Dl[32], Ll[32];
    // the two transposed tiles live in the shift scratch, which is free once the tile's scores and keep flags are in registers: 51.6 KiB, three
    // workgroups a CU instead of two
    ra_u16* PmT = reinterpret_cast<ra_u16*>(Gs);
    ra_u16* dST = PmT + 32 * RA_P32;
    static_assert(2 * 32 * RA_P32 * sizeof(ra_u16) <= 32 * RA_PG * sizeof(float), "both tiles fit the scratch");
    const int lane = threadIdx.x, jl = lane & 31, hi = lane >> 5;
    philox_stream(seed, offset, rng_state);
    const int T = T_, nI = (T + 31) / 32, C = H * 64;
    const int jb = blockIdx.x % nI, bh = blockIdx.x / nI, h = bh % H, b = bh / H, j0 = jb * 32;
    const E* qb = q + (long)b * T * ld + h * 64;
    const E* gb = dout + (long)b * T * C + h * 64;
    const E* pb = pos + h * 64;
    const unsigned char* mrow = mask ? mask + (long)b * T : nullptr;
    ra_load_bias(bias, bu, bv, pdtype, h, lane);
    ra_stage<E, false>(Ks, RA_P64, k + (long)b * T * ld + h * 64, ld, j0, 32, T, nullptr, lane);
    ra_stage<E, false>(Vs, RA_P64, v + (long)b * T * ld + h * 64, ld, j0, 32, T, nullptr, lane);
    __syncthreads();
    ra_acc k0 = {0}, k1 = {0}, v0 = {0}, v1 = {0};
#pragma unroll 1
    for (int i0 = 0; i0 < T; i0 += 32) {
        ra_stage<E, false>(Qu, RA_P64, qb, ld, i0, 32, T, bias, lane);
        ra_stage<E, false>(Qv, RA_P64, qb, ld, i0, 32, T, bias + 64, lane);
        ra_stage<E, true>(QuT, RA_P32, qb, ld, i0, 32, T, bias, lane);
        ra_stage<E, false>(dOs, RA_P64, gb, C, i0, 32, T, nullptr, lane);
        ra_stage<E, true>(dOT, RA_P32, gb, C, i0, 32, T, nullptr, lane);
        ra_stage<E, false>(Ps, RA_P64, pb, C, T - 1 - i0 - 31 + j0, 64, 2 * T - 1, nullptr, lane);
        __syncthreads();
        float Dr[16], Lr[16], pm[16], ds[16];
        ra_row_consts<E>(dOs, out + (long)b * T * C + h * 64, lse + ((long)b * H + h) * T, i0, T, C, Dl, Ll, lane, Dr, Lr);
        ra_grad_tile<E>(Qu, Qv, Ks, Ps, Vs, dOs, Gs, i0, j0, T, mrow, Dr, Lr, keep_scale, thr, seed, offset, b, h, H, lane, pm, ds);
        ra_store_t<E>(PmT, pm, lane);
        ra_store_t<E>(dST, ds, lane);
        __syncthreads();
        ra_mma_nt<E, 2>(v0, PmT, RA_P32, dOT, RA_P32, lane);
        ra_mma_nt<E, 2>(v1, PmT, RA_P32, dOT + 32 * RA_P32, RA_P32, lane);
        ra_mma_nt<E, 2>(k0, dST, RA_P32, QuT, RA_P32, lane);
        ra_mma_nt<E, 2>(k1, dST, RA_P32, QuT + 32 * RA_P32, RA_P32, lane);
        __syncthreads();
    }
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int j = j0 + RA_ROW(reg, hi);
        if (j < T) {
            const long at = ((long)b * T + j) * C + h * 64 + jl;
            if (dk) { dk[at] = from_f<E>(k0[reg]); dk[at + 32] = from_f<E>(k1[reg]); }
            if (dv) { dv[at] = from_f<E>(v0[reg]); dv[at + 32] = from_f<E>(v1[reg]); }
        }
    }
}

// ---------------------------------------------------------------- backward, owner of 32 queries: dq and one partial of du, dv
template <typename E>
__global__ __launch_bounds__(64) void ra_bwd_q_kernel(const E* __restrict__ dout, const E* __restrict__ q, const E* __restrict__ k,
                                                      const E* __restrict__ v, long ld, const E* __restrict__ pos, const void* __restrict__ bu,
                                                      const void* __restrict__ bv, int pdtype, const unsigned char* __restrict__ mask,
                                                      const E* __restrict__ out, const float* __restrict__ lse, float keep_scale, uint32_t thr,
                                                      uint64_t seed, uint64_t offset, const uint64_t* __restrict__ rng_state, E* __restrict__ dq,
                                                      float* __restrict__ part_u, float* __restrict__ part_v, int T_, int H)
{
    __shared__ __attribute__((aligned(16))) ra_u16 Qu[32 * RA_P64], Qv[32 * RA_P64], Ks[32 * RA_P64], Vs[32 * RA_P64], dOs[32 * RA_P64], Ps[64 * RA_P64],
        KT[64 * RA_P32], PosT[64 * RA_P64], dSs[32 * RA_P32], dG[32 * RA_P64];
    __shared__ float Gs[32 * RA_PG], bias[128], Dl[32], Ll[32];
    const int lane = threadIdx.x, jl = lane & 31, hi = lane >> 5;
    philox_stream(seed, offset, rng_state);
    const int T = T_, nI = (T + 31) / 32, C = H * 64;
    const int ib = blockIdx.x % nI, bh = blockIdx.x / nI, h = bh % H, b = bh / H, i0 = ib * 32;
    const E* qb = q + (long)b * T * ld + h * 64;
    const E* kb = k + (long)b * T * ld + h * 64;
    const E* vb = v + (long)b * T * ld + h * 64;
    const E* pb = pos + h * 64;
    const unsigned char* mrow = mask ? mask + (long)b * T : nullptr;
    ra_load_bias(bias, bu, bv, pdtype, h, lane);
    __syncthreads();
    ra_stage<E, false>(Qu, RA_P64, qb, ld, i0, 32, T, bias, lane);
    ra_stage<E, false>(Qv, RA_P64, qb, ld, i0, 32, T, bias + 64, lane);
    ra_stage<E, false>(dOs, RA_P64, dout + (long)b * T * C + h * 64, C, i0, 32, T, nullptr, lane);
    __syncthreads();
    float Dr[16], Lr[16];
    ra_row_consts<E>(dOs, out + (long)b * T * C + h * 64, lse + ((long)b * H + h) * T, i0, T, C, Dl, Ll, lane, Dr, Lr);
    ra_acc a0 = {0}, a1 = {0}, b0 = {0}, b1 = {0};
#pragma unroll 1
    for (int j0 = 0; j0 < T; j0 += 32) {
        const int rb = T - 1 - i0 - 31 + j0;
        ra_stage<E, false>(Ks, RA_P64, kb, ld, j0, 32, T, nullptr, lane);
        ra_stage<E, true>(KT, RA_P32, kb, ld, j0, 32, T, nullptr, lane);
        ra_stage<E, false>(Vs, RA_P64, vb, ld, j0, 32, T, nullptr, lane);
        ra_stage<E, false>(Ps, RA_P64, pb, C, rb, 64, 2 * T - 1, nullptr, lane);
        ra_stage<E, true>(PosT, RA_P64, pb, C, rb, 64, 2 * T - 1, nullptr, lane);
        for (int x = lane; x < 32 * RA_P64 / 8; x += 64) reinterpret_cast<uint4*>(dG)[x] = make_uint4(0u, 0u, 0u, 0u);
        __syncthreads();
        float pm[16], ds[16];
        ra_grad_tile<E>(Qu, Qv, Ks, Ps, Vs, dOs, Gs, i0, j0, T, mrow, Dr, Lr, keep_scale, thr, seed, offset, b, h, H, lane, pm, ds);
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int il = RA_ROW(reg, hi);
            const ra_u16 x = Ra<E>::bits(ds[reg]);
            dSs[il * RA_P32 + jl] = x;
            dG[il * RA_P64 + 31 - il + jl] = x;
        }
        __syncthreads();
        ra_mma_nt<E, 2>(a0, dSs, RA_P32, KT, RA_P32, lane);
        ra_mma_nt<E, 2>(a1, dSs, RA_P32, KT + 32 * RA_P32, RA_P32, lane);
        ra_mma_nt<E, 4>(b0, dG, RA_P64, PosT, RA_P64, lane);
        ra_mma_nt<E, 4>(b1, dG, RA_P64, PosT + 32 * RA_P64, RA_P64, lane);
        __syncthreads();
    }
    float su0 = 0.f, su1 = 0.f, sv0 = 0.f, sv1 = 0.f;                       // rows past T carry dS = 0
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int i = i0 + RA_ROW(reg, hi);
        su0 += a0[reg]; su1 += a1[reg]; sv0 += b0[reg]; sv1 += b1[reg];
        if (dq && i < T) {
            const long at = ((long)b * T + i) * C + h * 64 + jl;
            dq[at] = from_f<E>(a0[reg] + b0[reg]);
            dq[at + 32] = from_f<E>(a1[reg] + b1[reg]);
        }
    }
    su0 += __shfl_xor(su0, 32, 64); su1 += __shfl_xor(su1, 32, 64); sv0 += __shfl_xor(sv0, 32, 64); sv1 += __shfl_xor(sv1, 32, 64);
    if (hi == 0) {
        const long at = ((long)b * nI + ib) * C + h * 64 + jl;
        if (part_u) { part_u[at] = su0; part_u[at + 32] = su1; }
        if (part_v) { part_v[at] = sv0; part_v[at + 32] = sv1; }
    }
}

// ---------------------------------------------------------------- backward, owner of 32 position rows of a sample: a partial of dPos
template <typename E>
__global__ __launch_bounds__(64) void ra_bwd_pos_kernel(const E* __restrict__ dout, const E* __restrict__ q, const E* __restrict__ k,
                                                        const E* __restrict__ v, long ld, const E* __restrict__ pos, const void* __restrict__ bu,
                                                        const void* __restrict__ bv, int pdtype, const unsigned char* __restrict__ mask,
                                                        const E* __restrict__ out, const float* __restrict__ lse, float keep_scale, uint32_t thr,
                                                        uint64_t seed, uint64_t offset, const uint64_t* __restrict__ rng_state,
                                                        float* __restrict__ part_pos, int T_, int H)
{
    __shared__ __attribute__((aligned(16))) ra_u16 Qu[32 * RA_P64], Qv[32 * RA_P64], Ks[32 * RA_P64], Vs[32 * RA_P64], dOs[32 * RA_P64], Ps[64 * RA_P64],
        QvT[64 * RA_P32], dGT[32 * RA_P32];
    __shared__ float Gs[32 * RA_PG], bias[128], Dl[32], Ll[32];
    const int lane = threadIdx.x, jl = lane & 31, hi = lane >> 5;
    philox_stream(seed, offset, rng_state);
    const int T = T_, NP = 2 * T - 1, nR = (NP + 31) / 32, C = H * 64;
    const int rbk = blockIdx.x % nR, bh = blockIdx.x / nR, h = bh % H, b = bh / H, r0 = rbk * 32;
    const E* qb = q + (long)b * T * ld + h * 64;
    const E* kb = k + (long)b * T * ld + h * 64;
    const E* vb = v + (long)b * T * ld + h * 64;
    const E* gb = dout + (long)b * T * C + h * 64;
    const E* pb = pos + h * 64;
    const unsigned char* mrow = mask ? mask + (long)b * T : nullptr;
    ra_load_bias(bias, bu, bv, pdtype, h, lane);
    __syncthreads();
    ra_acc p0 = {0}, p1 = {0};
#pragma unroll 1
    for (int i0 = 0; i0 < T; i0 += 32) {
        // dG[i][r] = dS[i][j], j = r - (T-1) + i: queries i0 + il and rows r0 + rl meet the 63 keys jb + il + rl
        const int jb = r0 - (T - 1) + i0;
        if (jb + 62 < 0 || jb >= T) continue;
        ra_stage<E, false>(Qu, RA_P64, qb, ld, i0, 32, T, bias, lane);
        ra_stage<E, false>(Qv, RA_P64, qb, ld, i0, 32, T, bias + 64, lane);
        ra_stage<E, true>(QvT, RA_P32, qb, ld, i0, 32, T, bias + 64, lane);
        ra_stage<E, false>(dOs, RA_P64, gb, C, i0, 32, T, nullptr, lane);
        __syncthreads();
        float Dr[16], Lr[16];
        ra_row_consts<E>(dOs, out + (long)b * T * C + h * 64, lse + ((long)b * H + h) * T, i0, T, C, Dl, Ll, lane, Dr, Lr);
#pragma unroll 1
        for (int t = 0; t < 2; ++t) {
            const int j0 = jb + 32 * t;
            ra_stage<E, false>(Ks, RA_P64, kb, ld, j0, 32, T, nullptr, lane);
            ra_stage<E, false>(Vs, RA_P64, vb, ld, j0, 32, T, nullptr, lane);
            ra_stage<E, false>(Ps, RA_P64, pb, C, T - 1 - i0 - 31 + j0, 64, NP, nullptr, lane);
            __syncthreads();
            float pm[16], ds[16];
            ra_grad_tile<E>(Qu, Qv, Ks, Ps, Vs, dOs, Gs, i0, j0, T, mrow, Dr, Lr, keep_scale, thr, seed, offset, b, h, H, lane, pm, ds);
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int il = RA_ROW(reg, hi), rl = 32 * t + jl - il;         // every [rl][il] is written by exactly one of the two tiles
                if (rl >= 0 && rl < 32) dGT[rl * RA_P32 + il] = Ra<E>::bits(ds[reg]);
            }
            __syncthreads();
        }
        ra_mma_nt<E, 2>(p0, dGT, RA_P32, QvT, RA_P32, lane);
        ra_mma_nt<E, 2>(p1, dGT, RA_P32, QvT + 32 * RA_P32, RA_P32, lane);
        __syncthreads();
    }
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int r = r0 + RA_ROW(reg, hi);
        if (r < NP) {
            const long at = ((long)b * NP + r) * C + h * 64 + jl;
            part_pos[at] = p0[reg];
            part_pos[at + 32] = p1[reg];
        }
    }
}

// ---------------------------------------------------------------- tails: the partials in ascending order
template <typename E>
__global__ __launch_bounds__(256) void ra_pos_merge_kernel(const float* __restrict__ part, int B, long n, E* __restrict__ dpos)
{
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    float acc = 0.f;
    for (int b = 0; b < B; ++b) acc += part[(long)b * n + e];
    dpos[e] = from_f<E>(acc);
}
__global__ __launch_bounds__(256) void ra_bias_merge_kernel(const float* __restrict__ part_u, const float* __restrict__ part_v, long nchunks, int C,
                                                            void* __restrict__ du, void* __restrict__ dv, int pdtype)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= 2 * C) return;
    const int c = e % C;
    const float* part = e < C ? part_u : part_v;
    void* o = e < C ? du : dv;
    if (!o) return;
    float acc = 0.f;
    for (long x = 0; x < nchunks; ++x) acc += part[x * C + c];
    param_store(o, pdtype, c, acc);
}

// what the entry points check; 1: nothing to do (B == 0), 0: go on, < 0: refused
static int ra_check(const char* who, int act_dtype, int param_dtype, int B, int T, int H, long ld)
{
    if ((act_dtype != DSP_F16 && act_dtype != DSP_BF16) || (param_dtype != act_dtype && param_dtype != DSP_F32)) {
        set_error("%s: dtype codes %d (q, k, v, pos, out and their gradients: fp16 or bf16) / %d (bias_u, bias_v: the same, or fp32)", who, act_dtype, param_dtype);
        return DSP_EINVAL;
    }
    if (B < 0 || T < 1 || T > DSP_RELPOS_TRAIN_MAX_T || H < 1 || H > 1024 || ld < (long)H * 64 || (ld % 8) ||
        (long)B * H * ((2L * T - 1 + 31) / 32) > (1L << 30)) {
        set_error("%s: bad sizes B=%d T=%d H=%d ld=%ld (1 <= T <= %d, 1 <= H <= 1024, ld >= 64 H and a multiple of 8, B H ceil((2T-1)/32) <= 2^30)", who, B, T, H,
                  ld, DSP_RELPOS_TRAIN_MAX_T);
        return DSP_EINVAL;
    }
    return B == 0 ? 1 : 0;
}

static size_t ra_part_bias_floats(long B, long T, long H) { return (size_t)(B * ((T + 31) / 32) * H * 64); }

}  // namespace dsp

using namespace dsp;

#define RA_DISPATCH(dtype, ...) DSP_DISPATCH_ELEM_16(dtype, E, __VA_ARGS__)

extern "C" size_t dsp_relpos_attention_train_workspace_bytes(int B, int T, int H)
{
    if (B <= 0 || T <= 0 || H <= 0) return 0;
    const size_t floats = 2 * ra_part_bias_floats(B, T, H) + (size_t)B * (size_t)(2L * T - 1) * (size_t)H * 64;
    return a16(floats * sizeof(float));
}

static int ra_fwd(const char* who, const void* q, const void* k, const void* v, long ld, const void* pos, const void* bias_u, const void* bias_v,
                  const unsigned char* pad_mask, float keep_scale, unsigned int thr, uint64_t seed, uint64_t offset, const uint64_t* rng_state,
                  void* out, float* lse, int act_dtype, int param_dtype, int B, int T, int H, dsp_stream_t stream)
{
    DSP_GATE(rng_state_gate(who, rng_state));
    const int rc = ra_check(who, act_dtype, param_dtype, B, T, H, ld);
    if (rc) return rc < 0 ? rc : DSP_OK;
    if (!q || !k || !v || !pos || !bias_u || !bias_v || !out || !lse || out == q || out == k || out == v || out == pos) {
        set_error("%s: null or aliased pointer", who); return DSP_EINVAL;
    }
    if (thr > (1u << 24)) { set_error("%s: thr %u above 2^24", who, thr); return DSP_EINVAL; }
    DSP_GATE(tensors16_gate(who, q, k, v, pos, bias_u, bias_v, out, lse));
    const unsigned grid = (unsigned)((long)B * H * ((T + 31) / 32));
    hipStream_t st = as_stream(stream);
    RA_DISPATCH(act_dtype, hipLaunchKernelGGL((ra_fwd_kernel<E>), dim3(grid), dim3(64), 0, st, (const E*)q, (const E*)k, (const E*)v, ld, (const E*)pos,
                                              bias_u, bias_v, param_dtype, pad_mask, keep_scale, (uint32_t)thr, seed, offset, rng_state, (E*)out, lse,
                                              T, H));
    return check_launch(who);
}

extern "C" int dsp_relpos_attention_train_fwd(const void* q, const void* k, const void* v, long ld, const void* pos, const void* bias_u,
                                              const void* bias_v, const unsigned char* pad_mask, float keep_scale, unsigned int thr, uint64_t seed,
                                              uint64_t offset, void* out, float* lse, int act_dtype, int param_dtype, int B, int T, int H,
                                              dsp_stream_t stream)
{
    return ra_fwd("relpos_attention_train_fwd", q, k, v, ld, pos, bias_u, bias_v, pad_mask, keep_scale, thr, seed, offset, nullptr, out, lse,
                  act_dtype, param_dtype, B, T, H, stream);
}

extern "C" int dsp_relpos_attention_train_fwd_state(const void* q, const void* k, const void* v, long ld, const void* pos, const void* bias_u,
                                                    const void* bias_v, const unsigned char* pad_mask, float keep_scale, unsigned int thr,
                                                    uint64_t seed, uint64_t offset, void* out, float* lse, int act_dtype, int param_dtype, int B,
                                                    int T, int H, const uint64_t* rng_state, dsp_stream_t stream)
{
    return ra_fwd("relpos_attention_train_fwd_state", q, k, v, ld, pos, bias_u, bias_v, pad_mask, keep_scale, thr, seed, offset, rng_state, out, lse,
                  act_dtype, param_dtype, B, T, H, stream);
}

static int ra_bwd(const char* who, const void* dout, const void* q, const void* k, const void* v, long ld, const void* pos, const void* bias_u,
                  const void* bias_v, const unsigned char* pad_mask, const void* out, const float* lse, float keep_scale, unsigned int thr,
                  uint64_t seed, uint64_t offset, const uint64_t* rng_state, void* dq, void* dk, void* dv, void* dpos, void* dbias_u, void* dbias_v,
                  void* workspace, size_t workspace_bytes, int act_dtype, int param_dtype, int B, int T, int H, dsp_stream_t stream)
{
    DSP_GATE(rng_state_gate(who, rng_state));
    const int rc = ra_check(who, act_dtype, param_dtype, B, T, H, ld);
    if (rc) return rc < 0 ? rc : DSP_OK;
    if (!dq && !dk && !dv && !dpos && !dbias_u && !dbias_v) return DSP_OK;
    if (!dout || !q || !k || !v || !pos || !bias_u || !bias_v || !out || !lse) { set_error("%s: null pointer", who); return DSP_EINVAL;}
    const void* ins[] = {dout, q, k, v, pos, bias_u, bias_v, out, lse, pad_mask};
    void* outs[] = {dq, dk, dv, dpos, dbias_u, dbias_v};
    DSP_GATE(alias_gate(who, outs, 6, ins, 10, "an output aliases an input", "two outputs alias"));
    if (thr > (1u << 24)) { set_error("%s: thr %u above 2^24", who, thr); return DSP_EINVAL; }
    DSP_GATE(tensors16_gate(who, dout, q, k, v, pos, bias_u, bias_v, out, lse, dq, dk, dv, dpos, dbias_u, dbias_v));
    if (dpos || dbias_u || dbias_v)
        DSP_GATE(workspace_gate(who, workspace, workspace_bytes, dsp_relpos_attention_train_workspace_bytes(B, T, H),
                                "dsp_relpos_attention_train_workspace_bytes"));
    const int nI = (T + 31) / 32, nR = (2 * T - 1 + 31) / 32, C = H * 64;
    float* part_u = (float*)workspace;
    float* part_v = part_u ? part_u + ra_part_bias_floats(B, T, H) : nullptr;
    float* part_pos = part_u ? part_v + ra_part_bias_floats(B, T, H) : nullptr;
    hipStream_t st = as_stream(stream);
#define RA_IN (const E*)dout, (const E*)q, (const E*)k, (const E*)v, ld, (const E*)pos, bias_u, bias_v, param_dtype, pad_mask, (const E*)out, lse, keep_scale, \
              (uint32_t)thr, seed, offset, rng_state
    if (dk || dv)
        RA_DISPATCH(act_dtype, hipLaunchKernelGGL((ra_bwd_kv_kernel<E>), dim3((unsigned)((long)B * H * nI)), dim3(64), 0, st, RA_IN, (E*)dk, (E*)dv, T, H));
    if (dq || dbias_u || dbias_v) {
        RA_DISPATCH(act_dtype, hipLaunchKernelGGL((ra_bwd_q_kernel<E>), dim3((unsigned)((long)B * H * nI)), dim3(64), 0, st, RA_IN, (E*)dq,
                                                  dbias_u ? part_u : (float*)nullptr, dbias_v ? part_v : (float*)nullptr, T, H));
        if (dbias_u || dbias_v)
            hipLaunchKernelGGL(ra_bias_merge_kernel, dim3((unsigned)((2 * C + 255) / 256)), dim3(256), 0, st, part_u, part_v, (long)B * nI, C, dbias_u, dbias_v,
                               param_dtype);
    }
    if (dpos) {
        const long n = (2L * T - 1) * C;
        RA_DISPATCH(act_dtype, hipLaunchKernelGGL((ra_bwd_pos_kernel<E>), dim3((unsigned)((long)B * H * nR)), dim3(64), 0, st, RA_IN, part_pos, T, H));
        RA_DISPATCH(act_dtype, hipLaunchKernelGGL((ra_pos_merge_kernel<E>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, part_pos, B, n, (E*)dpos));
    }
#undef RA_IN
    return check_launch(who);
}

extern "C" int dsp_relpos_attention_train_bwd(const void* dout, const void* q, const void* k, const void* v, long ld, const void* pos,
                                              const void* bias_u, const void* bias_v, const unsigned char* pad_mask, const void* out, const float* lse,
                                              float keep_scale, unsigned int thr, uint64_t seed, uint64_t offset, void* dq, void* dk, void* dv,
                                              void* dpos, void* dbias_u, void* dbias_v, void* workspace, size_t workspace_bytes, int act_dtype,
                                              int param_dtype, int B, int T, int H, dsp_stream_t stream)
{
    return ra_bwd("relpos_attention_train_bwd", dout, q, k, v, ld, pos, bias_u, bias_v, pad_mask, out, lse, keep_scale, thr, seed, offset, nullptr, dq,
                  dk, dv, dpos, dbias_u, dbias_v, workspace, workspace_bytes, act_dtype, param_dtype, B, T, H, stream);
}

extern "C" int dsp_relpos_attention_train_bwd_state(const void* dout, const void* q, const void* k, const void* v, long ld, const void* pos,
                                                    const void* bias_u, const void* bias_v, const unsigned char* pad_mask, const void* out,
                                                    const float* lse, float keep_scale, unsigned int thr, uint64_t seed, uint64_t offset, void* dq,
                                                    void* dk, void* dv, void* dpos, void* dbias_u, void* dbias_v, void* workspace,
                                                    size_t workspace_bytes, int act_dtype, int param_dtype, int B, int T, int H,
                                                    const uint64_t* rng_state, dsp_stream_t stream)
{
    return ra_bwd("relpos_attention_train_bwd_state", dout, q, k, v, ld, pos, bias_u, bias_v, pad_mask, out, lse, keep_scale, thr, seed, offset,
                  rng_state, dq, dk, dv, dpos, dbias_u, dbias_v, workspace, workspace_bytes, act_dtype, param_dtype, B, T, H, stream);
}
