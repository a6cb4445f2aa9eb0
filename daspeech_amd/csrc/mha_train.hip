// mha_train.hip — multi-head attention under autograd (the NAT decoder's self- and encoder attention, the FFT layers), gfx950, fp16 / bf16 data:
//     s(b,h,i,j) = q_i . k_j / 8      masked keys (pad_mask[b,j] != 0): -inf                                   (head width 64)
//     P = softmax_j(s)   lse = log sum_j exp s   A = keep ? P / (1-p) : 0   o_i = sum_j A_ij v_j
// and its backward (include/daspeech_decode.h: dsp_mha_train_fwd / _bwd).  q [B,N,H*64] with row stride ldq; k, v [B,M,H*64] with one common
// row stride ldkv; N and M independent.  No [B,H,N,M] tensor is written to global memory in either direction: the forward keeps o and lse,
// the backward recomputes P from q, k and lse.
//
// relpos_attention_train.hip without the position term, on its helpers (ra_frag.h) — and with the workgroup that file's measurements asked
// for: MH_WAVES = 4 waves, each OWNING 32 rows (the workgroup: 128), which share every streamed tile of 32 rows of the other side.
//   * what a wave owns stays in registers as matrix-core operands for the whole kernel (its q rows, q and dO rows, or k and v rows: lane l
//     holds row l & 31, channels 16 s + 8 (l >> 5) .. + 7 of k step s — the operand layout of ra_frag.h read straight from global memory);
//   * a streamed tile is staged ONCE for the four waves, one 16-byte load per thread and matrix, and the NEXT tile's loads are issued before
//     the current tile's products and written to LDS after them (mh_tile_load / the stores below);
//   * the first product of a tile is taken TRANSPOSED to what that file takes (S^T = K Q^T where a wave owns queries), so the owned row is on
//     the lane: the soft-max statistics, lse and D are one value a lane (two lanes a row, met by one shuffle), a lane's 16 score elements
//     are four whole Philox calls of the mask rule, and P / dS go from the accumulator straight into the next product's B operand
//     (mh_pack / mh_mma_acc: no LDS round trip), whose result — o, dq, dk, dv — is accumulated transposed and stored as rows;
//   * only the dk / dv pass, where the key is on the lane and the mask rule's four consecutive keys are on four lanes, shares a tile's
//     Philox calls through a per-wave 1 KiB of LDS (mh_wave_sync: the wave's own order is enough); a tile costs two workgroup barriers.
//   LDS: forward 9.5 KiB, D / dq pass 14 KiB, dk / dv pass 23.3 KiB.
//
// Backward, two owners (each recomputes P = exp(s - lse) and dS = P o (dO V^T o m - D) / 8 for the tiles it visits), in this order:
//   mh_bwd_q_kernel   a wave owns 32 queries:  D_i = sum_j (P o m)_ij (dO V^T)_ij (= dO_i . o_i, with o in fp32), then dq = dS K
//                                              streams the key tiles (k, v) twice; D [B,H,N] fp32 goes to the workspace
//   mh_bwd_kv_kernel  a wave owns 32 keys:     dV = (P o m)^T dO,  dK = dS^T Q        streams query tiles (q, dO, D, lse)
// No float atomics, no hand-off between workgroups (the second launch reads what the first one wrote): the same inputs give the same bits.
//
// The dropout mask is never stored: element e = ((b H + h) N + i) Mp + j, Mp = M rounded up to a multiple of 4, of the rule in philox.h.
#include "common.h"
#include "host_gates.h"
#include "philox.h"
#include "ra_frag.h"
#include "../../include/daspeech_decode.h"

namespace dsp {

constexpr int MH_WAVES = 4;                     // waves of a workgroup
constexpr int MH_THREADS = 64 * MH_WAVES;
constexpr int MH_OWN = 32 * MH_WAVES;           // rows a workgroup owns (DSP_MHA_TRAIN_OWN_ROWS)
// __launch_bounds__(MH_THREADS, 2): two waves per SIMD, so two workgroups of a CU overlap each other's barriers and staging
constexpr int MH_TILE = 32;                     // rows of a streamed tile (DSP_MHA_TRAIN_TILE_ROWS): 32 x 8 16-byte chunks, one per thread
static_assert(MH_THREADS == MH_TILE * 8, "one 16-byte chunk of a streamed tile per thread");
static_assert(MH_OWN == DSP_MHA_TRAIN_OWN_ROWS && MH_TILE == DSP_MHA_TRAIN_TILE_ROWS, "the header states the tiling");

// LDS written by some lanes of a wave and read by other lanes of the SAME wave: the wave's LDS operations execute in program order, so only
// the compiler has to be held to it
__device__ __forceinline__ void mh_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the 16-byte chunk of thread tid of the tile of rows row0 .. row0+31 (64 columns from src on): row row0 + (tid >> 3), columns 8 (tid & 7) .. + 7;
// rows from R on as zeros
template <typename E>
__device__ __forceinline__ uint4 mh_tile_load(const E* src, long ld, int row0, int R, int tid)
{
    const int row = row0 + (tid >> 3);
    return row < R ? *reinterpret_cast<const uint4*>(src + (long)row * ld + (tid & 7) * 8) : make_uint4(0u, 0u, 0u, 0u);
}
// that chunk into the image [32 rows][64 columns] ...
__device__ __forceinline__ void mh_tile_store(ra_u16* dst, uint4 u, int tid)
{
    *reinterpret_cast<uint4*>(dst + (tid >> 3) * RA_P64 + (tid & 7) * 8) = u;
}
// ... and into the image [64 columns][32 rows]
__device__ __forceinline__ void mh_tile_store_t(ra_u16* dst, uint4 u, int tid)
{
    const int rl = tid >> 3, c8 = (tid & 7) * 8;
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int x = 0; x < 4; ++x) {
        dst[(c8 + 2 * x) * RA_P32 + rl] = (ra_u16)(w[x] & 0xffffu);
        dst[(c8 + 2 * x + 1) * RA_P32 + rl] = (ra_u16)(w[x] >> 16);
    }
}

// the four operand fragments of the 32 rows from row0 on, straight from global memory (rows from R on as zeros)
template <typename E>
__device__ __forceinline__ void mh_frag_load(typename Ra<E>::V (&f)[4], const E* src, long ld, int row0, int R, int lane)
{
    const int row = row0 + (lane & 31), k0 = (lane >> 5) * 8;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        uint4 u = make_uint4(0u, 0u, 0u, 0u);
        if (row < R) u = *reinterpret_cast<const uint4*>(src + (long)row * ld + 16 * s + k0);
        __builtin_memcpy(&f[s], &u, 16);
    }
}
// acc += A . B^T over the 64 channels: A an LDS image [32][RA_P64], B the fragments a wave holds of its own rows
template <typename E>
__device__ __forceinline__ void mh_mma_rb(ra_acc& acc, const ra_u16* a, const typename Ra<E>::V (&b)[4], int lane)
{
    using V = typename Ra<E>::V;
#pragma unroll
    for (int s = 0; s < 4; ++s) acc = Ra<E>::mma(*reinterpret_cast<const V*>(a + (lane & 31) * RA_P64 + 16 * s + (lane >> 5) * 8), b[s], acc);
}

// A tile that a product has just left in registers (its column on the lane, its rows RA_ROW(reg, hi) in the registers) as the B operand of the
// NEXT product, with no trip through LDS: registers 8 s .. 8 s + 7 are k step s, so slot x of the lane's 8 is row 16 s + 4 hi + x (x < 4) or
// 16 s + 8 + 4 hi + (x - 4).  A contraction may visit its index in any order as long as both operands agree, so the A operand — an LDS image
// [32 rows][RA_P32] with the contracted index contiguous — is read in that order: two 8-byte reads instead of one of 16 bytes.
template <typename E>
__device__ __forceinline__ void mh_pack(typename Ra<E>::V (&b)[2], const float (&x)[16])
{
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        ra_u16 e[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) e[t] = Ra<E>::bits(x[8 * s + t]);
        __builtin_memcpy(&b[s], e, 16);
    }
}
template <typename E>
__device__ __forceinline__ void mh_mma_acc(ra_acc& acc, const ra_u16* a, const typename Ra<E>::V (&b)[2], int lane)
{
    using V = typename Ra<E>::V;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const ra_u16* row = a + (lane & 31) * RA_P32 + 16 * s + 4 * (lane >> 5);
        const uint2 lo = *reinterpret_cast<const uint2*>(row), up = *reinterpret_cast<const uint2*>(row + 8);
        const uint4 u = make_uint4(lo.x, lo.y, up.x, up.y);
        V va;
        __builtin_memcpy(&va, &u, 16);
        acc = Ra<E>::mma(va, b[s], acc);
    }
}

// bit r of the result: row r of the streamed tile (rows row0 .. row0 + 31 of R) is a key that counts (in range, not masked) — one byte per lane, one ballot
__device__ __forceinline__ uint32_t mh_valid_rows(const unsigned char* mrow, int row0, int R, int lane)
{
    const int j = row0 + (lane & 31);
    return (uint32_t)__ballot(j < R && !(mrow && mrow[j]));
}

// the keep bits of a lane's 16 elements where the QUERY is on the lane and the keys RA_ROW(reg, hi) of the tile are in the registers: registers
// 4 g .. 4 g + 3 are four consecutive keys from a multiple of 4 on, which is one Philox call of the rule (philox.h) — four calls a lane, nothing shared
__device__ __forceinline__ uint32_t mh_keep_bits(int b, int h, int H, int N, int Mp, int i, int j0, int hi, uint64_t seed, uint64_t offset, uint32_t thr)
{
    uint32_t bits = 0u;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        bool keep[4];
        keep_flags<4>(ra_elem(b, h, H, N, Mp, i, j0 + 8 * g + 4 * hi), seed, offset, thr, keep);
#pragma unroll
        for (int r = 0; r < 4; ++r) bits |= (keep[r] ? 1u : 0u) << (4 * g + r);
    }
    return bits;
}

// 64 channels of one row, which a lane holds transposed (channel 32 t + RA_ROW(reg, hi) in register reg of tile t), times f -> dst (the row's 64 channels)
template <typename E>
__device__ __forceinline__ void mh_store_row(E* dst, const ra_acc& t0, const ra_acc& t1, float f, int hi)
{
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float x0[4] = {t0[4 * g] * f, t0[4 * g + 1] * f, t0[4 * g + 2] * f, t0[4 * g + 3] * f};
        const float x1[4] = {t1[4 * g] * f, t1[4 * g + 1] * f, t1[4 * g + 2] * f, t1[4 * g + 3] * f};
        store_f<E, 4>(dst + 8 * g + 4 * hi, x0);
        store_f<E, 4>(dst + 32 + 8 * g + 4 * hi, x1);
    }
}

// ---------------------------------------------------------------- forward
// S^T = K Q^T: the wave's query il is on the lane (both halves of the wave hold the same 32 queries, each 16 of the tile's 32 keys), so the
// running maximum and sum of a row are one value a lane, and o is accumulated transposed (o^T = V^T P^T: channels in the registers), so the
// rescaling of a row is a lane's own factor.
template <typename E>
__global__ __launch_bounds__(MH_THREADS, 2) void mh_fwd_kernel(const E* __restrict__ q, long ldq, const E* __restrict__ k, const E* __restrict__ v, long ldkv,
                                                               const unsigned char* __restrict__ mask, float keep_scale, uint32_t thr, uint64_t seed,
                                                               uint64_t offset, const uint64_t* __restrict__ rng_state, E* __restrict__ out,
                                                               float* __restrict__ lse, int N, int M, int H)
{
    using V = typename Ra<E>::V;
    __shared__ __attribute__((aligned(16))) ra_u16 Ks[32 * RA_P64], Vt[64 * RA_P32];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, il = lane & 31, hi = lane >> 5;
    philox_stream(seed, offset, rng_state);
    const int nI = (N + MH_OWN - 1) / MH_OWN, C = H * 64, Mp = (M + 3) & ~3;
    const int ib = blockIdx.x % nI, bh = blockIdx.x / nI, h = bh % H, b = bh / H, i0 = ib * MH_OWN + wave * 32, i = i0 + il;
    const E* kb = k + (long)b * M * ldkv + h * 64;
    const E* vb = v + (long)b * M * ldkv + h * 64;
    const unsigned char* mrow = mask ? mask + (long)b * M : nullptr;
    const bool active = i0 < N;                                             // wave-uniform: a wave past the last row only helps staging
    V qf[4];
    mh_frag_load<E>(qf, q + (long)b * N * ldq + h * 64, ldq, i0, N, lane);
    float m = NEG_INF, l = 0.f;
    ra_acc o0 = {0}, o1 = {0};
    uint4 ku = mh_tile_load<E>(kb, ldkv, 0, M, tid), vu = mh_tile_load<E>(vb, ldkv, 0, M, tid);
#pragma unroll 1
    for (int j0 = 0; j0 < M; j0 += MH_TILE) {
        __syncthreads();                                                    // the previous tile has been read
        mh_tile_store(Ks, ku, tid);
        mh_tile_store_t(Vt, vu, tid);
        __syncthreads();
        if (j0 + MH_TILE < M) { ku = mh_tile_load<E>(kb, ldkv, j0 + MH_TILE, M, tid); vu = mh_tile_load<E>(vb, ldkv, j0 + MH_TILE, M, tid); }
        if (!active) continue;
        ra_acc sc = {0};
        mh_mma_rb<E>(sc, Ks, qf, lane);
        const uint32_t valid = mh_valid_rows(mrow, j0, M, lane);
        float p[16], mx = NEG_INF;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            p[reg] = (valid >> RA_ROW(reg, hi)) & 1u ? sc[reg] * 0.125f : NEG_INF;
            mx = fmaxf(mx, p[reg]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float mn = fmaxf(m, mx);
        const float ms = mn == NEG_INF ? 0.f : mn;                          // nothing but masked keys so far: every weight is 0
        const float a = expf(m - ms);
        float ps = 0.f;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) { p[reg] = expf(p[reg] - ms); ps += p[reg]; }
        l = fmaf(l, a, ps);                                                 // this half's 16 keys of every tile; the halves meet at the end
        m = mn;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) { o0[reg] *= a; o1[reg] *= a; }
        if (thr) {
            const uint32_t kept = mh_keep_bits(b, h, H, N, Mp, i, j0, hi, seed, offset, thr);
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) p[reg] = (kept >> reg) & 1u ? p[reg] : 0.f;
        }
        V pb[2];
        mh_pack<E>(pb, p);
        mh_mma_acc<E>(o0, Vt, pb, lane);
        mh_mma_acc<E>(o1, Vt + 32 * RA_P32, pb, lane);
    }
    if (!active) return;
    l += __shfl_xor(l, 32, 64);
    if (i < N) {
        mh_store_row<E>(out + ((long)b * N + i) * C + h * 64, o0, o1, (thr ? keep_scale : 1.f) / l, hi);     // every key masked: 0 * inf = NaN, as torch's soft-max
        if (hi == 0) lse[((long)b * H + h) * N + i] = m + logf(l);
    }
}

// ---------------------------------------------------------------- backward, a wave owns 32 queries: D, then dq
// Two walks over the key tiles, in the forward's orientation (query on the lane, dq accumulated transposed).  The first forms
// D_i = sum_j (P o m)_ij dP_ij — which is dO_i . o_i with o in fp32: the product with the ROUNDED o of the forward costs a row whose P sits on
// one key its cancellation (dS = P (dP - D) is zero there), and in bf16 that alone is several times the error of torch's lines — keeps it in
// a register and writes it to dsum [B,H,N] for the dk / dv pass.  The second forms dS and dq (dq == nullptr: the first walk only).
template <typename E>
__global__ __launch_bounds__(MH_THREADS, 2) void mh_bwd_q_kernel(const E* __restrict__ dout, const E* __restrict__ q, long ldq, const E* __restrict__ k,
                                                                 const E* __restrict__ v, long ldkv, const unsigned char* __restrict__ mask,
                                                                 const float* __restrict__ lse, float keep_scale, uint32_t thr, uint64_t seed,
                                                                 uint64_t offset, const uint64_t* __restrict__ rng_state, float* __restrict__ dsum,
                                                                 E* __restrict__ dq, int N, int M, int H)
{
    using V = typename Ra<E>::V;
    __shared__ __attribute__((aligned(16))) ra_u16 Ks[32 * RA_P64], Vs[32 * RA_P64], KT[64 * RA_P32];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, il = lane & 31, hi = lane >> 5;
    philox_stream(seed, offset, rng_state);
    const int nI = (N + MH_OWN - 1) / MH_OWN, C = H * 64, Mp = (M + 3) & ~3;
    const int ib = blockIdx.x % nI, bh = blockIdx.x / nI, h = bh % H, b = bh / H, i0 = ib * MH_OWN + wave * 32, i = i0 + il;
    const E* kb = k + (long)b * M * ldkv + h * 64;
    const E* vb = v + (long)b * M * ldkv + h * 64;
    const unsigned char* mrow = mask ? mask + (long)b * M : nullptr;
    const bool active = i0 < N;
    const float ks = thr ? keep_scale : 1.f;
    V qf[4], gf[4];
    mh_frag_load<E>(qf, q + (long)b * N * ldq + h * 64, ldq, i0, N, lane);
    mh_frag_load<E>(gf, dout + (long)b * N * C + h * 64, C, i0, N, lane);
    const float L = i < N ? lse[((long)b * H + h) * N + i] : __builtin_huge_valf();      // rows past N: +inf, so that P = 0 there
    float D = 0.f;
    ra_acc a0 = {0}, a1 = {0};
    const int passes = dq ? 2 : 1;                                          // workgroup-uniform
#pragma unroll 1
    for (int pass = 0; pass < passes; ++pass) {
        uint4 ku = mh_tile_load<E>(kb, ldkv, 0, M, tid), vu = mh_tile_load<E>(vb, ldkv, 0, M, tid);
#pragma unroll 1
        for (int j0 = 0; j0 < M; j0 += MH_TILE) {
            __syncthreads();                                                // the previous tile has been read
            mh_tile_store(Ks, ku, tid);
            mh_tile_store(Vs, vu, tid);
            if (pass) mh_tile_store_t(KT, ku, tid);
            __syncthreads();
            if (j0 + MH_TILE < M) { ku = mh_tile_load<E>(kb, ldkv, j0 + MH_TILE, M, tid); vu = mh_tile_load<E>(vb, ldkv, j0 + MH_TILE, M, tid); }
            if (!active) continue;
            ra_acc sc = {0}, dp = {0};
            mh_mma_rb<E>(sc, Ks, qf, lane);
            mh_mma_rb<E>(dp, Vs, gf, lane);
            const uint32_t valid = mh_valid_rows(mrow, j0, M, lane);
            const uint32_t kept = thr ? mh_keep_bits(b, h, H, N, Mp, i, j0, hi, seed, offset, thr) : 0xffffu;
            if (pass == 0) {
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const float p = expf(((valid >> RA_ROW(reg, hi)) & 1u ? sc[reg] * 0.125f : NEG_INF) - L);
                    D = fmaf((kept >> reg) & 1u ? p : 0.f, dp[reg], D);   // this half's 16 keys of every tile; the halves meet below
                }
                continue;
            }
            float ds[16];
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const float p = expf(((valid >> RA_ROW(reg, hi)) & 1u ? sc[reg] * 0.125f : NEG_INF) - L);
                ds[reg] = p * (dp[reg] * ((kept >> reg) & 1u ? ks : 0.f) - D) * 0.125f;
            }
            V db[2];
            mh_pack<E>(db, ds);
            mh_mma_acc<E>(a0, KT, db, lane);
            mh_mma_acc<E>(a1, KT + 32 * RA_P32, db, lane);
        }
        if (pass == 0 && active) {
            D = ks * (D + __shfl_xor(D, 32, 64));
            if (hi == 0 && i < N) dsum[((long)b * H + h) * N + i] = D;
        }
    }
    if (active && dq && i < N) mh_store_row<E>(dq + ((long)b * N + i) * C + h * 64, a0, a1, 1.f, hi);
}

// the keep flags of a wave's tile where the KEY is on the lane (queries i0 .. i0+31 in the registers, keys j0 .. j0+31; j0 is a multiple of 32): a
// lane's registers are 16 different queries, one element of a Philox call each, so the tile's 32 x 8 calls are shared out and the flags pass as
// bytes kb[32][32] through the wave's own 1 KiB; a lane reads the flag of register reg at kb[RA_ROW(reg, lane >> 5) * 32 + (lane & 31)]
__device__ __forceinline__ void mh_keep_fill(unsigned char* kb, int b, int h, int H, int N, int Mp, int i0, int j0, uint64_t seed, uint64_t offset,
                                             uint32_t thr, int lane)
{
    ra_keep_fill(kb, b, h, H, N, Mp, i0, j0, seed, offset, thr, lane);
    mh_wave_sync();
}

// ---------------------------------------------------------------- backward, a wave owns 32 keys: dK, dV
// S = Q K^T with the wave's key on the lane and the tile's queries in the registers; dV and dK are accumulated transposed (dV^T = dO^T (P o m),
// dK^T = Q^T dS), P o keep and dS going from the accumulator layout straight into the operand.
template <typename E>
__global__ __launch_bounds__(MH_THREADS, 2) void mh_bwd_kv_kernel(const E* __restrict__ dout, const E* __restrict__ q, long ldq, const E* __restrict__ k,
                                                                  const E* __restrict__ v, long ldkv, const unsigned char* __restrict__ mask,
                                                                  const float* __restrict__ lse, const float* __restrict__ dsum, float keep_scale,
                                                                  uint32_t thr, uint64_t seed, uint64_t offset, const uint64_t* __restrict__ rng_state,
                                                                  E* __restrict__ dk, E* __restrict__ dv, int N, int M, int H)
{
    using V = typename Ra<E>::V;
    __shared__ __attribute__((aligned(16))) ra_u16 Qs[32 * RA_P64], dOs[32 * RA_P64], QT[64 * RA_P32], dOT[64 * RA_P32];
    __shared__ __attribute__((aligned(16))) unsigned char kbs[MH_WAVES][1024];
    __shared__ float Dl[32], Ll[32];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, jl = lane & 31, hi = lane >> 5;
    philox_stream(seed, offset, rng_state);
    const int nJ = (M + MH_OWN - 1) / MH_OWN, C = H * 64, Mp = (M + 3) & ~3;
    const int jb = blockIdx.x % nJ, bh = blockIdx.x / nJ, h = bh % H, b = bh / H, j0 = jb * MH_OWN + wave * 32, j = j0 + jl;
    const E* qb = q + (long)b * N * ldq + h * 64;
    const E* gb = dout + (long)b * N * C + h * 64;
    const float* lb = lse + ((long)b * H + h) * N;
    const float* db = dsum + ((long)b * H + h) * N;
    const bool active = j0 < M;
    V kfr[4], vfr[4];
    mh_frag_load<E>(kfr, k + (long)b * M * ldkv + h * 64, ldkv, j0, M, lane);
    mh_frag_load<E>(vfr, v + (long)b * M * ldkv + h * 64, ldkv, j0, M, lane);
    const bool ok = j < M && !(mask && mask[(long)b * M + j]);
    ra_acc k0 = {0}, k1 = {0}, v0 = {0}, v1 = {0};
    const float ks = thr ? keep_scale : 1.f;
    const int rl = tid >> 3;                                                // the row of the streamed tile this thread stages
    uint4 qu = mh_tile_load<E>(qb, ldq, 0, N, tid), gu = mh_tile_load<E>(gb, C, 0, N, tid);
    // lse and D of row rl of the tile (rows past N: lse = +inf, so that P = 0 there)
    float lu = rl < N ? lb[rl] : __builtin_huge_valf(), du = rl < N ? db[rl] : 0.f;
#pragma unroll 1
    for (int i0 = 0; i0 < N; i0 += MH_TILE) {
        __syncthreads();                                                    // the previous tile has been read
        mh_tile_store(Qs, qu, tid);
        mh_tile_store_t(QT, qu, tid);
        mh_tile_store(dOs, gu, tid);
        mh_tile_store_t(dOT, gu, tid);
        if ((tid & 7) == 0) { Dl[rl] = du; Ll[rl] = lu; }
        __syncthreads();
        if (i0 + MH_TILE < N) {
            const int nx = i0 + MH_TILE;
            qu = mh_tile_load<E>(qb, ldq, nx, N, tid); gu = mh_tile_load<E>(gb, C, nx, N, tid);
            lu = nx + rl < N ? lb[nx + rl] : __builtin_huge_valf();
            du = nx + rl < N ? db[nx + rl] : 0.f;
        }
        if (!active) continue;
        ra_acc sc = {0}, dp = {0};
        mh_mma_rb<E>(sc, Qs, kfr, lane);
        mh_mma_rb<E>(dp, dOs, vfr, lane);
        const unsigned char* kf = kbs[wave] + hi * 128 + jl;               // RA_ROW(reg, hi) * 32 + jl = RA_ROW(reg, 0) * 32 + this
        if (thr) mh_keep_fill(kbs[wave], b, h, H, N, Mp, i0, j0, seed, offset, thr, lane);
        float pm[16], ds[16];
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int il = RA_ROW(reg, hi);
            const float p = expf((ok ? sc[reg] * 0.125f : NEG_INF) - Ll[il]);
            const float f = thr && !kf[RA_ROW(reg, 0) * 32] ? 0.f : 1.f;
            pm[reg] = p * f;
            ds[reg] = p * (dp[reg] * f * ks - Dl[il]) * 0.125f;
        }
        V pb[2], sb[2];
        mh_pack<E>(pb, pm);
        mh_pack<E>(sb, ds);
        mh_mma_acc<E>(v0, dOT, pb, lane);
        mh_mma_acc<E>(v1, dOT + 32 * RA_P32, pb, lane);
        mh_mma_acc<E>(k0, QT, sb, lane);
        mh_mma_acc<E>(k1, QT + 32 * RA_P32, sb, lane);
    }
    if (!active || j >= M) return;
    const long at = ((long)b * M + j) * C + h * 64;
    if (dk) mh_store_row<E>(dk + at, k0, k1, 1.f, hi);
    if (dv) mh_store_row<E>(dv + at, v0, v1, ks, hi);
}

// what the entry points check; 1: nothing to do (B == 0), 0: go on, < 0: refused
static int mh_check(const char* who, int act_dtype, int B, int N, int M, int H, long ldq, long ldkv, unsigned int thr)
{
    if (act_dtype != DSP_F16 && act_dtype != DSP_BF16) {
        set_error("%s: dtype code %d (q, k, v, out and their gradients: fp16 or bf16)", who, act_dtype);
        return DSP_EINVAL;
    }
    if (B < 0 || N < 1 || N > DSP_MHA_TRAIN_MAX_LEN || M < 1 || M > DSP_MHA_TRAIN_MAX_LEN || H < 1 || H > 1024 || ldq < (long)H * 64 || (ldq % 8) ||
        ldkv < (long)H * 64 || (ldkv % 8) || (long)B * H * ((DSP_MHA_TRAIN_MAX_LEN + MH_OWN - 1) / MH_OWN) > (1L << 30)) {
        set_error("%s: bad sizes B=%d N=%d M=%d H=%d ldq=%ld ldkv=%ld (1 <= N, M <= %d, 1 <= H <= 1024, strides >= 64 H and multiples of 8, B H <= 2^25)", who, B, N,
                  M, H, ldq, ldkv, DSP_MHA_TRAIN_MAX_LEN);
        return DSP_EINVAL;
    }
    if (thr > (1u << 24)) { set_error("%s: thr %u above 2^24", who, thr); return DSP_EINVAL; }
    return B == 0 ? 1 : 0;
}

}  // namespace dsp

using namespace dsp;

#define MH_DISPATCH(dtype, ...) DSP_DISPATCH_ELEM_16(dtype, E, __VA_ARGS__)

static int mh_fwd(const char* who, const void* q, long ldq, const void* k, const void* v, long ldkv, const unsigned char* pad_mask, float keep_scale,
                  unsigned int thr, uint64_t seed, uint64_t offset, const uint64_t* rng_state, void* out, float* lse, int act_dtype, int B, int N,
                  int M, int H, dsp_stream_t stream)
{
    DSP_GATE(rng_state_gate(who, rng_state));
    const int rc = mh_check(who, act_dtype, B, N, M, H, ldq, ldkv, thr);
    if (rc) return rc < 0 ? rc : DSP_OK;
    if (!q || !k || !v || !out || !lse || out == q || out == k || out == v || (const void*)lse == q || (const void*)lse == k || (const void*)lse == v ||
        (const void*)lse == out) {
        set_error("%s: null or aliased pointer", who); return DSP_EINVAL;
    }
    DSP_GATE(tensors16_gate(who, q, k, v, out, lse));
    const unsigned grid = (unsigned)((long)B * H * ((N + MH_OWN - 1) / MH_OWN));
    hipStream_t st = as_stream(stream);
    MH_DISPATCH(act_dtype, hipLaunchKernelGGL((mh_fwd_kernel<E>), dim3(grid), dim3(MH_THREADS), 0, st, (const E*)q, ldq, (const E*)k, (const E*)v, ldkv, pad_mask,
                                              keep_scale, (uint32_t)thr, seed, offset, rng_state, (E*)out, lse, N, M, H));
    return check_launch(who);
}

extern "C" int dsp_mha_train_fwd(const void* q, long ldq, const void* k, const void* v, long ldkv, const unsigned char* pad_mask, float keep_scale,
                                 unsigned int thr, uint64_t seed, uint64_t offset, void* out, float* lse, int act_dtype, int B, int N, int M, int H,
                                 dsp_stream_t stream)
{
    return mh_fwd("mha_train_fwd", q, ldq, k, v, ldkv, pad_mask, keep_scale, thr, seed, offset, nullptr, out, lse, act_dtype, B, N, M, H, stream);
}

extern "C" int dsp_mha_train_fwd_state(const void* q, long ldq, const void* k, const void* v, long ldkv, const unsigned char* pad_mask,
                                       float keep_scale, unsigned int thr, uint64_t seed, uint64_t offset, void* out, float* lse, int act_dtype,
                                       int B, int N, int M, int H, const uint64_t* rng_state, dsp_stream_t stream)
{
    return mh_fwd("mha_train_fwd_state", q, ldq, k, v, ldkv, pad_mask, keep_scale, thr, seed, offset, rng_state, out, lse, act_dtype, B, N, M, H,
                  stream);
}

extern "C" size_t dsp_mha_train_workspace_bytes(int B, int N, int M, int H)
{
    if (B <= 0 || N <= 0 || M <= 0 || H <= 0) return 0;
    return a16((size_t)B * (size_t)H * (size_t)N * sizeof(float));      // D [B,H,N]
}

static int mh_bwd(const char* who, const void* dout, const void* q, long ldq, const void* k, const void* v, long ldkv, const unsigned char* pad_mask,
                  const float* lse, float keep_scale, unsigned int thr, uint64_t seed, uint64_t offset, const uint64_t* rng_state, void* dq,
                  void* dk, void* dv, void* workspace, size_t workspace_bytes, int act_dtype, int B, int N, int M, int H, dsp_stream_t stream)
{
    DSP_GATE(rng_state_gate(who, rng_state));
    const int rc = mh_check(who, act_dtype, B, N, M, H, ldq, ldkv, thr);
    if (rc) return rc < 0 ? rc : DSP_OK;
    if (!dq && !dk && !dv) return DSP_OK;
    if (!dout || !q || !k || !v || !lse) { set_error("%s: null pointer", who); return DSP_EINVAL; }
    const void* ins[] = {dout, q, k, v, lse, pad_mask};
    void* outs[] = {dq, dk, dv, workspace};
    DSP_GATE(alias_gate(who, outs, 4, ins, 6, "an output aliases an input", "two outputs alias"));
    DSP_GATE(tensors16_gate(who, dout, q, k, v, lse, dq, dk, dv));
    DSP_GATE(workspace_gate(who, workspace, workspace_bytes, dsp_mha_train_workspace_bytes(B, N, M, H), "dsp_mha_train_workspace_bytes"));
    float* dsum = (float*)workspace;
    hipStream_t st = as_stream(stream);
#define MH_IN (const E*)dout, (const E*)q, ldq, (const E*)k, (const E*)v, ldkv, pad_mask, lse
    // the owner of the queries first: it forms D for both (without dq: its first walk only)
    MH_DISPATCH(act_dtype, hipLaunchKernelGGL((mh_bwd_q_kernel<E>), dim3((unsigned)((long)B * H * ((N + MH_OWN - 1) / MH_OWN))), dim3(MH_THREADS), 0, st, MH_IN,
                                              keep_scale, (uint32_t)thr, seed, offset, rng_state, dsum, (E*)dq, N, M, H));
    if (dk || dv)
        MH_DISPATCH(act_dtype, hipLaunchKernelGGL((mh_bwd_kv_kernel<E>), dim3((unsigned)((long)B * H * ((M + MH_OWN - 1) / MH_OWN))), dim3(MH_THREADS), 0, st, MH_IN,
                                                  (const float*)dsum, keep_scale, (uint32_t)thr, seed, offset, rng_state, (E*)dk, (E*)dv, N, M,
                                                  H));
#undef MH_IN
    return check_launch(who);
}

extern "C" int dsp_mha_train_bwd(const void* dout, const void* q, long ldq, const void* k, const void* v, long ldkv, const unsigned char* pad_mask,
                                 const float* lse, float keep_scale, unsigned int thr, uint64_t seed, uint64_t offset, void* dq, void* dk, void* dv,
                                 void* workspace, size_t workspace_bytes, int act_dtype, int B, int N, int M, int H, dsp_stream_t stream)
{
    return mh_bwd("mha_train_bwd", dout, q, ldq, k, v, ldkv, pad_mask, lse, keep_scale, thr, seed, offset, nullptr, dq, dk, dv, workspace,
                  workspace_bytes, act_dtype, B, N, M, H, stream);
}

extern "C" int dsp_mha_train_bwd_state(const void* dout, const void* q, long ldq, const void* k, const void* v, long ldkv,
                                       const unsigned char* pad_mask, const float* lse, float keep_scale, unsigned int thr, uint64_t seed,
                                       uint64_t offset, void* dq, void* dk, void* dv, void* workspace, size_t workspace_bytes, int act_dtype, int B,
                                       int N, int M, int H, const uint64_t* rng_state, dsp_stream_t stream)
{
    return mh_bwd("mha_train_bwd_state", dout, q, ldq, k, v, ldkv, pad_mask, lse, keep_scale, thr, seed, offset, rng_state, dq, dk, dv, workspace,
                  workspace_bytes, act_dtype, B, N, M, H, stream);
}
