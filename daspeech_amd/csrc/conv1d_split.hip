// conv1d_split.hip — fp32-accurate Conv1d on the fp16 matrix cores ("3 x fp16" split), for the FastSpeech2 FFT feed-forward
// (fairseq/models/text_to_speech/fastspeech2.py:42-63 PositionwiseFeedForward: Conv1d(256,1024,9) - ReLU - Conv1d(1024,256,9)).
//
// MIOpen serves these fp32 convolutions at 60-70 TFLOP/s (1.0 / 1.2 ms each at B=32 x 483 frames: 9 of the 41 ms of the S2ST
// pipeline).  The mel tolerance (1e-4) rules out plain fp16 operands, but not the matrix cores: with
//     x = xh + xl * 2^-11,  w = wh + wl * 2^-11      (xh = fp16(x), xl = fp16((x - xh) * 2^11); same for w)
// the three products  xh.wh,  xh.wl,  xl.wh  are EXACT in the fp32 accumulator (11 x 11 significant bits) and the dropped xl.wl term
// is 2^-22 relative: fp32-GEMM accuracy at a third of the fp16 MFMA rate.  The lo parts carry their own 2^11 scale so that they live
// in the normal fp16 range; their products go to a second accumulator that is folded in with 2^-11 at the end.
//   x [B,T,CI] fp32 channels-last (row stride ldx), taps k with shift k - (K-1)/2 ("same" padding), weights pre-split and stored in
//   MFMA fragment order (dsp_conv1d_split_pack), out [B,T,M] fp32 = [out +] bias + conv, optional ReLU.
#include "common.h"
#include "split_frag.h"
#include "split_operand.h"
#include <stdlib.h>
#include "../../include/daspeech_decode.h"

namespace dsp {

typedef _Float16 cs_h8 __attribute__((ext_vector_type(8)));
typedef float cs_f4 __attribute__((ext_vector_type(4)));

struct CsParams {
    const float* x; const _Float16* wh; const _Float16* wl; const float* bias; float* out;
    int B, T, M, ntaps; long ldx, ldo;
    int relu, accumulate;          // relu: activation after the bias — 0 none, 1 ReLU, 2 SiLU, 3 GELU(erf)
    int nslices; long wslice;      // the input is nslices x CI channels wide; slice s uses weights + s * wslice (halves)
    const float* res; long ldr; float alpha;      // out = res + alpha * act(bias + conv)   (res may be NULL: out = alpha * act(...))
    const float* ln_w; const float* ln_b; float ln_eps;   // LayerNorm of the input rows while they are staged (256-channel one-tap layers: the row sits in half a wave)
    int kparts, tap_groups; float* part;          // split-K: kparts = nslices * tap_groups workgroups per output tile, raw partial sums to part [kparts][B][T][M]
    const int* lens; int slack;                   // ragged batch: rows >= lens[b] + slack of sample b are padding nobody reads — their
                                                  // tiles are not computed, the output rows are written as zeros
    int mper;                                     // output tiles per workgroup: blockIdx.y owns tiles [y * mper, (y + 1) * mper) of the row tile it
};                                                // staged ONCE (cs_plan; 1 for multi-slice and split-K launches)

template <int CI, int MT, int NT, int WM, int WN>
__global__ __launch_bounds__(WM * WN * 64) void conv1d_split_kernel(CsParams p)
{
    extern __shared__ __attribute__((aligned(16))) char cs_smem[];
    constexpr int CH = CI / 8, NC = CI / 32;
    constexpr int MI = MT / WM / 16, NI = NT / WN / 16;
    constexpr int NTH = WM * WN * 64;                     // 8 waves, or 16 (r05: four waves per SIMD under one resident workgroup)
    static_assert((WM * WN == 8 || WM * WN == 16) && MI >= 1 && NI >= 1, "8 or 16 waves");
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // (a scalar: wm, wn, the weight pointers stay out of the VGPRs)
    const int wm = wave % WM, wn = wave / WM;
    const int lr = lane & 15, lk = lane >> 4;
    const int kp = p.kparts > 1 ? (int)(blockIdx.y % p.kparts) : 0;
    const int b = blockIdx.z, t0 = blockIdx.x * NT;
    // the workgroup's output tiles m_begin .. m_end - 1: the staged rows serve all of them
    const int m_begin = p.kparts > 1 ? (int)(blockIdx.y / p.kparts) : (int)blockIdx.y * p.mper;
    const int m_end = min(m_begin + (p.kparts > 1 ? 1 : p.mper), (p.M + MT - 1) / MT);
    if (p.lens && t0 >= p.lens[b] + p.slack) {          // a tile of padding rows (block-uniform): zeros, so that they stay finite
        if (p.accumulate) return;
        const int m0 = m_begin * MT;
        const int cw = min((m_end - m_begin) * MT, p.M - m0) >> 2;      // float4 columns of this range of tiles
        const int rows = min(NT, p.T - t0);
        float* dst = p.kparts > 1 ? p.part + ((size_t)kp * p.B + b) * p.T * p.M : p.out + (size_t)b * p.T * p.ldo;     // split-K: the partial sums are zero
        const size_t ld = p.kparts > 1 ? (size_t)p.M : (size_t)p.ldo;
        for (int e = tid; e < rows * cw; e += NTH) {
            const int r = e / cw, c4 = e - r * cw;
            *reinterpret_cast<float4*>(dst + (size_t)(t0 + r) * ld + m0 + c4 * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        return;
    }
    const int P = (p.ntaps - 1) / 2;
    const int R = NT + p.ntaps - 1;
    char* th = cs_smem;                                   // hi tile  [R][CI] halves, 16-byte chunks XOR-swizzled
    char* tl = cs_smem + (size_t)R * CI * 2;              // lo tile
    const float* X = p.x + (size_t)b * p.T * p.ldx;

    const int tl_base = wn * (NI * 16);
    const int Mt = (p.M + 15) >> 4;
    using BF = SplitBFrag<CI>;
    const uint32_t lane_off = (uint32_t)lane * 16u;
    const int row_l = tl_base + lr;                       // the lane's row of column tile 0, before the tap's shift
    // split-K: this workgroup owns ONE input slice and one group of taps (short sequences: a 1024 -> 256, K = 9 layer on 61 positions
    // is 64 workgroups of 288 K-steps otherwise); the partial sums meet in cs_reduce_kernel
    int sl_lo = 0, sl_hi = p.nslices, k_lo = 0, k_hi = p.ntaps;
    if (p.kparts > 1) {
        const int tpg = (p.ntaps + p.tap_groups - 1) / p.tap_groups;
        sl_lo = kp / p.tap_groups; sl_hi = sl_lo + 1;
        k_lo = (kp % p.tap_groups) * tpg; k_hi = min(p.ntaps, k_lo + tpg);
    }
    const int sb = k_lo * NC, nsteps = (k_hi - k_lo) * NC;
    // ---- the output tiles of this workgroup, one after the other.  More than one only where the staged rows are the whole reduction
    //      (one slice, no split-K): they are staged before the first tile and are read-only from that barrier on, so every later tile
    //      starts from zero accumulators, runs the K loop from its own weight fragments and leaves through the epilogue, without a barrier.
    for (int mi = m_begin; mi < m_end; ++mi) {
    const int co_base = mi * MT + wm * (MI * 16);
    const int tile0 = co_base >> 4;
    cs_f4 acc0[MI][NI], acc1[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) { acc0[i][j] = (cs_f4){0.f, 0.f, 0.f, 0.f}; acc1[i][j] = (cs_f4){0.f, 0.f, 0.f, 0.f}; }
    // input slices of CI channels one after the other through the same LDS tiles; the accumulators stay in registers
    for (int sl = sl_lo; sl < sl_hi; ++sl) {
    const float* Xs = X + (size_t)sl * CI;
    const _Float16* WH = p.wh + (size_t)sl * p.wslice;
    const _Float16* WL = p.wl + (size_t)sl * p.wslice;
    if (mi == m_begin) {                                  // (several slices: one output tile)
    if (sl > sl_lo) __syncthreads();                      // every wave is done with the previous slice's tiles
    // ---- stage: rows t0-P .. t0+NT-1+P, zero outside [0,T); split into hi / lo*2^11.  All of a lane's row chunks (R*CH/512 <= 10) are
    //      requested together, UNCONDITIONALLY from a clamped row: predicated loads wait for one another (r01h s_memtime accounting: 10 k
    //      cycles of staging per slice, eight dependent round trips, against 17 k cycles of MFMA loop) ----
    {
        constexpr int CS_U = 4;                                // 8 sixteen-byte requests per lane in flight (more spills: 256 VGPRs)
        const int n = R * CH;
        for (int e0 = tid; e0 < n; e0 += NTH * CS_U) {
            float4 va[CS_U], vc[CS_U];
            bool ok[CS_U];
#pragma unroll
            for (int u = 0; u < CS_U; ++u) {
                const int e = e0 + u * NTH, ec = e < n ? e : 0;
                const int row = ec / CH, ch = ec - row * CH;
                const int tg = t0 - P + row;
                ok[u] = e < n && tg >= 0 && tg < p.T;
                const float* src = Xs + (size_t)(ok[u] ? tg : 0) * p.ldx + ch * 8;
                va[u] = *reinterpret_cast<const float4*>(src);
                vc[u] = *reinterpret_cast<const float4*>(src + 4);
            }
#pragma unroll
            for (int u = 0; u < CS_U; ++u) {
                const int e = e0 + u * NTH;
                if (e < n) {
                    const int row = e / CH, ch = e - row * CH;
                    float f[8] = {va[u].x, va[u].y, va[u].z, va[u].w, vc[u].x, vc[u].y, vc[u].z, vc[u].w};
                    if constexpr (CI == 256 && NT == 64 && MT == 256) {
                        if (p.ln_w) {                        // one tap, one slice (host-checked): every lane is here; the row's 32 chunks are 32 consecutive lanes
                            float s1 = 0.f;
#pragma unroll
                            for (int i = 0; i < 8; ++i) s1 += f[i];
#pragma unroll
                            for (int o = 16; o > 0; o >>= 1) s1 += __shfl_xor(s1, o, 64);
                            const float mean = s1 * (1.f / CI);
                            float q = 0.f;
#pragma unroll
                            for (int i = 0; i < 8; ++i) { const float d = f[i] - mean; q += d * d; }
#pragma unroll
                            for (int o = 16; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
                            const float rstd = rsqrtf(q * (1.f / CI) + p.ln_eps);
                            const float4 w0 = *reinterpret_cast<const float4*>(p.ln_w + ch * 8), w1 = *reinterpret_cast<const float4*>(p.ln_w + ch * 8 + 4);
                            const float4 b0 = *reinterpret_cast<const float4*>(p.ln_b + ch * 8), b1 = *reinterpret_cast<const float4*>(p.ln_b + ch * 8 + 4);
                            const float w8[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w}, b8[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
                            for (int i = 0; i < 8; ++i) f[i] = (f[i] - mean) * rstd * w8[i] + b8[i];
                        }
                    }
                    cs_h8 vh, vl;
#pragma unroll
                    for (int i = 0; i < 8; ++i) split_hi_lo(ok[u] ? f[i] : 0.f, vh, vl, i);
                    const size_t o = ((size_t)row * CH + split_swz<CI>(row, ch)) * 16;
                    *reinterpret_cast<cs_h8*>(th + o) = vh;
                    *reinterpret_cast<cs_h8*>(tl + o) = vl;
                }
            }
        }
    }
    __syncthreads();
    }

    // addresses: split_frag.h.  Weights: scalar pointers to the wave's M tiles of step sb, one step's stride apart; load_a takes the steps in
    // order.  (A tile past M reads tile 0: its rows are never stored.)
    SplitWeights wq = {reinterpret_cast<const char*>(WH) + (size_t)sb * Mt * 1024, reinterpret_cast<const char*>(WL) + (size_t)sb * Mt * 1024, (uint32_t)Mt * 1024u};
    uint32_t toff[MI];
#pragma unroll
    for (int i = 0; i < MI; ++i) toff[i] = (tile0 + i < Mt ? (uint32_t)(tile0 + i) : 0u) * 1024u;
    auto load_a = [&](cs_h8 (&ah)[MI], cs_h8 (&al)[MI]) {
        const uint32_t lo16 = split_keep(lane_off);
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            ah[i] = *reinterpret_cast<const cs_h8*>(wq.hi + toff[i] + lo16);
            al[i] = *reinterpret_cast<const cs_h8*>(wq.lo + toff[i] + lo16);
        }
        wq.next();
    };
    uint32_t tap = 0;                                     // BF::tap_base of the current tap: set at its first step
    auto do_step = [&](int step, const cs_h8 (&ah)[MI], const cs_h8 (&al)[MI]) {
        const int k = step / NC, c = step - k * NC;
        if (c == 0) tap = split_keep(BF::tap_base(row_l + k, lk));
        const uint32_t o = BF::step(tap, c);
        const char* ph = th + o;
        const char* pl = tl + o;
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            const cs_h8 bh = *reinterpret_cast<const cs_h8*>(ph + j * BF::TILE_BYTES);
            const cs_h8 bl = *reinterpret_cast<const cs_h8*>(pl + j * BF::TILE_BYTES);
#pragma unroll
            for (int i = 0; i < MI; ++i) {
                acc0[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], bh, acc0[i][j], 0, 0, 0);
                acc1[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], bl, acc1[i][j], 0, 0, 0);
                acc1[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[i], bh, acc1[i][j], 0, 0, 0);
            }
        }
    };
    // 3-deep register ring of weight fragments: a request is two steps (>= 48 MFMAs per wave) ahead of its use
    cs_h8 ah0[MI], al0[MI], ah1[MI], al1[MI], ah2[MI], al2[MI];
    if (nsteps > 0) load_a(ah0, al0);
    if (nsteps > 1) load_a(ah1, al1);
    for (int step = 0; step < nsteps; step += 3) {
        if (step + 2 < nsteps) load_a(ah2, al2);
        do_step(sb + step, ah0, al0);
        if (step + 1 < nsteps) {
            if (step + 3 < nsteps) load_a(ah0, al0);
            do_step(sb + step + 1, ah1, al1);
        }
        if (step + 2 < nsteps) {
            if (step + 4 < nsteps) load_a(ah1, al1);
            do_step(sb + step + 2, ah2, al2);
        }
    }

    }     // slices

    int t0i = t0;                                         // (opaque: the rows' output addresses are formed here, per tile, not kept across the K loop)
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+s"(t0i));
#endif
    if (p.kparts > 1) {                                   // raw partial sums; bias, activation, residual: cs_reduce_kernel
        float* P = p.part + ((size_t)kp * p.B + b) * p.T * p.M;
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            const int co = co_base + i * 16 + lk * 4;
            if (co >= p.M) continue;
#pragma unroll
            for (int j = 0; j < NI; ++j) {
                const int t = t0i + tl_base + j * 16 + lr;
                if (t >= p.T) continue;
                *reinterpret_cast<float4*>(P + (size_t)t * p.M + co) = make_float4(acc0[i][j][0] + acc1[i][j][0] * (1.f / 2048.f), acc0[i][j][1] + acc1[i][j][1] * (1.f / 2048.f),
                                                                                 acc0[i][j][2] + acc1[i][j][2] * (1.f / 2048.f), acc0[i][j][3] + acc1[i][j][3] * (1.f / 2048.f));
            }
        }
        return;
    }
    // ---- epilogue: D fragment = 4 consecutive output channels of one frame per lane -> one 16-byte fp32 store ----
#pragma unroll
    for (int i = 0; i < MI; ++i) {
        const int co = co_base + i * 16 + lk * 4;
        if (co >= p.M) continue;
        float bv[4] = {0.f, 0.f, 0.f, 0.f};
        if (p.bias) {
#pragma unroll
            for (int e = 0; e < 4; ++e) bv[e] = p.bias[co + e];
        }
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            const int t = t0i + tl_base + j * 16 + lr;
            if (t >= p.T) continue;
            float* O = p.out + ((size_t)b * p.T + t) * p.ldo + co;
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (acc0[i][j][e] + acc1[i][j][e] * (1.f / 2048.f)) + bv[e];
            if (p.accumulate) {
                const float4 old = *reinterpret_cast<const float4*>(O);
                v[0] += old.x; v[1] += old.y; v[2] += old.z; v[3] += old.w;
            }
            split_act(v, p.relu);
            if (p.res) {
                const float4 r4 = *reinterpret_cast<const float4*>(p.res + ((size_t)b * p.T + t) * p.ldr + co);
                v[0] = r4.x + p.alpha * v[0]; v[1] = r4.y + p.alpha * v[1]; v[2] = r4.z + p.alpha * v[2]; v[3] = r4.w + p.alpha * v[3];
            } else if (p.alpha != 1.f) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] *= p.alpha;
            }
            *reinterpret_cast<float4*>(O) = make_float4(v[0], v[1], v[2], v[3]);
        }
    }
    }     // output tiles
}

// fp32 weight [ntaps][M][CI] (tap-major) -> hi / lo fp16 in fragment order [ntaps][CI/32][ceil(M/16)][64][8] (the order of
// hifigan_conv.hip's hg_pack_weights_kernel)
__global__ void conv1d_split_pack_kernel(const float* __restrict__ w, _Float16* __restrict__ wh, _Float16* __restrict__ wl,
                                         int ntaps, int M, int CI)
{
    const int Mt = (M + 15) >> 4, NC = CI / 32;
    const long n = (long)ntaps * NC * Mt * 512;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
        const int h = (int)(e & 7), ln = (int)((e >> 3) & 63);
        long r = e >> 9;
        const int tile = (int)(r % Mt); r /= Mt;
        const int c = (int)(r % NC); const int k = (int)(r / NC);
        const int co = tile * 16 + (ln & 15), ci = c * 32 + (ln >> 4) * 8 + h;
        const float v = (co < M) ? w[((size_t)k * M + co) * CI + ci] : 0.f;
        split_hi_lo(v, wh[e], wl[e]);
    }
}

int split_pack_launch(const char* who, const float* w, _Float16* w_hi, _Float16* w_lo, long n, int ntaps, int M, int CI, hipStream_t st)
{
    int grid = (int)((n + 255) / 256); if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(conv1d_split_pack_kernel, dim3(grid), dim3(256), 0, st, w, w_hi, w_lo, ntaps, M, CI);
    return check_launch(who);
}

// out = res + alpha * act(bias + part[0] + part[1] + ...): the K-parts in a fixed order
__global__ __launch_bounds__(256) void cs_reduce_kernel(const float* __restrict__ part, int KP, long n, const float* __restrict__ bias, int M, int act,
                                                        const float* __restrict__ res, long ldr, float alpha, float* __restrict__ out, long ldo)
{
    const long n4 = n >> 2;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n4; e += (long)gridDim.x * 256) {
        const long idx = e << 2, row = idx / M; const int c = (int)(idx - row * M);
        float4 s4 = *reinterpret_cast<const float4*>(part + idx);
        for (int k = 1; k < KP; ++k) {
            const float4 q = *reinterpret_cast<const float4*>(part + (size_t)k * n + idx);
            s4.x += q.x; s4.y += q.y; s4.z += q.z; s4.w += q.w;
        }
        float v[4] = {s4.x, s4.y, s4.z, s4.w};
        if (bias) { const float4 bb = *reinterpret_cast<const float4*>(bias + c); v[0] += bb.x; v[1] += bb.y; v[2] += bb.z; v[3] += bb.w; }
#pragma unroll
        for (int i = 0; i < 4; ++i) {                     // split_act's chain, spelled out: through the helper this kernel comes out as other code
            if (act == 1) v[i] = fmaxf(v[i], 0.f);
            else if (act == 2) v[i] = v[i] / (1.f + __expf(-v[i]));
            else if (act == 3) v[i] = 0.5f * v[i] * (1.f + erff(v[i] * 0.70710678118654752f));
        }
        float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
        if (res) r = *reinterpret_cast<const float4*>(res + row * ldr + c);
        *reinterpret_cast<float4*>(out + row * ldo + c) = make_float4(r.x + alpha * v[0], r.y + alpha * v[1], r.z + alpha * v[2], r.w + alpha * v[3]);
    }
}

// ---- launch plan: which instance, how the rows are tiled, which output tiles a workgroup owns.  Host arithmetic only (no device call:
//      dsp_conv1d_split_plan answers without a GPU).
enum CsInst { CS_256_256_128 = 0, CS_256_128_64, CS_256_256_64, CS_512_256_32, CS_512_256_64x16, CS_512_256_64, CS_128_128_256, CS_NONE };
// per_cu: workgroups a CU holds (registers and the one-tap LDS tiles); batch_rows: dense one-tap launches may tile the B * T rows as one
// sequence (not <256,128,64>: its 12 us launches did not get shorter with 198 workgroups instead of 256, profiles/r09_stage_once.txt)
struct CsInstInfo { int MT, NT, per_cu; bool batch_rows; };
static const CsInstInfo cs_inst_info[CS_NONE] = {{256, 128, 1, true}, {128, 64, 2, false}, {256, 64, 1, true}, {256, 32, 1, true}, {256, 64, 1, true},
                                                 {256, 64, 1, true}, {128, 256, 1, true}};

static CsInst cs_pick(int B, int T, int CI, int nslices, int M, int ntaps, long kmul, bool has_ln)
{
    if (has_ln) return CS_256_256_64;                          // the instance that carries the staged LayerNorm
    switch (CI) {
        case 256: {
            // 128-row tiles (8 time sub-tiles per wave, one workgroup per CU) when they fill the chip, 64-row tiles (two per CU) for the
            // narrow layers: 256 -> 256 projections on 12.6 k rows are 99 workgroups at 128 rows
            const long wgs128 = (long)((T + 127) / 128) * ((M + 255) / 256) * B * kmul;
            if (wgs128 >= 256) return CS_256_256_128;
            // under-filled launches (the Conformer's 256 -> 256 projections on 4.4 k positions: 69 workgroups of 256 output channels) take
            // 128-channel output tiles: twice the workgroups at 124 VGPRs, two per CU (the 256-channel tile needs 188: one per CU).
            // Acoustic stage 14.60 -> 14.25 ms; applied to every 64-row launch: 14.47 (the input tile is staged twice)
            const long wgs64 = (long)((T + 63) / 64) * ((M + 255) / 256) * B * kmul;
            if (wgs64 < 150) return CS_256_128_64;
            return CS_256_256_64;
        }
        case 512: {
            // (r03: a 512-wide Linear layer run as two 256-wide slices — 65 KB tiles, two workgroups per CU — is no faster: 14.59 vs 14.55 ms of
            //  GPU time per acoustic batch.)
            // launches that would leave CUs idle with 64-frame tiles (the Conformer's 2048 -> 256 on 4.4 k positions: 69 workgroups)
            // take 32-frame tiles, two workgroups per CU: 52.7 -> 36.7 us; where the 64-frame tiles fill the chip they are 10-20 % faster
            // (at 192 workgroups the 64-frame tiles still win: 34.3 vs 38.9 us for 1024 -> 256 on 10.6 k positions; 128-channel tiles: no gain)
            const long wgs64 = (long)((T + 63) / 64) * ((M + 255) / 256) * B * kmul;
            if (ntaps <= 9 && wgs64 < 128) return CS_512_256_32;
            // r05: one-tap, one-slice layers (the NAT decoder's 512 -> 512 / 1536 / 2048 projections) as 16-wave workgroups, 16 output channels per
            // wave: four waves per SIMD under the one resident workgroup (122 VGPRs), bit-identical results, 5-8 % faster (tools/cs_var_bench.py:
            // 39.8 -> 36.7, 98.7 -> 91.4, 116.6 -> 108.6 us; 512 output channels per workgroup: 2.2 x slower (spills), 8 x 2 waves: +18 %;
            // multi-slice and K = 9 layers: no difference; the 256-wide instances: no gain at 64 rows, +20 % at 128 rows)
            if (ntaps == 1 && nslices == 1 && kmul == 1) return CS_512_256_64x16;
            return CS_512_256_64;
        }
        case 128: return CS_128_128_256;
    }
    return CS_NONE;
}

struct CsPlan { CsInst inst; int B, T, row_tiles, m_tiles, ranges, mper; };

// The instance comes from the caller's (B, T), as it always has.  Then:
//  * a dense one-tap, one-slice layer is a GEMM over the B * T rows (the ABI has no batch stride: sample b starts at row b * T), so its
//    rows may be tiled as ONE sequence of B * T: no partial tile per sample (T = 197 - 200 in 64-row tiles: 128 tiles for 99 tiles' worth).
//    Taken where the traced time drops: the launch then fits one round of resident workgroups, or needs fewer rounds than before
//    (256 -> 768 with the staged LayerNorm: 384 and 300 workgroups are both two rounds, 27.8 us either way: tiled per sample as before);
//  * where the staged rows are the whole reduction (one slice, no split-K; any number of taps) a workgroup runs a contiguous range of
//    output tiles from the rows it staged once.  Ranges per row tile (equal lengths: a divisor of the tile count): the number with the
//    fewest K-steps on a CU's critical path, rounds of resident workgroups x (staging, counted as one tap's K loop, + the range's
//    tiles x taps); among equals the most ranges.  Measured per layer in profiles/r09_stage_once.txt: the 512-wide decoder layers run
//    every output tile of a row tile in one workgroup (224 workgroups, one round), 256 -> 1024, K = 9 two tiles (staging is 1 / 37 of a
//    tile's work: the round count decides), the short 256-wide layers one tile per workgroup as before.
static CsPlan cs_plan(int B, int T, int CI, int nslices, int M, int ntaps, bool has_lens, int tap_groups, bool has_ln, int n_cus)
{
    CsPlan pl;
    const long kmul = tap_groups > 0 ? (long)nslices * tap_groups : 1;
    pl.inst = cs_pick(B, T, CI, nslices, M, ntaps, kmul, has_ln);
    pl.B = B; pl.T = T; pl.row_tiles = 0; pl.m_tiles = 0; pl.ranges = 0; pl.mper = 1;
    if (pl.inst == CS_NONE) return pl;
    const CsInstInfo& ii = cs_inst_info[pl.inst];
    const bool whole = nslices == 1 && kmul == 1;            // one staged tile serves the whole reduction
    const size_t lds = (size_t)2 * (ii.NT + ntaps - 1) * CI * 2;
    const long resident = (long)(n_cus > 0 ? n_cus : 1) * (lds * ii.per_cu > 160 * 1024 ? 1 : ii.per_cu);
    pl.m_tiles = (M + ii.MT - 1) / ii.MT;
    pl.row_tiles = ((T + ii.NT - 1) / ii.NT) * B;
    pl.ranges = pl.m_tiles;
    if (!whole) return pl;
    // ranges for a number of row tiles -> rounds of resident workgroups the launch then takes
    auto choose = [&](long row_tiles, int& ranges) -> long {
        long best = -1, rounds = 0;
        for (int r = 1; r <= pl.m_tiles; ++r) {
            if (pl.m_tiles % r) continue;
            const long rd = (row_tiles * r + resident - 1) / resident, cost = rd * (1 + (long)(pl.m_tiles / r) * ntaps);
            if (best < 0 || cost <= best) { best = cost; ranges = r; rounds = rd; }
        }
        return rounds;
    };
    const long rounds = choose(pl.row_tiles, pl.ranges);
    if (ntaps == 1 && !has_lens && ii.batch_rows && (long)B * T <= 0x7fffffffL) {
        const long flat_tiles = ((long)B * T + ii.NT - 1) / ii.NT;
        int ranges_flat = 1;
        const long rounds_flat = choose(flat_tiles, ranges_flat);
        if (rounds_flat == 1 || rounds_flat < rounds) { pl.T = B * T; pl.B = 1; pl.row_tiles = (int)flat_tiles; pl.ranges = ranges_flat; }
    }
    pl.mper = pl.m_tiles / pl.ranges;
    return pl;
}

static int cs_cus_override = 0;                      // dsp_conv1d_split_plan_cus: plan launches as for a device of this many CUs (0: ask the device)

static int cs_device_cus()
{
    if (cs_cus_override > 0) return cs_cus_override;
    static int cached[64] = {0};
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return 256; }
    if (dev >= 0 && dev < 64 && cached[dev] > 0) return cached[dev];
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) { (void)hipGetLastError(); return 256; }
    if (dev >= 0 && dev < 64) cached[dev] = cus;
    return cus;
}

template <int CI, int MT, int NT, int WM, int WN>
static int cs_launch(const CsParams& p, const CsPlan& pl, hipStream_t st)
{
    const size_t lds = (size_t)2 * (NT + p.ntaps - 1) * CI * 2;
    if (lds > 160 * 1024) { set_error("conv1d_split: tiles need %zu bytes of LDS", lds); return DSP_EINVAL; }
    auto k = conv1d_split_kernel<CI, MT, NT, WM, WN>;
    set_max_dynamic_lds((const void*)k, (int)lds);
    // p.B / p.T are the plan's (one sequence of B * T rows for a dense one-tap layer)
    hipLaunchKernelGGL(k, dim3((p.T + NT - 1) / NT, p.kparts > 1 ? pl.m_tiles * p.kparts : pl.ranges, p.B), dim3(WM * WN * 64), lds, st, p);
    return check_launch("conv1d_split");
}

}  // namespace dsp

using namespace dsp;

extern "C" long dsp_conv1d_split_packed_elems(int ntaps, int M, int CI)
{
    if (ntaps < 1 || M < 1 || CI < 32 || (CI & 31)) return -1;
    return (long)ntaps * (CI / 32) * ((M + 15) / 16) * 512;
}

extern "C" int dsp_conv1d_split_pack(const float* w_tap_major, void* w_hi, void* w_lo, int ntaps, int M, int CI, dsp_stream_t stream)
{
    const long n = dsp_conv1d_split_packed_elems(ntaps, M, CI);
    if (n < 0 || !w_tap_major || !w_hi || !w_lo) { set_error("conv1d_split_pack: bad arguments"); return DSP_EINVAL; }
    return split_pack_launch("conv1d_split_pack", w_tap_major, (_Float16*)w_hi, (_Float16*)w_lo, n, ntaps, M, CI, as_stream(stream));
}

static int cs_run(const float* x, long ldx, const void* w_hi, const void* w_lo, const float* bias, float* out, long ldo,
                  int B, int T, int CI, int nslices, int M, int ntaps, int relu, int accumulate, const float* res, long ldr, float alpha,
                  dsp_stream_t stream, const int* lens = nullptr, int slack = 0, int tap_groups = 0, float* part = nullptr,
                  const float* ln_w = nullptr, const float* ln_b = nullptr, float ln_eps = 0.f)
{
    if (B < 0 || T < 1 || M < 4 || (M & 3) || ntaps < 1 || !(ntaps & 1) || ntaps > 31 || nslices < 1 || ldx < (long)CI * nslices || ldo < M ||
        (ldx & 3) || (ldo & 3)) {
        set_error("conv1d_split: bad sizes B=%d T=%d CI=%d M=%d taps=%d", B, T, CI, M, ntaps); return DSP_EINVAL; }
    if (B == 0) return DSP_OK;
    if (!x || !w_hi || !w_lo || !out) { set_error("conv1d_split: null pointer"); return DSP_EINVAL; }
    if ((((uintptr_t)x) | ((uintptr_t)out)) & 15) { set_error("conv1d_split: x / out must be 16-byte aligned"); return DSP_EINVAL; }
    CsParams p;
    p.x = x; p.wh = (const _Float16*)w_hi; p.wl = (const _Float16*)w_lo; p.bias = bias; p.out = out;
    p.B = B; p.T = T; p.M = M; p.ntaps = ntaps; p.ldx = ldx; p.ldo = ldo; p.relu = relu; p.accumulate = accumulate;
    p.nslices = nslices; p.wslice = dsp_conv1d_split_packed_elems(ntaps, M, CI);
    p.res = res; p.ldr = ldr; p.alpha = alpha; p.lens = lens; p.slack = slack;
    p.ln_w = ln_w; p.ln_b = ln_b; p.ln_eps = ln_eps;
    if (ln_w && (!ln_b || CI != 256 || nslices != 1 || ntaps != 1 || tap_groups > 0 || (((uintptr_t)ln_w | (uintptr_t)ln_b) & 15))) {
        set_error("conv1d_split: the staged LayerNorm needs a one-tap layer over exactly 256 input channels"); return DSP_EINVAL; }
    p.kparts = tap_groups > 0 ? nslices * tap_groups : 1; p.tap_groups = tap_groups > 0 ? tap_groups : 1; p.part = part;
    if (res && (((uintptr_t)res & 15) || ldr < M || (ldr & 3))) { set_error("conv1d_split: residual must be 16-byte aligned with row stride >= M"); return DSP_EINVAL; }
    hipStream_t st = as_stream(stream);
    const CsPlan pl = cs_plan(B, T, CI, nslices, M, ntaps, lens != nullptr, tap_groups, ln_w != nullptr, cs_device_cus());
    p.B = pl.B; p.T = pl.T; p.mper = pl.mper;
    switch (pl.inst) {
        case CS_256_256_128: return cs_launch<256, 256, 128, 8, 1>(p, pl, st);
        case CS_256_128_64: return cs_launch<256, 128, 64, 8, 1>(p, pl, st);
        case CS_256_256_64: return cs_launch<256, 256, 64, 8, 1>(p, pl, st);
        case CS_512_256_32: return cs_launch<512, 256, 32, 8, 1>(p, pl, st);
        case CS_512_256_64x16: return cs_launch<512, 256, 64, 16, 1>(p, pl, st);
        case CS_512_256_64: return cs_launch<512, 256, 64, 8, 1>(p, pl, st);
        case CS_128_128_256: return cs_launch<128, 128, 256, 4, 2>(p, pl, st);
        case CS_NONE: break;
    }
    set_error("conv1d_split: unsupported slice width %d (128, 256, 512; wider inputs are nslices slices)", CI);
    return DSP_EINVAL;
}

// Plan every later launch of this process as for a device of n_cus CUs; 0 returns to the device's own count.  The results do not depend
// on it (tests run the output-tile loop at shapes that would otherwise give every tile its own workgroup).  Returns the previous value.
extern "C" int dsp_conv1d_split_plan_cus(int n_cus)
{
    const int old = cs_cus_override;
    cs_cus_override = n_cus > 0 ? n_cus : 0;
    return old;
}

extern "C" int dsp_conv1d_split_plan(int B, int T, int CI, int nslices, int M, int ntaps, int has_lens, int has_ln, int tap_groups, int n_cus, int out[6])
{
    if (!out || B < 1 || T < 1 || M < 4 || ntaps < 1 || nslices < 1 || tap_groups < 0 || n_cus < 1) { set_error("conv1d_split_plan: bad arguments"); return DSP_EINVAL; }
    if (has_ln && (CI != 256 || nslices != 1 || ntaps != 1 || tap_groups > 0)) { set_error("conv1d_split_plan: the staged LayerNorm needs a one-tap layer over 256 channels"); return DSP_EINVAL; }
    const CsPlan pl = cs_plan(B, T, CI, nslices, M, ntaps, has_lens != 0, tap_groups, has_ln != 0, n_cus);
    if (pl.inst == CS_NONE) { set_error("conv1d_split_plan: unsupported slice width %d", CI); return DSP_EINVAL; }
    out[0] = pl.T; out[1] = pl.row_tiles; out[2] = pl.m_tiles; out[3] = pl.ranges;
    out[4] = cs_inst_info[pl.inst].MT; out[5] = cs_inst_info[pl.inst].NT;
    return DSP_OK;
}

extern "C" int dsp_conv1d_split(const float* x, long ldx, const void* w_hi, const void* w_lo, const float* bias, float* out, long ldo,
                                int B, int T, int CI, int nslices, int M, int ntaps, int relu, int accumulate, dsp_stream_t stream)
{
    return cs_run(x, ldx, w_hi, w_lo, bias, out, ldo, B, T, CI, nslices, M, ntaps, relu, accumulate, nullptr, 0, 1.f, stream);
}

extern "C" int dsp_conv1d_split_residual(const float* x, long ldx, const void* w_hi, const void* w_lo, const float* bias, const float* res,
                                         long ldr, float alpha, float* out, long ldo, int B, int T, int CI, int nslices, int M, int ntaps,
                                         int relu, dsp_stream_t stream)
{
    return cs_run(x, ldx, w_hi, w_lo, bias, out, ldo, B, T, CI, nslices, M, ntaps, relu, 0, res, ldr, alpha, stream);
}

extern "C" int dsp_conv1d_split_ragged(const float* x, long ldx, const void* w_hi, const void* w_lo, const float* bias, const float* res,
                                       long ldr, float alpha, float* out, long ldo, int B, int T, int CI, int nslices, int M, int ntaps,
                                       int relu, const int* lens, int slack, dsp_stream_t stream)
{
    if (lens && slack < 0) { set_error("conv1d_split_ragged: negative slack"); return DSP_EINVAL; }
    return cs_run(x, ldx, w_hi, w_lo, bias, out, ldo, B, T, CI, nslices, M, ntaps, relu, 0, res, ldr, alpha, stream, lens, slack);
}

extern "C" size_t dsp_conv1d_split_ksplit_workspace_bytes(int B, int T, int M, int nslices, int tap_groups)
{
    if (B < 1 || T < 1 || M < 4 || nslices < 1 || tap_groups < 1) return 0;
    return (size_t)nslices * tap_groups * B * T * M * sizeof(float);
}

extern "C" int dsp_conv1d_split_ksplit(const float* x, long ldx, const void* w_hi, const void* w_lo, const float* bias, const float* res, long ldr,
                                       float alpha, float* out, long ldo, int B, int T, int CI, int nslices, int M, int ntaps, int act,
                                       int tap_groups, void* workspace, size_t workspace_bytes, const int* lens, int slack, dsp_stream_t stream)
{
    if (tap_groups < 1 || tap_groups > ntaps || nslices * tap_groups < 2 || nslices * tap_groups > 64) {
        set_error("conv1d_split_ksplit: tap_groups=%d with %d slices and %d taps", tap_groups, nslices, ntaps); return DSP_EINVAL; }
    const size_t need = dsp_conv1d_split_ksplit_workspace_bytes(B, T, M, nslices, tap_groups);
    if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 15)) { set_error("conv1d_split_ksplit: workspace of %zu bytes, %zu needed (16-byte aligned)", workspace_bytes, need); return DSP_EINVAL; }
    if (act < 0 || act > 3 || (M & 3)) { set_error("conv1d_split_ksplit: bad activation / width"); return DSP_EINVAL; }
    if (B == 0) return DSP_OK;
    if (lens && slack < 0) { set_error("conv1d_split_ksplit: negative slack"); return DSP_EINVAL; }
    int rc = cs_run(x, ldx, w_hi, w_lo, nullptr, out, ldo, B, T, CI, nslices, M, ntaps, 0, 0, nullptr, 0, 1.f, stream, lens, slack, tap_groups, (float*)workspace);
    if (rc != DSP_OK) return rc;
    if (res && (((uintptr_t)res & 15) || ldr < M || (ldr & 3))) { set_error("conv1d_split_ksplit: residual must be 16-byte aligned with row stride >= M"); return DSP_EINVAL; }
    const long n = (long)B * T * M;
    int grid = (int)((n / 4 + 255) / 256); if (grid > 2048) grid = 2048;
    hipLaunchKernelGGL(cs_reduce_kernel, dim3(grid), dim3(256), 0, as_stream(stream), (const float*)workspace, nslices * tap_groups, n, bias, M, act, res, ldr, alpha, out, ldo);
    return check_launch("conv1d_split_ksplit(reduce)");
}

extern "C" int dsp_linear_ln_split(const float* x, long ldx, const float* ln_w, const float* ln_b, float ln_eps, const void* w_hi, const void* w_lo,
                                   const float* bias, const float* res, long ldr, float alpha, float* out, long ldo, int B, int T, int M, int act,
                                   const int* lens, int slack, dsp_stream_t stream)
{
    if (!ln_w || !ln_b) { set_error("linear_ln_split: LayerNorm weight and bias are required"); return DSP_EINVAL; }
    if (lens && slack < 0) { set_error("linear_ln_split: negative slack"); return DSP_EINVAL; }
    return cs_run(x, ldx, w_hi, w_lo, bias, out, ldo, B, T, 256, 1, M, 1, act, 0, res, ldr, alpha, stream, lens, slack, 0, nullptr, ln_w, ln_b, ln_eps);
}
