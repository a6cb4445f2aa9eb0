// conformer_train.hip — the inner half of the Conformer convolution module under autograd, gfx950:
//     y = SiLU(BatchNorm_train(depthwise_conv1d(x)))      on the channels-last [B,T,C] tensor, fp32 / fp16 / bf16 storage, fp32 arithmetic
// (fairseq conformer_layer.py ConvolutionModule in training mode: batch statistics, running-buffer update), and its backward.
//
// Layout of the work, the same in every kernel here: a lane owns one 16-byte group of channels and walks it four channels at a time (the
// 4 x K taps of a pass stay in registers: 124 VGPRs at K = 31; the eight channels of a 16-bit group at once would need 248), a thread
// computes CM_TT consecutive frames of one sample from the K + CM_TT - 1 input rows that slide through its registers, as
// dwconv_bn_silu_kernel does.  A workgroup is 32 channel groups x 8 tile slots; blockIdx.x is a CHUNK of DSP_CONVMOD_CHUNK_TILES
// consecutive time tiles (flattened over the batch), blockIdx.y a block of 32 channel groups.
//
// z = depthwise(x) is never stored: every kernel that needs it recomputes its tile from x (31 FMAs per element against 4 bytes written and
// read again).  dz is stored once, in fp32, in the backward's workspace: dx needs it on K - 1 halo rows per tile, and recomputing it there
// means z, u and du on the halo as well.
//
// Reductions over N = B*T (mean / var, dbeta, dgamma, dw) are two-stage: a workgroup reduces its chunk in a fixed order (a thread its
// tiles in ascending order, then the 8 tile slots in ascending order through LDS) and writes one partial per chunk to the workspace; the
// consumer merges the partials in ASCENDING chunk order.  The statistics are merged as (count, mean, M2) triples (Chan et al.), each
// tile's M2 from its centred values.  No float atomics, no hand-off between workgroups inside a launch: same inputs, same bits.
#include "common.h"
#include "host_gates.h"
#include "partial_merge.h"
#include "../../include/daspeech_decode.h"

namespace dsp {

constexpr int CM_TT = DSP_CONVMOD_TIME_TILE;              // frames per thread
constexpr int CM_TY = 8;                                  // tile slots per workgroup
constexpr int CM_CG = 32;                                 // channel groups per workgroup
constexpr int CM_TPT = DSP_CONVMOD_CHUNK_TILES / CM_TY;   // tiles per thread
constexpr int CM_KG = 8;                                  // taps per round of the dw reduction through LDS
static_assert(DSP_CONVMOD_CHUNK_TILES % CM_TY == 0, "a chunk is a whole number of tiles per slot");

// (count, mean, M2) of a set  <-  the same of a second, disjoint set (Chan, Golub, LeVeque); either may be empty
__device__ __forceinline__ void chan_merge(float& na, float& ma, float& qa, float nb, float mb, float qb)
{
    if (nb == 0.f) return;
    const float n = na + nb, d = mb - ma, r = nb / n;
    ma += d * r;
    qa += qb + d * d * na * r;
    na = n;
}

template <typename T, int K> __device__ __forceinline__ void load_taps(const T* __restrict__ w, int c, float (&wr)[4][K])
{
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int k = 0; k < K; ++k) wr[i][k] = to_f(w[(c + i) * K + k]);
}

// out[u][i] = sum_k wr[i][FLIP ? K-1-k : k] * in[t0 + u + k - P][i], rows outside [0, T) are zero.  X points at (sample, row 0, channel c).
// FLIP = false: the depthwise convolution; FLIP = true: its data gradient (in = dz)
template <typename T, int K, bool FLIP>
__device__ __forceinline__ void conv_tile(const T* __restrict__ X, int T_, int C, int t0, const float (&wr)[4][K], float (&acc)[CM_TT][4])
{
    constexpr int P = (K - 1) / 2;
#pragma unroll
    for (int u = 0; u < CM_TT; ++u)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[u][i] = 0.f;
#pragma unroll
    for (int s = 0; s < K + CM_TT - 1; ++s) {
        const int ti = t0 - P + s;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (ti >= 0 && ti < T_) load_f<T, 4>(X + (size_t)ti * C, v);
#pragma unroll
        for (int u = 0; u < CM_TT; ++u) {
            const int k = s - u;
            if (k >= 0 && k < K) {
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[u][i] = fmaf(v[i], wr[i][FLIP ? K - 1 - k : k], acc[u][i]);
            }
        }
    }
}

// the thread's place: channel group, tile slot; tile j of the thread in chunk blockIdx.x
struct CmThread {
    int lx, ty;
    __device__ __forceinline__ CmThread() : lx(threadIdx.x % CM_CG), ty(threadIdx.x / CM_CG) {}
    __device__ __forceinline__ long tile(int j) const { return (long)blockIdx.x * DSP_CONVMOD_CHUNK_TILES + j * CM_TY + ty; }
};

__device__ __forceinline__ float silu_grad_factor(float u, float& s)
{
    s = 1.f / (1.f + expf(-u));
    return s * (1.f + u * (1.f - s));
}

// ---------------------------------------------------------------- forward 1: per chunk and channel (count, mean, M2) of z
template <typename T, int K>
__global__ __launch_bounds__(256) void cm_stats_kernel(const T* __restrict__ x, const T* __restrict__ w, float* __restrict__ part,
                                                       int B, int T_, int C)
{
    constexpr int V = 16 / (int)sizeof(T), NH = V / 4, CB = CM_CG * V;
    __shared__ float red[3][CM_TY][CB];
    const CmThread th;
    const int cg = blockIdx.y * CM_CG + th.lx;
    const int nt = (T_ + CM_TT - 1) / CM_TT;
    const long ntiles = (long)B * nt;
#pragma unroll 1
    for (int h = 0; h < NH; ++h) {
        const int c = cg * V + h * 4;
        float n = 0.f, mean[4] = {0.f, 0.f, 0.f, 0.f}, m2[4] = {0.f, 0.f, 0.f, 0.f};
        if (c < C) {
            float wr[4][K];
            load_taps<T, K>(w, c, wr);
#pragma unroll 1
            for (int j = 0; j < CM_TPT; ++j) {
                const long q = th.tile(j);
                if (q >= ntiles) break;
                const int b = (int)(q / nt), t0 = (int)(q % nt) * CM_TT;
                float acc[CM_TT][4];
                conv_tile<T, K, false>(x + (size_t)b * T_ * C + c, T_, C, t0, wr, acc);
                const int cnt = (T_ - t0 < CM_TT) ? T_ - t0 : CM_TT;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float s = 0.f;
#pragma unroll
                    for (int u = 0; u < CM_TT; ++u) if (u < cnt) s += acc[u][i];
                    const float tm = s / (float)cnt;
                    float tq = 0.f;
#pragma unroll
                    for (int u = 0; u < CM_TT; ++u) if (u < cnt) { const float d = acc[u][i] - tm; tq = fmaf(d, d, tq); }
                    float ni = n;                                          // the count is the same for the four channels
                    chan_merge(ni, mean[i], m2[i], (float)cnt, tm, tq);
                }
                n += (float)cnt;
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int cl = th.lx * V + h * 4 + i;
            red[0][th.ty][cl] = n; red[1][th.ty][cl] = mean[i]; red[2][th.ty][cl] = m2[i];
        }
    }
    __syncthreads();
    const int cl = threadIdx.x, c = blockIdx.y * CB + cl;
    if (cl < CB && c < C) {
        float n = 0.f, m = 0.f, q = 0.f;
#pragma unroll
        for (int y = 0; y < CM_TY; ++y) chan_merge(n, m, q, red[0][y][cl], red[1][y][cl], red[2][y][cl]);
        float* o = part + (size_t)blockIdx.x * 3 * C;
        o[c] = n; o[C + c] = m; o[2 * C + c] = q;
    }
}

// ---------------------------------------------------------------- forward 2: merge the chunks, y = SiLU(gamma * zh + beta); chunk 0 keeps the statistics
template <typename T, int K>
__global__ __launch_bounds__(256) void cm_fwd_apply_kernel(const T* __restrict__ x, const T* __restrict__ w, const void* __restrict__ gamma,
                                                           const void* __restrict__ beta, int bn_dtype, void* __restrict__ run_mean,
                                                           void* __restrict__ run_var, float momentum, float eps, const float* __restrict__ part,
                                                           int nchunks, T* __restrict__ y, float* __restrict__ save_mean,
                                                           float* __restrict__ save_invstd, int B, int T_, int C)
{
    constexpr int V = 16 / (int)sizeof(T), NH = V / 4, CB = CM_CG * V;
    __shared__ float sm[4][CB];                                       // mean, invstd, gamma, beta
    {
        const int cl = threadIdx.x, c = blockIdx.y * CB + cl;
        if (cl < CB && c < C) {
            float n = 0.f, m = 0.f, q = 0.f;
            for (int k = 0; k < nchunks; ++k) {
                const float* p = part + (size_t)k * 3 * C;
                chan_merge(n, m, q, p[c], p[C + c], p[2 * C + c]);
            }
            const float var = q / n, invstd = 1.f / sqrtf(var + eps);
            sm[0][cl] = m; sm[1][cl] = invstd; sm[2][cl] = param_load(gamma, bn_dtype, c); sm[3][cl] = param_load(beta, bn_dtype, c);
            if (blockIdx.x == 0) {
                save_mean[c] = m; save_invstd[c] = invstd;
                if (run_mean) param_store(run_mean, bn_dtype, c, (1.f - momentum) * param_load(run_mean, bn_dtype, c) + momentum * m);
                if (run_var) param_store(run_var, bn_dtype, c, (1.f - momentum) * param_load(run_var, bn_dtype, c) + momentum * (q / (n - 1.f)));
            }
        }
    }
    __syncthreads();
    const CmThread th;
    const int cg = blockIdx.y * CM_CG + th.lx;
    const int nt = (T_ + CM_TT - 1) / CM_TT;
    const long ntiles = (long)B * nt;
#pragma unroll 1
    for (int h = 0; h < NH; ++h) {
        const int c = cg * V + h * 4, cl = th.lx * V + h * 4;
        if (c >= C) break;
        float wr[4][K];
        load_taps<T, K>(w, c, wr);
#pragma unroll 1
        for (int j = 0; j < CM_TPT; ++j) {
            const long q = th.tile(j);
            if (q >= ntiles) break;
            const int b = (int)(q / nt), t0 = (int)(q % nt) * CM_TT;
            float acc[CM_TT][4];
            conv_tile<T, K, false>(x + (size_t)b * T_ * C + c, T_, C, t0, wr, acc);
#pragma unroll
            for (int u = 0; u < CM_TT; ++u) {
                if (t0 + u < T_) {
                    float o[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float uu = sm[2][cl + i] * ((acc[u][i] - sm[0][cl + i]) * sm[1][cl + i]) + sm[3][cl + i];
                        o[i] = uu / (1.f + expf(-uu));
                    }
                    store_f<T, 4>(y + ((size_t)b * T_ + t0 + u) * C + c, o);
                }
            }
        }
    }
}

// ---------------------------------------------------------------- backward 1: per chunk and channel  sum du,  sum du * zh
template <typename T, int K>
__global__ __launch_bounds__(256) void cm_bwd_sums_kernel(const T* __restrict__ x, const T* __restrict__ w, const T* __restrict__ gy,
                                                          const void* __restrict__ gamma, const void* __restrict__ beta, int bn_dtype,
                                                          const float* __restrict__ save_mean, const float* __restrict__ save_invstd,
                                                          float* __restrict__ part, int B, int T_, int C)
{
    constexpr int V = 16 / (int)sizeof(T), NH = V / 4, CB = CM_CG * V;
    __shared__ float red[2][CM_TY][CB];
    const CmThread th;
    const int cg = blockIdx.y * CM_CG + th.lx;
    const int nt = (T_ + CM_TT - 1) / CM_TT;
    const long ntiles = (long)B * nt;
#pragma unroll 1
    for (int h = 0; h < NH; ++h) {
        const int c = cg * V + h * 4;
        float sb[4] = {0.f, 0.f, 0.f, 0.f}, sg[4] = {0.f, 0.f, 0.f, 0.f};
        if (c < C) {
            float wr[4][K], mean[4], invstd[4], g[4], be[4];
            load_taps<T, K>(w, c, wr);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                mean[i] = save_mean[c + i]; invstd[i] = save_invstd[c + i];
                g[i] = param_load(gamma, bn_dtype, c + i); be[i] = param_load(beta, bn_dtype, c + i);
            }
#pragma unroll 1
            for (int j = 0; j < CM_TPT; ++j) {
                const long q = th.tile(j);
                if (q >= ntiles) break;
                const int b = (int)(q / nt), t0 = (int)(q % nt) * CM_TT;
                float acc[CM_TT][4];
                conv_tile<T, K, false>(x + (size_t)b * T_ * C + c, T_, C, t0, wr, acc);
#pragma unroll
                for (int u = 0; u < CM_TT; ++u) {
                    if (t0 + u < T_) {
                        float go[4];
                        load_f<T, 4>(gy + ((size_t)b * T_ + t0 + u) * C + c, go);
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const float zh = (acc[u][i] - mean[i]) * invstd[i];
                            float s;
                            const float du = go[i] * silu_grad_factor(g[i] * zh + be[i], s);
                            sb[i] += du; sg[i] = fmaf(du, zh, sg[i]);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int cl = th.lx * V + h * 4 + i;
            red[0][th.ty][cl] = sb[i]; red[1][th.ty][cl] = sg[i];
        }
    }
    __syncthreads();
    const int cl = threadIdx.x, c = blockIdx.y * CB + cl;
    if (cl < CB && c < C) {
        float a = 0.f, g = 0.f;
#pragma unroll
        for (int y = 0; y < CM_TY; ++y) { a += red[0][y][cl]; g += red[1][y][cl]; }
        float* o = part + (size_t)blockIdx.x * 2 * C;
        o[c] = a; o[C + c] = g;
    }
}

// ---------------------------------------------------------------- backward 2: merge dbeta / dgamma (chunk 0 writes them), dz in fp32
template <typename T, int K>
__global__ __launch_bounds__(256) void cm_bwd_dz_kernel(const T* __restrict__ x, const T* __restrict__ w, const T* __restrict__ gy,
                                                        const void* __restrict__ gamma, const void* __restrict__ beta, int bn_dtype,
                                                        const float* __restrict__ save_mean, const float* __restrict__ save_invstd,
                                                        const float* __restrict__ part, int nchunks, void* __restrict__ dgamma,
                                                        void* __restrict__ dbeta, float* __restrict__ dz, int B, int T_, int C)
{
    constexpr int V = 16 / (int)sizeof(T), NH = V / 4, CB = CM_CG * V;
    __shared__ float sm[2][CB];                                       // dbeta / N, dgamma / N
    {
        const int cl = threadIdx.x, c = blockIdx.y * CB + cl;
        if (cl < CB && c < C) {
            float a = 0.f, g = 0.f;
            for (int k = 0; k < nchunks; ++k) {
                const float* p = part + (size_t)k * 2 * C;
                a += p[c]; g += p[C + c];
            }
            const float N = (float)B * (float)T_;
            sm[0][cl] = a / N; sm[1][cl] = g / N;
            if (blockIdx.x == 0) {
                if (dbeta) param_store(dbeta, bn_dtype, c, a);
                if (dgamma) param_store(dgamma, bn_dtype, c, g);
            }
        }
    }
    if (!dz) return;                                                   // block-uniform: only dgamma / dbeta were asked for
    __syncthreads();
    const CmThread th;
    const int cg = blockIdx.y * CM_CG + th.lx;
    const int nt = (T_ + CM_TT - 1) / CM_TT;
    const long ntiles = (long)B * nt;
#pragma unroll 1
    for (int h = 0; h < NH; ++h) {
        const int c = cg * V + h * 4, cl = th.lx * V + h * 4;
        if (c >= C) break;
        float wr[4][K], mean[4], invstd[4], g[4], be[4];
        load_taps<T, K>(w, c, wr);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            mean[i] = save_mean[c + i]; invstd[i] = save_invstd[c + i];
            g[i] = param_load(gamma, bn_dtype, c + i); be[i] = param_load(beta, bn_dtype, c + i);
        }
#pragma unroll 1
        for (int j = 0; j < CM_TPT; ++j) {
            const long q = th.tile(j);
            if (q >= ntiles) break;
            const int b = (int)(q / nt), t0 = (int)(q % nt) * CM_TT;
            float acc[CM_TT][4];
            conv_tile<T, K, false>(x + (size_t)b * T_ * C + c, T_, C, t0, wr, acc);
#pragma unroll
            for (int u = 0; u < CM_TT; ++u) {
                if (t0 + u < T_) {
                    const size_t at = ((size_t)b * T_ + t0 + u) * C + c;
                    float go[4], o[4];
                    load_f<T, 4>(gy + at, go);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float zh = (acc[u][i] - mean[i]) * invstd[i];
                        float s;
                        const float du = go[i] * silu_grad_factor(g[i] * zh + be[i], s);
                        o[i] = g[i] * invstd[i] * (du - sm[0][cl + i] - zh * sm[1][cl + i]);
                    }
                    store_f<float, 4>(dz + at, o);
                }
            }
        }
    }
}

// ---------------------------------------------------------------- backward 3: dx = flipped depthwise(dz); per chunk, channel and tap  sum dz * x
template <typename T, int K, bool DX, bool DW>
__global__ __launch_bounds__(256) void cm_bwd_dxdw_kernel(const T* __restrict__ x, const T* __restrict__ w, const float* __restrict__ dz,
                                                          T* __restrict__ dx, float* __restrict__ wpart, int B, int T_, int C)
{
    constexpr int V = 16 / (int)sizeof(T), NH = V / 4, P = (K - 1) / 2;
    __shared__ float red[DW ? CM_TY : 1][DW ? CM_CG : 1][4][CM_KG];
    const CmThread th;
    const int cg = blockIdx.y * CM_CG + th.lx;
    const int nt = (T_ + CM_TT - 1) / CM_TT;
    const long ntiles = (long)B * nt;
#pragma unroll 1
    for (int h = 0; h < NH; ++h) {
        const int c = cg * V + h * 4;                                  // c >= C: the lane only takes part in the barriers below
        if (DX && c < C) {
            float wr[4][K];
            load_taps<T, K>(w, c, wr);
#pragma unroll 1
            for (int j = 0; j < CM_TPT; ++j) {
                const long q = th.tile(j);
                if (q >= ntiles) break;
                const int b = (int)(q / nt), t0 = (int)(q % nt) * CM_TT;
                float acc[CM_TT][4];
                conv_tile<float, K, true>(dz + (size_t)b * T_ * C + c, T_, C, t0, wr, acc);
#pragma unroll
                for (int u = 0; u < CM_TT; ++u)
                    if (t0 + u < T_) store_f<T, 4>(dx + ((size_t)b * T_ + t0 + u) * C + c, acc[u]);
            }
        }
        if (DW) {
            float da[4][K];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int k = 0; k < K; ++k) da[i][k] = 0.f;
            if (c < C) {
#pragma unroll 1
                for (int j = 0; j < CM_TPT; ++j) {
                    const long q = th.tile(j);
                    if (q >= ntiles) break;
                    const int b = (int)(q / nt), t0 = (int)(q % nt) * CM_TT;
                    const size_t base = (size_t)b * T_ * C + c;
                    float g[CM_TT][4];
#pragma unroll
                    for (int u = 0; u < CM_TT; ++u) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) g[u][i] = 0.f;
                        if (t0 + u < T_) load_f<float, 4>(dz + base + (size_t)(t0 + u) * C, g[u]);
                    }
                    // input row t0 - P + s meets output row t0 + u at tap k = s - u
#pragma unroll
                    for (int s = 0; s < K + CM_TT - 1; ++s) {
                        const int ti = t0 - P + s;
                        float v[4] = {0.f, 0.f, 0.f, 0.f};
                        if (ti >= 0 && ti < T_) load_f<T, 4>(x + base + (size_t)ti * C, v);
#pragma unroll
                        for (int u = 0; u < CM_TT; ++u) {
                            const int k = s - u;
                            if (k >= 0 && k < K) {
#pragma unroll
                                for (int i = 0; i < 4; ++i) da[i][k] = fmaf(g[u][i], v[i], da[i][k]);
                            }
                        }
                    }
                }
            }
            // the 8 tile slots in ascending order, CM_KG taps per round
#pragma unroll
            for (int k0 = 0; k0 < K; k0 += CM_KG) {
                __syncthreads();
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int k = 0; k < CM_KG; ++k) red[th.ty][th.lx][i][k] = (k0 + k < K) ? da[i][(k0 + k < K) ? k0 + k : 0] : 0.f;
                __syncthreads();
                for (int e = threadIdx.x; e < CM_CG * 4 * CM_KG; e += 256) {
                    const int k = e % CM_KG, i = (e / CM_KG) % 4, lx = e / (CM_KG * 4);
                    const int cc = (blockIdx.y * CM_CG + lx) * V + h * 4 + i;
                    if (cc < C && k0 + k < K) {
                        float a = 0.f;
#pragma unroll
                        for (int y = 0; y < CM_TY; ++y) a += red[y][lx][i][k];
                        wpart[((size_t)blockIdx.x * C + cc) * K + k0 + k] = a;
                    }
                }
            }
        }
    }
}

// backward 4: dw[c,k] = its chunk sums in ascending chunk order, merge_store_kernel (partial_merge.h)

static long cm_chunks(int B, int T) { return ((long)B * ((T + CM_TT - 1) / CM_TT) + DSP_CONVMOD_CHUNK_TILES - 1) / DSP_CONVMOD_CHUNK_TILES; }
// the workspace: [chunks][3][C] statistics (forward) or [chunks][2][C] dbeta / dgamma sums (backward) | dz [B,T,C] | [chunks][C][K] dw sums
static size_t cm_stat_bytes(int B, int T, int C) { return a16((size_t)cm_chunks(B, T) * 3 * C * sizeof(float)); }
static size_t cm_dz_bytes(int B, int T, int C) { return a16((size_t)B * T * C * sizeof(float)); }
static size_t cm_wpart_bytes(int B, int T, int C, int K) { return a16((size_t)cm_chunks(B, T) * C * K * sizeof(float)); }

// what both entry points check; 1: nothing to do (B == 0), 0: go on, < 0: refused
static int cm_check(const char* who, int act_dtype, int bn_dtype, int B, int T, int C, int K)
{
    const int es = elem_size(act_dtype);
    if (!es || !elem_size(bn_dtype) || (bn_dtype != act_dtype && bn_dtype != DSP_F32)) {
        set_error("%s: dtype codes %d (x, w, y) / %d (BatchNorm tensors: the same, or fp32)", who, act_dtype, bn_dtype); return DSP_EINVAL;
    }
    const int V = 16 / es;
    if (B < 0 || T < 1 || C < V || (C % V)) { set_error("%s: bad sizes B=%d T=%d C=%d (C a multiple of %d)", who, B, T, C, V); return DSP_EINVAL; }
    if (K != 3 && K != 7 && K != 15 && K != 31) { set_error("%s: kernel size %d (3, 7, 15, 31)", who, K); return DSP_EINVAL; }
    if (B == 0) return 1;
    if ((long)B * T < 2) { set_error("%s: batch statistics need B*T >= 2", who); return DSP_EINVAL; }
    if ((long)B * T > (1L << 24) || (size_t)C * K > 0x7fffffffu) {          // row counts are carried in fp32: exact up to 2^24
        set_error("%s: shape too large (B*T <= 2^24)", who); return DSP_EINVAL;
    }
    return 0;
}

}  // namespace dsp

using namespace dsp;

#define CM_K_SWITCH(K, ...)                                                      \
    switch (K) {                                                                 \
        case 31: { constexpr int KK = 31; __VA_ARGS__; } break;                  \
        case 15: { constexpr int KK = 15; __VA_ARGS__; } break;                  \
        case 7: { constexpr int KK = 7; __VA_ARGS__; } break;                    \
        default: { constexpr int KK = 3; __VA_ARGS__; } break;                   \
    }
#define CM_DISPATCH(dtype, K, ...) DSP_DISPATCH_ELEM(dtype, E, CM_K_SWITCH(K, __VA_ARGS__))

extern "C" size_t dsp_dwconv_bn_silu_train_workspace_bytes(int B, int T, int C, int K)
{
    if (B <= 0 || T < 1 || C < 1 || K < 1) return 0;
    return cm_stat_bytes(B, T, C) + cm_dz_bytes(B, T, C) + cm_wpart_bytes(B, T, C, K);
}

extern "C" int dsp_dwconv_bn_silu_train_fwd(const void* x, const void* w, const void* gamma, const void* beta, void* running_mean,
                                            void* running_var, float momentum, float eps, void* y, float* save_mean, float* save_invstd,
                                            void* workspace, size_t workspace_bytes, int act_dtype, int bn_dtype, int B, int T, int C, int K,
                                            dsp_stream_t stream)
{
    const char* who = "dwconv_bn_silu_train_fwd";
    const int rc = cm_check(who, act_dtype, bn_dtype, B, T, C, K);
    if (rc) return rc < 0 ? rc : DSP_OK;
    if (!x || !w || !gamma || !beta || !y || !save_mean || !save_invstd || x == y || save_mean == save_invstd) {
        set_error("%s: null or aliased pointer", who); return DSP_EINVAL;
    }
    if (!on16(x, y)) { set_error("%s: x / y must be 16-byte aligned", who); return DSP_EINVAL; }
    DSP_GATE(workspace_gate(who, workspace, workspace_bytes, cm_stat_bytes(B, T, C), "dsp_dwconv_bn_silu_train_workspace_bytes"));
    const int V = 16 / elem_size(act_dtype);
    const int nchunks = (int)cm_chunks(B, T);
    const dim3 grid((unsigned)nchunks, (unsigned)((C / V + CM_CG - 1) / CM_CG));
    float* part = (float*)workspace;
    hipStream_t st = as_stream(stream);
    CM_DISPATCH(act_dtype, K, hipLaunchKernelGGL((cm_stats_kernel<E, KK>), grid, dim3(256), 0, st, (const E*)x, (const E*)w, part, B, T, C));
    CM_DISPATCH(act_dtype, K, hipLaunchKernelGGL((cm_fwd_apply_kernel<E, KK>), grid, dim3(256), 0, st, (const E*)x, (const E*)w, gamma, beta, bn_dtype,
                                                 running_mean, running_var, momentum, eps, part, nchunks, (E*)y, save_mean, save_invstd, B, T, C));
    return check_launch(who);
}

extern "C" int dsp_dwconv_bn_silu_train_bwd(const void* x, const void* w, const void* gamma, const void* beta, const float* save_mean,
                                            const float* save_invstd, const void* grad_y, void* dx, void* dw, void* dgamma, void* dbeta,
                                            void* workspace, size_t workspace_bytes, int act_dtype, int bn_dtype, int B, int T, int C, int K,
                                            dsp_stream_t stream)
{
    const char* who = "dwconv_bn_silu_train_bwd";
    const int rc = cm_check(who, act_dtype, bn_dtype, B, T, C, K);
    if (rc) return rc < 0 ? rc : DSP_OK;
    if (!dx && !dw && !dgamma && !dbeta) return DSP_OK;
    if (!x || !w || !gamma || !beta || !save_mean || !save_invstd || !grad_y || dx == x || dx == grad_y || (dw && dw == w)) {
        set_error("%s: null or aliased pointer", who); return DSP_EINVAL;
    }
    if (!on16(x, grad_y, dx)) { set_error("%s: x / grad_y / dx must be 16-byte aligned", who); return DSP_EINVAL; }
    DSP_GATE(workspace_gate(who, workspace, workspace_bytes, dsp_dwconv_bn_silu_train_workspace_bytes(B, T, C, K),
                            "dsp_dwconv_bn_silu_train_workspace_bytes"));
    const int V = 16 / elem_size(act_dtype);
    const int nchunks = (int)cm_chunks(B, T);
    const unsigned gy_ = (unsigned)((C / V + CM_CG - 1) / CM_CG);
    const dim3 grid((unsigned)nchunks, gy_);
    float* part = (float*)workspace;
    float* dz = (float*)((char*)workspace + cm_stat_bytes(B, T, C));
    float* wpart = (float*)((char*)dz + cm_dz_bytes(B, T, C));
    const bool need_dz = dx || dw;
    hipStream_t st = as_stream(stream);
    CM_DISPATCH(act_dtype, K, hipLaunchKernelGGL((cm_bwd_sums_kernel<E, KK>), grid, dim3(256), 0, st, (const E*)x, (const E*)w, (const E*)grad_y, gamma,
                                                 beta, bn_dtype, save_mean, save_invstd, part, B, T, C));
    CM_DISPATCH(act_dtype, K, hipLaunchKernelGGL((cm_bwd_dz_kernel<E, KK>), need_dz ? grid : dim3(1, gy_), dim3(256), 0, st, (const E*)x, (const E*)w,
                                                 (const E*)grad_y, gamma, beta, bn_dtype, save_mean, save_invstd, part, nchunks, dgamma, dbeta,
                                                 need_dz ? dz : (float*)nullptr, B, T, C));
    if (dx && dw) {
        CM_DISPATCH(act_dtype, K, hipLaunchKernelGGL((cm_bwd_dxdw_kernel<E, KK, true, true>), grid, dim3(256), 0, st, (const E*)x, (const E*)w, dz, (E*)dx,
                                                     wpart, B, T, C));
    } else if (dx) {
        CM_DISPATCH(act_dtype, K, hipLaunchKernelGGL((cm_bwd_dxdw_kernel<E, KK, true, false>), grid, dim3(256), 0, st, (const E*)x, (const E*)w, dz, (E*)dx,
                                                     wpart, B, T, C));
    } else if (dw) {
        CM_DISPATCH(act_dtype, K, hipLaunchKernelGGL((cm_bwd_dxdw_kernel<E, KK, false, true>), grid, dim3(256), 0, st, (const E*)x, (const E*)w, dz,
                                                     (E*)nullptr, wpart, B, T, C));
    }
    if (dw) {
        const int CK = C * K;
        DSP_DISPATCH_ELEM(act_dtype, E, hipLaunchKernelGGL(merge_store_kernel<E>, dim3((CK + 255) / 256), dim3(256), 0, st, wpart, nchunks, (long)CK, (E*)dw));
    }
    return check_launch(who);
}
