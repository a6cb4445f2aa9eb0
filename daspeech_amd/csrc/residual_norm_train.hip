// residual_norm_train.hip — residual + dropout + LayerNorm under autograd, gfx950:
//     s = residual + alpha * dropout(h [+ bias]);   y = LayerNorm(s)          rows R = prod(leading dims), columns C, fp32 / fp16 / bf16 storage,
// fp32 arithmetic, and its backward (include/daspeech_decode.h: dsp_resnorm_train_fwd / _bwd).  The pattern of every pre-norm (Conformer) and
// post-norm (NAT decoder, FastSpeech2 FFT) residual site of the training step: one forward launch, one backward launch and a merge tail.
//
// Layout of the work, the same in both kernels: a lane owns 16-byte groups of columns (V = 4 or 8 elements, 16-byte loads and stores), W lanes
// own a row (W = 8, 16, 32 or 64: the power of two that covers the C / V groups of a row; at W < 64 a wave works on 64 / W consecutive rows at
// once), a lane of a full wave takes NG = 1, 2, 4 or 8 groups 64 groups apart (C <= 2048).  The row stays in registers between its reductions;
// every row reduction is a butterfly of __shfl_xor over the W lanes: no LDS, and every lane ends with the same bits.
//
// The dropout mask is never stored: element e = r * C + c keeps its value when word (e & 3) of Philox4x32-10(counter = (e >> 2, offset),
// key = seed) has its top 24 bits >= thr.  A 16-byte group is V / 4 Philox calls; the backward draws the same words again.
//
// Column sums of the backward (dgamma, dbeta, dbias): a lane adds the rows it owns, in ascending order, into registers (3 x NG x V); the
// 64 / W row slots of a wave are folded by a butterfly, the four waves of the workgroup through LDS in ascending wave order; the workgroup
// writes one fp32 partial per column for its chunk of DSP_RESNORM_CHUNK_ROWS rows, and rn_bwd_merge_kernel adds the chunks in ASCENDING
// order.  No float atomics, no hand-off between workgroups inside a launch: same inputs, same bits.
#include "common.h"
#include "host_gates.h"
#include "philox.h"
#include "../../include/daspeech_decode.h"

namespace dsp {

constexpr int RN_CHUNK = DSP_RESNORM_CHUNK_ROWS;          // rows per workgroup of the backward = rows per workspace partial
constexpr int RN_WAVES = 4;
constexpr int RN_MIN_W = 64 * RN_WAVES / RN_CHUNK;       // fewest lanes per row: one pass of the four waves covers a chunk at most
constexpr int RN_FWD_PASSES = 2;                          // forward: passes of the four waves per workgroup (no partials: small workgroups)
static_assert(RN_CHUNK % RN_WAVES == 0 && RN_MIN_W >= 1 && 64 % RN_MIN_W == 0, "a chunk is a whole number of wave passes");

// ---------------------------------------------------------------- forward
template <typename T, int NG>
__global__ __launch_bounds__(256) void rn_fwd_kernel(const T* __restrict__ h, const T* __restrict__ res, const void* __restrict__ bias,
                                                     const void* __restrict__ gamma, const void* __restrict__ beta, int pdtype, float eps,
                                                     float alpha, float keep_scale, uint32_t thr, uint64_t seed, uint64_t offset,
                                                     const uint64_t* __restrict__ rng_state, T* __restrict__ s_out, T* __restrict__ y,
                                                     float* __restrict__ stats, long R, int C, int W)
{
    constexpr int V = elems16<T>;
    philox_stream(seed, offset, rng_state);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rpw = 64 / W, sub = lane / W, l = lane % W, G = C / V;
    const float invC = 1.f / (float)C;
    float ga[NG][V], be[NG][V], bi[NG][V];
    bool cv[NG];
#pragma unroll
    for (int k = 0; k < NG; ++k) {
        const int c = (k * 64 + l) * V;
        cv[k] = k * 64 + l < G;
#pragma unroll
        for (int i = 0; i < V; ++i) { ga[k][i] = 0.f; be[k][i] = 0.f; bi[k][i] = 0.f; }
        if (cv[k]) {
            param_load_f<T>(gamma, pdtype, c, ga[k]);
            param_load_f<T>(beta, pdtype, c, be[k]);
            if (h && bias) param_load_f<T>(bias, pdtype, c, bi[k]);
        }
    }
#pragma unroll 1
    for (int it = 0; it < RN_FWD_PASSES; ++it) {
        const long row = ((long)blockIdx.x * RN_FWD_PASSES + it) * (RN_WAVES * rpw) + wave * rpw + sub;
        const bool rv = row < R;                                           // the shuffles below need every lane: rows past R carry zeros
        float v[NG][V];
        float sum = 0.f;
#pragma unroll
        for (int k = 0; k < NG; ++k) {
#pragma unroll
            for (int i = 0; i < V; ++i) v[k][i] = 0.f;
            if (rv && cv[k]) {
                const size_t at = (size_t)row * C + (size_t)(k * 64 + l) * V;
                load_f<T>(res + at, v[k]);
                if (h) {
                    float hv[V];
                    load_f<T>(h + at, hv);
                    if (thr) {
                        bool keep[V];
                        keep_flags<V>((uint64_t)at, seed, offset, thr, keep);
#pragma unroll
                        for (int i = 0; i < V; ++i) v[k][i] = fmaf(alpha, keep[i] ? (hv[i] + bi[k][i]) * keep_scale : 0.f, v[k][i]);
                    } else {
#pragma unroll
                        for (int i = 0; i < V; ++i) v[k][i] = fmaf(alpha, hv[i] + bi[k][i], v[k][i]);
                    }
#pragma unroll
                    for (int i = 0; i < V; ++i) v[k][i] = to_f(from_f<T>(v[k][i]));      // the statistics are those of s as stored
                    store_f(s_out + at, v[k]);
                }
#pragma unroll
                for (int i = 0; i < V; ++i) sum += v[k][i];
            }
        }
        float mean = lanes_sum(sum, W) * invC;
        // the mean in two steps, as layer_norm_kernel (conformer_ops.hip): the centred values carry the rounding that the first sum lost
        float e = 0.f;
#pragma unroll
        for (int k = 0; k < NG; ++k)
            if (cv[k]) {
#pragma unroll
                for (int i = 0; i < V; ++i) { v[k][i] -= mean; e += v[k][i]; }
            }
        const float corr = lanes_sum(e, W) * invC;
        mean += corr;
        float q = 0.f;
#pragma unroll
        for (int k = 0; k < NG; ++k)
            if (cv[k]) {
#pragma unroll
                for (int i = 0; i < V; ++i) { v[k][i] -= corr; q = fmaf(v[k][i], v[k][i], q); }
            }
        const float rstd = 1.f / sqrtf(lanes_sum(q, W) * invC + eps);
        if (rv) {
#pragma unroll
            for (int k = 0; k < NG; ++k)
                if (cv[k]) {
                    float o[V];
#pragma unroll
                    for (int i = 0; i < V; ++i) o[i] = fmaf(v[k][i] * rstd, ga[k][i], be[k][i]);
                    store_f(y + (size_t)row * C + (size_t)(k * 64 + l) * V, o);
                }
            if (l == 0) *reinterpret_cast<float2*>(stats + 2 * row) = make_float2(mean, rstd);
        }
    }
}

// ---------------------------------------------------------------- backward: dresidual, dh, one partial of dgamma / dbeta / dbias per chunk
template <typename T, int NG>
__global__ __launch_bounds__(256) void rn_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ ds, const T* __restrict__ s,
                                                     const float* __restrict__ stats, const void* __restrict__ gamma, int pdtype, float alpha,
                                                     float keep_scale, uint32_t thr, uint64_t seed, uint64_t offset,
                                                     const uint64_t* __restrict__ rng_state, T* __restrict__ dh, T* __restrict__ dres,
                                                     float* __restrict__ part, int want_dh, long R, int C, int W)
{
    constexpr int V = elems16<T>;
    philox_stream(seed, offset, rng_state);
    __shared__ float red[RN_WAVES][NG * 64 * V];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rpw = 64 / W, sub = lane / W, l = lane % W, G = C / V;
    const float invC = 1.f / (float)C;
    float ga[NG][V], ag[NG][V], ab[NG][V], ah[NG][V];
    bool cv[NG];
#pragma unroll
    for (int k = 0; k < NG; ++k) {
        cv[k] = k * 64 + l < G;
#pragma unroll
        for (int i = 0; i < V; ++i) { ga[k][i] = 0.f; ag[k][i] = 0.f; ab[k][i] = 0.f; ah[k][i] = 0.f; }
        if (cv[k] && dy) param_load_f<T>(gamma, pdtype, (k * 64 + l) * V, ga[k]);
    }
    const int passes = RN_CHUNK / (RN_WAVES * rpw);
#pragma unroll 1
    for (int it = 0; it < passes; ++it) {
        const long row = (long)blockIdx.x * RN_CHUNK + (long)(it * RN_WAVES + wave) * rpw + sub;
        const bool rv = row < R;
        float mean = 0.f, rstd = 0.f;
        // without dy (y was not used) neither s nor stats is read and both may be NULL: rstd = 0 leaves g = ds
        if (rv && dy) { const float2 st = *reinterpret_cast<const float2*>(stats + 2 * row); mean = st.x; rstd = st.y; }
        float xh[NG][V], gy[NG][V];
        float a = 0.f, b = 0.f;
#pragma unroll
        for (int k = 0; k < NG; ++k) {
#pragma unroll
            for (int i = 0; i < V; ++i) { xh[k][i] = 0.f; gy[k][i] = 0.f; }
            if (rv && cv[k] && dy) {
                const size_t at = (size_t)row * C + (size_t)(k * 64 + l) * V;
                load_f<T>(s + at, xh[k]);
                load_f<T>(dy + at, gy[k]);
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    xh[k][i] = (xh[k][i] - mean) * rstd;
                    const float dx = gy[k][i] * ga[k][i];
                    a += dx; b = fmaf(dx, xh[k][i], b);
                }
            }
        }
        if (dy) { a = lanes_sum(a, W) * invC; b = lanes_sum(b, W) * invC; }      // kernel-uniform
        if (rv) {
#pragma unroll
            for (int k = 0; k < NG; ++k)
                if (cv[k]) {
                    const size_t at = (size_t)row * C + (size_t)(k * 64 + l) * V;
                    float g[V];
#pragma unroll
                    for (int i = 0; i < V; ++i) g[i] = 0.f;
                    if (ds) load_f<T>(ds + at, g);
#pragma unroll
                    for (int i = 0; i < V; ++i) {
                        g[i] = fmaf(rstd, gy[k][i] * ga[k][i] - a - xh[k][i] * b, g[i]);
                        ag[k][i] = fmaf(gy[k][i], xh[k][i], ag[k][i]);
                        ab[k][i] += gy[k][i];
                    }
                    if (dres) store_f(dres + at, g);
                    if (want_dh) {
                        if (thr) {
                            bool keep[V];
                            keep_flags<V>((uint64_t)at, seed, offset, thr, keep);
#pragma unroll
                            for (int i = 0; i < V; ++i) g[i] = keep[i] ? alpha * keep_scale * g[i] : 0.f;
                        } else {
#pragma unroll
                            for (int i = 0; i < V; ++i) g[i] = alpha * g[i];
                        }
#pragma unroll
                        for (int i = 0; i < V; ++i) ah[k][i] += g[i];
                        if (dh) store_f(dh + at, g);
                    }
                }
        }
    }
    if (!part) return;                                                     // kernel-uniform: no column sum was asked for
    // the row slots of the wave (butterfly), then the four waves in ascending order through LDS; one quantity per round
#pragma unroll 1
    for (int qn = 0; qn < 3; ++qn) {
        __syncthreads();
#pragma unroll
        for (int k = 0; k < NG; ++k) {
#pragma unroll
            for (int i = 0; i < V; ++i) {
                float t = qn == 0 ? ag[k][i] : (qn == 1 ? ab[k][i] : ah[k][i]);
                for (int o = W; o < 64; o <<= 1) t += __shfl_xor(t, o, 64);
                if (sub == 0 && cv[k]) red[wave][(k * 64 + l) * V + i] = t;
            }
        }
        __syncthreads();
        for (int c = threadIdx.x; c < C; c += 256) {
            float t = red[0][c];
#pragma unroll
            for (int w = 1; w < RN_WAVES; ++w) t += red[w][c];
            part[((size_t)blockIdx.x * 3 + qn) * C + c] = t;
        }
    }
}

// ---------------------------------------------------------------- backward tail: the chunks in ascending order
// The partials are a [nchunks][3 * C] matrix; a workgroup owns 64 of its columns.  One thread per column adding nchunks values it loads itself
// is a chain of nchunks load latencies (0.45 ms at 1600 chunks), so the loads are taken off the chain: all 256 threads bring a tile of
// RN_MT chunks x 64 columns into LDS (RN_MT / 4 independent loads each, rows of 256 bytes), then one thread per column adds the tile's
// values in ascending chunk order — the same sum, in the same order, as the plain loop.
constexpr int RN_MT = 128;
__global__ __launch_bounds__(256) void rn_bwd_merge_kernel(const float* __restrict__ part, long nchunks, void* __restrict__ dgamma,
                                                           void* __restrict__ dbeta, void* __restrict__ dbias, int pdtype, int C)
{
    __shared__ float tile[RN_MT][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int e = blockIdx.x * 64 + tx, E = 3 * C;
    float acc = 0.f;
#pragma unroll 1
    for (long k0 = 0; k0 < nchunks; k0 += RN_MT) {
        float r[RN_MT / 4];
#pragma unroll
        for (int j = 0; j < RN_MT / 4; ++j) {
            const long k = k0 + ty + 4 * j;
            r[j] = (k < nchunks && e < E) ? part[(size_t)k * E + e] : 0.f;
        }
        __syncthreads();                                                   // the tile before this one has been added
#pragma unroll
        for (int j = 0; j < RN_MT / 4; ++j) tile[ty + 4 * j][tx] = r[j];
        __syncthreads();
        if (ty == 0) {
            const int n = (int)(nchunks - k0 < RN_MT ? nchunks - k0 : RN_MT);
            for (int k = 0; k < n; ++k) acc += tile[k][tx];
        }
    }
    if (ty != 0 || e >= E) return;
    const int qn = e / C, c = e % C;
    void* out = qn == 0 ? dgamma : (qn == 1 ? dbeta : dbias);
    if (out) param_store(out, pdtype, c, acc);
}

// ---------------------------------------------------------------- the mask alone, as bytes
__global__ __launch_bounds__(256) void rn_keep_mask_kernel(uint64_t seed, uint64_t offset, const uint64_t* __restrict__ rng_state, uint32_t thr,
                                                           unsigned char* __restrict__ out, long n)
{
    philox_stream(seed, offset, rng_state);
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (4 * g >= n) return;
    bool keep[4];
    keep_flags<4>((uint64_t)(4 * g), seed, offset, thr, keep);
    for (int i = 0; i < 4; ++i)
        if (4 * g + i < n) out[4 * g + i] = keep[i] ? 1 : 0;
}

// ---------------------------------------------------------------- state[1] += by: the one kernel that writes a dropout state
__global__ void rn_state_advance_kernel(uint64_t* __restrict__ state, uint64_t by)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) state[1] += by;
}

static long rn_chunks(long R) { return (R + RN_CHUNK - 1) / RN_CHUNK; }

// what both entry points check; 1: nothing to do (R == 0), 0: go on, < 0: refused
static int rn_check(const char* who, int act_dtype, int param_dtype, long R, int C, const uint64_t* rng_state)
{
    DSP_GATE(rng_state_gate(who, rng_state));
    const int es = elem_size(act_dtype);
    if (!es || !elem_size(param_dtype) || (param_dtype != act_dtype && param_dtype != DSP_F32)) {
        set_error("%s: dtype codes %d (h, residual, s, y and their gradients) / %d (gamma, beta, bias: the same, or fp32)", who, act_dtype, param_dtype);
        return DSP_EINVAL;
    }
    const int V = 16 / es;
    if (R < 0 || R > (1L << 24) || C < V || (C % V) || C > 2048) {
        set_error("%s: bad sizes R=%ld C=%d (R <= 2^24, C a multiple of %d, C <= 2048)", who, R, C, V); return DSP_EINVAL;
    }
    return R == 0 ? 1 : 0;
}

// lanes per row and 16-byte groups per lane
static void rn_plan(int G, int& W, int& NG)
{
    W = RN_MIN_W; NG = 1;
    while (W < 64 && W < G) W <<= 1;
    while (NG * 64 < G) NG <<= 1;
}

}  // namespace dsp

using namespace dsp;

#define RN_NG_SWITCH4(NG_, ...)                                                  \
    switch (NG_) {                                                               \
        case 1: { constexpr int NGC = 1; __VA_ARGS__; } break;                   \
        case 2: { constexpr int NGC = 2; __VA_ARGS__; } break;                   \
        default: { constexpr int NGC = 4; __VA_ARGS__; } break;                  \
    }
// C <= 2048: at most 8 groups of four fp32 per lane, 4 groups of eight 16-bit elements
#define RN_DISPATCH(dtype, NG_, ...)                                             \
    if ((dtype) == DSP_F32 && NG_ == 8) { using E = float; constexpr int NGC = 8; __VA_ARGS__; } \
    else DSP_DISPATCH_ELEM(dtype, E, RN_NG_SWITCH4(NG_, __VA_ARGS__))

extern "C" size_t dsp_resnorm_train_workspace_bytes(int64_t R, int C)
{
    if (R <= 0 || C < 1) return 0;
    return a16((size_t)rn_chunks((long)R) * 3 * (size_t)C * sizeof(float));
}

static int rn_fwd(const char* who, const void* h, const void* residual, const void* bias, const void* gamma, const void* beta, float eps,
                  float alpha, float keep_scale, unsigned int thr, uint64_t seed, uint64_t offset, const uint64_t* rng_state, void* s, void* y,
                  float* stats, int act_dtype, int param_dtype, int64_t R, int C, dsp_stream_t stream)
{
    const int rc = rn_check(who, act_dtype, param_dtype, (long)R, C, rng_state);
    if (rc) return rc < 0 ? rc : DSP_OK;
    if (!residual || !gamma || !beta || !y || !stats || (h && !s) || y == residual || y == h || (h && (s == residual || s == h || s == y))) {
        set_error("%s: null or aliased pointer", who); return DSP_EINVAL;
    }
    if (thr > (1u << 24)) { set_error("%s: thr %u above 2^24", who, thr); return DSP_EINVAL; }
    if (!on16(h, residual, bias, gamma, beta, h ? s : nullptr, y) || ((uintptr_t)stats & 7)) {
        set_error("%s: tensors must be 16-byte aligned (stats: 8)", who); return DSP_EINVAL;
    }
    int W, NG;
    rn_plan(C / (16 / elem_size(act_dtype)), W, NG);
    const long rows_per_wg = (long)RN_FWD_PASSES * RN_WAVES * (64 / W);
    const unsigned grid = (unsigned)((R + rows_per_wg - 1) / rows_per_wg);
    hipStream_t st = as_stream(stream);
    RN_DISPATCH(act_dtype, NG, hipLaunchKernelGGL((rn_fwd_kernel<E, NGC>), dim3(grid), dim3(256), 0, st, (const E*)h, (const E*)residual, bias, gamma,
                                                  beta, param_dtype, eps, alpha, keep_scale, (uint32_t)thr, seed, offset, rng_state, (E*)s, (E*)y, stats,
                                                  (long)R, C, W));
    return check_launch(who);
}

extern "C" int dsp_resnorm_train_fwd(const void* h, const void* residual, const void* bias, const void* gamma, const void* beta, float eps,
                                     float alpha, float keep_scale, unsigned int thr, uint64_t seed, uint64_t offset, void* s, void* y,
                                     float* stats, int act_dtype, int param_dtype, int64_t R, int C, dsp_stream_t stream)
{
    return rn_fwd("resnorm_train_fwd", h, residual, bias, gamma, beta, eps, alpha, keep_scale, thr, seed, offset, nullptr, s, y, stats, act_dtype,
                  param_dtype, R, C, stream);
}

extern "C" int dsp_resnorm_train_fwd_state(const void* h, const void* residual, const void* bias, const void* gamma, const void* beta, float eps,
                                           float alpha, float keep_scale, unsigned int thr, uint64_t seed, uint64_t offset, void* s, void* y,
                                           float* stats, int act_dtype, int param_dtype, int64_t R, int C, const uint64_t* rng_state,
                                           dsp_stream_t stream)
{
    return rn_fwd("resnorm_train_fwd_state", h, residual, bias, gamma, beta, eps, alpha, keep_scale, thr, seed, offset, rng_state, s, y, stats,
                  act_dtype, param_dtype, R, C, stream);
}

static int rn_bwd(const char* who, const void* dy, const void* ds, const void* s, const float* stats, const void* gamma, float alpha,
                  float keep_scale, unsigned int thr, uint64_t seed, uint64_t offset, const uint64_t* rng_state, void* dh, void* dresidual,
                  void* dbias, void* dgamma, void* dbeta, void* workspace, size_t workspace_bytes, int act_dtype, int param_dtype, int64_t R, int C,
                  dsp_stream_t stream)
{
    const int rc = rn_check(who, act_dtype, param_dtype, (long)R, C, rng_state);
    if (rc) return rc < 0 ? rc : DSP_OK;
    if (!dh && !dresidual && !dbias && !dgamma && !dbeta) return DSP_OK;
    if ((dy && (!s || !stats || !gamma)) || (dh && (dh == dy || dh == ds || dh == s || dh == dresidual)) ||
        (dresidual && (dresidual == dy || dresidual == ds || dresidual == s))) {
        set_error("%s: null or aliased pointer", who); return DSP_EINVAL;
    }
    if (thr > (1u << 24)) { set_error("%s: thr %u above 2^24", who, thr); return DSP_EINVAL; }
    if (!on16(dy, ds, s, gamma, dh, dresidual) || ((uintptr_t)stats & 7)) {
        set_error("%s: tensors must be 16-byte aligned (stats: 8)", who); return DSP_EINVAL;
    }
    const bool sums = dbias || dgamma || dbeta;
    if (sums) DSP_GATE(workspace_gate(who, workspace, workspace_bytes, dsp_resnorm_train_workspace_bytes(R, C), "dsp_resnorm_train_workspace_bytes"));
    int W, NG;
    rn_plan(C / (16 / elem_size(act_dtype)), W, NG);
    const long nchunks = rn_chunks((long)R);
    float* part = sums ? (float*)workspace : (float*)nullptr;
    hipStream_t st = as_stream(stream);
    RN_DISPATCH(act_dtype, NG, hipLaunchKernelGGL((rn_bwd_kernel<E, NGC>), dim3((unsigned)nchunks), dim3(256), 0, st, (const E*)dy, (const E*)ds,
                                                  (const E*)s, stats, gamma, param_dtype, alpha, keep_scale, (uint32_t)thr, seed, offset, rng_state,
                                                  (E*)dh, (E*)dresidual, part, (dh || dbias) ? 1 : 0, (long)R, C, W));
    if (sums)
        hipLaunchKernelGGL(rn_bwd_merge_kernel, dim3((unsigned)((3 * C + 63) / 64)), dim3(256), 0, st, part, nchunks, dgamma, dbeta, dbias, param_dtype, C);
    return check_launch(who);
}

extern "C" int dsp_resnorm_train_bwd(const void* dy, const void* ds, const void* s, const float* stats, const void* gamma, float alpha,
                                     float keep_scale, unsigned int thr, uint64_t seed, uint64_t offset, void* dh, void* dresidual, void* dbias,
                                     void* dgamma, void* dbeta, void* workspace, size_t workspace_bytes, int act_dtype, int param_dtype,
                                     int64_t R, int C, dsp_stream_t stream)
{
    return rn_bwd("resnorm_train_bwd", dy, ds, s, stats, gamma, alpha, keep_scale, thr, seed, offset, nullptr, dh, dresidual, dbias, dgamma, dbeta,
                  workspace, workspace_bytes, act_dtype, param_dtype, R, C, stream);
}

extern "C" int dsp_resnorm_train_bwd_state(const void* dy, const void* ds, const void* s, const float* stats, const void* gamma, float alpha,
                                           float keep_scale, unsigned int thr, uint64_t seed, uint64_t offset, void* dh, void* dresidual,
                                           void* dbias, void* dgamma, void* dbeta, void* workspace, size_t workspace_bytes, int act_dtype,
                                           int param_dtype, int64_t R, int C, const uint64_t* rng_state, dsp_stream_t stream)
{
    return rn_bwd("resnorm_train_bwd_state", dy, ds, s, stats, gamma, alpha, keep_scale, thr, seed, offset, rng_state, dh, dresidual, dbias, dgamma,
                  dbeta, workspace, workspace_bytes, act_dtype, param_dtype, R, C, stream);
}

static int rn_keep_mask(const char* who, uint64_t seed, uint64_t offset, const uint64_t* rng_state, unsigned int thr, unsigned char* out, int64_t n,
                        dsp_stream_t stream)
{
    DSP_GATE(rng_state_gate(who, rng_state));
    if (n < 0 || n > (1L << 36) || thr > (1u << 24)) { set_error("%s: bad arguments n=%ld thr=%u", who, (long)n, thr); return DSP_EINVAL; }
    if (n == 0) return DSP_OK;
    if (!out) { set_error("%s: null pointer", who); return DSP_EINVAL; }
    const long groups = (n + 3) / 4;
    hipLaunchKernelGGL(rn_keep_mask_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, as_stream(stream), seed, offset, rng_state,
                       (uint32_t)thr, out, (long)n);
    return check_launch(who);
}

extern "C" int dsp_dropout_keep_mask(uint64_t seed, uint64_t offset, unsigned int thr, unsigned char* out, int64_t n, dsp_stream_t stream)
{
    return rn_keep_mask("dropout_keep_mask", seed, offset, nullptr, thr, out, n, stream);
}

extern "C" int dsp_dropout_keep_mask_state(uint64_t seed, uint64_t offset, unsigned int thr, unsigned char* out, int64_t n, const uint64_t* rng_state,
                                           dsp_stream_t stream)
{
    return rn_keep_mask("dropout_keep_mask_state", seed, offset, rng_state, thr, out, n, stream);
}

extern "C" int dsp_dropout_state_advance(uint64_t* rng_state, uint64_t by, dsp_stream_t stream)
{
    const char* who = "dropout_state_advance";
    if (!rng_state || ((uintptr_t)rng_state & 7)) { set_error("%s: rng_state must be a non-null, 8-byte aligned pointer", who); return DSP_EINVAL; }
    hipLaunchKernelGGL(rn_state_advance_kernel, dim3(1), dim3(64), 0, as_stream(stream), rng_state, by);
    return check_launch(who);
}
