// posterior_f64.hip — F1 (posterior of the expect strategy) and its fused product with the features for DOUBLE alpha / beta (gfx950).
//
// The reference computes exp(alpha + beta - logsumexp) in the dtype of alpha (s2s_dag_fastspeech2_loss.py:259-262), so a float64
// (alpha, beta) pair from the double DP (dag_dp_f64.hip) gives a float64 posterior.  The kernels of decode_tts.hip compute in fp32 and
// keep whole rows in LDS; these are their double counterparts — same stance as dag_dp_f64.hip / logsoftmax_gather_f64.hip: every
// intermediate is a double (lane accumulators, wave shuffles, LDS tiles, the row statistics) and only the accurate exp / log are used.
//
//   dsp_posterior_f64               score[b,t,:] = exp(a + b - LSE_j(a + b)); a row without a finite entry gives zeros
//   dsp_posterior_features_f64      out[b,t,:]  = sum_j score[b,t,j] * features[b,j,:]      (+ lse[B,T], -inf for dead rows)
//   dsp_posterior_features_bwd_f64  dF[b,j,:]   = sum_t score[b,t,j] * dOut[b,t,:]          (score rebuilt from alpha, beta, lse)
//
// Row pass (p64_rows_kernel): one wave per (b, t) row — exact maximum, sum of exp(s - max), lse = max + log(sum), the operations of the
// reference in its order; it writes `lse` and / or the normalised row.
//
// Product pass (p64_product_kernel<NC, BWD, OWN_LSE>): a blocked matrix product out[M, D] = P[M, K] . X[K, D] per sample whose left
// operand is never read from memory but rebuilt tile by tile:  forward M = T, K = L, P[m][k] = exp(s[m][k] - lse[m]);  backward M = L,
// K = T, P[m][k] = exp(s[k][m] - lse[k]).  A 256-thread workgroup owns TM = 32 rows x TN = 64 NC columns (NC = 1, 2 or 4 by the feature
// width) and walks K in chunks of KC = 16: the chunk's P tile (2 exp per thread) and X tile go to LDS, each thread accumulates a
// 4 x 2 NC register tile with v_fma_f64, P as two 16-byte LDS broadcasts and X as NC 16-byte LDS reads per k.  LDS is 4.3 KB + 8 NC KB
// whatever L and T are, which is what lets the double path reach L = 10240 (a [8][L] image of doubles would end at L = 2400).
// The reduction over K is one fixed sequential chain per output element and no atomics are used: two calls give the same bits.
// Any T, L, D >= 1 (odd D and D = 1 included: X loads and output stores are per element, bounds checked).
// When the caller wants no `lse` (NULL) the forward builds the statistics of its 32 rows itself (OWN_LSE), once per column slab.
//
// Plain FMA, not v_mfma_f64_16x16x4_f64: on this part the f64 matrix instruction has the vector unit's rate (no throughput to gain), and
// the FMA chain has an order that is easy to state and to reproduce on a CPU.
#include "common.h"
#include "../../include/daspeech_decode.h"

namespace dsp {

#define P64_NEG (-__builtin_huge_val())
typedef double p64_d2 __attribute__((ext_vector_type(2)));

constexpr int P64_TM = 32;             // output rows per workgroup
constexpr int P64_KC = 16;             // reduction chunk
constexpr int P64_AS = P64_TM + 2;     // row stride of the P tile [KC][TM + 2]: 16-byte aligned rows, conflict-free writes along k

// log-sum-exp of one row of alpha + beta by one wave; -inf for a row without a finite entry (or with a +inf / NaN maximum)
__device__ __forceinline__ double p64_row_lse(const double* __restrict__ a, const double* __restrict__ b, int L, int lane) {
    double m = P64_NEG;
    for (int j = lane; j < L; j += 64) m = fmax(m, a[j] + b[j]);
    m = wave_max(m);
    if (!(m > P64_NEG) || isinf(m)) return P64_NEG;
    double s = 0.0;
    for (int j = lane; j < L; j += 64) s += exp(a[j] + b[j] - m);
    s = wave_sum(s);
    return m + log(s);
}

__global__ __launch_bounds__(256) void p64_rows_kernel(const double* __restrict__ alpha, const double* __restrict__ beta,
                                                       double* __restrict__ score, double* __restrict__ lse_out, long nrows, int L)
{
    const int lane = threadIdx.x & 63;
    for (long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6); row < nrows; row += (long)gridDim.x * 4) {
        const double* a = alpha + (size_t)row * L; const double* b = beta + (size_t)row * L;
        const double lse = p64_row_lse(a, b, L, lane);
        if (lse_out && lane == 0) lse_out[row] = lse;
        if (score) {
            double* o = score + (size_t)row * L;
            if (lse == P64_NEG) { for (int j = lane; j < L; j += 64) o[j] = 0.0; }
            else { for (int j = lane; j < L; j += 64) o[j] = exp(a[j] + b[j] - lse); }
        }
    }
}

template <int NC, bool BWD, bool OWN_LSE>
__global__ __launch_bounds__(256) void p64_product_kernel(const double* __restrict__ alpha, const double* __restrict__ beta,
                                                          const double* __restrict__ lse, const double* __restrict__ X,
                                                          double* __restrict__ out, int T, int L, int D)
{
    constexpr int TN = 64 * NC;
    __shared__ __attribute__((aligned(16))) double As[P64_KC * P64_AS];
    __shared__ __attribute__((aligned(16))) double Bs[P64_KC * TN];
    __shared__ double lse_s[P64_TM];
    const int M = BWD ? L : T, K = BWD ? T : L;
    const int b = blockIdx.z, m0 = blockIdx.y * P64_TM, n0 = blockIdx.x * TN;
    const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
    const double* A0 = alpha + (size_t)b * T * L; const double* B0 = beta + (size_t)b * T * L;
    const double* Xb = X + (size_t)b * K * D;
    if (!BWD) {                                            // the 32 rows' statistics: from the row pass, or built here
        if (OWN_LSE) {
            const int lane = tid & 63, wave = tid >> 6;
            for (int r = wave; r < P64_TM; r += 4) {
                const int t = m0 + r;
                const double v = t < T ? p64_row_lse(A0 + (size_t)t * L, B0 + (size_t)t * L, L, lane) : P64_NEG;
                if (lane == 0) lse_s[r] = v;
            }
        } else if (tid < P64_TM) {
            lse_s[tid] = (m0 + tid < T) ? lse[(size_t)b * T + m0 + tid] : P64_NEG;
        }
    }
    double acc[4][2 * NC];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < 2 * NC; ++c) acc[i][c] = 0.0;

    for (int k0 = 0; k0 < K; k0 += P64_KC) {
        __syncthreads();                                   // the previous chunk's readers are done (first pass: lse_s is written)
#pragma unroll
        for (int u = 0; u < P64_KC * P64_TM / 256; ++u) {  // P tile: consecutive threads walk the contiguous axis of alpha / beta
            const int e = tid + u * 256;
            const int k = BWD ? e / P64_TM : e % P64_KC, r = BWD ? e % P64_TM : e / P64_KC;
            const int t = BWD ? k0 + k : m0 + r, j = BWD ? m0 + r : k0 + k;
            double pv = 0.0;
            if (t < T && j < L) {
                const double ls = BWD ? lse[(size_t)b * T + t] : lse_s[r];
                if (ls != P64_NEG) { const size_t o = (size_t)t * L + j; pv = exp(A0[o] + B0[o] - ls); }
            }
            As[k * P64_AS + r] = pv;
        }
#pragma unroll
        for (int u = 0; u < P64_KC * TN / 256; ++u) {      // X tile: rows of features / grad_out, zero beyond K and D
            const int e = tid + u * 256;
            const int k = e / TN, c = e - k * TN;
            Bs[e] = (k0 + k < K && n0 + c < D) ? Xb[(size_t)(k0 + k) * D + n0 + c] : 0.0;
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < P64_KC; ++k) {
            const p64_d2 a01 = *reinterpret_cast<const p64_d2*>(&As[k * P64_AS + ty * 4]);
            const p64_d2 a23 = *reinterpret_cast<const p64_d2*>(&As[k * P64_AS + ty * 4 + 2]);
            const double av[4] = {a01.x, a01.y, a23.x, a23.y};
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const p64_d2 x = *reinterpret_cast<const p64_d2*>(&Bs[k * TN + c * 64 + tx * 2]);
#pragma unroll
                for (int i = 0; i < 4; ++i) { acc[i][2 * c] = fma(av[i], x.x, acc[i][2 * c]); acc[i][2 * c + 1] = fma(av[i], x.y, acc[i][2 * c + 1]); }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + ty * 4 + i;
        if (m >= M) continue;
        double* o = out + ((size_t)b * M + m) * D;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const int n = n0 + c * 64 + tx * 2;
            if (n < D) o[n] = acc[i][2 * c];
            if (n + 1 < D) o[n + 1] = acc[i][2 * c + 1];
        }
    }
}

template <bool BWD, bool OWN_LSE>
static void launch_product64(const double* alpha, const double* beta, const double* lse, const double* X, double* out,
                             int B, int T, int L, int D, hipStream_t st)
{
    const int M = BWD ? L : T;
    const int NC = D <= 64 ? 1 : (D <= 128 ? 2 : 4);
    const dim3 grid((D + 64 * NC - 1) / (64 * NC), (M + P64_TM - 1) / P64_TM, B);
    if (NC == 1) hipLaunchKernelGGL((p64_product_kernel<1, BWD, OWN_LSE>), grid, dim3(256), 0, st, alpha, beta, lse, X, out, T, L, D);
    else if (NC == 2) hipLaunchKernelGGL((p64_product_kernel<2, BWD, OWN_LSE>), grid, dim3(256), 0, st, alpha, beta, lse, X, out, T, L, D);
    else hipLaunchKernelGGL((p64_product_kernel<4, BWD, OWN_LSE>), grid, dim3(256), 0, st, alpha, beta, lse, X, out, T, L, D);
}

static int launch_rows64(const double* alpha, const double* beta, double* score, double* lse, int B, int T, int L, hipStream_t st)
{
    const long nrows = (long)B * T;
    const long g = (nrows + 3) / 4;
    hipLaunchKernelGGL(p64_rows_kernel, dim3((unsigned)(g < 16384 ? g : 16384)), dim3(256), 0, st, alpha, beta, score, lse, nrows, L);
    return DSP_OK;
}

}  // namespace dsp

using namespace dsp;

extern "C" int dsp_posterior_f64(const double* alpha, const double* beta, double* score, int B, int T, int L, dsp_stream_t stream)
{
    if (B < 0 || T < 1 || L < 1) { set_error("posterior_f64: bad sizes B=%d T=%d L=%d", B, T, L); return DSP_EINVAL; }
    if (B == 0) return DSP_OK;
    if (!alpha || !beta || !score) { set_error("posterior_f64: null pointer"); return DSP_EINVAL; }
    launch_rows64(alpha, beta, score, nullptr, B, T, L, as_stream(stream));
    return check_launch("posterior_f64");
}

extern "C" int dsp_posterior_features_f64(const double* alpha, const double* beta, const double* features, double* out, double* lse,
                                          int B, int T, int L, int D, dsp_stream_t stream)
{
    if (B < 0 || T < 1 || L < 1 || D < 1) { set_error("posterior_features_f64: bad sizes B=%d T=%d L=%d D=%d", B, T, L, D); return DSP_EINVAL; }
    if (B == 0) return DSP_OK;
    if (!alpha || !beta || !features || !out) { set_error("posterior_features_f64: null pointer"); return DSP_EINVAL; }
    if (B > 65535 || (T + P64_TM - 1) / P64_TM > 65535) { set_error("posterior_features_f64: B=%d / T=%d beyond the launch grid", B, T); return DSP_EINVAL; }
    hipStream_t st = as_stream(stream);
    if (lse) {
        launch_rows64(alpha, beta, nullptr, lse, B, T, L, st);
        const int rc = check_launch("posterior_features_f64(rows)");
        if (rc != DSP_OK) return rc;
        launch_product64<false, false>(alpha, beta, lse, features, out, B, T, L, D, st);
    } else {
        launch_product64<false, true>(alpha, beta, nullptr, features, out, B, T, L, D, st);
    }
    return check_launch("posterior_features_f64");
}

extern "C" int dsp_posterior_features_bwd_f64(const double* alpha, const double* beta, const double* lse, const double* grad_out,
                                              double* grad_features, int B, int T, int L, int D, dsp_stream_t stream)
{
    if (B < 0 || T < 1 || L < 1 || D < 1) { set_error("posterior_features_bwd_f64: bad sizes B=%d T=%d L=%d D=%d", B, T, L, D); return DSP_EINVAL; }
    if (B == 0) return DSP_OK;
    if (!alpha || !beta || !lse || !grad_out || !grad_features) { set_error("posterior_features_bwd_f64: null pointer"); return DSP_EINVAL; }
    if (B > 65535 || (L + P64_TM - 1) / P64_TM > 65535) { set_error("posterior_features_bwd_f64: B=%d / L=%d beyond the launch grid", B, L); return DSP_EINVAL; }
    launch_product64<true, false>(alpha, beta, lse, grad_out, grad_features, B, T, L, D, as_stream(stream));
    return check_launch("posterior_features_bwd_f64");
}
