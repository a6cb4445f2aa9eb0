// glance.hip — the glancing step of DAG training, gfx950 (DASpeech/criterions/nat_dag_loss.py:130-132 force-emit, :223-255 reveal selection).
//
//   force-emit        out[b,t,j] = revealed[b,j] && t != path[b,j] ? -inf : match[b,t,j] — one streaming pass over [B,T,L] (one read, one write),
//                     and its gradient grad[b,t,j] = revealed[b,j] ? 0 : grad_out[b,t,j].  A thread owns four columns: it loads their path /
//                     revealed once and walks the rows of its chunk with 16-byte accesses.  Values are selected, never computed.  No LDS, no
//                     atomics, no scratch.
//   glance_oracle     oracle[b,j] = tgt[b, max(path[b,j], 0)] and the integer count of aligned vertices whose arg-max token equals it.
//   glance_reveal     keep_prob / revealed / glanced per vertex.  number-random and cmlm keep the counts[b] largest scores of a row: the
//                     threshold is found by an exact radix select (4 x 8 bits) on the order-preserving integer image of the floats, the row held
//                     in LDS — no sort.  The histograms are integer counts, so the result does not depend on thread timing.
#include "common.h"
#include "../../include/daspeech_decode.h"

namespace dsp {

constexpr int FE_THREADS = 256;
constexpr int FE_STEPS = 32;                           // rows one thread walks: a chunk is FE_STEPS * (FE_THREADS / TX) rows

// ---- four consecutive elements: 16-byte accesses (VEC) or one element at a time; `sl` (elements between columns) is 1 under VEC
template <typename T> struct Quad { T v[4]; };

template <typename T, bool VEC>
__device__ __forceinline__ Quad<T> load4(const T* __restrict__ p, long sl)
{
    Quad<T> q;
    if constexpr (VEC) {
        constexpr int NQ = 4 * (int)sizeof(T) / 16;
        const uint4* s = reinterpret_cast<const uint4*>(p);
        uint4 u[NQ];
#pragma unroll
        for (int i = 0; i < NQ; ++i) u[i] = s[i];
        __builtin_memcpy(&q, u, sizeof(q));
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) q.v[i] = p[i * sl];
    }
    return q;
}

template <typename T, bool VEC>
__device__ __forceinline__ void store4(T* __restrict__ p, const Quad<T>& q)
{
    if constexpr (VEC) {
        constexpr int NQ = 4 * (int)sizeof(T) / 16;
        uint4 u[NQ];
        __builtin_memcpy(u, &q, sizeof(q));
        uint4* d = reinterpret_cast<uint4*>(p);
#pragma unroll
        for (int i = 0; i < NQ; ++i) d[i] = u[i];
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) p[i] = q.v[i];
    }
}

// BWD = false: force-emit (path != nullptr).  BWD = true: its gradient (path unused).
// grid (column tiles of 4 * TX, row chunks, B); block FE_THREADS = TX column threads x TY row threads.
template <typename T, bool VEC_IN, bool VEC_OUT, bool BWD>
__global__ __launch_bounds__(FE_THREADS) void force_emit_kernel(const T* __restrict__ in, long sb, long st, long sl, const int64_t* __restrict__ path,
                                                                const unsigned char* __restrict__ revealed, T* __restrict__ out, long ldo,
                                                                int T_, int L, int tx_log2)
{
    const int TX = 1 << tx_log2, TY = FE_THREADS >> tx_log2;
    const int tx = threadIdx.x & (TX - 1), ty = threadIdx.x >> tx_log2;
    const int c = (blockIdx.x * TX + tx) * 4;
    if (c >= L) return;
    const int b = blockIdx.z;
    const int n = L - c < 4 ? L - c : 4;                // columns this thread owns
    bool rev[4];
    long p[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        rev[i] = i < n && revealed[(size_t)b * L + c + i] != 0;
        p[i] = (!BWD && i < n) ? (long)path[(size_t)b * L + c + i] : -1;
    }
    const T fill = BWD ? (T)0 : (T)(-__builtin_huge_valf());
    const T* src = in + (size_t)b * sb + (size_t)c * sl;
    T* dst = out + (size_t)b * T_ * ldo + c;
    const int t0 = blockIdx.y * (FE_STEPS * TY) + ty;
    const int t1 = min(T_, (int)(blockIdx.y + 1) * (FE_STEPS * TY));
    if (n == 4) {
#pragma unroll 4
        for (int t = t0; t < t1; t += TY) {
            Quad<T> q = load4<T, VEC_IN>(src + (size_t)t * st, sl);
#pragma unroll
            for (int i = 0; i < 4; ++i) q.v[i] = (rev[i] && (BWD || p[i] != t)) ? fill : q.v[i];
            store4<T, VEC_OUT>(dst + (size_t)t * ldo, q);
        }
    } else {                                            // the tail of a row whose length is off the 4 grid: its own columns only
        for (int t = t0; t < t1; t += TY)
            for (int i = 0; i < n; ++i) {
                const T v = src[(size_t)t * st + i * sl];
                dst[(size_t)t * ldo + i] = (rev[i] && (BWD || p[i] != t)) ? fill : v;
            }
    }
}

static inline bool mult16(const void* base, long sb, long st, int B, int T_, int es)
{
    return ((uintptr_t)base & 15) == 0 && (T_ < 2 || ((st * es) & 15) == 0) && (B < 2 || ((sb * es) & 15) == 0);
}

template <typename T, bool BWD>
static int force_emit_launch(const char* what, const void* in, long sb, long st, long sl, const int64_t* path, const unsigned char* revealed,
                             void* out, long ldo, int B, int T_, int L, hipStream_t stream)
{
    const int es = (int)sizeof(T);
    const bool vin = sl == 1 && mult16(in, sb, st, B, T_, es);
    const bool vout = mult16(out, (long)T_ * ldo, ldo, B, T_, es);
    const int groups = (L + 3) / 4;
    const int tx_log2 = groups <= 16 ? 4 : (groups <= 64 ? 6 : 8);
    const int TX = 1 << tx_log2, TY = FE_THREADS >> tx_log2;
    const long gy = ((long)T_ + FE_STEPS * TY - 1) / (FE_STEPS * TY);
    if (gy > 65535 || B > 65535) { set_error("%s: T = %d / B = %d beyond the grid", what, T_, B); return DSP_EINVAL; }
    const dim3 grid((unsigned)((groups + TX - 1) / TX), (unsigned)gy, (unsigned)B);
#define FE_LAUNCH(VI, VO)                                                                                                               \
    hipLaunchKernelGGL((force_emit_kernel<T, VI, VO, BWD>), grid, dim3(FE_THREADS), 0, stream, (const T*)in, sb, st, sl, path, revealed, \
                       (T*)out, ldo, T_, L, tx_log2)
    if (vin && vout) FE_LAUNCH(true, true);
    else if (vout) FE_LAUNCH(false, true);
    else FE_LAUNCH(false, false);
#undef FE_LAUNCH
    return check_launch(what);
}

static int force_emit_args(const char* what, const void* in, int dtype, int64_t sb, int64_t st, int64_t sl, const void* aux, const void* out,
                           int64_t ldo, int B, int T_, int L)
{
    if (dtype != DSP_F32 && dtype != DSP_F64) { set_error("%s: unsupported dtype %d (DSP_F32 / DSP_F64)", what, dtype); return DSP_EINVAL; }
    if (B < 0 || T_ < 0 || L < 0 || ldo < L || sb < 0 || st < 0 || sl < 0) { set_error("%s: bad sizes", what); return DSP_EINVAL; }
    if ((long)B * T_ * L == 0) return 1;                // nothing to do
    if (!in || !aux || !out) { set_error("%s: null pointer", what); return DSP_EINVAL; }
    return DSP_OK;
}

// ---------------------------------------------------------------- reveal selection
constexpr int GL_THREADS = 256;

__device__ __forceinline__ uint32_t float_key(float f)            // larger float <=> larger key (-0.0 just below +0.0)
{
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_float(uint32_t k)
{
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// one block per sample
__global__ __launch_bounds__(GL_THREADS) void glance_oracle_kernel(const int64_t* __restrict__ tgt, const int64_t* __restrict__ path,
                                                                   const int64_t* __restrict__ guess, int64_t* __restrict__ oracle,
                                                                   int64_t* __restrict__ n_right, int T_, int L)
{
    __shared__ int part[GL_THREADS / 64];
    const int b = blockIdx.x;
    int cnt = 0;
    for (int j = threadIdx.x; j < L; j += GL_THREADS) {
        const long p = (long)path[(size_t)b * L + j];
        long q = p < 0 ? 0 : p;
        q = q > T_ - 1 ? T_ - 1 : q;                    // a path never points beyond the target; keeps the read inside tgt if one does
        const int64_t o = tgt[(size_t)b * T_ + q];
        oracle[(size_t)b * L + j] = o;
        cnt += (p >= 0 && guess[(size_t)b * L + j] == o);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int w = 0; w < GL_THREADS / 64; ++w) s += part[w];
        n_right[b] = s;
    }
}

// one block per sample; dynamic LDS: L keys (mode 1)
__global__ __launch_bounds__(GL_THREADS) void glance_reveal_kernel(const float* __restrict__ scores, const void* __restrict__ param, int mode,
                                                                   const float* __restrict__ unif, const int64_t* __restrict__ path,
                                                                   const int64_t* __restrict__ oracle, const int64_t* __restrict__ prev,
                                                                   float* __restrict__ keep_prob, unsigned char* __restrict__ revealed,
                                                                   int64_t* __restrict__ glanced, int L)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t keys[];
    __shared__ int hist[256];
    __shared__ uint32_t sel[2];                          // chosen key prefix, rank left inside it
    const int b = blockIdx.x;
    const size_t row = (size_t)b * L;
    float thr = 0.f, prob = 0.f;
    if (mode == 0) {
        prob = ((const float*)param)[b];
    } else {
        const long cnt = (long)((const int64_t*)param)[b];
        for (int j = threadIdx.x; j < L; j += GL_THREADS)
            keys[j] = float_key(path[row + j] >= 0 ? scores[row + j] : -100.f);
        long r = cnt - 1;                               // the threshold is the score of rank r from the top
        r = r < 0 ? 0 : (r > L - 1 ? L - 1 : r);
        if (threadIdx.x == 0) { sel[0] = 0u; sel[1] = (uint32_t)r; }
        for (int shift = 24; shift >= 0; shift -= 8) {
            hist[threadIdx.x] = 0;                      // GL_THREADS == 256 bins
            __syncthreads();
            const uint32_t prefix = sel[0];
            const uint32_t himask = shift == 24 ? 0u : (0xffffffffu << (shift + 8));
            for (int j = threadIdx.x; j < L; j += GL_THREADS) {
                const uint32_t k = keys[j];
                if ((k & himask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1);
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                uint32_t left = sel[1];
                int d = 255;
                for (; d > 0; --d) {
                    const uint32_t h = (uint32_t)hist[d];
                    if (left < h) break;
                    left -= h;
                }
                sel[0] = prefix | ((uint32_t)d << shift);
                sel[1] = left;
            }
            __syncthreads();
        }
        thr = cnt == 0 ? 100.f : key_float(sel[0]);
    }
    for (int j = threadIdx.x; j < L; j += GL_THREADS) {
        const bool on = path[row + j] >= 0;
        float kp;
        if (mode == 0) kp = prob * (on ? 1.f : 0.f);
        else kp = key_float(keys[j]) >= thr ? 1.f : 0.f;
        const bool rv = unif[row + j] < kp;
        keep_prob[row + j] = kp;
        revealed[row + j] = rv ? 1 : 0;
        glanced[row + j] = rv ? oracle[row + j] : prev[row + j];
    }
}

}  // namespace dsp

using namespace dsp;

extern "C" int dsp_force_emit(const void* match, int dtype, int64_t sb, int64_t st, const int64_t* path, const unsigned char* revealed,
                              void* out, int64_t ldo, int B, int T, int L, dsp_stream_t stream)
{
    const int rc = force_emit_args("force_emit", match, dtype, sb, st, 1, path, out, ldo, B, T, L);
    if (rc) return rc > 0 ? DSP_OK : rc;
    if (!revealed) { set_error("force_emit: null pointer"); return DSP_EINVAL; }
    if (dtype == DSP_F32)
        return force_emit_launch<float, false>("force_emit", match, sb, st, 1, path, revealed, out, ldo, B, T, L, as_stream(stream));
    return force_emit_launch<double, false>("force_emit", match, sb, st, 1, path, revealed, out, ldo, B, T, L, as_stream(stream));
}

extern "C" int dsp_force_emit_bwd(const void* grad_out, int dtype, int64_t sb, int64_t st, int64_t sl, const unsigned char* revealed,
                                  void* grad_match, int64_t ldg, int B, int T, int L, dsp_stream_t stream)
{
    const int rc = force_emit_args("force_emit_bwd", grad_out, dtype, sb, st, sl, revealed, grad_match, ldg, B, T, L);
    if (rc) return rc > 0 ? DSP_OK : rc;
    if (dtype == DSP_F32)
        return force_emit_launch<float, true>("force_emit_bwd", grad_out, sb, st, sl, nullptr, revealed, grad_match, ldg, B, T, L, as_stream(stream));
    return force_emit_launch<double, true>("force_emit_bwd", grad_out, sb, st, sl, nullptr, revealed, grad_match, ldg, B, T, L, as_stream(stream));
}

extern "C" int dsp_glance_oracle(const int64_t* tgt, const int64_t* path, const int64_t* guess, int64_t* oracle, int64_t* n_right,
                                 int B, int T, int L, dsp_stream_t stream)
{
    if (B < 0 || T < 1 || L < 1) { set_error("glance_oracle: bad sizes"); return DSP_EINVAL; }
    if (B == 0) return DSP_OK;
    if (!tgt || !path || !guess || !oracle || !n_right) { set_error("glance_oracle: null pointer"); return DSP_EINVAL; }
    hipLaunchKernelGGL(glance_oracle_kernel, dim3((unsigned)B), dim3(GL_THREADS), 0, as_stream(stream), tgt, path, guess, oracle, n_right, T, L);
    return check_launch("glance_oracle");
}

extern "C" int dsp_glance_reveal(const float* scores, const void* param, int mode, const float* unif, const int64_t* path, const int64_t* oracle,
                                 const int64_t* prev, float* keep_prob, unsigned char* revealed, int64_t* glanced, int B, int L,
                                 dsp_stream_t stream)
{
    if (mode != DSP_GLANCE_PROB && mode != DSP_GLANCE_COUNT) { set_error("glance_reveal: mode %d", mode); return DSP_EINVAL; }
    if (B < 0 || L < 1 || L > DSP_GLANCE_MAX_L) { set_error("glance_reveal: L = %d (1 .. %d)", L, DSP_GLANCE_MAX_L); return DSP_EINVAL; }
    if (B == 0) return DSP_OK;
    if (!param || !unif || !path || !oracle || !prev || !keep_prob || !revealed || !glanced || (mode == DSP_GLANCE_COUNT && !scores)) {
        set_error("glance_reveal: null pointer");
        return DSP_EINVAL;
    }
    const size_t lds = mode == DSP_GLANCE_COUNT ? (size_t)L * sizeof(uint32_t) : 0;
    hipLaunchKernelGGL(glance_reveal_kernel, dim3((unsigned)B), dim3(GL_THREADS), lds, as_stream(stream), scores, param, mode, unif, path, oracle,
                       prev, keep_prob, revealed, glanced, L);
    return check_launch("glance_reveal");
}
