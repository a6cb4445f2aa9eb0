// fp16_optim.hip — the optimizer half of the fp16 training step, gfx950 (fairseq/optim/fp16_optimizer.py:111-211 + fairseq/optim/adam.py; C ABI
// and the multi-tensor problem: include/daspeech_optim.h).
//
//   grad_sumsq   S = sum float(g)^2 over the 16-bit gradients: 2 B per element, one fp32 partial per work item, one workgroup adds them in double.
//   adam_step    g = c * float(g16), decoupled decay, Adam on the flat fp32 master / exp_avg / exp_avg_sq, the 16-bit parameter rounded from the
//                stored master: 2 + 12 read, 12 + 2 written per element, no flat fp32 gradient.
//   scale_step   one thread: from S and the optimizer state (a block of 8-byte slots, daspeech_optim.h) the norm, the overflow decision, the
//                clip coefficient, the loss scale, the step count with its bias corrections and the Adam scalars — the host arithmetic of
//                FP16FlatOptimizer._step_hip and DynamicLossScaler in double, bit for bit, so that a step waits for nothing.
//   adam_step_state   adam_step with its scalars and the `applied` flag read from that state instead of the argument list: the same kernel.
//
// One workgroup serves one work item (a run of <= chunk elements of one tensor).  The fp32 streams carry 24 of the 28 bytes of an element, so they
// decide the layout: an item peels elements until its FLAT index is a multiple of 4, then every thread moves groups of four as float4; what is
// left over (<= 3 + 3 elements) goes one at a time.  The 16-bit side of a group sits wherever the tensor's flat offset puts it: 8-byte, 4-byte
// or 2-byte pieces, chosen once per item (uniform over the workgroup).  The sum of squares is grouped by eight from the item's first element —
// by index, not by address — so that its summation order, and with it every bit of S, does not depend on where the gradients were allocated.
// No LDS beyond the reductions' few words, no atomics, no scratch.
#include "common.h"
#include "host_gates.h"
#include "../../include/daspeech_optim.h"

namespace dsp {

constexpr int FO_THREADS = 256;
constexpr int FO_CHUNK_GRID = 2048, FO_CHUNK_MAX = 65536;

// N consecutive 16-bit elements <-> floats through pieces of A bytes (A = 2: one element at a time); p is A-byte aligned
template <typename T, int N, int A> __device__ __forceinline__ void load_pieces(const T* __restrict__ p, float* f)
{
    if constexpr (A == 2) {
#pragma unroll
        for (int i = 0; i < N; ++i) f[i] = to_f(p[i]);
    } else {
        constexpr int WP = A / 4;                       // 32-bit words per access
        static_assert((N / 2) % WP == 0, "load_pieces: N elements in whole pieces");
        uint32_t w[N / 2];
#pragma unroll
        for (int i = 0; i < N / 2; i += WP) {
            if constexpr (WP == 4) {
                const uint4 u = *reinterpret_cast<const uint4*>(p + 2 * i);
                w[i] = u.x; w[i + 1] = u.y; w[i + 2] = u.z; w[i + 3] = u.w;
            } else if constexpr (WP == 2) {
                const uint2 u = *reinterpret_cast<const uint2*>(p + 2 * i);
                w[i] = u.x; w[i + 1] = u.y;
            } else {
                w[i] = *reinterpret_cast<const uint32_t*>(p + 2 * i);
            }
        }
#pragma unroll
        for (int i = 0; i < N / 2; ++i) Word<T>::unpack(w[i], f + 2 * i);
    }
}
template <typename T, int N, int A> __device__ __forceinline__ void store_pieces(T* __restrict__ p, const float* f)
{
    if constexpr (A == 2) {
#pragma unroll
        for (int i = 0; i < N; ++i) p[i] = from_f<T>(f[i]);
    } else {
        constexpr int WP = A / 4;
        static_assert((N / 2) % WP == 0, "store_pieces: N elements in whole pieces");
        uint32_t w[N / 2];
#pragma unroll
        for (int i = 0; i < N / 2; ++i) w[i] = Word<T>::pack(f + 2 * i);
#pragma unroll
        for (int i = 0; i < N / 2; i += WP) {
            if constexpr (WP == 2) *reinterpret_cast<uint2*>(p + 2 * i) = make_uint2(w[i], w[i + 1]);
            else *reinterpret_cast<uint32_t*>(p + 2 * i) = w[i];
        }
    }
}

// ---------------------------------------------------------------- sum of squares
template <typename T, int A>
__device__ __forceinline__ float sumsq_groups(const T* __restrict__ g, int ngroups)
{
    float acc = 0.f;
    for (int i = threadIdx.x; i < ngroups; i += FO_THREADS) {
        float f[8];
        load_pieces<T, 8, A>(g + 8 * (size_t)i, f);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc += f[j] * f[j];
    }
    return acc;
}

// grid: one workgroup per item.  partial[item] = sum of squares of the item's gradient elements: thread t adds the groups of eight
// t, t + 256, ... in that order, then element 8 * ngroups + t of the tail; butterfly over the wave; the four waves in order.
template <typename T>
__global__ __launch_bounds__(FO_THREADS) void fo_sumsq_kernel(const void* const* __restrict__ grads, const int64_t* __restrict__ items,
                                                              float* __restrict__ partial)
{
    __shared__ float wsum[FO_THREADS / DSP_WAVE];
    const int64_t* it = items + 3 * (size_t)blockIdx.x;
    const T* g = (const T*)grads[it[0]];
    if (g == nullptr) {                                 // uniform over the workgroup
        if (threadIdx.x == 0) partial[blockIdx.x] = 0.f;
        return;
    }
    g += it[1];
    const int cnt = (int)it[2];
    const int ngroups = cnt >> 3, ntail = cnt & 7;
    const unsigned a = (unsigned)((uintptr_t)g & 15u);
    float acc;
    if (a == 0) acc = sumsq_groups<T, 16>(g, ngroups);
    else if ((a & 7u) == 0) acc = sumsq_groups<T, 8>(g, ngroups);
    else if ((a & 3u) == 0) acc = sumsq_groups<T, 4>(g, ngroups);
    else acc = sumsq_groups<T, 2>(g, ngroups);
    if ((int)threadIdx.x < ntail) {
        const float f = to_f(g[8 * (size_t)ngroups + threadIdx.x]);
        acc += f * f;
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & (DSP_WAVE - 1)) == 0) wsum[threadIdx.x / DSP_WAVE] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = wsum[0];
#pragma unroll
        for (int w = 1; w < FO_THREADS / DSP_WAVE; ++w) s += wsum[w];
        partial[blockIdx.x] = s;
    }
}

// one workgroup: S = sum of the partials in double; thread t adds items t, t + 256, ... ascending, thread 0 the 256 sums ascending
__global__ __launch_bounds__(FO_THREADS) void fo_sumsq_tail_kernel(const float* __restrict__ partial, int64_t n_items, double* __restrict__ S)
{
    __shared__ double tsum[FO_THREADS];
    double s = 0.0;
    for (int64_t k = threadIdx.x; k < n_items; k += FO_THREADS) s += (double)partial[k];
    tsum[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double r = 0.0;
        for (int t = 0; t < FO_THREADS; ++t) r += tsum[t];
        *S = r;
    }
}

// ---------------------------------------------------------------- Adam
struct AdamScalars {
    float c, beta1, beta2, eps, decay, step, omb1, omb2, sqrt_bias2;      // decay = 1 - lr*wd, step = lr / bias1, omb = 1 - beta
};

__device__ __forceinline__ void adam_one(float g16, float& p, float& m, float& v, const AdamScalars& k)
{
    const float g = k.c * g16;
    p = p * k.decay;
    m = k.beta1 * m + k.omb1 * g;
    v = k.beta2 * v + k.omb2 * g * g;
    p = p - k.step * m / (sqrtf(v) / k.sqrt_bias2 + k.eps);
}

// the groups of four from `head` on: fp32 as float4 (P + head is 16-byte aligned), the 16-bit side in pieces of A bytes
template <typename T, int A, bool HAS_G>
__device__ __forceinline__ void adam_groups(const T* __restrict__ g, T* __restrict__ q, float* __restrict__ P, float* __restrict__ M,
                                            float* __restrict__ V, int nvec, const AdamScalars& k)
{
#pragma unroll 2
    for (int i = threadIdx.x; i < nvec; i += FO_THREADS) {
        const size_t e = 4 * (size_t)i;
        float gf[4] = {0.f, 0.f, 0.f, 0.f};
        if constexpr (HAS_G) load_pieces<T, 4, A>(g + e, gf);
        const float4 p4 = *reinterpret_cast<const float4*>(P + e);
        const float4 m4 = *reinterpret_cast<const float4*>(M + e);
        const float4 v4 = *reinterpret_cast<const float4*>(V + e);
        float p[4] = {p4.x, p4.y, p4.z, p4.w}, m[4] = {m4.x, m4.y, m4.z, m4.w}, v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) adam_one(gf[j], p[j], m[j], v[j], k);
        *reinterpret_cast<float4*>(P + e) = make_float4(p[0], p[1], p[2], p[3]);
        *reinterpret_cast<float4*>(M + e) = make_float4(m[0], m[1], m[2], m[3]);
        *reinterpret_cast<float4*>(V + e) = make_float4(v[0], v[1], v[2], v[3]);
        store_pieces<T, 4, A>(q + e, p);
    }
}

// where the kernel takes its scalars from: the argument list (the host decided that the step is applied), or the optimizer state that
// fo_scale_step_kernel wrote in the launch before (applied == 0: the workgroup returns before its first store)
struct ScalarsByValue {
    AdamScalars k;
    __device__ __forceinline__ bool load(AdamScalars& out) const { out = k; return true; }
};
struct ScalarsFromState {
    const uint64_t* state;
    __device__ __forceinline__ bool load(AdamScalars& out) const
    {
        if (*reinterpret_cast<const int*>(state + DSP_OPTIM_SLOT_APPLIED) == 0) return false;      // uniform over the grid
        out = *reinterpret_cast<const AdamScalars*>(state + DSP_OPTIM_SLOT_SCALARS);
        return true;
    }
};

// grid: one workgroup per item
template <typename T, typename SRC>
__global__ __launch_bounds__(FO_THREADS) void fo_adam_kernel(const void* const* __restrict__ grads, void* const* __restrict__ params16,
                                                             const int64_t* __restrict__ offsets, const int64_t* __restrict__ items,
                                                             float* __restrict__ master, float* __restrict__ exp_avg,
                                                             float* __restrict__ exp_avg_sq, SRC src)
{
    AdamScalars k;
    if (!src.load(k)) return;
    const int64_t* it = items + 3 * (size_t)blockIdx.x;
    const int64_t ti = it[0], first = it[1];
    const int cnt = (int)it[2];
    const T* g = (const T*)grads[ti];
    const bool has_g = g != nullptr;                    // uniform over the workgroup
    if (has_g) g += first;
    T* q = (T*)params16[ti] + first;
    const int64_t f0 = offsets[ti] + first;
    float *P = master + f0, *M = exp_avg + f0, *V = exp_avg_sq + f0;
    int head = (int)((4 - (f0 & 3)) & 3);               // elements before the flat index reaches a multiple of 4
    head = head < cnt ? head : cnt;
    const int nvec = (cnt - head) >> 2;
    const int tail0 = head + 4 * nvec;
    // head and tail, at most 3 + 3 elements, one thread each
    {
        const int t = (int)threadIdx.x;
        int e = -1;
        if (t < head) e = t;
        else if (t - head < cnt - tail0) e = tail0 + (t - head);
        if (e >= 0) {
            float p = P[e], m = M[e], v = V[e];
            adam_one(has_g ? to_f(g[e]) : 0.f, p, m, v, k);
            P[e] = p; M[e] = m; V[e] = v;
            q[e] = from_f<T>(p);
        }
    }
    if (nvec == 0) return;
    const unsigned a = (unsigned)(((uintptr_t)(q + head) | (has_g ? (uintptr_t)(g + head) : (uintptr_t)0)) & 7u);
#define FO_GROUPS(A)                                                                                    \
    do {                                                                                                \
        if (has_g) adam_groups<T, A, true>(g + head, q + head, P + head, M + head, V + head, nvec, k);  \
        else adam_groups<T, A, false>(nullptr, q + head, P + head, M + head, V + head, nvec, k);        \
    } while (0)
    if (a == 0) FO_GROUPS(8);
    else if ((a & 3u) == 0) FO_GROUPS(4);
    else FO_GROUPS(2);
#undef FO_GROUPS
}

static_assert(sizeof(AdamScalars) == 4 * DSP_OPTIM_N_SCALARS, "AdamScalars: the floats of the state's scalar slots");
static_assert(8 * (DSP_OPTIM_STATE_SLOTS - DSP_OPTIM_SLOT_SCALARS) >= (int)sizeof(AdamScalars), "AdamScalars past the end of the state");

// The Adam scalars derived in double and rounded once: 1 - beta2 from a float beta2 would carry the float's error at 1000 x its relative size.
// One function for the host entry and the device update.  Contraction off: hipcc contracts by default, and 1 - lr*wd fused into an fma on
// the device would differ in the last bit from what the host computes.
__host__ __device__ inline AdamScalars derive_scalars(double c, double lr, double beta1, double beta2, double eps, double lr_wd, double bias1,
                                                      double sqrt_bias2)
{
#pragma clang fp contract(off)
    AdamScalars k;
    k.c = (float)c; k.beta1 = (float)beta1; k.beta2 = (float)beta2; k.eps = (float)eps;
    k.decay = (float)(1.0 - lr_wd); k.step = (float)(lr / bias1); k.omb1 = (float)(1.0 - beta1); k.omb2 = (float)(1.0 - beta2);
    k.sqrt_bias2 = (float)sqrt_bias2;
    return k;
}

struct ScaleConsts {
    double beta1, beta2, eps, weight_decay, clip_norm, scale_factor, min_loss_scale;
    int64_t scale_window;
};

// One thread.  Every operation is an IEEE double multiply, add, divide or square root in the order of FP16FlatOptimizer._step_hip and
// DynamicLossScaler, so plain host floats reproduce every slot bit for bit — which holds only with floating-point contraction OFF in this
// body: hipcc contracts by default, and 1 - pow1*beta1 or 1 - lr*wd fused into an fma would differ from the host in the last bit.
// Plain vector stores, no atomics.
__global__ __launch_bounds__(64) void fo_scale_step_kernel(const double* __restrict__ S_ptr, uint64_t* __restrict__ state, ScaleConsts k)
{
#pragma clang fp contract(off)
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double* sd = reinterpret_cast<double*>(state);
    int64_t* si = reinterpret_cast<int64_t*>(state);
    const double S = *S_ptr;
    double loss_scale = sd[DSP_OPTIM_SLOT_LOSS_SCALE];
    int64_t iter = si[DSP_OPTIM_SLOT_ITER];
    const double lr = sd[DSP_OPTIM_SLOT_LR];
    double c = sd[DSP_OPTIM_SLOT_GRAD_MULT] / loss_scale;
    const double nv = (S == S && S >= 0.0) ? fabs(c) * sqrt(S) : __builtin_nan("");
    sd[DSP_OPTIM_SLOT_GRAD_NORM] = nv;
    int* applied = reinterpret_cast<int*>(state + DSP_OPTIM_SLOT_APPLIED);
    if (nv != nv || nv == __builtin_inf()) {            // the overflow: the scale shrinks, nothing else moves
        si[DSP_OPTIM_SLOT_LAST_OVERFLOW_ITER] = iter;
        loss_scale = loss_scale / k.scale_factor;
        iter += 1;
        if (loss_scale <= k.min_loss_scale) *reinterpret_cast<int*>(state + DSP_OPTIM_SLOT_FLOOR_HIT) = 1;      // sticky
        *applied = 0;
    } else {
        if (k.clip_norm > 0.0 && nv > k.clip_norm) c = c * (k.clip_norm / (nv + 1e-6));
        const double pow1 = sd[DSP_OPTIM_SLOT_POW1] * k.beta1, pow2 = sd[DSP_OPTIM_SLOT_POW2] * k.beta2;
        si[DSP_OPTIM_SLOT_T] += 1;
        sd[DSP_OPTIM_SLOT_POW1] = pow1;
        sd[DSP_OPTIM_SLOT_POW2] = pow2;
        const double bias1 = 1.0 - pow1, sqrt_bias2 = sqrt(1.0 - pow2);
        *reinterpret_cast<AdamScalars*>(state + DSP_OPTIM_SLOT_SCALARS) =
            derive_scalars(c, lr, k.beta1, k.beta2, k.eps, lr * k.weight_decay, bias1, sqrt_bias2);
        *applied = 1;
        if ((iter - si[DSP_OPTIM_SLOT_LAST_OVERFLOW_ITER]) % k.scale_window == 0) loss_scale = loss_scale * k.scale_factor;
        iter += 1;
    }
    sd[DSP_OPTIM_SLOT_LOSS_SCALE] = loss_scale;
    si[DSP_OPTIM_SLOT_ITER] = iter;
    *reinterpret_cast<float*>(state + DSP_OPTIM_SLOT_LOSS_SCALE_F32) = (float)loss_scale;
}

static bool chunk_on_grid(int chunk) { return chunk >= FO_CHUNK_GRID && chunk <= FO_CHUNK_MAX && chunk % FO_CHUNK_GRID == 0; }

}  // namespace dsp

using namespace dsp;

extern "C" size_t dsp_fp16_optim_workspace_bytes(int64_t n_items)
{
    if (n_items <= 0) return 0;
    return a16((size_t)n_items * sizeof(float));
}

extern "C" int dsp_fp16_optim_grad_sumsq(const void* const* grads, int dtype, int N, const int64_t* items, int64_t n_items, int chunk,
                                         void* workspace, size_t workspace_bytes, double* S, dsp_stream_t stream)
{
    if (dtype != DSP_F16 && dtype != DSP_BF16) { set_error("fp16_optim_grad_sumsq: unsupported dtype %d (DSP_F16 / DSP_BF16)", dtype); return DSP_EINVAL; }
    if (N < 0 || n_items < 0 || n_items > 0x7fffffffLL) { set_error("fp16_optim_grad_sumsq: bad sizes"); return DSP_EINVAL; }
    if (!chunk_on_grid(chunk)) { set_error("fp16_optim_grad_sumsq: chunk = %d (a multiple of %d up to %d)", chunk, FO_CHUNK_GRID, FO_CHUNK_MAX); return DSP_EINVAL; }
    if (N == 0 || n_items == 0) return DSP_OK;
    if (!grads || !items || !workspace || !S) { set_error("fp16_optim_grad_sumsq: null pointer"); return DSP_EINVAL; }
    if (((uintptr_t)workspace & 3) != 0 || ((uintptr_t)S & 7) != 0) { set_error("fp16_optim_grad_sumsq: workspace / S misaligned"); return DSP_EINVAL; }
    if (workspace_bytes < dsp_fp16_optim_workspace_bytes(n_items)) {
        set_error("fp16_optim_grad_sumsq: workspace %zu < %zu bytes", workspace_bytes, dsp_fp16_optim_workspace_bytes(n_items));
        return DSP_ENOSPC;
    }
    float* partial = (float*)workspace;
    DSP_DISPATCH_ELEM_16(dtype, T,
        hipLaunchKernelGGL((fo_sumsq_kernel<T>), dim3((unsigned)n_items), dim3(FO_THREADS), 0, as_stream(stream), grads, items, partial));
    const int rc = check_launch("fp16_optim_grad_sumsq");
    if (rc) return rc;
    hipLaunchKernelGGL(fo_sumsq_tail_kernel, dim3(1), dim3(FO_THREADS), 0, as_stream(stream), (const float*)partial, n_items, S);
    return check_launch("fp16_optim_grad_sumsq (tail)");
}

extern "C" int dsp_fp16_optim_adam_step(const void* const* grads, void* const* params16, int dtype, const int64_t* offsets, int N,
                                        const int64_t* items, int64_t n_items, int chunk, float* master, float* exp_avg, float* exp_avg_sq,
                                        double c, double lr, double beta1, double beta2, double eps, double lr_wd, double bias1, double sqrt_bias2,
                                        int t, dsp_stream_t stream)
{
    if (dtype != DSP_F16 && dtype != DSP_BF16) { set_error("fp16_optim_adam_step: unsupported dtype %d (DSP_F16 / DSP_BF16)", dtype); return DSP_EINVAL; }
    if (N < 0 || n_items < 0 || n_items > 0x7fffffffLL) { set_error("fp16_optim_adam_step: bad sizes"); return DSP_EINVAL; }
    if (!chunk_on_grid(chunk)) { set_error("fp16_optim_adam_step: chunk = %d (a multiple of %d up to %d)", chunk, FO_CHUNK_GRID, FO_CHUNK_MAX); return DSP_EINVAL; }
    if (t < 1) { set_error("fp16_optim_adam_step: step count t = %d (>= 1)", t); return DSP_EINVAL; }
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) { set_error("fp16_optim_adam_step: betas (%g, %g) outside [0, 1)", beta1, beta2); return DSP_EINVAL; }
    if (!(bias1 > 0.0) || !(sqrt_bias2 > 0.0)) { set_error("fp16_optim_adam_step: bias corrections (%g, %g) must be positive", bias1, sqrt_bias2); return DSP_EINVAL; }
    if (N == 0 || n_items == 0) return DSP_OK;
    if (!grads || !params16 || !offsets || !items || !master || !exp_avg || !exp_avg_sq) { set_error("fp16_optim_adam_step: null pointer"); return DSP_EINVAL; }
    if ((((uintptr_t)master | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) != 0) {
        set_error("fp16_optim_adam_step: master / exp_avg / exp_avg_sq must start on a 16-byte boundary");
        return DSP_EINVAL;
    }
    ScalarsByValue src;
    src.k = derive_scalars(c, lr, beta1, beta2, eps, lr_wd, bias1, sqrt_bias2);
    DSP_DISPATCH_ELEM_16(dtype, T,
        hipLaunchKernelGGL((fo_adam_kernel<T, ScalarsByValue>), dim3((unsigned)n_items), dim3(FO_THREADS), 0, as_stream(stream), grads, params16,
                           offsets, items, master, exp_avg, exp_avg_sq, src));
    return check_launch("fp16_optim_adam_step");
}

extern "C" int dsp_fp16_optim_scale_step(const double* S, void* state, double beta1, double beta2, double eps, double weight_decay,
                                         double clip_norm, double scale_factor, int64_t scale_window, double min_loss_scale, dsp_stream_t stream)
{
    if (!S || !state) { set_error("fp16_optim_scale_step: null pointer"); return DSP_EINVAL; }
    if (((uintptr_t)S & 7) != 0 || ((uintptr_t)state & 7) != 0) { set_error("fp16_optim_scale_step: S / state must start on an 8-byte boundary"); return DSP_EINVAL; }
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) { set_error("fp16_optim_scale_step: betas (%g, %g) outside [0, 1)", beta1, beta2); return DSP_EINVAL; }
    if (!(scale_factor > 1.0) || scale_window < 1) {
        set_error("fp16_optim_scale_step: scale_factor = %g (> 1), scale_window = %lld (>= 1)", scale_factor, (long long)scale_window);
        return DSP_EINVAL;
    }
    ScaleConsts k;
    k.beta1 = beta1; k.beta2 = beta2; k.eps = eps; k.weight_decay = weight_decay; k.clip_norm = clip_norm; k.scale_factor = scale_factor;
    k.min_loss_scale = min_loss_scale; k.scale_window = scale_window;
    hipLaunchKernelGGL(fo_scale_step_kernel, dim3(1), dim3(64), 0, as_stream(stream), S, (uint64_t*)state, k);
    return check_launch("fp16_optim_scale_step");
}

extern "C" int dsp_fp16_optim_adam_step_state(const void* const* grads, void* const* params16, int dtype, const int64_t* offsets, int N,
                                              const int64_t* items, int64_t n_items, int chunk, float* master, float* exp_avg,
                                              float* exp_avg_sq, const void* state, dsp_stream_t stream)
{
    if (dtype != DSP_F16 && dtype != DSP_BF16) { set_error("fp16_optim_adam_step_state: unsupported dtype %d (DSP_F16 / DSP_BF16)", dtype); return DSP_EINVAL; }
    if (N < 0 || n_items < 0 || n_items > 0x7fffffffLL) { set_error("fp16_optim_adam_step_state: bad sizes"); return DSP_EINVAL; }
    if (!chunk_on_grid(chunk)) { set_error("fp16_optim_adam_step_state: chunk = %d (a multiple of %d up to %d)", chunk, FO_CHUNK_GRID, FO_CHUNK_MAX); return DSP_EINVAL; }
    if (N == 0 || n_items == 0) return DSP_OK;
    if (!grads || !params16 || !offsets || !items || !master || !exp_avg || !exp_avg_sq) { set_error("fp16_optim_adam_step_state: null pointer"); return DSP_EINVAL; }
    if (!state || ((uintptr_t)state & 7) != 0) { set_error("fp16_optim_adam_step_state: state null or off its 8-byte boundary"); return DSP_EINVAL; }
    if ((((uintptr_t)master | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) != 0) {
        set_error("fp16_optim_adam_step_state: master / exp_avg / exp_avg_sq must start on a 16-byte boundary");
        return DSP_EINVAL;
    }
    ScalarsFromState src;
    src.state = (const uint64_t*)state;
    DSP_DISPATCH_ELEM_16(dtype, T,
        hipLaunchKernelGGL((fo_adam_kernel<T, ScalarsFromState>), dim3((unsigned)n_items), dim3(FO_THREADS), 0, as_stream(stream), grads, params16,
                           offsets, items, master, exp_avg, exp_avg_sq, src));
    return check_launch("fp16_optim_adam_step_state");
}
