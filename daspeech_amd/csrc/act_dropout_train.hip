// act_dropout_train.hip — bias + activation + dropout (and GLU) between the GEMMs of a feed-forward block, under autograd, gfx950:
//     u = h + bias;   y = keep ? keep_scale * act(u) : 0            act: identity / relu / silu / gelu (erf form), Cout = Cin
//     y = keep ? keep_scale * u[:, :Cout] * sigmoid(u[:, Cout:]) : 0                      act: glu, Cout = Cin / 2
// rows R = prod(leading dims), fp32 / fp16 / bf16 storage, fp32 arithmetic, and its backward (include/daspeech_decode.h:
// dsp_act_dropout_train_fwd / _bwd).  One forward launch; one backward launch and, when the bias gradient is asked for, a merge tail.
//
// Layout of the work, the same in both kernels: a workgroup owns a chunk of DSP_ACTDROP_CHUNK_ROWS rows times a slab of 64 16-byte groups of
// OUTPUT columns; a lane owns one group (V = 4 or 8 elements; with glu the value group and the gate group Cout columns further on) and walks
// rows of the chunk in ascending order — all of them in the backward, whose workgroup is one wave, so that a column's sum forms in one lane's
// registers; a wave's share of them in the forward, which sums nothing.  Nothing is shared between lanes: no LDS, no shuffles, no barriers.
//
// The dropout mask is never stored: output element e = r * Cout + c keeps its value by the rule of philox.h; the backward recomputes u, the
// derivative of the activation and the mask from h, bias and (seed, offset, thr).
//
// dbias: a lane adds dh of its columns over the rows of its chunk, in row order, in fp32 registers before dh is rounded; the workgroup writes
// one fp32 partial per input column for its chunk, and ad_dbias_merge_kernel adds the chunks in ASCENDING order.  No float atomics, no hand-off
// between workgroups inside a launch: same inputs, same bits.
#include "common.h"
#include "host_gates.h"
#include "partial_merge.h"
#include "philox.h"
#include "../../include/daspeech_decode.h"

namespace dsp {

constexpr int AD_CHUNK = DSP_ACTDROP_CHUNK_ROWS;           // rows per workgroup = rows per workspace partial
constexpr int AD_SLAB = 64;                                // 16-byte column groups per workgroup: one per lane
constexpr int AD_MAX_CIN = DSP_ACTDROP_MAX_CIN;

__device__ __forceinline__ float ad_sigmoid(float u) { return 1.f / (1.f + expf(-u)); }

// act(u) of the four one-operand activations
template <int ACT> __device__ __forceinline__ float ad_act(float u)
{
    if constexpr (ACT == DSP_ACT_RELU) return u > 0.f ? u : 0.f;
    else if constexpr (ACT == DSP_ACT_SILU) return u * ad_sigmoid(u);
    else if constexpr (ACT == DSP_ACT_GELU) return 0.5f * u * (1.f + erff(u * 0.70710678118654752f));
    else return u;
}
// act'(u)
template <int ACT> __device__ __forceinline__ float ad_dact(float u)
{
    if constexpr (ACT == DSP_ACT_RELU) return u > 0.f ? 1.f : 0.f;
    else if constexpr (ACT == DSP_ACT_SILU) { const float s = ad_sigmoid(u); return s * (1.f + u * (1.f - s)); }
    else if constexpr (ACT == DSP_ACT_GELU)
        return 0.5f * (1.f + erff(u * 0.70710678118654752f)) + u * (0.39894228040143268f * expf(-0.5f * u * u));
    else return 1.f;
}

// ---------------------------------------------------------------- forward
// Nothing is summed here, so the 32 rows of a chunk are shared out among the AD_FWD_WAVES waves of the workgroup, AD_FWD_ROWS consecutive rows
// each: a lane still owns one column group, and all its loads are issued before the first activation (one wave per chunk and slab, as the
// backward has it, leaves less than one wave per SIMD at 6 400 x 2 048 and ran at a fifth of the memory rate).
constexpr int AD_FWD_WAVES = 8;
constexpr int AD_FWD_ROWS = AD_CHUNK / AD_FWD_WAVES;
static_assert(AD_FWD_ROWS * AD_FWD_WAVES == AD_CHUNK, "the waves of the forward share out a chunk");

template <typename T, int ACT>
__global__ __launch_bounds__(64 * AD_FWD_WAVES) void ad_fwd_kernel(const T* __restrict__ h, long ld_h, const void* __restrict__ bias, int pdtype,
                                                                   float keep_scale, uint32_t thr, uint64_t seed, uint64_t offset,
                                                                   const uint64_t* __restrict__ rng_state, T* __restrict__ y, long R, int Cout)
{
    constexpr int V = elems16<T>;
    philox_stream(seed, offset, rng_state);
    constexpr bool GLU = ACT == DSP_ACT_GLU;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = ((int)blockIdx.y * AD_SLAB + lane) * V;
    const long rb = (long)blockIdx.x * AD_CHUNK + wave * AD_FWD_ROWS;
    if (c >= Cout || rb >= R) return;                                      // nothing below needs the whole wave or workgroup
    float ba[V], bg[V];
#pragma unroll
    for (int i = 0; i < V; ++i) { ba[i] = 0.f; bg[i] = 0.f; }
    if (bias) {
        param_load_f<T>(bias, pdtype, c, ba);
        if constexpr (GLU) param_load_f<T>(bias, pdtype, c + Cout, bg);
    }
    float a[AD_FWD_ROWS][V], g[GLU ? AD_FWD_ROWS : 1][V];
#pragma unroll
    for (int k = 0; k < AD_FWD_ROWS; ++k)
        if (rb + k < R) {
            const T* row = h + (size_t)(rb + k) * (size_t)ld_h + c;
            load_f<T>(row, a[k]);
            if constexpr (GLU) load_f<T>(row + Cout, g[k]);
        }
#pragma unroll
    for (int k = 0; k < AD_FWD_ROWS; ++k)
        if (rb + k < R) {
            float o[V];
            if constexpr (GLU) {
#pragma unroll
                for (int i = 0; i < V; ++i) o[i] = (a[k][i] + ba[i]) * ad_sigmoid(g[k][i] + bg[i]);
            } else {
#pragma unroll
                for (int i = 0; i < V; ++i) o[i] = ad_act<ACT>(a[k][i] + ba[i]);
            }
            const size_t at = (size_t)(rb + k) * (size_t)Cout + c;
            if (thr) {
                bool keep[V];
                keep_flags<V>((uint64_t)at, seed, offset, thr, keep);
#pragma unroll
                for (int i = 0; i < V; ++i) o[i] = keep[i] ? o[i] * keep_scale : 0.f;
            }
            store_f(y + at, o);
        }
}

// ---------------------------------------------------------------- backward: dh, one partial of dbias per chunk
template <typename T, int ACT>
__global__ __launch_bounds__(64) void ad_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ h, long ld_h,
                                                    const void* __restrict__ bias, int pdtype, float keep_scale, uint32_t thr, uint64_t seed,
                                                    uint64_t offset, const uint64_t* __restrict__ rng_state, T* __restrict__ dh,
                                                    float* __restrict__ part, long R, int Cout)
{
    constexpr int V = elems16<T>;
    philox_stream(seed, offset, rng_state);
    constexpr bool GLU = ACT == DSP_ACT_GLU;
    const int Cin = GLU ? 2 * Cout : Cout;
    const int c = ((int)blockIdx.y * AD_SLAB + (int)threadIdx.x) * V;
    if (c >= Cout) return;
    float ba[V], bg[V], sa[V], sg[V];
#pragma unroll
    for (int i = 0; i < V; ++i) { ba[i] = 0.f; bg[i] = 0.f; sa[i] = 0.f; sg[i] = 0.f; }
    if (bias) {
        param_load_f<T>(bias, pdtype, c, ba);
        if constexpr (GLU) param_load_f<T>(bias, pdtype, c + Cout, bg);
    }
    const long r0 = (long)blockIdx.x * AD_CHUNK, r1 = r0 + AD_CHUNK < R ? r0 + AD_CHUNK : R;
#pragma unroll 4
    for (long r = r0; r < r1; ++r) {
        const T* row = h + (size_t)r * (size_t)ld_h + c;
        const size_t at = (size_t)r * (size_t)Cout + c;
        float a[V], d[V];
        load_f<T>(row, a);
        load_f<T>(dy + at, d);
        if (thr) {
            bool keep[V];
            keep_flags<V>((uint64_t)at, seed, offset, thr, keep);
#pragma unroll
            for (int i = 0; i < V; ++i) d[i] = keep[i] ? d[i] * keep_scale : 0.f;
        }
        T* out = dh ? dh + (size_t)r * (size_t)Cin + c : nullptr;
        if constexpr (GLU) {
            float g[V], dg[V];
            load_f<T>(row + Cout, g);
#pragma unroll
            for (int i = 0; i < V; ++i) {
                const float s = ad_sigmoid(g[i] + bg[i]);
                dg[i] = d[i] * (a[i] + ba[i]) * (s * (1.f - s));
                d[i] = d[i] * s;
                sg[i] += dg[i];
            }
            if (out) store_f(out + Cout, dg);
        } else {
#pragma unroll
            for (int i = 0; i < V; ++i) d[i] = d[i] * ad_dact<ACT>(a[i] + ba[i]);
        }
#pragma unroll
        for (int i = 0; i < V; ++i) sa[i] += d[i];
        if (out) store_f(out, d);
    }
    if (!part) return;                                                     // kernel-uniform: no bias gradient was asked for
    float* p = part + (size_t)blockIdx.x * (size_t)Cin + c;
    store_f(p, sa);
    if constexpr (GLU) store_f(p + Cout, sg);
}

// ---------------------------------------------------------------- backward tail: the chunks in ascending order
// The partials are a [nchunks][Cin] matrix; a workgroup owns 64 of its columns (partial_merge.h: the tiled form).
__global__ __launch_bounds__(256) void ad_dbias_merge_kernel(const float* __restrict__ part, long nchunks, void* __restrict__ dbias, int pdtype,
                                                             int Cin)
{
    const int c = blockIdx.x * 64 + (threadIdx.x & 63);
    const float acc = merge_column_tiled<128>(part, nchunks, Cin, c);
    if ((threadIdx.x >> 6) == 0 && c < Cin) param_store(dbias, pdtype, c, acc);
}

static long ad_chunks(long R) { return (R + AD_CHUNK - 1) / AD_CHUNK; }

// what both entry points check; 1: nothing to do (R == 0), 0: go on, < 0: refused
static int ad_check(const char* who, int act, int act_dtype, int param_dtype, long R, int Cin, long ld_h, unsigned int thr,
                    const uint64_t* rng_state)
{
    DSP_GATE(rng_state_gate(who, rng_state));
    const int es = elem_size(act_dtype);
    if (!es || !elem_size(param_dtype) || (param_dtype != act_dtype && param_dtype != DSP_F32)) {
        set_error("%s: dtype codes %d (h, y and their gradients) / %d (bias, dbias: the same, or fp32)", who, act_dtype, param_dtype);
        return DSP_EINVAL;
    }
    if (act < DSP_ACT_IDENTITY || act > DSP_ACT_GLU) { set_error("%s: unknown activation code %d", who, act); return DSP_EINVAL; }
    const int V = 16 / es;
    if (R < 0 || R > (1L << 24) || Cin < V || (Cin % V) || Cin > AD_MAX_CIN || ld_h < Cin || (ld_h % V)) {
        set_error("%s: bad sizes R=%ld Cin=%d ld_h=%ld (R <= 2^24, Cin and ld_h multiples of %d, Cin <= %d, ld_h >= Cin)", who, R, Cin, ld_h, V,
                  AD_MAX_CIN);
        return DSP_EINVAL;
    }
    if (act == DSP_ACT_GLU && (Cin / V) % 2) {
        set_error("%s: glu needs an even number of 16-byte groups per row, got Cin=%d (%d groups)", who, Cin, Cin / V); return DSP_EINVAL;
    }
    if (thr > (1u << 24)) { set_error("%s: thr %u above 2^24", who, thr); return DSP_EINVAL; }
    return R == 0 ? 1 : 0;
}

}  // namespace dsp

using namespace dsp;

#define AD_DISPATCH(dtype, act, ...)                                                                     \
    DSP_DISPATCH_ELEM(dtype, E, switch (act) {                                                           \
        case DSP_ACT_IDENTITY: { constexpr int ACT = DSP_ACT_IDENTITY; __VA_ARGS__; } break;             \
        case DSP_ACT_RELU: { constexpr int ACT = DSP_ACT_RELU; __VA_ARGS__; } break;                     \
        case DSP_ACT_SILU: { constexpr int ACT = DSP_ACT_SILU; __VA_ARGS__; } break;                     \
        case DSP_ACT_GELU: { constexpr int ACT = DSP_ACT_GELU; __VA_ARGS__; } break;                     \
        default: { constexpr int ACT = DSP_ACT_GLU; __VA_ARGS__; } break;                                \
    })

extern "C" size_t dsp_act_dropout_train_workspace_bytes(int64_t R, int Cin)
{
    if (R <= 0 || Cin < 1) return 0;
    return a16((size_t)ad_chunks((long)R) * (size_t)Cin * sizeof(float));
}

static int ad_fwd(const char* who, const void* h, long ld_h, const void* bias, int act, float keep_scale, unsigned int thr, uint64_t seed,
                  uint64_t offset, const uint64_t* rng_state, void* y, int act_dtype, int param_dtype, int64_t R, int Cin, dsp_stream_t stream)
{
    const int rc = ad_check(who, act, act_dtype, param_dtype, (long)R, Cin, ld_h, thr, rng_state);
    if (rc) return rc < 0 ? rc : DSP_OK;
    if (!h || !y || y == h || (bias && (bias == h || bias == y))) { set_error("%s: null or aliased pointer", who); return DSP_EINVAL; }
    DSP_GATE(tensors16_gate(who, h, bias, y));
    const int V = 16 / elem_size(act_dtype), Cout = act == DSP_ACT_GLU ? Cin / 2 : Cin;
    const dim3 grid((unsigned)ad_chunks((long)R), (unsigned)((Cout / V + AD_SLAB - 1) / AD_SLAB));
    hipStream_t st = as_stream(stream);
    AD_DISPATCH(act_dtype, act, hipLaunchKernelGGL((ad_fwd_kernel<E, ACT>), grid, dim3(64 * AD_FWD_WAVES), 0, st, (const E*)h, ld_h, bias, param_dtype, keep_scale,
                                                   (uint32_t)thr, seed, offset, rng_state, (E*)y, (long)R, Cout));
    return check_launch(who);
}

extern "C" int dsp_act_dropout_train_fwd(const void* h, long ld_h, const void* bias, int act, float keep_scale, unsigned int thr, uint64_t seed,
                                         uint64_t offset, void* y, int act_dtype, int param_dtype, int64_t R, int Cin, dsp_stream_t stream)
{
    return ad_fwd("act_dropout_train_fwd", h, ld_h, bias, act, keep_scale, thr, seed, offset, nullptr, y, act_dtype, param_dtype, R, Cin, stream);
}

extern "C" int dsp_act_dropout_train_fwd_state(const void* h, long ld_h, const void* bias, int act, float keep_scale, unsigned int thr,
                                               uint64_t seed, uint64_t offset, void* y, int act_dtype, int param_dtype, int64_t R, int Cin,
                                               const uint64_t* rng_state, dsp_stream_t stream)
{
    return ad_fwd("act_dropout_train_fwd_state", h, ld_h, bias, act, keep_scale, thr, seed, offset, rng_state, y, act_dtype, param_dtype, R, Cin,
                  stream);
}

static int ad_bwd(const char* who, const void* dy, const void* h, long ld_h, const void* bias, int act, float keep_scale, unsigned int thr,
                  uint64_t seed, uint64_t offset, const uint64_t* rng_state, void* dh, void* dbias, void* workspace, size_t workspace_bytes,
                  int act_dtype, int param_dtype, int64_t R, int Cin, dsp_stream_t stream)
{
    const int rc = ad_check(who, act, act_dtype, param_dtype, (long)R, Cin, ld_h, thr, rng_state);
    if (rc) return rc < 0 ? rc : DSP_OK;
    if (!dh && !dbias) return DSP_OK;
    if (!dy || !h || (dh && (dh == dy || dh == h || dh == bias || dh == dbias)) || (dbias && (dbias == dy || dbias == h || dbias == bias))) {
        set_error("%s: null or aliased pointer", who); return DSP_EINVAL;
    }
    DSP_GATE(tensors16_gate(who, dy, h, bias, dh, dbias));
    if (dbias)
        DSP_GATE(workspace_gate(who, workspace, workspace_bytes, dsp_act_dropout_train_workspace_bytes(R, Cin), "dsp_act_dropout_train_workspace_bytes"));
    const int V = 16 / elem_size(act_dtype), Cout = act == DSP_ACT_GLU ? Cin / 2 : Cin;
    const long nchunks = ad_chunks((long)R);
    const dim3 grid((unsigned)nchunks, (unsigned)((Cout / V + AD_SLAB - 1) / AD_SLAB));
    float* part = dbias ? (float*)workspace : (float*)nullptr;
    hipStream_t st = as_stream(stream);
    AD_DISPATCH(act_dtype, act, hipLaunchKernelGGL((ad_bwd_kernel<E, ACT>), grid, dim3(64), 0, st, (const E*)dy, (const E*)h, ld_h, bias, param_dtype,
                                                   keep_scale, (uint32_t)thr, seed, offset, rng_state, (E*)dh, part, (long)R, Cout));
    if (dbias)
        hipLaunchKernelGGL(ad_dbias_merge_kernel, dim3((unsigned)((Cin + 63) / 64)), dim3(256), 0, st, part, nchunks, dbias, param_dtype, Cin);
    return check_launch(who);
}

extern "C" int dsp_act_dropout_train_bwd(const void* dy, const void* h, long ld_h, const void* bias, int act, float keep_scale, unsigned int thr,
                                         uint64_t seed, uint64_t offset, void* dh, void* dbias, void* workspace, size_t workspace_bytes,
                                         int act_dtype, int param_dtype, int64_t R, int Cin, dsp_stream_t stream)
{
    return ad_bwd("act_dropout_train_bwd", dy, h, ld_h, bias, act, keep_scale, thr, seed, offset, nullptr, dh, dbias, workspace, workspace_bytes,
                  act_dtype, param_dtype, R, Cin, stream);
}

extern "C" int dsp_act_dropout_train_bwd_state(const void* dy, const void* h, long ld_h, const void* bias, int act, float keep_scale,
                                               unsigned int thr, uint64_t seed, uint64_t offset, void* dh, void* dbias, void* workspace,
                                               size_t workspace_bytes, int act_dtype, int param_dtype, int64_t R, int Cin,
                                               const uint64_t* rng_state, dsp_stream_t stream)
{
    return ad_bwd("act_dropout_train_bwd_state", dy, h, ld_h, bias, act, keep_scale, thr, seed, offset, rng_state, dh, dbias, workspace,
                  workspace_bytes, act_dtype, param_dtype, R, Cin, stream);
}
