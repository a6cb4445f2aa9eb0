// conv1d_train.h — what the two channels-last Conv1d training operators share (conv1d_train.hip: stride 1; conv1d_stride2_train.hip: stride 2):
// the operand types and the fragment read of the "NT" v_mfma_f32_32x32x16 products, the weight re-lay, the weight gradient over row splits with
// its ascending merge, the chunked column sums of the bias gradient, and the host half behind the C entries, written once for a STRIDE of
// 1 or 2: the size check, the workspace question and its carving, the gate sequences of the two entries.  The .hip files keep their
// extern "C" entries and the convolution launches, which differ.  Everything here is a template, an inline function or has internal
// linkage: each of the two translation units gets its own copy.
#pragma once
#include "common.h"
#include "host_gates.h"
#include "partial_merge.h"
#include "../../include/daspeech_decode.h"

namespace dsp {

typedef _Float16 cv_h8 __attribute__((ext_vector_type(8)));
typedef __bf16 cv_b8 __attribute__((ext_vector_type(8)));
typedef float cv_acc __attribute__((ext_vector_type(16)));
typedef unsigned short cv_u16;

constexpr int CV_ROWS = DSP_CONV1D_TRAIN_ROW_TILE;        // rows of a sample per workgroup of the convolution kernels
constexpr int CV_COLS = 128;                              // output columns per workgroup
constexpr int CV_KC = 64;                                 // reduction channels per staged image
constexpr int CV_PITCH = 72;                              // pitch (elements) of an LDS image with 64 k values: 144 bytes, 16-byte aligned rows
constexpr int CV_MAX_K = DSP_CONV1D_TRAIN_MAX_K;
constexpr int CV_WG_ROWS = DSP_CONV1D_TRAIN_WGRAD_ROWS;   // rows per split of the weight gradient (one workspace partial each)
constexpr int CV_WG_TILE = 128;                           // co and ci per workgroup of cv_wgrad_kernel
constexpr int CV_DB_CHUNK = 256;                          // rows per partial of the bias gradient
constexpr int CV_MAX_C = DSP_CONV1D_TRAIN_MAX_C;
static_assert(CV_ROWS == 64 && CV_WG_ROWS % 64 == 0, "the wave layouts are written for 64-row tiles");
#define CV_ROW(reg, hi) (((reg) & 3) + 8 * ((reg) >> 2) + 4 * (hi))

template <typename E> struct Cv;
template <> struct Cv<__half> {
    using V = cv_h8;
    static __device__ __forceinline__ cv_acc mma(V a, V b, cv_acc c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
};
template <> struct Cv<__hip_bfloat16> {
    using V = cv_b8;
    static __device__ __forceinline__ cv_acc mma(V a, V b, cv_acc c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
};

// the 16-byte operand of lane `lane` for k step s of an image row block starting at img (k contiguous, CV_PITCH)
template <typename E> __device__ __forceinline__ typename Cv<E>::V cv_frag(const cv_u16* img, int s, int lane)
{
    return *reinterpret_cast<const typename Cv<E>::V*>(img + (lane & 31) * CV_PITCH + 16 * s + 8 * (lane >> 5));
}

// ---------------------------------------------------------------- weight re-lay: [Cout][Cin][K] -> [K][Cout][Cin], or [K][Cin][Cout] with the taps reversed
static __global__ __launch_bounds__(256) void cv_pack_kernel(const cv_u16* __restrict__ w, cv_u16* __restrict__ wp, int Cin, int Cout, int K,
                                                             int transposed)
{
    const long n = (long)K * Cin * Cout, e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const int k = (int)(e / ((long)Cin * Cout));
    const int rem = (int)(e - (long)k * Cin * Cout);
    int co, ci, tap;
    if (!transposed) { co = rem / Cin; ci = rem - co * Cin; tap = k; }
    else { ci = rem / Cout; co = rem - ci * Cout; tap = K - 1 - k; }
    wp[e] = w[((long)co * Cin + ci) * K + tap];
}

// ---------------------------------------------------------------- weight gradient: one fp32 partial per split of the rows
// two rows (r, r + 1) of 8 channels -> eight 32-bit words of the transposed image [channel][row]
__device__ __forceinline__ void cv_put_t(cv_u16* dst, uint4 u0, uint4 u1, int g, int p)
{
    const uint32_t w0[4] = {u0.x, u0.y, u0.z, u0.w}, w1[4] = {u1.x, u1.y, u1.z, u1.w};
#pragma unroll
    for (int x = 0; x < 4; ++x) {
        *reinterpret_cast<uint32_t*>(dst + (8 * g + 2 * x) * CV_PITCH + 2 * p) = (w0[x] & 0xffffu) | (w1[x] << 16);
        *reinterpret_cast<uint32_t*>(dst + (8 * g + 2 * x + 1) * CV_PITCH + 2 * p) = (w0[x] >> 16) | (w1[x] & 0xffff0000u);
    }
}

// dy [B*T rows] against the x row that tap k of output row (b, t) reads: STRIDE * t + k - P of sample b's Tx rows (STRIDE 1: Tx = T)
template <typename E, int STRIDE>
__global__ __launch_bounds__(256) void cv_wgrad_kernel(const E* __restrict__ dy, long ld_dy, const E* __restrict__ x, long ld_x,
                                                       float* __restrict__ part, int T, int Tx, int BT, int Cin, int Cout, int K, int ci_tiles)
{
    __shared__ __attribute__((aligned(16))) cv_u16 Ds[CV_WG_TILE * CV_PITCH], Xs[CV_WG_TILE * CV_PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave & 1, wc = wave >> 1;
    const int ci0 = ((int)blockIdx.x % ci_tiles) * CV_WG_TILE, co0 = ((int)blockIdx.x / ci_tiles) * CV_WG_TILE;
    const int k = blockIdx.y, split = blockIdx.z, sh = k - (K - 1) / 2;
    const int r_begin = split * CV_WG_ROWS, r_end = r_begin + CV_WG_ROWS < BT ? r_begin + CV_WG_ROWS : BT;
    // a thread stages row pair p of channel groups g0 and g0 + 8 (8 channels each) of both images
    const int p = tid & 31, g0 = tid >> 5;
    uint4 dreg[2][2], xreg[2][2];
#define CV_LOAD_ROWS(r0)                                                                                                           \
    _Pragma("unroll") for (int q = 0; q < 2; ++q) {                                                                                \
        const int r = (r0) + 2 * p + q;                                                                                            \
        const bool in = r < r_end;                                                                                                 \
        const int bb = in ? r / T : 0, ts = STRIDE * (r - bb * T) + sh;                                                            \
        const bool xin = in && ts >= 0 && ts < Tx;                                                                                 \
        const size_t xr = STRIDE == 1 ? (size_t)(r + sh) : (size_t)bb * (size_t)Tx + (size_t)ts;                                   \
        _Pragma("unroll") for (int j = 0; j < 2; ++j) {                                                                            \
            const int g = g0 + 8 * j;                                                                                              \
            dreg[j][q] = (in && co0 + 8 * g < Cout) ? *reinterpret_cast<const uint4*>(dy + (size_t)r * (size_t)ld_dy + co0 + 8 * g) \
                                                    : make_uint4(0u, 0u, 0u, 0u);                                                  \
            xreg[j][q] = (xin && ci0 + 8 * g < Cin) ? *reinterpret_cast<const uint4*>(x + xr * (size_t)ld_x + ci0 + 8 * g)          \
                                                    : make_uint4(0u, 0u, 0u, 0u);                                                  \
        }                                                                                                                          \
    }
    cv_acc acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) acc[i][j][reg] = 0.f;
    CV_LOAD_ROWS(r_begin)
#pragma unroll 1
    for (int r0 = r_begin; r0 < r_end; r0 += 64) {
        __syncthreads();                                                    // the products of the rows before these have read both images
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            cv_put_t(Ds, dreg[j][0], dreg[j][1], g0 + 8 * j, p);
            cv_put_t(Xs, xreg[j][0], xreg[j][1], g0 + 8 * j, p);
        }
        __syncthreads();
        if (r0 + 64 < r_end) { CV_LOAD_ROWS(r0 + 64) }                      // in flight while these rows are multiplied
        const cv_u16* A = Ds + 64 * wr * CV_PITCH;
        const cv_u16* Bt = Xs + 64 * wc * CV_PITCH;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const typename Cv<E>::V va0 = cv_frag<E>(A, s, lane), va1 = cv_frag<E>(A + 32 * CV_PITCH, s, lane);
            const typename Cv<E>::V vb0 = cv_frag<E>(Bt, s, lane), vb1 = cv_frag<E>(Bt + 32 * CV_PITCH, s, lane);
            acc[0][0] = Cv<E>::mma(va0, vb0, acc[0][0]);
            acc[0][1] = Cv<E>::mma(va0, vb1, acc[0][1]);
            acc[1][0] = Cv<E>::mma(va1, vb0, acc[1][0]);
            acc[1][1] = Cv<E>::mma(va1, vb1, acc[1][1]);
        }
    }
#undef CV_LOAD_ROWS
    const int col = lane & 31, hi = lane >> 5;
    float* pk = part + ((size_t)split * K + k) * (size_t)Cout * (size_t)Cin;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int ci = ci0 + 64 * wc + 32 * j + col;
            if (ci >= Cin) continue;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int co = co0 + 64 * wr + 32 * i + CV_ROW(reg, hi);
                if (co < Cout) pk[(size_t)co * Cin + ci] = acc[i][j][reg];
            }
        }
}

// the splits in ascending order; [K][Cout][Cin] fp32 -> [Cout][Cin][K] in the data dtype, rounded once
template <typename E>
__global__ __launch_bounds__(256) void cv_wgrad_merge_kernel(const float* __restrict__ part, int nsplit, int Cin, int Cout, int K, E* __restrict__ dw)
{
    const long n = (long)K * Cin * Cout, e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const float acc = merge_plain(part, nsplit, (size_t)n, (size_t)e);
    const int k = (int)(e / ((long)Cin * Cout));
    const int rem = (int)(e - (long)k * Cin * Cout);
    const int co = rem / Cin, ci = rem - co * Cin;
    dw[((size_t)co * Cin + ci) * K + k] = from_f<E>(acc);
}

// ---------------------------------------------------------------- bias gradient: column sums in a fixed order
// a workgroup owns 64 columns x CV_DB_CHUNK rows; thread (tx, ty) adds rows ty, ty + 4, ... in ascending order, then the four in ascending ty
template <typename E>
__global__ __launch_bounds__(256) void cv_db_part_kernel(const E* __restrict__ dy, long ld_dy, int BT, int Cout, float* __restrict__ part)
{
    __shared__ float red[4][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6, c = (int)blockIdx.y * 64 + tx;
    const int r0 = (int)blockIdx.x * CV_DB_CHUNK, r1 = r0 + CV_DB_CHUNK < BT ? r0 + CV_DB_CHUNK : BT;
    float a = 0.f;
    for (int r = r0 + ty; r < r1; r += 4) a += to_f(dy[(size_t)r * (size_t)ld_dy + c]);
    red[ty][tx] = a;
    __syncthreads();
    if (ty == 0) part[(size_t)blockIdx.x * Cout + c] = ((red[0][tx] + red[1][tx]) + red[2][tx]) + red[3][tx];
}
static __global__ __launch_bounds__(256) void cv_db_merge_kernel(const float* __restrict__ part, int nchunks, int Cout, void* __restrict__ db,
                                                                 int bdtype)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= Cout) return;
    param_store(db, bdtype, c, merge_plain(part, nchunks, (size_t)Cout, (size_t)c));
}

static inline size_t cv_pack_bytes(int Cin, int Cout, int K) { return a16((size_t)K * Cin * Cout * 2); }
static inline int cv_splits(long BT) { return (int)((BT + CV_WG_ROWS - 1) / CV_WG_ROWS); }
static inline int cv_db_chunks(long BT) { return (int)((BT + CV_DB_CHUNK - 1) / CV_DB_CHUNK); }

// ---------------------------------------------------------------- the host half behind the C entries, STRIDE 1 or 2
template <int STRIDE> static inline int cv_tout(int T) { return STRIDE == 1 ? T : (T - 1) / 2 + 1; }      // rows of y and dy per sample

// what the entry points check; 1: nothing to do (no rows), 0: go on, < 0: refused.  Stride 2 takes Cin in steps of 16 (the filterbank's 80).
template <int STRIDE>
static int cv_check(const char* who, int act_dtype, int bias_dtype, int B, int T, int Cin, int Cout, int K, long ld_a, int Ca, long ld_b, int Cb)
{
    constexpr int CIN_STEP = STRIDE == 1 ? 64 : 16;
    if ((act_dtype != DSP_F16 && act_dtype != DSP_BF16) || (bias_dtype != act_dtype && bias_dtype != DSP_F32)) {
        set_error("%s: dtype codes %d (x, W, y and their gradients: fp16 or bf16) / %d (bias, db: the same, or fp32)", who, act_dtype, bias_dtype);
        return DSP_EINVAL;
    }
    if (Cin < CIN_STEP || Cout < 64 || (Cin % CIN_STEP) || (Cout % 64) || Cin > CV_MAX_C || Cout > CV_MAX_C || K < 1 || K > CV_MAX_K || !(K & 1)) {
        if (STRIDE == 1)
            set_error("%s: Cin=%d Cout=%d K=%d not served (channels multiples of 64 up to %d, K odd and 1 <= K <= %d)", who, Cin, Cout, K, CV_MAX_C,
                      CV_MAX_K);
        else
            set_error("%s: Cin=%d Cout=%d K=%d not served (Cin a multiple of 16 from 16, Cout a multiple of 64, both up to %d, K odd and 1 <= K <= %d)",
                      who, Cin, Cout, K, CV_MAX_C, CV_MAX_K);
        return DSP_EINVAL;
    }
    if (B < 0 || T < 1 || (long)B * T > (1L << 24) || ld_a < Ca || (ld_a % 8) || ld_b < Cb || (ld_b % 8)) {
        if (STRIDE == 1)
            set_error("%s: bad sizes B=%d T=%d row strides %ld / %ld (T >= 1, B T <= 2^24, a row stride at least the channel count and a multiple of 8)",
                      who, B, T, ld_a, ld_b);
        else
            set_error("%s: bad sizes B=%d T=%d row strides %ld / %ld (T >= 1 input rows, B T <= 2^24, a row stride at least the channel count and a "
                      "multiple of 8)", who, B, T, ld_a, ld_b);
        return DSP_EINVAL;
    }
    return B == 0 ? 1 : 0;
}

// the workspace: the re-laid weight (phase 0: the forward stops here) | [splits][K][Cout][Cin] dW partials | [chunks][Cout] db partials
static inline size_t cv_wpart_bytes(long rows, int Cin, int Cout, int K) { return a16((size_t)cv_splits(rows) * (size_t)K * Cin * Cout * sizeof(float)); }
template <int STRIDE> static size_t cv_workspace_bytes(int phase, int B, int T, int Cin, int Cout, int K)
{
    if (B <= 0 || T <= 0 || Cin <= 0 || Cout <= 0 || K <= 0) return 0;
    const size_t pack = cv_pack_bytes(Cin, Cout, K);
    if (phase == 0) return pack;
    const long rows = (long)B * cv_tout<STRIDE>(T);
    return pack + cv_wpart_bytes(rows, Cin, Cout, K) + a16((size_t)cv_db_chunks(rows) * (size_t)Cout * sizeof(float));
}
struct CvWorkspace { void* wp; float* part_w; float* part_b; };
template <int STRIDE> static CvWorkspace cv_carve(void* workspace, int B, int T, int Cin, int Cout, int K)
{
    float* part_w = (float*)((char*)workspace + cv_pack_bytes(Cin, Cout, K));
    return {workspace, part_w, (float*)((char*)part_w + cv_wpart_bytes((long)B * cv_tout<STRIDE>(T), Cin, Cout, K))};
}

// the gates of the two entries, in the order in which they report; asked: the entry's workspace question as its message names it
template <int STRIDE>
static int cv_fwd_gates(const char* who, const char* asked, const void* x, long ld_x, const void* w, const void* bias, const void* y, long ld_y,
                        const void* workspace, size_t workspace_bytes, int act_dtype, int bias_dtype, int B, int T, int Cin, int Cout, int K)
{
    const int rc = cv_check<STRIDE>(who, act_dtype, bias_dtype, B, T, Cin, Cout, K, ld_x, Cin, ld_y, Cout);
    if (rc) return rc;
    if (!x || !w || !y || y == x || y == w || y == bias || workspace == x || workspace == w || workspace == y || (bias && workspace == bias)) {
        set_error("%s: null or aliased pointer", who); return DSP_EINVAL;
    }
    DSP_GATE(tensors16_gate(who, x, w, bias, y));
    return workspace_gate(who, workspace, workspace_bytes, cv_workspace_bytes<STRIDE>(0, B, T, Cin, Cout, K), asked);
}
template <int STRIDE>
static int cv_bwd_gates(const char* who, const char* asked, const void* dy, long ld_dy, const void* x, long ld_x, const void* w, void* dx, void* dw,
                        void* db, const void* workspace, size_t workspace_bytes, int act_dtype, int bias_dtype, int B, int T, int Cin, int Cout, int K)
{
    const int rc = cv_check<STRIDE>(who, act_dtype, bias_dtype, B, T, Cin, Cout, K, ld_x, Cin, ld_dy, Cout);
    if (rc) return rc;
    if (!dx && !dw && !db) return 1;
    if (!dy || !x || !w) { set_error("%s: null pointer", who); return DSP_EINVAL; }
    const void* ins[] = {dy, x, w, workspace};
    void* outs[] = {dx, dw, db};
    DSP_GATE(alias_gate(who, outs, 3, ins, 4, "an output aliases an input or the workspace", "two outputs alias"));
    if (workspace == dy || workspace == x || workspace == w) { set_error("%s: the workspace aliases an input", who); return DSP_EINVAL; }
    DSP_GATE(tensors16_gate(who, dy, x, w, dx, dw, db));
    return workspace_gate(who, workspace, workspace_bytes, cv_workspace_bytes<STRIDE>(1, B, T, Cin, Cout, K), asked);
}

// dW and db of a backward over the B * cv_tout(T) rows of dy, from the carved workspace
template <typename E, int STRIDE>
static void cv_launch_param_grads(hipStream_t st, const void* dy, long ld_dy, const void* x, long ld_x, const CvWorkspace& ws, void* dw, void* db,
                                  int bdtype, int B, int T, int Cin, int Cout, int K)
{
    const int To = cv_tout<STRIDE>(T), rows = B * To;
    if (dw) {
        const int ci_tiles = (Cin + CV_WG_TILE - 1) / CV_WG_TILE, co_tiles = (Cout + CV_WG_TILE - 1) / CV_WG_TILE, nsplit = cv_splits(rows);
        const size_t nw = (size_t)K * Cin * Cout;
        hipLaunchKernelGGL((cv_wgrad_kernel<E, STRIDE>), dim3((unsigned)(ci_tiles * co_tiles), (unsigned)K, (unsigned)nsplit), dim3(256), 0, st,
                           (const E*)dy, ld_dy, (const E*)x, ld_x, ws.part_w, To, T, rows, Cin, Cout, K, ci_tiles);
        hipLaunchKernelGGL((cv_wgrad_merge_kernel<E>), dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, st, ws.part_w, nsplit, Cin, Cout, K, (E*)dw);
    }
    if (db) {
        const int nchunks = cv_db_chunks(rows);
        hipLaunchKernelGGL((cv_db_part_kernel<E>), dim3((unsigned)nchunks, (unsigned)(Cout / 64)), dim3(256), 0, st, (const E*)dy, ld_dy, rows, Cout,
                           ws.part_b);
        hipLaunchKernelGGL(cv_db_merge_kernel, dim3((unsigned)((Cout + 255) / 256)), dim3(256), 0, st, ws.part_b, nchunks, Cout, db, bdtype);
    }
}

}  // namespace dsp
