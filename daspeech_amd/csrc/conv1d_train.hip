// conv1d_train.hip — Conv1d(Cin, Cout, K, stride 1, dilation 1, groups 1, padding P = (K-1)/2) on CHANNELS-LAST data under autograd, gfx950,
// fp16 / bf16 (include/daspeech_decode.h: dsp_conv1d_train_fwd / _bwd):
//     y [b,t,co]  = [bias[co] +] sum_k sum_ci x[b, t+k-P, ci] . W[co,ci,k]            rows outside [0, T) of a sample count as zeros
//     dx[b,t,ci]  = sum_k sum_co dy[b, t-k+P, co] . W[co,ci,k]
//     dW[co,ci,k] = sum_b sum_t  dy[b,t,co] . x[b, t+k-P, ci]
//     db[co]      = sum_b sum_t  dy[b,t,co]
// the FastSpeech2 feed-forward convolutions (256 -> 1024 -> 256, K 9) and the variance predictors' (256 -> 256, K 3) of the training step, without
// the transposes to channels-first and back.  Every product is v_mfma_f32_32x32x16_f16 / _bf16 in the "NT" form of
// relpos_attention_train.hip: C[32][32] += A[32][k] . B^T[32][k], both operands read from LDS images whose k index is contiguous (one 16-byte
// read per lane and k step), the result with its column (the B^T row) on the lane and its rows in the registers (CV_ROW).
//
// W [Cout][Cin][K] (nn.Conv1d's layout) is re-laid per call by cv_pack_kernel into the workspace: [K][Cout][Cin] for the forward, and
// [K][Cin][Cout] with the taps REVERSED for dx, which makes dx the forward kernel on dy (t - k + P = t + (K-1-k) - P).
//
//   cv_conv_kernel    a workgroup of 4 waves owns 64 rows of ONE sample x 128 output columns (a wave: 32 x 64).  Per 64 input channels the rows
//                     t0-P .. t0+63+P are staged once (rows outside the sample as zeros) and a tap is a row offset into that image; the
//                     128 x 64 weight tile of each (channel block, tap) goes through registers (loaded while the tile before it is multiplied)
//                     into LDS.  Columns past Cout (Cout = 64, 192) are staged as zeros and not stored.
//   cv_wgrad_kernel   a workgroup of 4 waves owns (128 co x 128 ci, one tap, one split of DSP_CONV1D_TRAIN_WGRAD_ROWS rows of the flattened
//                     B*T); it walks its rows 64 at a time in ascending order, dy and the tap-shifted x staged TRANSPOSED (row index
//                     contiguous, two rows per 32-bit LDS write), and writes one fp32 partial [split][K][Cout][Cin];
//   cv_wgrad_merge_kernel   adds the splits in ASCENDING order, rounds once and writes nn.Conv1d's layout.
//   cv_db_part_kernel / cv_db_merge_kernel   column sums of dy over chunks of 256 rows, then the chunks in ascending order.
// No float atomics, no hand-off between workgroups: the same inputs give the same bits on every call, and dx, dW, db are separate launches, so
// leaving one out does not change the others.  Every row is computed, padded frames included.
#include "common.h"
#include "../../include/daspeech_decode.h"

namespace dsp {

typedef _Float16 cv_h8 __attribute__((ext_vector_type(8)));
typedef __bf16 cv_b8 __attribute__((ext_vector_type(8)));
typedef float cv_acc __attribute__((ext_vector_type(16)));
typedef unsigned short cv_u16;

constexpr int CV_ROWS = DSP_CONV1D_TRAIN_ROW_TILE;        // rows of a sample per workgroup of cv_conv_kernel
constexpr int CV_COLS = 128;                              // output columns per workgroup
constexpr int CV_KC = 64;                                 // reduction channels per staged image
constexpr int CV_PITCH = 72;                              // pitch (elements) of an LDS image with 64 k values: 144 bytes, 16-byte aligned rows
constexpr int CV_MAX_K = DSP_CONV1D_TRAIN_MAX_K;
constexpr int CV_XROWS = CV_ROWS + CV_MAX_K - 1;          // the row tile and its halo
constexpr int CV_WG_ROWS = DSP_CONV1D_TRAIN_WGRAD_ROWS;   // rows per split of the weight gradient (one workspace partial each)
constexpr int CV_WG_TILE = 128;                           // co and ci per workgroup of cv_wgrad_kernel
constexpr int CV_DB_CHUNK = 256;                          // rows per partial of the bias gradient
constexpr int CV_MAX_C = DSP_CONV1D_TRAIN_MAX_C;
static_assert(CV_ROWS == 64 && CV_WG_ROWS % 64 == 0, "the wave layout below is written for 64-row tiles");
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
__global__ __launch_bounds__(256) void cv_pack_kernel(const cv_u16* __restrict__ w, cv_u16* __restrict__ wp, int Cin, int Cout, int K, int transposed)
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

// ---------------------------------------------------------------- forward, and dx on dy with the transposed, tap-reversed weight
// out[b,t,n] = [bias[n] +] sum_k sum_c in[b, t+k-P, c] . wp[k][n][c]
template <typename E>
__global__ __launch_bounds__(256) void cv_conv_kernel(const E* __restrict__ in, long ld_in, const E* __restrict__ wp, const void* __restrict__ bias,
                                                      int bdtype, E* __restrict__ out, long ld_out, int T, int Nin, int Nout, int K, int tiles)
{
    __shared__ __attribute__((aligned(16))) cv_u16 Xs[CV_XROWS * CV_PITCH], Ws[CV_COLS * CV_PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave & 1, wc = wave >> 1;
    const int b = (int)blockIdx.x / tiles, t0 = ((int)blockIdx.x % tiles) * CV_ROWS, n0 = (int)blockIdx.y * CV_COLS;
    const int P = (K - 1) / 2, nx = CV_ROWS + K - 1, nc = Nin / CV_KC;
    const E* inb = in + (size_t)b * (size_t)T * (size_t)ld_in;
    // the weight tile of (channel block c, tap k): 128 rows x 8 quads, 4 quads a thread
    const int wrow = tid >> 3, wq = (tid & 7) * 8;
    uint4 wreg[4];
#define CV_LOAD_W(c, k)                                                                                                            \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                                                                \
        const int n = n0 + wrow + 32 * j;                                                                                          \
        wreg[j] = n < Nout ? *reinterpret_cast<const uint4*>(wp + ((size_t)(k) * Nout + n) * (size_t)Nin + (c) * CV_KC + wq)       \
                           : make_uint4(0u, 0u, 0u, 0u);                                                                           \
    }
    cv_acc a0 = {0}, a1 = {0};
    CV_LOAD_W(0, 0)
#pragma unroll 1
    for (int c = 0; c < nc; ++c) {
        __syncthreads();                                                    // the products of the block before this one have read Xs and Ws
        for (int i = tid; i < nx * 8; i += 256) {
            const int rl = i >> 3, q = (i & 7) * 8, t = t0 - P + rl;
            uint4 u = make_uint4(0u, 0u, 0u, 0u);
            if (t >= 0 && t < T) u = *reinterpret_cast<const uint4*>(inb + (size_t)t * (size_t)ld_in + c * CV_KC + q);
            *reinterpret_cast<uint4*>(Xs + rl * CV_PITCH + q) = u;
        }
#pragma unroll 1
        for (int k = 0; k < K; ++k) {
            if (k) __syncthreads();                                         // the tap before this one has read Ws
#pragma unroll
            for (int j = 0; j < 4; ++j) *reinterpret_cast<uint4*>(Ws + (wrow + 32 * j) * CV_PITCH + wq) = wreg[j];
            __syncthreads();
            const int kn = k + 1 < K ? k + 1 : 0, cn = k + 1 < K ? c : c + 1;
            if (cn < nc) { CV_LOAD_W(cn, kn) }                              // in flight while this tile is multiplied
            const cv_u16* A = Xs + (32 * wr + k) * CV_PITCH;
            const cv_u16* Bt = Ws + 64 * wc * CV_PITCH;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const typename Cv<E>::V va = cv_frag<E>(A, s, lane);
                a0 = Cv<E>::mma(va, cv_frag<E>(Bt, s, lane), a0);
                a1 = Cv<E>::mma(va, cv_frag<E>(Bt + 32 * CV_PITCH, s, lane), a1);
            }
        }
    }
#undef CV_LOAD_W
    const int col = lane & 31, hi = lane >> 5;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int n = n0 + 64 * wc + 32 * h + col;
        if (n >= Nout) continue;
        const float bv = bias ? param_load(bias, bdtype, n) : 0.f;
        E* o = out + (size_t)b * (size_t)T * (size_t)ld_out + n;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int t = t0 + 32 * wr + CV_ROW(reg, hi);
            if (t < T) o[(size_t)t * (size_t)ld_out] = from_f<E>((h ? a1[reg] : a0[reg]) + bv);
        }
    }
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

template <typename E>
__global__ __launch_bounds__(256) void cv_wgrad_kernel(const E* __restrict__ dy, long ld_dy, const E* __restrict__ x, long ld_x,
                                                       float* __restrict__ part, int T, int BT, int Cin, int Cout, int K, int ci_tiles)
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
        const int bb = in ? r / T : 0, ts = r - bb * T + sh;                                                                       \
        const bool xin = in && ts >= 0 && ts < T;                                                                                  \
        _Pragma("unroll") for (int j = 0; j < 2; ++j) {                                                                            \
            const int g = g0 + 8 * j;                                                                                              \
            dreg[j][q] = (in && co0 + 8 * g < Cout) ? *reinterpret_cast<const uint4*>(dy + (size_t)r * (size_t)ld_dy + co0 + 8 * g) \
                                                    : make_uint4(0u, 0u, 0u, 0u);                                                  \
            xreg[j][q] = (xin && ci0 + 8 * g < Cin) ? *reinterpret_cast<const uint4*>(x + (size_t)(r + sh) * (size_t)ld_x + ci0 + 8 * g) \
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
    float acc = 0.f;
    for (int s = 0; s < nsplit; ++s) acc += part[(size_t)s * n + e];
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
__global__ __launch_bounds__(256) void cv_db_merge_kernel(const float* __restrict__ part, int nchunks, int Cout, void* __restrict__ db, int bdtype)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= Cout) return;
    float acc = 0.f;
    for (int k = 0; k < nchunks; ++k) acc += part[(size_t)k * Cout + c];
    param_store(db, bdtype, c, acc);
}

static size_t cv_align16(size_t n) { return (n + 15) & ~(size_t)15; }
static size_t cv_pack_bytes(int Cin, int Cout, int K) { return cv_align16((size_t)K * Cin * Cout * 2); }
static int cv_splits(long BT) { return (int)((BT + CV_WG_ROWS - 1) / CV_WG_ROWS); }
static int cv_db_chunks(long BT) { return (int)((BT + CV_DB_CHUNK - 1) / CV_DB_CHUNK); }

// what the entry points check; 1: nothing to do (no rows), 0: go on, < 0: refused
static int cv_check(const char* who, int act_dtype, int bias_dtype, int B, int T, int Cin, int Cout, int K, long ld_a, int Ca, long ld_b, int Cb)
{
    if ((act_dtype != DSP_F16 && act_dtype != DSP_BF16) || (bias_dtype != act_dtype && bias_dtype != DSP_F32)) {
        set_error("%s: dtype codes %d (x, W, y and their gradients: fp16 or bf16) / %d (bias, db: the same, or fp32)", who, act_dtype, bias_dtype);
        return DSP_EINVAL;
    }
    if (Cin < 64 || Cout < 64 || (Cin % 64) || (Cout % 64) || Cin > CV_MAX_C || Cout > CV_MAX_C || K < 1 || K > CV_MAX_K || !(K & 1)) {
        set_error("%s: Cin=%d Cout=%d K=%d not served (channels multiples of 64 up to %d, K odd and 1 <= K <= %d)", who, Cin, Cout, K, CV_MAX_C,
                  CV_MAX_K);
        return DSP_EINVAL;
    }
    if (B < 0 || T < 1 || (long)B * T > (1L << 24) || ld_a < Ca || (ld_a % 8) || ld_b < Cb || (ld_b % 8)) {
        set_error("%s: bad sizes B=%d T=%d row strides %ld / %ld (T >= 1, B T <= 2^24, a row stride at least the channel count and a multiple of 8)",
                  who, B, T, ld_a, ld_b);
        return DSP_EINVAL;
    }
    return B == 0 ? 1 : 0;
}

template <typename E>
static void cv_launch_conv(hipStream_t st, const void* in, long ld_in, const void* w, void* wp, int transposed, const void* bias, int bdtype,
                           void* out, long ld_out, int B, int T, int Nin, int Nout, int Cin, int Cout, int K)
{
    const long n = (long)K * Cin * Cout;
    hipLaunchKernelGGL(cv_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const cv_u16*)w, (cv_u16*)wp, Cin, Cout, K, transposed);
    const int tiles = (T + CV_ROWS - 1) / CV_ROWS;
    hipLaunchKernelGGL((cv_conv_kernel<E>), dim3((unsigned)((long)B * tiles), (unsigned)((Nout + CV_COLS - 1) / CV_COLS)), dim3(256), 0, st,
                       (const E*)in, ld_in, (const E*)wp, bias, bdtype, (E*)out, ld_out, T, Nin, Nout, K, tiles);
}

}  // namespace dsp

using namespace dsp;

extern "C" size_t dsp_conv1d_train_workspace_bytes(int phase, int B, int T, int Cin, int Cout, int K)
{
    if (B <= 0 || T <= 0 || Cin <= 0 || Cout <= 0 || K <= 0) return 0;
    const size_t pack = cv_pack_bytes(Cin, Cout, K);
    if (phase == 0) return pack;
    const long BT = (long)B * T;
    return pack + cv_align16((size_t)cv_splits(BT) * (size_t)K * Cin * Cout * sizeof(float)) +
           cv_align16((size_t)cv_db_chunks(BT) * (size_t)Cout * sizeof(float));
}

extern "C" int dsp_conv1d_train_fwd(const void* x, long ld_x, const void* w, const void* bias, void* y, long ld_y, void* workspace,
                                    size_t workspace_bytes, int act_dtype, int bias_dtype, int B, int T, int Cin, int Cout, int K,
                                    dsp_stream_t stream)
{
    const char* who = "conv1d_train_fwd";
    const int rc = cv_check(who, act_dtype, bias_dtype, B, T, Cin, Cout, K, ld_x, Cin, ld_y, Cout);
    if (rc) return rc < 0 ? rc : DSP_OK;
    if (!x || !w || !y || y == x || y == w || y == bias || workspace == x || workspace == w || workspace == y || (bias && workspace == bias)) {
        set_error("%s: null or aliased pointer", who); return DSP_EINVAL;
    }
    if ((((uintptr_t)x) | ((uintptr_t)w) | ((uintptr_t)bias) | ((uintptr_t)y)) & 15) { set_error("%s: tensors must be 16-byte aligned", who); return DSP_EINVAL; }
    if (!workspace || ((uintptr_t)workspace & 15) || workspace_bytes < dsp_conv1d_train_workspace_bytes(0, B, T, Cin, Cout, K)) {
        set_error("%s: workspace of dsp_conv1d_train_workspace_bytes(0, ...) bytes (16-byte aligned) needed", who);
        return workspace && !((uintptr_t)workspace & 15) ? DSP_ENOSPC : DSP_EINVAL;
    }
    hipStream_t st = as_stream(stream);
    DSP_DISPATCH_ELEM_16(act_dtype, E, cv_launch_conv<E>(st, x, ld_x, w, workspace, 0, bias, bias_dtype, y, ld_y, B, T, Cin, Cout, Cin, Cout, K));
    return check_launch(who);
}

extern "C" int dsp_conv1d_train_bwd(const void* dy, long ld_dy, const void* x, long ld_x, const void* w, void* dx, void* dw, void* db,
                                    void* workspace, size_t workspace_bytes, int act_dtype, int bias_dtype, int B, int T, int Cin, int Cout,
                                    int K, dsp_stream_t stream)
{
    const char* who = "conv1d_train_bwd";
    const int rc = cv_check(who, act_dtype, bias_dtype, B, T, Cin, Cout, K, ld_x, Cin, ld_dy, Cout);
    if (rc) return rc < 0 ? rc : DSP_OK;
    if (!dx && !dw && !db) return DSP_OK;
    if (!dy || !x || !w) { set_error("%s: null pointer", who); return DSP_EINVAL; }
    const void* ins[] = {dy, x, w, workspace};
    void* outs[] = {dx, dw, db};
    for (int a = 0; a < 3; ++a) {
        if (!outs[a]) continue;
        for (const void* in : ins)
            if (outs[a] == in) { set_error("%s: an output aliases an input or the workspace", who); return DSP_EINVAL; }
        for (int c = a + 1; c < 3; ++c)
            if (outs[a] == outs[c]) { set_error("%s: two outputs alias", who); return DSP_EINVAL; }
    }
    if (workspace == dy || workspace == x || workspace == w) { set_error("%s: the workspace aliases an input", who); return DSP_EINVAL; }
    if ((((uintptr_t)dy) | ((uintptr_t)x) | ((uintptr_t)w) | ((uintptr_t)dx) | ((uintptr_t)dw) | ((uintptr_t)db)) & 15) {
        set_error("%s: tensors must be 16-byte aligned", who); return DSP_EINVAL;
    }
    if (!workspace || ((uintptr_t)workspace & 15) || workspace_bytes < dsp_conv1d_train_workspace_bytes(1, B, T, Cin, Cout, K)) {
        set_error("%s: workspace of dsp_conv1d_train_workspace_bytes(1, ...) bytes (16-byte aligned) needed", who);
        return workspace && !((uintptr_t)workspace & 15) ? DSP_ENOSPC : DSP_EINVAL;
    }
    const int BT = B * T, nsplit = cv_splits(BT), nchunks = cv_db_chunks(BT);
    const size_t nw = (size_t)K * Cin * Cout;
    char* base = (char*)workspace;
    void* wp = base;
    float* part_w = (float*)(base + cv_pack_bytes(Cin, Cout, K));
    float* part_b = (float*)((char*)part_w + cv_align16((size_t)nsplit * nw * sizeof(float)));
    hipStream_t st = as_stream(stream);
    if (dx)      // the forward kernel on dy: Nin = Cout, Nout = Cin, the weight [K][Cin][Cout] with the taps reversed
        DSP_DISPATCH_ELEM_16(act_dtype, E, cv_launch_conv<E>(st, dy, ld_dy, w, wp, 1, nullptr, bias_dtype, dx, (long)Cin, B, T, Cout, Cin, Cin, Cout, K));
    if (dw) {
        const int ci_tiles = (Cin + CV_WG_TILE - 1) / CV_WG_TILE, co_tiles = (Cout + CV_WG_TILE - 1) / CV_WG_TILE;
        DSP_DISPATCH_ELEM_16(act_dtype, E, {
            hipLaunchKernelGGL((cv_wgrad_kernel<E>), dim3((unsigned)(ci_tiles * co_tiles), (unsigned)K, (unsigned)nsplit), dim3(256), 0, st, (const E*)dy,
                               ld_dy, (const E*)x, ld_x, part_w, T, BT, Cin, Cout, K, ci_tiles);
            hipLaunchKernelGGL((cv_wgrad_merge_kernel<E>), dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, st, part_w, nsplit, Cin, Cout, K, (E*)dw);
        });
    }
    if (db) {
        DSP_DISPATCH_ELEM_16(act_dtype, E, hipLaunchKernelGGL((cv_db_part_kernel<E>), dim3((unsigned)nchunks, (unsigned)(Cout / 64)), dim3(256), 0, st,
                                                              (const E*)dy, ld_dy, BT, Cout, part_b));
        hipLaunchKernelGGL(cv_db_merge_kernel, dim3((unsigned)((Cout + 255) / 256)), dim3(256), 0, st, part_b, nchunks, Cout, db, bias_dtype);
    }
    return check_launch(who);
}
