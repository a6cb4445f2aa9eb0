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
// The operand types, cv_pack_kernel and the kernels of dW and db live in conv1d_train.h, shared with conv1d_stride2_train.hip:
//   cv_wgrad_kernel   a workgroup of 4 waves owns (128 co x 128 ci, one tap, one split of DSP_CONV1D_TRAIN_WGRAD_ROWS rows of the flattened
//                     B*T); it walks its rows 64 at a time in ascending order, dy and the tap-shifted x staged TRANSPOSED (row index
//                     contiguous, two rows per 32-bit LDS write), and writes one fp32 partial [split][K][Cout][Cin];
//   cv_wgrad_merge_kernel, cv_db_part_kernel / cv_db_merge_kernel   the splits, and dy's column sums over chunks of 256 rows, in ASCENDING order.
// No float atomics, no hand-off between workgroups: the same inputs give the same bits on every call, and dx, dW, db are separate launches, so
// leaving one out does not change the others.  Every row is computed, padded frames included.
#include "conv1d_train.h"

namespace dsp {

constexpr int CV_XROWS = CV_ROWS + CV_MAX_K - 1;          // the row tile and its halo

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
    return cv_workspace_bytes<1>(phase, B, T, Cin, Cout, K);
}

extern "C" int dsp_conv1d_train_fwd(const void* x, long ld_x, const void* w, const void* bias, void* y, long ld_y, void* workspace,
                                    size_t workspace_bytes, int act_dtype, int bias_dtype, int B, int T, int Cin, int Cout, int K,
                                    dsp_stream_t stream)
{
    const char* who = "conv1d_train_fwd";
    const int rc = cv_fwd_gates<1>(who, "dsp_conv1d_train_workspace_bytes(0, ...)", x, ld_x, w, bias, y, ld_y, workspace, workspace_bytes, act_dtype,
                                   bias_dtype, B, T, Cin, Cout, K);
    if (rc) return rc < 0 ? rc : DSP_OK;
    hipStream_t st = as_stream(stream);
    DSP_DISPATCH_ELEM_16(act_dtype, E, cv_launch_conv<E>(st, x, ld_x, w, workspace, 0, bias, bias_dtype, y, ld_y, B, T, Cin, Cout, Cin, Cout, K));
    return check_launch(who);
}

extern "C" int dsp_conv1d_train_bwd(const void* dy, long ld_dy, const void* x, long ld_x, const void* w, void* dx, void* dw, void* db,
                                    void* workspace, size_t workspace_bytes, int act_dtype, int bias_dtype, int B, int T, int Cin, int Cout,
                                    int K, dsp_stream_t stream)
{
    const char* who = "conv1d_train_bwd";
    const int rc = cv_bwd_gates<1>(who, "dsp_conv1d_train_workspace_bytes(1, ...)", dy, ld_dy, x, ld_x, w, dx, dw, db, workspace, workspace_bytes,
                                   act_dtype, bias_dtype, B, T, Cin, Cout, K);
    if (rc) return rc < 0 ? rc : DSP_OK;
    const CvWorkspace ws = cv_carve<1>(workspace, B, T, Cin, Cout, K);
    hipStream_t st = as_stream(stream);
    if (dx)      // the forward kernel on dy: Nin = Cout, Nout = Cin, the weight [K][Cin][Cout] with the taps reversed
        DSP_DISPATCH_ELEM_16(act_dtype, E, cv_launch_conv<E>(st, dy, ld_dy, w, ws.wp, 1, nullptr, bias_dtype, dx, (long)Cin, B, T, Cout, Cin, Cin, Cout, K));
    DSP_DISPATCH_ELEM_16(act_dtype, E, (cv_launch_param_grads<E, 1>(st, dy, ld_dy, x, ld_x, ws, dw, db, bias_dtype, B, T, Cin, Cout, K)));
    return check_launch(who);
}
