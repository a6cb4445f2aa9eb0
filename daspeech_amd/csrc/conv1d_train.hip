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
//   cv_wgrad_merge_kernel   adds the splits in ASCENDING order, rounds once and writes nn.Conv1d's layout.
//   cv_db_part_kernel / cv_db_merge_kernel   column sums of dy over chunks of 256 rows, then the chunks in ascending order.
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
    const int BT = B * T;
    char* base = (char*)workspace;
    void* wp = base;
    float* part_w = (float*)(base + cv_pack_bytes(Cin, Cout, K));
    float* part_b = (float*)((char*)part_w + cv_align16((size_t)cv_splits(BT) * (size_t)K * Cin * Cout * sizeof(float)));
    hipStream_t st = as_stream(stream);
    if (dx)      // the forward kernel on dy: Nin = Cout, Nout = Cin, the weight [K][Cin][Cout] with the taps reversed
        DSP_DISPATCH_ELEM_16(act_dtype, E, cv_launch_conv<E>(st, dy, ld_dy, w, wp, 1, nullptr, bias_dtype, dx, (long)Cin, B, T, Cout, Cin, Cin, Cout, K));
    if (dw) DSP_DISPATCH_ELEM_16(act_dtype, E, (cv_launch_wgrad<E, 1>(st, dy, ld_dy, x, ld_x, part_w, dw, T, T, BT, Cin, Cout, K)));
    if (db) DSP_DISPATCH_ELEM_16(act_dtype, E, cv_launch_db<E>(st, dy, ld_dy, part_b, db, bias_dtype, BT, Cout));
    return check_launch(who);
}
