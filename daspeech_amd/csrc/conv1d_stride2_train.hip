// conv1d_stride2_train.hip — Conv1d(Cin, Cout, K, STRIDE 2, dilation 1, groups 1, padding P = (K-1)/2) on CHANNELS-LAST data under autograd,
// gfx950, fp16 / bf16 (include/daspeech_decode.h: dsp_conv1d_s2_train_fwd / _bwd).  T_out = (T - 1) / 2 + 1, rows outside [0, T) of a sample
// count as zeros:
//     y [b,t,co]  = [bias[co] +] sum_k sum_ci x[b, 2t+k-P, ci] . W[co,ci,k]                                      t in [0, T_out)
//     dx[b,u,ci]  = sum_{k : (u+P-k) even, 0 <= (u+P-k)/2 < T_out} sum_co dy[b, (u+P-k)/2, co] . W[co,ci,k]
//     dW[co,ci,k] = sum_b sum_t  dy[b,t,co] . x[b, 2t+k-P, ci]
//     db[co]      = sum_b sum_t  dy[b,t,co]
// the two convolutions of the encoder's Conv1dSubsampler (80 -> 1024 and 512 -> 512, K 5) in the training step, without the transposes to
// channels-first and back.  The structure is conv1d_train.hip's (conv1d_train.h holds what the two share): 4-wave workgroups,
// v_mfma_f32_32x32x16 in the "NT" form on LDS images of pitch 72, the weight tile of the next (channel block, tap) in registers while this one
// is multiplied, fixed-order fp32 partials, no float atomics, no hand-off between workgroups.
//
//   cs_conv_kernel<E, true>    forward.  A workgroup owns 64 output rows of ONE sample x 128 columns.  Per 64 input channels the rows
//                     2 t0 - P .. 2 (t0 + 63) + P are staged as TWO images, the even and the odd local rows: tap k of output row m reads local
//                     row 2m + k, which is row m + (k >> 1) of image k & 1 — the stride-1 fragment addressing (a single image read at a row
//                     stride of 2 x 144 bytes would put eight-lane groups on the same banks).  Cin is a multiple of 16: the last channel block
//                     may hold 16 / 32 / 48 channels; the columns behind them are zeros in both LDS images, are never loaded from memory
//                     (behind column Cin of a row-strided x lies someone else's data) and their k steps are skipped.
//   cs_conv_kernel<E, false>   dx, the parity r = u & 1 of the output row in the grid.  Rows u = 2m + r are a STRIDE-1 convolution over dy with
//                     the taps k = k0 + 2j, k0 = (r + P) & 1: dy row m + d - j, d = (r + P - k0) / 2, read from cv_pack_kernel's transposed,
//                     tap-reversed weight.  A parity without a tap (K = 1: the odd rows) multiplies nothing and stores zeros.
//   cv_wgrad_kernel<E, 2> / cv_wgrad_merge_kernel / cv_db_part_kernel / cv_db_merge_kernel   over the B * T_out rows of dy; a tap that never lands
//                     inside a sample (T = 1, K = 5: four of the five) accumulates zeros and is written as zero.
#include "conv1d_train.h"

namespace dsp {

constexpr int CS_IMG = CV_ROWS + CV_MAX_K / 2;            // rows of one parity image: the row tile and the halo of (K - 1) / 2 pair offsets

// FWD:  out[b, m, n]      = [bias[n] +] sum_k sum_c in[b, 2m + k - P, c] . wp[k][n][c]                   m in [0, Tout), in has Tin rows a sample
// !FWD: out[b, 2m + r, n] = sum_j sum_c in[b, m + j - Poff, c] . wp[w0 + 2j][n][c]   j in [0, nj)        2m + r in [0, Tout), r = blockIdx.z
template <typename E, bool FWD>
__global__ __launch_bounds__(256) void cs_conv_kernel(const E* __restrict__ in, long ld_in, const E* __restrict__ wp, const void* __restrict__ bias,
                                                      int bdtype, E* __restrict__ out, long ld_out, int Tin, int Tout, int Nin, int Nout, int K,
                                                      int tiles)
{
    __shared__ __attribute__((aligned(16))) cv_u16 Xs[(FWD ? 2 : 1) * CS_IMG * CV_PITCH], Ws[CV_COLS * CV_PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave & 1, wc = wave >> 1;
    const int b = (int)blockIdx.x / tiles, t0 = ((int)blockIdx.x % tiles) * CV_ROWS, n0 = (int)blockIdx.y * CV_COLS;
    const int P = (K - 1) / 2, r = FWD ? 0 : (int)blockIdx.z;
    // the taps of this launch: their count, the first packed tap and the input row of (m = 0, j = 0)
    const int k0 = (r + P) & 1;
    const int nj = FWD ? K : (K - k0 + 1) / 2;
    const int w0 = FWD ? 0 : K - 1 - k0 - 2 * (nj - 1);
    const int Poff = FWD ? P : nj - 1 - (r + P - k0) / 2;
    const int M = FWD ? Tout : (Tout - r + 1) / 2;                          // output rows of a sample this launch (this parity) owns
    if (t0 >= M) return;                                                    // the odd parity has one tile fewer where T <= 64 (mod 128)
    const int nx = FWD ? 2 * (CV_ROWS - 1) + K : CV_ROWS + nj - 1;
    const int nc = nj ? (Nin + CV_KC - 1) / CV_KC : 0;
    const E* inb = in + (size_t)b * (size_t)Tin * (size_t)ld_in;
    // the weight tile of (channel block c, tap j): 128 rows x 8 quads, 4 quads a thread
    const int wrow = tid >> 3, wq = (tid & 7) * 8;
    uint4 wreg[4];
#define CS_LOAD_W(c, j)                                                                                                            \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                                                \
        const int n = n0 + wrow + 32 * i;                                                                                          \
        wreg[i] = (n < Nout && (c) * CV_KC + wq < Nin)                                                                             \
                      ? *reinterpret_cast<const uint4*>(wp + ((size_t)(w0 + (FWD ? 1 : 2) * (j)) * Nout + n) * (size_t)Nin + (c) * CV_KC + wq) \
                      : make_uint4(0u, 0u, 0u, 0u);                                                                                \
    }
    cv_acc a0 = {0}, a1 = {0};
    if (nc) { CS_LOAD_W(0, 0) }
#pragma unroll 1
    for (int c = 0; c < nc; ++c) {
        __syncthreads();                                                    // the products of the block before this one have read Xs and Ws
        for (int i = tid; i < nx * 8; i += 256) {
            const int rl = i >> 3, q = (i & 7) * 8, t = (FWD ? 2 : 1) * t0 - Poff + rl;
            uint4 u = make_uint4(0u, 0u, 0u, 0u);
            if (t >= 0 && t < Tin && c * CV_KC + q < Nin) u = *reinterpret_cast<const uint4*>(inb + (size_t)t * (size_t)ld_in + c * CV_KC + q);
            *reinterpret_cast<uint4*>(Xs + (FWD ? (rl & 1) * CS_IMG + (rl >> 1) : rl) * CV_PITCH + q) = u;
        }
        const int ns = Nin - c * CV_KC >= CV_KC ? 4 : (Nin - c * CV_KC) / 16;      // k steps of 16 channels that hold any
#pragma unroll 1
        for (int j = 0; j < nj; ++j) {
            if (j) __syncthreads();                                         // the tap before this one has read Ws
#pragma unroll
            for (int i = 0; i < 4; ++i) *reinterpret_cast<uint4*>(Ws + (wrow + 32 * i) * CV_PITCH + wq) = wreg[i];
            __syncthreads();
            const int jn = j + 1 < nj ? j + 1 : 0, cn = j + 1 < nj ? c : c + 1;
            if (cn < nc) { CS_LOAD_W(cn, jn) }                              // in flight while this tile is multiplied
            const cv_u16* A = Xs + (32 * wr + (FWD ? (j & 1) * CS_IMG + (j >> 1) : j)) * CV_PITCH;
            const cv_u16* Bt = Ws + 64 * wc * CV_PITCH;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                if (s < ns) {
                    const typename Cv<E>::V va = cv_frag<E>(A, s, lane);
                    a0 = Cv<E>::mma(va, cv_frag<E>(Bt, s, lane), a0);
                    a1 = Cv<E>::mma(va, cv_frag<E>(Bt + 32 * CV_PITCH, s, lane), a1);
                }
            }
        }
    }
#undef CS_LOAD_W
    const int col = lane & 31, hi = lane >> 5;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int n = n0 + 64 * wc + 32 * h + col;
        if (n >= Nout) continue;
        const float bv = bias ? param_load(bias, bdtype, n) : 0.f;
        E* o = out + (size_t)b * (size_t)Tout * (size_t)ld_out + n;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int m = t0 + 32 * wr + CV_ROW(reg, hi);
            if (m < M) o[(size_t)(FWD ? m : 2 * m + r) * (size_t)ld_out] = from_f<E>((h ? a1[reg] : a0[reg]) + bv);
        }
    }
}

}  // namespace dsp

using namespace dsp;

extern "C" size_t dsp_conv1d_s2_train_workspace_bytes(int phase, int B, int T, int Cin, int Cout, int K)
{
    return cv_workspace_bytes<2>(phase, B, T, Cin, Cout, K);
}

extern "C" int dsp_conv1d_s2_train_fwd(const void* x, long ld_x, const void* w, const void* bias, void* y, long ld_y, void* workspace,
                                       size_t workspace_bytes, int act_dtype, int bias_dtype, int B, int T, int Cin, int Cout, int K,
                                       dsp_stream_t stream)
{
    const char* who = "conv1d_s2_train_fwd";
    const int rc = cv_fwd_gates<2>(who, "dsp_conv1d_s2_train_workspace_bytes(0, ...)", x, ld_x, w, bias, y, ld_y, workspace, workspace_bytes, act_dtype,
                                   bias_dtype, B, T, Cin, Cout, K);
    if (rc) return rc < 0 ? rc : DSP_OK;
    hipStream_t st = as_stream(stream);
    const long n = (long)K * Cin * Cout;
    const int To = cv_tout<2>(T), tiles = (To + CV_ROWS - 1) / CV_ROWS;
    hipLaunchKernelGGL(cv_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const cv_u16*)w, (cv_u16*)workspace, Cin, Cout, K, 0);
    DSP_DISPATCH_ELEM_16(act_dtype, E,
                         hipLaunchKernelGGL((cs_conv_kernel<E, true>), dim3((unsigned)((long)B * tiles), (unsigned)((Cout + CV_COLS - 1) / CV_COLS)),
                                            dim3(256), 0, st, (const E*)x, ld_x, (const E*)workspace, bias, bias_dtype, (E*)y, ld_y, T, To, Cin, Cout,
                                            K, tiles));
    return check_launch(who);
}

extern "C" int dsp_conv1d_s2_train_bwd(const void* dy, long ld_dy, const void* x, long ld_x, const void* w, void* dx, void* dw, void* db,
                                       void* workspace, size_t workspace_bytes, int act_dtype, int bias_dtype, int B, int T, int Cin, int Cout,
                                       int K, dsp_stream_t stream)
{
    const char* who = "conv1d_s2_train_bwd";
    const int rc = cv_bwd_gates<2>(who, "dsp_conv1d_s2_train_workspace_bytes(1, ...)", dy, ld_dy, x, ld_x, w, dx, dw, db, workspace, workspace_bytes,
                                   act_dtype, bias_dtype, B, T, Cin, Cout, K);
    if (rc) return rc < 0 ? rc : DSP_OK;
    const CvWorkspace ws = cv_carve<2>(workspace, B, T, Cin, Cout, K);
    hipStream_t st = as_stream(stream);
    if (dx) {    // both parities of the rows of dx in one launch: a stride-1 convolution each over dy, Nin = Cout, Nout = Cin
        const long n = (long)K * Cin * Cout;
        const int tiles = ((T + 1) / 2 + CV_ROWS - 1) / CV_ROWS;
        hipLaunchKernelGGL(cv_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const cv_u16*)w, (cv_u16*)ws.wp, Cin, Cout, K, 1);
        DSP_DISPATCH_ELEM_16(act_dtype, E,
                             hipLaunchKernelGGL((cs_conv_kernel<E, false>),
                                                dim3((unsigned)((long)B * tiles), (unsigned)((Cin + CV_COLS - 1) / CV_COLS), 2u), dim3(256), 0, st,
                                                (const E*)dy, ld_dy, (const E*)ws.wp, nullptr, bias_dtype, (E*)dx, (long)Cin, cv_tout<2>(T), T, Cout, Cin, K,
                                                tiles));
    }
    DSP_DISPATCH_ELEM_16(act_dtype, E, (cv_launch_param_grads<E, 2>(st, dy, ld_dy, x, ld_x, ws, dw, db, bias_dtype, B, T, Cin, Cout, K)));
    return check_launch(who);
}
