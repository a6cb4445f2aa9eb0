// extract_links_f64.hip — the transition producer (extract_links.hip) and its backward for DOUBLE q / k / log_gates (gfx950).
//
// Same specification as the fp32 entry points (include/daspeech_decode.h, DAGDecoder.extract_links, s2t_conformer_dag.py:171-212, banded branch):
//     s[i,d,h]   = scale * q[b,i,h,:].k[b,i+d+1,h,:] (+ dist_bias[d])                 valid iff i+d+1 < min(L, out_len[b])
//     p[i,d,h]   = softmax over the valid d of s[i,.,h]
//     links[i,d] = logsumexp_h(log p[i,d,h] + log_gates[b,i,h])                        -inf where invalid
//     stats[b,i,h,:] = (window max, log of the window's sum of exp(s - max));  (-inf, 0) for a row without a successor
//   backward, G = grad_links with entries of -inf links ignored, w[i,d,h] = exp(log p + log_gates - links[i,d]):
//     d log_gates[i,h] = SA[i,h] = sum_d G[i,d] w[i,d,h]        ds[i,d,h] = G[i,d] w[i,d,h] - p[i,d,h] SA[i,h]
//     dq[i,h,:] = scale sum_d ds[i,d,h] k[i+d+1,h,:]            dk[j,h,:] = scale sum_i ds[i,j-i-1,h] q[i,h,:]
//
// Stance of dag_dp_f64.hip / logsoftmax_gather_f64.hip / posterior_f64.hip: every intermediate is a double (dot-product accumulators, half-wave
// shuffles, the LDS score image, stats), only the accurate exp / log are used, products run on v_fma_f64 (the f64 matrix instruction has the
// vector unit's rate on this part, posterior_f64.hip).  A checking path: the ground truth of the fp32 / matrix-core link kernels that fits on
// the device (the torch formulation needs a [B,L,L,H] double tensor), and the first step of the double chain links -> dag_loss -> backward.
//
// ONE kernel family, the tiled walk of extract_links.hip (extract_links_tiled_kernel / _bwd_tiled_kernel) in double: a workgroup owns
// XL64_IT = 4 consecutive owner rows and walks their partner rows — thread = (head, partner): 8 heads x 32 partners per step, the partner row
// streamed from global memory in 8-channel chunks against the owners' rows in LDS (broadcast reads) — in tiles of TW partners whose
// [4][8][TW] image of doubles lives in LDS (256 B per partner):
//   forward   pass 1 streams every successor once and keeps an online (max, sum) per (vertex, head); pass 2 recomputes the scores tile by
//             tile and emits the tile's links;
//   backward  two launches.  Owners = source vertices i (dq, d log_gates): pass 1 accumulates SA the streaming way, pass 2 builds ds per
//             tile and contracts it with the tile's k rows.  Owners = successors j (dk, TRANSPOSED): every k row GATHERS over its <= TR
//             predecessors, whose soft-max state the forward left in `stats` and the first launch in grad_log_gates — scores are computed
//             twice per backward instead of scattering ds with atomics.
// TW = the partner range of a workgroup (TR + 3, rounded up to 32) up to XL64_TW = 384: one tile, nothing is walked twice in pass 2; windows
// beyond 381 successors take several tiles (LDS: 97 KB image + up to 32 KB of owner rows).  Any 1 <= TR <= L-1.
// Every reduction has one fixed order and there are no atomics: two calls on the same tensors give the same bits.  The backward writes every
// element of grad_q, grad_k and grad_log_gates (rows at or beyond the graph: zeros).
#include "common.h"
#include "../../include/daspeech_decode.h"
#include <atomic>

namespace dsp {

extern std::atomic<unsigned int> g_xl_ran;     // extract_links.hip: the kernel families launched since the last dsp_extract_links_debug_ran()

#define XL64_NEG (-__builtin_huge_val())
typedef double xl64_d2 __attribute__((ext_vector_type(2)));

constexpr int XL64_H = 8;                      // heads of the link predictor
constexpr int XL64_IT = 4;                     // owner rows per workgroup
constexpr int XL64_TW = 384;                   // widest tile (partners)
constexpr int XL64_PAD = 4;                    // row padding of the [IT][H][TW + PAD] image: the heads of one partner fall into different banks

// dot[ii] = own[ii][h][:] . prow[:] for the workgroup's XL64_IT owner rows; the ONE routine every pass and both directions use, so a
// recomputed score has the bits of the first computation.  Two FMA chains (even / odd channels) per product, added at the end.
template <int CK>
__device__ __forceinline__ void xl64_dots(const double* __restrict__ own, const double* __restrict__ prow, int h, double (&dot)[XL64_IT])
{
    double a0[XL64_IT], a1[XL64_IT];
#pragma unroll
    for (int ii = 0; ii < XL64_IT; ++ii) { a0[ii] = 0.0; a1[ii] = 0.0; }
#pragma unroll 2
    for (int c = 0; c < CK; c += 8) {
        xl64_d2 pv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) pv[u] = *reinterpret_cast<const xl64_d2*>(prow + c + 2 * u);
#pragma unroll
        for (int ii = 0; ii < XL64_IT; ++ii) {
            const double* orow = own + (ii * XL64_H + h) * CK + c;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const xl64_d2 ov = *reinterpret_cast<const xl64_d2*>(orow + 2 * u);
                a0[ii] = fma(ov.x, pv[u].x, a0[ii]); a1[ii] = fma(ov.y, pv[u].y, a1[ii]);
            }
        }
    }
#pragma unroll
    for (int ii = 0; ii < XL64_IT; ++ii) dot[ii] = a0[ii] + a1[ii];
}

__device__ __forceinline__ double xl64_score(double dot, double scale, const double* __restrict__ dist_bias, int d)
{
    return fma(dot, scale, dist_bias ? dist_bias[d] : 0.0);
}

template <int CK>
__global__ __launch_bounds__(256) void xl64_fwd_kernel(
    const double* __restrict__ q, const double* __restrict__ k, const double* __restrict__ log_gates,
    const int64_t* __restrict__ out_len, const double* __restrict__ dist_bias, double* __restrict__ links,
    double* __restrict__ stats /* [B,L,H,2] or NULL */, int L, int TR, double scale, int TW)
{
    extern __shared__ __attribute__((aligned(16))) double xl64_smem[];
    const int TWs = TW + XL64_PAD;
    double* qs = xl64_smem;                                 // [IT][H][CK]
    double* sc = qs + XL64_IT * XL64_H * CK;                // [IT][H][TWs]  scores of the current tile, slot = successor - tile start
    double* red = sc + (size_t)XL64_IT * XL64_H * TWs;      // [IT][H][2]
    const int b = blockIdx.y;
    const int tid = threadIdx.x, d0 = tid & 31, h = tid >> 5;
    const int64_t Lb64 = out_len[b];
    const int Lb = Lb64 < 0 ? 0 : (Lb64 > L ? L : (int)Lb64);
    const size_t rowstride = (size_t)XL64_H * CK;
    const int i0 = blockIdx.x * XL64_IT;
    const int nit = min(XL64_IT, L - i0);
    for (int e = tid; e < XL64_IT * XL64_H * CK; e += 256) qs[e] = e < nit * XL64_H * CK ? q[((size_t)b * L + i0) * rowstride + e] : 0.0;
    __syncthreads();
    const int jend = min(Lb, i0 + nit + TR);                // successors beyond the graph never score
    // ---- pass 1: online soft-max state per (owner, head) over all successors
    double m[XL64_IT], sm[XL64_IT];
#pragma unroll
    for (int ii = 0; ii < XL64_IT; ++ii) { m[ii] = XL64_NEG; sm[ii] = 0.0; }
    for (int jc = i0 + 1; jc < jend; jc += 32) {
        const int j = jc + d0;
        const bool live = j < jend;
        double dot[XL64_IT];
        xl64_dots<CK>(qs, k + ((size_t)b * L + (live ? j : jc)) * rowstride + (size_t)h * CK, h, dot);
#pragma unroll
        for (int ii = 0; ii < XL64_IT; ++ii) {
            const int d = j - (i0 + ii) - 1;
            if (live && ii < nit && d >= 0 && d < TR) {
                const double sv = xl64_score(dot[ii], scale, dist_bias, d);
                if (sv > m[ii]) { sm[ii] = sm[ii] * exp(m[ii] - sv) + 1.0; m[ii] = sv; }        // (m = -inf: exp(-inf) = 0)
                else sm[ii] += exp(sv - m[ii]);
            }
        }
    }
#pragma unroll
    for (int ii = 0; ii < XL64_IT; ++ii) {
        double M = m[ii];
#pragma unroll
        for (int o = 16; o >= 1; o >>= 1) M = fmax(M, __shfl_xor(M, o, 32));
        double S = (m[ii] == XL64_NEG) ? 0.0 : sm[ii] * exp(m[ii] - M);
#pragma unroll
        for (int o = 16; o >= 1; o >>= 1) S += __shfl_xor(S, o, 32);
        if (d0 == 0) {
            const double ls = (M == XL64_NEG) ? 0.0 : log(S);
            red[(ii * XL64_H + h) * 2] = M; red[(ii * XL64_H + h) * 2 + 1] = ls;
            if (stats && ii < nit) { double* st = stats + (((size_t)b * L + i0 + ii) * XL64_H + h) * 2; st[0] = M; st[1] = ls; }
        }
    }
    __syncthreads();
    // ---- pass 2: tiles of successors
    for (int jt = i0 + 1; jt < jend; jt += TW) {
        const int jte = min(jt + TW, jend);
        for (int jc = jt; jc < jte; jc += 32) {
            const int j = jc + d0;
            const bool live = j < jte;
            double dot[XL64_IT];
            xl64_dots<CK>(qs, k + ((size_t)b * L + (live ? j : jc)) * rowstride + (size_t)h * CK, h, dot);
            if (live) {
#pragma unroll
                for (int ii = 0; ii < XL64_IT; ++ii) {
                    const int d = j - (i0 + ii) - 1;
                    sc[(size_t)(ii * XL64_H + h) * TWs + (j - jt)] = (ii < nit && d >= 0 && d < TR) ? xl64_score(dot[ii], scale, dist_bias, d) : XL64_NEG;
                }
            }
        }
        __syncthreads();
        for (int ii = 0; ii < nit; ++ii) {
            const int i = i0 + ii;
            double gate[XL64_H], mh[XL64_H], lh[XL64_H];
#pragma unroll
            for (int hh = 0; hh < XL64_H; ++hh) {
                gate[hh] = log_gates[((size_t)b * L + i) * XL64_H + hh]; mh[hh] = red[(ii * XL64_H + hh) * 2]; lh[hh] = red[(ii * XL64_H + hh) * 2 + 1];
            }
            for (int js = tid; js < jte - jt; js += 256) {
                const int d = jt + js - i - 1;
                if (d < 0 || d >= TR) continue;
                double v[XL64_H], m2 = XL64_NEG;
#pragma unroll
                for (int hh = 0; hh < XL64_H; ++hh) {
                    const double sx = sc[(size_t)(ii * XL64_H + hh) * TWs + js];
                    v[hh] = (sx == XL64_NEG) ? XL64_NEG : ((sx - mh[hh]) - lh[hh]) + gate[hh];
                    m2 = fmax(m2, v[hh]);
                }
                double r = XL64_NEG;
                if (m2 != XL64_NEG) {
                    double acc = 0.0;
#pragma unroll
                    for (int hh = 0; hh < XL64_H; ++hh) acc += exp(v[hh] - m2);
                    r = m2 + log(acc);
                }
                links[((size_t)b * L + i) * TR + d] = r;
            }
        }
        __syncthreads();
    }
    // ---- slots without a successor inside the graph
    for (int ii = 0; ii < nit; ++ii) {
        const int i = i0 + ii;
        for (int d = max(0, jend - i - 1) + tid; d < TR; d += 256) links[((size_t)b * L + i) * TR + d] = XL64_NEG;
    }
}

// OWNER rows are source vertices i (dq and d log_gates = SA; partners = successors) or, TRANSPOSED, successors j (dk; partners = sources,
// whose SA the first launch wrote to `dgate`)
template <int CK, bool TRANSPOSED>
__global__ __launch_bounds__(256) void xl64_bwd_kernel(
    const double* __restrict__ q, const double* __restrict__ k, const double* __restrict__ log_gates,
    const int64_t* __restrict__ out_len, const double* __restrict__ dist_bias, const double* __restrict__ links,
    const double* __restrict__ G, const double* __restrict__ stats, double* __restrict__ dgate,
    double* __restrict__ dout /* dq or dk */, int L, int TR, double scale, int TW)
{
    extern __shared__ __attribute__((aligned(16))) double xl64_smem[];
    constexpr int CK4 = CK / 4;
    const int TWs = TW + XL64_PAD;
    double* own = xl64_smem;                                // [IT][H][CK]
    double* sc = own + XL64_IT * XL64_H * CK;               // [IT][H][TWs]  ds of the current tile, slot = partner - tile start
    double* red = sc + (size_t)XL64_IT * XL64_H * TWs;      // [IT][H]       SA of the owner rows (first launch)
    const int b = blockIdx.y;
    const int tid = threadIdx.x, d0 = tid & 31, h = tid >> 5;
    const int64_t Lb64 = out_len[b];
    const int Lb = Lb64 < 0 ? 0 : (Lb64 > L ? L : (int)Lb64);
    const size_t rowstride = (size_t)XL64_H * CK;
    const int o0 = blockIdx.x * XL64_IT;
    const int nit = min(XL64_IT, L - o0);
    const double* OWN = TRANSPOSED ? k : q;
    const double* PAR = TRANSPOSED ? q : k;
    for (int e = tid; e < XL64_IT * XL64_H * CK; e += 256) own[e] = e < nit * XL64_H * CK ? OWN[((size_t)b * L + o0) * rowstride + e] : 0.0;
    __syncthreads();
    // partner range: successors o0+1 .. o0+nit-1+TR inside the graph, or sources o0-TR .. o0+nit-2
    const int pbeg = TRANSPOSED ? max(0, o0 - TR) : (o0 + 1);
    const int pend = TRANSPOSED ? min(o0 + nit - 1, Lb) : min(Lb, o0 + nit + TR);
    double o_mx[XL64_IT] = {}, o_ls[XL64_IT] = {}, o_g[XL64_IT] = {};      // soft-max state of the owner rows (dq launch), this thread's head
    if (!TRANSPOSED) {
#pragma unroll
        for (int oo = 0; oo < XL64_IT; ++oo) {
            const size_t so = ((size_t)b * L + min(o0 + oo, L - 1)) * XL64_H + h;
            o_mx[oo] = stats[2 * so]; o_ls[oo] = stats[2 * so + 1]; o_g[oo] = log_gates[so];
        }
        // ---- pass 1: SA[owner][head] = sum_d G w
        double sa[XL64_IT];
#pragma unroll
        for (int oo = 0; oo < XL64_IT; ++oo) sa[oo] = 0.0;
        for (int pc = pbeg; pc < pend; pc += 32) {
            const int pp = pc + d0;
            const bool live = pp < pend;
            double dot[XL64_IT];
            xl64_dots<CK>(own, PAR + ((size_t)b * L + (live ? pp : pc)) * rowstride + (size_t)h * CK, h, dot);
#pragma unroll
            for (int oo = 0; oo < XL64_IT; ++oo) {
                const int o = o0 + oo, d = pp - o - 1;
                if (live && oo < nit && d >= 0 && d < TR && o_mx[oo] != XL64_NEG) {
                    const double sv = xl64_score(dot[oo], scale, dist_bias, d);
                    const size_t lo = ((size_t)b * L + o) * TR + d;
                    const double lk = links[lo];
                    if (lk != XL64_NEG) sa[oo] += G[lo] * exp(((sv - o_mx[oo]) - o_ls[oo]) + o_g[oo] - lk);
                }
            }
        }
#pragma unroll
        for (int oo = 0; oo < XL64_IT; ++oo) {
            double v = sa[oo];
#pragma unroll
            for (int o = 16; o >= 1; o >>= 1) v += __shfl_xor(v, o, 32);
            if (d0 == 0) { red[oo * XL64_H + h] = v; if (oo < nit) dgate[((size_t)b * L + o0 + oo) * XL64_H + h] = v; }
        }
        __syncthreads();
    }
    // contraction: thread = (owner group, head, 4 channels)
    const int c4 = tid & (CK4 - 1), hh = (tid / CK4) % XL64_H, op = tid / (CK4 * XL64_H);
    constexpr int NOP = 256 / (CK4 * XL64_H);              // owner groups per pass (4 for CK 32, 2 for CK 64, 1 for CK 128)
    constexpr int OPG = XL64_IT / NOP;                     // owner rows per thread
    double acc[OPG][4];
#pragma unroll
    for (int x = 0; x < OPG; ++x)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[x][c] = 0.0;
    for (int pt = pbeg; pt < pend; pt += TW) {
        const int pte = min(pt + TW, pend);
        for (int pc = pt; pc < pte; pc += 32) {
            const int pp = pc + d0;
            const bool live = pp < pte;
            double dot[XL64_IT];
            xl64_dots<CK>(own, PAR + ((size_t)b * L + (live ? pp : pc)) * rowstride + (size_t)h * CK, h, dot);
            double st_mx = 0.0, st_ls = 0.0, st_g = 0.0, st_sa = 0.0;
            if (TRANSPOSED && live) {                       // the soft-max row is the PARTNER (source vertex pp)
                const size_t so = ((size_t)b * L + pp) * XL64_H + h;
                st_mx = stats[2 * so]; st_ls = stats[2 * so + 1]; st_g = log_gates[so]; st_sa = dgate[so];
            }
            if (live) {
#pragma unroll
                for (int oo = 0; oo < XL64_IT; ++oo) {
                    const int o = o0 + oo;
                    const int d = TRANSPOSED ? (o - pp - 1) : (pp - o - 1);
                    double dsv = 0.0;
                    if (oo < nit && d >= 0 && d < TR && (!TRANSPOSED || o < Lb)) {
                        const double sv = xl64_score(dot[oo], scale, dist_bias, d);
                        const double mxv = TRANSPOSED ? st_mx : o_mx[oo], lsv = TRANSPOSED ? st_ls : o_ls[oo], gv = TRANSPOSED ? st_g : o_g[oo];
                        const double sav = TRANSPOSED ? st_sa : red[oo * XL64_H + h];
                        const size_t lo = TRANSPOSED ? (((size_t)b * L + pp) * TR + d) : (((size_t)b * L + o) * TR + d);
                        if (mxv != XL64_NEG) {
                            const double lk = links[lo], ls = (sv - mxv) - lsv;
                            const double A = (lk == XL64_NEG) ? 0.0 : G[lo] * exp(ls + gv - lk);
                            dsv = A - exp(ls) * sav;
                        }
                    }
                    sc[(size_t)(oo * XL64_H + h) * TWs + (pp - pt)] = dsv;
                }
            }
        }
        __syncthreads();
        for (int pp = pt; pp < pte; ++pp) {
            const double* prow = PAR + ((size_t)b * L + pp) * rowstride + (size_t)hh * CK + c4 * 4;
            const xl64_d2 p01 = *reinterpret_cast<const xl64_d2*>(prow), p23 = *reinterpret_cast<const xl64_d2*>(prow + 2);
#pragma unroll
            for (int x = 0; x < OPG; ++x) {
                const double dsv = sc[(size_t)((op * OPG + x) * XL64_H + hh) * TWs + (pp - pt)];
                acc[x][0] = fma(dsv, p01.x, acc[x][0]); acc[x][1] = fma(dsv, p01.y, acc[x][1]);
                acc[x][2] = fma(dsv, p23.x, acc[x][2]); acc[x][3] = fma(dsv, p23.y, acc[x][3]);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int x = 0; x < OPG; ++x) {
        const int oo = op * OPG + x;
        if (oo < nit) {
            double* o = dout + ((size_t)b * L + o0 + oo) * rowstride + (size_t)hh * CK + c4 * 4;
            xl64_d2 r01, r23;
            r01.x = acc[x][0] * scale; r01.y = acc[x][1] * scale; r23.x = acc[x][2] * scale; r23.y = acc[x][3] * scale;
            *reinterpret_cast<xl64_d2*>(o) = r01; *reinterpret_cast<xl64_d2*>(o + 2) = r23;
        }
    }
}

static int xl64_check(const char* fn, int B, int L, int H, int CK, int TR)
{
    if (B < 0 || L < 1) { set_error("%s: bad sizes B=%d L=%d", fn, B, L); return DSP_EINVAL; }
    if (H != XL64_H) { set_error("%s: needs %d heads (got H=%d)", fn, XL64_H, H); return DSP_EINVAL; }
    if (!(CK == 32 || CK == 64 || CK == 128)) { set_error("%s: head width %d (32, 64 or 128)", fn, CK); return DSP_EINVAL; }
    if (TR < 1 || TR > L - 1) { set_error("%s: window TR=%d outside 1 .. L-1 = %d", fn, TR, L - 1); return DSP_EINVAL; }
    if (B > 65535) { set_error("%s: B=%d beyond the launch grid", fn, B); return DSP_EINVAL; }
    return DSP_OK;
}

// tile width of a call: the partner range of a workgroup in one tile where it fits, XL64_TW otherwise
static int xl64_tile(int TR) { const int need = ((TR + XL64_IT - 1 + 31) / 32) * 32; return need < XL64_TW ? need : XL64_TW; }
static size_t xl64_lds(int CK, int TW) { return ((size_t)XL64_IT * XL64_H * CK + (size_t)XL64_IT * XL64_H * (TW + XL64_PAD) + 2 * XL64_IT * XL64_H) * sizeof(double); }
static unsigned int xl64_walk_bit(int TR, int TW) { return TR + XL64_IT - 1 > TW ? 512u : 0u; }

}  // namespace dsp

using namespace dsp;

extern "C" int dsp_extract_links_f64(const double* q, const double* k, const double* log_gates, const int64_t* out_len,
                                     const double* dist_bias, double* links, double* stats, int B, int L, int H, int CK, int TR, double scale,
                                     dsp_stream_t stream)
{
    const int rc = xl64_check("extract_links_f64", B, L, H, CK, TR);
    if (rc) return rc;
    if (B == 0) return DSP_OK;
    if (!q || !k || !log_gates || !out_len || !links) { set_error("extract_links_f64: null pointer"); return DSP_EINVAL; }
    if ((((uintptr_t)q) | ((uintptr_t)k)) & 15) { set_error("extract_links_f64: q / k must be 16-byte aligned"); return DSP_EINVAL; }
    const int TW = xl64_tile(TR);
    const size_t lds = xl64_lds(CK, TW);
    auto kern = CK == 64 ? xl64_fwd_kernel<64> : (CK == 32 ? xl64_fwd_kernel<32> : xl64_fwd_kernel<128>);
    if (lds > 48 * 1024) set_max_dynamic_lds((const void*)kern, (int)lds);
    hipLaunchKernelGGL(kern, dim3((L + XL64_IT - 1) / XL64_IT, B), dim3(256), lds, as_stream(stream),
                       q, k, log_gates, out_len, dist_bias, links, stats, L, TR, scale, TW);
    g_xl_ran |= 128u | xl64_walk_bit(TR, TW);
    return check_launch("extract_links_f64");
}

template <int CK>
static int xl64_bwd_launch(const double* q, const double* k, const double* g, const int64_t* ol, const double* bias, const double* links, const double* G,
                           const double* stats, double* dq, double* dk, double* dg, int B, int L, int TR, double scale, hipStream_t st)
{
    const int TW = xl64_tile(TR);
    const size_t lds = xl64_lds(CK, TW);
    auto ka = xl64_bwd_kernel<CK, false>;
    auto kb = xl64_bwd_kernel<CK, true>;
    if (lds > 48 * 1024) {
        set_max_dynamic_lds((const void*)ka, (int)lds);
        set_max_dynamic_lds((const void*)kb, (int)lds);
    }
    const dim3 grid((L + XL64_IT - 1) / XL64_IT, B);
    g_xl_ran |= 256u | xl64_walk_bit(TR, TW);
    hipLaunchKernelGGL(ka, grid, dim3(256), lds, st, q, k, g, ol, bias, links, G, stats, dg, dq, L, TR, scale, TW);
    const int rc = check_launch("extract_links_bwd_f64(dq, dgate)");
    if (rc) return rc;
    hipLaunchKernelGGL(kb, grid, dim3(256), lds, st, q, k, g, ol, bias, links, G, stats, dg, dk, L, TR, scale, TW);
    return check_launch("extract_links_bwd_f64(dk)");
}

extern "C" int dsp_extract_links_bwd_f64(const double* q, const double* k, const double* log_gates, const int64_t* out_len, const double* dist_bias,
                                         const double* links, const double* grad_links, const double* stats,
                                         double* grad_q, double* grad_k, double* grad_log_gates, int B, int L, int H, int CK, int TR, double scale,
                                         dsp_stream_t stream)
{
    const int rc = xl64_check("extract_links_bwd_f64", B, L, H, CK, TR);
    if (rc) return rc;
    if (B == 0) return DSP_OK;
    if (!q || !k || !log_gates || !out_len || !links || !grad_links || !stats || !grad_q || !grad_k || !grad_log_gates) {
        set_error("extract_links_bwd_f64: null pointer"); return DSP_EINVAL;
    }
    if ((((uintptr_t)q) | ((uintptr_t)k) | ((uintptr_t)grad_q) | ((uintptr_t)grad_k)) & 15) {
        set_error("extract_links_bwd_f64: q / k / grad_q / grad_k must be 16-byte aligned"); return DSP_EINVAL;
    }
    hipStream_t st = as_stream(stream);
    if (CK == 64) return xl64_bwd_launch<64>(q, k, log_gates, out_len, dist_bias, links, grad_links, stats, grad_q, grad_k, grad_log_gates, B, L, TR, scale, st);
    if (CK == 32) return xl64_bwd_launch<32>(q, k, log_gates, out_len, dist_bias, links, grad_links, stats, grad_q, grad_k, grad_log_gates, B, L, TR, scale, st);
    return xl64_bwd_launch<128>(q, k, log_gates, out_len, dist_bias, links, grad_links, stats, grad_q, grad_k, grad_log_gates, B, L, TR, scale, st);
}
