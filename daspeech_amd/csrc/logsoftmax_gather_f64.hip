// logsoftmax_gather_f64.hip — K1 and its backward for DOUBLE logits (gfx950).
//
// The reference dispatches its gather for double as well (logsoftmax_gather.cu:46-58,340-347: double logits are computed in double and
// `selected_result` is at::kDouble).  The kernels of logsoftmax_gather.hip compute in fp32 and carry float* match / g / row_stats, so double
// gets its own two entry points, dsp_logsoftmax_gather_f64 / dsp_logsoftmax_gather_bwd_f64 — same stance as dag_dp_f64.hip: every
// intermediate is a double (lane accumulators, wave shuffles, LDS slots, the staged match tile, the row statistics, the scatter image), and
// only the accurate exp / log are used, because the point of the dtype is double accuracy.
//
// Forward (lsg64_fwd_kernel) — the traffic shape of the fp32 generic kernel (lsg_fwd_kernel):
//   * one 256-thread workgroup walks a tile of RT consecutive vertices; RT = 16 halved until the [S][RT] stage of doubles fits 60 KB
//     (the fp32 kernel's allowance: S = 512 gives RT = 8 here where fp32 takes 16);
//   * the row is read ONCE from HBM with 16-byte loads (two doubles per lane per load, four loads in flight per lane); a lane folds the
//     eight values of a pass into its online (max, sum) with ONE rescale — 9 exp per 8 logits instead of 3 per 2; wave shuffles + one LDS
//     hop combine the lanes;
//   * the S gathered logits and the optional softmax store re-read the row while it is L2-resident;
//   * gathered values are staged in LDS as [S][RT] doubles, `match` is written in RT-double runs along the vertex axis;
//   * a row that starts off the 16-byte grid (odd V: every other row) peels ONE head element and, when what is left is odd, one tail
//     element; the body moves as 16-byte vectors.
//   Three modes: softmax stored in place (write_softmax), "lazy" (row_stats: two doubles per row, (max, 1/sum exp), logits untouched), or
//   neither (only `match` is written).
//   Rows on the 16-byte grid of up to 8192 columns take lsg64_fwd_reg_kernel instead (the row in registers, one exp per logit, the softmax
//   stored from the registers; see there).  Softmax stores are non-temporal in both kernels (the stored row is not read again by this
//   launch; at C2 the eager forward went 4.5 -> 4.0 ms with them), the row loads stay temporal because the gathers re-read the row from L2.
//
// Backward (lsg64_bwd_kernel): row <- softmax * (-(sum_s g)) + scatter_add(g), in place; softmax is the buffer's content, or
//   exp(x - max) * inv from the row statistics in the lazy form.  A workgroup owns RT consecutive rows and stages their [S][RT] gradient tile
//   through LDS (runs along the vertex axis of a [B,S,L] gradient).  The scatter image in LDS covers a COLUMN CHUNK of CH doubles
//   (CH = 4096, 32 KB; a V-double image would end near 16 K columns and leave one workgroup per CU long before): a row is processed chunk by
//   chunk — scatter the gradients whose index falls into the chunk (LDS atomic add, duplicates accumulate like scatter_add_), stream the
//   chunk (non-temporal 16-byte loads and stores), re-zero what was touched.  The S (index, gradient) pairs are re-scanned per chunk; S is
//   a few hundred against thousands of columns.  Any V is served; rows of up to CH columns take one chunk.
//   atomicAdd(double*) on the LDS image compiles to the native ds_add_f64 (no compare-and-swap loop in the disassembly: 0 x ds_cmpst /
//   cmpswap, 1 x ds_add_f64 per instance).
//
// Code-object metadata (hipcc -O3, gfx950):      VGPRs   scratch
//   lsg64_fwd_kernel                               105     0
//   lsg64_fwd_reg_kernel<2 / 4 / 8 / 16>   73 / 83 / 95 / 137     0
//   lsg64_bwd_kernel<false>  (from the softmax)     48     0
//   lsg64_bwd_kernel<true>   (lazy)                 82     0
#include "common.h"

namespace dsp {

#define L64_NEG (-__builtin_huge_val())
typedef double lsg_d2 __attribute__((ext_vector_type(2)));

template <bool NT>
__device__ __forceinline__ lsg_d2 lsg64_ld(const double* p)
{
    if constexpr (NT) return __builtin_nontemporal_load(reinterpret_cast<const lsg_d2*>(p));
    else return *reinterpret_cast<const lsg_d2*>(p);
}
template <bool NT>
__device__ __forceinline__ void lsg64_st(double* p, lsg_d2 v)
{
    if constexpr (NT) __builtin_nontemporal_store(v, reinterpret_cast<lsg_d2*>(p));
    else *reinterpret_cast<lsg_d2*>(p) = v;
}

// A row of doubles is 8-byte aligned; the 16-byte body starts after `head` (0 or 1) elements and holds nb vectors, `tail` (0 or 1) follows.
struct Peel64 {
    int head, nb, tail;
    __device__ __forceinline__ Peel64(const double* row, int V) {
        head = (((uintptr_t)row & 15) != 0 && V > 0) ? 1 : 0;
        nb = (V - head) >> 1; tail = (V - head) & 1;
    }
};

__device__ __forceinline__ void online_merge64(double& m, double& s, double m2, double s2) {
    const double nm = fmax(m, m2);
    if (nm == L64_NEG) { s = 0.0; m = nm; return; }
    s = s * exp(m - nm) + s2 * exp(m2 - nm);
    m = nm;
}

// block-wide (max, sum-exp) of one row; result broadcast to every thread.  red = 2 x 8 doubles of LDS.
__device__ __forceinline__ void row_max_sum64(const double* row, int V, const Peel64& pl, double* red, double& m_out, double& s_out) {
    const int tid = threadIdx.x;
    double m = L64_NEG, s = 0.0;
    if (tid == 0 && pl.head) { const double x = row[0]; if (x != L64_NEG) { m = x; s = 1.0; } }
    if (tid == 1 && pl.tail) { const double x = row[V - 1]; if (x != L64_NEG) { m = x; s = 1.0; } }
    const double* body = row + pl.head;
    for (int i0 = tid; i0 < pl.nb; i0 += 4 * 256) {
        lsg_d2 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u * 256;
            v[u].x = L64_NEG; v[u].y = L64_NEG;
            if (i < pl.nb) v[u] = lsg64_ld<false>(body + 2 * (size_t)i);
        }
        double lm = fmax(v[0].x, v[0].y);
#pragma unroll
        for (int u = 1; u < 4; ++u) lm = fmax(lm, fmax(v[u].x, v[u].y));
        const double nm = fmax(m, lm);
        if (nm != L64_NEG) {
            double acc = s * exp(m - nm);
#pragma unroll
            for (int u = 0; u < 4; ++u) acc += exp(v[u].x - nm) + exp(v[u].y - nm);
            s = acc;
        }
        m = nm;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
        online_merge64(m, s, m2, s2);
    }
    const int wave = tid >> 6;
    __syncthreads();                          // red[] free (previous row's readers are done)
    if ((tid & 63) == 0) { red[wave] = m; red[8 + wave] = s; }
    __syncthreads();
    m = red[0]; s = red[8];
#pragma unroll
    for (int w = 1; w < 4; ++w) online_merge64(m, s, red[w], red[8 + w]);
    m_out = m; s_out = s;
}

__global__ __launch_bounds__(256) void lsg64_fwd_kernel(
    double* __restrict__ x, const int64_t* __restrict__ idx, int64_t isb, int64_t isj, int64_t iss,
    double* __restrict__ out, int64_t osb, int64_t osj, int64_t oss,
    int B, int L, int V, int S, int RT, int write_softmax, double* __restrict__ stats)
{
    extern __shared__ __attribute__((aligned(16))) double smem64[];
    double* red = smem64;             // 16 doubles
    double* stage = smem64 + 16;      // [S][RT]
    const int tid = threadIdx.x;
    const int tiles_per_b = (L + RT - 1) / RT;
    const long ntiles = (long)B * tiles_per_b;
    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int b = (int)(tile / tiles_per_b);
        const int j0 = (int)(tile % tiles_per_b) * RT;
        const int nr = min(RT, L - j0);
        for (int r = 0; r < nr; ++r) {
            double* row = x + ((size_t)b * L + (j0 + r)) * V;
            const Peel64 pl(row, V);
            double m, s;
            row_max_sum64(row, V, pl, red, m, s);
            const double ls = log(s);
            if (stats && tid == 0) { double* st2 = stats + 2 * ((size_t)b * L + (j0 + r)); st2[0] = m; st2[1] = 1.0 / s; }
            for (int k = tid; k < S; k += 256) {
                int64_t t = idx[b * isb + (int64_t)(j0 + r) * isj + k * iss];
                t = t < 0 ? 0 : (t >= V ? V - 1 : t);
                stage[k * RT + r] = (row[t] - m) - ls;               // logsoftmax_gather.cu:293
            }
            if (write_softmax) {
                __syncthreads();                                      // gathers read the ORIGINAL logits
                const double inv = 1.0 / s;
                if (tid == 0 && pl.head) row[0] = exp(row[0] - m) * inv;
                if (tid == 1 && pl.tail) row[V - 1] = exp(row[V - 1] - m) * inv;
                double* body = row + pl.head;
                for (int i0 = tid; i0 < pl.nb; i0 += 2 * 256) {
                    const int i1 = i0 + 256;
                    lsg_d2 v0 = lsg64_ld<false>(body + 2 * (size_t)i0), v1;
                    if (i1 < pl.nb) v1 = lsg64_ld<false>(body + 2 * (size_t)i1);
                    v0.x = exp(v0.x - m) * inv; v0.y = exp(v0.y - m) * inv;
                    lsg64_st<true>(body + 2 * (size_t)i0, v0);
                    if (i1 < pl.nb) {
                        v1.x = exp(v1.x - m) * inv; v1.y = exp(v1.y - m) * inv;
                        lsg64_st<true>(body + 2 * (size_t)i1, v1);
                    }
                }
            }
        }
        __syncthreads();
        const int tot = S * nr;
        if (osj == 1 || oss != 1) {          // runs along the vertex axis: [B,S,L] layout
            for (int e = tid; e < tot; e += 256) {
                const int k = e / nr, r = e - k * nr;
                out[b * osb + (int64_t)(j0 + r) * osj + k * oss] = stage[k * RT + r];
            }
        } else {                             // runs along S: the reference's [B,L,S] layout
            for (int e = tid; e < tot; e += 256) {
                const int r = e / S, k = e - r * S;
                out[b * osb + (int64_t)(j0 + r) * osj + k * oss] = stage[k * RT + r];
            }
        }
        __syncthreads();
    }
}

// Register-resident forward for rows on the 16-byte grid of up to NV x 256 vectors (V <= 8192 at NV = 16: 64 VGPRs of row per lane): the row
// is read ONCE into registers, the max is taken exactly, every logit costs ONE exp (exp(x - max) replaces the logit in its register, the
// sum follows) and the softmax is stored straight from the registers — no second pass over the logits and no second exp per element, which
// is what the generic kernel's softmax store pays (fp64 exp is a long VALU sequence: at C2 the store pass cost as much as the row pass).
template <int NV>
__global__ __launch_bounds__(256) void lsg64_fwd_reg_kernel(
    double* __restrict__ x, const int64_t* __restrict__ idx, int64_t isb, int64_t isj, int64_t iss,
    double* __restrict__ out, int64_t osb, int64_t osj, int64_t oss,
    int B, int L, int V, int S, int RT, int write_softmax, double* __restrict__ stats)
{
    extern __shared__ __attribute__((aligned(16))) double smem64[];
    double* red = smem64;             // 16 doubles: [0..3] wave maxima, [8..11] wave sums
    double* stage = smem64 + 16;      // [S][RT]
    const int tid = threadIdx.x;
    const int nb = V >> 1;            // V is even and the rows are 16-byte aligned (launch_fwd64)
    const int tiles_per_b = (L + RT - 1) / RT;
    const long ntiles = (long)B * tiles_per_b;
    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int b = (int)(tile / tiles_per_b);
        const int j0 = (int)(tile % tiles_per_b) * RT;
        const int nr = min(RT, L - j0);
        for (int r = 0; r < nr; ++r) {
            double* row = x + ((size_t)b * L + (j0 + r)) * V;
            lsg_d2 v[NV];
#pragma unroll
            for (int k = 0; k < NV; ++k) {
                const int i = k * 256 + tid;
                v[k].x = L64_NEG; v[k].y = L64_NEG;
                if (i < nb) v[k] = lsg64_ld<false>(row + 2 * (size_t)i);
            }
            double m = L64_NEG;
#pragma unroll
            for (int k = 0; k < NV; ++k) m = fmax(m, fmax(v[k].x, v[k].y));
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
            if ((tid & 63) == 0) red[tid >> 6] = m;
            __syncthreads();
            m = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
            const double mm = (m == L64_NEG) ? 0.0 : m;           // (an all -inf row is outside the contract; keep it free of NaN)
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < NV; ++k) { v[k].x = exp(v[k].x - mm); v[k].y = exp(v[k].y - mm); s += v[k].x + v[k].y; }      // padding lanes: exp(-inf) = 0
            s = wave_sum(s);
            if ((tid & 63) == 0) red[8 + (tid >> 6)] = s;
            __syncthreads();
            s = (red[8] + red[9]) + (red[10] + red[11]);
            const double ls = log(s);
            if (stats && tid == 0) { double* st2 = stats + 2 * ((size_t)b * L + (j0 + r)); st2[0] = m; st2[1] = 1.0 / s; }
            for (int k = tid; k < S; k += 256) {
                int64_t t = idx[b * isb + (int64_t)(j0 + r) * isj + k * iss];
                t = t < 0 ? 0 : (t >= V ? V - 1 : t);
                stage[k * RT + r] = (row[t] - m) - ls;               // logsoftmax_gather.cu:293
            }
            if (write_softmax) {
                __syncthreads();                                      // gathers read the ORIGINAL logits
                const double inv = 1.0 / s;
#pragma unroll
                for (int k = 0; k < NV; ++k) {
                    const int i = k * 256 + tid;
                    if (i < nb) { lsg_d2 o; o.x = v[k].x * inv; o.y = v[k].y * inv; lsg64_st<true>(row + 2 * (size_t)i, o); }
                }
            }
        }
        __syncthreads();
        const int tot = S * nr;
        if (osj == 1 || oss != 1) {
            for (int e = tid; e < tot; e += 256) {
                const int k = e / nr, r = e - k * nr;
                out[b * osb + (int64_t)(j0 + r) * osj + k * oss] = stage[k * RT + r];
            }
        } else {
            for (int e = tid; e < tot; e += 256) {
                const int r = e / S, k = e - r * S;
                out[b * osb + (int64_t)(j0 + r) * osj + k * oss] = stage[k * RT + r];
            }
        }
        __syncthreads();
    }
}

// backward: row <- softmax * (-(sum_s g)) + scatter_add(g)     (dag_loss.py:293-295), the scatter image a column chunk at a time
template <bool LAZY>
__global__ __launch_bounds__(256) void lsg64_bwd_kernel(
    double* __restrict__ x, const int64_t* __restrict__ idx, int64_t isb, int64_t isj, int64_t iss,
    const double* __restrict__ g, int64_t gsb, int64_t gsj, int64_t gss,
    int B, int L, int V, int S, int RT, int CH, const double* __restrict__ stats)
{
    extern __shared__ __attribute__((aligned(16))) double smem64[];
    double* red = smem64;             // 16 doubles
    double* delta = smem64 + 16;      // [CH + 2]  scatter image of the current column chunk (chunk 0 also holds the peeled head element)
    double* gt = delta + CH + 2;      // [S][RT]
    const int tid = threadIdx.x;
    for (int v = tid; v < CH + 2; v += 256) delta[v] = 0.0;
    const int tiles_per_b = (L + RT - 1) / RT;
    const long ntiles = (long)B * tiles_per_b;
    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int b = (int)(tile / tiles_per_b);
        const int j0 = (int)(tile % tiles_per_b) * RT;
        const int nr = min(RT, L - j0);
        __syncthreads();                                   // previous tile's gt / delta use is over
        const int tot = S * nr;
        if (gsj == 1) {                                    // [B][S][L] gradients: runs along j
            for (int e = tid; e < tot; e += 256) { const int k = e / nr, r = e - k * nr; gt[k * RT + r] = g[b * gsb + (int64_t)(j0 + r) + k * gss]; }
        } else {
            for (int e = tid; e < tot; e += 256) { const int r = e / S, k = e - r * S; gt[k * RT + r] = g[b * gsb + (int64_t)(j0 + r) * gsj + k * gss]; }
        }
        __syncthreads();
        for (int r = 0; r < nr; ++r) {
            const size_t srow = (size_t)b * L + (j0 + r);
            double* row = x + srow * V;
            const int head = (((uintptr_t)row & 15) != 0) ? 1 : 0;
            // LAZY: the buffer still holds the LOGITS; softmax = exp(x - m) * inv from the forward's row statistics
            const double rm = LAZY ? stats[2 * srow] : 0.0, rinv = LAZY ? stats[2 * srow + 1] : 1.0;
            const int64_t ibase = b * isb + (int64_t)(j0 + r) * isj;
            double neg = 0.0;
            // chunk c covers the columns [lo, hi): chunk 0 starts at column 0 (with the head element), the others on the 16-byte grid
            for (int lo = 0; lo < V;) {
                const int vlo = lo == 0 ? head : lo;                               // first column of the chunk's 16-byte body
                const int hi = (int)min((long)V, (long)vlo + CH);
                double gs = 0.0;
                for (int k = tid; k < S; k += 256) {
                    const double gv = gt[k * RT + r];
                    int64_t t = idx[ibase + k * iss];
                    t = t < 0 ? 0 : (t >= V ? V - 1 : t);
                    gs += gv;
                    if (t >= lo && t < hi) atomicAdd(&delta[(int)t - lo], gv);
                }
                if (lo == 0) {
                    gs = wave_sum(gs);
                    if ((tid & 63) == 0) red[tid >> 6] = gs;
                }
                __syncthreads();
                if (lo == 0) neg = -(red[0] + red[1] + red[2] + red[3]);
                if (lo == 0 && head && tid == 0) { const double xv = row[0]; row[0] = (LAZY ? exp(xv - rm) * rinv : xv) * neg + delta[0]; }
                const int npair = (hi - vlo) >> 1;
                if (((hi - vlo) & 1) && tid == 255) {                              // odd remainder: the row's last column
                    const double xv = row[hi - 1]; row[hi - 1] = (LAZY ? exp(xv - rm) * rinv : xv) * neg + delta[hi - 1 - lo];
                }
                double* body = row + vlo;
                const double* dl = delta + (vlo - lo);
                for (int i0 = tid; i0 < npair; i0 += 4 * 256) {
                    lsg_d2 v[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int i = i0 + u * 256;
                        if (i < npair) v[u] = lsg64_ld<true>(body + 2 * (size_t)i);
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int i = i0 + u * 256;
                        if (i < npair) {
                            lsg_d2 o;
                            o.x = (LAZY ? exp(v[u].x - rm) * rinv : v[u].x) * neg + dl[2 * i];
                            o.y = (LAZY ? exp(v[u].y - rm) * rinv : v[u].y) * neg + dl[2 * i + 1];
                            lsg64_st<true>(body + 2 * (size_t)i, o);
                        }
                    }
                }
                __syncthreads();
                for (int k = tid; k < S; k += 256) {                               // re-zero only what was touched
                    int64_t t = idx[ibase + k * iss];
                    t = t < 0 ? 0 : (t >= V ? V - 1 : t);
                    if (t >= lo && t < hi) delta[(int)t - lo] = 0.0;
                }
                __syncthreads();
                lo = hi;
            }
        }
    }
}

static int launch_fwd64(double* logits, const int64_t* idx, int64_t isb, int64_t isj, int64_t iss, double* match,
                        int64_t osb, int64_t osj, int64_t oss, int B, int L, int V, int S, int ws, hipStream_t st, double* stats)
{
    int RT = 16;
    while (RT > 1 && (size_t)S * RT * sizeof(double) > 60 * 1024) RT >>= 1;
    if ((size_t)S * RT * sizeof(double) > 150 * 1024) { set_error("logsoftmax_gather_f64: S=%d too large for LDS staging", S); return DSP_EINVAL; }
    if (RT > L) { RT = 1; while (RT * 2 <= L) RT *= 2; }
    const size_t lds = (16 + (size_t)S * RT) * sizeof(double);
    const long ntiles = (long)B * ((L + RT - 1) / RT);
    const int grid = (int)(ntiles < 2048 ? ntiles : 2048);
    const int nvec = (V / 2 + 255) / 256;
    if (V % 2 == 0 && (uintptr_t)logits % 16 == 0 && nvec <= 16) {            // every row on the 16-byte grid and short enough for the registers
        auto kr = nvec <= 2 ? lsg64_fwd_reg_kernel<2> : nvec <= 4 ? lsg64_fwd_reg_kernel<4> : nvec <= 8 ? lsg64_fwd_reg_kernel<8> : lsg64_fwd_reg_kernel<16>;
        if (lds > 48 * 1024) set_max_dynamic_lds((const void*)kr, (int)lds);
        hipLaunchKernelGGL(kr, dim3(grid), dim3(256), lds, st, logits, idx, isb, isj, iss, match, osb, osj, oss, B, L, V, S, RT, ws, stats);
        return check_launch("logsoftmax_gather_f64(reg)");
    }
    if (lds > 48 * 1024) set_max_dynamic_lds((const void*)lsg64_fwd_kernel, (int)lds);
    hipLaunchKernelGGL(lsg64_fwd_kernel, dim3(grid), dim3(256), lds, st, logits, idx, isb, isj, iss, match, osb, osj, oss,
                       B, L, V, S, RT, ws, stats);
    return check_launch("logsoftmax_gather_f64");
}

template <bool LAZY>
static int launch_bwd64(double* sm, const int64_t* idx, int64_t isb, int64_t isj, int64_t iss, const double* g,
                        int64_t gsb, int64_t gsj, int64_t gss, int B, int L, int V, int S, hipStream_t st, const double* stats)
{
    // column chunk of the scatter image: the whole row when it is short, else 4096 doubles (even: chunks after the first stay on the 16-byte grid)
    const int CH = V < 4096 ? ((V + 1) & ~1) : 4096;
    int RT = 8;
    while (RT > 1 && (16 + (size_t)CH + 2 + (size_t)S * RT) * sizeof(double) > 78 * 1024) RT >>= 1;       // two workgroups per CU
    if (RT > L) { RT = 1; while (RT * 2 <= L) RT *= 2; }
    const size_t lds = (16 + (size_t)CH + 2 + (size_t)S * RT) * sizeof(double);
    if (lds > 150 * 1024) { set_error("logsoftmax_gather_bwd_f64: S=%d too large for LDS staging", S); return DSP_EINVAL; }
    const long ntiles = (long)B * ((L + RT - 1) / RT);
    const int grid = (int)(ntiles < 4096 ? ntiles : 4096);
    auto k = lsg64_bwd_kernel<LAZY>;
    if (lds > 48 * 1024) set_max_dynamic_lds((const void*)k, (int)lds);
    hipLaunchKernelGGL(k, dim3(grid), dim3(256), lds, st, sm, idx, isb, isj, iss, g, gsb, gsj, gss, B, L, V, S, RT, CH, stats);
    return check_launch("logsoftmax_gather_bwd_f64");
}

}  // namespace dsp

extern "C" int dsp_logsoftmax_gather_f64(double* logits, const int64_t* idx, int64_t idx_sb, int64_t idx_sj, int64_t idx_ss,
                                         double* match, int64_t out_sb, int64_t out_sj, int64_t out_ss, double* row_stats,
                                         int B, int L, int V, int S, int write_softmax, dsp_stream_t stream)
{
    using namespace dsp;
    if (B < 0 || L < 0 || V <= 0 || S < 0) { set_error("logsoftmax_gather_f64: bad sizes B=%d L=%d V=%d S=%d", B, L, V, S); return DSP_EINVAL; }
    if (write_softmax && row_stats) { set_error("logsoftmax_gather_f64: write_softmax and row_stats are exclusive (the lazy form leaves the logits untouched)"); return DSP_EINVAL; }
    if (B == 0 || L == 0) return DSP_OK;
    if (!logits || (S > 0 && (!idx || !match))) { set_error("logsoftmax_gather_f64: null pointer"); return DSP_EINVAL; }
    if ((uintptr_t)logits % 8 || (uintptr_t)match % 8 || (uintptr_t)row_stats % 8) { set_error("logsoftmax_gather_f64: pointers must be 8-byte aligned"); return DSP_EINVAL; }
    return launch_fwd64(logits, idx, idx_sb, idx_sj, idx_ss, match, out_sb, out_sj, out_ss, B, L, V, S, write_softmax ? 1 : 0, as_stream(stream), row_stats);
}

extern "C" int dsp_logsoftmax_gather_bwd_f64(double* inout, const int64_t* idx, int64_t idx_sb, int64_t idx_sj, int64_t idx_ss,
                                             const double* g, int64_t g_sb, int64_t g_sj, int64_t g_ss, const double* row_stats,
                                             int B, int L, int V, int S, dsp_stream_t stream)
{
    using namespace dsp;
    if (B < 0 || L < 0 || V <= 0 || S < 0) { set_error("logsoftmax_gather_bwd_f64: bad sizes B=%d L=%d V=%d S=%d", B, L, V, S); return DSP_EINVAL; }
    if (B == 0 || L == 0) return DSP_OK;
    if (!inout || (S > 0 && (!idx || !g))) { set_error("logsoftmax_gather_bwd_f64: null pointer"); return DSP_EINVAL; }
    if ((uintptr_t)inout % 8 || (uintptr_t)g % 8 || (uintptr_t)row_stats % 8) { set_error("logsoftmax_gather_bwd_f64: pointers must be 8-byte aligned"); return DSP_EINVAL; }
    hipStream_t st = as_stream(stream);
    if (row_stats) return launch_bwd64<true>(inout, idx, idx_sb, idx_sj, idx_ss, g, g_sb, g_sj, g_ss, B, L, V, S, st, row_stats);
    return launch_bwd64<false>(inout, idx, idx_sb, idx_sj, idx_ss, g, g_sb, g_sj, g_ss, B, L, V, S, st, nullptr);
}
