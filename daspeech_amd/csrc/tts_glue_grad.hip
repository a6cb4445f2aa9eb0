// tts_glue_grad.hip — the variance-adaptor glue under autograd, gfx950: an out-of-place bucketize + embedding add in the model's dtype that
// keeps its bucket indices, the gradient of the embedding table, and the gradient of the length regulator (fastspeech2.py:98-114,169-210).
// Both gradients are sums of gradient rows that share a destination.  They are written as "inverted index + per-destination sum in a fixed
// order": every destination row is owned by one wave, which adds its source rows in ascending order in fp32 and rounds once.  No float
// atomics and no hand-off between workgroups inside a launch, so the bits do not depend on how the grid is scheduled.
//
// All of it is HBM-/latency-bound row traffic: 16-byte accesses per lane when the rows and pointers allow it, a scalar path otherwise.
#include "common.h"
#include "embed_rows.h"          // wave_sum_rows, embed_chunk_sum_kernel, chunk_range: shared with embed_entry_train.hip
#include "../../include/daspeech_decode.h"

namespace dsp {

// ---------------------------------------------------------------- F6b': out = x + emb[bucketize(v)], idx kept; one wave per row
template <typename T>
__global__ __launch_bounds__(256) void bucketize_embed_add_fwd_kernel(const T* __restrict__ x, const float* __restrict__ v,
                                                                      const float* __restrict__ bins, int nb, const T* __restrict__ emb,
                                                                      T* __restrict__ out, int32_t* __restrict__ idx, long n, int C, bool vec)
{
    constexpr int V = 16 / (int)sizeof(T);
    const int lane = threadIdx.x & 63;
    for (long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6); r < n; r += (long)gridDim.x * 4) {
        const float val = v[r];
        int lo = 0, hi = nb;                          // first index with bins[idx] >= val  (right=False)
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (bins[mid] >= val) hi = mid; else lo = mid + 1; }
        if (lane == 0) idx[r] = lo;
        const T* e = emb + (size_t)lo * C;
        const T* xr = x + (size_t)r * C;
        T* o = out + (size_t)r * C;
        if (vec) {
            for (int c = lane * V; c < C; c += 64 * V) {
                float a[V], b[V];
                load_f<T, V>(xr + c, a);
                load_f<T, V>(e + c, b);
#pragma unroll
                for (int j = 0; j < V; ++j) a[j] += b[j];
                store_f<T, V>(o + c, a);
            }
        } else {
            for (int c = lane; c < C; c += 64) o[c] = from_f<T>(to_f(xr[c]) + to_f(e[c]));
        }
    }
}

// ---------------------------------------------------------------- table gradient, step 1: rows per bucket (one wave per bucket)
__global__ __launch_bounds__(256) void embed_count_kernel(const int32_t* __restrict__ idx, long n, int K, int32_t* __restrict__ counts)
{
    const int lane = threadIdx.x & 63;
    for (int k = blockIdx.x * 4 + (threadIdx.x >> 6); k < K; k += gridDim.x * 4) {
        int c = 0;
        for (long r = lane; r < n; r += 64) c += (idx[r] == k);
        c = wave_sum(c);
        if (lane == 0) counts[k] = c;
    }
}

// step 2: the inverted index.  Bucket k's wave finds where its list and its chunks start (integer prefix sums over the buckets before
// it) and writes its rows to perm in ascending order: ballot + prefix popcount over 64 rows at a time.
__global__ __launch_bounds__(256) void embed_index_kernel(const int32_t* __restrict__ idx, long n, int K, const int32_t* __restrict__ counts,
                                                          int32_t* __restrict__ offs, int32_t* __restrict__ cstart, int32_t* __restrict__ perm)
{
    const int lane = threadIdx.x & 63;
    for (int k = blockIdx.x * 4 + (threadIdx.x >> 6); k < K; k += gridDim.x * 4) {
        int o = 0, cs = 0;
        for (int j = lane; j < k; j += 64) { const int c = counts[j]; o += c; cs += (c + EG_CHUNK - 1) / EG_CHUNK; }
        o = wave_sum(o); cs = wave_sum(cs);
        if (lane == 0) {
            offs[k] = o; cstart[k] = cs;
            if (k == K - 1) cstart[K] = cs + (counts[k] + EG_CHUNK - 1) / EG_CHUNK;
        }
        int pos = o;
        for (long r0 = 0; r0 < n; r0 += 64) {               // wave-uniform trip count: every lane takes part in the ballot
            const long r = r0 + lane;
            const bool hit = r < n && idx[r] == k;
            const unsigned long long b = __ballot(hit);
            if (hit) perm[pos + __popcll(b & ((1ull << lane) - 1ull))] = (int32_t)r;
            pos += __popcll(b);
        }
    }
}

// step 3: embed_chunk_sum_kernel (embed_rows.h): one wave per chunk of EG_CHUNK list entries, partial[w,:] = the chunk's rows in list order

// step 4: one wave per bucket: its chunk sums in chunk order, one rounding to the table's dtype; no rows: zeros
template <typename T>
__global__ __launch_bounds__(256) void embed_reduce_kernel(const float* __restrict__ partial, const int32_t* __restrict__ cstart,
                                                           T* __restrict__ out, int K, int C, long max_chunks, bool vec)
{
    const int lane = threadIdx.x & 63;
    for (int k = blockIdx.x * 4 + (threadIdx.x >> 6); k < K; k += gridDim.x * 4) {
        long c0, c1;
        chunk_range(cstart, k, max_chunks, c0, c1);
        wave_sum_rows<float, T>(partial, out + (size_t)k * C, C, vec, lane, c1 - c0, [&](long i) { return (size_t)(c0 + i); });
    }
}

// ---------------------------------------------------------------- F7': grad_x[b,t,:] = sum of grad_out[b, cum[t-1] .. cum[t]-1, :]; one wave per row
template <typename T>
__global__ __launch_bounds__(256) void lr_bwd_kernel(const T* __restrict__ g, const int64_t* __restrict__ cum, T* __restrict__ gx,
                                                     long rows, int N, int C, int maxlen, bool vec)
{
    const int lane = threadIdx.x & 63;
    for (long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += (long)gridDim.x * 4) {
        const long b = r / N;
        long s = (r % N) ? (long)cum[r - 1] : 0, e = (long)cum[r];
        s = s < 0 ? 0 : (s > maxlen ? maxlen : s);          // the frames of a sample end at cum[b,N-1] <= maxlen: nothing beyond is read
        e = e < s ? s : (e > maxlen ? maxlen : e);
        const T* gb = g + (size_t)b * maxlen * C;
        wave_sum_rows<T, T>(gb, gx + (size_t)r * C, C, vec, lane, e - s, [&](long i) { return (size_t)(s + i); });
    }
}

static size_t eg_int_bytes(int64_t n, int K) { return a16(((size_t)3 * K + 1 + (size_t)n) * sizeof(int32_t)); }
static long eg_max_chunks(int64_t n, int K) { return (long)((n + EG_CHUNK - 1) / EG_CHUNK) + K; }

}  // namespace dsp

using namespace dsp;

#define GG_DISPATCH(dtype, CALL) DSP_DISPATCH_ELEM(dtype, T, CALL)

extern "C" int dsp_bucketize_embed_add_fwd(const void* x, int dtype, const float* v, const float* bins, int nb, const void* emb,
                                           void* out, int32_t* idx, int64_t n, int C, dsp_stream_t stream)
{
    const int es = elem_size(dtype);
    if (!es) { set_error("bucketize_embed_add_fwd: unsupported dtype %d", dtype); return DSP_EINVAL; }
    if (n < 0 || nb < 0 || C < 1) { set_error("bucketize_embed_add_fwd: bad sizes"); return DSP_EINVAL; }
    if (n == 0) return DSP_OK;
    if (!x || !v || (nb && !bins) || !emb || !out || !idx) { set_error("bucketize_embed_add_fwd: null pointer"); return DSP_EINVAL; }
    const bool vec = aligned16(x, out, (size_t)C * es, 0) && aligned16(emb, nullptr, 0, 0);
    hipStream_t st = as_stream(stream);
    GG_DISPATCH(dtype, hipLaunchKernelGGL(bucketize_embed_add_fwd_kernel<T>, dim3(wave_grid((long)n)), dim3(256), 0, st, (const T*)x, v, bins, nb,
                                          (const T*)emb, (T*)out, idx, (long)n, C, vec));
    return check_launch("bucketize_embed_add_fwd");
}

extern "C" size_t dsp_embed_grad_workspace_bytes(int64_t n, int nb, int C)
{
    if (n <= 0 || nb < 0 || C < 1) return 0;
    return eg_int_bytes(n, nb + 1) + (size_t)eg_max_chunks(n, nb + 1) * C * sizeof(float);
}

extern "C" int dsp_embed_grad(const void* grad_out, int dtype, const int32_t* idx, void* grad_emb, int64_t n, int nb, int C,
                              void* workspace, size_t workspace_bytes, dsp_stream_t stream)
{
    const int es = elem_size(dtype);
    if (!es) { set_error("embed_grad: unsupported dtype %d", dtype); return DSP_EINVAL; }
    if (n < 0 || n > 0x7fffffffLL || nb < 0 || C < 1) { set_error("embed_grad: bad sizes"); return DSP_EINVAL; }
    if (!grad_emb) { set_error("embed_grad: null pointer"); return DSP_EINVAL; }
    const int K = nb + 1;
    hipStream_t st = as_stream(stream);
    if (n == 0) {                                          // no rows: the whole table is zero
        const hipError_t e = hipMemsetAsync(grad_emb, 0, (size_t)K * C * es, st);
        if (e != hipSuccess) { set_error("embed_grad: %s", hipGetErrorString(e)); return (int)e; }
        return DSP_OK;
    }
    if (!grad_out || !idx) { set_error("embed_grad: null pointer"); return DSP_EINVAL; }
    if (!workspace || !on16(workspace) || workspace_bytes < dsp_embed_grad_workspace_bytes(n, nb, C)) {
        set_error("embed_grad: workspace of %zu bytes (16-byte aligned) needed, see dsp_embed_grad_workspace_bytes", dsp_embed_grad_workspace_bytes(n, nb, C));
        return workspace && on16(workspace) ? DSP_ENOSPC : DSP_EINVAL;
    }
    int32_t* counts = (int32_t*)workspace;
    int32_t* offs = counts + K;
    int32_t* cstart = offs + K;                            // [K + 1]
    int32_t* perm = cstart + K + 1;                        // [n]
    float* partial = (float*)((char*)workspace + eg_int_bytes(n, K));
    const long max_chunks = eg_max_chunks(n, K);
    const bool vec_in = aligned16(grad_out, partial, (size_t)C * es, (size_t)C * 4);
    const bool vec_out = aligned16(partial, grad_emb, (size_t)C * 4, (size_t)C * es);
    hipLaunchKernelGGL(embed_count_kernel, dim3(wave_grid(K)), dim3(256), 0, st, idx, (long)n, K, counts);
    hipLaunchKernelGGL(embed_index_kernel, dim3(wave_grid(K)), dim3(256), 0, st, idx, (long)n, K, counts, offs, cstart, perm);
    GG_DISPATCH(dtype, hipLaunchKernelGGL(embed_chunk_sum_kernel<T>, dim3(wave_grid(max_chunks)), dim3(256), 0, st, (const T*)grad_out, counts, offs,
                                          cstart, perm, partial, K, C, max_chunks, vec_in));
    GG_DISPATCH(dtype, hipLaunchKernelGGL(embed_reduce_kernel<T>, dim3(wave_grid(K)), dim3(256), 0, st, partial, cstart, (T*)grad_emb, K, C,
                                          max_chunks, vec_out));
    return check_launch("embed_grad");
}

extern "C" int dsp_length_regulator_bwd(const void* grad_out, int dtype, const int64_t* cum, void* grad_x, int B, int N, int C, int maxlen,
                                        dsp_stream_t stream)
{
    const int es = elem_size(dtype);
    if (!es || B < 0 || N < 0 || C < 1 || maxlen < 0) { set_error("length_regulator_bwd: bad arguments"); return DSP_EINVAL; }
    if (B == 0 || N == 0) return DSP_OK;
    if (!cum || !grad_x || (maxlen && !grad_out)) { set_error("length_regulator_bwd: null pointer"); return DSP_EINVAL; }
    const long rows = (long)B * N;
    const bool vec = aligned16(grad_out, grad_x, (size_t)C * es, 0);
    GG_DISPATCH(dtype, hipLaunchKernelGGL(lr_bwd_kernel<T>, dim3(wave_grid(rows)), dim3(256), 0, as_stream(stream), (const T*)grad_out, cum,
                                          (T*)grad_x, rows, N, C, maxlen, vec));
    return check_launch("length_regulator_bwd");
}
