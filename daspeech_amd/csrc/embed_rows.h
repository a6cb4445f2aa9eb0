// embed_rows.h — "per-destination sum of gradient rows in a fixed order", the device code shared by the table gradients of
// tts_glue_grad.hip (dsp_embed_grad) and embed_entry_train.hip (dsp_embed_entry_bwd): a wave adds the rows of a list in list order in fp32
// and rounds once; a destination's list is cut into chunks of DSP_EMBED_GRAD_CHUNK rows, one wave each (embed_chunk_sum_kernel), and the
// destination's chunk sums are added in chunk order.  How the lists (counts, offs, cstart, perm) come about is the business of the caller.
#pragma once
#include "common.h"
#include "host_gates.h"
#include "../../include/daspeech_decode.h"

namespace dsp {

constexpr int EG_CHUNK = DSP_EMBED_GRAD_CHUNK;        // rows of one bucket that one wave sums
constexpr int GG_MAX_WG = 1024;                       // 4 waves each: a launch serves at most 4096 rows per trip of its grid-stride loop

static inline bool aligned16(const void* a, const void* b, size_t row_a, size_t row_b)
{
    return on16(a, b) && ((row_a | row_b) & 15) == 0;
}

static inline unsigned wave_grid(long waves) { const long g = (waves + 3) / 4; return (unsigned)(g < 1 ? 1 : (g > GG_MAX_WG ? GG_MAX_WG : g)); }

// dst[0..C) = sum over i in [0, m) of src[row(i), 0..C) — one wave, list order, fp32 accumulation, one rounding to TO; m == 0 writes zeros.
// Four rows are in flight at a time; the adds stay in list order.  SCALED: the fp32 sum times `scale` before the rounding.
template <typename TI, typename TO, bool SCALED = false, typename RowFn>
__device__ __forceinline__ void wave_sum_rows(const TI* __restrict__ src, TO* __restrict__ dst, int C, bool vec, int lane, long m, RowFn row,
                                              float scale = 1.f)
{
    constexpr int V = 16 / (int)(sizeof(TI) < sizeof(TO) ? sizeof(TI) : sizeof(TO));
    if (vec) {
        for (int c = lane * V; c < C; c += 64 * V) {
            float acc[V];
#pragma unroll
            for (int j = 0; j < V; ++j) acc[j] = 0.f;
            long i = 0;
            for (; i + 4 <= m; i += 4) {
                float f0[V], f1[V], f2[V], f3[V];
                load_f<TI, V>(src + row(i) * C + c, f0);
                load_f<TI, V>(src + row(i + 1) * C + c, f1);
                load_f<TI, V>(src + row(i + 2) * C + c, f2);
                load_f<TI, V>(src + row(i + 3) * C + c, f3);
#pragma unroll
                for (int j = 0; j < V; ++j) acc[j] = (((acc[j] + f0[j]) + f1[j]) + f2[j]) + f3[j];
            }
            for (; i < m; ++i) {
                float f0[V];
                load_f<TI, V>(src + row(i) * C + c, f0);
#pragma unroll
                for (int j = 0; j < V; ++j) acc[j] += f0[j];
            }
            if constexpr (SCALED) {
#pragma unroll
                for (int j = 0; j < V; ++j) acc[j] *= scale;
            }
            store_f<TO, V>(dst + c, acc);
        }
    } else {
        for (int c = lane; c < C; c += 64) {
            float acc = 0.f;
            for (long i = 0; i < m; ++i) acc += to_f(src[row(i) * C + c]);
            if constexpr (SCALED) acc *= scale;
            dst[c] = from_f<TO>(acc);
        }
    }
}

// one wave per chunk of EG_CHUNK list entries: partial[w,:] = sum of the chunk's gradient rows in list order (fp32).  counts / offs [K]:
// rows and list start of a bucket; cstart [K + 1]: first chunk of a bucket (cstart[K]: all chunks); perm: the lists, rows ascending.
template <typename T>
__global__ __launch_bounds__(256) void embed_chunk_sum_kernel(const T* __restrict__ g, const int32_t* __restrict__ counts,
                                                              const int32_t* __restrict__ offs, const int32_t* __restrict__ cstart,
                                                              const int32_t* __restrict__ perm, float* __restrict__ partial,
                                                              int K, int C, long max_chunks, bool vec)
{
    const int lane = threadIdx.x & 63;
    long total = cstart[K];
    if (total > max_chunks) total = max_chunks;             // cannot happen (sum of ceil(count / chunk) <= n / chunk + K); keeps the writes in
    for (long w = (long)blockIdx.x * 4 + (threadIdx.x >> 6); w < total; w += (long)gridDim.x * 4) {
        int lo = 0, hi = K - 1;                             // the last bucket whose first chunk is <= w: the one that owns chunk w
        while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (cstart[mid] <= w) lo = mid; else hi = mid - 1; }
        const int j = (int)(w - cstart[lo]);
        const int base = offs[lo] + j * EG_CHUNK;
        int m = counts[lo] - j * EG_CHUNK;
        m = m < 0 ? 0 : (m > EG_CHUNK ? EG_CHUNK : m);
        const int32_t* list = perm + base;
        wave_sum_rows<T, float>(g, partial + (size_t)w * C, C, vec, lane, m, [&](long i) { return (size_t)list[i]; });
    }
}

// the chunks [c0, c1) of one bucket in chunk order, clamped to the partials that exist: what the per-bucket reduce of either file adds
__device__ __forceinline__ void chunk_range(const int32_t* __restrict__ cstart, int k, long max_chunks, long& c0, long& c1)
{
    c0 = cstart[k]; c1 = cstart[k + 1];
    if (c1 > max_chunks) c1 = max_chunks;
    if (c0 > c1) c0 = c1;
}

}  // namespace dsp
