// partial_merge.h — the last step of a gradient that was summed as fp32 partials: "add the partials of an element in ASCENDING order, round
// once".  The partials are a [n_parts][n] matrix, element e of part s at part[s * n + e]; the order of addition is part of the operators'
// contract (the same inputs give the same bits on every call), so both forms add s = 0, 1, 2, ... and nothing else.
//
//   merge_plain         one thread walks its element's column itself.  Right for a handful of parts (row splits, samples).
//   merge_column_tiled  for many parts (act_dropout: one per 32 rows; resnorm keeps its own copy): a thread adding n_parts values it loads itself is a
//                       chain of n_parts load latencies (0.45 ms at 1600 chunks), so the loads are taken off the chain — all 256 threads
//                       of the workgroup bring a tile of MT parts x 64 columns into LDS (MT / 4 independent loads each, rows of 256
//                       bytes), then thread (tx, ty == 0) adds its column's MT values in ascending order: the same sum, in the same
//                       order, as the plain loop.  Workgroups of 256 threads owning 64 columns; every thread of the workgroup must call.
// A site's kernel is one of the two and its own store (a dtype code, a transposed layout, a choice between outputs).
#pragma once
#include "common.h"

namespace dsp {

template <typename N>
__device__ __forceinline__ float merge_plain(const float* part, N n_parts, size_t n, size_t e)
{
    float acc = 0.f;
    for (N s = 0; s < n_parts; ++s) acc += part[(size_t)s * n + e];
    return acc;
}

// the sum of column e (< n, or nothing is loaded) in thread ty == 0 of the column; the other threads return 0
template <int MT>
__device__ __forceinline__ float merge_column_tiled(const float* part, long n_parts, int n, int e)
{
    __shared__ float tile[MT][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    float acc = 0.f;
#pragma unroll 1
    for (long k0 = 0; k0 < n_parts; k0 += MT) {
        float r[MT / 4];
#pragma unroll
        for (int j = 0; j < MT / 4; ++j) {
            const long k = k0 + ty + 4 * j;
            r[j] = (k < n_parts && e < n) ? part[(size_t)k * n + e] : 0.f;
        }
        __syncthreads();                                                   // the tile before this one has been added
#pragma unroll
        for (int j = 0; j < MT / 4; ++j) tile[ty + 4 * j][tx] = r[j];
        __syncthreads();
        if (ty == 0) {
            const int m = (int)(n_parts - k0 < MT ? n_parts - k0 : MT);
            for (int k = 0; k < m; ++k) acc += tile[k][tx];
        }
    }
    return acc;
}

// out[e] = the merged element, rounded to E: the tail of a gradient kept in the data dtype and the layout of its partials
template <typename E>
__global__ __launch_bounds__(256) void merge_store_kernel(const float* __restrict__ part, int n_parts, long n, E* __restrict__ out)
{
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    out[e] = from_f<E>(merge_plain(part, n_parts, (size_t)n, (size_t)e));
}

}  // namespace dsp
