// path_features_train.hip — the argmax strategy's features_on_path under autograd, gfx950 (wave64 throughout): a stable compaction of the
// feature rows of the vertices on the path (include/daspeech_decode.h: dsp_path_features_fwd / _bwd).
//     on[b,j]  = path[b,j] >= 0 && (j > 0 || !skip_first)            n[b] = min(sum_j on[b,j], W)
//     out[b,r,:] = features[b, j_r, :]  for r < n[b], j_r the r-th vertex with `on` set in ascending j;   exact zeros for r >= n[b]
//     pad[b,r] = r >= n[b]
//     dfeatures[b,j,:] = dy[b,r,:] where j = j_r for some r < n[b], else exact zeros
// Only the sign of a path value is read: no value is an index, so no path content leads to an access outside a tensor.
//
// Forward, one launch: a workgroup of four waves owns PF_TILE_W consecutive output rows of one sample.  Its waves take the sample's path row
// in chunks of 64 vertices, one __ballot and one __popcll each (kept in LDS); wave 0 turns the chunk counts into an exclusive prefix by
// wave scans of 64 counts; then every flagged lane has its rank (prefix + lanes_before) and the ones whose rank falls into the tile write
// their vertex into the tile's source list.  Each workgroup rescans the row — L * 8 bytes, L2-resident — instead of a first launch that
// would write the ranks out.  Then a wave moves a row: source row or zeros, 16 bytes per lane.
// Backward, one launch: a workgroup owns PF_TILE_L consecutive vertices of one sample (tile_positions of row_compact.h: the flagged
// vertices before the tile by one strided pass, the tile's own flags as one ballot), and a wave writes each of its rows of dfeatures: the
// dy row of the vertex's rank, or zeros.  Every element of dfeatures is written exactly once: no memset, no atomics.
//
// Rows move as raw 16-byte quads (the uint4 form elem_io.h names for a kernel with a move of its own kind): a copy widens and rounds
// nothing, so the kernels exist once for the three dtypes and the bits of a row, NaN payloads included, are those of its source.
//
// Algorithmic HBM bytes (es: element size): forward B * (L * 8 + 2 * W * C * es + W + 8), backward B * (L * 8 + (n + L) * C * es) —
// a few MB at the training shapes: the bound is the launch latency.  The tile sizes are read off the shapes (B = 32, W = 64: 256
// forward workgroups; L = 400: 800 backward workgroups), not measured.
#include "common.h"
#include "host_gates.h"
#include "row_compact.h"
#include "../../include/daspeech_decode.h"

namespace dsp {

constexpr int PF_TILE_W = DSP_PATH_FEATURES_TILE_W;        // output rows of one sample per forward workgroup: 4 waves x 2 rows
constexpr int PF_TILE_L = DSP_PATH_FEATURES_TILE_L;        // vertices of one sample per backward workgroup: 4 waves x 4 rows
constexpr int PF_MAX_L = DSP_PATH_FEATURES_MAX_L;
constexpr int PF_MAX_CHUNKS = PF_MAX_L / 64;               // ballots and counts of one path row in LDS: 12 KiB
static_assert(PF_TILE_W % 4 == 0 && PF_TILE_L % 4 == 0 && PF_TILE_L <= 32 && PF_MAX_L % 64 == 0, "four waves share a tile");

// path [B,L] through its two strides (elements), int64 or int32
struct PfPath {
    const void* p; long sb, sc; int is64, skip_first;
    __device__ __forceinline__ bool on(int b, int j) const
    {
        const size_t at = (size_t)b * (size_t)sb + (size_t)j * (size_t)sc;
        const bool nonneg = is64 ? ((const int64_t*)p)[at] >= 0 : ((const int32_t*)p)[at] >= 0;
        return nonneg && (j > 0 || !skip_first);
    }
};

// a wave moves one row of Q quads: src, or zeros when src is null (wave-uniform)
__device__ __forceinline__ void pf_move_row(uint4* __restrict__ dst, const uint4* __restrict__ src, int Q, int lane)
{
    if (src) { for (int q = lane; q < Q; q += 64) dst[q] = src[q]; }
    else { for (int q = lane; q < Q; q += 64) dst[q] = make_uint4(0u, 0u, 0u, 0u); }
}

__global__ __launch_bounds__(256) void pf_fwd_kernel(const uint4* __restrict__ feat, long ld_q, PfPath path, uint4* __restrict__ out,
                                                     unsigned char* __restrict__ pad, int64_t* __restrict__ n_out, int L, int W, int Q,
                                                     int tiles)
{
    __shared__ unsigned long long bal[PF_MAX_CHUNKS];
    __shared__ int pre[PF_MAX_CHUNKS];
    __shared__ int src[PF_TILE_W];
    __shared__ int total_s;
    const int b = (int)(blockIdx.x / (unsigned)tiles), r0 = (int)(blockIdx.x % (unsigned)tiles) * PF_TILE_W;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nchunks = (L + 63) >> 6;
    for (int k = wave; k < nchunks; k += 4) {                              // wave-uniform trip count: every lane takes part in the ballot
        const int j = k * 64 + lane;
        const unsigned long long m = __ballot(j < L && path.on(b, j));
        if (lane == 0) { bal[k] = m; pre[k] = __popcll(m); }
    }
    __syncthreads();
    if (wave == 0) {                                                       // exclusive prefix over the chunk counts, 64 at a time
        int carry = 0;
        for (int base = 0; base < nchunks; base += 64) {
            const int k = base + lane;
            const int v = k < nchunks ? pre[k] : 0;
            int inc = v;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int u = __shfl_up(inc, d, 64);
                if (lane >= d) inc += u;
            }
            if (k < nchunks) pre[k] = carry + inc - v;
            carry += __shfl(inc, 63, 64);
        }
        if (lane == 0) total_s = carry;
    }
    __syncthreads();
    const int n = total_s < W ? total_s : W;
    const int r1 = r0 + PF_TILE_W < n ? r0 + PF_TILE_W : n;                // the tile's rows with a source: [r0, r1)
    for (int k = wave; k < nchunks; k += 4) {
        if (pre[k] >= r1) break;                                           // wave-uniform; the prefix never decreases
        const unsigned long long m = bal[k];
        const int rank = pre[k] + lanes_before(m, lane);
        if (((m >> lane) & 1ull) && rank >= r0 && rank < r1) src[rank - r0] = k * 64 + lane;       // each rank of [r0, r1) exactly once
    }
    __syncthreads();
    if ((int)threadIdx.x < PF_TILE_W && r0 + (int)threadIdx.x < W) pad[(size_t)b * (size_t)W + r0 + threadIdx.x] = r0 + (int)threadIdx.x >= n;
    if (r0 == 0 && threadIdx.x == 0) n_out[b] = n;
#pragma unroll 1
    for (int i = wave; i < PF_TILE_W; i += 4) {
        const int r = r0 + i;
        if (r >= W) break;                                                 // wave-uniform
        const uint4* s = r < n ? feat + ((size_t)b * (size_t)L + (size_t)src[i]) * (size_t)ld_q : (const uint4*)nullptr;
        pf_move_row(out + ((size_t)b * (size_t)W + (size_t)r) * (size_t)Q, s, Q, lane);
    }
}

__global__ __launch_bounds__(256) void pf_bwd_kernel(const uint4* __restrict__ dy, long sb_q, long sr_q, PfPath path, uint4* __restrict__ dfeat,
                                                     int L, int W, int Q, int tiles)
{
    const int b = (int)(blockIdx.x / (unsigned)tiles), t0 = (int)(blockIdx.x % (unsigned)tiles) * PF_TILE_L;
    int before; unsigned flags;
    tile_positions<PF_TILE_L>([&](int t) { return path.on(b, t); }, t0, L, before, flags);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll 1
    for (int j = 0; j < PF_TILE_L / 4; ++j) {
        const int i = wave * (PF_TILE_L / 4) + j, t = t0 + i;
        if (t >= L) break;                                                 // wave-uniform
        const int rank = before + __popc(flags & ((1u << i) - 1u));        // flagged vertices before t
        const bool has = ((flags >> i) & 1u) && rank < W;                  // the surplus beyond W has no row of dy
        const uint4* s = has ? dy + (size_t)b * (size_t)sb_q + (size_t)rank * (size_t)sr_q : (const uint4*)nullptr;
        pf_move_row(dfeat + ((size_t)b * (size_t)L + (size_t)t) * (size_t)Q, s, Q, lane);
    }
}

static int pf_check(const char* who, int dtype, int B, int L, int W, int C, const void* path, long path_sb, long path_sc, int path64)
{
    const int es = elem_size(dtype);
    if (!es) { set_error("%s: unsupported dtype code %d", who, dtype); return DSP_EINVAL; }
    const int VE = 16 / es;
    if (B < 0 || L < 1 || L > PF_MAX_L || W < 0 || C < VE || (C % VE) || (int64_t)B * L > (1LL << 24) || (int64_t)B * W > (1LL << 24) ||
        (int64_t)C * es > (1LL << 24)) {
        set_error("%s: bad sizes B=%d L=%d W=%d C=%d (1 <= L <= %d, W >= 0, C a multiple of %d, B*L and B*W at most 2^24)", who, B, L, W, C,
                  PF_MAX_L, VE);
        return DSP_EINVAL;
    }
    if (!path || path_sb < 0 || path_sc < 0 || ((uintptr_t)path & (path64 ? 7 : 3))) {
        set_error("%s: path must be non-null, on the grid of its element type, with non-negative strides", who);
        return DSP_EINVAL;
    }
    return 0;
}

}  // namespace dsp

using namespace dsp;

extern "C" int dsp_path_features_fwd(const void* features, long ld_f, const void* path, long path_sb, long path_sc, int path64, int skip_first,
                                     void* out, unsigned char* pad, int64_t* n, int dtype, int B, int L, int W, int C, dsp_stream_t stream)
{
    const char* who = "path_features_fwd";
    const int rc = pf_check(who, dtype, B, L, W, C, path, path_sb, path_sc, path64);
    if (rc) return rc;
    if (B == 0 || W == 0) return DSP_OK;                                   // nothing to write (W == 0: n would be zeros, left to the caller)
    const int VE = 16 / elem_size(dtype);
    if (ld_f < C || (ld_f % VE)) { set_error("%s: row pitch %ld (>= C, a multiple of %d)", who, ld_f, VE); return DSP_EINVAL; }
    if (!features || !out || !pad || !n || out == features) { set_error("%s: null or aliased pointer", who); return DSP_EINVAL; }
    if (!on16(features, out) || (((uintptr_t)n) & 7)) {
        set_error("%s: features and out must be 16-byte aligned, n 8-byte", who); return DSP_EINVAL;
    }
    const int tiles = (W + PF_TILE_W - 1) / PF_TILE_W;
    const PfPath pp{path, path_sb, path_sc, path64, skip_first};
    hipLaunchKernelGGL(pf_fwd_kernel, dim3((unsigned)B * (unsigned)tiles), dim3(256), 0, as_stream(stream), (const uint4*)features,
                       ld_f / VE, pp, (uint4*)out, pad, n, L, W, C / VE, tiles);
    return check_launch(who);
}

extern "C" int dsp_path_features_bwd(const void* dy, long dy_sb, long dy_sr, const void* path, long path_sb, long path_sc, int path64,
                                     int skip_first, void* dfeatures, int dtype, int B, int L, int W, int C, dsp_stream_t stream)
{
    const char* who = "path_features_bwd";
    const int rc = pf_check(who, dtype, B, L, W, C, path, path_sb, path_sc, path64);
    if (rc) return rc;
    if (B == 0) return DSP_OK;
    const int VE = 16 / elem_size(dtype);
    if (!dfeatures || !on16(dfeatures) || dfeatures == dy) { set_error("%s: dfeatures must be non-null, 16-byte aligned, not dy", who); return DSP_EINVAL; }
    if (W > 0 && (!dy || !on16(dy) || dy_sb < 0 || dy_sr < 0 || (dy_sb % VE) || (dy_sr % VE))) {
        set_error("%s: dy must be non-null and 16-byte aligned, its batch and row strides %ld, %ld non-negative multiples of %d", who, dy_sb,
                  dy_sr, VE);
        return DSP_EINVAL;
    }
    const int tiles = (L + PF_TILE_L - 1) / PF_TILE_L;
    const PfPath pp{path, path_sb, path_sc, path64, skip_first};
    hipLaunchKernelGGL(pf_bwd_kernel, dim3((unsigned)B * (unsigned)tiles), dim3(256), 0, as_stream(stream), (const uint4*)dy, dy_sb / VE,
                       dy_sr / VE, pp, (uint4*)dfeatures, L, W, C / VE, tiles);
    return check_launch(who);
}
