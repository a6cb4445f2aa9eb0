// embed_entry_train.hip — the input embeddings of the decoder and of the TTS half under autograd, gfx950 (wave64 throughout):
//     token entry       y[b,t,:] = m * (embed_scale * E[tok[b,t]] + P[pos[b,t]]),  pos = pad + keep * cumsum(keep),  keep = tok != pad
//     positional add    y[b,t,:] = m * (x[b,t,:] + alpha * tab[pos[b,t]]),         pos = min(pad + keep * cumsum(keep), NT - 1),  keep = !mask
// with m the Philox keep flag of philox.h times keep_scale on the element index of the contiguous y (thr == 0: no mask path), fp32
// arithmetic, one rounding, and their backward passes (include/daspeech_decode.h: dsp_embed_entry_fwd / _bwd, dsp_pos_add_fwd / _bwd).
//
// Forward, one launch each: a workgroup of four waves owns EE_TILE = 16 consecutive positions of one sample.  Its 256 threads count the kept
// elements BEFORE the tile (tile_positions of row_compact.h: one strided pass over the row's prefix, one LDS exchange), every wave takes the
// keep flags of the tile itself as one ballot, and a row's position is that count plus a prefix popcount: left padding, interior pads and
// all-pad rows need nothing else.
// Then each wave moves four rows with 16-byte accesses.  tok32 (-1: a token outside [0, V), which contributes a zero row) and pos32 are kept
// for the backward.
//
// Token entry, backward.  g = dy * m is written ONCE as fp32 [n, C] when thr != 0 (with thr == 0 the sums read dy itself): both table
// gradients read it, and drawing the mask again inside two sums would cost the Philox rounds twice.  dE and dP are ONE problem: 2n list
// entries (entry r: key tok32[r]; entry n + r: key V + pos32[r]) over K = V + NP keys; entries of row `pad` of either table and of
// out-of-range tokens are left out, which is what makes their gradient rows exact zeros.  The inverted index:
//     1. counts[key] by integer atomic adds, one per distinct key of a wave's 64 entries (the result does not depend on order);
//     2. one exclusive scan over the K counts by one workgroup: list starts, chunk starts, and the list of keys with more than
//        DSP_EMBED_ENTRY_SORT_MAX rows;
//     3. keys with at most DSP_EMBED_ENTRY_SORT_MAX rows: every entry takes a slot of its key's list by an integer atomic (any order), then
//        the key's wave sorts the list ascending (rank sort, one value per lane).  Keys with more rows (at most 2n / 65 of them): one
//        workgroup per key, whose 16 waves each own a span of the entries, count their hits, and write them by ballot + prefix popcount
//        (embed_index_kernel's compaction, ascending by construction);
//     4. the chunk sums and the per-key reduce of embed_rows.h (shared with dsp_embed_grad): rows added in ascending r, chunks of
//        DSP_EMBED_GRAD_CHUNK rows, chunk sums in chunk order, embed_scale applied in fp32 before the one rounding.
// Cost bound: steps 1 and 3 touch each entry O(1) times, except that a key above the threshold re-reads all 2n keys (8n bytes, L2-resident)
// — at most 2n / 65 such keys, in the training pattern one or two; step 2 is O(K); step 4 reads every g row twice (once per table).  Nothing
// grows as V * n / 64.  No float atomics, no hand-off between workgroups: the bits do not depend on the grid's schedule, and one gradient
// alone has the bits it has next to the other (the keys of the table left out simply have no entries).
//
// Positional add, backward: dx = dy * m and, per chunk of DSP_POS_ADD_CHUNK_ROWS rows, one wave's partial of sum g * tab[pos] (a lane adds
// its columns over the chunk's rows in row order, then a butterfly over the lanes); a one-workgroup tail adds the partials in index order
// and rounds once to alpha's dtype.  dalpha is ONE number out of n * C products of either sign: with fp32 accumulators its error is an ulp of
// the partial sums, which are far larger than the result.  So a lane accumulates in double, and a partial is written as TWO fp32 values
// (head and tail of the double); the tail kernel adds them in double.
//
// Algorithmic HBM bytes (es: element size, n = B * L rows, tokens 8 bytes each):
//     dsp_embed_entry_fwd   n * (8 + 3 * C * es + 8)        tokens, an E row, a P row, a y row, tok32 + pos32 (the prefix re-reads hit L2)
//     dsp_embed_entry_bwd   n * C * (es + 4) [thr != 0]  +  2 * n * C * 4 (or es)  +  2 * chunks * C * 4  +  (V + NP) * C * es  +  O(n + K) ints
//     dsp_pos_add_fwd       n * (1 + 2 * C * es + C * ts + 4)     mask, x, y, a table row (L2: NT rows), pos32
//     dsp_pos_add_bwd       n * (2 * C * es [dx] + C * ts [dalpha] + 4)
// All of it is row traffic at a few MB per call: the bound is these bytes plus the launch latencies.
#include "common.h"
#include "host_gates.h"
#include "philox.h"
#include "embed_rows.h"
#include "row_compact.h"
#include "../../include/daspeech_decode.h"

namespace dsp {

constexpr int EE_TILE = 16;                                // positions of one sample per forward workgroup: 4 waves x 4 rows
constexpr int EE_SORT_MAX = DSP_EMBED_ENTRY_SORT_MAX;
constexpr int EE_MAX_C = DSP_EMBED_ENTRY_MAX_C;
constexpr int PA_CHUNK = DSP_POS_ADD_CHUNK_ROWS;
static_assert(EE_SORT_MAX <= 64, "a key's wave sorts one value per lane");

// ---------------------------------------------------------------- token entry, forward
template <typename T>
__global__ __launch_bounds__(256) void ee_fwd_kernel(const int64_t* __restrict__ tokens, long ld_tok, const T* __restrict__ E,
                                                     const T* __restrict__ P, int64_t pad, float embed_scale, float keep_scale, uint32_t thr,
                                                     uint64_t seed, uint64_t offset, const uint64_t* __restrict__ rng_state, T* __restrict__ y,
                                                     int32_t* __restrict__ tok32, int32_t* __restrict__ pos32, int L, int V, int NP, int C, int tiles)
{
    constexpr int VE = elems16<T>;
    philox_stream(seed, offset, rng_state);
    const int b = (int)(blockIdx.x / (unsigned)tiles), t0 = (int)(blockIdx.x % (unsigned)tiles) * EE_TILE;
    const int64_t* row = tokens + (size_t)b * (size_t)ld_tok;
    int before; unsigned flags;
    tile_positions<EE_TILE>([&](int t) { return row[t] != pad; }, t0, L, before, flags);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll 1
    for (int j = 0; j < EE_TILE / 4; ++j) {
        const int i = wave * (EE_TILE / 4) + j, t = t0 + i;
        if (t >= L) break;                                                 // wave-uniform
        const int64_t tk = row[t];
        const bool keep = (flags >> i) & 1u;
        long pos = (long)pad + (keep ? (long)(before + __popc(flags & ((2u << i) - 1u))) : 0L);
        pos = pos < 0 ? 0 : (pos > NP - 1 ? NP - 1 : pos);                 // the caller keeps L + pad + 1 <= NP; nothing outside P is read
        const bool inside = tk >= 0 && tk < (int64_t)V;
        const size_t r = (size_t)b * (size_t)L + (size_t)t;
        if (lane == 0) { tok32[r] = inside ? (int32_t)tk : -1; pos32[r] = (int32_t)pos; }
        const T* e = E + (size_t)(inside ? tk : 0) * (size_t)C;
        const T* p = P + (size_t)pos * (size_t)C;
        for (int c = lane * VE; c < C; c += 64 * VE) {
            float fe[VE], fp[VE];
            load_f<T, VE>(e + c, fe);
            load_f<T, VE>(p + c, fp);
#pragma unroll
            for (int q = 0; q < VE; ++q) fe[q] = inside ? embed_scale * fe[q] + fp[q] : fp[q];
            const size_t at = r * (size_t)C + c;
            if (thr) {
                bool k[VE];
                keep_flags<VE>((uint64_t)at, seed, offset, thr, k);
#pragma unroll
                for (int q = 0; q < VE; ++q) fe[q] = k[q] ? fe[q] * keep_scale : 0.f;
            }
            store_f<T, VE>(y + at, fe);
        }
    }
}

// ---------------------------------------------------------------- g = dy * m as fp32 (thr != 0 only)
template <typename T, typename TO>
__global__ __launch_bounds__(256) void ee_mask_kernel(const T* __restrict__ dy, TO* __restrict__ g, long groups, float keep_scale, uint32_t thr,
                                                      uint64_t seed, uint64_t offset, const uint64_t* __restrict__ rng_state)
{
    constexpr int VE = elems16<T>;
    philox_stream(seed, offset, rng_state);
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < groups; q += (long)gridDim.x * 256) {
        float f[VE]; bool k[VE];
        load_f<T, VE>(dy + q * VE, f);
        keep_flags<VE>((uint64_t)(q * VE), seed, offset, thr, k);
#pragma unroll
        for (int i = 0; i < VE; ++i) f[i] = k[i] ? f[i] * keep_scale : 0.f;
        store_f<TO, VE>(g + q * VE, f);
    }
}

// ---------------------------------------------------------------- the inverted index
// key of list entry e in [0, 2n): the token half then the position half; -1: the entry is left out (row `pad`, an out-of-range token)
struct EeKeys {
    const int32_t* tok32; const int32_t* pos32; int n, V, NP, pad;
    __device__ __forceinline__ int key(int e) const
    {
        if (e < n) { const int k = tok32[e]; return (k < 0 || k >= V || k == pad) ? -1 : k; }
        const int q = pos32[e - n];
        return (q < 0 || q >= NP || q == pad) ? -1 : V + q;
    }
    __device__ __forceinline__ int row(int e) const { return e < n ? e : e - n; }
};

// step 0: counts and cursor to zero — a kernel, not a memset: as a node of a captured graph the launch is ordered with the kernels around it
// exactly as on the stream, and everything below trusts these 2K integers (a stale cursor leaves list slots unwritten, and a list entry is a
// row index that embed_chunk_sum_kernel reads through)
__global__ __launch_bounds__(256) void ee_zero_kernel(int32_t* __restrict__ p, long n)
{
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) p[i] = 0;
}

// step 1: counts.  A wave adds once per distinct key of its 64 entries (the training pattern has one key in nearly all of them).
__global__ __launch_bounds__(256) void ee_count_kernel(EeKeys ks, int e0, int e1, int32_t* __restrict__ counts)
{
    const int lane = threadIdx.x & 63;
    for (long base = (long)e0 + ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64; base < e1; base += (long)gridDim.x * 256) {
        const long e = base + lane;
        const int k = e < e1 ? ks.key((int)e) : -1;
        unsigned long long todo = __ballot(k >= 0);
        while (todo) {                                                     // wave-uniform
            const int leader = __ffsll((long long)todo) - 1;
            const int kl = __shfl(k, leader, 64);
            const unsigned long long same = __ballot(k == kl);
            if (lane == leader) atomicAdd(&counts[kl], __popcll(same));
            todo &= ~same;
        }
    }
}

// step 2: one workgroup of 1024.  offs / cstart: exclusive sums of the counts / of their chunk numbers; big: the keys above EE_SORT_MAX,
// ascending, nbig of them (at most max_big: there cannot be more)
__global__ __launch_bounds__(1024) void ee_scan_kernel(const int32_t* __restrict__ counts, int K, int32_t* __restrict__ offs,
                                                       int32_t* __restrict__ cstart, int32_t* __restrict__ big, int32_t* __restrict__ nbig,
                                                       int max_big)
{
    __shared__ int wo[16], wc[16], wb[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int per = (K + 1023) / 1024;
    const int k0 = tid * per < K ? tid * per : K, k1 = k0 + per < K ? k0 + per : K;
    int so = 0, sc = 0, sb = 0;
    for (int k = k0; k < k1; ++k) { const int c = counts[k]; so += c; sc += (c + EG_CHUNK - 1) / EG_CHUNK; sb += c > EE_SORT_MAX; }
    int io = so, ic = sc, ib = sb;                                         // inclusive scan over the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int uo = __shfl_up(io, d, 64), uc = __shfl_up(ic, d, 64), ub = __shfl_up(ib, d, 64);
        if (lane >= d) { io += uo; ic += uc; ib += ub; }
    }
    if (lane == 63) { wo[wave] = io; wc[wave] = ic; wb[wave] = ib; }
    __syncthreads();
    int o = io - so, c = ic - sc, bi = ib - sb;
    for (int w = 0; w < wave; ++w) { o += wo[w]; c += wc[w]; bi += wb[w]; }
    for (int k = k0; k < k1; ++k) {
        const int n = counts[k];
        offs[k] = o; cstart[k] = c;
        if (n > EE_SORT_MAX) { if (bi < max_big) big[bi] = k; ++bi; }
        o += n; c += (n + EG_CHUNK - 1) / EG_CHUNK;
    }
    if (tid == 1023) { cstart[K] = c; *nbig = bi < max_big ? bi : max_big; }
}

// step 3a: the entries of the keys up to EE_SORT_MAX rows take a slot of their list, in any order
__global__ __launch_bounds__(256) void ee_scatter_kernel(EeKeys ks, int e0, int e1, const int32_t* __restrict__ counts,
                                                         const int32_t* __restrict__ offs, int32_t* __restrict__ cursor,
                                                         int32_t* __restrict__ perm)
{
    for (long e = (long)e0 + (long)blockIdx.x * 256 + threadIdx.x; e < e1; e += (long)gridDim.x * 256) {
        const int k = ks.key((int)e);
        if (k < 0) continue;
        const int c = counts[k];
        if (c > EE_SORT_MAX) continue;
        const int slot = atomicAdd(&cursor[k], 1);
        if (slot < c) perm[offs[k] + slot] = ks.row((int)e);               // always: c counted these very entries
    }
}

// step 3b: workgroups [0, big_wgs): one key above EE_SORT_MAX at a time, its list written ascending; the others: 16 keys each, a wave sorts
// the list of a key with 2 .. EE_SORT_MAX rows
__global__ __launch_bounds__(1024) void ee_order_kernel(EeKeys ks, int e0, int e1, int K, const int32_t* __restrict__ counts,
                                                        const int32_t* __restrict__ offs, const int32_t* __restrict__ big,
                                                        const int32_t* __restrict__ nbig, int32_t* __restrict__ perm, int big_wgs)
{
    __shared__ int wcnt[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if ((int)blockIdx.x < big_wgs) {
        const int nb = *nbig;
        const long E = (long)e1 - e0;
        const long span = ((E + 15) / 16 + 63) / 64 * 64;                  // entries per wave, whole groups of 64
        const long lo = e0 + wave * span, hi = lo + span < e1 ? lo + span : e1;
        for (int j = blockIdx.x; j < nb; j += big_wgs) {                   // workgroup-uniform
            const int k = big[j];
            int c = 0;
            for (long e = lo + lane; e < hi; e += 64) c += ks.key((int)e) == k;
            c = wave_sum(c);
            __syncthreads();                                               // the previous key's counts have been read
            if (lane == 0) wcnt[wave] = c;
            __syncthreads();
            int at = offs[k];
            for (int w = 0; w < wave; ++w) at += wcnt[w];
            const int end = offs[k] + counts[k];
            for (long e = lo; e < hi; e += 64) {                           // wave-uniform trip count: every lane takes part in the ballot
                const long me = e + lane;
                const bool hit = me < hi && ks.key((int)me) == k;
                const unsigned long long bal = __ballot(hit);
                const int dst = at + lanes_before(bal, lane);
                if (hit && dst < end) perm[dst] = ks.row((int)me);
                at += __popcll(bal);
            }
        }
        return;
    }
    const int k = ((int)blockIdx.x - big_wgs) * 16 + wave;
    if (k >= K) return;
    const int c = counts[k];
    if (c < 2 || c > EE_SORT_MAX) return;
    int32_t* list = perm + offs[k];
    const int v = lane < c ? list[lane] : 0x7fffffff;
    int rank = 0;
    for (int j = 0; j < c; ++j) rank += __shfl(v, j, 64) < v;              // the rows of a list are distinct
    if (lane < c) list[rank] = v;
}

// step 4b: one wave per key: its chunk sums in chunk order, times embed_scale for a row of dE, one rounding; no rows: zeros
template <typename T>
__global__ __launch_bounds__(256) void ee_reduce_kernel(const float* __restrict__ partial, const int32_t* __restrict__ cstart,
                                                        T* __restrict__ dE, T* __restrict__ dP, int V, int K, int C, long max_chunks,
                                                        float embed_scale)
{
    const int lane = threadIdx.x & 63;
    const int kb = dE ? 0 : V, ke = dP ? K : V;
    for (int k = kb + blockIdx.x * 4 + (threadIdx.x >> 6); k < ke; k += gridDim.x * 4) {
        long c0, c1;
        chunk_range(cstart, k, max_chunks, c0, c1);
        T* out = k < V ? dE + (size_t)k * C : dP + (size_t)(k - V) * C;
        wave_sum_rows<float, T, true>(partial, out, C, true, lane, c1 - c0, [&](long i) { return (size_t)(c0 + i); },
                                      k < V ? embed_scale : 1.f);
    }
}

// ---------------------------------------------------------------- positional add, forward
template <typename T>
__global__ __launch_bounds__(256) void pa_fwd_kernel(const T* __restrict__ x, long ld_x, const unsigned char* __restrict__ mask,
                                                     const void* __restrict__ tab, int tab_dtype, const void* __restrict__ alpha,
                                                     int alpha_dtype, int pad, float keep_scale, uint32_t thr, uint64_t seed, uint64_t offset,
                                                     const uint64_t* __restrict__ rng_state, T* __restrict__ y, int32_t* __restrict__ pos32, int N,
                                                     int NT, int C, int tiles)
{
    constexpr int VE = elems16<T>;
    philox_stream(seed, offset, rng_state);
    const int b = (int)(blockIdx.x / (unsigned)tiles), t0 = (int)(blockIdx.x % (unsigned)tiles) * EE_TILE;
    const unsigned char* row = mask + (size_t)b * (size_t)N;
    int before; unsigned flags;
    tile_positions<EE_TILE>([&](int t) { return row[t] == 0; }, t0, N, before, flags);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float a = param_load(alpha, alpha_dtype, 0);
#pragma unroll 1
    for (int j = 0; j < EE_TILE / 4; ++j) {
        const int i = wave * (EE_TILE / 4) + j, t = t0 + i;
        if (t >= N) break;                                                 // wave-uniform
        const bool keep = (flags >> i) & 1u;
        int pos = pad + (keep ? before + __popc(flags & ((2u << i) - 1u)) : 0);
        pos = pos > NT - 1 ? NT - 1 : pos;
        const size_t r = (size_t)b * (size_t)N + (size_t)t;
        if (lane == 0) pos32[r] = pos;
        const T* xr = x + r * (size_t)ld_x;
        for (int c = lane * VE; c < C; c += 64 * VE) {
            float fx[VE], ft[VE];
            load_f<T, VE>(xr + c, fx);
            param_load_f<T, VE>(tab, tab_dtype, pos * C + c, ft);
#pragma unroll
            for (int q = 0; q < VE; ++q) fx[q] = fx[q] + a * ft[q];
            const size_t at = r * (size_t)C + c;
            if (thr) {
                bool k[VE];
                keep_flags<VE>((uint64_t)at, seed, offset, thr, k);
#pragma unroll
                for (int q = 0; q < VE; ++q) fx[q] = k[q] ? fx[q] * keep_scale : 0.f;
            }
            store_f<T, VE>(y + at, fx);
        }
    }
}

// ---------------------------------------------------------------- positional add, backward: dx, and one partial of dalpha per chunk of rows
template <typename T>
__global__ __launch_bounds__(64) void pa_bwd_kernel(const T* __restrict__ dy, const void* __restrict__ tab, int tab_dtype,
                                                    const int32_t* __restrict__ pos32, float keep_scale, uint32_t thr, uint64_t seed,
                                                    uint64_t offset, const uint64_t* __restrict__ rng_state, T* __restrict__ dx,
                                                    float* __restrict__ part, long R, int NT, int C)
{
    constexpr int VE = elems16<T>;
    philox_stream(seed, offset, rng_state);
    const int lane = threadIdx.x;
    const long r0 = (long)blockIdx.x * PA_CHUNK, r1 = r0 + PA_CHUNK < R ? r0 + PA_CHUNK : R;
    double acc = 0.0;
    for (long r = r0; r < r1; ++r) {
        int pos = part ? pos32[r] : 0;
        pos = pos < 0 ? 0 : (pos > NT - 1 ? NT - 1 : pos);
        for (int c = lane * VE; c < C; c += 64 * VE) {
            const size_t at = (size_t)r * (size_t)C + c;
            float g[VE];
            load_f<T, VE>(dy + at, g);
            if (thr) {
                bool k[VE];
                keep_flags<VE>((uint64_t)at, seed, offset, thr, k);
#pragma unroll
                for (int q = 0; q < VE; ++q) g[q] = k[q] ? g[q] * keep_scale : 0.f;
                if (dx) store_f<T, VE>(dx + at, g);
            }
            if (part) {
                float ft[VE];
                param_load_f<T, VE>(tab, tab_dtype, pos * C + c, ft);
#pragma unroll
                for (int q = 0; q < VE; ++q) acc = fma((double)g[q], (double)ft[q], acc);
            }
        }
    }
    if (!part) return;                                                     // kernel-uniform
    acc = wave_sum(acc);
    if (lane == 0) {
        const float head = (float)acc;
        part[2 * (size_t)blockIdx.x] = head;
        part[2 * (size_t)blockIdx.x + 1] = (float)(acc - (double)head);
    }
}

// the tail: one workgroup; 256 partials (head + tail) at a time come into LDS, one thread adds them in index order
__global__ __launch_bounds__(256) void pa_dalpha_kernel(const float* __restrict__ part, long nchunks, void* __restrict__ dalpha, int alpha_dtype)
{
    __shared__ double tile[256];
    double acc = 0.0;
    for (long k0 = 0; k0 < nchunks; k0 += 256) {
        const long k = k0 + threadIdx.x;
        const double v = k < nchunks ? (double)part[2 * k] + (double)part[2 * k + 1] : 0.0;
        __syncthreads();                                                   // the tile before this one has been added
        tile[threadIdx.x] = v;
        __syncthreads();
        if (threadIdx.x == 0) {
            const int m = (int)(nchunks - k0 < 256 ? nchunks - k0 : 256);
            for (int i = 0; i < m; ++i) acc += tile[i];
        }
    }
    if (threadIdx.x == 0) param_store(dalpha, alpha_dtype, 0, (float)acc);
}

static long ee_max_big(int64_t n) { return (long)(2 * n / (EE_SORT_MAX + 1)) + 1; }
static long ee_max_chunks(int64_t n, int K) { return (long)((2 * n + EG_CHUNK - 1) / EG_CHUNK) + (K < 2 * n ? K : 2 * n); }
// ints of the index: counts [K], cursor [K], offs [K], cstart [K + 1], nbig [1], big [max_big], perm [2n]
static size_t ee_int_bytes(int64_t n, int K) { return a16(((size_t)4 * K + 2 + (size_t)ee_max_big(n) + (size_t)2 * n) * sizeof(int32_t)); }

static int ee_check(const char* who, int dtype, int64_t n, int V, int NP, int C, int64_t pad, unsigned int thr)
{
    const int es = elem_size(dtype);
    if (!es) { set_error("%s: unsupported dtype code %d", who, dtype); return DSP_EINVAL; }
    const int VE = 16 / es;
    if (n < 0 || n > (1LL << 24) || V < 1 || NP < 1 || (long)V + NP > 0x7fffffffL || C < VE || (C % VE) || C > EE_MAX_C || pad < 0 || pad >= NP) {
        set_error("%s: bad sizes n=%lld V=%d NP=%d C=%d pad=%lld (n <= 2^24, C a multiple of %d, C <= %d, 0 <= pad < NP)", who, (long long)n, V, NP,
                  C, (long long)pad, VE, EE_MAX_C);
        return DSP_EINVAL;
    }
    if (thr > (1u << 24)) { set_error("%s: thr %u above 2^24", who, thr); return DSP_EINVAL; }
    return n == 0 ? 1 : 0;
}

static int pa_check(const char* who, int act_dtype, int tab_dtype, int alpha_dtype, int64_t R, int NT, int C, unsigned int thr)
{
    const int es = elem_size(act_dtype);
    if (!es || (tab_dtype != act_dtype && tab_dtype != DSP_F32) || (alpha_dtype != act_dtype && alpha_dtype != DSP_F32)) {
        set_error("%s: dtype codes %d (x, y and their gradients) / %d (table) / %d (alpha): the same, or fp32", who, act_dtype, tab_dtype,
                  alpha_dtype);
        return DSP_EINVAL;
    }
    const int VE = 16 / es;
    if (R < 0 || R > (1LL << 24) || NT < 1 || C < VE || (C % VE) || C > EE_MAX_C || (long)NT * C > 0x7fffffffL) {
        set_error("%s: bad sizes R=%lld NT=%d C=%d (R <= 2^24, C a multiple of %d, C <= %d)", who, (long long)R, NT, C, VE, EE_MAX_C);
        return DSP_EINVAL;
    }
    if (thr > (1u << 24)) { set_error("%s: thr %u above 2^24", who, thr); return DSP_EINVAL; }
    return R == 0 ? 1 : 0;
}

}  // namespace dsp

using namespace dsp;

static int ee_fwd(const char* who, const int64_t* tokens, long ld_tok, const void* E, const void* P, int64_t pad, float embed_scale,
                  float keep_scale, unsigned int thr, uint64_t seed, uint64_t offset, const uint64_t* rng_state, void* y, int32_t* tok32,
                  int32_t* pos32, int dtype, int B, int L, int V, int NP, int C, dsp_stream_t stream)
{
    DSP_GATE(rng_state_gate(who, rng_state));
    if (B < 0 || L < 0) { set_error("%s: bad sizes B=%d L=%d", who, B, L); return DSP_EINVAL; }
    const int rc = ee_check(who, dtype, (int64_t)B * L, V, NP, C, pad, thr);
    if (rc) return rc < 0 ? rc : DSP_OK;
    if (ld_tok < L) { set_error("%s: token row stride %ld below L=%d", who, ld_tok, L); return DSP_EINVAL; }
    if (!tokens || !E || !P || !y || !tok32 || !pos32 || y == E || y == P) { set_error("%s: null or aliased pointer", who); return DSP_EINVAL; }
    if (!on16(E, P, y) || (((uintptr_t)tokens) & 7) || ((((uintptr_t)tok32) | ((uintptr_t)pos32)) & 3)) {
        set_error("%s: tables and y must be 16-byte aligned, tokens 8-byte", who); return DSP_EINVAL;
    }
    const int tiles = (L + EE_TILE - 1) / EE_TILE;
    DSP_DISPATCH_ELEM(dtype, T, hipLaunchKernelGGL(ee_fwd_kernel<T>, dim3((unsigned)B * (unsigned)tiles), dim3(256), 0, as_stream(stream), tokens,
                                                   ld_tok, (const T*)E, (const T*)P, pad, embed_scale, keep_scale, (uint32_t)thr, seed, offset,
                                                   rng_state, (T*)y, tok32, pos32, L, V, NP, C, tiles));
    return check_launch(who);
}

extern "C" int dsp_embed_entry_fwd(const int64_t* tokens, long ld_tok, const void* E, const void* P, int64_t pad, float embed_scale,
                                   float keep_scale, unsigned int thr, uint64_t seed, uint64_t offset, void* y, int32_t* tok32, int32_t* pos32,
                                   int dtype, int B, int L, int V, int NP, int C, dsp_stream_t stream)
{
    return ee_fwd("embed_entry_fwd", tokens, ld_tok, E, P, pad, embed_scale, keep_scale, thr, seed, offset, nullptr, y, tok32, pos32, dtype, B, L, V,
                  NP, C, stream);
}

extern "C" int dsp_embed_entry_fwd_state(const int64_t* tokens, long ld_tok, const void* E, const void* P, int64_t pad, float embed_scale,
                                         float keep_scale, unsigned int thr, uint64_t seed, uint64_t offset, void* y, int32_t* tok32,
                                         int32_t* pos32, int dtype, int B, int L, int V, int NP, int C, const uint64_t* rng_state,
                                         dsp_stream_t stream)
{
    return ee_fwd("embed_entry_fwd_state", tokens, ld_tok, E, P, pad, embed_scale, keep_scale, thr, seed, offset, rng_state, y, tok32, pos32, dtype,
                  B, L, V, NP, C, stream);
}

extern "C" size_t dsp_embed_entry_bwd_workspace_bytes(int64_t n, int V, int NP, int C, unsigned int thr)
{
    if (n <= 0 || V < 1 || NP < 1 || C < 1) return 0;
    const int K = V + NP;
    return ee_int_bytes(n, K) + (thr ? a16((size_t)n * C * sizeof(float)) : 0) + a16((size_t)ee_max_chunks(n, K) * C * sizeof(float));
}

static int ee_bwd(const char* who, const void* dy, const int32_t* tok32, const int32_t* pos32, int64_t pad, float embed_scale, float keep_scale,
                  unsigned int thr, uint64_t seed, uint64_t offset, const uint64_t* rng_state, void* dE, void* dP, void* workspace,
                  size_t workspace_bytes, int dtype, int64_t n, int V, int NP, int C, dsp_stream_t stream)
{
    DSP_GATE(rng_state_gate(who, rng_state));
    const int rc = ee_check(who, dtype, n, V, NP, C, pad, thr);
    if (rc < 0) return rc;
    if (!dE && !dP) return DSP_OK;
    if (!on16(dy, dE, dP) || (dE && dE == dP) || (dy && (dy == dE || dy == dP))) {
        set_error("%s: gradients must be 16-byte aligned and distinct", who); return DSP_EINVAL;
    }
    const int es = elem_size(dtype);
    hipStream_t st = as_stream(stream);
    if (rc == 1) {                                                         // no rows: both tables are zero
        hipError_t e = dE ? hipMemsetAsync(dE, 0, (size_t)V * C * es, st) : hipSuccess;
        if (e == hipSuccess && dP) e = hipMemsetAsync(dP, 0, (size_t)NP * C * es, st);
        if (e != hipSuccess) { set_error("%s: %s", who, hipGetErrorString(e)); return (int)e; }
        return DSP_OK;
    }
    if (!dy || !tok32 || !pos32) { set_error("%s: null pointer", who); return DSP_EINVAL; }
    const size_t need = dsp_embed_entry_bwd_workspace_bytes(n, V, NP, C, thr);
    if (!workspace || !on16(workspace) || workspace_bytes < need) {
        set_error("%s: workspace of %zu bytes (16-byte aligned) needed, see dsp_embed_entry_bwd_workspace_bytes", who, need);
        return workspace && on16(workspace) ? DSP_ENOSPC : DSP_EINVAL;
    }
    const int K = V + NP, N = (int)n;
    const long max_big = ee_max_big(n), max_chunks = ee_max_chunks(n, K);
    int32_t* counts = (int32_t*)workspace;
    int32_t* cursor = counts + K;
    int32_t* offs = cursor + K;
    int32_t* cstart = offs + K;                                            // [K + 1]
    int32_t* nbig = cstart + K + 1;
    int32_t* big = nbig + 1;                                               // [max_big]
    int32_t* perm = big + max_big;                                         // [2n]
    char* fl = (char*)workspace + ee_int_bytes(n, K);
    float* g32 = thr ? (float*)fl : nullptr;
    float* partial = (float*)(fl + (thr ? a16((size_t)n * C * sizeof(float)) : 0));
    const int e0 = dE ? 0 : N, e1 = dP ? 2 * N : N;                        // the entries of a table that is not asked for do not exist
    const EeKeys ks{tok32, pos32, N, V, NP, (int)pad};
    hipLaunchKernelGGL(ee_zero_kernel, dim3(wave_grid(((long)2 * K + 63) / 64)), dim3(256), 0, st, counts, (long)2 * K);      // counts and cursor
    if (thr) {
        const long groups = (long)n * C * es / 16;
        const unsigned grid = (unsigned)((groups + 255) / 256 > 4096 ? 4096 : (groups + 255) / 256);
        DSP_DISPATCH_ELEM(dtype, T, hipLaunchKernelGGL((ee_mask_kernel<T, float>), dim3(grid), dim3(256), 0, st, (const T*)dy, g32, groups,
                                                       keep_scale, (uint32_t)thr, seed, offset, rng_state));
    }
    const long E = (long)e1 - e0;
    hipLaunchKernelGGL(ee_count_kernel, dim3(wave_grid((E + 63) / 64)), dim3(256), 0, st, ks, e0, e1, counts);
    hipLaunchKernelGGL(ee_scan_kernel, dim3(1), dim3(1024), 0, st, counts, K, offs, cstart, big, nbig, (int)max_big);
    hipLaunchKernelGGL(ee_scatter_kernel, dim3(wave_grid((E + 63) / 64)), dim3(256), 0, st, ks, e0, e1, counts, offs, cursor, perm);
    const int big_wgs = (int)(max_big < 32 ? max_big : 32);
    hipLaunchKernelGGL(ee_order_kernel, dim3((unsigned)(big_wgs + (K + 15) / 16)), dim3(1024), 0, st, ks, e0, e1, K, counts, offs, big, nbig, perm,
                       big_wgs);
    if (thr) {
        hipLaunchKernelGGL(embed_chunk_sum_kernel<float>, dim3(wave_grid(max_chunks)), dim3(256), 0, st, (const float*)g32, counts, offs, cstart,
                           perm, partial, K, C, max_chunks, true);
    } else {
        DSP_DISPATCH_ELEM(dtype, T, hipLaunchKernelGGL(embed_chunk_sum_kernel<T>, dim3(wave_grid(max_chunks)), dim3(256), 0, st, (const T*)dy, counts,
                                                       offs, cstart, perm, partial, K, C, max_chunks, true));
    }
    DSP_DISPATCH_ELEM(dtype, T, hipLaunchKernelGGL(ee_reduce_kernel<T>, dim3(wave_grid(K)), dim3(256), 0, st, partial, cstart, (T*)dE, (T*)dP, V, K, C,
                                                   max_chunks, embed_scale));
    return check_launch(who);
}

extern "C" int dsp_embed_entry_bwd(const void* dy, const int32_t* tok32, const int32_t* pos32, int64_t pad, float embed_scale, float keep_scale,
                                   unsigned int thr, uint64_t seed, uint64_t offset, void* dE, void* dP, void* workspace,
                                   size_t workspace_bytes, int dtype, int64_t n, int V, int NP, int C, dsp_stream_t stream)
{
    return ee_bwd("embed_entry_bwd", dy, tok32, pos32, pad, embed_scale, keep_scale, thr, seed, offset, nullptr, dE, dP, workspace, workspace_bytes,
                  dtype, n, V, NP, C, stream);
}

extern "C" int dsp_embed_entry_bwd_state(const void* dy, const int32_t* tok32, const int32_t* pos32, int64_t pad, float embed_scale,
                                         float keep_scale, unsigned int thr, uint64_t seed, uint64_t offset, void* dE, void* dP, void* workspace,
                                         size_t workspace_bytes, int dtype, int64_t n, int V, int NP, int C, const uint64_t* rng_state,
                                         dsp_stream_t stream)
{
    return ee_bwd("embed_entry_bwd_state", dy, tok32, pos32, pad, embed_scale, keep_scale, thr, seed, offset, rng_state, dE, dP, workspace,
                  workspace_bytes, dtype, n, V, NP, C, stream);
}

static int pa_fwd(const char* who, const void* x, long ld_x, const unsigned char* padding_mask, const void* tab, const void* alpha, int pad,
                  float keep_scale, unsigned int thr, uint64_t seed, uint64_t offset, const uint64_t* rng_state, void* y, int32_t* pos32,
                  int act_dtype, int tab_dtype, int alpha_dtype, int B, int N, int NT, int C, dsp_stream_t stream)
{
    DSP_GATE(rng_state_gate(who, rng_state));
    if (B < 0 || N < 0 || pad < 0) { set_error("%s: bad sizes B=%d N=%d pad=%d", who, B, N, pad); return DSP_EINVAL; }
    const int rc = pa_check(who, act_dtype, tab_dtype, alpha_dtype, (int64_t)B * N, NT, C, thr);
    if (rc) return rc < 0 ? rc : DSP_OK;
    const int VE = 16 / elem_size(act_dtype);
    if (ld_x < C || (ld_x % VE)) { set_error("%s: row pitch %ld (>= C, a multiple of %d)", who, ld_x, VE); return DSP_EINVAL; }
    if (!x || !padding_mask || !tab || !alpha || !y || !pos32 || y == x || y == tab) { set_error("%s: null or aliased pointer", who); return DSP_EINVAL; }
    if (!on16(x, tab, y)) { set_error("%s: x, the table and y must be 16-byte aligned", who); return DSP_EINVAL; }
    const int tiles = (N + EE_TILE - 1) / EE_TILE;
    DSP_DISPATCH_ELEM(act_dtype, T, hipLaunchKernelGGL(pa_fwd_kernel<T>, dim3((unsigned)B * (unsigned)tiles), dim3(256), 0, as_stream(stream),
                                                       (const T*)x, ld_x, padding_mask, tab, tab_dtype, alpha, alpha_dtype, pad, keep_scale,
                                                       (uint32_t)thr, seed, offset, rng_state, (T*)y, pos32, N, NT, C, tiles));
    return check_launch(who);
}

extern "C" int dsp_pos_add_fwd(const void* x, long ld_x, const unsigned char* padding_mask, const void* tab, const void* alpha, int pad,
                               float keep_scale, unsigned int thr, uint64_t seed, uint64_t offset, void* y, int32_t* pos32, int act_dtype,
                               int tab_dtype, int alpha_dtype, int B, int N, int NT, int C, dsp_stream_t stream)
{
    return pa_fwd("pos_add_fwd", x, ld_x, padding_mask, tab, alpha, pad, keep_scale, thr, seed, offset, nullptr, y, pos32, act_dtype, tab_dtype,
                  alpha_dtype, B, N, NT, C, stream);
}

extern "C" int dsp_pos_add_fwd_state(const void* x, long ld_x, const unsigned char* padding_mask, const void* tab, const void* alpha, int pad,
                                     float keep_scale, unsigned int thr, uint64_t seed, uint64_t offset, void* y, int32_t* pos32, int act_dtype,
                                     int tab_dtype, int alpha_dtype, int B, int N, int NT, int C, const uint64_t* rng_state, dsp_stream_t stream)
{
    return pa_fwd("pos_add_fwd_state", x, ld_x, padding_mask, tab, alpha, pad, keep_scale, thr, seed, offset, rng_state, y, pos32, act_dtype,
                  tab_dtype, alpha_dtype, B, N, NT, C, stream);
}

extern "C" size_t dsp_pos_add_bwd_workspace_bytes(int64_t R)
{
    if (R <= 0) return 0;
    return a16((size_t)((R + PA_CHUNK - 1) / PA_CHUNK) * 2 * sizeof(float));
}

static int pa_bwd(const char* who, const void* dy, const void* tab, const int32_t* pos32, float keep_scale, unsigned int thr, uint64_t seed,
                  uint64_t offset, const uint64_t* rng_state, void* dx, void* dalpha, void* workspace, size_t workspace_bytes, int act_dtype,
                  int tab_dtype, int alpha_dtype, int64_t R, int NT, int C, dsp_stream_t stream)
{
    DSP_GATE(rng_state_gate(who, rng_state));
    const int rc = pa_check(who, act_dtype, tab_dtype, alpha_dtype, R, NT, C, thr);
    if (rc < 0) return rc;
    if (!dx && !dalpha) return DSP_OK;
    hipStream_t st = as_stream(stream);
    if (rc == 1) {                                                         // no rows: the empty sum
        if (dalpha) {
            const hipError_t e = hipMemsetAsync(dalpha, 0, (size_t)elem_size(alpha_dtype), st);
            if (e != hipSuccess) { set_error("%s: %s", who, hipGetErrorString(e)); return (int)e; }
        }
        return DSP_OK;
    }
    if (!dy || (dalpha && (!tab || !pos32)) || dx == dy) { set_error("%s: null or aliased pointer", who); return DSP_EINVAL; }
    if (!on16(dy, tab, dx)) { set_error("%s: dy, the table and dx must be 16-byte aligned", who); return DSP_EINVAL; }
    if (dalpha) DSP_GATE(workspace_gate(who, workspace, workspace_bytes, dsp_pos_add_bwd_workspace_bytes(R), "dsp_pos_add_bwd_workspace_bytes"));
    const long nchunks = (long)((R + PA_CHUNK - 1) / PA_CHUNK);
    float* part = dalpha ? (float*)workspace : (float*)nullptr;
    if (dx && !thr) {                                                      // dx = dy: a caller that can hand dy on passes dx = NULL
        const hipError_t e = hipMemcpyAsync(dx, dy, (size_t)R * C * elem_size(act_dtype), hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) { set_error("%s: %s", who, hipGetErrorString(e)); return (int)e; }
        if (!dalpha) return DSP_OK;
    }
    DSP_DISPATCH_ELEM(act_dtype, T, hipLaunchKernelGGL(pa_bwd_kernel<T>, dim3((unsigned)nchunks), dim3(64), 0, st, (const T*)dy, tab, tab_dtype, pos32,
                                                       keep_scale, (uint32_t)thr, seed, offset, rng_state, (T*)dx, part, (long)R, NT, C));
    if (dalpha) hipLaunchKernelGGL(pa_dalpha_kernel, dim3(1), dim3(256), 0, st, (const float*)part, nchunks, dalpha, alpha_dtype);
    return check_launch(who);
}

extern "C" int dsp_pos_add_bwd(const void* dy, const void* tab, const int32_t* pos32, float keep_scale, unsigned int thr, uint64_t seed,
                               uint64_t offset, void* dx, void* dalpha, void* workspace, size_t workspace_bytes, int act_dtype, int tab_dtype,
                               int alpha_dtype, int64_t R, int NT, int C, dsp_stream_t stream)
{
    return pa_bwd("pos_add_bwd", dy, tab, pos32, keep_scale, thr, seed, offset, nullptr, dx, dalpha, workspace, workspace_bytes, act_dtype,
                  tab_dtype, alpha_dtype, R, NT, C, stream);
}

extern "C" int dsp_pos_add_bwd_state(const void* dy, const void* tab, const int32_t* pos32, float keep_scale, unsigned int thr, uint64_t seed,
                                     uint64_t offset, void* dx, void* dalpha, void* workspace, size_t workspace_bytes, int act_dtype,
                                     int tab_dtype, int alpha_dtype, int64_t R, int NT, int C, const uint64_t* rng_state, dsp_stream_t stream)
{
    return pa_bwd("pos_add_bwd_state", dy, tab, pos32, keep_scale, thr, seed, offset, rng_state, dx, dalpha, workspace, workspace_bytes, act_dtype,
                  tab_dtype, alpha_dtype, R, NT, C, stream);
}
