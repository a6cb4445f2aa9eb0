// dag_strip.h — the launch structure and strip -> strip hand-off protocol of the banded DP kernels.  Internal; included by
// dag_dp_strip4g / strip2g / strip1g / strip2 / banded / maxstrip / maxstripw.hip and by nothing else.  One definition of each piece:
// the compute waves (row heads, exponent machinery, fallbacks) stay in their files.
//
// LAUNCH STRUCTURE.  A sample's L vertices are cut into column strips of W vertices; one workgroup owns a (sample, direction, strip) for all
// T rows.  The previous DP row of the strip plus a TRP-wide halo (the neighbour strip's boundary columns) is double-buffered in LDS, one
// workgroup barrier per row.  Next to the compute waves a workgroup runs three helper waves: the LOADER streams match rows into an LDS ring
// by LDS-DMA, the FETCH wave brings the halo of each row in, the PUBLISH wave hands this strip's boundary columns on.  (dag_dp_banded.hip
// has no helper waves and dag_dp_strip2.hip one: there the compute lanes next to the halo fetch and publish.)
//
// TICKETS.  Workgroups do not use blockIdx: each draws a ticket from counters[0].  Tickets count through the strips in dependency order
// (alpha left to right, beta right to left), all samples and directions of one position before the next, so a strip's producer always holds
// a SMALLER ticket than its consumer: the oldest unfinished workgroup never waits on one that has not been scheduled.  No residency
// assumption, no grid barrier, no deadlock.
//
// HAND-OFF.  For every row t a producer stores its TRP boundary values as 8-byte granules {tag (high word), fp32 value (low word)} with
// tag = tag_base + 1 + t.  A granule is ONE naturally aligned 8-byte store and ONE 8-byte load, both relaxed at agent scope (sc1 accesses,
// coherent across the device's CUs and XCDs): the value and the tag that vouches for it cannot be seen apart, so no flag, fence or release / acquire
// pair is needed, and a tag that is not the wanted one — zeroed memory, or an earlier launch's, whose tags are all <= tag_base — is simply
// "not yet".  The consumer requests granules STRIP_CH rows ahead and re-reads only on a tag mismatch (halo_wait).
//
// THE SPIN LIMIT.  halo_wait gives up after STRIP_SPIN_LIMIT polls: it sets bit 0 of the error word counters[1] and goes on with whatever
// the granule holds.  The launch then ends with wrong values instead of hanging, and the host reports the error word
// (dsp_dag_last_launch_status).  No test can reach this path, so these lines are correct by inspection only: this is the place to inspect.
#pragma once
#include "dag_dp.h"

namespace dsp {

typedef unsigned long long u64;
typedef unsigned int u32;

// One kernel argument block for all seven families (a family ignores the fields it has no use for).
struct StripParams {
    const float* match; const float* links; const int64_t* out_len; const int64_t* tgt_len;
    float* alpha; float* beta; int32_t* trace;
    u64* halo;                                // granules [dirslot][b][strip][t][TRP]
    u32* counters;                            // [0] ticket dispenser, [1] error word (bit 0: a halo wait hit the spin limit), [2] cells that took an
                                              // exact log-space fallback (dsp_dag_last_fallback_count); [3 ..] slots of the instrumentation builds
    u32 tag_base;
    int B, T, L, TR, NS, ndir;
    int ldm, ldo;                             // row pitches (elements) of match and of alpha / beta / alpha_max: >= L
    int dbg;                                  // instrumentation builds (-DDSP_PROF, -DDSP_MX_PROF) only; 0 in the product
};

constexpr u32 STRIP_SPIN_LIMIT = 1u << 22;
constexpr int STRIP_RING = 8;                 // match rows in the LDS ring; the loader runs RING - 1 rows ahead
constexpr int STRIP_CH = 4;                   // halo prefetch distance of the fetch wave (rows)
constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;
constexpr float EXP_BIAS = 120.f;             // exp space: stored / scaled values reach 2^120, a row sum stays under 2^126
constexpr int DEAD_EXP = -(1 << 30);          // exp space: group exponent of a group with no live vertex; far below any finite fp32 score

// ---- small device helpers ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ u64 gran_load(const u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void gran_store(u64* p, u32 tag, float v) {
    __hip_atomic_store(p, ((u64)tag << 32) | (u64)__float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// The row barrier: LDS traffic done, raw s_barrier.  No vmcnt wait — the loader's LDS-DMAs stay in flight across it (__syncthreads would
// drain them).
__device__ __forceinline__ void strip_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}
struct StripBarrier { __device__ __forceinline__ void operator()() const { strip_barrier(); } };
__device__ __forceinline__ float pair_max(float v) {             // lanes 2m, 2m+1: quad_perm [1,0,3,2]
    return fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, false)));
}
__device__ __forceinline__ float quad_max(float v) {             // lanes 4m .. 4m+3: then quad_perm [2,3,0,1]
    v = pair_max(v);
    return fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, false)));
}
// s_waitcnt vmcnt(N).  The gfx9 encoding has six bits for the counter (simm16[3:0] and [15:14]): 0 .. 63.
template <int N> __device__ __forceinline__ void wait_vmcnt() {
    static_assert(N >= 0 && N <= 63, "s_waitcnt encodes vmcnt 0 .. 63");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// ---- tickets ----------------------------------------------------------------------------------------------------------------------------
// `slot` is a 4-byte LDS word of the caller's; returns after a workgroup barrier.
__device__ __forceinline__ u32 strip_take_ticket(u32* slot, u32* counters) {
    if (threadIdx.x == 0) *slot = atomicAdd(&counters[0], 1u);
    __syncthreads();
    return *slot;
}
struct StripTicket { int so, b, dirslot, s; bool is_beta; };     // so: position in dependency order; s: the strip; dirslot: halo plane
// ndir: directions in this launch (1 or 2); has_beta: the kernel implements the beta direction at all (the max-DPs: ndir = 1, false)
__device__ __forceinline__ StripTicket strip_ticket_decode(u32 ticket, const StripParams& p, int ndir, bool has_beta) {
    StripTicket k;
    const int per = ndir * p.B;
    k.so = (int)(ticket / per);
    const int rem = (int)(ticket % per);
    k.is_beta = has_beta && (p.alpha == nullptr || (ndir == 2 && rem >= p.B));
    k.b = rem % p.B;
    k.dirslot = (ndir == 2 && rem >= p.B) ? 1 : 0;
    k.s = k.is_beta ? (p.NS - 1 - k.so) : k.so;
    return k;
}
// a strip with nothing reachable in it (or a sample with invalid lengths): -inf everywhere, no hand-off
__device__ __forceinline__ bool strip_is_dead(const StripParams& p, int Lb, int Tb, int j0) {
    const bool valid = !(Tb <= 0 || Lb <= 0 || Tb > p.T || Lb > p.L);
    return !valid || j0 >= Lb;
}
// ... its fill, one column per thread (kernels whose rows are 16-byte aligned keep a vector fill of their own)
__device__ __forceinline__ void strip_fill_dead(float* O, int ldo, int T, int j0, int W, int jlim, int nthreads) {
    for (int jj = j0 + (int)threadIdx.x; jj < j0 + W && jj < jlim; jj += nthreads)
        for (int t = 0; t < T; ++t) O[(size_t)t * ldo + jj] = NEG_INF;
}

// ---- who hands what to whom -------------------------------------------------------------------------------------------------------------
struct StripHalo { const u64* in; u64* out; bool has_producer, has_consumer; };
__device__ __forceinline__ StripHalo strip_halo(const StripParams& p, const StripTicket& k, bool beta, int W, int TRP, int Lb) {
    StripHalo h;
    const int j0 = k.s * W;
    h.has_producer = k.so > 0 && (beta ? (j0 + W < Lb) : true);          // beta: the right strip exists and is live
    h.has_consumer = beta ? (k.s > 0) : (k.s < p.NS - 1 && j0 + W < Lb);
    const int prod_strip = beta ? k.s + 1 : k.s - 1;
    h.in = p.halo + ((size_t)(k.dirslot * p.B + k.b) * p.NS + (h.has_producer ? prod_strip : 0)) * (size_t)p.T * TRP;
    h.out = p.halo + ((size_t)(k.dirslot * p.B + k.b) * p.NS + k.s) * (size_t)p.T * TRP;
    return h;
}

// ---- the spin-wait ----------------------------------------------------------------------------------------------------------------------
// Wait until the lane's GPL granules at `row` carry the tag `want`, for every active lane of the wave; g holds what was prefetched and
// comes back with the granules.  Only granules with a stale tag are read again.
template <int GPL, int SLEEP = 1>
__device__ __forceinline__ void halo_wait(const u64* row, u32 want, u64 (&g)[GPL], u32* counters, int lane) {
    u32 spins = 0;
    for (;;) {
        bool ok = true;
#pragma unroll
        for (int e = 0; e < GPL; ++e) ok &= (u32)(g[e] >> 32) == want;
        if (__all(ok)) break;
#pragma unroll
        for (int e = 0; e < GPL; ++e) if ((u32)(g[e] >> 32) != want) g[e] = gran_load(row + e);
        if (++spins > STRIP_SPIN_LIMIT) { if (lane == 0) atomicOr(&counters[1], 1u); break; }
        __builtin_amdgcn_s_sleep(SLEEP);
    }
}

// ---- helper waves -----------------------------------------------------------------------------------------------------------------------
// Row `it` of the iteration is DP row t = it (alpha, max) or nrows - 1 - it (beta).  Every helper wave passes the prologue barrier and then
// one barrier per row, like the compute waves; `bar` is strip_barrier unless the kernel wraps it (strip4g's profiled build).
template <bool BETA> __device__ __forceinline__ int strip_row(int it, int nrows) { return BETA ? (nrows - 1 - it) : it; }

// LOADER: match rows -> LDS ring by LDS-DMA, DMA_BYTES (4 or 16: rows 16-byte aligned) per lane, PD rows ahead.  The wave issues loads only,
// so vmcnt retires them in order and one counted wait per row is sound.
template <int W, int DMA_BYTES, int RING, int PD, bool BETA, class Bar = StripBarrier>
__device__ __forceinline__ void strip_loader_wave(const float* M, int ldm, float* Mring, int j0, int L, int nrows, int lane, Bar bar = Bar()) {
    constexpr int EPL = DMA_BYTES / 4, PIECE = 64 * EPL, NDMA = W / PIECE;      // elements per lane, per DMA; DMAs per row
    static_assert((DMA_BYTES == 4 || DMA_BYTES == 16) && W % PIECE == 0 && PD < RING, "loader geometry");
    auto issue_row = [&](int itr) {
        const float* rowp = M + (size_t)strip_row<BETA>(itr, nrows) * ldm;
        float* slot = Mring + (size_t)(itr % RING) * W;
#pragma unroll
        for (int i = 0; i < NDMA; ++i) {
            const int col = j0 + i * PIECE + lane * EPL;
            const float* g = rowp + (col < L ? col : 0);          // out-of-range lanes re-read a valid address
            const auto src = (const __attribute__((address_space(1))) void*)g;
            const auto dst = (__attribute__((address_space(3))) void*)(slot + i * PIECE);
            if constexpr (DMA_BYTES == 16) __builtin_amdgcn_global_load_lds(src, dst, 16, 0, 0);      // (the builtin wants a literal size)
            else __builtin_amdgcn_global_load_lds(src, dst, 4, 0, 0);
        }
    };
    for (int r = 0; r < PD && r < nrows; ++r) issue_row(r);
    wait_vmcnt<0>();
    bar();                                       // prologue barrier
    for (int it = 0; it < nrows; ++it) {
        const int nx = it + PD;                  // its slot was last read at least one barrier ago (PD < RING)
        if (nx < nrows) {
            issue_row(nx);
            wait_vmcnt<(PD - 1) * NDMA>();       // row it+1 has landed; rows it+2 .. it+PD, NDMA DMAs each, may stay in flight
        } else {
            wait_vmcnt<0>();
        }
        bar();
    }
}

// FETCH: TRP granules per row, GPL per lane (lanes >= TRP / GPL idle).
template <int TRP, int GPL> __device__ __forceinline__ bool strip_halo_lane(int lane) { return TRP / GPL >= 64 || lane < TRP / GPL; }
template <int TRP, int GPL, bool BETA>
__device__ __forceinline__ void halo_load_row(const u64* hin, int itr, int nrows, int lane, u64 (&dst)[GPL]) {
    const bool on = itr < nrows && strip_halo_lane<TRP, GPL>(lane);
#pragma unroll
    for (int e = 0; e < GPL; ++e) dst[e] = on ? gran_load(hin + (size_t)strip_row<BETA>(itr, nrows) * TRP + GPL * lane + e) : 0;
}
// before the prologue barrier: rows 0 .. CH-1 requested
template <int TRP, int GPL, int CH, bool BETA>
__device__ __forceinline__ void strip_fetch_prime(const u64* hin, bool has_producer, int nrows, int lane, u64 (&g)[CH][GPL]) {
#pragma unroll
    for (int k = 0; k < CH; ++k)
#pragma unroll
        for (int e = 0; e < GPL; ++e) g[k][e] = 0;
    if (has_producer) {
#pragma unroll
        for (int k = 0; k < CH; ++k) halo_load_row<TRP, GPL, BETA>(hin, k, nrows, lane, g[k]);
    }
}
// the row loop: rolling prefetch — row it+CH is requested when row it has been consumed, so every request has CH row times to land and a
// consumer settles about CH + 3 rows behind its producer.  store(it, hv) writes the row's halo values (-inf without a producer) into LDS
// buffer it & 1: the exp-space kernels convert them, the log-space and max kernels store them.
template <int TRP, int GPL, int CH, bool BETA, class Store, class Bar = StripBarrier>
__device__ __forceinline__ void strip_fetch_rows(const StripParams& p, const u64* hin, bool has_producer, int nrows, int lane,
                                                 u64 (&g)[CH][GPL], Store store, Bar bar = Bar()) {
    bar();                                       // prologue barrier
    for (int itb = 0; itb < nrows; itb += CH) {
#pragma unroll
        for (int k = 0; k < CH; ++k) {
            const int it = itb + k;
            if (it >= nrows) break;
            const int t = strip_row<BETA>(it, nrows);
            float hv[GPL];
#pragma unroll
            for (int e = 0; e < GPL; ++e) hv[e] = NEG_INF;
            if (has_producer && strip_halo_lane<TRP, GPL>(lane)) {
                u64 x[GPL];
#pragma unroll
                for (int e = 0; e < GPL; ++e) x[e] = g[k][e];
                halo_wait<GPL>(hin + (size_t)t * TRP + GPL * lane, p.tag_base + 1u + (u32)t, x, p.counters, lane);
#pragma unroll
                for (int e = 0; e < GPL; ++e) hv[e] = __uint_as_float((u32)x[e]);
            }
            store(it, hv);
            if (has_producer) halo_load_row<TRP, GPL, BETA>(hin, it + CH, nrows, lane, g[k]);
            bar();
        }
    }
}

// PUBLISH: after barrier it-1 row it-1 is complete in LDS buffer (it-1) & 1 and the compute waves write the other one.  `boundary` points
// at the TRP boundary columns of buffer 0 (alpha, max: the strip's last TRP columns, beta: its first), the buffers are RL floats apart.
template <int TRP, int GPL, bool BETA, class Bar = StripBarrier>
__device__ __forceinline__ void strip_publish_wave(const StripParams& p, u64* hout, const float* boundary, int RL, bool has_consumer,
                                                   int nrows, int lane, Bar bar = Bar()) {
    const bool pl = has_consumer && strip_halo_lane<TRP, GPL>(lane);
    auto publish = [&](int itp) {                // row of iteration itp - 1
        const int tp = strip_row<BETA>(itp - 1, nrows);
#pragma unroll
        for (int e = 0; e < GPL; ++e)
            gran_store(hout + (size_t)tp * TRP + GPL * lane + e, p.tag_base + 1u + (u32)tp, boundary[((itp - 1) & 1) * RL + GPL * lane + e]);
    };
    bar();                                       // prologue barrier
    for (int it = 0; it < nrows; ++it) {
        if (it > 0 && pl) publish(it);
        bar();
    }
    if (pl && nrows > 0) publish(nrows);
}

// ---- host side --------------------------------------------------------------------------------------------------------------------------
static inline size_t strip_halo_bytes(int ndir, int B, int NS, int T, int TRP) { return (size_t)ndir * B * NS * T * TRP * sizeof(u64); }

// the argument block without its scratch (banded_acquire_ws fills halo / counters / tag_base)
static inline StripParams strip_params(const float* match, const float* links, const int64_t* out_len, const int64_t* tgt_len,
                                       float* alpha, float* beta, int32_t* trace, int B, int T, int L, int TR, int NS, int ndir, int ldm, int ldo)
{
    StripParams p;
    p.match = match; p.links = links; p.out_len = out_len; p.tgt_len = tgt_len; p.alpha = alpha; p.beta = beta; p.trace = trace;
    p.halo = nullptr; p.counters = nullptr; p.tag_base = 0;
    p.B = B; p.T = T; p.L = L; p.TR = TR; p.NS = NS; p.ndir = ndir; p.ldm = ldm; p.ldo = ldo; p.dbg = 0;
    return p;
}
static inline int strip_acquire(StripParams& p, size_t halo_bytes, hipStream_t st) {
    return banded_acquire_ws(st, halo_bytes, p.T, &p.counters, &p.halo, &p.tag_base);
}
template <class K>
static inline int launch_strip(K kernel, const StripParams& p, int nwg, int threads, size_t lds_bytes, hipStream_t st, const char* what)
{
    if (lds_bytes) set_max_dynamic_lds((const void*)kernel, (int)lds_bytes);
    hipLaunchKernelGGL(kernel, dim3((unsigned)nwg), dim3(threads), lds_bytes, st, p);
    return check_launch(what);
}

}  // namespace dsp
