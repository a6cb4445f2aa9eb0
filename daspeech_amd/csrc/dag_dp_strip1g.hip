// dag_dp_strip1g.hip — banded DAG DP for windows 65 .. 128 in EXP SPACE: K2 alpha || K3 beta, ONE vertex per lane (r06).
//
// Third member of the strip family (dag_dp_strip4g.hip: 4 vertices x 32 transitions per lane, dag_dp_strip2g.hip: 2 x 64): the same 128
// transition weights in a lane's registers, here for one vertex with a 128-wide window.  Until r06 these windows fell onto the dense-window
// matrix-core DP, which is built for windows of thousands of vertices and is at its worst on narrow bands (B = 32, T = 64, L = 4096: 5.1 ms at
// TR = 65 against 0.19 ms for TR = 64 on the strips — a 27 x step at a dispatch boundary).
//   * column strips of 256 vertices, launch structure and hand-off of dag_strip.h with 128 boundary columns (two granules per helper lane);
//   * previous row in LDS as values 2^(a2 - X) with one integer exponent per group of 4 vertices = a QUAD of lanes (two quad-permutes);
//   * a lane's window is the 132 values from the 16-byte boundary under its first predecessor: 33 ds_read_b128, too many to hold at once next to
//     the weights, so they stream through two 6-read register buffers — chunk c+1 is requested before chunk c is consumed; the 33 group
//     exponents are read first (the row's reference exponent needs all of them);
//   * the transition tile of the prologue is loaded in two halves of 64 slots (a 384 x 129 tile would not fit the LDS);
//   * guard and fallbacks as strip2g: sums under 2^-97 (2^30 for a column with a flushed weight) take the diagonal's single-transition
//     shortcut or the exact log-space form; windows under 125 drop the groups without a predecessor from the row's reference.
// Replaces calculate_alpha_kernel / calculate_beta_kernel (dag_loss.cu:40-140,178-274) for 64 < translen <= 128.
#include "dag_strip.h"

// the row's LDS issue groups (generated: operand numbers and byte offsets)
#define HEAD_ASM "ds_read_b32 %0, %24\n\t" \
                                 "ds_read2_b32 %1, %25 offset0:0 offset1:1\n\t" \
                                 "ds_read2_b32 %2, %25 offset0:2 offset1:3\n\t" \
                                 "ds_read2_b32 %3, %25 offset0:4 offset1:5\n\t" \
                                 "ds_read2_b32 %4, %25 offset0:6 offset1:7\n\t" \
                                 "ds_read2_b32 %5, %25 offset0:8 offset1:9\n\t" \
                                 "ds_read2_b32 %6, %25 offset0:10 offset1:11\n\t" \
                                 "ds_read2_b32 %7, %25 offset0:12 offset1:13\n\t" \
                                 "ds_read2_b32 %8, %25 offset0:14 offset1:15\n\t" \
                                 "ds_read2_b32 %9, %25 offset0:16 offset1:17\n\t" \
                                 "ds_read2_b32 %10, %25 offset0:18 offset1:19\n\t" \
                                 "ds_read2_b32 %11, %25 offset0:20 offset1:21\n\t" \
                                 "ds_read2_b32 %12, %25 offset0:22 offset1:23\n\t" \
                                 "ds_read2_b32 %13, %25 offset0:24 offset1:25\n\t" \
                                 "ds_read2_b32 %14, %25 offset0:26 offset1:27\n\t" \
                                 "ds_read2_b32 %15, %25 offset0:28 offset1:29\n\t" \
                                 "ds_read2_b32 %16, %25 offset0:30 offset1:31\n\t" \
                                 "ds_read_b32 %17, %25 offset:128\n\t" \
                                 "ds_read_b128 %18, %26\n\t" \
                                 "ds_read_b128 %19, %26 offset:16\n\t" \
                                 "ds_read_b128 %20, %26 offset:32\n\t" \
                                 "ds_read_b128 %21, %26 offset:48\n\t" \
                                 "ds_read_b128 %22, %26 offset:64\n\t" \
                                 "ds_read_b128 %23, %26 offset:80"
#define CHUNK6_1 "ds_read_b128 %0, %6 offset:96\n\t" \
                                 "ds_read_b128 %1, %6 offset:112\n\t" \
                                 "ds_read_b128 %2, %6 offset:128\n\t" \
                                 "ds_read_b128 %3, %6 offset:144\n\t" \
                                 "ds_read_b128 %4, %6 offset:160\n\t" \
                                 "ds_read_b128 %5, %6 offset:176"
#define CHUNK6_2 "ds_read_b128 %0, %6 offset:192\n\t" \
                                 "ds_read_b128 %1, %6 offset:208\n\t" \
                                 "ds_read_b128 %2, %6 offset:224\n\t" \
                                 "ds_read_b128 %3, %6 offset:240\n\t" \
                                 "ds_read_b128 %4, %6 offset:256\n\t" \
                                 "ds_read_b128 %5, %6 offset:272"
#define CHUNK6_3 "ds_read_b128 %0, %6 offset:288\n\t" \
                                 "ds_read_b128 %1, %6 offset:304\n\t" \
                                 "ds_read_b128 %2, %6 offset:320\n\t" \
                                 "ds_read_b128 %3, %6 offset:336\n\t" \
                                 "ds_read_b128 %4, %6 offset:352\n\t" \
                                 "ds_read_b128 %5, %6 offset:368"
#define CHUNK6_4 "ds_read_b128 %0, %6 offset:384\n\t" \
                                 "ds_read_b128 %1, %6 offset:400\n\t" \
                                 "ds_read_b128 %2, %6 offset:416\n\t" \
                                 "ds_read_b128 %3, %6 offset:432\n\t" \
                                 "ds_read_b128 %4, %6 offset:448\n\t" \
                                 "ds_read_b128 %5, %6 offset:464"
#define CHUNK3_5 "ds_read_b128 %0, %3 offset:480\n\t" \
                                 "ds_read_b128 %1, %3 offset:496\n\t" \
                                 "ds_read_b128 %2, %3 offset:512"

namespace dsp {

typedef float h1_v2f __attribute__((ext_vector_type(2)));
typedef float h1_v4f __attribute__((ext_vector_type(4)));
typedef int h1_v2i __attribute__((ext_vector_type(2)));

constexpr int H1_NT = 256;                    // compute lanes = columns per strip
constexpr int H1_W = H1_NT;
constexpr int H1_TRP = 128;                   // window / halo width
constexpr int H1_RL = H1_W + H1_TRP;          // 384
constexpr int H1_GL = H1_RL / 4;              // 96
template <bool BETA>
__device__ __forceinline__ void strip1g_body(const StripParams& p, char* smem_raw, const StripTicket& k)
{
    const int b = k.b, s = k.s;
    constexpr int W = H1_W, RL = H1_RL, GL = H1_GL, NCW = H1_NT / 64, TRP = H1_TRP;
    float* Abuf = reinterpret_cast<float*>(smem_raw);          // [2][RL]  exact row, log2 domain
    float* Vbuf = Abuf + 2 * RL;                               // [2][RL]  V = 2^(a2 - X[group])
    int* Xbuf = reinterpret_cast<int*>(Vbuf + 2 * RL);         // [2][GL]  group exponents
    float* Mring = reinterpret_cast<float*>(Xbuf + 2 * GL);    // [RING][W] match rows

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = p.T, L = p.L, TR = p.TR;
    const int j0 = s * W;
    const int Lb = (int)p.out_len[b], Tb = (int)p.tgt_len[b];
    const float* M = p.match + (size_t)b * T * p.ldm;
    const float* K = p.links + (size_t)b * L * TR;
    float* O = (BETA ? p.beta : p.alpha) + (size_t)b * T * p.ldo;
    const int LDO = p.ldo, LPAD = min(p.ldo, (L + 3) & ~3);
    const int nrows = Tb;

    const StripHalo halo = strip_halo(p, k, BETA, W, TRP, Lb);
    // LDS geometry: alpha li = col - j0 + 128 (halo [0,128)); beta li = col - j0 (halo [W, W+128))
    const int halo_li0 = BETA ? W : 0;
    const int own_li0 = BETA ? 0 : TRP;

    // ---- prologue: transitions -> registers through an LDS tile, in two halves of 64 slots.  tile[r][dd] = links[rlo + r][64 h + dd]
    // (pitch 65), -inf outside the graph / beyond TR.  The tile overlays the main-loop buffers, which are not live yet.
    const int l = tid;                           // compute lanes: the lane's vertex
    const int par = l & 3;                       // position inside the 4-vertex group: the window starts `par` elements before the lane's own
    const int j = j0 + l;
    h1_v2f E2[66];                               // E2[i] = (weight of window element 2i, of 2i+1); 0 where the element is no predecessor
#pragma unroll
    for (int i = 0; i < 66; ++i) { E2[i].x = NEG_INF; E2[i].y = NEG_INF; }
    for (int h = 0; h < 2; ++h) {
        float* tile = reinterpret_cast<float*>(smem_raw);
        {
            constexpr int NTHR = H1_NT + 192, RPP = NTHR / 64;     // 7 rows per pass
            const int rlo = BETA ? j0 : (j0 - TRP);
            const int dd = tid & 63, r0 = tid >> 6, slot = 64 * h + dd;
            for (int rb = r0; rb < W + TRP; rb += 8 * RPP) {
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int i = rlo + rb + u * RPP;
                    const bool ok = slot < TR && i >= 0 && i < L;
                    const float raw = K[(size_t)(ok ? i : 0) * TR + (ok ? slot : 0)];
                    v[u] = ok ? raw : NEG_INF;
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) { const int r = rb + u * RPP; if (r < W + TRP) tile[r * 65 + dd] = v[u]; }
            }
        }
        __syncthreads();
        if (wave < NCW) {
#pragma unroll
            for (int q = 0; q < 132; ++q) {
                const int d = BETA ? (q - par) : (TRP + par - q);              // runtime (lane's position in its group): computed tile address
                if (d >= 64 * h + 1 && d <= 64 * h + 64) {
                    float v = BETA ? tile[l * 65 + (d - 1 - 64 * h)] : tile[(l - d + TRP) * 65 + (d - 1 - 64 * h)];
                    if (BETA && j + d >= Lb) v = NEG_INF;
                    if (q & 1) E2[q >> 1].y = v * LOG2E; else E2[q >> 1].x = v * LOG2E;
                }
            }
        }
        __syncthreads();                         // tile consumed: the next half (or the main-loop buffers) may overwrite it
    }

    if (wave < NCW) {
        // =========================================================== compute waves
        __builtin_amdgcn_s_setprio(2);
        const bool col_ok = j < L;
        auto cell_active = [&](int col, int t) -> bool {
            if (!BETA) return col >= t && col < Lb && (long)col <= (long)t * TR;
            const int rem = Tb - 1 - t, gap = Lb - 1 - col;
            return col >= t && gap >= rem && (long)gap <= (long)rem * TR;
        };
        auto liidx = [&](int d) -> int { return BETA ? (l + d) : (TRP + l - d); };          // LDS row index of the element at distance d
        float lmax, sthr;
        {
            float mx = NEG_INF;
#pragma unroll
            for (int i = 0; i < 66; ++i) mx = fmaxf(mx, fmaxf(E2[i].x, E2[i].y));
            if (mx == NEG_INF) mx = 0.f;
            lmax = mx;
            bool flushed = false;
#pragma unroll
            for (int i = 0; i < 66; ++i) {
                flushed |= ((E2[i].x != NEG_INF) & (E2[i].x - mx < -120.f)) | ((E2[i].y != NEG_INF) & (E2[i].y - mx < -120.f));
                E2[i].x = __builtin_amdgcn_exp2f(E2[i].x - mx); E2[i].y = __builtin_amdgcn_exp2f(E2[i].y - mx);
            }
            sthr = flushed ? 0x1p30f : 0x1p-97f;
        }
        // weight of distance 1 (the diagonal shortcut): window element 127 + par (alpha) / 1 + par (beta), four static candidates
        auto Eval1 = [&]() -> float {
            const int q0 = BETA ? 1 : 127;
            const float c0 = (q0 & 1) ? E2[q0 >> 1].y : E2[q0 >> 1].x, c1 = ((q0 + 1) & 1) ? E2[(q0 + 1) >> 1].y : E2[(q0 + 1) >> 1].x;
            const float c2 = ((q0 + 2) & 1) ? E2[(q0 + 2) >> 1].y : E2[(q0 + 2) >> 1].x, c3 = ((q0 + 3) & 1) ? E2[(q0 + 3) >> 1].y : E2[(q0 + 3) >> 1].x;
            return par == 0 ? c0 : (par == 1 ? c1 : (par == 2 ? c2 : c3));
        };
        // first (alpha) / last (beta) window group that holds a predecessor: window element of distance TR is 128 + par - TR resp. par + TR
        const int gcut = BETA ? ((par + TR) >> 2) : ((TRP + par - TR) >> 2);
        strip_barrier();                            // prologue barrier: match row 0 is in the ring

        for (int it = 0; it < nrows; ++it) {
            const int t = BETA ? (Tb - 1 - it) : it;
            const int cur = it & 1, prv = cur ^ 1;
            float a2 = NEG_INF;
            if (it == 0) {
                const float m0 = Mring[(size_t)(it % STRIP_RING) * W + l];
                const bool seed = BETA ? (j == Lb - 1) : (j == 0);
                if (seed) a2 = m0 * LOG2E;
            } else {
                // ---- row head: match, 33 group exponents, the first 6 window groups — one issue group; the other 27 groups stream through
                // two register buffers (chunk c+1 requested before chunk c is consumed).  LDS returns in order; lgkmcnt counts to 15.
                float mt; h1_v2i xa[16]; int x32; h1_v4f pa[6], pb[6];
                const u32 vaddr = (u32)(uintptr_t)(__attribute__((address_space(3))) void*)(Vbuf + prv * RL + 4 * (l >> 2));
                {
                    const u32 maddr = (u32)(uintptr_t)(__attribute__((address_space(3))) void*)(Mring + (size_t)(it % STRIP_RING) * W + l);
                    const u32 xaddr = (u32)(uintptr_t)(__attribute__((address_space(3))) void*)(Xbuf + prv * GL + (l >> 2));
                    asm volatile(HEAD_ASM
                                 : "=&v"(mt), "=&v"(xa[0]), "=&v"(xa[1]), "=&v"(xa[2]), "=&v"(xa[3]), "=&v"(xa[4]), "=&v"(xa[5]), "=&v"(xa[6]), "=&v"(xa[7]),
                                   "=&v"(xa[8]), "=&v"(xa[9]), "=&v"(xa[10]), "=&v"(xa[11]), "=&v"(xa[12]), "=&v"(xa[13]), "=&v"(xa[14]), "=&v"(xa[15]), "=&v"(x32),
                                   "=&v"(pa[0]), "=&v"(pa[1]), "=&v"(pa[2]), "=&v"(pa[3]), "=&v"(pa[4]), "=&v"(pa[5])
                                 : "v"(maddr), "v"(xaddr), "v"(vaddr)
                                 : "memory");
                }
                // match + the 17 exponent reads are the first 18 of 24 operations: done when at most 6 are outstanding
                asm volatile("s_waitcnt lgkmcnt(6)" : "+v"(mt), "+v"(xa[0]), "+v"(xa[1]), "+v"(xa[2]), "+v"(xa[3]), "+v"(xa[4]), "+v"(xa[5]), "+v"(xa[6]), "+v"(xa[7]),
                             "+v"(xa[8]), "+v"(xa[9]), "+v"(xa[10]), "+v"(xa[11]), "+v"(xa[12]), "+v"(xa[13]), "+v"(xa[14]), "+v"(xa[15]), "+v"(x32));
                const bool okc = cell_active(j, t);
                const float base = lmax + mt * LOG2E;
                int xw[33];
#pragma unroll
                for (int g = 0; g < 16; ++g) { xw[2 * g] = xa[g].x; xw[2 * g + 1] = xa[g].y; }
                xw[32] = x32;
                if (TR < 125) {                  // groups without a predecessor: out of the window (see strip2g)
#pragma unroll
                    for (int g = 0; g < 33; ++g) if (BETA ? (g > gcut) : (g < gcut)) xw[g] = DEAD_EXP;
                }
                int refi = xw[0];
#pragma unroll
                for (int g = 1; g < 33; ++g) refi = max(refi, xw[g]);
                const bool any_live = refi != DEAD_EXP;
                if (!any_live) refi = 0;
                h1_v2f S2[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) { S2[c].x = 0.f; S2[c].y = 0.f; }
#define H1_ISSUE6(buf, c) asm volatile(CHUNK6_##c : "=&v"(buf[0]), "=&v"(buf[1]), "=&v"(buf[2]), "=&v"(buf[3]), "=&v"(buf[4]), "=&v"(buf[5]) : "v"(vaddr) : "memory");
#define H1_GROUP(buf, k, g, n) \
                { asm volatile("s_waitcnt lgkmcnt(" #n ")" : "+v"(buf[k])); \
                  const int kg = xw[g] - refi; \
                  h1_v2f wa, wb; wa.x = ldexpf(buf[k].x, kg); wa.y = ldexpf(buf[k].y, kg); wb.x = ldexpf(buf[k].z, kg); wb.y = ldexpf(buf[k].w, kg); \
                  S2[(2 * (g)) & 3] = __builtin_elementwise_fma(wa, E2[2 * (g)], S2[(2 * (g)) & 3]); \
                  S2[(2 * (g) + 1) & 3] = __builtin_elementwise_fma(wb, E2[2 * (g) + 1], S2[(2 * (g) + 1) & 3]); }
                // chunk 0 (groups 0..5) is in pa; request chunk 1 into pb, consume pa: element k of pa has landed when at most (5 - k) + 6 are outstanding
                H1_ISSUE6(pb, 1)
                H1_GROUP(pa, 0, 0, 11) H1_GROUP(pa, 1, 1, 10) H1_GROUP(pa, 2, 2, 9) H1_GROUP(pa, 3, 3, 8) H1_GROUP(pa, 4, 4, 7) H1_GROUP(pa, 5, 5, 6)
                H1_ISSUE6(pa, 2)
                H1_GROUP(pb, 0, 6, 11) H1_GROUP(pb, 1, 7, 10) H1_GROUP(pb, 2, 8, 9) H1_GROUP(pb, 3, 9, 8) H1_GROUP(pb, 4, 10, 7) H1_GROUP(pb, 5, 11, 6)
                H1_ISSUE6(pb, 3)
                H1_GROUP(pa, 0, 12, 11) H1_GROUP(pa, 1, 13, 10) H1_GROUP(pa, 2, 14, 9) H1_GROUP(pa, 3, 15, 8) H1_GROUP(pa, 4, 16, 7) H1_GROUP(pa, 5, 17, 6)
                H1_ISSUE6(pa, 4)
                H1_GROUP(pb, 0, 18, 11) H1_GROUP(pb, 1, 19, 10) H1_GROUP(pb, 2, 20, 9) H1_GROUP(pb, 3, 21, 8) H1_GROUP(pb, 4, 22, 7) H1_GROUP(pb, 5, 23, 6)
                asm volatile(CHUNK3_5 : "=&v"(pb[0]), "=&v"(pb[1]), "=&v"(pb[2]) : "v"(vaddr) : "memory");        // groups 30 .. 32
                H1_GROUP(pa, 0, 24, 8) H1_GROUP(pa, 1, 25, 7) H1_GROUP(pa, 2, 26, 6) H1_GROUP(pa, 3, 27, 5) H1_GROUP(pa, 4, 28, 4) H1_GROUP(pa, 5, 29, 3)
                H1_GROUP(pb, 0, 30, 2) H1_GROUP(pb, 1, 31, 1) H1_GROUP(pb, 2, 32, 0)
#undef H1_GROUP
#undef H1_ISSUE6
                const h1_v2f t2 = (S2[0] + S2[1]) + (S2[2] + S2[3]);
                const float S = t2.x + t2.y;
                const float ref = (float)refi;
                // ---- row tail
                const bool okl = okc & any_live;
                const bool flag = okl & !(S >= sthr && S <= 0x1p126f);
                a2 = (okl & !flag) ? (__builtin_amdgcn_logf(S) + (ref + base)) : NEG_INF;
                if (__builtin_expect(flag, 0)) {
                    float r = NEG_INF;
                    // (0) the DP's diagonal cell has ONE live transition: a2 = a2_prev(predecessor) + log2(weight) + base, no sum
                    const int dl = BETA ? (Lb - Tb + 1 + t - j) : (j - t + 1);
                    bool done = false;
                    if (dl == 1 && sthr == 0x1p-97f) {
                        const float ap = Abuf[prv * RL + liidx(1)];
                        const float e1 = Eval1();
                        if (e1 > 0.f) { r = (ap != NEG_INF) ? (ap + __builtin_amdgcn_logf(e1) + base) : NEG_INF; done = true; }
                    }
                    if (!done) {
                        // (b) exact log-space value: previous row from LDS, raw transitions re-read from HBM
                        float amax = NEG_INF;
                        for (int d = 1; d <= TRP; ++d) amax = fmaxf(amax, Abuf[prv * RL + liidx(d)]);
                        if (amax != NEG_INF) {
                            atomicAdd(&p.counters[2], 1u);
                            float mx = NEG_INF, sum = 0.f;
                            for (int d0 = 1; d0 <= TRP; d0 += 8) {
                                float lk[8];
#pragma unroll
                                for (int u = 0; u < 8; ++u) {
                                    const int d = d0 + u;
                                    const int row = BETA ? j : (j - d);
                                    const bool ok = d <= TR && row >= 0 && row < L && (!BETA || j + d < Lb);
                                    const float raw = K[(size_t)(ok ? row : 0) * TR + (ok ? d - 1 : 0)];
                                    lk[u] = ok ? raw * LOG2E : NEG_INF;
                                }
#pragma unroll
                                for (int u = 0; u < 8; ++u) {
                                    const int d = d0 + u;
                                    const float v = Abuf[prv * RL + liidx(d)] + lk[u];
                                    const float nm = fmaxf(mx, v);
                                    if (nm != NEG_INF) sum = sum * __builtin_amdgcn_exp2f(mx - nm) + __builtin_amdgcn_exp2f(v - nm);
                                    mx = nm;
                                }
                            }
                            if (mx != NEG_INF) r = __builtin_amdgcn_logf(sum) + mx + mt * LOG2E;
                        }
                    }
                    a2 = r;
                }
            }
            // ---- write the row: group exponent X = ceil(largest of the QUAD's four) - 120
            float vn; int xn;
            {
                const float amax = quad_max(a2);
                const bool dead = amax == NEG_INF;
                const float cf = dead ? 0.f : ceilf(amax) - EXP_BIAS;
                vn = __builtin_amdgcn_exp2f(a2 - cf);
                xn = dead ? DEAD_EXP : (int)cf;
            }
            Vbuf[cur * RL + own_li0 + l] = vn;
            if (par == 0) Xbuf[cur * GL + (own_li0 >> 2) + (l >> 2)] = xn;
            Abuf[cur * RL + own_li0 + l] = a2;
            if (col_ok) {
                O[(size_t)t * LDO + j] = a2 * LN2;
                if (j + 1 == L) for (int c = L; c < LPAD; ++c) O[(size_t)t * LDO + c] = NEG_INF;         // the owner of the last column fills the pitch padding
            }
            strip_barrier();
        }
        if (col_ok) for (int t = Tb; t < T; ++t) {                                      // rows the recurrence never reaches
            O[(size_t)t * LDO + j] = NEG_INF;
            if (j + 1 == L) for (int c = L; c < LPAD; ++c) O[(size_t)t * LDO + c] = NEG_INF;
        }
    } else if (wave == NCW) {
        // loader wave: 4 bytes per lane (rows of a dense tensor are not 16-byte aligned in general)
        strip_loader_wave<W, 4, STRIP_RING, STRIP_RING - 1, BETA>(M, p.ldm, Mring, j0, L, nrows, lane);
    } else if (wave == NCW + 1) {
        // fetch wave: two boundary values per lane; the halo's 32 groups of 4 columns = pairs of lanes
        u64 g[STRIP_CH][2];
        strip_fetch_prime<TRP, 2, STRIP_CH, BETA>(halo.in, halo.has_producer, nrows, lane, g);
        strip_fetch_rows<TRP, 2, STRIP_CH, BETA>(p, halo.in, halo.has_producer, nrows, lane, g, [&](int it, const float (&hv)[2]) {
            const int cur = it & 1;
            const float gm = pair_max(fmaxf(hv[0], hv[1]));
            const bool dead = gm == NEG_INF;
            const float cf = dead ? 0.f : ceilf(gm) - EXP_BIAS;
            *reinterpret_cast<float2*>(Abuf + cur * RL + halo_li0 + 2 * lane) = make_float2(hv[0], hv[1]);
            *reinterpret_cast<float2*>(Vbuf + cur * RL + halo_li0 + 2 * lane) = make_float2(__builtin_amdgcn_exp2f(hv[0] - cf), __builtin_amdgcn_exp2f(hv[1] - cf));
            if ((lane & 1) == 0) Xbuf[cur * GL + (halo_li0 >> 2) + (lane >> 1)] = dead ? DEAD_EXP : (int)cf;
        });
    } else {
        // publish wave.  alpha: the strip's last 128 columns (li W .. W+127); beta: its first 128 (li 0 .. 127)
        strip_publish_wave<TRP, 2, BETA>(p, halo.out, Abuf + (BETA ? 0 : W), RL, halo.has_consumer, nrows, lane);
    }
}

__global__ __launch_bounds__(H1_NT + 192) void dag_strip1g_kernel(StripParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];          // 16-byte header (ticket); everything else starts at +16
    const StripTicket k = strip_ticket_decode(strip_take_ticket(reinterpret_cast<u32*>(smem_raw), p.counters), p, p.ndir, true);
    const int j0 = k.s * H1_W;
    if (strip_is_dead(p, (int)p.out_len[k.b], (int)p.tgt_len[k.b], j0)) {
        strip_fill_dead((k.is_beta ? p.beta : p.alpha) + (size_t)k.b * p.T * p.ldo, p.ldo, p.T, j0, H1_W, min(p.ldo, (p.L + 3) & ~3), H1_NT + 192);
        return;
    }
    if (k.is_beta) strip1g_body<true>(p, smem_raw + 16, k);
    else strip1g_body<false>(p, smem_raw + 16, k);
}

// ------------------------------------------------------------------------------------------------ host side
bool strip1g_supported(int L, int TR) { return TR > 64 && TR <= H1_TRP && L >= 1; }
size_t strip1g_ws_bytes(int B, int T, int L, int ndir) { return strip_halo_bytes(ndir, B, (L + H1_W - 1) / H1_W, T, H1_TRP); }

int launch_dag_strip1g(const float* match, const float* links, const int64_t* out_len, const int64_t* tgt_len,
                       float* alpha, float* beta, int B, int T, int L, int TR, int ldm, int ldo, hipStream_t st)
{
    const int ndir = (alpha && beta) ? 2 : 1;
    StripParams p = strip_params(match, links, out_len, tgt_len, alpha, beta, nullptr, B, T, L, TR, (L + H1_W - 1) / H1_W, ndir, ldm, ldo);
    int rc = strip_acquire(p, strip1g_ws_bytes(B, T, L, ndir), st);
    if (rc) return rc;
    const size_t lds_main = (size_t)(4 * H1_RL + 2 * H1_GL + STRIP_RING * H1_W) * 4 + 16;
    const size_t lds_tile = (size_t)(H1_W + H1_TRP) * 65 * 4 + 16;
    const size_t lds = (lds_main > lds_tile ? lds_main : lds_tile) + 32;
    return launch_strip(dag_strip1g_kernel, p, ndir * B * p.NS, H1_NT + 192, lds, st, "dag_loss_fwd(strip1g)");
}

}  // namespace dsp
