// capi_dag.hip — extern "C" entry points of the DP ops: argument checks, and the one place that decides which kernel family runs.
#include "dag_dp.h"
#include <algorithm>
#include <string.h>

namespace dsp {

struct CallerWsScope {
    hipStream_t st;
    CallerWsScope(void* p, size_t n, hipStream_t s) : st(s) { caller_ws_begin(p, n); status_begin(st); }
    ~CallerWsScope() { status_end(st); caller_ws_end(); }
};

// ---- kernel selection ----------------------------------------------------------------------------------------------------------------------
// The kernel families (one dag_dp_*.hip file each; dag_dp_generic.hip serves any shape and whatever the others do not take).  F_NONE: no
// family serves these rows / this call, the entry point says why.
enum Family { F_NONE, F_GENERIC, F_STRIP4G, F_STRIP2G, F_STRIP1G, F_STRIP2, F_BANDED, F_DENSE_MFMA, F_MAXSTRIP, F_MAXSTRIPW, F_DENSE_MAX };
static constexpr unsigned fam(Family f) { return 1u << f; }

// dsp_dag_set_option("dp_path", n) pins the families a launch of the calling THREAD may pick (a test pinning a family does not change what
// another thread's calls launch); the generic kernels serve whatever the pinned families do not take.  (3 and 6 were the strip4 / strip4h
// generations, removed in r02: like any other value they leave the generic kernels only.)
struct Pin { unsigned fwd, align; };
static Pin pin_of(int dp_path)
{
    switch (dp_path) {
    case 0: return {fam(F_STRIP4G) | fam(F_STRIP2G) | fam(F_STRIP1G) | fam(F_BANDED) | fam(F_DENSE_MFMA),          // auto
                    fam(F_MAXSTRIP) | fam(F_MAXSTRIPW) | fam(F_DENSE_MAX) | fam(F_STRIP2) | fam(F_BANDED)};
    case 2: return {fam(F_BANDED), fam(F_BANDED)};
    case 4: return {fam(F_STRIP2), fam(F_STRIP2)};
    case 5: return {fam(F_STRIP4G), 0};
    case 7: return {0, fam(F_MAXSTRIP) | fam(F_MAXSTRIPW)};
    case 8: return {fam(F_STRIP2G) | fam(F_STRIP1G), 0};
    case 9: return {fam(F_DENSE_MFMA), fam(F_DENSE_MAX)};
    default: return {0, 0};                                   // 1: the generic kernels
    }
}
static thread_local int g_path = 0;
static unsigned int g_last_fallbacks = 0;
static unsigned int g_dbg[64] = {0};

// rows16: every row starts on a 16-byte boundary and holds round4(L) columns (what the 4-columns-per-lane strips read and write)
static bool rows16(int L, int ldm, int ldo, uintptr_t ptrs)
{
    const int L4 = (L + 3) & ~3;
    return !(ldm & 3) && !(ldo & 3) && ldm >= L4 && ldo >= L4 && !(ptrs & 15);
}

// dag_loss forward.  Pitched rows (ld != L) are served by the strip families of windows <= 128 only.
static Family select_fwd(int L, int TR, bool pitched, bool rows_16)
{
    const unsigned m = pin_of(g_path).fwd;
    if ((m & fam(F_STRIP4G)) && strip4g_supported(L, TR, rows_16)) return F_STRIP4G;
    if ((m & fam(F_STRIP2G)) && strip2g_supported(L, TR)) return F_STRIP2G;
    if ((m & fam(F_STRIP1G)) && strip1g_supported(L, TR)) return F_STRIP1G;
    if (pitched) return F_NONE;
    if ((m & fam(F_STRIP2)) && strip2_supported(L, TR, rows_16)) return F_STRIP2;
    if ((m & fam(F_BANDED)) && banded_supported(L, TR)) return F_BANDED;
    if ((m & fam(F_DENSE_MFMA)) && dense_mfma_supported(L, TR)) return F_DENSE_MFMA;
    return F_GENERIC;
}

// dag_best_alignment.  Pitched rows: the values-only strips (windows <= 128).  Without a trace buffer only the values-only strips and the
// blocked max-plus kernels serve; with one, the traced strips + trace walk take windows <= 64 (the banded ones before the dense kernels on
// windows 33 .. 64: C2 at TR = 64 2.0 ms against 3.1).
static Family select_align(int L, int TR, bool pitched, bool rows_16, bool trace)
{
    const unsigned m = pin_of(g_path).align;
    if (pitched) {
        if ((m & fam(F_MAXSTRIP)) && maxstrip_supported(L, TR, rows_16)) return F_MAXSTRIP;
        if ((m & fam(F_MAXSTRIPW)) && maxstripw_supported(L, TR)) return F_MAXSTRIPW;
        return F_NONE;
    }
    if ((m & fam(F_MAXSTRIPW)) && maxstripw_supported(L, TR)) return F_MAXSTRIPW;
    const bool row_image = (size_t)L * 4 <= 160 * 1024;                      // the trace walk keeps one row of the path in LDS
    const bool traced = (m & (fam(F_STRIP2) | fam(F_BANDED))) != 0;
    const bool mid = TR > 32 && TR <= 64 && trace && (m & fam(F_BANDED)) && row_image && banded_supported(L, TR);
    if ((m & fam(F_DENSE_MAX)) && !mid && dense_max_supported(L, TR)) return F_DENSE_MAX;
    if (!trace || !traced) {                                                   // a given trace goes to the traced strips unless the pin excludes them
        if ((m & fam(F_MAXSTRIP)) && maxstrip_supported(L, TR, rows_16)) return F_MAXSTRIP;
        if (!trace) return F_NONE;
    }
    if (row_image) {
        if ((m & fam(F_STRIP2)) && strip2_supported(L, TR, rows_16)) return F_STRIP2;
        if ((m & fam(F_BANDED)) && banded_supported(L, TR)) return F_BANDED;
    }
    return F_GENERIC;
}

// ---- workspace: what the chosen family's launch takes from the caller (ws_piece per caller_ws_take / banded_acquire_ws) ---------------------------
static size_t acquired(size_t halo_bytes) { return ws_piece(DP_WS_COUNTERS + halo_bytes); }

static size_t fwd_ws_bytes(Family f, int B, int T, int L, int TR, int ndir)
{
    switch (f) {
    case F_STRIP4G: return acquired(strip4g_ws_bytes(B, T, L, ndir));
    case F_STRIP2G: return acquired(strip2g_ws_bytes(B, T, L, ndir));
    case F_STRIP1G: return acquired(strip1g_ws_bytes(B, T, L, ndir));
    case F_STRIP2: return acquired(strip2_ws_bytes(B, T, L, ndir));
    case F_BANDED: return acquired(banded_ws_bytes(B, T, L, TR, ndir));
    case F_DENSE_MFMA:                          // + the stand-by log-space kernels' hand-off rows and their copy of the transition matrix
        return acquired(dense_mfma_ws_bytes(B, T, L, ndir, true)) + ws_piece(links_copy_bytes(B, L, TR));
    case F_GENERIC: return generic_fwd_ws_bytes(B, L, TR, ndir);
    default: return 0;
    }
}

static size_t align_ws_bytes(Family f, int B, int T, int L, int TR)
{
    switch (f) {
    case F_MAXSTRIP: return acquired(maxstrip_ws_bytes(B, T, L));
    case F_MAXSTRIPW: return acquired(maxstripw_ws_bytes(B, T, L, TR));
    case F_DENSE_MAX: return acquired(dense_max_ws_bytes(B, T, L, true));
    case F_STRIP2: return acquired(strip2_ws_bytes(B, T, L, 1));
    case F_BANDED: return acquired(banded_ws_bytes(B, T, L, TR, 1));
    case F_GENERIC: return generic_align_ws_bytes(B, L, TR);
    default: return 0;
    }
}

static int check_dims(const char* fn, int B, int T, int L, int TR) {
    if (B < 0 || T < 1 || L < 1 || TR < 1) { set_error("%s: bad sizes B=%d T=%d L=%d TR=%d", fn, B, T, L, TR); return DSP_EINVAL; }
    return DSP_OK;
}
}  // namespace dsp

using namespace dsp;

// The largest take of the families the selection may return for this shape under the calling thread's pin: dense or pitched rows (a pitched
// caller asks with L rounded up to 4; 16-byte aligned bases), alpha and / or beta.
extern "C" size_t dsp_dag_workspace_bytes(int B, int T, int L, int TR)
{
    if (B <= 0 || T <= 0 || L <= 0 || TR <= 0) return 0;
    size_t n = 0;
    for (const bool pitched : {false, true})
        for (int ndir = 1; ndir <= 2; ++ndir)
            n = std::max(n, fwd_ws_bytes(select_fwd(L, TR, pitched, pitched || !(L & 3)), B, T, L, TR, ndir));
    return n;
}

// ... and of the alignment (dsp_dag_best_alignment_ws / _ld), with and without a trace buffer.
extern "C" size_t dsp_dag_alignment_workspace_bytes(int B, int T, int L, int TR)
{
    if (B <= 0 || T <= 0 || L <= 0 || TR <= 0) return 0;
    size_t n = 0;
    for (const bool pitched : {false, true})
        for (const bool trace : {false, true})
            n = std::max(n, align_ws_bytes(select_align(L, TR, pitched, pitched || !(L & 3), trace), B, T, L, TR));
    return n;
}

// Row pitches (r06, ABI 2): ld_match / ld_ab are the distances in ELEMENTS between consecutive target rows of match and of alpha / beta
// (batch stride = T * ld).  Dense tensors have ld = L (dsp_dag_loss_fwd).  A graph whose length is not a multiple of 4 — three in four are —
// keeps its rows on 16-byte boundaries by a pitch rounded up to 4: the strip kernels (windows <= 128) then serve it without a padded copy
// (dag_logsoftmax_gather_inplace writes `match` with such a pitch itself).  The other kernel families take dense tensors only.
static int check_ld(const char* fn, int L, int ld_match, int ld_ab)
{
    if (ld_match < L || ld_ab < L) { set_error("%s: row pitch smaller than L (ld_match=%d ld_ab=%d L=%d)", fn, ld_match, ld_ab, L); return DSP_EINVAL; }
    return DSP_OK;
}

extern "C" int dsp_dag_loss_fwd_ld(const float* match, int ld_match, const float* links, const int64_t* out_len, const int64_t* tgt_len,
                                   float* alpha, float* beta, int ld_ab, float* loss, int B, int T, int L, int TR,
                                   void* workspace, size_t workspace_bytes, dsp_stream_t stream)
{
    CallerWsScope ws_scope(workspace, workspace_bytes, as_stream(stream));
    int rc = check_dims("dag_loss_fwd", B, T, L, TR);
    if (rc) return rc;
    if (B == 0) return DSP_OK;
    if (!match || !links || !out_len || !tgt_len || (!alpha && !beta)) { set_error("dag_loss_fwd: null pointer"); return DSP_EINVAL; }
    if ((rc = check_ld("dag_loss_fwd", L, ld_match, ld_ab))) return rc;
    hipStream_t st = as_stream(stream);
    const bool pitched = ld_match != L || ld_ab != L;
    switch (select_fwd(L, TR, pitched, rows16(L, ld_match, ld_ab, (uintptr_t)match | (uintptr_t)alpha | (uintptr_t)beta))) {
    case F_STRIP4G: rc = launch_dag_strip4g(match, links, out_len, tgt_len, alpha, beta, B, T, L, TR, ld_match, ld_ab, st); break;
    case F_STRIP2G: rc = launch_dag_strip2g(match, links, out_len, tgt_len, alpha, beta, B, T, L, TR, ld_match, ld_ab, st); break;
    case F_STRIP1G: rc = launch_dag_strip1g(match, links, out_len, tgt_len, alpha, beta, B, T, L, TR, ld_match, ld_ab, st); break;
    case F_STRIP2: rc = launch_dag_strip2(0, match, links, out_len, tgt_len, alpha, beta, nullptr, B, T, L, TR, st); break;
    case F_BANDED: rc = launch_dag_banded(0, match, links, out_len, tgt_len, alpha, beta, nullptr, B, T, L, TR, st); break;
    case F_DENSE_MFMA: rc = launch_dag_dense_mfma(match, links, out_len, tgt_len, alpha, beta, B, T, L, TR, st); break;
    case F_GENERIC: rc = launch_dag_fwd_generic(match, links, out_len, tgt_len, alpha, beta, B, T, L, TR, st); break;
    default:
        set_error("dag_loss_fwd: pitched rows (ld_match=%d ld_ab=%d, L=%d) are served by the strip kernels of windows <= 128 only (TR <= 32: 16-byte "
                  "aligned pointers, pitches that are multiples of 4); TR=%d / this kernel pin needs dense tensors", ld_match, ld_ab, L, TR);
        return DSP_EINVAL;
    }
    if (rc) return rc;
    if (loss) rc = launch_pick_loss(alpha, beta, out_len, tgt_len, loss, B, T, L, ld_ab, st);
    return rc;
}

extern "C" int dsp_dag_loss_fwd(const float* match, const float* links, const int64_t* out_len, const int64_t* tgt_len,
                                float* alpha, float* beta, float* loss, int B, int T, int L, int TR,
                                void* workspace, size_t workspace_bytes, dsp_stream_t stream)
{
    return dsp_dag_loss_fwd_ld(match, L, links, out_len, tgt_len, alpha, beta, L, loss, B, T, L, TR, workspace, workspace_bytes, stream);
}

extern "C" int dsp_dag_loss_bwd_ld(const float* grad_out, const float* alpha, const float* beta, int ld_ab, const float* match, int ld_match,
                                   const float* links, const int64_t* out_len, const int64_t* tgt_len,
                                   float* grad_match, int ld_grad_match, float* grad_links, int B, int T, int L, int TR,
                                   void* workspace, size_t workspace_bytes, dsp_stream_t stream)
{
    (void)workspace; (void)workspace_bytes;
    int rc = check_dims("dag_loss_bwd", B, T, L, TR);
    if (rc) return rc;
    if (B == 0) return DSP_OK;
    if (!grad_out || !alpha || !beta || !match || !links || !out_len || !tgt_len) { set_error("dag_loss_bwd: null pointer"); return DSP_EINVAL; }
    if ((rc = check_ld("dag_loss_bwd", L, ld_match, ld_ab))) return rc;
    if (grad_match && ld_grad_match < L) { set_error("dag_loss_bwd: ld_grad_match=%d smaller than L=%d", ld_grad_match, L); return DSP_EINVAL; }
    if (ld_ab != L && TR > 128) { set_error("dag_loss_bwd: pitched alpha / beta are served for TR <= 128 only (TR=%d)", TR); return DSP_EINVAL; }
    return launch_dag_bwd_generic(grad_out, alpha, beta, match, links, out_len, tgt_len, grad_match, grad_links, B, T, L, TR,
                                  ld_ab, ld_match, grad_match ? ld_grad_match : L, as_stream(stream));
}

extern "C" int dsp_dag_loss_bwd(const float* grad_out, const float* alpha, const float* beta, const float* match,
                                const float* links, const int64_t* out_len, const int64_t* tgt_len,
                                float* grad_match, float* grad_links, int B, int T, int L, int TR,
                                void* workspace, size_t workspace_bytes, dsp_stream_t stream)
{
    return dsp_dag_loss_bwd_ld(grad_out, alpha, beta, L, match, L, links, out_len, tgt_len, grad_match, L, grad_links, B, T, L, TR,
                               workspace, workspace_bytes, stream);
}

static int best_alignment_impl(const float* match, const float* links, const int64_t* out_len, const int64_t* tgt_len,
                               float* alpha_max, int32_t* trace, int64_t* path, int B, int T, int L, int TR, dsp_stream_t stream,
                               int ld_match = 0, int ld_am = 0);

extern "C" int dsp_dag_best_alignment(const float* match, const float* links, const int64_t* out_len, const int64_t* tgt_len,
                                      float* alpha_max, int32_t* trace, int64_t* path, int B, int T, int L, int TR,
                                      dsp_stream_t stream)
{
    CallerWsScope ws_scope(nullptr, 0, as_stream(stream));                                                       // library scratch
    return best_alignment_impl(match, links, out_len, tgt_len, alpha_max, trace, path, B, T, L, TR, stream);
}

extern "C" int dsp_dag_best_alignment_ws(const float* match, const float* links, const int64_t* out_len, const int64_t* tgt_len,
                                         float* alpha_max, int32_t* trace, int64_t* path, int B, int T, int L, int TR,
                                         void* workspace, size_t workspace_bytes, dsp_stream_t stream)
{
    CallerWsScope ws_scope(workspace, workspace_bytes, as_stream(stream));
    return best_alignment_impl(match, links, out_len, tgt_len, alpha_max, trace, path, B, T, L, TR, stream);
}

// ... with row pitches (see dsp_dag_loss_fwd_ld): ld_match / ld_am = elements between consecutive rows of match / alpha_max.  Pitched rows are
// served by the values-only strip DP + back-trace (windows <= 128, no trace tensor); `trace` must be dense ([B,T,L]) if given and is left untouched.
extern "C" int dsp_dag_best_alignment_ld(const float* match, int ld_match, const float* links, const int64_t* out_len, const int64_t* tgt_len,
                                         float* alpha_max, int ld_am, int32_t* trace, int64_t* path, int B, int T, int L, int TR,
                                         void* workspace, size_t workspace_bytes, dsp_stream_t stream)
{
    CallerWsScope ws_scope(workspace, workspace_bytes, as_stream(stream));
    return best_alignment_impl(match, links, out_len, tgt_len, alpha_max, trace, path, B, T, L, TR, stream, ld_match, ld_am);
}

static int best_alignment_impl(const float* match, const float* links, const int64_t* out_len, const int64_t* tgt_len,
                               float* alpha_max, int32_t* trace, int64_t* path, int B, int T, int L, int TR, dsp_stream_t stream,
                               int ld_match, int ld_am)
{
    int rc = check_dims("dag_best_alignment", B, T, L, TR);
    if (rc) return rc;
    if (B == 0) return DSP_OK;
    if (!match || !links || !out_len || !tgt_len || !alpha_max || !path) { set_error("dag_best_alignment: null pointer"); return DSP_EINVAL; }
    hipStream_t st = as_stream(stream);
    if (ld_match == 0) ld_match = L;
    if (ld_am == 0) ld_am = L;
    if ((rc = check_ld("dag_best_alignment", L, ld_match, ld_am))) return rc;
    const bool pitched = ld_match != L || ld_am != L;
    // (a trace buffer is dense and only the traced kernels write it: its alignment counts on dense rows only)
    const uintptr_t ptrs = (uintptr_t)match | (uintptr_t)alpha_max | (pitched ? 0 : (uintptr_t)trace);
    switch (select_align(L, TR, pitched, rows16(L, ld_match, ld_am, ptrs), trace != nullptr)) {
    case F_MAXSTRIP: return launch_dag_maxstrip(match, links, out_len, tgt_len, alpha_max, path, B, T, L, TR, ld_match, ld_am, st);
    case F_MAXSTRIPW: return launch_dag_maxstripw(match, links, out_len, tgt_len, alpha_max, path, B, T, L, TR, ld_match, ld_am, st);
    case F_DENSE_MAX: return launch_dag_dense_max(match, links, out_len, tgt_len, alpha_max, path, B, T, L, TR, st);
    case F_STRIP2:
        if ((rc = launch_dag_strip2(1, match, links, out_len, tgt_len, alpha_max, nullptr, trace, B, T, L, TR, st))) return rc;
        return launch_backtrace(trace, out_len, tgt_len, path, B, T, L, st);
    case F_BANDED:
        if ((rc = launch_dag_banded(1, match, links, out_len, tgt_len, alpha_max, nullptr, trace, B, T, L, TR, st))) return rc;
        return launch_backtrace(trace, out_len, tgt_len, path, B, T, L, st);
    case F_GENERIC: return launch_best_alignment_generic(match, links, out_len, tgt_len, alpha_max, trace, path, B, T, L, TR, st);
    default:
        if (pitched)
            set_error("dag_best_alignment: pitched rows (ld_match=%d ld_alpha_max=%d, L=%d) are served by the strip kernels of windows <= 128 only "
                      "(TR <= 32: L <= 8192, 16-byte aligned pointers, pitches that are multiples of 4)", ld_match, ld_am, L);
        else
            set_error("dag_best_alignment: this shape / kernel family needs a trace buffer (see dsp_dag_alignment_trace_optional)");
        return DSP_EINVAL;
    }
}

extern "C" int dsp_dag_max_alpha(const float* match, const float* links, const int64_t* out_len, const int64_t* tgt_len,
                                 float* alpha_max, int32_t* trace, int B, int T, int L, int TR, dsp_stream_t stream)
{
    int rc = check_dims("dag_max_alpha", B, T, L, TR);
    if (rc) return rc;
    if (B == 0) return DSP_OK;
    if (!match || !links || !out_len || !tgt_len || !alpha_max || !trace) { set_error("dag_max_alpha: null pointer"); return DSP_EINVAL; }
    CallerWsScope ws_scope(nullptr, 0, as_stream(stream));
    return launch_max_alpha_generic(match, links, out_len, tgt_len, alpha_max, trace, B, T, L, TR, as_stream(stream));
}

extern "C" int dsp_dag_backtrace(const int32_t* trace, const int64_t* out_len, const int64_t* tgt_len, int64_t* path, int B, int T, int L,
                                 dsp_stream_t stream)
{
    if (B < 0 || T < 1 || L < 1) { set_error("dag_backtrace: bad sizes"); return DSP_EINVAL; }
    if (B == 0) return DSP_OK;
    if (!trace || !out_len || !tgt_len || !path) { set_error("dag_backtrace: null pointer"); return DSP_EINVAL; }
    return launch_backtrace(trace, out_len, tgt_len, path, B, T, L, as_stream(stream));
}

// The same two halves on the dense-window kernels (blocked max-plus DP, 2-byte block trace, back-trace that recomputes the arg-max of the cells
// it visits): what the Viterbi graph decode runs when the window is wider than 32 (the model's default: --max-transition-length 99999).
extern "C" int dsp_dag_max_alpha_blocks_supported(int L, int TR) { return ((pin_of(g_path).align & fam(F_DENSE_MAX)) && dense_max_supported(L, TR)) ? 1 : 0; }

extern "C" int dsp_dag_max_alpha_blocks(const float* match, const float* links, const int64_t* out_len, const int64_t* tgt_len,
                                        float* alpha_max, uint16_t* block_trace, int B, int T, int L, int TR, dsp_stream_t stream)
{
    int rc = check_dims("dag_max_alpha_blocks", B, T, L, TR);
    if (rc) return rc;
    if (B == 0) return DSP_OK;
    if (!match || !links || !out_len || !tgt_len || !alpha_max || !block_trace) { set_error("dag_max_alpha_blocks: null pointer"); return DSP_EINVAL; }
    if (!dense_max_supported(L, TR)) { set_error("dag_max_alpha_blocks: L=%d TR=%d is not a dense-window shape (see dsp_dag_max_alpha_blocks_supported)", L, TR); return DSP_EINVAL; }
    CallerWsScope ws_scope(nullptr, 0, as_stream(stream));
    return launch_dag_dense_max(match, links, out_len, tgt_len, alpha_max, nullptr, B, T, L, TR, as_stream(stream), block_trace);
}

extern "C" int dsp_dag_backtrace_blocks(const float* alpha_max, const uint16_t* block_trace, const float* links, const int64_t* out_len,
                                        const int64_t* tgt_len, int64_t* path, int B, int T, int L, int TR, dsp_stream_t stream)
{
    int rc = check_dims("dag_backtrace_blocks", B, T, L, TR);
    if (rc) return rc;
    if (B == 0) return DSP_OK;
    if (!alpha_max || !block_trace || !links || !out_len || !tgt_len || !path) { set_error("dag_backtrace_blocks: null pointer"); return DSP_EINVAL; }
    if (!dense_max_supported(L, TR)) { set_error("dag_backtrace_blocks: L=%d TR=%d is not a dense-window shape", L, TR); return DSP_EINVAL; }
    return launch_dag_dense_backtrace(alpha_max, block_trace, links, out_len, tgt_len, path, B, T, L, TR, as_stream(stream));
}

// May the caller hand this op PITCHED rows (dsp_dag_loss_fwd_ld / _bwd_ld: op 0, dsp_dag_best_alignment_ld: op 1) for a graph of L vertices?  Only
// the strip families (windows <= 128) take them, so the answer follows the calling thread's dp_path pin like the dispatch itself does.
extern "C" int dsp_dag_pitch_supported(int op, int L, int TR)
{
    if (L < 1) return 0;
    return (op == 0 ? select_fwd(L, TR, true, true) : select_align(L, TR, true, true, false)) != F_NONE ? 1 : 0;
}

extern "C" int dsp_dag_alignment_trace_optional(int L, int TR)
{
    return select_align(L, TR, false, !(L & 3), false) != F_NONE ? 1 : 0;
}

static void set_dp_path(int v) { g_path = v; }
static const struct { const char* name; void (*set)(int); } k_options[] = {
    {"dp_path", set_dp_path}, {"k5_path", set_k5_path}, {"k5_fuse", set_k5_fuse}, {"dm_mt", set_dm_mt}, {"dm_budget", set_dm_budget},
    {"dx_mt", set_dx_mt}, {"xl_tile", set_xl_tile}, {"xl_mfma", set_xl_mfma}, {"xl_contract", set_xl_contract},
};

extern "C" int dsp_dag_set_option(const char* name, int value)
{
    for (const auto& o : k_options)
        if (name && !strcmp(name, o.name)) { o.set(value); return DSP_OK; }
    set_error("dsp_dag_set_option: unknown option");
    return DSP_EINVAL;
}

extern "C" int dsp_dag_last_launch_status(dsp_stream_t stream, unsigned int* host_word)
{
    if (!host_word) { set_error("dsp_dag_last_launch_status: null pointer"); return DSP_EINVAL; }
    int rc = banded_last_error_word(as_stream(stream), g_dbg);
    host_word[0] = g_dbg[0];
    g_last_fallbacks = g_dbg[1];
    return rc;
}

extern "C" int dsp_dag_debug_k5(unsigned int* out4) { return out4 ? k5_diag(out4) : DSP_EINVAL; }

extern "C" const unsigned int* dsp_dag_debug_words(void) { return g_dbg; }

extern "C" unsigned int dsp_dag_last_fallback_count(void) { return g_last_fallbacks; }
