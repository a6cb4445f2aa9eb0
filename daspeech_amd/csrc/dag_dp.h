// dag_dp.h — the DP launchers of the dag_dp_*.hip files, their *_supported predicates and workspace sizes, the scratch helpers they share
// (dag_dp_banded.hip), and the backward / option setters the C ABI (capi_dag.hip) calls.  Internal: one declaration of each, so that the
// compiler checks every call against its definition.
#pragma once
#include "common.h"

namespace dsp {

// ---- scratch (dag_dp_banded.hip) ---------------------------------------------------------------------------------------------------
// The C ABI opens the caller's workspace for the calling thread (caller_ws_begin / caller_ws_end); a launcher carves 256-byte aligned
// pieces out of it (caller_ws_take: NULL = too small, the launcher then uses library scratch).  banded_acquire_ws takes
// DP_WS_COUNTERS bytes of counters + `halo_bytes` for the row hand-off of one launch.
constexpr size_t DP_WS_COUNTERS = 256;
// what a piece of n bytes costs in the caller workspace, as the workspace queries count it: rounded up to 256 + 512 of slack for the alignment
static inline size_t ws_piece(size_t n) { return ((n + 255) & ~(size_t)255) + 512; }
void caller_ws_begin(void* p, size_t n);
void caller_ws_end();
void* caller_ws_take(size_t n);
int banded_acquire_ws(hipStream_t st, size_t halo_bytes, int T, unsigned int** counters, unsigned long long** halo, unsigned int* tag_base);
void status_begin(hipStream_t st);
void status_end(hipStream_t st);
bool status_export(hipStream_t st, const unsigned int** src, unsigned int** dst);
int banded_last_error_word(hipStream_t st, unsigned int* word);

// ---- log-sum DP (dag_loss forward) ---------------------------------------------------------------------------------------------------
// rows16: every row of match / alpha / beta (alpha_max) starts on a 16-byte boundary and holds round4(L) columns (16-byte aligned pointers,
// pitches that are multiples of 4).  *_ws_bytes: the halo_bytes a launch passes to banded_acquire_ws (ndir = 2: alpha and beta).
bool strip4g_supported(int L, int TR, bool rows16);                          // dag_dp_strip4g.hip: windows <= 32, exp space
size_t strip4g_ws_bytes(int B, int T, int L, int ndir);
int launch_dag_strip4g(const float*, const float*, const int64_t*, const int64_t*, float*, float*, int, int, int, int, int, int, hipStream_t);
bool strip2g_supported(int L, int TR);                                       // dag_dp_strip2g.hip: windows 33 .. 64
size_t strip2g_ws_bytes(int B, int T, int L, int ndir);
int launch_dag_strip2g(const float*, const float*, const int64_t*, const int64_t*, float*, float*, int, int, int, int, int, int, hipStream_t);
bool strip1g_supported(int L, int TR);                                       // dag_dp_strip1g.hip: windows 65 .. 128
size_t strip1g_ws_bytes(int B, int T, int L, int ndir);
int launch_dag_strip1g(const float*, const float*, const int64_t*, const int64_t*, float*, float*, int, int, int, int, int, int, hipStream_t);
bool dense_mfma_supported(int L, int TR);                                    // dag_dp_dense_mfma.hip: dense windows on the matrix cores
size_t dense_mfma_ws_bytes(int B, int T, int L, int ndir, bool standby);
int launch_dag_dense_mfma(const float*, const float*, const int64_t*, const int64_t*, float*, float*, int, int, int, int, hipStream_t);

// ---- both DPs (mode 0: log-sum alpha / beta, mode 1: max-alpha + trace) -------------------------------------------------------------------
bool strip2_supported(int L, int TR, bool rows16);                           // dag_dp_strip2.hip: windows <= 32, log space, loader wave
size_t strip2_ws_bytes(int B, int T, int L, int ndir);
int launch_dag_strip2(int mode, const float*, const float*, const int64_t*, const int64_t*, float*, float*, int32_t*, int, int, int, int, hipStream_t);
bool banded_supported(int L, int TR);                                        // dag_dp_banded.hip: windows <= 64, log space
size_t banded_ws_bytes(int B, int T, int L, int TR, int ndir);
int launch_dag_banded(int mode, const float*, const float*, const int64_t*, const int64_t*, float*, float*, int32_t*, int, int, int, int, hipStream_t);

// ---- max-DP (dag_best_alignment) ---------------------------------------------------------------------------------------------------------
bool maxstrip_supported(int L, int TR, bool rows16);                         // dag_dp_maxstrip.hip: windows <= 32, values only + lazy back-trace
size_t maxstrip_ws_bytes(int B, int T, int L);
int launch_dag_maxstrip(const float*, const float*, const int64_t*, const int64_t*, float*, int64_t*, int, int, int, int, int, int, hipStream_t);
bool maxstripw_supported(int L, int TR);                                     // dag_dp_maxstripw.hip: windows 33 .. 128, values only
size_t maxstripw_ws_bytes(int B, int T, int L, int TR);
int launch_dag_maxstripw(const float*, const float*, const int64_t*, const int64_t*, float*, int64_t*, int, int, int, int, int, int, hipStream_t);
bool dense_max_supported(int L, int TR);                                     // dag_dp_dense_max.hip: dense windows, blocked max-plus
size_t dense_max_ws_bytes(int B, int T, int L, bool own_block_trace);
int launch_dag_dense_max(const float*, const float*, const int64_t*, const int64_t*, float*, int64_t*, int, int, int, int, hipStream_t,
                         unsigned short* block_trace = nullptr);
int launch_dag_dense_backtrace(const float*, const unsigned short*, const float*, const int64_t*, const int64_t*, int64_t*, int, int, int, int, hipStream_t);

// ---- row-sequential log-space kernels (dag_dp_generic.hip): any shape, and the stand-by behind the matrix-core DP -----------------------------
size_t links_copy_bytes(int B, int L, int TR);                               // the re-laid-out transition matrix (caller_ws_take)
size_t dense_rows_gated_bytes(int B, int L, int ndir);                       // hand-off rows of the wave-per-column kernels
bool dense_rows_gated_supported(int L);
size_t generic_fwd_ws_bytes(int B, int L, int TR, int ndir);                 // launch_dag_fwd_generic: all its pieces (ws_piece)
size_t generic_align_ws_bytes(int B, int L, int TR);                         // launch_best_alignment_generic: all its pieces
int launch_dag_fwd_generic(const float*, const float*, const int64_t*, const int64_t*, float*, float*, int, int, int, int, hipStream_t);
int launch_dag_dense_rows_gated(const float*, const float*, const int64_t*, const int64_t*, float*, float*, int, int, int, int,
                                unsigned int*, unsigned long long*, unsigned int, const unsigned int*, hipStream_t);
int launch_pick_loss(const float*, const float*, const int64_t*, const int64_t*, float*, int, int, int, int, hipStream_t);
int launch_max_alpha_generic(const float*, const float*, const int64_t*, const int64_t*, float*, int32_t*, int, int, int, int, hipStream_t);
int launch_backtrace(const int32_t*, const int64_t*, const int64_t*, int64_t*, int, int, int, hipStream_t);
int launch_best_alignment_generic(const float*, const float*, const int64_t*, const int64_t*, float*, int32_t*, int64_t*, int, int, int, int, hipStream_t);

// ---- backward (dag_grad.hip) ---------------------------------------------------------------------------------------------------------------
int launch_dag_bwd_generic(const float*, const float*, const float*, const float*, const float*, const int64_t*, const int64_t*,
                           float*, float*, int, int, int, int, int, int, int, hipStream_t);
int k5_diag(unsigned int* out);

// ---- per-thread kernel pins (dsp_dag_set_option) ---------------------------------------------------------------------------------------------
void set_k5_path(int v);          // dag_grad.hip
void set_k5_fuse(int v);
void set_dm_mt(int v);            // dag_dp_dense_mfma.hip
void set_dm_budget(int v);
void set_dx_mt(int v);            // dag_dp_dense_max.hip
void set_xl_tile(int v);          // extract_links.hip
void set_xl_mfma(int v);          // extract_links_mfma.hip
void set_xl_contract(int v);

}  // namespace dsp
