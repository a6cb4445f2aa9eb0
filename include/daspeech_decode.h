/* daspeech_decode.h — C ABI of the inference-side steps of the DASpeech hot path (libdaspeech_hip.so).
 *
 * These entry points replace Python / torch code of the reference that runs on the host or as chains of small torch ops:
 *   graph decode (lookahead / greedy)   DASpeech/models/s2s_conformer_dag_fastspeech2.py:201-243   (F2, F3 in SURVEY.md §2.3)
 *   posterior of the "expect" strategy   DASpeech/criterions/s2s_dag_fastspeech2_loss.py:259-261     (F1)
 *   variance-adaptor glue               fairseq/fairseq/models/text_to_speech/fastspeech2.py:169-210 (F6)
 *   length regulator                    fairseq/fairseq/models/text_to_speech/fastspeech2.py:98-114  (F7)
 * Conventions as in daspeech_dag.h (device pointers, caller-allocated outputs, hipStream_t as void*, int return codes). */
#ifndef DASPEECH_DECODE_H
#define DASPEECH_DECODE_H

#include "daspeech_dag.h"

#ifdef __cplusplus
extern "C" {
#endif

/* F2a  per-vertex argmax token and its log-probability            (s2s_conformer_dag_fastspeech2.py:207-208)
 *   logits [B,L,V] (dtype code as in daspeech_dag.h, read only); tok [B,L] int32 = argmax_v (first maximum);
 *   score [B,L] fp32 = max_v log_softmax(logits) = -log sum_v exp(x_v - max). */
int dsp_argmax_logp(const void* logits, int dtype, int32_t* tok, float* score, int B, int L, int V, dsp_stream_t stream);

/* F2b  best successor of every vertex on the COMPACT links layout  (:209-217; replaces restore_valid_links + dense argmax)
 *   links [B,L,TR] fp32; score [B,L] fp32 (ignored when greedy != 0); next[b,i] = argmax_j (links[b,i,j-i-1] + score[b,j]*beta)
 *   with the dense row's tie rule: first maximum = smallest j; a row without any finite entry gives 0. */
int dsp_lookahead_next(const float* links, const float* score, float beta, int greedy, int32_t* next,
                       int B, int L, int TR, dsp_stream_t stream);

/* F3a  follow the path 0 -> ... -> L_b-1, collapse repeats, drop pads        (:219-233)
 *   out_tokens [B,cap] int64 (pad-filled; [b,0] = token of vertex 0), keep_idx [B,cap] int32 = vertex of each kept non-bos
 *   token (-1 padded), n_feat [B] int32 = number of kept non-bos tokens. cap >= L is always enough. */
int dsp_follow_path(const int32_t* next, const int32_t* tok, const int64_t* out_len, int pad,
                    int64_t* out_tokens, int32_t* keep_idx, int32_t* n_feat, int B, int L, int cap, dsp_stream_t stream);

/* F3a' the token pass of the viterbi / jointviterbi strategies                 (s2s_conformer_dag_fastspeech2.py:283-299)
 *   path [B,L] int64 (DP row of every vertex on the back-traced chain, -1 elsewhere: dsp_dag_backtrace / dsp_dag_backtrace_blocks),
 *   pred_length [B] int64 (chosen length), unreachable [B] uint8 (no length reaches the final vertex: the token of vertex 0 is emitted,
 *   as the reference does), tok [B,L] int32.  Visited = DP rows 1 .. pred_length, graph order; a token is kept if it is the last visited
 *   one, or not <pad> and different from the next visited token.  out_tokens [B,cap] int64 (pad-filled), keep_idx [B,cap] int32 (vertex of
 *   each kept token, -1 padded: the index list of dsp_gather_rows), n_keep [B] int32. */
int dsp_viterbi_collect(const int64_t* path, const int64_t* pred_length, const unsigned char* unreachable, const int32_t* tok, int pad,
                        int64_t* out_tokens, int32_t* keep_idx, int32_t* n_keep, int B, int L, int cap, dsp_stream_t stream);

/* F3b  gather the decoder states of the kept vertices, zero padded            (:232,234,241; _collate_frames)
 *   features [B,L,D] (dtype code), keep_idx [B,cap]; out [B,Fmax,D] same dtype: out[b,k] = features[b,keep_idx[b,k]] for
 *   k < n_feat[b], 0 after.  Pure copy: bit-exact. */
int dsp_gather_rows(const void* features, int dtype, const int32_t* keep_idx, const int32_t* n_feat, void* out,
                    int B, int L, int D, int cap, int Fmax, dsp_stream_t stream);

/* F0   transition log-probabilities of the graph, compact layout             (DAGDecoder.extract_links, s2t_conformer_dag.py:171-212)
 *   q, k [B,L,H,CK] fp32, CK = 32, 64 or 128 (query_linear / key_linear of [features ; link positional embedding], H = 8 heads),
 *   log_gates [B,L,H] fp32 (log_softmax of gate_linear), out_len [B] int64, dist_bias [TR] fp32 or NULL (benchmark calibration),
 *   scale = 1/sqrt(CK).  links[b,i,d] = logsumexp_h( log_softmax_d(q_i.k_{i+d+1} * scale, over valid successors) + log_gates[b,i,h] ),
 *   -inf where i+d+1 >= out_len[b] or >= L; rows without a successor are all -inf.  Only the band is computed — the reference's
 *   [B,L,L,H] content tensor and its gather (:183-196) never exist.  Inference path (no gradient).
 *   Any TR up to L-1: windows whose [4 vertices][TR][8 heads] score image exceeds LDS (TR above ~1100) are walked in tiles of 512 successors
 *   (online soft-max state in a first pass, per-tile emission in a second); the same holds for the two training entry points below. */
int dsp_extract_links(const float* q, const float* k, const float* log_gates, const int64_t* out_len,
                      const float* dist_bias, float* links, int B, int L, int H, int CK, int TR, float scale,
                      dsp_stream_t stream);
/* The TRAINING side of F0 (the step in front of dag_loss: s2t_conformer_dag.py:171-212 under autograd), still on the compact band only:
 *   dsp_extract_links_train   the same forward, additionally writing `stats` [B,L,H,2] = (window maximum, log of the window's sum of
 *                             exp(score - maximum)) per source vertex and head — all the state the backward needs besides q, k, links;
 *   dsp_extract_links_bwd     grad_links [B,L,TR] (entries of -inf links are ignored) -> grad_q, grad_k [B,L,H,CK], grad_log_gates [B,L,H].
 *                             Scores are recomputed per 4-vertex tile, d(score) lives in LDS only: no [B,L,L,H] tensor in either direction. */
int dsp_extract_links_train(const float* q, const float* k, const float* log_gates, const int64_t* out_len,
                            const float* dist_bias, float* links, float* stats, int B, int L, int H, int CK, int TR, float scale,
                            dsp_stream_t stream);
int dsp_extract_links_bwd(const float* q, const float* k, const float* log_gates, const int64_t* out_len, const float* dist_bias,
                          const float* links, const float* grad_links, const float* stats,
                          float* grad_q, float* grad_k, float* grad_log_gates, int B, int L, int H, int CK, int TR, float scale,
                          dsp_stream_t stream);

/* F0 on the matrix cores (r05; csrc/extract_links_mfma.hip): the same three operators for the released link predictor (H = 8, CK = 64), scores as
 *   32 x 32 blocks on the fp16 matrix cores with fp32 accuracy (operands split hi + lo 2^-11, three MFMAs per product), the backward's
 *   contractions on the fp32 matrix-core path; they need a scratch buffer the caller owns (the split k / q rows in MFMA fragment order):
 *   dsp_extract_links_workspace  bytes for one call (phase 0 = inference forward, 1 = training forward, 2 = backward); 0 bytes = this shape is
 *                                served by the entry points above (other head widths, short graphs / narrow windows — or option "xl_mfma" 0;
 *                                "xl_mfma" 1 forces the matrix-core kernels wherever H = 8, CK = 64);
 *   dsp_extract_links_ws         dsp_extract_links (stats = NULL) / dsp_extract_links_train (stats [B,L,H,2]) — same outputs, same `stats`;
 *   dsp_extract_links_bwd_ws     dsp_extract_links_bwd.
 *   Operand range: the split keeps k and q * scale * log2(e) as fp16 pairs — finite for |k|, |q| * 0.18 < 65 504 (the link predictor's
 *   projections are O(1..10)); beyond that the scores become inf / NaN where the fp32-FMA entry points above still work.
 *   B = 32, L = 4096, TR = L-1 (BASELINE's graph with the README's --max-transition-length 99999): see DESIGN.md §8 for the measured times. */
int dsp_extract_links_workspace(int B, int L, int H, int CK, int TR, int phase, size_t* bytes);
int dsp_extract_links_ws(const float* q, const float* k, const float* log_gates, const int64_t* out_len, const float* dist_bias,
                         float* links, float* stats, int B, int L, int H, int CK, int TR, float scale,
                         void* workspace, size_t workspace_bytes, dsp_stream_t stream);
int dsp_extract_links_bwd_ws(const float* q, const float* k, const float* log_gates, const int64_t* out_len, const float* dist_bias,
                             const float* links, const float* grad_links, const float* stats,
                             float* grad_q, float* grad_k, float* grad_log_gates, int B, int L, int H, int CK, int TR, float scale,
                             void* workspace, size_t workspace_bytes, dsp_stream_t stream);

/* F0 for DOUBLE q / k / log_gates (csrc/extract_links_f64.hip): the same forward (stats = NULL: inference, else the training forward writing
 *   stats [B,L,H,2]) and backward as dsp_extract_links / _train / _bwd with every tensor a contiguous double — q, k [B,L,H,CK], log_gates
 *   [B,L,H], dist_bias [TR] or NULL, links / grad_links [B,L,TR], stats [B,L,H,2] = (window maximum, log of the window's sum of exp(score -
 *   maximum)), (-inf, 0) for a row without a successor.  Every intermediate is a double (dot-product accumulators, shuffles, the LDS score
 *   image), accurate exp / log only, products on v_fma_f64.  H = 8, CK = 32, 64 or 128, 1 <= TR <= L-1: a window of up to 381 successors is one
 *   LDS tile per 4-vertex workgroup, a wider one is walked in tiles of 384 (online soft-max state first, emission second).  No [B,L,L,H] tensor
 *   in either direction and no workspace: the backward recomputes the scores, and every k row gathers over its <= TR predecessors — no
 *   floating-point atomics, two calls on the same tensors give the same bits.  The backward writes EVERY element of grad_q, grad_k and
 *   grad_log_gates (rows at or beyond the graph: zeros); entries of grad_links under -inf links are ignored.  q, k, grad_q, grad_k 16-byte
 *   aligned.  Null pointers, H != 8, another CK, TR < 1 or TR > L-1: DSP_EINVAL (dsp_last_error says which) before any launch; B == 0: DSP_OK
 *   without a launch.  The ground truth of the fp32 and matrix-core kernels above that fits on the device, and the first operator of the
 *   double chain links -> dsp_dag_loss_fwd_f64 -> backward.  Measured times: DESIGN.md §7. */
int dsp_extract_links_f64(const double* q, const double* k, const double* log_gates, const int64_t* out_len,
                          const double* dist_bias, double* links, double* stats, int B, int L, int H, int CK, int TR, double scale,
                          dsp_stream_t stream);
int dsp_extract_links_bwd_f64(const double* q, const double* k, const double* log_gates, const int64_t* out_len, const double* dist_bias,
                              const double* links, const double* grad_links, const double* stats,
                              double* grad_q, double* grad_k, double* grad_log_gates, int B, int L, int H, int CK, int TR, double scale,
                              dsp_stream_t stream);

/* diagnostics (r06): the extract_links kernel families launched by this process since the last call (then cleared) — bit 0 one-image forward,
 *   1 tiled forward, 2 matrix-core forward, 3 one-image backward, 4 tiled backward, 5 matrix-core backward with exact-fp32 contractions,
 *   6 matrix-core backward with bf16-triple contractions, 7 double forward (dsp_extract_links_f64), 8 double backward
 *   (dsp_extract_links_bwd_f64), 9 a double launch walked its window in more than one tile.  The "xl_tile" / "xl_mfma" / "xl_contract" options
 *   (fp32 families only) are PROCESS-wide (PyTorch runs an autograd backward on its own worker thread); tests assert through this word that the
 *   family they pinned is the one that ran. */
unsigned int dsp_extract_links_debug_ran(void);
/* RANGE of the matrix-core kernels (dsp_extract_links_ws / _bwd_ws): operands are split into fp16 hi / lo pieces, so |k| and |q| * scale * log2(e)
 *   must stay under 65 000 (link-predictor inputs are projections of layer-normed features: |x| ~ 1-10).  A larger operand is clamped — the call
 *   returns finite, wrong values for it — and raises a device flag; this call returns the flag (1 = some operand was clamped since the last call)
 *   and clears it.  It synchronises the device: for tests and debugging.  The fp32-FMA kernels (dsp_extract_links, "xl_mfma" 0) have no limit. */
unsigned int dsp_extract_links_debug_range(void);

/* F1   posterior of the forward-backward pass                                  (s2s_dag_fastspeech2_loss.py:259-261)
 *   score[b,t,:] = exp(alpha+beta - logsumexp_j(alpha+beta)), NaN -> 0 (rows without any finite entry). fp32 [B,T,L]. */
int dsp_posterior(const float* alpha, const float* beta, float* score, int B, int T, int L, dsp_stream_t stream);
/* F1 fused with its consumer (:259-262): out[b,t,:] = sum_j score[b,t,j] * features[b,j,:] without the [B,T,L] score tensor.
 *   features [B,L,D], out [B,T,D] fp32 (D even), lse [B,T] (row log-sum-exp of alpha+beta; -inf for rows without a finite entry,
 *   whose output is 0) or NULL.  dsp_posterior_features_bwd: grad_features[b,j,:] = sum_t score[b,t,j] * grad_out[b,t,:], the
 *   score rebuilt from alpha, beta and lse (alpha / beta carry no gradient: the reference detaches them, dag_loss.py:180-186). */
int dsp_posterior_features(const float* alpha, const float* beta, const float* features, float* out, float* lse,
                           int B, int T, int L, int D, dsp_stream_t stream);
int dsp_posterior_features_bwd(const float* alpha, const float* beta, const float* lse, const float* grad_out, float* grad_features,
                               int B, int T, int L, int D, dsp_stream_t stream);
/* F1 for DOUBLE alpha / beta (csrc/posterior_f64.hip): the reference computes the posterior in the dtype of alpha, so the float64 pair of
 *   dsp_dag_loss_fwd_f64 gives a float64 score; every intermediate is a double, accurate exp / log only.  Same semantics as the three fp32
 *   entry points above (dead rows: score and out 0, lse -inf; lse may be NULL in dsp_posterior_features_f64; no gradient to alpha / beta),
 *   wider envelope: any T, L, D >= 1 (odd D and D = 1 included) — L and T are walked in chunks, nothing row-sized lives in LDS.  features
 *   [B,L,D], out / grad_out [B,T,D], grad_features [B,L,D], lse [B,T], all double and contiguous.  No floating-point atomics: two calls on
 *   the same tensors give the same bits.  Bad sizes / null pointers: DSP_EINVAL; B == 0: DSP_OK without a launch. */
int dsp_posterior_f64(const double* alpha, const double* beta, double* score, int B, int T, int L, dsp_stream_t stream);
int dsp_posterior_features_f64(const double* alpha, const double* beta, const double* features, double* out, double* lse,
                               int B, int T, int L, int D, dsp_stream_t stream);
int dsp_posterior_features_bwd_f64(const double* alpha, const double* beta, const double* lse, const double* grad_out,
                                   double* grad_features, int B, int T, int L, int D, dsp_stream_t stream);

/* F6a predicted durations                                                     (fastspeech2.py:202-205)
 *   dur = clamp(round((exp(log_dur) - 1) * factor), 0) as int64, 0 where pad_mask != 0 (uint8/bool). */
int dsp_durations(const float* log_dur, const uint8_t* pad_mask, float factor, int64_t* dur, int64_t n, dsp_stream_t stream);

/* F6b  x += Embedding[bucketize(v, bins)]                                      (fastspeech2.py:169-177,207-210)
 *   x [n,C] fp32 in/out, v [n] fp32, bins [nb] fp32 ascending (torch.bucketize right=False), emb [nb+1,C] fp32. */
int dsp_bucketize_embed_add(float* x, const float* v, const float* bins, int nb, const float* emb, int64_t n, int C,
                            dsp_stream_t stream);

/* F7   length regulator                                                        (fastspeech2.py:98-114)
 *   step 1: dsp_length_regulator_lens  : out_lens[b] = sum_t dur[b,t]; cum [B,N] int64 scratch = inclusive prefix sums.
 *   step 2: dsp_length_regulator_expand: out [B,maxlen,C] (dtype code) = rows of x [B,N,C] repeated dur times, zero padded.
 *   The caller reads max(out_lens) between the two (the output shape depends on it; the reference syncs B*N times). */
int dsp_length_regulator_lens(const int64_t* dur, int64_t* cum, int64_t* out_lens, int B, int N, dsp_stream_t stream);
int dsp_length_regulator_expand(const void* x, int dtype, const int64_t* cum, void* out, int B, int N, int C, int maxlen,
                                dsp_stream_t stream);

/* F6b', F7'  the variance-adaptor glue under autograd (csrc/tts_glue_grad.hip).  x / emb / out / grad tensors share one dtype code (DSP_F32 /
 *   DSP_F16 / DSP_BF16); every sum is accumulated in fp32 and rounded once to that dtype; every output element is written.  Both gradients
 *   add the rows that share a destination in ASCENDING source order, one wave per destination, without float atomics: the same inputs give
 *   the same bits on every run, whatever the grid's schedule.
 *
 *   dsp_bucketize_embed_add_fwd: out [n,C] = x [n,C] + emb[idx[r]] with idx [n] int32 (an output) = first index with bins[idx] >= v[r]
 *     (torch.bucketize right=False, the search of dsp_bucketize_embed_add); v [n], bins [nb] fp32 (widened half values compare as torch
 *     compares them), emb [nb+1,C].  The add is (float)x + (float)e rounded once: the bits of torch's add in that dtype.  Out of place.
 *
 *   dsp_embed_grad: grad_emb [nb+1,C] : grad_emb[k,:] = sum over the rows r with idx[r] == k of grad_out [n,C][r,:], rows in ascending r;
 *     a bucket without a row gets exact zeros; idx values outside [0, nb] select no bucket.  The inverted index is built on the device (a
 *     count and a stable ballot compaction per bucket, O(n * (nb+1) / 64) wave steps: meant for tables of a few hundred rows); a bucket's
 *     list is cut into chunks of DSP_EMBED_GRAD_CHUNK rows, each summed by one wave in list order, and the bucket's chunk sums are added
 *     in chunk order.  workspace: dsp_embed_grad_workspace_bytes(n, nb, C) bytes of device memory, 16-byte aligned (DSP_ENOSPC if smaller).
 *
 *   dsp_length_regulator_bwd: grad_x [B,N,C] : grad_x[b,t,:] = sum over f in [cum[b,t-1], cum[b,t]) of grad_out [B,maxlen,C][b,f,:]
 *     (cum[b,-1] = 0), frames in ascending f; cum [B,N] int64 as dsp_length_regulator_lens wrote it, maxlen as passed to
 *     dsp_length_regulator_expand.  NEVER READS PADDING FRAMES: frames at or beyond cum[b,N-1] (and beyond maxlen) are not touched, so
 *     they may hold anything.  A row of zero duration is written as zeros. */
#define DSP_EMBED_GRAD_CHUNK 64
int dsp_bucketize_embed_add_fwd(const void* x, int dtype, const float* v, const float* bins, int nb, const void* emb, void* out, int32_t* idx,
                                int64_t n, int C, dsp_stream_t stream);
size_t dsp_embed_grad_workspace_bytes(int64_t n, int nb, int C);
int dsp_embed_grad(const void* grad_out, int dtype, const int32_t* idx, void* grad_emb, int64_t n, int nb, int C,
                   void* workspace, size_t workspace_bytes, dsp_stream_t stream);
int dsp_length_regulator_bwd(const void* grad_out, int dtype, const int64_t* cum, void* grad_x, int B, int N, int C, int maxlen,
                             dsp_stream_t stream);

/* G1, G2  the glancing step of DAG training (csrc/glance.hip; DASpeech/criterions/nat_dag_loss.py:130-132 and :223-255).
 *
 *   dsp_force_emit: force-emit of the revealed vertices, out of place, one read and one write of [B,T,L]:
 *       out[b,t,j] = match[b,t,j]                                  where revealed[b,j] == 0
 *       out[b,t,j] = t == path[b,j] ? match[b,t,j] : -inf          where revealed[b,j] != 0   (path[b,j] = -1: a column of -inf)
 *     Values are copied, never recomputed.  dtype DSP_F32 or DSP_F64 (a code these two entry points alone take).  match [B,T,L] with unit
 *     stride along L, `st` elements between rows and `sb` between samples (any values: the gather's pitched view, a dense tensor, a
 *     misaligned view); path [B,L] int64, revealed [B,L] bytes, both contiguous; out [B,T,L] with row pitch ldo >= L and samples T*ldo
 *     apart.  16-byte accesses where base and pitches allow them (fp32: base % 16 == 0, st % 4 == 0, sb % 4 == 0), element accesses
 *     otherwise and for the last L % 4 columns of a row.  Only columns < L are read or written: pitch padding may hold anything and stays
 *     untouched.
 *
 *   dsp_force_emit_bwd: its gradient, grad_match[b,t,j] = revealed[b,j] ? 0 : grad_out[b,t,j].  grad_out [B,T,L] with ANY element strides
 *     (sb, st, sl >= 0; 0 = a broadcast dimension); grad_match as `out` above (row pitch ldg).
 *
 *   dsp_glance_oracle: oracle[b,j] = tgt[b, max(path[b,j], 0)] and n_right[b] = #{ j : path[b,j] >= 0 and guess[b,j] == oracle[b,j] } (an
 *     integer count).  tgt [B,T], path / guess / oracle [B,L], n_right [B], all int64 contiguous.  One workgroup per sample.
 *
 *   dsp_glance_reveal: per vertex  keep_prob [B,L] fp32, revealed [B,L] bytes (0 / 1) = unif < keep_prob, glanced [B,L] int64 =
 *     revealed ? oracle : prev.  unif [B,L] fp32; path, oracle, prev [B,L] int64.
 *       mode DSP_GLANCE_PROB:  param = prob [B] fp32;  keep_prob[b,j] = prob[b] * (path[b,j] >= 0 ? 1 : 0)   (the IEEE product)
 *       mode DSP_GLANCE_COUNT: param = counts [B] int64, scores [B,L] fp32.  Scores of vertices with path < 0 count as -100.  keep_prob is 1
 *         where the score is >= the row's counts[b]-th largest score and 0 elsewhere: ties with the threshold are all kept, the
 *         comparison is IEEE (-0.0 ties +0.0); counts[b] == 0 compares against 100 (keeps nothing); counts[b] beyond the number of
 *         aligned vertices reaches the -100 fill and keeps the whole row (counts beyond L act as L, below 0 as 1).  Scores must not be NaN.
 *         The threshold comes from an exact radix select over the row held in LDS (no sort; integer histograms: the same bits on every
 *         run), which bounds the row: 1 <= L <= DSP_GLANCE_MAX_L in both modes. */
#define DSP_F64 3
#define DSP_GLANCE_MAX_L 16000
#define DSP_GLANCE_PROB 0
#define DSP_GLANCE_COUNT 1
int dsp_force_emit(const void* match, int dtype, int64_t sb, int64_t st, const int64_t* path, const unsigned char* revealed, void* out,
                   int64_t ldo, int B, int T, int L, dsp_stream_t stream);
int dsp_force_emit_bwd(const void* grad_out, int dtype, int64_t sb, int64_t st, int64_t sl, const unsigned char* revealed, void* grad_match,
                       int64_t ldg, int B, int T, int L, dsp_stream_t stream);
int dsp_glance_oracle(const int64_t* tgt, const int64_t* path, const int64_t* guess, int64_t* oracle, int64_t* n_right, int B, int T, int L,
                      dsp_stream_t stream);
int dsp_glance_reveal(const float* scores, const void* param, int mode, const float* unif, const int64_t* path, const int64_t* oracle,
                      const int64_t* prev, float* keep_prob, unsigned char* revealed, int64_t* glanced, int B, int L, dsp_stream_t stream);

/* Conformer convolution module, eval mode (fairseq conformer_layer.py ConvolutionModule: depthwise_conv -> batch_norm -> SiLU),
 * on the channels-last tensor:   y[b,t,c] = SiLU( BN_eval( sum_k w[c,k] * x[b,t+k-(K-1)/2,c] ) ),  zero padding outside [0,T).
 *   x, y [B,T,C] fp32 (16-byte aligned, C % 4 == 0, y != x); w [C,K] fp32 (the Conv1d(C,C,K,groups=C) weight [C,1,K]);
 *   bn_w / bn_b may be NULL (affine off); K in {3, 7, 15, 31}. */
int dsp_dwconv_bn_silu(const float* x, const float* w, const float* bn_w, const float* bn_b, const float* bn_mean,
                       const float* bn_var, float eps, float* y, int B, int T, int C, int K, dsp_stream_t stream);

/* The same three steps in TRAINING mode, under autograd (csrc/conformer_train.hip): batch statistics, running-buffer update, backward.
 *   With N = B*T, P = (K-1)/2, zero padding outside [0,T), no padding mask (the reference's ConvolutionModule takes none):
 *     z = depthwise(x);  mean[c], var[c] (biased) over the N values of channel c;  invstd = 1/sqrt(var + eps);  zh = (z - mean) * invstd;
 *     u = gamma*zh + beta;  y = u*sigmoid(u);  running_mean <- (1-momentum)*running_mean + momentum*mean;
 *     running_var <- (1-momentum)*running_var + momentum*var*N/(N-1)        (num_batches_tracked is the caller's)
 *   backward from grad_y:  du = grad_y * s*(1 + u*(1-s)), s = sigmoid(u);  dbeta = sum du;  dgamma = sum du*zh;
 *     dz = gamma*invstd*(du - dbeta/N - zh*dgamma/N);  dx[b,t,c] = sum_k w[c,k]*dz[b,t-k+P,c];  dw[c,k] = sum_{b,t} dz[b,t,c]*x[b,t+k-P,c].
 *   x, y, grad_y, dx [B,T,C] and w, dw [C,K] share the dtype code act_dtype (DSP_F32 / DSP_F16 / DSP_BF16); gamma, beta, the running
 *   buffers, dgamma and dbeta [C] share bn_dtype (act_dtype, or DSP_F32); save_mean / save_invstd [C] are fp32 (forward outputs, backward
 *   inputs).  All arithmetic is fp32, the statistics included; every output is rounded once to its dtype.  x / y / grad_y / dx 16-byte
 *   aligned, C a multiple of the channels in 16 bytes (4 or 8), K in {3, 7, 15, 31}, 2 <= B*T <= 2^24.
 *   EVERY OUTPUT ELEMENT IS WRITTEN.  Every reduction over N is two-stage: one partial per chunk of DSP_CONVMOD_CHUNK_TILES time tiles
 *   (DSP_CONVMOD_TIME_TILE frames each, tiles numbered sample by sample) reduced in a fixed order inside one workgroup, then the partials
 *   added in ASCENDING chunk order; the variance from (count, mean, M2) triples of centred values, never from E[z^2] - mean^2.  NO FLOAT
 *   ATOMICS and no hand-off between workgroups: the same inputs give the same bits on every call.
 *   running_mean / running_var may be NULL (not tracked); each of dx / dw / dgamma / dbeta may be NULL: only what is asked for is computed,
 *   and leaving one out does not change the bits of the others.  workspace: dsp_dwconv_bn_silu_train_workspace_bytes(B, T, C, K) bytes of
 *   device memory, 16-byte aligned, for either call (contents need not survive between them; DSP_ENOSPC if smaller); host arithmetic only,
 *   0 for B == 0, monotone in every argument, a multiple of 16.  z is never stored (recomputed from x where needed); dz is kept in fp32 in
 *   the backward's workspace.  Bad sizes, null or aliased pointers, misalignment: DSP_EINVAL before any launch; B == 0: DSP_OK. */
#define DSP_CONVMOD_TIME_TILE 8
#define DSP_CONVMOD_CHUNK_TILES 16
size_t dsp_dwconv_bn_silu_train_workspace_bytes(int B, int T, int C, int K);
int dsp_dwconv_bn_silu_train_fwd(const void* x, const void* w, const void* gamma, const void* beta, void* running_mean, void* running_var,
                                 float momentum, float eps, void* y, float* save_mean, float* save_invstd, void* workspace,
                                 size_t workspace_bytes, int act_dtype, int bn_dtype, int B, int T, int C, int K, dsp_stream_t stream);
int dsp_dwconv_bn_silu_train_bwd(const void* x, const void* w, const void* gamma, const void* beta, const float* save_mean,
                                 const float* save_invstd, const void* grad_y, void* dx, void* dw, void* dgamma, void* dbeta,
                                 void* workspace, size_t workspace_bytes, int act_dtype, int bn_dtype, int B, int T, int C, int K,
                                 dsp_stream_t stream);

/* Residual + dropout + LayerNorm under autograd (csrc/residual_norm_train.hip): the residual sites of the training step,
 *     s = residual + alpha * dropout(h [+ bias]);   y = LayerNorm(s)
 *   on contiguous channels-last tensors of R rows (the product of the leading dimensions) and C columns.  Per row, in fp32:
 *     z = h + bias (bias may be NULL);  d = keep ? z * keep_scale : 0;  s = residual + alpha * d, ROUNDED to the data dtype and written;
 *     mean and rstd = 1/sqrt(var + eps) (biased variance) of the rounded s — what a LayerNorm applied to the stored s sees, and what lets the
 *     backward rebuild xhat = (s - mean) * rstd from the saved s;  y = gamma * xhat + beta;  stats[r] = (mean, rstd), fp32 [R,2].
 *   h == NULL: s = residual, nothing is written to `s` (may be NULL), the call is a plain LayerNorm under autograd (the first norm of a block).
 *   The mask is counter-based and never stored: with e = r*C + c, the four words of Philox4x32-10 with key (seed lo, seed hi) and counter
 *   (g lo, g hi, offset lo, offset hi), g = e >> 2, serve elements 4g .. 4g+3 in order, and keep <=> (word >> 8) >= thr, where the caller
 *   computes thr = ceil(p * 2^24) in double and keep_scale = 1/(1-p).  thr == 0: no dropout — no mask path at all, keep_scale is not read.
 *   dsp_dropout_keep_mask writes the same mask of n elements as bytes (1 = keep), for tests and diagnostics.
 *   backward from dy and / or ds (either may be NULL: that output was not used; without dy neither s, stats nor gamma is read and they may be
 *   NULL too, dgamma and dbeta are then zeros) with the saved s and stats and the same
 *   (alpha, keep_scale, thr, seed, offset):   dxhat = dy * gamma;   g = ds + rstd * (dxhat - mean_c(dxhat) - xhat * mean_c(dxhat * xhat));
 *     dresidual = g;  dh = alpha * keep * keep_scale * g;  dgamma = sum_r dy * xhat;  dbeta = sum_r dy;  dbias = sum_r dh (before rounding).
 *   h, residual, s, y, dy, ds, dh, dresidual share the dtype code act_dtype (DSP_F32 / DSP_F16 / DSP_BF16); gamma, beta, bias, dgamma, dbeta,
 *   dbias [C] share param_dtype (act_dtype, or DSP_F32).  All 16-byte aligned, C a multiple of the elements in 16 bytes (4 or 8), C <= 2048,
 *   R <= 2^24.  EVERY OUTPUT ELEMENT IS WRITTEN.  The column sums are two-stage: one fp32 partial per chunk of DSP_RESNORM_CHUNK_ROWS rows,
 *   reduced in a fixed order inside one workgroup, then the partials added in ASCENDING chunk order.  NO FLOAT ATOMICS and no hand-off
 *   between workgroups: the same inputs give the same bits on every call.  Each of dh / dresidual / dbias / dgamma / dbeta may be NULL, and
 *   leaving one out does not change the bits of the others (dbias without dh is served: with thr == 0 and alpha == 1, dh equals dresidual).
 *   workspace (backward, needed when a column sum is asked for): dsp_resnorm_train_workspace_bytes(R, C) bytes of device memory, 16-byte
 *   aligned (DSP_ENOSPC if smaller); host arithmetic only, 0 for an empty problem, monotone in each argument, a multiple of 16.
 *   Bad sizes, null or aliased pointers, misalignment: DSP_EINVAL before any launch; R == 0: DSP_OK. */
#define DSP_RESNORM_CHUNK_ROWS 32
size_t dsp_resnorm_train_workspace_bytes(int64_t R, int C);
int dsp_resnorm_train_fwd(const void* h, const void* residual, const void* bias, const void* gamma, const void* beta, float eps, float alpha,
                          float keep_scale, unsigned int thr, uint64_t seed, uint64_t offset, void* s, void* y, float* stats, int act_dtype,
                          int param_dtype, int64_t R, int C, dsp_stream_t stream);
int dsp_resnorm_train_bwd(const void* dy, const void* ds, const void* s, const float* stats, const void* gamma, float alpha, float keep_scale,
                          unsigned int thr, uint64_t seed, uint64_t offset, void* dh, void* dresidual, void* dbias, void* dgamma, void* dbeta,
                          void* workspace, size_t workspace_bytes, int act_dtype, int param_dtype, int64_t R, int C, dsp_stream_t stream);
int dsp_dropout_keep_mask(uint64_t seed, uint64_t offset, unsigned int thr, unsigned char* out, int64_t n, dsp_stream_t stream);

/* Bias + activation + dropout (and GLU) under autograd (csrc/act_dropout_train.hip): the element-wise pass between the two GEMMs of a
 * feed-forward block of the training step, on R rows (the product of the leading dimensions).  With u = h + bias in fp32 (bias may be NULL):
 *     act = DSP_ACT_IDENTITY / _RELU / _SILU / _GELU (erf form):  Cout = Cin,      y[r,c] = keep ? keep_scale * act(u[r,c]) : 0
 *     act = DSP_ACT_GLU:                                          Cout = Cin / 2,  y[r,c] = keep ? keep_scale * u[r,c] * sigmoid(u[r,c+Cout]) : 0
 *   (the first half of a row is gated by the second, as F.glu(dim=-1)).  h [R,Cin] has unit column stride and the row pitch ld_h (elements,
 *   >= Cin: a contiguous tensor or a column slice of a wider one); y [R,Cout] is contiguous.
 *   The mask follows dsp_resnorm_train_fwd's rule (above) on the element index e = r*Cout + c of the OUTPUT: dsp_dropout_keep_mask over
 *   n = R*Cout elements, read as [R,Cout], is the mask applied.  It is never stored.  thr == 0: no dropout — no mask path at all, keep_scale
 *   is not read.
 *   backward from dy [R,Cout] contiguous with h, bias and the same (act, keep_scale, thr, seed, offset); u, the derivative and the mask are
 *   recomputed, nothing else of the forward is needed.  With m = keep * keep_scale (1 with thr == 0):
 *     dh = dy * m * act'(u):   identity 1;  relu u > 0;  silu s(1 + u(1 - s)), s = sigmoid(u);  gelu Phi(u) + u phi(u);
 *     glu, a = u[:, :Cout], g = u[:, Cout:], s = sigmoid(g):   dh[:, :Cout] = dy * m * s;   dh[:, Cout:] = dy * m * a * s(1 - s)
 *     dbias[c] = sum_r dh[r,c], summed in fp32 BEFORE dh is rounded to the data dtype.
 *   dh [R,Cin] is contiguous (whatever ld_h is); dbias [Cin].
 *   h, y, dy, dh share the dtype code act_dtype (DSP_F32 / DSP_F16 / DSP_BF16); bias and dbias share param_dtype (act_dtype, or DSP_F32).
 *   All arithmetic is fp32.  All pointers 16-byte aligned, Cin and ld_h multiples of the elements in 16 bytes (4 or 8; glu: Cin a multiple of
 *   twice that, so that Cout is on the grid too), Cin <= DSP_ACTDROP_MAX_CIN, R <= 2^24.  EVERY OUTPUT ELEMENT IS WRITTEN.  dbias is two-stage:
 *   a thread owns a 16-byte column group and adds the rows of its chunk of DSP_ACTDROP_CHUNK_ROWS rows in row order, one fp32 partial
 *   [chunks, Cin] goes to the workspace, and a tail kernel adds the partials in ASCENDING chunk order.  NO FLOAT ATOMICS and no hand-off between
 *   workgroups: the same inputs give the same bits on every call.  dh and dbias may each be NULL, and leaving one out does not change the bits
 *   of the other; with both NULL the call returns DSP_OK without a launch.
 *   workspace (backward, needed for dbias only; without dbias none is read and no tail is launched): dsp_act_dropout_train_workspace_bytes(R,
 *   Cin) bytes of device memory, 16-byte aligned (DSP_ENOSPC if smaller); host arithmetic only, 0 for an empty problem, monotone in each
 *   argument, a multiple of 16.
 *   Bad sizes, null or aliased pointers, misalignment, an unknown act, glu with an odd number of 16-byte groups per row: DSP_EINVAL
 *   (dsp_last_error says which) before any launch; R == 0: DSP_OK without a launch. */
#define DSP_ACT_IDENTITY 0
#define DSP_ACT_RELU 1
#define DSP_ACT_SILU 2
#define DSP_ACT_GELU 3
#define DSP_ACT_GLU 4
#define DSP_ACTDROP_CHUNK_ROWS 32
#define DSP_ACTDROP_MAX_CIN 8192
size_t dsp_act_dropout_train_workspace_bytes(int64_t R, int Cin);
int dsp_act_dropout_train_fwd(const void* h, long ld_h, const void* bias, int act, float keep_scale, unsigned int thr, uint64_t seed,
                              uint64_t offset, void* y, int act_dtype, int param_dtype, int64_t R, int Cin, dsp_stream_t stream);
int dsp_act_dropout_train_bwd(const void* dy, const void* h, long ld_h, const void* bias, int act, float keep_scale, unsigned int thr,
                              uint64_t seed, uint64_t offset, void* dh, void* dbias, void* workspace, size_t workspace_bytes, int act_dtype,
                              int param_dtype, int64_t R, int Cin, dsp_stream_t stream);

/* The input embeddings of the decoder and of the TTS half under autograd (csrc/embed_entry_train.hip).  Both operators take the positions
 * from a cumulative count of the kept elements of a sample's row — correct for left padding, interior pads and all-pad rows —, compute in fp32,
 * round once, and apply the dropout mask of dsp_resnorm_train_fwd's rule (above) on the element index e = r*C + c of the contiguous output
 * (dsp_dropout_keep_mask over n*C elements, read as [n,C], is the mask applied; thr == 0: no mask path at all, keep_scale is not read).
 *
 *   dsp_embed_entry_fwd: tokens [B,L] int64 with unit column stride and ld_tok elements between rows (8-byte aligned); E [V,C] and P [NP,C]
 *     in one dtype code, which is also y's.  keep = tokens != pad;  pos[b,t] = pad + keep * #{ t' <= t : tokens[b,t'] != pad }
 *     (DAGDecoder.positions);  y[b,t,:] = m * (embed_scale * E[tok] + P[pos]), y [B*L,C] contiguous.  Row `pad` of either table is read as it
 *     is stored.  A token outside [0, V) contributes a zero embedding row and still counts as non-pad; nothing outside a table is read (the
 *     caller keeps L + pad + 1 <= NP; a larger position would be clamped to NP - 1).  Outputs for the backward: tok32 [B*L] int32 (-1 for a
 *     token outside [0, V)) and pos32 [B*L] int32.  One launch.
 *
 *   dsp_embed_entry_bwd: with g = dy * m (dy [n,C] contiguous, n = B*L):
 *       dE[v,:] = embed_scale * sum over the rows r with tok32[r] == v of g[r,:]        dP[q,:] = sum over the rows r with pos32[r] == q of g[r,:]
 *     rows added in ASCENDING r in fp32, embed_scale applied in fp32, ONE rounding.  Every row of dE [V,C] and dP [NP,C] is written; row `pad`
 *     of both (padding_idx), rows without a source and the share of out-of-range tokens are exact zeros.  Either of dE / dP may be NULL, and
 *     one alone has the bits it has next to the other; both NULL: DSP_OK without a launch.  g is written once as fp32 [n,C] into the workspace
 *     when thr != 0 (with thr == 0 the sums read dy).  Both gradients come from ONE inverted index over 2n list entries and V + NP keys:
 *     integer atomic counts, one exclusive scan, then per key — at most DSP_EMBED_ENTRY_SORT_MAX rows: slots taken in any order and the list
 *     sorted ascending by the key's wave; more rows: a workgroup writes the list by ballot compaction over all entries (at most 2n / 65 such
 *     keys exist) — and the chunk sums (DSP_EMBED_GRAD_CHUNK rows a chunk) and per-key reduce that dsp_embed_grad uses.  The cost does not grow
 *     as V * n / 64.  NO FLOAT ATOMICS and no hand-off between workgroups: the same inputs give the same bits on every call.
 *     workspace: dsp_embed_entry_bwd_workspace_bytes(n, V, NP, C, thr) bytes of device memory, 16-byte aligned (DSP_ENOSPC if smaller), may
 *     hold anything on entry; host arithmetic only, 0 for an empty problem, a multiple of 16.
 *
 *   dsp_pos_add_fwd: x [B,N,C] read as B*N rows of unit column stride ld_x elements apart (>= C, a multiple of the elements in 16 bytes),
 *     padding_mask [B,N] bytes (non-zero: padding), tab [NT,C] in the data dtype or fp32, alpha ONE element on the device in the data dtype
 *     or fp32.  keep = !mask;  pos = min(pad + keep * cumsum(keep), NT - 1) (positions_from_padding_mask, then the clamp);
 *     y = m * (x + alpha * tab[pos]), y [B*N,C] contiguous; pos32 [B*N] int32 is kept for the backward.  One launch.
 *
 *   dsp_pos_add_bwd: dx = dy * m (dx NULL: not computed — with thr == 0 it is dy itself and the caller hands dy on; a non-NULL dx with
 *     thr == 0 gets a copy), dalpha = sum over rows and columns of g * tab[pos] with g = dy * m: one wave per chunk of DSP_POS_ADD_CHUNK_ROWS
 *     rows writes a partial (a lane adds its columns over the rows in row order, then a butterfly over the lanes), a one-workgroup tail
 *     adds the partials in index order and rounds once to alpha's dtype.  The lanes and the tail accumulate in double and a partial is
 *     stored as two fp32 values (head, tail): dalpha is one number out of R*C products of either sign, and fp32 accumulators would leave it
 *     with an ulp of partial sums far larger than the result.  dalpha NULL: skipped (tab and pos32 are then not read).
 *     workspace (needed for dalpha only): dsp_pos_add_bwd_workspace_bytes(R) bytes, 16-byte aligned, may hold anything on entry.
 *
 *   All four: fp32 / fp16 / bf16, C a multiple of the elements in 16 bytes (4 or 8), C <= DSP_EMBED_ENTRY_MAX_C, at most 2^24 rows, tables,
 *   data tensors and gradients 16-byte aligned.  EVERY OUTPUT ELEMENT IS WRITTEN.  Bad sizes, null or aliased pointers, misalignment:
 *   DSP_EINVAL before any launch; no rows: DSP_OK (the gradients of the tables / of alpha are then zeros). */
#define DSP_EMBED_ENTRY_MAX_C 2048
#define DSP_EMBED_ENTRY_SORT_MAX 64
#define DSP_POS_ADD_CHUNK_ROWS 32
int dsp_embed_entry_fwd(const int64_t* tokens, long ld_tok, const void* E, const void* P, int64_t pad, float embed_scale, float keep_scale,
                        unsigned int thr, uint64_t seed, uint64_t offset, void* y, int32_t* tok32, int32_t* pos32, int dtype, int B, int L, int V,
                        int NP, int C, dsp_stream_t stream);
size_t dsp_embed_entry_bwd_workspace_bytes(int64_t n, int V, int NP, int C, unsigned int thr);
int dsp_embed_entry_bwd(const void* dy, const int32_t* tok32, const int32_t* pos32, int64_t pad, float embed_scale, float keep_scale,
                        unsigned int thr, uint64_t seed, uint64_t offset, void* dE, void* dP, void* workspace, size_t workspace_bytes, int dtype,
                        int64_t n, int V, int NP, int C, dsp_stream_t stream);
int dsp_pos_add_fwd(const void* x, long ld_x, const unsigned char* padding_mask, const void* tab, const void* alpha, int pad, float keep_scale,
                    unsigned int thr, uint64_t seed, uint64_t offset, void* y, int32_t* pos32, int act_dtype, int tab_dtype, int alpha_dtype, int B,
                    int N, int NT, int C, dsp_stream_t stream);
size_t dsp_pos_add_bwd_workspace_bytes(int64_t R);
int dsp_pos_add_bwd(const void* dy, const void* tab, const int32_t* pos32, float keep_scale, unsigned int thr, uint64_t seed, uint64_t offset,
                    void* dx, void* dalpha, void* workspace, size_t workspace_bytes, int act_dtype, int tab_dtype, int alpha_dtype, int64_t R, int NT,
                    int C, dsp_stream_t stream);

/* The four TTS losses of the training objective under autograd (csrc/tts_loss_train.hip), the masks taken from the lengths: no mask tensor,
 * no selection, no host read.  feat_out [B,F,C], feat_post (NULL, or shaped like feat_out) and target [B,Fa,C] are given as a base pointer,
 * a batch stride and a row stride in elements (>= 0; unit column stride), so that the rows f < F_ = min(F, Fa) are read in place; the six
 * [B,N] tensors (log_dur_out, pitch_out, energy_out, pitches, energies in the data dtype; durations int64 with dur64 != 0, else int32) are
 * contiguous; audio_lens and src_lens are [B], int64 with len64 != 0, else int32.  With m_b = min(max(audio_lens[b], 0), F_),
 * s_b = min(max(src_lens[b], 0), N), n_mel = C * sum_b m_b and n_src = sum_b s_b (integers):
 *     losses[0] = l1     = sum_{b, f < m_b, c} |feat_out[b,f,c] - target[b,f,c]| / n_mel  (+ the same sum over feat_post, also / n_mel)
 *     losses[1] = dur    = sum_{b, n < s_b} (log_dur_out[b,n] - log(durations[b,n] + 1))^2 / n_src
 *     losses[2] = pitch  = sum_{b, n < s_b} (pitch_out[b,n]  - pitches[b,n])^2 / n_src
 *     losses[3] = energy = sum_{b, n < s_b} (energy_out[b,n] - energies[b,n])^2 / n_src
 *   Data is DSP_F32 / DSP_F16 / DSP_BF16 (one code for all floating tensors); everything is computed in fp32 on the exactly widened inputs —
 *   the difference, the log, the squares — and the four results are fp32.  Rows at or beyond a length are never read.  An empty selection
 *   gives 0 / 0 = NaN; non-finite inputs propagate.  inv_counts[0] = 1 / n_mel, inv_counts[1] = 1 / n_src (fp32) is what the backward keeps.
 *   forward, two launches.  The rows (b, f) of the [B,F_] grid, in that order, are cut into chunks of DSP_TTSLOSS_CHUNK_ROWS rows, the B*N
 *   elements of the [B,N] grid into chunks of DSP_TTSLOSS_CHUNK_ELEMS; one wave owns a chunk: lane l adds the valid terms of its elements in
 *   ascending order (16-byte form: the groups l, l + 64, ... of the chunk's rows * C / V groups, V = 4 or 8 elements, each group element by
 *   element; scalar form: the elements l, l + 64, ...), the 64 lanes fold by xor butterfly, and the chunk's fp32 partials go to slot `chunk` of
 *   the workspace — [l1 | post | dur | pitch | energy] — with plain stores.  The chunk -> slot mapping follows from the shapes alone, not from
 *   the lengths, the grid or the schedule.  The tail (one workgroup of 256) adds each array's slots t, t + 256, ... in ascending order in
 *   thread t, folds each wave, adds the four waves in order, forms n_mel and n_src from the lengths and divides once.  NO FLOAT ATOMICS, no
 *   hand-off between workgroups inside a launch, and the workspace is never assumed to be zero: the same inputs give the same bits.
 *   backward, one launch, from grad_losses (fp32 [4], device) and inv_counts with the forward's inputs; the differences are recomputed:
 *     d_feat_out = d_feat_post = grad[0] * sign(a - b) / n_mel   (sign(0) = sign(NaN) = 0);   d_x = grad[i] * 2 (a - b) / n_src  for the
 *   three [B,N] predictions, each value rounded once to the data dtype.  d_feat_out and d_feat_post are contiguous [B,F,C], d_log_dur, d_pitch
 *   and d_energy contiguous [B,N]; EVERY ELEMENT of every gradient given IS WRITTEN — rows at or beyond m_b / s_b and rows F_ .. F-1 get exact
 *   zeros.  Targets get no gradient.  Every gradient pointer may be NULL without changing the bits of the others (d_feat_post needs feat_post).
 *   16-byte accesses per lane are used where C is a multiple of the elements in 16 bytes and every mel pointer and stride is on that grid,
 *   a scalar path otherwise; pointers need the alignment of their element type only.
 *   workspace (forward): dsp_tts_loss_workspace_bytes(B, F_, N) bytes, 16-byte aligned (DSP_ENOSPC if smaller) — host arithmetic only, 0 for
 *   an empty problem, monotone in each argument, a multiple of 16.
 *   Bad sizes (B < 0, F_ < 1, F_ > F, C < 1, N < 1, B*F*C or B*N above DSP_TTSLOSS_MAX_ELEMS), an unknown dtype, a negative stride, a null
 *   pointer other than feat_post and the gradients, a pointer off the grid of its element type, an output that aliases an input or another
 *   output: DSP_EINVAL (dsp_last_error says which) before any launch.  B == 0, or a backward with every gradient NULL: DSP_OK without a
 *   launch (nothing is written). */
#define DSP_TTSLOSS_CHUNK_ROWS 32
#define DSP_TTSLOSS_CHUNK_ELEMS 1024
#define DSP_TTSLOSS_MAX_ELEMS (1L << 30)
size_t dsp_tts_loss_workspace_bytes(int B, int F_, int N);
int dsp_tts_loss_fwd(const void* feat_out, long fo_sb, long fo_sr, const void* feat_post, long fp_sb, long fp_sr, const void* target, long tg_sb,
                     long tg_sr, const void* audio_lens, const void* log_dur_out, const void* pitch_out, const void* energy_out,
                     const void* durations, const void* pitches, const void* energies, const void* src_lens, int len64, int dur64, float* losses,
                     float* inv_counts, void* workspace, size_t workspace_bytes, int dtype, int B, int F_, int C, int N, dsp_stream_t stream);
int dsp_tts_loss_bwd(const float* grad_losses, const float* inv_counts, const void* feat_out, long fo_sb, long fo_sr, const void* feat_post,
                     long fp_sb, long fp_sr, const void* target, long tg_sb, long tg_sr, const void* audio_lens, const void* log_dur_out,
                     const void* pitch_out, const void* energy_out, const void* durations, const void* pitches, const void* energies,
                     const void* src_lens, int len64, int dur64, void* d_feat_out, void* d_feat_post, void* d_log_dur, void* d_pitch,
                     void* d_energy, int dtype, int B, int F, int F_, int C, int N, dsp_stream_t stream);

/* The argmax strategy's features_on_path under autograd (csrc/path_features_train.hip): a stable compaction of feature rows, no sort, no
 * atomics, no width read from the device.  features [B,L,C] in DSP_F32 / DSP_F16 / DSP_BF16, read as B*L rows of unit column stride ld_f
 * elements apart (>= C, a multiple of the elements in 16 bytes); path [B,L] int64 (path64 != 0) or int32 through its batch and column
 * strides in elements (>= 0), of which ONLY THE SIGN of a value is read; W >= 0 the width of the result, a host integer.
 *     on[b,j] = path[b,j] >= 0 && (j > 0 || !skip_first)          n[b] = min(sum_j on[b,j], W)
 *   dsp_path_features_fwd, one launch that writes all three outputs completely (no memset, no workspace):
 *     out[b,r,:] = features[b, j_r, :] for r < n[b], j_r the r-th vertex with `on` set in ascending j; EXACT ZEROS for r >= n[b] — written,
 *     not multiplied: NaN or Inf in a row that is not selected never shows.  out [B,W,C] contiguous, pad [B,W] bytes (1: r >= n[b]),
 *     n [B] int64.  A path with more than W vertices on drops the surplus.  W == 0 (or B == 0): DSP_OK without a launch, nothing is written.
 *   dsp_path_features_bwd, one launch that writes EVERY element of dfeatures [B,L,C] (contiguous) exactly once, without float atomics:
 *     dfeatures[b,j,:] = dy[b,r,:] where j = j_r for some r < n[b], else exact zeros.  dy [B,W,C] is read through its batch and row strides
 *     in elements (>= 0, multiples of the elements in 16 bytes; unit column stride; 0 for a broadcast); with W == 0 dy is not read.
 *   Rows move as 16-byte quads, bit for bit: the result does not depend on the dtype beyond its element size.  A workgroup of the forward
 *   owns DSP_PATH_FEATURES_TILE_W rows of one sample's result, one of the backward DSP_PATH_FEATURES_TILE_L vertices; each rescans its
 *   sample's path row (ballots and popcounts over chunks of 64 vertices, a prefix over the chunk counts).
 *   Bad sizes (B < 0, L < 1, L > DSP_PATH_FEATURES_MAX_L, W < 0, C no multiple of the elements in 16 bytes, B*L or B*W above 2^24), an unknown
 *   dtype, a negative stride, a null or aliased pointer, features / out / dy / dfeatures off the 16-byte grid: DSP_EINVAL before any launch. */
#define DSP_PATH_FEATURES_TILE_W 8
#define DSP_PATH_FEATURES_TILE_L 16
#define DSP_PATH_FEATURES_MAX_L 65536
int dsp_path_features_fwd(const void* features, long ld_f, const void* path, long path_sb, long path_sc, int path64, int skip_first, void* out,
                          unsigned char* pad, int64_t* n, int dtype, int B, int L, int W, int C, dsp_stream_t stream);
int dsp_path_features_bwd(const void* dy, long dy_sb, long dy_sr, const void* path, long path_sb, long path_sc, int path64, int skip_first,
                          void* dfeatures, int dtype, int B, int L, int W, int C, dsp_stream_t stream);

/* Conformer relative-position self-attention under autograd (csrc/relpos_attention_train.hip), fp16 / bf16 data, head width 64:
 *     s(b,h,i,j) = ((q_i + u_h).k_j + (q_i + v_h).pos[T-1-i+j]) / 8,  keys with pad_mask[b,j] != 0: -inf
 *     P = softmax_j(s);  lse(b,h,i) = log sum_j exp s;  A = keep ? P * keep_scale : 0;  out_i = sum_j A_ij v_j
 *   q, k, v [B,T,H,64] with one common row stride ld (elements; >= 64 H, a multiple of 8; samples T*ld apart: contiguous tensors or the column
 *   slices of a stacked projection), pos [2T-1,H,64] contiguous (linear_pos of the relative positional encoding, rows for relative positions
 *   T-1 .. -(T-1)), bias_u / bias_v [H,64], pad_mask [B,T] bytes or NULL, out [B,T,H*64] contiguous in the data dtype, lse [B,H,T] fp32 (saved
 *   for the backward).  Scores, soft-max statistics and accumulators are fp32; q + u, q + v and P are rounded to the data dtype once, where
 *   they become matrix-core operands.  Every query row is computed, padded ones too.  A sample whose keys are all masked gets NaN rows, as
 *   torch's soft-max gives; no mask leads to an access out of range.
 *   The mask follows dsp_resnorm_train_fwd's rule (above) on the element index e = ((b*H + h)*T + i)*Tp + j, Tp = T rounded up to a multiple
 *   of 4: dsp_dropout_keep_mask over n = B*H*T*Tp elements, read as [B,H,T,Tp], is the mask applied.  thr == 0: no mask path.
 *   backward from dout [B,T,H*64] contiguous with the forward's inputs, out, lse and (keep_scale, thr, seed, offset); with m = keep * keep_scale
 *   and D_i = dout_i . out_i:   dV = (P o m)^T dout;  dP = (dout V^T) o m;  dS = P o (dP - D) / 8;  dK = dS^T (q + u);
 *     dG[i, T-1-i+j] = dS[i,j];  dq = dS K + dG pos;  dpos = sum_b dG^T (q + v);  dbias_u = sum_{b,i} dS K;  dbias_v = sum_{b,i} dG pos.
 *   P is recomputed; no [B,H,T,T] or [B,H,T,2T-1] tensor is written to memory in either direction.  dq, dk, dv [B,T,H*64] and dpos
 *   [2T-1,H*64] contiguous in the data dtype, dbias_u / dbias_v [H,64] in param_dtype (act_dtype, or DSP_F32, as bias_u / bias_v).
 *   act_dtype is DSP_F16 or DSP_BF16 (fp32 data is not served).  All pointers 16-byte aligned.  EVERY OUTPUT ELEMENT IS WRITTEN.  dpos and the
 *   bias gradients are fp32 partials (per sample; per sample and block of 32 queries) added in ASCENDING order by tail kernels.  NO FLOAT
 *   ATOMICS and no hand-off between workgroups: the same inputs give the same bits on every call.  Each of the six gradients may be NULL, and
 *   leaving one out does not change the bits of the others.
 *   workspace (backward, needed for dpos, dbias_u or dbias_v): dsp_relpos_attention_train_workspace_bytes(B, T, H) bytes of device memory,
 *   16-byte aligned (DSP_ENOSPC if smaller); host arithmetic only, 0 for an empty problem, monotone in each argument, a multiple of 16.
 *   1 <= T <= DSP_RELPOS_TRAIN_MAX_T, 1 <= H <= 1024.  Bad sizes, null required pointers, misalignment, an output that aliases an input:
 *   DSP_EINVAL before any launch; B == 0: DSP_OK. */
#define DSP_RELPOS_TRAIN_MAX_T 2048
size_t dsp_relpos_attention_train_workspace_bytes(int B, int T, int H);
int dsp_relpos_attention_train_fwd(const void* q, const void* k, const void* v, long ld, const void* pos, const void* bias_u, const void* bias_v,
                                   const unsigned char* pad_mask, float keep_scale, unsigned int thr, uint64_t seed, uint64_t offset, void* out,
                                   float* lse, int act_dtype, int param_dtype, int B, int T, int H, dsp_stream_t stream);
int dsp_relpos_attention_train_bwd(const void* dout, const void* q, const void* k, const void* v, long ld, const void* pos, const void* bias_u,
                                   const void* bias_v, const unsigned char* pad_mask, const void* out, const float* lse, float keep_scale,
                                   unsigned int thr, uint64_t seed, uint64_t offset, void* dq, void* dk, void* dv, void* dpos, void* dbias_u,
                                   void* dbias_v, void* workspace, size_t workspace_bytes, int act_dtype, int param_dtype, int B, int T, int H,
                                   dsp_stream_t stream);

/* Multi-head attention under autograd (csrc/mha_train.hip), fp16 / bf16 data, head width 64 — the relative-position entries above without the
 * position term and with a key length of its own (self-attention: M = N; encoder attention: M = the memory's length):
 *     s(b,h,i,j) = q_i . k_j / 8,  keys with pad_mask[b,j] != 0: -inf
 *     P = softmax_j(s);  lse(b,h,i) = log sum_j exp s;  A = keep ? P * keep_scale : 0;  out_i = sum_j A_ij v_j
 *   q [B,N,H,64] with row stride ldq, k and v [B,M,H,64] with one common row stride ldkv (elements; >= 64 H, multiples of 8; samples N*ldq and
 *   M*ldkv apart: contiguous tensors, or the column slices of a stacked q|k|v or k|v projection), pad_mask [B,M] bytes or NULL, out [B,N,H*64]
 *   contiguous in the data dtype, lse [B,H,N] fp32 (saved for the backward).  Scores, soft-max statistics and accumulators are fp32; P o keep
 *   is rounded to the data dtype once, where it becomes a matrix-core operand, and keep_scale multiplies the fp32 result.  Every query row is computed, padded ones too.  A sample whose keys are all
 *   masked gets NaN in its own rows, as torch's soft-max gives, and harms no other; no mask leads to an access out of range.
 *   The mask follows dsp_resnorm_train_fwd's rule (above) on the element index e = ((b*H + h)*N + i)*Mp + j, Mp = M rounded up to a multiple of
 *   4: dsp_dropout_keep_mask over n = B*H*N*Mp elements, read as [B,H,N,Mp], is the mask applied.  thr == 0: no mask path.
 *   backward from dout [B,N,H*64] contiguous with the forward's inputs, lse and (keep_scale, thr, seed, offset); with m = keep * keep_scale,
 *   dP = (dout V^T) o m and D_i = sum_j P_ij dP_ij (= dout_i . out_i with out in fp32: the forward's out is NOT read — its rounding to the data
 *   dtype would cost a row whose P sits on one key the cancellation of dS, which torch's soft-max backward has):
 *     dV = (P o m)^T dout;  dS = P o (dP - D) / 8;  dK = dS^T q;  dq = dS K.
 *   P is recomputed; no [B,H,N,M] tensor is written to memory in either direction.  dq [B,N,H*64], dk and dv [B,M,H*64] contiguous in the data
 *   dtype.  workspace (backward, always): dsp_mha_train_workspace_bytes(B, N, M, H) bytes of device memory, 16-byte aligned (DSP_ENOSPC if
 *   smaller) — D [B,H,N] in fp32, written by the pass that owns the queries and read by the one that owns the keys; host arithmetic only, 0 for
 *   an empty problem, monotone in each argument, a multiple of 16.  act_dtype is DSP_F16 or DSP_BF16 (fp32 data is not served).  All pointers 16-byte aligned.  EVERY
 *   OUTPUT ELEMENT IS WRITTEN.  A workgroup owns DSP_MHA_TRAIN_OWN_ROWS queries (forward, dq) or keys (dk, dv) of one (sample, head) and walks the
 *   other side in tiles of DSP_MHA_TRAIN_TILE_ROWS in ascending order.  NO FLOAT ATOMICS and no hand-off between workgroups: the same inputs
 *   give the same bits on every call.  Each of the three gradients may be NULL, and leaving one out does not change the bits of the others.
 *   1 <= N, M <= DSP_MHA_TRAIN_MAX_LEN, 1 <= H <= 1024, B*H <= 2^25.  Bad sizes, null required pointers, misalignment, a stride that is not a
 *   multiple of 8 or is below 64 H, an output that aliases an input: DSP_EINVAL before any launch; B == 0: DSP_OK. */
#define DSP_MHA_TRAIN_MAX_LEN 4096
#define DSP_MHA_TRAIN_OWN_ROWS 128
#define DSP_MHA_TRAIN_TILE_ROWS 32
int dsp_mha_train_fwd(const void* q, long ldq, const void* k, const void* v, long ldkv, const unsigned char* pad_mask, float keep_scale,
                      unsigned int thr, uint64_t seed, uint64_t offset, void* out, float* lse, int act_dtype, int B, int N, int M, int H,
                      dsp_stream_t stream);
size_t dsp_mha_train_workspace_bytes(int B, int N, int M, int H);
int dsp_mha_train_bwd(const void* dout, const void* q, long ldq, const void* k, const void* v, long ldkv, const unsigned char* pad_mask,
                      const float* lse, float keep_scale, unsigned int thr, uint64_t seed, uint64_t offset, void* dq, void* dk, void* dv,
                      void* workspace, size_t workspace_bytes, int act_dtype, int B, int N, int M, int H, dsp_stream_t stream);

/* The dropout state on the device: the masked launches above for a stream that is being captured into a graph, where no host integer can
 * name the offset of a replay.  rng_state points at TWO uint64 of device memory, {seed, offset}, 8-byte aligned.  Every ..._state entry is the
 * entry of the same name with ONE more argument before the stream, `const uint64_t* rng_state`, and runs the SAME kernel:
 *     rng_state != NULL:  the kernel uses seed = rng_state[0] and offset = rng_state[1] + `offset` — the `seed` argument is not read, and the
 *                         `offset` argument is the call's distance from the state's offset (a host integer: 0, 4, 8, ... for the masked calls
 *                         of one pass, as the default generator's offset would have moved);
 *     rng_state == NULL:  (seed, offset) as given — the entry without the suffix, bit for bit.
 *   The state is read ONCE per thread at kernel entry through a kernel argument (a uniform load, not one per element), when the kernel runs:
 *   a replayed graph draws from whatever the state holds at that moment.  None of these kernels writes it.  A misaligned rng_state:
 *   DSP_EINVAL before any launch; everything else as the entry without the suffix says.
 *   dsp_dropout_state_advance: rng_state[1] += by, one tiny launch on the stream (an ordinary vector store) — the ONLY kernel that writes a
 *   state.  Recorded as the last node of a graph, it leaves the state where one eager pass of `by / 4` masked calls leaves the generator, so
 *   every replay draws new masks without host work.  A backward reads the state its forward read, so it has to run before the advance. */
int dsp_resnorm_train_fwd_state(const void* h, const void* residual, const void* bias, const void* gamma, const void* beta, float eps,
                                float alpha, float keep_scale, unsigned int thr, uint64_t seed, uint64_t offset, void* s, void* y, float* stats,
                                int act_dtype, int param_dtype, int64_t R, int C, const uint64_t* rng_state, dsp_stream_t stream);
int dsp_resnorm_train_bwd_state(const void* dy, const void* ds, const void* s, const float* stats, const void* gamma, float alpha,
                                float keep_scale, unsigned int thr, uint64_t seed, uint64_t offset, void* dh, void* dresidual, void* dbias,
                                void* dgamma, void* dbeta, void* workspace, size_t workspace_bytes, int act_dtype, int param_dtype, int64_t R,
                                int C, const uint64_t* rng_state, dsp_stream_t stream);
int dsp_dropout_keep_mask_state(uint64_t seed, uint64_t offset, unsigned int thr, unsigned char* out, int64_t n, const uint64_t* rng_state,
                                dsp_stream_t stream);
int dsp_act_dropout_train_fwd_state(const void* h, long ld_h, const void* bias, int act, float keep_scale, unsigned int thr, uint64_t seed,
                                    uint64_t offset, void* y, int act_dtype, int param_dtype, int64_t R, int Cin, const uint64_t* rng_state,
                                    dsp_stream_t stream);
int dsp_act_dropout_train_bwd_state(const void* dy, const void* h, long ld_h, const void* bias, int act, float keep_scale, unsigned int thr,
                                    uint64_t seed, uint64_t offset, void* dh, void* dbias, void* workspace, size_t workspace_bytes,
                                    int act_dtype, int param_dtype, int64_t R, int Cin, const uint64_t* rng_state, dsp_stream_t stream);
int dsp_embed_entry_fwd_state(const int64_t* tokens, long ld_tok, const void* E, const void* P, int64_t pad, float embed_scale, float keep_scale,
                              unsigned int thr, uint64_t seed, uint64_t offset, void* y, int32_t* tok32, int32_t* pos32, int dtype, int B, int L,
                              int V, int NP, int C, const uint64_t* rng_state, dsp_stream_t stream);
int dsp_embed_entry_bwd_state(const void* dy, const int32_t* tok32, const int32_t* pos32, int64_t pad, float embed_scale, float keep_scale,
                              unsigned int thr, uint64_t seed, uint64_t offset, void* dE, void* dP, void* workspace, size_t workspace_bytes,
                              int dtype, int64_t n, int V, int NP, int C, const uint64_t* rng_state, dsp_stream_t stream);
int dsp_pos_add_fwd_state(const void* x, long ld_x, const unsigned char* padding_mask, const void* tab, const void* alpha, int pad,
                          float keep_scale, unsigned int thr, uint64_t seed, uint64_t offset, void* y, int32_t* pos32, int act_dtype,
                          int tab_dtype, int alpha_dtype, int B, int N, int NT, int C, const uint64_t* rng_state, dsp_stream_t stream);
int dsp_pos_add_bwd_state(const void* dy, const void* tab, const int32_t* pos32, float keep_scale, unsigned int thr, uint64_t seed,
                          uint64_t offset, void* dx, void* dalpha, void* workspace, size_t workspace_bytes, int act_dtype, int tab_dtype,
                          int alpha_dtype, int64_t R, int NT, int C, const uint64_t* rng_state, dsp_stream_t stream);
int dsp_relpos_attention_train_fwd_state(const void* q, const void* k, const void* v, long ld, const void* pos, const void* bias_u,
                                         const void* bias_v, const unsigned char* pad_mask, float keep_scale, unsigned int thr, uint64_t seed,
                                         uint64_t offset, void* out, float* lse, int act_dtype, int param_dtype, int B, int T, int H,
                                         const uint64_t* rng_state, dsp_stream_t stream);
int dsp_relpos_attention_train_bwd_state(const void* dout, const void* q, const void* k, const void* v, long ld, const void* pos,
                                         const void* bias_u, const void* bias_v, const unsigned char* pad_mask, const void* out, const float* lse,
                                         float keep_scale, unsigned int thr, uint64_t seed, uint64_t offset, void* dq, void* dk, void* dv,
                                         void* dpos, void* dbias_u, void* dbias_v, void* workspace, size_t workspace_bytes, int act_dtype,
                                         int param_dtype, int B, int T, int H, const uint64_t* rng_state, dsp_stream_t stream);
int dsp_mha_train_fwd_state(const void* q, long ldq, const void* k, const void* v, long ldkv, const unsigned char* pad_mask, float keep_scale,
                            unsigned int thr, uint64_t seed, uint64_t offset, void* out, float* lse, int act_dtype, int B, int N, int M, int H,
                            const uint64_t* rng_state, dsp_stream_t stream);
int dsp_mha_train_bwd_state(const void* dout, const void* q, long ldq, const void* k, const void* v, long ldkv, const unsigned char* pad_mask,
                            const float* lse, float keep_scale, unsigned int thr, uint64_t seed, uint64_t offset, void* dq, void* dk, void* dv,
                            void* workspace, size_t workspace_bytes, int act_dtype, int B, int N, int M, int H, const uint64_t* rng_state,
                            dsp_stream_t stream);
int dsp_dropout_state_advance(uint64_t* rng_state, uint64_t by, dsp_stream_t stream);

/* Conv1d(Cin, Cout, K, stride 1, dilation 1, groups 1, padding P = (K-1)/2) on CHANNELS-LAST data under autograd (csrc/conv1d_train.hip),
 * fp16 / bf16 data — the FastSpeech2 feed-forward and variance-predictor convolutions of the training step without their transposes:
 *     y [b,t,co]  = [bias[co] +] sum_k sum_ci x[b, t+k-P, ci] * W[co,ci,k]        rows outside [0, T) of a sample count as zeros
 *     dx[b,t,ci]  = sum_k sum_co dy[b, t-k+P, co] * W[co,ci,k]
 *     dW[co,ci,k] = sum_b sum_t  dy[b,t,co] * x[b, t+k-P, ci]
 *     db[co]      = sum_b sum_t  dy[b,t,co]
 *   x [B,T,Cin], y [B,T,Cout] and dy [B,T,Cout] have unit column stride and the row strides ld_x / ld_y / ld_dy (elements; at least the channel
 *   count, multiples of 8; samples T*ld apart: a contiguous tensor or the column slice of a wider one); dx [B,T,Cin] is contiguous.  W and dW
 *   [Cout,Cin,K] contiguous, nn.Conv1d's own layout, in the data dtype; dW is rounded once from fp32.  bias / db [Cout] in bias_dtype
 *   (act_dtype, or DSP_F32); bias may be NULL.  act_dtype is DSP_F16 or DSP_BF16.  Every product runs on the matrix cores with fp32
 *   accumulators; y, dx are rounded once (the bias is added in fp32 before that).  Every row is computed, padded frames included.
 *   Served: Cin and Cout multiples of 64 up to DSP_CONV1D_TRAIN_MAX_C, K odd, 1 <= K <= DSP_CONV1D_TRAIN_MAX_K, T >= 1, B*T <= 2^24.
 *   A workgroup of the forward (and of dx, the same kernel on dy with the transposed, tap-reversed weight) owns DSP_CONV1D_TRAIN_ROW_TILE rows
 *   of ONE sample.  dW: the flattened B*T rows are cut into splits of DSP_CONV1D_TRAIN_WGRAD_ROWS rows, each split's fp32 partial goes to the
 *   workspace and a tail adds the splits in ASCENDING order; db: column sums over chunks of 256 rows, the chunks added in ascending order.
 *   NO FLOAT ATOMICS and no hand-off between workgroups: the same inputs give the same bits on every call.  dx, dW, db may each be NULL, and
 *   leaving one out does not change the bits of the others; with all three NULL the call returns DSP_OK without a launch.
 *   workspace: dsp_conv1d_train_workspace_bytes(phase, ...) bytes of device memory, 16-byte aligned (DSP_ENOSPC if smaller), phase 0 for the
 *   forward (the re-laid weight), 1 for the backward (the re-laid weight and the partials); host arithmetic only, 0 for an empty problem,
 *   monotone in each size, a multiple of 16.  Nothing in it outlives the call: the weight is re-laid on every call.
 *   Bad sizes or dtype codes, null required pointers, misalignment, an output that aliases an input: DSP_EINVAL (dsp_last_error says which)
 *   before any launch; B == 0: DSP_OK without a launch. */
#define DSP_CONV1D_TRAIN_ROW_TILE 64
#define DSP_CONV1D_TRAIN_WGRAD_ROWS 1024
#define DSP_CONV1D_TRAIN_MAX_K 15
#define DSP_CONV1D_TRAIN_MAX_C 8192
size_t dsp_conv1d_train_workspace_bytes(int phase, int B, int T, int Cin, int Cout, int K);
int dsp_conv1d_train_fwd(const void* x, long ld_x, const void* w, const void* bias, void* y, long ld_y, void* workspace, size_t workspace_bytes,
                         int act_dtype, int bias_dtype, int B, int T, int Cin, int Cout, int K, dsp_stream_t stream);
int dsp_conv1d_train_bwd(const void* dy, long ld_dy, const void* x, long ld_x, const void* w, void* dx, void* dw, void* db, void* workspace,
                         size_t workspace_bytes, int act_dtype, int bias_dtype, int B, int T, int Cin, int Cout, int K, dsp_stream_t stream);

/* The same convolution with STRIDE 2 (csrc/conv1d_stride2_train.hip) — the two layers of the encoder's Conv1dSubsampler in the training step:
 *     T_out = (T - 1) / 2 + 1 (integer division)
 *     y [b,t,co]  = [bias[co] +] sum_k sum_ci x[b, 2t+k-P, ci] * W[co,ci,k]        t in [0, T_out); rows outside [0, T) of a sample count as zeros
 *     dx[b,u,ci]  = sum over the k with (u+P-k) even and 0 <= (u+P-k)/2 < T_out of sum_co dy[b, (u+P-k)/2, co] * W[co,ci,k]
 *     dW[co,ci,k] = sum_b sum_t  dy[b,t,co] * x[b, 2t+k-P, ci]
 *     db[co]      = sum_b sum_t  dy[b,t,co]
 *   The argument lists, layouts, dtypes, rounding, return codes and the workspace contract are those of dsp_conv1d_train_*; T is the INPUT
 *   length: x and dx have T rows a sample, y and dy T_out.  Rows of dx that no tap reaches (K = 1: the odd rows) and taps of dW that never land
 *   inside a sample (T = 1: all but the centre) are written as zeros.
 *   Served: Cin a multiple of 16 from 16 (the last block of 64 reduction channels may hold 16 / 32 / 48: memory behind column Cin of a row is
 *   never read), Cout a multiple of 64, both up to DSP_CONV1D_TRAIN_MAX_C, K odd, 1 <= K <= DSP_CONV1D_TRAIN_MAX_K, T >= 1, B*T <= 2^24.
 *   A workgroup of the forward owns DSP_CONV1D_TRAIN_ROW_TILE rows of y of ONE sample, one of dx as many rows of one parity of ONE sample; dW
 *   and db are cut over the flattened B*T_out rows as the stride-1 operator cuts B*T.  No float atomics, no hand-off between workgroups: the
 *   same inputs give the same bits on every call, and leaving out one of dx / dW / db does not change the bits of the others. */
size_t dsp_conv1d_s2_train_workspace_bytes(int phase, int B, int T, int Cin, int Cout, int K);
int dsp_conv1d_s2_train_fwd(const void* x, long ld_x, const void* w, const void* bias, void* y, long ld_y, void* workspace, size_t workspace_bytes,
                            int act_dtype, int bias_dtype, int B, int T, int Cin, int Cout, int K, dsp_stream_t stream);
int dsp_conv1d_s2_train_bwd(const void* dy, long ld_dy, const void* x, long ld_x, const void* w, void* dx, void* dw, void* db, void* workspace,
                            size_t workspace_bytes, int act_dtype, int bias_dtype, int B, int T, int Cin, int Cout, int K, dsp_stream_t stream);

/* fp32-accurate Conv1d ("same" padding, stride 1) on the fp16 matrix cores by operand splitting (x = xh + xl/2048, w = wh + wl/2048;
 * the products xh.wh, xh.wl, xl.wh are exact in the fp32 accumulator, the dropped xl.wl term is 2^-22 relative) — for the
 * FastSpeech2 FFT feed-forward convolutions (fairseq fastspeech2.py:42-63), which MIOpen runs at 60-70 TFLOP/s in fp32.
 * Range: operands are split into fp16 hi / lo parts, so |x| and |w| must stay below the fp16 maximum (65504; larger values become
 * inf) — true of layer-normalised activations and trained weights, not of arbitrary data; values under 6e-5 keep fewer than 22 bits.
 *   dsp_conv1d_split_pack   fp32 weight, tap-major [ntaps][M][CI] -> w_hi, w_lo (dsp_conv1d_split_packed_elems halves each)
 *   dsp_conv1d_split        x [B,T,nslices*CI] fp32, row stride ldx (a channel slice of a wider tensor is fine); out [B,T,M] fp32, row
 *                           stride ldo;  out = act([out +] bias + conv(x)), act = relu: 0 none, 1 ReLU, 2 SiLU, 3 GELU (erf).
 *                           ntaps = 1 is a Linear layer.  CI in {128, 256, 512} is the SLICE width: a wider input is nslices slices
 *                           walked inside one launch (w_hi / w_lo hold the slices' packed weights one after the other);
 *                           accumulate = 1 adds to what `out` holds.  ntaps odd, M % 4 == 0. */
long dsp_conv1d_split_packed_elems(int ntaps, int M, int CI);
int dsp_conv1d_split_pack(const float* w_tap_major, void* w_hi, void* w_lo, int ntaps, int M, int CI, dsp_stream_t stream);
int dsp_conv1d_split(const float* x, long ldx, const void* w_hi, const void* w_lo, const float* bias, float* out, long ldo,
                     int B, int T, int CI, int nslices, int M, int ntaps, int relu, int accumulate, dsp_stream_t stream);
/* same with the layer's residual connection in the epilogue:  out = res + alpha * act(bias + conv(x))   (res [B,T,M], row stride ldr;
 * out may be res) — `x + 0.5 * ffn(x)`, `x + attn(x)` without separate scale / add launches */
int dsp_conv1d_split_residual(const float* x, long ldx, const void* w_hi, const void* w_lo, const float* bias, const float* res, long ldr,
                              float alpha, float* out, long ldo, int B, int T, int CI, int nslices, int M, int ntaps, int relu,
                              dsp_stream_t stream);
/* Launch shape (the result does not depend on it, bit for bit): a workgroup stages one tile of input rows and runs a contiguous range
 * of output-channel tiles from it where the staged rows are the whole reduction (one slice, no split-K); a dense one-tap, one-slice
 * layer tiles its rows as one sequence of B * T, which is what [B,T,.] with row strides and no batch stride is.  The library exports
 * the choice as a host-only question, kept out of this header's declarations (tests pin it; it needs no GPU):
 *   int dsp_conv1d_split_plan(int B, int T, int CI, int nslices, int M, int ntaps, int has_lens, int has_ln, int tap_groups, int n_cus,
 *                             int out[6])   -> rows per launch, row tiles, output tiles, ranges of output tiles per row tile,
 *                                              output-tile width, row-tile height;  tap_groups = 0: no split-K.
 *   int dsp_conv1d_split_plan_cus(int n_cus) -> plans every later launch as for a device of n_cus CUs (0: the device's own count);
 *                                              returns the previous setting. */


/* the same for a ragged batch: lens [B] (device, int32) are the samples' valid lengths; a time tile that starts at or after
 * lens[b] + slack is padding no valid output depends on (slack = the frames of padding later convolutions still reach into: 0 for
 * position-wise layers, (K-1)/2 per convolution that follows) — it is not computed and its output rows are written as ZEROS (finite, so
 * that masked attention keys and later position-wise layers stay finite).  Rows below that bound get exactly the bits of
 * dsp_conv1d_split_residual.  res may be NULL with alpha = 1 (plain layer); lens may be NULL (dense batch). */
int dsp_conv1d_split_ragged(const float* x, long ldx, const void* w_hi, const void* w_lo, const float* bias, const float* res, long ldr,
                            float alpha, float* out, long ldo, int B, int T, int CI, int nslices, int M, int ntaps, int relu,
                            const int* lens, int slack, dsp_stream_t stream);

/* act(W . LayerNorm(x) + b) [as residual / alpha of dsp_conv1d_split_residual] for a Linear layer over exactly 256 input channels: the
 * LayerNorm (torch semantics, weight and bias [256]) is applied while the row tile is staged — a row's 256 channels sit in half a wave —
 * so pre-norm blocks (the Conformer's self-attention and convolution modules: LayerNorm -> linear_q|k|v, LayerNorm -> pointwise_conv1,
 * conformer_layer.py:254-281) need no LayerNorm launch and no normalised copy of x in HBM.  w_hi / w_lo as dsp_conv1d_split_pack packs a
 * one-tap layer; lens / slack as dsp_conv1d_split_ragged (NULL: dense). */
int dsp_linear_ln_split(const float* x, long ldx, const float* ln_w, const float* ln_b, float ln_eps, const void* w_hi, const void* w_lo,
                        const float* bias, const float* res, long ldr, float alpha, float* out, long ldo, int B, int T, int M, int act,
                        const int* lens, int slack, dsp_stream_t stream);

/* the same layer for SHORT sequences (few time tiles: the FastSpeech2 encoder's K = 9 convolutions over ~60 phoneme positions leave
 * three quarters of the CUs idle and run a 288-step reduction per workgroup): the K dimension is split over nslices * tap_groups
 * workgroups per output tile (one 512-channel input slice and ceil(ntaps / tap_groups) taps each), raw partial sums go to `workspace`
 * (dsp_conv1d_split_ksplit_workspace_bytes) and a second launch adds them in a fixed order with bias, activation and residual:
 *   out = res + alpha * act(bias + sum over parts).   Not bit-identical to dsp_conv1d_split (different association of the K sum).
 * lens / slack as dsp_conv1d_split_ragged (NULL: dense); skipped tiles contribute zero partial sums, so their rows come back as
 * res + alpha * act(bias) — finite padding. */
size_t dsp_conv1d_split_ksplit_workspace_bytes(int B, int T, int M, int nslices, int tap_groups);
int dsp_conv1d_split_ksplit(const float* x, long ldx, const void* w_hi, const void* w_lo, const float* bias, const float* res, long ldr, float alpha,
                            float* out, long ldo, int B, int T, int CI, int nslices, int M, int ntaps, int act, int tap_groups,
                            void* workspace, size_t workspace_bytes, const int* lens, int slack, dsp_stream_t stream);

/* The Conformer's feed-forward module in one matrix-core launch (+ a fixed-order reduction of the hidden-channel groups), fp32 accuracy:
 *   out = res + alpha * (W2 . act(W1 . LN(x) + b1) + b2)          (fairseq conformer_layer.py:140-146 called as x + 0.5 * ffn(x), :254-281)
 * x [B,T,C] (row stride ldx), ln_w / ln_b [C] or both NULL (no LayerNorm), W1 [H,C] and W2 [C,H] as packed by dsp_conv1d_split_pack
 * (one tap; W2 in 512-channel input slices as dsp_conv1d_split takes them), b1 [H], b2 [C] or NULL, res [B,T,C] (row stride ldr) or
 * NULL, out [B,T,C] (row stride ldo; may be res).  act as dsp_conv1d_split's relu argument (0 none, 1 ReLU, 2 SiLU, 3 GELU).
 * C = 256, H a multiple of 512.  workspace: dsp_ffn_split_workspace_bytes(B, T, C, H) bytes of device memory (partial sums).
 * post_ln_w / post_ln_b (both or neither) + out_ln [B,T,C] contiguous: the reduction also writes LayerNorm(out) there (the block that
 * follows in a pre-norm layer starts with one); out itself may then be NULL when only the normalised rows are needed. */
size_t dsp_ffn_split_workspace_bytes(int B, int T, int C, int H);
int dsp_ffn_split(const float* x, long ldx, const float* ln_w, const float* ln_b, float ln_eps, const void* w1_hi, const void* w1_lo, const float* b1,
                  const void* w2_hi, const void* w2_lo, const float* b2, const float* res, long ldr, float alpha, float* out, long ldo,
                  void* workspace, size_t workspace_bytes, int B, int T, int C, int H, int act, const float* post_ln_w, const float* post_ln_b,
                  float post_ln_eps, float* out_ln, dsp_stream_t stream);

/* LayerNorm over the last dimension (torch.nn.LayerNorm semantics: biased variance, eps inside the square root), one wave per row:
 * x, y [rows, C] fp32 contiguous (y may be x), w / b [C] or NULL, C % 4 == 0, C <= 2048, all pointers 16-byte aligned. */
int dsp_layer_norm(const float* x, const float* w, const float* b, float eps, float* y, long rows, int C, dsp_stream_t stream);

/* Conformer relative-position self-attention (fairseq conformer_layer.py / espnet RelPositionMultiHeadedAttention), fused, fp32:
 *   out[b,i,h,:] = sum_j softmax_j( ((q_i + u_h).k_j + (q_i + v_h).p_{(T-1)-i+j}) / sqrt(dk) ; keys with pad_mask[b,j] != 0 -> -inf ) v_j
 * q, k, v [B,T,H,dk] fp32 with `ld` floats between consecutive positions (H*dk for separate linear_q / linear_k / linear_v outputs,
 * 3*H*dk for the slices of a fused projection; samples T*ld apart), out [B,T,H,dk] contiguous, p [2T-1,H,dk] (linear_pos of
 * the relative positional encoding, rows for relative positions T-1 .. -(T-1)), bias_u / bias_v [H,dk], pad_mask [B,T] bytes or NULL.
 * dk = 64, any T.  Runs on the fp16 matrix cores at fp32 accuracy like dsp_attention_split (below); the [query][relative position]
 * product is formed per 32-query x 64-position block and shifted into [query][key] through LDS. */
int dsp_relpos_attention(const float* q, const float* k, const float* v, long ld, const float* p, const float* bias_u, const float* bias_v,
                         const unsigned char* pad_mask, float* out, int B, int T, int H, int DK, dsp_stream_t stream);

/* Multi-head attention with a key padding mask (fairseq modules/multihead_attention.py in eval mode: softmax(q k^T * scale + mask) v), at fp32
 * accuracy on the fp16 matrix cores (every operand split into an fp16 hi / lo pair, three MFMAs per product):
 *   out[b,i,h,:] = sum_j softmax_j( scale * q[b,i,h,:] . k[b,j,h,:] ; keys with key_pad_mask[b,j] != 0 -> -inf ) v[b,j,h,:]
 * q [B,N,H,dk], k / v [B,M,H,dk] fp32 as row-strided views (ldq / ldk / ldv floats between consecutive positions, >= H*dk, %4 == 0;
 * samples N*ldq / M*ldk / M*ldv apart: the slices of a fused q|k|v projection are served without a copy), key_pad_mask [B,M] bytes or
 * NULL, out [B,N,H*dk] contiguous.  dk = 64 or 128.  A sample whose keys are all masked gets NaN rows, as torch's soft-max does.
 * q_lens [B] (device int32) or NULL: queries at or after q_lens[b] + q_slack are padding no valid output depends on; their 32-query
 * groups are not computed and their output rows are written as zeros (see dsp_conv1d_split_ragged).
 * Range (this entry point and dsp_relpos_attention): q, k, v and the position projection are split into fp16 hi / lo parts as in
 * dsp_conv1d_split, so every entry — the rows of masked keys included, which are staged like any other before their weight becomes
 * exp(-inf) = 0 — must stay inside the fp16 range (|x| <= 65504); finite padding rows inside it cannot reach a valid query. */
int dsp_attention_split(const float* q, long ldq, const float* k, long ldk, const float* v, long ldv, const unsigned char* key_pad_mask,
                        float* out, int B, int N, int M, int H, int DK, float scale, const int* q_lens, int q_slack, dsp_stream_t stream);


#ifdef __cplusplus
}
#endif
#endif /* DASPEECH_DECODE_H */
