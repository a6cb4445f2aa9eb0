"""Inference-side HIP ops of the DASpeech hot path (C ABI: include/daspeech_decode.h).

Host-side mirror of the reference code these replace:
  graph_decode        DASpeech/models/s2s_conformer_dag_fastspeech2.py:201-243 (lookahead / greedy branch of forward_decoder)
  extract_links / extract_links_autograd   DASpeech/models/s2t_conformer_dag.py:171-212
                      (float64 q, k or log_gates: the double kernels of csrc/extract_links_f64.hip — float64 links and double-accurate
                      gradients, so the double chain of custom_ops/dag_double.py STARTS at the links: q / k / gates -> links -> dag_loss ->
                      backward; every other dtype takes the fp32 / matrix-core kernels, as before)
  posterior / expect_features   DASpeech/criterions/s2s_dag_fastspeech2_loss.py:259-263
                      (float64 alpha or beta: the double kernels of csrc/posterior_f64.hip — the reference computes the posterior in the
                      dtype of alpha, so the double DAG chain of custom_ops/dag_double.py continues through this step; every other
                      dtype takes the fp32 kernels, as before)
  predicted_durations / bucketize_embed_add / length_regulate   fairseq/fairseq/models/text_to_speech/fastspeech2.py:98-114,169-210
  bucketize_embed_add_autograd / length_regulate_autograd   the same two steps under autograd (csrc/tts_glue_grad.hip): fp32 / fp16 / bf16,
                      backward kernels that add rows in a fixed order without float atomics (bit-reproducible gradients)
  force_emit / glance_select   DASpeech/criterions/nat_dag_loss.py:130-132,223-255 — the glancing step of DAG training (csrc/glance.hip):
                      force-emit of the revealed vertices in one pass from `path` / `keep_word_mask`, with its gradient, and the reveal
                      selection by an exact radix select; these two keep their torch formulation for CPU tensors and unserved inputs
                      (set_glance_hip(False): always), with the same bits
  dwconv_bn_silu_autograd   fairseq/fairseq/modules/conformer_layer.py ConvolutionModule (depthwise_conv -> batch_norm -> SiLU) in TRAINING mode,
                      under autograd on the channels-last tensor (csrc/conformer_train.hip): fp32 / fp16 / bf16, batch statistics and the
                      running-buffer update, a backward whose reductions run in a fixed order without float atomics; ConformerLayer keeps
                      its torch lines where dwconv_bn_silu_autograd_served says no (set_conv_module_hip(False): always)
  residual_dropout_layer_norm_autograd   the residual sites of the layers in TRAINING mode, s = residual + alpha * dropout(h [+ bias]); y = LayerNorm(s)
                      (fairseq conformer_layer.py:254-281, transformer_layer.py:467-511, fastspeech2.py:42-95), under autograd
                      (csrc/residual_norm_train.hip): fp32 / fp16 / bf16, the mask recomputed from a Philox counter keyed by the default CUDA
                      generator — or, inside DropoutState.draws(), by the dropout state on the device, which is what lets a captured graph
                      (torch.cuda.graph) run this operator and the five below that draw masks, with new masks on every replay —, column sums in a
                      fixed order without float atomics; ConformerLayer / NATDecoderLayer / FFTLayer keep their
                      torch lines where residual_dropout_layer_norm_served says no (set_residual_norm_hip(False): always);
                      residual_dropout_layer_norm_checked / _sites_served are internal to those layers (no argument checks: not an API)
  bias_act_dropout_autograd   the element-wise pass between the two GEMMs of a feed-forward block in TRAINING mode, y = dropout(act(h + bias))
                      with act identity / relu / silu / gelu / glu (fairseq conformer_layer.py:140-146,86-90, transformer_layer.py:501-507,
                      s2s_conformer_dag_fastspeech2.py:24-39), under autograd (csrc/act_dropout_train.hip): fp32 / fp16 / bf16, h and bias the only
                      saved tensors (mask, activation and derivative recomputed), the bias gradient a fixed-order column sum without float
                      atomics; the layers keep their torch lines where bias_act_dropout_served says no (set_act_dropout_hip(False): always);
                      bias_act_dropout_checked / _sites_served are internal to those layers
  relpos_attention_autograd   fairseq espnet_multihead_attention.py RelPositionMultiHeadedAttention between the projections and linear_out, in
                      TRAINING mode under autograd (csrc/relpos_attention_train.hip): fp16 / bf16, scores + relative shift + mask + soft-max +
                      dropout + value product in one launch, a backward that recomputes the probabilities (no [B,h,T,T] tensor is kept) and
                      sums in a fixed order without float atomics; RelPosSelfAttention keeps its torch lines where
                      relpos_attention_autograd_served says no (set_relpos_attention_hip(False): always); relpos_attention_checked is
                      internal to that layer
  mha_attention_autograd   fairseq multihead_attention.py between the projections and out_proj — the NAT decoder's self- and encoder attention
                      (_MHA) and the FFT layers (_SelfAttention) in TRAINING mode under autograd (csrc/mha_train.hip): fp16 / bf16, query and
                      key lengths independent, q / k / v taken as views of stacked projections, scores + mask + soft-max + dropout + value
                      product in one launch, a backward of two launches that recomputes the probabilities (no [B,h,N,M] tensor is kept) without
                      float atomics, the dropout mask on the shared Philox rule; the layers keep their torch lines
                      (F.scaled_dot_product_attention) where mha_attention_autograd_served says no (set_mha_attention_hip(False): always);
                      mha_attention_checked is internal to those layers
  conv1d_channels_last_autograd  fairseq fastspeech2.py:42-70,117-151 — the Conv1d layers of PositionwiseFeedForward and VariancePredictor (stride 1,
                      "same" zero padding) in TRAINING mode on the channels-last tensor, without the transposes (csrc/conv1d_train.hip): fp16 / bf16,
                      forward, input, weight and bias gradients on the matrix cores with fp32 accumulators, x and weight the only saved tensors,
                      the weight and bias gradients fixed-order sums without float atomics; _ConvFFN / VariancePredictor keep their torch lines
                      where conv1d_channels_last_served says no (set_conv1d_train_hip(False): always); conv1d_channels_last_checked /
                      _sites_served are internal to those layers
  conv1d_stride2_channels_last_autograd  fairseq speech_to_text/modules/convolution.py:13-59 — the two Conv1d(K 5, STRIDE 2, padding 2) of the
                      encoder's Conv1dSubsampler in TRAINING mode on the channels-last tensor, without the transposes
                      (csrc/conv1d_stride2_train.hip): the same contract as conv1d_channels_last_autograd with T_out = (T-1)//2 + 1 rows of y, Cin
                      a multiple of 16 (the 80 filterbank channels) and Cout of 64; Conv1dSubsampler keeps its torch lines where
                      conv1d_stride2_channels_last_served says no (set_conv1d_stride2_train_hip(False): always);
                      conv1d_stride2_channels_last_checked / _sites_served are internal to that layer
  tts_losses_autograd   DASpeech/criterions/s2s_dag_fastspeech2_loss.py:266-290 — the l1 (+ postnet), duration, pitch and energy losses of the
                      released objective as one operator under autograd (csrc/tts_loss_train.hip): fp32 / fp16 / bf16 data, fp32 arithmetic and
                      four fp32 results, the masks taken from the lengths on the device (no mask tensor, no boolean selection, no host read),
                      the mel tensors read through their strides (no [:, :F_] slice), sums in a fixed order without float atomics, a backward of
                      one launch that recomputes the differences and writes dense gradients; S2SDAGFastSpeech2Loss keeps its torch lines
                      where tts_losses_served says no (set_tts_loss_hip(False): always); tts_losses_checked is internal to that criterion
  embed_entry_autograd   DASpeech/models (fairseq nonautoregressive_transformer.py:340-349) — the entry of DAGDecoder.extract_features,
                      dropout(embed_scale * embed_tokens(tokens) + embed_positions(positions(tokens))), as one launch under autograd
                      (csrc/embed_entry_train.hip): fp32 / fp16 / bf16 tables, positions from a cumulative count (left padding, interior
                      pads, all-pad rows), the mask on the shared Philox rule, and a backward that builds ONE inverted index for both table
                      gradients (integer atomic counts, a scan, sorted or ballot-compacted lists) and adds a table row's gradient rows in
                      ascending order in fp32 without float atomics; DAGDecoder keeps its torch lines where embed_entry_served says no
                      (set_embed_entry_hip(False): always); embed_entry_checked is internal to that layer
  positional_add_dropout_autograd   fastspeech2_noemb.py:150-151,166 — dropout(x + alpha * pos_table[positions(mask)]) of FastSpeech2NoEmb, one
                      launch under autograd (csrc/embed_entry_train.hip): row-pitched x, the table in the data dtype or fp32, dx = dy * mask
                      (dy itself without dropout) and the gradient of the one-element alpha as a fixed-order two-stage sum; the model keeps
                      its torch lines where positional_add_dropout_served says no (the same switch); positional_add_dropout_checked is
                      internal to that model
  path_features_autograd   DASpeech/criterions/s2s_dag_fastspeech2_loss.py:241-246 — the argmax strategy's features_on_path and its padding mask
                      as one launch under autograd (csrc/path_features_train.hip): fp32 / fp16 / bf16, a stable compaction of the feature rows
                      of the vertices on the path by ballots and popcounts, the width a host integer (no argsort, no host read of the widest
                      count), rows copied bit for bit, a backward of one launch that writes every gradient row once without atomics, path
                      and the sizes the only things saved; S2SDAGFastSpeech2Loss keeps its torch lines where path_features_served says no
                      (set_path_features_hip(False): always); path_features_checked is internal to that criterion
No CPU fallback elsewhere: GPU tensors only.
Layouts: whatever the equivalent torch expression takes — views at odd storage offsets, pitched or transposed tensors, broadcast
gradients — is served with its strides, copied to a dense 16-byte-aligned tensor (_dense16), or answered "not served" (_on_grid) so that the
caller's torch lines run; the alignment gates of the C ABI are never reached with something they refuse.
The training operators share one host layer: each states its dtype / shape / layout rule once, in a _..._problem() function
that returns None or the reason — the ..._served() predicate asks it behind the switch and autocast gates, the raising ..._autograd() function
raises the reason (_settled: after a dense copy where the reason begins with _LAYOUT) — and every autograd.Function launches through _launch
(device, raw stream, return code), with _dropout_call / _dropout_thr_scale for the generator bookkeeping (DropoutState / _masked where the
random state lives on the device: graph capture), _row_pitch for row-pitched views, the
dtype tables _FLOAT_CODES / _HALF_CODES, _ptr and _workspace.
"""
import ctypes
import math
import types
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _lib
from .dropout_state import (DropoutState, _DRAWS, _NOT_GPU_DEVICE, _StateDraws, _active_dropout_state, _capture_ok, _capturing,      # the dropout state on
                            _device_index)                                                                                       # the device: public here


_NOT_GPU = "expected GPU tensors (HIP op, no CPU path)"


def _gpu(name, *ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError(f"{name}: {_NOT_GPU}")


def _gpu_problem(*ts) -> Optional[str]:
    """None when _gpu has nothing against these tensors, else its reason — asked through _gpu, as every other operator asks"""
    try:
        _gpu("", *ts)
    except RuntimeError:
        return _NOT_GPU
    return None


def _mask_bytes(m: Optional[Tensor]) -> Optional[Tensor]:
    """a [B,T] padding mask as bytes for the C ABI: contiguous bool tensors are reinterpreted (no launch), anything else is converted"""
    if m is None:
        return None
    if m.dtype == torch.bool and m.is_contiguous():
        return m.view(torch.uint8)
    return m.to(torch.uint8).contiguous()


def _on_grid(*ts) -> bool:
    """every tensor given (None allowed) starts on a 16-byte boundary: the question the "not served" answers ask before a launch whose
    kernel reads with 16-byte loads — a contiguous view at an odd storage offset (a parameter of a flattened buffer, x[:, 1:] of a
    one-utterance batch) is off it"""
    for t in ts:
        if t is not None and t.data_ptr() % 16:
            return False
    return True


def _as_handed_over(*ts) -> bool:
    """every tensor given (None allowed) is contiguous and starts on a 16-byte boundary: what a served rule asks of the parameters, which a
    layer hands to the _checked function as they are"""
    for t in ts:
        if t is not None and (t.data_ptr() % 16 or not t.is_contiguous()):
            return False
    return True


def _dense16(t: Optional[Tensor]) -> Optional[Tensor]:
    """t itself when it is contiguous and starts on a 16-byte boundary, else a dense copy (fresh allocations are on the grid): what the
    wrappers without a torch path hand to the C ABI, whose gates refuse everything else.  The copy is a torch op, so gradients pass."""
    if t is None or (t.is_contiguous() and t.data_ptr() % 16 == 0):
        return t
    return t.clone(memory_format=torch.contiguous_format)


def _code(t: Tensor) -> int:
    c = _lib.DTYPE_CODES.get(str(t.dtype))
    if c is None:
        raise RuntimeError(f"unsupported dtype {t.dtype}")
    return c


# ------------------------------------------------------------------------------------------------ host layer of the training operators
_FLOAT_CODES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}      # _lib.DTYPE_CODES by dtype object: no str() on the per-site path
_HALF_CODES = {torch.float16: 1, torch.bfloat16: 2}                         # the matrix-core operators: 16-bit data only
_LAYOUT = "layout"           # how a _..._problem() reason begins where a dense copy of the data tensors settles it


def _ptr(t: Optional[Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _workspace(dev, nbytes: int) -> Optional[Tensor]:
    return torch.empty((nbytes,), dtype=torch.uint8, device=dev) if nbytes else None


def _launch(dev, entry, *args) -> None:
    """entry(*args, stream) with the device of `dev` current and `stream` its current raw stream; a non-zero return code raises under the
    entry's name.  The training operators are ~100 calls a step and the step is launch bound: the raw stream handle instead of a Stream
    object, no device guard when the device is the current one already (else the previous one is put back, also when the entry raises), and a
    plain function, not a context manager.  Tensors are allocated with their device spelled out, so only the entry needs the guard."""
    cur = torch.cuda.current_device()
    idx = cur if dev.index is None else dev.index
    if idx != cur:
        torch.cuda.set_device(idx)
    try:
        rc = entry(*args, torch._C._cuda_getCurrentRawStream(idx))
    finally:
        if idx != cur:
            torch.cuda.set_device(cur)
    if rc:
        _lib.check(rc, entry.__name__)


def _row_pitch(t: Tensor) -> Optional[int]:
    """the row pitch (elements) when t [..., C] reads as rows of unit column stride, all one pitch apart; None for any other layout"""
    C = t.shape[-1]
    if t.is_contiguous():
        return C
    if t.stride(-1) != 1 and C > 1:
        return None
    ld = span = None
    for size, stride in zip(reversed(t.shape[:-1]), reversed(t.stride()[:-1])):
        if size == 1:
            continue
        if ld is None:
            ld = stride
        elif stride != span:
            return None
        span = stride * size
    return C if ld is None else ld


def _settled(name: str, problem, args: tuple, dense: int, p: float = 0.0) -> tuple:
    """args as problem(*args) takes them: a reason that begins with _LAYOUT is settled by dense copies of the first `dense` tensors (torch
    ops: gradients pass through) and asked about once more; anything left in the way, a dropout probability outside [0, 1) included, raises"""
    why = problem(*args)
    if why is not None and why.startswith(_LAYOUT):
        args = tuple(_dense16(t) for t in args[:dense]) + tuple(args[dense:])
        why = problem(*args)
    if why is None and not 0.0 <= p < 1.0:
        why = f"dropout probability has to be in [0, 1), got {p}"
    if why is not None:
        raise RuntimeError(f"{name}: {why}")
    return args


def argmax_logp(logits: Tensor) -> Tuple[Tensor, Tensor]:
    """tok[b,j] = argmax_v logits (first max), score[b,j] = max_v log_softmax(logits)   (:207-208)."""
    _gpu("argmax_logp", logits)
    x = logits.detach().contiguous()
    B, L, V = x.shape
    lib = _lib.load()
    with torch.cuda.device(x.device):
        tok = torch.empty((B, L), dtype=torch.int32, device=x.device)
        score = torch.empty((B, L), dtype=torch.float32, device=x.device)
        _lib.check(lib.dsp_argmax_logp(_lib.ptr(x), _code(x), _lib.ptr(tok), _lib.ptr(score), B, L, V,
                                       _lib.current_stream_handle()), "dsp_argmax_logp")
    return tok, score


def lookahead_next(links: Tensor, score: Optional[Tensor], decode_beta: float = 1.0, greedy: bool = False) -> Tensor:
    """next[b,i] = argmax_j(links[b,i,j-i-1] + decode_beta*score[b,j]) on the compact layout (:209-217)."""
    _gpu("lookahead_next", links, score)
    k = links.detach().to(torch.float32).contiguous()
    B, L, TR = k.shape
    sc = None if greedy else score.detach().to(torch.float32).contiguous()
    lib = _lib.load()
    with torch.cuda.device(k.device):
        nxt = torch.empty((B, L), dtype=torch.int32, device=k.device)
        _lib.check(lib.dsp_lookahead_next(_lib.ptr(k), _lib.ptr(sc), float(decode_beta), 1 if greedy else 0, _lib.ptr(nxt),
                                          B, L, TR, _lib.current_stream_handle()), "dsp_lookahead_next")
    return nxt


def graph_decode(logits: Tensor, links: Tensor, features: Tensor, output_length: Tensor, pad: int,
                 decode_beta: float = 1.0, strategy: str = "lookahead"):
    """Lookahead / greedy graph decode.  Returns (output_tokens [B,N] int64 pad-filled, features [B,F,D] zero padded,
    features_padding_mask [B,F] bool, feature_lengths [B] int64).  One host sync (the output shapes), vs. three `.tolist()`
    round trips + per-sample Python loops in the reference (:208-243)."""
    if strategy not in ("lookahead", "greedy"):
        raise NotImplementedError(f"decode strategy {strategy}")
    _gpu("graph_decode", logits, links, features, output_length)
    B, L, V = logits.shape
    tok, score = argmax_logp(logits)
    nxt = lookahead_next(links, score, decode_beta, greedy=(strategy == "greedy"))
    feats = features.detach().contiguous()
    D = feats.shape[2]
    ol = output_length.to(torch.long).contiguous()
    lib = _lib.load()
    dev = logits.device
    with torch.cuda.device(dev):
        cap = L
        out_tok = torch.empty((B, cap), dtype=torch.long, device=dev)
        keep = torch.empty((B, cap), dtype=torch.int32, device=dev)
        nfeat = torch.empty((B,), dtype=torch.int32, device=dev)
        _lib.check(lib.dsp_follow_path(_lib.ptr(nxt), _lib.ptr(tok), _lib.ptr(ol), int(pad), _lib.ptr(out_tok), _lib.ptr(keep),
                                       _lib.ptr(nfeat), B, L, cap, _lib.current_stream_handle()), "dsp_follow_path")
        fmax = int(nfeat.max().item()) if B else 0          # the one sync: output shapes depend on it
        out_feat = torch.empty((B, fmax, D), dtype=feats.dtype, device=dev)
        if fmax:
            _lib.check(lib.dsp_gather_rows(_lib.ptr(feats), _code(feats), _lib.ptr(keep), _lib.ptr(nfeat), _lib.ptr(out_feat),
                                           B, L, D, cap, fmax, _lib.current_stream_handle()), "dsp_gather_rows")
    lens = nfeat.to(torch.long)
    mask = torch.arange(fmax, device=dev).unsqueeze(0) >= lens.unsqueeze(1)      # lengths_to_padding_mask
    return out_tok[:, : fmax + 1].contiguous(), out_feat, mask, lens


def extract_links(q: Tensor, k: Tensor, log_gates: Tensor, output_length: Tensor, TR: int,
                  dist_bias: Optional[Tensor] = None) -> Tensor:
    """Fused compact transition log-probabilities [B, L, TR] fp32 from the link predictor's q / k [B,L,H,CK] and
    log_gates [B,L,H] (s2t_conformer_dag.py:171-212); inference only (no gradient).  float64 q, k or log_gates: float64 links from the
    double kernels (dsp_extract_links_f64), the other inputs widened."""
    _gpu("extract_links", q, k, log_gates, output_length)
    if _links_f64(q, k, log_gates):
        return _links_f64_forward(q, k, log_gates, output_length, int(TR), dist_bias, False)[5]
    qf = _dense16(q.detach().to(torch.float32))
    kf = _dense16(k.detach().to(torch.float32))
    gf = _dense16(log_gates.detach().to(torch.float32))
    ol = output_length.to(torch.long).contiguous()
    B, L, H, CK = qf.shape
    bias = None if dist_bias is None else _dense16(dist_bias.detach().to(device=qf.device, dtype=torch.float32))
    lib = _lib.load()
    with torch.cuda.device(qf.device):
        links = torch.empty((B, L, TR), dtype=torch.float32, device=qf.device)
        ws = _links_workspace(lib, B, L, H, CK, TR, 0, qf.device)
        if ws is not None:                # the matrix-core kernels (csrc/extract_links_mfma.hip)
            _lib.check(lib.dsp_extract_links_ws(_lib.ptr(qf), _lib.ptr(kf), _lib.ptr(gf), _lib.ptr(ol), _lib.ptr(bias), _lib.ptr(links), None,
                                                B, L, H, CK, TR, float(CK) ** -0.5, _lib.ptr(ws), ws.numel(), _lib.current_stream_handle()),
                       "dsp_extract_links_ws")
        else:
            _lib.check(lib.dsp_extract_links(_lib.ptr(qf), _lib.ptr(kf), _lib.ptr(gf), _lib.ptr(ol), _lib.ptr(bias), _lib.ptr(links),
                                             B, L, H, CK, TR, float(CK) ** -0.5, _lib.current_stream_handle()), "dsp_extract_links")
    return links


def _links_workspace(lib, B: int, L: int, H: int, CK: int, TR: int, phase: int, device) -> Optional[Tensor]:
    """Scratch for the matrix-core link kernels (phase 0 inference / 1 training forward / 2 backward), or None when the library serves this
    shape with the fp32-FMA kernels (dsp_extract_links_workspace reports 0 bytes)."""
    import ctypes
    n = ctypes.c_size_t(0)
    _lib.check(lib.dsp_extract_links_workspace(B, L, H, CK, TR, phase, ctypes.byref(n)), "dsp_extract_links_workspace")
    return torch.empty(n.value, dtype=torch.uint8, device=device) if n.value else None


class _ExtractLinksFn(torch.autograd.Function):
    """Fused link producer under autograd: forward = dsp_extract_links_train (compact band + per-row soft-max state), backward =
    dsp_extract_links_bwd (scores recomputed per tile; no [B,L,L,H] tensor in either direction)."""

    @staticmethod
    def forward(ctx, q, k, log_gates, output_length, TR, dist_bias):
        qf = _dense16(q.detach().to(torch.float32))
        kf = _dense16(k.detach().to(torch.float32))
        gf = _dense16(log_gates.detach().to(torch.float32))
        ol = output_length.to(torch.long).contiguous()
        B, L, H, CK = qf.shape
        bias = None if dist_bias is None else _dense16(dist_bias.detach().to(device=qf.device, dtype=torch.float32))
        lib = _lib.load()
        with torch.cuda.device(qf.device):
            links = torch.empty((B, L, TR), dtype=torch.float32, device=qf.device)
            stats = torch.empty((B, L, H, 2), dtype=torch.float32, device=qf.device)
            ws = _links_workspace(lib, B, L, H, CK, TR, 1, qf.device)
            if ws is not None:
                _lib.check(lib.dsp_extract_links_ws(_lib.ptr(qf), _lib.ptr(kf), _lib.ptr(gf), _lib.ptr(ol), _lib.ptr(bias), _lib.ptr(links),
                                                    _lib.ptr(stats), B, L, H, CK, TR, float(CK) ** -0.5, _lib.ptr(ws), ws.numel(),
                                                    _lib.current_stream_handle()), "dsp_extract_links_ws")
            else:
                _lib.check(lib.dsp_extract_links_train(_lib.ptr(qf), _lib.ptr(kf), _lib.ptr(gf), _lib.ptr(ol), _lib.ptr(bias), _lib.ptr(links),
                                                       _lib.ptr(stats), B, L, H, CK, TR, float(CK) ** -0.5, _lib.current_stream_handle()),
                           "dsp_extract_links_train")
        ctx.save_for_backward(qf, kf, gf, ol, links, stats, bias if bias is not None else qf.new_empty(0))
        ctx.TR, ctx.has_bias, ctx.in_dtypes = TR, bias is not None, (q.dtype, k.dtype, log_gates.dtype)
        ctx.mark_non_differentiable(output_length)
        return links

    @staticmethod
    def backward(ctx, grad_links):
        qf, kf, gf, ol, links, stats, bias = ctx.saved_tensors
        B, L, H, CK = qf.shape
        g = _dense16(grad_links.detach().to(torch.float32))
        lib = _lib.load()
        with torch.cuda.device(qf.device):
            dq, dk = torch.empty_like(qf), torch.empty_like(kf)
            dg = torch.empty_like(gf)
            ws = _links_workspace(lib, B, L, H, CK, ctx.TR, 2, qf.device)
            if ws is not None:
                _lib.check(lib.dsp_extract_links_bwd_ws(_lib.ptr(qf), _lib.ptr(kf), _lib.ptr(gf), _lib.ptr(ol), _lib.ptr(bias if ctx.has_bias else None),
                                                        _lib.ptr(links), _lib.ptr(g), _lib.ptr(stats), _lib.ptr(dq), _lib.ptr(dk), _lib.ptr(dg),
                                                        B, L, H, CK, ctx.TR, float(CK) ** -0.5, _lib.ptr(ws), ws.numel(),
                                                        _lib.current_stream_handle()), "dsp_extract_links_bwd_ws")
            else:
                _lib.check(lib.dsp_extract_links_bwd(_lib.ptr(qf), _lib.ptr(kf), _lib.ptr(gf), _lib.ptr(ol), _lib.ptr(bias if ctx.has_bias else None),
                                                     _lib.ptr(links), _lib.ptr(g), _lib.ptr(stats), _lib.ptr(dq), _lib.ptr(dk), _lib.ptr(dg),
                                                     B, L, H, CK, ctx.TR, float(CK) ** -0.5, _lib.current_stream_handle()), "dsp_extract_links_bwd")
        dt = ctx.in_dtypes
        return dq.to(dt[0]), dk.to(dt[1]), dg.to(dt[2]), None, None, None


def _links_f64(q: Tensor, k: Tensor, log_gates: Tensor) -> bool:
    """float64 q, k or log_gates: the link producer runs on the double kernels (the other inputs are widened, which is exact) — narrowing a
    double tensor silently would hand back fp32 accuracy under a float64 dtype"""
    return q.dtype == torch.float64 or k.dtype == torch.float64 or log_gates.dtype == torch.float64


def _links_f64_forward(q, k, log_gates, output_length, TR: int, dist_bias, need_stats: bool):
    """dsp_extract_links_f64 on the widened inputs: (q, k, log_gates, out_len, dist_bias or None, links, stats or None), all float64.  No
    workspace, no matrix-core kernels."""
    for t in (q, k, log_gates, dist_bias):
        if t is not None and not t.is_floating_point():
            raise RuntimeError(f"extract_links: expected floating-point tensors, got {t.dtype}")
    qd = _dense16(q.detach().to(torch.float64))
    kd = _dense16(k.detach().to(torch.float64))
    gd = _dense16(log_gates.detach().to(torch.float64))
    ol = output_length.to(device=qd.device, dtype=torch.long).contiguous()
    B, L, H, CK = qd.shape
    bias = None if dist_bias is None else _dense16(dist_bias.detach().to(device=qd.device, dtype=torch.float64))
    if tuple(kd.shape) != (B, L, H, CK) or tuple(gd.shape) != (B, L, H) or ol.numel() != B or (bias is not None and bias.numel() < TR):
        raise RuntimeError(f"extract_links: shapes q {tuple(qd.shape)} k {tuple(kd.shape)} log_gates {tuple(gd.shape)} out_len {tuple(ol.shape)}"
                           f" dist_bias {None if bias is None else tuple(bias.shape)} TR {TR}")
    lib = _lib.load()
    with torch.cuda.device(qd.device):
        links = torch.empty((B, L, TR), dtype=torch.float64, device=qd.device)
        stats = torch.empty((B, L, H, 2), dtype=torch.float64, device=qd.device) if need_stats else None
        _lib.check(lib.dsp_extract_links_f64(_lib.ptr(qd), _lib.ptr(kd), _lib.ptr(gd), _lib.ptr(ol), _lib.ptr(bias), _lib.ptr(links), _lib.ptr(stats),
                                             B, L, H, CK, TR, float(CK) ** -0.5, _lib.current_stream_handle()), "dsp_extract_links_f64")
    return qd, kd, gd, ol, bias, links, stats


def _links_f64_backward(qd, kd, gd, ol, bias, links, stats, grad_links, TR: int):
    """dsp_extract_links_bwd_f64: (grad_q, grad_k, grad_log_gates) float64; grad_links of any floating dtype is widened"""
    B, L, H, CK = qd.shape
    g = _dense16(grad_links.detach().to(torch.float64))
    lib = _lib.load()
    with torch.cuda.device(qd.device):
        dq, dk, dg = torch.empty_like(qd), torch.empty_like(kd), torch.empty_like(gd)
        _lib.check(lib.dsp_extract_links_bwd_f64(_lib.ptr(qd), _lib.ptr(kd), _lib.ptr(gd), _lib.ptr(ol), _lib.ptr(bias), _lib.ptr(links), _lib.ptr(g),
                                                 _lib.ptr(stats), _lib.ptr(dq), _lib.ptr(dk), _lib.ptr(dg), B, L, H, CK, TR, float(CK) ** -0.5,
                                                 _lib.current_stream_handle()), "dsp_extract_links_bwd_f64")
    return dq, dk, dg


class _ExtractLinksF64Fn(torch.autograd.Function):
    """_ExtractLinksFn for float64 q, k or log_gates (dsp_extract_links_f64 / _bwd_f64): inputs, links and the per-row soft-max state are saved
    in double, the links come back float64 and every gradient in its input's dtype.  Launch helpers of its own: a double tensor cannot reach
    an fp32 launch."""

    @staticmethod
    def forward(ctx, q, k, log_gates, output_length, TR, dist_bias):
        qd, kd, gd, ol, bias, links, stats = _links_f64_forward(q, k, log_gates, output_length, TR, dist_bias, True)
        ctx.save_for_backward(qd, kd, gd, ol, links, stats, bias if bias is not None else qd.new_empty(0))
        ctx.TR, ctx.has_bias, ctx.in_dtypes = TR, bias is not None, (q.dtype, k.dtype, log_gates.dtype)
        ctx.mark_non_differentiable(output_length)
        return links

    @staticmethod
    def backward(ctx, grad_links):
        qd, kd, gd, ol, links, stats, bias = ctx.saved_tensors
        dq, dk, dg = _links_f64_backward(qd, kd, gd, ol, bias if ctx.has_bias else None, links, stats, grad_links, ctx.TR)
        dt = ctx.in_dtypes
        return dq.to(dt[0]), dk.to(dt[1]), dg.to(dt[2]), None, None, None


def extract_links_autograd(q: Tensor, k: Tensor, log_gates: Tensor, output_length: Tensor, TR: int,
                           dist_bias: Optional[Tensor] = None) -> Tensor:
    """`extract_links` with gradients w.r.t. q, k and log_gates (training: the step in front of dag_loss).  `dist_bias` is a constant.
    float64 q, k or log_gates: float64 links and double-accurate gradients (in each input's dtype) from the double kernels."""
    _gpu("extract_links", q, k, log_gates, output_length)
    if _links_f64(q, k, log_gates):
        return _ExtractLinksF64Fn.apply(q, k, log_gates, output_length, int(TR), dist_bias)
    return _ExtractLinksFn.apply(q, k, log_gates, output_length, int(TR), dist_bias)


def _is_f64(alpha: Tensor, beta: Tensor) -> bool:
    """float64 alpha or beta: the step runs on the double kernels (the other one is widened, which is exact) — narrowing a double tensor
    silently would hand back fp32 accuracy under a float64 dtype"""
    return alpha.dtype == torch.float64 or beta.dtype == torch.float64


def posterior(alpha: Tensor, beta: Tensor) -> Tensor:
    """score = exp(alpha + beta - logsumexp_j(alpha + beta)), NaN -> 0   (s2s_dag_fastspeech2_loss.py:259-260).  fp32, or float64 when
    alpha or beta is float64 (dsp_posterior_f64)."""
    _gpu("posterior", alpha, beta)
    if _is_f64(alpha, beta):
        a = alpha.detach().to(torch.float64).contiguous()
        b = beta.detach().to(torch.float64).contiguous()
        B, T, L = a.shape
        lib = _lib.load()
        with torch.cuda.device(a.device):
            score = torch.empty_like(a)
            _lib.check(lib.dsp_posterior_f64(_lib.ptr(a), _lib.ptr(b), _lib.ptr(score), B, T, L, _lib.current_stream_handle()),
                       "dsp_posterior_f64")
        return score
    a = alpha.detach().to(torch.float32).contiguous()
    b = beta.detach().to(torch.float32).contiguous()
    B, T, L = a.shape
    lib = _lib.load()
    with torch.cuda.device(a.device):
        score = torch.empty_like(a)
        _lib.check(lib.dsp_posterior(_lib.ptr(a), _lib.ptr(b), _lib.ptr(score), B, T, L, _lib.current_stream_handle()),
                   "dsp_posterior")
    return score


class _PosteriorFeaturesFn(torch.autograd.Function):
    """score @ features with the row soft-max of alpha + beta fused in (no [B,T,L] score tensor in either direction); gradient w.r.t.
    the features only — alpha / beta are detached, as the reference's are (dag_loss.py:180-186)."""

    @staticmethod
    def forward(ctx, alpha, beta, features):
        a = alpha.detach().to(torch.float32).contiguous()
        b = beta.detach().to(torch.float32).contiguous()
        f = features.detach().to(torch.float32).contiguous()
        B, T, L = a.shape
        D = f.shape[2]
        lib = _lib.load()
        with torch.cuda.device(a.device):
            out = torch.empty((B, T, D), dtype=torch.float32, device=a.device)
            lse = torch.empty((B, T), dtype=torch.float32, device=a.device)
            _lib.check(lib.dsp_posterior_features(_lib.ptr(a), _lib.ptr(b), _lib.ptr(f), _lib.ptr(out), _lib.ptr(lse), B, T, L, D,
                                                  _lib.current_stream_handle()), "dsp_posterior_features")
        ctx.save_for_backward(a, b, lse)
        ctx.fdtype, ctx.L = features.dtype, L
        return out.to(features.dtype)

    @staticmethod
    def backward(ctx, grad_out):
        a, b, lse = ctx.saved_tensors
        B, T, L = a.shape
        g = grad_out.detach().to(torch.float32).contiguous()
        D = g.shape[2]
        lib = _lib.load()
        with torch.cuda.device(a.device):
            df = torch.empty((B, L, D), dtype=torch.float32, device=a.device)
            _lib.check(lib.dsp_posterior_features_bwd(_lib.ptr(a), _lib.ptr(b), _lib.ptr(lse), _lib.ptr(g), _lib.ptr(df), B, T, L, D,
                                                      _lib.current_stream_handle()), "dsp_posterior_features_bwd")
        return None, None, df.to(ctx.fdtype)


class _PosteriorFeaturesF64Fn(torch.autograd.Function):
    """_PosteriorFeaturesFn for float64 alpha / beta (dsp_posterior_features_f64 / _bwd_f64): alpha, beta and the row log-sum-exps are saved
    in double, the features of any floating dtype are widened for the product, result and gradient come back in the features' dtype."""

    @staticmethod
    def forward(ctx, alpha, beta, features):
        a = alpha.detach().to(torch.float64).contiguous()
        b = beta.detach().to(torch.float64).contiguous()
        f = features.detach().to(torch.float64).contiguous()
        B, T, L = a.shape
        D = f.shape[2]
        lib = _lib.load()
        with torch.cuda.device(a.device):
            out = torch.empty((B, T, D), dtype=torch.float64, device=a.device)
            lse = torch.empty((B, T), dtype=torch.float64, device=a.device)
            _lib.check(lib.dsp_posterior_features_f64(_lib.ptr(a), _lib.ptr(b), _lib.ptr(f), _lib.ptr(out), _lib.ptr(lse), B, T, L, D,
                                                      _lib.current_stream_handle()), "dsp_posterior_features_f64")
        ctx.save_for_backward(a, b, lse)
        ctx.fdtype = features.dtype
        return out.to(features.dtype)

    @staticmethod
    def backward(ctx, grad_out):
        a, b, lse = ctx.saved_tensors
        B, T, L = a.shape
        g = grad_out.detach().to(torch.float64).contiguous()
        D = g.shape[2]
        lib = _lib.load()
        with torch.cuda.device(a.device):
            df = torch.empty((B, L, D), dtype=torch.float64, device=a.device)
            _lib.check(lib.dsp_posterior_features_bwd_f64(_lib.ptr(a), _lib.ptr(b), _lib.ptr(lse), _lib.ptr(g), _lib.ptr(df), B, T, L, D,
                                                          _lib.current_stream_handle()), "dsp_posterior_features_bwd_f64")
        return None, None, df.to(ctx.fdtype)


def posterior_features(alpha: Tensor, beta: Tensor, features: Tensor) -> Tensor:
    """[B,T,D] = softmax_j(alpha + beta) @ features, fused (dsp_posterior_features): the posterior never exists in HBM; differentiable
    w.r.t. `features`.  Falls back to the two-step form when the shape does not fit the kernel (odd D, rows beyond LDS).
    float64 alpha or beta: the double kernels (dsp_posterior_features_f64, any T / L / D, no fallback); the result keeps the features'
    dtype, so float64 features give a full double result."""
    _gpu("posterior_features", alpha, beta, features)
    if _is_f64(alpha, beta):
        if not features.is_floating_point():
            raise RuntimeError(f"posterior_features: features must be floating point, got {features.dtype}")
        return _PosteriorFeaturesF64Fn.apply(alpha, beta, features)
    B, T, L = alpha.shape
    if features.shape[2] % 2 or 8 * max(L, T) * 4 > 150 * 1024:
        return torch.matmul(posterior(alpha, beta).to(features.dtype), features)
    return _PosteriorFeaturesFn.apply(alpha, beta, features)


def expect_features(alpha: Tensor, beta: Tensor, features: Tensor) -> Tensor:
    """Expected hidden states of the "expect" strategy: (score @ features)[:, 1:]   (:259-263), fused: see posterior_features."""
    return posterior_features(alpha, beta, features)[:, 1:, :]


def predicted_durations(log_dur: Tensor, padding_mask: Tensor, d_factor: float = 1.0) -> Tensor:
    """clamp(round((exp(log_dur)-1)*d_factor), 0).long(), 0 at pads   (fastspeech2.py:202-205)."""
    _gpu("predicted_durations", log_dur, padding_mask)
    ld = log_dur.detach().to(torch.float32).contiguous()
    pm = padding_mask.to(torch.uint8).contiguous()
    lib = _lib.load()
    with torch.cuda.device(ld.device):
        dur = torch.empty(ld.shape, dtype=torch.long, device=ld.device)
        _lib.check(lib.dsp_durations(_lib.ptr(ld), _lib.ptr(pm), float(d_factor), _lib.ptr(dur), ld.numel(),
                                     _lib.current_stream_handle()), "dsp_durations")
    return dur


def bucketize_embed_add(x: Tensor, values: Tensor, bins: Tensor, emb_weight: Tensor) -> Tensor:
    """x + Embedding(bucketize(values, bins))  — pitch / energy embedding of the variance adaptor (fastspeech2.py:169-177,207-210).
    Returns a new tensor (x is not modified)."""
    _gpu("bucketize_embed_add", x, values, bins, emb_weight)
    out = x.detach().to(torch.float32).contiguous().clone()
    v = values.detach().to(torch.float32).contiguous()
    bn = bins.detach().to(torch.float32).contiguous()
    em = emb_weight.detach().to(torch.float32).contiguous()
    C = out.shape[-1]
    n = v.numel()
    assert out.numel() == n * C and em.shape[0] == bn.numel() + 1 and em.shape[1] == C
    lib = _lib.load()
    with torch.cuda.device(out.device):
        _lib.check(lib.dsp_bucketize_embed_add(_lib.ptr(out), _lib.ptr(v), _lib.ptr(bn), bn.numel(), _lib.ptr(em), n, C,
                                               _lib.current_stream_handle()), "dsp_bucketize_embed_add")
    return out.to(x.dtype)


def _length_regulate(x: Tensor, durations: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """the two launches of the length regulator -> (out [B,max,C], out_lens [B], cum [B,N] inclusive prefix sums of the durations)"""
    xx = x.detach().contiguous()
    dur = durations.to(torch.long).contiguous()
    B, N, C = xx.shape
    lib = _lib.load()
    dev = xx.device
    with torch.cuda.device(dev):
        cum = torch.empty((B, N), dtype=torch.long, device=dev)
        lens = torch.empty((B,), dtype=torch.long, device=dev)
        _lib.check(lib.dsp_length_regulator_lens(_lib.ptr(dur), _lib.ptr(cum), _lib.ptr(lens), B, N,
                                                 _lib.current_stream_handle()), "dsp_length_regulator_lens")
        maxlen = int(lens.max().item()) if B else 0
        out = torch.empty((B, maxlen, C), dtype=xx.dtype, device=dev)
        if maxlen:
            _lib.check(lib.dsp_length_regulator_expand(_lib.ptr(xx), _code(xx), _lib.ptr(cum), _lib.ptr(out), B, N, C, maxlen,
                                                       _lib.current_stream_handle()), "dsp_length_regulator_expand")
    return out, lens, cum


def length_regulate(x: Tensor, durations: Tensor) -> Tuple[Tensor, Tensor]:
    """LengthRegulator.forward (fastspeech2.py:98-114): rows of x [B,N,C] repeated durations[b,t] times, zero padded to the
    batch maximum; returns (out [B,max,C], out_lens [B] int64).  One sync for the output shape (the reference: B*N)."""
    _gpu("length_regulate", x, durations)
    return _length_regulate(x, durations)[:2]


EMBED_GRAD_CHUNK = 64        # DSP_EMBED_GRAD_CHUNK: rows of one bucket that one wave sums in dsp_embed_grad


class _BucketizeEmbedAddFn(torch.autograd.Function):
    """x + emb_weight[bucketize(values, bins)] in the dtype of x (dsp_bucketize_embed_add_fwd keeps the bucket indices); the gradient of x is
    the incoming gradient itself, the gradient of the table is dsp_embed_grad: per bucket, its rows in ascending order, no float atomics."""

    @staticmethod
    def forward(ctx, x, values, bins, emb_weight):
        xx = x.detach().contiguous()
        v = values.detach().to(torch.float32).contiguous()
        bn = bins.detach().to(torch.float32).contiguous()
        em = emb_weight.detach().contiguous()
        C = xx.shape[-1]
        n = v.numel()
        dev = xx.device
        with torch.cuda.device(dev):
            out = torch.empty_like(xx)
            idx = torch.empty((n,), dtype=torch.int32, device=dev)
            if n:
                _lib.check(_lib.load().dsp_bucketize_embed_add_fwd(_lib.ptr(xx), _code(xx), _lib.ptr(v), _lib.ptr(bn), bn.numel(), _lib.ptr(em),
                                                                   _lib.ptr(out), _lib.ptr(idx), n, C, _lib.current_stream_handle()),
                           "dsp_bucketize_embed_add_fwd")
        ctx.save_for_backward(idx)
        ctx.rows, ctx.C = em.shape[0], C
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        idx, = ctx.saved_tensors
        grad_emb = None
        if ctx.needs_input_grad[3]:
            n, K, C = idx.numel(), ctx.rows, ctx.C
            dev = grad_out.device
            if n == 0:
                grad_emb = torch.zeros((K, C), dtype=grad_out.dtype, device=dev)
            else:
                g = grad_out.contiguous()
                lib = _lib.load()
                with torch.cuda.device(dev):
                    grad_emb = torch.empty((K, C), dtype=g.dtype, device=dev)
                    nbytes = int(lib.dsp_embed_grad_workspace_bytes(n, K - 1, C))
                    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
                    _lib.check(lib.dsp_embed_grad(_lib.ptr(g), _code(g), _lib.ptr(idx), _lib.ptr(grad_emb), n, K - 1, C, _lib.ptr(ws), nbytes,
                                                  _lib.current_stream_handle()), "dsp_embed_grad")
        return (grad_out if ctx.needs_input_grad[0] else None), None, None, grad_emb


def bucketize_embed_add_autograd(x: Tensor, values: Tensor, bins: Tensor, emb_weight: Tensor) -> Tensor:
    """x [...,C] + Embedding(bucketize(values [...], bins)) in the dtype of x, differentiable w.r.t. x and emb_weight [len(bins)+1, C]
    (fastspeech2.py:169-177,207-210).  x and emb_weight share one dtype: fp32, fp16 or bf16 (float64 is refused, never narrowed — the
    caller keeps torch ops for it).  The backward is bit-reproducible: see _BucketizeEmbedAddFn."""
    if x.dtype != emb_weight.dtype or str(x.dtype) not in _lib.DTYPE_CODES:
        raise RuntimeError(f"bucketize_embed_add_autograd: x and emb_weight must share one of fp32 / fp16 / bf16, got {x.dtype} and {emb_weight.dtype}")
    _gpu("bucketize_embed_add_autograd", x, values, bins, emb_weight)
    if (x.dim() < 1 or emb_weight.dim() != 2 or emb_weight.shape[1] != x.shape[-1] or emb_weight.shape[0] != bins.numel() + 1
            or values.numel() * x.shape[-1] != x.numel()):
        raise RuntimeError(f"bucketize_embed_add_autograd: shapes x {tuple(x.shape)}, values {tuple(values.shape)}, bins {tuple(bins.shape)}, "
                           f"emb_weight {tuple(emb_weight.shape)} do not fit")
    return _BucketizeEmbedAddFn.apply(x, values, bins, emb_weight)


class _LengthRegulateFn(torch.autograd.Function):
    """length_regulate with a backward: grad_x[b,t] = the sum of the gradient frames of phoneme t in ascending order
    (dsp_length_regulator_bwd on the saved prefix sums; padding frames of grad_out are never read)."""

    @staticmethod
    def forward(ctx, x, durations):
        out, lens, cum = _length_regulate(x, durations)
        ctx.save_for_backward(cum)
        ctx.dims = tuple(x.shape) + (out.shape[1],)
        ctx.mark_non_differentiable(lens)
        return out, lens

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out, _grad_lens):
        cum, = ctx.saved_tensors
        B, N, C, maxlen = ctx.dims
        dev = grad_out.device
        if B * N == 0 or maxlen == 0:
            return torch.zeros((B, N, C), dtype=grad_out.dtype, device=dev), None
        g = grad_out.contiguous()
        with torch.cuda.device(dev):
            gx = torch.empty((B, N, C), dtype=g.dtype, device=dev)
            _lib.check(_lib.load().dsp_length_regulator_bwd(_lib.ptr(g), _code(g), _lib.ptr(cum), _lib.ptr(gx), B, N, C, maxlen,
                                                            _lib.current_stream_handle()), "dsp_length_regulator_bwd")
        return gx, None


def length_regulate_autograd(x: Tensor, durations: Tensor) -> Tuple[Tensor, Tensor]:
    """length_regulate, differentiable w.r.t. x [B,N,C] (fp32 / fp16 / bf16; float64 is refused, never narrowed): the two forward launches
    of length_regulate, and dsp_length_regulator_bwd as the backward.  out_lens [B] int64 carries no gradient."""
    _gpu("length_regulate_autograd", x, durations)
    if x.dim() != 3 or durations.shape != x.shape[:2]:
        raise RuntimeError(f"length_regulate_autograd: x {tuple(x.shape)} must be [B,N,C] and durations {tuple(durations.shape)} [B,N]")
    _code(x)
    return _LengthRegulateFn.apply(x, durations)


# ------------------------------------------------------------------------------------------------ glancing (csrc/glance.hip)
GLANCE_HIP = True          # set_glance_hip(False): force_emit / glance_select keep their torch formulations on every input
GLANCE_MAX_L = 16000       # DSP_GLANCE_MAX_L: the longest graph whose score row dsp_glance_reveal holds in one workgroup's LDS
GLANCE_STRATEGIES = (None, "number-random", "cmlm")
_F64_CODE = 3              # DSP_F64: taken by dsp_force_emit / dsp_force_emit_bwd only (DTYPE_CODES keeps no double entry)


def set_glance_hip(on: bool) -> bool:
    """Switch the HIP glancing ops (force_emit, glance_select) on or off; returns the previous setting.  Off: the torch formulations run, on
    GPU tensors too — the tests and tools/glance_bench.py compare the two in one process."""
    global GLANCE_HIP
    old, GLANCE_HIP = GLANCE_HIP, bool(on)
    return old


def emission_mask(path: Tensor, T: int) -> Tensor:
    """[B,T,L] bool: vertex j emits target path[b,j] (nat_dag_loss.py:225), built through a scratch row for the off-path -1"""
    B, L = path.shape
    return torch.zeros(B, T + 1, L, device=path.device, dtype=torch.bool).scatter_(1, path.unsqueeze(1) + 1, 1)[:, 1:]


def _force_emit_torch(match_all: Tensor, path: Tensor, revealed: Tensor) -> Tensor:
    """the criterion's expression (nat_dag_loss.py:130-132) with the emission mask rebuilt from the path"""
    matchmask = emission_mask(path, match_all.shape[1])
    glat_prev_mask = revealed.unsqueeze(1)
    return match_all.masked_fill(glat_prev_mask, 0) + \
        match_all.masked_fill(~matchmask, float("-inf")).masked_fill(~glat_prev_mask, 0).detach()


def force_emit_served(match_all: Tensor, path: Tensor, revealed: Tensor) -> bool:
    """True when force_emit runs dsp_force_emit on these tensors: the switch is on, GPU tensors of one device, match_all [B,T,L] fp32 or
    float64 with unit stride along L (any row pitch, any base), path [B,L] int64, revealed [B,L] bool, nothing empty."""
    if not GLANCE_HIP or match_all.dim() != 3 or match_all.dtype not in (torch.float32, torch.float64):
        return False
    B, T, L = match_all.shape
    if not (match_all.is_cuda and path.device == match_all.device and revealed.device == match_all.device):
        return False
    if tuple(path.shape) != (B, L) or tuple(revealed.shape) != (B, L) or path.dtype != torch.long or revealed.dtype != torch.bool:
        return False
    return B * T * L > 0 and B < 65536 and match_all.stride(2) == 1


class _ForceEmitFn(torch.autograd.Function):
    """dsp_force_emit / dsp_force_emit_bwd.  fp32: result and gradient are [B,T,L] views of buffers with rows pitched to a multiple of 4 (what
    the DP ops and the gather's backward take without a copy); float64: dense."""

    @staticmethod
    def _empty(B, T, L, like):
        if like.dtype == torch.float32:
            from .custom_ops.dag_loss import _pitched_empty, _round4
            return _pitched_empty(B, T, L, like.device), _round4(L)
        return torch.empty((B, T, L), dtype=like.dtype, device=like.device), L

    @staticmethod
    def forward(ctx, match_all, path, revealed):
        m = match_all.detach()
        B, T, L = m.shape
        p = path.contiguous()
        rv = revealed.contiguous()
        with torch.cuda.device(m.device):
            out, ldo = _ForceEmitFn._empty(B, T, L, m)
            _lib.check(_lib.load().dsp_force_emit(_lib.ptr(m), 0 if m.dtype == torch.float32 else _F64_CODE, m.stride(0), m.stride(1), _lib.ptr(p),
                                                  _lib.ptr(rv.view(torch.uint8)), _lib.ptr(out), ldo, B, T, L, _lib.current_stream_handle()),
                       "dsp_force_emit")
        ctx.save_for_backward(rv)
        ctx.dims = (B, T, L)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        rv, = ctx.saved_tensors
        B, T, L = ctx.dims
        g = grad_out.detach()
        with torch.cuda.device(g.device):
            gm, ldg = _ForceEmitFn._empty(B, T, L, g)
            _lib.check(_lib.load().dsp_force_emit_bwd(_lib.ptr(g), 0 if g.dtype == torch.float32 else _F64_CODE, g.stride(0), g.stride(1), g.stride(2),
                                                      _lib.ptr(rv.view(torch.uint8)), _lib.ptr(gm), ldg, B, T, L, _lib.current_stream_handle()),
                       "dsp_force_emit_bwd")
        return gm, None, None


def force_emit(match_all: Tensor, path: Tensor, revealed: Tensor) -> Tensor:
    """Force-emit of the glanced vertices (nat_dag_loss.py:130-132), out of place: a revealed vertex j (revealed [B,L] bool) may emit only the
    target it is aligned to, out[b,t,j] = match_all[b,t,j] if t == path[b,j] else -inf (path [B,L] int64, -1 = not aligned: a column of -inf);
    every other vertex keeps its column.  Values are copied.  Differentiable w.r.t. match_all: revealed columns get no gradient.
    Inputs that force_emit_served accepts take one pass of dsp_force_emit (fp32 result with pitched rows, which dag_loss / dag_best_alignment
    take without a copy; float64 dense); CPU tensors, fp16 / bf16, other strides and set_glance_hip(False) keep the torch expression."""
    if force_emit_served(match_all, path, revealed):
        return _ForceEmitFn.apply(match_all, path, revealed)
    return _force_emit_torch(match_all, path, revealed)


def _top_scored(scores: Tensor, counts: Tensor) -> Tensor:
    """1.0 where a position's score reaches its row's `counts[b]`-th largest score (nothing for a zero count) — the reference's
    threshold form (nat_dag_loss.py:236-239): ties with the threshold are all kept, and a count beyond the number of aligned vertices
    (a sample without a valid alignment: every score is the -100 fill) keeps every position."""
    thresh = scores.sort(descending=True)[0].gather(-1, (counts - 1).clip(min=0).unsqueeze(-1)).squeeze(-1)
    thresh = thresh.masked_fill(counts == 0, 100)
    return (scores >= thresh.unsqueeze(-1)).to(scores.dtype)


def _glance_served(tgt_tokens, path, guess, prev_output_tokens, unif) -> bool:
    if not GLANCE_HIP or not tgt_tokens.is_cuda or tgt_tokens.dim() != 2 or path.dim() != 2:
        return False
    B, L = path.shape
    if not (1 <= L <= GLANCE_MAX_L and B >= 1 and tgt_tokens.shape[1] >= 1):
        return False
    for t in (tgt_tokens, path, guess, prev_output_tokens):
        if t.device != tgt_tokens.device or t.dtype != torch.long:
            return False
    if tuple(guess.shape) != (B, L) or tuple(prev_output_tokens.shape) != (B, L) or tgt_tokens.shape[0] != B:
        return False
    return unif is None or (unif.dtype == torch.float32 and tuple(unif.shape) == (B, L))


@torch.no_grad()
def glance_select(tgt_tokens: Tensor, path: Tensor, guess: Tensor, prev_output_tokens: Tensor, n_tgt: Tensor, context_p: float,
                  glance_strategy: Optional[str] = None, noise: Tensor = None, unif: Tensor = None, unif_n: Tensor = None):
    """The per-vertex work of the glancing (nat_dag_loss.py:223-255) once the alignment is known -> dict(oracle [B,L] int64 the token each vertex
    is aligned to, n_right [B] int64 aligned vertices already predicted right, keep_prob [B,L] fp32, revealed [B,L] bool, glanced [B,L]
    int64 = revealed ? oracle : prev_output_tokens).  tgt_tokens [B,T], path [B,L] (-1 off the alignment), guess [B,L] the arg-max tokens,
    n_tgt [B] target lengths.  glance_strategy / noise / unif / unif_n as criterions.glat_function (draws are taken on the device, in the
    reference's order, when None).  No gradient.
    GPU tensors with L <= GLANCE_MAX_L: two launches (dsp_glance_oracle, dsp_glance_reveal — an exact selection of the threshold score instead
    of a sort); the per-sample float scalars (the counts, the probability of strategy None) stay torch expressions, so their bits are
    torch's.  CPU tensors, longer graphs, a replayed `unif` that is not fp32 and set_glance_hip(False) keep the torch formulation; both give
    the same bits."""
    if glance_strategy not in GLANCE_STRATEGIES:
        raise ValueError(f"glance strategy {glance_strategy!r} (supported: {GLANCE_STRATEGIES})")
    dev = tgt_tokens.device
    u = None if unif is None else unif.to(prev_output_tokens.device)
    hip = _glance_served(tgt_tokens, path, guess, prev_output_tokens, u)
    B, L = path.shape
    on_path = None
    if hip:
        lib = _lib.load()
        tgt, pth, gs, prev = tgt_tokens.contiguous(), path.contiguous(), guess.contiguous(), prev_output_tokens.contiguous()
        with torch.cuda.device(dev):
            oracle = torch.empty((B, L), dtype=torch.long, device=dev)
            n_right = torch.empty((B,), dtype=torch.long, device=dev)
            _lib.check(lib.dsp_glance_oracle(_lib.ptr(tgt), _lib.ptr(pth), _lib.ptr(gs), _lib.ptr(oracle), _lib.ptr(n_right), B, tgt.shape[1], L,
                                             _lib.current_stream_handle()), "dsp_glance_oracle")
    else:
        on_path = path >= 0
        oracle = tgt_tokens.gather(-1, path.clip(min=0))                   # the token each vertex is aligned to (pad-free on the path)
        n_right = ((guess == oracle) & on_path).sum(1)
    scores = counts = prob = None
    if glance_strategy is None:
        prob = (n_tgt - n_right) / n_tgt * context_p
    else:
        scores = torch.randn(oracle.shape, device=dev, dtype=torch.float) if noise is None else noise.to(dev, torch.float)
        if glance_strategy == "number-random":
            counts = ((n_tgt - n_right) * context_p + 0.5).to(torch.long)
        else:
            draw = torch.rand_like(n_tgt, dtype=torch.float) if unif_n is None else unif_n.to(dev, torch.float)
            counts = (n_tgt * draw + 0.5).to(torch.long)
    if u is None:
        u = torch.rand(prev_output_tokens.shape, device=prev_output_tokens.device)
    if hip and (counts is not None or prob.dtype == torch.float32):
        param = (prob if counts is None else counts).contiguous()
        sc = None if scores is None else scores.contiguous()
        u = u.contiguous()
        with torch.cuda.device(dev):
            keep_prob = torch.empty((B, L), dtype=torch.float32, device=dev)
            revealed = torch.empty((B, L), dtype=torch.bool, device=dev)
            glanced = torch.empty((B, L), dtype=torch.long, device=dev)
            _lib.check(lib.dsp_glance_reveal(_lib.ptr(sc), _lib.ptr(param), 0 if counts is None else 1, _lib.ptr(u), _lib.ptr(pth), _lib.ptr(oracle),
                                             _lib.ptr(prev), _lib.ptr(keep_prob), _lib.ptr(revealed.view(torch.uint8)), _lib.ptr(glanced), B, L,
                                             _lib.current_stream_handle()), "dsp_glance_reveal")
    else:
        on_path = path >= 0 if on_path is None else on_path
        if counts is None:
            keep_prob = prob.unsqueeze(-1) * on_path.float()
        else:
            keep_prob = _top_scored(scores.clone().masked_fill_(~on_path, -100), counts)
        revealed = u < keep_prob
        glanced = torch.where(revealed, oracle, prev_output_tokens)
    return {"oracle": oracle, "n_right": n_right, "keep_prob": keep_prob, "revealed": revealed, "glanced": glanced}


def restore_valid_links(links: Tensor) -> Tensor:
    """compact [B,L,TR] -> dense [B,L,L] with -inf elsewhere (s2t_conformer_dag.py:157-169); only the Viterbi strategies need
    it — lookahead / greedy run on the compact layout."""
    B, L, TR = links.shape
    idx = torch.arange(L, device=links.device).unsqueeze(1) + torch.arange(TR, device=links.device).unsqueeze(0) + 1
    idx = idx.masked_fill(idx >= L, L)
    res = torch.full((B, L, L + 1), float("-inf"), dtype=torch.float, device=links.device)
    res.scatter_(2, idx.unsqueeze(0).expand(B, -1, -1), links.float())
    return res[:, :, :L]


@torch.no_grad()
def viterbi_decode(logits: Tensor, links: Tensor, features: Tensor, output_length: Tensor, pad: int, decode_beta: float = 1.0,
                   decode_viterbibeta: float = 1.0, joint: bool = True, src_upsample_scale: float = 0.5):
    """`viterbi` / `jointviterbi` strategies of forward_decoder (s2s_conformer_dag_fastspeech2.py:244-304) on the HIP max-DP.

    The reference's loop `alpha, index = max(alpha[:, :, None] + dense_links, dim=1) [+ score * beta]` (:258-262) is the alignment
    DP K6 with an emission row that does not depend on the step: row 0 of the DP is the start vertex alone (emission
    `score[0]*beta` for jointviterbi, 0 otherwise), rows 1.. carry `score[j]*beta` (every row for jointviterbi, row 1 only for
    viterbi, :252), and the emission of each sample's FINAL vertex is 0, so that `alpha_max[m+2, L_b-1]` is exactly the
    reference's `max_j(scores[m][j] + links[j, L_b-1])` (:267-269) and `trace[m+2, L_b-1]` its arg-max (:278).  Same float
    operations in the same order (one add per transition, max, one add per cell) and the same tie rule (smallest index), so
    tokens and lengths are those of `viterbi_decode_torch`, which restates the reference loop.  The DP runs on the compact
    links — the dense `[B, L, L]` restore and the L/4 torch launches per batch are gone."""
    B, L, V = logits.shape
    TR = links.shape[2]
    dev = logits.device
    tok32, sc = argmax_logp(logits)                                       # unreduced_logits / unreduced_tokens (:207-208), one pass over the logits
    tok32 = tok32.contiguous()
    max_length = max(1, int(L / 8 / src_upsample_scale))                 # (:256)
    T = max_length + 2
    olen = output_length.to(torch.int64).contiguous()
    scb = (sc * decode_beta).contiguous()
    match = (scb if joint else torch.zeros_like(scb)).unsqueeze(1).repeat(1, T, 1)
    match[:, 1] = scb
    if not joint:
        match[:, 0] = 0
    ar = torch.arange(B, device=dev)
    match[ar, :, (olen - 1).clamp(min=0)] = 0
    links_c = links.float().contiguous()
    rows = torch.full((B,), T, dtype=torch.int64, device=dev)
    amax = torch.empty((B, T, L), dtype=torch.float32, device=dev)
    lib = _lib.load()
    # windows wider than 32 (the model's default): the blocked max-plus DP + block trace of the dense-window alignment kernels; narrow windows
    # keep the row-sequential DP with its arg-max trace.  alpha_max, tie rule and therefore tokens / lengths are the same either way.
    blocks = bool(lib.dsp_dag_max_alpha_blocks_supported(L, TR))
    trace = torch.empty((B, T, L), dtype=torch.int16 if blocks else torch.int32, device=dev)
    with torch.cuda.device(dev):
        st = _lib.current_stream_handle()
        if blocks:
            _lib.check(lib.dsp_dag_max_alpha_blocks(_lib.ptr(match), _lib.ptr(links_c), _lib.ptr(olen), _lib.ptr(rows), _lib.ptr(amax), _lib.ptr(trace),
                                                    B, T, L, TR, st), "dsp_dag_max_alpha_blocks")
        else:
            _lib.check(lib.dsp_dag_max_alpha(_lib.ptr(match), _lib.ptr(links_c), _lib.ptr(olen), _lib.ptr(rows), _lib.ptr(amax), _lib.ptr(trace),
                                             B, T, L, TR, st), "dsp_dag_max_alpha")
        best = amax[ar, 2:, (olen - 1).clamp(min=0)]                     # [B, M]: best score of every length (:267-269)
        lengths = (torch.arange(max_length, device=dev) + 1).unsqueeze(0).float()
        _, pred_length = torch.max(best / lengths ** decode_viterbibeta, dim=1)
        pred_length = pred_length + 1                                    # (:275-276)
        path = torch.empty((B, L), dtype=torch.int64, device=dev)
        start_rows = (pred_length + 2).contiguous()                       # bound to a name: must outlive the launch
        if blocks:
            _lib.check(lib.dsp_dag_backtrace_blocks(_lib.ptr(amax), _lib.ptr(trace), _lib.ptr(links_c), _lib.ptr(olen), _lib.ptr(start_rows), _lib.ptr(path),
                                                    B, T, L, TR, st), "dsp_dag_backtrace_blocks")
        else:
            _lib.check(lib.dsp_dag_backtrace(_lib.ptr(trace), _lib.ptr(olen), _lib.ptr(start_rows), _lib.ptr(path), B, T, L, st),
                       "dsp_dag_backtrace")
    # the token pass (:283-299) in one kernel: vertices visited at DP rows 1 .. pred_length in graph order, a token kept if it is the last
    # visited one or (not pad and different from the next visited token).  The final vertex out of reach within max_length steps (a window far
    # narrower than the model's): every candidate score is -inf, the reference's arg-maxes all return index 0 (:267-278) and it emits the one
    # token of vertex 0 — reproduced on the device, not "fixed" (no host-side branch: it would synchronise every decode batch for a corner case)
    unreach = torch.isneginf(best).all(dim=1).to(torch.uint8).contiguous()
    feats = features.detach().contiguous()
    D = feats.shape[2]
    with torch.cuda.device(dev):
        cap = L
        out_tok = torch.empty((B, cap), dtype=torch.long, device=dev)
        keep = torch.empty((B, cap), dtype=torch.int32, device=dev)
        nk = torch.empty((B,), dtype=torch.int32, device=dev)
        pl = pred_length.to(torch.int64).contiguous()
        _lib.check(lib.dsp_viterbi_collect(_lib.ptr(path), _lib.ptr(pl), _lib.ptr(unreach), _lib.ptr(tok32), int(pad), _lib.ptr(out_tok), _lib.ptr(keep),
                                           _lib.ptr(nk), B, L, cap, _lib.current_stream_handle()), "dsp_viterbi_collect")
        fmax = int(nk.max().item()) if B else 0              # the one sync: output shapes depend on it
        out_feat = torch.empty((B, fmax, D), dtype=feats.dtype, device=dev)
        if fmax:
            _lib.check(lib.dsp_gather_rows(_lib.ptr(feats), _code(feats), _lib.ptr(keep), _lib.ptr(nk), _lib.ptr(out_feat),
                                           B, L, D, cap, fmax, _lib.current_stream_handle()), "dsp_gather_rows")
    n_keep = nk.to(torch.long)
    mask = torch.arange(fmax, device=dev).unsqueeze(0) >= n_keep.unsqueeze(1)
    return out_tok[:, :fmax].contiguous(), out_feat, mask, n_keep


def viterbi_decode_torch(logits: Tensor, links: Tensor, features: Tensor, output_length: Tensor, pad: int, decode_beta: float = 1.0,
                         decode_viterbibeta: float = 1.0, joint: bool = True, src_upsample_scale: float = 0.5):
    """The same decode as a restatement of the reference loop in torch (device-agnostic; the checker of `viterbi_decode`):
    max_length = int(L / 8 / scale) max-product steps over the dense links, length-normalised best end, back-trace by batched
    gathers (the reference back-traces per sample on the host).  Returns like graph_decode."""
    B, L, V = logits.shape
    dense = restore_valid_links(links)
    logp = torch.log_softmax(logits.float(), dim=-1)
    sc, tok = logp.max(dim=-1)                                           # unreduced_logits / unreduced_tokens (:207-208)
    alpha = dense[:, 0].clone()                                          # (:248) — the reference aliases links[:,0]; harmless
    if joint:
        alpha = alpha + sc[:, 0].unsqueeze(1) * decode_beta              # (:249-250)
    alpha = alpha + sc * decode_beta                                     # (:252) applied for both strategies
    max_length = max(1, int(L / 8 / src_upsample_scale))                 # (:256)
    scores, indexs = [alpha], []
    for _ in range(max_length - 1):
        alpha, index = torch.max(alpha.unsqueeze(-1) + dense, dim=1)     # (:258)
        if joint:
            alpha = alpha + sc * decode_beta
        scores.append(alpha); indexs.append(index)
    scores = torch.stack(scores, 0)                                      # [M,B,L]
    ar = torch.arange(B, device=logits.device)
    link_last = dense[ar, :, (output_length - 1)].unsqueeze(0)           # link of every vertex into the final vertex (:267)
    best, max_idx = torch.max(scores + link_last, dim=-1)                # [M,B]
    lengths = (torch.arange(max_length, device=logits.device) + 1).unsqueeze(-1).float()
    _, pred_length = torch.max(best / lengths ** decode_viterbibeta, dim=0)
    pred_length = pred_length + 1                                        # (:275-276)
    j = max_idx.gather(0, (pred_length - 1).unsqueeze(0)).squeeze(0)     # end vertex per sample (:278)
    # batched back-trace: path[b, k] = k-th vertex from the END
    path = torch.full((B, max_length), -1, dtype=torch.long, device=logits.device)
    path[:, 0] = j
    if indexs:
        idx_all = torch.stack(indexs, 0)                                 # [M-1,B,L]
        for k in range(max_length - 1):
            step = pred_length - k - 2                                   # (:287) indexs[length-k-2]
            live = step >= 0
            nj = idx_all[step.clamp(min=0), ar, j]
            j = torch.where(live, nj, j)
            path[:, k + 1] = torch.where(live, j, torch.full_like(j, -1))
    valid = path >= 0
    ptok = tok.gather(1, path.clamp(min=0))
    nxt_tok = torch.cat([torch.full((B, 1), -12345, device=ptok.device, dtype=ptok.dtype), ptok[:, :-1]], dim=1)   # token visited just before (backward order)
    keep = valid & ((torch.arange(max_length, device=ptok.device).unsqueeze(0) == 0) | ((ptok != pad) & (ptok != nxt_tok)))
    n_keep = keep.sum(1)
    fmax = int(n_keep.max().item())
    # forward order = reversed backward order; compact the kept entries to the left
    order = torch.argsort((~keep.flip(1)).to(torch.int8), dim=1, stable=True)
    fwd_path = path.flip(1).gather(1, order)[:, :fmax]
    fwd_tok = ptok.flip(1).gather(1, order)[:, :fmax]
    mask = torch.arange(fmax, device=ptok.device).unsqueeze(0) >= n_keep.unsqueeze(1)
    out_tok = fwd_tok.masked_fill(mask, pad)
    out_feat = features.gather(1, fwd_path.clamp(min=0).unsqueeze(-1).expand(-1, -1, features.shape[-1])).masked_fill(mask.unsqueeze(-1), 0)
    return out_tok, out_feat, mask, n_keep


def dwconv_bn_silu(x: Tensor, conv_weight: Tensor, bn: "torch.nn.BatchNorm1d") -> Tensor:
    """SiLU(BatchNorm_eval(depthwise_conv1d(x))) on channels-last x [B,T,C] — the middle of the Conformer convolution module in
    eval mode (include/daspeech_decode.h: dsp_dwconv_bn_silu).  conv_weight is the Conv1d(C, C, K, groups=C) weight [C,1,K]."""
    _gpu("dwconv_bn_silu", x, conv_weight)
    xf = _dense16(x.detach().to(torch.float32))            # .contiguous() alone keeps a contiguous view at an odd offset, which the C side refuses
    B, T, C = xf.shape
    wt = _dense16(conv_weight.detach().to(torch.float32).reshape(C, -1))
    K = wt.shape[1]
    f = lambda t: None if t is None else _dense16(t.detach().to(torch.float32))
    bw, bb, bm, bv = f(bn.weight), f(bn.bias), f(bn.running_mean), f(bn.running_var)
    lib = _lib.load()
    with torch.cuda.device(xf.device):
        y = torch.empty_like(xf)
        _lib.check(lib.dsp_dwconv_bn_silu(_lib.ptr(xf), _lib.ptr(wt), _lib.ptr(bw), _lib.ptr(bb), _lib.ptr(bm), _lib.ptr(bv), float(bn.eps),
                                          _lib.ptr(y), B, T, C, K, _lib.current_stream_handle()), "dsp_dwconv_bn_silu")
    return y.to(x.dtype)


# ------------------------------------------------------------------------------------------------ convolution module under autograd (csrc/conformer_train.hip)
CONV_MODULE_HIP = True       # set_conv_module_hip(False): ConformerLayer keeps its torch lines in training on every input
CONVMOD_TIME_TILE = 8        # DSP_CONVMOD_TIME_TILE: frames per thread
CONVMOD_CHUNK_TILES = 16     # DSP_CONVMOD_CHUNK_TILES: time tiles per reduction chunk (one workspace partial each)
CONVMOD_KERNEL_SIZES = (3, 7, 15, 31)


def set_conv_module_hip(on: bool) -> bool:
    """Switch the HIP convolution-module operator of ConformerLayer's training branch on or off; returns the previous setting.  Off:
    dwconv_bn_silu_autograd_served answers False and the torch lines run — the tests and tools/convmod_bench.py compare the two in one process."""
    global CONV_MODULE_HIP
    old, CONV_MODULE_HIP = CONV_MODULE_HIP, bool(on)
    return old


def _bn_tensors(bn):
    return [t for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var) if t is not None]


def _convmod_problem(x, conv_weight, bn) -> Optional[str]:
    """None when dsp_dwconv_bn_silu_train_fwd / _bwd compute this module on (a dense copy of) x, else what is in the way: dtypes, then GPU
    tensors, then shapes"""
    ts = _bn_tensors(bn)
    if (x.dtype not in _FLOAT_CODES or conv_weight.dtype != x.dtype or bn.weight is None or bn.bias is None
            or not (all(t.dtype == x.dtype for t in ts) or all(t.dtype == torch.float32 for t in ts))):
        return ("expected GPU tensors with x and conv_weight in one of fp32 / fp16 / bf16 and the BatchNorm parameters and buffers in that dtype "
                f"or all in fp32, got {x.dtype}, {conv_weight.dtype} and {[str(t.dtype) for t in ts]}")
    why = _gpu_problem(x, conv_weight, *ts)
    if why is not None:
        return why
    C, K = (x.shape[-1], conv_weight.shape[-1]) if x.dim() == 3 and conv_weight.dim() == 3 else (0, 0)
    if (C < 1 or C % (16 // x.element_size()) or not 2 <= x.shape[0] * x.shape[1] <= (1 << 24)
            or tuple(conv_weight.shape) != (C, 1, K) or K not in CONVMOD_KERNEL_SIZES or bn.num_features != C or bn.momentum is None
            or any(t.device != x.device for t in [conv_weight] + ts)):
        return (f"x {tuple(x.shape)} / conv_weight {tuple(conv_weight.shape)} are not served (x [B,T,C] with B*T >= 2 and C a multiple of the "
                "channels in 16 bytes, conv_weight [C,1,K] with K in 3 / 7 / 15 / 31, a momentum, everything on one device)")
    return None


def dwconv_bn_silu_autograd_served(x: Tensor, conv: "torch.nn.Conv1d", bn: "torch.nn.BatchNorm1d") -> bool:
    """True when dwconv_bn_silu_autograd serves ConformerLayer's training branch on these arguments: the switch is on, autocast off, x a
    contiguous GPU tensor [B,T,C] in fp32 / fp16 / bf16 with B*T >= 2 and C a multiple of the channels in 16 bytes (4, or 8 for the 16-bit
    dtypes: a lane owns one 16-byte group), conv the depthwise Conv1d(C, C, K, padding=(K-1)//2, groups=C, bias=False) with K in 3 / 7 / 15 /
    31 and the dtype of x, bn an affine BatchNorm1d(C) in training mode with a momentum, its parameters and buffers all in that dtype or all
    in fp32.  Everything else (eval mode with gradients, autocast, float64, CPU) keeps the torch formulation."""
    if not CONV_MODULE_HIP or torch.is_autocast_enabled():
        return False
    if _convmod_problem(x, conv.weight, bn) is not None:
        return False
    K = conv.kernel_size[0]
    if (K != conv.weight.shape[-1] or conv.bias is not None or conv.stride[0] != 1 or conv.dilation[0] != 1 or conv.groups != x.shape[2]
            or conv.padding != ((K - 1) // 2,) or getattr(conv, "padding_mode", "zeros") != "zeros" or not (bn.training and bn.affine)):
        return False
    return x.is_contiguous() and x.data_ptr() % 16 == 0      # 16-byte loads of x: a contiguous view at an odd offset keeps the torch lines


class _DwconvBnSiluTrainFn(torch.autograd.Function):
    """dsp_dwconv_bn_silu_train_fwd / _bwd.  Saved for the backward: x, the weights, gamma, beta and the fp32 batch mean / invstd — z is
    recomputed from x.  The running buffers are updated in place by the forward (the batch statistics never visit the host)."""

    @staticmethod
    def forward(ctx, x, w, gamma, beta, running_mean, running_var, momentum, eps):
        xx = _dense16(x.detach())
        B, T, C = xx.shape
        wt = w.detach().reshape(C, -1).contiguous()
        K = wt.shape[1]
        g, b = gamma.detach().contiguous(), beta.detach().contiguous()
        lib = _lib.load()
        dev = xx.device
        y = torch.empty_like(xx)
        mean = torch.empty((C,), dtype=torch.float32, device=dev)
        invstd = torch.empty((C,), dtype=torch.float32, device=dev)
        if B:
            nbytes = int(lib.dsp_dwconv_bn_silu_train_workspace_bytes(B, T, C, K))
            ws = _workspace(dev, nbytes)
            _launch(dev, lib.dsp_dwconv_bn_silu_train_fwd, xx.data_ptr(), wt.data_ptr(), g.data_ptr(), b.data_ptr(), _ptr(running_mean),
                    _ptr(running_var), float(momentum), float(eps), y.data_ptr(), mean.data_ptr(), invstd.data_ptr(), _ptr(ws), nbytes,
                    _FLOAT_CODES[xx.dtype], _FLOAT_CODES[g.dtype], B, T, C, K)
        ctx.save_for_backward(xx, wt, g, b, mean, invstd)
        ctx.wshape = tuple(w.shape)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        xx, wt, g, b, mean, invstd = ctx.saved_tensors
        B, T, C = xx.shape
        K = wt.shape[1]
        need = ctx.needs_input_grad
        gy = _dense16(grad_y)                          # autograd may hand over a narrow of a larger gradient, or a broadcast
        lib = _lib.load()
        dev = xx.device
        dx = torch.empty_like(xx) if need[0] else None
        dw = torch.empty_like(wt) if need[1] else None
        dg = torch.empty_like(g) if need[2] else None
        db = torch.empty_like(b) if need[3] else None
        if B and any(need[:4]):
            nbytes = int(lib.dsp_dwconv_bn_silu_train_workspace_bytes(B, T, C, K))
            ws = _workspace(dev, nbytes)
            _launch(dev, lib.dsp_dwconv_bn_silu_train_bwd, xx.data_ptr(), wt.data_ptr(), g.data_ptr(), b.data_ptr(), mean.data_ptr(),
                    invstd.data_ptr(), gy.data_ptr(), _ptr(dx), _ptr(dw), _ptr(dg), _ptr(db), _ptr(ws), nbytes, _FLOAT_CODES[xx.dtype],
                    _FLOAT_CODES[g.dtype], B, T, C, K)
        return dx, (None if dw is None else dw.view(ctx.wshape)), dg, db, None, None, None, None


def dwconv_bn_silu_autograd(x: Tensor, conv_weight: Tensor, bn: "torch.nn.BatchNorm1d") -> Tensor:
    """SiLU(BatchNorm_train(depthwise_conv1d(x))) on channels-last x [B,T,C] — the middle of the Conformer convolution module in training
    mode, differentiable w.r.t. x, conv_weight [C,1,K], bn.weight and bn.bias (include/daspeech_decode.h: dsp_dwconv_bn_silu_train_fwd /
    _bwd).  Batch statistics over all B*T frames (no padding mask, as the reference); bn.running_mean / running_var / num_batches_tracked
    are updated as nn.BatchNorm1d updates them, and left alone with track_running_stats=False.  fp32 / fp16 / bf16 (float64 is refused,
    never narrowed); the BatchNorm tensors in the dtype of x or all in fp32.  Bit-reproducible forward and backward."""
    why = _convmod_problem(x, conv_weight, bn)
    if why is not None:
        raise RuntimeError(f"dwconv_bn_silu_autograd: {why}")
    track = bn.running_mean is not None and bn.running_var is not None
    y = _DwconvBnSiluTrainFn.apply(x, conv_weight, bn.weight, bn.bias, bn.running_mean if track else None, bn.running_var if track else None,
                                   bn.momentum, bn.eps)
    if track and bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    return y


# ------------------------------------------------------------------------------------------------ residual + dropout + LayerNorm under autograd (csrc/residual_norm_train.hip)
RESIDUAL_NORM_HIP = True     # set_residual_norm_hip(False): the layers keep their torch lines in training on every input
RESNORM_CHUNK_ROWS = 32      # DSP_RESNORM_CHUNK_ROWS: rows per reduction chunk of the backward (one workspace partial each)
RESNORM_MAX_C = 2048


def set_residual_norm_hip(on: bool) -> bool:
    """Switch the HIP residual + dropout + LayerNorm operator of the training branches (ConformerLayer, NATDecoderLayer, FastSpeech2 FFTLayer)
    on or off; returns the previous setting.  Off: residual_dropout_layer_norm_served answers False and the torch lines run."""
    global RESIDUAL_NORM_HIP
    old, RESIDUAL_NORM_HIP = RESIDUAL_NORM_HIP, bool(on)
    return old


def dropout_threshold(p: float) -> int:
    """thr = ceil(p * 2^24), in double: an element is kept when the top 24 bits of its Philox word are >= thr (p = 0: 0, everything kept)"""
    if not 0.0 <= p < 1.0:
        raise ValueError(f"dropout probability has to be in [0, 1), got {p}")
    return min(int(math.ceil(float(p) * 16777216.0)), 1 << 24)


def _reserve_dropout_stream(device) -> Tuple[int, int]:
    """(seed, offset) of the default CUDA generator of `device` for one masked call, and the generator's offset moved on by 4 (torch's own
    kernels keep it a multiple of 4).  Host operations only: no launch, no sync.  The same generator state gives the same pair, so
    torch.cuda.manual_seed / set_rng_state reproduce and restore the masks."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    gen = torch.cuda.default_generators[idx]
    seed, offset = int(gen.initial_seed()), int(gen.get_offset())
    gen.set_offset(offset + 4)
    return seed & 0xFFFFFFFFFFFFFFFF, offset


def _dropout_call(p: float, training: bool, device):
    """(p_eff, seed, offset) of one call of a training operator: dropout is active with `training and p > 0`, and only then is a (seed, offset)
    reserved (the generator's offset moves on by 4, else by nothing).  Inside DropoutState.draws() on that device the pair is
    (_StateDraws, intra) instead — the state on the device and the call's distance from its offset; the generator is not touched."""
    p_eff = float(p) if training else 0.0
    if p_eff > 0.0:
        if _DRAWS:
            st = _DRAWS.get(_device_index(device))
            if st is not None:
                return (p_eff,) + st._reserve()
        seed, offset = _reserve_dropout_stream(device)
        return p_eff, seed, offset
    return p_eff, 0, 0


def _masked(lib, name: str, seed, offset) -> tuple:
    """(entry, seed, offset, tail) of a masked launch: the entry `name` with host integers; for a _StateDraws the entry name_state with
    (0, intra) and the state pointer as the tail — the argument before the stream.  Raises when the scope that reserved the call has exited."""
    if seed.__class__ is _StateDraws:
        return getattr(lib, name + "_state"), 0, offset, (seed.pointer(),)
    return getattr(lib, name), seed, offset, ()


def _dropout_thr_scale(p: float) -> Tuple[int, float]:
    """(thr, keep scale) the kernels take for the effective probability p: (0, 1.0) without dropout"""
    thr = dropout_threshold(p) if p > 0.0 else 0
    return thr, (1.0 / (1.0 - p) if thr else 1.0)


def dropout_keep_mask(seed, offset: int, p: float, shape, device=None) -> Tensor:
    """The keep mask (bool, `shape`) that residual_dropout_layer_norm_autograd applies for (seed, offset, p) to a contiguous tensor of that
    shape (dsp_dropout_keep_mask): for tests and diagnostics — the operator itself stores no mask.  The device form takes a DropoutState in
    place of the seed and an intra in place of the offset, dropout_keep_mask(state, intra, p, shape): the mask for seed = state[0],
    offset = state[1] + intra, read on the device when the launch runs (dsp_dropout_keep_mask_state) — the one a masked call that reserved
    `intra` inside state.draws() applies; it works inside and outside a scope and does not move the state."""
    if isinstance(seed, DropoutState):
        device, tail = seed.device, (_lib.ptr(seed.tensor),)
        entry, name, seed = _lib.load().dsp_dropout_keep_mask_state, "dsp_dropout_keep_mask_state", 0
    else:
        device, tail = torch.device(device), ()
        if device.type != "cuda":
            raise RuntimeError(f"dropout_keep_mask: {_NOT_GPU_DEVICE}")
        entry, name = _lib.load().dsp_dropout_keep_mask, "dsp_dropout_keep_mask"
    with torch.cuda.device(device):
        out = torch.empty(tuple(shape), dtype=torch.uint8, device=device)
        _lib.check(entry(int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset), dropout_threshold(p), _lib.ptr(out), out.numel(), *tail,
                         _lib.current_stream_handle()), name)
    return out.view(torch.bool)


def _resnorm_shape_ok(x) -> bool:
    C = x.shape[-1] if x.dim() >= 1 else 0
    return x.dim() >= 2 and C >= 1 and C % (16 // x.element_size()) == 0 and C <= RESNORM_MAX_C and 1 <= x.numel() // C <= (1 << 24)


def _resnorm_param_dtypes_ok(w, b, bias, dt) -> bool:
    """an affine LayerNorm whose weight w and bias b (and `bias`) are in dt or all in fp32: the dtype question about the parameters, asked by
    _resnorm_problem and once per site by _sites_served"""
    if w is None or b is None:
        return False
    pd = w.dtype
    return (pd == dt or pd == torch.float32) and b.dtype == pd and (bias is None or bias.dtype == pd)


def _resnorm_param_shapes_ok(normalized_shape, w, b, bias, C: int, dev) -> bool:
    """a LayerNorm(C) whose weight and bias (and `bias`) are [C] tensors on dev: the shape question about the parameters, asked after
    _resnorm_param_dtypes_ok by the same two"""
    return (len(normalized_shape) == 1 and normalized_shape[0] == C and w.dim() == 1 and w.numel() == C and b.dim() == 1 and b.numel() == C
            and w.device == dev and b.device == dev and (bias is None or (bias.dim() == 1 and bias.numel() == C and bias.device == dev)))


def _resnorm_problem(h, residual, ln, bias) -> Optional[str]:
    """None when dsp_resnorm_train_fwd / _bwd compute this site on (dense copies of) these tensors, else what is in the way: dtypes, then GPU
    tensors, then shapes.  `bias` is not read without h, so not asked about."""
    x = residual
    bias = bias if h is not None else None
    w, b = getattr(ln, "weight", None), getattr(ln, "bias", None)
    params = [t for t in (w, b, bias) if t is not None]
    if x.dtype not in _FLOAT_CODES or (h is not None and h.dtype != x.dtype) or not _resnorm_param_dtypes_ok(w, b, bias, x.dtype):
        return ("expected GPU tensors with h and residual in one of fp32 / fp16 / bf16 and an affine LayerNorm whose weight and bias (and `bias`) "
                f"are in that dtype or all in fp32, got {[str(t.dtype) for t in (x, h) if t is not None]} and {[str(t.dtype) for t in params]}")
    why = _gpu_problem(x, h, *params)
    if why is not None:
        return why
    if (not _resnorm_shape_ok(x) or (h is not None and (h.shape != x.shape or h.device != x.device))
            or not _resnorm_param_shapes_ok(ln.normalized_shape, w, b, bias, x.shape[-1], x.device)):
        return (f"residual {tuple(x.shape)} / h {None if h is None else tuple(h.shape)} / LayerNorm {tuple(ln.normalized_shape)} are not served "
                f"([..., C] with C a multiple of the elements in 16 bytes, C <= {RESNORM_MAX_C}, 1 <= rows <= 2^24, h of the shape of residual, "
                "LayerNorm(C), everything on one device)")
    return None


def residual_dropout_layer_norm_served(h: Optional[Tensor], residual: Tensor, ln: "torch.nn.LayerNorm", *, bias: Optional[Tensor] = None,
                                       masked: Optional[bool] = None) -> bool:
    """True when residual_dropout_layer_norm_autograd serves a training branch on these arguments: the switch is on, autocast off, residual
    (and h, when given: same shape, dtype and device) a contiguous GPU tensor [..., C] in fp32 / fp16 / bf16 with C a multiple of the elements
    in 16 bytes, C <= 2048 and at most 2^24 rows, ln an affine LayerNorm(C) whose weight and bias (and `bias`) are in that dtype or all in
    fp32; while a graph is being captured only inside DropoutState.draws() on that device (the state on the device takes the place of the host's random offset) or with masked=False (a call that draws no mask: p == 0 or not training) — `masked` left at None means "h is given": the call of this very question; a caller that asks with h = None as a stand-in for an h it
    has yet to make dense says what its call will draw.  Everything else keeps the torch lines."""
    if not RESIDUAL_NORM_HIP or torch.is_autocast_enabled():
        return False
    if _resnorm_problem(h, residual, ln, bias) is not None:
        return False
    if not residual.is_contiguous() or (h is not None and not h.is_contiguous()):
        return False
    if not _on_grid(residual, h, ln.weight, ln.bias, bias if h is not None else None):         # 16-byte loads of every one of them
        return False
    return _capture_ok(residual.device, h is not None if masked is None else masked)


def residual_dropout_layer_norm_sites_served(x: Tensor, sites, masked: bool = True) -> bool:
    """residual_dropout_layer_norm_served(x, x, ln, bias=bias) for every (ln, bias) of `sites` — the residual sites of ONE layer, whose block
    outputs have the shape, dtype and device of the layer input x — with the questions about x, the switch, autocast and the stream asked
    once: a layer asks this once per forward, and the step follows the host time of these sites.  `masked` as there."""
    if not RESIDUAL_NORM_HIP or torch.is_autocast_enabled():
        return False
    dt = x.dtype
    if not (x.is_cuda and dt in _FLOAT_CODES and x.is_contiguous() and _resnorm_shape_ok(x) and x.data_ptr() % 16 == 0):
        return False
    C, dev = x.shape[-1], x.device
    for ln, bias in sites:
        w, b = ln.weight, ln.bias
        if not (_resnorm_param_dtypes_ok(w, b, bias, dt) and _resnorm_param_shapes_ok(ln.normalized_shape, w, b, bias, C, dev)
                and _on_grid(w, b, bias)):
            return False
    return _capture_ok(dev, masked)


class _ResidualNormTrainFn(torch.autograd.Function):
    """dsp_resnorm_train_fwd / _bwd.  Saved for the backward: s (an output; the residual itself when h is None), the fp32 row statistics and
    gamma — no mask: the backward draws it again from (seed, offset, thr)."""

    @staticmethod
    def forward(ctx, h, residual, bias, gamma, beta, eps, alpha, p, seed, offset):
        C = residual.shape[-1]
        R = residual.numel() // C
        has_h = h is not None
        has_bias = has_h and bias is not None
        thr, scale = _dropout_thr_scale(p if has_h else 0.0)
        lib = _lib.load()
        dev = residual.device
        y = torch.empty_like(residual)
        s = torch.empty_like(residual) if has_h else None
        stats = torch.empty((R, 2), dtype=torch.float32, device=dev)
        entry, sd, off, tail = _masked(lib, "dsp_resnorm_train_fwd", seed, offset)
        _launch(dev, entry, h.data_ptr() if has_h else None, residual.data_ptr(), bias.data_ptr() if has_bias else None,
                gamma.data_ptr(), beta.data_ptr(), eps, alpha, scale, thr, sd, off, s.data_ptr() if has_h else None, y.data_ptr(),
                stats.data_ptr(), _FLOAT_CODES[residual.dtype], _FLOAT_CODES[gamma.dtype], R, C, *tail)
        ctx.save_for_backward(s if has_h else residual, stats, gamma)
        ctx.call = (alpha, scale, thr, seed, offset, has_h, has_bias)
        ctx.set_materialize_grads(False)
        if has_h:
            return s, y
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        s, stats, g = ctx.saved_tensors
        alpha, scale, thr, seed, offset, has_h, has_bias = ctx.call
        ds, dy = grads if has_h else (None, grads[0])
        need = ctx.needs_input_grad
        if ds is None and dy is None:
            return (None,) * 10
        C = s.shape[-1]
        R = s.numel() // C
        if ds is not None and (not ds.is_contiguous() or ds.data_ptr() % 16):       # a broadcast, a transpose, a narrow at an odd offset
            ds = _dense16(ds)
        if dy is not None and (not dy.is_contiguous() or dy.data_ptr() % 16):
            dy = _dense16(dy)
        lib = _lib.load()
        dev = s.device
        want_dh, want_dres = has_h and need[0], need[1]
        shared = want_dh and want_dres and thr == 0 and alpha == 1.0      # dh equals dresidual: one tensor for both
        dres = torch.empty_like(s) if want_dres else None
        dh = torch.empty_like(s) if (want_dh and not shared) else None
        dbias = torch.empty_like(g) if (has_bias and need[2]) else None
        dgamma = torch.empty_like(g) if need[3] else None
        dbeta = torch.empty_like(g) if need[4] else None
        if dy is None:                                                 # y was not used: its parameters get zeros, not stale memory
            for t in (dgamma, dbeta):
                if t is not None:
                    t.zero_()
        kg, kb = (dgamma, dbeta) if dy is not None else (None, None)
        sums = kg is not None or kb is not None or dbias is not None
        nbytes = int(lib.dsp_resnorm_train_workspace_bytes(R, C)) if sums else 0
        ws = _workspace(dev, nbytes)
        if dh is not None or dres is not None or sums:
            entry, sd, off, tail = _masked(lib, "dsp_resnorm_train_bwd", seed, offset)
            _launch(dev, entry, _ptr(dy), _ptr(ds), s.data_ptr(), stats.data_ptr(), g.data_ptr(), alpha, scale, thr, sd,
                    off, _ptr(dh), _ptr(dres), _ptr(dbias), _ptr(kg), _ptr(kb), _ptr(ws), nbytes, _FLOAT_CODES[s.dtype],
                    _FLOAT_CODES[g.dtype], R, C, *tail)
        return (dres if shared else dh), dres, dbias, dgamma, dbeta, None, None, None, None, None


def residual_dropout_layer_norm_checked(h, residual, ln, bias=None, alpha=1.0, p=0.0, training=True, return_sum=True):
    """INTERNAL to the package's layers: residual_dropout_layer_norm_autograd WITHOUT its argument checks, valid only on arguments that
    residual_dropout_layer_norm_served / _sites_served accepted (~100 sites a training step, and the step is launch bound).  The kernels
    trust what they are handed: any other caller uses residual_dropout_layer_norm_autograd."""
    if h is None:
        return _ResidualNormTrainFn.apply(None, residual, None, ln.weight, ln.bias, ln.eps, 1.0, 0.0, 0, 0)
    if not h.is_contiguous() or h.data_ptr() % 16:      # the served rule looked at the residual; a block's output is dense, a view of it is copied
        h = _dense16(h)
    p_eff, seed, offset = _dropout_call(p, training, residual.device)
    out = _ResidualNormTrainFn.apply(h, residual, bias, ln.weight, ln.bias, ln.eps, float(alpha), p_eff, seed, offset)
    return out if return_sum else out[1]


def residual_dropout_layer_norm_autograd(h: Optional[Tensor], residual: Tensor, ln: "torch.nn.LayerNorm", *, bias: Optional[Tensor] = None,
                                         alpha: float = 1.0, p: float = 0.0, training: bool = True, return_sum: bool = True):
    """s = residual + alpha * dropout(h [+ bias], p);  y = ln(s)  — differentiable w.r.t. h, residual, bias, ln.weight and ln.bias
    (include/daspeech_decode.h: dsp_resnorm_train_fwd / _bwd).  Returns (s, y), or y alone with return_sum=False or h None (a plain
    LayerNorm under autograd: s would be the residual itself).  The LayerNorm sees s as stored (rounded to the dtype), as torch's does.
    Dropout is active with `training and p > 0`: the mask comes from a counter-based Philox stream keyed by the default CUDA generator of the
    tensors' device (seed, offset), whose offset such a call advances by 4 — the same generator state gives the same mask, successive calls
    differ, torch.cuda.set_rng_state restores the stream; calls with p = 0 do not touch the generator.  The masks are not torch's F.dropout
    masks.  fp32 / fp16 / bf16 (float64 is refused, never narrowed); ln.weight, ln.bias and bias in the dtype of the data or all in fp32.
    Bit-reproducible forward and backward."""
    why = _resnorm_problem(h, residual, ln, bias)
    if why is None and not 0.0 <= p < 1.0:
        why = f"p {p} is not served (0 <= p < 1)"
    if why is not None:
        raise RuntimeError(f"residual_dropout_layer_norm_autograd: {why}")
    w, b = ln.weight, ln.bias
    if not _on_grid(w, b, bias if h is not None else None) or not (w.is_contiguous() and b.is_contiguous() and (bias is None or bias.is_contiguous())):
        # parameters that are views (a flattened buffer, a broadcast): dense copies, gradients pass through
        ln, bias = types.SimpleNamespace(weight=_dense16(w), bias=_dense16(b), eps=ln.eps), _dense16(bias)
    return residual_dropout_layer_norm_checked(None if h is None else _dense16(h), _dense16(residual), ln, bias, alpha, p, training, return_sum)


# ------------------------------------------------------------------------------------------------ bias + activation + dropout (and GLU) under autograd (csrc/act_dropout_train.hip)
ACT_DROPOUT_HIP = True       # set_act_dropout_hip(False): the layers keep their torch lines between the GEMMs in training on every input
ACTDROP_CHUNK_ROWS = 32      # DSP_ACTDROP_CHUNK_ROWS: rows per reduction chunk of the backward (one workspace partial each)
ACTDROP_MAX_CIN = 8192       # DSP_ACTDROP_MAX_CIN
ACT_CODES = {"identity": 0, "relu": 1, "silu": 2, "gelu": 3, "glu": 4}      # DSP_ACT_*


def set_act_dropout_hip(on: bool) -> bool:
    """Switch the HIP bias + activation + dropout operator of the training branches (ConformerLayer, NATDecoderLayer, FFNAdapter,
    ConformerEncoder's input Linear) on or off; returns the previous setting.  Off: bias_act_dropout_served answers False and the torch
    lines run."""
    global ACT_DROPOUT_HIP
    old, ACT_DROPOUT_HIP = ACT_DROPOUT_HIP, bool(on)
    return old


def _actdrop_width_ok(C: int, act, itemsize: int) -> bool:
    V = 16 // itemsize
    return act in ACT_CODES and V <= C <= ACTDROP_MAX_CIN and C % (2 * V if act == "glu" else V) == 0


def _actdrop_bias_ok(bias, C: int, dt, dev) -> bool:
    return bias.dim() == 1 and bias.shape[0] == C and bias.device == dev and (bias.dtype == dt or bias.dtype == torch.float32)


def _actdrop_problem(h, bias, act) -> Optional[str]:
    """None when dsp_act_dropout_train_fwd / _bwd take these tensors as they are, else what is in the way (a layout that a dense copy settles
    begins with _LAYOUT)"""
    if not (isinstance(h, Tensor) and h.dim() >= 2):
        return "h has to be a [..., Cin] tensor of at least two dimensions"
    if act not in ACT_CODES:
        return f"unknown activation {act!r} (one of {', '.join(ACT_CODES)})"
    dt = h.dtype
    if dt not in _FLOAT_CODES:
        return f"h has to be fp32, fp16 or bf16, got {dt} (float64 is refused, never narrowed)"
    C, V = h.shape[-1], 16 // h.element_size()
    if not _actdrop_width_ok(C, act, h.element_size()) or h.numel() // C > (1 << 24):
        return (f"h {tuple(h.shape)} with {act} is not served (Cin a multiple of {V} elements — twice that with glu —, Cin <= {ACTDROP_MAX_CIN}, "
                f"at most 2^24 rows)")
    if bias is not None and not _actdrop_bias_ok(bias, C, dt, h.device):
        return f"bias has to be [{C}] on the device of h, in its dtype or in fp32, got {tuple(bias.shape)} {bias.dtype}"
    if not h.is_cuda:
        return _NOT_GPU
    ld = _row_pitch(h)
    if ld is None or ld < C or ld % V or h.data_ptr() % 16:
        return _LAYOUT + ": h needs unit column stride, one row pitch on the 16-byte grid and 16-byte alignment"
    return None


def bias_act_dropout_served(h: Tensor, bias: Optional[Tensor], act: str, masked: bool = True) -> bool:
    """True when bias_act_dropout_autograd serves a training branch on these arguments as they are: the switch is on, autocast off, h a GPU
    tensor [..., Cin] in fp32 / fp16 / bf16 with Cin a multiple of the elements in 16 bytes (twice that with glu) and at most 8192, unit
    column stride, rows one common pitch apart (a multiple of those elements) and a 16-byte aligned start, bias None or [Cin] contiguous and
    aligned in that dtype or fp32 on the same device, `act` one of ACT_CODES; while a graph is being captured only inside DropoutState.draws() on that device (the state on the device takes the place of the host's random offset) or with masked=False (a call that draws no mask: p == 0 or not training).  Everything else — CPU tensors, float64, another layout, an unknown activation — keeps the torch lines."""
    if not ACT_DROPOUT_HIP or torch.is_autocast_enabled():
        return False
    if _actdrop_problem(h, bias, act) is not None:
        return False
    return _as_handed_over(bias) and _capture_ok(h.device, masked)


def bias_act_dropout_sites_served(x: Tensor, sites, masked: bool = True) -> bool:
    """bias_act_dropout_served(F.linear(x, W), bias, act) for every (Cin, bias, act) of `sites` — the activation sites of ONE layer, each
    behind a bias-free F.linear of a tensor with the leading dimensions, dtype and device of the layer input x, whose result is a fresh dense
    tensor [..., Cin] — asked BEFORE those products exist, with the questions about the switch, autocast, x and the stream asked once: a
    layer asks this once per forward, and the step follows the host time of these sites.  `masked` as there."""
    if not ACT_DROPOUT_HIP or torch.is_autocast_enabled():
        return False
    dt = x.dtype
    if not (x.is_cuda and dt in _FLOAT_CODES and x.dim() >= 2 and x.shape[-1] >= 1 and x.numel() // x.shape[-1] <= (1 << 24)):
        return False
    dev, size = x.device, x.element_size()
    for C, bias, act in sites:
        if not _actdrop_width_ok(C, act, size):
            return False
        if bias is not None and not (_actdrop_bias_ok(bias, C, dt, dev) and _as_handed_over(bias)):
            return False
    return _capture_ok(dev, masked)


class _BiasActDropoutTrainFn(torch.autograd.Function):
    """dsp_act_dropout_train_fwd / _bwd.  Saved for the backward: h and bias — no mask, no y, no u: the backward recomputes all three."""

    @staticmethod
    def forward(ctx, h, bias, act, ld, p, seed, offset):
        Cin = h.shape[-1]
        Cout = Cin // 2 if act == 4 else Cin
        R = h.numel() // Cin
        thr, scale = _dropout_thr_scale(p)
        lib = _lib.load()
        dev = h.device
        y = torch.empty(h.shape[:-1] + (Cout,), dtype=h.dtype, device=dev)
        if R:
            entry, sd, off, tail = _masked(lib, "dsp_act_dropout_train_fwd", seed, offset)
            _launch(dev, entry, h.data_ptr(), ld, None if bias is None else bias.data_ptr(), act, scale, thr, sd, off,
                    y.data_ptr(), _FLOAT_CODES[h.dtype], _FLOAT_CODES[(h if bias is None else bias).dtype], R, Cin, *tail)
        ctx.save_for_backward(h, bias)
        ctx.call = (act, ld, scale, thr, seed, offset)
        ctx.set_materialize_grads(False)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        h, bias = ctx.saved_tensors
        act, ld, scale, thr, seed, offset = ctx.call
        need = ctx.needs_input_grad
        want_dh, want_db = need[0], bias is not None and need[1]
        if dy is None or not (want_dh or want_db):
            return (None,) * 7
        Cin = h.shape[-1]
        R = h.numel() // Cin
        if not dy.is_contiguous() or dy.data_ptr() % 16:                    # a broadcast, a transpose, a narrow at an odd offset
            dy = _dense16(dy)
        lib = _lib.load()
        dev = h.device
        dh = torch.empty(h.shape, dtype=h.dtype, device=dev) if want_dh else None
        dbias = torch.empty_like(bias) if want_db else None
        if R:
            nbytes = int(lib.dsp_act_dropout_train_workspace_bytes(R, Cin)) if want_db else 0
            ws = _workspace(dev, nbytes)
            entry, sd, off, tail = _masked(lib, "dsp_act_dropout_train_bwd", seed, offset)
            _launch(dev, entry, dy.data_ptr(), h.data_ptr(), ld, _ptr(bias), act, scale, thr, sd, off, _ptr(dh),
                    _ptr(dbias), _ptr(ws), nbytes, _FLOAT_CODES[h.dtype], _FLOAT_CODES[(h if bias is None else bias).dtype], R, Cin, *tail)
        elif dbias is not None:
            dbias.zero_()                                                  # no rows: the empty sum
        return dh, dbias, None, None, None, None, None


def bias_act_dropout_checked(h, bias, act, p=0.0, training=True):
    """INTERNAL to the package's layers: bias_act_dropout_autograd WITHOUT its argument checks, valid only on arguments that
    bias_act_dropout_served / _sites_served accepted.  The kernels trust what they are handed: any other caller uses
    bias_act_dropout_autograd."""
    ld = _row_pitch(h)
    if ld is None or ld % (16 // h.element_size()) or h.data_ptr() % 16:      # _sites_served asked before h existed; a GEMM's output is dense, a view of it is copied
        h, ld = h.clone(memory_format=torch.contiguous_format), h.shape[-1]
    p_eff, seed, offset = _dropout_call(p, training, h.device)
    return _BiasActDropoutTrainFn.apply(h, bias, ACT_CODES[act], ld, p_eff, seed, offset)


def bias_act_dropout_autograd(h: Tensor, bias: Optional[Tensor], act: str, p: float = 0.0, training: bool = True) -> Tensor:
    """y = dropout(act(h + bias), p)  — the element-wise pass between the two GEMMs of a feed-forward block, differentiable w.r.t. h and
    bias (include/daspeech_decode.h: dsp_act_dropout_train_fwd / _bwd).  act: "identity", "relu", "silu", "gelu" (erf form, as F.gelu) give
    y of the shape of h; "glu" gives y [..., Cin/2] = u[..., :Cin/2] * sigmoid(u[..., Cin/2:]) with u = h + bias, as F.glu(dim=-1).
    h [..., Cin] fp32 / fp16 / bf16 (float64 is refused, never narrowed) on the GPU, bias None or [Cin] in that dtype or fp32; a layout the
    kernels do not take (another column stride, rows of several pitches, a start off the 16-byte grid) is copied to a dense tensor, gradients
    pass through.  All arithmetic is fp32; y is rounded once.  Saved for the backward: h and bias only — u, the derivative and the mask are
    recomputed.  Dropout is active with `training and p > 0`; the mask is the one dropout_keep_mask(seed, offset, p, (R, Cout), device) gives
    for the R rows and Cout columns of y, for the (seed, offset) the call reserves from the default CUDA generator of h's device (its offset
    moves on by 4; calls with p = 0 or training=False do not touch the generator) — the same generator state gives the same mask, successive
    calls differ, torch.cuda.set_rng_state restores the stream.  The masks are not torch's F.dropout masks.  The bias gradient is summed in fp32
    in a fixed order without float atomics: forward and backward are bit-reproducible.  Raises RuntimeError on what is not served."""
    h, bias, act = _settled("bias_act_dropout_autograd", _actdrop_problem, (h, bias, act), 1, p)
    return bias_act_dropout_checked(h, _dense16(bias), act, p, training)


# ------------------------------------------------------------------------------------------------ decoder and TTS input embeddings under autograd (csrc/embed_entry_train.hip)
EMBED_ENTRY_HIP = True       # set_embed_entry_hip(False): DAGDecoder.extract_features and FastSpeech2NoEmb.forward keep their torch lines
EMBED_ENTRY_MAX_C = 2048     # DSP_EMBED_ENTRY_MAX_C
EMBED_ENTRY_SORT_MAX = 64    # DSP_EMBED_ENTRY_SORT_MAX: a key with more rows than this takes the ballot compaction, else the sorted fill
POS_ADD_CHUNK_ROWS = 32      # DSP_POS_ADD_CHUNK_ROWS: rows per fp32 partial of dalpha


def set_embed_entry_hip(on: bool) -> bool:
    """Switch the HIP embedding-entry operators of the training branches (DAGDecoder.extract_features, FastSpeech2NoEmb.forward) on or off;
    returns the previous setting.  Off: embed_entry_served and positional_add_dropout_served answer False and the torch lines run."""
    global EMBED_ENTRY_HIP
    old, EMBED_ENTRY_HIP = EMBED_ENTRY_HIP, bool(on)
    return old


def _entry_width_ok(C: int, itemsize: int) -> bool:
    V = 16 // itemsize
    return V <= C <= EMBED_ENTRY_MAX_C and C % V == 0


def _embed_entry_problem(tokens, E, P, pad) -> Optional[str]:
    """None when dsp_embed_entry_fwd / _bwd take these tensors (tokens through its row stride or a contiguous copy), else what is in the way
    (tables that a dense copy settles: the reason begins with _LAYOUT)"""
    if not (isinstance(tokens, Tensor) and tokens.dim() == 2 and tokens.dtype == torch.int64):
        return "tokens has to be a [B, L] int64 tensor"
    if not (isinstance(E, Tensor) and isinstance(P, Tensor) and E.dim() == 2 and P.dim() == 2 and E.shape[1] == P.shape[1]):
        return "the token table [V, C] and the position table [NP, C] have to be matrices of one width"
    if E.dtype not in _FLOAT_CODES or P.dtype != E.dtype:
        return f"both tables have to be in one of fp32 / fp16 / bf16, got {E.dtype} and {P.dtype} (float64 is refused, never narrowed)"
    (B, L), C, NP = tokens.shape, E.shape[1], P.shape[0]
    if not (_entry_width_ok(C, E.element_size()) and E.shape[0] >= 1 and 0 <= pad < NP and L + pad + 1 <= NP and B * L <= (1 << 24)):
        return (f"tokens {tuple(tokens.shape)} / tables {tuple(E.shape)}, {tuple(P.shape)} / pad {pad} are not served (C a multiple of "
                f"{16 // E.element_size()} elements, C <= {EMBED_ENTRY_MAX_C}, L + pad + 1 <= NP, B * L <= 2^24)")
    why = _gpu_problem(tokens, E, P)
    if why is not None:
        return why
    if not (tokens.device == E.device == P.device):
        return "tokens and both tables have to be on one device"
    if not _as_handed_over(E, P):
        return _LAYOUT + ": the tables have to be contiguous and start on a 16-byte boundary"
    return None


def embed_entry_served(tokens: Tensor, embed_tokens: "torch.nn.Embedding", embed_positions: "torch.nn.Embedding", masked: bool = True) -> bool:
    """True when embed_entry_autograd serves a training branch on these arguments as they are: the switch is on, autocast off, tokens a GPU
    int64 tensor [B, L], both nn.Embedding weights on that device in one of fp32 / fp16 / bf16, contiguous and on the 16-byte grid (a view
    into a flat parameter buffer at an odd offset is NOT served: the torch lines run), one padding_idx, C a multiple of the elements in 16
    bytes and at most 2048, L + pad + 1 <= NP, B * L <= 2^24; while a graph is being captured only inside DropoutState.draws() on that device (the state on the device takes the place of the host's random offset) or with masked=False (a call that draws no mask: p == 0 or not training).  Everything else keeps the torch lines."""
    if not EMBED_ENTRY_HIP or torch.is_autocast_enabled():
        return False
    pad = embed_tokens.padding_idx
    if pad is None or embed_positions.padding_idx != pad:
        return False
    if _embed_entry_problem(tokens, embed_tokens.weight, embed_positions.weight, pad) is not None:
        return False
    return _capture_ok(tokens.device, masked)


class _EmbedEntryFn(torch.autograd.Function):
    """dsp_embed_entry_fwd / _bwd.  Saved for the backward: tok32 and pos32 (int32 [B*L]) — no mask, no y."""

    @staticmethod
    def forward(ctx, tokens, E, P, pad, embed_scale, ld, p, seed, offset):
        B, L = tokens.shape
        V, C = E.shape
        NP = P.shape[0]
        thr, scale = _dropout_thr_scale(p)
        lib = _lib.load()
        dev = E.device
        y = torch.empty((B, L, C), dtype=E.dtype, device=dev)
        idx = torch.empty((2, B * L), dtype=torch.int32, device=dev)
        if B * L:
            entry, sd, off, tail = _masked(lib, "dsp_embed_entry_fwd", seed, offset)
            _launch(dev, entry, tokens.data_ptr(), ld, E.data_ptr(), P.data_ptr(), pad, embed_scale, scale, thr, sd, off,
                    y.data_ptr(), idx[0].data_ptr(), idx[1].data_ptr(), _FLOAT_CODES[E.dtype], B, L, V, NP, C, *tail)
        ctx.save_for_backward(idx)
        ctx.call = (pad, embed_scale, scale, thr, seed, offset, V, NP, C, E.dtype)
        ctx.set_materialize_grads(False)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        pad, embed_scale, scale, thr, seed, offset, V, NP, C, dt = ctx.call
        need = ctx.needs_input_grad
        if dy is None or not (need[1] or need[2]):
            return (None,) * 9
        if not dy.is_contiguous() or dy.data_ptr() % 16:                    # a broadcast, a transpose, a narrow at an odd offset
            dy = _dense16(dy)
        n = idx.shape[1]
        lib = _lib.load()
        dev = idx.device
        dE = torch.empty((V, C), dtype=dt, device=dev) if need[1] else None
        dP = torch.empty((NP, C), dtype=dt, device=dev) if need[2] else None
        nbytes = int(lib.dsp_embed_entry_bwd_workspace_bytes(n, V, NP, C, thr))
        ws = _workspace(dev, nbytes)
        entry, sd, off, tail = _masked(lib, "dsp_embed_entry_bwd", seed, offset)
        _launch(dev, entry, dy.data_ptr(), idx[0].data_ptr(), idx[1].data_ptr(), pad, embed_scale, scale, thr, sd, off,
                _ptr(dE), _ptr(dP), _ptr(ws), nbytes, _FLOAT_CODES[dt], n, V, NP, C, *tail)
        return None, dE, dP, None, None, None, None, None, None


def embed_entry_checked(tokens, E, P, pad, embed_scale, p=0.0, training=True):
    """INTERNAL to the package's layers: embed_entry_autograd WITHOUT its argument checks, valid only on arguments that embed_entry_served
    accepted.  The kernels trust what they are handed: any other caller uses embed_entry_autograd."""
    B, L = tokens.shape
    if (L > 1 and tokens.stride(1) != 1) or (B > 1 and tokens.stride(0) < L):      # a transpose, a broadcast: the rows of a column slice are read in place
        tokens = tokens.contiguous()
    ld = tokens.stride(0) if B > 1 else L
    p_eff, seed, offset = _dropout_call(p, training, E.device)
    return _EmbedEntryFn.apply(tokens, E, P, int(pad), float(embed_scale), ld, p_eff, seed, offset)


def embed_entry_autograd(tokens: Tensor, E: Tensor, P: Tensor, pad: int, scale: float, p: float = 0.0, training: bool = True) -> Tensor:
    """y [B, L, C] = dropout(scale * E[tokens] + P[positions(tokens)], p)  — the entry of DAGDecoder.extract_features (token embedding times
    embed_scale plus learned positions, fairseq nonautoregressive_transformer.py:340-349), differentiable w.r.t. both tables
    (include/daspeech_decode.h: dsp_embed_entry_fwd / _bwd).  positions = pad + keep * cumsum(keep) with keep = tokens != pad, so left
    padding, interior pads and all-pad rows are served; a token outside [0, V) gives a zero embedding row (torch raises there) and still
    counts as non-pad.  tokens [B, L] int64 on the GPU (a column slice of a wider tensor is read in place); E [V, C] and P [NP, C] in one of
    fp32 / fp16 / bf16 (float64 is refused, never narrowed) with L + pad + 1 <= NP; tables that are not contiguous or start off the 16-byte
    grid (views into a flat parameter buffer) are COPIED to dense tensors, gradients pass through.  fp32 arithmetic, one rounding.  The
    gradients add the rows of a table row in ascending order in fp32 without float atomics, row `pad` of both is zero (padding_idx):
    forward and backward are bit-reproducible.  Dropout is active with `training and p > 0`; the mask is the one
    dropout_keep_mask(seed, offset, p, (B * L, C), device) gives for the (seed, offset) the call reserves from the default CUDA generator of
    the tables' device (its offset moves on by 4; calls with p = 0 or training=False leave the generator alone).  The masks are not torch's
    F.dropout masks.  Raises RuntimeError on what is not served."""
    tokens, E, P, pad = _settled("embed_entry_autograd", _embed_entry_problem, (tokens, E, P, pad), 3, p)
    return embed_entry_checked(tokens, E, P, pad, scale, p, training)


def _posadd_problem(x, table, padding_mask, alpha) -> Optional[str]:
    """None when dsp_pos_add_fwd / _bwd take these tensors as they are, else what is in the way (a layout of x or the table that a dense copy
    settles begins with _LAYOUT)"""
    if not (isinstance(x, Tensor) and x.dim() == 3):
        return "x has to be a [B, N, C] tensor"
    dt = x.dtype
    if dt not in _FLOAT_CODES:
        return f"x has to be fp32, fp16 or bf16, got {dt} (float64 is refused, never narrowed)"
    B, N, C = x.shape
    if not (isinstance(padding_mask, Tensor) and padding_mask.shape == (B, N) and padding_mask.dtype in (torch.bool, torch.uint8)):
        return f"padding_mask has to be a [{B}, {N}] bool tensor"
    if not (isinstance(table, Tensor) and table.dim() == 2 and table.shape[1] == C and table.shape[0] >= 1 and table.dtype in (dt, torch.float32)
            and not table.requires_grad):
        return f"the table has to be [NT, {C}] in the dtype of x or in fp32, without gradient"
    if not (isinstance(alpha, Tensor) and alpha.numel() == 1 and alpha.dtype in (dt, torch.float32)):
        return "alpha has to be one element in the dtype of x or in fp32"
    if not _entry_width_ok(C, x.element_size()) or B * N > (1 << 24) or table.numel() >= (1 << 31):
        return (f"x {tuple(x.shape)} is not served (C a multiple of {16 // x.element_size()} elements, C <= {EMBED_ENTRY_MAX_C}, "
                "at most 2^24 rows)")
    why = _gpu_problem(x, padding_mask, table, alpha)
    if why is not None:
        return why
    if not (x.device == padding_mask.device == table.device == alpha.device):
        return "x, padding_mask, the table and alpha have to be on one device"
    ld = _row_pitch(x)
    if ld is None or ld < C or ld % (16 // x.element_size()) or x.data_ptr() % 16 or not _as_handed_over(table):
        return _LAYOUT + ": x needs unit column stride, one row pitch on the 16-byte grid and 16-byte alignment, the table a dense aligned start"
    return None


def positional_add_dropout_served(x: Tensor, padding_mask: Tensor, table: Tensor, alpha: Tensor, masked: bool = True) -> bool:
    """True when positional_add_dropout_autograd serves a training branch on these arguments as they are: the switch (set_embed_entry_hip)
    is on, autocast off, x a GPU tensor [B, N, C] in fp32 / fp16 / bf16 with C a multiple of the elements in 16 bytes and at most 2048, unit
    column stride, rows one common pitch apart and a 16-byte aligned start, padding_mask [B, N] bool, the table [NT, C] contiguous and aligned
    in that dtype or fp32 without gradient, alpha one element in that dtype or fp32, everything on one device; while a graph is being captured only inside DropoutState.draws() on that device (the state on the device takes the place of the host's random offset) or with masked=False (a call that draws no mask: p == 0 or not training).  Everything else keeps the torch lines."""
    if not EMBED_ENTRY_HIP or torch.is_autocast_enabled():
        return False
    if _posadd_problem(x, table, padding_mask, alpha) is not None:
        return False
    return _capture_ok(x.device, masked)


class _PosAddDropoutFn(torch.autograd.Function):
    """dsp_pos_add_fwd / _bwd.  Saved for the backward: the table and pos32 — no mask, no y."""

    @staticmethod
    def forward(ctx, x, mask, table, alpha, ld, p, seed, offset):
        B, N, C = x.shape
        NT = table.shape[0]
        thr, scale = _dropout_thr_scale(p)
        lib = _lib.load()
        dev = x.device
        y = torch.empty((B, N, C), dtype=x.dtype, device=dev)
        pos = torch.empty((B * N,), dtype=torch.int32, device=dev)
        codes = (_FLOAT_CODES[x.dtype], _FLOAT_CODES[table.dtype], _FLOAT_CODES[alpha.dtype])
        if B * N:
            entry, sd, off, tail = _masked(lib, "dsp_pos_add_fwd", seed, offset)
            _launch(dev, entry, x.data_ptr(), ld, mask.data_ptr(), table.data_ptr(), alpha.data_ptr(), 1, scale, thr, sd, off,
                    y.data_ptr(), pos.data_ptr(), codes[0], codes[1], codes[2], B, N, NT, C, *tail)
        ctx.save_for_backward(table, pos)
        ctx.call = (scale, thr, seed, offset, codes, alpha.shape)
        ctx.set_materialize_grads(False)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        table, pos = ctx.saved_tensors
        scale, thr, seed, offset, codes, ashape = ctx.call
        need = ctx.needs_input_grad
        want_dx, want_da = need[0], need[3]
        if dy is None or not (want_dx or want_da):
            return (None,) * 8
        if not (want_da or thr):
            return dy, None, None, None, None, None, None, None            # dx = dy: no launch
        if not dy.is_contiguous() or dy.data_ptr() % 16:                    # a broadcast, a transpose, a narrow at an odd offset
            dy = _dense16(dy)
        R, C = pos.shape[0], dy.shape[-1]
        lib = _lib.load()
        dev = dy.device
        dx = dy if not thr else (torch.empty(dy.shape, dtype=dy.dtype, device=dev) if want_dx else None)
        dalpha = torch.empty(ashape, dtype=[torch.float32, torch.float16, torch.bfloat16][codes[2]], device=dev) if want_da else None
        if R:
            nbytes = int(lib.dsp_pos_add_bwd_workspace_bytes(R)) if want_da else 0
            ws = _workspace(dev, nbytes)
            entry, sd, off, tail = _masked(lib, "dsp_pos_add_bwd", seed, offset)
            _launch(dev, entry, dy.data_ptr(), table.data_ptr(), pos.data_ptr(), scale, thr, sd, off,
                    _ptr(dx) if thr else None, _ptr(dalpha), _ptr(ws), nbytes, codes[0], codes[1], codes[2], R, table.shape[0], C, *tail)
        elif dalpha is not None:
            dalpha.zero_()                                                 # no rows: the empty sum
        return (dx if want_dx else None), None, None, dalpha, None, None, None, None


def positional_add_dropout_checked(x, padding_mask, table, alpha, p=0.0, training=True):
    """INTERNAL to the package's layers: positional_add_dropout_autograd WITHOUT its argument checks, valid only on arguments that
    positional_add_dropout_served accepted."""
    p_eff, seed, offset = _dropout_call(p, training, x.device)
    return _PosAddDropoutFn.apply(x, _mask_bytes(padding_mask), table, alpha, _row_pitch(x), p_eff, seed, offset)


def positional_add_dropout_autograd(x: Tensor, padding_mask: Tensor, table: Tensor, alpha: Tensor, p: float = 0.0,
                                    training: bool = True) -> Tensor:
    """y = dropout(x + alpha * table[min(positions_from_padding_mask(padding_mask), NT - 1)], p)  — the two positional sites of
    FastSpeech2NoEmb.forward (fastspeech2_noemb.py:150-151,166), differentiable w.r.t. x and the one-element alpha
    (include/daspeech_decode.h: dsp_pos_add_fwd / _bwd).  x [B, N, C] fp32 / fp16 / bf16 on the GPU (float64 is refused, never narrowed),
    padding_mask [B, N] bool (True: padding), table [NT, C] and alpha in that dtype or fp32, the table without gradient.  A row-pitched view
    of x is read in place; any other layout (x[:, 1:] of a batch, a transpose, a start off the 16-byte grid) and a table that is a view are
    copied to dense tensors, gradients pass through.  y has the dtype of x (torch's own lines promote to fp32 when the table is fp32 and x is
    not).  fp32 arithmetic, one rounding; dalpha is a fixed-order two-stage fp32 sum: forward and backward are bit-reproducible.  Dropout as
    in embed_entry_autograd, the mask that of dropout_keep_mask(seed, offset, p, (B * N, C), device); without dropout dx is dy itself.
    Raises RuntimeError on what is not served."""
    x, table, padding_mask, alpha = _settled("positional_add_dropout_autograd", _posadd_problem, (x, table, padding_mask, alpha), 2, p)
    return positional_add_dropout_checked(x, padding_mask, table, alpha, p, training)


# ------------------------------------------------------------------------------------------------ relative-position attention under autograd (csrc/relpos_attention_train.hip)
RELPOS_ATTENTION_HIP = True   # set_relpos_attention_hip(False): RelPosSelfAttention keeps its torch lines in training on every input
RELPOS_TRAIN_MAX_T = 2048     # DSP_RELPOS_TRAIN_MAX_T


def set_relpos_attention_hip(on: bool) -> bool:
    """Switch the HIP relative-position attention of RelPosSelfAttention's training branch on or off; returns the previous setting.
    Off: relpos_attention_autograd_served answers False and the torch lines run."""
    global RELPOS_ATTENTION_HIP
    old, RELPOS_ATTENTION_HIP = RELPOS_ATTENTION_HIP, bool(on)
    return old


def _relpos_train_problem(q, k, v, pos, bias_u, bias_v, pad_mask, heads) -> Optional[str]:
    """None when dsp_relpos_attention_train_fwd / _bwd take these tensors as they are, else what is in the way"""
    if not (isinstance(q, Tensor) and q.dim() == 3):
        return "q has to be a [B,T,C] tensor"
    B, T, C = q.shape
    dt, dev = q.dtype, q.device
    if dt not in _HALF_CODES:
        return f"q, k, v and pos have to be fp16 or bf16, got {dt} (fp32 keeps the torch lines; float64 is refused, never narrowed)"
    if heads < 1 or C != heads * 64:
        return f"head width {C // max(heads, 1)}: only 64 is served"
    if not 1 <= T <= RELPOS_TRAIN_MAX_T:
        return f"T = {T} outside 1 .. {RELPOS_TRAIN_MAX_T}"
    if not q.is_cuda:
        return _NOT_GPU
    ld = q.stride(1)
    for t in (q, k, v):
        if (t.shape != q.shape or t.dtype != dt or t.device != dev or t.stride(2) != 1 or t.stride(1) != ld or (B > 1 and t.stride(0) != T * ld)
                or t.data_ptr() % 16):
            if t.shape != q.shape or t.dtype != dt or t.device != dev:
                return "q, k, v need one shape, dtype and device"
            return _LAYOUT + ": q, k, v need unit column stride, one common row stride and 16-byte alignment"
    if ld < C or ld % 8:
        return _LAYOUT + f": row stride {ld} of q, k, v has to be a multiple of 8 elements"
    if pos.dtype != dt or pos.device != dev or pos.numel() != (2 * T - 1) * C or pos.shape[-1] != C and tuple(pos.shape[-2:]) != (heads, 64):
        return f"pos has to hold the [2T-1, C] projected positions in {dt}"
    pd = bias_u.dtype
    if (pd != dt and pd != torch.float32) or bias_v.dtype != pd or bias_u.device != dev or bias_v.device != dev \
            or tuple(bias_u.shape) != (heads, 64) or tuple(bias_v.shape) != (heads, 64):
        return "bias_u / bias_v have to be [heads, 64] in the data dtype or both in fp32"
    if pad_mask is not None and (tuple(pad_mask.shape) != (B, T) or pad_mask.device != dev):
        return "pad_mask has to be [B,T] on the device of q"
    return None


def relpos_attention_autograd_served(q: Tensor, k: Tensor, v: Tensor, pos: Tensor, bias_u: Tensor, bias_v: Tensor, pad_mask: Optional[Tensor],
                                     heads: int, masked: bool = True) -> bool:
    """True when relpos_attention_autograd serves RelPosSelfAttention's training branch on these arguments: the switch is on, autocast off,
    q / k / v [B,T,heads*64] GPU tensors in fp16 or bf16 with one common row stride (a multiple of 8 elements), pos the [2T-1, heads*64]
    projected positions in that dtype, bias_u / bias_v [heads,64] in that dtype or fp32, T <= 2048; while a graph is being captured only inside DropoutState.draws() on that device (the state on the device takes the place of the host's random offset) or with masked=False (a call that draws no mask: p == 0 or not training).  Everything else — fp32 data, CPU tensors, another head width — keeps the torch lines."""
    if not RELPOS_ATTENTION_HIP or torch.is_autocast_enabled():
        return False
    if _relpos_train_problem(q, k, v, pos, bias_u, bias_v, pad_mask, heads) is not None:
        return False
    return _as_handed_over(pos, bias_u, bias_v) and _capture_ok(q.device, masked)


class _RelPosAttentionTrainFn(torch.autograd.Function):
    """dsp_relpos_attention_train_fwd / _bwd.  Saved for the backward: q, k, v, pos, the biases, o, the fp32 lse and the mask bytes — no
    probabilities and no dropout mask: the backward recomputes both."""

    @staticmethod
    def forward(ctx, q, k, v, pos, bias_u, bias_v, mask, heads, p, seed, offset):
        B, T, C = q.shape
        thr, scale = _dropout_thr_scale(p)
        lib = _lib.load()
        dev = q.device
        o = torch.empty((B, T, C), dtype=q.dtype, device=dev)
        lse = torch.empty((B, heads, T), dtype=torch.float32, device=dev)
        entry, sd, off, tail = _masked(lib, "dsp_relpos_attention_train_fwd", seed, offset)
        _launch(dev, entry, q.data_ptr(), k.data_ptr(), v.data_ptr(), q.stride(1), pos.data_ptr(), bias_u.data_ptr(),
                bias_v.data_ptr(), _ptr(mask), scale, thr, sd, off, o.data_ptr(), lse.data_ptr(), _HALF_CODES[q.dtype],
                _FLOAT_CODES[bias_u.dtype], B, T, heads, *tail)
        ctx.save_for_backward(q, k, v, pos, bias_u, bias_v, o, lse, mask)
        ctx.call = (heads, scale, thr, seed, offset)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(lse)
        return o, lse

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, do, _dlse):
        q, k, v, pos, bias_u, bias_v, o, lse, mask = ctx.saved_tensors
        heads, scale, thr, seed, offset = ctx.call
        need = ctx.needs_input_grad
        if do is None or not any(need[:6]):
            return (None,) * 11
        B, T, C = q.shape
        if not do.is_contiguous() or do.data_ptr() % 16:
            do = _dense16(do)
        lib = _lib.load()
        dev = q.device
        dq = torch.empty((B, T, C), dtype=q.dtype, device=dev) if need[0] else None
        dk = torch.empty((B, T, C), dtype=q.dtype, device=dev) if need[1] else None
        dv = torch.empty((B, T, C), dtype=q.dtype, device=dev) if need[2] else None
        dpos = torch.empty(pos.shape, dtype=q.dtype, device=dev) if need[3] else None
        du = torch.empty_like(bias_u) if need[4] else None
        dbv = torch.empty_like(bias_v) if need[5] else None
        nbytes = int(lib.dsp_relpos_attention_train_workspace_bytes(B, T, heads)) if (need[3] or need[4] or need[5]) else 0
        ws = _workspace(dev, nbytes)
        entry, sd, off, tail = _masked(lib, "dsp_relpos_attention_train_bwd", seed, offset)
        _launch(dev, entry, do.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(), q.stride(1), pos.data_ptr(),
                bias_u.data_ptr(), bias_v.data_ptr(), _ptr(mask), o.data_ptr(), lse.data_ptr(), scale, thr, sd, off, _ptr(dq), _ptr(dk),
                _ptr(dv), _ptr(dpos), _ptr(du), _ptr(dbv), _ptr(ws), nbytes, _HALF_CODES[q.dtype], _FLOAT_CODES[bias_u.dtype], B, T, heads, *tail)
        return dq, dk, dv, dpos, du, dbv, None, None, None, None, None


def relpos_attention_checked(q, k, v, pos, bias_u, bias_v, pad_mask, heads, p=0.0, training=True, return_lse=False):
    """INTERNAL to RelPosSelfAttention: relpos_attention_autograd WITHOUT its argument checks, valid only on arguments that
    relpos_attention_autograd_served accepted.  The kernels trust what they are handed: any other caller uses relpos_attention_autograd."""
    p_eff, seed, offset = _dropout_call(p, training, q.device)
    if not pos.is_contiguous():
        pos = pos.contiguous()
    o, lse = _RelPosAttentionTrainFn.apply(q, k, v, pos, bias_u, bias_v, _mask_bytes(pad_mask), heads, p_eff, seed, offset)
    return (o, lse) if return_lse else o


def relpos_attention_autograd(q: Tensor, k: Tensor, v: Tensor, pos: Tensor, bias_u: Tensor, bias_v: Tensor, pad_mask: Optional[Tensor], heads: int,
                              p: float = 0.0, training: bool = True, return_lse: bool = False):
    """Conformer relative-position attention (fairseq espnet_multihead_attention.py RelPositionMultiHeadedAttention, between the projections
    and linear_out) under autograd, one HIP launch forward (include/daspeech_decode.h: dsp_relpos_attention_train_fwd / _bwd):
        o_i = sum_j dropout(softmax_j(((q_i + u).k_j + (q_i + v).pos[T-1-i+j]) / 8; pad_mask[b,j]: -inf), p)_ij v_j      per head of width 64
    differentiable w.r.t. q, k, v, pos, bias_u and bias_v.  q, k, v [B,T,heads*64] fp16 / bf16 with one common row stride, pos the projected
    positions ([2T-1, heads*64], a leading 1 allowed), bias_u / bias_v [heads,64] in that dtype or fp32, pad_mask [B,T] bool or None.  Returns
    o [B,T,heads*64] (with return_lse: and the fp32 log-sum-exp [B,heads,T]).  No [B,h,T,T] tensor is kept: the backward recomputes the
    probabilities.  Dropout is active with `training and p > 0`; the mask is the one dropout_keep_mask(seed, offset, p, (B, heads, T, Tp),
    device)[..., :T] gives, Tp = T rounded up to 4, for the (seed, offset) the call reserves from the device's default CUDA generator (its
    offset moves on by 4; calls with p = 0 do not touch the generator).  Bit-reproducible forward and backward.  Raises on what is not served."""
    q, k, v = _settled("relpos_attention_autograd", _relpos_train_problem, (q, k, v, pos, bias_u, bias_v, pad_mask, heads), 3, p)[:3]
    return relpos_attention_checked(q, k, v, _dense16(pos), _dense16(bias_u), _dense16(bias_v), pad_mask, heads, p, training, return_lse)


# ------------------------------------------------------------------------------------------------ multi-head attention under autograd (csrc/mha_train.hip)
MHA_ATTENTION_HIP = True      # set_mha_attention_hip(False): _MHA / _SelfAttention keep their torch lines in training on every input
MHA_TRAIN_MAX_LEN = 4096      # DSP_MHA_TRAIN_MAX_LEN


def set_mha_attention_hip(on: bool) -> bool:
    """Switch the HIP multi-head attention of the training branches of _MHA (NAT decoder) and _SelfAttention (FFT layers) on or off; returns
    the previous setting.  Off: mha_attention_autograd_served answers False and the torch lines run."""
    global MHA_ATTENTION_HIP
    old, MHA_ATTENTION_HIP = MHA_ATTENTION_HIP, bool(on)
    return old


def _mha_train_problem(q, k, v, pad_mask, heads) -> Optional[str]:
    """None when dsp_mha_train_fwd / _bwd take these tensors as they are, else what is in the way"""
    if not (isinstance(q, Tensor) and q.dim() == 3 and isinstance(k, Tensor) and k.dim() == 3 and isinstance(v, Tensor)):
        return "q has to be a [B,N,C] tensor, k and v [B,M,C] tensors"
    B, N, C = q.shape
    M = k.shape[1]
    dt, dev = q.dtype, q.device
    if dt not in _HALF_CODES:
        return f"q, k and v have to be fp16 or bf16, got {dt} (fp32 keeps the torch lines; float64 is refused, never narrowed)"
    if heads < 1 or C != heads * 64:
        return f"head width {C // max(heads, 1)}: only 64 is served"
    if not (1 <= N <= MHA_TRAIN_MAX_LEN and 1 <= M <= MHA_TRAIN_MAX_LEN):
        return f"N = {N}, M = {M} outside 1 .. {MHA_TRAIN_MAX_LEN}"
    if not q.is_cuda:
        return _NOT_GPU
    if k.shape != (B, M, C) or v.shape != k.shape or k.dtype != dt or v.dtype != dt or k.device != dev or v.device != dev:
        return "q [B,N,C], k and v [B,M,C] need one dtype and device"
    ldq, ldkv = q.stride(1), k.stride(1)
    if q.stride(2) != 1 or (B > 1 and q.stride(0) != N * ldq) or q.data_ptr() % 16:
        return _LAYOUT + ": q needs unit column stride, samples N rows apart and 16-byte alignment"
    for t in (k, v):
        if t.stride(2) != 1 or t.stride(1) != ldkv or (B > 1 and t.stride(0) != M * ldkv) or t.data_ptr() % 16:
            return _LAYOUT + ": k, v need unit column stride, one common row stride and 16-byte alignment"
    if ldq < C or ldq % 8 or ldkv < C or ldkv % 8:
        return _LAYOUT + f": row strides {ldq} (q) and {ldkv} (k, v) have to be multiples of 8 elements"
    if pad_mask is not None and (tuple(pad_mask.shape) != (B, M) or pad_mask.device != dev):
        return "pad_mask has to be [B,M] on the device of q"
    return None


def mha_attention_autograd_served(q: Tensor, k: Tensor, v: Tensor, pad_mask: Optional[Tensor], heads: int, masked: bool = True) -> bool:
    """True when mha_attention_autograd serves the training branch of _MHA / _SelfAttention on these arguments: the switch is on, autocast off,
    q [B,N,heads*64] and k, v [B,M,heads*64] GPU tensors in fp16 or bf16 (row strides multiples of 8 elements, one for k and v), N, M <= 4096,
    pad_mask [B,M] or None; while a graph is being captured only inside DropoutState.draws() on that device (the state on the device takes the place of the host's random offset) or with masked=False (a call that draws no mask: p == 0 or not training).  Everything else — fp32
    data, CPU tensors, another head width — keeps the torch lines."""
    if not MHA_ATTENTION_HIP or torch.is_autocast_enabled():
        return False
    if _mha_train_problem(q, k, v, pad_mask, heads) is not None:
        return False
    return _capture_ok(q.device, masked)


class _MhaTrainFn(torch.autograd.Function):
    """dsp_mha_train_fwd / _bwd.  Saved for the backward: q, k, v, the fp32 lse and the mask bytes — no probabilities and no dropout mask: the
    backward recomputes both (and D_i = dO_i . o_i from them in fp32, so o is not kept here either: out_proj keeps it as its input)."""

    @staticmethod
    def forward(ctx, q, k, v, mask, heads, p, seed, offset):
        B, N, C = q.shape
        M = k.shape[1]
        thr, scale = _dropout_thr_scale(p)
        lib = _lib.load()
        dev = q.device
        o = torch.empty((B, N, C), dtype=q.dtype, device=dev)
        lse = torch.empty((B, heads, N), dtype=torch.float32, device=dev)
        entry, sd, off, tail = _masked(lib, "dsp_mha_train_fwd", seed, offset)
        _launch(dev, entry, q.data_ptr(), q.stride(1), k.data_ptr(), v.data_ptr(), k.stride(1), _ptr(mask), scale, thr, sd, off,
                o.data_ptr(), lse.data_ptr(), _HALF_CODES[q.dtype], B, N, M, heads, *tail)
        ctx.save_for_backward(q, k, v, lse, mask)
        ctx.call = (heads, scale, thr, seed, offset)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(lse)
        return o, lse

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, do, _dlse):
        q, k, v, lse, mask = ctx.saved_tensors
        heads, scale, thr, seed, offset = ctx.call
        need = ctx.needs_input_grad
        if do is None or not any(need[:3]):
            return (None,) * 8
        B, N, C = q.shape
        M = k.shape[1]
        if not do.is_contiguous() or do.data_ptr() % 16:
            do = _dense16(do)
        lib = _lib.load()
        dev = q.device
        dq = torch.empty((B, N, C), dtype=q.dtype, device=dev) if need[0] else None
        dk = torch.empty((B, M, C), dtype=q.dtype, device=dev) if need[1] else None
        dv = torch.empty((B, M, C), dtype=q.dtype, device=dev) if need[2] else None
        nbytes = int(lib.dsp_mha_train_workspace_bytes(B, N, M, heads))     # D [B,H,N] fp32, rounded up to 16 bytes: the library's own answer
        ws = _workspace(dev, nbytes)
        entry, sd, off, tail = _masked(lib, "dsp_mha_train_bwd", seed, offset)
        _launch(dev, entry, do.data_ptr(), q.data_ptr(), q.stride(1), k.data_ptr(), v.data_ptr(), k.stride(1), _ptr(mask), lse.data_ptr(),
                scale, thr, sd, off, _ptr(dq), _ptr(dk), _ptr(dv), _ptr(ws), nbytes, _HALF_CODES[q.dtype], B, N, M, heads, *tail)
        return dq, dk, dv, None, None, None, None, None


def mha_attention_checked(q, k, v, pad_mask, heads, p=0.0, training=True, return_lse=False):
    """INTERNAL to _MHA / _SelfAttention: mha_attention_autograd WITHOUT its argument checks, valid only on arguments that
    mha_attention_autograd_served accepted.  The kernels trust what they are handed: any other caller uses mha_attention_autograd."""
    p_eff, seed, offset = _dropout_call(p, training, q.device)
    o, lse = _MhaTrainFn.apply(q, k, v, _mask_bytes(pad_mask), heads, p_eff, seed, offset)
    return (o, lse) if return_lse else o


def mha_attention_autograd(q: Tensor, k: Tensor, v: Tensor, pad_mask: Optional[Tensor], heads: int, p: float = 0.0, training: bool = True,
                           return_lse: bool = False):
    """Multi-head attention (fairseq multihead_attention.py between the projections and out_proj: the NAT decoder's self- and encoder
    attention, the FFT layers) under autograd, one HIP launch forward and two backward (include/daspeech_decode.h: dsp_mha_train_fwd / _bwd):
        o_i = sum_j dropout(softmax_j(q_i . k_j / 8; pad_mask[b,j]: -inf), p)_ij v_j      per head of width 64
    differentiable w.r.t. q, k and v.  q [B,N,heads*64], k and v [B,M,heads*64] fp16 / bf16 (N and M independent; views into a stacked q|k|v or
    k|v projection are taken as they are: row strides that are multiples of 8 elements, one for k and v), pad_mask [B,M] bool or None.  Returns
    o [B,N,heads*64] (with return_lse: and the fp32 log-sum-exp [B,heads,N]).  No [B,h,N,M] tensor is kept: the backward recomputes the
    probabilities.  Dropout is active with `training and p > 0`; the mask is the one dropout_keep_mask(seed, offset, p, (B, heads, N, Mp),
    device)[..., :M] gives, Mp = M rounded up to 4, for the (seed, offset) the call reserves from the device's default CUDA generator (its
    offset moves on by 4; calls with p = 0 do not touch the generator).  Bit-reproducible forward and backward.  Raises on what is not served."""
    q, k, v = _settled("mha_attention_autograd", _mha_train_problem, (q, k, v, pad_mask, heads), 3, p)[:3]
    return mha_attention_checked(q, k, v, pad_mask, heads, p, training, return_lse)


# ------------------------------------------------------------------------------------------------ channels-last Conv1d under autograd (csrc/conv1d_train.hip)
CONV1D_TRAIN_HIP = True         # set_conv1d_train_hip(False): _ConvFFN / VariancePredictor keep their torch lines in training on every input
CONV1D_TRAIN_ROW_TILE = 64       # DSP_CONV1D_TRAIN_ROW_TILE: rows of one sample per workgroup of the forward and of dx
CONV1D_TRAIN_WGRAD_ROWS = 1024   # DSP_CONV1D_TRAIN_WGRAD_ROWS: rows of the flattened B*T per split of the weight gradient (one workspace partial each)
CONV1D_TRAIN_MAX_K = 15          # DSP_CONV1D_TRAIN_MAX_K
CONV1D_TRAIN_MAX_C = 8192        # DSP_CONV1D_TRAIN_MAX_C
CONV1D_STRIDE2_TRAIN_HIP = True  # set_conv1d_stride2_train_hip(False): Conv1dSubsampler keeps its torch lines in training on every input
CONV1D_STRIDE2_CIN_GRID = 16     # the stride-2 operator's input channels: multiples of one k step of the matrix-core product (80 = 64 + 16)


def set_conv1d_train_hip(on: bool) -> bool:
    """Switch the HIP channels-last convolution of the training branches (FastSpeech2 _ConvFFN, VariancePredictor) on or off; returns the
    previous setting.  Off: conv1d_channels_last_served answers False and the torch lines run."""
    global CONV1D_TRAIN_HIP
    old, CONV1D_TRAIN_HIP = CONV1D_TRAIN_HIP, bool(on)
    return old


def _conv1d_module_problem(conv, stride: int = 1) -> Optional[str]:
    """None when `conv` is a convolution the operator of this stride computes, else what is in the way"""
    if not isinstance(conv, torch.nn.Conv1d):
        return "conv has to be an nn.Conv1d"
    K = conv.kernel_size[0]
    if conv.stride != (stride,):
        return f"stride {conv.stride[0]}: only {stride} is served"
    if conv.dilation != (1,):
        return f"dilation {conv.dilation[0]}: only 1 is served"
    if conv.groups != 1:
        return f"groups {conv.groups}: only 1 is served"
    if K % 2 == 0 or not 1 <= K <= CONV1D_TRAIN_MAX_K:
        return f"kernel size {K}: odd sizes from 1 to {CONV1D_TRAIN_MAX_K} are served"
    if conv.padding != ((K - 1) // 2,) or conv.padding_mode != "zeros":
        return f"padding {conv.padding} ({conv.padding_mode}): only zero padding of (K-1)/2 = {(K - 1) // 2} is served"
    return None


def _conv1d_channels_ok(C: int, grid: int = 64) -> bool:
    return grid <= C <= CONV1D_TRAIN_MAX_C and C % grid == 0


def _conv1d_train_problem(x, weight, bias, stride: int = 1) -> Optional[str]:
    """None when dsp_conv1d_train_fwd / _bwd (stride 2: dsp_conv1d_s2_train_fwd / _bwd) take these tensors as they are, else what is in the way
    (a layout of x that a dense copy settles begins with _LAYOUT)"""
    if not (isinstance(x, Tensor) and x.dim() == 3):
        return "x has to be a [B,T,Cin] tensor"
    if not (isinstance(weight, Tensor) and weight.dim() == 3):
        return "weight has to be a [Cout,Cin,K] tensor"
    B, T, Cin = x.shape
    dt, dev = x.dtype, x.device
    if dt not in _HALF_CODES or weight.dtype != dt:
        return f"x and weight have to be fp16 or bf16, got {dt} and {weight.dtype} (fp32 keeps the torch lines; float64 is refused, never narrowed)"
    Cout, Cw, K = weight.shape
    if Cw != Cin:
        return f"weight {tuple(weight.shape)} does not fit x with {Cin} channels (groups 1: [Cout, {Cin}, K])"
    if stride == 2 and not (_conv1d_channels_ok(Cin, CONV1D_STRIDE2_CIN_GRID) and _conv1d_channels_ok(Cout)):
        return (f"Cin = {Cin} / Cout = {Cout}: Cin a multiple of {CONV1D_STRIDE2_CIN_GRID} and Cout a multiple of 64, both up to "
                f"{CONV1D_TRAIN_MAX_C}, are served")
    if stride == 1 and not (_conv1d_channels_ok(Cin) and _conv1d_channels_ok(Cout)):
        return f"Cin = {Cin} / Cout = {Cout}: multiples of 64 up to {CONV1D_TRAIN_MAX_C} are served"
    if K % 2 == 0 or not 1 <= K <= CONV1D_TRAIN_MAX_K:
        return f"kernel size {K}: odd sizes from 1 to {CONV1D_TRAIN_MAX_K} are served"
    if T < 1 or B * T > (1 << 24):
        return f"x {tuple(x.shape)}: T >= 1 and at most 2^24 rows are served"
    if bias is not None and (tuple(bias.shape) != (Cout,) or (bias.dtype != dt and bias.dtype != torch.float32)):
        return f"bias has to be [{Cout}] in the dtype of x or in fp32, got {tuple(bias.shape)} {bias.dtype}"
    if not x.is_cuda:
        return _NOT_GPU
    if weight.device != dev or (bias is not None and bias.device != dev):
        return "x, weight and bias have to be on one device"
    ld = _row_pitch(x)
    if ld is None or ld < Cin or ld % 8 or x.data_ptr() % 16:
        return _LAYOUT + ": x needs unit column stride, one row stride on the 16-byte grid and 16-byte alignment"
    return None


def conv1d_channels_last_served(x: Tensor, conv: "torch.nn.Conv1d") -> bool:
    """True when conv1d_channels_last_autograd serves a training branch for `conv` on the channels-last x [B,T,Cin] as it is: the switch is on,
    autocast off, x a GPU tensor in fp16 or bf16 with unit column stride, one row stride on the 16-byte grid and a 16-byte aligned start,
    conv an nn.Conv1d(Cin, Cout, K) with stride 1, dilation 1, groups 1 and zero padding (K-1)//2, K odd and at most 15, both channel counts
    multiples of 64, weight and bias contiguous and aligned in the dtype of x (bias: or fp32).  Everything else — CPU tensors, fp32, float64,
    the postnet's 80 channels — keeps the torch lines; the subsampler's stride 2 is conv1d_stride2_channels_last_served's question."""
    if not CONV1D_TRAIN_HIP or torch.is_autocast_enabled():
        return False
    if _conv1d_module_problem(conv) is not None or _conv1d_train_problem(x, conv.weight, conv.bias) is not None:
        return False
    return _as_handed_over(conv.weight, conv.bias)


def conv1d_channels_last_sites_served(x: Tensor, convs) -> bool:
    """conv1d_channels_last_served for a CHAIN of convolutions of one layer, asked before the tensors between them exist: the first reads x,
    each later one a fresh dense tensor with the leading dimensions, dtype and device of x and the channels its predecessor leaves."""
    if not CONV1D_TRAIN_HIP or torch.is_autocast_enabled() or not conv1d_channels_last_served(x, convs[0]):
        return False
    C = convs[0].out_channels
    for conv in convs[1:]:
        w, b = conv.weight, conv.bias
        if (_conv1d_module_problem(conv) is not None or conv.in_channels != C or not _conv1d_channels_ok(conv.out_channels)
                or w.dtype != x.dtype or w.device != x.device or not _as_handed_over(w, b)):
            return False
        if b is not None and ((b.dtype != x.dtype and b.dtype != torch.float32) or b.device != x.device):
            return False
        C = conv.out_channels
    return True


_CONV1D_ENTRIES = {1: ("dsp_conv1d_train_workspace_bytes", "dsp_conv1d_train_fwd", "dsp_conv1d_train_bwd"),
                   2: ("dsp_conv1d_s2_train_workspace_bytes", "dsp_conv1d_s2_train_fwd", "dsp_conv1d_s2_train_bwd")}      # by stride


class _Conv1dTrainFn(torch.autograd.Function):
    """dsp_conv1d_train_fwd / _bwd, and with stride 2 dsp_conv1d_s2_train_fwd / _bwd (y and dy then have (T - 1) // 2 + 1 rows a sample).  Saved
    for the backward: x and weight, nothing else — the re-laid weight lives in a workspace that does not outlive the call, so no copy can go
    stale when the optimizer changes the weight."""

    @staticmethod
    def forward(ctx, x, weight, bias, ld, stride=1):
        B, T, Cin = x.shape
        Cout, _, K = weight.shape
        lib = _lib.load()
        ws_bytes, fwd, _ = _CONV1D_ENTRIES[stride]
        dev = x.device
        y = torch.empty((B, (T - 1) // stride + 1, Cout), dtype=x.dtype, device=dev)
        if B * T:
            nbytes = int(getattr(lib, ws_bytes)(0, B, T, Cin, Cout, K))
            ws = _workspace(dev, nbytes)
            _launch(dev, getattr(lib, fwd), x.data_ptr(), ld, weight.data_ptr(), _ptr(bias), y.data_ptr(), Cout, _ptr(ws), nbytes,
                    _HALF_CODES[x.dtype], _FLOAT_CODES[(x if bias is None else bias).dtype], B, T, Cin, Cout, K)
        ctx.save_for_backward(x, weight)
        ctx.call = (ld, None if bias is None else bias.dtype, stride)
        ctx.set_materialize_grads(False)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        ld, bias_dtype, stride = ctx.call
        need = ctx.needs_input_grad
        want_dx, want_dw, want_db = need[0], need[1], bias_dtype is not None and need[2]
        if dy is None or not (want_dx or want_dw or want_db):
            return None, None, None, None, None
        B, T, Cin = x.shape
        Cout, _, K = weight.shape
        ld_dy = _row_pitch(dy)
        if ld_dy is None or ld_dy < Cout or ld_dy % 8 or dy.data_ptr() % 16:       # a transpose, a broadcast, a narrow at an odd offset
            dy, ld_dy = dy.clone(memory_format=torch.contiguous_format), Cout
        lib = _lib.load()
        ws_bytes, _, bwd = _CONV1D_ENTRIES[stride]
        dev = x.device
        dx = torch.empty((B, T, Cin), dtype=x.dtype, device=dev) if want_dx else None
        dw = torch.empty((Cout, Cin, K), dtype=x.dtype, device=dev) if want_dw else None
        db = torch.empty((Cout,), dtype=bias_dtype, device=dev) if want_db else None
        if B * T:
            nbytes = int(getattr(lib, ws_bytes)(1, B, T, Cin, Cout, K))
            ws = _workspace(dev, nbytes)
            _launch(dev, getattr(lib, bwd), dy.data_ptr(), ld_dy, x.data_ptr(), ld, weight.data_ptr(), _ptr(dx), _ptr(dw), _ptr(db),
                    _ptr(ws), nbytes, _HALF_CODES[x.dtype], _FLOAT_CODES[bias_dtype or x.dtype], B, T, Cin, Cout, K)
        else:
            for t in (dw, db):                                              # no rows: the empty sums
                if t is not None:
                    t.zero_()
        return dx, dw, db, None, None


def conv1d_channels_last_checked(x, weight, bias=None):
    """INTERNAL to the package's layers: conv1d_channels_last_autograd WITHOUT its argument checks, valid only on arguments that
    conv1d_channels_last_served / _sites_served accepted.  The kernels trust what they are handed: any other caller uses
    conv1d_channels_last_autograd."""
    ld = _row_pitch(x)
    if ld is None or ld % 8 or x.data_ptr() % 16:       # _sites_served asked before x existed; an operator's output is dense, a view of it is copied
        x, ld = x.clone(memory_format=torch.contiguous_format), x.shape[-1]
    return _Conv1dTrainFn.apply(x, weight, bias, ld)


def conv1d_channels_last_autograd(x: Tensor, weight: Tensor, bias: Optional[Tensor] = None) -> Tensor:
    """y[b,t,co] = [bias[co] +] sum_k sum_ci x[b, t+k-P, ci] weight[co,ci,k], P = (K-1)/2, rows outside [0, T) of a sample as zeros — what
    F.conv1d(x.transpose(1, 2), weight, bias, padding=P).transpose(1, 2) computes, on the channels-last tensor without the transposes, and
    differentiable w.r.t. x, weight and bias (include/daspeech_decode.h: dsp_conv1d_train_fwd / _bwd).  x [B,T,Cin] fp16 / bf16 on the GPU
    (fp32 keeps the torch lines; float64 is refused, never narrowed), weight [Cout,Cin,K] in nn.Conv1d's layout and the dtype of x, bias
    [Cout] in that dtype or fp32, Cin and Cout multiples of 64, K odd and at most 15.  A view of x with unit column stride and one row stride
    on the 16-byte grid (the column slice of a wider tensor) is read as it is; any other layout, a weight or a bias that is a view, and an
    incoming gradient that is not dense are copied, gradients pass through.  Every product runs on the matrix cores with fp32 accumulators
    and each result is rounded once.  Saved for the backward: x and weight only.  The weight gradient's sum over the B*T rows and the bias
    gradient's run in a fixed order without float atomics: forward and backward are bit-reproducible.  Raises RuntimeError on what is not served."""
    x, weight, bias = _settled("conv1d_channels_last_autograd", _conv1d_train_problem, (x, weight, bias), 1)
    return conv1d_channels_last_checked(x, _dense16(weight), _dense16(bias))


# ------------------------------------------------------------------------------------------------ stride-2 channels-last Conv1d under autograd (csrc/conv1d_stride2_train.hip)
def set_conv1d_stride2_train_hip(on: bool) -> bool:
    """Switch the HIP stride-2 channels-last convolution of Conv1dSubsampler's training branch on or off; returns the previous setting.  Off:
    conv1d_stride2_channels_last_served answers False and the torch lines run."""
    global CONV1D_STRIDE2_TRAIN_HIP
    old, CONV1D_STRIDE2_TRAIN_HIP = CONV1D_STRIDE2_TRAIN_HIP, bool(on)
    return old


def _conv1d_s2_module_problem(conv) -> Optional[str]:
    """_conv1d_module_problem for the stride-2 operator: the same rule with stride 2"""
    return _conv1d_module_problem(conv, 2)


def _conv1d_s2_train_problem(x, weight, bias) -> Optional[str]:
    """_conv1d_train_problem for dsp_conv1d_s2_train_fwd / _bwd: the same rule with Cin on the grid of 16"""
    return _conv1d_train_problem(x, weight, bias, 2)


def conv1d_stride2_channels_last_served(x: Tensor, conv: "torch.nn.Conv1d") -> bool:
    """True when conv1d_stride2_channels_last_autograd serves a training branch for `conv` on the channels-last x [B,T,Cin] as it is: the
    switch is on, autocast off, x a GPU tensor in fp16 or bf16 with unit column stride, one row stride on the 16-byte grid and a 16-byte
    aligned start, conv an nn.Conv1d(Cin, Cout, K) with stride 2, dilation 1, groups 1 and zero padding (K-1)//2, K odd and at most 15, Cin
    a multiple of 16 and Cout of 64, weight and bias contiguous and aligned in the dtype of x (bias: or fp32).  Everything else — CPU
    tensors, fp32, float64, another stride — keeps the torch lines."""
    if not CONV1D_STRIDE2_TRAIN_HIP or torch.is_autocast_enabled():
        return False
    if _conv1d_s2_module_problem(conv) is not None or _conv1d_s2_train_problem(x, conv.weight, conv.bias) is not None:
        return False
    return _as_handed_over(conv.weight, conv.bias)


def conv1d_stride2_channels_last_sites_served(x: Tensor, convs) -> bool:
    """conv1d_stride2_channels_last_served for the CHAIN of convolutions of Conv1dSubsampler, asked once per forward before the tensors
    between them exist: the first reads x, each later one a fresh dense tensor with the dtype and device of x and HALF the channels its
    predecessor leaves (the GLU between them)."""
    if not CONV1D_STRIDE2_TRAIN_HIP or torch.is_autocast_enabled() or not conv1d_stride2_channels_last_served(x, convs[0]):
        return False
    C = convs[0].out_channels // 2
    for conv in convs[1:]:
        w, b = conv.weight, conv.bias
        if (_conv1d_s2_module_problem(conv) is not None or conv.in_channels != C or not _conv1d_channels_ok(C, CONV1D_STRIDE2_CIN_GRID)
                or not _conv1d_channels_ok(conv.out_channels) or w.dtype != x.dtype or w.device != x.device or not _as_handed_over(w, b)):
            return False
        if b is not None and ((b.dtype != x.dtype and b.dtype != torch.float32) or b.device != x.device):
            return False
        C = conv.out_channels // 2
    return True


def conv1d_stride2_channels_last_checked(x, weight, bias=None):
    """INTERNAL to the package's layers: conv1d_stride2_channels_last_autograd WITHOUT its argument checks, valid only on arguments that
    conv1d_stride2_channels_last_served / _sites_served accepted."""
    ld = _row_pitch(x)
    if ld is None or ld % 8 or x.data_ptr() % 16:       # _sites_served asked before x existed; an operator's output is dense, a view of it is copied
        x, ld = x.clone(memory_format=torch.contiguous_format), x.shape[-1]
    return _Conv1dTrainFn.apply(x, weight, bias, ld, 2)


def conv1d_stride2_channels_last_autograd(x: Tensor, weight: Tensor, bias: Optional[Tensor] = None) -> Tensor:
    """y[b,t,co] = [bias[co] +] sum_k sum_ci x[b, 2t+k-P, ci] weight[co,ci,k] for t in [0, (T-1)//2 + 1), P = (K-1)/2, rows outside [0, T) of
    a sample as zeros — what F.conv1d(x.transpose(1, 2), weight, bias, stride=2, padding=P).transpose(1, 2) computes, on the channels-last
    tensor without the transposes, and differentiable w.r.t. x, weight and bias (include/daspeech_decode.h: dsp_conv1d_s2_train_fwd / _bwd).
    x [B,T,Cin] fp16 / bf16 on the GPU (fp32 keeps the torch lines; float64 is refused, never narrowed), weight [Cout,Cin,K] in nn.Conv1d's
    layout and the dtype of x, bias [Cout] in that dtype or fp32, Cin a multiple of 16, Cout a multiple of 64, K odd and at most 15.  Views,
    rounding, the saved tensors (x and weight only) and bit-reproducibility are conv1d_channels_last_autograd's; a gradient of x that
    autograd does not ask for (the filterbank input of the first layer) is not computed.  Raises RuntimeError on what is not served."""
    x, weight, bias = _settled("conv1d_stride2_channels_last_autograd", _conv1d_s2_train_problem, (x, weight, bias), 1)
    return conv1d_stride2_channels_last_checked(x, _dense16(weight), _dense16(bias))


# ------------------------------------------------------------------------------------------------ the four TTS losses under autograd (csrc/tts_loss_train.hip)
TTS_LOSS_HIP = True          # set_tts_loss_hip(False): S2SDAGFastSpeech2Loss keeps its torch lines (masks, selections, F.l1_loss / F.mse_loss) on every input
TTSLOSS_CHUNK_ROWS = 32      # DSP_TTSLOSS_CHUNK_ROWS: mel rows per reduction chunk of the forward (one workspace partial each)
TTSLOSS_CHUNK_ELEMS = 1024   # DSP_TTSLOSS_CHUNK_ELEMS: [B,N] elements per reduction chunk
TTSLOSS_MAX_ELEMS = 1 << 30  # DSP_TTSLOSS_MAX_ELEMS
_INT_LENS = (torch.int64, torch.int32)


def set_tts_loss_hip(on: bool) -> bool:
    """Switch the HIP TTS-loss operator of S2SDAGFastSpeech2Loss on or off; returns the previous setting.  Off: tts_losses_served answers
    False and the criterion's torch lines run."""
    global TTS_LOSS_HIP
    old, TTS_LOSS_HIP = TTS_LOSS_HIP, bool(on)
    return old


def _tts_loss_problem(feat_out, feat_post, target_audio, audio_lens, log_dur_out, pitch_out, energy_out, durations, pitches, energies,
                      src_lens) -> Optional[str]:
    """None when dsp_tts_loss_fwd / _bwd take these tensors as they are, else what is in the way (a layout that a dense copy settles begins
    with _LAYOUT)"""
    mel = (feat_out, target_audio) if feat_post is None else (feat_out, target_audio, feat_post)
    var = (log_dur_out, pitch_out, energy_out, pitches, energies)
    for t in mel + var + (audio_lens, durations, src_lens):
        if not isinstance(t, Tensor):
            return "every argument except feat_post has to be a tensor"
    dt, dev = feat_out.dtype, feat_out.device
    if dt not in _FLOAT_CODES:
        return f"the data has to be fp32, fp16 or bf16, got {dt} (float64 is refused, never narrowed)"
    for t in mel + var:
        if t.dtype != dt:
            return f"one floating dtype for all data tensors: {dt} and {t.dtype}"
    if durations.dtype not in _INT_LENS or audio_lens.dtype not in _INT_LENS or src_lens.dtype not in _INT_LENS:
        return "durations and both length vectors have to be int64 or int32"
    if feat_out.dim() != 3 or target_audio.dim() != 3 or log_dur_out.dim() != 2:
        return "feat_out [B,F,C], target_audio [B,Fa,C] and the variance tensors [B,N] expected"
    B, F, C = feat_out.shape
    Fa, N = target_audio.shape[1], log_dur_out.shape[1]
    if target_audio.shape[0] != B or target_audio.shape[2] != C or (feat_post is not None and feat_post.shape != feat_out.shape):
        return (f"feat_out {tuple(feat_out.shape)}, target_audio {tuple(target_audio.shape)} and feat_post have to share B and C, "
                f"feat_post the whole shape of feat_out")
    for t in var + (durations,):
        if t.shape != (B, N):
            return f"the six variance tensors have to share the shape [{B},{N}], got {tuple(t.shape)}"
    if audio_lens.shape != (B,) or src_lens.shape != (B,):
        return f"both length vectors have to be [{B}]"
    if min(B, F, Fa, C, N) < 1 or B * max(F, Fa) * C > TTSLOSS_MAX_ELEMS or B * N > TTSLOSS_MAX_ELEMS:
        return f"sizes outside the operator's limits (every dimension >= 1, B*F*C and B*N at most 2^30): B={B} F={F} Fa={Fa} C={C} N={N}"
    if target_audio.requires_grad or pitches.requires_grad or energies.requires_grad:
        return "the targets must not require grad (they get no gradient)"
    for t in mel + var + (audio_lens, durations, src_lens):
        if not t.is_cuda:
            return _NOT_GPU
        if t.device != dev:
            return "all tensors have to be on one device"
    for t in mel:
        if (t.stride(2) != 1 and C > 1) or t.data_ptr() % t.element_size():
            return _LAYOUT + ": feat_out, feat_post and target_audio need unit column stride and a start on the element grid"
    for t in var + (durations, audio_lens, src_lens):
        if not t.is_contiguous() or t.data_ptr() % t.element_size():
            return _LAYOUT + ": the [B,N] tensors and the length vectors have to be contiguous"
    return None


def tts_losses_served(feat_out, feat_post, target_audio, audio_lens, log_dur_out, pitch_out, energy_out, durations, pitches, energies,
                      src_lens) -> bool:
    """True when tts_losses_autograd serves these arguments as they are: the switch is on, autocast off, GPU tensors of one floating dtype
    (fp32 / fp16 / bf16), feat_out [B,F,C], feat_post None or shaped like it, target_audio [B,Fa,C] — each with unit column stride, any batch
    and row stride —, the six [B,N] tensors of one shape and contiguous (durations int64 / int32), both length vectors [B] int64 / int32 and
    contiguous, no target that requires grad, every dimension >= 1 and B*F*C, B*N at most 2^30.  There is no randomness: a capturing stream
    is no reason to decline.  Everything else — CPU tensors, float64, mixed dtypes, another layout — keeps the torch lines."""
    if not TTS_LOSS_HIP or torch.is_autocast_enabled():
        return False
    return _tts_loss_problem(feat_out, feat_post, target_audio, audio_lens, log_dur_out, pitch_out, energy_out, durations, pitches, energies,
                             src_lens) is None


def _tts_loss_forward(feat_out, feat_post, target_audio, audio_lens, log_dur_out, pitch_out, energy_out, durations, pitches, energies,
                      src_lens):
    """dsp_tts_loss_fwd: (losses fp32 [4], inv_counts fp32 [2], call) — `call` is what both entry points take between the pointers"""
    B, F, C = feat_out.shape
    F_, N = min(F, target_audio.shape[1]), log_dur_out.shape[1]
    dev = feat_out.device
    lib = _lib.load()
    losses = torch.empty((4,), dtype=torch.float32, device=dev)
    inv = torch.empty((2,), dtype=torch.float32, device=dev)
    nbytes = int(lib.dsp_tts_loss_workspace_bytes(B, F_, N))
    ws = _workspace(dev, nbytes)
    post = (None, 0, 0) if feat_post is None else (feat_post.data_ptr(), feat_post.stride(0), feat_post.stride(1))
    ins = (feat_out.data_ptr(), feat_out.stride(0), feat_out.stride(1)) + post + \
        (target_audio.data_ptr(), target_audio.stride(0), target_audio.stride(1), audio_lens.data_ptr(), log_dur_out.data_ptr(),
         pitch_out.data_ptr(), energy_out.data_ptr(), durations.data_ptr(), pitches.data_ptr(), energies.data_ptr(), src_lens.data_ptr(),
         int(audio_lens.dtype == torch.int64), int(durations.dtype == torch.int64))
    _launch(dev, lib.dsp_tts_loss_fwd, *ins, losses.data_ptr(), inv.data_ptr(), _ptr(ws), nbytes, _FLOAT_CODES[feat_out.dtype], B, F_, C, N)
    return losses, inv, ins


class _TtsLossFn(torch.autograd.Function):
    """dsp_tts_loss_fwd / _bwd.  Saved for the backward: the inputs and the two reciprocals — no mask, no difference."""

    @staticmethod
    def forward(ctx, feat_out, feat_post, target_audio, audio_lens, log_dur_out, pitch_out, energy_out, durations, pitches, energies, src_lens):
        losses, inv, ins = _tts_loss_forward(feat_out, feat_post, target_audio, audio_lens, log_dur_out, pitch_out, energy_out, durations,
                                             pitches, energies, src_lens)
        ctx.save_for_backward(feat_out, feat_post, target_audio, audio_lens, log_dur_out, pitch_out, energy_out, durations, pitches, energies,
                              src_lens, inv)
        ctx.ins = ins
        return losses

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        saved = ctx.saved_tensors
        feat_out, feat_post, log_dur_out, inv = saved[0], saved[1], saved[4], saved[11]
        need = ctx.needs_input_grad
        dev = feat_out.device
        if g.dtype != torch.float32 or not g.is_contiguous():              # a broadcast gradient (losses.sum()), another dtype
            g = g.to(torch.float32).contiguous()
        B, F, C = feat_out.shape
        F_, N = min(F, saved[2].shape[1]), log_dur_out.shape[1]
        d_fo = torch.empty((B, F, C), dtype=feat_out.dtype, device=dev) if need[0] else None
        d_fp = torch.empty((B, F, C), dtype=feat_out.dtype, device=dev) if feat_post is not None and need[1] else None
        d_var = [torch.empty((B, N), dtype=feat_out.dtype, device=dev) if need[i] else None for i in (4, 5, 6)]
        _launch(dev, _lib.load().dsp_tts_loss_bwd, g.data_ptr(), inv.data_ptr(), *ctx.ins, _ptr(d_fo), _ptr(d_fp), _ptr(d_var[0]), _ptr(d_var[1]),
                _ptr(d_var[2]), _FLOAT_CODES[feat_out.dtype], B, F, F_, C, N)
        return d_fo, d_fp, None, None, d_var[0], d_var[1], d_var[2], None, None, None, None


def tts_losses_checked(feat_out, feat_post, target_audio, audio_lens, log_dur_out, pitch_out, energy_out, durations, pitches, energies,
                       src_lens):
    """INTERNAL to the package's criterion: tts_losses_autograd WITHOUT its argument checks, valid only on arguments that tts_losses_served
    accepted.  The kernels trust what they are handed: any other caller uses tts_losses_autograd."""
    if audio_lens.dtype != src_lens.dtype:                                  # one width for both length vectors
        audio_lens, src_lens = audio_lens.to(torch.int64), src_lens.to(torch.int64)
    args = (feat_out, feat_post, target_audio, audio_lens, log_dur_out, pitch_out, energy_out, durations, pitches, energies, src_lens)
    if torch.is_grad_enabled() and (feat_out.requires_grad or log_dur_out.requires_grad or pitch_out.requires_grad or energy_out.requires_grad
                                    or (feat_post is not None and feat_post.requires_grad)):
        return _TtsLossFn.apply(*args)
    return _tts_loss_forward(*args)[0]                                      # nothing is saved


def tts_losses_autograd(feat_out: Tensor, feat_post: Optional[Tensor], target_audio: Tensor, audio_lens: Tensor, log_dur_out: Tensor,
                        pitch_out: Tensor, energy_out: Tensor, durations: Tensor, pitches: Tensor, energies: Tensor, src_lens: Tensor) -> Tensor:
    """The four TTS losses of the released objective as one fp32 tensor [4] = (l1, dur, pitch, energy), differentiable w.r.t. feat_out,
    feat_post, log_dur_out, pitch_out and energy_out (include/daspeech_decode.h: dsp_tts_loss_fwd / _bwd).  With F_ = min(F, Fa),
    m_b = min(audio_lens[b], F_), s_b = min(src_lens[b], N), n_mel = C * sum_b m_b, n_src = sum_b s_b:
        l1     = sum_{b, f<m_b, c} |feat_out - target_audio| / n_mel   (+ the same sum over feat_post when it is given, also / n_mel)
        dur    = sum_{b, n<s_b} (log_dur_out - log(durations + 1))^2 / n_src;   pitch, energy: the same on (pitch_out, pitches), (energy_out, energies)
    — what the criterion's masks, boolean selections, F.l1_loss and F.mse_loss compute, with the masks taken from the lengths on the device:
    no mask tensor, no selection, NO HOST READ of device data in forward or backward.  feat_out [B,F,C], feat_post None or like it,
    target_audio [B,Fa,C] in fp32 / fp16 / bf16 (one dtype; float64 is refused, never narrowed) on the GPU, the six [B,N] tensors of one shape
    (durations int64 / int32), lengths [B] int64 / int32; the targets must not require grad.  The mel tensors are read through their batch and
    row strides (the [:, :F_] slices never exist; F != Fa needs no copy); a layout the kernels do not take — another column stride, a
    non-contiguous [B,N] tensor — is copied to a dense tensor, gradients pass through.  All arithmetic is fp32 on the exactly widened inputs
    and the result is fp32 for every data dtype; an empty selection gives NaN as torch's mean of nothing; non-finite inputs propagate.  The
    sums run in a fixed order without float atomics: forward and backward are bit-reproducible.  Gradients are dense, every element written
    (exact zeros beyond the lengths), rounded once to the data dtype; sign(0) = sign(NaN) = 0 in the L1 gradient as in torch.  Saved for the
    backward: the inputs and two reciprocals; under torch.no_grad(), or when no input requires grad, nothing.  Raises RuntimeError on what is
    not served."""
    args = _settled("tts_losses_autograd", _tts_loss_problem, (feat_out, feat_post, target_audio, audio_lens, log_dur_out, pitch_out,
                                                               energy_out, durations, pitches, energies, src_lens), 11)
    return tts_losses_checked(*args)


# ------------------------------------------------------------------------------------------------ the argmax strategy's path features under autograd (csrc/path_features_train.hip)
PATH_FEATURES_HIP = True         # set_path_features_hip(False): S2SDAGFastSpeech2Loss keeps its torch lines (argsort, host read of the width, gather) on every input
PATH_FEATURES_TILE_W = 8         # DSP_PATH_FEATURES_TILE_W: rows of the result per forward workgroup
PATH_FEATURES_TILE_L = 16        # DSP_PATH_FEATURES_TILE_L: vertices per backward workgroup
PATH_FEATURES_MAX_L = 65536      # DSP_PATH_FEATURES_MAX_L
PATH_FEATURES_MAX_ROWS = 1 << 24


def set_path_features_hip(on: bool) -> bool:
    """Switch the HIP path-features operator of S2SDAGFastSpeech2Loss's argmax strategy on or off; returns the previous setting.  Off:
    path_features_served answers False and the criterion's torch lines run."""
    global PATH_FEATURES_HIP
    old, PATH_FEATURES_HIP = PATH_FEATURES_HIP, bool(on)
    return old


def _path_features_problem(features, path, width) -> Optional[str]:
    """None when dsp_path_features_fwd / _bwd take these tensors as they are, else what is in the way (a layout of the features that a dense
    copy settles begins with _LAYOUT; path is read through its strides in any layout)"""
    if not (isinstance(features, Tensor) and isinstance(path, Tensor)):
        return "features and path have to be tensors"
    if features.dtype not in _FLOAT_CODES:
        return f"features has to be fp32, fp16 or bf16, got {features.dtype} (float64 is refused, never narrowed)"
    if features.dim() != 3:
        return "features [B, L, C] expected"
    B, L, C = features.shape
    if path.dtype not in _INT_LENS or path.shape != (B, L):
        return f"path has to be a [{B}, {L}] int64 or int32 tensor"
    if not isinstance(width, int) or isinstance(width, bool) or width < 0:
        return f"the width has to be a host integer >= 0, got {width!r}"
    per = 16 // features.element_size()
    if not (B >= 1 and 1 <= L <= PATH_FEATURES_MAX_L and C >= per and C % per == 0 and B * L <= PATH_FEATURES_MAX_ROWS
            and B * width <= PATH_FEATURES_MAX_ROWS and C * features.element_size() <= PATH_FEATURES_MAX_ROWS):
        return (f"features {tuple(features.shape)} / width {width} are not served (B, L >= 1, L <= {PATH_FEATURES_MAX_L}, C a multiple of {per} "
                f"elements, B * L and B * width at most 2^24)")
    why = _gpu_problem(features, path)
    if why is not None:
        return why
    if features.device != path.device:
        return "features and path have to be on one device"
    ld = _row_pitch(features)
    if ld is None or ld < C or ld % per or features.data_ptr() % 16:
        return _LAYOUT + ": features needs unit column stride, one row pitch on the 16-byte grid and a 16-byte aligned start"
    return None


def path_features_served(features: Tensor, path: Tensor, width: int) -> bool:
    """True when path_features_autograd serves these arguments as they are: the switch is on, autocast off, features a GPU tensor [B, L, C]
    in fp32 / fp16 / bf16 with C a multiple of the elements in 16 bytes, unit column stride, rows one common pitch apart and a 16-byte aligned
    start and pitch, path [B, L] int64 / int32 on that device (any strides), B, L >= 1, L <= 65 536, width a host integer >= 0, B * L and
    B * width at most 2^24.  There is no randomness and no host read: a capturing stream is no reason to decline.  Everything else — CPU
    tensors, float64, another layout — keeps the torch lines."""
    if not PATH_FEATURES_HIP or torch.is_autocast_enabled():
        return False
    return _path_features_problem(features, path, width) is None


def _path_strides(path: Tensor) -> Tuple[int, int]:
    """batch and column stride of path [B, L] for the C ABI: the stride of a dimension of length 1 is never used, and torch leaves it arbitrary"""
    return (path.stride(0) if path.shape[0] > 1 else 0), (path.stride(1) if path.shape[1] > 1 else 0)


def _path_features_forward(features, path, width, skip_first, ld):
    """dsp_path_features_fwd: (out [B,W,C], pad [B,W] bool, n [B] int64), width >= 1"""
    B, L, C = features.shape
    dev = features.device
    out = torch.empty((B, width, C), dtype=features.dtype, device=dev)
    pad = torch.empty((B, width), dtype=torch.bool, device=dev)
    n = torch.empty((B,), dtype=torch.int64, device=dev)
    _launch(dev, _lib.load().dsp_path_features_fwd, features.data_ptr(), ld, path.data_ptr(), *_path_strides(path), int(path.dtype == torch.int64),
            int(skip_first), out.data_ptr(), pad.data_ptr(), n.data_ptr(), _FLOAT_CODES[features.dtype], B, L, width, C)
    return out, pad, n


class _PathFeaturesFn(torch.autograd.Function):
    """dsp_path_features_fwd / _bwd.  Saved for the backward: path and the sizes — no index, no rank, no feature."""

    @staticmethod
    def forward(ctx, features, path, width, skip_first, ld):
        out, pad, n = _path_features_forward(features, path, width, skip_first, ld)
        ctx.save_for_backward(path)
        ctx.call = (tuple(features.shape), features.dtype, width, skip_first)
        ctx.mark_non_differentiable(pad, n)
        ctx.set_materialize_grads(False)
        return out, pad, n

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy, _dpad, _dn):
        (path,) = ctx.saved_tensors
        (B, L, C), dt, width, skip_first = ctx.call
        if dy is None or not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        if dy.dtype != dt:
            dy = dy.to(dt)
        per = 16 // dy.element_size()
        sb, sr = (dy.stride(0) if B > 1 else 0), (dy.stride(1) if width > 1 else 0)      # a broadcast (stride 0) is read in place
        if (dy.stride(2) != 1 and C > 1) or dy.data_ptr() % 16 or sb % per or sr % per:      # a transpose, a narrow at an odd offset or pitch
            dy = dy.clone(memory_format=torch.contiguous_format)
            sb, sr = width * C, C
        dev = dy.device
        dfeatures = torch.empty((B, L, C), dtype=dt, device=dev)
        _launch(dev, _lib.load().dsp_path_features_bwd, dy.data_ptr(), sb, sr, path.data_ptr(), *_path_strides(path),
                int(path.dtype == torch.int64), int(skip_first), dfeatures.data_ptr(), _FLOAT_CODES[dt], B, L, width, C)
        return dfeatures, None, None, None, None


def path_features_checked(features, path, width, skip_first=True):
    """INTERNAL to the package's criterion: path_features_autograd WITHOUT its argument checks, valid only on arguments that
    path_features_served accepted.  The kernels trust what they are handed: any other caller uses path_features_autograd."""
    if width == 0:                                                          # empty tensors, no launch: a view keeps the gradient's route
        B = features.shape[0]
        return (features[:, :0], torch.empty((B, 0), dtype=torch.bool, device=features.device),
                torch.zeros((B,), dtype=torch.int64, device=features.device))
    ld = _row_pitch(features)
    if torch.is_grad_enabled() and features.requires_grad:
        return _PathFeaturesFn.apply(features, path, width, bool(skip_first), ld)
    return _path_features_forward(features, path, width, bool(skip_first), ld)      # nothing is saved


def path_features_autograd(features: Tensor, path: Tensor, width: int, skip_first: bool = True) -> Tuple[Tensor, Tensor, Tensor]:
    """(out [B, W, C], pad [B, W] bool, n [B] int64): the feature rows of the vertices on the path, compacted in vertex order — the argmax
    strategy's features_on_path and features_padding_mask (DASpeech/criterions/s2s_dag_fastspeech2_loss.py:241-246), differentiable w.r.t.
    features (include/daspeech_decode.h: dsp_path_features_fwd / _bwd).  With on[b,j] = path[b,j] >= 0 and (j > 0 or not skip_first) and
    n[b] = min(sum_j on[b,j], W):  out[b,r] = features[b, j_r] for r < n[b], j_r the r-th vertex with `on` set; exact zeros (written, not
    multiplied: NaN in a row that is not selected never shows) and pad = True for r >= n[b].  W is a HOST integer — in the criterion
    tgt_tokens.shape[1] - 1 —, so forward and backward hold NO HOST READ of device data; vertices on the path beyond W are dropped, and
    only the sign of a path value is read.  features [B, L, C] fp32 / fp16 / bf16 on the GPU (float64 is refused, never narrowed), C a
    multiple of the elements in 16 bytes; a row-pitched view is read in place, any other layout (a transpose, a start off the 16-byte grid)
    is copied to a dense tensor, gradients pass through; path int64 / int32 in any layout.  Rows are copied bit for bit, one launch each way,
    no sort, no atomics: the gradient of a feature row is the one row of dy it was copied to, or exact zero, every element written.  Saved
    for the backward: path and the sizes; under torch.no_grad(), or when features does not require grad, nothing.  W == 0 returns empty
    tensors without a launch.  pad and n are not differentiable.  Raises RuntimeError on what is not served."""
    features, path, width = _settled("path_features_autograd", _path_features_problem, (features, path, width), 1)
    return path_features_checked(features, path, width, skip_first)


class SplitConv1d:
    """fp32-accurate Conv1d(Cin, Cout, K, padding=(K-1)//2) on the fp16 matrix cores (include/daspeech_decode.h: dsp_conv1d_split).
    Packs the weight once (hi / lo fp16 in MFMA fragment order, per 512-channel input slice); call with channels-last x [B,T,Cin]."""

    def __init__(self, weight: Tensor, bias: Optional[Tensor]):
        _gpu("SplitConv1d", weight)
        lib = _lib.load()
        Cout, Cin, K = weight.shape
        self.Cout, self.Cin, self.K = Cout, Cin, K
        self.bias = None if bias is None else _dense16(bias.detach().float())      # the split-K reduction reads it with 16-byte loads
        step = Cin if Cin <= 512 else 512          # (256-channel slices with 128-row tiles: 125 vs 95 us for 2048 -> 256; r04 for the 512-wide decoder GEMMs: 3 - 10 % faster, not taken)
        assert Cin % step == 0 and step in (128, 256, 512) and Cout % 4 == 0 and K % 2 == 1, (Cin, Cout, K)
        self.step, self.nslices = step, Cin // step
        with torch.cuda.device(weight.device):
            st = _lib.current_stream_handle()
            n = lib.dsp_conv1d_split_packed_elems(K, Cout, step)
            self.hi = torch.empty((self.nslices * n,), dtype=torch.float16, device=weight.device); self.lo = torch.empty_like(self.hi)
            for sl in range(self.nslices):
                wt = weight.detach().float()[:, sl * step:(sl + 1) * step, :].permute(2, 0, 1).contiguous()        # [K][Cout][step]
                _lib.check(lib.dsp_conv1d_split_pack(_lib.ptr(wt), ctypes.c_void_p(self.hi.data_ptr() + 2 * sl * n),
                                                     ctypes.c_void_p(self.lo.data_ptr() + 2 * sl * n), K, Cout, step, st), "dsp_conv1d_split_pack")

    ACT = {None: 0, "relu": 1, "silu": 2, "gelu": 3}
    KSPLIT = True              # short sequences: split deep reductions over workgroups (set False to time / compare the single-launch form)

    def _tap_groups(self, B: int, T: int) -> int:
        """tap groups for the split-K form, 0 = one launch: only when the layer would occupy under half of the 256 CUs with a reduction
        of >= 4 slice-taps per workgroup (the FastSpeech2 encoder's second FFT convolution: 1024 -> 256, K = 9 over ~60 positions)"""
        if not SplitConv1d.KSPLIT or self.Cout % 4:
            return 0
        wgs = B * ((T + 63) // 64) * ((self.Cout + 255) // 256)
        if wgs >= 128 or self.nslices * self.K < 4:
            return 0
        tg = 1
        while tg < self.K and wgs * self.nslices * tg < 256 and tg < 3:
            tg += 1
        return tg if self.nslices * tg >= 2 else 0


    def __call__(self, x: Tensor, relu: bool = False, act: Optional[str] = None, residual: Optional[Tensor] = None, alpha: float = 1.0,
                 lens: Optional[Tensor] = None, slack: int = 0) -> Tensor:
        """act(conv(x) + bias), or residual + alpha * that when a residual [B,T,Cout] is given.  lens [B] int32 (ragged batch): time tiles
        starting at or after lens[b] + slack are padding and are not computed: they come back as zeros (dsp_conv1d_split_ragged) or, in
        the split-K form of short sequences, as residual + alpha * act(bias) — finite either way."""
        _gpu("SplitConv1d", x)
        code = 1 if relu else self.ACT[act]
        assert x.dtype == torch.float32 and x.dim() == 3 and x.shape[2] == self.Cin
        B, T, _ = x.shape
        # served as it is: unit column stride, rows pitched by a multiple of 4 floats with the batches dense over them, the base on the 16-byte
        # grid (a contiguous tensor, a column slice of a fused projection); every other view is copied (there is no torch path from here)
        if x.stride(2) != 1 or x.stride(1) % 4 or x.stride(1) < self.Cin or (B > 1 and x.stride(0) != T * x.stride(1)) or x.data_ptr() % 16:
            x = x.clone(memory_format=torch.contiguous_format)
        r = None                                             # the residual as the kernels take it: dense fp32 on the grid
        if residual is not None:
            r = _dense16(residual if residual.dtype == torch.float32 else residual.float())
            assert tuple(r.shape) == (B, T, self.Cout)
        lib = _lib.load()
        with torch.cuda.device(x.device):
            st = _lib.current_stream_handle()
            out = torch.empty((B, T, self.Cout), dtype=torch.float32, device=x.device)
            tg = self._tap_groups(B, T)
            if lens is not None:
                assert lens.dtype == torch.int32 and lens.is_cuda and lens.is_contiguous() and lens.numel() == B
            if tg:
                # short sequence: split the reduction over slices x tap groups so that the launch fills the chip (dsp_conv1d_split_ksplit)
                nws = lib.dsp_conv1d_split_ksplit_workspace_bytes(B, T, self.Cout, self.nslices, tg)
                ws = torch.empty((nws // 4,), dtype=torch.float32, device=x.device)
                _lib.check(lib.dsp_conv1d_split_ksplit(_lib.ptr(x), x.stride(1), _lib.ptr(self.hi), _lib.ptr(self.lo), _lib.ptr(self.bias), _lib.ptr(r), self.Cout,
                                                       float(alpha), _lib.ptr(out), self.Cout, B, T, self.step, self.nslices, self.Cout, self.K, code, tg,
                                                       _lib.ptr(ws), nws, _lib.ptr(lens), int(slack), st), "dsp_conv1d_split_ksplit")
            elif lens is not None:
                assert lens.dtype == torch.int32 and lens.is_cuda and lens.is_contiguous() and lens.numel() == B
                _lib.check(lib.dsp_conv1d_split_ragged(_lib.ptr(x), x.stride(1), _lib.ptr(self.hi), _lib.ptr(self.lo), _lib.ptr(self.bias), _lib.ptr(r),
                                                       self.Cout, float(alpha), _lib.ptr(out), self.Cout, B, T, self.step, self.nslices, self.Cout,
                                                       self.K, code, _lib.ptr(lens), int(slack), st), "dsp_conv1d_split_ragged")
            elif residual is not None or alpha != 1.0:
                _lib.check(lib.dsp_conv1d_split_residual(_lib.ptr(x), x.stride(1), _lib.ptr(self.hi), _lib.ptr(self.lo), _lib.ptr(self.bias), _lib.ptr(r),
                                                         self.Cout, float(alpha), _lib.ptr(out), self.Cout, B, T, self.step, self.nslices, self.Cout,
                                                         self.K, code, st), "dsp_conv1d_split_residual")
            else:
                _lib.check(lib.dsp_conv1d_split(_lib.ptr(x), x.stride(1), _lib.ptr(self.hi), _lib.ptr(self.lo), _lib.ptr(self.bias), _lib.ptr(out),
                                                self.Cout, B, T, self.step, self.nslices, self.Cout, self.K, code, 0, st), "dsp_conv1d_split")
        return out


SPLIT_GEMM = True          # set_split_gemm(False): every Linear / FFT convolution goes back to torch (hipBLASLt / MIOpen fp32)


def set_split_gemm(on: bool) -> bool:
    """Switch the fp32-accurate matrix-core GEMM / conv path of eval-mode inference on or off; returns the previous setting."""
    global SPLIT_GEMM
    old, SPLIT_GEMM = SPLIT_GEMM, bool(on)
    return old


def valid_lengths(pad_mask: Optional[Tensor]) -> Optional[Tensor]:
    """[B] int32: one past the last position that is not padding (a ragged batch's row bounds for the `lens` arguments below)"""
    if pad_mask is None or not pad_mask.is_cuda:
        return None
    T = pad_mask.shape[1]
    return ((~pad_mask) * torch.arange(1, T + 1, device=pad_mask.device, dtype=torch.int32)).amax(1).to(torch.int32).contiguous()


def split_linear(x: Tensor, lin, act: Optional[str] = None, residual: Optional[Tensor] = None, alpha: float = 1.0,
                 lens: Optional[Tensor] = None, slack: int = 0) -> Optional[Tensor]:
    """act(x @ W^T + b) at fp32 accuracy on the fp16 matrix cores (a SplitConv1d with one tap), or None when the shape / mode is not
    served (caller falls back to F.linear): eval-mode inference in fp32 on the GPU, in_features 128 / 256 / 512 or a multiple of 512,
    out_features % 4 == 0, at least 128 rows.  The packed weight is cached on the module."""
    if (not SPLIT_GEMM or torch.is_grad_enabled() or not x.is_cuda or x.dtype != torch.float32 or torch.is_autocast_enabled() or lin.weight.dtype != torch.float32
            or x.dim() != 3 or not x.is_contiguous() or x.shape[0] * x.shape[1] < 128 or x.data_ptr() % 16):
        return None                                                # (x off the 16-byte grid: F.linear takes it; the residual is copied by SplitConv1d)
    wt = lin.weight                                                # nn.Linear [out,in] or a kernel-1 nn.Conv1d [out,in,1]
    if wt.dim() == 3 and wt.shape[2] != 1:
        return None
    cout, cin = wt.shape[0], wt.shape[1]
    if not ((cin in (128, 256, 512) or (cin > 512 and cin % 512 == 0)) and cout % 4 == 0 and cout >= 128):
        return None                                                # narrow outputs (gates, mel projection) waste the 256-row weight tile
    bias = getattr(lin, "bias", None)                              # nn.Embedding used as a tied output projection has none
    key = (lin.weight.data_ptr(), lin.weight._version, None if bias is None else bias._version)
    cache = getattr(lin, "_dsp_split", None)
    if cache is None or cache[0] != key:
        cache = (key, SplitConv1d(wt if wt.dim() == 3 else wt.unsqueeze(-1), bias))
        lin._dsp_split = cache
    return cache[1](x, act=act, residual=residual, alpha=alpha, lens=lens, slack=slack)


def linear(x: Tensor, lin, act: Optional[str] = None, residual: Optional[Tensor] = None, alpha: float = 1.0, lens: Optional[Tensor] = None,
           slack: int = 0) -> Tensor:
    """[residual + alpha *] act(lin(x)): through split_linear where it applies (eval-mode fp32 inference on the GPU), torch otherwise.
    `lin` is an nn.Linear or a kernel-1 nn.Conv1d (applied on the channels-last x).  lens [B] int32: rows from lens[b] + slack on are padding
    that may come back as zeros (whole tiles are skipped on the split path; the torch path computes them)."""
    if not lin.training:
        y = split_linear(x, lin, act, residual, alpha, lens, slack)
        if y is not None:
            return y
    y = torch.nn.functional.linear(x, lin.weight if lin.weight.dim() == 2 else lin.weight.squeeze(-1), getattr(lin, "bias", None))
    if act is not None:
        y = {"relu": torch.relu, "silu": torch.nn.functional.silu, "gelu": torch.nn.functional.gelu}[act](y)
    if alpha != 1.0:
        y = alpha * y
    return y if residual is None else residual + y


class _CatLinear:
    """the weights / biases of several nn.Linear over the same input stacked into one [sum(out), in] projection"""

    def __init__(self, lins):
        self.weight = torch.cat([l.weight.detach() for l in lins], 0)
        self.bias = torch.cat([(l.bias.detach() if l.bias is not None else torch.zeros(l.weight.shape[0], dtype=l.weight.dtype, device=l.weight.device))
                               for l in lins], 0)
        self.training = False


def linear_fused(x: Tensor, lins, lens: Optional[Tensor] = None, slack: int = 0) -> tuple:
    """(lin(x) for lin in lins) for nn.Linear modules sharing the input x: in eval-mode fp32 inference on the GPU ONE split GEMM over the
    stacked weights (cached on the first module) whose output columns are returned as row-strided views — every output column sees the
    same reduction as in its own GEMM, so the values are bit-identical to separate calls; separate `linear` calls otherwise."""
    first = lins[0]
    if (SPLIT_GEMM and not first.training and not torch.is_grad_enabled() and x.is_cuda and x.dtype == torch.float32 and not torch.is_autocast_enabled()
            and x.dim() == 3 and x.is_contiguous() and x.data_ptr() % 16 == 0 and x.shape[0] * x.shape[1] >= 128
            and all(l.weight.dim() == 2 and l.weight.dtype == torch.float32 for l in lins)):
        key = tuple((l.weight.data_ptr(), l.weight._version, None if l.bias is None else l.bias._version) for l in lins)
        cache = getattr(first, "_dsp_cat", None)
        if cache is None or cache[0] != key:
            cache = (key, _CatLinear(lins))
            first._dsp_cat = cache
        y = split_linear(x, cache[1], lens=lens, slack=slack)
        if y is not None:
            outs, o = [], 0
            for l in lins:
                outs.append(y[..., o:o + l.weight.shape[0]]); o += l.weight.shape[0]
            return tuple(outs)
    return tuple(linear(x, l, lens=lens, slack=slack) for l in lins)


def _packed(lin) -> Optional["SplitConv1d"]:
    """the SplitConv1d (packed hi / lo weights) split_linear caches on an nn.Linear, built on first use"""
    wt = lin.weight
    bias = getattr(lin, "bias", None)
    key = (wt.data_ptr(), wt._version, None if bias is None else bias._version)
    cache = getattr(lin, "_dsp_split", None)
    if cache is None or cache[0] != key:
        cache = (key, SplitConv1d(wt if wt.dim() == 3 else wt.unsqueeze(-1), bias))
        lin._dsp_split = cache
    return cache[1]


def ffn_fused(x: Tensor, ln: Optional["torch.nn.LayerNorm"], lin1, lin2, act: str, residual: Optional[Tensor] = None, alpha: float = 1.0,
              post_ln: Optional["torch.nn.LayerNorm"] = None, need_out: bool = True):
    """[residual +] alpha * lin2(act(lin1(ln(x)))) in one matrix-core launch at fp32 accuracy (dsp_ffn_split: the hidden activations stay in
    LDS, LayerNorm runs while the tile is staged), or None when the shape / mode is not served: eval-mode fp32 inference on the GPU,
    256 channels in and out, hidden width a multiple of 512.  With post_ln the reduction also applies that LayerNorm to its result (the
    next block of a pre-norm layer starts with one) and the call returns (out, post_ln(out)); need_out=False: (None, post_ln(out))."""
    if (not SPLIT_GEMM or torch.is_grad_enabled() or lin1.training or not x.is_cuda or x.dtype != torch.float32 or torch.is_autocast_enabled() or x.dim() != 3
            or not x.is_contiguous() or lin1.weight.dtype != torch.float32 or lin1.weight.dim() != 2 or lin2.weight.dim() != 2
            or lin2.weight.dtype != torch.float32 or x.data_ptr() % 16):
        return None                                   # (null biases are handled by the kernels: `if (p.b1)`, `if (p.b2)`)
    B, T, C = x.shape
    H = lin1.weight.shape[0]
    if C != 256 or tuple(lin1.weight.shape) != (H, C) or tuple(lin2.weight.shape) != (C, H) or H % 512 or B * T < 128:
        return None
    for n_ in (ln, post_ln):
        if n_ is not None and (tuple(n_.normalized_shape) != (C,) or n_.weight is None or n_.bias is None or n_.weight.dtype != torch.float32
                               or n_.weight.data_ptr() % 16 or n_.bias.data_ptr() % 16 or not n_.weight.is_contiguous() or not n_.bias.is_contiguous()):
            return None
    lib = _lib.load()
    p1, p2 = _packed(lin1), _packed(lin2)
    r = None
    if residual is not None:
        r = _dense16(residual if residual.dtype == torch.float32 else residual.float())
        assert tuple(r.shape) == (B, T, C)
    with torch.cuda.device(x.device):
        nws = lib.dsp_ffn_split_workspace_bytes(B, T, C, H)
        ws = torch.empty((nws // 4,), dtype=torch.float32, device=x.device)
        out = torch.empty_like(x) if (need_out or post_ln is None) else None
        out_ln = None if post_ln is None else torch.empty_like(x)
        _lib.check(lib.dsp_ffn_split(_lib.ptr(x), x.stride(1), _lib.ptr(None if ln is None else ln.weight), _lib.ptr(None if ln is None else ln.bias),
                                     float(ln.eps) if ln is not None else 0.0, _lib.ptr(p1.hi), _lib.ptr(p1.lo), _lib.ptr(p1.bias), _lib.ptr(p2.hi),
                                     _lib.ptr(p2.lo), _lib.ptr(p2.bias), _lib.ptr(r), C, float(alpha), _lib.ptr(out), C, _lib.ptr(ws), nws, B, T, C, H,
                                     SplitConv1d.ACT[act], _lib.ptr(None if post_ln is None else post_ln.weight),
                                     _lib.ptr(None if post_ln is None else post_ln.bias), float(post_ln.eps) if post_ln is not None else 0.0,
                                     _lib.ptr(out_ln), _lib.current_stream_handle()), "dsp_ffn_split")
    return out if post_ln is None else (out, out_ln)


def linear_ln(x: Tensor, ln: "torch.nn.LayerNorm", lins, act: Optional[str] = None, lens: Optional[Tensor] = None, slack: int = 0) -> tuple:
    """(lin(ln(x)) for lin in lins): for 256-channel inputs in eval-mode fp32 inference on the GPU ONE split GEMM over the stacked weights with
    the LayerNorm applied while the row tile is staged (dsp_linear_ln_split) — no LayerNorm launch, no normalised copy of x; otherwise
    layer_norm followed by linear_fused."""
    first = lins[0]
    if (SPLIT_GEMM and not first.training and not ln.training and not torch.is_grad_enabled() and x.is_cuda and x.dtype == torch.float32
            and not torch.is_autocast_enabled() and x.dim() == 3 and x.is_contiguous() and x.shape[2] == 256 and x.shape[0] * x.shape[1] >= 128
            and tuple(ln.normalized_shape) == (256,) and ln.weight is not None and ln.bias is not None and ln.weight.dtype == torch.float32
            and _on_grid(x, ln.weight, ln.bias) and ln.weight.is_contiguous() and ln.bias.is_contiguous()
            and all(l.weight.dim() in (2, 3) and l.weight.shape[1] == 256 and l.weight.dtype == torch.float32 and (l.weight.dim() == 2 or l.weight.shape[2] == 1)
                    for l in lins)):
        if len(lins) == 1:
            pk = _packed(first)
        else:
            key = tuple((l.weight.data_ptr(), l.weight._version, None if l.bias is None else l.bias._version) for l in lins)
            cache = getattr(first, "_dsp_cat", None)
            if cache is None or cache[0] != key:
                cache = (key, _CatLinear(lins))
                first._dsp_cat = cache
            pk = _packed(cache[1])
        if pk.Cout % 4 == 0 and pk.Cout >= 128:
            B, T, _ = x.shape
            lib = _lib.load()
            with torch.cuda.device(x.device):
                y = torch.empty((B, T, pk.Cout), dtype=torch.float32, device=x.device)
                _lib.check(lib.dsp_linear_ln_split(_lib.ptr(x), x.stride(1), _lib.ptr(ln.weight), _lib.ptr(ln.bias), float(ln.eps), _lib.ptr(pk.hi), _lib.ptr(pk.lo),
                                                   _lib.ptr(pk.bias), None, 0, 1.0, _lib.ptr(y), pk.Cout, B, T, pk.Cout, SplitConv1d.ACT[act], _lib.ptr(lens),
                                                   int(slack), _lib.current_stream_handle()), "dsp_linear_ln_split")
            outs, o = [], 0
            for l in lins:
                outs.append(y[..., o:o + l.weight.shape[0]]); o += l.weight.shape[0]
            return tuple(outs)
    xn = layer_norm(x, ln)
    if len(lins) == 1:
        return (linear(xn, first, act=act, lens=lens, slack=slack),)
    assert act is None
    return linear_fused(xn, lins, lens=lens, slack=slack)


def layer_norm(x: Tensor, ln: "torch.nn.LayerNorm") -> Tensor:
    """ln(x): the one-wave-per-row HIP kernel (dsp_layer_norm) in eval-mode fp32 inference on the GPU, torch otherwise."""
    C = x.shape[-1]
    if (SPLIT_GEMM and not ln.training and not torch.is_grad_enabled() and x.is_cuda and x.dtype == torch.float32 and not torch.is_autocast_enabled()
            and x.is_contiguous() and tuple(ln.normalized_shape) == (C,) and C % 4 == 0 and C <= 2048 and (ln.weight is None or ln.weight.dtype == torch.float32)
            and _on_grid(x, ln.weight, ln.bias) and (ln.weight is None or (ln.weight.is_contiguous() and ln.bias.is_contiguous()))):
        lib = _lib.load()
        with torch.cuda.device(x.device):
            y = torch.empty_like(x)
            _lib.check(lib.dsp_layer_norm(_lib.ptr(x), _lib.ptr(ln.weight), _lib.ptr(ln.bias), float(ln.eps), _lib.ptr(y), x.numel() // C, C,
                                          _lib.current_stream_handle()), "dsp_layer_norm")
        return y
    return ln(x)


def relpos_attention(q: Tensor, k: Tensor, v: Tensor, p: Tensor, bias_u: Tensor, bias_v: Tensor, pad_mask: Optional[Tensor], heads: int) -> Optional[Tensor]:
    """Fused Conformer relative-position attention (dsp_relpos_attention): q, k, v [B,T,C] fp32 (C = heads * 64) with one common row stride
    (contiguous tensors or the three column slices of a fused projection), p [1 or none, 2T-1, C], bias_u / bias_v [heads, 64], pad_mask
    [B,T] bool.  Returns [B,T,C] contiguous, or None when the shape / mode is not served."""
    B, T, C = q.shape
    ld = q.stride(1)
    if (not SPLIT_GEMM or torch.is_grad_enabled() or not q.is_cuda or q.dtype != torch.float32 or torch.is_autocast_enabled() or C != heads * 64
            or any(t.stride(2) != 1 or t.stride(1) != ld or t.stride(0) != T * ld or t.data_ptr() % 16 or t.shape != q.shape for t in (q, k, v)) or ld % 4):
        return None
    pp = p.reshape(-1, C).contiguous()
    if pp.shape[0] != 2 * T - 1 or pp.dtype != torch.float32 or tuple(bias_u.shape) != (heads, 64) or tuple(bias_v.shape) != (heads, 64):
        return None
    lib = _lib.load()
    pm = _mask_bytes(pad_mask)
    bu, bv = bias_u.detach().float().contiguous(), bias_v.detach().float().contiguous()      # named: must outlive the launch
    # the kernel reads all three with 16-byte loads: a view at an odd storage offset gets an aligned copy instead of a C-side error
    pp, bu, bv = (t if t.data_ptr() % 16 == 0 else t.clone() for t in (pp, bu, bv))
    with torch.cuda.device(q.device):
        out = torch.empty((B, T, C), dtype=torch.float32, device=q.device)
        _lib.check(lib.dsp_relpos_attention(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), ld, _lib.ptr(pp), _lib.ptr(bu), _lib.ptr(bv), _lib.ptr(pm),
                                            _lib.ptr(out), B, T, heads, 64, _lib.current_stream_handle()), "dsp_relpos_attention")
    return out


def attention(q: Tensor, k: Tensor, v: Tensor, key_pad_mask: Optional[Tensor], heads: int, q_lens: Optional[Tensor] = None,
              q_slack: int = 0) -> Optional[Tensor]:
    """softmax(q k^T / sqrt(dk) + key padding) v per head at fp32 accuracy on the fp16 matrix cores (dsp_attention_split): q [B,N,C],
    k / v [B,M,C] fp32, possibly column slices of a wider projection output (row-strided views; unit stride inside a row), C = heads * dk
    with dk 64 or 128, key_pad_mask [B,M] bool or None.  Returns [B,N,C] contiguous, or None when the shape / mode is not served
    (training, autocast, other head widths: the caller keeps torch's scaled_dot_product_attention).  q_lens [B] int32: queries from
    q_lens[b] + q_slack on are padding; their 32-query groups are skipped and come back as zeros."""
    B, N, C = q.shape
    M = k.shape[1]
    dk = C // heads
    if (not SPLIT_GEMM or torch.is_grad_enabled() or not q.is_cuda or torch.is_autocast_enabled() or dk * heads != C or dk not in (64, 128)
            or any(t.dtype != torch.float32 or t.stride(2) != 1 or t.stride(0) != t.shape[1] * t.stride(1) or t.stride(1) % 4 or t.data_ptr() % 16
                   for t in (q, k, v)) or k.shape != v.shape or k.shape[0] != B or k.shape[2] != C or N < 1 or M < 1):
        return None
    lib = _lib.load()
    pm = _mask_bytes(key_pad_mask)
    with torch.cuda.device(q.device):
        out = torch.empty((B, N, C), dtype=torch.float32, device=q.device)
        _lib.check(lib.dsp_attention_split(_lib.ptr(q), q.stride(1), _lib.ptr(k), k.stride(1), _lib.ptr(v), v.stride(1), _lib.ptr(pm), _lib.ptr(out),
                                           B, N, M, heads, dk, float(dk) ** -0.5, _lib.ptr(q_lens), int(q_slack), _lib.current_stream_handle()),
                   "dsp_attention_split")
    return out
