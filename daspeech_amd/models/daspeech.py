"""DASpeech model glue in PyTorch-ROCm: Conformer encoder -> DA-Transformer (NAT) decoder with the links head -> FFN adapter
-> FastSpeech2-NoEmb -> (vocoder), behind the reference's plugin names.

Mirrors (structure, tensor contracts, argument names; dense layers are plain torch = hipBLASLt/MIOpen MFMA GEMMs):
  S2TConformerDAGModel           DASpeech/models/s2t_conformer_dag.py:60-443     (links head :140-212, graph size :281-283)
  S2SConformerDAGFastSpeech2     DASpeech/models/s2s_conformer_dag_fastspeech2.py:42-354 (forward :143-173, forward_decoder :194-243)
  S2TConformerEncoder            fairseq/fairseq/models/speech_to_text/s2t_conformer.py:32-162
  ConformerEncoderLayer          fairseq/fairseq/modules/conformer_layer.py:21-286, espnet_multihead_attention.py:111-198
  NATransformerDecoder           fairseq/fairseq/models/nat/nonautoregressive_transformer.py:207-366
The DAG ops and the graph decode are the HIP kernels of this repo (daspeech_amd.custom_ops / daspeech_amd.decode_ops).
Random weights of the released architecture (README.md:288-300) are what the synthetic benchmarks use.
"""
import math
import random
from contextlib import contextmanager
from types import SimpleNamespace
from typing import Dict, Optional

import torch
import torch.nn.functional as F
from torch import Tensor, nn

from .. import decode_ops
from .fastspeech2 import FFNAdapter, FastSpeech2NoEmb

PAD, BOS, EOS, UNK = 1, 0, 2, 3          # fairseq Dictionary defaults

DEFAULT_ARGS = dict(
    input_feat=80, conv_channels=1024, conv_kernels=(5, 5),
    encoder_layers=12, encoder_embed_dim=256, encoder_ffn_embed_dim=2048, encoder_attention_heads=4, depthwise_kernel=31,
    decoder_layers=4, decoder_embed_dim=512, decoder_ffn_embed_dim=2048, decoder_attention_heads=8,
    vocab_size=512, max_target_positions=1024, src_upsample_scale=0.5, max_transition_length=99999,
    decode_strategy="lookahead", decode_beta=1.0, decode_viterbibeta=1.0, adaptor_ffn_dim=1024,
    # README.md:241-243,300-302: --dropout 0.1 --attention-dropout 0.1 --relu-dropout 0.1 (active in train() mode only, at the reference's sites)
    dropout=0.1, attention_dropout=0.1, activation_dropout=0.1,
)


def _drop(x: Tensor, p: float, training: bool) -> Tensor:
    return F.dropout(x, p, True) if training and p > 0 else x


# ------------------------------------------------------------------------------------------------ Conformer encoder
class Conv1dSubsampler(nn.Module):
    """Two stride-2 Conv1d + GLU (speech_to_text/modules/convolution.py:13-59): T -> ~T/4."""

    def __init__(self, in_ch, mid_ch, out_ch, kernels=(5, 5)):
        super().__init__()
        n = len(kernels)
        self.conv_layers = nn.ModuleList(
            nn.Conv1d(in_ch if i == 0 else mid_ch // 2, mid_ch if i < n - 1 else out_ch * 2, k, stride=2, padding=k // 2)
            for i, k in enumerate(kernels))

    def out_lengths(self, lens: Tensor) -> Tensor:
        for _ in self.conv_layers:
            lens = ((lens.float() - 1) / 2 + 1).floor().long()
        return lens

    @staticmethod
    def _fold_stride2(conv: nn.Conv1d):
        """A stride-2 Conv1d(C, Cout, K, padding=K//2) over x[B,T,C] is a stride-1 "same" convolution over the frame PAIRS
        x2[t'] = (x[2t'], x[2t'+1]) (2C channels, zero frame appended to an odd T): y[t] = sum_k w[k] x[2t+k-p] and 2t+k-p = 2(t+a)+r
        puts tap k on pair t+a, half r.  Returns (weight [Cout, Cp, K'], Cp): Cp = 2C rounded up to what the matrix-core kernel
        takes (zero weights on the padding channels and on the half-taps the original does not have)."""
        w = conv.weight.detach().float()
        Cout, C, K = w.shape
        p = K // 2
        amin, amax = (0 - p) // 2, (K - 1 - p) // 2
        A = max(-amin, amax)
        C2 = 2 * C
        Cp = next(c for c in (128, 256, 512) if c >= C2) if C2 <= 512 else (C2 + 511) // 512 * 512
        wf = torch.zeros(Cout, Cp, 2 * A + 1, dtype=torch.float32, device=w.device)
        for k in range(K):
            a, r = (k - p) // 2, (k - p) % 2
            wf[:, r * C:(r + 1) * C, a + A] = w[:, :, k]
        return wf, Cp

    def forward(self, x: Tensor, lens: Tensor):
        if (decode_ops.SPLIT_GEMM and not self.training and not torch.is_grad_enabled() and x.is_cuda and x.dtype == torch.float32
                and not torch.is_autocast_enabled() and self.conv_layers[0].weight.dtype == torch.float32):
            # eval, fp32: the two stride-2 convolutions on the matrix cores at fp32 accuracy (operand splitting), channels-last, as
            # stride-1 convolutions over frame pairs.  MIOpen has no fp32 solver for the first one (80 input channels, stride 2) and
            # runs its naive kernel: 4.0 ms per batch of 32 — a sixth of the whole S2ST batch (profiles/r02g_s2st_kernel_stats.csv)
            key = tuple((c.weight.data_ptr(), c.weight._version) for c in self.conv_layers)
            if getattr(self, "_split_key", None) != key:
                ok = all(c.stride == (2,) and c.dilation == (1,) and c.groups == 1 and c.kernel_size[0] % 2 == 1
                         and c.padding == (c.kernel_size[0] // 2,) and c.out_channels % 4 == 0 for c in self.conv_layers)
                self._split = None
                if ok:
                    self._split = []
                    for c in self.conv_layers:
                        wf, Cp = self._fold_stride2(c)
                        self._split.append((decode_ops.SplitConv1d(wf, c.bias), Cp))
                self._split_key = key
            if self._split is not None:
                for conv, Cp in self._split:
                    B, T, C = x.shape
                    if T % 2: x = F.pad(x, (0, 0, 0, 1))
                    x2 = x.reshape(B, (T + 1) // 2, 2 * C)
                    if Cp != 2 * C: x2 = F.pad(x2, (0, Cp - 2 * C))
                    x = F.glu(conv(x2.contiguous()), dim=-1)
                return x, self.out_lengths(lens)
        if (self.training or torch.is_grad_enabled()) and decode_ops.conv1d_stride2_channels_last_sites_served(x, self.conv_layers):
            # training, fp16 / bf16: the stride-2 convolutions under autograd on the channels-last tensor (csrc/conv1d_stride2_train.hip), no
            # transposes, no MIOpen; bias + GLU as the HIP operator between the GEMMs where it is served (else the bias in the convolution)
            fused = decode_ops.bias_act_dropout_sites_served(x, [(c.out_channels, c.bias, "glu") for c in self.conv_layers])
            for conv in self.conv_layers:
                if fused:
                    x = decode_ops.conv1d_stride2_channels_last_checked(x, conv.weight)
                    x = decode_ops.bias_act_dropout_checked(x, conv.bias, "glu", 0.0, self.training)
                else:
                    x = F.glu(decode_ops.conv1d_stride2_channels_last_checked(x, conv.weight, conv.bias), dim=-1)
            return x, self.out_lengths(lens)
        x = x.transpose(1, 2)                        # B x C x T
        for conv in self.conv_layers:
            x = F.glu(conv(x), dim=1)
        return x.transpose(1, 2), self.out_lengths(lens)


_POS_TABLES: Dict[tuple, Tensor] = {}           # (T, dim, device, dtype) -> table; the table is a constant of its key (read-only)


def rel_positional_encoding(T: int, dim: int, device, dtype) -> Tensor:
    """[1, 2T-1, dim] sinusoid over relative positions T-1 .. -(T-1) (modules/positional_encoding.py RelPositionalEncoding)."""
    key = (T, dim, str(device), dtype)
    hit = _POS_TABLES.get(key)
    if hit is not None:
        return hit
    per_dev = [k for k in _POS_TABLES if k[2] == key[2]]
    if len(per_dev) >= 64:                                  # bounded per device: drop that device's oldest entries only
        for k in per_dev[:32]:
            del _POS_TABLES[k]
    # built outside inference mode and without a graph: a table first requested under torch.inference_mode() would otherwise be an
    # inference tensor and break a later training forward of the same length.  Shared by every model of the process: READ-ONLY.
    with torch.inference_mode(False), torch.no_grad():
        table = _rel_positional_encoding(T, dim, device, dtype)
    _POS_TABLES[key] = table
    return table


def _rel_positional_encoding(T: int, dim: int, device, dtype) -> Tensor:
    pos = torch.arange(T - 1, -T, -1.0, device=device).unsqueeze(1)
    div = torch.exp(torch.arange(0, dim, 2, device=device).float() * -(math.log(10000.0) / dim))
    pe = torch.zeros(2 * T - 1, dim, device=device)
    pe[:, 0::2] = torch.sin(pos * div)
    pe[:, 1::2] = torch.cos(pos * div)
    return pe.unsqueeze(0).to(dtype)


class RelPosSelfAttention(nn.Module):
    def __init__(self, dim, heads, dropout=0.0):
        super().__init__()
        self.h, self.dk = heads, dim // heads
        self.p_attn = dropout                       # on the attention probabilities (espnet_multihead_attention.py:40,82)
        self.linear_q, self.linear_k, self.linear_v, self.linear_out = (nn.Linear(dim, dim) for _ in range(4))
        self.linear_pos = nn.Linear(dim, dim, bias=False)
        self.cache_position_projection = False
        self.pos_bias_u = nn.Parameter(torch.zeros(heads, self.dk))
        self.pos_bias_v = nn.Parameter(torch.zeros(heads, self.dk))
        nn.init.xavier_uniform_(self.pos_bias_u); nn.init.xavier_uniform_(self.pos_bias_v)

    @staticmethod
    def rel_shift(x: Tensor) -> Tensor:              # [B,h,T,2T-1] -> [B,h,T,T]
        B, h, T, P = x.shape
        x = F.pad(x, (1, 0)).view(B, h, P + 1, T)[:, :, 1:].reshape(B, h, T, P)
        return x[..., : P // 2 + 1]

    def _projected_positions(self, pos: Tensor) -> Tensor:
        """linear_pos(pos).  With `cache_position_projection = True` (a serving option, OFF by default and in bench.py: the reference computes
        it in every forward, fairseq espnet_multihead_attention.py:217-218) eval-mode inference keeps the projection per (position table,
        weight version) instead of recomputing it for every batch (12 small GEMMs per encoder pass)."""
        w = self.linear_pos.weight
        if torch.is_grad_enabled() or self.training or not self.cache_position_projection:
            return decode_ops.linear(pos, self.linear_pos)
        key = (pos.data_ptr(), tuple(pos.shape), w.data_ptr(), w._version)
        cache = self.__dict__.setdefault("_pos_proj", {})
        hit = cache.get(key)
        if hit is None:
            if len(cache) >= 64:
                cache.clear()
            cache[key] = hit = (decode_ops.linear(pos, self.linear_pos), pos)         # the table is kept alive with its projection
        return hit[0]

    def forward(self, x: Tensor, pos: Tensor, pad_mask: Optional[Tensor], residual: Optional[Tensor] = None, ln: Optional[nn.LayerNorm] = None) -> Tensor:
        """ln (eval-mode fast path only): the block's pre-LayerNorm, applied inside the stacked q|k|v projection instead of by the caller"""
        B, T, C = x.shape
        L_ = decode_ops.linear
        pp = None                                   # linear_pos(pos), where the training branch has computed it already
        if ln is not None and (self.training or self.dk != 64):
            x, ln = decode_ops.layer_norm(x, ln), None
        if not self.training and self.dk == 64:
            if ln is not None:
                qf, kf, vf = decode_ops.linear_ln(x, ln, (self.linear_q, self.linear_k, self.linear_v))
            else:
                qf, kf, vf = decode_ops.linear_fused(x, (self.linear_q, self.linear_k, self.linear_v))
            o = decode_ops.relpos_attention(qf, kf, vf, self._projected_positions(pos), self.pos_bias_u, self.pos_bias_v, pad_mask, self.h)
            if o is not None:                                         # one fused HIP kernel for scores, shift, soft-max and the value product
                return L_(o, self.linear_out, residual=residual)
            qf, kf, vf = qf.contiguous(), kf.contiguous(), vf.contiguous()
            q, k, v = qf.view(B, T, self.h, self.dk), kf.view(B, T, self.h, self.dk).transpose(1, 2), vf.view(B, T, self.h, self.dk).transpose(1, 2)
        else:
            qf, kf, vf = L_(x, self.linear_q), L_(x, self.linear_k), L_(x, self.linear_v)
            if self.dk == 64 and qf.is_cuda and qf.dtype != torch.float32:
                # scores, shift, mask, soft-max, dropout and the value product as ONE HIP operator with its own backward
                # (csrc/relpos_attention_train.hip): no [B,h,T,T] tensor is kept for autograd
                pp = L_(pos, self.linear_pos).reshape(-1, C)
                if decode_ops.relpos_attention_autograd_served(qf, kf, vf, pp, self.pos_bias_u, self.pos_bias_v, pad_mask, self.h):
                    o = decode_ops.relpos_attention_checked(qf, kf, vf, pp, self.pos_bias_u, self.pos_bias_v, pad_mask, self.h,
                                                            p=self.p_attn, training=self.training)
                    return L_(o, self.linear_out, residual=residual)
            q = qf.view(B, T, self.h, self.dk)
            k = kf.view(B, T, self.h, self.dk).transpose(1, 2)
            v = vf.view(B, T, self.h, self.dk).transpose(1, 2)
        p = (L_(pos, self.linear_pos) if pp is None else pp).view(1, -1, self.h, self.dk).transpose(1, 2)
        ac = torch.matmul((q + self.pos_bias_u).transpose(1, 2), k.transpose(-2, -1))
        bd = self.rel_shift(torch.matmul((q + self.pos_bias_v).transpose(1, 2), p.transpose(-2, -1)))
        scores = (ac + bd) / math.sqrt(self.dk)
        if pad_mask is not None:
            scores = scores.masked_fill(pad_mask.view(B, 1, 1, T), float("-inf"))
        att = _drop(torch.softmax(scores, dim=-1), self.p_attn, self.training)
        return decode_ops.linear(torch.matmul(att, v).transpose(1, 2).reshape(B, T, C), self.linear_out, residual=residual)


class ConformerLayer(nn.Module):
    def __init__(self, dim, ffn, heads, dw_kernel, dropout=0.0):
        super().__init__()
        self.p = dropout                            # one rate for every dropout of the layer (conformer_layer.py:175-227)
        def ffn_block():
            return nn.ModuleDict(dict(layer_norm=nn.LayerNorm(dim), w_1=nn.Linear(dim, ffn), w_2=nn.Linear(ffn, dim)))
        self.ffn1, self.ffn2 = ffn_block(), ffn_block()
        self.self_attn_layer_norm = nn.LayerNorm(dim)
        self.self_attn = RelPosSelfAttention(dim, heads, dropout)
        self.conv_module = nn.ModuleDict(dict(
            layer_norm=nn.LayerNorm(dim), pointwise_conv1=nn.Conv1d(dim, 2 * dim, 1, bias=False),
            depthwise_conv=nn.Conv1d(dim, dim, dw_kernel, padding=(dw_kernel - 1) // 2, groups=dim, bias=False),
            batch_norm=nn.BatchNorm1d(dim), pointwise_conv2=nn.Conv1d(dim, dim, 1, bias=False)))
        self.final_layer_norm = nn.LayerNorm(dim)

    @staticmethod
    def _ffn(m, x):
        """x + 0.5 * w_2(silu(w_1(layer_norm(x))))  — the macaron half-step, residual included."""
        y = decode_ops.ffn_fused(x, m["layer_norm"], m["w_1"], m["w_2"], "silu", residual=x, alpha=0.5)      # one launch, hidden activations in LDS
        if y is not None:
            return y
        L_ = decode_ops.linear                 # fp32-accurate split GEMMs (bias, SiLU, scale and residual in their epilogues) in eval-mode
        return L_(L_(decode_ops.layer_norm(x, m["layer_norm"]), m["w_1"], act="silu"), m["w_2"], residual=x, alpha=0.5)      # fp32 inference, torch otherwise

    def _resnorm_served(self, x):
        """one question per forward for the four wired sites (their LayerNorm and the bias that rides in the operator)"""
        return decode_ops.residual_dropout_layer_norm_sites_served(x, (
            (self.self_attn_layer_norm, self.ffn1["w_2"].bias), (self.conv_module["layer_norm"], None), (self.ffn2["layer_norm"], None),
            (self.final_layer_norm, self.ffn2["w_2"].bias)))

    def _actdrop_served(self, x):
        """one question per forward for the three activation sites (both SiLU + dropout passes with the bias of their w_1, and the GLU)"""
        w1, w2 = self.ffn1["w_1"], self.ffn2["w_1"]
        return decode_ops.bias_act_dropout_sites_served(x, (
            (w1.out_features, w1.bias, "silu"), (w2.out_features, w2.bias, "silu"), (self.conv_module["pointwise_conv1"].out_channels, None, "glu")))

    def _forward_train_resnorm(self, x, pos, pad_mask, ad):
        """The training branch with every `x = x + alpha * dropout(block(LayerNorm(x)))` boundary as one HIP operator (csrc/residual_norm_train.hip):
        the residual add, the dropout and the NEXT block's LayerNorm in one pass that returns both the sum and its norm; the bias of each
        w_2 rides in the operator, so that Linear runs without it and its bias gradient is one of the operator's column sums."""
        c, p, tr = self.conv_module, self.p, self.training
        rn = decode_ops.residual_dropout_layer_norm_checked
        bad = decode_ops.bias_act_dropout_checked

        def ffn(m, y):                              # conformer_layer.py:140-146 up to w_2's product: dropout1 after the activation
            if ad:                                  # bias + SiLU + dropout1 as one HIP operator (csrc/act_dropout_train.hip); w_1's bias rides in it
                return F.linear(bad(F.linear(y, m["w_1"].weight), m["w_1"].bias, "silu", p, tr), m["w_2"].weight)
            return F.linear(_drop(F.silu(m["w_1"](y)), p, tr), m["w_2"].weight)
        y = self.ffn1["layer_norm"](x)             # a LayerNorm alone: the operator's h = None form is slower than torch's here
        x, y = rn(ffn(self.ffn1, y), x, self.self_attn_layer_norm, bias=self.ffn1["w_2"].bias, alpha=0.5, p=p, training=tr)
        x, y = rn(self.self_attn(y, pos, pad_mask), x, c["layer_norm"], p=p, training=tr)                 # :267
        y = F.linear(y, c["pointwise_conv1"].weight.squeeze(-1))
        y = bad(y, None, "glu") if ad else F.glu(y, dim=-1)
        if decode_ops.dwconv_bn_silu_autograd_served(y, c["depthwise_conv"], c["batch_norm"]):
            y = decode_ops.dwconv_bn_silu_autograd(y, c["depthwise_conv"].weight, c["batch_norm"])
        else:
            y = F.silu(c["batch_norm"](c["depthwise_conv"](y.transpose(1, 2)))).transpose(1, 2)
        x, y = rn(F.linear(y, c["pointwise_conv2"].weight.squeeze(-1)), x, self.ffn2["layer_norm"], p=p, training=tr)      # :100
        return rn(ffn(self.ffn2, y), x, self.final_layer_norm, bias=self.ffn2["w_2"].bias, alpha=0.5, p=p, training=tr, return_sum=False)

    def forward(self, x, pos, pad_mask):
        c = self.conv_module
        if self.training or torch.is_grad_enabled():
            p, tr = self.p, self.training
            ad = self._actdrop_served(x)               # the element-wise passes between the GEMMs as HIP operators (same conditions)
            if self._resnorm_served(x):                # the block boundaries as HIP operators (GPU, fp32 / fp16 / bf16, no autocast)
                return self._forward_train_resnorm(x, pos, pad_mask, ad)
            # otherwise plain torch ops only (the step is host-launch bound: every helper indirection and extra view costs)
            bad = decode_ops.bias_act_dropout_checked

            def ffn(m, x):                          # conformer_layer.py:140-146: dropout1 after the activation, dropout2 after w_2
                if ad:
                    return x + 0.5 * _drop(m["w_2"](bad(F.linear(m["layer_norm"](x), m["w_1"].weight), m["w_1"].bias, "silu", p, tr)), p, tr)
                return x + 0.5 * _drop(m["w_2"](_drop(F.silu(m["w_1"](m["layer_norm"](x))), p, tr)), p, tr)
            x = ffn(self.ffn1, x)
            x = x + _drop(self.self_attn(self.self_attn_layer_norm(x), pos, pad_mask), p, tr)          # :267
            # the two pointwise (kernel 1) convolutions are GEMMs on the [B,T,C] layout the layer already has: F.linear on the
            # checkpoint's [out, in, 1] weights instead of Conv1d, which MIOpen runs as im2col + GEMM between two transposes
            if ad:
                y = bad(F.linear(c["layer_norm"](x), c["pointwise_conv1"].weight.squeeze(-1)), None, "glu")
            else:
                y = F.glu(F.linear(c["layer_norm"](x), c["pointwise_conv1"].weight.squeeze(-1)), dim=-1)
            if decode_ops.dwconv_bn_silu_autograd_served(y, c["depthwise_conv"], c["batch_norm"]):
                # depthwise conv + batch-statistics BN + SiLU and their backward as HIP passes over [B,T,C] (csrc/conformer_train.hip): no transposes
                y = decode_ops.dwconv_bn_silu_autograd(y, c["depthwise_conv"].weight, c["batch_norm"])
                x = x + _drop(F.linear(y, c["pointwise_conv2"].weight.squeeze(-1)), p, tr)              # :100
            else:
                y = F.silu(c["batch_norm"](c["depthwise_conv"](y.transpose(1, 2))))
                x = x + _drop(F.linear(y.transpose(1, 2), c["pointwise_conv2"].weight.squeeze(-1)), p, tr)  # :100
            x = ffn(self.ffn2, x)
            return self.final_layer_norm(x)
        # pre-norm blocks with their LayerNorms folded into the kernels around them (eval): ffn1 (LayerNorm while staging) -> attention (its
        # LayerNorm inside the stacked q|k|v projection) -> convolution module (its LayerNorm inside pointwise_conv1) -> ffn2, whose
        # reduction also applies final_layer_norm
        x = self._ffn(self.ffn1, x)
        x = self.self_attn(x, pos, pad_mask, residual=x, ln=self.self_attn_layer_norm)
        y = F.glu(decode_ops.linear_ln(x, c["layer_norm"], (c["pointwise_conv1"],))[0], dim=-1)
        dw = c["depthwise_conv"]
        if y.is_cuda and y.shape[-1] % 4 == 0 and dw.kernel_size[0] in (3, 7, 15, 31) and dw.bias is None:
            y = decode_ops.dwconv_bn_silu(y, dw.weight, c["batch_norm"])       # one HIP pass on [B,T,C], no transposes
        else:
            y = F.silu(c["batch_norm"](dw(y.transpose(1, 2)))).transpose(1, 2)
        x = decode_ops.linear(y.contiguous(), c["pointwise_conv2"], residual=x)
        m = self.ffn2
        fused = decode_ops.ffn_fused(x, m["layer_norm"], m["w_1"], m["w_2"], "silu", residual=x, alpha=0.5, post_ln=self.final_layer_norm, need_out=False)
        if fused is not None:
            return fused[1]
        x = self._ffn(self.ffn2, x)
        return decode_ops.layer_norm(x, self.final_layer_norm)


class ConformerEncoder(nn.Module):
    def __init__(self, a):
        super().__init__()
        self.subsample = Conv1dSubsampler(a.input_feat, a.conv_channels, a.encoder_embed_dim, a.conv_kernels)
        self.embed_scale = math.sqrt(a.encoder_embed_dim)
        self.linear = nn.Linear(a.encoder_embed_dim, a.encoder_embed_dim)
        self.conformer_layers = nn.ModuleList(
            ConformerLayer(a.encoder_embed_dim, a.encoder_ffn_embed_dim, a.encoder_attention_heads, a.depthwise_kernel, a.dropout)
            for _ in range(a.encoder_layers))
        self.p = a.dropout

    def forward(self, src_tokens: Tensor, src_lengths: Tensor) -> Dict[str, Tensor]:
        x, lens = self.subsample(src_tokens, src_lengths)
        T = x.shape[1]
        pad_mask = torch.arange(T, device=x.device).unsqueeze(0) >= lens.unsqueeze(1)
        lin = self.linear
        if self.training and self.p > 0 and decode_ops.bias_act_dropout_sites_served(x, ((lin.out_features, lin.bias, "identity"),)):
            # bias + dropout as one HIP operator (csrc/act_dropout_train.hip): the Linear runs without its bias
            x = decode_ops.bias_act_dropout_checked(F.linear(self.embed_scale * x, lin.weight), lin.bias, "identity", self.p, True)
        else:
            x = _drop(decode_ops.linear(self.embed_scale * x, self.linear), self.p, self.training)    # s2t_conformer.py:119-120
        pos = rel_positional_encoding(T, x.shape[-1], x.device, x.dtype)
        for layer in self.conformer_layers:
            x = layer(x, pos, pad_mask)
        return {"encoder_out": x, "encoder_padding_mask": pad_mask, "encoder_lengths": lens}


# ------------------------------------------------------------------------------------------------ NAT decoder + links head
class _MHA(nn.Module):
    def __init__(self, dim, heads, kdim=None, dropout=0.0):
        super().__init__()
        kdim = kdim or dim
        self.h = heads
        self.p_attn = dropout                       # --attention-dropout, on the attention probabilities (multihead_attention.py)
        self.q_proj, self.out_proj = nn.Linear(dim, dim), nn.Linear(dim, dim)
        self.k_proj, self.v_proj = nn.Linear(kdim, dim), nn.Linear(kdim, dim)

    def forward(self, x, mem, mem_pad, residual=None, lens=None, mem_lens=None):
        """lens / mem_lens [B] int32 (eval-mode GPU inference, optional): rows of x / mem from there on are padding nothing valid depends
        on — a Transformer layer has no path from a padded position to a valid one — and the matrix-core kernels skip their tiles."""
        B, N, C = x.shape
        M = mem.shape[1]
        L_ = decode_ops.linear
        if not self.training:
            # eval: stacked projections (q|k|v of self-attention, k|v of the encoder attention) and the fp32-accurate matrix-core attention
            if mem is x:
                qf, kf, vf = decode_ops.linear_fused(x, (self.q_proj, self.k_proj, self.v_proj), lens=lens)
            else:
                qf = L_(x, self.q_proj, lens=lens)
                kf, vf = decode_ops.linear_fused(mem, (self.k_proj, self.v_proj), lens=mem_lens)
            o = decode_ops.attention(qf, kf, vf, mem_pad, self.h, q_lens=lens)
            if o is not None:
                return L_(o, self.out_proj, residual=residual, lens=lens)
            q, k, v = (t.reshape(B, -1, self.h, C // self.h).transpose(1, 2) for t in (qf, kf, vf))
        else:
            q, k, v = L_(x, self.q_proj), L_(mem, self.k_proj), L_(mem, self.v_proj)
            if decode_ops.mha_attention_autograd_served(q, k, v, mem_pad, self.h):
                # fp16 / bf16 on the GPU: the projections as they are ([B,.,C], no transposes, no additive mask tensor), scores + mask +
                # soft-max + dropout + value product as one HIP operator (csrc/mha_train.hip), its output straight into out_proj
                o = decode_ops.mha_attention_checked(q, k, v, mem_pad, self.h, p=self.p_attn, training=True)
                return decode_ops.linear(o, self.out_proj, residual=residual)
            q = q.view(B, N, self.h, -1).transpose(1, 2)
            k = k.view(B, M, self.h, -1).transpose(1, 2)
            v = v.view(B, M, self.h, -1).transpose(1, 2)
        mask = None
        if mem_pad is not None:
            mask = torch.zeros(B, 1, 1, M, dtype=x.dtype, device=x.device).masked_fill(mem_pad.view(B, 1, 1, M), float("-inf"))
        o = F.scaled_dot_product_attention(q, k, v, attn_mask=mask, dropout_p=self.p_attn if self.training else 0.0)
        return decode_ops.linear(o.transpose(1, 2).reshape(B, N, C), self.out_proj, residual=residual)


class NATDecoderLayer(nn.Module):
    """Post-norm Transformer decoder layer without causal mask (modules/transformer_layer.py, NAT usage)."""

    def __init__(self, dim, ffn, heads, enc_dim, dropout=0.0, attention_dropout=0.0, activation_dropout=0.0):
        super().__init__()
        self.p, self.p_act = dropout, activation_dropout                                  # transformer_layer.py:263-298
        self.self_attn, self.self_attn_layer_norm = _MHA(dim, heads, dropout=attention_dropout), nn.LayerNorm(dim)
        self.encoder_attn, self.encoder_attn_layer_norm = _MHA(dim, heads, enc_dim, dropout=attention_dropout), nn.LayerNorm(dim)
        self.fc1, self.fc2, self.final_layer_norm = nn.Linear(dim, ffn), nn.Linear(ffn, dim), nn.LayerNorm(dim)

    def forward(self, x, self_pad, enc, enc_pad, lens=None, enc_lens=None):
        if self.training or torch.is_grad_enabled():
            p, tr = self.p, self.training                                                 # transformer_layer.py:467,497,507,511
            rn = decode_ops.residual_dropout_layer_norm_checked
            ad = decode_ops.bias_act_dropout_sites_served(x, ((self.fc1.out_features, self.fc1.bias, "gelu"),))
            if decode_ops.residual_dropout_layer_norm_sites_served(x, ((self.self_attn_layer_norm, None), (self.encoder_attn_layer_norm, None),
                                                                       (self.final_layer_norm, self.fc2.bias))):
                # each post-norm site (residual add, dropout, LayerNorm) as one HIP operator (csrc/residual_norm_train.hip); fc2's bias rides in it
                x = rn(self.self_attn(x, x, self_pad), x, self.self_attn_layer_norm, p=p, training=tr, return_sum=False)
                x = rn(self.encoder_attn(x, enc, enc_pad), x, self.encoder_attn_layer_norm, p=p, training=tr, return_sum=False)
                if ad:                                 # fc1's bias + GELU + activation dropout as one HIP operator (csrc/act_dropout_train.hip)
                    h = decode_ops.bias_act_dropout_checked(F.linear(x, self.fc1.weight), self.fc1.bias, "gelu", self.p_act, tr)
                    h = F.linear(h, self.fc2.weight)
                else:
                    h = F.linear(_drop(F.gelu(self.fc1(x)), self.p_act, tr), self.fc2.weight)
                return rn(h, x, self.final_layer_norm, bias=self.fc2.bias, p=p, training=tr, return_sum=False)
            x = self.self_attn_layer_norm(x + _drop(self.self_attn(x, x, self_pad), p, tr))
            x = self.encoder_attn_layer_norm(x + _drop(self.encoder_attn(x, enc, enc_pad), p, tr))
            if ad:
                h = decode_ops.bias_act_dropout_checked(F.linear(x, self.fc1.weight), self.fc1.bias, "gelu", self.p_act, tr)
                return self.final_layer_norm(x + _drop(self.fc2(h), p, tr))
            return self.final_layer_norm(x + _drop(self.fc2(_drop(F.gelu(self.fc1(x)), self.p_act, tr)), p, tr))
        x = decode_ops.layer_norm(self.self_attn(x, x, self_pad, residual=x, lens=lens, mem_lens=lens), self.self_attn_layer_norm)
        x = decode_ops.layer_norm(self.encoder_attn(x, enc, enc_pad, residual=x, lens=lens, mem_lens=enc_lens), self.encoder_attn_layer_norm)
        return decode_ops.layer_norm(decode_ops.linear(decode_ops.linear(x, self.fc1, act="gelu", lens=lens), self.fc2, residual=x, lens=lens),
                                     self.final_layer_norm)


class DAGDecoder(nn.Module):
    def __init__(self, a):
        super().__init__()
        d = a.decoder_embed_dim
        self.a = a
        self.embed_tokens = nn.Embedding(a.vocab_size, d, padding_idx=PAD)
        self.embed_positions = nn.Embedding(a.max_target_positions + PAD + 1, d, padding_idx=PAD)
        self.embed_scale = math.sqrt(d)
        self.layers = nn.ModuleList(NATDecoderLayer(d, a.decoder_ffn_embed_dim, a.decoder_attention_heads, a.encoder_embed_dim,
                                                    a.dropout, a.attention_dropout, a.activation_dropout) for _ in range(a.decoder_layers))
        # links head (s2t_conformer_dag.py:75-92: links_feature = feature:position)
        self.link_positional = nn.Embedding(a.max_target_positions + PAD + 1, d, padding_idx=PAD)
        self.query_linear, self.key_linear = nn.Linear(2 * d, d), nn.Linear(2 * d, d)
        self.gate_linear = nn.Linear(2 * d, a.decoder_attention_heads)
        self.ragged = True                      # eval-mode GPU inference: skip the tiles of padded graph positions (they reach no valid one)
        self.fused_links = True                 # fused compact-band HIP kernels, forward and backward (False: the torch formulation)

    @staticmethod
    def positions(tokens: Tensor) -> Tensor:
        keep = tokens.ne(PAD).int()
        return (torch.cumsum(keep, dim=1) * keep).long() + PAD

    def ragged_lengths(self, prev_output_tokens: Tensor) -> Optional[Tensor]:
        """[B] int32 valid graph lengths for the tile-skipping kernels of eval-mode GPU inference (None: compute every padded row)"""
        if self.ragged and not self.training and not torch.is_grad_enabled() and prev_output_tokens.is_cuda:
            return decode_ops.valid_lengths(prev_output_tokens.eq(PAD))
        return None

    def extract_features(self, prev_output_tokens: Tensor, enc: Dict[str, Tensor], lens: Optional[Tensor] = None) -> Tensor:
        if (self.training or torch.is_grad_enabled()) and decode_ops.embed_entry_served(prev_output_tokens, self.embed_tokens, self.embed_positions):
            # token embedding, learned positions and the embedding dropout as one HIP operator (csrc/embed_entry_train.hip); its backward
            # builds one inverted index for both tables (nearly every graph vertex is <unk>)
            x = decode_ops.embed_entry_checked(prev_output_tokens, self.embed_tokens.weight, self.embed_positions.weight, PAD, self.embed_scale,
                                               self.a.dropout, self.training)
        else:
            x = self.embed_scale * self.embed_tokens(prev_output_tokens) + self.embed_positions(self.positions(prev_output_tokens))
            x = _drop(x, self.a.dropout, self.training)                                   # nonautoregressive_transformer.py:349
        pad = prev_output_tokens.eq(PAD)
        enc_lens = None if lens is None else decode_ops.valid_lengths(enc["encoder_padding_mask"])
        for layer in self.layers:
            x = layer(x, pad, enc["encoder_out"], enc["encoder_padding_mask"], lens, enc_lens)
        return x

    def output_layer(self, feats: Tensor, lens: Optional[Tensor] = None) -> Tensor:
        return decode_ops.linear(feats, self.embed_tokens, lens=lens)        # --share-decoder-input-output-embed (weight [V, d], no bias)

    def extract_links(self, feats: Tensor, prev_output_tokens: Tensor, dist_bias: Optional[Tensor] = None, lens: Optional[Tensor] = None) -> Tensor:
        """Compact transition log-probs [B, L, TR] fp32 — float64 for float64 `feats` — (s2t_conformer_dag.py:171-212, banded branch
        :191-202).  `dist_bias` [>= TR] (optional, not in the reference) is added to the content score of distance d before the window soft-max."""
        a = self.a
        B, L, d = feats.shape
        h, ck = a.decoder_attention_heads, d // a.decoder_attention_heads
        fp = torch.cat([feats, self.link_positional(self.positions(prev_output_tokens))], dim=-1)
        # float64 features (a double-precision check): q, k and the gates stay double, and so do the links of either branch below — the
        # double kernels of csrc/extract_links_f64.hip, or the torch formulation; every other dtype gives fp32 links, as in the reference
        lt = torch.float64 if feats.dtype == torch.float64 else torch.float
        q = decode_ops.linear(fp, self.query_linear, lens=lens).view(B, L, h, ck).to(lt)
        k = decode_ops.linear(fp, self.key_linear, lens=lens).view(B, L, h, ck).to(lt)
        log_gates = F.log_softmax(decode_ops.linear(fp, self.gate_linear), dim=-1, dtype=lt)                            # [B,L,h]
        TR = min(a.max_transition_length, L - 1)
        # the fused kernels keep one tile's scores in LDS: up to TR ~ 1100 (ck = 64) the whole window is ONE tile; wider windows — the README's
        # --max-transition-length 99999 on graphs up to BASELINE's L = 4096 — are walked in 512-slot tiles (r05: extract_links_tiled_kernel,
        # forward and backward), so every window stays on the HIP path
        if feats.is_cuda and h == 8 and ck in (32, 64, 128) and TR >= 1 and self.fused_links \
                and not (dist_bias is not None and dist_bias.requires_grad and torch.is_grad_enabled()):
            # the band only, fused (csrc/extract_links.hip) — no [B,L,L,h] content tensor, no gather; under autograd the backward
            # recomputes the scores tile by tile from q, k and [B,L,h] soft-max state (dsp_extract_links_bwd)
            bias = None if dist_bias is None else dist_bias[:TR]
            olen = prev_output_tokens.ne(PAD).sum(-1)
            if torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or log_gates.requires_grad):
                return decode_ops.extract_links_autograd(q, k, log_gates, olen, TR, bias)
            return decode_ops.extract_links(q, k, log_gates, olen, TR, bias)
        content = torch.einsum("bicf,bjcf->bijc", q, k) / (ck ** 0.5)                               # [B,L,L,h]
        idx = torch.arange(L, device=feats.device).unsqueeze(1) + torch.arange(TR, device=feats.device).unsqueeze(0) + 1
        out_len = prev_output_tokens.ne(PAD).sum(-1)
        invalid = idx.unsqueeze(0) >= out_len.view(B, 1, 1)                                          # [B,L,TR]
        gidx = idx.unsqueeze(0).masked_fill(invalid, 0)
        band = content.gather(2, gidx.unsqueeze(-1).expand(-1, -1, -1, h))
        if dist_bias is not None:
            band = band + dist_bias[:TR].to(band).view(1, 1, TR, 1)
        band = band.masked_fill(invalid.unsqueeze(-1), float("-inf"))
        nouse = invalid.all(-1)                                                                      # [B,L]
        band = band.masked_fill(nouse.view(B, L, 1, 1), 0.0)                # avoid NaN rows; re-masked below (:199-201)
        band = F.log_softmax(band, dim=2).masked_fill(invalid.unsqueeze(-1), float("-inf"))
        band = band.masked_fill(nouse.view(B, L, 1, 1), float("-inf"))
        from ..custom_ops import logsumexp_keepdim                 # -inf safe (no NaN gradients on fully masked entries)
        return logsumexp_keepdim(band + log_gates.unsqueeze(2), -1).squeeze(-1).masked_fill(invalid, float("-inf"))


@contextmanager
def _same_draws(seed: int, device, active: bool):
    """The reference runs both decoder passes of the GLAT forward under `torch_seed(rand_seed)` (s2t_conformer_dag.py:39-50,214-215): the
    same dropout masks in the glancing pass and in the training pass, the surrounding random stream untouched.
    While a decode_ops.DropoutState.draws() scope is active on the model's device (a graph capture refuses a reseeded generator, and the
    HIP operators draw from the state there): the first pass under a seed marks the state's host counter, a later pass under that seed
    rewinds to the mark — the same masks — and the generator is not touched.  What differs from the eager form there, by construction:
    the passes CONSUME offsets of the scope (the surrounding stream is not left untouched: the calls behind the pair go on from the highest
    offset either pass reached); marks pair up — the second pass under a seed rewinds and forgets the mark, so a third pass under the same
    seed in that scope starts a pair of its own instead of sharing masks; and only the HIP operators' masks are repeated — a dropout
    site that stays on its torch lines inside the scope (fp32 attention, a switched-off operator) draws from the generator in both passes
    and is NOT the same in the two, as nothing reseeds it."""
    if not active:
        yield
        return
    state = decode_ops._active_dropout_state(device)
    if state is not None:
        mark = state._seed_marks.pop(seed, None)
        if mark is None:
            state._seed_marks[seed] = state.mark()
            yield
        else:
            state.rewind(mark)
            try:
                yield
            finally:
                state._catch_up()            # a second pass that drew fewer masks leaves no spent offset to the calls behind it
        return
    if device.type == "cuda":
        # the generator of the MODEL's device (not the current one): state saved, seeded and restored on that device
        state = torch.cuda.get_rng_state(device)
        with torch.cuda.device(device):
            torch.cuda.manual_seed(seed)
        try:
            yield
        finally:
            torch.cuda.set_rng_state(state, device)
    else:
        state = torch.random.get_rng_state()
        torch.random.manual_seed(seed)
        try:
            yield
        finally:
            torch.random.set_rng_state(state)


# ------------------------------------------------------------------------------------------------ models
class S2TConformerDAGModel(nn.Module):
    """registered name: s2t_conformer_dag"""

    def __init__(self, **kw):
        super().__init__()
        self.args = SimpleNamespace(**{**DEFAULT_ARGS, **kw})
        self.pad, self.bos, self.eos, self.unk = PAD, BOS, EOS, UNK
        self.encoder = ConformerEncoder(self.args)
        self.decoder = DAGDecoder(self.args)

    # ---- reference checkpoints ----------------------------------------------------------------------
    # fairseq saves {"model": state_dict, "cfg": ..., ...} (checkpoint_utils.py:288).  Parameter names here follow the reference
    # modules, so the state dict loads key for key once the entries that are not parameters of this implementation are set
    # aside: the tied output projection (a second name for decoder.embed_tokens.weight, s2t_conformer_dag.py:96-97), the length
    # predictor embedding of the NAT base decoder (unused by the DAG decode), fairseq's `version` buffers and the
    # `_float_tensor` placeholders of sinusoidal position tables, and the token embedding the FastSpeech2 encoder's parent class
    # builds but FastSpeech2EncoderNoEmb never reads.  PINNED (r03) to the key -> shape manifest of the reference model built with the
    # README's flags (tests/golden/ckpt_manifest.json, generated by tests/golden/make_golden_model.py from the reference's own
    # build_model): every one of its 736 keys is either loaded or in this list.  `strict=True` reports any other difference.
    _IGNORED_CKPT_SUFFIXES = (".version", "._float_tensor", "decoder.embed_length.weight", "tts.embed_tokens.weight")

    def load_reference_state_dict(self, ckpt: Dict, strict: bool = True):
        sd = ckpt["model"] if isinstance(ckpt, dict) and "model" in ckpt and isinstance(ckpt["model"], dict) else ckpt
        sd = {k: v for k, v in sd.items() if not k.endswith(self._IGNORED_CKPT_SUFFIXES)}
        tied = sd.pop("decoder.output_projection.weight", None)
        if tied is not None and "decoder.embed_tokens.weight" in sd and not torch.equal(tied, sd["decoder.embed_tokens.weight"]):
            raise ValueError("checkpoint has an UNTIED decoder.output_projection (trained without --share-decoder-input-output-embed): "
                             "not supported")
        own = self.state_dict()
        missing = [k for k in own if k not in sd and not k.endswith("num_batches_tracked")]
        unexpected = [k for k in sd if k not in own]
        bad_shape = [k for k in sd if k in own and tuple(sd[k].shape) != tuple(own[k].shape)]
        if strict and (missing or unexpected or bad_shape):
            raise KeyError(f"reference checkpoint does not match: missing={missing[:8]} unexpected={unexpected[:8]} shape={bad_shape[:8]} "
                           f"({len(missing)}/{len(unexpected)}/{len(bad_shape)} keys)")
        self.load_state_dict({k: v for k, v in sd.items() if k in own and k not in bad_shape}, strict=False)
        return missing, unexpected

    # graph size: L = clamp(src_upsample_scale * src_frames, 2, max_target_positions)   (s2t_conformer_dag.py:281-283)
    def initialize_output_tokens_by_src(self, src_lengths: Tensor, max_src_len: int = None) -> Tensor:
        """`max_src_len` (the padded frame count of the batch, a host integer) spares the device->host sync on `L.max()`; the
        graph is then as wide as the longest utterance COULD be, which is what it is in a batch padded to its longest."""
        L = (src_lengths.float() * self.args.src_upsample_scale).long().clamp(2, self.args.max_target_positions)
        if max_src_len is not None:
            maxl = min(max(int(float(max_src_len) * self.args.src_upsample_scale), 2), self.args.max_target_positions)
        else:
            maxl = int(L.max().item())
        ar = torch.arange(maxl, device=src_lengths.device).unsqueeze(0)
        toks = torch.full((len(L), maxl), self.unk, dtype=torch.long, device=src_lengths.device)
        toks = toks.masked_fill(ar >= L.unsqueeze(1), self.pad)
        toks[:, 0] = self.bos
        return toks.scatter(1, (L - 1).unsqueeze(1), self.eos)

    def forward_encoder(self, src_tokens, src_lengths):
        return self.encoder(src_tokens, src_lengths)

    def decode_graph(self, prev_output_tokens, enc):
        lens = self.decoder.ragged_lengths(prev_output_tokens)       # eval-mode GPU inference: padded graph positions are not computed
        feats = self.decoder.extract_features(prev_output_tokens, enc, lens=lens)
        logits = self.decoder.output_layer(feats, lens)
        return logits, self.decoder.extract_links(feats, prev_output_tokens, lens=lens), feats

    def initialize_output_tokens_by_tokens(self, src_tokens: Tensor, src_lengths: Tensor) -> Tensor:
        """The criteria's entry point (nat_dag_loss.py:191): graph skeleton <bos> <unk>... <eos> of length scale * src_len."""
        return self.initialize_output_tokens_by_src(src_lengths, max_src_len=src_tokens.shape[1])

    def forward(self, src_tokens, src_lengths, prev_output_tokens, tgt_tokens=None, glat=None, glat_function=None):
        """Training forward with the GLAT two-pass scheme (s2s_conformer_dag_fastspeech2.py:143-173): pass 1 (no gradient unless
        glat["require_glance_grad"]) picks the glanced positions through `glat_function(self, word_ins_out, tgt_tokens,
        prev_output_tokens, glat, links=links)`, pass 2 produces word_ins / links / features; glat_info is merged into the result."""
        enc = self.encoder(src_tokens, src_lengths)
        glat_info = None
        seeded = self.training and max(self.args.dropout, self.args.attention_dropout, self.args.activation_dropout) > 0
        rand_seed = random.randint(0, 19260817) if seeded else 0                                             # s2t_conformer_dag.py:242
        if glat and glat_function is not None and tgt_tokens is not None:
            with torch.set_grad_enabled(bool(glat.get("require_glance_grad", False)) and torch.is_grad_enabled()):
                with _same_draws(rand_seed, src_tokens.device, seeded):
                    logits, links, _ = self.decode_graph(prev_output_tokens, enc)
                prev_output_tokens, tgt_tokens, glat_info = glat_function(self, logits, tgt_tokens, prev_output_tokens, glat, links=links)
                logits = None
            # Under torch.autocast the first pass has just filled the autocast cache with low-precision copies of the decoder's
            # weights made WITHOUT gradient history; pass 2 would reuse them and no gradient would reach the decoder's Linear layers
            # or the link predictor (r02: 86 of 695 parameters never trained under `--fp16`-style autocast).  The reference runs a
            # pure fp16 model under fairseq's FP16Optimizer and has no such cache.
            if torch.is_autocast_enabled() and torch.is_grad_enabled():
                torch.clear_autocast_cache()
        with _same_draws(rand_seed, src_tokens.device, seeded):
            logits, links, feats = self.decode_graph(prev_output_tokens, enc)
        ret = {"word_ins": {"out": logits, "tgt": tgt_tokens, "mask": tgt_tokens.ne(self.pad) if tgt_tokens is not None else None,
                            "nll_loss": True, "features": feats},
               "links": links, "prev_output_tokens": prev_output_tokens}
        if glat_info is not None:
            ret.update(glat_info)
        return ret

    @torch.no_grad()
    def forward_decoder(self, prev_output_tokens: Tensor, enc: Dict[str, Tensor]):
        """Graph decode on the GPU: lookahead / greedy (s2s_conformer_dag_fastspeech2.py:194-243) through the HIP decode ops, viterbi /
        jointviterbi (:244-304) on the dense-window alignment kernels."""
        logits, links, feats = self.decode_graph(prev_output_tokens, enc)
        out_len = prev_output_tokens.ne(self.pad).sum(-1)
        if self.args.decode_strategy in ("viterbi", "jointviterbi"):
            toks, ofeat, mask, lens = decode_ops.viterbi_decode(
                logits, links, feats, out_len, self.pad, self.args.decode_beta, getattr(self.args, "decode_viterbibeta", 1.0),
                self.args.decode_strategy == "jointviterbi", self.args.src_upsample_scale)
            return {"output_tokens": toks, "features": ofeat, "features_padding_mask": mask, "feature_lengths": lens}
        toks, ofeat, mask, lens = decode_ops.graph_decode(logits, links, feats, out_len, self.pad, self.args.decode_beta,
                                                          self.args.decode_strategy)
        return {"output_tokens": toks, "features": ofeat, "features_padding_mask": mask, "feature_lengths": lens}


class S2SConformerDAGFastSpeech2Model(S2TConformerDAGModel):
    """registered name: s2s_conformer_dag_fastspeech2"""

    def __init__(self, **kw):
        tts_kw = kw.pop("tts", {})
        super().__init__(**kw)
        a = self.args
        tts_kw = {"dropout": a.dropout, "attention_dropout": a.attention_dropout, **tts_kw}                 # one args namespace in the reference
        self.tts = FastSpeech2NoEmb(**tts_kw)
        self.adaptor = FFNAdapter(a.decoder_embed_dim, a.adaptor_ffn_dim, self.tts.args.embed_dim, a.dropout)  # s2s_conformer_dag_fastspeech2.py:71-76
