"""torch float64 restatement of the relative-position attention training operator (include/daspeech_decode.h: dsp_relpos_attention_train_fwd /
_bwd) with an explicit keep mask: the forward (o, lse) and all six gradients by the operator's own formulas (an index gather for the
relative shift, no autograd), the module's training lines (rel_shift formulation, any dtype, the yardstick of the GPU tests), and the
padded-pitch mask index rule.  Shared by tests/test_relpos_train_ref.py (CPU: pins this file to torch float64 autograd of the module's lines)
and tests/test_gpu_relpos_train.py (GPU: the kernels against it)."""
import math

import torch
import torch.nn.functional as F

from tests import util_resnorm_ref as R

DK = 64
MAX_T = 2048                 # DSP_RELPOS_TRAIN_MAX_T


def padded(T):
    return (T + 3) // 4 * 4


def keep_mask(seed, offset, p, B, H, T):
    """bool [B,H,T,T]: element e = ((b*H + h)*T + i)*Tp + j of the residual operator's mask rule, Tp = T rounded up to a multiple of 4"""
    Tp = padded(T)
    return torch.from_numpy(R.keep_mask(seed, offset, p, B * H * T * Tp).reshape(B, H, T, Tp)[..., :T].copy())


def rel_shift(x):
    """the module's pad / view / slice / reshape ([B,h,T,2T-1] -> [B,h,T,T])"""
    B, h, T, P = x.shape
    x = F.pad(x, (1, 0)).view(B, h, P + 1, T)[:, :, 1:].reshape(B, h, T, P)
    return x[..., : P // 2 + 1]


def module_lines(q, k, v, pos, bias_u, bias_v, pad_mask, H, keep=None, p=0.0):
    """RelPosSelfAttention's training lines between the projections and linear_out, in the dtype of the arguments, with an explicit keep mask in
    place of F.dropout.  q, k, v [B,T,C], pos [2T-1,C], bias_u / bias_v [H,64], pad_mask [B,T] bool or None.  Returns (o [B,T,C], lse [B,H,T])."""
    B, T, C = q.shape
    dk = C // H
    qh = q.view(B, T, H, dk)
    kh, vh = k.view(B, T, H, dk).transpose(1, 2), v.view(B, T, H, dk).transpose(1, 2)
    ph = pos.view(1, -1, H, dk).transpose(1, 2)
    ac = torch.matmul((qh + bias_u.to(q.dtype)).transpose(1, 2), kh.transpose(-2, -1))
    bd = rel_shift(torch.matmul((qh + bias_v.to(q.dtype)).transpose(1, 2), ph.transpose(-2, -1)))
    scores = (ac + bd) / math.sqrt(dk)
    if pad_mask is not None:
        scores = scores.masked_fill(pad_mask.view(B, 1, 1, T), float("-inf"))
    att = torch.softmax(scores, dim=-1)
    if keep is not None:
        att = torch.where(keep, att / (1.0 - p), torch.zeros_like(att))
    o = torch.matmul(att, vh).transpose(1, 2).reshape(B, T, C)
    return o, torch.logsumexp(scores.float() if scores.dtype != torch.float64 else scores, dim=-1)


def _shift_index(T):
    i = torch.arange(T).view(T, 1)
    j = torch.arange(T).view(1, T)
    return T - 1 - i + j                                                    # [T,T] position row of (query i, key j)


def forward(q, k, v, pos, bias_u, bias_v, pad_mask, H, keep=None, p=0.0):
    """float64.  Returns dict(o [B,T,C], lse [B,H,T], P [B,H,T,T])."""
    B, T, C = q.shape
    qh = q.view(B, T, H, DK).permute(0, 2, 1, 3)                            # [B,H,T,64]
    kh = k.view(B, T, H, DK).permute(0, 2, 1, 3)
    vh = v.view(B, T, H, DK).permute(0, 2, 1, 3)
    ph = pos.view(2 * T - 1, H, DK).permute(1, 0, 2)                        # [H,2T-1,64]
    ac = torch.einsum("bhid,bhjd->bhij", qh + bias_u.view(1, H, 1, DK), kh)
    G = torch.einsum("bhid,hrd->bhir", qh + bias_v.view(1, H, 1, DK), ph)
    bd = torch.gather(G, 3, _shift_index(T).expand(B, H, T, T))
    s = (ac + bd) / 8.0
    if pad_mask is not None:
        s = s.masked_fill(pad_mask.view(B, 1, 1, T), float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    P = torch.exp(s - lse.unsqueeze(-1))
    A = P if keep is None else torch.where(keep, P / (1.0 - p), torch.zeros_like(P))
    o = torch.einsum("bhij,bhjd->bihd", A, vh).reshape(B, T, C)
    return dict(o=o, lse=lse, P=P)


def backward(q, k, v, pos, bias_u, bias_v, pad_mask, H, do, keep=None, p=0.0):
    """float64, by the formulas of the header.  Returns dict(dq, dk, dv, dpos, du, dv_bias)."""
    B, T, C = q.shape
    f = forward(q, k, v, pos, bias_u, bias_v, pad_mask, H, keep, p)
    P = f["P"]
    m = torch.ones_like(P) if keep is None else keep.to(P.dtype) / (1.0 - p)
    qh = q.view(B, T, H, DK).permute(0, 2, 1, 3)
    kh = k.view(B, T, H, DK).permute(0, 2, 1, 3)
    vh = v.view(B, T, H, DK).permute(0, 2, 1, 3)
    ph = pos.view(2 * T - 1, H, DK).permute(1, 0, 2)
    doh = do.view(B, T, H, DK).permute(0, 2, 1, 3)
    oh = f["o"].view(B, T, H, DK).permute(0, 2, 1, 3)
    D = (doh * oh).sum(-1, keepdim=True)
    dV = torch.einsum("bhij,bhid->bhjd", P * m, doh)
    dP = torch.einsum("bhid,bhjd->bhij", doh, vh) * m
    dS = P * (dP - D) / 8.0
    dQac = torch.einsum("bhij,bhjd->bhid", dS, kh)
    dK = torch.einsum("bhij,bhid->bhjd", dS, qh + bias_u.view(1, H, 1, DK))
    dG = torch.zeros(B, H, T, 2 * T - 1, dtype=P.dtype)
    dG.scatter_(3, _shift_index(T).expand(B, H, T, T), dS)
    dQbd = torch.einsum("bhir,hrd->bhid", dG, ph)
    dPos = torch.einsum("bhir,bhid->rhd", dG, qh + bias_v.view(1, H, 1, DK))
    back = lambda t: t.permute(0, 2, 1, 3).reshape(B, T, C)
    return dict(dq=back(dQac + dQbd), dk=back(dK), dv=back(dV), dpos=dPos.reshape(2 * T - 1, C), du=dQac.sum((0, 2)), dv_bias=dQbd.sum((0, 2)))


def pad_masks(kind, B, T):
    """None, a ragged mask, or one whose last sample has a single valid key (bool [B,T], True = padding)"""
    if kind == "none":
        return None
    if kind == "ragged":
        lens = [max(1, T - (2 * b + 1) * max(1, T // 5)) if b else T for b in range(B)]
        if B == 1:
            lens = [max(1, T - max(1, T // 3))]
    else:
        lens = [T] * (B - 1) + [1]
    return torch.arange(T).unsqueeze(0) >= torch.tensor(lens).unsqueeze(1)


def inputs(seed, B, T, H):
    """float64 test data at the scale of the layer's projections, and a cotangent"""
    g = torch.Generator().manual_seed(seed)
    C = H * DK
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    return dict(q=rn(B, T, C), k=rn(B, T, C), v=rn(B, T, C), pos=rn(2 * T - 1, C), bias_u=0.5 * rn(H, DK), bias_v=0.5 * rn(H, DK), do=rn(B, T, C))
