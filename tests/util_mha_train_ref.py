"""torch float64 restatement of the multi-head attention training operator (include/daspeech_decode.h: dsp_mha_train_fwd / _bwd) with an
explicit keep mask: the forward (o, lse) and the three gradients by the operator's own formulas (no autograd), the modules' training lines as
explicit torch ops in any dtype (matmul, masked_fill, softmax, keep / (1 - p), matmul: the yardstick of the GPU tests — they take a given
mask, which F.scaled_dot_product_attention cannot), and the padded-pitch mask index rule.  Query length N and key length M are independent.
Shared by tests/test_mha_train_ref.py (CPU: pins this file to torch float64 autograd of those lines and to SDPA) and
tests/test_gpu_mha_train.py (GPU: the kernels against it)."""
import math

import torch

from tests import util_resnorm_ref as R

DK = 64
MAX_LEN = 4096               # DSP_MHA_TRAIN_MAX_LEN


def padded(M):
    return (M + 3) // 4 * 4


def keep_mask(seed, offset, p, B, H, N, M):
    """bool [B,H,N,M]: element e = ((b*H + h)*N + i)*Mp + j of the residual operator's mask rule, Mp = M rounded up to a multiple of 4"""
    Mp = padded(M)
    return torch.from_numpy(R.keep_mask(seed, offset, p, B * H * N * Mp).reshape(B, H, N, Mp)[..., :M].copy())


def module_lines(q, k, v, pad, H, keep=None, p=0.0):
    """the training lines of _MHA / _SelfAttention between the projections and out_proj, in the dtype of the arguments, with an explicit keep
    mask in place of SDPA's dropout.  q [B,N,C], k, v [B,M,C], pad [B,M] bool or None.  Returns (o [B,N,C], lse [B,H,N])."""
    B, N, C = q.shape
    M = k.shape[1]
    dk = C // H
    qh = q.view(B, N, H, dk).transpose(1, 2)
    kh = k.view(B, M, H, dk).transpose(1, 2)
    vh = v.view(B, M, H, dk).transpose(1, 2)
    scores = torch.matmul(qh, kh.transpose(-2, -1)) / math.sqrt(dk)
    if pad is not None:
        scores = scores.masked_fill(pad.view(B, 1, 1, M), float("-inf"))
    att = torch.softmax(scores, dim=-1)
    if keep is not None:
        att = torch.where(keep, att / (1.0 - p), torch.zeros_like(att))
    o = torch.matmul(att, vh).transpose(1, 2).reshape(B, N, C)
    return o, torch.logsumexp(scores.float() if scores.dtype != torch.float64 else scores, dim=-1)


def _heads(t, H):
    B, L, _ = t.shape
    return t.view(B, L, H, DK).permute(0, 2, 1, 3)                          # [B,H,L,64]


def forward(q, k, v, pad, H, keep=None, p=0.0):
    """float64.  Returns dict(o [B,N,C], lse [B,H,N], P [B,H,N,M])."""
    B, N, C = q.shape
    M = k.shape[1]
    s = torch.einsum("bhid,bhjd->bhij", _heads(q, H), _heads(k, H)) / 8.0
    if pad is not None:
        s = s.masked_fill(pad.view(B, 1, 1, M), float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    P = torch.exp(s - lse.unsqueeze(-1))
    A = P if keep is None else torch.where(keep, P / (1.0 - p), torch.zeros_like(P))
    o = torch.einsum("bhij,bhjd->bihd", A, _heads(v, H)).reshape(B, N, C)
    return dict(o=o, lse=lse, P=P)


def backward(q, k, v, pad, H, do, keep=None, p=0.0):
    """float64, by the formulas of the header.  Returns dict(dq [B,N,C], dk [B,M,C], dv [B,M,C])."""
    B, N, C = q.shape
    M = k.shape[1]
    f = forward(q, k, v, pad, H, keep, p)
    P = f["P"]
    m = torch.ones_like(P) if keep is None else keep.to(P.dtype) / (1.0 - p)
    qh, kh, vh, doh, oh = (_heads(t, H) for t in (q, k, v, do, f["o"]))
    D = (doh * oh).sum(-1, keepdim=True)
    dV = torch.einsum("bhij,bhid->bhjd", P * m, doh)
    dS = P * (torch.einsum("bhid,bhjd->bhij", doh, vh) * m - D) / 8.0
    dK = torch.einsum("bhij,bhid->bhjd", dS, qh)
    dQ = torch.einsum("bhij,bhjd->bhid", dS, kh)
    back = lambda t, L: t.permute(0, 2, 1, 3).reshape(B, L, C)
    return dict(dq=back(dQ, N), dk=back(dK, M), dv=back(dV, M))


def pad_masks(kind, B, M):
    """None, a ragged mask, or one whose last sample has a single valid key (bool [B,M], True = padding)"""
    if kind == "none":
        return None
    if kind == "ragged":
        lens = [max(1, M - (2 * b + 1) * max(1, M // 5)) if b else M for b in range(B)]
        if B == 1:
            lens = [max(1, M - max(1, M // 3))]
    else:
        lens = [M] * (B - 1) + [1]
    return torch.arange(M).unsqueeze(0) >= torch.tensor(lens).unsqueeze(1)


def inputs(seed, B, N, M, H):
    """float64 test data at the scale of the layers' projections, and a cotangent"""
    g = torch.Generator().manual_seed(seed)
    C = H * DK
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    return dict(q=rn(B, N, C), k=rn(B, M, C), v=rn(B, M, C), do=rn(B, N, C))
