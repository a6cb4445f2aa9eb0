"""torch float64 restatement of the bias + activation + dropout operator (include/daspeech_decode.h: dsp_act_dropout_train_fwd / _bwd) with an
explicit keep mask: the forward and both gradients by the operator's own formulas (no autograd), and the torch lines the operator replaces (any
dtype, the yardstick of the GPU tests).  Shared by tests/test_actdrop_ref.py (CPU: pins this file to torch float64 autograd of the torch
lines) and tests/test_gpu_actdrop_autograd.py (GPU: the kernels against it)."""
import math

import torch
import torch.nn.functional as F

ACTS = ("identity", "relu", "silu", "gelu", "glu")
CHUNK_ROWS = 32              # DSP_ACTDROP_CHUNK_ROWS
MAX_CIN = 8192               # DSP_ACTDROP_MAX_CIN


def out_width(act, Cin):
    return Cin // 2 if act == "glu" else Cin


def _sigmoid(u):
    return 1.0 / (1.0 + torch.exp(-u))


def _Phi(u):
    return 0.5 * (1.0 + torch.erf(u / math.sqrt(2.0)))


def _phi(u):
    return torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)


def _m(keep, p, like):
    """keep * keep_scale as float64 ([R,Cout]); ones without a mask"""
    if keep is None:
        return torch.ones_like(like)
    return keep.to(torch.float64) / (1.0 - p)


def forward(h, bias, act, keep=None, p=0.0):
    """y [R,Cout] float64 from h [R,Cin], bias [Cin] or None, keep [R,Cout] bool or None"""
    u = h.to(torch.float64)
    if bias is not None:
        u = u + bias.to(torch.float64)
    if act == "glu":
        C = u.shape[-1] // 2
        a = u[..., :C] * _sigmoid(u[..., C:])
    elif act == "identity":
        a = u
    elif act == "relu":
        a = torch.where(u > 0, u, torch.zeros_like(u))
    elif act == "silu":
        a = u * _sigmoid(u)
    elif act == "gelu":
        a = u * _Phi(u)
    else:
        raise ValueError(act)
    return a * _m(keep, p, a)


def backward(h, bias, act, dy, keep=None, p=0.0):
    """(dh [R,Cin], dbias [Cin]) float64 by the header's formulas"""
    u = h.to(torch.float64)
    if bias is not None:
        u = u + bias.to(torch.float64)
    d = dy.to(torch.float64)
    d = d * _m(keep, p, d)
    if act == "glu":
        C = u.shape[-1] // 2
        a, s = u[..., :C], _sigmoid(u[..., C:])
        dh = torch.cat([d * s, d * a * s * (1.0 - s)], dim=-1)
    elif act == "identity":
        dh = d
    elif act == "relu":
        dh = d * (u > 0).to(torch.float64)
    elif act == "silu":
        s = _sigmoid(u)
        dh = d * s * (1.0 + u * (1.0 - s))
    elif act == "gelu":
        dh = d * (_Phi(u) + u * _phi(u))
    else:
        raise ValueError(act)
    return dh, dh.reshape(-1, dh.shape[-1]).sum(0)


def torch_lines(h, bias, act, keep=None, p=0.0):
    """the lines the operator replaces, in the dtype of the arguments, with an explicit keep mask in place of F.dropout (differentiable)"""
    u = h if bias is None else h + bias.to(h.dtype)
    a = {"identity": lambda t: t, "relu": F.relu, "silu": F.silu, "gelu": F.gelu, "glu": lambda t: F.glu(t, dim=-1)}[act](u)
    return a if keep is None else a * keep.to(a.dtype) / (1.0 - p)


def inputs(seed, R, Cin, act):
    """float64 h [R,Cin], bias [Cin], dy [R,Cout] with values on both sides of every activation's bend"""
    g = torch.Generator().manual_seed(seed)
    h = 2.0 * torch.randn(R, Cin, generator=g, dtype=torch.float64)
    bias = 0.5 * torch.randn(Cin, generator=g, dtype=torch.float64)
    dy = torch.randn(R, out_width(act, Cin), generator=g, dtype=torch.float64)
    return h, bias, dy
