"""numpy float64 restatement of the residual + dropout + LayerNorm operator (include/daspeech_decode.h: dsp_resnorm_train_fwd / _bwd) with an
explicit keep mask, and a numpy Philox4x32-10 with the operator's mask rule.  Shared by tests/test_resnorm_ref.py (CPU: pins this file to
torch float64 autograd and to the published Philox known answers) and tests/test_gpu_resnorm_autograd.py (GPU: the kernels against it)."""
import math

import numpy as np

CHUNK_ROWS = 32              # DSP_RESNORM_CHUNK_ROWS
MAX_C = 2048

_M0, _M1 = 0xD2511F53, 0xCD9E8D57
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints) of one shape, key: two ints -> four uint32 arrays.  Salmon et al., SC'11."""
    c = [np.asarray(x, dtype=np.uint64) & _MASK32 for x in counter]
    k0, k1 = int(key[0]) & _MASK32, int(key[1]) & _MASK32
    for _ in range(10):
        p0 = np.uint64(_M0) * c[0]
        p1 = np.uint64(_M1) * c[2]
        h0, l0 = p0 >> np.uint64(32), p0 & np.uint64(_MASK32)
        h1, l1 = p1 >> np.uint64(32), p1 & np.uint64(_MASK32)
        c = [h1 ^ c[1] ^ np.uint64(k0), l1, h0 ^ c[3] ^ np.uint64(k1), l0]
        k0, k1 = (k0 + _W0) & _MASK32, (k1 + _W1) & _MASK32
    return [x.astype(np.uint32) for x in c]


def threshold(p):
    """thr = ceil(p * 2^24) in double"""
    return int(math.ceil(float(p) * 16777216.0))


def keep_mask(seed, offset, p, n):
    """bool [n]: element e is kept when word (e & 3) of Philox(counter = (g lo, g hi, offset lo, offset hi), key = (seed lo, seed hi)), g = e >> 2,
    has (word >> 8) >= thr"""
    thr = threshold(p)
    g = np.arange((n + 3) // 4, dtype=np.uint64)
    off = int(offset)
    shape = g.shape
    words = philox4x32_10((g & np.uint64(_MASK32), g >> np.uint64(32), np.full(shape, off & _MASK32, dtype=np.uint64),
                           np.full(shape, (off >> 32) & _MASK32, dtype=np.uint64)), (int(seed) & _MASK32, (int(seed) >> 32) & _MASK32))
    w = np.stack(words, axis=1).reshape(-1)[:n]
    return (w >> np.uint32(8)).astype(np.int64) >= thr


def forward(h, residual, bias, gamma, beta, eps, alpha, p, keep, round_s=None):
    """float64 arrays [R,C] / [C]; h None: s = residual.  keep: bool [R,C] or None (no dropout).  round_s: the rounding of s to the data dtype
    (a callable on a float64 array) — the statistics are those of the rounded s.  Returns dict(s, y, mean, rstd)."""
    if h is None:
        s = residual.copy()
    else:
        z = h + (0.0 if bias is None else bias)
        d = z if keep is None else np.where(keep, z / (1.0 - p), 0.0)
        s = residual + alpha * d
        if round_s is not None:
            s = round_s(s)
    mean = s.mean(axis=1, keepdims=True)
    var = ((s - mean) ** 2).mean(axis=1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    y = gamma * ((s - mean) * rstd) + beta
    return dict(s=s, y=y, mean=mean[:, 0], rstd=rstd[:, 0])


def backward(s, gamma, eps, alpha, p, keep, dy, ds, has_h=True):
    """gradients from dy and / or ds (None: zero) at the stored s.  Returns dict(dresidual, dh, dbias, dgamma, dbeta)."""
    mean = s.mean(axis=1, keepdims=True)
    var = ((s - mean) ** 2).mean(axis=1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    xh = (s - mean) * rstd
    dyv = np.zeros_like(s) if dy is None else dy
    dxh = dyv * gamma
    g = rstd * (dxh - dxh.mean(axis=1, keepdims=True) - xh * (dxh * xh).mean(axis=1, keepdims=True))
    if ds is not None:
        g = g + ds
    out = dict(dresidual=g, dgamma=(dyv * xh).sum(axis=0), dbeta=dyv.sum(axis=0))
    if has_h:
        dh = alpha * g if keep is None else np.where(keep, alpha * g / (1.0 - p), 0.0)
        out.update(dh=dh, dbias=dh.sum(axis=0))
    return out


def inputs(seed, R, C):
    """float64 test data: a residual with a row offset (mean far from 0), h, bias, gamma around 1, beta, two cotangents"""
    rng = np.random.default_rng(seed)
    res = rng.standard_normal((R, C)) + rng.standard_normal((R, 1)) * 2.0
    h = rng.standard_normal((R, C)) * 1.5
    bias = rng.standard_normal(C) * 0.3
    gamma = 1.0 + 0.25 * rng.standard_normal(C)
    beta = 0.2 * rng.standard_normal(C)
    dy = rng.standard_normal((R, C))
    ds = rng.standard_normal((R, C)) * 0.7
    return dict(residual=res, h=h, bias=bias, gamma=gamma, beta=beta, dy=dy, ds=ds)
