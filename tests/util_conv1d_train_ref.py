"""torch float64 restatement of the channels-last Conv1d training operator (include/daspeech_decode.h: dsp_conv1d_train_fwd / _bwd) by its four
formulas, with explicit shifted slices — no F.conv1d, no autograd:
    y [b,t,co]  = [bias[co] +] sum_k sum_ci x[b, t+k-P, ci] W[co,ci,k]           P = (K-1)/2, rows outside [0, T) of a sample count as zeros
    dx[b,t,ci]  = sum_k sum_co dy[b, t-k+P, co] W[co,ci,k]
    dW[co,ci,k] = sum_b sum_t  dy[b,t,co] x[b, t+k-P, ci]
    db[co]      = sum_b sum_t  dy[b,t,co]
Shared by tests/test_conv1d_train_ref.py (CPU: pins this file to float64 autograd of F.conv1d on the transposed tensors) and
tests/test_gpu_conv1d_train.py (GPU: the kernels against it)."""
import torch
import torch.nn.functional as F

ROW_TILE = 64                # DSP_CONV1D_TRAIN_ROW_TILE
WGRAD_ROWS = 1024            # DSP_CONV1D_TRAIN_WGRAD_ROWS
MAX_K = 15                   # DSP_CONV1D_TRAIN_MAX_K
MAX_C = 8192                 # DSP_CONV1D_TRAIN_MAX_C


def inputs(seed, B, T, Cin, Cout, K):
    """x, W, bias, dy in float64; W scaled so that y is of order 1"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    return dict(x=r(B, T, Cin), w=r(Cout, Cin, K) / (Cin * K) ** 0.5, bias=r(Cout), dy=r(B, T, Cout))


def _taps(T, K):
    """(k, lo, hi, shift) per tap: output rows lo .. hi-1 read input rows lo+shift .. hi-1+shift, shift = k - P; the rest of the tap is padding"""
    P = (K - 1) // 2
    for k in range(K):
        s = k - P
        lo, hi = max(0, -s), min(T, T - s)
        if lo < hi:
            yield k, lo, hi, s


def forward(x, w, bias=None):
    B, T, Cin = x.shape
    Cout, _, K = w.shape
    y = torch.zeros(B, T, Cout, dtype=x.dtype)
    for k, lo, hi, s in _taps(T, K):
        y[:, lo:hi] += x[:, lo + s:hi + s] @ w[:, :, k].t()
    return y if bias is None else y + bias


def backward(x, w, dy):
    """dx, dw, db of the formulas above"""
    B, T, Cin = x.shape
    Cout, _, K = w.shape
    dx = torch.zeros_like(x)
    dw = torch.zeros_like(w)
    for k, lo, hi, s in _taps(T, K):
        dx[:, lo + s:hi + s] += dy[:, lo:hi] @ w[:, :, k]
        dw[:, :, k] = torch.einsum("bto,bti->oi", dy[:, lo:hi], x[:, lo + s:hi + s])
    return dict(dx=dx, dw=dw, db=dy.sum(dim=(0, 1)))


def torch_lines(x, w, bias, dy):
    """the lines the operator replaces, in the dtype of the arguments, under autograd: transpose -> F.conv1d -> transpose.  Returns y and the
    gradients (db None without a bias)."""
    leaves = [t.detach().clone().requires_grad_() for t in (x, w)] + ([] if bias is None else [bias.detach().clone().requires_grad_()])
    K = w.shape[2]
    y = F.conv1d(leaves[0].transpose(1, 2), leaves[1], None if bias is None else leaves[2], padding=(K - 1) // 2).transpose(1, 2)
    grads = torch.autograd.grad(y, leaves, dy)
    out = dict(y=y.detach(), dx=grads[0], dw=grads[1])
    if bias is not None:
        out["db"] = grads[2]
    return out
