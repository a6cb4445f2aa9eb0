"""torch float64 restatement of the stride-2 channels-last Conv1d training operator (include/daspeech_decode.h: dsp_conv1d_s2_train_fwd / _bwd) by
its four formulas, with explicit strided slices — no F.conv1d, no autograd.  T_out = (T - 1) // 2 + 1, P = (K - 1) / 2, rows outside [0, T) of a
sample count as zeros:
    y [b,t,co]  = [bias[co] +] sum_k sum_ci x[b, 2t+k-P, ci] W[co,ci,k]                                  t in [0, T_out)
    dx[b,u,ci]  = sum_{k : (u+P-k) even, 0 <= (u+P-k)/2 < T_out} sum_co dy[b, (u+P-k)/2, co] W[co,ci,k]
    dW[co,ci,k] = sum_b sum_t  dy[b,t,co] x[b, 2t+k-P, ci]
    db[co]      = sum_b sum_t  dy[b,t,co]
Shared by tests/test_conv1d_stride2_ref.py (CPU: pins this file to float64 autograd of F.conv1d(stride=2) on the transposed tensors) and
tests/test_gpu_conv1d_stride2.py (GPU: the kernels against it)."""
import torch
import torch.nn.functional as F

ROW_TILE = 64                # DSP_CONV1D_TRAIN_ROW_TILE
WGRAD_ROWS = 1024            # DSP_CONV1D_TRAIN_WGRAD_ROWS
MAX_K = 15                   # DSP_CONV1D_TRAIN_MAX_K
MAX_C = 8192                 # DSP_CONV1D_TRAIN_MAX_C


def t_out(T):
    return (T - 1) // 2 + 1


def inputs(seed, B, T, Cin, Cout, K):
    """x, W, bias, dy in float64; W scaled so that y is of order 1"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    return dict(x=r(B, T, Cin), w=r(Cout, Cin, K) / (Cin * K) ** 0.5, bias=r(Cout), dy=r(B, t_out(T), Cout))


def taps(T, K):
    """(k, lo, hi) per tap that lands inside a sample: output rows lo .. hi-1 read input rows 2 lo + k - P, 2 (lo + 1) + k - P, ...; for the
    other output rows, and for the taps not listed, the tap is padding"""
    P = (K - 1) // 2
    for k in range(K):
        s = k - P
        lo = max(0, (-s + 1) // 2)                      # the first t with 2t + s >= 0
        hi = min(t_out(T), (T - 1 - s) // 2 + 1)        # one past the last t with 2t + s <= T - 1
        if lo < hi:
            yield k, lo, hi


def _rows(k, lo, hi, K):
    """the slice of input rows that output rows lo .. hi-1 read through tap k"""
    s = k - (K - 1) // 2
    return slice(2 * lo + s, 2 * (hi - 1) + s + 1, 2)


def forward(x, w, bias=None):
    B, T, Cin = x.shape
    Cout, _, K = w.shape
    y = torch.zeros(B, t_out(T), Cout, dtype=x.dtype)
    for k, lo, hi in taps(T, K):
        y[:, lo:hi] += x[:, _rows(k, lo, hi, K)] @ w[:, :, k].t()
    return y if bias is None else y + bias


def backward(x, w, dy):
    """dx, dw, db of the formulas above"""
    B, T, Cin = x.shape
    Cout, _, K = w.shape
    dx = torch.zeros_like(x)
    dw = torch.zeros_like(w)
    for k, lo, hi in taps(T, K):
        dx[:, _rows(k, lo, hi, K)] += dy[:, lo:hi] @ w[:, :, k]
        dw[:, :, k] = torch.einsum("bto,bti->oi", dy[:, lo:hi], x[:, _rows(k, lo, hi, K)])
    return dict(dx=dx, dw=dw, db=dy.sum(dim=(0, 1)))


def torch_lines(x, w, bias, dy):
    """the lines the operator replaces, in the dtype of the arguments, under autograd: transpose -> F.conv1d(stride=2) -> transpose.  Returns y
    and the gradients (db None without a bias)."""
    leaves = [t.detach().clone().requires_grad_() for t in (x, w)] + ([] if bias is None else [bias.detach().clone().requires_grad_()])
    K = w.shape[2]
    y = F.conv1d(leaves[0].transpose(1, 2), leaves[1], None if bias is None else leaves[2], stride=2, padding=(K - 1) // 2).transpose(1, 2)
    grads = torch.autograd.grad(y, leaves, dy)
    out = dict(y=y.detach(), dx=grads[0], dw=grads[1])
    if bias is not None:
        out["db"] = grads[2]
    return out
