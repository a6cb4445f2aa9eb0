"""The HiFi-GAN layer exactly as include/daspeech_hifigan.h defines it, in plain torch: a sum over taps of shifted matmuls (no conv
call, so it is the definition and not another convolution implementation).  dtype and device are those of the inputs: fp64 tensors
give the reference, fp32 tensors the plain fp32 evaluation the GPU tests measure accumulation error against.

    v[b,t,m] = sum_k  w[k,m,:] . lrelu(x[b, t+shifts[k], :])          rows < 0 or >= valid_len(b) read as 0
    STORE     out[t][co]            = scale * (v + bias + res)          Tout == T, Cout == M
    ACCUM     out[t][co]           += scale * (v + bias + res)
    UPSAMPLE  out[q*u + r - pad][co] = scale * (v[q][(r, co)] + bias[co] + res),   q = 0..T, M = u * Cout phase-major rows (r, co)

valid_len(b) = min(T, lens[b] * len_mul) (T without lens).  Output rows at or past an utterance's valid length (times u for UPSAMPLE)
are unspecified for the layers (the kernels skip whole tiles there): compare rows below it only.  ref_post writes zeros there.
"""
import torch

OUT_STORE, OUT_ACCUM, OUT_UPSAMPLE = 0, 1, 2


def lrelu(x, slope):
    return torch.where(x > 0, x, x * slope)


def valid_lens(B, T, lens=None, len_mul=1):
    if lens is None:
        return [T] * B
    return [min(T, int(n) * len_mul) for n in (lens.tolist() if hasattr(lens, "tolist") else lens)]


def _masked(x, lens, len_mul):
    B, T, _ = x.shape
    if lens is None:
        return x
    vl = torch.tensor(valid_lens(B, T, lens, len_mul), device=x.device)
    return x * (torch.arange(T, device=x.device)[None, :, None] < vl[:, None, None]).to(x.dtype)


def _layer(x, w, bias, res, out_prev, shifts, pre_slope, scale, out_mode, up_u, up_pad, Tout, Cout, lens, len_mul, absolute):
    B, T, CI = x.shape
    ntaps, M, _ = w.shape
    assert len(shifts) == ntaps and w.shape[2] == CI
    mag = (lambda t: t.abs()) if absolute else (lambda t: t)
    a = _masked(mag(lrelu(x, pre_slope)), lens, len_mul)
    ncol = T + 1 if out_mode == OUT_UPSAMPLE else T
    P = max(max(abs(s) for s in shifts), 1)
    ap = a.new_zeros(B, T + 2 * P + 1, CI)
    ap[:, P:P + T] = a
    v = a.new_zeros(B, ncol, M)
    for k, s in enumerate(shifts):
        v = v + ap[:, P + s:P + s + ncol] @ mag(w[k]).transpose(0, 1)
    if out_mode == OUT_UPSAMPLE:
        assert M == up_u * Cout
        # column q, row (r, co) -> time q*u + r - pad: the [B, ncol, u, Cout] view IS time-major from time -pad on
        v = v.reshape(B, ncol * up_u, Cout)[:, up_pad:up_pad + Tout]
        assert v.shape[1] == Tout, "Tout must not exceed (T + 1) * u - pad"
    else:
        assert M == Cout and Tout == T
    if bias is not None:
        v = v + mag(bias)
    if res is not None:
        v = v + mag(res)
    v = v * abs(scale) if absolute else v * scale
    if out_mode == OUT_ACCUM:
        v = v + mag(out_prev)
    return v


def ref_layer(x, w, bias, res, out_prev, shifts, pre_slope, scale, out_mode, up_u, up_pad, Tout, Cout, lens=None, len_mul=1):
    """x [B,T,CI], w [ntaps,M,CI] tap-major, bias [Cout] / res [B,Tout,Cout] / out_prev [B,Tout,Cout] or None -> out [B,Tout,Cout]."""
    return _layer(x, w, bias, res, out_prev, shifts, pre_slope, scale, out_mode, up_u, up_pad, Tout, Cout, lens, len_mul, False)


def ref_abs_layer(x, w, bias, res, out_prev, shifts, pre_slope, scale, out_mode, up_u, up_pad, Tout, Cout, lens=None, len_mul=1):
    """The same sums over |w|, |lrelu(x)|, |bias|, |res| (|out_prev| for ACCUM): the magnitude A every rounding error of the layer is
    proportional to."""
    return _layer(x, w, bias, res, out_prev, shifts, pre_slope, scale, out_mode, up_u, up_pad, Tout, Cout, lens, len_mul, True)


def conv_shifts(ntaps, dil):
    return [(k - (ntaps - 1) // 2) * dil for k in range(ntaps)]


def ref_unit(x, w1, b1, w2, b2, ntaps, dil, slope, scale, accumulate=False, out_prev=None, lens=None, len_mul=1, mid_round=None):
    """One ResBlock1 unit: out = scale * (x + b2 + c2(lrelu(b1 + c1(lrelu(x))))) [+ out_prev]; c1 dilation dil, c2 dilation 1, the
    intermediate zero outside [0, valid_len) (c2's zero padding).  mid_round: rounding of the intermediate where the hardware path
    stores it narrower (fp16 storage), e.g. lambda h: h.half().to(h.dtype)."""
    B, T, C = x.shape
    h = ref_layer(x, w1, b1, None, None, conv_shifts(ntaps, dil), slope, 1.0, OUT_STORE, 1, 0, T, C, lens, len_mul)
    if mid_round is not None:
        h = mid_round(h)
    return ref_layer(h, w2, b2, x, out_prev if accumulate else None, conv_shifts(ntaps, 1), slope, scale,
                     OUT_ACCUM if accumulate else OUT_STORE, 1, 0, T, C, lens, len_mul)


def _post_sum(x, w, slope, lens, len_mul, absolute):
    K, C = w.shape
    T = x.shape[1]
    return _layer(x, w.reshape(K, 1, C), None, None, None, conv_shifts(K, 1), slope, 1.0, OUT_STORE, 1, 0, T, 1, lens, len_mul, absolute)[..., 0]


def ref_post(x, w, bias, slope, lens=None, len_mul=1, pre_tanh=False):
    """conv_post: wav[b][t] = tanh(bias + sum_{k,c} w[k][c] * lrelu(x[b][t + k - (K-1)/2][c])), zeros at and past the valid length.
    x [B,T,C], w [K,C], bias a float -> [B,T].  pre_tanh=True returns (the sum before tanh, the same sum over magnitudes) instead."""
    live = _masked(x.new_ones(x.shape[0], x.shape[1], 1), lens, len_mul)[..., 0]
    s = (_post_sum(x, w, slope, lens, len_mul, False) + bias) * live
    if pre_tanh:
        return s, (_post_sum(x, w, slope, lens, len_mul, True) + abs(bias)) * live
    return torch.tanh(s) * live
