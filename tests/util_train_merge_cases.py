"""The cases of tests/test_gpu_train_merge_parent.py and of its recorder tests/golden/make_train_merge_parent.py: the parameter gradients whose
last step is a fixed-order merge of fp32 partials (csrc/partial_merge.h), at the smallest shapes that reach every branch of those tails.

Inputs are drawn on the CPU from a seeded generator, so they are the same bits on every machine; p = 0, training mode.  run(name) returns
{gradient name: tensor}; the fixture holds them under "<case>/<gradient>".

    actdrop / resnorm, R = 4133, C = 72   130 chunks of 32 rows: one full LDS tile of 128 chunks, a second tile of 2, a last chunk of 5 rows;
                                          a column block of 64 and a ragged one of 8 (resnorm: 3 * 72 = 216 columns, three blocks and 24)
    actdrop / resnorm, R = 37             2 chunks, one tile
    conv1d 2 x 600                        1200 rows: 2 weight-gradient splits of 1024, 5 bias chunks of 256, the last ragged
    conv1d 1 x 8                          one split, one chunk
    conv1d stride 2, 2 x 1201             601 output rows a sample
    convmod 2 x 100, C = 72, K = 7        2 chunks
    relpos 3 x 40, one head               dpos over 3 samples, dbias_u / dbias_v over 2 row chunks a sample
"""
import torch

F16, F32 = torch.float16, torch.float32


def _draw(gen, shape, dtype, scale=0.5):
    return (torch.randn(shape, generator=gen, dtype=torch.float32) * scale).to(dtype)


def _actdrop(R):
    def run(dev):
        from daspeech_amd import decode_ops as D
        g = torch.Generator().manual_seed(1000 + R)
        h = _draw(g, (R, 72), F16).to(dev)
        bias = _draw(g, (72,), F32).to(dev).requires_grad_()
        gy = _draw(g, (R, 72), F16).to(dev)
        y = D.bias_act_dropout_autograd(h, bias, "gelu", p=0.0, training=True)
        (db,) = torch.autograd.grad(y, [bias], gy)
        return {"dbias": db}
    return run


def _resnorm(R):
    def run(dev):
        from daspeech_amd import decode_ops as D
        g = torch.Generator().manual_seed(2000 + R)
        h = _draw(g, (R, 72), F16).to(dev)
        res = _draw(g, (R, 72), F16).to(dev)
        bias = _draw(g, (72,), F32).to(dev).requires_grad_()
        ln = torch.nn.LayerNorm(72).to(dev)
        with torch.no_grad():
            ln.weight.copy_(1.0 + _draw(g, (72,), F32, 0.25).to(dev))
            ln.bias.copy_(_draw(g, (72,), F32).to(dev))
        gs, gy = _draw(g, (R, 72), F16).to(dev), _draw(g, (R, 72), F16).to(dev)
        s, y = D.residual_dropout_layer_norm_autograd(h, res, ln, bias=bias, p=0.0, training=True)
        db, dg, dbt = torch.autograd.grad([s, y], [bias, ln.weight, ln.bias], [gs, gy])
        return {"dbias": db, "dgamma": dg, "dbeta": dbt}
    return run


def _conv(op, B, T, Cin, Cout, K):
    def run(dev):
        from daspeech_amd import decode_ops as D
        g = torch.Generator().manual_seed(3000 + 7 * T + K)
        x = _draw(g, (B, T, Cin), F16).to(dev)
        w = _draw(g, (Cout, Cin, K), F16, 0.1).to(dev).requires_grad_()
        bias = _draw(g, (Cout,), F32).to(dev).requires_grad_()
        y = getattr(D, op)(x, w, bias)
        gy = _draw(g, tuple(y.shape), F16).to(dev)
        dw, db = torch.autograd.grad(y, [w, bias], gy)
        return {"dw": dw, "db": db}
    return run


def _convmod(dev):
    from daspeech_amd import decode_ops as D
    g = torch.Generator().manual_seed(4000)
    B, T, C, K = 2, 100, 72, 7
    x = _draw(g, (B, T, C), F16).to(dev)
    w = _draw(g, (C, 1, K), F16).to(dev).requires_grad_()
    bn = torch.nn.BatchNorm1d(C).to(dev).train()
    with torch.no_grad():
        bn.weight.copy_(1.0 + _draw(g, (C,), F32, 0.25).to(dev))
        bn.bias.copy_(_draw(g, (C,), F32).to(dev))
    gy = _draw(g, (B, T, C), F16).to(dev)
    y = D.dwconv_bn_silu_autograd(x, w, bn)
    dw, dg, db = torch.autograd.grad(y, [w, bn.weight, bn.bias], gy)
    return {"dw": dw, "dgamma": dg, "dbeta": db}


def _relpos(dev):
    from daspeech_amd import decode_ops as D
    g = torch.Generator().manual_seed(5000)
    B, T, C = 3, 40, 64
    q, k, v = (_draw(g, (B, T, C), F16).to(dev) for _ in range(3))
    pos = _draw(g, (2 * T - 1, C), F16).to(dev).requires_grad_()
    bu, bv = (_draw(g, (1, C), F32).to(dev).requires_grad_() for _ in range(2))
    go = _draw(g, (B, T, C), F16).to(dev)
    o = D.relpos_attention_autograd(q, k, v, pos, bu, bv, None, 1, p=0.0, training=True)
    dpos, du, dv = torch.autograd.grad(o, [pos, bu, bv], go)
    return {"dpos": dpos, "dbias_u": du, "dbias_v": dv}


CASES = {
    "actdrop_gelu_R4133": _actdrop(4133),
    "actdrop_gelu_R37": _actdrop(37),
    "resnorm_bias_R4133": _resnorm(4133),
    "resnorm_bias_R37": _resnorm(37),
    "conv1d_2x600": _conv("conv1d_channels_last_autograd", 2, 600, 64, 64, 3),
    "conv1d_1x8": _conv("conv1d_channels_last_autograd", 1, 8, 64, 64, 3),
    "conv1d_s2_2x1201": _conv("conv1d_stride2_channels_last_autograd", 2, 1201, 16, 64, 5),
    "convmod_2x100": _convmod,
    "relpos_3x40": _relpos,
}


def run(name, dev="cuda:0"):
    out = CASES[name](torch.device(dev))
    torch.cuda.synchronize()
    return out
