"""CPU-side surface of the residual + dropout + LayerNorm operator under autograd (csrc/residual_norm_train.hip): the C symbols and the macro
are declared, bound and exported, the workspace question is host arithmetic with the stated properties, decode_ops refuses what it does not
serve before any device call, residual_dropout_layer_norm_served says no to each unserved condition, and the three layer classes in
training mode keep the torch lines, bit for bit, where the operator does not run (CPU tensors)."""
import copy
import os
import re

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["dsp_resnorm_train_fwd", "dsp_resnorm_train_bwd", "dsp_resnorm_train_workspace_bytes", "dsp_dropout_keep_mask"]


def test_new_symbols_are_declared_bound_and_exported():
    from daspeech_amd import _lib, build, decode_ops
    text = open(os.path.join(ROOT, "include", "daspeech_decode.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in include/daspeech_decode.h"
        assert name in _lib.SIGNATURES
    m = re.search(r"#define\s+DSP_RESNORM_CHUNK_ROWS\s+(\d+)", code)
    assert m and int(m.group(1)) == decode_ops.RESNORM_CHUNK_ROWS
    assert re.search(r"#define\s+DSP_ABI_VERSION\s+2\b", open(os.path.join(ROOT, "include", "daspeech_dag.h")).read())
    build.build()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name)
    for name in ("residual_dropout_layer_norm_autograd", "residual_dropout_layer_norm_served", "set_residual_norm_hip", "dropout_keep_mask"):
        assert callable(getattr(decode_ops, name))


def test_workspace_question_is_host_arithmetic():
    from daspeech_amd import _lib, build, decode_ops
    build.build()
    ws = _lib.load().dsp_resnorm_train_workspace_bytes
    CH = decode_ops.RESNORM_CHUNK_ROWS
    assert ws(0, 256) == 0 and ws(-3, 256) == 0 and ws(100, 0) == 0           # an empty problem
    grid = [(1, 8), (CH, 8), (CH + 1, 8), (CH + 1, 16), (6 * CH + 53, 16), (6 * CH + 53, 512), (6400, 512), (6400, 2048), (1 << 24, 2048)]
    vals = [ws(*g) for g in grid]
    assert all(v > 0 and v % 16 == 0 for v in vals)
    assert vals == sorted(vals)                                             # each entry raises one argument of the one before
    assert ws(CH, 8) == ws(1, 8) and ws(CH + 1, 8) == 2 * ws(CH, 8)         # one partial of three fp32 columns sums per chunk
    assert ws(CH, 8) == 3 * 8 * 4
    for i, step_by in ((0, 1), (1, 4)):                                     # monotone in each argument on its own
        prev = 0
        for step in range(0, 70):
            a = [5, 8]
            a[i] += step * step_by
            v = ws(*a)
            assert v >= prev and v % 16 == 0, (a, v, prev)
            prev = v


class _OnGpu:
    """what residual_dropout_layer_norm_served reads of a tensor, answering as a contiguous GPU tensor would: the rule is pure argument
    inspection, so each unserved condition can be checked one at a time without a device"""

    def __init__(self, shape, dtype, contiguous=True, cuda=True, device="cuda:0", offset=0):
        self.shape, self.dtype, self._c, self.is_cuda = torch.Size(shape), dtype, contiguous, cuda
        self.device = torch.device(device) if cuda else torch.device("cpu")
        self._offset = offset                          # elements past a 16-byte boundary

    def data_ptr(self):
        return 0x7F0000001000 + self._offset * self.element_size()

    def dim(self):
        return len(self.shape)

    def numel(self):
        return self.shape.numel()

    def is_contiguous(self):
        return self._c

    def element_size(self):
        return torch.empty((), dtype=self.dtype).element_size()


class _Ln:
    def __init__(self, C, dtype):
        self.weight, self.bias, self.normalized_shape, self.eps = _OnGpu((C,), dtype), _OnGpu((C,), dtype), (C,), 1e-5


def _args(dtype=torch.float32, shape=(2, 5, 8), param_dtype=None, with_h=True, with_bias=False):
    pd = dtype if param_dtype is None else param_dtype
    x = _OnGpu(shape, dtype)
    h = _OnGpu(shape, dtype) if with_h else None
    return h, x, _Ln(shape[-1], pd), (_OnGpu((shape[-1],), pd) if with_bias else None)


def test_served_rule_says_no_to_each_unserved_condition():
    from daspeech_amd import decode_ops

    def served(h, x, ln, bias):
        return decode_ops.residual_dropout_layer_norm_served(h, x, ln, bias=bias)
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        assert served(*_args(dtype)) and served(*_args(dtype, param_dtype=torch.float32, with_bias=True)) and served(*_args(dtype, with_h=False))
    assert served(*_args(shape=(1, 4))) and served(*_args(shape=(3, 2048))) and served(*_args(torch.float16, shape=(2, 3, 4, 16)))
    assert served(*_args(shape=(1 << 24, 4)))

    def no(change=None, **kw):
        a = list(_args(**kw))
        if change is not None:
            change(a)
        assert not served(*a), kw

    no(lambda a: a.__setitem__(1, _OnGpu(a[1].shape, a[1].dtype, cuda=False)))                 # CPU
    no(lambda a: a.__setitem__(0, _OnGpu(a[0].shape, a[0].dtype, cuda=False)))
    no(lambda a: a.__setitem__(1, _OnGpu(a[1].shape, a[1].dtype, contiguous=False)))           # not contiguous
    no(lambda a: a.__setitem__(0, _OnGpu(a[0].shape, a[0].dtype, contiguous=False)))
    for dtype in (torch.float32, torch.float16, torch.bfloat16):                               # odd offset: contiguous, but off the 16-byte grid
        for off in (1, 3):
            no(lambda a: a.__setitem__(1, _OnGpu(a[1].shape, a[1].dtype, offset=off)), dtype=dtype)        # the residual
            no(lambda a: a.__setitem__(0, _OnGpu(a[0].shape, a[0].dtype, offset=off)), dtype=dtype)        # h
            no(lambda a: a.__setitem__(1, _OnGpu(a[1].shape, a[1].dtype, offset=off)), dtype=dtype, with_h=False)
            no(lambda a: setattr(a[2], "weight", _OnGpu((8,), a[2].weight.dtype, offset=off)), dtype=dtype)    # the parameters: views of a flat buffer
            no(lambda a: setattr(a[2], "bias", _OnGpu((8,), a[2].bias.dtype, offset=off)), dtype=dtype)
            no(lambda a: setattr(a[2], "weight", _OnGpu((8,), torch.float32, offset=off)), dtype=dtype, param_dtype=torch.float32)
            no(lambda a: a.__setitem__(3, _OnGpu((8,), a[3].dtype, offset=off)), dtype=dtype, with_bias=True)
        per = 16 // torch.empty((), dtype=dtype).element_size()                               # a whole number of 16-byte units: on the grid again
        a = list(_args(dtype, with_bias=True))
        a[0], a[1], a[3] = _OnGpu(a[0].shape, dtype, offset=per), _OnGpu(a[1].shape, dtype, offset=2 * per), _OnGpu((8,), dtype, offset=per)
        a[2].weight = _OnGpu((8,), dtype, offset=3 * per)
        assert served(*a)
    a = list(_args(with_h=False, with_bias=True))                                              # no h: `bias` is not read, so not asked about
    a[3] = _OnGpu((8,), torch.float32, offset=1)
    assert served(*a)
    no(lambda a: a.__setitem__(0, _OnGpu(a[0].shape, torch.float16)))                          # h of another dtype
    no(lambda a: a.__setitem__(0, _OnGpu((2, 5, 16), a[0].dtype)))                             # h of another shape
    no(lambda a: a.__setitem__(0, _OnGpu(a[0].shape, a[0].dtype, device="cuda:1")))            # h on another device
    no(dtype=torch.float64)                                                                    # float64
    no(shape=(2, 5, 6))                                                                        # C % 4
    no(dtype=torch.float16, shape=(2, 5, 12))                                                  # C % 8 for the 16-bit dtypes
    no(dtype=torch.bfloat16, shape=(2, 5, 4))
    no(shape=(3, 2052))                                                                        # C > 2048
    no(shape=((1 << 24) + 1, 4))                                                               # more than 2^24 rows
    no(shape=(0, 8))                                                                           # no rows
    no(shape=(8,))                                                                             # no row dimension
    no(dtype=torch.float16, param_dtype=torch.bfloat16)                                        # parameters neither the data dtype nor fp32
    no(lambda a: setattr(a[2], "bias", _OnGpu((8,), torch.float16)))                           # LayerNorm tensors of mixed dtypes
    no(lambda a: a.__setitem__(3, _OnGpu((8,), torch.float16)), with_bias=True)                # `bias` of another dtype than the LayerNorm's
    no(lambda a: setattr(a[2], "weight", None))                                                # elementwise_affine=False
    no(lambda a: setattr(a[2], "normalized_shape", (5, 8)))                                    # a norm over two dimensions
    no(lambda a: setattr(a[2], "normalized_shape", (16,)))
    no(lambda a: setattr(a[2], "weight", _OnGpu((8,), torch.float32, device="cuda:1")))
    torch.set_autocast_enabled(True)                                                           # autocast: torch keeps the lines
    try:
        assert not served(*_args())
    finally:
        torch.set_autocast_enabled(False)
    old = decode_ops.set_residual_norm_hip(False)                                              # the switch
    try:
        assert not served(*_args())
        assert decode_ops.set_residual_norm_hip(True) is False
        assert served(*_args())
    finally:
        decode_ops.set_residual_norm_hip(old)
    # real CPU tensors: never served
    assert not decode_ops.residual_dropout_layer_norm_served(torch.zeros(2, 5, 8), torch.zeros(2, 5, 8), nn.LayerNorm(8))


def test_the_layers_one_question_per_forward_agrees_with_the_per_site_rule():
    """residual_dropout_layer_norm_sites_served(x, ((ln, bias), ...)) == all(served(x, x, ln, bias=bias)) on served and unserved arguments"""
    from daspeech_amd import decode_ops
    sites_served, served = decode_ops.residual_dropout_layer_norm_sites_served, decode_ops.residual_dropout_layer_norm_served

    def both(x, sites):
        a = sites_served(x, sites)
        assert a == all(served(x, x, ln, bias=b) for ln, b in sites), (x.shape, x.dtype)
        return a
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        x = _OnGpu((2, 5, 8), dtype)
        assert both(x, ((_Ln(8, dtype), None), (_Ln(8, dtype), _OnGpu((8,), dtype))))
        assert both(x, ((_Ln(8, torch.float32), _OnGpu((8,), torch.float32)),))
    x = _OnGpu((2, 5, 8), torch.float16)
    ok = (_Ln(8, torch.float16), None)
    assert not both(x, (ok, (_Ln(8, torch.bfloat16), None)))                                   # one site's parameters in another dtype
    assert not both(x, (ok, (_Ln(8, torch.float16), _OnGpu((8,), torch.float32))))             # a bias of another dtype than its LayerNorm
    assert not both(x, (ok, (_Ln(16, torch.float16), None)))                                   # a LayerNorm of another width
    mixed = _Ln(8, torch.float16)
    mixed.bias = _OnGpu((8,), torch.float32)
    assert not both(x, ((mixed, None),))
    off = _Ln(8, torch.float16)
    off.weight = None
    assert not both(x, ((off, None),))
    other = _Ln(8, torch.float16)
    other.weight = _OnGpu((8,), torch.float16, device="cuda:1")
    assert not both(x, ((other, None),))
    for off in (1, 5):                                                                         # odd offsets: x, one site's weight, bias or `bias`
        assert not both(_OnGpu((2, 5, 8), torch.float16, offset=off), (ok,))
        for field in ("weight", "bias"):
            odd = _Ln(8, torch.float16)
            setattr(odd, field, _OnGpu((8,), torch.float16, offset=off))
            assert not both(x, (ok, (odd, None)))
        assert not both(x, (ok, (_Ln(8, torch.float16), _OnGpu((8,), torch.float16, offset=off))))
    assert both(_OnGpu((2, 5, 8), torch.float16, offset=8), ((_Ln(8, torch.float16), _OnGpu((8,), torch.float16, offset=16)),))
    for bad in (_OnGpu((2, 5, 8), torch.float16, cuda=False), _OnGpu((2, 5, 8), torch.float16, contiguous=False), _OnGpu((2, 5, 8), torch.float64),
                _OnGpu((2, 5, 12), torch.float16), _OnGpu((3, 2056), torch.float16), _OnGpu((8,), torch.float16)):
        assert not both(bad, ((_Ln(bad.shape[-1], bad.dtype), None),))
    old = decode_ops.set_residual_norm_hip(False)
    try:
        assert not both(x, (ok,))
    finally:
        decode_ops.set_residual_norm_hip(old)
    torch.set_autocast_enabled(True)
    try:
        assert not both(x, (ok,))
    finally:
        torch.set_autocast_enabled(False)
    assert not sites_served(torch.zeros(2, 5, 8), ((nn.LayerNorm(8), None),))


def test_operator_refuses_before_any_device_call():
    from daspeech_amd import decode_ops
    op = decode_ops.residual_dropout_layer_norm_autograd
    gen_state = torch.random.get_rng_state()
    x = torch.zeros(2, 5, 8, requires_grad=True)
    with pytest.raises(RuntimeError, match="GPU tensors"):                                      # CPU tensors
        op(x, x, nn.LayerNorm(8), p=0.1)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        op(None, x, nn.LayerNorm(8))
    with pytest.raises(RuntimeError, match="GPU tensors"):                                      # float64 is refused, never narrowed
        op(x.double(), x.double(), nn.LayerNorm(8).double())
    for hd, rd, pd, bd in ((torch.float16, torch.float32, torch.float32, None), (torch.float32, torch.float32, torch.float16, None),
                           (torch.float16, torch.float16, torch.bfloat16, None), (torch.float16, torch.float16, torch.float16, torch.float32),
                           (torch.float64, torch.float64, torch.float32, None)):
        bias = None if bd is None else torch.zeros(8, dtype=bd)
        with pytest.raises(RuntimeError, match="GPU tensors"):                                  # mixed dtypes: checked on the arguments alone
            op(torch.zeros(2, 5, 8, dtype=hd), torch.zeros(2, 5, 8, dtype=rd), nn.LayerNorm(8).to(pd), bias=bias)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        op(x, x, nn.LayerNorm(8, elementwise_affine=False))
    with pytest.raises(RuntimeError, match="GPU device"):
        decode_ops.dropout_keep_mask(1, 0, 0.1, (4, 8), "cpu")
    assert torch.equal(torch.random.get_rng_state(), gen_state)


def test_unserved_shapes_are_refused_with_the_shape_in_the_message(monkeypatch):
    """the shape rule sits behind the GPU check; with that check stubbed out it is reached on CPU tensors and still raises before any device call"""
    from daspeech_amd import decode_ops
    monkeypatch.setattr(decode_ops, "_gpu", lambda *a, **k: None)
    monkeypatch.setattr(decode_ops, "_reserve_dropout_stream", lambda *a: pytest.fail("the generator was touched"))
    monkeypatch.setattr(decode_ops._lib, "load", lambda: pytest.fail("the library was loaded"))
    op = decode_ops.residual_dropout_layer_norm_autograd
    for shape, C in (((2, 5, 6), 6), ((3, 2052), 2052), ((8,), 8), ((0, 8), 8)):
        with pytest.raises(RuntimeError, match="not served"):
            op(torch.zeros(shape), torch.zeros(shape), nn.LayerNorm(C), p=0.1)
    with pytest.raises(RuntimeError, match="not served"):
        op(torch.zeros(2, 5, 12, dtype=torch.float16), torch.zeros(2, 5, 12, dtype=torch.float16), nn.LayerNorm(12).half())
    with pytest.raises(RuntimeError, match="not served"):
        op(torch.zeros(2, 5, 8), torch.zeros(2, 4, 8), nn.LayerNorm(8))
    with pytest.raises(RuntimeError, match="not served"):
        op(torch.zeros(2, 5, 8), torch.zeros(2, 5, 8), nn.LayerNorm(8), p=1.0)
    with pytest.raises(RuntimeError, match="not served"):
        op(torch.zeros(2, 5, 8), torch.zeros(2, 5, 8), nn.LayerNorm((5, 8)))


# ---------------------------------------------------------------- the layer classes on the CPU: the torch lines, bit for bit

def _old_conformer(layer, x, pos, pad_mask):
    from daspeech_amd.models.daspeech import _drop
    c = layer.conv_module
    p, tr = layer.p, layer.training

    def ffn(m, x):
        return x + 0.5 * _drop(m["w_2"](_drop(F.silu(m["w_1"](m["layer_norm"](x))), p, tr)), p, tr)
    x = ffn(layer.ffn1, x)
    x = x + _drop(layer.self_attn(layer.self_attn_layer_norm(x), pos, pad_mask), p, tr)
    y = F.glu(F.linear(c["layer_norm"](x), c["pointwise_conv1"].weight.squeeze(-1)), dim=-1)
    y = F.silu(c["batch_norm"](c["depthwise_conv"](y.transpose(1, 2))))
    x = x + _drop(F.linear(y.transpose(1, 2), c["pointwise_conv2"].weight.squeeze(-1)), p, tr)
    x = ffn(layer.ffn2, x)
    return layer.final_layer_norm(x)


def _old_nat(layer, x, self_pad, enc, enc_pad):
    from daspeech_amd.models.daspeech import _drop
    p, tr = layer.p, layer.training
    x = layer.self_attn_layer_norm(x + _drop(layer.self_attn(x, x, self_pad), p, tr))
    x = layer.encoder_attn_layer_norm(x + _drop(layer.encoder_attn(x, enc, enc_pad), p, tr))
    return layer.final_layer_norm(x + _drop(layer.fc2(_drop(F.gelu(layer.fc1(x)), layer.p_act, tr)), p, tr))


def _old_fft(layer, x, pad):
    from daspeech_amd.models.fastspeech2 import _drop
    x = layer.layer_norm(layer.self_attn(x, pad, None, 0, residual=x))
    f = layer.ffn
    return f.layer_norm(_drop(f.ffn(x.transpose(1, 2)).transpose(1, 2), f.p, f.training) + x)


def _grads(layer, out, x, cot):
    params = [p for _, p in sorted(layer.named_parameters())]
    return torch.autograd.grad(out, [x] + params, cot, allow_unused=True)


def _same(layer, new, old, x0, cot):
    """layer(new) and its restatement (old) under the same seed: outputs and every gradient bit-equal"""
    res = []
    for fn in (new, old):
        m = copy.deepcopy(layer)
        torch.manual_seed(11)
        x = x0.clone().requires_grad_()
        out = fn(m, x)
        res.append((out, _grads(m, out, x, cot)))
    (oa, ga), (ob, gb) = res
    assert torch.equal(oa, ob)
    for u, v in zip(ga, gb):
        assert (u is None and v is None) or torch.equal(u, v)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_layers_in_training_mode_on_cpu_keep_the_torch_lines_bit_for_bit(dtype, p):
    from daspeech_amd.models.daspeech import ConformerLayer, NATDecoderLayer
    from daspeech_amd.models.fastspeech2 import FFTLayer
    torch.manual_seed(3)
    B, T, C = 2, 11, 16
    x0 = torch.randn(B, T, C, dtype=dtype)
    cot = torch.randn(B, T, C, dtype=dtype)
    pad = torch.arange(T).unsqueeze(0) >= torch.tensor([T, T - 3]).unsqueeze(1)
    pos = torch.randn(1, 2 * T - 1, C, dtype=dtype)
    conf = ConformerLayer(C, 32, 2, 7, dropout=p).to(dtype).train()
    _same(conf, lambda m, x: m(x, pos, pad), lambda m, x: _old_conformer(m, x, pos, pad), x0, cot)
    enc = torch.randn(B, 7, 24, dtype=dtype)
    enc_pad = torch.arange(7).unsqueeze(0) >= torch.tensor([7, 5]).unsqueeze(1)
    nat = NATDecoderLayer(C, 32, 2, 24, dropout=p, attention_dropout=p, activation_dropout=p).to(dtype).train()
    _same(nat, lambda m, x: m(x, pad, enc, enc_pad), lambda m, x: _old_nat(m, x, pad, enc, enc_pad), x0, cot)
    fft = FFTLayer(C, 2, 32, 3, dropout=p, attention_dropout=p).to(dtype).train()
    _same(fft, lambda m, x: m(x, pad), lambda m, x: _old_fft(m, x, pad), x0, cot)
