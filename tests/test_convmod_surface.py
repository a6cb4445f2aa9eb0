"""CPU-side surface of the convolution-module operator under autograd (csrc/conformer_train.hip): the C symbols are declared, bound and
exported, the workspace question is host arithmetic with the stated properties, decode_ops refuses what it does not serve before any
device call, dwconv_bn_silu_autograd_served says no to each unserved condition, and ConformerLayer in training mode keeps the torch lines,
bit for bit, where the operator does not run (CPU tensors)."""
import os
import re

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["dsp_dwconv_bn_silu_train_fwd", "dsp_dwconv_bn_silu_train_bwd", "dsp_dwconv_bn_silu_train_workspace_bytes"]


def test_new_symbols_are_declared_bound_and_exported():
    from daspeech_amd import _lib, build, decode_ops
    text = open(os.path.join(ROOT, "include", "daspeech_decode.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in include/daspeech_decode.h"
        assert name in _lib.SIGNATURES
    for macro, value in (("DSP_CONVMOD_TIME_TILE", decode_ops.CONVMOD_TIME_TILE), ("DSP_CONVMOD_CHUNK_TILES", decode_ops.CONVMOD_CHUNK_TILES)):
        m = re.search(r"#define\s+%s\s+(\d+)" % macro, code)
        assert m and int(m.group(1)) == value
    assert re.search(r"#define\s+DSP_ABI_VERSION\s+2\b", open(os.path.join(ROOT, "include", "daspeech_dag.h")).read())
    low = re.sub(r"\s*\n\s*\*\s*", " ", text.lower())                # the contracts the header states
    assert "every output element is written" in low and "ascending chunk order" in low and "no float atomics" in low
    build.build()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name)


def test_workspace_question_is_host_arithmetic():
    from daspeech_amd import _lib, build
    build.build()
    ws = _lib.load().dsp_dwconv_bn_silu_train_workspace_bytes
    assert ws(0, 100, 256, 31) == 0
    base = (4, 100, 64, 7)
    assert ws(*base) > 0
    grid = [(1, 1, 8, 3), (1, 7, 8, 3), (1, 8, 8, 3), (1, 9, 8, 3), (2, 9, 8, 3), (2, 9, 16, 3), (2, 9, 16, 7), (2, 129, 16, 7), (32, 200, 256, 31),
            (33, 200, 256, 31), (33, 201, 256, 31), (33, 201, 264, 31)]
    vals = [ws(*g) for g in grid]
    assert all(v > 0 and v % 16 == 0 for v in vals)
    assert vals == sorted(vals)                                   # each entry raises one argument of the one before
    for i in range(4):                                            # monotone in every argument on its own
        prev = 0
        for step in range(0, 40):
            a = list(base)
            a[i] += step * (8 if i == 2 else 1)
            v = ws(*a)
            assert v >= prev and v % 16 == 0, (a, v, prev)
            prev = v


def _layer_parts(C=8, K=7, dtype=torch.float32):
    conv = nn.Conv1d(C, C, K, padding=(K - 1) // 2, groups=C, bias=False).to(dtype)
    bn = nn.BatchNorm1d(C).to(dtype).train()
    return conv, bn


def test_operator_refuses_cpu_tensors_and_mismatched_dtypes_before_any_device_call():
    from daspeech_amd import decode_ops
    conv, bn = _layer_parts()
    x = torch.zeros(2, 5, 8, requires_grad=True)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        decode_ops.dwconv_bn_silu_autograd(x, conv.weight, bn)
    # the dtype rule is checked on the arguments alone, before anything touches a device
    for xd, wd, bd in ((torch.float16, torch.float32, torch.float32), (torch.float32, torch.bfloat16, torch.float32),
                       (torch.float64, torch.float64, torch.float64), (torch.float32, torch.float32, torch.float16),
                       (torch.float16, torch.float16, torch.bfloat16)):
        c2, b2 = _layer_parts(dtype=wd)
        b2 = b2.to(bd)
        with pytest.raises(RuntimeError, match="GPU tensors"):
            decode_ops.dwconv_bn_silu_autograd(torch.zeros(2, 5, 8, dtype=xd), c2.weight, b2)
    assert int(bn.num_batches_tracked) == 0


class _OnGpu:
    """what dwconv_bn_silu_autograd_served reads of a tensor, answering as a contiguous GPU tensor would: the rule is pure argument
    inspection, so each unserved condition can be checked one at a time without a device"""

    def __init__(self, shape, dtype, contiguous=True, cuda=True, offset=0):
        self.shape, self.dtype, self._c, self.is_cuda = torch.Size(shape), dtype, contiguous, cuda
        self.device = torch.device("cuda:0") if cuda else torch.device("cpu")
        self._offset = offset                          # elements past a 16-byte boundary

    def data_ptr(self):
        return 0x7F0000001000 + self._offset * self.element_size()

    def dim(self):
        return len(self.shape)

    def is_contiguous(self):
        return self._c

    def element_size(self):
        return torch.empty((), dtype=self.dtype).element_size()


class _Mod:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _served_args(dtype=torch.float32, C=8, K=7, B=2, T=5, bn_dtype=None):
    bd = dtype if bn_dtype is None else bn_dtype
    x = _OnGpu((B, T, C), dtype)
    conv = _Mod(weight=_OnGpu((C, 1, K), dtype), kernel_size=(K,), bias=None, stride=(1,), dilation=(1,), groups=C, padding=((K - 1) // 2,),
                padding_mode="zeros")
    bn = _Mod(weight=_OnGpu((C,), bd), bias=_OnGpu((C,), bd), running_mean=_OnGpu((C,), bd), running_var=_OnGpu((C,), bd), training=True,
              affine=True, momentum=0.1, num_features=C, eps=1e-5)
    return x, conv, bn


def test_served_rule_says_no_to_each_unserved_condition():
    from daspeech_amd import decode_ops
    served = decode_ops.dwconv_bn_silu_autograd_served
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        assert served(*_served_args(dtype, C=8))
        assert served(*_served_args(dtype, C=8, bn_dtype=torch.float32))
    assert served(*_served_args(torch.float32, C=4)) and served(*_served_args(B=2, T=1)) and served(*_served_args(B=1, T=2))
    for K in (3, 7, 15, 31):
        assert served(*_served_args(K=K))

    def no(change, **kw):
        x, conv, bn = _served_args(**kw)
        x, conv, bn = change(x, conv, bn) or (x, conv, bn)
        assert not served(x, conv, bn), (change.__code__.co_firstlineno, kw)

    no(lambda x, c, b: (_OnGpu(x.shape, x.dtype, cuda=False), c, b))                      # CPU
    no(lambda x, c, b: (_OnGpu(x.shape, x.dtype, contiguous=False), c, b))                # not contiguous
    no(lambda x, c, b: (_OnGpu((2, 5, 2, 8), x.dtype), c, b))                             # not [B,T,C]
    for dtype in (torch.float32, torch.float16, torch.bfloat16):                          # odd offset: contiguous, but off the 16-byte grid
        for off in (1, 2, 3):
            no(lambda x, c, b: (_OnGpu(x.shape, x.dtype, offset=off), c, b), dtype=dtype)
        per = 16 // torch.empty((), dtype=dtype).element_size()
        x, conv, bn = _served_args(dtype)
        assert served(_OnGpu(x.shape, dtype, offset=per), conv, bn) and served(_OnGpu(x.shape, dtype, offset=3 * per), conv, bn)
    # the parameters are read element by element: a flattened-buffer view of them is served (the C side asks nothing of them)
    x, conv, bn = _served_args()
    conv.weight = _OnGpu(conv.weight.shape, conv.weight.dtype, offset=1)
    bn.weight, bn.running_var = _OnGpu((8,), torch.float32, offset=1), _OnGpu((8,), torch.float32, offset=3)
    assert served(x, conv, bn)
    no(lambda x, c, b: None, C=6)                                                         # C % 4
    no(lambda x, c, b: None, dtype=torch.float16, C=12)                                   # C % 8 for the 16-bit dtypes
    no(lambda x, c, b: None, dtype=torch.bfloat16, C=4)
    no(lambda x, c, b: None, B=1, T=1)                                                    # B*T < 2
    no(lambda x, c, b: None, dtype=torch.float64)                                         # float64
    no(lambda x, c, b: setattr(c, "weight", _OnGpu(c.weight.shape, torch.float16)))       # conv weight of another dtype
    no(lambda x, c, b: None, dtype=torch.float16, bn_dtype=torch.bfloat16)                # BN neither the dtype of x nor fp32
    no(lambda x, c, b: setattr(b, "running_var", _OnGpu((8,), torch.float16)))            # BN tensors of mixed dtypes
    for K in (1, 5, 9, 33):
        no(lambda x, c, b: None, K=K)                                                     # kernel size
    no(lambda x, c, b: setattr(c, "stride", (2,)))
    no(lambda x, c, b: setattr(c, "dilation", (2,)))
    no(lambda x, c, b: setattr(c, "groups", 1))
    no(lambda x, c, b: setattr(c, "padding", (0,)))
    no(lambda x, c, b: setattr(c, "bias", _OnGpu((8,), torch.float32)))
    no(lambda x, c, b: setattr(b, "training", False))                                     # eval mode with gradients
    no(lambda x, c, b: setattr(b, "affine", False))
    no(lambda x, c, b: setattr(b, "momentum", None))
    # track_running_stats=False is served: no buffers to update
    x, conv, bn = _served_args()
    bn.running_mean = bn.running_var = None
    assert served(x, conv, bn)
    torch.set_autocast_enabled(True)                                                      # autocast: torch keeps the lines
    try:
        assert not served(*_served_args())
    finally:
        torch.set_autocast_enabled(False)
    old = decode_ops.set_conv_module_hip(False)                                           # the switch
    try:
        assert not served(*_served_args())
        assert decode_ops.set_conv_module_hip(True) is False
        assert served(*_served_args())
    finally:
        decode_ops.set_conv_module_hip(old)
    # real CPU modules: never served
    conv, bn = _layer_parts()
    assert not served(torch.zeros(2, 5, 8), conv, bn)


def _old_train_forward(layer, x, pos, pad_mask):
    """ConformerLayer.forward's training branch as it was before the operator: the torch lines, restated"""
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


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_conformer_layer_training_on_cpu_keeps_the_torch_lines_bit_for_bit(dtype):
    import copy
    from daspeech_amd.models.daspeech import ConformerLayer
    torch.manual_seed(3)
    B, T, C = 2, 11, 16
    a = ConformerLayer(C, 32, 2, 7, dropout=0.0).to(dtype).train()
    b = copy.deepcopy(a)
    x0 = torch.randn(B, T, C, dtype=dtype)
    pos = torch.randn(1, 2 * T - 1, C, dtype=dtype)
    pad = torch.arange(T).unsqueeze(0) >= torch.tensor([T, T - 3]).unsqueeze(1)
    cot = torch.randn(B, T, C, dtype=dtype)
    res = []
    for layer, fn in ((a, lambda *s: a(*s)), (b, lambda *s: _old_train_forward(b, *s))):
        x = x0.clone().requires_grad_()
        out = fn(x, pos, pad)
        params = [p for _, p in sorted(layer.named_parameters())]
        grads = torch.autograd.grad(out, [x] + params, cot, allow_unused=True)
        res.append((out, grads, layer.conv_module["batch_norm"]))
    (oa, ga, bna), (ob, gb, bnb) = res
    assert torch.equal(oa, ob)
    for u, v in zip(ga, gb):
        assert (u is None and v is None) or torch.equal(u, v)
    assert torch.equal(bna.running_mean, bnb.running_mean) and torch.equal(bna.running_var, bnb.running_var)
    assert int(bna.num_batches_tracked) == int(bnb.num_batches_tracked) == 1
