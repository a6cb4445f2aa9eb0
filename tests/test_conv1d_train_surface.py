"""CPU: the surface of the channels-last Conv1d training operator — the decode_ops names, what the `served` question declines, what the public
function refuses and why, the header's declarations, the host arithmetic of the workspace question, and that a CPU _ConvFFN / VariancePredictor
in training mode computes what its torch lines compute (the operator is a GPU path in fp16 / bf16; CPU and fp32 callers keep their lines)."""
import os
import re

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from daspeech_amd import _lib, decode_ops
from daspeech_amd.models.fastspeech2 import VariancePredictor, _ConvFFN
from tests import util_conv1d_train_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("conv1d_channels_last_autograd", "conv1d_channels_last_served", "conv1d_channels_last_checked", "set_conv1d_train_hip")
DTYPES = (torch.float16, torch.bfloat16, torch.float32, torch.float64)


def _x(dtype=torch.float16, B=2, T=9, C=64):
    return torch.zeros(B, T, C, dtype=dtype)


def _conv(cin=64, cout=64, K=3, dtype=torch.float16, **kw):
    kw.setdefault("padding", (K - 1) // 2)
    return nn.Conv1d(cin, cout, K, **kw).to(dtype)


def test_the_four_names_exist():
    for n in NAMES:
        assert callable(getattr(decode_ops, n)), n
    assert decode_ops.CONV1D_TRAIN_HIP is True
    assert (decode_ops.CONV1D_TRAIN_ROW_TILE, decode_ops.CONV1D_TRAIN_WGRAD_ROWS) == (A.ROW_TILE, A.WGRAD_ROWS)
    assert (decode_ops.CONV1D_TRAIN_MAX_K, decode_ops.CONV1D_TRAIN_MAX_C) == (A.MAX_K, A.MAX_C)


def test_served_declines_what_the_kernels_do_not_take():
    served = decode_ops.conv1d_channels_last_served
    for dtype in DTYPES:
        assert not served(_x(dtype), _conv(dtype=dtype))                    # CPU tensors of every dtype
    # what is in the way, by its own reason: the questions about the module, the dtype and the sizes come before the one about the device
    mod, why = decode_ops._conv1d_module_problem, decode_ops._conv1d_train_problem
    x = _x()
    assert mod(_conv()) is None and "GPU" in why(x, _conv().weight, _conv().bias)      # a CPU tensor is all that is in the way here
    assert "stride 2" in mod(_conv(stride=2)) and not served(x, _conv(stride=2))
    assert "dilation 2" in mod(_conv(dilation=2, padding=2)) and not served(x, _conv(dilation=2, padding=2))
    assert "groups 2" in mod(_conv(groups=2)) and not served(x, _conv(groups=2))
    assert "padding" in mod(_conv(K=5, padding=1)) and not served(x, _conv(K=5, padding=1))
    assert "padding" in mod(_conv(K=3, padding=1, padding_mode="reflect"))
    assert "kernel size 4" in mod(_conv(K=4, padding=2)) and not served(x, _conv(K=4, padding=2))
    assert "kernel size 17" in mod(_conv(K=17))
    assert "multiples of 64" in why(_x(C=80), _conv(80, 80).weight, None) and not served(_x(C=80), _conv(80, 80))
    assert "multiples of 64" in why(x, _conv(64, 80).weight, None) and not served(x, _conv(64, 80))
    for dtype in (torch.float32, torch.float64):
        assert "fp16 or bf16" in why(_x(dtype), _conv(dtype=dtype).weight, None)
    assert "never narrowed" in why(_x(torch.float64), _conv(dtype=torch.float64).weight, None)
    assert "does not fit" in why(x, _conv(128, 64).weight, None)
    assert "does not fit" in why(x, _conv(groups=2).weight, None)           # [Cout, Cin/2, K]
    assert "bias" in why(x, _conv().weight, torch.zeros(65, dtype=torch.float16))
    assert "[B,T,Cin]" in why(torch.zeros(9, 64, dtype=torch.float16), _conv().weight, None)
    old = decode_ops.set_conv1d_train_hip(False)
    try:
        assert old is True and decode_ops.CONV1D_TRAIN_HIP is False
        assert not served(x, _conv())
        assert not decode_ops.conv1d_channels_last_sites_served(x, (_conv(), _conv()))
    finally:
        assert decode_ops.set_conv1d_train_hip(old) is False
    assert decode_ops.CONV1D_TRAIN_HIP is True
    with torch.autocast("cpu", dtype=torch.bfloat16):
        assert not served(x, _conv())


@pytest.mark.parametrize("what,reason", [("cpu", "GPU"), ("fp32", "fp16 or bf16"), ("float64", "never narrowed"), ("channels80", "multiples of 64"),
                                         ("evenK", "kernel size 4"), ("groups2", "does not fit"), ("weight2d", "[Cout,Cin,K]"),
                                         ("bias", "bias has to be")])
def test_public_function_refuses_with_the_reason(what, reason):
    dtype = {"fp32": torch.float32, "float64": torch.float64}.get(what, torch.float16)
    C = 80 if what == "channels80" else 64
    x = _x(dtype, C=C)
    w = _conv(C, C, 4 if what == "evenK" else 3, dtype, groups=2 if what == "groups2" else 1).weight
    if what == "weight2d":
        w = w[:, :, 0]
    bias = torch.zeros(3, dtype=dtype) if what == "bias" else None
    with pytest.raises(RuntimeError, match=re.escape(reason)):
        decode_ops.conv1d_channels_last_autograd(x, w, bias)


def test_header_declares_the_three_entry_points():
    text = open(os.path.join(ROOT, "include", "daspeech_decode.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for n in ("dsp_conv1d_train_fwd", "dsp_conv1d_train_bwd", "dsp_conv1d_train_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % n, code), n
        assert n in _lib.SIGNATURES
    for name, value in (("ROW_TILE", decode_ops.CONV1D_TRAIN_ROW_TILE), ("WGRAD_ROWS", decode_ops.CONV1D_TRAIN_WGRAD_ROWS),
                        ("MAX_K", decode_ops.CONV1D_TRAIN_MAX_K), ("MAX_C", decode_ops.CONV1D_TRAIN_MAX_C)):
        assert re.search(r"#define\s+DSP_CONV1D_TRAIN_%s\s+%d\b" % (name, value), code), name
    assert _lib.ABI_VERSION == 2


def test_workspace_question_is_host_arithmetic():
    from daspeech_amd import build
    build.build()
    ws = _lib.load().dsp_conv1d_train_workspace_bytes
    for phase in (0, 1):
        assert ws(phase, 0, 9, 64, 64, 3) == 0 and ws(phase, 2, 0, 64, 64, 3) == 0 and ws(phase, 2, 9, 0, 64, 3) == 0
    S = A.WGRAD_ROWS
    for B, T, Cin, Cout, K in [(1, 1, 64, 64, 1), (3, 33, 64, 192, 9), (32, 62, 256, 256, 3), (32, 530, 256, 1024, 9), (1, S + 1, 64, 64, 3)]:
        n0, n1 = ws(0, B, T, Cin, Cout, K), ws(1, B, T, Cin, Cout, K)
        splits = (B * T + S - 1) // S
        assert n0 % 16 == 0 and n1 % 16 == 0
        assert n0 >= 2 * K * Cin * Cout                                     # the re-laid weight
        assert n1 >= n0 + 4 * splits * K * Cin * Cout + 4 * Cout            # ... the fp32 partials of dW, one per split, and of db
        for grown in ((B + 1, T, Cin, Cout, K), (B, T + 1, Cin, Cout, K), (B, T, Cin + 64, Cout, K), (B, T, Cin, Cout + 64, K), (B, T, Cin, Cout, K + 2)):
            assert ws(0, *grown) >= n0 and ws(1, *grown) >= n1


# ---------------------------------------------------------------- the two modules on the CPU: their torch lines, bit for bit

def _ffn_lines(m, x):
    """_ConvFFN.forward as it was before the operator was wired in (CPU: no HIP residual operator either)"""
    h = m.ffn(x.transpose(1, 2)).transpose(1, 2)
    return m.layer_norm((F.dropout(h, m.p, True) if m.training and m.p > 0 else h) + x)


def _predictor_lines(m, x):
    """VariancePredictor.forward as it was before the operator was wired in"""
    drop = lambda t: F.dropout(t, m.p, True) if m.training and m.p > 0 else t
    x = drop(m.ln1(m.conv1(x.transpose(1, 2)).transpose(1, 2)))
    x = drop(m.ln2(m.conv2(x.transpose(1, 2)).transpose(1, 2)))
    return m.proj(x).squeeze(2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("kind", ["ffn", "predictor"])
def test_cpu_modules_in_training_are_their_torch_lines(kind, dtype):
    """forward + backward of a CPU _ConvFFN(256, 1024, 9) / VariancePredictor(256, 256, 3) in training mode, with the switch on and off,
    against the lines they had before"""
    torch.manual_seed(0)
    B, T = 2, 7
    m, lines = (_ConvFFN(256, 1024, 9), _ffn_lines) if kind == "ffn" else (VariancePredictor(256, 256, 3), _predictor_lines)
    m = m.to(dtype).train()
    x0 = torch.randn(B, T, 256).to(dtype)
    params = [p for _, p in sorted(m.named_parameters())]

    def run(f):
        x = x0.clone().requires_grad_()
        out = f(x)
        cot = torch.ones_like(out) / 8
        return [out.detach()] + list(torch.autograd.grad(out, [x] + params, cot))

    want = run(lambda x: lines(m, x))
    for on in (True, False):
        old = decode_ops.set_conv1d_train_hip(on)
        try:
            got = run(m)
        finally:
            decode_ops.set_conv1d_train_hip(old)
        for g, w in zip(got, want):
            assert torch.equal(g, w), on
