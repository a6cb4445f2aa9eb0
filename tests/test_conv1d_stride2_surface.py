"""CPU: the surface of the stride-2 channels-last Conv1d training operator — the decode_ops names, the header's declarations and the binding,
what the C entries refuse before any device call, the reasons of the two _problem functions, what the `served` questions decline, the host
arithmetic of the workspace question, and that a CPU Conv1dSubsampler in training mode computes what its torch lines compute (the operator is a
GPU path in fp16 / bf16; CPU and fp32 callers keep their lines)."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from daspeech_amd import _lib, decode_ops
from daspeech_amd.models.daspeech import Conv1dSubsampler
from tests import util_conv1d_stride2_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("conv1d_stride2_channels_last_autograd", "conv1d_stride2_channels_last_served", "conv1d_stride2_channels_last_sites_served",
         "conv1d_stride2_channels_last_checked", "set_conv1d_stride2_train_hip", "_conv1d_s2_module_problem", "_conv1d_s2_train_problem")
ENTRIES = ("dsp_conv1d_s2_train_workspace_bytes", "dsp_conv1d_s2_train_fwd", "dsp_conv1d_s2_train_bwd")
DTYPES = (torch.float16, torch.bfloat16, torch.float32, torch.float64)


def _x(dtype=torch.float16, B=2, T=9, C=16):
    return torch.zeros(B, T, C, dtype=dtype)


def _conv(cin=16, cout=64, K=3, dtype=torch.float16, **kw):
    kw.setdefault("padding", (K - 1) // 2)
    kw.setdefault("stride", 2)
    return nn.Conv1d(cin, cout, K, **kw).to(dtype)


def test_the_names_exist():
    for n in NAMES:
        assert callable(getattr(decode_ops, n)), n
    assert isinstance(decode_ops.CONV1D_STRIDE2_TRAIN_HIP, bool)


def test_header_and_binding_declare_the_three_entry_points():
    text = open(os.path.join(ROOT, "include", "daspeech_decode.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for n in ENTRIES:
        assert re.search(r"\b%s\s*\(" % n, code), n
        assert n in _lib.SIGNATURES
    for s1, s2 in zip(("dsp_conv1d_train_workspace_bytes", "dsp_conv1d_train_fwd", "dsp_conv1d_train_bwd"), ENTRIES):
        assert _lib.SIGNATURES[s1][0] is _lib.SIGNATURES[s2][0] and _lib.SIGNATURES[s1][1] == _lib.SIGNATURES[s2][1]      # the stride-1 lists
    assert _lib.ABI_VERSION == 2


@pytest.fixture(scope="module")
def lib():
    from daspeech_amd import build
    build.build()
    return _lib.load()


def test_c_entries_refuse_before_any_device_call(lib):
    """every call below is refused by the argument checks: the pointers are host memory that no kernel is ever handed"""
    B, T, Cin, Cout, K = 2, 9, 16, 64, 3
    bufs = [ctypes.create_string_buffer(4096 + 16) for _ in range(8)]
    x, w, bias, y, ws, dx, dw, db = [(ctypes.addressof(b) + 15) & ~15 for b in bufs]
    nb0, nb1 = lib.dsp_conv1d_s2_train_workspace_bytes(0, B, T, Cin, Cout, K), lib.dsp_conv1d_s2_train_workspace_bytes(1, B, T, Cin, Cout, K)

    def fwd(x_=x, y_=y, ldx=Cin, ldy=Cout, Ci=Cin, Co=Cout, K_=K, nb=nb0):
        return lib.dsp_conv1d_s2_train_fwd(x_, ldx, w, bias, y_, ldy, ws, nb, 1, 1, B, T, Ci, Co, K_, None)

    def bwd(dy_=y, dx_=dx, ld=Cout, Ci=Cin, Co=Cout, K_=K, nb=nb1):
        return lib.dsp_conv1d_s2_train_bwd(dy_, ld, x, Cin, w, dx_, dw, db, ws, nb, 1, 1, B, T, Ci, Co, K_, None)

    for call in (fwd, bwd):
        for bad in (dict(Ci=8), dict(Ci=24), dict(Ci=0), dict(Ci=A.MAX_C + 16), dict(Co=80), dict(Co=32), dict(K_=4), dict(K_=17), dict(K_=0)):
            assert call(**bad) == -1, (call.__name__, bad)
            msg = lib.dsp_last_error()
            assert b"conv1d_s2_train_" + call.__name__.encode() in msg and b"multiple of 16" in msg and b"multiple of 64" in msg and b"K odd" in msg
    assert fwd(ldx=Cin + 4) == -1 and fwd(ldy=Cout + 4) == -1 and fwd(ldx=Cin - 8) == -1 and bwd(ld=Cout + 4) == -1      # off the 8-element grid
    assert b"multiple of 8" in lib.dsp_last_error()
    assert fwd(x_=x + 2) == -1 and b"16-byte aligned" in lib.dsp_last_error()                                              # a misaligned pointer
    assert bwd(dx_=dx + 2) == -1 and b"16-byte aligned" in lib.dsp_last_error()
    assert fwd(y_=x) == -1 and b"aliased" in lib.dsp_last_error()                                                          # an aliased output
    assert bwd(dx_=x) == -1 and b"aliases" in lib.dsp_last_error()
    assert bwd(dx_=dw) == -1 and b"two outputs alias" in lib.dsp_last_error()
    assert fwd(nb=nb0 - 1) == lib.dsp_conv1d_s2_train_bwd(y, Cout, x, Cin, w, dx, dw, db, ws, nb1 - 1, 1, 1, B, T, Cin, Cout, K, None) not in (0, -1)
    assert lib.dsp_conv1d_s2_train_fwd(x, Cin, w, bias, y, Cout, ws, nb0, 1, 1, 0, T, Cin, Cout, K, None) == 0          # no rows: nothing to do
    assert lib.dsp_conv1d_s2_train_bwd(y, Cout, x, Cin, w, None, None, None, None, 0, 1, 1, B, T, Cin, Cout, K, None) == 0      # nothing asked for


def test_workspace_question_is_host_arithmetic(lib):
    ws = lib.dsp_conv1d_s2_train_workspace_bytes
    for phase in (0, 1):
        assert ws(phase, 0, 9, 16, 64, 3) == 0 and ws(phase, 2, 0, 16, 64, 3) == 0 and ws(phase, 2, 9, 0, 64, 3) == 0
    S = A.WGRAD_ROWS
    for B, T, Cin, Cout, K in [(1, 1, 16, 64, 1), (3, 33, 80, 192, 5), (32, 2117, 80, 1024, 5), (1, 2 * S + 1, 16, 64, 3), (1, 2 * S, 16, 64, 3)]:
        n0, n1 = ws(0, B, T, Cin, Cout, K), ws(1, B, T, Cin, Cout, K)
        splits = (B * A.t_out(T) + S - 1) // S                              # the rows of dy, not of x
        assert n0 % 16 == 0 and n1 % 16 == 0
        assert n0 >= 2 * K * Cin * Cout                                     # the re-laid weight
        assert n0 + 4 * splits * K * Cin * Cout + 4 * Cout <= n1 < n0 + 4 * (splits + 1) * K * Cin * Cout + 4 * (B * T // 256 + 2) * Cout
        for grown in ((B + 1, T, Cin, Cout, K), (B, T + 1, Cin, Cout, K), (B, T, Cin + 16, Cout, K), (B, T, Cin, Cout + 64, K), (B, T, Cin, Cout, K + 2)):
            assert ws(0, *grown) >= n0 and ws(1, *grown) >= n1


def test_the_reasons_of_the_problem_functions():
    mod, why = decode_ops._conv1d_s2_module_problem, decode_ops._conv1d_s2_train_problem
    served = decode_ops.conv1d_stride2_channels_last_served
    x = _x()
    assert mod(_conv()) is None and "GPU" in why(x, _conv().weight, _conv().bias)      # a CPU tensor is all that is in the way here
    assert mod(_conv(stride=1)) == "stride 1: only 2 is served" and not served(x, _conv(stride=1))
    assert "dilation 2" in mod(_conv(dilation=2, padding=2))
    assert "groups 2" in mod(_conv(groups=2))
    assert "padding" in mod(_conv(K=5, padding=1)) and "padding" in mod(_conv(K=3, padding_mode="reflect"))
    assert "kernel size 4" in mod(_conv(K=4, padding=2)) and "kernel size 17" in mod(_conv(K=17))
    assert "conv has to be an nn.Conv1d" == mod(nn.Linear(4, 4))
    for cin in (8, 24, 72):
        assert "Cin a multiple of 16" in why(_x(C=cin), _conv(cin, 64).weight, None)
    assert "Cout a multiple of 64" in why(x, _conv(16, 80).weight, None) and "Cout a multiple of 64" in why(x, _conv(16, 32).weight, None)
    assert why(_x(C=80), _conv(80, 64).weight, None) == why(_x(C=16), _conv(16, 1024).weight, None) == decode_ops._NOT_GPU      # the real widths pass the rule
    for dtype in (torch.float32, torch.float64):
        assert "fp16 or bf16" in why(_x(dtype), _conv(dtype=dtype).weight, None)
    assert "fp32 keeps the torch lines" in why(_x(torch.float32), _conv(dtype=torch.float32).weight, None)
    assert "never narrowed" in why(_x(torch.float64), _conv(dtype=torch.float64).weight, None)
    assert "does not fit" in why(x, _conv(32, 64).weight, None)
    assert "bias" in why(x, _conv().weight, torch.zeros(65, dtype=torch.float16))
    assert "[B,T,Cin]" in why(torch.zeros(9, 16, dtype=torch.float16), _conv().weight, None)
    # the stride-1 rule did not move: 80 channels and stride 2 are still its refusals
    assert "multiples of 64" in decode_ops._conv1d_train_problem(_x(C=80), _conv(80, 64).weight, None)
    assert decode_ops._conv1d_module_problem(_conv()) == "stride 2: only 1 is served"


def test_served_is_false_on_cpu_with_the_switch_off_and_under_autocast():
    served, sites = decode_ops.conv1d_stride2_channels_last_served, decode_ops.conv1d_stride2_channels_last_sites_served
    for dtype in DTYPES:
        assert not served(_x(dtype), _conv(dtype=dtype)) and not sites(_x(dtype), (_conv(dtype=dtype), _conv(32, 64, dtype=dtype)))
    x = _x()
    default = decode_ops.CONV1D_STRIDE2_TRAIN_HIP
    old = decode_ops.set_conv1d_stride2_train_hip(False)
    try:
        assert old is default and decode_ops.CONV1D_STRIDE2_TRAIN_HIP is False
        assert not served(x, _conv()) and not sites(x, (_conv(), _conv(32, 64)))
        assert decode_ops.CONV1D_TRAIN_HIP is True                          # the stride-1 operator has its own switch
    finally:
        assert decode_ops.set_conv1d_stride2_train_hip(old) is False
    assert decode_ops.CONV1D_STRIDE2_TRAIN_HIP is default
    with torch.autocast("cpu", dtype=torch.bfloat16):
        assert not served(x, _conv()) and not sites(x, (_conv(),))


@pytest.mark.parametrize("what,reason", [("cpu", "GPU"), ("fp32", "fp16 or bf16"), ("float64", "never narrowed"), ("channels24", "Cin a multiple of 16"),
                                         ("cout80", "Cout a multiple of 64"), ("evenK", "kernel size 4"), ("weight2d", "[Cout,Cin,K]"),
                                         ("bias", "bias has to be")])
def test_public_function_refuses_with_the_reason(what, reason):
    dtype = {"fp32": torch.float32, "float64": torch.float64}.get(what, torch.float16)
    C = 24 if what == "channels24" else 16
    x = _x(dtype, C=C)
    w = _conv(C, 80 if what == "cout80" else 64, 4 if what == "evenK" else 3, dtype).weight
    if what == "weight2d":
        w = w[:, :, 0]
    bias = torch.zeros(3, dtype=dtype) if what == "bias" else None
    with pytest.raises(RuntimeError, match=re.escape(reason)):
        decode_ops.conv1d_stride2_channels_last_autograd(x, w, bias)


# ---------------------------------------------------------------- the module on the CPU: its torch lines, bit for bit

def _subsampler_lines(m, x, lens):
    """Conv1dSubsampler.forward as it was before the operator was wired in"""
    x = x.transpose(1, 2)
    for conv in m.conv_layers:
        x = F.glu(conv(x), dim=1)
    return x.transpose(1, 2), m.out_lengths(lens)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_cpu_subsampler_in_training_is_its_torch_lines(dtype, monkeypatch):
    """forward + backward of a CPU Conv1dSubsampler(80, 128, 64) in train(), with the switch on and off, against the lines it had before; the
    new branch is not taken on the CPU"""
    torch.manual_seed(0)
    B, T = 2, 11
    m = Conv1dSubsampler(80, 128, 64).to(dtype).train()
    x0 = torch.randn(B, T, 80).to(dtype)
    lens = torch.tensor([T, T - 4])
    params = [p for _, p in sorted(m.named_parameters())]
    calls = []
    real = decode_ops.conv1d_stride2_channels_last_checked
    monkeypatch.setattr(decode_ops, "conv1d_stride2_channels_last_checked", lambda *a, **k: (calls.append(1), real(*a, **k))[1])

    def run(f):
        x = x0.clone().requires_grad_()
        out, out_lens = f(x)
        cot = torch.ones_like(out) / 8
        return [out.detach(), out_lens] + list(torch.autograd.grad(out, [x] + params, cot))

    want = run(lambda x: _subsampler_lines(m, x, lens))
    assert want[0].shape == (B, 3, 64) and want[1].tolist() == [3, 2]
    for on in (True, False):
        old = decode_ops.set_conv1d_stride2_train_hip(on)
        try:
            got = run(lambda x: m(x, lens))
        finally:
            decode_ops.set_conv1d_stride2_train_hip(old)
        for g, w in zip(got, want):
            assert torch.equal(g, w), on
    assert not calls
