"""CPU: the surface of the bias + activation + dropout training operator — the decode_ops names, what the `served` question declines, what the
public function refuses, the header's declarations, the host arithmetic of the workspace question, and that FFNAdapter and ConformerEncoder
in training mode on CPU compute the bits of the lines they had before the operator was wired in (the operator is a GPU path; the layer
classes are covered by tests/test_resnorm_surface.py)."""
import math
import os
import re
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from daspeech_amd import _lib, decode_ops
from daspeech_amd.models import daspeech as M
from daspeech_amd.models.fastspeech2 import FFNAdapter
from tests import util_actdrop_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bias_act_dropout_autograd", "bias_act_dropout_served", "bias_act_dropout_checked", "set_act_dropout_hip")


def _h(dtype=torch.float16, R=5, C=64):
    return torch.zeros(R, C, dtype=dtype)


def test_the_names_and_constants_exist():
    for n in NAMES:
        assert callable(getattr(decode_ops, n)), n
    assert decode_ops.ACT_DROPOUT_HIP is True
    assert (decode_ops.ACTDROP_CHUNK_ROWS, decode_ops.ACTDROP_MAX_CIN) == (A.CHUNK_ROWS, A.MAX_CIN)
    assert tuple(decode_ops.ACT_CODES) == A.ACTS and list(decode_ops.ACT_CODES.values()) == [0, 1, 2, 3, 4]


def test_served_declines_what_the_kernels_do_not_take():
    served, why = decode_ops.bias_act_dropout_served, decode_ops._actdrop_problem
    for dtype in (torch.float16, torch.bfloat16, torch.float32, torch.float64):
        assert not served(_h(dtype), None, "silu")                               # CPU tensors
    assert "float64" in why(_h(torch.float64), None, "silu")                    # by its own reason, before the question about the device
    assert "GPU" in why(_h(), None, "silu")
    assert not served(_h(C=68), None, "silu") and "not served" in why(_h(C=68), None, "silu")      # a width off the grid
    assert "not served" in why(_h(C=24), None, "glu")                # glu: an odd number of 16-byte groups
    assert "GPU" in why(_h(C=16), None, "glu") and "GPU" in why(_h(C=24), None, "gelu")      # these stop at the device only
    assert not served(_h(), torch.zeros(32, dtype=torch.float16), "silu")       # a bias of another width
    assert "bias" in why(_h(), torch.zeros(32, dtype=torch.float16), "silu")
    assert "bias" in why(_h(), torch.zeros(64, dtype=torch.bfloat16), "silu")       # nor of another 16-bit dtype
    assert "GPU" in why(_h(), torch.zeros(64, dtype=torch.float32), "silu")      # an fp32 bias is taken
    assert not served(_h(), None, "tanh") and "unknown activation" in why(_h(), None, "tanh")
    with torch.autocast("cpu", dtype=torch.bfloat16):
        assert not served(_h(), None, "silu")
    old = decode_ops.set_act_dropout_hip(False)
    try:
        assert old is True and decode_ops.ACT_DROPOUT_HIP is False
        assert not served(_h(), None, "silu")
        assert not decode_ops.bias_act_dropout_sites_served(_h(), ((64, None, "silu"),))
    finally:
        assert decode_ops.set_act_dropout_hip(old) is False
    assert decode_ops.ACT_DROPOUT_HIP is True


def test_row_pitch_of_views():
    pitch = decode_ops._row_pitch
    t = torch.zeros(4, 6, 64)
    assert pitch(t) == 64 and pitch(t[:, :, :32]) == 64 and pitch(t[:, 1:2, :32]) == 6 * 64 and pitch(t[0:1, 2:3, 8:16]) == 8
    assert pitch(t[:, :3, :32]) is None                                         # rows of two pitches
    assert pitch(t.transpose(0, 1)) is None and pitch(t.transpose(1, 2)) is None
    assert pitch(t[:, :, ::2]) is None


@pytest.mark.parametrize("case", ["cpu-fp16", "cpu-fp32", "float64", "off-grid", "bias-width", "switch-off", "autocast", "p", "act"])
def test_public_function_refuses(case):
    h, bias, act, p = _h(), None, "silu", 0.1
    if case == "cpu-fp32":
        h = _h(torch.float32)
    elif case == "float64":
        h = _h(torch.float64)
    elif case == "off-grid":
        h = _h(C=68)
    elif case == "bias-width":
        bias = torch.zeros(32, dtype=torch.float16)
    elif case == "p":
        p = 1.0
    elif case == "act":
        act = "tanh"
    old = decode_ops.set_act_dropout_hip(case != "switch-off")
    try:
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=case == "autocast"):
            with pytest.raises(RuntimeError) as e:
                decode_ops.bias_act_dropout_autograd(h, bias, act, p)
    finally:
        decode_ops.set_act_dropout_hip(old)
    assert "bias_act_dropout_autograd" in str(e.value)
    if case == "float64":
        assert "float64" in str(e.value) and "never narrowed" in str(e.value)


def test_header_declares_the_three_entry_points():
    text = open(os.path.join(ROOT, "include", "daspeech_decode.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for n in ("dsp_act_dropout_train_fwd", "dsp_act_dropout_train_bwd", "dsp_act_dropout_train_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % n, code), n
        assert n in _lib.SIGNATURES
    assert re.search(r"#define\s+DSP_ACTDROP_CHUNK_ROWS\s+%d\b" % decode_ops.ACTDROP_CHUNK_ROWS, code)
    assert re.search(r"#define\s+DSP_ACTDROP_MAX_CIN\s+%d\b" % decode_ops.ACTDROP_MAX_CIN, code)
    for name, c in decode_ops.ACT_CODES.items():
        assert re.search(r"#define\s+DSP_ACT_%s\s+%d\b" % (name.upper(), c), code), name
    assert _lib.ABI_VERSION == 2


def test_workspace_question_is_host_arithmetic():
    from daspeech_amd import build
    build.build()
    ws = _lib.load().dsp_act_dropout_train_workspace_bytes
    assert ws(0, 2048) == 0 and ws(-1, 2048) == 0 and ws(5, 0) == 0
    for R, C in [(1, 4), (31, 8), (32, 24), (33, 264), (6400, 2048), (1 << 24, 8192)]:
        n = ws(R, C)
        assert n % 16 == 0 and n >= -(-R // A.CHUNK_ROWS) * C * 4
        assert ws(R + 1, C) >= n and ws(R + A.CHUNK_ROWS, C) > n and ws(R, C + 1) >= n and ws(R, C + 8) > n


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_cpu_ffn_adapter_in_training_is_its_torch_lines(p):
    torch.manual_seed(0)
    m = FFNAdapter(16, 32, 24, dropout=p).train()
    x = torch.randn(2, 9, 16, requires_grad=True)
    cot = torch.randn(2, 9, 24)
    params = [q for _, q in sorted(m.named_parameters())]
    torch.manual_seed(7)
    out = m(x)
    got = torch.autograd.grad(out, [x] + params, cot)
    torch.manual_seed(7)
    y = F.relu(F.linear(x, m.fc1.weight, m.fc1.bias))
    y = F.dropout(y, p, True) if p > 0 else y
    want = F.linear(y, m.fc2.weight, m.fc2.bias)
    ref = torch.autograd.grad(want, [x] + params, cot)
    assert torch.equal(out, want)
    for g, r in zip(got, ref):
        assert torch.equal(g, r)


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_cpu_conformer_encoder_in_training_is_its_torch_lines(p):
    """the encoder's input Linear + dropout in front of its layers (which tests/test_resnorm_surface.py pins): subsample, scale, Linear,
    dropout, the positions and the layers, written out"""
    torch.manual_seed(0)
    a = SimpleNamespace(**dict(M.DEFAULT_ARGS, input_feat=8, conv_channels=16, encoder_layers=2, encoder_embed_dim=16, encoder_ffn_embed_dim=32,
                               encoder_attention_heads=2, depthwise_kernel=3, dropout=p))
    enc = M.ConformerEncoder(a).train()
    src = torch.randn(2, 37, 8)
    lens = torch.tensor([37, 30])
    params = [q for _, q in sorted(enc.named_parameters())]
    torch.manual_seed(7)
    out = enc(src, lens)["encoder_out"]
    cot = torch.randn(out.shape, generator=torch.Generator().manual_seed(1))
    got = torch.autograd.grad(out, params, cot, allow_unused=True)
    for bn in (l.conv_module["batch_norm"] for l in enc.conformer_layers):      # the second pass starts from the same running buffers
        bn.reset_running_stats()
    torch.manual_seed(7)
    x, ln = enc.subsample(src, lens)
    T = x.shape[1]
    pad = torch.arange(T).unsqueeze(0) >= ln.unsqueeze(1)
    x = F.linear(math.sqrt(16) * x, enc.linear.weight, enc.linear.bias)
    x = F.dropout(x, p, True) if p > 0 else x
    pos = M.rel_positional_encoding(T, 16, x.device, x.dtype)
    for layer in enc.conformer_layers:
        x = layer(x, pos, pad)
    ref = torch.autograd.grad(x, params, cot, allow_unused=True)
    assert torch.equal(out, x)
    for g, r in zip(got, ref):
        assert (g is None and r is None) or torch.equal(g, r)
