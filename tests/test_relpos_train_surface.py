"""CPU: the surface of the relative-position attention training operator — the decode_ops names, what the `served` question declines, what the
public function refuses, the header's declarations, the host arithmetic of the workspace question, and that a CPU RelPosSelfAttention in
training mode computes what its torch lines compute (the operator is a GPU path; CPU and fp32 callers keep their lines)."""
import math
import os
import re

import pytest
import torch

from daspeech_amd import _lib, decode_ops
from daspeech_amd.models.daspeech import RelPosSelfAttention
from tests import util_relpos_train_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("relpos_attention_autograd", "relpos_attention_autograd_served", "set_relpos_attention_hip")


def _args(dtype=torch.float16, B=2, T=9, H=2, dk=64):
    C = H * dk
    z = lambda *s: torch.zeros(*s, dtype=dtype)
    return [z(B, T, C), z(B, T, C), z(B, T, C), z(2 * T - 1, C), z(H, dk), z(H, dk)]


def test_the_three_names_exist():
    for n in NAMES:
        assert callable(getattr(decode_ops, n)), n
    assert callable(decode_ops.relpos_attention_checked)                    # the layer's unchecked entry
    assert decode_ops.RELPOS_TRAIN_MAX_T == A.MAX_T >= 1500


def test_served_declines_what_the_kernels_do_not_take():
    served = decode_ops.relpos_attention_autograd_served
    for dtype in (torch.float16, torch.bfloat16, torch.float32, torch.float64):
        assert not served(*_args(dtype), None, 2)                           # CPU tensors
    assert not served(*_args(dk=32), None, 2)                               # head width 32
    # what is in the way, by its own reason (the questions about dtype, head width and T come before the one about the device)
    why = decode_ops._relpos_train_problem
    assert "fp16 or bf16" in why(*_args(torch.float32), None, 2) and "fp16 or bf16" in why(*_args(torch.float64), None, 2)
    assert "head width 32" in why(*_args(dk=32), None, 2)
    assert "T = %d" % (A.MAX_T + 1) in why(*_args(T=A.MAX_T + 1, B=1, H=1), None, 1)
    assert "GPU" in why(*_args(), None, 2)
    old = decode_ops.set_relpos_attention_hip(False)
    try:
        assert old is True
        assert not served(*_args(), None, 2)
    finally:
        assert decode_ops.set_relpos_attention_hip(old) is False
    assert decode_ops.RELPOS_ATTENTION_HIP is True


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32, torch.float64])
def test_public_function_refuses_cpu_and_float64(dtype):
    with pytest.raises(RuntimeError):
        decode_ops.relpos_attention_autograd(*_args(dtype), None, 2)


def test_header_declares_the_three_entry_points():
    text = open(os.path.join(ROOT, "include", "daspeech_decode.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for n in ("dsp_relpos_attention_train_fwd", "dsp_relpos_attention_train_bwd", "dsp_relpos_attention_train_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % n, code), n
        assert n in _lib.SIGNATURES
    assert re.search(r"#define\s+DSP_RELPOS_TRAIN_MAX_T\s+%d\b" % decode_ops.RELPOS_TRAIN_MAX_T, code)
    assert _lib.ABI_VERSION == 2


def test_workspace_question_is_host_arithmetic():
    from daspeech_amd import build
    build.build()
    ws = _lib.load().dsp_relpos_attention_train_workspace_bytes
    assert ws(0, 9, 4) == 0 and ws(2, 0, 4) == 0 and ws(2, 9, 0) == 0
    for B, T, H in [(1, 1, 1), (3, 33, 4), (32, 200, 4), (32, 1500, 4)]:
        n = ws(B, T, H)
        assert n % 16 == 0 and n >= B * (2 * T - 1) * H * 64 * 4
        assert ws(B + 1, T, H) >= n and ws(B, T + 1, H) >= n and ws(B, T, H + 1) >= n


@pytest.mark.parametrize("dk", [64, 16])
@pytest.mark.parametrize("with_mask", [False, True])
def test_cpu_layer_in_training_is_its_torch_lines(dk, with_mask):
    """forward + backward of a CPU RelPosSelfAttention(...).train() against the lines it had before the operator was wired in"""
    torch.manual_seed(0)
    H, B, T = 2, 2, 9
    C = H * dk
    att = RelPosSelfAttention(C, H, dropout=0.0).train()
    x = torch.randn(B, T, C, requires_grad=True)
    pos = torch.randn(1, 2 * T - 1, C)
    pad = (torch.arange(T).unsqueeze(0) >= torch.tensor([T, T - 3]).unsqueeze(1)) if with_mask else None
    cot = torch.randn(B, T, C)
    out = att(x, pos, pad)
    params = [p for _, p in sorted(att.named_parameters())]
    got = torch.autograd.grad(out, [x] + params, cot)

    q = att.linear_q(x).view(B, T, H, dk)
    k = att.linear_k(x).view(B, T, H, dk).transpose(1, 2)
    v = att.linear_v(x).view(B, T, H, dk).transpose(1, 2)
    p = att.linear_pos(pos).view(1, -1, H, dk).transpose(1, 2)
    ac = torch.matmul((q + att.pos_bias_u).transpose(1, 2), k.transpose(-2, -1))
    bd = RelPosSelfAttention.rel_shift(torch.matmul((q + att.pos_bias_v).transpose(1, 2), p.transpose(-2, -1)))
    scores = (ac + bd) / math.sqrt(dk)
    if pad is not None:
        scores = scores.masked_fill(pad.view(B, 1, 1, T), float("-inf"))
    want = att.linear_out(torch.matmul(torch.softmax(scores, dim=-1), v).transpose(1, 2).reshape(B, T, C))
    ref = torch.autograd.grad(want, [x] + params, cot)
    assert torch.equal(out, want)
    for g, r in zip(got, ref):
        assert torch.equal(g, r)
