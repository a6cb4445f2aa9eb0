"""CPU: the surface of the multi-head attention training operator — the decode_ops names, what the `served` question declines, what the public
function refuses, the header's declarations, and that CPU _MHA / _SelfAttention modules in training mode give the same bits with the switch on
and off (the operator is a GPU path; CPU and fp32 callers keep their lines)."""
import os
import re

import pytest
import torch

from daspeech_amd import _lib, decode_ops
from daspeech_amd.models.daspeech import _MHA
from daspeech_amd.models.fastspeech2 import _SelfAttention
from tests import util_mha_train_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mha_attention_autograd", "mha_attention_autograd_served", "mha_attention_checked", "set_mha_attention_hip")


def _args(dtype=torch.float16, B=2, N=9, M=5, H=2, dk=64):
    C = H * dk
    z = lambda *s: torch.zeros(*s, dtype=dtype)
    return [z(B, N, C), z(B, M, C), z(B, M, C)]


def test_the_names_exist():
    for n in NAMES:
        assert callable(getattr(decode_ops, n)), n
    assert decode_ops.MHA_ATTENTION_HIP is True
    assert decode_ops.MHA_TRAIN_MAX_LEN == A.MAX_LEN == 4096
    assert "mha_attention_autograd" in decode_ops.__doc__


def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "daspeech_decode.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for n in ("dsp_mha_train_fwd", "dsp_mha_train_bwd", "dsp_mha_train_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % n, code), n
        assert n in _lib.SIGNATURES
    assert re.search(r"#define\s+DSP_MHA_TRAIN_MAX_LEN\s+%d\b" % decode_ops.MHA_TRAIN_MAX_LEN, code)


def test_served_declines_what_the_kernels_do_not_take():
    served, why = decode_ops.mha_attention_autograd_served, decode_ops._mha_train_problem
    for dtype in (torch.float16, torch.bfloat16, torch.float32, torch.float64):
        assert not served(*_args(dtype), None, 2)                           # CPU tensors
    assert "GPU" in why(*_args(), None, 2)
    assert not served(*_args(torch.float32), None, 2)
    assert "fp16 or bf16" in why(*_args(torch.float32), None, 2) and "never narrowed" in why(*_args(torch.float64), None, 2)
    assert not served(*_args(dk=32), None, 2) and "head width 32" in why(*_args(dk=32), None, 2)
    assert "outside 1 .. 4096" in why(*_args(B=1, N=A.MAX_LEN + 1, H=1), None, 1) and "outside 1 .. 4096" in why(*_args(B=1, M=A.MAX_LEN + 1, H=1), None, 1)
    old = decode_ops.set_mha_attention_hip(False)
    try:
        assert old is True
        assert not served(*_args(), None, 2)
    finally:
        assert decode_ops.set_mha_attention_hip(old) is False
    assert decode_ops.MHA_ATTENTION_HIP is True


def test_shape_and_layout_reasons():
    """the questions behind the device question, asked without a device through stand-ins that carry a CPU tensor's shape, strides and dtype
    and answer is_cuda with True: a [B,N] mask where N != M and k / v of different row strides are in the way, the second by layout"""
    why = decode_ops._mha_train_problem

    class OnGpu:                                                            # a tensor's shape, strides and dtype with is_cuda answered True
        def __init__(self, t, ptr=0):
            self.t, self.ptr = t, ptr
            self.shape, self.dtype, self.device, self.is_cuda = t.shape, t.dtype, t.device, True

        def dim(self):
            return self.t.dim()

        def stride(self, i):
            return self.t.stride(i)

        def data_ptr(self):
            return self.ptr

    B, N, M, H = 2, 9, 5, 2
    C = H * 64
    q = torch.zeros(B, N, C, dtype=torch.float16)
    kv = torch.zeros(B, M, 2 * C, dtype=torch.float16)
    k3 = torch.zeros(B, M, 3 * C, dtype=torch.float16)
    served_like = lambda *a: why(*a)
    import daspeech_amd.decode_ops as D
    real = D.Tensor
    D.Tensor = (real, OnGpu)                                                # isinstance(q, Tensor) takes the stand-ins
    try:
        ok = served_like(OnGpu(q), OnGpu(kv[..., :C]), OnGpu(kv[..., C:]), None, H)
        assert ok is None, ok                                               # views into a stacked k|v projection are taken as they are
        assert ok is None and served_like(OnGpu(q), OnGpu(kv[..., :C]), OnGpu(kv[..., C:]), torch.zeros(B, M, dtype=torch.bool), H) is None
        bad_mask = served_like(OnGpu(q), OnGpu(kv[..., :C]), OnGpu(kv[..., C:]), torch.zeros(B, N, dtype=torch.bool), H)
        assert bad_mask is not None and "[B,M]" in bad_mask and not bad_mask.startswith(D._LAYOUT)
        strides = served_like(OnGpu(q), OnGpu(kv[..., :C]), OnGpu(k3[..., :C]), None, H)
        assert strides is not None and strides.startswith(D._LAYOUT)
        assert served_like(OnGpu(q, ptr=8), OnGpu(kv[..., :C]), OnGpu(kv[..., C:]), None, H).startswith(D._LAYOUT)
    finally:
        D.Tensor = real


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32, torch.float64])
def test_public_function_refuses_cpu_and_float64(dtype):
    with pytest.raises(RuntimeError):
        decode_ops.mha_attention_autograd(*_args(dtype), None, 2)


def _run(module, args, cot):
    out = module(*args)
    params = [p for _, p in sorted(module.named_parameters())]
    return [out.detach()] + list(torch.autograd.grad(out, params, cot))


@pytest.mark.parametrize("with_mask", [False, True])
def test_cpu_modules_in_training_give_the_same_bits_with_the_switch_on_and_off(with_mask):
    torch.manual_seed(0)
    B, N, M = 2, 9, 5
    mha = _MHA(128, 2, kdim=64).train()
    sa = _SelfAttention(128, 2).train()
    x, mem, cot = torch.randn(B, N, 128), torch.randn(B, M, 64), torch.randn(B, N, 128)
    mem_pad = (torch.arange(M).unsqueeze(0) >= torch.tensor([M, M - 2]).unsqueeze(1)) if with_mask else None
    x_pad = (torch.arange(N).unsqueeze(0) >= torch.tensor([N, N - 3]).unsqueeze(1)) if with_mask else None
    res = {}
    for on in (True, False):
        old = decode_ops.set_mha_attention_hip(on)
        try:
            res[on] = _run(mha, (x, mem, mem_pad), cot) + _run(sa, (x, x_pad), cot)
        finally:
            decode_ops.set_mha_attention_hip(old)
    for a, b in zip(res[True], res[False]):
        assert torch.equal(a, b)
    # and they are the lines the modules had before the operator was wired in
    q = mha.q_proj(x).view(B, N, 2, -1).transpose(1, 2)
    k = mha.k_proj(mem).view(B, M, 2, -1).transpose(1, 2)
    v = mha.v_proj(mem).view(B, M, 2, -1).transpose(1, 2)
    mask = None if mem_pad is None else torch.zeros(B, 1, 1, M).masked_fill(mem_pad.view(B, 1, 1, M), float("-inf"))
    o = torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=mask, dropout_p=0.0)
    assert torch.equal(res[True][0], mha.out_proj(o.transpose(1, 2).reshape(B, N, 128)))
