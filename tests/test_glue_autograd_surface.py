"""CPU-side surface of the differentiable variance-adaptor glue: the C symbols are declared and bound, the decode_ops functions exist and
refuse what they do not serve, and VarianceAdaptor keeps the torch formulation, bit for bit, where the HIP ops do not run (CPU tensors)."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["dsp_bucketize_embed_add_fwd", "dsp_embed_grad", "dsp_embed_grad_workspace_bytes", "dsp_length_regulator_bwd"]


def test_new_symbols_are_declared_bound_and_exported():
    from daspeech_amd import _lib, build, decode_ops
    text = open(os.path.join(ROOT, "include", "daspeech_decode.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in include/daspeech_decode.h"
        assert name in _lib.SIGNATURES
    m = re.search(r"#define\s+DSP_EMBED_GRAD_CHUNK\s+(\d+)", code)
    assert m and int(m.group(1)) == decode_ops.EMBED_GRAD_CHUNK
    assert re.search(r"#define\s+DSP_ABI_VERSION\s+2\b", open(os.path.join(ROOT, "include", "daspeech_dag.h")).read())
    assert "ascending" in text.lower() and "never reads padding frames" in text.lower()      # the contracts the header states
    build.build()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name)
    # the workspace question is host arithmetic: nothing for no rows, monotone in every argument
    ws = lib.dsp_embed_grad_workspace_bytes
    assert ws(0, 255, 256) == 0
    assert 0 < ws(1, 0, 1) <= ws(2, 0, 1) <= ws(4100, 0, 1) <= ws(4100, 255, 1) <= ws(4100, 255, 256)
    assert ws(4100, 255, 256) % 16 == 0


def test_autograd_ops_refuse_cpu_tensors_and_mismatched_dtypes():
    from daspeech_amd import decode_ops
    x = torch.zeros(2, 3, 4, requires_grad=True)
    v = torch.zeros(2, 3)
    bins = torch.tensor([0.0])
    w = torch.zeros(2, 4, requires_grad=True)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        decode_ops.bucketize_embed_add_autograd(x, v, bins, w)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        decode_ops.length_regulate_autograd(x, torch.ones(2, 3, dtype=torch.long))
    # the dtype rule is checked on the arguments alone, before anything touches a device
    for xd, wd in ((torch.float16, torch.float32), (torch.float32, torch.bfloat16), (torch.float64, torch.float64), (torch.int32, torch.int32)):
        with pytest.raises(RuntimeError, match="fp32 / fp16 / bf16"):
            decode_ops.bucketize_embed_add_autograd(torch.zeros(2, 3, 4, dtype=xd), v, bins, torch.zeros(2, 4, dtype=wd))


def _old_forward(va, x, padding_mask, durations, pitches, energies, d_factor=1.0, p_factor=1.0, e_factor=1.0):
    """VarianceAdaptor.forward under grad as it was before the HIP autograd ops: the torch formulation, restated"""
    B, N, C = x.shape
    log_dur_out = va.duration_predictor(x)
    pitch_out = va.pitch_predictor(x)
    pv = pitch_out * p_factor if pitches is None else pitches
    x = x + F.embedding(torch.bucketize(pv.detach(), va.pitch_bins), va.embed_pitch.weight)
    energy_out = va.energy_predictor(x)
    ev = energy_out * e_factor if energies is None else energies
    x = x + F.embedding(torch.bucketize(ev.detach(), va.energy_bins), va.embed_energy.weight)
    if durations is None:
        durations = torch.clamp(torch.round((torch.exp(log_dur_out.detach()) - 1) * d_factor).long(), min=0).masked_fill(padding_mask, 0)
    out_lens = durations.sum(1)
    maxlen = int(out_lens.max()) if B else 0
    cum = durations.cumsum(1)
    frames = torch.arange(maxlen, device=x.device).unsqueeze(0).expand(B, -1)
    src = torch.searchsorted(cum, frames.contiguous(), right=True).clamp(max=max(N - 1, 0))
    x = x.gather(1, src.unsqueeze(-1).expand(-1, -1, C)) * (frames < out_lens.unsqueeze(1)).unsqueeze(-1).to(x.dtype)
    if pitches is None:
        pitch_out = pitch_out * p_factor
    if energies is None:
        energy_out = energy_out * e_factor
    return x, out_lens, log_dur_out, pitch_out, energy_out


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("teacher", [True, False])
def test_variance_adaptor_on_cpu_keeps_the_torch_formulation_bit_for_bit(dtype, teacher):
    from daspeech_amd.models.fastspeech2 import VarianceAdaptor
    assert callable(getattr(VarianceAdaptor, "_forward_torch"))
    torch.manual_seed(5)
    va = VarianceAdaptor(32, 32, 3, 16, -4.66, 5.73, -4.95, 3.22, dropout=0.0).to(dtype)
    B, N = 3, 11
    x0 = torch.randn(B, N, 32, dtype=dtype)
    pmask = torch.arange(N).unsqueeze(0) >= torch.tensor([11, 7, 2]).unsqueeze(1)
    dur = torch.randint(0, 5, (B, N)).masked_fill(pmask, 0) if teacher else None
    pit = (torch.rand(B, N) * 10 - 4.6).to(dtype) if teacher else None
    ene = (torch.rand(B, N) * 8 - 4.9).to(dtype) if teacher else None
    params = [va.embed_pitch.weight, va.embed_energy.weight, va.pitch_predictor.proj.weight]
    results = []
    for fn in (lambda *a: va(*a), lambda *a: _old_forward(va, *a)):
        x = x0.clone().requires_grad_()
        with torch.enable_grad():
            outs = fn(x, pmask, dur, pit, ene)
            torch.manual_seed(9)
            loss = sum((o * torch.randn(o.shape, dtype=dtype)).sum() for o in outs if o.is_floating_point())
            grads = torch.autograd.grad(loss, [x] + params, allow_unused=True)
        results.append((outs, grads))
    (oa, ga), (ob, gb) = results
    assert oa[0].dtype == dtype and oa[1].dtype == torch.long
    for a, b in zip(oa, ob):
        assert torch.equal(a, b)
    for a, b in zip(ga, gb):
        assert (a is None and b is None) or torch.equal(a, b)
