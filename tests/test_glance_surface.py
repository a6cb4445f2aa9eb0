"""CPU-side checks of the glancing operators (csrc/glance.hip behind decode_ops.force_emit / decode_ops.glance_select): the C ABI declares
and binds the entry points, the switch round-trips, and on CPU tensors both operators and criterions.glat_function keep the torch
formulation — compared here with the criterion's force-emit expression and with the oracle's restatement of the reference's glancing
(oracle/graph_oracle.py).  The kernels themselves: tests/test_gpu_glance_ops.py."""
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import graph_oracle as gorc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 1
NINF = float("-inf")
ENTRY_POINTS = ("dsp_force_emit", "dsp_force_emit_bwd", "dsp_glance_oracle", "dsp_glance_reveal")


def test_header_declares_and_binding_lists_the_entry_points():
    from daspeech_amd import _lib, decode_ops
    text = open(os.path.join(ROOT, "include", "daspeech_decode.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    docs = "".join(re.findall(r"/\*.*?\*/", text, flags=re.S))
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES, name
        assert name + ":" in docs, name                         # its doc block
    assert len(_lib.SIGNATURES["dsp_force_emit"][1]) == 12 and len(_lib.SIGNATURES["dsp_force_emit_bwd"][1]) == 12
    assert len(_lib.SIGNATURES["dsp_glance_oracle"][1]) == 9 and len(_lib.SIGNATURES["dsp_glance_reveal"][1]) == 13
    # the header's row bound is the one the Python side dispatches on
    assert int(re.search(r"#define\s+DSP_GLANCE_MAX_L\s+(\d+)", code).group(1)) == decode_ops.GLANCE_MAX_L
    assert int(re.search(r"#define\s+DSP_F64\s+(\d+)", code).group(1)) == decode_ops._F64_CODE
    assert _lib.ABI_VERSION == int(re.search(r"#define\s+DSP_ABI_VERSION\s+(\d+)", open(os.path.join(ROOT, "include", "daspeech_dag.h")).read()).group(1))


def test_kernel_source_is_picked_up_by_the_build():
    from daspeech_amd import build
    assert os.path.join(build.CSRC, "glance.hip") in build.sources()


def test_switch_round_trips():
    from daspeech_amd import decode_ops
    assert callable(decode_ops.force_emit) and callable(decode_ops.glance_select)
    first = decode_ops.set_glance_hip(False)
    try:
        assert first is True                                    # on by default
        assert decode_ops.set_glance_hip(True) is False
        assert decode_ops.set_glance_hip(True) is True
    finally:
        decode_ops.set_glance_hip(first)
    assert decode_ops.GLANCE_HIP is True


def _criterion_expression(match_all, matchmask, keep_word_mask):
    """daspeech_amd/criterions.py, _dag_loss_core (nat_dag_loss.py:130-132)"""
    glat_prev_mask = keep_word_mask.unsqueeze(1)
    return match_all.masked_fill(glat_prev_mask, 0) + \
        match_all.masked_fill(~matchmask, float("-inf")).masked_fill(~glat_prev_mask, 0).detach()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16])
@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 3, 5), (3, 7, 6)])
def test_force_emit_on_cpu_is_the_torch_expression(shape, dtype):
    from daspeech_amd import decode_ops
    B, T, L = shape
    gen = torch.Generator().manual_seed(B * 100 + T * 10 + L)
    match = (torch.randn(B, T, L, generator=gen) * 2 - 3).to(dtype)
    match[0, 0, 0] = NINF
    path = torch.randint(-1, T, (B, L), generator=gen)
    revealed = torch.rand(B, L, generator=gen) < 0.5
    path[0, L - 1] = -1
    revealed[0, L - 1] = True                                   # a revealed vertex without an alignment: a column of -inf
    matchmask = torch.zeros(B, T + 1, L, dtype=torch.bool).scatter_(1, path.unsqueeze(1) + 1, 1)[:, 1:]
    assert torch.equal(decode_ops.emission_mask(path, T), matchmask)
    assert not decode_ops.force_emit_served(match, path, revealed)
    a = match.clone().requires_grad_()
    b = match.clone().requires_grad_()
    out = decode_ops.force_emit(a, path, revealed)
    want = _criterion_expression(b, matchmask, revealed)
    assert out.dtype == dtype and torch.equal(out, want)
    assert torch.isneginf(out[0, :, L - 1]).all()
    g = torch.randn(B, T, L, generator=gen).to(dtype)
    out.backward(g)
    want.backward(g)
    assert torch.equal(a.grad, b.grad) and torch.equal(a.grad, g.masked_fill(revealed.unsqueeze(1), 0))


def _hand_case():
    """the hand case of tests/test_graph_golden.py: path = (0, -1, 1, 2), oracle = (5, 5, 6, 7), two vertices already right"""
    V = 10
    logits = np.full((1, 4, V), -2.0, np.float32)
    logits[0, 0, 5] = 5; logits[0, 1, 9] = 5; logits[0, 2, 9] = 5; logits[0, 2, 6] = 4; logits[0, 3, 7] = 5
    ln = math.log
    links = np.array([[[ln(.5), ln(.5), NINF], [ln(.5), ln(.5), NINF], [0.0, NINF, NINF], [NINF, NINF, NINF]]], np.float32)
    prev = np.array([[0, 3, 3, 2]]); tgt = np.array([[5, 6, 7]])
    return logits, links, prev, tgt


@pytest.mark.parametrize("strategy,p,noise,unif,unif_n", [
    ("number-random", 1.0, [[0.3, 9.0, -0.2, 0.1]], [[0.5, 0.5, 0.5, 0.5]], None),
    ("number-random", 3.0, [[0.3, 9.0, -0.2, 0.1]], [[0.5, 0.5, 0.5, 0.5]], None),          # a count of 3: every aligned vertex
    ("number-random", 0.2, [[0.0, 9.0, -0.0, 0.0]], [[0.5, 0.5, 0.5, 0.5]], None),          # a count of 0: nothing
    ("cmlm", 0.5, [[0.5, 9.0, 0.5, -1.0]], [[0.5, 0.5, 0.5, 0.5]], [0.4]),                  # count 1, two scores tie at the threshold
    (None, 0.6, None, [[0.1, 0.0, 0.3, 0.19]], None),
])
def test_glat_function_on_cpu_matches_the_oracle(strategy, p, noise, unif, unif_n):
    from daspeech_amd.criterions import glat_function
    logits, links, prev, tgt = _hand_case()
    f = lambda a: None if a is None else np.asarray(a, np.float32)
    noise, unif, unif_n = f(noise), f(unif), f(unif_n)
    o = gorc.glat(logits, links, prev, tgt, p, strategy, noise=noise, unif=unif, pad=PAD, unif_n=unif_n)
    t = lambda a: None if a is None else torch.from_numpy(a)
    gp, gt, info = glat_function(SimpleNamespace(pad=PAD), t(logits.copy()), t(tgt), t(prev), {"context_p": p}, links=t(links),
                                 glance_strategy=strategy, torch_ops=True, noise=t(noise), unif=t(unif), unif_n=t(unif_n))
    assert sorted(info) == sorted(["glat_accu", "glat_context_p", "glat_keep", "matchmask", "keep_word_mask", "glat_prev_output_tokens", "path",
                                   "oracle", "same_num"])
    for key in ("path", "matchmask", "oracle", "same_num", "keep_word_mask"):
        np.testing.assert_array_equal(info[key].numpy(), o[key], err_msg=key)
    np.testing.assert_array_equal(gp.numpy(), o["glat_prev_output_tokens"])
    assert gp is info["glat_prev_output_tokens"] and gt.tolist() == tgt.tolist()
    assert float(info["glat_accu"]) == pytest.approx(float(o["glat_accu"]), rel=1e-6)
    assert float(info["glat_keep"]) == pytest.approx(float(o["glat_keep"]), rel=1e-6)


def test_glance_select_on_cpu_matches_the_oracle():
    from daspeech_amd import decode_ops
    logits, links, prev, tgt = _hand_case()
    noise = np.array([[0.5, 9.0, 0.5, -1.0]], np.float32)
    unif = np.full((1, 4), 0.5, np.float32)
    o = gorc.glat(logits, links, prev, tgt, 1.0, "number-random", noise=noise, unif=unif, pad=PAD)
    t = torch.from_numpy
    sel = decode_ops.glance_select(t(tgt), t(o["path"]), t(logits).argmax(-1), t(prev), torch.tensor([3]), 1.0, "number-random",
                                   noise=t(noise), unif=t(unif))
    np.testing.assert_array_equal(sel["oracle"].numpy(), o["oracle"])
    np.testing.assert_array_equal(sel["n_right"].numpy(), o["same_num"])
    np.testing.assert_array_equal(sel["keep_prob"].numpy(), o["keep_prob"])
    np.testing.assert_array_equal(sel["revealed"].numpy(), o["keep_word_mask"])
    np.testing.assert_array_equal(sel["glanced"].numpy(), o["glat_prev_output_tokens"])
    assert sel["keep_prob"].tolist() == [[1.0, 0.0, 1.0, 0.0]]                # count 1, both 0.5 tie with the threshold; 9.0 is off the path
    with pytest.raises(ValueError):
        decode_ops.glance_select(t(tgt), t(o["path"]), t(logits).argmax(-1), t(prev), torch.tensor([3]), 1.0, "best-first")
    assert decode_ops.GLANCE_MAX_L * 4 + 256 * 4 + 8 <= 64 * 1024             # the score row, the histogram and the selection state in one workgroup's LDS
