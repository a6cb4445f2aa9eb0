"""CPU: tests/util_mha_train_ref.py (the float64 restatement the GPU tests of the multi-head attention operator compare against) pinned to
torch float64 autograd of the modules' own training lines and, without mask and dropout, to F.scaled_dot_product_attention — to 1e-11, the
bound the relative-position restatement is held to — and its mask index rule to the residual operator's keep_mask."""
import pytest
import torch
import torch.nn.functional as F

from tests import util_mha_train_ref as A
from tests import util_resnorm_ref as R

TOL = 1e-11
SHAPES = [(1, 1), (2, 3), (9, 5), (33, 40)]
NAMES = ("q", "k", "v")


def _close(a, b):
    return torch.allclose(a, b, rtol=0, atol=TOL * max(1.0, float(b.abs().max())))


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("mask_kind", ["none", "ragged"])
@pytest.mark.parametrize("N,M", SHAPES)
def test_restatement_equals_autograd_of_the_module_lines(N, M, mask_kind, p):
    B, H = 2, 2
    t = A.inputs(5 + N + 3 * M, B, N, M, H)
    pm = A.pad_masks(mask_kind, B, M)
    keep = A.keep_mask(11, 8, p, B, H, N, M) if p > 0 else None
    leaves = [t[n].clone().requires_grad_() for n in NAMES]
    o, lse = A.module_lines(*leaves, pm, H, keep, p)
    grads = torch.autograd.grad(o, leaves, t["do"])
    f = A.forward(t["q"], t["k"], t["v"], pm, H, keep, p)
    b = A.backward(t["q"], t["k"], t["v"], pm, H, t["do"], keep, p)
    assert f["o"].shape == (B, N, H * 64) and f["lse"].shape == (B, H, N)
    assert _close(f["o"], o.detach()) and _close(f["lse"], lse.detach())
    for name, g in zip(("dq", "dk", "dv"), grads):
        assert b[name].shape == g.shape, name
        assert _close(b[name], g), name


@pytest.mark.parametrize("N,M", SHAPES)
def test_restatement_equals_sdpa_without_mask_and_dropout(N, M):
    B, H = 2, 2
    t = A.inputs(50 + N + 3 * M, B, N, M, H)
    leaves = [t[n].clone().requires_grad_() for n in NAMES]
    qh, kh, vh = (x.view(B, -1, H, 64).transpose(1, 2) for x in leaves)
    o = F.scaled_dot_product_attention(qh, kh, vh).transpose(1, 2).reshape(B, N, H * 64)
    grads = torch.autograd.grad(o, leaves, t["do"])
    assert _close(A.forward(t["q"], t["k"], t["v"], None, H)["o"], o.detach())
    b = A.backward(t["q"], t["k"], t["v"], None, H, t["do"])
    for name, g in zip(("dq", "dk", "dv"), grads):
        assert _close(b[name], g), name


@pytest.mark.parametrize("N,M", [(1, 1), (2, 3), (3, 4), (5, 9), (9, 5), (33, 40)])
def test_mask_index_rule_is_the_residual_rule_at_a_padded_pitch(N, M):
    B, H, p, seed, offset = 2, 3, 0.4, 77, 12
    Mp = A.padded(M)
    assert Mp % 4 == 0 and M <= Mp < M + 4
    got = A.keep_mask(seed, offset, p, B, H, N, M).numpy()
    flat = R.keep_mask(seed, offset, p, B * H * N * Mp)
    assert got.shape == (B, H, N, M)
    for b, h, i, j in [(0, 0, 0, 0), (1, 2, N - 1, M - 1), (1, 0, N // 2, 0), (0, 1, 0, M - 1)]:
        assert got[b, h, i, j] == flat[((b * H + h) * N + i) * Mp + j]
    # four consecutive keys of one query share one Philox call at every M: a row starts on a counter boundary
    assert all((((b * H + h) * N + i) * Mp) % 4 == 0 for b in range(B) for h in range(H) for i in range(N))
