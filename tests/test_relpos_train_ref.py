"""CPU: tests/util_relpos_train_ref.py (the float64 restatement the GPU tests of the relative-position attention operator compare against)
pinned to torch float64 autograd of the module's own training lines (rel_shift formulation), and its mask index rule to the residual
operator's keep_mask."""
import numpy as np
import pytest
import torch

from tests import util_relpos_train_ref as A
from tests import util_resnorm_ref as R

TOL = 1e-11


def _case(T, mask_kind, p, B=2, H=2, seed=5):
    t = A.inputs(seed + T, B, T, H)
    pm = A.pad_masks(mask_kind, B, T)
    keep = A.keep_mask(11, 8, p, B, H, T) if p > 0 else None
    return t, pm, keep


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("mask_kind", ["none", "ragged"])
@pytest.mark.parametrize("T", [1, 2, 9, 33])
def test_restatement_equals_autograd_of_the_module_lines(T, mask_kind, p):
    t, pm, keep = _case(T, mask_kind, p)
    H = 2
    leaves = {n: t[n].clone().requires_grad_() for n in ("q", "k", "v", "pos", "bias_u", "bias_v")}
    o, lse = A.module_lines(leaves["q"], leaves["k"], leaves["v"], leaves["pos"], leaves["bias_u"], leaves["bias_v"], pm, H, keep, p)
    grads = torch.autograd.grad(o, list(leaves.values()), t["do"])
    f = A.forward(t["q"], t["k"], t["v"], t["pos"], t["bias_u"], t["bias_v"], pm, H, keep, p)
    b = A.backward(t["q"], t["k"], t["v"], t["pos"], t["bias_u"], t["bias_v"], pm, H, t["do"], keep, p)
    assert torch.allclose(f["o"], o.detach(), rtol=0, atol=TOL * max(1.0, float(o.abs().max())))
    assert torch.allclose(f["lse"], lse.detach(), rtol=0, atol=TOL * max(1.0, float(lse.abs().max())))
    for name, g in zip(("dq", "dk", "dv", "dpos", "du", "dv_bias"), grads):
        assert b[name].shape == g.shape, name
        assert torch.allclose(b[name], g, rtol=0, atol=TOL * max(1.0, float(g.abs().max()))), name
    # D_i = sum_j P_ij dP_ij, with dropout too
    Bn, Tn = t["q"].shape[:2]
    m = torch.ones_like(f["P"]) if keep is None else keep.double() / (1.0 - p)
    doh = t["do"].view(Bn, Tn, H, 64).permute(0, 2, 1, 3)
    vh = t["v"].view(Bn, Tn, H, 64).permute(0, 2, 1, 3)
    dP = torch.einsum("bhid,bhjd->bhij", doh, vh) * m
    D = (doh * f["o"].view(Bn, Tn, H, 64).permute(0, 2, 1, 3)).sum(-1)
    assert torch.allclose((f["P"] * dP).sum(-1), D, rtol=0, atol=1e-10 * max(1.0, float(D.abs().max())))


@pytest.mark.parametrize("T", [1, 2, 3, 4, 9, 33])
def test_mask_index_rule_is_the_residual_rule_at_a_padded_pitch(T):
    B, H, p, seed, offset = 2, 3, 0.4, 77, 12
    Tp = A.padded(T)
    assert Tp % 4 == 0 and T <= Tp < T + 4
    got = A.keep_mask(seed, offset, p, B, H, T).numpy()
    flat = R.keep_mask(seed, offset, p, B * H * T * Tp)
    for b, h, i, j in [(0, 0, 0, 0), (1, 2, T - 1, T - 1), (1, 0, T // 2, 0), (0, 1, 0, T - 1)]:
        assert got[b, h, i, j] == flat[((b * H + h) * T + i) * Tp + j]
    assert got.shape == (B, H, T, T)
    # four consecutive keys of one query share one Philox call at every T: a row starts on a counter boundary
    assert all((((b * H + h) * T + i) * Tp) % 4 == 0 for b in range(B) for h in range(H) for i in range(T))


def test_rel_shift_is_the_index_gather():
    T = 7
    x = torch.arange(2 * 3 * T * (2 * T - 1), dtype=torch.float64).view(2, 3, T, 2 * T - 1)
    idx = A._shift_index(T).expand(2, 3, T, T)
    assert torch.equal(A.rel_shift(x), torch.gather(x, 3, idx))
    assert np.array_equal(A._shift_index(3).numpy(), np.array([[2, 3, 4], [1, 2, 3], [0, 1, 2]]))
