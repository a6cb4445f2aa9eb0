"""CPU: tests/util_actdrop_ref.py (the float64 restatement of the bias + activation + dropout operator by its own formulas) against float64
autograd of the torch lines the operator replaces: F.silu / F.gelu / F.relu / F.glu of (h + bias), times mask / (1 - p).  Agreement to
1e-11, the bound of the residual and relative-position reference tests."""
import pytest
import torch

from tests import util_actdrop_ref as A

TOL = 1e-11


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("R", [1, 2, 33])
@pytest.mark.parametrize("act", A.ACTS)
def test_restatement_matches_float64_autograd_of_the_torch_lines(act, R, with_bias, p):
    Cin = 24
    h, bias, dy = A.inputs(1000 * R + Cin, R, Cin, act)
    Cout = A.out_width(act, Cin)
    keep = None
    if p > 0:
        keep = torch.rand(R, Cout, generator=torch.Generator().manual_seed(R)) >= p
        assert keep.any() and not keep.all() or R * Cout < 8
    hh = h.clone().requires_grad_()
    bb = bias.clone().requires_grad_() if with_bias else None
    want = A.torch_lines(hh, bb, act, keep, p)
    assert want.dtype == torch.float64 and tuple(want.shape) == (R, Cout)
    grads = torch.autograd.grad(want, [hh] + ([bb] if with_bias else []), dy)

    y = A.forward(h, bias if with_bias else None, act, keep, p)
    dh, dbias = A.backward(h, bias if with_bias else None, act, dy, keep, p)
    scale = lambda t: max(float(t.detach().abs().max()), 1.0)
    assert float((y - want.detach()).abs().max()) <= TOL * scale(want)
    assert float((dh - grads[0]).abs().max()) <= TOL * scale(grads[0])
    if with_bias:
        assert float((dbias - grads[1]).abs().max()) <= TOL * scale(grads[1])
    else:
        assert float((dbias - grads[0].sum(0)).abs().max()) <= TOL * scale(grads[0].sum(0))
