"""Pins the float64 restatements of tests/util_glue_grad_ref.py to torch CPU float64 autograd of the formulation the variance adaptor used in
training: x + F.embedding(bucketize(v, bins), W), and the length regulator as one gather."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import util_glue_grad_ref as R
from tests import util_glue_ref as G


@pytest.mark.parametrize("case", [(61, 300, 8, 17), (62, 5, 12, 2), (63, 3, 4, 0), (64, 1, 1, 1)])
def test_embed_grad_ref_is_torch_float64_autograd(case):
    seed, n, C, nb = case
    x, v, bins, emb = G.bucketize_inputs(seed, n, C, nb)
    g = np.random.default_rng(seed + 1).standard_normal((n, C))
    W = torch.from_numpy(emb).double().requires_grad_()
    X = torch.from_numpy(x).double().requires_grad_()
    idx = torch.bucketize(torch.from_numpy(v).double(), torch.from_numpy(bins).double())
    np.testing.assert_array_equal(idx.numpy(), G.bucketize_ref(v, bins))
    out = X + F.embedding(idx, W)
    gx, gw = torch.autograd.grad(out, (X, W), torch.from_numpy(g))
    np.testing.assert_array_equal(gx.numpy(), g)              # the gradient of x is the incoming gradient
    ref = R.embed_grad_ref(g, idx.numpy(), nb + 1)
    np.testing.assert_allclose(ref, gw.numpy(), rtol=1e-13, atol=1e-13)
    m, a = R.embed_grad_terms(g, idx.numpy(), nb + 1)
    assert m.sum() == n and np.all(a >= np.abs(ref) - 1e-12)
    empty = np.bincount(idx.numpy(), minlength=nb + 1) == 0
    assert np.all(ref[empty] == 0.0)


def _gather_regulator(x, durations):
    """the gather form of the length regulator (the training formulation of VarianceAdaptor)"""
    B, N, C = x.shape
    out_lens = durations.sum(1)
    maxlen = int(out_lens.max()) if B else 0
    cum = durations.cumsum(1)
    frames = torch.arange(maxlen).unsqueeze(0).expand(B, -1)
    src = torch.searchsorted(cum, frames.contiguous(), right=True).clamp(max=max(N - 1, 0))
    return x.gather(1, src.unsqueeze(-1).expand(-1, -1, C)) * (frames < out_lens.unsqueeze(1)).unsqueeze(-1).to(x.dtype)


@pytest.mark.parametrize("case", [(71, 3, 5, 6), (72, 2, 1, 1), (73, 2, 40, 3)])
def test_length_regulator_bwd_ref_is_torch_float64_autograd(case):
    seed, B, N, C = case
    rng = np.random.default_rng(seed)
    dur = rng.integers(0, 7, (B, N))
    dur[0, N // 2] = 0
    dur[B - 1] = 0                                            # one sample of zero length
    dur[0, N - 1] = 30                                        # one long segment: the other samples end far before maxlen
    x = torch.from_numpy(rng.standard_normal((B, N, C))).requires_grad_()
    out = _gather_regulator(x, torch.from_numpy(dur))
    g = rng.standard_normal(tuple(out.shape))
    gx, = torch.autograd.grad(out, x, torch.from_numpy(g))
    ref = R.length_regulator_bwd_ref(g, dur)
    np.testing.assert_allclose(ref, gx.numpy(), rtol=1e-13, atol=1e-13)
    assert np.all(ref[dur == 0] == 0.0)
    gp = g.copy()                                             # padding frames are never read
    for b in range(B):
        gp[b, int(dur[b].sum()):] = np.nan
    np.testing.assert_array_equal(R.length_regulator_bwd_ref(gp, dur), ref)
    m, a = R.length_regulator_bwd_terms(gp, dur)
    assert not np.isnan(a).any() and np.array_equal(m[:, :, 0], dur) and np.all(a >= np.abs(ref) - 1e-12)


def test_sum_bound_terms():
    assert R.sum_bound(1, 0.0, 0.0, 24) == 0.0
    b = R.sum_bound(np.array([4.0]), np.array([8.0]), np.array([-2.0]), 11)
    assert b[0] == 4 * 2.0 ** -24 * 8 + 2.0 ** -11 * 2
    assert R.SIGNIFICAND_BITS == {"float32": 24, "float16": 11, "bfloat16": 8}
