"""dag_logsoftmax_gather_inplace on float64 logits (csrc/logsoftmax_gather_f64.hip) against the project's fp64 CPU oracle: the three forward
modes, the backward from the stored softmax and from the lazy row statistics, the chain gather -> dag_loss -> backward / dag_best_alignment,
the criterion's route, and agreement with the fp32 kernels.

Tolerances are the ones tests/test_dag_double.py holds the double DP to: 1e-12 / 1e-12 on values, rtol 1e-12 / atol 1e-11 on the loss,
rtol 1e-9 / atol 1e-12 on gradients.  An independent double implementation with another summation order (torch's CPU
log_softmax(float64).gather and its autograd) differs from the oracle by < 3e-14 on these shapes; an fp32 computation misses every bound."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import dag_oracle as orc
from tests.util_inputs import make_dag_inputs

pytestmark = pytest.mark.gpu

B = 3
# (V, S, L): duplicate indices (S > distinct targets at V = 37), odd / even row alignment, the register-width boundary of the fp32 design
# (8192), rows wider than an LDS image of doubles (20000, 33000); L = 50 is not a multiple of 4, one case with L = 48
CASES = [(37, 17, 50), (512, 17, 50), (1000, 17, 50), (8192, 40, 50), (10001, 17, 50), (20000, 17, 50), (33000, 9, 50), (512, 17, 48)]


def dev():
    return torch.device("cuda:0")


def ops():
    from daspeech_amd import custom_ops
    return custom_ops


def _inputs(V, S, L):
    """As test_gpu_dag_ops.py::test_oracle_logsoftmax_gather, in double, with three -inf logits in row (0, 0), one of them gathered."""
    rng = np.random.default_rng(V)
    x = rng.standard_normal((B, L, V)) * 3
    tgt = rng.integers(0, V, (B, S))
    c = int(tgt[0, 0])
    for col in (c, (c + 1) % V, (c + V // 2) % V):
        x[0, 0, col] = -np.inf
    idx = np.broadcast_to(tgt[:, None, :], (B, L, S))
    return rng, x, tgt, idx


def _check_match(match, ref, L, S):
    assert match.dtype == torch.float64 and tuple(match.shape) == (B, L, S)
    assert match.transpose(1, 2).is_contiguous()
    got = match.detach().cpu().numpy()
    assert np.isneginf(ref).any()
    assert np.array_equal(np.isneginf(got), np.isneginf(ref)) and not np.isnan(got).any() and not np.isposinf(got).any()
    fin = np.isfinite(ref)
    err = np.abs(got[fin] - ref[fin]).max()
    print(f"match: max abs error {err:.3e}")
    np.testing.assert_allclose(got[fin], ref[fin], rtol=1e-12, atol=1e-12)


@pytest.fixture
def lazy_mode(request):
    prev = ops().set_lazy_softmax(request.param)
    yield request.param
    ops().set_lazy_softmax(prev)


@pytest.mark.parametrize("lazy_mode", [False, True], indirect=True, ids=["eager", "lazy"])
@pytest.mark.parametrize("V,S,L", CASES)
def test_forward_with_gradient_matches_the_fp64_oracle(V, S, L, lazy_mode):
    rng, x, tgt, idx = _inputs(V, S, L)
    ref, sm = orc.logsoftmax_gather(x, idx, np.float64, want_softmax=True)
    xt = torch.from_numpy(x).to(dev()).requires_grad_()
    work = xt.clone()
    tg = torch.from_numpy(tgt).to(dev())
    ptr = work.data_ptr()
    out_x, match = ops().dag_logsoftmax_gather_inplace(work, tg.unsqueeze(1).expand(-1, L, -1))
    _check_match(match, ref, L, S)
    assert out_x.data_ptr() == ptr and out_x.dtype == torch.float64
    if lazy_mode:
        assert np.array_equal(out_x.detach().cpu().numpy(), x)                      # logits untouched, bit for bit
    else:
        got_sm = out_x.detach().cpu().numpy()
        print(f"softmax: max abs error {np.abs(got_sm - sm).max():.3e}")
        np.testing.assert_allclose(got_sm, sm, rtol=0, atol=1e-12)
        assert (got_sm[0, 0][np.isneginf(x[0, 0])] == 0).all()


@pytest.mark.parametrize("V,S,L", CASES)
def test_forward_without_gradient_writes_nothing_but_match(V, S, L):
    rng, x, tgt, idx = _inputs(V, S, L)
    ref = orc.logsoftmax_gather(x, idx, np.float64)
    tg = torch.from_numpy(tgt).to(dev())
    work = torch.from_numpy(x).to(dev())
    out_x, match = ops().dag_logsoftmax_gather_inplace(work, tg.unsqueeze(1).expand(-1, L, -1))
    _check_match(match, ref, L, S)
    assert out_x.data_ptr() == work.data_ptr() and np.array_equal(work.cpu().numpy(), x)
    # a materialised (non-expanded) index tensor gives the same bits
    _, match2 = ops().dag_logsoftmax_gather_inplace(torch.from_numpy(x).to(dev()), tg.unsqueeze(1).expand(-1, L, -1).contiguous())
    assert torch.equal(match2, match)


@pytest.mark.parametrize("lazy_mode", [False, True], indirect=True, ids=["eager", "lazy"])
@pytest.mark.parametrize("V,S,L,go_kind", [(V, S, L, "dense") for V, S, L in CASES] + [(1000, 17, 50, "strided"), (10001, 17, 50, "float32"),
                                                                                      (20000, 17, 50, "strided")])
def test_backward_matches_the_fp64_oracle(V, S, L, go_kind, lazy_mode):
    rng, x, tgt, idx = _inputs(V, S, L)
    _, sm = orc.logsoftmax_gather(x, idx, np.float64, want_softmax=True)
    w = rng.standard_normal((B, L, S))
    if go_kind == "float32":
        w = w.astype(np.float32).astype(np.float64)                                # exactly representable: widening loses nothing
    gref = orc.logsoftmax_gather_bwd(sm, idx, w, np.float64)
    xt = torch.from_numpy(x).to(dev()).requires_grad_()
    work = xt.clone()
    tg = torch.from_numpy(tgt).to(dev())
    out_x, match = ops().dag_logsoftmax_gather_inplace(work, tg.unsqueeze(1).expand(-1, L, -1))
    wt = torch.from_numpy(w).to(dev())
    if go_kind == "strided":
        wide = torch.zeros((B, L, 2 * S + 1), dtype=torch.float64, device=dev())
        go = wide[:, :, 1::2]
        go.copy_(wt)
        assert not go.is_contiguous()
    elif go_kind == "float32":
        go = wt.float()
    else:
        go = wt
    (gx,) = torch.autograd.grad([match], [xt], grad_outputs=[go])
    assert gx.dtype == torch.float64
    got = gx.cpu().numpy()
    print(f"gradient: max abs error {np.abs(got - gref).max():.3e}")
    np.testing.assert_allclose(got, gref, rtol=1e-9, atol=1e-12)
    # the gradient was written into the logits buffer, in both forms
    assert np.array_equal(out_x.detach().cpu().numpy(), got)


def test_backward_launch_widens_a_float32_gradient():
    """The launch helper itself: a float32, non-contiguous [B,L,S] gradient is widened to double (autograd may already have cast it)."""
    import sys
    import daspeech_amd.custom_ops  # noqa: F401
    dl = sys.modules["daspeech_amd.custom_ops.dag_loss"]           # (the package attribute of that name is the function)
    V, S, L = 1000, 17, 50
    rng, x, tgt, idx = _inputs(V, S, L)
    _, sm = orc.logsoftmax_gather(x, idx, np.float64, want_softmax=True)
    w32 = rng.standard_normal((B, S, L)).astype(np.float32)
    gref = orc.logsoftmax_gather_bwd(sm, idx, w32.transpose(0, 2, 1).astype(np.float64), np.float64)
    tg = torch.from_numpy(tgt).to(dev())
    buf = torch.from_numpy(sm).to(dev())
    g = torch.from_numpy(w32).to(dev()).transpose(1, 2)                            # [B,L,S] view of [B,S,L] float32
    out = dl._lsg64_backward(buf, tg.unsqueeze(1).expand(-1, L, -1), g)
    assert out.data_ptr() == buf.data_ptr()
    np.testing.assert_allclose(out.cpu().numpy(), gref, rtol=1e-9, atol=1e-12)


def _oracle_chain(x, tgt, links, ol, tl, grad_out=None):
    """logsoftmax_gather -> dag_alpha / dag_beta -> dag_grad -> logsoftmax_gather_bwd, all np.float64.
    -> (loss[B], d (sum_b grad_out_b * loss_b) / d logits, match [B,T,L])."""
    Bn, L, V = x.shape
    idx = np.broadcast_to(tgt[:, None, :], (Bn, L, tgt.shape[1]))
    m_bls, sm = orc.logsoftmax_gather(x, idx, np.float64, want_softmax=True)
    m = np.ascontiguousarray(m_bls.transpose(0, 2, 1))
    a = orc.dag_alpha(m, links, ol, tl, np.float64)
    b = orc.dag_beta(m, links, ol, tl, np.float64)
    loss = b[:, 0, 0].copy()
    go = np.ones(Bn) if grad_out is None else grad_out
    gm, _ = orc.dag_grad(go, a, b, m, links, ol, tl, np.float64)
    gx = orc.logsoftmax_gather_bwd(sm, idx, np.ascontiguousarray(gm.transpose(0, 2, 1)), np.float64)
    return loss, gx, m


def _chain_inputs(seed, Bn, T, L, TR, V):
    _, links, ol, tl = make_dag_inputs(seed, Bn, T, L, TR)
    rng = np.random.default_rng(1000 + seed)
    x = rng.standard_normal((Bn, L, V)) * 3
    tgt = rng.integers(0, V, (Bn, T))
    return x, tgt, links.astype(np.float64), ol, tl


CHAIN_CASES = [(5, 3, 40, 700, 32, 96), (6, 2, 25, 300, 299, 96)]        # banded, and a dense window


@pytest.mark.parametrize("seed,Bn,T,L,TR,V", CHAIN_CASES)
def test_chain_gather_dag_loss_backward_and_alignment(seed, Bn, T, L, TR, V):
    x, tgt, links, ol, tl = _chain_inputs(seed, Bn, T, L, TR, V)
    loss64, gx64, m64 = _oracle_chain(x, tgt, links, ol, tl)
    assert np.isfinite(loss64).all()
    xt = torch.from_numpy(x).to(dev()).requires_grad_()
    work = xt.clone()
    tg, kt, olt, tlt = (torch.from_numpy(a).to(dev()) for a in (tgt, links, ol, tl))
    _, match = ops().dag_logsoftmax_gather_inplace(work, tg.unsqueeze(1).expand(-1, L, -1))
    m_all = match.transpose(1, 2)
    assert m_all.dtype == torch.float64 and m_all.is_contiguous()
    loss = ops().dag_loss(m_all, kt, olt, tlt)
    assert loss.dtype == torch.float64 and "F64" in type(loss.grad_fn).__name__
    ln = loss.detach().cpu().numpy()
    print(f"loss: max abs error {np.abs(ln - loss64).max():.3e}")
    np.testing.assert_allclose(ln, loss64, rtol=1e-12, atol=1e-11)
    path = ops().dag_best_alignment(m_all.detach(), kt, olt, tlt)
    np.testing.assert_array_equal(path.cpu().numpy(), orc.dag_best_alignment(m64, links, ol, tl, np.float64))
    (gx,) = torch.autograd.grad(loss.sum(), [xt])
    assert gx.dtype == torch.float64
    print(f"d loss / d logits: max abs error {np.abs(gx.cpu().numpy() - gx64).max():.3e}")
    np.testing.assert_allclose(gx.cpu().numpy(), gx64, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("seed,Bn,T,L,TR,V", CHAIN_CASES)
def test_criterion_takes_double_logits(seed, Bn, T, L, TR, V):
    from daspeech_amd.criterions import NATDAGLoss
    import sys
    import daspeech_amd.custom_ops  # noqa: F401
    dl = sys.modules["daspeech_amd.custom_ops.dag_loss"]           # (the package attribute of that name is the function)
    x, tgt, links, ol, tl = _chain_inputs(seed, Bn, T, L, TR, V)
    loss64, gx64, _ = _oracle_chain(x, tgt, links, ol, tl, grad_out=-1.0 / (Bn * tl.astype(np.float64)))
    want = -(loss64 / tl).mean()
    xt = torch.from_numpy(x).to(dev()).requires_grad_()
    work = xt.clone()
    tg, kt, olt, tlt = (torch.from_numpy(a).to(dev()) for a in (tgt, links, ol, tl))
    out_mask = torch.arange(L, device=dev()).unsqueeze(0) < olt.unsqueeze(1)
    tgt_mask = torch.arange(T, device=dev()).unsqueeze(0) < tlt.unsqueeze(1)
    res = NATDAGLoss()._compute_dag_loss(work, out_mask, tg, tgt_mask, kt, model=SimpleNamespace(pad=1))
    assert dl.LAZY_SOFTMAX is False                                                 # the criterion ran the gather lazily and restored the mode
    assert np.array_equal(work.detach().cpu().numpy(), x)                           # ... so the logits are still the logits
    loss = res["loss"]
    assert loss.dtype == torch.float64 and int(res["invalid_nsentences"]) == 0
    np.testing.assert_allclose(float(loss.detach()), want, rtol=1e-12, atol=0)
    (gx,) = torch.autograd.grad(loss, [xt])
    print(f"criterion gradient: max abs error {np.abs(gx.cpu().numpy() - gx64).max():.3e}")
    np.testing.assert_allclose(gx.cpu().numpy(), gx64, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("V,S,L", CASES)
def test_double_and_fp32_kernels_agree_on_fp32_logits(V, S, L):
    """Two code paths for one function: the fp32 kernels on fp32 logits and the double kernels on their exact widening agree to the fp32
    oracle tolerance, while the double result keeps its own 1e-12 against the oracle."""
    rng, x, tgt, idx = _inputs(V, S, L)
    x32 = x.astype(np.float32)
    xw = x32.astype(np.float64)
    ref = orc.logsoftmax_gather(xw, idx, np.float64)
    tg = torch.from_numpy(tgt).to(dev())
    sel = tg.unsqueeze(1).expand(-1, L, -1)
    _, m32 = ops().dag_logsoftmax_gather_inplace(torch.from_numpy(x32).to(dev()), sel)
    _, m64 = ops().dag_logsoftmax_gather_inplace(torch.from_numpy(xw).to(dev()), sel)
    assert m32.dtype == torch.float32 and m64.dtype == torch.float64
    _check_match(m64, ref, L, S)
    a, b = m32.cpu().numpy().astype(np.float64), m64.cpu().numpy()
    assert np.array_equal(np.isneginf(a), np.isneginf(b))
    np.testing.assert_allclose(a, b, rtol=2e-6, atol=2e-6)
