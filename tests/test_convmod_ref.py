"""tests/util_convmod_ref.py (the numpy float64 restatement the GPU tests of the convolution-module operator measure against) pinned to
torch's own float64 autograd on the CPU: F.conv1d(groups=C) -> F.batch_norm(training=True) -> F.silu, every output and gradient to 1e-12
relative, and nn.BatchNorm1d's buffers after one step."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import util_convmod_ref as R

EPS = 1e-5


def rel(got, ref):
    return float(np.abs(np.asarray(got) - ref).max() / max(np.abs(ref).max(), 1e-300))


@pytest.mark.parametrize("shape", R.EDGE_SHAPES + [(3, 2 * R.TIME_TILE * R.CHUNK_TILES + 5, 8, 7)], ids=lambda s: "B%d-T%d-C%d-K%d" % s)
def test_reference_matches_torch_float64_autograd(shape):
    B, T, C, K = shape
    x, w, gamma, beta, gy, rm, rv = R.inputs(11 + T + K, B, T, C, K)
    tx = torch.from_numpy(x).requires_grad_()
    tw = torch.from_numpy(w).view(C, 1, K).clone().requires_grad_()
    tg = torch.from_numpy(gamma).requires_grad_()
    tb = torch.from_numpy(beta).requires_grad_()
    trm, trv = torch.from_numpy(rm).clone(), torch.from_numpy(rv).clone()
    z = F.conv1d(tx.transpose(1, 2), tw, None, 1, (K - 1) // 2, 1, C)
    y = F.silu(F.batch_norm(z, trm, trv, tg, tb, True, 0.1, EPS)).transpose(1, 2)
    dx, dw, dg, db = torch.autograd.grad(y, [tx, tw, tg, tb], torch.from_numpy(gy))
    f = R.forward(x, w, gamma, beta, EPS, rm, rv, 0.1)
    g = R.backward(x, w, gamma, beta, EPS, gy)
    figs = dict(y=rel(f["y"], y.detach().numpy()), running_mean=rel(f["running_mean"], trm.numpy()), running_var=rel(f["running_var"], trv.numpy()),
                dx=rel(g["dx"], dx.numpy()), dw=rel(g["dw"], dw.view(C, K).numpy()), dgamma=rel(g["dgamma"], dg.numpy()),
                dbeta=rel(g["dbeta"], db.numpy()))
    print("convmod-ref", shape, {k: "%.2e" % v for k, v in figs.items()})
    for name, v in figs.items():
        assert v <= 1e-12, (name, v)


@pytest.mark.parametrize("track", [True, False])
def test_reference_matches_batchnorm1d_buffers_after_one_step(track):
    B, T, C, K = 3, 21, 8, 15
    x, w, gamma, beta, gy, rm, rv = R.inputs(5, B, T, C, K)
    bn = torch.nn.BatchNorm1d(C, eps=EPS, momentum=0.1, track_running_stats=track).double().train()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(gamma)); bn.bias.copy_(torch.from_numpy(beta))
        if track:
            bn.running_mean.copy_(torch.from_numpy(rm)); bn.running_var.copy_(torch.from_numpy(rv))
    z = torch.from_numpy(R.depthwise(x, w)).transpose(1, 2)
    y = F.silu(bn(z)).transpose(1, 2)
    f = R.forward(x, w, gamma, beta, EPS, rm if track else None, rv if track else None, 0.1)
    assert rel(f["y"], y.detach().numpy()) <= 1e-12
    if track:
        assert rel(f["running_mean"], bn.running_mean.numpy()) <= 1e-12 and rel(f["running_var"], bn.running_var.numpy()) <= 1e-12
        assert int(bn.num_batches_tracked) == 1
    else:
        assert f["running_mean"] is None and f["running_var"] is None and bn.running_mean is None
