"""CPU: pins tests/util_resnorm_ref.py — the float64 restatement the GPU tests measure the residual + dropout + LayerNorm kernels against —
to torch float64 autograd of   F.layer_norm(res + alpha * (h + bias) * keep / (1 - p), ...)   at 1e-12, its Philox4x32-10 to the published
known answers (Random123 kat_vectors), and the mask threshold rule."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import util_resnorm_ref as R

EPS = 1e-5
TOL = 1e-12


def rel(got, ref):
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


@pytest.mark.parametrize("shape", [(1, 8), (3, 72), (17, 256), (5, 2048)])
@pytest.mark.parametrize("p,alpha,with_bias", [(0.0, 1.0, True), (0.1, 0.5, True), (0.1, 1.0, False), (0.5, 0.5, False)])
def test_restatement_matches_torch_float64_autograd(shape, p, alpha, with_bias):
    Rr, C = shape
    a = R.inputs(11 * Rr + C, Rr, C)
    keep = None if p == 0 else R.keep_mask(5, 8, p, Rr * C).reshape(Rr, C)
    bias = a["bias"] if with_bias else None
    f = R.forward(a["h"], a["residual"], bias, a["gamma"], a["beta"], EPS, alpha, p, keep)
    g = R.backward(f["s"], a["gamma"], EPS, alpha, p, keep, a["dy"], a["ds"])
    t = {k: torch.from_numpy(v).requires_grad_() for k, v in a.items() if k in ("h", "residual", "bias", "gamma", "beta")}
    z = t["h"] + (t["bias"] if with_bias else 0.0)
    if keep is not None:
        z = z * torch.from_numpy(keep).to(torch.float64) / (1.0 - p)
    s = t["residual"] + alpha * z
    y = F.layer_norm(s, (C,), t["gamma"], t["beta"], EPS)
    wrt = [t["h"], t["residual"], t["gamma"], t["beta"]] + ([t["bias"]] if with_bias else [])
    grads = torch.autograd.grad([y, s], wrt, [torch.from_numpy(a["dy"]), torch.from_numpy(a["ds"])], retain_graph=True)
    assert rel(f["s"], s.detach().numpy()) <= TOL and rel(f["y"], y.detach().numpy()) <= TOL
    names = ["dh", "dresidual", "dgamma", "dbeta"] + (["dbias"] if with_bias else [])
    for name, gt in zip(names, grads):
        assert rel(g[name], gt.numpy()) <= TOL, name
    # y alone (post-norm) and s alone
    gy = R.backward(f["s"], a["gamma"], EPS, alpha, p, keep, a["dy"], None)
    ty = torch.autograd.grad(y, [t["h"], t["residual"]], torch.from_numpy(a["dy"]), retain_graph=True)
    assert rel(gy["dh"], ty[0].numpy()) <= TOL and rel(gy["dresidual"], ty[1].numpy()) <= TOL
    gs = R.backward(f["s"], a["gamma"], EPS, alpha, p, keep, None, a["ds"])
    ts = torch.autograd.grad(s, [t["h"], t["residual"]], torch.from_numpy(a["ds"]), retain_graph=True)
    assert rel(gs["dh"], ts[0].numpy()) <= TOL and rel(gs["dresidual"], ts[1].numpy()) <= TOL
    assert not gs["dgamma"].any() and not gs["dbeta"].any()


def test_plain_layer_norm_form():
    a = R.inputs(3, 7, 40)
    f = R.forward(None, a["residual"], None, a["gamma"], a["beta"], EPS, 1.0, 0.0, None)
    g = R.backward(f["s"], a["gamma"], EPS, 1.0, 0.0, None, a["dy"], None, has_h=False)
    x = torch.from_numpy(a["residual"]).requires_grad_()
    w, b = torch.from_numpy(a["gamma"]).requires_grad_(), torch.from_numpy(a["beta"]).requires_grad_()
    y = F.layer_norm(x, (40,), w, b, EPS)
    gx, gw, gb = torch.autograd.grad(y, [x, w, b], torch.from_numpy(a["dy"]))
    assert np.array_equal(f["s"], a["residual"]) and rel(f["y"], y.detach().numpy()) <= TOL
    assert rel(g["dresidual"], gx.numpy()) <= TOL and rel(g["dgamma"], gw.numpy()) <= TOL and rel(g["dbeta"], gb.numpy()) <= TOL
    assert "dh" not in g


KAT = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


@pytest.mark.parametrize("counter,key,want", KAT)
def test_philox_known_answers(counter, key, want):
    got = R.philox4x32_10([np.array([c]) for c in counter], key)
    assert " ".join("%08x" % int(w[0]) for w in got) == want


def test_philox_is_elementwise_and_the_mask_reads_its_words_in_order():
    ctr = [np.array([0, 0xFFFFFFFF, 7]), np.array([0, 0xFFFFFFFF, 0]), np.array([0, 0xFFFFFFFF, 12]), np.array([0, 0xFFFFFFFF, 0])]
    one = R.philox4x32_10([c[:1] for c in ctr], (0, 0))
    many = R.philox4x32_10(ctr, (0, 0))
    assert all(int(a[0]) == int(b[0]) for a, b in zip(one, many))
    # seed 9 | 3 << 32, offset 12: element 4g + i is word i of counter (g, 0, 12, 0) under key (9, 3)
    seed, off, p = 9 | (3 << 32), 12, 0.5
    m = R.keep_mask(seed, off, p, 4 * 9 + 3)
    assert m.shape == (39,)
    for g in (0, 7, 9):
        w = R.philox4x32_10([np.array([g]), np.array([0]), np.array([12]), np.array([0])], (9, 3))
        for i in range(4):
            if 4 * g + i < 39:
                assert bool(m[4 * g + i]) == ((int(w[i][0]) >> 8) >= R.threshold(p))
    assert not np.array_equal(m, R.keep_mask(seed, off + 4, p, 39)) and not np.array_equal(m, R.keep_mask(seed + 1, off, p, 39))
    assert np.array_equal(m, R.keep_mask(seed, off, p, 39))
    big = 0x1_0000_0004                                                 # the high offset word is part of the counter
    assert not np.array_equal(R.keep_mask(seed, 4, p, 39), R.keep_mask(seed, big, p, 39))


def test_mask_threshold():
    assert R.threshold(0.0) == 0 and R.threshold(0.5) == 1 << 23
    assert R.threshold(0.1) == 1677722                                  # ceil(1677721.6)
    assert R.keep_mask(1, 0, 0.0, 1000).all()                           # p = 0 keeps everything
    # p just below 1: thr reaches 2^24 and never passes it, and a 24-bit word is at most 2^24 - 1: nothing is kept
    for p in (1.0 - 2.0 ** -25, 1.0 - 2.0 ** -53):
        assert R.threshold(p) == 1 << 24
        assert not R.keep_mask(1, 0, p, 4096).any()
    assert R.threshold(1.0 - 2.0 ** -24) == (1 << 24) - 1
    n = 200000
    for p in (0.1, 0.5):
        share = R.keep_mask(1234, 4, p, n).mean()
        assert abs(share - (1 - p)) <= 5 * np.sqrt(p * (1 - p) / n), (p, share)


def test_the_python_side_computes_the_same_threshold():
    from daspeech_amd import decode_ops
    for p in (0.0, 0.1, 0.25, 0.5, 1.0 - 2.0 ** -25):
        assert decode_ops.dropout_threshold(p) == R.threshold(p)
    assert decode_ops.RESNORM_CHUNK_ROWS == R.CHUNK_ROWS and decode_ops.RESNORM_MAX_C == R.MAX_C
    with pytest.raises(ValueError):
        decode_ops.dropout_threshold(1.0)
