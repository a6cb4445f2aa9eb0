"""CPU: the float64 restatement of the stride-2 channels-last Conv1d training operator (tests/util_conv1d_stride2_ref.py: explicit strided
slices, no autograd) against float64 autograd of F.conv1d(stride=2, padding=P) on the transposed tensors, to 1e-12 relative — so that the GPU
tests compare the kernels with formulas that are known to be the convolution's — and the structural facts the kernels rely on: T_out, the rows
of dx that no tap reaches, the taps of dW that never land inside a sample."""
import pytest
import torch

from tests import util_conv1d_stride2_ref as A

KS = (1, 3, 5, 15)
CASES = [(B, T, K) for K in KS for T in sorted({1, 2, 3, 4, K - 1, K, K + 1, 9} - {0}) for B in (1, 3)]
CIN, COUT = 16, 64


def _close(got, want):
    scale = max(float(want.abs().max()), 1e-300)
    assert got.shape == want.shape
    assert float((got - want).abs().max()) <= 1e-12 * scale


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("case", CASES, ids=["B%d-T%d-K%d" % c for c in CASES])
def test_restatement_is_float64_autograd_of_conv1d_stride2(case, with_bias):
    B, T, K = case
    t = A.inputs(11 + T + K, B, T, CIN, COUT, K)
    bias = t["bias"] if with_bias else None
    want = A.torch_lines(t["x"], t["w"], bias, t["dy"])
    assert want["y"].shape == (B, A.t_out(T), COUT)                          # T_out = (T - 1) // 2 + 1 is F.conv1d's own count
    _close(A.forward(t["x"], t["w"], bias), want["y"])
    got = A.backward(t["x"], t["w"], t["dy"])
    _close(got["dx"], want["dx"])
    _close(got["dw"], want["dw"])
    if with_bias:
        _close(got["db"], want["db"])
    else:
        assert "db" not in want


@pytest.mark.parametrize("T", [1, 2, 7, 8])
def test_one_tap_leaves_the_odd_rows_of_dx_exactly_zero(T):
    """K = 1: only the even input rows are read, so the odd rows of dx are zeros that a kernel has to WRITE — in torch's autograd too"""
    t = A.inputs(3, 2, T, CIN, COUT, 1)
    got, want = A.backward(t["x"], t["w"], t["dy"]), A.torch_lines(t["x"], t["w"], None, t["dy"])
    for dx in (got["dx"], want["dx"]):
        assert not dx[:, 1::2].any() and dx[:, 0::2].abs().min() > 0


@pytest.mark.parametrize("T,K,landing", [(1, 5, {2}), (1, 15, {7}), (2, 5, {2, 3}), (3, 15, {5, 6, 7, 8, 9}), (9, 5, {0, 1, 2, 3, 4})])
def test_taps_that_never_land_are_exactly_zero_in_dw(T, K, landing):
    """tap k lands when some 2t + k - P is inside [0, T): at T = 1, K = 5 that is the centre tap alone"""
    assert {k for k, _, _ in A.taps(T, K)} == landing
    t = A.inputs(4, 3, T, CIN, COUT, K)
    got, want = A.backward(t["x"], t["w"], t["dy"]), A.torch_lines(t["x"], t["w"], None, t["dy"])
    for dw in (got["dw"], want["dw"]):
        for k in range(K):
            assert bool(dw[:, :, k].any()) == (k in landing), k


def test_a_tap_never_reads_the_neighbouring_sample():
    """sample 1 of a batch computed alone gives what it gives in the batch"""
    t = A.inputs(5, 3, 6, CIN, COUT, 15)
    y = A.forward(t["x"], t["w"], t["bias"])
    assert torch.equal(A.forward(t["x"][1:2], t["w"], t["bias"]), y[1:2])
    g, g1 = A.backward(t["x"], t["w"], t["dy"]), A.backward(t["x"][1:2], t["w"], t["dy"][1:2])
    assert torch.equal(g1["dx"], g["dx"][1:2])
