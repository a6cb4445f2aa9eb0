"""CPU: the float64 restatement of the channels-last Conv1d training operator (tests/util_conv1d_train_ref.py: explicit shifted slices, no
autograd) against float64 autograd of F.conv1d on the transposed tensors, to 1e-11 — so that the GPU tests compare the kernels with formulas
that are known to be the convolution's."""
import pytest
import torch

from tests import util_conv1d_train_ref as A

# (B, T, Cin, Cout, K): one frame, one frame under nine taps, T < K twice, several tiles of nothing in particular
CASES = [(1, 1, 64, 64, 1), (1, 1, 64, 64, 9), (2, 2, 64, 128, 3), (3, 5, 128, 64, 9), (3, 33, 64, 64, 5)]


def _close(got, want):
    scale = max(float(want.abs().max()), 1e-300)
    assert float((got - want).abs().max()) <= 1e-11 * scale


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("case", CASES, ids=["B%d-T%d-%dto%d-K%d" % c for c in CASES])
def test_restatement_is_float64_autograd_of_conv1d(case, with_bias):
    B, T, Cin, Cout, K = case
    t = A.inputs(11 + T + K, B, T, Cin, Cout, K)
    bias = t["bias"] if with_bias else None
    want = A.torch_lines(t["x"], t["w"], bias, t["dy"])
    _close(A.forward(t["x"], t["w"], bias), want["y"])
    got = A.backward(t["x"], t["w"], t["dy"])
    _close(got["dx"], want["dx"])
    _close(got["dw"], want["dw"])
    if with_bias:
        _close(got["db"], want["db"])
    else:
        assert "db" not in want


def test_a_tap_never_reads_the_neighbouring_sample():
    """sample 1 of a batch computed alone gives what it gives in the batch"""
    t = A.inputs(5, 3, 5, 64, 64, 9)
    y = A.forward(t["x"], t["w"], t["bias"])
    assert torch.equal(A.forward(t["x"][1:2], t["w"], t["bias"]), y[1:2])
    g, g1 = A.backward(t["x"], t["w"], t["dy"]), A.backward(t["x"][1:2], t["w"], t["dy"][1:2])
    assert torch.equal(g1["dx"], g["dx"][1:2])
