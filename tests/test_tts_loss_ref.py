"""CPU: the float64 reference of the TTS-loss operator against the criterion's own torch lines in float64 — the formulas, F_ = min(F, Fa), the
clamps of the lengths and n_mel / n_src — and the derived bound of the forward's error (tests/util_tts_loss_ref.py)."""
import math

import pytest
import torch

from tests import util_tts_loss_ref as U


CASES = [
    # B, F, Fa, C, N, audio lengths, src lengths
    (3, 7, 9, 80, 5, [2, 1, 9], [3, 1, 5]),              # a length beyond F_ is clamped
    (2, 9, 7, 5, 6, [7, 4], [6, 2]),                     # F > Fa
    (4, 33, 33, 8, 65, None, None),
    (1, 1, 1, 1, 1, None, None),
    (3, 12, 12, 16, 9, [0, 5, 12], [0, 9, 4]),           # an empty utterance among others
]


@pytest.mark.parametrize("post", [False, True])
@pytest.mark.parametrize("shape", CASES)
def test_reference_is_the_criterions_lines_in_float64(shape, post):
    B, F, Fa, C, N, al, sl = shape
    case = U.make_case(B, F, Fa, C, N, al, sl, dtype=torch.float64, seed=B * 100 + N, post=post)
    ref = U.reference_f64(case)
    got = U.torch_lines(*U.args_of(case))
    for name, r, t in zip(U.LOSSES, ref, got):
        assert float(t) == pytest.approx(r, rel=1e-12), name


def test_reference_of_nothing_is_nan_as_torchs_mean():
    case = U.make_case(2, 4, 4, 8, 3, [0, 0], [0, 0], dtype=torch.float64)
    ref = U.reference_f64(case)
    got = U.torch_lines(*U.args_of(case))
    assert all(math.isnan(r) for r in ref) and all(math.isnan(float(t)) for t in got)


def test_reference_counts():
    """n_mel = C * sum_b min(len, F_), n_src = sum_b min(len, N): constant differences make the sums countable"""
    case = U.make_case(3, 7, 9, 4, 5, [0, 1, 9], [0, 1, 7], dtype=torch.float64)
    case["feat_out"] = case["target_audio"][:, :7] + 2.0
    case["feat_post"] = case["target_audio"][:, :7] - 1.0
    case["pitch_out"] = case["pitches"] + 3.0
    ref = U.reference_f64(case)
    assert ref[0] == pytest.approx(3.0, rel=1e-12) and ref[2] == pytest.approx(9.0, rel=1e-12)
    got = U.torch_lines(*U.args_of(case))
    assert float(got[0]) == pytest.approx(3.0, rel=1e-12) and float(got[2]) == pytest.approx(9.0, rel=1e-12)


def test_additions_on_longest_path():
    d = U.header_defines()
    R, E = d["DSP_TTSLOSS_CHUNK_ROWS"], d["DSP_TTSLOSS_CHUNK_ELEMS"]
    assert R >= 1 and E >= 64
    # one row of one element: the lane's single addition, two wave folds, one partial per tail thread, the four waves, the postnet term
    assert U.additions_on_longest_path(1, 1, 1, 1) == 1 + 6 + 1 + 6 + 3 + 1
    # grows with the chunk a lane walks and with the partials a tail thread walks, never shrinks
    prev = 0
    for F_ in (1, R // 2, R, R + 1, 300 * R):
        p = U.additions_on_longest_path(2, F_, 80, 7)
        assert p >= prev
        prev = p
    assert U.additions_on_longest_path(2, 300 * R, 80, 7) > U.additions_on_longest_path(2, R, 80, 7)
    # the C5 shape: the worst case of the derived bound stays inside the 3e-5 that tests/test_s2s_criterion_golden.py allows the losses
    path = U.additions_on_longest_path(32, 528, 80, 62)
    assert path <= 256
    assert (256 + 4) * 2.0 ** -24 < 1.6e-5 < 3e-5
    assert U.forward_bound(32, 528, 80, 62) == (path + 4) * 2.0 ** -24
