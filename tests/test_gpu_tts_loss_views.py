"""GPU: decode_ops.tts_losses_autograd on what torch accepts but a fresh allocation never is (tests/util_views.py): a slice of a larger buffer
(row and batch pitch, unit column stride), a target at an odd storage offset, a transposed [B,N] prediction, an expanded (stride-0) target.
Each is served with its strides, or settled by a dense copy inside the raising function after tts_losses_served said no; the result agrees
with float64 within the derived bound of the forward and with the 4 x rule of the gradients, as the dense call does.  The test registers the
operator's public names in the table of tests/test_gpu_views.py (imported as pytest itself imports it, so the table filled is the table
read), where test_every_public_operator_has_a_row looks for them."""
import pytest
import torch

import test_gpu_views as TV
from tests import util_tts_loss_ref as U
from tests import util_views as V
from tests.util_4x_rule import check_4x, f64

pytestmark = pytest.mark.gpu

DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
SHAPE = (3, 37, 35, 80, 21)                                    # B, F, Fa, C, N: more than one chunk of rows, F > Fa
LENS = ([35, 0, 17], [21, 9, 0])


def _slice_of_larger(t):
    B, F, C = t.shape
    wide = torch.full((B, F + 3, C + 16), float("nan"), dtype=t.dtype, device=t.device)      # what lies around the slice is never to be read
    v = wide[:, :F, :C]
    v.copy_(t)
    return v


def _views(case):
    """name -> (the case with one tensor in another layout, what tts_losses_served answers)"""
    out = {}
    c = dict(case)
    c["feat_out"] = _slice_of_larger(case["feat_out"])
    assert c["feat_out"].stride() == ((37 + 3) * 96, 96, 1)
    out["slice_of_larger_buffer"] = (c, True)
    c = dict(case)
    c["target_audio"] = V.at_offset(case["target_audio"])
    assert c["target_audio"].data_ptr() % 16 and c["target_audio"].is_contiguous()
    out["target_at_odd_offset"] = (c, True)
    c = dict(case)
    c["pitch_out"] = V.via_transpose(case["pitch_out"])
    assert not c["pitch_out"].is_contiguous()
    out["transposed_prediction"] = (c, False)
    c = dict(case)
    c["target_audio"] = V.expanded(case["target_audio"], 0)
    assert c["target_audio"].stride(0) == 0
    out["expanded_target"] = (c, True)
    return out


@TV.covers("tts_losses_autograd", "tts_losses_served", "tts_losses_checked", "set_tts_loss_hip")
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_views_agree_with_the_dense_call(dtype):
    from daspeech_amd import decode_ops
    B, F, Fa, C, N = SHAPE
    case = U.make_case(B, F, Fa, C, N, *LENS, dtype=DTYPES[dtype], device="cuda", seed=11, post=True)
    case["target_audio"] = case["target_audio"][:1].repeat(B, 1, 1)          # constant along the batch: the expanded view has these values
    g = (torch.rand(4, generator=torch.Generator().manual_seed(6)) + 0.5).cuda()
    bound = U.forward_bound(B, min(F, Fa), C, N)
    ref_losses = U.reference_f64(case)
    tor = U.backward_of(U.torch_lines, U.with_grad(case), g)
    ref = {k: f64(v) for k, v in U.backward_of(U.torch_lines, U.with_grad(case, dtype=torch.float64), g.double())[1].items()}
    dense = U.backward_of(decode_ops.tts_losses_autograd, U.with_grad(case), g)
    for name, (c, served) in _views(case).items():
        for k in U.GRAD_NAMES:
            c[k] = c[k].detach().requires_grad_(True)                        # the view itself is the leaf: its layout stays
        assert decode_ops.tts_losses_served(*U.args_of(c)) is served, name
        losses, grads = U.backward_of(decode_ops.tts_losses_autograd, c, g)
        for i, lname in enumerate(U.LOSSES):
            assert abs(float(losses[i]) - ref_losses[i]) <= bound * abs(ref_losses[i]), (name, lname)
        check_4x(f"tts_loss view {name} {dtype}", grads, tor[1], ref)
        for k, v in grads.items():                                           # element-wise work: the layout does not change a gradient's bits
            assert torch.equal(v, dense[1][k]), (name, k)
        if served:
            assert torch.equal(losses[1:], dense[0][1:]), name               # the [B,N] sums do not depend on the mel tensors' layout
            with torch.no_grad():                                            # what the criterion calls after `served` said yes: the same launch
                assert torch.equal(decode_ops.tts_losses_checked(*U.args_of(c)), losses), name
            old = decode_ops.set_tts_loss_hip(False)
            try:
                assert old is True and decode_ops.tts_losses_served(*U.args_of(c)) is False
            finally:
                assert decode_ops.set_tts_loss_hip(old) is False
