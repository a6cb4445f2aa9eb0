"""GPU: decode_ops.tts_losses_autograd (csrc/tts_loss_train.hip) against float64 and against the criterion's torch lines in the same dtype.

The forward's bound is derived, not measured (tests/util_tts_loss_ref.py: forward_bound); the gradients follow the 4 x rule of the training
operators (tests/util_4x_rule.py).  Shapes: the smallest at which the kernels take another path — empty and one-row utterances, a channel
count off the 16-byte grid (scalar path), one row past a chunk, one element past a wave, F > Fa, a single element, and a batch of nothing."""
import functools
import math

import pytest
import torch

from tests import util_tts_loss_ref as U
from tests.util_4x_rule import check_4x, f64

pytestmark = pytest.mark.gpu

CHUNK = U.header_defines()["DSP_TTSLOSS_CHUNK_ROWS"]
DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
CASES = {
    "empty_and_one_row": (3, 7, 9, 80, 5, [0, 1, 9], [0, 1, 5]),
    "scalar_chunk_edge": (2, CHUNK + 1, CHUNK + 1, 5, 65, None, None),
    "F_above_Fa": (2, 3 * CHUNK - 1, 2 * CHUNK, 80, 63, None, None),
    "smallest": (1, 1, 1, 1, 1, None, None),
    "nothing": (4, 40, 40, 80, 64, [0] * 4, [0] * 4),
}


def _case(name, dtype):
    B, F, Fa, C, N, al, sl = CASES[name]
    return U.make_case(B, F, Fa, C, N, al, sl, dtype=DTYPES[dtype], device="cuda", seed=len(name), post=True)


def _drop_post(case):
    out = dict(case)
    out["feat_post"] = None
    return out


def _grad_weights():
    return (torch.rand(4, generator=torch.Generator().manual_seed(5)) * 1.5 + 0.5).cuda()


def _poison(case):
    """fill and free NaN tensors of the sizes the operator is about to ask the caching allocator for: its outputs, its gradients, its
    workspace — an element the kernels do not write then reads as NaN"""
    from daspeech_amd import _lib
    B, F, C = case["feat_out"].shape
    N = case["log_dur_out"].shape[1]
    dt = case["feat_out"].dtype
    nbytes = int(_lib.load().dsp_tts_loss_workspace_bytes(B, min(F, case["target_audio"].shape[1]), N))
    junk = [torch.full((B, F, C), float("nan"), dtype=dt, device="cuda") for _ in range(2)]
    junk += [torch.full((B, N), float("nan"), dtype=dt, device="cuda") for _ in range(3)]
    junk += [torch.full((n,), float("nan"), dtype=torch.float32, device="cuda") for n in (4, 2, 4, max(nbytes // 4, 1))]
    del junk


def _hip(case, g, names=U.GRAD_NAMES):
    from daspeech_amd import decode_ops
    c = U.with_grad(case, names)
    assert decode_ops.tts_losses_served(*U.args_of(c))
    _poison(c)
    return U.backward_of(decode_ops.tts_losses_autograd, c, g)


@functools.lru_cache(maxsize=None)
def _results(name, dtype, post):
    """the operator, the torch lines in the same dtype and in float64 on one case: computed once, shared by the tests below"""
    case = _case(name, dtype)
    if not post:
        case = _drop_post(case)
    g = _grad_weights()
    hip = _hip(case, g)
    tor = U.backward_of(U.torch_lines, U.with_grad(case), g)
    ref = U.backward_of(U.torch_lines, U.with_grad(case, dtype=torch.float64), g.double())
    return {"case": case, "g": g, "hip": hip, "torch": tor, "ref": (U.reference_f64(case), {k: f64(v) for k, v in ref[1].items()})}


PARAMS = [(n, d, p) for n in CASES for d in DTYPES for p in (True, False)]


@pytest.mark.parametrize("name,dtype,post", PARAMS)
def test_forward_within_the_derived_bound(name, dtype, post):
    r = _results(name, dtype, post)
    B, F, Fa, C, N = CASES[name][:5]
    bound = U.forward_bound(B, min(F, Fa), C, N)
    losses = r["hip"][0]
    assert losses.dtype == torch.float32 and tuple(losses.shape) == (4,)
    for i, lname in enumerate(U.LOSSES):
        got, ref, tor = float(losses[i]), r["ref"][0][i], float(r["torch"][0][i])
        print(f"tts_loss {name} {dtype} post={post} {lname}: hip {got!r} f64 {ref!r} rel {abs(got - ref) / abs(ref) if ref else 0:.3e} bound {bound:.3e}")
        if math.isnan(ref):
            assert name == "nothing" and math.isnan(got) and math.isnan(tor), lname        # 0 / 0, as torch's mean of nothing
        else:
            assert abs(got - ref) <= bound * abs(ref), (lname, got, ref, bound)


@pytest.mark.parametrize("name,dtype,post", PARAMS)
def test_gradients_follow_the_4x_rule_and_are_fully_written(name, dtype, post):
    r = _results(name, dtype, post)
    hip, tor, ref = r["hip"][1], r["torch"][1], r["ref"][1]
    assert sorted(hip) == sorted(ref) == sorted(k for k in U.GRAD_NAMES if post or k != "feat_post")
    for k, v in hip.items():
        assert v.dtype == DTYPES[dtype] and v.shape == r["case"][k].shape
    check_4x(f"tts_loss {name} {dtype} post={post}", hip, tor, ref)      # (asserts that no element reads as the allocator's NaN)
    # exact zeros outside the lengths and on the rows F_ .. F-1
    case = r["case"]
    B, F, Fa, C, N = CASES[name][:5]
    F_ = min(F, Fa)
    for b in range(B):
        m = min(int(case["audio_lens"][b]), F_)
        s = min(int(case["src_lens"][b]), N)
        for k, v in hip.items():
            tail = v[b, m:] if v.dim() == 3 else v[b, s:]
            assert not tail.any(), (k, b)
    if name == "nothing":
        assert all(not v.any() for v in hip.values())


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_two_calls_give_the_same_bits(dtype):
    for name in ("empty_and_one_row", "F_above_Fa"):
        r = _results(name, dtype, True)
        losses, grads = _hip(r["case"], r["g"])
        assert torch.equal(losses.view(torch.int32), r["hip"][0].view(torch.int32))
        for k, v in grads.items():
            assert torch.equal(v, r["hip"][1][k]), k


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_leaving_outputs_out_keeps_the_bits_of_the_rest(dtype):
    r = _results("F_above_Fa", dtype, True)
    full_losses, full = r["hip"]
    for names in (("pitch_out",), ("feat_out", "energy_out"), ("feat_post", "log_dur_out")):
        losses, grads = _hip(r["case"], r["g"], names)
        assert sorted(grads) == sorted(names)
        assert torch.equal(losses, full_losses)
        for k in names:
            assert torch.equal(grads[k], full[k]), (names, k)
    # without feat_post: only l1 changes
    losses, grads = _hip(_drop_post(r["case"]), r["g"])
    assert torch.equal(losses[1:], full_losses[1:]) and float(losses[0]) < float(full_losses[0])
    assert sorted(grads) == sorted(k for k in U.GRAD_NAMES if k != "feat_post")
    for k, v in grads.items():
        assert torch.equal(v, full[k]), k


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_non_finite_inputs_propagate_as_in_torch(dtype):
    base = _case("empty_and_one_row", dtype)
    g = _grad_weights()
    case = dict(base)
    case["feat_out"] = base["feat_out"].clone()
    case["feat_out"][2, 3, 17] = float("inf")
    losses, grads = _hip(case, g)
    assert math.isinf(float(losses[0])) and float(losses[0]) > 0 and torch.isfinite(losses[1:]).all()
    assert all(torch.isfinite(v).all() for v in grads.values())
    case = dict(base)
    case["pitch_out"] = base["pitch_out"].clone()
    case["pitch_out"][2, 1] = float("nan")
    losses, grads = _hip(case, g)
    assert math.isnan(float(losses[2])) and torch.isfinite(losses[[0, 1, 3]]).all()
    nan = torch.isnan(grads["pitch_out"])
    assert bool(nan[2, 1]) and int(nan.sum()) == 1
    assert all(torch.isfinite(v).all() for k, v in grads.items() if k != "pitch_out")
    # a NaN beyond the lengths is never read
    case = dict(base)
    case["target_audio"] = base["target_audio"].clone()
    case["target_audio"][1, 1:] = float("nan")
    case["pitches"] = base["pitches"].clone()
    case["pitches"][1, 1:] = float("nan")
    ref = _results("empty_and_one_row", dtype, True)["hip"]
    losses, grads = _hip(case, g)
    assert torch.equal(losses, ref[0]) and all(torch.equal(v, ref[1][k]) for k, v in grads.items())


def test_no_host_wait_in_forward_or_backward():
    from daspeech_amd import decode_ops
    case = _case("empty_and_one_row", "fp16")
    g = _grad_weights()
    hip_in, tor_in = U.with_grad(case), U.with_grad(case)
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    control = None
    try:
        torch.cuda.set_sync_debug_mode("error")
        U.backward_of(decode_ops.tts_losses_autograd, hip_in, g)
        try:
            U.backward_of(U.torch_lines, tor_in, g)
        except RuntimeError as e:
            control = str(e)
    finally:
        torch.cuda.set_sync_debug_mode(old)
    if control is None:
        pytest.skip("the control (boolean-mask selections under set_sync_debug_mode('error')) does not raise on this torch build")
    assert "synchroniz" in control
    assert torch.isfinite(hip_in["feat_out"].grad).all()


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_without_gradient_nothing_is_recorded(dtype):
    from daspeech_amd import decode_ops
    r = _results("scalar_chunk_edge", dtype, True)
    with torch.no_grad():
        losses = decode_ops.tts_losses_autograd(*U.args_of(U.with_grad(r["case"])))
    assert losses.grad_fn is None and not losses.requires_grad and torch.equal(losses, r["hip"][0])
    losses = decode_ops.tts_losses_autograd(*U.args_of(r["case"]))          # no input requires grad
    assert losses.grad_fn is None and not losses.requires_grad and torch.equal(losses, r["hip"][0])


def test_gates_on_gpu_tensors():
    from daspeech_amd import decode_ops
    case = _case("smallest", "fp16")
    assert decode_ops.tts_losses_served(*U.args_of(case))
    with torch.autocast("cuda", dtype=torch.float16):
        assert not decode_ops.tts_losses_served(*U.args_of(case))
    old = decode_ops.set_tts_loss_hip(False)
    try:
        assert not decode_ops.tts_losses_served(*U.args_of(case))
    finally:
        decode_ops.set_tts_loss_hip(old)
    for key in ("audio_lens", "src_lens", "durations"):                      # int32 lengths and durations, also mixed with int64
        c = dict(case)
        c[key] = case[key].to(torch.int32)
        assert decode_ops.tts_losses_served(*U.args_of(c))
        assert torch.equal(decode_ops.tts_losses_autograd(*U.args_of(c)), decode_ops.tts_losses_autograd(*U.args_of(case))), key
