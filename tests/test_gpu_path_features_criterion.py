"""GPU: S2SDAGFastSpeech2Loss (training strategy argmax) with the path-features operator switched on against the same criterion on its torch
lines (set_path_features_hip(False)), in training mode after the same seeds.  Tolerances and their reason are those of
tests/test_gpu_tts_loss_criterion.py, i.e. of tests/test_s2s_criterion_golden.py: loss and float logging outputs to rel 3e-5, the total
gradient norm to 3e-4, sampled tensors to 3e-4 * max|ref| (ten times that for tensors of at most 4 elements: global scalars are one
cancelling sum that moves run to run).  A counter on path_features_checked shows that the operator ran."""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LOG_F = ("loss", "dag-loss", "tts-loss", "l1-loss", "dur-loss", "pitch-loss", "energy-loss")


def _run(m, sample, on):
    from daspeech_amd import decode_ops
    from daspeech_amd.criterions import S2SDAGFastSpeech2Loss
    calls = []
    checked = decode_ops.path_features_checked

    def counted(features, path, width, *a):
        calls.append((tuple(features.shape), width))
        return checked(features, path, width, *a)
    old = decode_ops.set_path_features_hip(on)
    decode_ops.path_features_checked = counted
    try:
        m.zero_grad(set_to_none=True)
        crit = S2SDAGFastSpeech2Loss(glat_p="0.5", glance_strategy="number-random", tts_loss_weight=5.0, training_strategy="argmax")
        crit.train()
        random.seed(1234)                                        # the model draws the seed of its two GLAT passes from Python's generator
        torch.manual_seed(1234)
        torch.cuda.manual_seed(1234)
        loss, _, log = crit(m, sample)
        loss.backward()
    finally:
        decode_ops.path_features_checked = checked
        decode_ops.set_path_features_hip(old)
    grads = {k: p.grad.detach().double().cpu().numpy() for k, p in m.named_parameters() if p.grad is not None}
    return float(loss.detach()), {k: float(log[k]) for k in LOG_F}, grads, calls


def test_argmax_criterion_with_the_operator_vs_its_torch_lines():
    from daspeech_amd.synthetic import make_s2st_batch
    from tests.test_gpu_model import small_model
    m = small_model().train()
    s = make_s2st_batch(3, "cuda", seed=1, min_frames=120, max_frames=200)
    s["update_num"] = 1000
    loss_ref, log_ref, g_ref, calls = _run(m, s, False)
    assert calls == []
    loss, log, g, calls = _run(m, s, True)
    assert len(calls) == 1 and calls[0][1] == s["target_text"].shape[1] - 1 == s["durations"].shape[1]      # the operator ran, once
    assert np.isfinite(loss) and loss == pytest.approx(loss_ref, rel=3e-5)
    for k in LOG_F:
        assert log[k] == pytest.approx(log_ref[k], rel=3e-5, abs=1e-7), k
    assert sorted(g) == sorted(g_ref) and len(g) > 50
    total = float(np.sqrt(sum((x ** 2).sum() for x in g.values())))
    total_ref = float(np.sqrt(sum((x ** 2).sum() for x in g_ref.values())))
    assert total == pytest.approx(total_ref, rel=3e-4)
    keys = sorted(g_ref)
    for key in keys[:: max(len(keys) // 24, 1)] + [k for k in keys if g_ref[k].size <= 4]:
        ref, got = g_ref[key], g[key]
        w = 10.0 if ref.size <= 4 else 1.0
        assert np.abs(got - ref).max() <= 3e-4 * w * np.abs(ref).max() + 1e-7 * total_ref, (key, np.abs(got - ref).max(), np.abs(ref).max())


def test_argmax_branch_holds_no_host_read_on_served_inputs():
    """the lines the operator replaces, on the criterion's own tensors: with the switch off they stop under set_sync_debug_mode("error") at
    the read of the widest count, with it on path_features_checked runs through — forward and backward"""
    from daspeech_amd import decode_ops
    from tests import util_path_features_ref as U
    B, L, C, T = 3, 96, 256, 14
    x = U.make_features(B, L, C, torch.float16, 1, "cuda").requires_grad_(True)
    on = torch.zeros((B, L), dtype=torch.bool)
    on[0, ::10], on[1, :6:5], on[2, ::8] = True, True, True      # 9, 1 and 11 vertices behind <bos>
    path = U.ranks_where(on).cuda()
    W = T - 1
    assert decode_ops.path_features_served(x, path, W)
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("error")
        out, pad, n = decode_ops.path_features_checked(x, path, W)
        out.float().sum().backward()
    finally:
        torch.cuda.set_sync_debug_mode(old)
    ref = U.backward_of(U.reference, x.detach(), path, W, torch.ones((B, W, C), dtype=torch.float16, device="cuda"))
    assert torch.equal(out.detach(), ref[0]) and torch.equal(pad, ref[1]) and torch.equal(n, ref[2]) and torch.equal(x.grad, ref[3])
    assert int(n.max()) < W and pad[:, -1].all()                 # a batch whose longest target is shorter than the padded width: all-pad columns
