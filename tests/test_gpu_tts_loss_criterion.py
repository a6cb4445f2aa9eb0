"""GPU: S2SDAGFastSpeech2Loss with the TTS-loss operator switched on against the same criterion on its torch lines (set_tts_loss_hip(False)),
in training mode after the same seeds.  Tolerances and their reason are those of tests/test_s2s_criterion_golden.py: loss and float logging
outputs to rel 3e-5, the total gradient norm to 3e-4, sampled tensors to 3e-4 * max|ref| (ten times that for tensors of at most 4 elements:
global scalars are one cancelling sum that moves run to run).  A counter on tts_losses_checked shows that the operator ran."""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LOG_F = ("loss", "dag-loss", "tts-loss", "l1-loss", "dur-loss", "pitch-loss", "energy-loss")


def _model(postnet):
    if not postnet:
        from tests.test_gpu_model import small_model
        return small_model()
    from daspeech_amd.models.daspeech import S2SConformerDAGFastSpeech2Model
    torch.manual_seed(0)
    return S2SConformerDAGFastSpeech2Model(encoder_layers=2, decoder_layers=1, tts=dict(enc_layers=1, dec_layers=1, add_postnet=True)).cuda()


def _run(m, sample, strategy, on):
    from daspeech_amd import decode_ops
    from daspeech_amd.criterions import S2SDAGFastSpeech2Loss
    calls = []
    checked = decode_ops.tts_losses_checked

    def counted(*a):
        calls.append(a[1] is not None)
        return checked(*a)
    old = decode_ops.set_tts_loss_hip(on)
    decode_ops.tts_losses_checked = counted
    try:
        m.zero_grad(set_to_none=True)
        crit = S2SDAGFastSpeech2Loss(glat_p="0.5", glance_strategy="number-random", tts_loss_weight=5.0, training_strategy=strategy)
        crit.train()
        random.seed(1234)                                        # the model draws the seed of its two GLAT passes from Python's generator
        torch.manual_seed(1234)
        torch.cuda.manual_seed(1234)
        loss, _, log = crit(m, sample)
        loss.backward()
    finally:
        decode_ops.tts_losses_checked = checked
        decode_ops.set_tts_loss_hip(old)
    grads = {k: p.grad.detach().double().cpu().numpy() for k, p in m.named_parameters() if p.grad is not None}
    return float(loss.detach()), {k: float(log[k]) for k in LOG_F}, grads, calls


@pytest.mark.parametrize("strategy,postnet", [("expect", False), ("argmax", False), ("expect", True)])
def test_criterion_with_the_operator_vs_its_torch_lines(strategy, postnet):
    from daspeech_amd.synthetic import make_s2st_batch
    m = _model(postnet).train()
    s = make_s2st_batch(3, "cuda", seed=1, min_frames=120, max_frames=200)
    s["update_num"] = 1000
    loss_ref, log_ref, g_ref, calls = _run(m, s, strategy, False)
    assert calls == []
    loss, log, g, calls = _run(m, s, strategy, True)
    assert calls == [postnet]                                    # the operator ran, once, with the second L1 term where the model has a postnet
    assert np.isfinite(loss) and loss == pytest.approx(loss_ref, rel=3e-5)
    for k in LOG_F:
        assert log[k] == pytest.approx(log_ref[k], rel=3e-5, abs=1e-7), k
    assert sorted(g) == sorted(g_ref) and len(g) > 50
    total = float(np.sqrt(sum((x ** 2).sum() for x in g.values())))
    total_ref = float(np.sqrt(sum((x ** 2).sum() for x in g_ref.values())))
    assert total == pytest.approx(total_ref, rel=3e-4)
    keys = sorted(g_ref)
    for key in keys[:: max(len(keys) // 24, 1)] + [k for k in keys if g_ref[k].size <= 4 or k.startswith("tts.postnet.")]:
        ref, got = g_ref[key], g[key]
        w = 10.0 if ref.size <= 4 else 1.0
        assert np.abs(got - ref).max() <= 3e-4 * w * np.abs(ref).max() + 1e-7 * total_ref, (key, np.abs(got - ref).max(), np.abs(ref).max())
