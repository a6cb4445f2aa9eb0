"""CPU checks of the device optimizer state's update rule: its plain-float mirror (tests/util_optim_state_ref.py) against
fp16_trainer.DynamicLossScaler and the host lines of FP16FlatOptimizer._step_hip; the running-product bias corrections against 1 - b**t; the
slot indices of fp16_trainer against the header; and the surface of the device_scaler argument where no GPU is needed."""
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import util_optim_state_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_step(scaler, state, S, grad_mult, clip_norm, lr, betas, weight_decay):
    """the host arithmetic of FP16FlatOptimizer._step_hip after `S = float(self._S)`; state = {"t": applied steps}.
    -> (nv, applied, the doubles handed to dsp_fp16_optim_adam_step or None)"""
    c = grad_mult / scaler.loss_scale
    nv = abs(c) * math.sqrt(S) if S == S and S >= 0.0 else float("nan")
    if nv != nv or nv == float("inf"):
        scaler.overflow()
        return nv, False, None
    if clip_norm and nv > clip_norm:
        c *= clip_norm / (nv + 1e-6)
    t = state["t"] + 1
    b1, b2 = betas
    doubles = (c, lr, b1, b2, 1e-8, lr * weight_decay, 1.0 - b1 ** t, math.sqrt(1.0 - b2 ** t))
    state["t"] = t
    scaler.update()
    return nv, True, doubles


@pytest.mark.parametrize("scale_window", [2, 3])
def test_mirror_follows_the_host_scaler_and_step(scale_window):
    """The scripted S sequence, twice over (so that the window's growth and the overflows interleave): loss scale, iter, last overflow, the
    applied sequence and the norm are EQUAL; the doubles of an applied step are equal but for the two bias corrections, whose float
    roundings are (running product against pow: test_running_product_bias_corrections)."""
    from daspeech_amd.fp16_trainer import DynamicLossScaler
    lr, betas, wd, clip = 0.1, (0.9, 0.999), 0.01, 1.0
    scaler = DynamicLossScaler(init_scale=2.0 ** 7, scale_window=scale_window)
    st = {"t": 0}
    mir = M.MirrorState(lr, betas, 1e-8, wd, clip, init_scale=2.0 ** 7, scale_window=scale_window, grad_mult=0.5)
    applied_seq = []
    for S in M.S_SCRIPT + M.S_SCRIPT:
        nv, ok, doubles = _host_step(scaler, st, S, 0.5, clip, lr, betas, wd)
        got = mir.step(S)
        applied_seq.append(got)
        assert bool(got) is ok
        assert M.bits(mir.grad_norm) == M.bits(nv)
        assert mir.loss_scale == scaler.loss_scale and mir.iter == scaler._iter and mir.last_overflow_iter == scaler._last_overflow_iter
        assert mir.t == st["t"] and mir.loss_scale_f32 == np.float32(scaler.loss_scale)
        if ok:
            assert mir.doubles[:6] == doubles[:6]
            assert np.float32(mir.doubles[1] / mir.doubles[6]) == np.float32(doubles[1] / doubles[6])
            assert np.float32(mir.doubles[7]) == np.float32(doubles[7])
    assert applied_seq == [1, 1, 0, 0, 0, 1] * 2
    assert mir.floor_hit == 0


def test_mirror_clips_and_sets_the_floor_flag():
    mir = M.MirrorState(0.1, clip_norm=1.0, init_scale=4.0, min_loss_scale=1.0)
    assert mir.step(1.0e9) == 1 and mir.grad_norm > 1.0
    assert float(mir.scalars[0]) == pytest.approx(0.25 / (mir.grad_norm + 1e-6), rel=1e-6)      # c: unscale times the clip coefficient
    assert mir.step(float("inf")) == 0 and mir.floor_hit == 0 and mir.loss_scale == 2.0
    assert mir.step(float("nan")) == 0 and mir.floor_hit == 1 and mir.loss_scale == 1.0
    assert mir.step(0.25) == 1 and mir.floor_hit == 1                                            # sticky
    noclip = M.MirrorState(0.1, clip_norm=None, init_scale=4.0)
    assert noclip.step(1.0e9) == 1 and float(noclip.scalars[0]) == 0.25


def test_running_product_bias_corrections():
    """beta^t as t multiplications against b ** t: the doubles differ in their last bits (by 1.4e-14 relative at the most here), the floats
    the Adam kernel gets do not — 0 differences in 240 000 comparisons."""
    n = diff = 0
    worst = 0.0
    for b in (0.9, 0.98, 0.999):
        run = np.empty(20000)
        p = 1.0
        for i in range(20000):
            p = p * b
            run[i] = p
        pw = np.array([b ** k for k in range(1, 20001)])
        for a, r in ((1.0 / (1.0 - run), 1.0 / (1.0 - pw)), (np.sqrt(1.0 - run), np.sqrt(1.0 - pw))):
            worst = max(worst, float((np.abs(a - r) / r).max()))
        for lr in (1e-4, 5e-4, 0.1):
            diff += int((np.float32(lr / (1.0 - run)) != np.float32(lr / (1.0 - pw))).sum())
            n += 20000
        diff += int((np.float32(np.sqrt(1.0 - run)) != np.float32(np.sqrt(1.0 - pw))).sum())
        n += 20000
    print(f"bias corrections: {diff} differences in {n} comparisons, largest relative difference of the doubles {worst:.2e}")
    assert n == 240000 and diff == 0


def test_slot_indices_are_the_headers():
    from daspeech_amd import fp16_trainer as F
    text = open(os.path.join(ROOT, "include", "daspeech_optim.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define DSP_OPTIM_(\w+) (\d+)", text)}
    assert len(defs) == 15
    for k, v in defs.items():
        assert getattr(F, k) == v, k                                                             # SLOT_*, N_SCALARS, STATE_SLOTS
    slots = sorted(v for k, v in defs.items() if k.startswith("SLOT_"))
    assert slots == list(range(13)) and defs["STATE_SLOTS"] * 8 >= defs["SLOT_SCALARS"] * 8 + 4 * defs["N_SCALARS"]
    assert len(M.SCALAR_NAMES) == defs["N_SCALARS"]


def test_device_scaler_surface_without_a_gpu():
    from daspeech_amd.fp16_trainer import FP16FlatOptimizer
    assert inspect.signature(FP16FlatOptimizer.__init__).parameters["device_scaler"].default is False
    params = [torch.nn.Parameter(torch.randn(5).half()), torch.nn.Parameter(torch.randn(2, 3).half())]
    with pytest.raises(ValueError, match="hip_step"):
        FP16FlatOptimizer(params, hip_step=False, device_scaler=True)
    with pytest.raises(RuntimeError, match="hip_step=True"):
        FP16FlatOptimizer(params, device_scaler=True)
    with pytest.raises(RuntimeError, match="hip_step=True"):
        FP16FlatOptimizer(params, hip_step=True, device_scaler=True)
    opt = FP16FlatOptimizer(params, hip_step=False)
    assert opt.device_scaler is False and opt.hip_step is False
    with pytest.raises(NotImplementedError, match="hip_step"):
        opt.state_dict()
    with pytest.raises(NotImplementedError, match="hip_step"):
        opt.load_state_dict({})
    opt.check()                                                                                  # host mode: nothing to read
