"""The device optimizer state's update rule (include/daspeech_optim.h, dsp_fp16_optim_scale_step) in plain Python floats: every line is one IEEE
double multiply, add, divide or square root in the kernel's order, so equal inputs give equal bits in every slot.
tests/test_optim_state_ref.py holds it against fp16_trainer.DynamicLossScaler and the host formulas of FP16FlatOptimizer._step_hip; the GPU
tests hold the kernel against it."""
import math
import struct

import numpy as np

# the scripted sums of squares of the issue: small, large enough to clip, inf, nan, negative, zero (at grad_mult 1 and loss scale 128, clip_norm 1)
S_SCRIPT = (0.25, 1.0e9, float("inf"), float("nan"), -1.0, 0.0)
SCALAR_NAMES = ("c", "beta1", "beta2", "eps", "decay", "step", "omb1", "omb2", "sqrt_bias2")      # AdamScalars, in the state's order


def bits(x: float) -> int:
    """the int64 whose bytes are the double x"""
    return struct.unpack("<q", struct.pack("<d", x))[0]


class MirrorState:
    def __init__(self, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, clip_norm=1.0, init_scale=2.0 ** 7, scale_factor=2.0,
                 scale_window=2000, min_loss_scale=1e-4, grad_mult=1.0):
        self.beta1, self.beta2, self.eps, self.weight_decay = float(betas[0]), float(betas[1]), float(eps), float(weight_decay)
        self.clip_norm, self.scale_factor, self.scale_window = float(clip_norm or 0.0), float(scale_factor), int(scale_window)
        self.min_loss_scale = float(min_loss_scale)
        self.loss_scale, self.iter, self.last_overflow_iter = float(init_scale), 0, -1
        self.t, self.pow1, self.pow2 = 0, 1.0, 1.0
        self.lr, self.grad_mult = float(lr), float(grad_mult)
        self.grad_norm, self.applied, self.floor_hit = 0.0, 0, 0
        self.doubles = None                  # of the last applied step: (c, lr, beta1, beta2, eps, lr_wd, bias1, sqrt_bias2), what
        self.scalars = [np.float32(0.0)] * 9    # dsp_fp16_optim_adam_step takes; and the nine floats derived from them

    @property
    def loss_scale_f32(self):
        return np.float32(self.loss_scale)

    def step(self, S: float) -> int:
        c = self.grad_mult / self.loss_scale
        nv = abs(c) * math.sqrt(S) if (S == S and S >= 0.0) else float("nan")
        self.grad_norm = nv
        if nv != nv or nv == float("inf"):
            self.last_overflow_iter = self.iter
            self.loss_scale = self.loss_scale / self.scale_factor
            self.iter += 1
            if self.loss_scale <= self.min_loss_scale:
                self.floor_hit = 1
            self.applied = 0
        else:
            if self.clip_norm > 0.0 and nv > self.clip_norm:
                c = c * (self.clip_norm / (nv + 1e-6))
            self.t += 1
            self.pow1 = self.pow1 * self.beta1
            self.pow2 = self.pow2 * self.beta2
            bias1 = 1.0 - self.pow1
            sqrt_bias2 = math.sqrt(1.0 - self.pow2)
            lr_wd = self.lr * self.weight_decay
            self.doubles = (c, self.lr, self.beta1, self.beta2, self.eps, lr_wd, bias1, sqrt_bias2)
            self.scalars = [np.float32(x) for x in (c, self.beta1, self.beta2, self.eps, 1.0 - lr_wd, self.lr / bias1, 1.0 - self.beta1,
                                                    1.0 - self.beta2, sqrt_bias2)]
            self.applied = 1
            if (self.iter - self.last_overflow_iter) % self.scale_window == 0:
                self.loss_scale = self.loss_scale * self.scale_factor
            self.iter += 1
        return self.applied
