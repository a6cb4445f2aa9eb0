"""One step of the fp16 trainer's optimizer half restated in float64 (daspeech_amd/fp16_trainer.py, include/daspeech_optim.h): sum of squares of
the 16-bit gradients, unscale, clip, decoupled decay + Adam, and the 16-bit parameter as the rounding of the fp32-rounded master.  numpy only, no
torch optimizer; tests/test_fp16_optim_ref.py holds it against torch.optim.AdamW in float64."""
import math

import numpy as np

SIZE_LISTS = ([1], [7, 1, 9], [8, 2047, 2048, 2049], [1, 4099, 1, 64])      # the size lists of the issue's cases, at chunk 2048
CHUNK = 2048


def adam_elements(g, p, m, v, t, c, lr, beta1, beta2, eps, wd):
    """the per-element lines of dsp_fp16_optim_adam_step in float64; g is float(g16) (0 without a gradient).  Returns p, m, v."""
    g = c * g
    p = p * (1.0 - lr * wd)
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    p = p - (lr / (1.0 - beta1 ** t)) * m / (np.sqrt(v) / math.sqrt(1.0 - beta2 ** t) + eps)
    return p, m, v


def naive_items(sizes, chunk):
    """the work items by the plainest loop there is: walk every element, start a new item at a tensor's first element and wherever the flat
    index is a multiple of chunk"""
    items, flat = [], 0
    for ti, n in enumerate(sizes):
        for e in range(n):
            if e == 0 or flat % chunk == 0:
                items.append([ti, e, 0])
            items[-1][2] += 1
            flat += 1
    return [tuple(i) for i in items]


class RefOptimizer:
    """float64 state of the flat optimizer: master, exp_avg, exp_avg_sq (one flat array each), step count, loss scale handled by the caller"""

    def __init__(self, params, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, clip_norm=1.0):
        self.sizes = [int(np.asarray(p).size) for p in params]
        self.master = np.concatenate([np.asarray(p, dtype=np.float64).reshape(-1) for p in params])
        self.exp_avg = np.zeros_like(self.master)
        self.exp_avg_sq = np.zeros_like(self.master)
        self.t = 0
        self.lr, self.betas, self.eps, self.wd, self.clip_norm = lr, betas, eps, weight_decay, clip_norm

    def flat_grad(self, grads):
        """grads: one array (the 16-bit values, any float dtype) or None per tensor -> the flat float64 gradient, zeros where None"""
        out = []
        for g, n in zip(grads, self.sizes):
            out.append(np.zeros(n) if g is None else np.asarray(g, dtype=np.float64).reshape(-1))
        return np.concatenate(out)

    def step(self, grads, grad_mult, loss_scale):
        """-> (nv, updated?); nv = c * sqrt(sum g^2), the norm of the unscaled gradient before clipping"""
        g = self.flat_grad(grads)
        c = grad_mult / loss_scale
        with np.errstate(over="ignore", invalid="ignore"):
            nv = c * math.sqrt(float(np.sum(g * g))) if np.isfinite(g).all() else float("nan")
        if not math.isfinite(nv):
            return nv, False
        if self.clip_norm and nv > self.clip_norm:
            c *= self.clip_norm / (nv + 1e-6)
        self.t += 1
        self.master, self.exp_avg, self.exp_avg_sq = adam_elements(g, self.master, self.exp_avg, self.exp_avg_sq, self.t, c, self.lr,
                                                                   self.betas[0], self.betas[1], self.eps, self.wd)
        return nv, True

    def params16(self, np_dtype=np.float16):
        """the 16-bit parameters: the rounding of the master as stored in fp32"""
        return [x.astype(np_dtype) for x in np.split(self.master.astype(np.float32), np.cumsum(self.sizes)[:-1])]
