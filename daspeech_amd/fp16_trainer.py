"""The optimizer half of the reference's `--fp16` training step (README.md:241,274; BASELINE C5), for bench.py and the C5 tests.

fairseq trains DASpeech with a HALF-PRECISION MODEL (model.half(), trainer.py:_setup / fp16) under FP16Optimizer
(fairseq/fairseq/optim/fp16_optimizer.py:252-330 with `build_fp32_params(flatten=True)` :38-72): one flat fp32 master copy of all
parameters, fp16 gradients copied into a flat fp32 gradient (:111-145), multiply_grads / clip_grad_norm on that ONE tensor (:187-211), Adam on
that one tensor, master copied back into the fp16 parameters (:146-170), loss scale from DynamicLossScaler
(fairseq/fairseq/optim/dynamic_loss_scaler.py:7-70: x2 after `scale_window` overflow-free updates, /2 on an overflow, which skips the update).
torch.autocast — what r01-r03 timed — is not what the reference does and costs ~1 500 cast launches per step on this model.

Here: the same scheme on one of two paths, chosen when the optimizer is built.
  torch path   multi-tensor copies (torch._foreach_copy_) instead of fairseq's per-parameter Python loops, torch's fused AdamW on the master.
  HIP step     csrc/fp16_optim.hip (include/daspeech_optim.h): the norm read from the fp16 gradients themselves, then ONE pass that unscales,
               clips, decays, updates master and moments and writes the fp16 parameters — no flat fp32 gradient exists."""
import math
from typing import Iterable, List, Sequence, Tuple

import torch

FUSED_STEP_HIP = True        # set_fused_step_hip(False): an FP16FlatOptimizer built with hip_step=None takes the torch path
HIP_STEP_CHUNK = 2048        # largest work item of the HIP step (elements): a multiple of 2048 up to 65536; tools/fp16_optim_bench.py --chunk


def set_fused_step_hip(on: bool) -> bool:
    """Switch the HIP optimizer step on or off for optimizers built from now on (hip_step=None); returns the previous setting.  An existing
    optimizer keeps its path: the two keep their moments in different places."""
    global FUSED_STEP_HIP
    old, FUSED_STEP_HIP = FUSED_STEP_HIP, bool(on)
    return old


def build_work_items(sizes: Sequence[int], chunk: int) -> List[Tuple[int, int, int]]:
    """The work items (tensor index, first element within the tensor, count) of tensors of `sizes` elements laid end to end in the flat
    arrays: tensors in order, each cut at the multiples of `chunk` of the FLAT index, so that an item never crosses a tensor, holds at most
    `chunk` elements, and — chunk being a multiple of 4 — starts on the fp32 arrays' 16-byte grid everywhere but at a tensor's first element.
    Every (tensor, element) is in exactly one item; empty tensors give none."""
    if chunk < 1:
        raise ValueError(f"chunk = {chunk}")
    items, off = [], 0
    for ti, n in enumerate(sizes):
        e = 0
        while e < n:
            cnt = min(n - e, chunk - (off + e) % chunk)
            items.append((ti, e, cnt))
            e += cnt
        off += n
    return items


def _hip_step_problem(params) -> str:
    """None when the HIP step serves this parameter list, else the reason"""
    dev = params[0].device
    if dev.type != "cuda":
        return f"parameters on {dev}: the HIP step needs CUDA tensors"
    if any(p.device != dev for p in params):
        return "parameters on more than one device"
    if any(not p.is_contiguous() for p in params):
        return "a parameter that is not contiguous"
    try:
        from . import _lib
        _lib.load()
    except Exception as e:                                                                   # no library: not served (hip_step=True raises this)
        return f"libdaspeech_hip does not load: {e}"
    return None


class DynamicLossScaler:
    """dynamic_loss_scaler.py:7-70 (tolerance 0, no threshold)."""

    def __init__(self, init_scale=2.0 ** 7, scale_factor=2.0, scale_window=2000, min_loss_scale=1e-4):
        self.loss_scale, self.scale_factor, self.scale_window, self.min_loss_scale = float(init_scale), scale_factor, scale_window, min_loss_scale
        self._iter, self._last_overflow_iter = 0, -1

    def update(self):
        if (self._iter - self._last_overflow_iter) % self.scale_window == 0:
            self.loss_scale *= self.scale_factor
        self._iter += 1

    def overflow(self):
        self._last_overflow_iter = self._iter
        self.loss_scale /= self.scale_factor
        self._iter += 1
        if self.loss_scale <= self.min_loss_scale:
            raise FloatingPointError(f"Minimum loss scale reached ({self.min_loss_scale})")


class FP16FlatOptimizer:
    """fp16 parameters / gradients, flat fp32 master + Adam (fairseq's `adam`: decoupled weight decay, fairseq/optim/adam.py:195-198).

    hip_step: None — the HIP step when FUSED_STEP_HIP is on and the parameter list is served (one CUDA device, contiguous, the library loads);
    True — the HIP step or an error; False — the torch path.  Fixed for the object's life; `self.hip_step` tells which one runs.  With the HIP
    step the moments are the flat fp32 tensors `exp_avg` / `exp_avg_sq`, the step count is `step_count`, and neither a flat gradient
    (`master.grad is None`) nor a torch optimizer exists."""

    def __init__(self, params: Iterable[torch.nn.Parameter], lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, clip_norm=1.0,
                 init_scale=2.0 ** 7, scale_window=2000, hip_step=None):
        self.params = [p for p in params if p.requires_grad]
        assert self.params and all(p.dtype == torch.float16 for p in self.params), "FP16FlatOptimizer wants a model.half() model"
        if hip_step is None:
            hip_step = FUSED_STEP_HIP and _hip_step_problem(self.params) is None
        elif hip_step:
            why = _hip_step_problem(self.params)
            if why is not None:
                raise RuntimeError(f"FP16FlatOptimizer(hip_step=True): {why}")
        self.hip_step = bool(hip_step)
        n = sum(p.numel() for p in self.params)
        dev = self.params[0].device
        self.master = torch.nn.Parameter(torch.empty(n, dtype=torch.float32, device=dev))
        sizes = [p.numel() for p in self.params]
        self._mviews = [v.view_as(p) for v, p in zip(self.master.data.split(sizes), self.params)]
        torch._foreach_copy_(self._mviews, [p.data for p in self.params])
        if self.hip_step:
            self.lr, self.betas, self.eps, self.weight_decay = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
            if not (0.0 <= self.betas[0] < 1.0 and 0.0 <= self.betas[1] < 1.0):
                raise ValueError(f"betas {betas} outside [0, 1)")
            self._init_hip_step(sizes, dev)
        else:
            self.master.grad = torch.zeros(n, dtype=torch.float32, device=dev)
            self._gviews = [v.view_as(p) for v, p in zip(self.master.grad.split(sizes), self.params)]
            self.opt = torch.optim.AdamW([self.master], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, fused=True)
        self.scaler = DynamicLossScaler(init_scale=init_scale, scale_window=scale_window)
        self.clip_norm = clip_norm
        self.last_grad_norm = None

    def _init_hip_step(self, sizes, dev):
        """Moments, tables and workspace of the HIP step.  Everything but the gradient-pointer table is built once."""
        from . import _lib
        lib = _lib.load()
        n, N = sum(sizes), len(sizes)
        self.exp_avg = torch.zeros(n, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(n, dtype=torch.float32, device=dev)
        self.step_count = 0
        self.chunk = HIP_STEP_CHUNK
        items = build_work_items(sizes, self.chunk)
        self._n_items = len(items)
        self._items = torch.tensor(items, dtype=torch.int64).reshape(-1, 3).to(dev)
        offsets = [0] * N
        for i in range(1, N):
            offsets[i] = offsets[i - 1] + sizes[i - 1]
        self._offsets = torch.tensor(offsets, dtype=torch.int64).to(dev)
        self._pptr = torch.tensor([p.data_ptr() for p in self.params], dtype=torch.int64).to(dev)
        self._gptr_host = torch.zeros(N, dtype=torch.int64).pin_memory()
        self._gptr_np = self._gptr_host.numpy()
        self._gptr = torch.zeros(N, dtype=torch.int64, device=dev)
        self._ws_bytes = int(lib.dsp_fp16_optim_workspace_bytes(self._n_items))
        self._ws = torch.empty(max(self._ws_bytes, 16), dtype=torch.uint8, device=dev)
        self._S = torch.zeros(1, dtype=torch.float64, device=dev)
        self._sumsq, self._adam = lib.dsp_fp16_optim_grad_sumsq, lib.dsp_fp16_optim_adam_step

    def zero_grad(self):
        for p in self.params:
            p.grad = None

    def backward(self, loss: torch.Tensor):
        (loss.float() * self.scaler.loss_scale).backward()                                   # fp16_optimizer.py:101-109

    def step(self, grad_mult: float = 1.0) -> bool:
        """Unscale (x grad_mult: the trainer's world_size / sample_size, trainer.py:932-946), clip, update.  Returns False when the step
        was skipped on an overflow (fairseq raises OverflowError and the trainer moves on, trainer.py:1020-1028)."""
        if self.hip_step:
            return self._step_hip(grad_mult)
        grads = [p.grad if p.grad is not None else torch.zeros_like(p) for p in self.params]
        torch._foreach_copy_(self._gviews, grads)                                            # :111-145, one multi-tensor launch
        g = self.master.grad
        g.mul_(grad_mult / self.scaler.loss_scale)                                           # :172-186
        norm = torch.linalg.vector_norm(g)
        nv = float(norm)                                                                     # (fairseq syncs here too: the norm is logged and checked, :191-211)
        self.last_grad_norm = nv
        if nv != nv or nv == float("inf"):
            self.scaler.overflow()
            return False
        if self.clip_norm and nv > self.clip_norm:
            g.mul_(self.clip_norm / (nv + 1e-6))
        self.opt.step()
        with torch.no_grad():                                                                # :146-170 — into the parameters THEMSELVES, so that
            torch._foreach_copy_(self.params, self._mviews)                                  # p._version advances (weight caches key on it)
        self.scaler.update()
        return True

    def _step_hip(self, grad_mult: float) -> bool:
        from . import decode_ops
        dev = self.master.device
        N = len(self.params)
        # the gradients of this step: the tensors are new every step (zero_grad drops them), so their addresses are collected every step
        keep = []                                                                            # contiguous copies stay alive until the launches are queued
        ptrs, f16 = [], torch.float16
        for p in self.params:                                                                # ~700 tensors on a launch-bound step: kept lean
            g = p.grad
            if g is None:
                ptrs.append(0)
                continue
            if g.dtype is not f16 or not g.is_cuda:
                raise RuntimeError(f"FP16FlatOptimizer: gradient {g.dtype} on {g.device} of a parameter {p.dtype} on {p.device}")
            if not g.is_contiguous():
                g = g.contiguous()
                keep.append(g)
            ptrs.append(g.data_ptr())
        # the pinned table is rewritten at the next step: safe, because float(S) below waits for this stream, the copy included
        self._gptr_np[:] = ptrs
        self._gptr.copy_(self._gptr_host, non_blocking=True)
        gp, it = self._gptr.data_ptr(), self._items.data_ptr()
        decode_ops._launch(dev, self._sumsq, gp, 1, N, it, self._n_items, self.chunk, self._ws.data_ptr(), self._ws_bytes, self._S.data_ptr())
        S = float(self._S)                                                                   # the step's one sync (fairseq: :191-211)
        c = grad_mult / self.scaler.loss_scale
        nv = abs(c) * math.sqrt(S) if S == S and S >= 0.0 else float("nan")
        self.last_grad_norm = nv
        if nv != nv or nv == float("inf"):
            self.scaler.overflow()
            return False
        if self.clip_norm and nv > self.clip_norm:
            c *= self.clip_norm / (nv + 1e-6)
        t = self.step_count + 1
        b1, b2 = self.betas
        decode_ops._launch(dev, self._adam, gp, self._pptr.data_ptr(), 1, self._offsets.data_ptr(), N, it, self._n_items, self.chunk,
                           self.master.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(),
                           c, self.lr, b1, b2, self.eps, self.lr * self.weight_decay, 1.0 - b1 ** t, math.sqrt(1.0 - b2 ** t), t)
        self.step_count = t
        torch.autograd.graph.increment_version(self.params)                                  # raw-pointer writes: the weight caches key on p._version
        del keep
        self.scaler.update()
        return True


def half_sample(sample):
    """trainer.py:_prepare_sample under --fp16: every float32 tensor of the batch becomes float16 (utils.apply_to_sample(apply_half))."""
    if isinstance(sample, dict):
        return {k: half_sample(v) for k, v in sample.items()}
    if torch.is_tensor(sample) and sample.dtype == torch.float32:
        return sample.half()
    return sample
