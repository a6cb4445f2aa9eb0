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
               clips, decays, updates master and moments and writes the fp16 parameters — no flat fp32 gradient exists.
The HIP step has two modes.  By default the host reads the norm (the step's one sync) and decides overflow, clip coefficient, loss scale and
bias corrections itself.  With device_scaler=True those decisions are one more launch on a small state block in device memory
(dsp_fp16_optim_scale_step): step() queues three launches and waits for nothing, and backward() + step() can be captured and replayed."""
import math
from typing import Iterable, List, Sequence, Tuple

import torch

FUSED_STEP_HIP = True        # set_fused_step_hip(False): an FP16FlatOptimizer built with hip_step=None takes the torch path
HIP_STEP_CHUNK = 2048        # largest work item of the HIP step (elements): a multiple of 2048 up to 65536; tools/fp16_optim_bench.py --chunk


# the slots of the device optimizer state (include/daspeech_optim.h, DSP_OPTIM_SLOT_*: 8 bytes each; 4-byte fields in the low half)
SLOT_LOSS_SCALE, SLOT_LOSS_SCALE_F32, SLOT_ITER, SLOT_LAST_OVERFLOW_ITER, SLOT_T, SLOT_POW1, SLOT_POW2 = 0, 1, 2, 3, 4, 5, 6
SLOT_LR, SLOT_GRAD_MULT, SLOT_GRAD_NORM, SLOT_APPLIED, SLOT_FLOOR_HIT, SLOT_SCALARS = 7, 8, 9, 10, 11, 12
N_SCALARS, STATE_SLOTS = 9, 17


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


class DeviceLossScaler:
    """What `opt.scaler` is with device_scaler=True: the DynamicLossScaler's fields read from the optimizer state on the device.  Every read
    copies the state to the host and so SYNCHRONISES with the optimizer's stream; nothing in backward() or step() reads them."""

    def __init__(self, opt, scale_factor=2.0, scale_window=2000, min_loss_scale=1e-4):
        self._opt, self.scale_factor, self.scale_window, self.min_loss_scale = opt, scale_factor, scale_window, min_loss_scale

    @property
    def loss_scale(self) -> float:
        return float(self._opt._read_state()[0][SLOT_LOSS_SCALE])

    @property
    def _iter(self) -> int:
        return int(self._opt._read_state()[1][SLOT_ITER])

    @property
    def _last_overflow_iter(self) -> int:
        return int(self._opt._read_state()[1][SLOT_LAST_OVERFLOW_ITER])


class FP16FlatOptimizer:
    """fp16 parameters / gradients, flat fp32 master + Adam (fairseq's `adam`: decoupled weight decay, fairseq/optim/adam.py:195-198).

    hip_step: None — the HIP step when FUSED_STEP_HIP is on and the parameter list is served (one CUDA device, contiguous, the library loads);
    True — the HIP step or an error; False — the torch path.  Fixed for the object's life; `self.hip_step` tells which one runs.  With the HIP
    step the moments are the flat fp32 tensors `exp_avg` / `exp_avg_sq`, the step count is `step_count`, and neither a flat gradient
    (`master.grad is None`) nor a torch optimizer exists.

    device_scaler: False — the host reads the norm and decides (one sync a step).  True (needs the HIP step) — the decisions are made on the
    device: `step()` returns the 0-dim int32 device tensor `applied` instead of a bool and never synchronises, `last_grad_norm` is a 0-dim
    float64 device tensor, `backward()` multiplies by the loss scale as a device scalar, and both can be captured into a graph after one eager
    step with the same gradient tensors.  `step_count`, `scaler.loss_scale` and `check()` then read the state, which SYNCHRONISES; change the
    learning rate with `set_lr` (and `grad_mult` with `set_grad_mult` or step's argument) before a capture and between replays, not inside."""

    def __init__(self, params: Iterable[torch.nn.Parameter], lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, clip_norm=1.0,
                 init_scale=2.0 ** 7, scale_window=2000, hip_step=None, device_scaler=False):
        self.params = [p for p in params if p.requires_grad]
        assert self.params and all(p.dtype == torch.float16 for p in self.params), "FP16FlatOptimizer wants a model.half() model"
        self.device_scaler = bool(device_scaler)
        if self.device_scaler:
            if hip_step is not None and not hip_step:
                raise ValueError("FP16FlatOptimizer(device_scaler=True) needs the HIP step: hip_step=False was asked for")
            hip_step = True
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
        if self.device_scaler:
            self._init_device_scaler(dev)

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

    def _init_device_scaler(self, dev):
        """The device mode's state block, its views, the second pinned pointer table and the two entries.  `self.scaler` (built by the
        constructor with the defaults of DynamicLossScaler) hands its fields over to the state and becomes a DeviceLossScaler."""
        from . import _lib
        lib = _lib.load()
        host = self.scaler
        self.scaler = DeviceLossScaler(self, host.scale_factor, host.scale_window, host.min_loss_scale)
        self._state = torch.zeros(STATE_SLOTS, dtype=torch.int64, device=dev)
        self._state_f64, self._state_f32, self._state_i32 = (self._state.view(t) for t in (torch.float64, torch.float32, torch.int32))
        self._loss_scale_f32 = self._state_f32[2 * SLOT_LOSS_SCALE_F32]                       # 0-dim views: what backward() and step() hand out
        self._applied = self._state_i32[2 * SLOT_APPLIED]
        self._lr_slot, self._grad_mult_slot = self._state_f64[SLOT_LR:SLOT_LR + 1], self._state_f64[SLOT_GRAD_MULT:SLOT_GRAD_MULT + 1]
        self.last_grad_norm = self._state_f64[SLOT_GRAD_NORM]
        self._write_state(host.loss_scale, host._iter, host._last_overflow_iter, 0, self.lr, 1.0)
        # the pointer table: the addresses last uploaded, and two pinned buffers taken in turn, each guarded by an event recorded after its upload
        self._gptr_last = None
        self._gptr_hosts = [self._gptr_host, torch.zeros(len(self.params), dtype=torch.int64).pin_memory()]
        self._gptr_nps = [h.numpy() for h in self._gptr_hosts]
        self._gptr_events = [torch.cuda.Event(), torch.cuda.Event()]
        self._gptr_turn = 0
        self._scale_step, self._adam_state = lib.dsp_fp16_optim_scale_step, lib.dsp_fp16_optim_adam_step_state

    def _write_state(self, loss_scale, it, last_overflow_iter, t, lr, grad_mult):
        """the whole state from host values (construction and load_state_dict): pow1 / pow2 as t multiplications, exact by construction"""
        import numpy as np
        h = np.zeros(STATE_SLOTS, dtype=np.int64)
        d, f = h.view(np.float64), h.view(np.float32)
        pow1 = pow2 = 1.0
        for _ in range(t):
            pow1 *= self.betas[0]
            pow2 *= self.betas[1]
        d[SLOT_LOSS_SCALE], f[2 * SLOT_LOSS_SCALE_F32] = loss_scale, loss_scale
        h[SLOT_ITER], h[SLOT_LAST_OVERFLOW_ITER], h[SLOT_T] = it, last_overflow_iter, t
        d[SLOT_POW1], d[SLOT_POW2], d[SLOT_LR], d[SLOT_GRAD_MULT] = pow1, pow2, lr, grad_mult
        self._state.copy_(torch.from_numpy(h))
        self._lr_written, self._grad_mult_written = float(lr), float(grad_mult)

    def _read_state(self):
        """the state on the host as (float64 view, int64 view, int32 view) of one copy — a synchronising read"""
        import numpy as np
        h = self._state.cpu().numpy()
        return h.view(np.float64), h, h.view(np.int32)

    @property
    def step_count(self) -> int:
        """applied steps.  With device_scaler=True this reads the state and so synchronises."""
        if self.device_scaler:
            return int(self._read_state()[1][SLOT_T])
        return self._step_count

    @step_count.setter
    def step_count(self, t: int):
        self._step_count = t

    def _write_slot(self, slot, value, what):
        """one input slot through a fill_ of a one-element view: a kernel argument, no sync.  A capture would freeze the value into the graph."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"FP16FlatOptimizer: {what} changes to {value} while the stream is capturing: write it before the capture "
                               f"and between replays (set_lr / set_grad_mult), not inside")
        slot.fill_(value)

    def set_lr(self, lr: float):
        """The learning rate of the next steps.  Device mode: one slot write, queued only when the value differs from the one last written."""
        lr = float(lr)
        if self.hip_step:
            self.lr = lr
            if self.device_scaler and lr != self._lr_written:
                self._write_slot(self._lr_slot, lr, "lr")
                self._lr_written = lr
        else:
            for g in self.opt.param_groups:
                g["lr"] = lr

    def set_grad_mult(self, grad_mult: float):
        """Device mode: the factor step() multiplies the gradients by (beside 1 / loss_scale), written ahead of a capture or between replays."""
        if not self.device_scaler:
            raise RuntimeError("FP16FlatOptimizer.set_grad_mult: device_scaler=True only; pass grad_mult to step()")
        grad_mult = float(grad_mult)
        if grad_mult != self._grad_mult_written:
            self._write_slot(self._grad_mult_slot, grad_mult, "grad_mult")
            self._grad_mult_written = grad_mult

    def check(self):
        """Device mode: raise the FloatingPointError that DynamicLossScaler.overflow raises on the host once the loss scale has reached its
        floor (the state's sticky flag).  Reads the state: call it where a sync is affordable, e.g. with the logging.  Host mode: nothing to
        do, step() raises there."""
        if self.device_scaler and int(self._read_state()[2][2 * SLOT_FLOOR_HIT]):
            raise FloatingPointError(f"Minimum loss scale reached ({self.scaler.min_loss_scale})")

    def mark_params_updated(self):
        """Advance the parameters' versions (the inference-side weight caches key on `_version`).  step() calls it; a graph REPLAY of step()
        cannot, so call it after replays before such a cache is used."""
        torch.autograd.graph.increment_version(self.params)

    def zero_grad(self):
        for p in self.params:
            p.grad = None

    def backward(self, loss: torch.Tensor):
        if self.device_scaler:
            (loss.float() * self._loss_scale_f32).backward()                                 # a device scalar: a replay uses the scale of its time
            return
        (loss.float() * self.scaler.loss_scale).backward()                                   # fp16_optimizer.py:101-109

    def step(self, grad_mult: float = 1.0) -> bool:
        """Unscale (x grad_mult: the trainer's world_size / sample_size, trainer.py:932-946), clip, update.  Returns False when the step
        was skipped on an overflow (fairseq raises OverflowError and the trainer moves on, trainer.py:1020-1028).  With device_scaler=True
        the same answer comes back as the 0-dim int32 device tensor `applied` (1 / 0) and nothing is waited for."""
        if self.device_scaler:
            return self._step_device(grad_mult)
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


    def _step_device(self, grad_mult: float) -> torch.Tensor:
        """The HIP step with the decisions on the device: the norm, the state update (dsp_fp16_optim_scale_step) and the Adam pass that reads
        its scalars and `applied` from the state — queued, never waited for.  Returns `applied` (0-dim int32, on the device)."""
        from . import decode_ops
        dev = self.master.device
        N = len(self.params)
        keep = []                                                                            # as in _step_hip
        ptrs, f16 = [], torch.float16
        for p in self.params:
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
        self.set_lr(self.lr)                                                                 # `opt.lr = x` is honoured as in host mode
        self.set_grad_mult(grad_mult)
        if ptrs != self._gptr_last:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("FP16FlatOptimizer: the gradient tensors are not the ones of the last step and the stream is capturing: "
                                   "run one eager step with these gradient tensors before capturing")
            # no sync orders the host's next write after this upload any more: the buffer written now was uploaded two uploads ago, and its
            # event says that upload is done — a wait that never blocks in practice
            i = self._gptr_turn
            if not self._gptr_events[i].query():
                self._gptr_events[i].synchronize()
            self._gptr_nps[i][:] = ptrs
            self._gptr.copy_(self._gptr_hosts[i], non_blocking=True)
            self._gptr_events[i].record()
            self._gptr_turn, self._gptr_last = i ^ 1, ptrs
        gp, it, st = self._gptr.data_ptr(), self._items.data_ptr(), self._state.data_ptr()
        decode_ops._launch(dev, self._sumsq, gp, 1, N, it, self._n_items, self.chunk, self._ws.data_ptr(), self._ws_bytes, self._S.data_ptr())
        b1, b2 = self.betas
        sc = self.scaler
        decode_ops._launch(dev, self._scale_step, self._S.data_ptr(), st, b1, b2, self.eps, self.weight_decay, float(self.clip_norm or 0.0),
                           sc.scale_factor, sc.scale_window, sc.min_loss_scale)
        decode_ops._launch(dev, self._adam_state, gp, self._pptr.data_ptr(), 1, self._offsets.data_ptr(), N, it, self._n_items, self.chunk,
                           self.master.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), st)
        self.mark_params_updated()                                                           # applied or not is not known here: a version too many is harmless
        del keep
        return self._applied

    # ------------------------------------------------------------------------------------------------ checkpoints (the HIP step, both modes)
    def state_dict(self) -> dict:
        """Master, moments (clones), step count, scaler fields and the hyperparameters.  Device mode reads its state: a sync."""
        if not self.hip_step:
            raise NotImplementedError("FP16FlatOptimizer.state_dict: the HIP step only (hip_step=True); the torch path keeps its moments in "
                                      "torch.optim.AdamW")
        if self.device_scaler:
            d, i, _ = self._read_state()
            t, scale, it, last = int(i[SLOT_T]), float(d[SLOT_LOSS_SCALE]), int(i[SLOT_ITER]), int(i[SLOT_LAST_OVERFLOW_ITER])
        else:
            t, scale, it, last = self.step_count, self.scaler.loss_scale, self.scaler._iter, self.scaler._last_overflow_iter
        return {"master": self.master.detach().clone(), "exp_avg": self.exp_avg.clone(), "exp_avg_sq": self.exp_avg_sq.clone(),
                "step_count": t, "loss_scale": scale, "iter": it, "last_overflow_iter": last,
                "sizes": [p.numel() for p in self.params], "betas": self.betas, "lr": self.lr, "eps": self.eps,
                "weight_decay": self.weight_decay, "clip_norm": self.clip_norm, "scale_window": self.scaler.scale_window}

    def load_state_dict(self, sd: dict):
        """Take over a state_dict of either mode.  The sizes and betas must be this optimizer's (the running bias corrections depend on the
        betas); lr is taken over, the other hyperparameters stay as constructed.  The fp16 parameters become the rounding of the loaded master
        and their versions advance."""
        if not self.hip_step:
            raise NotImplementedError("FP16FlatOptimizer.load_state_dict: the HIP step only (hip_step=True)")
        sizes = [p.numel() for p in self.params]
        if list(sd["sizes"]) != sizes:
            raise ValueError(f"load_state_dict: saved for {len(sd['sizes'])} tensors of {sum(sd['sizes'])} elements, this optimizer has "
                             f"{len(sizes)} of {sum(sizes)} (or other sizes)")
        if tuple(float(b) for b in sd["betas"]) != self.betas:
            raise ValueError(f"load_state_dict: saved with betas {tuple(sd['betas'])}, this optimizer has {self.betas}")
        t = int(sd["step_count"])
        if t < 0:
            raise ValueError(f"load_state_dict: step_count = {t}")
        with torch.no_grad():
            self.master.copy_(sd["master"])
            self.exp_avg.copy_(sd["exp_avg"])
            self.exp_avg_sq.copy_(sd["exp_avg_sq"])
            torch._foreach_copy_(self.params, self._mviews)                                  # into the parameters themselves: versions advance
        self.lr = float(sd["lr"])
        if self.device_scaler:
            self._write_state(float(sd["loss_scale"]), int(sd["iter"]), int(sd["last_overflow_iter"]), t, self.lr, self._grad_mult_written)
        else:
            self.step_count = t
            self.scaler.loss_scale, self.scaler._iter, self.scaler._last_overflow_iter = float(sd["loss_scale"]), int(sd["iter"]), int(sd["last_overflow_iter"])


def half_sample(sample):
    """trainer.py:_prepare_sample under --fp16: every float32 tensor of the batch becomes float16 (utils.apply_to_sample(apply_half))."""
    if isinstance(sample, dict):
        return {k: half_sample(v) for k, v in sample.items()}
    if torch.is_tensor(sample) and sample.dtype == torch.float32:
        return sample.half()
    return sample
