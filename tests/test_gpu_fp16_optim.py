"""GPU tests of the fp16 trainer's HIP optimizer step (csrc/fp16_optim.hip, include/daspeech_optim.h, daspeech_amd/fp16_trainer.py).

Tolerance: the 4 x rule (tests/util_4x_rule.py) against the float64 restatement of tests/util_fp16_optim_ref.py; the yardstick is the same class
with hip_step=False (torch's copies, vector_norm and fused AdamW) on the same inputs, or, for the direct entry points, the same lines written with
torch's fp32 ops.  The shapes are the smallest that reach every path at chunk 2048: one element, segments at odd flat offsets, sizes at, below and
above the chunk, tensors of one element between larger ones; 16-bit addresses on and off the 8- and 4-byte grids."""
import math

import numpy as np
import pytest
import torch

from tests import util_fp16_optim_ref as R
from tests.util_4x_rule import check_4x, f64

pytestmark = pytest.mark.gpu

DEV = "cuda"
IDS = ["-".join(map(str, s)) for s in R.SIZE_LISTS]
LR = 0.1                     # a wrong update is an error of order 1, not lost under the master's magnitude
SCALE, MULT = 128.0, 0.5


def _make_params(sizes, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(n, generator=g).half().to(DEV)) for n in sizes]


def _grad_values(sizes, seed):
    """fp16 gradient values of magnitude 400 .. 800: after the unscale by 0.5 / 128 every element is above 1.5, so the norm exceeds 1"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for n in sizes:
        sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
        out.append((sign * (400.0 + 400.0 * torch.rand(n, generator=g))).half())
    return out


def _odd_view(v):
    """the values of v as a view that starts 2 bytes past a 16-byte boundary"""
    buf = torch.zeros(v.numel() + 8, dtype=v.dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    out = buf[1:1 + v.numel()]
    out.copy_(v)
    assert out.data_ptr() % 16 == 2
    return out


def _strided_view(v):
    buf = torch.zeros(2 * v.numel(), dtype=v.dtype, device=DEV)
    out = buf[::2]
    out.copy_(v)
    return out


def _state(opt):
    if opt.hip_step:
        return {"master": opt.master.detach().clone(), "exp_avg": opt.exp_avg.clone(), "exp_avg_sq": opt.exp_avg_sq.clone()}
    st = opt.opt.state[opt.master]                             # empty before the first step
    zero = torch.zeros_like(opt.master.detach())
    return {"master": opt.master.detach().clone(), "exp_avg": st.get("exp_avg", zero).clone(), "exp_avg_sq": st.get("exp_avg_sq", zero).clone()}


@pytest.mark.parametrize("clip_norm,wd", [(1.0, 0.01), (None, 0.0)], ids=["clip-wd", "noclip-nowd"])
@pytest.mark.parametrize("sizes", R.SIZE_LISTS, ids=IDS)
def test_three_steps_against_float64_and_the_torch_path(sizes, clip_norm, wd):
    """Three steps of one gradient sequence through the HIP step, the torch path and the float64 restatement: loss scale 128, grad_mult 0.5; in
    step 2 the last tensor has no gradient (its moments keep decaying); tensor 0's gradient is a view 2 bytes off a 16-byte boundary, and the
    second tensor's (where there is one) a strided view."""
    from daspeech_amd.fp16_trainer import FP16FlatOptimizer
    N = len(sizes)
    ph, pt = _make_params(sizes, 1), _make_params(sizes, 1)
    kw = dict(lr=LR, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd, clip_norm=clip_norm, init_scale=SCALE)
    hip = FP16FlatOptimizer(ph, hip_step=True, **kw)
    tor = FP16FlatOptimizer(pt, hip_step=False, **kw)
    assert hip.hip_step is True and tor.hip_step is False and hip.chunk % 2048 == 0
    assert hip.master.grad is None and not hasattr(hip, "opt") and not hasattr(hip, "_gviews")
    ref = R.RefOptimizer([f64(p) for p in ph], LR, (0.9, 0.999), 1e-8, wd, clip_norm)
    for step in range(3):
        vals = _grad_values(sizes, 10 + step)
        none_at = N - 1 if step == 1 else -1
        hip.zero_grad(); tor.zero_grad()
        for i in range(N):
            if i == none_at:
                continue
            v = vals[i].to(DEV)
            g = _odd_view(v) if i == 0 else (_strided_view(v) if i == 1 else v.clone())
            if i == 1 and sizes[i] > 1:
                assert not g.is_contiguous()
            ph[i].grad = g
            pt[i].grad = v.clone()
        before_h, before_t, before_r = _state(hip), _state(tor), ref.master.copy()
        versions = [p._version for p in ph]
        assert hip.scaler.loss_scale == tor.scaler.loss_scale
        scale = hip.scaler.loss_scale
        assert hip.step(MULT) is True and tor.step(MULT) is True
        nv, ok = ref.step([None if i == none_at else f64(vals[i]) for i in range(N)], MULT, scale)
        assert ok and (none_at == 0 or nv > 1.0)
        assert hip.step_count == step + 1 and hip.master.grad is None
        after_h, after_t = _state(hip), _state(tor)
        got_h = dict(after_h, nv=torch.tensor([hip.last_grad_norm], dtype=torch.float32),
                     update=(after_h["master"].double() - before_h["master"].double()).float())
        got_t = dict(after_t, nv=torch.tensor([tor.last_grad_norm], dtype=torch.float32),
                     update=(after_t["master"].double() - before_t["master"].double()).float())
        want = {"nv": np.array([nv]), "master": ref.master, "exp_avg": ref.exp_avg, "exp_avg_sq": ref.exp_avg_sq,
                "update": ref.master - before_r}
        check_4x(f"fp16_optim {sizes} step {step + 1}", got_h, got_t, want)
        for p, mv, v0 in zip(ph, hip._mviews, versions):
            assert torch.equal(p.data, mv.half()), "the fp16 parameter is not the rounding of the stored master"
            assert p._version > v0
    assert hip.scaler.loss_scale == tor.scaler.loss_scale


# ---------------------------------------------------------------------------------------------------- the entry points themselves
class _Problem:
    """The multi-tensor problem on raw pointers: gradients and 16-bit parameters carved out of two buffers with chosen element offsets (so
    that 16-bit addresses fall on and off the 8- / 4-byte grids whatever the flat offsets are), NaN-filled parameters, workspace and S."""

    def __init__(self, sizes, dtype, g_shift=0, p_shift=0, seed=0, none_at=()):
        from daspeech_amd import _lib
        from daspeech_amd.fp16_trainer import build_work_items
        self.lib = _lib.load()
        self.sizes, self.dtype, self.code = list(sizes), dtype, _lib.DTYPE_CODES[str(dtype)]
        self.N, self.n = len(sizes), sum(sizes)
        gen = torch.Generator().manual_seed(seed)
        self.offsets = [int(x) for x in np.concatenate([[0], np.cumsum(sizes)[:-1]])] if sizes else []
        items = build_work_items(sizes, R.CHUNK)
        self.n_items = len(items)
        self.items = torch.tensor(items, dtype=torch.int64).reshape(-1, 3).to(DEV)
        # every tensor gets its own 8-element-aligned slot (+ shift) in the two 16-bit buffers
        slots, at = [], 0
        for n in sizes:
            slots.append(at)
            at += (n + 7) // 8 * 8 + 8
        self.gbuf = torch.zeros(at + 8, dtype=dtype, device=DEV)
        self.pbuf = torch.full((at + 8,), float("nan"), dtype=dtype, device=DEV)
        self.g = [None if i in none_at else self.gbuf[s + g_shift:s + g_shift + n] for i, (s, n) in enumerate(zip(slots, sizes))]
        self.p16 = [self.pbuf[s + p_shift:s + p_shift + n] for s, n in zip(slots, sizes)]
        for g in self.g:
            if g is not None:
                g.copy_((torch.randn(g.numel(), generator=gen) * 300.0).to(dtype))
        self.master = torch.randn(self.n, generator=gen).to(DEV)
        self.m = (0.5 * torch.randn(self.n, generator=gen)).to(DEV)
        self.v = (0.5 * torch.rand(self.n, generator=gen) + 0.01).to(DEV)
        assert self.master.data_ptr() % 16 == 0 and self.m.data_ptr() % 16 == 0 and self.v.data_ptr() % 16 == 0
        self.gptr = torch.tensor([0 if g is None else g.data_ptr() for g in self.g], dtype=torch.int64).to(DEV)
        self.pptr = torch.tensor([p.data_ptr() for p in self.p16], dtype=torch.int64).to(DEV)
        self.offs = torch.tensor(self.offsets, dtype=torch.int64).to(DEV)
        self.ws_bytes = int(self.lib.dsp_fp16_optim_workspace_bytes(self.n_items))
        self.ws = torch.full((max(self.ws_bytes // 4, 4),), float("nan"), dtype=torch.float32, device=DEV)
        self.S = torch.full((1,), float("nan"), dtype=torch.float64, device=DEV)

    def stream(self):
        return torch.cuda.current_stream().cuda_stream

    def sumsq(self, **over):
        a = dict(grads=self.gptr.data_ptr(), dtype=self.code, N=self.N, items=self.items.data_ptr(), n_items=self.n_items, chunk=R.CHUNK,
                 ws=self.ws.data_ptr(), ws_bytes=self.ws_bytes, S=self.S.data_ptr())
        a.update(over)
        return self.lib.dsp_fp16_optim_grad_sumsq(a["grads"], a["dtype"], a["N"], a["items"], a["n_items"], a["chunk"], a["ws"], a["ws_bytes"],
                                                  a["S"], self.stream())

    SCALARS = dict(c=0.5 / 128.0, lr=LR, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01)

    def adam(self, t, **over):
        s = dict(self.SCALARS)
        a = dict(grads=self.gptr.data_ptr(), params=self.pptr.data_ptr(), dtype=self.code, offsets=self.offs.data_ptr(), N=self.N,
                 items=self.items.data_ptr(), n_items=self.n_items, chunk=R.CHUNK, master=self.master.data_ptr(), m=self.m.data_ptr(),
                 v=self.v.data_ptr(), t=t)
        for k, val in over.items():
            (s if k in s else a)["t" if k == "step" else k] = val
        t = a["t"]
        b1, b2 = s["beta1"], s["beta2"]
        bias1 = 1.0 - b1 ** t if t >= 1 and 0 <= b1 < 1 else 1.0
        sb2 = math.sqrt(1.0 - b2 ** t) if t >= 1 and 0 <= b2 < 1 else 1.0
        return self.lib.dsp_fp16_optim_adam_step(a["grads"], a["params"], a["dtype"], a["offsets"], a["N"], a["items"], a["n_items"], a["chunk"],
                                                 a["master"], a["m"], a["v"], s["c"], s["lr"], b1, b2, s["eps"], s["lr"] * s["wd"], bias1, sb2,
                                                 t, self.stream())

    def flat_g(self, dt=torch.float64):
        return torch.cat([torch.zeros(n, dtype=dt, device=DEV) if g is None else g.to(dt) for g, n in zip(self.g, self.sizes)])

    def flat_p16(self):
        return torch.cat(self.p16)


def _torch_fp32_lines(g, p, m, v, t, c, lr, beta1, beta2, eps, wd):
    """the yardstick of the direct tests: the header's lines with torch's fp32 ops"""
    g = g * c
    p = p * (1.0 - lr * wd)
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    p = p - (lr / (1.0 - beta1 ** t)) * m / (v.sqrt() / math.sqrt(1.0 - beta2 ** t) + eps)
    return p, m, v


@pytest.mark.parametrize("t", [1, 3])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("shifts", [(0, 0), (1, 3), (2, 2), (4, 0)], ids=["g0p0", "g1p3", "g2p2", "g4p0"])
@pytest.mark.parametrize("sizes", R.SIZE_LISTS, ids=IDS)
def test_entry_points_write_every_element(sizes, shifts, dtype, t):
    """NaN-filled 16-bit parameters and workspace, non-zero moments, the second tensor (where there is one) without a gradient: S, p, m, v
    meet the 4 x rule against float64, every partial and every 16-bit parameter is written, and the 16-bit parameter is the rounding of the
    fp32 value as stored."""
    pr = _Problem(sizes, dtype, g_shift=shifts[0], p_shift=shifts[1], seed=3, none_at=(1,) if len(sizes) > 1 else ())
    g64, g32 = pr.flat_g(), pr.flat_g(torch.float32)
    p0, m0, v0 = pr.master.clone(), pr.m.clone(), pr.v.clone()
    assert pr.sumsq() == 0 and pr.adam(t) == 0
    torch.cuda.synchronize()
    assert not torch.isnan(pr.ws[:pr.n_items]).any(), "a work item wrote no partial"
    k = pr.SCALARS
    rp, rm, rv = R.adam_elements(f64(g64), f64(p0), f64(m0), f64(v0), t, k["c"], k["lr"], k["beta1"], k["beta2"], k["eps"], k["wd"])
    tp, tm, tv = _torch_fp32_lines(g32, p0, m0, v0, t, k["c"], k["lr"], k["beta1"], k["beta2"], k["eps"], k["wd"])
    got = {"S": pr.S.float(), "master": pr.master, "exp_avg": pr.m, "exp_avg_sq": pr.v, "update": (pr.master.double() - p0.double()).float()}
    tor = {"S": (g32 * g32).sum().reshape(1), "master": tp, "exp_avg": tm, "exp_avg_sq": tv, "update": (tp.double() - p0.double()).float()}
    want = {"S": np.array([float((g64 * g64).sum())]), "master": rp, "exp_avg": rm, "exp_avg_sq": rv, "update": rp - f64(p0)}
    check_4x(f"fp16_optim entries {sizes} {shifts} t={t}", got, tor, want)
    p16 = pr.flat_p16()
    assert not torch.isnan(p16).any(), "a 16-bit parameter was not written"
    assert torch.equal(p16, pr.master.to(dtype))
    # nothing outside the tensors' slots was touched
    written = torch.zeros_like(pr.pbuf, dtype=torch.bool)
    for p in pr.p16:
        written[(p.data_ptr() - pr.pbuf.data_ptr()) // 2:][:p.numel()] = True
    assert torch.isnan(pr.pbuf[~written]).all()


@pytest.mark.parametrize("sizes", R.SIZE_LISTS, ids=IDS)
def test_equal_state_gives_equal_bits(sizes):
    runs = []
    for _ in range(2):
        pr = _Problem(sizes, torch.float16, g_shift=1, p_shift=0, seed=5)
        assert pr.sumsq() == 0 and pr.adam(3) == 0
        torch.cuda.synchronize()
        runs.append([pr.S.clone(), pr.master.clone(), pr.m.clone(), pr.v.clone(), pr.flat_p16()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    # ... and S does not depend on where the gradients lie: the same values at another address
    pr = _Problem(sizes, torch.float16, g_shift=4, p_shift=0, seed=5)
    assert pr.sumsq() == 0
    torch.cuda.synchronize()
    assert torch.equal(pr.S, runs[0][0])


def test_refusals_write_nothing():
    EINVAL, ENOSPC = -1, -2
    pr = _Problem([7, 1, 9], torch.float16, seed=7)
    p0, m0, v0 = pr.master.clone(), pr.m.clone(), pr.v.clone()
    for over in (dict(grads=None), dict(items=None), dict(ws=None), dict(S=None), dict(dtype=0), dict(dtype=3),
                 dict(chunk=0), dict(chunk=1000), dict(chunk=2048 + 4), dict(chunk=2048 * 33), dict(chunk=-2048)):
        assert pr.sumsq(**over) == EINVAL, over
    assert pr.sumsq(ws_bytes=pr.ws_bytes - 1) == ENOSPC and pr.sumsq(ws_bytes=0) == ENOSPC
    for over in (dict(grads=None), dict(params=None), dict(offsets=None), dict(items=None), dict(master=None), dict(m=None), dict(v=None),
                 dict(dtype=0), dict(master=pr.master.data_ptr() + 4), dict(m=pr.m.data_ptr() + 8), dict(v=pr.v.data_ptr() + 12),
                 dict(chunk=0), dict(chunk=1000), dict(chunk=2048 * 33), dict(step=0), dict(step=-1),
                 dict(beta1=1.0), dict(beta1=-0.1), dict(beta2=1.0), dict(beta2=1.5), dict(beta2=float("nan"))):
        assert pr.adam(1, **over) == EINVAL, over
    assert isinstance(pr.lib.dsp_last_error(), bytes) and b"fp16_optim" in pr.lib.dsp_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(pr.ws).all() and torch.isnan(pr.S).all() and torch.isnan(pr.pbuf).all()          # the poison is still there
    assert torch.equal(pr.master, p0) and torch.equal(pr.m, m0) and torch.equal(pr.v, v0)
    # an empty problem is fine, whatever the pointers
    assert pr.sumsq(N=0, grads=None, items=None, ws=None, S=None, n_items=0, ws_bytes=0) == 0
    assert pr.sumsq(n_items=0) == 0
    assert pr.adam(1, N=0, grads=None, params=None, offsets=None, items=None, master=None, m=None, v=None, n_items=0) == 0
    assert pr.adam(1, n_items=0) == 0
    torch.cuda.synchronize()
    assert torch.isnan(pr.S).all() and torch.isnan(pr.pbuf).all() and torch.equal(pr.master, p0)


# ---------------------------------------------------------------------------------------------------- overflow
@pytest.mark.parametrize("where", ["inf-in-the-one-element-tensor", "nan-in-the-last-element"])
def test_overflow_skips_the_step_and_leaves_the_state(where):
    from daspeech_amd.fp16_trainer import FP16FlatOptimizer
    sizes = [1, 4099, 1, 64]
    params = _make_params(sizes, 2)
    opt = FP16FlatOptimizer(params, lr=LR, hip_step=True, init_scale=SCALE)

    def set_grads(seed):
        for p, v in zip(params, _grad_values(sizes, seed)):
            p.grad = v.to(DEV)

    set_grads(20)
    assert opt.step() is True and opt.step_count == 1                           # non-zero moments before the overflow
    set_grads(21)
    if where.startswith("inf"):
        params[0].grad[0] = float("inf")
    else:
        params[-1].grad[-1] = float("nan")
    before = [opt.master.detach().clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()] + [p.detach().clone() for p in params]
    scale = opt.scaler.loss_scale
    assert opt.step() is False
    assert opt.scaler.loss_scale == scale / 2 and opt.step_count == 1 and not math.isfinite(opt.last_grad_norm)
    after = [opt.master.detach(), opt.exp_avg, opt.exp_avg_sq] + [p.detach() for p in params]
    for a, b in zip(after, before):
        assert torch.equal(a, b)
    set_grads(22)
    assert opt.step() is True and opt.step_count == 2 and math.isfinite(opt.last_grad_norm)
    assert not torch.equal(opt.master.detach(), before[0])
    for p, mv in zip(params, opt._mviews):
        assert torch.equal(p.data, mv.half())


# ---------------------------------------------------------------------------------------------------- a small real model
def test_small_model_trains_with_the_hip_step():
    from daspeech_amd.criterions import s2s_dag_fastspeech2_loss
    from daspeech_amd.fp16_trainer import FP16FlatOptimizer, half_sample
    from daspeech_amd.synthetic import make_s2st_batch
    from tests.test_gpu_model import small_model
    model = small_model().half().train()
    batch = half_sample(make_s2st_batch(3, "cuda", seed=2, min_frames=120, max_frames=160))
    opt = FP16FlatOptimizer(model.parameters(), lr=3e-4, init_scale=SCALE, hip_step=True)
    assert opt.hip_step is True and opt.master.grad is None
    # a twin on the torch path from the same initial state, for the first step
    twin = [torch.nn.Parameter(p.detach().clone()) for p in opt.params]
    tor = FP16FlatOptimizer(twin, lr=3e-4, init_scale=SCALE, hip_step=False)
    losses = []
    for i in range(3):
        opt.zero_grad()
        torch.manual_seed(7)                                   # same glancing and dropout draws: comparable losses
        loss, log = s2s_dag_fastspeech2_loss(model, batch, glat_p="0.5:0.1@200k", update_num=100000)
        assert torch.isfinite(loss)
        opt.backward(loss)
        if i == 0:
            rec = [None if p.grad is None else p.grad.detach().clone() for p in opt.params]          # one recorded set of gradients
            ref = R.RefOptimizer([f64(p) for p in opt.params], 3e-4, (0.9, 0.999), 1e-8, 0.01, 1.0)
            p_before = opt.master.detach().clone()
        assert opt.step() is True and np.isfinite(opt.last_grad_norm)
        if i == 0:
            for p, g in zip(twin, rec):
                p.grad = g
            assert tor.step() is True
            nv, ok = ref.step([None if g is None else f64(g) for g in rec], 1.0, SCALE)
            assert ok
            st = tor.opt.state[tor.master]
            got = {"nv": torch.tensor([opt.last_grad_norm], dtype=torch.float32), "master": opt.master.detach(), "exp_avg": opt.exp_avg,
                   "exp_avg_sq": opt.exp_avg_sq, "update": (opt.master.detach().double() - p_before.double()).float()}
            yard = {"nv": torch.tensor([tor.last_grad_norm], dtype=torch.float32), "master": tor.master.detach(), "exp_avg": st["exp_avg"],
                    "exp_avg_sq": st["exp_avg_sq"], "update": (tor.master.detach().double() - p_before.double()).float()}
            want = {"nv": np.array([nv]), "master": ref.master, "exp_avg": ref.exp_avg, "exp_avg_sq": ref.exp_avg_sq,
                    "update": ref.master - f64(p_before)}
            check_4x("fp16_optim small model step 1", got, yard, want)
        losses.append(float(loss))
    assert losses[2] < losses[0], losses
    for p, mv in zip(opt.params, opt._mviews):
        assert torch.equal(p.data, mv.half())
