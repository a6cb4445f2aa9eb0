"""GPU tests of the optimizer step that waits for nothing (FP16FlatOptimizer(device_scaler=True); dsp_fp16_optim_scale_step and
dsp_fp16_optim_adam_step_state, include/daspeech_optim.h) and of state_dict / load_state_dict of the HIP step.

Most checks are bit equality: the state update against its plain-float mirror (tests/util_optim_state_ref.py), the Adam entry that reads the
state against the existing one fed the mirror's doubles, the class in device mode against the class in host mode, a graph replay against an
eager twin.  Where a tolerance is needed it is the 4 x rule (tests/util_4x_rule.py) against the float64 restatement, the host mode as the
yardstick.  Shapes: util_fp16_optim_ref.SIZE_LISTS at chunk 2048."""
import numpy as np
import pytest
import torch

from tests import util_fp16_optim_ref as R
from tests import util_optim_state_ref as M
from tests.test_gpu_fp16_optim import DEV, IDS, LR, MULT, SCALE, _Problem, _grad_values, _make_params, _odd_view, _strided_view
from tests.util_4x_rule import check_4x, f64

pytestmark = pytest.mark.gpu

EINVAL = -1
BETAS, EPS, WD, CLIP = (0.9, 0.999), 1e-8, 0.01, 1.0


def _F():
    from daspeech_amd import fp16_trainer
    return fp16_trainer


def _lib():
    from daspeech_amd import _lib
    return _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _same_bits(x, y):
    """equality of the bytes (the 16-bit buffer keeps its NaN poison between the tensors)"""
    as_int = torch.int16 if x.element_size() == 2 else torch.int32
    return torch.equal(x.view(as_int), y.view(as_int))


# ---------------------------------------------------------------------------------------------------- the state entry alone
def _device_state(mir):
    """a device state block holding what the mirror holds now"""
    F = _F()
    h = np.zeros(F.STATE_SLOTS, dtype=np.int64)
    d, f = h.view(np.float64), h.view(np.float32)
    d[F.SLOT_LOSS_SCALE], f[2 * F.SLOT_LOSS_SCALE_F32] = mir.loss_scale, mir.loss_scale
    h[F.SLOT_ITER], h[F.SLOT_LAST_OVERFLOW_ITER], h[F.SLOT_T] = mir.iter, mir.last_overflow_iter, mir.t
    d[F.SLOT_POW1], d[F.SLOT_POW2], d[F.SLOT_LR], d[F.SLOT_GRAD_MULT] = mir.pow1, mir.pow2, mir.lr, mir.grad_mult
    return torch.from_numpy(h).to(DEV)


def _scale_step(S, state, mir):
    return _lib().dsp_fp16_optim_scale_step(S.data_ptr(), state.data_ptr(), mir.beta1, mir.beta2, mir.eps, mir.weight_decay, mir.clip_norm,
                                            mir.scale_factor, mir.scale_window, mir.min_loss_scale, _stream())


def _assert_state_is_mirror(state, mir, tag):
    F = _F()
    h = state.cpu().numpy()
    d, f, i32 = h.view(np.float64), h.view(np.float32), h.view(np.int32)
    for name, slot, want in (("loss_scale", F.SLOT_LOSS_SCALE, mir.loss_scale), ("pow1", F.SLOT_POW1, mir.pow1), ("pow2", F.SLOT_POW2, mir.pow2),
                             ("lr", F.SLOT_LR, mir.lr), ("grad_mult", F.SLOT_GRAD_MULT, mir.grad_mult), ("grad_norm", F.SLOT_GRAD_NORM, mir.grad_norm)):
        assert int(h[slot]) == M.bits(want), f"{tag} {name}: device {d[slot]!r} mirror {want!r}"
    for name, slot, want in (("iter", F.SLOT_ITER, mir.iter), ("last_overflow_iter", F.SLOT_LAST_OVERFLOW_ITER, mir.last_overflow_iter),
                             ("t", F.SLOT_T, mir.t)):
        assert int(h[slot]) == want, f"{tag} {name}"
    assert f[2 * F.SLOT_LOSS_SCALE_F32].tobytes() == np.float32(mir.loss_scale).tobytes(), f"{tag} loss_scale_f32"
    assert int(i32[2 * F.SLOT_APPLIED]) == mir.applied and int(i32[2 * F.SLOT_FLOOR_HIT]) == mir.floor_hit, f"{tag} applied / floor_hit"
    got = f[2 * F.SLOT_SCALARS:2 * F.SLOT_SCALARS + F.N_SCALARS]
    for name, g, w in zip(M.SCALAR_NAMES, got, mir.scalars):
        assert g.tobytes() == np.float32(w).tobytes(), f"{tag} AdamScalars.{name}: device {g!r} mirror {w!r}"


@pytest.mark.parametrize("scale_window,min_loss_scale", [(2, 64.0), (3, 32.0)], ids=["window2", "window3"])
def test_state_update_is_the_mirror_bit_for_bit(scale_window, min_loss_scale):
    """The scripted S (small, clipping, inf, nan, negative, zero), one value at a time into the device double, the state update alone: every
    slot equals the mirror's after every step.  The floor is set so that the SECOND overflow in a row reaches it; the flag then stays.  The
    host rewrites lr before the last step, as a scheduler would."""
    mir = M.MirrorState(LR, BETAS, EPS, WD, CLIP, init_scale=SCALE, scale_window=scale_window, min_loss_scale=min_loss_scale, grad_mult=MULT)
    F = _F()
    state = _device_state(mir)
    S = torch.zeros(1, dtype=torch.float64, device=DEV)
    floor = []
    for k, s in enumerate(M.S_SCRIPT):
        if k == len(M.S_SCRIPT) - 1:
            mir.lr = 0.05
            state.view(torch.float64)[F.SLOT_LR:F.SLOT_LR + 1].fill_(0.05)
        S.fill_(s)
        assert _scale_step(S, state, mir) == 0
        mir.step(s)
        _assert_state_is_mirror(state, mir, f"window {scale_window} step {k + 1} (S = {s})")
        floor.append(mir.floor_hit)
    assert floor == [0, 0, 0, 1, 1, 1]
    assert mir.t == 3 and mir.iter == 6


def test_state_entries_refuse_bad_pointers_and_constants():
    mir = M.MirrorState(LR)
    state = _device_state(mir)
    before = state.clone()
    S = torch.ones(1, dtype=torch.float64, device=DEV)
    lib = _lib()

    def call(S_ptr=S.data_ptr(), st=state.data_ptr(), b1=0.9, b2=0.999, factor=2.0, window=2000):
        return lib.dsp_fp16_optim_scale_step(S_ptr, st, b1, b2, EPS, WD, CLIP, factor, window, 1e-4, _stream())

    for over in (dict(S_ptr=None), dict(st=None), dict(S_ptr=S.data_ptr() + 4), dict(st=state.data_ptr() + 4), dict(b1=1.0), dict(b2=-0.5),
                 dict(b2=float("nan")), dict(factor=1.0), dict(factor=float("nan")), dict(window=0)):
        assert call(**over) == EINVAL, over
    assert b"fp16_optim_scale_step" in lib.dsp_last_error()
    pr = _Problem([7, 1, 9], torch.float16, seed=7)
    p0 = pr.master.clone()

    def adam(st, **over):
        a = dict(grads=pr.gptr.data_ptr(), params=pr.pptr.data_ptr(), dtype=pr.code, offsets=pr.offs.data_ptr(), N=pr.N,
                 items=pr.items.data_ptr(), n_items=pr.n_items, chunk=R.CHUNK, master=pr.master.data_ptr(), m=pr.m.data_ptr(), v=pr.v.data_ptr())
        a.update(over)
        return lib.dsp_fp16_optim_adam_step_state(a["grads"], a["params"], a["dtype"], a["offsets"], a["N"], a["items"], a["n_items"], a["chunk"],
                                                  a["master"], a["m"], a["v"], st, _stream())

    assert adam(None) == EINVAL and adam(state.data_ptr() + 4) == EINVAL
    assert b"fp16_optim_adam_step_state" in lib.dsp_last_error()
    for over in (dict(grads=None), dict(params=None), dict(offsets=None), dict(items=None), dict(master=None), dict(dtype=0),
                 dict(m=pr.m.data_ptr() + 8), dict(chunk=1000), dict(chunk=2048 * 33)):
        assert adam(state.data_ptr(), **over) == EINVAL, over
    assert adam(state.data_ptr(), N=0, grads=None, params=None, offsets=None, items=None, master=None, m=None, v=None, n_items=0) == 0
    assert adam(state.data_ptr(), n_items=0) == 0
    torch.cuda.synchronize()
    assert torch.equal(state, before) and torch.equal(pr.master, p0) and torch.isnan(pr.pbuf).all()


# ---------------------------------------------------------------------------------------------------- the Adam entry that reads the state
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("shifts", [(0, 0), (1, 3), (2, 2), (4, 0)], ids=["g0p0", "g1p3", "g2p2", "g4p0"])
@pytest.mark.parametrize("sizes", R.SIZE_LISTS, ids=IDS)
def test_adam_from_the_state_equals_adam_from_the_arguments(sizes, shifts, dtype):
    """Two equal problems (the second tensor, where there is one, without a gradient).  Two state updates bring the state to t = 2 with a
    clipping step; the existing entry gets the mirror's doubles, the new one the state: equal bits in master, both moments and the 16-bit
    parameters.  Then an overflow: with applied == 0 the new entry leaves all four arrays as they were."""
    none_at = (1,) if len(sizes) > 1 else ()
    a = _Problem(sizes, dtype, g_shift=shifts[0], p_shift=shifts[1], seed=3, none_at=none_at)
    b = _Problem(sizes, dtype, g_shift=shifts[0], p_shift=shifts[1], seed=3, none_at=none_at)
    assert torch.equal(a.master, b.master) and torch.equal(a.gbuf, b.gbuf)
    lib = _lib()
    mir = M.MirrorState(LR, BETAS, EPS, WD, CLIP, init_scale=SCALE, scale_window=2, grad_mult=MULT)
    state = _device_state(mir)
    S = torch.zeros(1, dtype=torch.float64, device=DEV)

    def adam_state():
        return lib.dsp_fp16_optim_adam_step_state(b.gptr.data_ptr(), b.pptr.data_ptr(), b.code, b.offs.data_ptr(), b.N, b.items.data_ptr(),
                                                  b.n_items, R.CHUNK, b.master.data_ptr(), b.m.data_ptr(), b.v.data_ptr(), state.data_ptr(),
                                                  _stream())

    for s in (0.25, 1.0e9):
        S.fill_(s)
        assert _scale_step(S, state, mir) == 0 and mir.step(s) == 1
        assert lib.dsp_fp16_optim_adam_step(a.gptr.data_ptr(), a.pptr.data_ptr(), a.code, a.offs.data_ptr(), a.N, a.items.data_ptr(), a.n_items,
                                            R.CHUNK, a.master.data_ptr(), a.m.data_ptr(), a.v.data_ptr(), *mir.doubles, mir.t, _stream()) == 0
        assert adam_state() == 0
        torch.cuda.synchronize()
        for name, x, y in (("master", a.master, b.master), ("exp_avg", a.m, b.m), ("exp_avg_sq", a.v, b.v), ("p16", a.flat_p16(), b.flat_p16())):
            assert not torch.isnan(y).any(), f"{name}: an element never written"
            assert torch.equal(x, y), f"{name} differs at t = {mir.t}"
    assert torch.equal(b.flat_p16(), b.master.to(dtype))
    before = [b.master.clone(), b.m.clone(), b.v.clone(), b.pbuf.clone()]
    S.fill_(float("inf"))
    assert _scale_step(S, state, mir) == 0 and mir.step(float("inf")) == 0
    assert adam_state() == 0
    torch.cuda.synchronize()
    _assert_state_is_mirror(state, mir, "after the overflow")
    for name, x, y in zip(("master", "exp_avg", "exp_avg_sq", "the 16-bit buffer"), before, [b.master, b.m, b.v, b.pbuf]):
        assert _same_bits(x, y), f"{name} changed on a skipped step"


# ---------------------------------------------------------------------------------------------------- the class: device mode against host mode
KW = dict(lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, clip_norm=CLIP, init_scale=SCALE, scale_window=2)


def _scaler_fields(opt):
    return opt.scaler.loss_scale, opt.scaler._iter, opt.scaler._last_overflow_iter, opt.step_count


def _arrays(opt):
    return [opt.master.detach(), opt.exp_avg, opt.exp_avg_sq] + [p.detach() for p in opt.params]


def _assert_equal_optimizers(a, b, tag):
    for name, x, y in zip(["master", "exp_avg", "exp_avg_sq"] + [f"param {i}" for i in range(len(a.params))], _arrays(a), _arrays(b)):
        assert torch.equal(x, y), f"{tag}: {name} differs"


def _six_step_values(sizes, step):
    """the 16-bit gradient values of step 1 .. 6 (None: no gradient): magnitudes 0.4 .. 0.8, whose unscaled norm stays below clip_norm 1 at
    these sizes; step 2 leaves the last tensor out, step 3 has one inf, step 5 is 1000 x larger and clips"""
    vals = _grad_values(sizes, 40 + step)
    vals = [v if step == 5 else (v.float() * 1e-3).half() for v in vals]
    if step == 2:
        vals[-1] = None
    if step == 3:
        vals[0][0] = float("inf")
    return vals


@pytest.mark.parametrize("sizes", R.SIZE_LISTS, ids=IDS)
def test_six_steps_device_mode_equals_host_mode(sizes):
    from daspeech_amd.fp16_trainer import FP16FlatOptimizer
    N = len(sizes)
    pd, ph = _make_params(sizes, 1), _make_params(sizes, 1)
    dev = FP16FlatOptimizer(pd, hip_step=True, device_scaler=True, **KW)
    host = FP16FlatOptimizer(ph, hip_step=True, **KW)
    assert dev.device_scaler is True and dev.hip_step is True and host.device_scaler is False
    ref = R.RefOptimizer([f64(p) for p in ph], LR, BETAS, EPS, WD, CLIP)
    applied_seq = []
    for step in range(1, 7):
        vals = _six_step_values(sizes, step)
        dev.zero_grad(); host.zero_grad()
        for i, v in enumerate(vals):
            if v is None:
                continue
            v = v.to(DEV)
            pd[i].grad = _odd_view(v) if i == 0 else (_strided_view(v) if i == 1 else v.clone())
            ph[i].grad = v.clone()
        scale = host.scaler.loss_scale
        assert dev.scaler.loss_scale == scale
        before_d, before_h, before_r = dev.master.detach().clone(), host.master.detach().clone(), ref.master.copy()
        versions = [p._version for p in pd]
        applied = dev.step(MULT)
        ok = host.step(MULT)
        assert torch.is_tensor(applied) and applied.dtype == torch.int32 and applied.dim() == 0 and applied.is_cuda
        assert int(applied) == int(ok), f"step {step}"
        applied_seq.append(int(applied))
        assert _scaler_fields(dev) == _scaler_fields(host), f"step {step}"
        nd = dev.last_grad_norm
        assert torch.is_tensor(nd) and nd.dtype == torch.float64 and nd.dim() == 0 and nd.is_cuda
        assert M.bits(float(nd)) == M.bits(host.last_grad_norm), f"step {step}: norm {float(nd)!r} vs {host.last_grad_norm!r}"
        assert (host.last_grad_norm > CLIP) == (step == 5) or step == 3
        _assert_equal_optimizers(dev, host, f"step {step}")
        nv, ref_ok = ref.step([None if v is None else f64(v) for v in vals], MULT, scale)
        assert ref_ok == ok
        if step in (1, 6):
            def pack(opt, before):
                return {"nv": torch.tensor([float(opt.last_grad_norm)], dtype=torch.float32), "master": opt.master.detach(),
                        "exp_avg": opt.exp_avg, "exp_avg_sq": opt.exp_avg_sq, "update": (opt.master.detach().double() - before.double()).float()}
            want = {"nv": np.array([nv]), "master": ref.master, "exp_avg": ref.exp_avg, "exp_avg_sq": ref.exp_avg_sq, "update": ref.master - before_r}
            check_4x(f"device scaler {sizes} step {step}", pack(dev, before_d), pack(host, before_h), want)
        if ok:
            assert all(p._version > v0 for p, v0 in zip(pd, versions))
            for p, mv in zip(pd, dev._mviews):
                assert torch.equal(p.data, mv.half())
    assert applied_seq == [1, 1, 0, 1, 1, 1]
    dev.check()                                                                              # the floor was not reached


def test_check_raises_once_the_floor_is_reached():
    from daspeech_amd.fp16_trainer import FP16FlatOptimizer
    params = _make_params([7, 1, 9], 1)
    opt = FP16FlatOptimizer(params, hip_step=True, device_scaler=True, init_scale=2.0 ** -12)      # the floor is 1e-4: 2^-13 is just above, 2^-14 below
    for p in params:
        p.grad = torch.full_like(p, float("nan"))
    assert int(opt.step()) == 0
    opt.check()
    assert int(opt.step()) == 0
    with pytest.raises(FloatingPointError, match="Minimum loss scale"):
        opt.check()


# ---------------------------------------------------------------------------------------------------- no host wait
def _products(params, xs):
    return sum((w * x).float().sum() for w, x in zip(params, xs))


def test_no_host_wait_in_backward_or_step():
    from daspeech_amd.fp16_trainer import FP16FlatOptimizer
    sizes = [7, 2049, 64]
    pd, ph = _make_params(sizes, 4), _make_params(sizes, 4)
    xs = [torch.randn(n, device=DEV).half() for n in sizes]
    dev = FP16FlatOptimizer(pd, hip_step=True, device_scaler=True, **KW)
    host = FP16FlatOptimizer(ph, hip_step=True, **KW)
    for opt, ps in ((dev, pd), (host, ph)):                                                  # warm-up: tables uploaded, kernels loaded
        opt.backward(_products(ps, xs))
        opt.step()
    held = [p.grad for p in pd]                                                              # keep the addresses taken: the next gradients are elsewhere
    first = [g.data_ptr() for g in held]
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    control = None
    try:
        torch.cuda.set_sync_debug_mode("error")
        for round_ in range(3):
            dev.zero_grad()
            dev.backward(_products(pd, xs))
            assert round_ > 0 or all(p.grad.data_ptr() != q for p, q in zip(pd, first))
            dev.step()
            dev.set_lr(LR * (round_ + 2))                                                    # a scheduler between steps: a slot write, no wait
        host.zero_grad()
        host.backward(_products(ph, xs))
        try:
            host.step()
        except RuntimeError as e:
            control = str(e)
    finally:
        torch.cuda.set_sync_debug_mode(old)
    assert control is not None and "synchroniz" in control, "the control (host mode reads the norm) did not raise"
    assert dev.step_count == 4 and all(torch.isfinite(p).all() for p in pd)


# ---------------------------------------------------------------------------------------------------- graph replay
def _static_setup(sizes, seed):
    from daspeech_amd.fp16_trainer import FP16FlatOptimizer
    params = _make_params(sizes, seed)
    opt = FP16FlatOptimizer(params, hip_step=True, device_scaler=True, **KW)
    for p in params:
        p.grad = torch.zeros_like(p)                                                         # static gradient tensors
    return params, opt


def test_graph_replay_of_step_equals_eager_steps():
    sizes = [8, 2047, 2048, 2049]
    pg, og = _static_setup(sizes, 6)
    pe, oe = _static_setup(sizes, 6)

    def fill(step, nan=False):
        vals = [(v.float() * 1e-3).half() for v in _grad_values(sizes, 60 + step)]
        if nan:
            vals[2][5] = float("nan")
        for ps in (pg, pe):
            for p, v in zip(ps, vals):
                p.grad.copy_(v)

    fill(0)
    og.step(MULT); oe.step(MULT)                                                             # one eager step: the pointer table holds these gradients
    g = torch.cuda.CUDAGraph()
    fill(1)
    with torch.cuda.graph(g):
        og.step(MULT)
    oe.step(MULT)                                                                            # the capture ran nothing: bring both to the same point
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(og._state, oe._state)
    _assert_equal_optimizers(og, oe, "first replay")
    seq = [1]
    for k in range(2, 5):
        fill(k, nan=(k == 2))
        g.replay()
        oe.step(MULT)
        torch.cuda.synchronize()
        assert torch.equal(og._state, oe._state), f"replay {k}: state slots differ"
        _assert_equal_optimizers(og, oe, f"replay {k}")
        seq.append(int(og._applied))
    assert seq == [1, 0, 1, 1] and og.step_count == 4 and og.scaler._iter == 5
    v0 = [p._version for p in pg]
    og.mark_params_updated()
    assert all(p._version == v + 1 for p, v in zip(pg, v0))
    # what a capture cannot take: gradient tensors the optimizer has not uploaded, and an input slot that would change inside the graph
    for p in pg:
        p.grad = torch.zeros_like(p)
    state = og._state.clone()
    dummy = torch.zeros(1, device=DEV)
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2):
        with pytest.raises(RuntimeError, match="run one eager step with these gradient tensors before capturing"):
            og.step(MULT)
        with pytest.raises(RuntimeError, match="before the capture and between replays"):
            og.step(0.25)
        dummy.add_(1.0)                                                                      # the capture ends normally, with one node
    torch.cuda.synchronize()
    assert torch.equal(og._state, state)                                                     # nothing was queued by the refused calls


def test_graph_replay_of_backward_and_step_uses_the_current_loss_scale():
    """No GEMM: loss = sum_i (w_i * x_i).float().sum() with static x_i, so dloss/dw_i = loss_scale * x_i in fp16.  Replay 1 has an x that
    overflows fp16 in the backward (128 * 1000 > 65504): the step is skipped and the scale halves.  Replay 2 must then produce the gradients
    of scale 64 — a graph that had frozen the host's 128.0 into the multiply would give twice the norm's S and other bits."""
    sizes = [7, 2049, 64]
    pg, og = _static_setup(sizes, 8)
    pe, oe = _static_setup(sizes, 8)
    xg = [torch.zeros(n, dtype=torch.float16, device=DEV) for n in sizes]
    xe = [torch.zeros(n, dtype=torch.float16, device=DEV) for n in sizes]
    gen = torch.Generator().manual_seed(9)
    x_normal = [torch.randn(n, generator=gen).half() for n in sizes]
    x_over = [x.clone() for x in x_normal]
    x_over[1][17] = 1000.0

    def set_x(vals):
        for xs in (xg, xe):
            for x, v in zip(xs, vals):
                x.copy_(v)

    def one(params, opt, xs):
        for p in params:
            p.grad.zero_()                                                                   # in place: the gradient tensors stay where they are
        opt.backward(_products(params, xs))
        opt.step()

    set_x(x_normal)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                                            # the warm-up of the capture recipe, on the capture's stream
        one(pg, og, xg)
    torch.cuda.current_stream().wait_stream(side)
    one(pe, oe, xe)
    ptrs = [p.grad.data_ptr() for p in pg]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        one(pg, og, xg)
    one(pe, oe, xe)
    g.replay()                                                                               # (bring both to the same point, as above)
    torch.cuda.synchronize()
    assert [p.grad.data_ptr() for p in pg] == ptrs
    assert torch.equal(og._state, oe._state) and og.scaler.loss_scale == SCALE * 2           # window 2: the second applied step doubles it
    scale = og.scaler.loss_scale
    set_x(x_over)
    g.replay(); one(pe, oe, xe)
    torch.cuda.synchronize()
    assert int(og._applied) == 0 and og.scaler.loss_scale == scale / 2 and torch.isinf(pg[1].grad[17])
    assert torch.equal(og._state, oe._state)
    set_x(x_normal)
    g.replay(); one(pe, oe, xe)
    torch.cuda.synchronize()
    assert int(og._applied) == 1
    for p, x in zip(pg, xg):
        assert torch.equal(p.grad, (torch.tensor(scale / 2, dtype=torch.float16, device=DEV) * x)), "the replay did not use the halved scale"
    assert M.bits(float(og.last_grad_norm)) == M.bits(float(oe.last_grad_norm))
    assert torch.equal(og._state, oe._state)
    _assert_equal_optimizers(og, oe, "replay after the overflow")


# ---------------------------------------------------------------------------------------------------- checkpoints
def _ckpt_step(opt, params, sizes, step):
    vals = [(v.float() * 1e-3).half() for v in _grad_values(sizes, 80 + step)]
    if step == 2:
        vals[-1][-1] = float("inf")
    for p, v in zip(params, vals):
        p.grad = v.to(DEV)
    return int(opt.step(MULT))


@pytest.mark.parametrize("save_mode,load_mode", [(False, False), (True, True), (False, True)], ids=["host-host", "device-device", "host-device"])
def test_state_dict_round_trip_continues_the_run(save_mode, load_mode):
    from daspeech_amd.fp16_trainer import FP16FlatOptimizer
    sizes = [1, 4099, 1, 64]
    ps = _make_params(sizes, 11)
    straight = FP16FlatOptimizer(ps, hip_step=True, device_scaler=load_mode, **KW)
    seq = [_ckpt_step(straight, ps, sizes, k) for k in range(1, 6)]
    assert seq == [1, 0, 1, 1, 1]
    p1 = _make_params(sizes, 11)
    first = FP16FlatOptimizer(p1, hip_step=True, device_scaler=save_mode, **KW)
    for k in range(1, 4):
        _ckpt_step(first, p1, sizes, k)
    sd = first.state_dict()
    assert sd["step_count"] == 2 and sd["iter"] == 3 and sd["last_overflow_iter"] == 1 and sd["sizes"] == sizes
    assert sd["master"].data_ptr() != first.master.data_ptr() and sd["exp_avg"].data_ptr() != first.exp_avg.data_ptr()
    p2 = _make_params(sizes, 11)
    second = FP16FlatOptimizer(p2, hip_step=True, device_scaler=load_mode, **KW)
    versions = [p._version for p in p2]
    second.load_state_dict(sd)
    assert all(p._version > v for p, v in zip(p2, versions))
    _assert_equal_optimizers(second, first, "after the load")
    assert _scaler_fields(second) == _scaler_fields(first)
    for k in range(4, 6):
        _ckpt_step(second, p2, sizes, k)
    _assert_equal_optimizers(second, straight, "two steps after the load")
    assert _scaler_fields(second) == _scaler_fields(straight)
    if load_mode:
        assert torch.equal(second._state, straight._state)
    # a dict of another problem is refused and leaves the optimizer as it is
    other = FP16FlatOptimizer(_make_params([7, 1, 9], 1), hip_step=True, device_scaler=load_mode, **KW)
    with pytest.raises(ValueError, match="load_state_dict"):
        other.load_state_dict(sd)
    bad = dict(sd, betas=(0.8, 0.999))
    with pytest.raises(ValueError, match="betas"):
        second.load_state_dict(bad)
    _assert_equal_optimizers(second, straight, "after the refused loads")
