"""CPU-side checks of the fp16 trainer's HIP optimizer step: the float64 restatement the GPU tests measure against
(tests/util_fp16_optim_ref.py) agrees with torch.optim.AdamW in float64; the work-item builder covers every element once; the workspace
question; which parameter lists are served; the module switch.  No device call."""
import numpy as np
import pytest
import torch

from tests import util_fp16_optim_ref as R


@pytest.mark.parametrize("clip_norm", [1.0, None])
def test_restatement_matches_torch_adamw_in_float64(clip_norm):
    """three steps, clipping active (the gradients' norm is far above 1) and inactive, the middle tensor without a gradient in step 2: its
    segment of the flat gradient is zero, so it decays and its moments decay — torch gets that as zeros in the flat gradient"""
    rng = np.random.default_rng(0)
    sizes = [7, 1, 9]
    params = [rng.standard_normal(n) for n in sizes]
    lr, betas, eps, wd, scale, mult = 0.1, (0.9, 0.999), 1e-8, 0.01, 128.0, 0.5
    ref = R.RefOptimizer(params, lr, betas, eps, wd, clip_norm)
    flat = torch.nn.Parameter(torch.from_numpy(np.concatenate(params)).clone())
    opt = torch.optim.AdamW([flat], lr=lr, betas=betas, eps=eps, weight_decay=wd)
    for step in range(3):
        grads = [rng.standard_normal(n) * 400.0 for n in sizes]
        if step == 1:
            grads[1] = None
        nv, ok = ref.step(grads, mult, scale)
        assert ok
        g = torch.from_numpy(ref.flat_grad(grads)) * (mult / scale)
        tn = float(torch.linalg.vector_norm(g))
        assert abs(nv - tn) <= 1e-12 * tn
        assert (tn > 1.0)
        if clip_norm and tn > clip_norm:
            g = g * (clip_norm / (tn + 1e-6))
        flat.grad = g
        opt.step()
        st = opt.state[flat]
        for name, got, want in (("master", ref.master, flat.detach()), ("exp_avg", ref.exp_avg, st["exp_avg"]),
                                ("exp_avg_sq", ref.exp_avg_sq, st["exp_avg_sq"])):
            err = float(np.abs(got - want.numpy()).max())
            assert err <= 1e-12, (step, name, err)
    p16 = ref.params16()
    assert [x.size for x in p16] == sizes and all(x.dtype == np.float16 for x in p16)
    assert np.array_equal(np.concatenate(p16), ref.master.astype(np.float32).astype(np.float16))


def test_restatement_reports_an_overflow_and_leaves_the_state():
    ref = R.RefOptimizer([np.ones(3), np.ones(1)], 0.1)
    before = ref.master.copy()
    for bad in (np.inf, np.nan):
        nv, ok = ref.step([np.ones(3), np.array([bad])], 1.0, 128.0)
        assert not ok and not np.isfinite(nv) and ref.t == 0 and np.array_equal(ref.master, before)


@pytest.mark.parametrize("sizes", R.SIZE_LISTS, ids=lambda s: "-".join(map(str, s)))
def test_work_items_cover_every_element_once(sizes):
    from daspeech_amd.fp16_trainer import build_work_items
    items = build_work_items(sizes, R.CHUNK)
    assert items == R.naive_items(sizes, R.CHUNK)
    assert items == build_work_items(list(sizes), R.CHUNK)                      # the order is a function of the sizes alone
    seen = [np.zeros(n, dtype=np.int64) for n in sizes]
    for ti, first, cnt in items:
        assert 1 <= cnt <= R.CHUNK
        assert 0 <= first and first + cnt <= sizes[ti]                          # no item crosses a tensor
        seen[ti][first:first + cnt] += 1
    assert all((s == 1).all() for s in seen)
    assert items == sorted(items)                                               # tensors in order, elements ascending
    # cut in FLAT index space: only a tensor's first item may start off the chunk grid
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    for ti, first, cnt in items:
        assert first == 0 or (offs[ti] + first) % R.CHUNK == 0


def test_work_items_of_nothing_and_of_empty_tensors():
    from daspeech_amd.fp16_trainer import build_work_items
    assert build_work_items([], 2048) == []
    assert build_work_items([0, 3, 0], 2048) == [(1, 0, 3)]
    with pytest.raises(ValueError):
        build_work_items([3], 0)


def test_workspace_bytes_properties():
    from daspeech_amd import _lib
    lib = _lib.load()
    ws = lib.dsp_fp16_optim_workspace_bytes
    assert ws(0) == 0 and ws(-5) == 0
    prev = 0
    for n in (1, 2, 3, 4, 5, 17, 1000, 45697, 2 ** 31 - 1):
        b = ws(n)
        assert b % 16 == 0 and b >= 4 * n and b >= prev, (n, b)
        prev = b


def test_cpu_parameters_are_not_served():
    from daspeech_amd.fp16_trainer import FP16FlatOptimizer
    params = [torch.nn.Parameter(torch.randn(5).half()), torch.nn.Parameter(torch.randn(2, 3).half())]
    opt = FP16FlatOptimizer(params, hip_step=None)
    assert opt.hip_step is False and opt.master.grad is not None and isinstance(opt.opt, torch.optim.AdamW)
    assert FP16FlatOptimizer(params, hip_step=False).hip_step is False
    with pytest.raises(RuntimeError, match="hip_step=True"):
        FP16FlatOptimizer(params, hip_step=True)


def test_switch_returns_the_previous_value():
    from daspeech_amd import fp16_trainer as F
    assert F.FUSED_STEP_HIP is True
    try:
        assert F.set_fused_step_hip(False) is True and F.FUSED_STEP_HIP is False
        assert F.set_fused_step_hip(False) is False
        assert F.set_fused_step_hip(True) is False and F.FUSED_STEP_HIP is True
    finally:
        F.set_fused_step_hip(True)
