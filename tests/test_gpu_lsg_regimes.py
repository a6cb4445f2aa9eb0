"""The fp32 / fp16 / bf16 logsoftmax-gather kernels (csrc/logsoftmax_gather.hip) against the float64 oracle at every launch regime of
launch_fwd / launch_bwd — the table, inputs, references and bounds of tests/util_lsg_regimes.py (checked on the CPU by
tests/test_lsg_regimes_ref.py, buffer extents included).  Everything goes through the four C entry points:

  forward   stats mode, read-only mode and write-softmax mode; `match` bit-identical across the index layouts (dense [B,L,S], storage [B,S,L];
            stride-0 expand against its dense copy) and the output layouts (pitched [B,S,ld], dense [B,L,S]) — the reductions have a fixed
            order; the row maximum of the statistics exact; logits bit-unchanged unless the softmax is asked for; guard rows around the
            logits, pitch columns, and guard floats behind `match` and the statistics untouched
  backward  from the stored softmax and from the logits + row statistics, each in both gradient layouts (gsj == 1, dense [B,L,S]) with both
            index layouts, within the bound (LDS float atomics on a repeated token have no fixed order)
  refusals  S past the forward's LDS staging, V past the backward's LDS row image: DSP_EINVAL, the error text set, nothing written.

Every check prints `LSG <row> <family> <quantity> err err32 bound`; profiles/lsg_regimes.txt keeps the worst of each family."""
import ctypes

import numpy as np
import pytest
import torch

from tests import util_lsg_regimes as U

pytestmark = pytest.mark.gpu

GUARD_VALUE = 1.25
EINVAL_RC = -1


def dev():
    return torch.device("cuda:0")


def lib():
    from daspeech_amd import _lib
    return _lib.load()


def stream():
    from daspeech_amd import _lib
    return _lib.current_stream_handle()


def i64(v):
    return ctypes.c_int64(int(v))


class Logits:
    """The [B,L,V] block of a case inside a buffer with guard rows on either side (tests/util_lsg_regimes.logits_layout)."""

    def __init__(self, case, x):
        self.case, self.dt = case, U.DTYPES[case.dtype]
        self.n, self.first, self.guard = U.logits_layout(case)
        self.count = case.B * case.L * case.V
        self.flat = torch.full((self.n,), GUARD_VALUE, dtype=self.dt, device=dev())
        assert self.flat.data_ptr() % 16 == 0
        self.flat[self.first:self.first + self.count] = torch.from_numpy(x).reshape(-1).to(self.dt)

    def clone(self):
        other = object.__new__(Logits)
        other.__dict__.update(self.__dict__)
        other.flat = self.flat.clone()
        assert other.flat.data_ptr() % 16 == 0
        return other

    def ptr(self):
        return ctypes.c_void_p(self.flat.data_ptr() + self.first * self.flat.element_size())

    def bits(self):
        return self.flat.view(torch.int32 if self.dt == torch.float32 else torch.int16).cpu().numpy()

    def block(self):
        c = self.case
        return self.flat[self.first:self.first + self.count].float().cpu().numpy().reshape(c.B, c.L, c.V)

    def guards_intact(self, orig_bits):
        b = self.bits()
        return np.array_equal(b[:self.first], orig_bits[:self.first]) and np.array_equal(b[self.first + self.count:], orig_bits[self.first + self.count:])


def _offsets(case, st):
    return (np.arange(case.B)[:, None, None] * st[0] + np.arange(case.L)[None, :, None] * st[1] + np.arange(case.S)[None, None, :] * st[2])


def _idx_dev(case, layout, values):
    numel, st = U.idx_layout(case, layout)
    assert U.max_offset(case, st) < numel
    vals = np.broadcast_to(values, (case.B, case.L, case.S))
    return torch.from_numpy(U.place(vals, numel, st, 0, np.int64)).to(dev()), st


def forward(case, lg, idx_layout, idx_values, out_layout, mode):
    """One forward launch -> (rc, match [B,L,S] float32, statistics [B,L,2] or None).  Asserts that nothing but match[b,j,s] was written into
    the NaN-filled output buffer (pitch columns and 64 guard floats included), nor behind the statistics."""
    B, L, V, S = case.B, case.L, case.V, case.S
    ib, ist = _idx_dev(case, idx_layout, idx_values)
    numel, ost, _ = U.out_layout(case, out_layout)
    assert U.max_offset(case, ost) < numel - U.GUARD_FLOATS
    ob = torch.full((numel,), float("nan"), dtype=torch.float32, device=dev())
    code = U.CODES[case.dtype]
    a = (lg.ptr(), code, ctypes.c_void_p(ib.data_ptr()), i64(ist[0]), i64(ist[1]), i64(ist[2]),
         ctypes.c_void_p(ob.data_ptr()), i64(ost[0]), i64(ost[1]), i64(ost[2]))
    stats = None
    if mode == "stats":
        sb = torch.full((B * L * 2 + U.GUARD_FLOATS,), float("nan"), dtype=torch.float32, device=dev())
        rc = lib().dsp_logsoftmax_gather_stats(*a, ctypes.c_void_p(sb.data_ptr()), B, L, V, S, stream())
    else:
        rc = lib().dsp_logsoftmax_gather(*a, B, L, V, S, 1 if mode == "ws" else 0, stream())
    torch.cuda.synchronize()
    out = ob.cpu().numpy()
    if rc != 0:
        assert np.isnan(out).all(), "a refused launch wrote into match"
        return rc, None, None
    off = _offsets(case, ost)
    written = np.zeros(numel, bool)
    written[off.ravel()] = True
    assert np.isnan(out[~written]).all(), "pitch columns / guard floats behind match were written"
    if mode == "stats":
        sv = sb.cpu().numpy()
        assert np.isnan(sv[B * L * 2:]).all(), "guard floats behind the statistics were written"
        stats = sv[:B * L * 2].reshape(B, L, 2)
        assert not np.isnan(stats).any()
    return rc, out[off], stats


def backward(case, lg, idx_layout, idx_values, g_layout, g_values, stats):
    B, L, V, S = case.B, case.L, case.V, case.S
    ib, ist = _idx_dev(case, idx_layout, idx_values)
    numel, gst = U.grad_layout(case, g_layout)
    assert U.max_offset(case, gst) < numel
    gb = torch.from_numpy(U.place(g_values, numel, gst, 0.0, np.float32)).to(dev())
    a = (lg.ptr(), U.CODES[case.dtype], ctypes.c_void_p(ib.data_ptr()), i64(ist[0]), i64(ist[1]), i64(ist[2]),
         ctypes.c_void_p(gb.data_ptr()), i64(gst[0]), i64(gst[1]), i64(gst[2]))
    if stats is None:
        rc = lib().dsp_logsoftmax_gather_bwd(*a, B, L, V, S, stream())
    else:
        sb = torch.from_numpy(np.ascontiguousarray(stats, np.float32)).to(dev())
        rc = lib().dsp_logsoftmax_gather_bwd_lazy(*a, ctypes.c_void_p(sb.data_ptr()), B, L, V, S, stream())
    torch.cuda.synchronize()
    return rc


def report(case, family, what, got, ref64, ref32, bound):
    ratio, err, bnd = U.worst(got, ref64, bound)
    fin = np.isfinite(ref64)
    err32 = float(np.abs(np.where(fin, ref32, 0.0).astype(np.float64) - np.where(fin, ref64, 0.0)).max())
    print(f"LSG {case.tag} {U.FAMILY_NAMES[family]} {what}: err {err:.3e} err32 {err32:.3e} bound {bnd:.3e}  (largest err / bound {ratio:.3f})")
    assert ratio <= 1.0, (case.tag, what, ratio, err, bnd)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.int32), np.ascontiguousarray(b, np.float32).view(np.int32))


def last_error():
    return lib().dsp_last_error().decode()


@pytest.mark.parametrize("case", [c for c in U.CASES if c.fwd != U.EINVAL], ids=lambda c: c.tag)
def test_case(case):
    inp, ref = U.make_inputs(case.tag), U.references(case.tag)
    B, L, V, S = case.B, case.L, case.V, case.S
    ffam = case.fwd[0]
    assert U.case_plan(case, 0)[:4] == tuple(case.fwd)
    orig = Logits(case, inp.x)
    orig_bits = orig.bits()
    assert np.array_equal(orig.block(), inp.x)
    mbound = U.match_bound(case, ref.match64, ref.match32, inp.row_scale)

    # ---- forward, statistics mode: dense per-row indices, pitched output
    la = orig.clone()
    rc, m_a, st = forward(case, la, "dense_bls", inp.idx, "pitched", "stats")
    assert rc == 0, last_error()
    assert np.array_equal(la.bits(), orig_bits), "the statistics forward wrote into the logits"
    report(case, ffam, "match", m_a, ref.match64, ref.match32, mbound)
    assert np.array_equal(st[..., 0], inp.x.max(axis=-1)), "the row maximum is exact"
    report(case, ffam, "1/s", st[..., 1], ref.inv64, ref.inv32, U.inv_bound(ref.inv64, ref.inv32))

    # ---- forward, read-only mode: indices stored [B,S,L], the reference's [B,L,S] output
    rc, m_b, _ = forward(case, la, "stored_bsl", inp.idx, "dense_bls", "ro")
    assert rc == 0, last_error()
    assert np.array_equal(la.bits(), orig_bits), "the read-only forward wrote into the logits"
    assert same_bits(m_a, m_b), "match differs between the index / output layouts"

    # ---- forward, softmax written in place: both layout pairs
    lc, lc2 = orig.clone(), orig.clone()
    rc, m_c, _ = forward(case, lc, "dense_bls", inp.idx, "pitched", "ws")
    assert rc == 0, last_error()
    rc, m_c2, _ = forward(case, lc2, "stored_bsl", inp.idx, "dense_bls", "ws")
    assert rc == 0, last_error()
    assert same_bits(m_a, m_c) and same_bits(m_a, m_c2), "match differs between the forward modes"
    assert lc.guards_intact(orig_bits) and lc2.guards_intact(orig_bits), "guard rows around the logits were written"
    assert np.array_equal(lc.bits(), lc2.bits()), "the stored softmax differs between the layouts"
    sm_dev = lc.block()
    assert not np.isnan(sm_dev).any() and not np.isinf(sm_dev).any()
    report(case, ffam, "softmax", sm_dev, ref.sm64, ref.sm32, U.softmax_bound(case, ref.sm64, ref.sm32))

    # ---- forward with one target row per sample: the stride-0 expand against its dense copy
    sh64, _, sh32, _ = U.forward_refs(inp.x, inp.shared_c)
    rc, m_e, _ = forward(case, la, "expand", inp.shared, "pitched", "ro")
    assert rc == 0, last_error()
    rc, m_d, _ = forward(case, la, "dense_bls", inp.shared, "dense_bls", "ro")
    assert rc == 0, last_error()
    assert same_bits(m_e, m_d), "match differs between the stride-0 expand and its dense copy"
    report(case, ffam, "match(expand)", m_e, sh64, sh32, U.match_bound(case, sh64, sh32, inp.row_scale))
    assert np.array_equal(la.bits(), orig_bits)

    # ---- backward
    if case.bwd == U.EINVAL:
        for stats, name in ((None, "logsoftmax_gather_bwd"), (st, "logsoftmax_gather_bwd")):
            before = lc.bits()
            assert backward(case, lc, "dense_bls", inp.idx, "bsl", inp.g, stats) == EINVAL_RC
            assert name in last_error() and str(V) in last_error()
            assert np.array_equal(lc.bits(), before), "a refused backward wrote into the buffer"
        return
    bfam = case.bwd[0]
    assert U.case_plan(case, 1)[:4] == tuple(case.bwd)
    ge64, ge32 = U.backward_refs(sm_dev, inp.idxc, inp.g)                  # from the device's own stored softmax
    ebound = U.grad_bound(case, ge64, ge32, U.grad_scale_rows(sm_dev, inp.idxc, inp.g))
    lbound = U.grad_bound(case, ref.glazy64, ref.glazy32, U.grad_scale_rows(ref.sm64, inp.idxc, inp.g))
    le, le2 = orig.clone(), orig.clone()
    for lg, il, gl, stats, what, r64, r32, bound in (
            (lc, "dense_bls", "bsl", None, "grad(eager, gsj=1)", ge64, ge32, ebound),
            (lc2, "stored_bsl", "dense_bls", None, "grad(eager, dense g)", ge64, ge32, ebound),
            (le, "dense_bls", "bsl", st, "grad(lazy, gsj=1)", ref.glazy64, ref.glazy32, lbound),
            (le2, "stored_bsl", "dense_bls", st, "grad(lazy, dense g)", ref.glazy64, ref.glazy32, lbound)):
        assert backward(case, lg, il, inp.idx, gl, inp.g, stats) == 0, last_error()
        assert lg.guards_intact(orig_bits), "guard rows around the buffer were written by the backward"
        got = lg.block()
        assert not np.isnan(got).any() and not np.isinf(got).any()
        report(case, bfam, what, got, r64, r32, bound)


def test_forward_refuses_an_s_beyond_its_lds_staging():
    case = U.BY_TAG["f32-S38401-fwd-refused"]
    assert case.fwd == U.EINVAL and U.case_plan(case, 0) == U.EINVAL
    inp = U.make_inputs(case.tag)
    lg = Logits(case, inp.x)
    bits = lg.bits()
    for mode in ("ws", "ro", "stats"):
        rc, _, _ = forward(case, lg, "dense_bls", inp.idx, "pitched", mode)           # (asserts that `match` stayed NaN)
        assert rc == EINVAL_RC and "logsoftmax_gather" in last_error() and "38401" in last_error()
        assert np.array_equal(lg.bits(), bits)


def test_empty_batches_are_no_ops():
    case = U.BY_TAG["f32-regl2"]
    inp = U.make_inputs(case.tag)
    lg = Logits(case, inp.x)
    bits = lg.bits()
    ib, ist = _idx_dev(case, "dense_bls", inp.idx)
    ob = torch.full((64,), float("nan"), device=dev())
    gb = torch.ones((64,), device=dev())
    sb = torch.full((64,), float("nan"), device=dev())
    p = lambda t: ctypes.c_void_p(t.data_ptr())        # noqa: E731
    for B, L in ((0, case.L), (case.B, 0), (0, 0)):
        a = (lg.ptr(), 0, p(ib), i64(ist[0]), i64(ist[1]), i64(ist[2]))
        assert lib().dsp_logsoftmax_gather(*a, p(ob), i64(1), i64(1), i64(1), B, L, case.V, case.S, 1, stream()) == 0
        assert lib().dsp_logsoftmax_gather_stats(*a, p(ob), i64(1), i64(1), i64(1), p(sb), B, L, case.V, case.S, stream()) == 0
        assert lib().dsp_logsoftmax_gather_bwd(*a, p(gb), i64(1), i64(1), i64(1), B, L, case.V, case.S, stream()) == 0
        assert lib().dsp_logsoftmax_gather_bwd_lazy(*a, p(gb), i64(1), i64(1), i64(1), p(sb), B, L, case.V, case.S, stream()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(lg.bits(), bits) and torch.isnan(ob).all() and torch.isnan(sb).all()


@pytest.mark.parametrize("lazy", [False, True], ids=["eager", "lazy"])
@pytest.mark.parametrize("case", [c for c in U.CASES if "ops" in c.flags], ids=lambda c: c.tag)
def test_operator_with_per_row_targets_under_autograd(case, lazy):
    """custom_ops.dag_logsoftmax_gather_inplace with a select_idx of its own per vertex: one row of the table per kernel family."""
    from daspeech_amd import custom_ops
    inp, ref = U.make_inputs(case.tag), U.references(case.tag)
    prev = custom_ops.set_lazy_softmax(lazy)
    try:
        x = torch.from_numpy(inp.x).to(U.DTYPES[case.dtype]).to(dev()).requires_grad_()
        work = x.clone()
        out_x, match = custom_ops.dag_logsoftmax_gather_inplace(work, torch.from_numpy(inp.idx).to(dev()))
        held = out_x.detach().float().cpu().numpy()
        report(case, case.fwd[0], f"operator match({'lazy' if lazy else 'eager'})", match.detach().cpu().numpy(), ref.match64, ref.match32,
               U.match_bound(case, ref.match64, ref.match32, inp.row_scale))
        (gx,) = torch.autograd.grad((match * torch.from_numpy(inp.g).to(dev())).sum(), [x])
        got = gx.float().cpu().numpy()
    finally:
        custom_ops.set_lazy_softmax(prev)
    if lazy:
        assert np.array_equal(held, inp.x), "the lazy forward left the logits alone"
        r64, r32, sm = ref.glazy64, ref.glazy32, ref.sm64
    else:
        report(case, case.fwd[0], "operator softmax", held, ref.sm64, ref.sm32, U.softmax_bound(case, ref.sm64, ref.sm32))
        r64, r32 = U.backward_refs(held, inp.idxc, inp.g)
        sm = held
    report(case, case.bwd[0], f"operator grad({'lazy' if lazy else 'eager'})", got, r64, r32,
           U.grad_bound(case, r64, r32, U.grad_scale_rows(sm, inp.idxc, inp.g)))
