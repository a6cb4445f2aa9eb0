"""The fp32 DAG kernels against the float64 oracle on batches that mix one full-size sample with tiny and mid-size ones: the case table, inputs and
references of tests/util_dag_skew.py (pinned on the CPU by tests/test_dag_skew_ref.py).  Every forward family, every backward path and every
alignment family of csrc/capi_dag.hip runs at every length pattern, in both sample orders; the error word (dag_strip.h:22-24) is read after every
launch.

Tolerances, the project's own (tests/test_gpu_dag_ops.py): alpha / beta / loss rtol 3e-6, atol 2e-5 T; gradients rtol 50 * 2e-5 T, atol 1e-7; paths
equal.  Every figure printed is the fraction of that tolerance used (`pytest -s`; profiles/dag_skew.txt holds a run).  A tensor beyond its tolerance
is not excused by hand: it may be at most 4 x as far from the fp64 oracle as the fp32 oracle is on the same inputs (U.yardstick: the reference's
own arithmetic, not the kernels).  A misplaced -inf, a NaN, a nonzero gradient outside the graph or a nonzero error word has no excuse."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

from tests import util_dag_skew as U

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def ops():
    from daspeech_amd import custom_ops
    return custom_ops


def lib():
    from daspeech_amd import _lib
    return _lib


def cu(a):
    return torch.from_numpy(np.array(a)).to(dev())                 # (a copy: the util's arrays are read-only)


def dev_inputs(cid, variant, order):
    inp = U.inputs(cid, variant, order)
    return cu(inp.match), cu(inp.links), cu(inp.out_len), cu(inp.tgt_len), cu(inp.w)


@contextlib.contextmanager
def pinned(**opts):
    """dsp_dag_set_option for the block; every option back to 0 (auto) afterwards"""
    try:
        for name, v in opts.items():
            lib().set_option(name, v)
        yield
    finally:
        for name in opts:
            lib().set_option(name, 0)


def status_ok(tag):
    assert lib().last_launch_status() == 0, f"{tag}: error word set (a halo wait hit the spin limit)"


def check(tag, cid, variant, got, ref, names):
    """each tensor inside its tolerance (or inside 4 x the fp32 oracle's distance from the fp64 oracle); -inf exactly where the oracle has it, no NaN"""
    case = U.BY_ID[cid]
    figs = {n: U.figure(got[n], getattr(ref, n), U.tol_of(case, n)) for n in names}
    print(f"dag-skew {tag}: " + "  ".join(f"{n} {v:.2e}" for n, v in figs.items()))
    over = [n for n, v in figs.items() if not v <= 1.0]
    if over and all(np.isfinite(figs[n]) for n in over):
        yard = U.yardstick(cid, variant)
        print(f"dag-skew {tag}: over the tolerance; fp32 oracle vs fp64 oracle: " + "  ".join(f"{n} {yard[n]:.2e}" for n in over))
        over = [n for n in over if not figs[n] <= 4.0 * yard[n]]
    assert not over, (tag, {n: figs[n] for n in over})
    return figs


def npy(t):
    return t.detach().cpu().numpy()


def poison(m, k):
    """The operators allocate their outputs with torch.empty, and the block the caching allocator hands back is usually the one the previous launch
    of the same shape left its (correct) results in.  NaN through blocks of those sizes first, so that an element a kernel does not write shows."""
    B, T, L = m.shape
    junk = [torch.full((B, T, (L + 3) & ~3), float("nan"), device=m.device) for _ in range(4)]
    junk += [torch.full(tuple(k.shape), float("nan"), device=m.device) for _ in range(2)]
    junk += [torch.full((B, L), -7, dtype=torch.long, device=m.device)]
    del junk


# ---------------------------------------------------------------------------------------------- forward

def forward(m, k, o, t, ndir):
    """ndir 2: alpha and beta in one launch (a gradient is wanted); 1: alpha only -> (loss, alpha, beta or None)"""
    if ndir == 2:
        m2 = m.clone().requires_grad_()
        poison(m, k)
        loss, (a, b) = ops().dag_loss_with_alpha_beta(m2, k, o, t)
        return loss.detach(), a, b
    poison(m, k)
    with torch.no_grad():
        loss, (a, _) = ops().dag_loss_with_alpha_beta(m, k, o, t)
        loss1 = ops().dag_loss(m, k, o, t)
    assert torch.equal(loss1, loss)
    return loss, a, None


FWD = [(c.cid, f, o) for c in U.CASES for f in c.fwd for o in U.ORDERS]


@pytest.mark.parametrize("cid,family,order", FWD, ids=["-".join(x) for x in FWD])
def test_forward_meets_the_oracle(cid, family, order):
    case, fam = U.BY_ID[cid], U.FAMILIES[family]
    with pinned(dp_path=fam.pin):
        assert bool(lib().load().dsp_dag_pitch_supported(0, case.L, case.TR)) == (family in ("strip4g", "strip2g", "strip1g"))
    for variant in case.variants:
        if variant == "ties":
            continue
        m, k, o, t, _ = dev_inputs(cid, variant, order)
        ref = U.reference(cid, variant, order)
        for mt in ((0, 1) if family == "dense_mfma" else (0,)):
            for ndir in (2, 1):
                tag = f"{cid}-{order}-{variant} {family} ndir {ndir}" + (f" dm_mt {mt}" if mt else "")
                with pinned(dp_path=fam.pin, dm_mt=mt):
                    loss, a, b = forward(m, k, o, t, ndir)
                    status_ok(tag)
                got = {"loss": npy(loss), "alpha": npy(a)}
                if b is not None:
                    got["beta"] = npy(b)
                check(tag, cid, variant, got, ref, tuple(got))


# Same family, same bits: a sample inside the skewed batch against the same sample alone (B = 1, the same T and L).  Left out, because the
# arithmetic legitimately depends on the batch there:
#   dense_mfma   the exact-redo budget grows with B and the weak-transition flag is one word per batch: both decide when the launch hands over to
#                the log-space kernels (dag_dp_dense_mfma.hip:956-957, :965-967)
#   wide cases   B decides between the NT = 256 / CPL = 4 kernels and the narrow ones (dag_dp_strip4g.hip:494, :523; dag_dp_maxstrip.hip:558, :584)
SAME = [(c.cid, f) for c in U.CASES if not c.cid.startswith("wide") for f in dict.fromkeys(c.fwd + c.align) if f != "dense_mfma"]


@pytest.mark.parametrize("cid,family", SAME, ids=["-".join(x) for x in SAME])
def test_a_sample_alone_gives_the_same_bits(cid, family):
    case, fam = U.BY_ID[cid], U.FAMILIES[family]
    with pinned(dp_path=fam.pin):
        if family in case.fwd:
            m, k, o, t, _ = dev_inputs(cid, "base", "fwd")
            loss, a, b = forward(m, k, o, t, 2)
            status_ok(f"{cid} {family}")
            for s in range(case.B):
                l1, a1, b1 = forward(m[s:s + 1].contiguous(), k[s:s + 1].contiguous(), o[s:s + 1].contiguous(), t[s:s + 1].contiguous(), 2)
                status_ok(f"{cid} {family} sample {s} alone")
                assert torch.equal(a1[0], a[s]) and torch.equal(b1[0], b[s]) and torch.equal(l1[0], loss[s]), (cid, family, s, U.lengths(case)[s])
        if family in case.align:
            m, k, o, t, _ = dev_inputs(cid, "ties", "fwd")
            path = ops().dag_best_alignment(m, k, o, t)
            status_ok(f"{cid} {family}")
            for s in range(case.B):
                p1 = ops().dag_best_alignment(m[s:s + 1].contiguous(), k[s:s + 1].contiguous(), o[s:s + 1].contiguous(), t[s:s + 1].contiguous())
                assert torch.equal(p1[0], path[s]), (cid, family, s, U.lengths(case)[s])


# ---------------------------------------------------------------------------------------------- backward

def backward(m, k, o, t, w, want=(True, True)):
    m2, k2 = m.clone().requires_grad_(want[0]), k.clone().requires_grad_(want[1])
    poison(m, k)
    loss = ops().dag_loss(m2, k2, o, t)
    leaves = [x for x, on in ((m2, want[0]), (k2, want[1])) if on]
    diag = (ctypes.c_uint * 4)()
    lib().load().dsp_dag_debug_k5(diag)                                                      # (reading resets the record)
    poison(m, k)
    grads = list(torch.autograd.grad((loss.nan_to_num(neginf=0.0) * w).sum(), leaves))       # the unreachable sample gets its w too: the kernels zero it
    torch.cuda.synchronize()
    lib().load().dsp_dag_debug_k5(diag)
    out = {"k5": int(diag[3])}                                                               # the grad_links family that ran (dag_grad.hip:525-526)
    if want[0]:
        out["gm"] = npy(grads.pop(0))
    if want[1]:
        out["gl"] = npy(grads.pop(0))
    return out


BWD = [(c.cid, o) for c in U.CASES if c.bwd for o in U.ORDERS]


@pytest.mark.parametrize("cid,order", BWD, ids=["-".join(x) for x in BWD])
def test_backward_meets_the_oracle(cid, order):
    """k5_path 0 .. 3 (dag_grad.hip:527, :575-627), k5_fuse 1 .. 3 where TR <= 32 (:528, :600-606), both gradients and one"""
    case = U.BY_ID[cid]
    out_tab, out_link, dead_grad = U.outside(case, order)
    runs = [dict(k5_path=p) for p in (0, 1, 2, 3)] + ([dict(k5_fuse=f) for f in (1, 2, 3)] if case.TR <= 32 else [])
    # the grad_links families the pins must reach between them (g_k5_last, dag_grad.hip:595, :606, :619, :626, :635, :641): 1 tiled log space,
    # 2 exp space, 3 dense block products, 4 / 5 the fused launches, 6 the planes of windows 33 .. 128
    if case.TR <= 32:
        reach = {1, 2, 4, 5}
    elif case.TR <= 128:
        reach = {1, 6} | ({3} if case.TR > 64 and case.L % 4 == 0 else set())          # (pitched alpha / beta never take the dense products: :620)
    else:
        reach = {1, 3}
    for variant in case.variants:
        if variant == "ties":
            continue
        m, k, o, t, w = dev_inputs(cid, variant, order)
        ref = U.reference(cid, variant, order)
        seen = set()
        for opts, want in [(r, (True, True)) for r in runs] + [({}, (True, False)), ({}, (False, True))]:
            with pinned(**opts):
                got = backward(m, k, o, t, w, want)
                k5 = got.pop("k5")
                tag = f"{cid}-{order}-{variant} backward {opts or ''}{'' if all(want) else ' only ' + ('gm' if want[0] else 'gl')} (family {k5})"
                status_ok(tag)
            seen.add(k5)
            check(tag, cid, variant, got, ref, tuple(got))
            if "gm" in got:
                assert not got["gm"][out_tab].any() and not got["gm"][dead_grad].any(), tag
            if "gl" in got:
                assert not got["gl"][out_link].any() and not got["gl"][dead_grad].any(), tag
        assert reach <= seen, (cid, order, variant, reach, seen)


# ---------------------------------------------------------------------------------------------- alignment

def abi_align(m, k, o, t, trace):
    """dsp_dag_best_alignment_ws on dense tensors, path and trace poisoned -> (rc, path)"""
    L_ = lib()
    B, T, L = m.shape
    TR = k.shape[2]
    amax = torch.full((B, T, L), float("nan"), dtype=torch.float32, device=dev())
    tr = torch.full((B, T, L), -7, dtype=torch.int32, device=dev()) if trace else None
    path = torch.full((B, L), -7, dtype=torch.long, device=dev())
    ws = torch.empty((max(1, L_.load().dsp_dag_alignment_workspace_bytes(B, T, L, TR)),), dtype=torch.uint8, device=dev())
    rc = L_.load().dsp_dag_best_alignment_ws(L_.ptr(m), L_.ptr(k), L_.ptr(o), L_.ptr(t), L_.ptr(amax), L_.ptr(tr), L_.ptr(path), B, T, L, TR,
                                             L_.ptr(ws), ws.numel(), L_.current_stream_handle())
    torch.cuda.synchronize()
    return rc, path


ALIGN = [(c.cid, o) for c in U.CASES for o in U.ORDERS]
ALIGN_PINS = (0, 7, 9, 4, 2, 1)


@pytest.mark.parametrize("cid,order", ALIGN, ids=["-".join(x) for x in ALIGN])
def test_alignment_is_the_oracles_path(cid, order):
    """every alignment pin, through the operator (pitched rows where the pinned family takes them) and through the C ABI on dense tensors with a
    trace tensor and, where the entry point allows, without one; scores rounded to halves, so that ties are decided by the rule, not by rounding"""
    case = U.BY_ID[cid]
    m, k, o, t, _ = dev_inputs(cid, "ties", order)
    ref = U.reference(cid, "ties", order).path
    pins = {U.FAMILIES[f].pin for f in case.align}
    assert pins <= set(ALIGN_PINS)
    for pin in ALIGN_PINS:
        for mt in ((0, 1, 2) if pin == 9 and "dense_max" in case.align else (0,)):
            with pinned(dp_path=pin, dx_mt=mt):
                poison(m, k)
                got = npy(ops().dag_best_alignment(m, k, o, t))
                status_ok(f"{cid}-{order} alignment pin {pin}")
                np.testing.assert_array_equal(got, ref, err_msg=f"{cid}-{order} pin {pin} dx_mt {mt} (operator)")
                optional = bool(lib().load().dsp_dag_alignment_trace_optional(case.L, case.TR))
                for trace in ((True, False) if optional else (True,)):
                    rc, path = abi_align(m, k, o, t, trace)
                    assert rc == 0, (pin, trace, lib().load().dsp_last_error())
                    status_ok(f"{cid}-{order} alignment pin {pin} trace {trace}")
                    np.testing.assert_array_equal(npy(path), ref, err_msg=f"{cid}-{order} pin {pin} dx_mt {mt} trace {trace} (C ABI)")
    print(f"dag-skew {cid}-{order}-ties alignment: pins {ALIGN_PINS} equal to the oracle's path, with and without a trace tensor")


# ---------------------------------------------------------------------------------------------- the C ABI, outputs poisoned

def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev())


def abi_fwd(m, k, o, t, alpha=True, beta=True):
    L_ = lib()
    B, T, L = m.shape
    TR = k.shape[2]
    a, b, ls = _nan(B, T, L), _nan(B, T, L), _nan(B)
    ws = torch.empty((max(1, L_.load().dsp_dag_workspace_bytes(B, T, L, TR)),), dtype=torch.uint8, device=dev())
    rc = L_.load().dsp_dag_loss_fwd(L_.ptr(m), L_.ptr(k), L_.ptr(o), L_.ptr(t), L_.ptr(a if alpha else None), L_.ptr(b if beta else None), L_.ptr(ls),
                                    B, T, L, TR, L_.ptr(ws), ws.numel(), L_.current_stream_handle())
    torch.cuda.synchronize()
    return rc, a, b, ls


def abi_bwd(w, a, b, m, k, o, t):
    L_ = lib()
    B, T, L = m.shape
    TR = k.shape[2]
    gm, gl = _nan(B, T, L), _nan(B, L, TR)
    rc = L_.load().dsp_dag_loss_bwd(L_.ptr(w), L_.ptr(a), L_.ptr(b), L_.ptr(m), L_.ptr(k), L_.ptr(o), L_.ptr(t), L_.ptr(gm), L_.ptr(gl), B, T, L, TR,
                                    None, 0, L_.current_stream_handle())
    torch.cuda.synchronize()
    return rc, gm, gl


POISONED = [(c, o) for c in ("w32", "dense-200", "wide") for o in U.ORDERS]          # a strip family, a dense family, the wide kernels


@pytest.mark.parametrize("cid,order", POISONED, ids=["-".join(x) for x in POISONED])
def test_abi_writes_every_element(cid, order):
    """alpha, beta, the loss, both gradients and the path are NaN / -7 before the call: dead strips, rows T_b .. T-1, columns L_b .. L-1 and the
    unreachable sample's gradients are all written by the kernels (the operators hand them torch.empty)"""
    case = U.BY_ID[cid]
    assert case.L % 4 == 0                                                       # dense tensors with 16-byte rows: the strip families serve them
    m, k, o, t, w = dev_inputs(cid, "base", order)
    ref = U.reference(cid, "base", order)
    rc, a, b, ls = abi_fwd(m, k, o, t)
    assert rc == 0
    status_ok(cid)
    check(f"{cid}-{order}-base C ABI forward", cid, "base", {"alpha": npy(a), "beta": npy(b), "loss": npy(ls)}, ref, ("alpha", "beta", "loss"))
    rc, a1, b1, l1 = abi_fwd(m, k, o, t, alpha=False)                            # beta only: every strip is a beta strip (dag_strip.h:94)
    assert rc == 0 and bool(torch.isnan(a1).all())
    status_ok(cid)
    check(f"{cid}-{order}-base C ABI beta only", cid, "base", {"beta": npy(b1), "loss": npy(l1)}, ref, ("beta", "loss"))
    rc, a2, b2, l2 = abi_fwd(m, k, o, t, beta=False)                             # alpha only: the loss is picked from alpha
    assert rc == 0 and bool(torch.isnan(b2).all())
    status_ok(cid)
    check(f"{cid}-{order}-base C ABI alpha only", cid, "base", {"alpha": npy(a2)}, ref, ("alpha",))
    want = ref.alpha[np.arange(case.B), U.inputs(cid, "base", order).tgt_len - 1, U.inputs(cid, "base", order).out_len - 1]
    assert U.figure(npy(l2), want, U.table_tol(case.T)) <= 1.0
    rc, gm, gl = abi_bwd(w, a, b, m, k, o, t)
    assert rc == 0
    check(f"{cid}-{order}-base C ABI backward", cid, "base", {"gm": npy(gm), "gl": npy(gl)}, ref, ("gm", "gl"))
    out_tab, out_link, dead_grad = U.outside(case, order)
    gm, gl = npy(gm), npy(gl)
    assert not gm[out_tab].any() and not gm[dead_grad].any() and not gl[out_link].any() and not gl[dead_grad].any()
    mt, kt, _, _, _ = dev_inputs(cid, "ties", order)
    pref = U.reference(cid, "ties", order).path
    for trace in (False, True):
        rc, path = abi_align(mt, kt, o, t, trace)
        assert rc == 0
        status_ok(cid)
        np.testing.assert_array_equal(npy(path), pref)
