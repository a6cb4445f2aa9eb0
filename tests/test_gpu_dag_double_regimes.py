"""The double-precision DAG kernels (csrc/dag_dp_f64.hip) against the float64 oracle at every launch regime: the case table, inputs and references
of tests/util_dag_double_regimes.py (pinned on the CPU by tests/test_dag_double_regimes_ref.py), through the operator names of custom_ops and
through the C ABI with poisoned outputs.

Tolerances: the ones tests/test_dag_double.py holds this path to — tables and loss rtol 1e-12 / atol 1e-11, gradients rtol 1e-9 / atol 1e-12; every
figure printed is the fraction of that tolerance used (`pytest -s`; profiles/dag_double_regimes.txt holds a run).  A tensor beyond its tolerance is
not excused by hand: it may be at most 4 x as far from the oracle as the CPU band DP of custom_ops/dag_double.py is on the same inputs (two float64
evaluations, neither of them the kernels).  No case uses that yardstick: the kernels' largest figure of the recorded run is 4e-4 of the tolerance (the band DP's own: 6e-4)."""
import numpy as np
import pytest
import torch

from tests import util_dag_double_regimes as U

pytestmark = pytest.mark.gpu

EINVAL = -1
NAMES = ("alpha", "beta", "loss", "gm", "gl")
TOL = {"alpha": U.TABLE_TOL, "beta": U.TABLE_TOL, "loss": U.TABLE_TOL, "gm": U.GRAD_TOL, "gl": U.GRAD_TOL}


def dev():
    return torch.device("cuda:0")


def ops():
    from daspeech_amd import custom_ops
    return custom_ops


def lib():
    from daspeech_amd import _lib
    return _lib


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def dev_inputs(cid, variant="base"):
    inp = U.inputs(cid, variant)
    return cu(inp.match), cu(inp.links), cu(inp.out_len), cu(inp.tgt_len), cu(inp.w)


def run_ops(cid, variant="base", want=(True, True), gout=None):
    """dag_loss_with_alpha_beta + backward, dag_loss + backward, dag_best_alignment on float64 CUDA tensors -> dict of CPU numpy arrays."""
    m, k, ol, tl, w = dev_inputs(cid, variant)
    gout = w if gout is None else gout
    out = {}
    for name in ("with_alpha_beta", "dag_loss"):
        m2, k2 = m.clone().requires_grad_(want[0]), k.clone().requires_grad_(want[1])
        if name == "with_alpha_beta":
            loss, (a, b) = ops().dag_loss_with_alpha_beta(m2, k2, ol, tl)
            assert a.dtype == b.dtype == torch.float64
        else:
            loss = ops().dag_loss(m2, k2, ol, tl)
        assert loss.dtype == torch.float64
        leaves = [t for t, on in ((m2, want[0]), (k2, want[1])) if on]
        grads = list(torch.autograd.grad(loss, leaves, gout))
        res = {"loss": loss.detach(), "grad_fn": type(loss.grad_fn).__name__}
        if want[0]:
            res["gm"] = grads.pop(0)
        if want[1]:
            res["gl"] = grads.pop(0)
        if name == "with_alpha_beta":
            res["alpha"], res["beta"] = a, b
            out.update(res)
        else:
            for n in ("loss", "gm", "gl"):                      # the same kernels on the same numbers (torch's own backward promises no such thing)
                assert n not in res or "F64" not in res["grad_fn"] or torch.equal(res[n], out[n]), (cid, variant, n)
    out["path"] = ops().dag_best_alignment(m, k, ol, tl)
    torch.cuda.synchronize()
    return {n: (v.cpu().numpy() if torch.is_tensor(v) else v) for n, v in out.items()}


def check(cid, variant, got, names=NAMES, ref=None, tag="kernels"):
    """Each tensor inside its tolerance (or inside 4 x the band DP's distance from the oracle); -inf exactly where the oracle has it, no NaN; the path."""
    ref = U.reference(cid, variant) if ref is None else ref
    figs = {n: U.figure(got[n], getattr(ref, n), TOL[n]) for n in names}
    print(f"dag64 {cid}-{variant}: {tag} vs oracle, fraction of the tolerance used: " + "  ".join(f"{n} {v:.2e}" for n, v in figs.items()))
    over = [n for n, v in figs.items() if not v <= 1.0]
    if over and all(np.isfinite(figs[n]) for n in over):
        yard = U.distances(cid, variant, grads=not U.BY_ID[cid].heavy)
        print(f"dag64 {cid}-{variant}: band DP vs oracle: " + "  ".join(f"{n} {yard[n]:.2e}" for n in over if n in yard))
        over = [n for n in over if not (n in yard and figs[n] <= 4.0 * yard[n])]
    assert not over, (cid, variant, {n: figs[n] for n in over})
    if "path" in got:
        np.testing.assert_array_equal(got["path"], ref.path)
    return figs


# ---------------------------------------------------------------------------------------------- the operator names

@pytest.mark.parametrize("cid,variant", U.PARAMS, ids=U.PARAM_IDS)
def test_every_regime_meets_the_oracle(cid, variant):
    got = run_ops(cid, variant)
    assert "F64" in got["grad_fn"]
    check(cid, variant, got)


def test_invalid_samples_beside_valid_ones():
    """T_b = 0, T_b = T + 1, L_b = 0, L_b = L + 1: loss -inf, tables -inf, gradients zero (U.reference states that contract), the path what the fp32
    operator gives for the sample; the valid first and last samples meet the oracle."""
    cid = "invalid"
    got = run_ops(cid)
    ref = U.reference(cid)
    check(cid, "base", got)
    bad = ~ref.valid
    assert bad.sum() == 4 and np.isneginf(got["loss"][bad]).all() and not got["gm"][bad].any() and not got["gl"][bad].any()
    m, k, ol, tl, _ = dev_inputs(cid)
    p32 = ops().dag_best_alignment(m.float(), k.float(), ol, tl).cpu().numpy()
    np.testing.assert_array_equal(got["path"][bad], p32[bad])


ONE_GRAD = ["guard-TR33-L41", "stride"]


@pytest.mark.parametrize("cid", ONE_GRAD)
def test_one_gradient_wanted(cid):
    both = run_ops(cid)
    only_m = run_ops(cid, want=(True, False))
    only_k = run_ops(cid, want=(False, True))
    assert "gl" not in only_m and "gm" not in only_k
    assert np.array_equal(only_m["gm"], both["gm"]) and np.array_equal(only_k["gl"], both["gl"])
    for r in (only_m, only_k):
        assert np.array_equal(r["loss"], both["loss"]) and np.array_equal(r["beta"], both["beta"]) and np.array_equal(r["alpha"], both["alpha"])
    check(cid, "base", both)


def test_incoming_gradients_in_float32_and_expanded():
    cid = "guard-TR33-L41"
    case, ref = U.BY_ID[cid], U.reference(cid)
    w = U.inputs(cid).w
    assert np.array_equal(w.astype(np.float32).astype(np.float64), w)            # 0.5, 1.5: float32 holds them
    dense = run_ops(cid)
    f32 = run_ops(cid, gout=cu(w.astype(np.float32)))
    assert np.array_equal(f32["gm"], dense["gm"]) and np.array_equal(f32["gl"], dense["gl"])
    check(cid, "base", f32)
    flat = run_ops(cid, gout=torch.full((case.B,), 0.75, dtype=torch.float64, device=dev()))
    exp = run_ops(cid, gout=torch.full((1,), 0.75, dtype=torch.float64, device=dev()).expand(case.B))
    assert np.array_equal(exp["gm"], flat["gm"]) and np.array_equal(exp["gl"], flat["gl"])
    scale = (0.75 / w)
    np.testing.assert_allclose(exp["gm"], ref.gm * scale[:, None, None], rtol=U.GRAD_TOL[0], atol=U.GRAD_TOL[1])
    np.testing.assert_allclose(exp["gl"], ref.gl * scale[:, None, None], rtol=U.GRAD_TOL[0], atol=U.GRAD_TOL[1])


def test_lds_attribute_small_large_small():
    """set_max_dynamic_lds (csrc/error.hip) only ever raises the attribute: L = 3073, then the cap, then 3073 again in one process, for the loss and
    the alignment; all three meet the oracle and the two L = 3073 results are the same bits."""
    first = run_ops("lds-3073")
    cap = run_ops("cap-10240")
    again = run_ops("lds-3073")
    check("lds-3073", "base", first)
    check("cap-10240", "base", cap)
    check("lds-3073", "base", again)
    for n in NAMES + ("path",):
        assert np.array_equal(first[n], again[n]), n


def test_above_the_cap_takes_the_torch_band_dp():
    cid = "above-cap-10241"
    got = run_ops(cid)
    assert "F64" not in got["grad_fn"]
    got["gl"] = np.nan_to_num(got["gl"], nan=0.0)                  # (autograd through an all -inf row, as in tests/test_dag_double.py)
    check(cid, "base", got, tag="torch band DP on the GPU")


# ---------------------------------------------------------------------------------------------- the C ABI, outputs poisoned

def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float64, device=dev())


def _sizes(cid):
    c = U.BY_ID[cid]
    return c.B, c.T, c.L, c.TR


def abi_fwd(cid, alpha=True, beta=True, loss=True, sizes=None, null_match=False):
    L_ = lib()
    m, k, ol, tl, _ = dev_inputs(cid)
    B, T, L, TR = _sizes(cid)
    a, b, ls = _nan(B, T, L), _nan(B, T, L), _nan(B)
    rc = L_.load().dsp_dag_loss_fwd_f64(None if null_match else L_.ptr(m), L_.ptr(k), L_.ptr(ol), L_.ptr(tl), L_.ptr(a if alpha else None),
                                        L_.ptr(b if beta else None), L_.ptr(ls if loss else None), *(sizes or (B, T, L, TR)), L_.current_stream_handle())
    torch.cuda.synchronize()
    return rc, a, b, ls


def abi_align(cid, sizes=None):
    L_ = lib()
    m, k, ol, tl, _ = dev_inputs(cid)
    B, T, L, TR = _sizes(cid)
    amax = _nan(B, T, L)
    trace = torch.full((B, T, L), -7, dtype=torch.int32, device=dev())
    path = torch.full((B, L), -7, dtype=torch.long, device=dev())
    rc = L_.load().dsp_dag_best_alignment_f64(L_.ptr(m), L_.ptr(k), L_.ptr(ol), L_.ptr(tl), L_.ptr(amax), L_.ptr(trace), L_.ptr(path),
                                              *(sizes or (B, T, L, TR)), L_.current_stream_handle())
    torch.cuda.synchronize()
    return rc, amax, trace, path


def abi_bwd(cid, alpha, beta, gm=True, gl=True, sizes=None):
    L_ = lib()
    m, k, ol, tl, w = dev_inputs(cid)
    B, T, L, TR = _sizes(cid)
    g_m, g_l = _nan(B, T, L), _nan(B, L, TR)
    rc = L_.load().dsp_dag_loss_bwd_f64(L_.ptr(w), L_.ptr(alpha), L_.ptr(beta), L_.ptr(m), L_.ptr(k), L_.ptr(ol), L_.ptr(tl), L_.ptr(g_m if gm else None),
                                        L_.ptr(g_l if gl else None), *(sizes or (B, T, L, TR)), L_.current_stream_handle())
    torch.cuda.synchronize()
    return rc, g_m, g_l


def untouched(*ts):
    return all(bool(torch.isnan(t).all()) if t.is_floating_point() else bool((t == -7).all()) for t in ts)


ABI_CASES = ["abi", "pass-1025"]


@pytest.mark.parametrize("cid", ABI_CASES)
def test_abi_forward_one_table_or_no_loss(cid):
    case, ref, inp = U.BY_ID[cid], U.reference(cid), U.inputs(cid)
    rc, a0, b0, l0 = abi_fwd(cid)
    assert rc == 0
    # every element written (rows t >= T_b and columns j >= L_b included: the oracle holds -inf there), nothing left of the poison
    check(cid, "base", {"alpha": a0.cpu().numpy(), "beta": b0.cpu().numpy(), "loss": l0.cpu().numpy()}, names=("alpha", "beta", "loss"), tag="C ABI")
    if cid == "abi":
        assert any(Tb < case.T for Tb, _ in U.lengths(case)) and any(Lb < case.L for _, Lb in U.lengths(case))
    rc, a1, b1, l1 = abi_fwd(cid, alpha=False)                                    # beta only: do_beta on blockIdx.y == 0
    assert rc == 0 and untouched(a1) and torch.equal(b1, b0) and torch.equal(l1, l0)
    rc, a2, b2, l2 = abi_fwd(cid, beta=False)                                     # alpha only: the loss is picked from alpha
    assert rc == 0 and untouched(b2) and torch.equal(a2, a0)
    want = ref.alpha[np.arange(case.B), inp.tgt_len - 1, inp.out_len - 1]
    assert U.figure(l2.cpu().numpy(), want, U.TABLE_TOL) <= 1.0
    rc, a3, b3, l3 = abi_fwd(cid, loss=False)
    assert rc == 0 and untouched(l3) and torch.equal(a3, a0) and torch.equal(b3, b0)


@pytest.mark.parametrize("cid", ABI_CASES)
def test_abi_alignment_writes_every_element(cid):
    """the max-DP adds and compares only: its table and trace are the oracle's, bit for bit"""
    from oracle import dag_oracle as orc
    inp = U.inputs(cid)
    path64, a64, tr64 = orc.dag_best_alignment(inp.match, inp.links, inp.out_len, inp.tgt_len, np.float64, want_internals=True)
    rc, amax, trace, path = abi_align(cid)
    assert rc == 0
    assert not torch.isnan(amax).any() and not (trace == -7).any() and not (path == -7).any()
    np.testing.assert_array_equal(amax.cpu().numpy(), a64)
    np.testing.assert_array_equal(trace.cpu().numpy(), tr64)
    np.testing.assert_array_equal(path.cpu().numpy(), path64)


@pytest.mark.parametrize("cid", ABI_CASES)
def test_abi_backward_one_gradient_or_none(cid):
    rc, a0, b0, _ = abi_fwd(cid)
    assert rc == 0
    rc, gm0, gl0 = abi_bwd(cid, a0, b0)
    assert rc == 0
    check(cid, "base", {"gm": gm0.cpu().numpy(), "gl": gl0.cpu().numpy()}, names=("gm", "gl"), tag="C ABI")
    rc, gm1, gl1 = abi_bwd(cid, a0, b0, gl=False)
    assert rc == 0 and torch.equal(gm1, gm0) and untouched(gl1)
    rc, gm2, gl2 = abi_bwd(cid, a0, b0, gm=False)
    assert rc == 0 and torch.equal(gl2, gl0) and untouched(gm2)
    rc, gm3, gl3 = abi_bwd(cid, a0, b0, gm=False, gl=False)
    assert rc == 0 and untouched(gm3, gl3)


def test_abi_empty_batch_and_refusals():
    cid = "abi"
    B, T, L, TR = _sizes(cid)
    _, a0, b0, _ = abi_fwd(cid)
    rc, a, b, ls = abi_fwd(cid, sizes=(0, T, L, TR))
    assert rc == 0 and untouched(a, b, ls)
    rc, amax, trace, path = abi_align(cid, sizes=(0, T, L, TR))
    assert rc == 0 and untouched(amax, trace, path)
    rc, gm, gl = abi_bwd(cid, a0, b0, sizes=(0, T, L, TR))
    assert rc == 0 and untouched(gm, gl)
    for sizes in ((B, 0, L, TR), (B, T, 0, TR), (B, T, L, 0), (-1, T, L, TR)):
        rc, a, b, ls = abi_fwd(cid, sizes=sizes)
        assert rc == EINVAL and untouched(a, b, ls), sizes
        rc, amax, trace, path = abi_align(cid, sizes=sizes)
        assert rc == EINVAL and untouched(amax, trace, path), sizes
        rc, gm, gl = abi_bwd(cid, a0, b0, sizes=sizes)
        assert rc == EINVAL and untouched(gm, gl), sizes
    # one vertex past the cap: refused by the size alone, before anything is launched
    for call in (abi_fwd, abi_align):
        rc, *outs = call(cid, sizes=(B, T, U.MAX_L + 1, TR))
        assert rc == EINVAL and untouched(*outs)
        assert "max 10240" in lib().load().dsp_last_error().decode()
    rc, a, b, ls = abi_fwd(cid, null_match=True)
    assert rc == EINVAL and untouched(a, b, ls)
    rc, a, b, ls = abi_fwd(cid, alpha=False, beta=False)
    assert rc == EINVAL and untouched(a, b, ls)
