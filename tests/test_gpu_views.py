"""Every HIP operator on tensors that torch accepts but a fresh allocation never is: a contiguous view off the 16-byte grid, pitched rows, a
column slice of a wider tensor, a transposed copy, a broadcast (tests/util_views.py) — for the arguments and for the gradients that autograd
hands to the backward.  The contract ("Layouts"):

  1. no layout that the equivalent torch expression takes produces an alignment or layout error from the C side: the wrapper serves it,
     copies it to a dense 16-byte-aligned tensor, or answers "not served" and the torch lines run;
  2. the result is the same operation: it meets the float64 reference under the rule of the operator's own GPU test, integer results exactly;
  3. where the wrapper copies, the identical launch runs: the bits of the call on fresh tensors (rows marked `bits`);
  4. what an operator documents as required keeps its Python-side error, with its message.

One row per operator: the smallest inputs that still take the vector paths, the reference and rule of the operator's existing test, the
tensor arguments to vary — each through every layout of util_views.every_variant, one at a time, then all at once.  A row reports every
layout that failed, not the first.  Nothing is skipped at run time: where an operator declines, the assertion is on what the public
function then returns."""
import copy
import ctypes
import functools
import os
import re
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import dag_oracle as orc
from tests import util_block_ref as BR
from tests import util_convmod_ref as CM
from tests import util_glue_grad_ref as GG
from tests import util_glue_ref as G
from tests import util_links_ref as LK
from tests import util_relpos_train_ref as RA
from tests import util_resnorm_ref as RN
from tests import util_views as V
from tests.util_4x_rule import check_4x                     # the 4 x rule of the training operators
from tests.util_inputs import make_dag_inputs

pytestmark = pytest.mark.gpu
NAN = float("nan")
VARIANT_NAMES = ("offset", "pitched", "pitched1", "colslice", "transposed", "expanded")
COVERED = {}                 # public name -> the test that runs it (filled by @covers; read by test_every_public_operator_has_a_row)
_FAULT = []


def covers(*names):
    def deco(fn):
        for n in names:
            COVERED.setdefault(n, fn.__name__)
        return fn
    return deco


@pytest.fixture(autouse=True)
def _nothing_after_a_fault():
    if _FAULT:
        pytest.fail(f"a GPU fault was met in {_FAULT[0]}: nothing more is started on the device from this module")
    yield


def D():
    from daspeech_amd import decode_ops
    return decode_ops


def OPS():
    from daspeech_amd import custom_ops
    return custom_ops


def LIB():
    from daspeech_amd import _lib
    return _lib


def cu(a, dtype=None):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to("cuda")


def f64(t):
    return t.detach().to(torch.float64).cpu().numpy()


def _abi_constant(name):
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "daspeech_dag.h")).read()
    return int(re.search(r"#define\s+%s\s+\(?(-?\d+)\)?" % name, text).group(1))


DSP_EINVAL = _abi_constant("DSP_EINVAL")


def leaf(t):
    """a leaf that requires grad and keeps the layout of t (detach keeps strides and offset)"""
    return t.detach().requires_grad_()


def same_bits(tag, got, want):
    got, want = (x if isinstance(x, (tuple, list)) else (x,) for x in (got, want))
    assert len(got) == len(want), tag
    for i, (g, w) in enumerate(zip(got, want)):
        if g is None or w is None:
            assert g is None and w is None, (tag, i)
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, (tag, i, g.dtype, w.dtype, tuple(g.shape), tuple(w.shape))
        if g.dtype == torch.bool or not g.dtype.is_floating_point:
            same = torch.equal(g, w)
        else:
            iw = {2: torch.int16, 4: torch.int32, 8: torch.int64}[g.element_size()]
            same = torch.equal(g.contiguous().view(iw), w.contiguous().view(iw))
        assert same, f"{tag}: output {i} differs from the call on fresh tensors in {int((g != w).sum())} elements"


def sweep(args, vary, call, judge=None, base=None, extra=(), collect=None):
    """every tensor of `vary` through every layout, one at a time, then all at once; `extra`: further (tag, {name: view}) runs.  Each result goes
    to judge(tag, out) — judge None: it has to have the bits of `base`.  Fails with the list of layouts that did not pass (collect: a list that
    takes them instead).  -> the number of layouts run"""
    per = {n: dict(V.every_variant(args[n])) for n in vary}
    runs = [(f"{n}:{vn}", {n: v}) for n in vary for vn, v in per[n].items()]
    if len(vary) > 1:
        for vn in VARIANT_NAMES:
            if any(vn in per[n] for n in vary):
                runs.append((f"all:{vn}", {n: per[n].get(vn, per[n]["offset"]) for n in vary}))
    runs += list(extra)
    fails = []
    for tag, repl in runs:
        try:
            out = call({**args, **repl})
            torch.cuda.synchronize()
            if judge is None:
                same_bits(tag, out, base)
            else:
                judge(tag, out)
        except (AssertionError, RuntimeError) as e:
            msg = f"{type(e).__name__}: {e}"
            if "illegal memory" in msg or "HIP error" in msg or "hipError" in msg:
                _FAULT.append(tag)
                raise
            fails.append(f"{tag}: {msg[:400]}")
    if collect is not None:
        collect.extend(fails)
        return len(runs)
    assert not fails, f"{len(fails)} of {len(runs)} layouts failed:\n" + "\n".join(fails)
    return len(runs)


def judged(name, got, ref, ref32, cap):
    """the rule of the inference kernels (tests/util_block_ref.judge): as accurate as torch's fp32 result against float64, never beyond cap"""
    err, err32, bound, ok = BR.judge(f64(got), f64(ref), f64(ref32), cap)
    assert not torch.isnan(got).any(), f"{name}: NaN in the result"
    assert ok, f"{name}: err {err:.3e} > bound {bound:.3e} (torch fp32: {err32:.3e})"


def judged_gemm(name, got, ref, ref32):
    """test_split_precision_conv1d_is_fp32_accurate's rule for the split GEMM / convolution: relative to the largest reference magnitude,
    under 4e-6 and under 8 x the error of torch's fp32 result + 1e-6"""
    scale = ref.abs().max().item()
    err = (got.double() - ref).abs().max().item() / scale
    err32 = (ref32.double() - ref).abs().max().item() / scale
    assert got.shape == ref.shape and torch.isfinite(got).all(), name
    assert err < 4e-6 and err < 8 * err32 + 1e-6, f"{name}: err {err:.3e} (torch fp32: {err32:.3e})"


def expanded_gradients(args, keys, call):
    """the gradient a plain .sum() sends back: all ones with stride 0 — the bits of the call on dense ones"""
    ones = {k: torch.ones_like(args[k], memory_format=torch.contiguous_format) for k in keys}
    base = call({**args, **ones})
    for k in keys:
        for d in range(ones[k].dim()):
            if ones[k].shape[d] > 1:
                same_bits(f"{k}:expanded{d}", call({**args, **ones, k: V.expanded(ones[k], d)}), base)
    same_bits("all:expanded", call({**args, **{k: V.expanded(ones[k]) for k in keys}}), base)


# ================================================================================================ DAG ops

DAG_SHAPES = [(2, 10, 128, 32), (3, 12, 130, 7), (2, 20, 300, 299), (2, 9, 96, 95), (1, 30, 1028, 32), (2, 15, 257, 64), (2, 16, 512, 32)]


def _dag_judge(T, ref):
    a64, b64, gm64, gl64, path_ref, fin_ref = ref

    def judge(tag, out):
        loss_ab, alpha, beta, loss, gm, gl, path = out
        a, b = alpha.cpu().numpy(), beta.cpu().numpy()
        assert np.array_equal(np.isneginf(a), np.isneginf(a64)) and np.array_equal(np.isneginf(b), np.isneginf(b64)), f"{tag}: -inf pattern"
        fa, fb = np.isfinite(a64), np.isfinite(b64)
        np.testing.assert_allclose(a[fa], a64[fa], rtol=3e-6, atol=2e-5 * T, err_msg=f"{tag} alpha")          # test_oracle_alpha_beta_loss
        np.testing.assert_allclose(b[fb], b64[fb], rtol=3e-6, atol=2e-5 * T, err_msg=f"{tag} beta")
        for l in (loss_ab, loss):
            l = l.cpu().numpy()
            assert np.array_equal(np.isfinite(l), fin_ref), f"{tag}: finite losses"
            np.testing.assert_allclose(l[fin_ref], b64[:, 0, 0][fin_ref], rtol=3e-6, atol=2e-5 * T, err_msg=f"{tag} loss")
        scale = 2e-5 * T                                                                                      # test_oracle_gradients
        np.testing.assert_allclose(gm.cpu().numpy(), gm64, rtol=50 * scale, atol=1e-7, err_msg=f"{tag} grad_match")
        np.testing.assert_allclose(gl.cpu().numpy(), gl64, rtol=50 * scale, atol=1e-7, err_msg=f"{tag} grad_links")
        np.testing.assert_array_equal(path.cpu().numpy(), path_ref, err_msg=f"{tag} path")                    # test_oracle_viterbi_bit_exact
    return judge


@covers("dag_loss", "dag_loss_with_alpha_beta", "dag_best_alignment")
@pytest.mark.parametrize("case", range(len(DAG_SHAPES)), ids=["x".join(map(str, s)) for s in DAG_SHAPES])
def test_dag_ops(case):
    """the cases of the former tools/fuzz_views.py, judged against oracle.dag_oracle as tests/test_gpu_dag_ops.py judges: alpha, beta, both
    losses, both gradients, and the alignment on quantised scores (exact ties).  links also 8 and 12 bytes off the grid: the peeled head and
    tail of the weak-transition scan, the scalar transition loads of the max strips, the lazy back-trace at TR = 32."""
    B, T, L, TR = DAG_SHAPES[case]
    match, links, ol, tl = make_dag_inputs(5 + case, B, T, L, TR)
    qm = (np.round(match * 2) / 2).astype(np.float32)
    ql = np.where(np.isfinite(links), np.round(links * 2) / 2, links).astype(np.float32)
    a64, b64 = orc.dag_alpha(match, links, ol, tl, np.float64), orc.dag_beta(match, links, ol, tl, np.float64)
    fin_ref = np.isfinite(b64[:, 0, 0])
    w = np.linspace(0.5, 1.5, B)
    gm64, gl64 = orc.dag_grad((w * fin_ref).astype(np.float64), a64, b64, match, links, ol, tl, np.float64)
    path_ref = orc.dag_best_alignment(qm, ql, ol, tl, np.float32)
    args = dict(match=cu(match), links=cu(links), qmatch=cu(qm), qlinks=cu(ql), ol=cu(ol), tl=cu(tl), gout=cu(w * fin_ref, torch.float32))

    def call(a):
        ops = OPS()
        m = leaf(a["match"])
        loss_ab, (alpha, beta) = ops.dag_loss_with_alpha_beta(m, a["links"], a["ol"], a["tl"])
        assert LIB().last_launch_status() == 0
        m2, k2 = leaf(a["match"]), leaf(a["links"])
        loss = ops.dag_loss(m2, k2, a["ol"], a["tl"])
        gm, gl = torch.autograd.grad(loss, [m2, k2], a["gout"])               # the gradient of the losses arrives in the layout of gout
        path = ops.dag_best_alignment(a["qmatch"], a["qlinks"], a["ol"], a["tl"])
        return loss_ab.detach(), alpha, beta, loss.detach(), gm, gl, path
    judge = _dag_judge(T, (a64, b64, gm64, gl64, path_ref, fin_ref))
    judge("fresh", call(args))
    extra = [(f"links+qlinks:offset{k}", {"links": V.at_offset(args["links"], k), "qlinks": V.at_offset(args["qlinks"], k)}) for k in (2, 3)]
    extra += [(f"match+qmatch:offset{k}", {"match": V.at_offset(args["match"], k), "qmatch": V.at_offset(args["qmatch"], k)}) for k in (2, 3)]
    sweep(args, ("match", "links", "qmatch", "qlinks", "ol", "tl", "gout"), call, judge, extra=extra)
    # the stride-0 gradient of a plain .sum(): all ones; a sample without a path has a -inf loss and no gradient, as under nan_to_num().sum()
    gm1, gl1 = orc.dag_grad(fin_ref.astype(np.float64), a64, b64, match, links, ol, tl, np.float64)
    ones = torch.ones(B, device="cuda")
    judge1 = _dag_judge(T, (a64, b64, gm1, gl1, path_ref, fin_ref))
    judge1("gout:ones", call({**args, "gout": ones}))
    if B > 1:
        judge1("gout:expanded", call({**args, "gout": V.expanded(ones)}))
    m2, k2 = leaf(args["match"]), leaf(args["links"])
    gm, gl = torch.autograd.grad(OPS().dag_loss(m2, k2, args["ol"], args["tl"]).nan_to_num(neginf=0.0).sum(), [m2, k2])
    np.testing.assert_allclose(gm.cpu().numpy(), gm1, rtol=50 * 2e-5 * T, atol=1e-7)
    np.testing.assert_allclose(gl.cpu().numpy(), gl1, rtol=50 * 2e-5 * T, atol=1e-7)


@covers("dag_loss", "dag_loss_with_alpha_beta", "dag_best_alignment")
@pytest.mark.parametrize("shape", [(2, 10, 128, 32), (2, 9, 96, 95)], ids=lambda s_: "x".join(map(str, s_)))
def test_dag_ops_float64(shape):
    """float64 tensors go to the double kernels behind custom_ops/dag_double.py, which copy every argument and the incoming gradient to dense
    tensors: every layout gives the bits of the call on fresh tensors, which meets the oracle by tests/test_dag_double.py's tolerances"""
    B, T, L, TR = shape
    match, links, ol, tl = make_dag_inputs(23 + L, B, T, L, TR)
    match, links = match.astype(np.float64), links.astype(np.float64)
    a64, b64 = orc.dag_alpha(match, links, ol, tl, np.float64), orc.dag_beta(match, links, ol, tl, np.float64)
    fin_ref = np.isfinite(b64[:, 0, 0])
    assert fin_ref.all()
    w = np.linspace(0.5, 1.5, B)
    gm64, gl64 = orc.dag_grad(w, a64, b64, match, links, ol, tl, np.float64)
    qm = np.round(match * 2) / 2
    ql = np.where(np.isfinite(links), np.round(links * 2) / 2, links)
    path_ref = orc.dag_best_alignment(qm, ql, ol, tl, np.float64)
    args = dict(match=cu(match), links=cu(links), qmatch=cu(qm), qlinks=cu(ql), ol=cu(ol), tl=cu(tl), gout=cu(w))

    def call(a):
        ops = OPS()
        m2, k2 = leaf(a["match"]), leaf(a["links"])
        loss, (alpha, beta) = ops.dag_loss_with_alpha_beta(m2, k2, a["ol"], a["tl"])
        gm, gl = torch.autograd.grad(loss, [m2, k2], a["gout"])
        m3, k3 = leaf(a["match"]), leaf(a["links"])
        g3 = torch.autograd.grad(ops.dag_loss(m3, k3, a["ol"], a["tl"]), [m3, k3], a["gout"])
        return loss.detach(), alpha, beta, gm, torch.nan_to_num(gl, nan=0.0), g3[0], torch.nan_to_num(g3[1], nan=0.0), ops.dag_best_alignment(a["qmatch"], a["qlinks"], a["ol"], a["tl"])
    base = call(args)
    loss, alpha, beta, gm, gl, gm3, gl3, path = base
    assert loss.dtype == torch.float64 and gm.dtype == torch.float64 and gl.dtype == torch.float64
    a, b = alpha.cpu().numpy(), beta.cpu().numpy()
    assert np.array_equal(np.isneginf(a), np.isneginf(a64)) and np.array_equal(np.isneginf(b), np.isneginf(b64))
    fa, fb = np.isfinite(a64), np.isfinite(b64)
    np.testing.assert_allclose(a[fa], a64[fa], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(b[fb], b64[fb], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(loss.cpu().numpy(), b64[:, 0, 0], rtol=1e-12, atol=1e-11)
    for g, r in ((gm, gm64), (gm3, gm64), (gl, gl64), (gl3, gl64)):
        np.testing.assert_allclose(g.cpu().numpy(), r, rtol=1e-9, atol=1e-12)
    np.testing.assert_array_equal(path.cpu().numpy(), path_ref)
    sweep(args, tuple(args), call, base=base)
    expanded_gradients(args, ("gout",), call)


BWD_CASES = [(2, 10, 128, 32), (2, 12, 256, 64)]          # (T = 12: the plane form is the cheaper estimate on the grid)


@covers("dag_loss")
@pytest.mark.parametrize("which", ["alpha", "beta", "g_links"])
@pytest.mark.parametrize("shape", BWD_CASES, ids=lambda s_: "x".join(map(str, s_)))
def test_backward_with_a_table_or_the_link_gradient_off_the_grid(shape, which):
    """dsp_dag_loss_bwd chooses its kernels by the alignment of alpha, beta and grad_links (rows16 in launch_dag_bwd_generic): on the grid the
    exp-space kernels (one launch for both gradients at TR <= 32, planes of 32 transitions for windows 33 .. 128), off it the element-wise
    grad_match kernel and the tiled log-space grad_links kernel.  The operators allocate all three fresh, so the second branch is reached
    through the C ABI only: each of the three 4 bytes off the grid in turn, outputs pre-filled with NaN, against orc.dag_grad under
    test_oracle_gradients' rule, like the aligned call.  The header documents no gate for them."""
    lib, L_ = LIB(), LIB().load()
    B, T, L, TR = shape
    match, links, ol, tl = make_dag_inputs(31 + L, B, T, L, TR)
    a64, b64 = orc.dag_alpha(match, links, ol, tl, np.float64), orc.dag_beta(match, links, ol, tl, np.float64)
    fin_ref = np.isfinite(b64[:, 0, 0])
    assert fin_ref.all()
    w = np.linspace(0.5, 1.5, B)
    gm64, gl64 = orc.dag_grad(w, a64, b64, match, links, ol, tl, np.float64)
    m, k, o, t, go = cu(match), cu(links), cu(ol), cu(tl), cu(w, torch.float32)
    with torch.no_grad():
        _, (alpha, beta) = OPS().dag_loss_with_alpha_beta(leaf(m), k, o, t)
    alpha, beta = alpha.contiguous(), beta.contiguous()
    assert alpha.data_ptr() % 16 == 0 and beta.data_ptr() % 16 == 0
    diag = (ctypes.c_uint * 4)()
    kinds = {}
    for off in (None, which):
        a_, b_ = (V.at_offset(alpha) if off == "alpha" else alpha), (V.at_offset(beta) if off == "beta" else beta)
        gm = torch.full((B, T, L), NAN, device="cuda")
        gl = torch.full((B, L, TR), NAN, device="cuda")
        gl = V.at_offset(gl) if off == "g_links" else gl
        L_.dsp_dag_debug_k5(diag)
        lib.check(L_.dsp_dag_loss_bwd(lib.ptr(go), lib.ptr(a_), lib.ptr(b_), lib.ptr(m), lib.ptr(k), lib.ptr(o), lib.ptr(t), lib.ptr(gm), lib.ptr(gl),
                                      B, T, L, TR, None, 0, lib.current_stream_handle()), "dsp_dag_loss_bwd")
        torch.cuda.synchronize()
        L_.dsp_dag_debug_k5(diag)
        kinds[off] = int(diag[3])
        assert not torch.isnan(gm).any() and not torch.isnan(gl).any(), f"{off}: an element of a gradient was never written"
        scale = 2e-5 * T
        np.testing.assert_allclose(gm.cpu().numpy(), gm64, rtol=50 * scale, atol=1e-7, err_msg=f"grad_match, {off} off the grid")
        np.testing.assert_allclose(gl.cpu().numpy(), gl64, rtol=50 * scale, atol=1e-7, err_msg=f"grad_links, {off} off the grid")
    assert kinds[None] in (5, 6) and kinds[which] == 1, kinds          # k5_last: fused / planes on the grid, the tiled kernel off it


@covers("dag_best_alignment")
@pytest.mark.parametrize("k", [1, 2, 3])
def test_alignment_without_a_trace_and_links_off_the_grid_takes_the_lazy_back_trace(k):
    """dsp_dag_best_alignment_ws at TR = 32 without a trace buffer runs the ring back-trace when `links` is on the 16-byte grid and the lazy one
    (scalar transition loads in the strips too) when it is not.  The Python operator hands over a trace buffer for such links, so the branch
    is reached through the C ABI only: the same path as the oracle's on quantised scores, every element of `path` written."""
    lib, L_ = LIB(), LIB().load()
    B, T, L, TR = 2, 16, 512, 32
    match, links, ol, tl = make_dag_inputs(19, B, T, L, TR)
    qm = (np.round(match * 2) / 2).astype(np.float32)
    ql = np.where(np.isfinite(links), np.round(links * 2) / 2, links).astype(np.float32)
    ref = orc.dag_best_alignment(qm, ql, ol, tl, np.float32)
    m, o, t = cu(qm), cu(ol), cu(tl)
    assert L_.dsp_dag_alignment_trace_optional(L, TR)
    nbytes = int(L_.dsp_dag_alignment_workspace_bytes(B, T, L, TR))
    got = []
    for kv in (cu(ql), V.at_offset(cu(ql), k)):
        alpha = torch.full((B, T, L), NAN, device="cuda")
        path = torch.full((B, L), -7, dtype=torch.long, device="cuda")
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")
        lib.check(L_.dsp_dag_best_alignment_ws(lib.ptr(m), lib.ptr(kv), lib.ptr(o), lib.ptr(t), lib.ptr(alpha), None, lib.ptr(path), B, T, L, TR,
                                               lib.ptr(ws), nbytes, lib.current_stream_handle()), "dsp_dag_best_alignment_ws")
        torch.cuda.synchronize()
        assert not (path == -7).any()
        np.testing.assert_array_equal(path.cpu().numpy(), ref)
        got.append(path)
    assert got[1].data_ptr() != got[0].data_ptr() and torch.equal(got[0], got[1])


@covers("dag_loss_with_alpha_beta")
@pytest.mark.parametrize("where", ["head", "tail"])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_weak_transition_scan_sees_its_peeled_head_and_tail(k, where):
    """dag_links_weak_kernel reads the transitions in 16-byte vectors between a scalar head and a scalar tail.  A dense-window batch whose ONLY
    transition under e^-86 is the first element (in the head of links 4, 8 or 12 bytes off the grid) or the last one (in the tail; that cell
    belongs to a vertex without successors, so the DP never reads it): the scan has to flag it and the stand-by log-space kernels give the
    result.  The same batch without the planted value stays on the matrix cores.
    "The stand-by fired" is last_dense_gave_up(): last_fallback_count() counts the cells the matrix-core DP redoes exactly, and a batch the scan
    refuses never starts that DP — measured 0 cells with gave_up True in all six planted cases, 0 cells and gave_up False in the six benign ones
    (the "weak" case of test_dense_dp_hands_unrepresentable_batches_to_the_log_space_kernels asserts the same flag)."""
    lib = LIB()
    B, T, L, TR = 2, 10, 160, 159                         # a window beyond 128: the strip families decline, the matrix-core DP takes it
    match, links, ol, tl = make_dag_inputs(41, B, T, L, TR, ragged=False)
    planted = links.copy()
    if where == "head":
        planted[0, 0, 0] = -100.0
        seen = planted
    else:
        assert np.isneginf(planted[B - 1, L - 1, TR - 1])
        planted[B - 1, L - 1, TR - 1] = -100.0
        seen = links                                         # no path uses the cell: the oracle sees the batch without it
    a64, b64 = orc.dag_alpha(match, seen, ol, tl, np.float64), orc.dag_beta(match, seen, ol, tl, np.float64)
    m, o, t = cu(match), cu(ol), cu(tl)
    for name, kk, expect in (("benign", links, False), ("planted", planted, True)):
        kv = V.at_offset(cu(kk), k)
        assert kv.data_ptr() % 16 == 4 * k
        alpha, beta = (torch.full((B, T, L), NAN, device="cuda") for _ in range(2))           # dsp_dag_loss_fwd itself, on poisoned outputs
        loss = torch.full((B,), NAN, device="cuda")
        nbytes = int(lib.load().dsp_dag_workspace_bytes(B, T, L, TR))
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")
        lib.check(lib.load().dsp_dag_loss_fwd(lib.ptr(m), lib.ptr(kv), lib.ptr(o), lib.ptr(t), lib.ptr(alpha), lib.ptr(beta), lib.ptr(loss), B, T, L, TR,
                                              lib.ptr(ws), nbytes, lib.current_stream_handle()), "dsp_dag_loss_fwd")
        assert lib.last_launch_status() == 0
        assert not torch.isnan(alpha).any() and not torch.isnan(beta).any() and not torch.isnan(loss).any(), "an output element was never written"
        gave_up, cells = lib.last_dense_gave_up(), lib.last_fallback_count()
        print(f"weak scan {where} offset {4 * k} bytes {name}: gave_up {gave_up} fallback cells {cells}")
        assert gave_up == expect, (name, gave_up, cells)
        ref_a, ref_b = (a64, b64) if name == "planted" else (orc.dag_alpha(match, links, ol, tl, np.float64), orc.dag_beta(match, links, ol, tl, np.float64))
        a, b = alpha.cpu().numpy(), beta.cpu().numpy()
        assert np.array_equal(np.isneginf(a), np.isneginf(ref_a)) and np.array_equal(np.isneginf(b), np.isneginf(ref_b))
        fa, fb = np.isfinite(ref_a), np.isfinite(ref_b)
        np.testing.assert_allclose(a[fa], ref_a[fa], rtol=3e-6, atol=2e-5 * T + 1e-4)        # (the stand-by rule of test_dense_dp_hands_unrepresentable_...)
        np.testing.assert_allclose(b[fb], ref_b[fb], rtol=3e-6, atol=2e-5 * T + 1e-4)
        np.testing.assert_allclose(loss.detach().cpu().numpy(), ref_b[:, 0, 0], rtol=3e-6, atol=2e-5 * T + 1e-4)


LSG_EPS = {torch.float32: 1e-6, torch.float16: 1e-3, torch.bfloat16: 8e-3}


@covers("dag_logsoftmax_gather_inplace")
@pytest.mark.parametrize("V_", [37, 264])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16, torch.float64], ids=["f32", "f16", "bf16", "f64"])
def test_dag_logsoftmax_gather_inplace(dtype, V_):
    """the index in every layout (materialised it is constant along the vertices, so `expanded` is the criterion's own expand), the in-place
    buffer at an odd offset (contiguous: served) and the gradient of the match in every layout; a non-contiguous in-place buffer keeps its
    error.  Rules: test_oracle_logsoftmax_gather, and test_gpu_lsg_double.py for float64."""
    B, L, S = 2, 21, 7
    rng = np.random.default_rng(V_)
    logits = torch.from_numpy(rng.standard_normal((B, L, V_)) * 3).to(dtype)
    tgt = rng.integers(0, V_, (B, S))
    idx = np.ascontiguousarray(np.broadcast_to(tgt[:, None, :], (B, L, S)))
    ref, sm = orc.logsoftmax_gather(logits.double().numpy(), idx, np.float64, want_softmax=True)
    w = rng.standard_normal((B, L, S)).astype(np.float32)
    dbl = dtype == torch.float64
    args = dict(logits=cu(logits), idx=cu(idx), go=cu(w, torch.float64 if dbl else torch.float32))

    def call(a):
        x = cu(logits).requires_grad_()
        res = a["logits"].data_ptr() % 16
        if res == 0:
            work = x.clone()
        else:                                            # a non-leaf at the offset of a["logits"] that autograd does not know as a view (an in-place
            es = x.element_size()                        # Function with two outputs is refused on views): set_ on a buffer's storage, then copy_
            buf = torch.empty(x.numel() + 16 // es + res // es, dtype=x.dtype, device=x.device)
            assert buf.data_ptr() % 16 == 0
            work = torch.empty(0, dtype=x.dtype, device=x.device).set_(buf.untyped_storage(), res // es, x.shape, x.stride())
            work.copy_(x)
        assert work.data_ptr() % 16 == res and work.is_contiguous() and not work._is_view() and work.requires_grad
        out_x, match = OPS().dag_logsoftmax_gather_inplace(work, a["idx"])
        assert out_x.data_ptr() == work.data_ptr()
        m, smx = match.detach().clone(), out_x.detach().clone()
        (gx,) = torch.autograd.grad([match], [x], grad_outputs=[a["go"]])
        return m, smx, gx

    def judge(tag, out):
        m, smx, gx = out
        assert m.dtype == (torch.float64 if dbl else torch.float32) and gx.dtype == dtype
        gref = orc.logsoftmax_gather_bwd(f64(smx) if not dbl else sm, idx, f64(args["go"]), np.float64)
        if dbl:
            np.testing.assert_allclose(f64(m), ref, rtol=1e-12, atol=1e-12, err_msg=f"{tag} match")
            np.testing.assert_allclose(f64(smx), sm, rtol=0, atol=1e-12, err_msg=f"{tag} softmax")
            np.testing.assert_allclose(f64(gx), gref, rtol=1e-9, atol=1e-12, err_msg=f"{tag} gradient")
        else:
            eps = LSG_EPS[dtype]
            np.testing.assert_allclose(f64(m), ref, rtol=2e-6, atol=2e-6, err_msg=f"{tag} match")
            np.testing.assert_allclose(f64(smx), sm, rtol=eps, atol=eps * 0.1, err_msg=f"{tag} softmax")
            np.testing.assert_allclose(f64(gx), gref, rtol=4 * eps, atol=4 * eps, err_msg=f"{tag} gradient")
    judge("fresh", call(args))
    off = {"logits": V.at_offset(args["logits"])}
    sweep(args, ("idx", "go"), call, judge, extra=[("logits:offset", off), ("all+logits:offset", {**off, "idx": V.expanded(args["idx"]), "go": V.at_offset(args["go"])})])
    expanded_gradients(args, ("go",), lambda a: tuple(t for t in call(a)))
    for name, bad in V.every_variant(args["logits"]):            # contract 4: the in-place buffer has to be contiguous
        if not bad.is_contiguous():
            with pytest.raises(RuntimeError, match="word_ins_out must be contiguous"):
                OPS().dag_logsoftmax_gather_inplace(bad, args["idx"])


# ================================================================================================ links, posterior, glue, decode

LINK_CASES = [(2, 64, 64, 7, (64, 41)), (2, 64, 64, 63, (64, 41)), (2, 150, 64, 7, (150, 97)), (2, 150, 64, 149, (150, 97))]       # H * CK = 512


@covers("extract_links", "extract_links_autograd")
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", LINK_CASES, ids=lambda c: "L%d-TR%d" % (c[1], c[3]))
def test_extract_links(case, dtype):
    """q, k, the gates, the lengths, the distance bias and the gradient of the links in every layout.  Every one of them is copied where the
    kernels cannot take it (bits), the call on fresh tensors meets the float64 band formulation: tests/test_gpu_links_double.py's tolerances
    for float64, test_fused_extract_links_backward_direct_q_k_gates' for fp32."""
    c, ref = LK.reference(case, True)
    TR = c["TR"]
    neg = torch.isneginf(ref["links"])
    wm = c["w"].masked_fill(neg, 0.0)                        # masked_loss's gradient of the links: w, nothing at the -inf entries
    args = dict(q=cu(c["q"], dtype), k=cu(c["k"], dtype), lg=cu(c["lg"], dtype), olen=cu(c["olen"]), bias=cu(c["bias"], dtype), w=cu(wm, dtype))

    def call(a):
        q, k, lg = leaf(a["q"]), leaf(a["k"]), leaf(a["lg"])
        links = D().extract_links_autograd(q, k, lg, a["olen"], TR, a["bias"])
        dq, dk, dg = torch.autograd.grad(links, [q, k, lg], a["w"])          # the gradient of the links arrives in the layout of w
        with torch.no_grad():
            inf = D().extract_links(a["q"], a["k"], a["lg"], a["olen"], TR, a["bias"])
        return links.detach(), dq, dk, dg, inf
    base = call(args)
    links, dq, dk, dg, inf = base
    assert links.dtype == dtype and torch.equal(torch.isneginf(links).cpu(), neg) and not torch.isnan(links).any()
    assert torch.equal(torch.isneginf(inf).cpu(), neg)
    if dtype == torch.float64:
        assert torch.equal(inf, links)
        torch.testing.assert_close(links.cpu()[~neg], ref["links"][~neg], rtol=1e-12, atol=1e-12)
        for n, g in (("dq", dq), ("dk", dk), ("dg", dg)):
            torch.testing.assert_close(g.cpu(), ref[n], rtol=1e-9, atol=1e-12, msg=lambda m: f"{n}: {m}")
    else:
        for l in (links, inf):
            torch.testing.assert_close(l.cpu().double()[~neg], ref["links"][~neg], rtol=1e-5, atol=2e-5)
        for n, g in (("dq", dq), ("dk", dk), ("dg", dg)):
            err = float((g.cpu().double() - ref[n]).abs().max())
            assert err <= 1e-5 * max(1.0, float(ref[n].abs().max())), (n, err)
    sweep(args, ("q", "k", "lg", "olen", "bias", "w"), call, base=base)
    expanded_gradients(args, ("w",), call)


@functools.lru_cache(maxsize=None)
def _posterior_case():
    B, T, L, TR, Dm = 3, 9, 70, 16, 32
    match, links, ol, tl = make_dag_inputs(17, B, T, L, TR)
    a = orc.dag_alpha(match, links, ol, tl, np.float64)
    b = orc.dag_beta(match, links, ol, tl, np.float64)
    rng = np.random.default_rng(0)
    feats = rng.standard_normal((B, L, Dm))
    go = rng.standard_normal((B, T, Dm))
    return a, b, feats, go, tl


def _posterior_ref(a, b, feats, go):
    """float64: score, score @ features and the gradient of the features (alpha / beta as given: fp32 values for the fp32 kernels)"""
    ta, tb = torch.from_numpy(a), torch.from_numpy(b)
    s = ta + tb
    score = torch.exp(s - torch.logsumexp(s, -1, keepdim=True)).nan_to_num(nan=0.0)
    f = torch.from_numpy(feats).requires_grad_()
    out = score @ f
    (df,) = torch.autograd.grad(out, f, torch.from_numpy(go))
    return score.numpy(), out.detach().numpy(), df.numpy()


@covers("posterior", "posterior_features", "expect_features")
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_posterior_ops(dtype):
    """alpha, beta, the features and the incoming gradient in every layout: all are copied (bits); the call on fresh tensors by the rules of
    test_posterior_and_expect / test_posterior_features_fused_forward_and_backward (fp32) and tests/test_gpu_posterior_double.py (1e-12)"""
    a, b, feats, go, tl = _posterior_case()
    a, b = (x.astype(np.float32).astype(np.float64) for x in (a, b)) if dtype == torch.float32 else (a, b)
    feats, go = (x.astype(np.float32).astype(np.float64) for x in (feats, go)) if dtype == torch.float32 else (feats, go)
    score_ref, out_ref, df_ref = _posterior_ref(a, b, feats, go)
    args = dict(alpha=cu(a, dtype), beta=cu(b, dtype), feats=cu(feats, dtype), go=cu(go, dtype))

    def call(x):
        f = leaf(x["feats"])
        out = D().posterior_features(x["alpha"], x["beta"], f)
        (df,) = torch.autograd.grad(out, f, x["go"])
        with torch.no_grad():
            return D().posterior(x["alpha"], x["beta"]), out.detach(), df, D().expect_features(x["alpha"], x["beta"], x["feats"])
    base = call(args)
    score, out, df, ex = base
    assert score.dtype == dtype and out.dtype == dtype and df.dtype == dtype
    tol = dict(rtol=1e-12, atol=1e-12) if dtype == torch.float64 else dict(rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(f64(score), score_ref, rtol=tol["rtol"], atol=1e-12 if dtype == torch.float64 else 1e-6)
    np.testing.assert_allclose(f64(out), out_ref, **tol)
    np.testing.assert_allclose(f64(df), df_ref, rtol=1e-9 if dtype == torch.float64 else 1e-4, atol=tol["atol"])
    assert torch.equal(ex, out[:, 1:])
    for bb in range(score.shape[0]):
        assert not score[bb, tl[bb]:].any() and not out[bb, tl[bb]:].any()
    sweep(args, ("alpha", "beta", "feats", "go"), call, base=base)
    expanded_gradients(args, ("go",), call)


@covers("argmax_logp", "lookahead_next", "graph_decode", "viterbi_decode")
def test_decode_ops():
    """logits, links, features, lengths in every layout: tokens, successors and kept rows exactly the oracle's (tests/test_gpu_decode_ops.py),
    scores within its 2e-6; viterbi_decode exactly its torch restatement; every layout the bits of the call on fresh tensors"""
    B, L, TR, Vn, Dm, pad = 4, 48, 6, 30, 16, 1
    rng = np.random.default_rng(3)
    _, links, ol, _ = make_dag_inputs(3, B, 4, L, TR)
    links = np.where(np.isfinite(links), np.round(links * 4) / 4, links).astype(np.float32)             # ties
    logits = (rng.standard_normal((B, L, Vn)) * 2).astype(np.float32)
    logits[:, ::5, pad] += 20.0
    logits[:, 1::7, 7] += 20.0; logits[:, 2::7, 7] += 20.0
    logits[0, 0, 5] = logits[0, 0, 9] = logits[0, 0].max() + 1                                           # an exact tie: the first index wins
    feats = rng.standard_normal((B, L, Dm)).astype(np.float32)
    sc_q = (np.round(-rng.random((B, L)) * 12) / 4).astype(np.float32)
    tok_ref, sc_ref = orc.argmax_logp(logits)
    args = dict(logits=cu(logits), links=cu(links), feats=cu(feats), ol=cu(ol), sc=cu(sc_q))

    def call(a):
        d = D()
        tok, sc = d.argmax_logp(a["logits"])
        nxt = d.lookahead_next(a["links"], a["sc"], 0.75, False)
        nxt_g = d.lookahead_next(a["links"], None, 1.0, True)
        gd = d.graph_decode(a["logits"], a["links"], a["feats"], a["ol"], pad, 1.0)
        vd = d.viterbi_decode(a["logits"], a["links"], a["feats"], a["ol"], pad, 1.0, 1.0, True)
        return (tok, sc, nxt, nxt_g) + tuple(gd) + tuple(vd)
    base = call(args)
    tok, sc, nxt, nxt_g = base[:4]
    np.testing.assert_array_equal(tok.cpu().numpy(), tok_ref)
    np.testing.assert_allclose(sc.cpu().numpy(), sc_ref, rtol=2e-6, atol=2e-6)
    np.testing.assert_array_equal(nxt.cpu().numpy(), orc.lookahead_next(links, sc_q, beta=0.75, greedy=False))
    np.testing.assert_array_equal(nxt_g.cpu().numpy(), orc.lookahead_next(links, sc_q, beta=1.0, greedy=True))
    out_tok, out_feat, mask, lens = base[4:8]
    toks_ref, keep_ref, nf_ref = orc.follow_path(orc.lookahead_next(links, sc_ref, 1.0), tok_ref, ol, pad)
    np.testing.assert_array_equal(lens.cpu().numpy(), nf_ref)
    for b in range(B):
        n = int(nf_ref[b])
        np.testing.assert_array_equal(out_feat[b, :n].cpu().numpy(), feats[b, keep_ref[b, :n]])
        assert not out_feat[b, n:].any() and mask[b].tolist() == [False] * n + [True] * (out_feat.shape[1] - n)
        got = out_tok[b].cpu().numpy()
        np.testing.assert_array_equal(got[: n + 1], toks_ref[b, : n + 1])
        assert np.all(got[n + 1:] == pad)
    want = D().viterbi_decode_torch(args["logits"], args["links"], args["feats"], args["ol"], pad, 1.0, 1.0, True)
    for g, w_ in zip(base[8:], want):
        assert torch.equal(g, w_)
    sweep(args, ("logits", "links", "feats", "ol", "sc"), call, base=base)


@covers("predicted_durations", "bucketize_embed_add", "bucketize_embed_add_autograd", "length_regulate", "length_regulate_autograd")
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
def test_variance_adaptor_glue(dtype):
    """rows of 16-byte multiples (C = 24) behind an off-grid base pointer (the scalar branches of decode_tts.hip and tts_glue_grad.hip), pitched
    and sliced rows, transposed and broadcast gradients.  Forward results are copies and one add: exactly the reference's; the two gradient sums
    within the derived bound of tests/test_gpu_glue_autograd.py in every layout."""
    d = D()
    n, C, nb, Bq, N = 300, 24, 9, 3, 7
    x, v, bins, emb = G.bucketize_inputs(65, n, C, nb)
    rng = np.random.default_rng(97)
    xr = rng.standard_normal((Bq, N, C)).astype(np.float32)
    dur = rng.poisson(3.0, (Bq, N)).astype(np.int64)
    dur[:, ::4] = 0
    maxlen = int(dur.sum(1).max())
    ld = (rng.standard_normal((4, 37)) * 1.2 + 1.0).astype(np.float32)
    pm = rng.random((4, 37)) < 0.2
    args = dict(x=cu(x, dtype).view(3, 100, C), v=cu(v).view(3, 100), bins=cu(bins), emb=cu(emb, dtype), go=cu(rng.standard_normal((3, 100, C)).astype(np.float32), dtype),
                xr=cu(xr, dtype), dur=cu(dur), gr=cu(rng.standard_normal((Bq, maxlen, C)).astype(np.float32), dtype), ld=cu(ld), pm=cu(pm))
    idx = G.bucketize_ref(v, bins)
    xs, es = f64(args["x"]).reshape(n, C), f64(args["emb"])
    fwd_ref = (torch.from_numpy(xs).to(dtype) + torch.from_numpy(es).to(dtype)[torch.from_numpy(idx)]).view(3, 100, C)       # one add in the dtype
    lr_ref, lens_ref = orc.length_regulate(f64(args["xr"]), dur)
    dur_ref = orc.durations(ld, pm, 1.0)
    bits = GG.SIGNIFICAND_BITS[str(dtype).split(".")[1]]

    def call(a):
        tx, tw = leaf(a["x"]), leaf(a["emb"])
        out = d.bucketize_embed_add_autograd(tx, a["v"], a["bins"], tw)
        gx, gw = torch.autograd.grad(out, (tx, tw), a["go"])
        tr = leaf(a["xr"])
        o2, lens = d.length_regulate_autograd(tr, a["dur"])
        (gxr,) = torch.autograd.grad(o2, tr, a["gr"])
        with torch.no_grad():
            plain = d.bucketize_embed_add(a["x"], a["v"], a["bins"], a["emb"])
            p2, l2 = d.length_regulate(a["xr"], a["dur"])
            pd = d.predicted_durations(a["ld"], a["pm"], 1.0)
        return out.detach(), gx, gw, o2.detach(), lens, gxr, plain, p2, l2, pd

    def judge(tag, o):
        out, gx, gw, o2, lens, gxr, plain, p2, l2, pd = o
        assert torch.equal(out.cpu(), fwd_ref), f"{tag}: bucketize_embed_add_autograd forward"
        assert torch.equal(gx, args["go"]), f"{tag}: the gradient of x is the incoming gradient"
        if dtype == torch.float32:
            assert torch.equal(plain.cpu(), fwd_ref), f"{tag}: bucketize_embed_add"
        else:                                            # the fp32 kernel on the widened tensors, rounded once more on the way back
            np.testing.assert_allclose(f64(plain), xs.reshape(3, 100, C) + es[idx].reshape(3, 100, C), rtol=2.0 ** -bits, atol=0, err_msg=tag)
        for got in (o2, p2):
            np.testing.assert_array_equal(f64(got), lr_ref, err_msg=f"{tag}: length_regulate")
        for got in (lens, l2):
            np.testing.assert_array_equal(got.cpu().numpy(), lens_ref, err_msg=tag)
        g = f64(args["go"]).reshape(n, C)
        m_, a_ = GG.embed_grad_terms(g, idx, nb + 1)
        ref = GG.embed_grad_ref(g, idx, nb + 1)
        err = np.abs(f64(gw) - ref)
        assert not np.isnan(f64(gw)).any() and np.all(err <= GG.sum_bound(m_, a_, ref, bits)), f"{tag}: embed_grad beyond the derived bound"
        g = f64(args["gr"])
        m_, a_ = GG.length_regulator_bwd_terms(g, dur)
        ref = GG.length_regulator_bwd_ref(g, dur)
        err = np.abs(f64(gxr) - ref)
        assert not np.isnan(f64(gxr)).any() and np.all(err <= GG.sum_bound(m_, a_, ref, bits)), f"{tag}: length_regulator_bwd beyond the derived bound"
        diff = np.abs(pd.cpu().numpy() - dur_ref)                                      # test_durations_and_bucketize
        assert diff.max() <= 1 and (diff > 0).mean() < 0.005 and np.all(pd.cpu().numpy()[pm] == 0), f"{tag}: predicted_durations"
    base = call(args)
    judge("fresh", base)
    vary = ("x", "v", "bins", "emb", "go", "xr", "dur", "gr", "ld", "pm")

    def both(tag, o):
        judge(tag, o)
        same_bits(tag, o, base)                       # fixed-order sums and copies: the scalar branches give the bits of the vector ones
    sweep(args, vary, call, both)
    expanded_gradients(args, ("go", "gr"), call)


def _glance_keys(r):
    return tuple(r[k] for k in ("oracle", "n_right", "keep_prob", "revealed", "glanced"))


@covers("force_emit", "glance_select", "force_emit_served")
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_glancing_ops(dtype):
    """force_emit serves any row pitch and base and declines other strides; glance_select copies: every layout of every argument — and of the
    gradient — gives the bits of the torch formulation on fresh tensors (tests/test_gpu_glance_ops.py's rule: equality)"""
    d = D()
    B, T, L, Vn = 2, 9, 259, 50
    gen = torch.Generator(device="cuda").manual_seed(2590)
    m = torch.randn(B, T, L, device="cuda", generator=gen, dtype=torch.float32).to(dtype) * 2 - 3
    m[torch.rand(B, T, L, device="cuda", generator=gen) < 0.1] = float("-inf")
    n_tgt = torch.tensor([T, T - 2], device="cuda")
    path = torch.full((B, L), -1, dtype=torch.long, device="cuda")
    for b in range(B):
        pos = torch.randperm(L, device="cuda", generator=gen)[: int(n_tgt[b])].sort().values
        path[b, pos] = torch.arange(int(n_tgt[b]), device="cuda")
    revealed = torch.rand(B, L, device="cuda", generator=gen) < 0.4
    go = torch.randn(B, T, L, device="cuda", generator=gen, dtype=torch.float32).to(dtype)
    tgt = torch.randint(4, Vn, (B, T), device="cuda", generator=gen)
    guess = torch.where(torch.rand(B, L, device="cuda", generator=gen) < 0.5, tgt.gather(-1, path.clip(min=0)), torch.randint(4, Vn, (B, L), device="cuda", generator=gen))
    prev = torch.randint(0, 4, (B, L), device="cuda", generator=gen)
    noise = torch.tensor([-1.0, -0.0, 0.0, 0.5, 1.0], device="cuda")[torch.randint(0, 5, (B, L), device="cuda", generator=gen)]
    unif = torch.rand(B, L, device="cuda", generator=gen)
    args = dict(m=m, path=path, revealed=revealed, go=go, tgt=tgt, guess=guess, prev=prev, n_tgt=n_tgt, noise=noise, unif=unif)

    def call(a):
        mm = leaf(a["m"])
        out = d.force_emit(mm, a["path"], a["revealed"])
        (gm,) = torch.autograd.grad(out, mm, a["go"])
        sel = d.glance_select(a["tgt"], a["path"], a["guess"], a["prev"], a["n_tgt"], 0.5, "number-random", noise=a["noise"], unif=a["unif"])
        sel0 = d.glance_select(a["tgt"], a["path"], a["guess"], a["prev"], a["n_tgt"], 0.3, None, unif=a["unif"])
        return (out.detach(), gm) + _glance_keys(sel) + _glance_keys(sel0)
    old = d.set_glance_hip(False)
    try:
        want = call(args)
    finally:
        d.set_glance_hip(old)
    assert d.force_emit_served(m, path, revealed) and d._glance_served(tgt, path, guess, prev, unif)
    same_bits("fresh", call(args), want)
    sweep(args, tuple(args), call, base=want)
    expanded_gradients(args, ("go",), call)


# ================================================================================================ inference blocks

ROWS_B, ROWS_T, C256 = 2, 70, 256                   # B * T = 140: the first size past the 128-row floor with a partial tile


def _rebind(mod, names, how):
    """a deep copy of the module whose named parameters / buffers are views of a flat buffer (`.data` rebound), packed-weight caches dropped"""
    m = copy.deepcopy(mod)
    for sub in m.modules():
        for key in ("_dsp_split", "_dsp_cat"):
            sub.__dict__.pop(key, None)
    for name in names:
        owner, _, attr = name.rpartition(".")
        obj = m.get_submodule(owner) if owner else m
        t = getattr(obj, attr)
        t.data = how(t.data)
    return m


def _param_runs(names):
    """(tag, how) for the parameters: each at an odd offset, all at an odd offset, all as broadcast-free column slices"""
    runs = [(f"{n}:offset", (n,), V.at_offset) for n in names]
    runs.append(("params:offset", tuple(names), V.at_offset))
    runs.append(("params:colslice", tuple(names), V.column_slice))
    return runs


def _block_sweep(args, vary, mods, pnames, call, judge):
    """call(args, mods): the tensor arguments through every layout with the modules as they are, then the parameters rebound with fresh tensors,
    then both.  mods: dict name -> module; pnames: dict name -> parameter names to rebind"""
    judge("fresh", call(args, mods))
    fails = []
    n = sweep(args, vary, lambda a: call(a, mods), judge, collect=fails)
    offs = {k: V.at_offset(args[k]) for k in vary}
    for mname, names in pnames.items():
        for tag, which, how in _param_runs(names):
            m2 = {**mods, mname: _rebind(mods[mname], which, how)}
            for t, a in ((f"{mname}.{tag}", args), (f"{mname}.{tag}+args:offset", {**args, **offs})):
                try:
                    out = call(a, m2)
                    torch.cuda.synchronize()
                    judge(t, out)
                except (AssertionError, RuntimeError) as e:
                    msg = f"{type(e).__name__}: {e}"
                    if "illegal memory" in msg or "HIP error" in msg or "hipError" in msg:
                        _FAULT.append(t)
                        raise
                    fails.append(f"{t}: {msg[:400]}")
    assert not fails, f"{len(fails)} layouts failed:\n" + "\n".join(fails)
    return n


def _x256(seed, B=ROWS_B, T=ROWS_T, C=C256):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, T, C, generator=g) * 1.7 + 0.2).cuda()


def _ln(C, seed):
    ln = torch.nn.LayerNorm(C).cuda().eval()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        ln.weight.copy_((1.0 + 0.2 * torch.randn(C, generator=g)).cuda()); ln.bias.copy_((0.2 * torch.randn(C, generator=g)).cuda())
    return ln


def _lin(cin, cout, seed):
    torch.manual_seed(seed)
    return torch.nn.Linear(cin, cout).cuda().eval()


def _act(name):
    return {None: lambda t: t, "relu": torch.relu, "silu": F.silu, "gelu": F.gelu}[name]


@covers("layer_norm")
def test_layer_norm():
    """x and the LayerNorm's weight / bias in every layout: the kernel, or torch where the wrapper declines — 2e-6 of float64 either way
    (test_layer_norm_against_float64)"""
    x, ln = _x256(81), _ln(C256, 82)

    def call(a, m):
        with torch.no_grad():
            return D().layer_norm(a["x"], m["ln"])

    def judge(tag, got):
        ref = F.layer_norm(x.double(), (C256,), ln.weight.double(), ln.bias.double(), ln.eps)
        judged(tag, got, ref, F.layer_norm(x, (C256,), ln.weight, ln.bias, ln.eps), 2e-6)
    _block_sweep(dict(x=x), ("x",), dict(ln=ln), dict(ln=("weight", "bias")), call, judge)


@covers("dwconv_bn_silu")
@pytest.mark.parametrize("K", [3, 31])
def test_dwconv_bn_silu(K):
    """eval mode: x, the depthwise weight and the four BatchNorm tensors in every layout — no torch path, so every one is copied where it has to
    be: the bits of the call on fresh tensors, which meets float64 by test_dwconv_bn_silu_against_float64's rule (1e-5)"""
    B, T, C = 2, 70, 256
    x, w, bw, bb, mean, var = G.dwconv_inputs(75, B, T, C, K)
    ref = G.dwconv_bn_silu_ref(x, w, bw, bb, mean, var, 1e-5)
    dw = torch.nn.Conv1d(C, C, K, padding=(K - 1) // 2, groups=C, bias=False).cuda()
    bn = torch.nn.BatchNorm1d(C, eps=1e-5).cuda().eval()
    with torch.no_grad():
        dw.weight.copy_(cu(w).unsqueeze(1)); bn.weight.copy_(cu(bw)); bn.bias.copy_(cu(bb)); bn.running_mean.copy_(cu(mean)); bn.running_var.copy_(cu(var))
        ref32 = F.silu(bn(dw(cu(x).transpose(1, 2)))).transpose(1, 2)

    def call(a, m):
        with torch.no_grad():
            return D().dwconv_bn_silu(a["x"], m["dw"].weight, m["bn"])
    base = call(dict(x=cu(x)), dict(dw=dw, bn=bn))
    judged("fresh", base, torch.from_numpy(ref), ref32, 1e-5)
    _block_sweep(dict(x=cu(x)), ("x",), dict(dw=dw, bn=bn), dict(dw=("weight",), bn=("weight", "bias", "running_mean", "running_var")), call,
                 lambda tag, got: same_bits(tag, got, base))


def _conv_ref(x, w, b, act, res, alpha, dt):
    y = F.conv1d(x.to(dt).transpose(1, 2), w.to(dt), None if b is None else b.to(dt), padding=(w.shape[2] - 1) // 2).transpose(1, 2)
    y = alpha * _act(act)(y)
    return y if res is None else res.to(dt) + y


@covers("SplitConv1d")
@pytest.mark.parametrize("K", [1, 9])
def test_split_conv1d_called_directly(K):
    """a pitched x and a view residual (and every other layout of both): SplitConv1d serves unit-stride rows with a pitch that is a multiple of
    4 on the grid and copies the rest; test_split_precision_conv1d_is_fp32_accurate's rule (8 x torch fp32 against float64)"""
    torch.manual_seed(K)
    conv = torch.nn.Conv1d(C256, C256, K, padding=(K - 1) // 2).cuda().eval()
    x, res = _x256(90 + K), _x256(190 + K)

    def call(a, m):
        sc = D().SplitConv1d(m["conv"].weight, m["conv"].bias)
        with torch.no_grad():
            return sc(a["x"], act="silu"), sc(a["x"], act="relu", residual=a["res"], alpha=0.5)

    def judge(tag, out):
        for got, (act, r, al) in zip(out, (("silu", None, 1.0), ("relu", res, 0.5))):
            ref = _conv_ref(x, conv.weight, conv.bias, act, r, al, torch.float64)
            with torch.no_grad():
                judged_gemm(f"{tag} {act}", got, ref, _conv_ref(x, conv.weight, conv.bias, act, r, al, torch.float32))
    _block_sweep(dict(x=x, res=res), ("x", "res"), dict(conv=conv), dict(conv=("bias",)), call, judge)


@covers("linear", "split_linear", "linear_fused", "linear_ln", "valid_lengths")
def test_linear_family():
    """linear (with activation, residual and scale), linear_fused and linear_ln on x, the residual and the parameters in every layout: the split
    GEMM where the wrapper serves, F.linear where it declines — the caps of tests/util_block_ref.py against float64 either way.  valid_lengths
    takes its mask in every layout too (pure torch: exact)."""
    x, res, ln = _x256(11), _x256(12), _ln(C256, 13)
    l1, lq, lk, lv = _lin(C256, 512, 14), _lin(C256, 256, 15), _lin(C256, 256, 16), _lin(C256, 256, 17)
    pad = torch.arange(ROWS_T, device="cuda").unsqueeze(0) >= torch.tensor([ROWS_T, 41], device="cuda").unsqueeze(1)

    def call(a, m):
        d = D()
        with torch.no_grad():
            y1 = d.linear(a["x"], m["l1"], act="gelu")
            y2 = d.linear(a["x"], m["lq"], residual=a["res"], alpha=0.5)
            q, k, v = d.linear_fused(a["x"], (m["lq"], m["lk"], m["lv"]))
            nq, nk = d.linear_ln(a["x"], m["ln"], (m["lq"], m["lk"]))
            (n1,) = d.linear_ln(a["x"], m["ln"], (m["l1"],), act="silu")
            return y1, y2, q, k, v, nq, nk, n1, d.valid_lengths(a["pad"])

    def judge(tag, out):
        y1, y2, q, k, v, nq, nk, n1, lens = out
        assert lens.tolist() == [ROWS_T, 41] and lens.dtype == torch.int32, tag

        def one(name, got, mod, act, r, al, xin64, xin32, cap):
            ref = al * _act(act)(F.linear(xin64, mod.weight.double(), mod.bias.double()))
            r32 = al * _act(act)(F.linear(xin32, mod.weight, mod.bias))
            if cap is None:
                judged_gemm(f"{tag} {name}", got, ref if r is None else r.double() + ref, r32 if r is None else r + r32)
            else:
                judged(f"{tag} {name}", got, ref if r is None else r.double() + ref, r32 if r is None else r + r32, cap)
        xn64 = F.layer_norm(x.double(), (C256,), ln.weight.double(), ln.bias.double(), ln.eps)
        xn32 = F.layer_norm(x, (C256,), ln.weight, ln.bias, ln.eps)
        one("linear gelu", y1, l1, "gelu", None, 1.0, x.double(), x, None)
        one("linear residual", y2, lq, None, res, 0.5, x.double(), x, None)
        for name, got, mod in (("q", q, lq), ("k", k, lk), ("v", v, lv)):
            one(f"linear_fused {name}", got, mod, None, None, 1.0, x.double(), x, None)
        for name, got, mod, act in (("q", nq, lq, None), ("k", nk, lk, None), ("l1", n1, l1, "silu")):
            one(f"linear_ln {name}", got, mod, act, None, 1.0, xn64, xn32, BR.LINEAR_LN_CAP)
    pn = dict(ln=("weight", "bias"), l1=("bias",), lq=("bias",))
    _block_sweep(dict(x=x, res=res, pad=pad), ("x", "res", "pad"), dict(ln=ln, l1=l1, lq=lq, lk=lk, lv=lv), pn, call, judge)


@covers("ffn_fused")
def test_ffn_fused():
    """x, the residual and the parameters (both LayerNorms, both biases) in every layout; where ffn_fused answers None the caller's two-GEMM
    lines are what the public path returns (ConformerLayer._ffn).  FFN_CAP of float64 (test_ffn_fused_matches_fp64_and_the_two_gemm_path)"""
    x, res = _x256(21), _x256(22)
    ln, post, l1, l2 = _ln(C256, 23), _ln(C256, 24), _lin(C256, 1024, 25), _lin(1024, C256, 26)

    def call(a, m):
        d = D()
        with torch.no_grad():
            got = d.ffn_fused(a["x"], m["ln"], m["l1"], m["l2"], "silu", residual=a["res"], alpha=0.5, post_ln=m["post"])
            if got is None:                          # not served: the lines of the caller
                out = d.linear(d.linear(d.layer_norm(a["x"], m["ln"]), m["l1"], act="silu"), m["l2"], residual=a["res"], alpha=0.5)
                got = (out, d.layer_norm(out, m["post"]))
            return got

    def judge(tag, out):
        o, oln = out
        h = F.silu(F.linear(F.layer_norm(x.double(), (C256,), ln.weight.double(), ln.bias.double(), ln.eps), l1.weight.double(), l1.bias.double()))
        ref = res.double() + 0.5 * F.linear(h, l2.weight.double(), l2.bias.double())
        h32 = F.silu(F.linear(F.layer_norm(x, (C256,), ln.weight, ln.bias, ln.eps), l1.weight, l1.bias))
        r32 = res + 0.5 * F.linear(h32, l2.weight, l2.bias)
        judged(f"{tag} out", o, ref, r32, BR.FFN_CAP)
        judged(f"{tag} post_ln", oln, F.layer_norm(ref, (C256,), post.weight.double(), post.bias.double(), post.eps),
               F.layer_norm(r32, (C256,), post.weight, post.bias, post.eps), 3e-6)
    assert D().ffn_fused(x, ln, l1, l2, "silu", residual=res, alpha=0.5, post_ln=post) is None          # (grad mode: declined; the sweep runs under no_grad)
    with torch.no_grad():
        assert D().ffn_fused(x, ln, l1, l2, "silu", residual=res, alpha=0.5, post_ln=post) is not None
    pn = dict(ln=("weight", "bias"), post=("weight", "bias"), l1=("bias",), l2=("bias",))
    _block_sweep(dict(x=x, res=res), ("x", "res"), dict(ln=ln, post=post, l1=l1, l2=l2), pn, call, judge)


@covers("linear", "layer_norm", "linear_ln", "ffn_fused", "SplitConv1d", "dwconv_bn_silu")
def test_tail_of_a_one_utterance_batch():
    """x[:, 1:] of a batch of one: torch calls it contiguous (the stride of a dimension of length 1 does not count) and with C = 256 it sits on
    the 16-byte grid, but its batch stride is not T * C.  The data is dense, so every block serves it: the bits of the call on a copy."""
    d = D()
    T = 140
    full = _x256(31, 1, T + 1, C256)
    x = full[:, 1:]
    assert x.is_contiguous() and x.data_ptr() % 16 == 0 and x.stride(0) != x.shape[1] * x.stride(1)
    ln, l1, l2 = _ln(C256, 32), _lin(C256, 512, 33), _lin(512, C256, 34)
    conv = torch.nn.Conv1d(C256, C256, 3, padding=1).cuda().eval()
    dw = torch.nn.Conv1d(C256, C256, 7, padding=3, groups=C256, bias=False).cuda()
    bn = torch.nn.BatchNorm1d(C256).cuda().eval()

    def call(t):
        with torch.no_grad():
            sc = d.SplitConv1d(conv.weight, conv.bias)
            return (d.layer_norm(t, ln), d.linear(t, l1, act="relu"), d.linear_ln(t, ln, (l1,))[0], d.ffn_fused(t, ln, l1, l2, "silu", residual=t, alpha=0.5),
                    sc(t, act="silu", residual=t), d.dwconv_bn_silu(t, dw.weight, bn))
    base = call(x.clone())
    assert all(o is not None for o in base)
    judged("layer_norm", base[0], F.layer_norm(x.double(), (C256,), ln.weight.double(), ln.bias.double(), ln.eps), F.layer_norm(x, (C256,), ln.weight, ln.bias, ln.eps), 2e-6)
    judged_gemm("linear", base[1], torch.relu(F.linear(x.double(), l1.weight.double(), l1.bias.double())), torch.relu(F.linear(x, l1.weight, l1.bias)))
    same_bits("x[:, 1:]", call(x), base)


ATT_T, ATT_H = 77, 2


def _sdpa(q, k, v, pad, H):
    B, N, C = q.shape
    sp = lambda t: t.reshape(B, t.shape[1], H, C // H).transpose(1, 2)
    m = None if pad is None else ~pad.reshape(B, 1, 1, -1)
    return F.scaled_dot_product_attention(sp(q), sp(k), sp(v), attn_mask=m).transpose(1, 2).reshape(B, N, C)


@covers("attention", "relpos_attention")
def test_attention_ops():
    """q, k, v, the mask, the positions and the two biases in every layout, dk = 64, T = 77: column slices and pitched rows are served, the rest
    is declined (the public path then is torch's scaled_dot_product_attention / the module's relative-position lines) — att_cap of the float64
    restatements of tests/util_block_ref.py either way"""
    B, T, H = 2, ATT_T, ATT_H
    C = H * 64
    g = torch.Generator().manual_seed(77)
    rn = lambda *s: torch.randn(*s, generator=g).cuda()
    q, k, v, pos, bu, bv = rn(B, T, C), rn(B, T, C), rn(B, T, C), rn(1, 2 * T - 1, C), 0.5 * rn(H, 64), 0.5 * rn(H, 64)
    pad = torch.arange(T, device="cuda").unsqueeze(0) >= torch.tensor([T, 50], device="cuda").unsqueeze(1)
    o64, s64 = BR.attention_ref(q.cpu(), k.cpu(), v.cpu(), pad.cpu(), H, 64 ** -0.5)
    r64, rs64 = BR.relpos_attention_ref(q.cpu(), k.cpu(), v.cpu(), pos[0].cpu(), bu.cpu(), bv.cpu(), pad.cpu(), H)
    o32 = BR.attention_ref(q.cpu(), k.cpu(), v.cpu(), pad.cpu(), H, 64 ** -0.5, dtype=torch.float32)[0]
    r32 = BR.relpos_attention_ref(q.cpu(), k.cpu(), v.cpu(), pos[0].cpu(), bu.cpu(), bv.cpu(), pad.cpu(), H, dtype=torch.float32)[0]
    served = []

    def call(a):
        d = D()
        with torch.no_grad():
            o = d.attention(a["q"], a["k"], a["v"], a["pad"], H)
            r = d.relpos_attention(a["q"], a["k"], a["v"], a["pos"], a["bu"], a["bv"], a["pad"], H)
            served.append((o is not None, r is not None))
            if o is None:
                o = _sdpa(a["q"], a["k"], a["v"], a["pad"], H)
            if r is None:                            # the module's relative-position lines
                r = RA.module_lines(a["q"].contiguous(), a["k"].contiguous(), a["v"].contiguous(), a["pos"].reshape(-1, C).contiguous(), a["bu"], a["bv"],
                                    a["pad"].contiguous(), H)[0]
            return o, r

    def judge(tag, out):
        o, r = out
        judged(f"{tag} attention", o, o64, o32, BR.att_cap(s64))
        judged(f"{tag} relpos_attention", r, r64, r32, BR.att_cap(rs64))
    args = dict(q=q, k=k, v=v, pad=pad, pos=pos, bu=bu, bv=bv)
    judge("fresh", call(args))
    assert served[-1] == (True, True)
    sweep(args, tuple(args), call, judge)
    both = [s for s in served if s == (True, True)]
    assert len(both) > 8, "column slices, pitched rows and copied positions / biases / masks stay on the HIP kernels"


# ================================================================================================ training operators

TRAIN_DTYPES = [torch.float32, torch.float16, torch.bfloat16]
TRAIN_IDS = ["f32", "f16", "bf16"]


def _grads(outs, ins, cots):
    return torch.autograd.grad(outs, ins, cots, allow_unused=True)


@covers("dwconv_bn_silu_autograd", "dwconv_bn_silu_autograd_served")
@pytest.mark.parametrize("dtype", TRAIN_DTYPES, ids=TRAIN_IDS)
def test_dwconv_bn_silu_autograd(dtype):
    """x, the incoming gradient and the parameters in every layout through the public operator (copies: the bits of the fresh call, which holds
    the 4 x rule against the module's torch lines in float64) and through the `served` predicate, which has to say no to every x it cannot hand
    over as it is — its answer decides between the operator and the torch lines, as in ConformerLayer"""
    d = D()
    B, T, C, K = 3, 5, 8, 31                                         # the smallest edge shape of tests/test_gpu_convmod_autograd.py with B * T > 8
    x, w, gamma, beta, gy, rm, rv = CM.inputs(7 * T + K + C, B, T, C, K)
    conv = torch.nn.Conv1d(C, C, K, padding=(K - 1) // 2, groups=C, bias=False).cuda().to(dtype)
    bn = torch.nn.BatchNorm1d(C).cuda().to(dtype).train()
    with torch.no_grad():
        conv.weight.copy_(cu(w, dtype).unsqueeze(1)); bn.weight.copy_(cu(gamma, dtype)); bn.bias.copy_(cu(beta, dtype))
        bn.running_mean.copy_(cu(rm, dtype)); bn.running_var.copy_(cu(rv, dtype))
    args = dict(x=cu(x, dtype), gy=cu(gy, dtype))

    def lines(a, cv, b, dt):
        xx, ww, g_, b_ = leaf(a["x"].to(dt)), leaf(cv.weight.to(dt)), leaf(b.weight.to(dt)), leaf(b.bias.to(dt))
        z = F.conv1d(xx.transpose(1, 2), ww, None, 1, (K - 1) // 2, 1, C)
        y = F.silu(F.batch_norm(z, None, None, g_, b_, True, 0.1, b.eps)).transpose(1, 2)
        return (y.detach(),) + tuple(_grads(y, [xx, ww, g_, b_], a["gy"].to(dt)))

    def op(a, cv, b, ask):
        if ask and not d.dwconv_bn_silu_autograd_served(a["x"], cv, b):
            return lines(a, cv, b, dtype), False
        xx, ww, g_, b_ = leaf(a["x"]), leaf(cv.weight), leaf(b.weight), leaf(b.bias)
        rm_, rv_ = V.at_offset(b.running_mean) if b.running_mean.data_ptr() % 16 else b.running_mean.clone(), b.running_var.clone()   # updated in place
        b2 = types.SimpleNamespace(weight=g_, bias=b_, running_mean=rm_, running_var=rv_, momentum=0.1, eps=b.eps, num_features=C, num_batches_tracked=None)
        y = d.dwconv_bn_silu_autograd(xx, ww, b2)
        return (y.detach(),) + tuple(_grads(y, [xx, ww, g_, b_], a["gy"])), True
    names = ("y", "dx", "dw", "dgamma", "dbeta")
    ref = dict(zip(names, (f64(t) for t in lines(args, conv, bn, torch.float64))))
    tor = dict(zip(names, lines(args, conv, bn, dtype)))
    base, _ = op(args, conv, bn, False)
    check_4x(f"views convmod {dtype}", dict(zip(names, base)), tor, ref)
    assert d.dwconv_bn_silu_autograd_served(args["x"], conv, bn)
    asked = []

    def call_public(a):
        return op(a, conv, bn, False)[0]

    def call_asked(a):
        out, hip = op(a, conv, bn, True)
        asked.append(hip)
        return out
    sweep(args, ("x", "gy"), call_public, base=base)
    expanded_gradients(args, ("gy",), call_public)
    sweep(args, ("x", "gy"), call_asked, lambda tag, out: check_4x(f"{tag} {dtype}", dict(zip(names, out)), tor, ref))
    assert any(asked) and not all(asked), "the gradient layouts stay with the operator, the x layouts it cannot take go to torch"
    for tag, which, how in _param_runs(("weight", "bias", "running_mean", "running_var")):
        b2 = _rebind(bn, which, how)
        c2 = _rebind(conv, ("weight",), how)
        assert d.dwconv_bn_silu_autograd_served(args["x"], c2, b2), tag          # read element by element: served as they are
        same_bits(tag, op(args, c2, b2, True)[0], base)


@covers("residual_dropout_layer_norm_autograd", "residual_dropout_layer_norm_served", "residual_dropout_layer_norm_sites_served",
        "residual_dropout_layer_norm_checked")
@pytest.mark.parametrize("dtype", TRAIN_DTYPES, ids=TRAIN_IDS)
def test_residual_dropout_layer_norm_autograd(dtype):
    """h, the residual, both incoming gradients, `bias` and the LayerNorm's parameters in every layout, p = 0: through the public operator
    (copies: the bits of the fresh call, which holds the 4 x rule against the torch lines in float64), and through the two predicates, whose
    answer decides between the `checked` entry and the torch lines as in the layers"""
    d = D()
    R, C = 33, 72                                                    # a chunk and one row, a ragged number of 16-byte groups per lane
    t = RN.inputs(3, R, C)
    ln = torch.nn.LayerNorm(C).cuda().to(dtype)
    with torch.no_grad():
        ln.weight.copy_(cu(t["gamma"], dtype)); ln.bias.copy_(cu(t["beta"], dtype))
    args = dict(h=cu(t["h"], dtype), res=cu(t["residual"], dtype), bias=cu(t["bias"], dtype), dy=cu(t["dy"], dtype), ds=cu(t["ds"], dtype))
    names = ("s", "y", "dh", "dres", "dbias", "dgamma", "dbeta")

    def lines(a, l, dt):
        h, r, b, g_, b_ = (leaf(x.to(dt)) for x in (a["h"], a["res"], a["bias"], l.weight, l.bias))
        s = r + 0.5 * (h + b)
        y = F.layer_norm(s, (C,), g_, b_, l.eps)
        return (s.detach(), y.detach()) + tuple(_grads([s, y], [h, r, b, g_, b_], [a["ds"].to(dt), a["dy"].to(dt)]))

    def op(a, l, ask):
        h, r, b, g_, b_ = (leaf(x) for x in (a["h"], a["res"], a["bias"], l.weight, l.bias))
        l2 = types.SimpleNamespace(weight=g_, bias=b_, eps=l.eps, normalized_shape=(C,))
        if ask == "served" and not d.residual_dropout_layer_norm_served(h, r, l2, bias=b):
            return lines(a, l, dtype), False
        if ask == "sites" and not d.residual_dropout_layer_norm_sites_served(r, ((l2, b),)):      # h is a block's output: `checked` copies a view of it
            return lines(a, l, dtype), False
        fn = d.residual_dropout_layer_norm_autograd if ask is None else d.residual_dropout_layer_norm_checked
        s, y = fn(h, r, l2, bias=b, alpha=0.5, p=0.0, training=True)
        return (s.detach(), y.detach()) + tuple(_grads([s, y], [h, r, b, g_, b_], [a["ds"], a["dy"]])), True
    ref = dict(zip(names, (f64(x) for x in lines(args, ln, torch.float64))))
    tor = dict(zip(names, lines(args, ln, dtype)))
    base, _ = op(args, ln, None)
    check_4x(f"views resnorm {dtype}", dict(zip(names, base)), tor, ref)
    same_bits("checked", op(args, ln, "served")[0], base)
    vary = ("h", "res", "bias", "dy", "ds")
    sweep(args, vary, lambda a: op(a, ln, None)[0], base=base)
    expanded_gradients(args, ("dy", "ds"), lambda a: op(a, ln, None)[0])
    for ask in ("served", "sites"):
        hips = []

        def call(a):
            out, hip = op(a, ln, ask)
            hips.append(hip)
            return out
        sweep(args, vary, call, lambda tag, out: check_4x(f"{ask} {tag} {dtype}", dict(zip(names, out)), tor, ref))
        assert any(hips) and not all(hips), ask
    for tag, which, how in _param_runs(("weight", "bias")):
        l2 = _rebind(ln, which, how)
        same_bits(f"public {tag}", op(args, l2, None)[0], base)
        for ask in ("served", "sites"):
            out, hip = op(args, l2, ask)
            assert hip == all(getattr(l2, n_).data_ptr() % 16 == 0 for n_ in ("weight", "bias")), (tag, ask)      # parameters off the grid: the torch lines
            check_4x(f"{ask} {tag} {dtype}", dict(zip(names, out)), tor, ref)


@covers("relpos_attention_autograd", "relpos_attention_autograd_served", "relpos_attention_checked")
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_relpos_attention_autograd(dtype):
    """q, k, v, the positions, the biases, the mask and the incoming gradient in every layout, p = 0, T = 33 (a block of 32 and one), B = 3,
    H = 1: the public operator copies what the kernels do not take (bits of the fresh call, which holds the 4 x rule against the module's torch
    lines in float64); the predicate decides between `checked` and the torch lines as RelPosSelfAttention does"""
    d = D()
    T, B, H = 33, 3, 1
    t = RA.inputs(1000 * T + 10 * B + H, B, T, H)
    pad = RA.pad_masks("ragged", B, T)
    args = {k: cu(v, dtype) for k, v in t.items()}
    args["pad"] = cu(pad)
    names = ("o", "dq", "dk", "dv", "dpos", "du", "dv_bias")
    ins = ("q", "k", "v", "pos", "bias_u", "bias_v")

    def lines(a, dt):
        x = [leaf(a[n].to(dt).contiguous()) for n in ins]
        o = RA.module_lines(*x, a["pad"].contiguous(), H)[0]
        return (o.detach(),) + tuple(_grads(o, x, a["do"].to(dt)))

    def op(a, ask):
        x = [leaf(a[n]) for n in ins]
        if ask and not d.relpos_attention_autograd_served(*x, a["pad"], H):
            return lines(a, dtype), False
        fn = d.relpos_attention_checked if ask else d.relpos_attention_autograd
        o = fn(*x, a["pad"], H, p=0.0, training=True)
        return (o.detach(),) + tuple(_grads(o, x, a["do"])), True
    ref = dict(zip(names, (f64(x) for x in lines(args, torch.float64))))
    tor = dict(zip(names, lines(args, dtype)))
    base, _ = op(args, False)
    check_4x(f"views relpos {dtype}", dict(zip(names, base)), tor, ref)
    vary = ins + ("pad", "do")
    sweep(args, vary, lambda a: op(a, False)[0], base=base)
    expanded_gradients(args, ("do",), lambda a: op(a, False)[0])
    hips = []

    def call(a):
        out, hip = op(a, True)
        hips.append(hip)
        return out
    sweep(args, vary, call, lambda tag, out: check_4x(f"{tag} {dtype}", dict(zip(names, out)), tor, ref))
    assert any(hips) and not all(hips)
    # fp32 is not served by this operator (fp32 layers keep their torch lines): the predicate says no and the public operator keeps its
    # documented error, on fresh tensors and on every layout alike
    a32 = {n: args[n].float() for n in ins}
    for tag, q32 in [("fresh", a32["q"])] + [(n, v_) for n, v_ in V.every_variant(a32["q"])]:
        x = [q32] + [a32[n] for n in ins[1:]]
        assert not d.relpos_attention_autograd_served(*x, args["pad"], H), tag
        with pytest.raises(RuntimeError, match="have to be fp16 or bf16, got torch.float32"):
            d.relpos_attention_autograd(*x, args["pad"], H)


@covers("set_conv_module_hip", "set_residual_norm_hip", "set_relpos_attention_hip")
@pytest.mark.parametrize("dtype", TRAIN_DTYPES, ids=TRAIN_IDS)
def test_conformer_layer_training_with_the_switches_on(dtype):
    """ConformerLayer in training mode (p = 0) on x, the positions and the mask in every layout, and with its LayerNorm / BatchNorm parameters as
    views of a flat buffer: the three training operators where their predicates say yes, the torch lines elsewhere — output and every gradient
    within 4 x of the all-torch layer (the three switches off) against the same layer in float64"""
    from daspeech_amd.models.daspeech import ConformerLayer
    d = D()
    B, T, C = 2, 11, 64
    torch.manual_seed(3)
    layer = ConformerLayer(C, 128, 1, 7, dropout=0.0).cuda().train()
    g = torch.Generator().manual_seed(4)
    x0, pos0, cot0 = (torch.randn(*s, generator=g).cuda() for s in ((B, T, C), (1, 2 * T - 1, C), (B, T, C)))
    pad = torch.arange(T, device="cuda").unsqueeze(0) >= torch.tensor([T, T - 3], device="cuda").unsqueeze(1)
    pnames = sorted(n for n, _ in layer.named_parameters())

    def run(m, a, dt):                               # (no copy of m: a deep copy would put rebound parameters back on the grid)
        x = leaf(a["x"].to(dt))
        out = m(x, a["pos"].to(dt), a["pad"])
        ps = dict(m.named_parameters())
        gr = _grads(out, [x] + [ps[n] for n in pnames], a["cot"].to(dt))
        res = dict(zip(["out", "dx"] + pnames, (out.detach(),) + tuple(gr)))
        res.pop("self_attn.linear_k.bias")           # zero in exact arithmetic (the soft-max ignores a shift of every score of a row): no scale for a figure
        return res
    args = dict(x=x0.to(dtype), pos=pos0.to(dtype), pad=pad, cot=cot0.to(dtype))
    ref = {k: f64(v) for k, v in run(copy.deepcopy(layer).double(), args, torch.float64).items()}
    lay = copy.deepcopy(layer).to(dtype)
    olds = (d.set_conv_module_hip(False), d.set_residual_norm_hip(False), d.set_relpos_attention_hip(False))
    try:
        tor = run(lay, args, dtype)
    finally:
        d.set_conv_module_hip(olds[0]); d.set_residual_norm_hip(olds[1]); d.set_relpos_attention_hip(olds[2])
    assert all(olds), "the switches are on by default"

    def judge(tag, out):
        check_4x(f"layer {tag} {dtype}", out, tor, ref)
    judge("fresh", run(lay, args, dtype))
    sweep(args, ("x", "pos", "pad", "cot"), lambda a: run(lay, a, dtype), judge)
    norm_params = [n for n in pnames if "layer_norm" in n or "batch_norm" in n or n.endswith("w_2.bias") or "pos_bias" in n]
    for tag, which, how in (("params:offset", norm_params, V.at_offset), ("params:colslice", norm_params, V.column_slice)):
        judge(tag, run(_rebind(lay, which, how), args, dtype))


# ================================================================================================ vocoder

@covers("HiFiGANHipRunner")
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_vocoder_mel_layouts(precision):
    """HiFiGANHipRunner.__call__ on a mel spectrogram [B, 80, T = 37] that is a transposed view, at an odd offset, and every other layout: the
    runner copies it into its own padded buffer, so every layout gives the bits of the fresh call, which tracks the torch fp32 generator as in
    tests/test_tts_golden.py (1e-4) and tools/fuzz_vocoder.py (fp16 storage: 2e-2 max, 2e-3 mean)"""
    from daspeech_amd.hifigan_ops import HiFiGANHipRunner
    from daspeech_amd.models import HiFiGANGenerator
    torch.manual_seed(6)
    gmod = HiFiGANGenerator().cuda().eval()
    with torch.no_grad():
        for p in gmod.parameters():
            p.copy_(torch.randn_like(p) / (p.shape[1] * p.shape[2]) ** 0.5 if p.dim() > 1 else torch.randn_like(p) * 0.05)
    run = HiFiGANHipRunner(gmod, precision=precision)
    mel = torch.randn(2, 80, 37, device="cuda")
    lens = torch.tensor([37, 20], device="cuda")
    mel = mel.masked_fill(torch.arange(37, device="cuda").view(1, 1, -1) >= lens.view(-1, 1, 1), 0)
    args = dict(mel=mel, lens=lens)

    def call(a):
        return run(a["mel"]), run(a["mel"], a["lens"])
    base = call(args)
    with torch.no_grad():
        ref = gmod(mel)
    err = (base[0] - ref).abs()
    if precision == "fp32":
        assert err.max().item() < 1e-4, err.max().item()
    else:
        assert err.max().item() < 2e-2 and err.mean().item() < 2e-3, (err.max().item(), err.mean().item())
    sweep(args, ("mel", "lens"), call, base=base)


# ================================================================================================ the C contract: gates and alignment-selected branches

def _rc_msg(rc):
    return rc, LIB().load().dsp_last_error().decode("utf-8", "replace")


def test_c_gates_refuse_off_grid_pointers_and_leave_the_output_alone():
    """the gates the wrappers now keep every caller away from are the C contract: DSP_EINVAL, a message naming the alignment, output untouched"""
    lib, L = LIB(), LIB().load()
    st = lib.current_stream_handle()
    rows, C = 9, 256
    x, w, b = (cu(t) for t in G.layer_norm_inputs(84, rows, C, 1.5, 3.0))
    for which in ("x", "w", "b", "y"):
        t = dict(x=x, w=w, b=b, y=torch.full((rows, C), NAN, device="cuda"))
        t[which] = V.at_offset(t[which])
        rc, msg = _rc_msg(L.dsp_layer_norm(lib.ptr(t["x"]), lib.ptr(t["w"]), lib.ptr(t["b"]), 1e-5, lib.ptr(t["y"]), rows, C, st))
        torch.cuda.synchronize()
        assert rc == DSP_EINVAL and "16-byte aligned" in msg, (which, rc, msg)
        assert torch.isnan(t["y"]).all(), which
    B, T, Cc, K = 2, 9, 64, 7
    xx, ww, bw, bb, mean, var = (cu(t) for t in G.dwconv_inputs(74, B, T, Cc, K))
    for which in ("x", "y"):
        t = dict(x=xx, y=torch.full((B, T, Cc), NAN, device="cuda"))
        t[which] = V.at_offset(t[which])
        rc, msg = _rc_msg(L.dsp_dwconv_bn_silu(lib.ptr(t["x"]), lib.ptr(ww), lib.ptr(bw), lib.ptr(bb), lib.ptr(mean), lib.ptr(var), 1e-5, lib.ptr(t["y"]),
                                               B, T, Cc, K, st))
        torch.cuda.synchronize()
        assert rc == DSP_EINVAL and "16-byte aligned" in msg, (which, rc, msg)
        assert torch.isnan(t["y"]).all(), which
    q = torch.randn(2, 64, 8, 64, device="cuda")
    g = torch.log_softmax(torch.randn(2, 64, 8, device="cuda"), -1)
    ol = torch.tensor([64, 41], device="cuda")
    for which in ("q", "k"):
        t = dict(q=q, k=q.clone())
        t[which] = V.at_offset(t[which])
        links = torch.full((2, 64, 7), NAN, device="cuda")
        rc, msg = _rc_msg(L.dsp_extract_links(lib.ptr(t["q"]), lib.ptr(t["k"]), lib.ptr(g), lib.ptr(ol), None, lib.ptr(links), 2, 64, 8, 64, 7, 0.125, st))
        torch.cuda.synchronize()
        assert rc == DSP_EINVAL and "16-byte aligned" in msg, (which, rc, msg)
        assert torch.isnan(links).all(), which


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_row_copies_and_gradient_sums_behind_an_off_grid_base_pointer(dtype):
    """dsp_gather_rows, dsp_length_regulator_expand, dsp_length_regulator_bwd and dsp_embed_grad choose 16-byte or element accesses by the
    alignment of base pointers and rows.  Rows of 16-byte multiples (C = 24) with the input, the output, or both 1 element off the grid, outputs
    pre-filled with NaN: exactly the rows the aligned call gives (copies and fixed-order sums)."""
    lib, L = LIB(), LIB().load()
    st = lib.current_stream_handle()
    code = lib.DTYPE_CODES[str(dtype)]
    B, Lg, Dm, cap = 3, 40, 24, 40
    rng = np.random.default_rng(5)
    feats = cu(rng.standard_normal((B, Lg, Dm)).astype(np.float32), dtype)
    keep = cu(np.stack([rng.permutation(Lg) for _ in range(B)]).astype(np.int32))
    nfeat = cu(np.array([40, 17, 0], np.int32))
    dur = rng.poisson(2.0, (B, Lg)).astype(np.int64)
    cum = cu(np.cumsum(dur, 1))
    maxlen = int(dur.sum(1).max())
    gout = cu(rng.standard_normal((B, maxlen, Dm)).astype(np.float32), dtype)
    idx = cu(rng.integers(0, 10, B * Lg).astype(np.int32))
    nbytes = int(L.dsp_embed_grad_workspace_bytes(B * Lg, 9, Dm))

    def poisoned(shape, off):
        t = torch.full(shape, NAN, dtype=dtype, device="cuda")
        return V.at_offset(t) if off else t

    def run(off_in, off_out):
        src = V.at_offset(feats) if off_in else feats
        g = V.at_offset(gout) if off_in else gout
        out1, out2, gx, ge = poisoned((B, cap, Dm), off_out), poisoned((B, maxlen, Dm), off_out), poisoned((B, Lg, Dm), off_out), poisoned((10, Dm), off_out)
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        lib.check(L.dsp_gather_rows(lib.ptr(src), code, lib.ptr(keep), lib.ptr(nfeat), lib.ptr(out1), B, Lg, Dm, cap, cap, st), "dsp_gather_rows")
        lib.check(L.dsp_length_regulator_expand(lib.ptr(src), code, lib.ptr(cum), lib.ptr(out2), B, Lg, Dm, maxlen, st), "dsp_length_regulator_expand")
        lib.check(L.dsp_length_regulator_bwd(lib.ptr(g), code, lib.ptr(cum), lib.ptr(gx), B, Lg, Dm, maxlen, st), "dsp_length_regulator_bwd")
        lib.check(L.dsp_embed_grad(lib.ptr(g.view(-1, Dm)[: B * Lg]), code, lib.ptr(idx), lib.ptr(ge), B * Lg, 9, Dm, lib.ptr(ws), nbytes, st), "dsp_embed_grad")
        torch.cuda.synchronize()
        return out1, out2, gx, ge
    base = run(False, False)
    ref1 = G.gather_rows_ref(feats.cpu().numpy() if dtype == torch.float32 else feats.float().cpu().numpy(), keep.cpu().numpy(), nfeat.cpu().numpy(), cap)
    np.testing.assert_array_equal(base[0].float().cpu().numpy(), ref1)
    ref2, _ = orc.length_regulate(f64(feats), dur)
    np.testing.assert_array_equal(f64(base[1]), ref2)
    assert not any(torch.isnan(t).any() for t in base)
    for off_in, off_out in ((True, False), (False, True), (True, True)):
        same_bits(f"in {off_in} out {off_out}", run(off_in, off_out), base)


@covers("torch_dag_loss", "torch_dag_best_alignment", "torch_dag_logsoftmax_gather_inplace", "logsumexp_keepdim", "emission_mask",
        "restore_valid_links", "viterbi_decode_torch")
def test_torch_formulations_take_every_layout():
    """the torch formulations that ship beside the operators (the CPU path and the checkers of the HIP ops) have no C side; torch serves every
    layout itself.  On the device, every layout against the call on fresh tensors: integers exactly, floats to 1e-6 (a strided reduction may
    add in another order) — and the fresh call against the HIP operator it restates"""
    ops, d = OPS(), D()
    B, T, L, TR, Vn = 2, 6, 24, 5, 11
    match, links, ol, tl = make_dag_inputs(9, B, T, L, TR)
    rng = np.random.default_rng(9)
    logits = (rng.standard_normal((B, L, Vn)) * 2).astype(np.float32)
    feats = rng.standard_normal((B, L, 8)).astype(np.float32)
    idx = np.ascontiguousarray(np.broadcast_to(rng.integers(0, Vn, (B, 1, T)), (B, L, T)))
    path = ops.dag_best_alignment(cu(match), cu(links), cu(ol), cu(tl))
    args = dict(match=cu(match), links=cu(links), ol=cu(ol), tl=cu(tl), logits=cu(logits), idx=cu(idx), feats=cu(feats), path=path)

    def call(a):
        dense = d.restore_valid_links(a["links"])
        loss = ops.torch_dag_loss(a["match"], dense, a["ol"], a["tl"])
        best = ops.torch_dag_best_alignment(a["match"].detach(), dense, a["ol"], a["tl"])      # (it turns requires_grad on: on a detached alias of the same layout)
        _, m = ops.torch_dag_logsoftmax_gather_inplace(a["logits"], a["idx"])
        vd = d.viterbi_decode_torch(a["logits"], a["links"], a["feats"], a["ol"], 1, 1.0, 1.0, True)
        return (dense, loss, best, m, ops.logsumexp_keepdim(a["match"], 1), d.emission_mask(a["path"], T)) + tuple(vd)
    base = call(args)

    def judge(tag, out):
        for i, (g, w_) in enumerate(zip(out, base)):
            assert g.shape == w_.shape and g.dtype == w_.dtype, (tag, i)
            if g.dtype.is_floating_point:
                torch.testing.assert_close(g, w_, rtol=1e-6, atol=1e-6, equal_nan=True, msg=lambda m_: f"{tag} output {i}: {m_}")
            else:
                assert torch.equal(g, w_), (tag, i)
    sweep(args, tuple(args), call, judge)
    dense, loss, best, m = base[:4]
    hip_loss = ops.dag_loss(args["match"], args["links"], args["ol"], args["tl"])
    fin = torch.isfinite(hip_loss)
    assert torch.equal(torch.isfinite(loss), fin)
    torch.testing.assert_close(loss[fin], hip_loss[fin], rtol=1e-5, atol=1e-4)
    assert torch.equal(best[fin], path[fin])
    _, hip_m = ops.dag_logsoftmax_gather_inplace(args["logits"].clone(), args["idx"])
    torch.testing.assert_close(m, hip_m, rtol=2e-6, atol=2e-6)


# ================================================================================================ the table is complete

NOT_APPLICABLE = {
    # switches
    "set_glance_hip": "switch: exercised by test_glancing_ops to obtain the torch formulation",
    "set_split_gemm": "switch: no tensor argument",
    # pure-host helpers
    "dropout_threshold": "host arithmetic on a float",
    "dropout_keep_mask": "no tensor argument (seed, offset, p, shape)",
}


def _public_names():
    import inspect
    d = D()
    own = [n for n, o in vars(d).items() if not n.startswith("_") and (inspect.isfunction(o) or inspect.isclass(o)) and getattr(o, "__module__", None) == d.__name__]
    return sorted(set(own) | set(OPS().__all__) | {"HiFiGANHipRunner"})


def test_every_public_operator_has_a_row():
    """every public function and class that daspeech_amd.decode_ops defines (it keeps no __all__: the module's own definitions without a leading
    underscore are the list, a superset of its docstring's), custom_ops.__all__ and the vocoder runner: a row above, or one written reason"""
    names = _public_names()
    assert len(names) > 50
    missing = [n for n in names if n not in COVERED and n not in NOT_APPLICABLE]
    assert not missing, f"no row in tests/test_gpu_views.py and no reason in NOT_APPLICABLE: {missing}"
    both = [n for n in names if n in COVERED and n in NOT_APPLICABLE]
    assert not both, both
    stale = [n for n in list(COVERED) + list(NOT_APPLICABLE) if n not in names]
    assert not stale, f"names that are not public operators any more: {stale}"
    assert all(isinstance(r, str) and r and "\n" not in r for r in NOT_APPLICABLE.values())
