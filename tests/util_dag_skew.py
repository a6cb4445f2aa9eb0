"""Case table, inputs and float64 references for the fp32 DAG kernels (the eleven families selected in csrc/capi_dag.hip:17-88) on batches that
mix one full-size sample with tiny and mid-size ones — what a padded training batch looks like and what tests/util_inputs.make_dag_inputs
(L_b >= L - 4, T_b >= T - 4) never produces.  tests/test_dag_skew_ref.py checks all of this on the CPU (the geometry each case exists for, the
oracle's values outside the graph, a second float64 evaluation, the fp32 oracle's distance); tests/test_gpu_dag_skew.py holds the kernels to it.
Nothing here needs a GPU.

Reference: oracle.dag_oracle in np.float64 on the fp32 inputs (alpha, beta, loss = beta[b, 0, 0], both gradients); the alignment in np.float32
(adds and compares only: what tests/test_gpu_dag_ops.py::test_oracle_viterbi_bit_exact compares with).

Tolerances, the project's own: alpha / beta / loss rtol 3e-6, atol 2e-5 T (test_oracle_alpha_beta_loss); gradients rtol 50 * 2e-5 T, atol 1e-7
(test_oracle_gradients); paths equal."""
import functools
import zlib
from collections import namedtuple

import numpy as np

from oracle import dag_oracle as orc
from tests.util_inputs import make_dag_inputs


def table_tol(T):
    return (3e-6, 2e-5 * T)


def grad_tol(T):
    return (50 * 2e-5 * T, 1e-7)


# ------------------------------------------------------------------------------------------------------------ launch geometry
# A restatement of the launchers, by file:line (csrc/).  dag_strip.h:46-48: STRIP_RING = 8 match rows in the LDS ring, STRIP_CH = 4 rows of halo
# prefetch; every strip family iterates nrows = T_b rows (dag_dp_strip4g.hip:72, strip2g:48, strip1g:100, strip2:45, banded:105, maxstrip:49,
# maxstripw:96).  dag_strip.h:101-104: a strip is dead when the sample is invalid or j0 = s W >= L_b; :116-117: has_producer / has_consumer.
#
#   family      selected by (capi_dag.hip:50-88)                          pin (capi_dag.hip:24-37)   strip / block width W             halo
#   strip4g     TR <= 32, 16-byte rows (dag_dp_strip4g.hip:491)           5                          4 NT (:464): 512, or 1024 when    32 (:26)
#                                                                                                   ndir B ceil(L/1024) >= 200 (:494-495, :523)
#   strip2g     32 < TR <= 64 (dag_dp_strip2g.hip:362)                    8                          512 (:26)                         64 (:27)
#   strip1g     64 < TR <= 128 (dag_dp_strip1g.hip:357)                   8                          256 (:78)                         128 (:79)
#   strip2      TR <= 32, L % 4 == 0, dense 16-byte rows (strip2:423)     4 (forward and alignment)  2 NT = 384 (:394, :421)           32 (:47)
#   banded      TR <= 64, dense rows (dag_dp_banded.hip:260)              2 (forward and alignment)  512 (:27)                         32 / 64 (:346)
#   dense_mfma  TR > 32, L >= 128, dense rows (dag_dp_dense_mfma.hip:913) 9                          64-column blocks (:58)            -
#   generic     whatever the pin leaves (capi_dag.hip:35, :60, :87)       1                          -                                 -
#   maxstrip    TR <= 32, L <= 8192, 16-byte rows (maxstrip:550-554)      7                          CPL 256 (:267): 512, or 1024 when 32 (:28)
#                                                                                                   B ceil(L/1024) >= 200 (:558-559, :584)
#   maxstripw   32 < TR <= 128 (dag_dp_maxstripw.hip:273)                 7                          CPL 256, TRP = 128 / CPL (:82): CPL = 2 for TR <= 64, else 1 (:298)
#   dense_max   TR > 32, L >= 128, dense rows (dag_dp_dense_max.hip:450)  9                          64-column blocks (:44)            -
# (maxstripw is listed twice below, once per CPL.)  The dense kernels have no dead blocks: every block fills rows T_b .. T-1 itself
# (dag_dp_dense_mfma.hip:150) and beta runs mirrored from u0 = L - L_b (:135); strips() gives their 64-column blocks all the same, so that the
# length patterns sit on block edges.
STRIP_RING, STRIP_CH = 8, 4
Family = namedtuple("Family", "name kind pin W halo tr_lo tr_hi")
FAMILIES = {f.name: f for f in [
    Family("strip4g", "fwd", 5, 512, 32, 1, 32),
    Family("strip2g", "fwd", 8, 512, 64, 33, 64),
    Family("strip1g", "fwd", 8, 256, 128, 65, 128),
    Family("strip2", "both", 4, 384, 32, 1, 32),
    Family("banded", "both", 2, 512, 64, 1, 64),
    Family("dense_mfma", "fwd", 9, 64, 0, 33, 1 << 30),
    Family("generic", "both", 1, 0, 0, 1, 1 << 30),
    Family("maxstrip", "align", 7, 512, 32, 1, 32),
    Family("maxstripw2", "align", 7, 512, 64, 33, 64),
    Family("maxstripw1", "align", 7, 256, 128, 65, 128),
    Family("dense_max", "align", 9, 64, 0, 33, 1 << 30),
]}


def wide(family, B, L, ndir):
    """the predicates that pick the NT = 256 strip4g kernel (dag_dp_strip4g.hip:494) and the CPL = 4 maxstrip kernel (dag_dp_maxstrip.hip:558)"""
    if family == "strip4g":
        return ndir * B * -(-L // 1024) >= 200
    if family == "maxstrip":
        return B * -(-L // 1024) >= 200
    return False


def strips(family, B, L, ndir):
    """(NS, W) of the launch: strips or 64-column blocks per (sample, direction) and their width; the generic kernels have one of width L"""
    if family == "generic":
        return 1, L
    W = 1024 if wide(family, B, L, ndir) else FAMILIES[family].W
    return -(-L // W), W


def dead(family, case, b, ndir=2, order="fwd"):
    """(dead strips of sample b, its last live strip or -1): dag_strip.h:101-104"""
    NS, W = strips(family, case.B, case.L, ndir)
    Tb, Lb = lengths(case, order)[b]
    valid = 1 <= Tb <= case.T and 1 <= Lb <= case.L
    gone = [s for s in range(NS) if not valid or s * W >= Lb]
    return gone, NS - len(gone) - 1


# ------------------------------------------------------------------------------------------------------------ the case table
# W: the width the length patterns are cut for; edges: explicit L_b around the block edges instead (the dense cases).  fwd / align: the families
# run on the case, each through its pin.  bwd: the backward is run.  small: the CPU band DP runs with autograd.
Case = namedtuple("Case", "cid B T L TR W edges fwd align bwd small variants")
ALL = ("base", "holes", "ties")
BANDED32 = dict(fwd=("strip4g", "strip2", "banded", "generic"), align=("maxstrip", "strip2", "banded", "generic"))
BANDED64 = dict(fwd=("strip2g", "banded", "dense_mfma", "generic"), align=("maxstripw2", "banded", "dense_max", "generic"))
BANDED128 = dict(fwd=("strip1g", "dense_mfma", "generic"), align=("maxstripw1", "dense_max", "generic"))
DENSE = dict(fwd=("dense_mfma", "generic"), align=("dense_max", "generic"), edges=(63, 64, 65, 127, 128, 129))


def tmin(Lb, TR):
    """the smallest T_b that reaches the end of a graph of L_b vertices: (t - 1) TR >= L_b - 1"""
    return 1 if Lb <= 1 else -(-(Lb - 1) // TR) + 1


def _c(cid, B, L, TR, W, fwd, align, T=None, edges=None, bwd=True, small=True, variants=ALL):
    T = tmin(L, TR) if T is None else T
    assert (T - 1) * TR >= L - 1
    return Case(cid, B, T, L, TR, W, edges, tuple(fwd), tuple(align), bwd, small, tuple(variants))


CASES = [
    # ---- three strips of 512 (strip2: 384), windows <= 32: the smallest L with a third strip that keeps 16-byte rows
    _c("w32", 0, 1028, 32, 512, **BANDED32),
    _c("w7", 0, 1028, 7, 512, **BANDED32),
    _c("w32-offgrid", 0, 1030, 32, 512, fwd=("strip4g", "banded", "generic"), align=("maxstrip", "banded", "generic")),          # pitched rows
    _c("w32-strip2", 0, 772, 32, 384, fwd=("strip2",), align=("strip2",)),                                                       # strip2's own edges
    # ---- windows 33 .. 64
    _c("w64", 0, 1028, 64, 512, **BANDED64),
    _c("w33", 0, 1028, 33, 512, **BANDED64),
    _c("w64-offgrid", 0, 1030, 64, 512, fwd=("strip2g", "generic"), align=("maxstripw2", "generic")),
    # ---- windows 65 .. 128: three strips of 256
    _c("w128", 0, 516, 128, 256, **BANDED128),
    _c("w65", 0, 516, 65, 256, **BANDED128),
    _c("w128-offgrid", 0, 518, 128, 256, fwd=("strip1g", "generic"), align=("maxstripw1", "generic")),
    # ---- dense windows: four 64-column blocks; sixteen, the window shared by 16 workgroups per (sample, direction)
    _c("dense-200", 0, 200, 199, 64, **DENSE),
    _c("dense-1024", 0, 1024, 1023, 64, T=3, **DENSE),
    # ---- the wide kernels: 2 * 34 * 3 = 204 workgroups pick strip4g's NT = 256; maxstrip's rule has no factor 2 and needs 67 samples
    _c("wide", 34, 2052, 32, 1024, fwd=("strip4g",), align=("maxstrip",), small=False),
    _c("wide-max", 67, 2052, 32, 1024, fwd=("strip4g",), align=("maxstrip",), bwd=False, small=False, variants=("base", "ties")),
]


def pattern(T, L, TR, W, edges=None):
    """(T_b, L_b) per sample: the full sample, then the short ones (module docstring of tests/test_dag_skew_ref.py says what each is for)"""
    if edges is None:
        edges = (W - 1, W, W + 1) + ((2 * W,) if L > 2 * W else ())
    lens = [(T, L), (1, 1), (2, 2), (min(3, T), min(2 * TR + 1, L))]
    lens += [(tmin(e, TR), e) for e in edges]
    lens.append((2, W + 2) if TR < W + 1 else (1, W + 2))          # valid, the end out of reach: (T_b - 1) TR < L_b - 1
    lens.append((min(5, T), 5))
    return lens


def _lens(case):
    p = pattern(case.T, case.L, case.TR, case.W, case.edges)
    if case.B == 0:
        return p
    return [p[0]] + [p[1 + (b - 1) % (len(p) - 1)] for b in range(1, case.B)]


CASES = [c._replace(B=len(_lens(c))) for c in CASES]
BY_ID = {c.cid: c for c in CASES}
assert len(BY_ID) == len(CASES)
ORDERS = ("fwd", "rev")


def lengths(case, order="fwd"):
    """(T_b, L_b) per sample.  rev: the same samples in reverse order — tickets go b = rem % B (dag_strip.h:95), so the full sample then draws the
    last ticket of every position."""
    lens = _lens(case)
    return lens if order == "fwd" else lens[::-1]


def reachable(case, b, order="fwd"):
    Tb, Lb = lengths(case, order)[b]
    return Tb <= Lb and (Tb - 1) * case.TR >= Lb - 1 and (Tb > 1 or Lb == 1)


def ordered(x, order):
    return x if order == "fwd" else np.ascontiguousarray(x[::-1])


# ------------------------------------------------------------------------------------------------------------ inputs

def spine(Tb, Lb):
    """a path 0 -> L_b - 1 in T_b - 1 steps of 1 .. ceil((L_b-1)/(T_b-1)) vertices: what the holes variant keeps open"""
    if Tb == 1:
        return np.zeros(1, np.int64)
    return (np.arange(Tb, dtype=np.int64) * (Lb - 1)) // (Tb - 1)


Inputs = namedtuple("Inputs", "match links out_len tgt_len w")


@functools.lru_cache(maxsize=3)
def _inputs(cid, variant):
    case = BY_ID[cid]
    B, T, L, TR = case.B, case.T, case.L, case.TR
    m, k, _, _ = make_dag_inputs(zlib.crc32(cid.encode()) % 100000, B, T, L, TR, ragged=False)
    lens = lengths(case)
    tl = np.array([x[0] for x in lens], np.int64)
    ol = np.array([x[1] for x in lens], np.int64)
    # transitions past each sample's own graph do not exist: masked and re-normalised per vertex, as make_dag_inputs does for its lengths
    i = np.arange(L)[None, :, None]
    d = np.arange(TR)[None, None, :]
    ok = (i + d + 1) < ol[:, None, None]
    k64 = np.where(ok, k.astype(np.float64), -np.inf)
    mx = np.max(np.where(ok, k64, -1e30), axis=-1, keepdims=True)
    s = np.where(ok, np.exp(k64 - mx), 0.0).sum(-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.where(ok, k64 - mx - np.log(np.where(s > 0, s, 1.0)), -np.inf).astype(np.float32)
    if variant == "ties":
        m = (np.round(m * 2) / 2).astype(np.float32)
        k = np.where(np.isfinite(k), np.round(k * 2) / 2, k).astype(np.float32)
    elif variant == "holes":
        rng = np.random.default_rng(zlib.crc32((cid + "/holes").encode()))
        i2, d2 = np.arange(L)[:, None], np.arange(TR)[None, :]
        t2, j2 = np.arange(T)[:, None], np.arange(L)[None, :]
        for b in range(B):
            if not reachable(case, b):
                continue
            Tb, Lb = lens[b]
            sp = spine(Tb, Lb)
            free_k = (i2 + d2 + 1) < Lb
            free_k[sp[:-1], np.diff(sp) - 1] = False
            free_m = (t2 < Tb) & (j2 >= t2) & (j2 < Lb)
            free_m[np.arange(Tb), sp] = False
            for arr, free in ((k[b], free_k), (m[b], free_m)):
                hit = free & (rng.random(free.shape) < 0.03)
                if not hit.any() and free.any():
                    cand = np.argwhere(free)
                    hit[tuple(cand[len(cand) // 2])] = True
                arr[hit] = -np.inf
    else:
        assert variant == "base"
    out = Inputs(m, k, ol, tl, np.linspace(0.5, 1.5, B).astype(np.float32))
    for x in out:
        x.setflags(write=False)
    return out


def inputs(cid, variant="base", order="fwd"):
    """fp32 match [B,T,L] and links [B,L,TR], int64 lengths, the incoming gradient w [B].  holes: 3 % (at least one) of the transitions inside each
    reachable sample's graph and of its live match entries are -inf, the spine and the first vertex excepted.  ties: finite scores rounded to
    halves.  rev: the same samples, last first."""
    return Inputs(*(ordered(x, order) for x in _inputs(cid, variant)))


# ------------------------------------------------------------------------------------------------------------ references
Ref = namedtuple("Ref", "alpha beta loss gm gl path")


def _oracle(inp, dtype, grads):
    m, k, ol, tl = inp.match, inp.links, inp.out_len, inp.tgt_len
    a = orc.dag_alpha(m, k, ol, tl, dtype)
    bt = orc.dag_beta(m, k, ol, tl, dtype)
    loss = bt[:, 0, 0].copy()
    gm = gl = None
    if grads:
        gm, gl = orc.dag_grad((inp.w * np.isfinite(loss)).astype(dtype), a, bt, m, k, ol, tl, dtype)
    return a, bt, loss, gm, gl


@functools.lru_cache(maxsize=3)
def _reference(cid, variant):
    inp = _inputs(cid, variant)
    a, bt, loss, gm, gl = _oracle(inp, np.float64, BY_ID[cid].bwd)
    path = orc.dag_best_alignment(inp.match, inp.links, inp.out_len, inp.tgt_len, np.float32)
    for x in (a, bt, loss, gm, gl, path):
        if x is not None:
            x.setflags(write=False)
    return Ref(a, bt, loss, gm, gl, path)


def reference(cid, variant="base", order="fwd"):
    """the oracle's results (float64; the path from the fp32 max-DP); gm / gl None where the case runs no backward.  Read-only."""
    return Ref(*(None if x is None else ordered(x, order) for x in _reference(cid, variant)))


def figure(got, ref, tol):
    """The largest |got - ref| / (atol + rtol |ref|) over the finite reference entries: <= 1 is inside the tolerance.  inf when a NaN, a +inf or a
    -inf is out of place."""
    got = np.asarray(got, np.float64)
    if got.shape != ref.shape or np.isnan(got).any() or np.isposinf(got).any() or not np.array_equal(np.isneginf(got), np.isneginf(ref)):
        return np.inf
    f = np.isfinite(ref)
    if not f.any():
        return 0.0
    rtol, atol = tol
    return float((np.abs(got[f] - ref[f]) / (atol + rtol * np.abs(ref[f]))).max())


def tol_of(case, name):
    return grad_tol(case.T) if name in ("gm", "gl") else table_tol(case.T)


def outside(case, order="fwd"):
    """masks of what lies outside each sample's graph: (rows >= T_b or columns >= L_b of a [B,T,L] table, transitions of a [B,L,TR] tensor that
    leave from or arrive at a vertex >= L_b); an unreachable sample lies outside altogether as far as the gradients go (`dead_grad`)"""
    lens = lengths(case, order)
    tb = np.array([x[0] for x in lens])[:, None, None]
    lb = np.array([x[1] for x in lens])[:, None, None]
    t = np.arange(case.T)[None, :, None]
    j = np.arange(case.L)[None, None, :]
    i = np.arange(case.L)[None, :, None]
    d = np.arange(case.TR)[None, None, :]
    dead_grad = np.array([not reachable(case, b, order) for b in range(case.B)])
    return (t >= tb) | (j >= lb), (i + d + 1) >= lb, dead_grad


@functools.lru_cache(maxsize=None)
def yardstick(cid, variant="base"):
    """figure() of the fp32 oracle (the reference's own arithmetic in the kernels' precision, not the kernels) against the fp64 oracle, per
    tensor: a kernel tensor beyond its tolerance may be at most 4 x this far from the fp64 oracle (the project's 4 x rule, tests/util_4x_rule.py)"""
    case, inp, ref = BY_ID[cid], _inputs(cid, variant), _reference(cid, variant)
    got = dict(zip(("alpha", "beta", "loss", "gm", "gl"), _oracle(inp, np.float32, case.bwd)))
    return {n: figure(v, getattr(ref, n), tol_of(case, n)) for n, v in got.items() if v is not None}


# ------------------------------------------------------------------------------------------------------------ the second fp64 evaluation

def band_dp(cid, variant="base", grads=True):
    """custom_ops/dag_double.py's torch band DP on CPU float64 tensors (the fp32 inputs widened) -> dict of numpy arrays.  The gradients come
    from autograd through the alpha recurrence; NaN (autograd through an all -inf row) counts as zero, as in tests/test_dag_double.py."""
    import torch
    from daspeech_amd.custom_ops import dag_double as dd
    inp = _inputs(cid, variant)
    m, k = torch.from_numpy(inp.match.astype(np.float64)), torch.from_numpy(inp.links.astype(np.float64))
    ol, tl = torch.from_numpy(inp.out_len.copy()), torch.from_numpy(inp.tgt_len.copy())
    out = {}
    if grads:
        m.requires_grad_()
        k.requires_grad_()
    a = dd.alpha_table(m, k, ol, tl)
    out["alpha"] = a.detach().numpy()
    with torch.no_grad():
        out["beta"] = dd.beta_table(m.detach(), k.detach(), ol, tl).numpy()
    loss = dd._pick_loss(a, ol, tl)
    out["loss"] = loss.detach().numpy()
    if grads:
        w = torch.from_numpy(inp.w.astype(np.float64))
        gm, gk = torch.autograd.grad((loss.nan_to_num(neginf=0.0) * w).sum(), [m, k])
        out["gm"], out["gl"] = torch.nan_to_num(gm, nan=0.0).numpy(), torch.nan_to_num(gk, nan=0.0).numpy()
    return out
