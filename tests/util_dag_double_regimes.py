"""Case table, inputs and float64 references for the double-precision DAG kernels (csrc/dag_dp_f64.hip behind custom_ops/dag_double.py) at every
launch regime of dsp_dag_loss_fwd_f64 / dsp_dag_loss_bwd_f64 / dsp_dag_best_alignment_f64.  tests/test_dag_double_regimes_ref.py checks all of
this on the CPU (each case against the geometry below, the planted -inf and ties, the torch band DP against the oracle);
tests/test_gpu_dag_double_regimes.py holds the kernels to it.  Nothing here needs a GPU.

Reference: oracle.dag_oracle in np.float64 (alpha, beta, loss = beta[b, 0, 0], both gradients, the alignment).  The oracle, like the
reference's kernels, does not define samples with invalid lengths (T_b or L_b of 0, or beyond T / L: it would index outside its tables), so
the expected values of such a sample are the contract of the kernels themselves (dag_dp_f64.hip:36-39, :97, :106-110, :127;
dag_dp_generic.hip:186): alpha and beta all -inf, loss -inf, both gradients zero, path all -1.  The valid samples next to it are the
oracle's, run on those samples alone.

Tolerances (what tests/test_dag_double.py holds this path to): tables and loss rtol 1e-12 / atol 1e-11, gradients rtol 1e-9 / atol 1e-12."""
import functools
import zlib
from collections import namedtuple

import numpy as np

from oracle import dag_oracle as orc
from tests.util_inputs import make_dag_inputs

TABLE_TOL = (1e-12, 1e-11)          # (rtol, atol) of alpha, beta and the loss
GRAD_TOL = (1e-9, 1e-12)            # ... of grad_match and grad_links
MAX_L = 10240

# ------------------------------------------------------------------------------------------------------------ launch geometry
# A restatement of dag_dp_f64.hip, by line of that file:
#   :19        constexpr int D64_THREADS = 1024, the workgroup of dag64_logsum_kernel / dag64_maxalpha_kernel (launches :198, :239)
#   :38 :41 :45 :65 :70 :152 :154 :158
#              for (int j = tid; j < L; j += D64_THREADS): ceil(L / 1024) passes over a row
#   :28-29 :142-143   prev = smem, cur = prev + L: two rows of doubles
#   :179       *lds = 2 * L * sizeof(double)
#   :180       if (*lds > 160 * 1024) -> DSP_EINVAL "... (max 10240)"
#   :197 :238  if (lds > 48 * 1024) set_max_dynamic_lds(kernel, lds)
#   :198       grid (B, (alpha && beta) ? 2 : 1)
#   :201       dag64_pick_loss_kernel: grid (B + 63) / 64, 64 threads
#   :217-218   gx = (T * L + 255) / 256, capped at 1024; dag64_grad_match_kernel grid (gx, B), 256 threads
#   :109       for (i = blockIdx.x * 256 + threadIdx.x; i < TL; i += gridDim.x * 256): a second trip when T * L > gx * 256
#   :222       dag64_grad_links_kernel: grid ((TR + 31) / 32, (L + 7) / 8, B), 256 threads = 8 vertices x 32 slots
#   :119-121   d = blockIdx.x * 32 + (tid & 31), i = blockIdx.y * 8 + (tid >> 5); if (i >= L || d >= TR) return
THREADS = 1024
Geometry = namedtuple("Geometry", "passes lds optin refused over64k link_grid d_idle i_idle match_blocks strides pick_blocks")


def geometry(B, T, L, TR):
    lds = 16 * L
    tl = T * L
    gx = min(1024, -(-tl // 256))
    lx, ly = -(-TR // 32), -(-L // 8)
    return Geometry(passes=-(-L // THREADS), lds=lds, optin=lds > 48 * 1024, refused=lds > 160 * 1024, over64k=lds > 64 * 1024,
                    link_grid=(lx, ly, B), d_idle=lx * 32 - TR, i_idle=ly * 8 - L, match_blocks=gx, strides=tl > gx * 256,
                    pick_blocks=-(-B // 64))


# ------------------------------------------------------------------------------------------------------------ the case table
# expect: the fields of geometry() the case exists for.  ragged: samples after the first are shorter (lengths()).  lens: explicit (T_b, L_b)
# per sample instead.  heavy: the CPU band DP runs without autograd on the case (with it, T x [B, L, TR] doubles and their temporaries stay alive).
Case = namedtuple("Case", "cid B T L TR ragged lens variants heavy expect")
ALL = ("base", "holes", "ties")
NO_TIES = ("base", "holes")         # graphs of a few vertices: too few cells for every sample to hold an exact tie


def _c(cid, B, T, L, TR, ragged=True, lens=None, variants=ALL, heavy=False, **expect):
    return Case(cid, B, T, L, TR, ragged, lens, tuple(variants), heavy, expect)


CASES = [
    # ---- passes of the 1024-thread loops: 1 (full), 1 (exactly), 2 (one column), 3 (one column).  T: the smallest with (T-1) TR >= L-1
    _c("pass-1023", 2, 17, 1023, 64, passes=1),
    _c("pass-1024", 2, 17, 1024, 64, passes=1),
    _c("pass-1025", 2, 17, 1025, 64, passes=2),
    _c("pass-2049", 2, 33, 2049, 64, passes=3),
    # ---- 48 KiB: the last launch without the attribute, the first with it
    _c("lds-3072", 2, 25, 3072, 128, passes=3, lds=48 * 1024, optin=False),
    _c("lds-3073", 2, 25, 3073, 128, passes=4, optin=True, over64k=False),
    # ---- 64 KiB
    _c("lds-4096", 1, 33, 4096, 128, lds=64 * 1024, optin=True, over64k=False),
    _c("lds-4097", 1, 33, 4097, 128, optin=True, over64k=True, passes=5),
    # ---- the cap: 160 KiB of dynamic LDS, every element of both rows in use (L_b = L)
    _c("cap-10240", 1, 11, 10240, 1024, ragged=False, heavy=True, passes=10, lds=160 * 1024, optin=True, refused=False),
    # ---- grad_match: T L = 276 570 > 1024 x 256 elements
    _c("stride", 1, 90, 3073, 64, match_blocks=1024, strides=True),
    # ---- loss pick: a second block of 64
    _c("pick-65", 65, 3, 6, 4, variants=NO_TIES, pick_blocks=2, strides=False),
    # ---- dense window at two passes
    _c("dense-1025", 1, 3, 1025, 1024, passes=2),
    # ---- rows past T_b, columns past L_b (the C ABI tests poison them)
    _c("abi", 3, 7, 41, 8, lens=((7, 41), (6, 38), (5, 33)), passes=1),
]
# ---- grad_links: idle slots d >= TR (TR = 31, 33) and idle vertices i >= L (L = 7, 9, 41) of the last block, alone and together
for _tr in (31, 32, 33):
    for _l in (7, 8, 9, 41):
        CASES.append(_c(f"guard-TR{_tr}-L{_l}", 2, 5 if _l == 41 else 4, _l, _tr, variants=ALL if _l == 41 else NO_TIES, link_grid=(-(-_tr // 32), -(-_l // 8), 2),
                        d_idle=-(-_tr // 32) * 32 - _tr, i_idle=-(-_l // 8) * 8 - _l))
# ---- invalid lengths beside valid samples (the first and the last)
INVALID = _c("invalid", 6, 6, 41, 8, lens=((6, 41), (0, 41), (7, 41), (6, 0), (6, 42), (6, 39)), variants=("base",), passes=1)
# ---- one vertex past the cap: custom_ops/dag_double.py:157-158 (_native) sends it to the torch band DP; the C entry points refuse it
ABOVE_CAP = _c("above-cap-10241", 1, 162, 10241, 64, ragged=False, variants=("base",), heavy=True, refused=True)
BY_ID = {c.cid: c for c in CASES + [INVALID, ABOVE_CAP]}
assert len(BY_ID) == len(CASES) + 2
PARAMS = [(c.cid, v) for c in CASES for v in c.variants]
PARAM_IDS = [f"{cid}-{v}" for cid, v in PARAMS]


def lengths(case):
    """(T_b, L_b) per sample.  Sample 0 spans the whole tensor; with `ragged` the others lose b % 4 vertices and, where the end stays
    reachable ((T_b - 1) TR >= L_b - 1), b % 2 target positions."""
    if case.lens is not None:
        return [tuple(x) for x in case.lens]
    out = []
    for b in range(case.B):
        Lb, Tb = case.L, case.T
        if case.ragged:
            Lb = max(2, case.L - b % 4)
            Tb = min(case.T - b % 2, Lb)
            if Tb < 2 or (Tb - 1) * case.TR < Lb - 1:
                Tb = min(case.T, Lb)
        out.append((Tb, Lb))
    return out


def is_valid(case, b):
    Tb, Lb = lengths(case)[b]
    return 1 <= Tb <= case.T and 1 <= Lb <= case.L


def reachable(case, b):
    Tb, Lb = lengths(case)[b]
    return is_valid(case, b) and Tb <= Lb and (Tb - 1) * case.TR >= Lb - 1 and (Tb > 1 or Lb == 1)


# ------------------------------------------------------------------------------------------------------------ inputs

def spine(Tb, Lb):
    """A path 0 -> L_b - 1 in T_b - 1 steps of 1 .. ceil((L_b-1)/(T_b-1)) vertices: what the holes variant keeps open."""
    if Tb == 1:
        return np.zeros(1, np.int64)
    return (np.arange(Tb, dtype=np.int64) * (Lb - 1)) // (Tb - 1)


Inputs = namedtuple("Inputs", "match links out_len tgt_len w")


@functools.lru_cache(maxsize=4)
def inputs(cid, variant="base"):
    """float64 match [B,T,L], links [B,L,TR] (tests/util_inputs.make_dag_inputs, widened), int64 lengths, the incoming gradient w [B].
    holes: 3 % (at least one) of the transitions inside each valid sample's graph and of its live match entries are -inf, the spine and the
    first vertex excepted.  ties: finite scores rounded to halves."""
    case = BY_ID[cid]
    B, T, L, TR = case.B, case.T, case.L, case.TR
    m, k, _, _ = make_dag_inputs(zlib.crc32(cid.encode()) % 100000, B, T, L, TR, ragged=False)
    m, k = m.astype(np.float64), k.astype(np.float64)
    lens = lengths(case)
    tl = np.array([x[0] for x in lens], np.int64)
    ol = np.array([x[1] for x in lens], np.int64)
    if variant == "ties":
        m = np.round(m * 2) / 2
        k = np.where(np.isfinite(k), np.round(k * 2) / 2, k)
    elif variant == "holes":
        rng = np.random.default_rng(zlib.crc32((cid + "/holes").encode()))
        i = np.arange(L)[:, None]
        d = np.arange(TR)[None, :]
        t = np.arange(T)[:, None]
        j = np.arange(L)[None, :]
        for b in range(B):
            if not is_valid(case, b):
                continue
            Tb, Lb = lens[b]
            sp = spine(Tb, Lb)
            free_k = (i + d + 1) < Lb
            free_k[sp[:-1], np.diff(sp) - 1] = False
            free_m = (t < Tb) & (j >= t) & (j < Lb)
            free_m[np.arange(Tb), sp] = False
            for arr, free in ((k[b], free_k), (m[b], free_m)):
                hit = free & (rng.random(free.shape) < 0.03)
                if not hit.any() and free.any():
                    cand = np.argwhere(free)
                    hit[tuple(cand[len(cand) // 2])] = True
                arr[hit] = -np.inf
    else:
        assert variant == "base"
    return Inputs(m, k, ol, tl, np.linspace(0.5, 1.5, B))


def hole_counts(cid):
    """per valid sample: (-inf transitions with both ends inside the graph, -inf match entries inside {t < T_b, t <= j < L_b})."""
    case = BY_ID[cid]
    inp = inputs(cid, "holes")
    i = np.arange(case.L)[:, None]
    d = np.arange(case.TR)[None, :]
    t = np.arange(case.T)[:, None]
    j = np.arange(case.L)[None, :]
    out = []
    for b in range(case.B):
        Tb, Lb = lengths(case)[b]
        out.append((int((np.isneginf(inp.links[b]) & ((i + d + 1) < Lb)).sum()), int((np.isneginf(inp.match[b]) & (t < Tb) & (j >= t) & (j < Lb)).sum())))
    return out


def tie_cells(cid, variant="ties", max_rows=4):
    """per sample: the cells (t, j) of the first `max_rows` DP rows whose best predecessor score is finite and attained by two predecessors or more
    (the max-DP of the oracle; all rows: max_rows=None)."""
    case = BY_ID[cid]
    inp = inputs(cid, variant)
    _, A, _ = orc.dag_best_alignment(inp.match, inp.links, inp.out_len, inp.tgt_len, np.float64, want_internals=True)
    L, TR = case.L, case.TR
    pred = np.arange(L)[:, None] - np.arange(TR)[None, :] - 1
    ok = pred >= 0
    predc = np.maximum(pred, 0)
    dd = np.broadcast_to(np.arange(TR)[None, :], (L, TR))
    out = []
    for b in range(case.B):
        Tb, Lb = lengths(case)[b]
        lt = np.where(ok, inp.links[b][predc, dd], -np.inf)
        n = 0
        for t in range(1, Tb if max_rows is None else min(Tb, 1 + max_rows)):
            cand = A[b, t - 1][predc] + lt
            mx = cand.max(axis=1)
            many = ((cand == mx[:, None]).sum(axis=1) >= 2) & np.isfinite(mx)
            n += int(many[t:Lb].sum())
        out.append(n)
    return out


# ------------------------------------------------------------------------------------------------------------ references
Ref = namedtuple("Ref", "alpha beta loss gm gl path valid")


@functools.lru_cache(maxsize=4)
def reference(cid, variant="base"):
    """The oracle's float64 results; samples with invalid lengths by the kernels' contract (see the module docstring).  Read-only."""
    case = BY_ID[cid]
    inp = inputs(cid, variant)
    B, T, L, TR = case.B, case.T, case.L, case.TR
    valid = np.array([is_valid(case, b) for b in range(B)])
    v = np.flatnonzero(valid)
    m, k, ol, tl = inp.match[v], inp.links[v], inp.out_len[v], inp.tgt_len[v]
    alpha = np.full((B, T, L), -np.inf)
    beta = np.full((B, T, L), -np.inf)
    gm = np.zeros((B, T, L))
    gl = np.zeros((B, L, TR))
    path = np.full((B, L), -1, np.int64)
    a = orc.dag_alpha(m, k, ol, tl, np.float64)
    bt = orc.dag_beta(m, k, ol, tl, np.float64)
    alpha[v], beta[v] = a, bt
    fin = np.isfinite(bt[:, 0, 0])
    gm[v], gl[v] = orc.dag_grad(inp.w[v] * fin, a, bt, m, k, ol, tl, np.float64)
    path[v] = orc.dag_best_alignment(m, k, ol, tl, np.float64)
    ref = Ref(alpha, beta, beta[:, 0, 0].copy(), gm, gl, path, valid)
    for x in ref:
        x.setflags(write=False)
    return ref


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


# ------------------------------------------------------------------------------------------------------------ the second fp64 evaluation

def band_dp(cid, variant="base", grads=True):
    """custom_ops/dag_double.py's torch band DP on CPU tensors -> dict(alpha, beta, loss, [gm, gl,] path) of numpy arrays.  The gradients come
    from autograd through the alpha recurrence; NaN in grad_links (autograd through an all -inf row) counts as zero, as in
    tests/test_dag_double.py."""
    import torch
    from daspeech_amd.custom_ops import dag_double as dd
    inp = inputs(cid, variant)
    m, k = torch.from_numpy(inp.match.copy()), torch.from_numpy(inp.links.copy())
    ol, tl = torch.from_numpy(inp.out_len.copy()), torch.from_numpy(inp.tgt_len.copy())
    out = {}
    if grads:
        m.requires_grad_()
        k.requires_grad_()
    a = dd.alpha_table(m, k, ol, tl)
    out["alpha"] = a.detach().numpy()
    with torch.no_grad():
        out["beta"] = dd.beta_table(m, k, ol, tl).numpy()
    loss = dd._pick_loss(a, ol, tl)
    out["loss"] = loss.detach().numpy()
    if grads:
        gm, gk = torch.autograd.grad((loss.nan_to_num(neginf=0.0) * torch.from_numpy(inp.w.copy())).sum(), [m, k])
        out["gm"], out["gl"] = torch.nan_to_num(gm, nan=0.0).numpy(), torch.nan_to_num(gk, nan=0.0).numpy()
    out["path"] = dd.dag_best_alignment(m.detach(), k.detach(), ol, tl).numpy()
    return out


def distances(cid, variant="base", grads=True):
    """figure() of the band DP against the oracle, per tensor: the yardstick of tests/test_gpu_dag_double_regimes.py."""
    ref, got = reference(cid, variant), band_dp(cid, variant, grads)
    d = {n: figure(got[n], getattr(ref, n), TABLE_TOL) for n in ("alpha", "beta", "loss")}
    if grads:
        d.update({n: figure(got[n], getattr(ref, n), GRAD_TOL) for n in ("gm", "gl")})
    d["path_equal"] = bool(np.array_equal(got["path"], ref.path))
    return d
