"""numpy float64 restatement of the expect strategy's posterior step (DASpeech/criterions/s2s_dag_fastspeech2_loss.py:259-262) and the
inputs the double-posterior tests share.

    s = alpha + beta;  m = max_j s;  lse = m + log(sum_j exp(s - m));  p = exp(s - lse), rows without a finite entry -> 0 (the NaN -> 0)
    out = p @ features;   backward w.r.t. the features: einsum('btl,btd->bld', p, grad_out)   (alpha / beta are detached)

`oracle.posterior_expect` is the fp32 statement of the same step; this one exists because a 1e-12 check needs a double reference."""
import numpy as np

from oracle import dag_oracle as orc
from tests.util_inputs import make_dag_inputs

# (seed, B, T, L, TR, D): ragged lengths (rows past T_b all -inf), an odd feature width that needs more than one column slab, D = 1, a
# banded graph, a dense window, L not a multiple of 4
CASES = [(31, 3, 9, 70, 16, 32), (32, 3, 21, 70, 16, 641), (33, 3, 21, 70, 16, 1), (34, 3, 40, 700, 32, 96), (35, 2, 25, 300, 299, 96),
         (36, 2, 12, 1030, 1029, 33)]
# |alpha + beta| reaches 1.26e3 here; reachable because (T - 1) * TR + 1 >= L
LARGE = (37, 2, 140, 4096, 32, 64)


def posterior_ref(alpha, beta, features=None, grad_out=None):
    """-> (p [B,T,L], lse [B,T] (-inf for dead rows), out [B,T,D] or None, grad_features [B,L,D] or None), all np.float64."""
    s = np.asarray(alpha, np.float64) + np.asarray(beta, np.float64)
    m = s.max(-1, keepdims=True)
    live = np.isfinite(m)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        e = np.exp(s - np.where(live, m, 0.0))
        lse = np.where(live, m + np.log(np.where(live, e.sum(-1, keepdims=True), 1.0)), -np.inf)
        p = np.where(live, np.exp(s - np.where(live, lse, 0.0)), 0.0)
    out = None if features is None else p @ np.asarray(features, np.float64)
    gf = None if grad_out is None else np.einsum("btl,btd->bld", p, np.asarray(grad_out, np.float64))
    return p, lse[..., 0], out, gf


def make_case(seed, B, T, L, TR, D):
    """-> dict(alpha, beta [B,T,L] float64 from the fp64 oracle DP, features [B,L,D], grad_out [B,T,D], out_len, tgt_len, match, links)."""
    match, links, ol, tl = make_dag_inputs(seed, B, T, L, TR)
    a = orc.dag_alpha(match, links, ol, tl, np.float64)
    b = orc.dag_beta(match, links, ol, tl, np.float64)
    rng = np.random.default_rng(7000 + seed)
    return dict(alpha=a, beta=b, features=rng.standard_normal((B, L, D)), grad_out=rng.standard_normal((B, T, D)), out_len=ol, tgt_len=tl,
                match=match, links=links)


def max_finite_abs(alpha, beta):
    s = alpha + beta
    return float(np.abs(s[np.isfinite(s)]).max())
