"""tests/util_dag_double_regimes.py on the CPU: (a) every case of the table reaches the launch regime of csrc/dag_dp_f64.hip it names, and the
table as a whole reaches every regime; (b) the oracle alone, on every case and variant, satisfies what tests/test_gpu_dag_double_regimes.py
relies on — finite losses for valid samples, -inf for invalid ones, real ties, real -inf inside the graph; (c) the torch band DP of
custom_ops/dag_double.py — the second float64 evaluation, the GPU test's yardstick — meets the oracle on the small and mid cases at the
tolerances of tests/test_dag_double.py.  No kernel is launched.  Figures: `pytest -s`."""
import numpy as np
import pytest

from tests import util_dag_double_regimes as U


# ---------------------------------------------------------------- (a)

@pytest.mark.parametrize("cid", sorted(U.BY_ID))
def test_cases_reach_the_regimes_they_name(cid):
    case = U.BY_ID[cid]
    g = U.geometry(case.B, case.T, case.L, case.TR)._asdict()
    assert case.expect, "a case names the regime it exists for"
    for name, want in case.expect.items():
        assert g[name] == want, (cid, name, g[name], want)
    assert len(U.lengths(case)) == case.B
    assert U.lengths(case)[0] == (case.T, case.L) or case.lens is not None
    for b in range(case.B):
        assert U.reachable(case, b) or not U.is_valid(case, b), (cid, b, U.lengths(case)[b])
    if not case.ragged:
        assert all(x == (case.T, case.L) for x in U.lengths(case))
    assert case.B <= 2 or "pick_blocks" in case.expect or case.lens is not None


def test_the_table_covers_every_regime():
    geo = {c.cid: U.geometry(c.B, c.T, c.L, c.TR) for c in U.CASES}
    assert {1, 2, 3, 10} <= {g.passes for g in geo.values()}
    assert {False, True} == {g.optin for g in geo.values()} == {g.over64k for g in geo.values()} == {g.strides for g in geo.values()}
    assert {c.L for c in U.CASES} >= {1023, 1024, 1025, 2049, 3072, 3073, 4096, 4097, U.MAX_L}
    assert any(g.lds == 160 * 1024 and not g.refused for g in geo.values()) and not any(g.refused for g in geo.values())
    cap = U.BY_ID["cap-10240"]
    assert cap.B == 1 and U.lengths(cap) == [(cap.T, cap.L)]                      # the last LDS element of both rows is a live column
    assert U.geometry(*U.ABOVE_CAP[1:5]).refused and U.ABOVE_CAP.L == U.MAX_L + 1
    assert any(g.pick_blocks == 2 for g in geo.values())
    # idle slots and idle vertices of the link gradient's last block: none, either, both
    combos = {(g.d_idle, g.i_idle) for cid, g in geo.items() if cid.startswith("guard-")}
    assert combos == {(d, i) for d in (1, 0, 31) for i in (1, 0, 7)}
    assert {c.TR for c in U.CASES if c.cid.startswith("guard-")} == {31, 32, 33}
    dense = U.BY_ID["dense-1025"]
    assert dense.TR == dense.L - 1
    # every sample kind of the invalid case, beside a valid first and last sample
    inv = U.INVALID
    assert [U.is_valid(inv, b) for b in range(inv.B)] == [True, False, False, False, False, True]
    assert [U.lengths(inv)[b] for b in range(1, 5)] == [(0, inv.L), (inv.T + 1, inv.L), (inv.T, 0), (inv.T, inv.L + 1)]


# ---------------------------------------------------------------- (b)

@pytest.mark.parametrize("cid,variant", U.PARAMS + [("invalid", "base"), ("above-cap-10241", "base")],
                         ids=U.PARAM_IDS + ["invalid-base", "above-cap-10241-base"])
def test_the_oracle_satisfies_what_the_gpu_test_relies_on(cid, variant):
    case = U.BY_ID[cid]
    inp, ref = U.inputs(cid, variant), U.reference(cid, variant)
    assert inp.match.dtype == inp.links.dtype == np.float64 and not np.isnan(inp.match).any() and not np.isnan(inp.links).any()
    for b in range(case.B):
        if ref.valid[b]:
            Tb, Lb = U.lengths(case)[b]
            assert np.isfinite(ref.loss[b]), (cid, variant, b)
            assert ref.loss[b] == ref.beta[b, 0, 0] and np.isfinite(ref.alpha[b, Tb - 1, Lb - 1])
            assert ref.path[b, 0] == 0 and ref.path[b, Lb - 1] == Tb - 1 and (ref.path[b] >= 0).sum() == Tb
        else:
            assert np.isneginf(ref.loss[b]) and np.isneginf(ref.alpha[b]).all() and np.isneginf(ref.beta[b]).all()
            assert not ref.gm[b].any() and not ref.gl[b].any() and (ref.path[b] == -1).all()
    assert not np.isnan(ref.gm).any() and not np.isnan(ref.gl).any() and np.isfinite(ref.gm).all() and np.isfinite(ref.gl).all()
    # alpha and beta tell the same story: alpha[T_b-1, L_b-1] is beta[0, 0] to the tolerance of the tables
    v = np.flatnonzero(ref.valid)
    a_end = ref.alpha[v, inp.tgt_len[v] - 1, inp.out_len[v] - 1]
    np.testing.assert_allclose(a_end, ref.loss[v], rtol=1e-12, atol=1e-11)
    if variant == "ties":
        n = U.tie_cells(cid)
        print(f"{cid}: cells with two or more equal best predecessors, per sample: {n}")
        assert all(x > 0 for x in n), (cid, n)
    if variant == "holes":
        n = U.hole_counts(cid)
        print(f"{cid}: (-inf transitions inside the graph, -inf live match entries) per sample: {n}")
        assert all(k > 0 and m > 0 for k, m in n), (cid, n)


# ---------------------------------------------------------------- (c)

@pytest.mark.parametrize("cid,variant", U.PARAMS + [("above-cap-10241", "base")], ids=U.PARAM_IDS + ["above-cap-10241-base"])
def test_the_band_dp_meets_the_oracle(cid, variant):
    """gradients where autograd's T saved [B, L, TR] tensors stay small (every case but the two marked heavy: the cap and its neighbour, which
    the GPU test runs through this band DP on the device)"""
    d = U.distances(cid, variant, grads=not U.BY_ID[cid].heavy)
    print(f"{cid}-{variant}: band DP vs oracle, fraction of the tolerance used: " + "  ".join(f"{k} {v:.2e}" for k, v in d.items() if k != "path_equal"))
    assert d.pop("path_equal")
    assert all(v <= 1.0 for v in d.values()), d
