"""tests/util_dag_skew.py on the CPU: (a) every case has the geometry it exists for — dead strips, a live strip whose right neighbour is dead
(has_consumer false in the middle of the row of strips, dag_strip.h:117), a beta hand-off that does not start at strip NS - 1 (:116), target
lengths below the loader ring, the halo prefetch and the backward's row quarters, the wide predicates; (b) the oracle alone defines everything
tests/test_gpu_dag_skew.py compares with: -inf / zero / -1 outside (T_b, L_b), finite ends for reachable samples, -inf loss for the unreachable
one, no NaN; (c) the torch band DP of custom_ops/dag_double.py, a second float64 evaluation, agrees with the oracle on the small cases at the
double table's tolerances; (d) the fp32 oracle's distance from the fp64 oracle, the GPU test's yardstick, is recorded.  No kernel is launched.
Figures: `pytest -s`.

What each sample of a case is for (util_dag_skew.pattern): (T, L) the only sample whose strips are all live; (1, 1), (2, 2), (3, 2 TR + 1) target
lengths under STRIP_CH = 4, STRIP_RING = 8 and under the four row quarters of the backward (dag_grad.hip:228-229), one to three live columns
or one full window in strip 0; (t, W - 1), (t, W), (t, W + 1) the last live column on either side of the first strip edge (t: the fewest rows that
reach it); (t, 2 W) two live strips exactly; a valid sample whose end is out of reach (live strips that hand on -inf only); T_b = L_b = 5."""
import numpy as np
import pytest

from tests import util_dag_skew as U

IDS = [c.cid for c in U.CASES]
STRIPPED = [(c.cid, f) for c in U.CASES for f in dict.fromkeys(c.fwd + c.align) if U.FAMILIES[f].halo]
PARAMS = [(c.cid, v) for c in U.CASES for v in c.variants]


# ---------------------------------------------------------------- (a)

@pytest.mark.parametrize("cid", IDS)
def test_the_length_pattern(cid):
    case = U.BY_ID[cid]
    lens = U.lengths(case)
    assert len(lens) == case.B and lens[0] == (case.T, case.L) and U.lengths(case, "rev") == lens[::-1]
    assert all(1 <= Tb <= case.T and 1 <= Lb <= case.L and Tb <= Lb for Tb, Lb in lens)                   # every sample valid
    if case.cid != "dense-1024":                                                                          # (T = 3 there: the shared-window hand-off)
        assert (case.T - 1) * case.TR >= case.L - 1 > (case.T - 2) * case.TR                              # the smallest T that reaches the end
    unreachable = [b for b in range(case.B) if not U.reachable(case, b)]
    assert unreachable and len({lens[b] for b in unreachable}) == 1
    Tb, Lb = lens[unreachable[0]]
    assert (Tb - 1) * case.TR < Lb - 1 and Lb > case.W
    tbs = {Tb for Tb, _ in lens}
    assert {1, 2} <= tbs and (3 in tbs or case.T < 3)
    assert any(Tb < U.STRIP_CH for Tb in tbs) and any(Tb < U.STRIP_RING for Tb in tbs) and any(Tb - 1 < 4 for Tb in tbs)
    lbs = {Lb for _, Lb in lens}
    want = set(case.edges) if case.edges else {case.W - 1, case.W, case.W + 1, 2 * case.W}
    assert want <= lbs and {1, 2, 5, min(2 * case.TR + 1, case.L)} <= lbs
    for b, (Tb, Lb) in enumerate(lens):
        if Lb in want:
            assert U.reachable(case, b) and (Tb == 1 or (Tb - 2) * case.TR < Lb - 1), (b, Tb, Lb)             # t is the smallest
    offgrid = cid.endswith("offgrid")
    assert (case.L % 4 != 0) == offgrid
    for f in case.fwd + case.align:
        fam = U.FAMILIES[f]
        assert fam.tr_lo <= case.TR <= fam.tr_hi, f
        assert f != "strip2" or case.L % 4 == 0
        assert not f.startswith("dense") or case.L >= 128
        assert (f in case.fwd and fam.kind in ("fwd", "both")) or (f in case.align and fam.kind in ("align", "both"))


@pytest.mark.parametrize("cid,family", STRIPPED, ids=[f"{c}-{f}" for c, f in STRIPPED])
def test_dead_strips_and_where_the_hand_off_ends(cid, family):
    case = U.BY_ID[cid]
    ndirs = (2, 1) if U.FAMILIES[family].kind != "align" else (1,)
    for ndir in ndirs:
        NS, W = U.strips(family, case.B, case.L, ndir)
        assert NS >= 3 and (NS - 1) * W < case.L, (NS, W)
        for order in U.ORDERS:
            full = 0 if order == "fwd" else case.B - 1
            info = [U.dead(family, case, b, ndir, order) for b in range(case.B)]
            assert info[full] == ([], NS - 1)
            for b, (gone, last) in enumerate(info):
                Lb = U.lengths(case, order)[b][1]
                assert gone == list(range(last + 1, NS)) and last == (Lb - 1) // W                           # live strips first, then dead ones
            assert sum(1 for gone, _ in info if gone) >= case.B - 4                                        # nearly every sample has dead strips
            assert any(gone and last >= 0 for gone, last in info)                                          # a live strip with a dead right neighbour
            assert any(0 < last < NS - 1 for _, last in info) or W != case.W                               # ... in the middle of the row, after a hand-off
            assert any(last != NS - 1 for _, last in info)                                                 # beta's first live strip is not NS - 1
            assert any(len(gone) == NS - 1 for gone, _ in info) and any(len(gone) == 1 for gone, _ in info) or W != case.W
    print(f"{cid} {family}: NS {NS} W {W}, dead strips per sample {[len(g) for g, _ in info]}")


def test_the_wide_predicates():
    w, wm, n = U.BY_ID["wide"], U.BY_ID["wide-max"], U.BY_ID["w32"]
    assert (w.B, w.T, w.L, w.TR) == (34, 66, 2052, 32) and 2 * w.B * 3 == 204
    assert U.wide("strip4g", w.B, w.L, 2) and U.strips("strip4g", w.B, w.L, 2) == (3, 1024)
    assert not U.wide("strip4g", w.B, w.L, 1) and U.strips("strip4g", w.B, w.L, 1) == (5, 512)             # one direction: the NT = 128 kernel, five strips
    assert not U.wide("maxstrip", w.B, w.L, 1) and U.strips("maxstrip", w.B, w.L, 1) == (5, 512)
    assert U.wide("maxstrip", wm.B, wm.L, 1) and U.strips("maxstrip", wm.B, wm.L, 1) == (3, 1024) and wm.B * 3 == 201
    assert not U.wide("maxstrip", wm.B - 1, wm.L, 1)
    assert U.wide("strip4g", wm.B, wm.L, 1) and U.wide("strip4g", wm.B, wm.L, 2)
    for c in U.CASES:
        if not c.cid.startswith("wide"):
            assert not U.wide("strip4g", c.B, c.L, 2) and not U.wide("maxstrip", c.B, c.L, 1)
    assert U.strips("strip4g", n.B, n.L, 2) == (3, 512) and U.strips("strip2", n.B, n.L, 2) == (3, 384)
    assert U.strips("strip1g", 10, 516, 2) == (3, 256) and U.strips("maxstripw1", 10, 516, 1) == (3, 256) and U.strips("maxstripw2", 10, 1028, 1) == (3, 512)
    assert U.strips("dense_mfma", 12, 200, 2) == (4, 64) and U.strips("dense_max", 12, 1024, 1) == (16, 64) and U.strips("generic", 3, 77, 2) == (1, 77)
    # sample 0 is full, samples 1 .. cycle through the short patterns
    lens = U.lengths(w)
    short = U.pattern(w.T, w.L, w.TR, w.W)[1:]
    assert lens[0] == (w.T, w.L) and lens[1:] == [short[(b - 1) % len(short)] for b in range(1, w.B)] and len(short) == 9


def test_every_family_and_pin_is_in_the_table():
    assert {f for c in U.CASES for f in c.fwd} == {n for n, f in U.FAMILIES.items() if f.kind in ("fwd", "both")}
    assert {f for c in U.CASES for f in c.align} == {n for n, f in U.FAMILIES.items() if f.kind in ("align", "both")}
    assert {f.pin for f in U.FAMILIES.values()} == {1, 2, 4, 5, 7, 8, 9}
    for fam in ("strip4g", "strip2g", "strip1g", "maxstrip", "maxstripw2", "maxstripw1"):                  # the families that serve pitched rows
        assert any(c.L % 4 and fam in c.fwd + c.align for c in U.CASES), fam


# ---------------------------------------------------------------- (b)

@pytest.mark.parametrize("cid,variant", PARAMS, ids=[f"{c}-{v}" for c, v in PARAMS])
def test_the_oracle_defines_everything_outside_the_graph(cid, variant):
    case = U.BY_ID[cid]
    inp, ref = U.inputs(cid, variant), U.reference(cid, variant)
    assert inp.match.dtype == inp.links.dtype == np.float32 and not np.isnan(inp.match).any() and not np.isnan(inp.links).any()
    out_tab, out_link, dead_grad = U.outside(case)
    assert np.isneginf(inp.links[out_link]).all()
    assert np.isneginf(ref.alpha[out_tab]).all() and np.isneginf(ref.beta[out_tab]).all()
    assert not np.isnan(ref.alpha).any() and not np.isnan(ref.beta).any() and not np.isposinf(ref.alpha).any() and not np.isposinf(ref.beta).any()
    if case.bwd:
        assert np.isfinite(ref.gm).all() and np.isfinite(ref.gl).all()
        assert not ref.gm[out_tab].any() and not ref.gl[out_link].any() and not ref.gm[dead_grad].any() and not ref.gl[dead_grad].any()
    j = np.arange(case.L)
    for b, (Tb, Lb) in enumerate(U.lengths(case)):
        assert (ref.path[b, Lb:] == -1).all()
        if U.reachable(case, b):
            assert np.isfinite(ref.loss[b]) and np.isfinite(ref.alpha[b, Tb - 1, Lb - 1]) and np.isfinite(ref.beta[b, 0, 0])
            assert abs(ref.alpha[b, Tb - 1, Lb - 1] - ref.loss[b]) <= 1e-9 * max(1.0, abs(ref.loss[b]))
            assert ref.path[b, 0] == 0 and ref.path[b, Lb - 1] == Tb - 1 and (ref.path[b] >= 0).sum() == Tb
            if case.bwd:
                assert ref.gm[b].any() and (Tb == 1 or ref.gl[b].any())
        else:
            assert np.isneginf(ref.loss[b]) and np.isneginf(ref.alpha[b, Tb - 1, Lb - 1])
    if variant == "holes":
        inside_k = ~out_link & np.isneginf(inp.links)
        inside_m = ~out_tab & np.isneginf(inp.match)
        n = [(int(inside_k[b].sum()), int(inside_m[b].sum())) for b in range(case.B)]
        print(f"{cid}: (-inf transitions inside the graph, -inf match entries inside (T_b, L_b)) per sample: {n[:12]}")
        assert all(k > 0 and m > 0 for b, (k, m) in enumerate(n) if U.reachable(case, b) and U.lengths(case)[b][1] > 5)
    if variant == "ties":
        assert np.array_equal(inp.match * 2, np.round(inp.match * 2))
    # the reversed batch is the same samples, last first
    rinp, rref = U.inputs(cid, variant, "rev"), U.reference(cid, variant, "rev")
    assert np.array_equal(rinp.out_len, inp.out_len[::-1]) and np.array_equal(rref.loss, ref.loss[::-1]) and np.array_equal(rref.path[0], ref.path[-1])


# ---------------------------------------------------------------- (c)

SMALL = [(c.cid, v) for c in U.CASES if c.small for v in ("base", "holes")]


@pytest.mark.parametrize("cid,variant", SMALL, ids=[f"{c}-{v}" for c, v in SMALL])
def test_the_band_dp_meets_the_oracle(cid, variant):
    """the tolerances of the double table (tests/util_dag_double_regimes.py): tables and loss rtol 1e-12 / atol 1e-11, gradients 1e-9 / 1e-12"""
    ref, got = U.reference(cid, variant), U.band_dp(cid, variant)
    d = {n: U.figure(got[n], getattr(ref, n), (1e-12, 1e-11)) for n in ("alpha", "beta", "loss")}
    d.update({n: U.figure(got[n], getattr(ref, n), (1e-9, 1e-12)) for n in ("gm", "gl")})
    print(f"{cid}-{variant}: band DP vs oracle, fraction of the double tolerance used: " + "  ".join(f"{k} {v:.2e}" for k, v in d.items()))
    assert all(v <= 1.0 for v in d.values()), d


# ---------------------------------------------------------------- (d)

@pytest.mark.parametrize("cid,variant", PARAMS, ids=[f"{c}-{v}" for c, v in PARAMS])
def test_the_fp32_oracle_yardstick(cid, variant):
    """the reference's own arithmetic in fp32 against itself in fp64: -inf in the same places, and the figure the GPU test may use"""
    y = U.yardstick(cid, variant)
    print(f"dag-skew yardstick {cid}-{variant}: fp32 oracle vs fp64 oracle, fraction of the tolerance used: " + "  ".join(f"{k} {v:.2e}" for k, v in y.items()))
    assert set(y) == ({"alpha", "beta", "loss", "gm", "gl"} if U.BY_ID[cid].bwd else {"alpha", "beta", "loss"})
    assert all(np.isfinite(v) for v in y.values()), y
