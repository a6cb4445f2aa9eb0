"""tests/util_links_regimes.py on the CPU: (a) the two float64 formulations of the link producer agree on every row of the case table;
(b) every row reaches the regime it names — live tile counts and their parity, FULL / partial blocks and EMIT's dead tiles, the running
maximum of the walk under `rise` and `fall`, the size of the scores, the XCD slot of every sample; (c) the bound that
tests/test_gpu_links_regimes.py applies holds the unmutated emulation of each kernel family's arithmetic on every row (= the fp32 evaluation
alone sits inside the cap on every slice) and rejects every mutant on the rows named for it — the evidence that these inputs tell a subtly
wrong kernel from a right one.  No kernel is launched.  Figures: `pytest -s`."""
import math

import pytest
import torch

from tests import util_links_regimes as U
from tests.util_links_ref import H, links_loop

VALUE_AGREE, GRAD_AGREE = 1e-12, 1e-9


def _row(rid):
    return U.ROW[rid]


# ---------------------------------------------------------------- (a)

@pytest.mark.parametrize("rid", U.IDS)
def test_the_two_float64_formulations_agree(rid):
    row = _row(rid)
    band, loop = U.reference(row), U.run64(row, links_loop)
    c = U.inputs(row)
    assert torch.equal(torch.isneginf(band["links"]), c["invalid"]) and torch.equal(torch.isneginf(loop["links"]), c["invalid"])
    rows = ~c["invalid"].all(-1)
    # every row with a successor spreads the gates' mass (their fp32 log-probabilities sum to 1 within 1e-7) over its window
    mass = torch.logsumexp(c["lg"].double(), -1)
    assert float((torch.logsumexp(band["links"], -1) - mass)[rows].abs().max()) <= 1e-11
    assert torch.equal(torch.isneginf(band["stats"][..., 0]), ~rows.unsqueeze(-1).expand(-1, -1, H))
    assert torch.equal(torch.isneginf(loop["stats"][..., 0]), torch.isneginf(band["stats"][..., 0]))
    fig = {}
    for n in U.NAMES:
        a, b = loop[n], band[n]
        assert torch.isfinite(b[~torch.isneginf(b)]).all() and not torch.isnan(a).any(), n
        f = torch.isfinite(b)
        # values: against max(1, |value|); gradients: against the tensor's largest magnitude (they scale with grad_links)
        den = b[f].abs().clamp_min(1.0) if n in ("links", "stats") else b.abs().max().clamp_min(1e-300)
        fig[n] = float(((a[f] - b[f]).abs() / den).max()) if f.any() else 0.0
    print(f"{rid}: loop vs chunked band  " + "  ".join(f"{n} {v:.1e}" for n, v in fig.items()))
    assert fig["links"] <= VALUE_AGREE and fig["stats"] <= VALUE_AGREE
    assert max(fig[n] for n in ("dq", "dk", "dg")) <= GRAD_AGREE
    # rows at or beyond the graph take no gradient, whatever grad_links holds there
    for b, n in enumerate(row.lens):
        for t in (band["dq"], band["dk"], band["dg"]):
            assert not t[b, min(n, row.L):].any()


# ---------------------------------------------------------------- (b)

def _window_tile_maxima(row):
    """per (sample, vertex, head): the float64 maxima of the 32-partner tiles of the window, in the order the matrix-core kernels walk them
    (far end first); -inf for a tile without a valid successor.  -> [B, L, H, T]"""
    c = U.inputs(row)
    B, L, TR, CK = row.B, row.L, row.TR, row.CK
    q, k = c["q"].double(), c["k"].double()
    j = torch.arange(L).view(L, 1) + torch.arange(TR).view(1, TR) + 1
    s = torch.stack([torch.einsum("lhc,ldhc->ldh", q[b], k[b][j.clamp(max=L - 1)]) for b in range(B)]) / math.sqrt(CK)
    if c["bias"] is not None:
        s = s + c["bias"].double().view(1, 1, TR, 1)
    s = s.masked_fill(c["invalid"].unsqueeze(-1), -math.inf)
    tiles = sorted(set((j >> 5).flatten().tolist()), reverse=True)
    return torch.stack([s.masked_fill(((j >> 5) != t).view(1, L, TR, 1), -math.inf).max(2).values for t in tiles], -1)


@pytest.mark.parametrize("rid", U.IDS)
def test_every_row_reaches_the_regime_it_names(rid):
    row = _row(rid)
    c, ref = U.inputs(row), U.reference(row)
    L, TR = row.L, row.TR
    facts = U.mfma_facts(row) if row.fam == "mfma" else set()
    mx = ref["stats"][..., 0]
    live = torch.isfinite(mx)
    if (~live).any() and all(min(n, L) >= 1 for n in row.lens):
        facts.add("nosucc")
    top = float(mx[live].abs().max())
    lo, hi = U.SCORE_INTERVAL[row.score]
    if lo <= top <= hi:
        facts.add("score")
    if row.score in ("rise", "fall"):
        tm = _window_tile_maxima(row)                                              # walked order: far end first
        fin = torch.isfinite(tm)
        run = torch.cummax(tm.masked_fill(~fin, -math.inf), -1).values             # the running maximum after each walked tile
        rises = (tm[..., 1:] > run[..., :-1]) & fin[..., 1:] & torch.isfinite(run[..., :-1])
        steps = fin[..., 1:] & torch.isfinite(run[..., :-1])                       # a tile walked after the first live one
        assert int(steps.sum()) > 500
        if row.score == "rise":
            assert bool(rises[steps].all()), "the running maximum rises on every walked tile"
        else:
            assert not bool(rises.any()), "the first tile walked holds the maximum"
        # and the ramp is what does it: neighbouring successors differ by SLOPE
        print(f"{rid}: {int(steps.sum())} tile steps after the first, the maximum rises on {int(rises.sum())}")
    if row.score == "gate_off":
        g = c["lg"].double()
        off = g[:, ::3, U.GATE_OFF_HEAD]
        rest = torch.cat([g[:, ::3, :U.GATE_OFF_HEAD], g[:, ::3, U.GATE_OFF_HEAD + 1:]], -1)
        assert float(off.max()) < float(rest.min()) - 60.0 and float(g[:, 1::3].min()) > -15.0
        assert abs((g.shape[1] + 2) // 3 / g.shape[1] - 1 / 3) < 0.01
        facts.add("gate_off")
    if row.score == "bias_steep":
        assert torch.equal(c["bias"], -0.5 * torch.arange(TR, dtype=torch.float32))
    if row.score == "bias_none":
        assert c["bias"] is None
    G = c["G"]
    if row.grad == "ranged":
        m = [float(G[b].abs().max()) for b in range(row.B)]
        if max(m) / min(m) > 2.0 ** 38 and min(m) < 2.0 ** -36:                  # 2^-40, 1 (and 2^40 from the third sample on)
            facts.add("ranged")
        assert row.B < 3 or max(m) > 2.0 ** 39
    if row.grad == "sparse":
        assert not G[:, 1::3].any() and G[:, 0::3].abs().min() > 0
        facts.add("sparse")
    if row.grad == "planted":
        inv = c["invalid"]
        assert torch.isfinite(G[~inv]).all() and not torch.isfinite(G[inv]).any()
        assert torch.isnan(G[inv]).any() and torch.isposinf(G[inv]).any() and torch.isneginf(G[inv]).any()
        # some of them sit where the matrix-core kernels stage them: inside the band, in the last live partner tile of a graph
        if row.fam == "mfma":
            hit = 0
            for b, n in enumerate(row.lens):
                if 1 < n < L and n % 32:
                    i = n - 2                                                     # successor n - 1 is the last valid one; slot d = 1 -> j = n
                    hit += int(TR > 1 and not torch.isfinite(G[b, i, 1]))
            assert hit or all(n >= L or n % 32 == 0 or n <= 1 for n in row.lens)
        assert torch.isfinite(ref["dq"]).all() and torch.isfinite(ref["dk"]).all() and torch.isfinite(ref["dg"]).all()
        facts.add("planted")
    if row.fam == "mfma" and row.B % 8 == 0:
        OT = 32 if L <= 1536 else 64
        m = U.xcd_map(row.B, L, OT)
        NQ = (L + OT - 1) // OT
        assert sorted((b, x) for _, b, x in m) == [(b, x) for b in range(row.B) for x in range(NQ)], "every (sample, owner tile) once"
        assert all(xcd == b % 8 for xcd, b, _ in m), "a sample stays on one XCD: slot = sample mod 8"
        facts.add("xcd")
        if any(b >= 8 for _, b, _ in m):
            assert {b for xcd, b, _ in m if xcd == 3} == {3 + 8 * n for n in range(row.B // 8)}
            assert len(set(row.lens)) == row.B, "all lengths differ: a swapped sample shows"
            facts.add("xcd_round2")
    if row.fam == "tiled":
        lds = (4 * 8 * row.CK + 4 * ((TR + 31) // 32) * 32 * 8 + 64) * 4
        if row.tile == 0:
            assert lds > 150 * 1024 and -(-TR // 512) == 3
            facts.add("auto_tiled")
        else:
            assert lds <= 150 * 1024 and TR > row.tile and min(TR % row.tile, row.tile - TR % row.tile) <= 1
    if row.fam == "one":
        assert (4 * 8 * row.CK + 4 * ((TR + 31) // 32) * 32 * 8 + 64) * 4 <= 150 * 1024 and row.tile == 0
    print(f"{rid}: largest |window maximum| {top:.2f}  reaches {sorted(facts)}")
    assert set(row.reach) <= facts, sorted(set(row.reach) - facts)


def test_the_table_as_a_whole():
    mc = [r for r in U.ROWS if r.fam == "mfma"]
    facts = set().union(*(U.mfma_facts(r) for r in mc))
    assert {"nlive%d" % n for n in range(1, 6)} <= facts
    assert {"live_odd", "live_even", "step_odd", "step_even", "bwd_odd", "bwd_even", "bwdT_odd", "bwdT_even", "dead", "full", "partial",
            "qg1", "qg2", "len32k-1", "len32k", "len32k+1", "triple_by_default"} <= facts
    assert any(r.L == 1536 for r in mc) and any(r.contract == (None,) and r.L > 1536 for r in mc)
    for score in ("peaked", "steep", "rise", "fall", "bias_steep", "bias_none", "gate_off"):
        assert any(r.score == score for r in mc), score
    for fam in ("mfma", "one", "tiled"):
        assert {r.grad for r in U.ROWS if r.fam == fam} >= {"unit", "ranged", "sparse", "planted"}, fam
    assert {r.CK for r in U.ROWS if r.fam == "one"} == {32, 64, 128} and {r.tile for r in U.ROWS if r.fam == "tiled"} == {0, 32, 64}
    assert len(U.ROWS) <= 48 and len(set(U.IDS)) == len(U.IDS)
    for m, rids in MUTANT_ROWS.items():
        assert m in U.MUTANTS and rids and all(r in U.ROW for r in rids)
    assert set(MUTANT_ROWS) == set(U.MUTANTS)


# ---------------------------------------------------------------- (c)

def _contracts(row):
    return row.contract if row.fam == "mfma" else (0,)


@pytest.mark.parametrize("rid", U.IDS)
def test_the_fp32_evaluation_sits_inside_the_cap_on_every_slice(rid):
    """= the bound holds the unmutated emulation: err_ref <= min(8 err_ref + 4 ulp scale, cap scale)  <=>  err_ref <= cap scale"""
    row = _row(rid)
    ref = U.reference(row)
    for ct in _contracts(row):
        emu = U.emulation(row, ct)
        for n in U.NAMES:
            vs = U.term_scale(row) if n in U.void_gradients(row) else None
            ok, ratio, err, bd, scale, _ = U.judge(n, emu[n], emu[n], ref[n], vs)
            rel = float(torch.where(scale > 0, err / scale.clamp_min(1e-300), err).max())
            print(f"{rid} contract {ct}: {n}: emulation's largest err / scale {rel:.2e} (cap {U.CAP:.0e})")
            assert ok, (rid, ct, n, U.figures(n, emu[n], emu[n], ref[n]))
            assert torch.equal(torch.isneginf(emu[n]), torch.isneginf(ref[n])) and not torch.isnan(emu[n]).any()
        for b, m in enumerate(row.lens):
            assert not emu["dq"][b, m:].any() and not emu["dk"][b, m:].any() and not emu["dg"][b, m:].any()


MUTANT_ROWS = {
    "lo_dropped": ("mc-B6-TR64-steep", "mc-B8-L70-TR69"),
    "first_tile_dropped": ("mc-B6-L160-TR159", "mc-B6-TR159-fall"),
    "last_tile_dropped": ("mc-B6-L160-TR159", "mc-B6-TR159-rise"),
    "band_edge": ("mc-B8-L70-TR7", "one-CK64-L70-TR33", "tiled32-L70-TR63"),
    "mask_by_L": ("mc-B8-L70-TR69", "one-CK32-L70-TR31"),
    "bias_shift": ("mc-B6-TR33-bias_steep", "mc-B6-L160-TR33", "one-CK64-L70-TR32-sparse"),
    "half_missing": ("mc-B6-L160-TR31", "mc-L65-TR33"),
    "no_rescale": ("mc-B6-TR159-rise", "mc-B6-TR64-steep"),
    "three_products": ("mc-L1570-TR97-default", "mc-B6-L160-TR159"),
    "no_sa_term": ("mc-B6-L160-TR64", "one-CK128-L70-TR69", "tiled64-L131-TR127"),
    "swap_b8": ("mc-B16-L70-TR7", "mc-B16-L70-TR69"),
    "g_leak": tuple(r.id for r in U.ROWS if r.grad == "planted"),
}


@pytest.mark.parametrize("mutant,rid", [(m, r) for m, rids in MUTANT_ROWS.items() for r in rids])
def test_the_bound_rejects_the_mutant(mutant, rid):
    row = _row(rid)
    ref = U.reference(row)
    ct = 1 if mutant == "three_products" else (_contracts(row)[0] or 0)
    emu, bad = U.emulation(row, ct), U.emulate(row, ct, mutant)
    verdict = {n: U.judge(n, bad[n], emu[n], ref[n], U.term_scale(row) if n in U.void_gradients(row) else None) for n in U.NAMES}
    for n, v in verdict.items():
        out = int((v[2] > v[3]).sum())
        fin = v[2][torch.isfinite(v[2])]
        print(f"{mutant} on {rid}: {n}: {out} of {v[2].numel()} slices outside the bound"
              + (f", largest finite err / scale {float((fin / v[4][torch.isfinite(v[2])].clamp_min(1e-300)).max()):.2e}" if fin.numel() else ""))
    assert not all(v[0] for v in verdict.values()), "the mutant passes the bound on every tensor"
    if mutant == "g_leak":
        # what the leak looks like: a NaN in dq, dk and dgate
        assert all(torch.isnan(bad[n]).any() for n in ("dq", "dk", "dg"))
    if mutant == "three_products":
        assert verdict["links"][0] and verdict["stats"][0] and verdict["dg"][0] and not (verdict["dq"][0] or verdict["dk"][0])
