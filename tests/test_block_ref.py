"""tests/util_block_ref.py on the CPU: each float64 reference against an independent torch formulation in double; every row of the case
tables reaches the regime it names; and the bound tests/test_gpu_block_regimes.py applies holds the unmutated emulation of the kernels'
arithmetic on every case input while every mutant is outside it on the cases named for it — the evidence that these inputs tell a subtly
wrong kernel from a right one.  Figures: `pytest -s`."""
import math

import numpy as np
import pytest
import torch

from tests import util_block_ref as U

F64 = torch.float64


def _t(a):
    return torch.from_numpy(np.asarray(a)).to(F64)


# ---------------------------------------------------------------- references against independent torch formulations

@pytest.mark.parametrize("act", [0, 1, 2, 3])
@pytest.mark.parametrize("with_ln", [False, True])
def test_ffn_ref_equals_a_torch_sequential_in_double(act, with_ln):
    rng = np.random.default_rng(act + 10 * with_ln)
    C, H, R = 256, 512, 37
    x, res = rng.standard_normal((R, C)), rng.standard_normal((R, C))
    ln_w, ln_b = 1 + 0.2 * rng.standard_normal(C), 0.2 * rng.standard_normal(C)
    w1, b1, w2, b2 = rng.standard_normal((H, C)) / 16, rng.standard_normal(H), rng.standard_normal((C, H)) / 22, rng.standard_normal(C)
    pw, pb = 1 + 0.2 * rng.standard_normal(C), 0.2 * rng.standard_normal(C)
    ln, l1, l2, post = torch.nn.LayerNorm(C, eps=1e-5).double(), torch.nn.Linear(C, H).double(), torch.nn.Linear(H, C).double(), torch.nn.LayerNorm(C, eps=1e-3).double()
    with torch.no_grad():
        for p, a in ((ln.weight, ln_w), (ln.bias, ln_b), (l1.weight, w1), (l1.bias, b1), (l2.weight, w2), (l2.bias, b2), (post.weight, pw), (post.bias, pb)):
            p.copy_(_t(a))
        fn = [torch.nn.Identity(), torch.nn.ReLU(), torch.nn.SiLU(), torch.nn.GELU()][act]
        seq = torch.nn.Sequential(*(([ln] if with_ln else []) + [l1, fn, l2]))
        want = _t(res) + 0.5 * seq(_t(x))
        want_ln = post(want)
    out, out_ln = U.ffn_ref(x, ln_w if with_ln else None, ln_b if with_ln else None, 1e-5, w1, b1, w2, b2, act, res, 0.5, pw, pb, 1e-3)
    torch.testing.assert_close(out, want, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(out_ln, want_ln, rtol=1e-11, atol=1e-11)
    none, _ = U.ffn_ref(x, None, None, 0.0, w1, None, w2, None, act, None, 0.5)
    torch.testing.assert_close(none, 0.5 * torch.nn.functional.linear(fn(torch.nn.functional.linear(_t(x), _t(w1))), _t(w2)), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("kind", ["none", "suffix", "holes", "lead40", "lone"])
def test_attention_ref_equals_sdpa_with_an_additive_mask(kind):
    rng = np.random.default_rng(3)
    B, N, M, H, dk = 2, 9, 65, 3, 64
    q, k, v = rng.standard_normal((B, N, H * dk)), rng.standard_normal((B, M, H * dk)), rng.standard_normal((B, M, H * dk))
    mask = U.key_masks(kind, B, M)
    out, scores = U.attention_ref(q, k, v, mask, H, 0.125)
    hd = lambda a: _t(a).view(B, -1, H, dk).transpose(1, 2)                            # noqa: E731
    add = None if mask is None else torch.zeros(B, 1, 1, M, dtype=F64).masked_fill(torch.from_numpy(mask).view(B, 1, 1, M), float("-inf"))
    want = torch.nn.functional.scaled_dot_product_attention(hd(q), hd(k), hd(v), attn_mask=add, scale=0.125).transpose(1, 2).reshape(B, N, H * dk)
    torch.testing.assert_close(out, want, rtol=1e-12, atol=1e-12)
    s = hd(q) @ hd(k).transpose(-1, -2) * 0.125
    fin = torch.isfinite(scores)
    torch.testing.assert_close(scores[fin], s[fin], rtol=1e-12, atol=1e-12)
    if mask is not None:
        assert torch.equal(~fin, torch.from_numpy(mask).view(B, 1, 1, M).expand(B, H, N, M))


def _rel_shift(x):
    """espnet_multihead_attention.py rel_shift: pad a zero column, view as [.., 2T, T], drop the first row, view back, keep T columns"""
    B, H, T, R = x.shape
    xp = torch.cat([torch.zeros(B, H, T, 1, dtype=x.dtype), x], -1).view(B, H, R + 1, T)
    return xp[:, :, 1:].reshape(B, H, T, R)[:, :, :, :T]


@pytest.mark.parametrize("T", [1, 5, 33])
def test_relpos_ref_equals_the_pad_and_reshape_rel_shift(T):
    rng = np.random.default_rng(T)
    B, H, dk = 2, 3, 64
    q, k, v = (rng.standard_normal((B, T, H * dk)) for _ in range(3))
    pos, bu, bv = rng.standard_normal((2 * T - 1, H * dk)), rng.standard_normal((H, dk)), rng.standard_normal((H, dk))
    mask = U.key_masks("suffix", B, T) if T > 1 else None
    out, _ = U.relpos_attention_ref(q, k, v, pos, bu, bv, mask, H)
    qd, kd, vd = (_t(a).view(B, T, H, dk) for a in (q, k, v))
    pd = _t(pos).view(2 * T - 1, H, dk)
    ac = torch.einsum("bihd,bjhd->bhij", qd + _t(bu), kd)
    bd = _rel_shift(torch.einsum("bihd,rhd->bhir", qd + _t(bv), pd))
    s = (ac + bd) / math.sqrt(dk)
    if mask is not None:
        s = s.masked_fill(torch.from_numpy(mask).view(B, 1, 1, T), float("-inf"))
    want = torch.einsum("bhij,bjhd->bihd", torch.softmax(s, -1), vd).reshape(B, T, H * dk)
    torch.testing.assert_close(out, want, rtol=1e-12, atol=1e-12)


# ---------------------------------------------------------------- the tables reach the regimes they name

def test_ffn_cases_reach_the_groups_chunks_and_reduce_trips_they_name():
    cs = [U.ffn_case(t) for t in U.FFN_CASES]
    for c in cs:
        assert U.ff_regime(c["B"], c["T"], c["H"]) == c["regime"], c["tag"]
        assert U.ff_workspace_bytes(c["B"], c["T"], c["H"]) == c["regime"][0] * c["B"] * c["T"] * 256 * 4
    # the table of the issue, every shape -> (G, nch)
    want = {(224, 3, 512): (1, 2), (224, 2, 2048): (1, 8), (257, 64, 512): (1, 2), (2, 65, 512): (2, 1), (1, 63, 1536): (2, 3), (112, 1, 2048): (2, 4),
            (112, 2, 1024): (2, 2), (56, 64, 2048): (4, 2), (1, 1, 1024): (4, 1), (2, 65, 3072): (4, 3), (1, 1, 2048): (8, 1), (3, 129, 4096): (8, 2)}
    assert {(c["B"], c["T"], c["H"]): c["regime"] for c in cs} == want
    assert {c["regime"][0] for c in cs} == {1, 2, 4, 8} and {c["regime"][1] for c in cs} == {1, 2, 3, 4, 8}
    assert {c["T"] for c in cs} >= {1, 63, 64, 65, 129}
    for a in range(4):
        assert sum(c["act"] == a for c in cs) >= 2, a
    assert {bool(c["ln"]) for c in cs} == {False, True} and {c["ln"] for c in cs} >= {"mean300", "const"}
    assert {(c["b1"], c["b2"]) for c in cs} == {(True, True), (False, True), (True, False), (False, False)}
    assert any(not c["res"] for c in cs)
    assert {c["xlay"] for c in cs} == {"c", "ld260", "slice768"} and any(c["ldr"] == 264 for c in cs) and any(c["ldo"] == 272 for c in cs)
    # reduce loops: one trip and more than one, in both kernels; the post-LayerNorm at rows % 4 = 1, 2, 3, with and without `out`
    plain = {U.ff_reduce_trips(c["B"], c["T"]) for c in cs if not c["post"]}
    post = {U.ff_reduce_ln_trips(c["B"], c["T"]) for c in cs if c["post"]}
    assert 1 in plain and max(plain) > 1 and 1 in post and max(post) > 1, (plain, post)
    assert U.ff_reduce_trips(257, 64) == 3 and U.ff_reduce_ln_trips(257, 64) == 2
    assert {(c["B"] * c["T"]) % 4 for c in cs if c["post"]} >= {1, 2, 3}
    assert {c["post"] for c in cs} == {"", "out", "only"}
    for names in U.FFN_MUTANT_CASES.values():
        assert set(names) <= set(U.FFN_CASES)
    # the steady-state loop runs 0, 1, 2, 3 and 7 times; G = 1 leaves ffn_reduce's k loop empty
    assert {c["regime"][1] - 1 for c in cs} == {0, 1, 2, 3, 7}
    # planted rows are what they claim
    x = U.ffn_inputs("g1-n2-trips")["x"].reshape(-1, 256)
    assert abs(float(x[:64].mean()) - 300) < 0.5 and 0.8 < float(x[:64].std()) < 1.2 and abs(float(x[64:].mean())) < 1
    xc = U.ffn_inputs("g8-n2-T129")["x"].reshape(-1, 256)
    assert (xc[5] == U.CONST_ROW_VALUE).all() and xc[4].std() > 1


def test_attention_cases_reach_the_tiles_masks_scores_and_work_orders_they_name():
    cs = [U.attention_inputs(t) for t in U.ATT_CASES]
    assert {c["N"] for c in cs} == {1, 31, 33, 65, 127, 129, 257} and {c["M"] for c in cs} == {1, 31, 32, 33, 64, 65, 97, 161}
    assert {c["dk"] for c in cs} == {64, 128}
    nts, lead, remap, nwork = set(), set(), set(), set()
    for c in cs:
        mask = c["key_mask"]
        for b in range(c["B"]):
            row = None if mask is None else mask[b]
            nts.add(U.at_nt(row, c["M"]))
            lead.add(U.at_leading_masked_tiles(row))
        remap.add((U.at_remap(c["B"], c["N"], c["H"]), U.at_ntq(c["N"])))
        nwork.add(U.at_nwork(c["B"], c["N"], c["H"]))
    assert nts == {1, 2, 3, 4, 5, 6}, nts
    assert lead >= {0, 1, 2}, lead                                       # the m_new == -inf branch once and twice on a live sample
    assert {(True, 1), (True, 3)} <= remap and {9, 15} <= nwork, (remap, nwork)
    assert {c["mask"] for c in cs} == {"none", "suffix", "lead40", "lead64", "holes", "lone", "dead"}
    assert {c["scores"] for c in cs} == {"flat", "peaked", "rising", "falling", "hot"}
    assert {c["layout"] for c in cs} == {"c", "kv2c", "qkv3c", "odd"}
    for c in cs:
        mask, M = c["key_mask"], c["M"]
        if c["mask"] == "lone":
            assert (~mask[0]).sum() == 1 and not mask[0, M - 1] and (M - 1) % 32 == 0 and U.at_nt(mask[0], M) == (M - 1) // 32 + 1
            assert (~mask[1]).sum() == 1 and not mask[1, 0]
            if c["B"] > 3:
                assert (~mask[3]).sum() == 1 and not mask[3, 31]
        if c["mask"] == "holes":
            assert mask[0, 20:53].all() and mask[0, 1::3].all() and not mask[0, 0] and 20 // 32 != 52 // 32
        if c["mask"] == "dead":
            assert mask[1].all() and not mask[0].all() and not mask[2 % c["B"]].all()
        if c["mask"] in ("lead40", "lead64"):
            n = int(c["mask"][4:])
            assert mask[0, :n].all() and not mask[0, n:].any() and U.at_leading_masked_tiles(mask[0]) == n // 32
        if mask is not None:                                             # junk in every masked row, nothing above the fp16 range
            assert (np.abs(c["k"][mask]) == U.PAD_JUNK).all() and (np.abs(c["v"][mask]) == U.PAD_JUNK).all()
        assert np.abs(c["k"]).max() < 65504 and np.abs(c["q"]).max() < 65504
    for names in list(U.ATT_MUTANT_CASES.values()) + list(U.ATT_EQUIVALENT_MUTANT_CASES.values()):
        assert set(names) <= set(U.ATT_CASES)


@pytest.mark.parametrize("tag", [t for t, c in U.ATT_CASES.items() if c[6] in ("rising", "falling", "hot", "flat", "peaked")])
def test_attention_score_shapes_are_what_their_names_say(tag):
    c = U.attention_inputs(tag)
    _, s64, _ = U.attention_refs(tag)
    mask = c["key_mask"]
    S = max(float(np.abs(s64[b][np.isfinite(s64[b])]).max()) for b in U.live_samples(mask, c["B"]))
    print(f"block-regimes scores {tag}: max |s| {S:.1f}")
    if c["scores"] == "hot":
        assert 62 < S < 80
    if c["scores"] == "flat":
        assert S < 16
    for b in U.live_samples(mask, c["B"]):
        nt = U.at_nt(None if mask is None else mask[b], c["M"])
        for h in range(c["H"]):
            tm = U.tile_maxima(s64[b, h], nt)
            live = [t for t in range(nt) if np.isfinite(tm[:, t]).all()]
            if c["scores"] == "rising":                                  # every live tile raises every query's maximum, by a clear margin
                for t0, t1 in zip(live, live[1:]):
                    assert (tm[:, t1] > tm[:, t0] + 1.0).all(), (tag, b, h, t1)
            if c["scores"] == "falling":                                 # the first live tile holds every query's maximum
                for t1 in live[1:]:
                    assert (tm[:, t1] < tm[:, live[0]] - 1.0).all(), (tag, b, h, t1)
    if c["scores"] in ("rising", "falling"):
        assert max(U.at_nt(None if mask is None else mask[b], c["M"]) for b in range(c["B"])) >= 2


def test_relpos_and_qlens_cases_reach_their_edges():
    cs = [U.relpos_inputs(t) for t in U.REL_CASES]
    assert {c["T"] for c in cs} == {1, 31, 32, 33, 127, 128, 129, 161, 257}
    assert {U.at_remap(c["B"], c["T"], c["H"]) for c in cs} == {False, True}
    assert {c["fused"] for c in cs} == {False, True} and {bool(np.any(c["bias_u"])) for c in cs} == {False, True}
    assert {c["pad_mask"] is not None for c in cs} == {False, True}
    # R0 = T - 32 - 128 qt goes negative at T < 32 and in the later query tiles: position rows below 0 must read as zeros
    assert any(c["T"] - 32 < 0 for c in cs) and any(c["T"] - 32 - 128 * (U.at_ntq(c["T"]) - 1) < 0 for c in cs if c["T"] > 128)
    N = U.QLENS_SHAPE["N"]
    assert set(U.QLENS) == {0, 1, 31, 32, 33, N, N + 50} and len(U.QLENS) == U.QLENS_SHAPE["B"]
    assert [U.q_rows_computed(n, N) for n in U.QLENS] == [0, 32, 32, 32, 64, N, N]
    assert [U.q_rows_computed(n + 5, N) for n in U.QLENS] == [32, 32, 64, 64, 64, N, N]


# ---------------------------------------------------------------- the bound holds the emulation and rejects the mutants

def _emulate_ffn(tag, with_res, mutant=None):
    d = U.ffn_inputs(tag)
    return U.emulate_ffn_split(d["x"], d["ln_w"], d["ln_b"], U.LN_EPS, d["w1"], d["b1"], d["w2"], d["b2"], d["act"], d["res"] if with_res else None,
                               U.FFN_ALPHA, d["post_w"], d["post_b"], U.LN_EPS, G=d["regime"][0], mutant=mutant)


@pytest.mark.parametrize("tag", list(U.FFN_CASES))
def test_ffn_emulation_is_inside_the_gpu_bound_on_every_case(tag):
    if U.ffn_case(tag)["res"]:                                           # a residual no larger than the branch it is added to
        branch, res = U.ffn_refs(tag, False)[0][0], U.ffn_inputs(tag)["res"]
        print(f"block-regimes scales {tag}: max |res| {np.abs(res).max():.2f} max |alpha * branch| {np.abs(branch).max():.2f}")
        assert np.abs(res).max() <= np.abs(branch).max()
    for with_res in U.ffn_twins(tag):
        out, out_ln = _emulate_ffn(tag, with_res)
        assert U.ffn_verdict(tag, with_res, out.numpy(), None if out_ln is None else out_ln.numpy(), kind="emulated-ffn")


@pytest.mark.parametrize("mutant,tag", [(m, t) for m, ts in U.FFN_MUTANT_CASES.items() for t in ts])
def test_ffn_mutants_are_outside_the_gpu_bound(mutant, tag):
    for with_res in U.ffn_twins(tag):
        out, out_ln = _emulate_ffn(tag, with_res, mutant)
        assert not U.ffn_verdict(tag, with_res, out.numpy(), None if out_ln is None else out_ln.numpy(), kind=f"mutant-{mutant}")


@pytest.mark.parametrize("i", range(len(U.LINEAR_LN_CASES)))
def test_linear_ln_emulation_is_inside_the_gpu_bound(i):
    d = U.linear_ln_inputs(i)
    got = U.emulate_linear_ln_split(d["x"], d["ln_w"], d["ln_b"], U.LN_EPS, d["w"], d["b"], d["act"])
    assert U.linear_ln_verdict(i, got.numpy(), kind="emulated-linear_ln")


def _emulate_att(tag, mutant=None, pad="junk"):
    d = U.attention_inputs(tag, pad)
    return U.emulate_attention_split(d["q"], d["k"], d["v"], d["key_mask"], d["H"], d["scale"], mutant=mutant).numpy()


@pytest.mark.parametrize("tag", list(U.ATT_CASES))
def test_attention_emulation_is_inside_the_gpu_bound_on_every_case(tag):
    got = _emulate_att(tag)
    assert U.attention_verdict(tag, got, kind="emulated-attention")
    if U.attention_inputs(tag)["key_mask"] is not None:                  # padding rows cannot leak: junk and zeros give the same bits
        assert np.array_equal(got, _emulate_att(tag, pad="zero"), equal_nan=True)


@pytest.mark.parametrize("mutant,tag", [(m, t) for m, ts in U.ATT_MUTANT_CASES.items() for t in ts])
def test_attention_mutants_are_outside_the_gpu_bound(mutant, tag):
    assert not U.attention_verdict(tag, _emulate_att(tag, mutant), kind=f"mutant-{mutant}")


@pytest.mark.parametrize("mutant,tag", [(m, t) for m, ts in U.ATT_EQUIVALENT_MUTANT_CASES.items() for t in ts])
def test_counting_key_tiles_from_m_changes_no_bit(mutant, tag):
    """the tile skip is exact: tiles past the last live key add weights of exactly 0 (util_block_ref.ATT_EQUIVALENT_MUTANT_CASES)"""
    mask = U.attention_inputs(tag)["key_mask"]
    assert any(U.at_nt(mask[b], mask.shape[1]) < (mask.shape[1] + 31) // 32 for b in range(mask.shape[0])), "the mutant walks more tiles"
    assert np.array_equal(_emulate_att(tag, mutant), _emulate_att(tag), equal_nan=True)


def _emulate_rel(tag, mutant=None):
    d = U.relpos_inputs(tag)
    return U.emulate_attention_split(d["q"], d["k"], d["v"], d["pad_mask"], d["H"], 0.125, d["pos"], d["bias_u"], d["bias_v"], mutant=mutant).numpy()


@pytest.mark.parametrize("tag", list(U.REL_CASES))
def test_relpos_emulation_is_inside_the_gpu_bound_on_every_case(tag):
    assert U.relpos_verdict(tag, _emulate_rel(tag), kind="emulated-relpos")


@pytest.mark.parametrize("mutant,tag", [(m, t) for m, ts in U.REL_MUTANT_CASES.items() for t in ts])
def test_relpos_mutants_are_outside_the_gpu_bound(mutant, tag):
    assert not U.relpos_verdict(tag, _emulate_rel(tag, mutant), kind=f"mutant-{mutant}")
