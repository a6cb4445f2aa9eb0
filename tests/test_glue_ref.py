"""CPU: the float64 references of tests/util_glue_ref.py against independent statements of the same steps (torch CPU float64 modules,
torch.bucketize, torch.log_softmax, the C oracle), <= 1e-12 or exact for integer outputs — and the input properties the GPU tests of
tests/test_gpu_glue_regimes.py rely on (dead rows beside live ones, bit-equal maxima that survive the cast to fp16 / bf16, values on and
beyond the bin edges)."""
import numpy as np
import pytest
import torch

from oracle import dag_oracle as orc
from tests import util_glue_ref as G
from tests import util_posterior_ref as P


def _close(got, want, tol=1e-12):
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape
    assert float(np.abs(got - want).max()) <= tol * max(1.0, float(np.abs(want).max()))


def test_posterior_ref_is_the_shared_one():
    assert G.posterior_ref is P.posterior_ref


@pytest.mark.parametrize("V", [1, 3, 600])
def test_argmax_logp_ref_matches_log_softmax_max_and_the_oracle(V):
    x = G.argmax_inputs(5 + V, 2, 7, V, ties=G.TIES if V == 600 else ())
    tok, sc = G.argmax_logp_ref(x)
    lp, ti = torch.log_softmax(torch.from_numpy(x).double(), -1).max(-1)
    _close(sc, lp.numpy())
    tok_o, sc_o = orc.argmax_logp(x)                          # the C oracle: first maximum, fp32 score
    np.testing.assert_array_equal(tok, tok_o)
    np.testing.assert_allclose(sc, sc_o, rtol=0, atol=2e-6)
    no_tie = np.ones(2 * 7, bool)
    if V == 600:
        no_tie[[r for r, _, _ in G.TIES]] = False
    np.testing.assert_array_equal(tok.reshape(-1)[no_tie], ti.numpy().reshape(-1)[no_tie])      # torch's max names no tie rule


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_planted_ties_are_bit_equal_maxima_after_the_cast(dtype):
    x = torch.from_numpy(G.argmax_inputs(21, 2, 7, 600, ties=G.TIES)).to(dtype)
    bits = x.view(torch.int16) if dtype != torch.float32 else x.view(torch.int32)
    xf = x.float().reshape(-1, 600)
    tok, _ = G.argmax_logp_ref(xf.numpy())
    for r, v1, v2 in G.TIES:
        assert v1 < v2 and bits.reshape(-1, 600)[r, v1] == bits.reshape(-1, 600)[r, v2]
        assert xf[r, v1] == xf[r].max() and int((xf[r] == xf[r].max()).sum()) == 2
        assert tok.reshape(-1)[r] == v1
    assert (G.TIES[0][1] >> 6) != (G.TIES[0][2] >> 6)                                    # two waves
    assert G.TIES[1][2] - G.TIES[1][1] == 256                                            # one thread of a 256-thread workgroup, two trips
    assert G.TIES[2][1] == 63 and G.TIES[2][2] == 64                                      # the wave boundary


@pytest.mark.parametrize("case", G.DWCONV_CASES)
@pytest.mark.parametrize("affine", [True, False])
def test_dwconv_bn_silu_ref_matches_the_torch_module_chain(case, affine):
    seed, B, T, C, K = case
    x, w, bw, bb, mean, var = G.dwconv_inputs(seed, B, T, C, K)
    eps = 1e-5
    dw = torch.nn.Conv1d(C, C, K, padding=(K - 1) // 2, groups=C, bias=False).double()
    bn = torch.nn.BatchNorm1d(C, eps=eps, affine=affine).double().eval()
    with torch.no_grad():
        dw.weight.copy_(torch.from_numpy(w).double().unsqueeze(1))
        bn.running_mean.copy_(torch.from_numpy(mean)); bn.running_var.copy_(torch.from_numpy(var))
        if affine:
            bn.weight.copy_(torch.from_numpy(bw)); bn.bias.copy_(torch.from_numpy(bb))
        want = torch.nn.functional.silu(bn(dw(torch.from_numpy(x).double().transpose(1, 2)))).transpose(1, 2)
    got = G.dwconv_bn_silu_ref(x, w, bw if affine else None, bb if affine else None, mean, var, eps)
    _close(got, want.numpy())


@pytest.mark.parametrize("case", G.LAYER_NORM_CASES)
@pytest.mark.parametrize("affine", [True, False])
def test_layer_norm_ref_matches_torch_double(case, affine):
    seed, rows, C, mean, spread = case
    x, w, b = G.layer_norm_inputs(seed, rows, C, mean, spread)
    xd = torch.from_numpy(x).double()
    want = torch.nn.functional.layer_norm(xd, (C,), torch.from_numpy(w).double() if affine else None,
                                          torch.from_numpy(b).double() if affine else None, 1e-5)
    got = G.layer_norm_ref(x, w if affine else None, b if affine else None, 1e-5)
    _close(got, want.numpy())
    if mean == 100.0:
        assert abs(float(x.mean()) - 100.0) < 0.01 and float(x.std()) < 0.02       # the row mean dwarfs its spread


@pytest.mark.parametrize("case", G.BUCKETIZE_CASES)
def test_bucketize_ref_matches_torch_bucketize_and_the_oracle(case):
    seed, n, C, nb = case
    x, v, bins, emb = G.bucketize_inputs(seed, n, C, nb)
    idx = G.bucketize_ref(v, bins)
    np.testing.assert_array_equal(idx, torch.bucketize(torch.from_numpy(v), torch.from_numpy(bins)).numpy())
    np.testing.assert_array_equal(idx, orc.bucketize(v, bins))
    out = G.bucketize_embed_add_ref(x, v, bins, emb)
    assert out.dtype == np.float32
    np.testing.assert_array_equal(out, (torch.from_numpy(x) + torch.from_numpy(emb)[torch.from_numpy(idx)]).numpy())
    # the inputs hold what the GPU test is about
    assert np.isneginf(v).any() and np.isposinf(v).any()
    if nb:
        assert np.isin(v, bins).sum() >= (3 if n > 8 else 1)                 # values exactly on an edge
        assert (v[np.isfinite(v)] < bins[0]).any() and (v[np.isfinite(v)] > bins[-1]).any()
        assert idx.min() == 0 and idx.max() == nb
        assert idx[np.isin(v, bins)].max() < nb                              # an edge value belongs to the bin it closes (right=False)
    else:
        assert np.all(idx == 0)
    if n > 4096:
        assert idx[4096] != idx[0] or idx[n - 1] != idx[n - 1 - 4096]        # a row of the second grid-stride trip differs from its partner


def test_gather_rows_ref_matches_the_oracle_walk():
    B, L, V, TR, D, pad = 3, 40, 11, 4, 7, 1
    ol = np.array([40, 2, 1], np.int64)
    logits, links, feats = G.decode_inputs(3, B, L, V, TR, D, ol, pad)
    tok, sc = orc.argmax_logp(logits)
    nxt = orc.lookahead_next(links, sc, 1.0)
    _, keep, nf = orc.follow_path(nxt, tok, ol, pad)
    fmax = int(nf.max()) + 2
    out = G.gather_rows_ref(feats, keep, nf, fmax)
    for b in range(B):
        last = tok[b, 0]; j = 0; kept = []
        while j != ol[b] - 1:                                 # the reference's host loop (s2s_conformer_dag_fastspeech2.py:219-243)
            j = nxt[b, j]; now = tok[b, j]
            if now != pad and now != last:
                kept.append(j)
            last = now
        assert len(kept) == nf[b]
        np.testing.assert_array_equal(out[b, : len(kept)], feats[b, kept])
        assert np.all(out[b, len(kept):] == 0)
    assert nf[0] > 0 and nf[1] <= 1 and nf[2] == 0 and fmax > nf.max()
    half = G.gather_rows_ref(feats.astype(np.float16), keep, nf, fmax)
    assert half.dtype == np.float16
    np.testing.assert_array_equal(half, out.astype(np.float16))


def test_all_pad_decode_inputs_emit_only_pad():
    ol = np.array([50, 2, 1], np.int64)
    logits, links, _ = G.decode_inputs(9, 3, 50, 11, 4, 7, ol, 1, all_pad=True)
    tok, sc = orc.argmax_logp(logits)
    assert np.all(tok == 1)
    _, keep, nf = orc.follow_path(orc.lookahead_next(links, sc, 1.0), tok, ol, 1)
    assert np.all(nf == 0) and np.all(keep == -1)


def test_decode_inputs_links_are_distributions_over_the_valid_successors():
    ol = np.array([30, 2, 1], np.int64)
    _, links, _ = G.decode_inputs(4, 3, 30, 11, 4, 7, ol, 1)
    i = np.arange(30)[None, :, None]; d = np.arange(4)[None, None, :]
    valid = (i + d + 1) < ol[:, None, None]
    np.testing.assert_array_equal(np.isfinite(links), valid)
    rows = valid.any(-1)
    with np.errstate(divide="ignore"):
        np.testing.assert_allclose(np.log(np.exp(links.astype(np.float64)).sum(-1))[rows], 0.0, atol=1e-6)


def test_posterior_ref_matches_torch_double_softmax_and_autograd():
    a, b, tl = G.ragged_posterior_inputs(51, 2, 9, 70)
    f, g = G.features_inputs(51, 2, 70, 9, 6)
    p, lse, out, gf = G.posterior_ref(a, b, f, g)
    s = torch.from_numpy(a).double() + torch.from_numpy(b).double()
    sm = torch.softmax(s, -1)
    sm = sm.masked_fill(torch.isnan(sm), 0.0)                 # the reference's NaN -> 0 (s2s_dag_fastspeech2_loss.py:260)
    fd = torch.from_numpy(f).double().requires_grad_()
    o = torch.matmul(sm, fd)
    (o * torch.from_numpy(g).double()).sum().backward()
    _close(p, sm.numpy()); _close(out, o.detach().numpy()); _close(gf, fd.grad.numpy())
    live = np.isfinite(lse)
    _close(lse[live], torch.logsumexp(s, -1).numpy()[live])


def test_posterior_inputs_hold_dead_rows_beside_live_ones():
    seed, B, T, L = G.POSTERIOR_STRIDE
    dead = G.stride_dead_rows(B * T)
    for scale in G.POSTERIOR_SCALES:
        a, b = G.posterior_inputs(seed, B, T, L, scale, dead)
        s = (a.astype(np.float64) + b).reshape(B * T, L)
        live = np.isfinite(s).any(-1)
        assert B * T == 4100 and not np.isposinf(s).any() and not np.isnan(s).any()
        np.testing.assert_array_equal(np.nonzero(~live)[0], dead)
        # rows r and r + 4096 share a workgroup: one live, one dead, both ways round
        assert live[0] and not live[4096] and live[2] and not live[4098]
        assert not live[1] and live[4097] and not live[3] and live[4099]
        assert (~live[4:4096]).sum() == len([r for r in range(4, 4096) if r % 7 == 0])
        assert np.isneginf(s[live]).any()                                    # -inf entries inside live rows
    for seed, B, T, L in G.POSTERIOR_SMALL:
        a, b = G.posterior_inputs(seed, B, T, L, 300.0)
        assert np.isfinite(a.astype(np.float64) + b).any(-1).all()
    for (seed, B, T, L) in [(52, 2, 9, 1537), (53, 2, 33, 9), (54, 2, 257, 9)]:
        a, b, tl = G.ragged_posterior_inputs(seed, B, T, L)
        live = np.isfinite(a.astype(np.float64) + b).any(-1)
        assert tl[0] == T and (tl[1:] < T).all()
        for bb in range(B):
            assert live[bb, : tl[bb]].all() and not live[bb, tl[bb]:].any()


def test_fp32_bound_is_capped_and_floored():
    assert G.fp32_bound(0.0, 1e-4) == 4 * 2.0 ** -23
    assert G.fp32_bound(1e-6, 1e-4) == 8e-6 + 4 * 2.0 ** -23
    assert G.fp32_bound(1.0, 2e-6) == 2e-6
    assert G.rel_err(np.array([1.0, 2.0 + 1e-6]), np.array([1.0, 2.0])) == pytest.approx(5e-7)
