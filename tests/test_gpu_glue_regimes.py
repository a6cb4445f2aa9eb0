"""The decode / TTS glue kernels (csrc/decode_tts.hip, csrc/conformer_ops.hip) against the float64 references of tests/util_glue_ref.py at the
launch regimes the workloads run and the older tests never reach: more rows than the 4096-workgroup grids (grid-stride loops), rows longer
than one trip of the block-stride loops, the dynamic-LDS opt-in, ties that cross waves, byte-copied feature rows, a 256-thread embedding add.

Integer and copy outputs are exact.  Float outputs must be as accurate as an fp32 implementation: torch's own fp32 result of the same step
(CPU) is measured against the same float64 reference in the same test, `err <= 8 * err32 + 4 fp32 ulps`, and never beyond the tolerance the
older tests of the kernel hold (G.fp32_bound).  Errors are max |got - ref| over the largest reference magnitude; every case prints its
figures (`pytest -s`, profiles/r07_glue_regimes.txt).  Where a case is about every output element being written, the C entry point is
called on a NaN-filled (integers: -7) buffer, so that a stale block of the caching allocator cannot stand in for a row the kernel skipped."""
import numpy as np
import pytest
import torch

from oracle import dag_oracle as orc
from tests import util_glue_ref as G
from tests import util_posterior_ref as P

pytestmark = pytest.mark.gpu
NAN = float("nan")


def D():
    from daspeech_amd import decode_ops
    return decode_ops


def LIB():
    from daspeech_amd import _lib
    return _lib


def cu(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to("cuda")


def poisoned(shape, dtype=torch.float32):
    return torch.full(shape, -7 if dtype in (torch.int32, torch.int64) else NAN, dtype=dtype, device="cuda")


def judge(kernel, case, got, ref, ref32, cap):
    got = np.asarray(got)
    err, err32 = G.rel_err(got, ref), G.rel_err(ref32, ref)
    bound = G.fp32_bound(err32, cap)
    ratio = err / err32 if err32 > 0 else (0.0 if err == 0 else float("inf"))
    print(f"glue-regimes {kernel} {case}: err {err:.3e} err32 {err32:.3e} ratio {ratio:.2f} bound {bound:.3e}")
    assert got.shape == np.asarray(ref).shape
    assert not np.isnan(got).any(), f"{kernel} {case}: an output element was never written (or is NaN)"
    assert err <= bound, f"{kernel} {case}: err {err:.3e} > bound {bound:.3e} (torch fp32: {err32:.3e})"


# ---------------------------------------------------------------- dsp_posterior

def _posterior_cap(a, b):
    """1e-4 (tests/test_gpu_decode_ops.py::test_posterior_and_expect); at large sums the fp32 rounding of alpha + beta itself, a relative
    error of max|alpha + beta| * 2^-23 in exp(alpha + beta - lse), takes over"""
    return max(1e-4, P.max_finite_abs(a.astype(np.float64), b.astype(np.float64)) * G.FP32_ULP)


def _softmax32(a, b):
    p = torch.softmax(torch.from_numpy(a) + torch.from_numpy(b), -1)
    return p.masked_fill(torch.isnan(p), 0.0)


def _posterior_direct(a, b):
    lib = LIB()
    ta, tb = cu(a), cu(b)
    B, T, L = a.shape
    out = poisoned((B, T, L))
    lib.check(lib.load().dsp_posterior(lib.ptr(ta), lib.ptr(tb), lib.ptr(out), B, T, L, lib.current_stream_handle()), "dsp_posterior")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check_posterior(case, got, a, b):
    p, lse, _, _ = G.posterior_ref(a, b)
    live = np.isfinite(lse)
    cap = _posterior_cap(a, b)
    judge("posterior", case, got, p, _softmax32(a, b).numpy(), cap)
    assert np.all(got[~live] == 0), "rows without a finite entry are exactly 0"
    sums = got.astype(np.float64).sum(-1)
    assert float(np.abs(sums[live] - 1.0).max()) <= cap, float(np.abs(sums[live] - 1.0).max())


@pytest.mark.parametrize("scale", G.POSTERIOR_SCALES)
@pytest.mark.parametrize("case", G.POSTERIOR_SMALL)
def test_posterior_row_lengths_around_a_wave_and_a_workgroup(case, scale):
    """L = 1, 63, 65, 256, 257: a single vertex, a partial wave, one lane of the second wave, exactly one trip of the 256-thread loops and
    the second trip with one live lane; synthetic alpha / beta at |sum| ~ 1 and ~ 1e3 with -inf entries"""
    seed, B, T, L = case
    a, b = G.posterior_inputs(seed, B, T, L, scale)
    _check_posterior((B, T, L, scale), _posterior_direct(a, b), a, b)


@pytest.mark.parametrize("scale", G.POSTERIOR_SCALES)
def test_posterior_grid_stride_rows_with_dead_and_live_partners(scale):
    """4100 rows on the 4096-workgroup grid: workgroups 0..3 serve rows r and r + 4096, one of them without a finite entry (both orders), so a
    loop that stops after its first row, or a dead first row that ends the workgroup, leaves NaN in the poisoned buffer"""
    seed, B, T, L = G.POSTERIOR_STRIDE
    a, b = G.posterior_inputs(seed, B, T, L, scale, G.stride_dead_rows(B * T))
    _check_posterior((B, T, L, scale), _posterior_direct(a, b), a, b)


def test_posterior_wrapper_on_dp_made_rows():
    """decode_ops.posterior on alpha / beta of the float64 oracle DP rounded to fp32 (L = 700: three trips), ragged target lengths"""
    c = P.make_case(*P.CASES[3])
    a, b = c["alpha"].astype(np.float32), c["beta"].astype(np.float32)
    got = D().posterior(cu(a), cu(b)).cpu().numpy()
    _check_posterior(tuple(a.shape) + ("dp",), got, a, b)
    for bb, tl in enumerate(c["tgt_len"]):
        assert np.all(got[bb, tl:] == 0) and np.all(got[bb, :tl].sum(-1) > 0.99)


# ---------------------------------------------------------------- dsp_posterior_features / _bwd

# (seed, B, T, L, D, fused): the LDS opt-in of the forward (8 * L * 4 > 48 KB), a feature width past one pass of the 256 column pairs, the
# last L the fused kernel takes and the first it does not, an odd width (fp32 two-step form); then the backward's second LDS fill trip
# (T * 8 > 256), many trips, and its LDS opt-in (8 * T * 4 > 48 KB)
FEATURE_CASES = [(52, 2, 9, 1537, 2, True), (55, 2, 9, 70, 514, True), (56, 1, 2, 4800, 2, True), (57, 1, 2, 4801, 2, False),
                 (58, 2, 9, 70, 33, False), (53, 2, 33, 9, 2, True), (54, 2, 257, 9, 6, True), (60, 1, 1537, 4, 2, True)]


def _features32(a, b, f, g):
    p = _softmax32(a, b)
    return torch.matmul(p, torch.from_numpy(f)).numpy(), torch.einsum("btl,btd->bld", p, torch.from_numpy(g)).numpy()


@pytest.mark.parametrize("case", FEATURE_CASES)
def test_posterior_features_forward_and_backward(case):
    """decode_ops.posterior_features under autograd against posterior_ref's `out` and `grad_features`; rows past a ragged T_b are dead:
    their output rows are exactly 0 and they add nothing to the gradient"""
    seed, B, T, L, Dm, fused = case
    a, b, tl = G.ragged_posterior_inputs(seed, B, T, L)
    f, g = G.features_inputs(seed, B, L, T, Dm)
    _, _, out_ref, gf_ref = G.posterior_ref(a, b, f, g)
    out32, gf32 = _features32(a, b, f, g)
    tf = cu(f).requires_grad_()
    out = D().posterior_features(cu(a), cu(b), tf)
    assert (type(out.grad_fn).__name__ == "_PosteriorFeaturesFnBackward") == fused, type(out.grad_fn).__name__
    out.backward(cu(g))
    got = out.detach().cpu().numpy()
    judge("posterior_features", (B, T, L, Dm), got, out_ref, out32, 1e-4)
    for bb in range(B):
        assert np.all(got[bb, tl[bb]:] == 0)
    judge("posterior_features_bwd", (B, T, L, Dm), tf.grad.cpu().numpy(), gf_ref, gf32, 1e-4)


def test_posterior_features_direct_calls_write_every_element():
    """dsp_posterior_features with the LDS opt-in (L = 1537) and dsp_posterior_features_bwd with 9 trips of the LDS fill (T = 257, L = 9: a
    full vertex block and a block of one) on NaN-filled buffers; lse is -inf on dead rows and the row's log-sum-exp elsewhere"""
    lib = LIB()
    st = lib.current_stream_handle()
    seed, B, T, L, Dm, _ = FEATURE_CASES[0]
    a, b, tl = G.ragged_posterior_inputs(seed, B, T, L)
    f, g = G.features_inputs(seed, B, L, T, Dm)
    _, lse_ref, out_ref, _ = G.posterior_ref(a, b, f, g)
    ta, tb, tf = cu(a), cu(b), cu(f)
    out, lse = poisoned((B, T, Dm)), poisoned((B, T))
    lib.check(lib.load().dsp_posterior_features(lib.ptr(ta), lib.ptr(tb), lib.ptr(tf), lib.ptr(out), lib.ptr(lse), B, T, L, Dm, st),
              "dsp_posterior_features")
    torch.cuda.synchronize()
    judge("posterior_features(direct)", (B, T, L, Dm), out.cpu().numpy(), out_ref, _features32(a, b, f, g)[0], 1e-4)
    live = np.isfinite(lse_ref)
    lse = lse.cpu().numpy()
    assert not live.all() and np.all(np.isneginf(lse[~live]))
    lse32 = torch.logsumexp(torch.from_numpy(a) + torch.from_numpy(b), -1).numpy()
    judge("posterior_features(direct) lse", (B, T, L, Dm), lse[live], lse_ref[live], lse32[live], 1e-4)

    seed, B, T, L, Dm, _ = FEATURE_CASES[6]
    a, b, tl = G.ragged_posterior_inputs(seed, B, T, L)
    f, g = G.features_inputs(seed, B, L, T, Dm)
    _, lse_ref, _, gf_ref = G.posterior_ref(a, b, f, g)
    ta, tb, tg, tl32 = cu(a), cu(b), cu(g), cu(lse_ref.astype(np.float32))
    df = poisoned((B, L, Dm))
    lib.check(lib.load().dsp_posterior_features_bwd(lib.ptr(ta), lib.ptr(tb), lib.ptr(tl32), lib.ptr(tg), lib.ptr(df), B, T, L, Dm, st),
              "dsp_posterior_features_bwd")
    torch.cuda.synchronize()
    judge("posterior_features_bwd(direct)", (B, T, L, Dm), df.cpu().numpy(), gf_ref, _features32(a, b, f, g)[1], 1e-4)


def test_posterior_features_forward_at_large_sums():
    """the fused forward at |alpha + beta| ~ 1e3, same bound as dsp_posterior there.  (The backward rebuilds the posterior from the saved row
    log-sum-exp, whose own fp32 rounding at that magnitude is part of its result: not held to the fp32-implementation bound here.)"""
    B, T, L, Dm = 2, 9, 70, 2
    a, b, tl = G.ragged_posterior_inputs(59, B, T, L, 300.0)
    f, g = G.features_inputs(59, B, L, T, Dm)
    _, _, out_ref, _ = G.posterior_ref(a, b, f, g)
    with torch.no_grad():
        out = D().posterior_features(cu(a), cu(b), cu(f))
    judge("posterior_features", (B, T, L, Dm, 300.0), out.cpu().numpy(), out_ref, _features32(a, b, f, g)[0], _posterior_cap(a, b))


# ---------------------------------------------------------------- dsp_argmax_logp

def _argmax_direct(x):
    lib = LIB()
    B, L, V = x.shape
    tok, score = poisoned((B, L), torch.int32), poisoned((B, L))
    lib.check(lib.load().dsp_argmax_logp(lib.ptr(x), lib.DTYPE_CODES[str(x.dtype)], lib.ptr(tok), lib.ptr(score), B, L, V,
                                         lib.current_stream_handle()), "dsp_argmax_logp")
    torch.cuda.synchronize()
    return tok.cpu().numpy(), score.cpu().numpy()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("shape", [(3, 1400, 3), (1, 5, 1), (2, 7, 600)])
def test_argmax_logp_grid_stride_one_class_and_ties_across_waves(shape, dtype):
    """4200 rows on the 4096-workgroup grid with V smaller than a wave; one class (score exactly 0); V = 600 with bit-equal maxima in two
    waves (thread 0's merge), in one thread's two trips (the strict >) and on the wave boundary: the smaller index wins, tokens are exact"""
    B, L, V = shape
    ties = G.TIES if V == 600 else ()
    xt = torch.from_numpy(G.argmax_inputs(90 + V, B, L, V, ties)).to(dtype)
    xw = xt.float()                                           # the widened input: what the kernel is asked about
    tok_ref, sc_ref = G.argmax_logp_ref(xw.numpy())
    sc32 = torch.log_softmax(xw, -1).max(-1).values.numpy()
    name = str(dtype).replace("torch.", "")
    for how, (tok, sc) in (("direct", _argmax_direct(xt.cuda())), ("wrapper", tuple(t.cpu().numpy() for t in D().argmax_logp(xt.cuda())))):
        np.testing.assert_array_equal(tok, tok_ref)
        judge(f"argmax_logp({how})", (B, L, V, name), sc, sc_ref, sc32, 2e-6)
        for r, v1, _ in ties:
            assert tok.reshape(-1)[r] == v1
    if V == 1:
        assert np.all(sc == 0)


# ---------------------------------------------------------------- dsp_follow_path + dsp_gather_rows through graph_decode

DEC = dict(B=3, L=3073, V=11, TR=4, pad=1, out_len=np.array([3073, 2, 1], np.int64))       # 16 * L > 48 KB: the LDS opt-in of the walk


def _bits(t):
    """a CPU tensor as integers of its element width: bf16 has no numpy dtype, and a copy is compared bit for bit"""
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16).numpy()


def _decode_reference(logits, links, pad, out_len):
    """the oracle's walk on the device's own tokens and scores (dsp_argmax_logp has its test above; a score that differs in the last bit must
    not be able to pick another successor here): next by the bit-exact orc.lookahead_next, then orc.follow_path"""
    tok, sc = D().argmax_logp(cu(logits))
    tok, sc = tok.cpu().numpy(), sc.cpu().numpy()
    np.testing.assert_array_equal(tok, orc.argmax_logp(logits)[0])
    nxt = orc.lookahead_next(links, sc, 1.0)
    return (tok,) + orc.follow_path(nxt, tok, out_len, pad)


@pytest.mark.parametrize("dtype,Dm", [(torch.float32, 7), (torch.float16, 7), (torch.bfloat16, 7), (torch.float16, 24)])
def test_graph_decode_long_graph_short_graphs_and_byte_copied_rows(dtype, Dm):
    """L = 3073 (LDS opt-in), graphs of 3073, 2 and 1 vertices in one batch, feature rows of 28 and 14 bytes (the byte-copy branch of the gather)
    and of 48 bytes (16-byte copies): tokens, lengths, mask and gathered rows bit-exact against oracle.follow_path"""
    B, L, V, TR, pad, ol = (DEC[k] for k in ("B", "L", "V", "TR", "pad", "out_len"))
    logits, links, feats = G.decode_inputs(100 + Dm, B, L, V, TR, Dm, ol, pad)
    ft = torch.from_numpy(feats).to(dtype)
    tok, toks_ref, keep_ref, nf_ref = _decode_reference(logits, links, pad, ol)
    out_tok, out_feat, mask, lens = D().graph_decode(cu(logits), cu(links), ft.cuda(), cu(ol), pad, 1.0)
    fmax = int(nf_ref.max())
    assert nf_ref[0] > 100 and nf_ref[1] <= 1 and nf_ref[2] == 0
    np.testing.assert_array_equal(lens.cpu().numpy(), nf_ref)
    np.testing.assert_array_equal(out_tok.cpu().numpy(), toks_ref[:, : fmax + 1])
    np.testing.assert_array_equal(mask.cpu().numpy(), np.arange(fmax)[None, :] >= nf_ref[:, None])
    assert out_feat.dtype == dtype and tuple(out_feat.shape) == (B, fmax, Dm)
    np.testing.assert_array_equal(_bits(out_feat.cpu()), G.gather_rows_ref(_bits(ft), keep_ref, nf_ref, fmax))
    assert out_tok[2].tolist() == [int(tok[2, 0])] + [pad] * fmax


def test_graph_decode_when_every_vertex_emits_pad():
    """no vertex is kept: lengths 0, an empty feature tensor, and the tokens are the start vertex's alone"""
    B, L, V, TR, pad, ol = (DEC[k] for k in ("B", "L", "V", "TR", "pad", "out_len"))
    logits, links, feats = G.decode_inputs(111, B, L, V, TR, 7, ol, pad, all_pad=True)
    out_tok, out_feat, mask, lens = D().graph_decode(cu(logits), cu(links), cu(feats), cu(ol), pad, 1.0)
    assert lens.tolist() == [0, 0, 0] and tuple(out_feat.shape) == (B, 0, 7) and tuple(mask.shape) == (B, 0)
    assert out_tok.cpu().tolist() == [[pad]] * B


@pytest.mark.parametrize("dtype,Dm", [(torch.float32, 7), (torch.float16, 7), (torch.float16, 24)])
def test_gather_rows_zero_fills_rows_past_every_length(dtype, Dm):
    """dsp_gather_rows with Fmax beyond every n_feat on a NaN-filled output: rows k >= n_feat[b] are exactly 0 next to copied ones, in the
    byte-copy branch (28 / 14-byte rows) and the 16-byte branch (48 bytes)"""
    lib = LIB()
    B, L, V, TR, pad, ol = (DEC[k] for k in ("B", "L", "V", "TR", "pad", "out_len"))
    logits, links, feats = G.decode_inputs(100 + Dm, B, L, V, TR, Dm, ol, pad)
    ft = torch.from_numpy(feats).to(dtype)
    _, _, keep_ref, nf_ref = _decode_reference(logits, links, pad, ol)
    fmax = int(nf_ref.max()) + 3
    tf, tk, tn = ft.cuda(), cu(keep_ref), cu(nf_ref)
    out = poisoned((B, fmax, Dm), dtype)
    lib.check(lib.load().dsp_gather_rows(lib.ptr(tf), lib.DTYPE_CODES[str(dtype)], lib.ptr(tk), lib.ptr(tn), lib.ptr(out), B, L, Dm, L, fmax,
                                         lib.current_stream_handle()), "dsp_gather_rows")
    torch.cuda.synchronize()
    got = out.cpu()
    assert not torch.isnan(got).any()
    np.testing.assert_array_equal(_bits(got), G.gather_rows_ref(_bits(ft), keep_ref, nf_ref, fmax))
    for bb in range(B):
        assert torch.all(got[bb, nf_ref[bb]:] == 0) and got[bb, nf_ref[bb]:].numel() >= 3 * Dm


# ---------------------------------------------------------------- dsp_bucketize_embed_add

@pytest.mark.parametrize("case", G.BUCKETIZE_CASES)
def test_bucketize_embed_add_wide_rows_grid_stride_and_no_bins(case):
    """C = 256 (the 256-thread launch) on 4100 rows (grid-stride), C = 260 (a second trip of the channel loop), no bins at all; values on the
    bin edges, below the first, above the last, -inf and +inf.  In place through the C entry point and through the wrapper: bit-exact"""
    lib = LIB()
    seed, n, C, nb = case
    x, v, bins, emb = G.bucketize_inputs(seed, n, C, nb)
    ref = G.bucketize_embed_add_ref(x, v, bins, emb)
    tx, tv, tb, te = cu(x), cu(v), cu(bins), cu(emb)
    got = D().bucketize_embed_add(tx, tv, tb, te)
    np.testing.assert_array_equal(got.cpu().numpy(), ref)
    np.testing.assert_array_equal(tx.cpu().numpy(), x)        # the wrapper leaves x alone
    lib.check(lib.load().dsp_bucketize_embed_add(lib.ptr(tx), lib.ptr(tv), lib.ptr(tb) if nb else None, nb, lib.ptr(te), n, C,
                                                 lib.current_stream_handle()), "dsp_bucketize_embed_add")
    torch.cuda.synchronize()
    np.testing.assert_array_equal(tx.cpu().numpy(), ref)


# ---------------------------------------------------------------- dsp_dwconv_bn_silu

def _dwconv_modules(w, bw, bb, mean, var, eps, dtype, device):
    C, K = w.shape
    dw = torch.nn.Conv1d(C, C, K, padding=(K - 1) // 2, groups=C, bias=False)
    bn = torch.nn.BatchNorm1d(C, eps=eps).eval()
    with torch.no_grad():
        dw.weight.copy_(torch.from_numpy(w).unsqueeze(1)); bn.weight.copy_(torch.from_numpy(bw)); bn.bias.copy_(torch.from_numpy(bb))
        bn.running_mean.copy_(torch.from_numpy(mean)); bn.running_var.copy_(torch.from_numpy(var))
    return dw.to(device=device, dtype=dtype), bn.to(device=device, dtype=dtype)


@pytest.mark.parametrize("case", G.DWCONV_CASES)
def test_dwconv_bn_silu_against_float64(case):
    """T = 1 under a 31-tap window (every tap but one in the padding), T = 8k + 1 (a frame block of one), C = 4 (one lane), C = 260, the model's
    (C, K) = (256, 31): against the float64 chain, as accurate as torch's fp32 Conv1d -> BatchNorm1d.eval() -> SiLU, never beyond 1e-5"""
    lib = LIB()
    seed, B, T, C, K = case
    x, w, bw, bb, mean, var = G.dwconv_inputs(seed, B, T, C, K)
    eps = 1e-5
    ref = G.dwconv_bn_silu_ref(x, w, bw, bb, mean, var, eps)
    dw, bn = _dwconv_modules(w, bw, bb, mean, var, eps, torch.float32, "cpu")
    with torch.no_grad():
        ref32 = torch.nn.functional.silu(bn(dw(torch.from_numpy(x).transpose(1, 2)))).transpose(1, 2).numpy()
    tx, tw, t1, t2, t3, t4 = (cu(t) for t in (x, w, bw, bb, mean, var))
    y = poisoned((B, T, C))
    lib.check(lib.load().dsp_dwconv_bn_silu(lib.ptr(tx), lib.ptr(tw), lib.ptr(t1), lib.ptr(t2), lib.ptr(t3), lib.ptr(t4), eps, lib.ptr(y),
                                            B, T, C, K, lib.current_stream_handle()), "dsp_dwconv_bn_silu")
    torch.cuda.synchronize()
    judge("dwconv_bn_silu(direct)", (B, T, C, K), y.cpu().numpy(), ref, ref32, 1e-5)
    gdw, gbn = _dwconv_modules(w, bw, bb, mean, var, eps, torch.float32, "cuda")
    with torch.no_grad():
        got = D().dwconv_bn_silu(tx, gdw.weight, gbn)
    judge("dwconv_bn_silu(wrapper)", (B, T, C, K), got.cpu().numpy(), ref, ref32, 1e-5)


# ---------------------------------------------------------------- dsp_layer_norm

@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("case", G.LAYER_NORM_CASES)
def test_layer_norm_against_float64(case, affine):
    """one row of one lane (C = 4), C = 260 (the second register slab holds one lane), C = 2048 (the widest instance), the model's 256 on
    9 rows (a workgroup of one row), and rows of mean 100 and spread 0.01: against float64, never beyond 2e-6"""
    lib = LIB()
    seed, rows, C, mean, spread = case
    x, w, b = G.layer_norm_inputs(seed, rows, C, mean, spread)
    if not affine:
        w = b = None
    eps = 1e-5
    ref = G.layer_norm_ref(x, w, b, eps)
    ref32 = torch.nn.functional.layer_norm(torch.from_numpy(x), (C,), None if w is None else torch.from_numpy(w),
                                           None if b is None else torch.from_numpy(b), eps).numpy()
    tx = cu(x)
    tw, tb = (None, None) if w is None else (cu(w), cu(b))
    y = poisoned((rows, C))
    lib.check(lib.load().dsp_layer_norm(lib.ptr(tx), lib.ptr(tw), lib.ptr(tb), eps, lib.ptr(y), rows, C, lib.current_stream_handle()),
              "dsp_layer_norm")
    torch.cuda.synchronize()
    judge("layer_norm(direct)", (rows, C, mean, spread, "affine" if affine else "plain"), y.cpu().numpy(), ref, ref32, 2e-6)
    ln = torch.nn.LayerNorm(C, eps=eps, elementwise_affine=affine).cuda().eval()
    with torch.no_grad():
        if affine:
            ln.weight.copy_(tw); ln.bias.copy_(tb)
        got = D().layer_norm(tx, ln)
    judge("layer_norm(wrapper)", (rows, C, mean, spread, "affine" if affine else "plain"), got.cpu().numpy(), ref, ref32, 2e-6)
