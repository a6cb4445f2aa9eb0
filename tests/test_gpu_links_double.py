"""decode_ops.extract_links / extract_links_autograd on float64 q, k or log_gates (csrc/extract_links_f64.hip) against the float64 band
reference of tests/util_links_ref.py (torch on CPU, gradients by CPU autograd).

Tolerances: rtol 1e-12 / atol 1e-12 on links and stats, rtol 1e-9 / atol 1e-12 on dq, dk and d log_gates (the figures tests/test_gpu_lsg_double.py
holds the double gather to).  On these cases two independent double formulations of the reference differ by <= 1e-15 on values (3.6e-15 on the
700-vertex window) and <= 3.2e-14 on gradients, an fp32 computation misses by >= 1.2e-7 on values and 4e-8 .. 1.8e-5 on gradients:
tests/test_links_double_surface.py prints the figures and asserts the margins (the value bound >= 10x the former, <= 1e-3 x the latter), the
wide-window case included — it needs no bound of its own."""
from types import SimpleNamespace

import pytest
import torch

from tests.util_links_ref import CASES, H, TILED, links_band, make_case, masked_loss, reference, run

pytestmark = pytest.mark.gpu

FWD_BIT, BWD_BIT, WALK_BIT = 1 << 7, 1 << 8, 1 << 9      # dsp_extract_links_debug_ran: double forward, double backward, window walked in tiles
IDS = lambda c: "B%d-L%d-CK%d-TR%d" % c[:4]


def dev():
    return torch.device("cuda:0")


def D():
    from daspeech_amd import decode_ops
    return decode_ops


def _ran():
    from daspeech_amd import _lib
    torch.cuda.synchronize()
    return int(_lib.load().dsp_extract_links_debug_ran())


def _close(got, want, rtol, atol, name=""):
    torch.testing.assert_close(got.cpu(), want, rtol=rtol, atol=atol, msg=lambda m: f"{name}: {m}")


def _device_run(c, use_bias, q=None, k=None, lg=None):
    """links (autograd), dq, dk, dg, links (inference), stats of the operators on the case's tensors (or the given replacements)"""
    olen = c["olen"].to(dev())
    bias = c["bias"].to(dev()) if use_bias else None
    q, k, lg = ((c[n] if t is None else t).to(dev()).clone().requires_grad_() for n, t in (("q", q), ("k", k), ("lg", lg)))
    links = D().extract_links_autograd(q, k, lg, olen, c["TR"], bias)
    masked_loss(links, c["w"].to(dev())).backward()
    with torch.no_grad():
        inf_links = D().extract_links(q, k, lg, olen, c["TR"], bias)
    stats = D()._links_f64_forward(q, k, lg, olen, c["TR"], bias, True)[6]           # dsp_extract_links_f64 with a stats pointer
    return links.detach(), q.grad, k.grad, lg.grad, inf_links, stats


def _check_against_reference(case, use_bias, want_bits):
    c, ref = reference(case, use_bias)
    _ran()
    links, dq, dk, dg, inf_links, stats = _device_run(c, use_bias)
    bits = _ran()
    assert links.dtype == torch.float64 and inf_links.dtype == torch.float64 and stats.dtype == torch.float64
    assert dq.dtype == torch.float64 and dk.dtype == torch.float64 and dg.dtype == torch.float64
    assert tuple(links.shape) == tuple(ref["links"].shape) and tuple(stats.shape) == tuple(ref["stats"].shape)
    assert bits == want_bits, bin(bits)                                              # the double kernels, and bits 0..6 (fp32 families) clear
    assert torch.equal(inf_links, links), "inference and training forward are the same kernel"
    neg = torch.isneginf(ref["links"])
    assert torch.equal(torch.isneginf(links).cpu(), neg) and not torch.isnan(links).any()
    fin = ~neg
    err = {n: float((g.cpu() - ref[n]).abs().max()) for n, g in (("dq", dq), ("dk", dk), ("dg", dg))}
    print(f"case {case} bias {use_bias}: max abs error links {float((links.cpu()[fin] - ref['links'][fin]).abs().max()):.3e}  grads {err}")
    _close(links.cpu()[fin], ref["links"][fin], 1e-12, 1e-12, "links")
    # every row with a successor is a distribution over its valid transitions
    rows = fin.any(-1)
    assert float(torch.logsumexp(links.cpu()[rows], -1).abs().max()) <= 1e-12
    # stats: (window max, log of the window's sum); (-inf, 0) for a row without a successor
    st, st_ref = stats.cpu(), ref["stats"]
    assert torch.equal(torch.isneginf(st[..., 0]), torch.isneginf(st_ref[..., 0])) and not torch.isnan(st).any()
    live = torch.isfinite(st_ref[..., 0])
    assert bool((st[..., 1][~live] == 0).all())
    _close(st[..., 0][live], st_ref[..., 0][live], 1e-12, 1e-12, "stats max")
    _close(st[..., 1][live], st_ref[..., 1][live], 1e-12, 1e-12, "stats log-sum")
    for n, g in (("dq", dq), ("dk", dk), ("dg", dg)):
        _close(g, ref[n], 1e-9, 1e-12, n)
    # rows at or beyond the graph get exact zeros (the buffers come from torch.empty)
    for b, n in enumerate(case[4]):
        assert not dq[b, n:].any() and not dk[b, n:].any() and not dg[b, n:].any()


@pytest.mark.parametrize("use_bias", [False, True])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_values_stats_and_gradients_match_the_float64_reference(case, use_bias):
    _check_against_reference(case, use_bias, FWD_BIT | BWD_BIT)


def test_window_walked_in_tiles():
    """a 699-successor window is beyond one LDS tile of the double kernels (384 partners): online soft-max state first, emission second, the
    backward's contractions accumulated across the tiles — the library reports the walk in bit 9"""
    _check_against_reference(TILED, True, FWD_BIT | BWD_BIT | WALK_BIT)


def test_mixed_dtypes():
    case = CASES[2]
    c, _ = reference(case, True)
    # fp32 q with float64 k (and fp16 gates): double links; each gradient in its input's dtype, the double result rounded once
    q32, lg16 = c["q"].float(), c["lg"].half()
    wide = dict(c, q=q32.double(), lg=lg16.double())
    ref = run(links_band, wide, True)
    _ran()
    links, dq, dk, dg, inf_links, _ = _device_run(c, True, q=q32, lg=lg16)
    assert _ran() == FWD_BIT | BWD_BIT
    assert links.dtype == torch.float64 and inf_links.dtype == torch.float64
    assert dq.dtype == torch.float32 and dk.dtype == torch.float64 and dg.dtype == torch.float16
    lw, dqw, dkw, dgw, _, _ = _device_run(wide, True)
    assert torch.equal(links, lw) and torch.equal(dk, dkw) and torch.equal(dq, dqw.float()) and torch.equal(dg, dgw.half())
    fin = torch.isfinite(ref["links"])
    assert torch.equal(torch.isfinite(links).cpu(), fin)
    _close(links.cpu()[fin], ref["links"][fin], 1e-12, 1e-12, "links")
    for n, g in (("dq", dqw), ("dk", dkw), ("dg", dgw)):
        _close(g, ref[n], 1e-9, 1e-12, n)
    # float64 gates alone select the double path; a float32 dist_bias is widened
    _ran()
    l2 = D().extract_links(q32.to(dev()), c["k"].float().to(dev()), c["lg"].to(dev()), c["olen"].to(dev()), c["TR"], c["bias"].float().to(dev()))
    assert l2.dtype == torch.float64 and _ran() == FWD_BIT
    # fp16 grad_links into the double backward (the Function's own backward: autograd would have cast it): widened, never narrowed
    olen = c["olen"].to(dev())
    qd, kd, gd, ol, bias, lk, stats = D()._links_f64_forward(c["q"].to(dev()), c["k"].to(dev()), c["lg"].to(dev()), olen, c["TR"], c["bias"].to(dev()), True)
    G16 = c["w"].half().to(dev())
    ctx = SimpleNamespace(saved_tensors=(qd, kd, gd, ol, lk, stats, bias), TR=c["TR"], has_bias=True, in_dtypes=(torch.float64,) * 3)
    dq, dk, dg = D()._ExtractLinksF64Fn.backward(ctx, G16)[:3]
    assert _ran() == FWD_BIT | BWD_BIT
    assert dq.dtype == torch.float64 and dk.dtype == torch.float64 and dg.dtype == torch.float64
    ref16 = run(links_band, dict(c, w=c["w"].half().double()), True)
    for n, g in (("dq", dq), ("dk", dk), ("dg", dg)):
        _close(g, ref16[n], 1e-9, 1e-12, n + " (fp16 grad_links)")


def test_fp32_inputs_keep_the_fp32_kernels():
    case = CASES[1]
    c, ref = reference(case, True)
    olen, bias = c["olen"].to(dev()), c["bias"].float().to(dev())
    res = []
    _ran()
    for _ in range(2):
        q, k, lg = (c[n].float().to(dev()).requires_grad_() for n in ("q", "k", "lg"))
        links = D().extract_links_autograd(q, k, lg, olen, c["TR"], bias)
        masked_loss(links, c["w"].float().to(dev())).backward()
        with torch.no_grad():
            inf_links = D().extract_links(q, k, lg, olen, c["TR"], bias)
        assert links.dtype == torch.float32 and inf_links.dtype == torch.float32 and q.grad.dtype == torch.float32
        res.append((links.detach(), inf_links))
    bits = _ran()
    assert bits and not bits & (FWD_BIT | BWD_BIT | WALK_BIT), bin(bits)
    for x, y in zip(*res):
        assert torch.equal(x, y)
    # half-precision inputs stay on the fp32 path as well
    assert D().extract_links(c["q"].half().to(dev()), c["k"].bfloat16().to(dev()), c["lg"].float().to(dev()), olen, c["TR"]).dtype == torch.float32
    assert not _ran() & (FWD_BIT | BWD_BIT)
    # and the fp32 result is the double one at fp32 accuracy
    fin = torch.isfinite(ref["links"])
    torch.testing.assert_close(res[0][0].cpu()[fin].double(), ref["links"][fin], rtol=1e-5, atol=2e-5)


def test_two_runs_of_the_backward_give_the_same_bits():
    c, _ = reference(CASES[1], True)
    a, b = _device_run(c, True), _device_run(c, True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_gradcheck():
    B, L, CK, TR = 1, 5, 32, 3
    g = torch.Generator().manual_seed(7)
    q, k = (torch.randn(B, L, H, CK, dtype=torch.float64, generator=g).mul(0.5).to(dev()).requires_grad_() for _ in range(2))
    lg = torch.log_softmax(torch.randn(B, L, H, dtype=torch.float64, generator=g), -1).to(dev()).requires_grad_()
    olen = torch.tensor([5], device=dev())

    def f(q, k, lg):
        links = D().extract_links_autograd(q, k, lg, olen, TR)
        return links.masked_fill(~torch.isfinite(links), 0.0)

    assert torch.autograd.gradcheck(f, (q, k, lg), eps=1e-6, atol=1e-7, rtol=1e-5)


def test_chain_links_to_dag_loss():
    """q, k, gates float64 -> extract_links_autograd -> custom_ops.dag_loss with a float64 match -> backward, against the CPU reference links fed
    to dag_double's torch band DP under CPU autograd"""
    from daspeech_amd import custom_ops
    from daspeech_amd.custom_ops import dag_double
    B, T, L, CK, TR = 2, 5, 14, 32, 6
    c = make_case((B, L, CK, TR, (14, 9)))
    tlen = torch.tensor([5, 3])
    g = torch.Generator().manual_seed(11)
    match = torch.randn(B, T, L, dtype=torch.float64, generator=g)
    wl = torch.tensor([1.0, 0.7], dtype=torch.float64)
    # CPU reference
    q, k, lg, m = (t.clone().requires_grad_() for t in (c["q"], c["k"], c["lg"], match))
    links, _ = links_band(q, k, lg, c["olen"], TR, c["bias"])
    loss_ref = dag_double._pick_loss(dag_double.alpha_table(m, links, c["olen"], tlen), c["olen"], tlen)
    assert torch.isfinite(loss_ref).all()
    (loss_ref * wl).sum().backward()
    # the device chain
    _ran()
    qd, kd, gd, md = (t.to(dev()).clone().requires_grad_() for t in (c["q"], c["k"], c["lg"], match))
    lk = D().extract_links_autograd(qd, kd, gd, c["olen"].to(dev()), TR, c["bias"].to(dev()))
    loss = custom_ops.dag_loss(md, lk, c["olen"].to(dev()), tlen.to(dev()))
    assert lk.dtype == torch.float64 and loss.dtype == torch.float64
    (loss * wl.to(dev())).sum().backward()
    assert _ran() == FWD_BIT | BWD_BIT
    print(f"chain: loss error {float((loss.detach().cpu() - loss_ref.detach()).abs().max()):.3e}  "
          f"dq {float((qd.grad.cpu() - q.grad).abs().max()):.3e}  dk {float((kd.grad.cpu() - k.grad).abs().max()):.3e}  dg {float((gd.grad.cpu() - lg.grad).abs().max()):.3e}")
    _close(loss.detach(), loss_ref.detach(), 1e-12, 1e-11, "loss")
    for n, a, b in (("dq", qd.grad, q.grad), ("dk", kd.grad, k.grad), ("dg", gd.grad, lg.grad), ("dmatch", md.grad, m.grad)):
        assert a.dtype == torch.float64
        _close(a, b, 1e-9, 1e-12, n)


@pytest.mark.parametrize("TRmax", [32, 99999])
def test_model_in_double(TRmax):
    """DAGDecoder(...).double(): the fused branch (the double kernels) against the torch formulation, both float64; the fp32 decoder keeps fp32 links"""
    from daspeech_amd.models.daspeech import BOS, DAGDecoder, DEFAULT_ARGS, EOS, PAD, UNK
    torch.manual_seed(11)
    a = SimpleNamespace(**{**DEFAULT_ARGS, "max_transition_length": TRmax, "decoder_layers": 0})
    dec = DAGDecoder(a).to(dev()).double().train()
    B, L = 3, 70
    lens = [70, 51, 2]
    prev = torch.full((B, L), PAD, dtype=torch.long, device=dev())
    for b, n in enumerate(lens):
        prev[b, :n] = UNK; prev[b, 0] = BOS; prev[b, n - 1] = EOS
    feats0 = torch.randn(B, L, a.decoder_embed_dim, dtype=torch.float64, device=dev())
    wgt, res = None, {}
    for fused in (True, False):
        dec.fused_links = fused
        dec.zero_grad(set_to_none=True)
        feats = feats0.clone().requires_grad_()
        _ran()
        links = dec.extract_links(feats, prev)
        if wgt is None:
            wgt = torch.randn_like(links)
        fin = torch.isfinite(links)
        loss = (links.masked_fill(~fin, 0.0) * wgt).sum() + 0.3 * torch.logsumexp(links.masked_fill(~fin, -1e4), -1).sum()
        loss.backward()
        assert _ran() == (FWD_BIT | BWD_BIT if fused else 0)
        res[fused] = (links.detach(), feats.grad.detach(), {n: p.grad.detach().clone() for n, p in dec.named_parameters() if p.grad is not None})
    (l1, g1, p1), (l0, g0, p0) = res[True], res[False]
    assert l1.dtype == torch.float64 and l0.dtype == torch.float64 and tuple(l1.shape) == (B, L, min(TRmax, L - 1))
    assert torch.equal(torch.isneginf(l1), torch.isneginf(l0))
    f = torch.isfinite(l0)
    torch.testing.assert_close(l1[f], l0[f], rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(g1, g0, rtol=1e-9, atol=1e-12)
    assert set(p1) == set(p0) and {"query_linear.weight", "key_linear.weight", "gate_linear.weight"} <= set(p1)
    for n in p0:
        assert p1[n].dtype == torch.float64
        torch.testing.assert_close(p1[n], p0[n], rtol=1e-9, atol=1e-12, msg=lambda m: f"{n}: {m}")
    with torch.no_grad():
        dec.fused_links = True
        assert dec.extract_links(feats0, prev).dtype == torch.float64 and _ran() == FWD_BIT
        dec32 = dec.float()
        for fused in (True, False):
            dec32.fused_links = fused
            assert dec32.extract_links(feats0.float(), prev).dtype == torch.float32
        assert not _ran() & (FWD_BIT | BWD_BIT)


def test_matrix_core_kernels_against_the_native_double_result():
    """The fp32 matrix-core link kernels (xl_mfma pinned to 1) on a 1024-vertex full window against the double kernels on the same fp32 inputs
    widened — the ground truth that fits on the device — at the tolerance tests/test_gpu_decode_ops.py::
    test_matrix_core_extract_links_equal_the_fp32_kernels holds between the fp32 families: <= 1e-5 of the largest value."""
    from daspeech_amd import _lib
    B, L, CK, TR = 2, 1024, 64, 1023
    g = torch.Generator().manual_seed(9)
    q0, k0 = (torch.randn(B, L, H, CK, generator=g).mul(0.5).to(dev()) for _ in range(2))
    g0 = torch.log_softmax(torch.randn(B, L, H, generator=g), -1).to(dev())
    w = torch.randn(B, L, TR, generator=g).to(dev())
    olen = torch.tensor([1024, 700], device=dev())
    bias = (-0.02 * torch.arange(TR).float()).to(dev())

    def fwd_bwd(cast):
        q, k, lg = (cast(t).clone().requires_grad_() for t in (q0, k0, g0))
        links = D().extract_links_autograd(q, k, lg, olen, TR, bias)
        masked_loss(links, w).backward()
        return links.detach(), q.grad, k.grad, lg.grad

    _ran()
    ref = fwd_bwd(lambda t: t.double())
    assert _ran() == FWD_BIT | BWD_BIT | WALK_BIT
    try:
        _lib.set_option("xl_mfma", 1)
        got = fwd_bwd(lambda t: t)
        bits = _ran()
    finally:
        _lib.set_option("xl_mfma", -1)
    assert bits & 0b100 and bits & 0b1100000 and not bits & (0b0011011 | FWD_BIT | BWD_BIT), bin(bits)
    for name, a, b in zip(("links", "dq", "dk", "dgate"), got, ref):
        assert a.dtype == torch.float32 and b.dtype == torch.float64
        assert torch.equal(torch.isneginf(a), torch.isneginf(b)), name
        f = torch.isfinite(b)
        assert torch.isfinite(a[f]).all(), name
        sc = max(1.0, float(b[f].abs().max()))
        err = float((a[f].double() - b[f]).abs().max())
        print(f"matrix-core vs double, {name}: {err:.3e} (largest value {sc:.3e})")
        assert err <= 1e-5 * sc, (name, err, sc)
