"""decode_ops.posterior / posterior_features / expect_features on float64 alpha / beta (csrc/posterior_f64.hip) against the numpy float64
restatement of the reference step (tests/util_posterior_ref.py) on alpha / beta from the fp64 oracle DP.

Tolerances are the ones tests/test_gpu_lsg_double.py holds the double gather to: rtol 1e-12 / atol 1e-12 on values (score, out, lse), rtol 1e-9 /
atol 1e-12 on the gradient to the features.  On these cases two independent double implementations (the reference and torch's CPU two-step)
differ by <= 7.2e-14 (tests/test_posterior_double_surface.py prints the figures); an fp32 computation misses by >= 1.5e-6.  On the large graph
|alpha + beta| reaches 1.2e3 and the bound follows its unit in the last place: atol = 16 * spacing(M) * max(1, |f|max), rtol 0."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import dag_oracle as orc
from tests.util_inputs import make_dag_inputs
from tests.util_posterior_ref import CASES, LARGE, make_case, max_finite_abs, posterior_ref

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def D():
    from daspeech_amd import decode_ops
    return decode_ops


def ops():
    from daspeech_amd import custom_ops
    return custom_ops


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev())


def _fn_name(out):
    """name of the autograd node that produced `out`, looking through a slice"""
    fn = out.grad_fn
    while fn is not None and "PosteriorFeatures" not in type(fn).__name__:
        fn = fn.next_functions[0][0] if fn.next_functions else None
    return type(fn).__name__ if fn is not None else ""


def _lse_of(a, b):
    """the row statistics the forward keeps for the backward, through the C entry point"""
    from daspeech_amd import _lib
    lib = _lib.load()
    B, T, L = a.shape
    f = torch.zeros((B, L, 1), dtype=torch.float64, device=a.device)
    out = torch.empty((B, T, 1), dtype=torch.float64, device=a.device)
    lse = torch.empty((B, T), dtype=torch.float64, device=a.device)
    with torch.cuda.device(a.device):
        _lib.check(lib.dsp_posterior_features_f64(_lib.ptr(a), _lib.ptr(b), _lib.ptr(f), _lib.ptr(out), _lib.ptr(lse), B, T, L, 1,
                                                  _lib.current_stream_handle()), "dsp_posterior_features_f64")
    torch.cuda.synchronize()
    return lse


def _check_dead_rows(score, out, lse, tl):
    for bb in range(len(tl)):
        assert (score[bb, tl[bb]:] == 0).all() and (out[bb, tl[bb]:] == 0).all() and np.isneginf(lse[bb, tl[bb]:]).all()
        assert np.isfinite(lse[bb, :tl[bb]]).all()
    assert not np.isnan(score).any() and not np.isnan(out).any() and not np.isnan(lse).any()


@pytest.mark.parametrize("seed,B,T,L,TR,Dm", CASES)
def test_values_match_the_float64_reference(seed, B, T, L, TR, Dm):
    c = make_case(seed, B, T, L, TR, Dm)
    p_ref, lse_ref, out_ref, gf_ref = posterior_ref(c["alpha"], c["beta"], c["features"], c["grad_out"])
    a, b = _t(c["alpha"]), _t(c["beta"])
    f = _t(c["features"]).requires_grad_()
    score = D().posterior(a, b)
    assert score.dtype == torch.float64 and tuple(score.shape) == (B, T, L)
    out = D().posterior_features(a, b, f)
    assert out.dtype == torch.float64 and tuple(out.shape) == (B, T, Dm) and "F64" in _fn_name(out)
    (gf,) = torch.autograd.grad(out, [f], grad_outputs=_t(c["grad_out"]))
    assert gf.dtype == torch.float64 and tuple(gf.shape) == (B, L, Dm)
    lse = _lse_of(a, b).cpu().numpy()
    sc, o, g = score.cpu().numpy(), out.detach().cpu().numpy(), gf.cpu().numpy()
    fin = np.isfinite(lse_ref)
    print(f"max finite |alpha+beta| {max_finite_abs(c['alpha'], c['beta']):.0f}: max abs error score {np.abs(sc - p_ref).max():.3e}  out "
          f"{np.abs(o - out_ref).max():.3e}  lse {np.abs(lse[fin] - lse_ref[fin]).max():.3e}  grad {np.abs(g - gf_ref).max():.3e}")
    _check_dead_rows(sc, o, lse, c["tgt_len"])
    assert np.array_equal(np.isneginf(lse), np.isneginf(lse_ref))
    np.testing.assert_allclose(sc, p_ref, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(o, out_ref, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(lse[fin], lse_ref[fin], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(g, gf_ref, rtol=1e-9, atol=1e-12)
    # expect_features drops row 0 of the same result
    ex = D().expect_features(a, b, f)
    assert ex.dtype == torch.float64 and torch.equal(ex.detach(), out.detach()[:, 1:, :]) and "F64" in _fn_name(ex)


def test_large_graph():
    seed, B, T, L, TR, Dm = LARGE
    c = make_case(seed, B, T, L, TR, Dm)
    M = max_finite_abs(c["alpha"], c["beta"])
    assert M > 1000
    p_ref, lse_ref, out_ref, gf_ref = posterior_ref(c["alpha"], c["beta"], c["features"], c["grad_out"])
    a, b = _t(c["alpha"]), _t(c["beta"])
    f = _t(c["features"]).requires_grad_()
    score = D().posterior(a, b).cpu().numpy()
    out = D().posterior_features(a, b, f)
    (gf,) = torch.autograd.grad(out, [f], grad_outputs=_t(c["grad_out"]))
    lse = _lse_of(a, b).cpu().numpy()
    o, g = out.detach().cpu().numpy(), gf.cpu().numpy()
    fin = np.isfinite(lse_ref)
    u = 16 * np.spacing(M)
    print(f"M {M:.0f}, 16 spacings {u:.3e}: max abs error score {np.abs(score - p_ref).max():.3e}  out {np.abs(o - out_ref).max():.3e}  "
          f"lse {np.abs(lse[fin] - lse_ref[fin]).max():.3e}  grad {np.abs(g - gf_ref).max():.3e}")
    _check_dead_rows(score, o, lse, c["tgt_len"])
    np.testing.assert_allclose(score, p_ref, rtol=0, atol=u)
    np.testing.assert_allclose(lse[fin], lse_ref[fin], rtol=0, atol=u)
    np.testing.assert_allclose(o, out_ref, rtol=0, atol=u * max(1.0, np.abs(c["features"]).max()))
    np.testing.assert_allclose(g, gf_ref, rtol=0, atol=u * max(1.0, np.abs(c["grad_out"]).max()))


def test_no_gradient_contract_beta_zero_is_the_softmax_of_alpha():
    seed, B, T, L, TR, Dm = CASES[3]
    c = make_case(seed, B, T, L, TR, Dm)
    zero = np.zeros_like(c["beta"])
    p_ref, _, out_ref, _ = posterior_ref(c["alpha"], zero, c["features"])
    al = c["alpha"]
    with np.errstate(invalid="ignore"):
        m = al.max(-1, keepdims=True)
        e = np.where(np.isfinite(m), np.exp(al - np.where(np.isfinite(m), m, 0.0)), 0.0)
        soft = np.where(np.isfinite(m), e / np.where(np.isfinite(m), e.sum(-1, keepdims=True), 1.0), 0.0)
    np.testing.assert_allclose(p_ref, soft, rtol=1e-12, atol=1e-12)
    a = _t(c["alpha"])
    score = D().posterior(a, torch.zeros_like(a))
    out = D().posterior_features(a, torch.zeros_like(a), _t(c["features"]))
    np.testing.assert_allclose(score.cpu().numpy(), soft, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(out.cpu().numpy(), out_ref, rtol=1e-12, atol=1e-12)


def test_chain_on_the_device():
    """float64 logits -> dag_logsoftmax_gather_inplace -> dag_loss_with_alpha_beta -> expect_features -> backward, against the numpy chain"""
    seed, Bn, T, L, TR, V, Dm = 5, 3, 40, 700, 32, 96, 96
    _, links32, ol, tl = make_dag_inputs(seed, Bn, T, L, TR)
    links = links32.astype(np.float64)
    rng = np.random.default_rng(1000 + seed)
    x = rng.standard_normal((Bn, L, V)) * 3
    tgt = rng.integers(0, V, (Bn, T))
    feats = rng.standard_normal((Bn, L, Dm))
    w = rng.standard_normal((Bn, T - 1, Dm))
    # the numpy chain
    idx = np.broadcast_to(tgt[:, None, :], (Bn, L, T))
    m = np.ascontiguousarray(orc.logsoftmax_gather(x, idx, np.float64).transpose(0, 2, 1))
    al = orc.dag_alpha(m, links, ol, tl, np.float64)
    be = orc.dag_beta(m, links, ol, tl, np.float64)
    wfull = np.concatenate([np.zeros((Bn, 1, Dm)), w], axis=1)
    _, _, out_ref, gf_ref = posterior_ref(al, be, feats, wfull)
    # the device chain
    xt = _t(x).requires_grad_()
    work = xt.clone()
    tg, kt, olt, tlt = _t(tgt), _t(links), _t(ol), _t(tl)
    _, match = ops().dag_logsoftmax_gather_inplace(work, tg.unsqueeze(1).expand(-1, L, -1))
    m_all = match.transpose(1, 2)
    loss, (a, b) = ops().dag_loss_with_alpha_beta(m_all, kt, olt, tlt)
    assert a.dtype == torch.float64 and b.dtype == torch.float64 and loss.dtype == torch.float64
    f = _t(feats).requires_grad_()
    ex = D().expect_features(a, b, f)
    assert ex.dtype == torch.float64 and tuple(ex.shape) == (Bn, T - 1, Dm)
    assert _fn_name(ex) == "_PosteriorFeaturesF64FnBackward"
    (ex * _t(w)).sum().backward()
    o, g = ex.detach().cpu().numpy(), f.grad.cpu().numpy()
    print(f"chain: max abs error expect {np.abs(o - out_ref[:, 1:]).max():.3e}  grad {np.abs(g - gf_ref).max():.3e}")
    np.testing.assert_allclose(o, out_ref[:, 1:], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(g, gf_ref, rtol=1e-9, atol=1e-12)
    assert f.grad.dtype == torch.float64


def test_mixed_dtypes():
    seed, B, T, L, TR, Dm = CASES[3]
    c = make_case(seed, B, T, L, TR, Dm)
    a = _t(c["alpha"])
    # float32 beta: its exact widening is what the double kernels see
    b32 = _t(c["beta"].astype(np.float32))
    p_ref, _, out_ref, gf_ref = posterior_ref(c["alpha"], c["beta"].astype(np.float32).astype(np.float64), c["features"], c["grad_out"])
    for al, be in ((a, b32), (b32, a)):                                             # either one may be the double tensor
        score = D().posterior(al, be)
        assert score.dtype == torch.float64
        np.testing.assert_allclose(score.cpu().numpy(), p_ref, rtol=1e-12, atol=1e-12)
    f64 = _t(c["features"]).requires_grad_()
    out64 = D().posterior_features(a, b32, f64)
    np.testing.assert_allclose(out64.detach().cpu().numpy(), out_ref, rtol=1e-12, atol=1e-12)
    # float32 / float16 features: the features' dtype comes back, the values are the double result of the widened features rounded once
    beta_w = c["beta"].astype(np.float32).astype(np.float64)
    for dt in (torch.float32, torch.float16):
        fl = _t(c["features"]).to(dt).requires_grad_()
        go = _t(c["grad_out"]).to(dt)
        out = D().posterior_features(a, b32, fl)
        assert out.dtype == dt and "F64" in _fn_name(out)
        (g,) = torch.autograd.grad(out, [fl], grad_outputs=go)
        assert g.dtype == dt
        fw = fl.detach().double().requires_grad_()
        wide = D().posterior_features(a, b32, fw)
        (gw,) = torch.autograd.grad(wide, [fw], grad_outputs=go.double())
        assert wide.dtype == torch.float64 and gw.dtype == torch.float64
        assert torch.equal(out.detach(), wide.detach().to(dt)) and torch.equal(g, gw.to(dt))
        _, _, o_ref, g_ref = posterior_ref(c["alpha"], beta_w, fw.detach().cpu().numpy(), go.double().cpu().numpy())
        np.testing.assert_allclose(wide.detach().cpu().numpy(), o_ref, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(gw.cpu().numpy(), g_ref, rtol=1e-9, atol=1e-12)
    # a strided grad_out through autograd
    wide = torch.zeros((B, T, 2 * Dm + 1), dtype=torch.float64, device=dev())
    go = wide[:, :, 1::2]
    go.copy_(_t(c["grad_out"]))
    assert not go.is_contiguous()
    (g,) = torch.autograd.grad(out64, [f64], grad_outputs=go)
    np.testing.assert_allclose(g.cpu().numpy(), gf_ref, rtol=1e-9, atol=1e-12)
    # the Function's own backward: a float32, strided gradient is widened and made contiguous (autograd may already have cast it)
    go32 = torch.zeros((B, T, 2 * Dm + 1), dtype=torch.float32, device=dev())[:, :, 1::2]
    go32.copy_(_t(c["grad_out"]))
    assert not go32.is_contiguous()
    _, _, _, gf32 = posterior_ref(c["alpha"], beta_w, None, go32.double().cpu().numpy())
    ctx = SimpleNamespace(saved_tensors=(a, b32.double(), _lse_of(a, b32.double())), fdtype=torch.float64)
    _, _, g = D()._PosteriorFeaturesF64Fn.backward(ctx, go32)
    assert g.dtype == torch.float64
    np.testing.assert_allclose(g.cpu().numpy(), gf32, rtol=1e-9, atol=1e-12)


def test_fp32_inputs_keep_the_fp32_kernels_bit_for_bit():
    """Two code paths, one function: fp32 alpha / beta / features launch exactly dsp_posterior / dsp_posterior_features[_bwd], and the double
    kernels on their exact widening agree with them at the fp32 test's tolerance."""
    from daspeech_amd import _lib
    B, T, L, TR, Dm = 3, 21, 70, 16, 640
    match, links, ol, tl = make_dag_inputs(23, B, T, L, TR)
    a32 = orc.dag_alpha(match, links, ol, tl, np.float32)
    b32 = orc.dag_beta(match, links, ol, tl, np.float32)
    f32 = np.random.default_rng(1).standard_normal((B, L, Dm)).astype(np.float32)
    w32 = np.random.default_rng(2).standard_normal((B, T, Dm)).astype(np.float32)
    ta, tb, w = _t(a32), _t(b32), _t(w32)
    f = _t(f32).requires_grad_()
    out = D().posterior_features(ta, tb, f)
    assert out.dtype == torch.float32 and _fn_name(out) == "_PosteriorFeaturesFnBackward"
    (g,) = torch.autograd.grad(out, [f], grad_outputs=w)
    score = D().posterior(ta, tb)
    assert score.dtype == torch.float32
    # what the fp32 entry points give when called directly on the same buffers
    lib = _lib.load()
    with torch.cuda.device(dev()):
        st = _lib.current_stream_handle()
        s_raw, o_raw = torch.empty_like(ta), torch.empty((B, T, Dm), dtype=torch.float32, device=dev())
        lse = torch.empty((B, T), dtype=torch.float32, device=dev())
        g_raw = torch.empty((B, L, Dm), dtype=torch.float32, device=dev())
        fd = f.detach()
        _lib.check(lib.dsp_posterior(_lib.ptr(ta), _lib.ptr(tb), _lib.ptr(s_raw), B, T, L, st), "dsp_posterior")
        _lib.check(lib.dsp_posterior_features(_lib.ptr(ta), _lib.ptr(tb), _lib.ptr(fd), _lib.ptr(o_raw), _lib.ptr(lse), B, T, L, Dm, st), "dsp_posterior_features")
        _lib.check(lib.dsp_posterior_features_bwd(_lib.ptr(ta), _lib.ptr(tb), _lib.ptr(lse), _lib.ptr(w), _lib.ptr(g_raw), B, T, L, Dm, st),
                   "dsp_posterior_features_bwd")
    torch.cuda.synchronize()
    assert torch.equal(score, s_raw) and torch.equal(out.detach(), o_raw) and torch.equal(g, g_raw)
    # the exact widening through the double kernels
    f64 = f.detach().double().requires_grad_()
    out64 = D().posterior_features(ta.double(), tb.double(), f64)
    assert out64.dtype == torch.float64 and "F64" in _fn_name(out64)
    (g64,) = torch.autograd.grad(out64, [f64], grad_outputs=w.double())
    np.testing.assert_allclose(out.detach().cpu().numpy(), out64.detach().cpu().numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(g.cpu().numpy(), g64.cpu().numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(score.cpu().numpy(), D().posterior(ta.double(), tb.double()).cpu().numpy(), rtol=1e-4, atol=1e-5)
    # half-precision alpha / beta stay on the fp32 path as well
    assert D().posterior(ta.half(), tb.half()).dtype == torch.float32


def test_two_calls_give_the_same_bits():
    for case in (CASES[1], CASES[3]):
        c = make_case(*case)
        a, b, go = _t(c["alpha"]), _t(c["beta"]), _t(c["grad_out"])
        res = []
        for _ in range(2):
            f = _t(c["features"]).requires_grad_()
            out = D().posterior_features(a, b, f)
            (g,) = torch.autograd.grad(out, [f], grad_outputs=go)
            res.append((D().posterior(a, b), out.detach().clone(), g.clone()))
        for x, y in zip(*res):
            assert torch.equal(x, y)


def test_null_lse_gives_the_same_output():
    """lse may be NULL in dsp_posterior_features_f64: the product pass then builds the row statistics itself"""
    from daspeech_amd import _lib
    lib = _lib.load()
    for case in (CASES[1], CASES[3]):
        c = make_case(*case)
        B, T, L, Dm = case[1], case[2], case[3], case[5]
        a, b, f = _t(c["alpha"]), _t(c["beta"]), _t(c["features"])
        want = D().posterior_features(a, b, f)
        out = torch.full((B, T, Dm), float("nan"), dtype=torch.float64, device=dev())
        with torch.cuda.device(dev()):
            _lib.check(lib.dsp_posterior_features_f64(_lib.ptr(a), _lib.ptr(b), _lib.ptr(f), _lib.ptr(out), None, B, T, L, Dm,
                                                      _lib.current_stream_handle()), "dsp_posterior_features_f64")
        torch.cuda.synchronize()
        assert torch.equal(out, want)


def test_no_score_tensor_is_allocated():
    """At (2, 64, 2048, ., 64) a [B,T,L] tensor of doubles is 2 MiB.  Forward plus backward may allocate the outputs ([B,T,D] and lse, under
    70 KB), the gradient the caller asked for ([B,L,D] doubles: 2 MiB here, as large as a score tensor, so it is taken out of the count) and
    the small autograd temporaries of `(out * w).sum()` — the saved tensors are the inputs.  Checked on the peak and, stricter, on the total
    of all bytes allocated in between (a temporary that is freed again still counts there)."""
    B, T, L, Dm = 2, 64, 2048, 64
    gen = torch.Generator(device=dev()).manual_seed(3)
    a = torch.randn((B, T, L), dtype=torch.float64, device=dev(), generator=gen) * 20
    b = torch.randn((B, T, L), dtype=torch.float64, device=dev(), generator=gen) * 20
    f = torch.randn((B, L, Dm), dtype=torch.float64, device=dev(), generator=gen).requires_grad_()
    w = torch.randn((B, T, Dm), dtype=torch.float64, device=dev(), generator=gen)
    D().posterior_features(a, b, f.detach())                                         # library load and first-launch allocations
    torch.cuda.synchronize()
    score_bytes = B * T * L * 8
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    total0 = torch.cuda.memory_stats()["allocated_bytes.all.allocated"]
    out = D().posterior_features(a, b, f)
    torch.cuda.synchronize()
    fwd_rise = torch.cuda.max_memory_allocated() - base
    (out * w).sum().backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    total = torch.cuda.memory_stats()["allocated_bytes.all.allocated"] - total0
    grad_bytes = f.grad.numel() * 8
    print(f"score tensor {score_bytes} B; forward peak rise {fwd_rise} B; forward + backward peak rise {rise} B, all bytes allocated {total} B, "
          f"of which the returned gradient {grad_bytes} B")
    assert fwd_rise < score_bytes
    assert rise - grad_bytes < score_bytes
    assert total - grad_bytes < score_bytes
    p_ref, _, out_ref, gf_ref = posterior_ref(a.cpu().numpy(), b.cpu().numpy(), f.detach().cpu().numpy(), w.cpu().numpy())
    np.testing.assert_allclose(out.detach().cpu().numpy(), out_ref, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(f.grad.cpu().numpy(), gf_ref, rtol=1e-9, atol=1e-12)
