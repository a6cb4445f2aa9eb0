"""CPU-side checks of the double-precision posterior's surface (csrc/posterior_f64.hip): the three symbols are declared with double*,
exported and bound, their argument validation answers without a device, the operators still refuse CPU tensors, and the numpy float64
reference the GPU tests use (tests/util_posterior_ref.py) agrees with an independent double implementation (torch's CPU two-step and its
autograd) and with the project's fp32 oracle.  No kernel is launched."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import dag_oracle as orc
from tests.util_posterior_ref import CASES, LARGE, make_case, max_finite_abs, posterior_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dsp_posterior_f64", "dsp_posterior_features_f64", "dsp_posterior_features_bwd_f64")
DSP_OK, DSP_EINVAL = 0, -1


@pytest.fixture(scope="module")
def lib():
    from daspeech_amd import build, _lib
    build.build()
    return _lib.load()


def _err(lib):
    return lib.dsp_last_error().decode("utf-8", "replace")


def test_symbols_are_declared_exported_and_bound(lib):
    from daspeech_amd import _lib
    text = open(os.path.join(ROOT, "include", "daspeech_decode.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    dag = open(os.path.join(ROOT, "include", "daspeech_dag.h")).read()
    raw = ctypes.CDLL(_lib.SO_PATH)
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(\s*const\s+double\s*\*", text), f"{n} is not declared with double* in include/daspeech_decode.h"
        assert hasattr(raw, n), f"{n} is not exported by {_lib.SO_PATH}"
        assert n in _lib.SIGNATURES
    # every pointer argument of the three is a double*
    for n in NAMES:
        args = re.search(r"\bint\s+" + n + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
        ptrs = [a for a in args.split(",") if "*" in a]
        assert ptrs and all(re.search(r"\bdouble\s*\*", a) for a in ptrs), (n, ptrs)
    # additive: the ABI version and the dtype codes of the fp32 entry points are what they were
    assert _lib.ABI_VERSION == 2 and lib.dsp_abi_version() == 2
    assert _lib.DTYPE_CODES == {"torch.float32": 0, "torch.float16": 1, "torch.bfloat16": 2}
    assert re.search(r"#define\s+DSP_ABI_VERSION\s+2\b", dag)


def _bufs(n=4):
    # host buffers only stand in for non-null pointers: every call below returns before a launch
    arrs = [(ctypes.c_double * 16)() for _ in range(n)]
    return arrs, [ctypes.cast(a, ctypes.c_void_p) for a in arrs]


def test_posterior_argument_validation(lib):
    keep, (pa, pb, ps, _) = _bufs()
    f = lib.dsp_posterior_f64
    assert f(pa, pb, ps, 1, 0, 4, None) == DSP_EINVAL                                # T = 0
    assert "posterior_f64" in _err(lib)
    assert f(pa, pb, ps, 1, 2, 0, None) == DSP_EINVAL                                # L = 0
    assert f(pa, pb, ps, -1, 2, 4, None) == DSP_EINVAL
    assert f(None, pb, ps, 1, 2, 4, None) == DSP_EINVAL
    assert "posterior_f64" in _err(lib) and "null" in _err(lib)
    assert f(pa, None, ps, 1, 2, 4, None) == DSP_EINVAL
    assert f(pa, pb, None, 1, 2, 4, None) == DSP_EINVAL
    assert f(pa, pb, ps, 0, 2, 4, None) == DSP_OK                                    # empty batch: nothing to launch
    assert f(None, None, None, 0, 2, 4, None) == DSP_OK


def test_posterior_features_argument_validation(lib):
    keep, (pa, pb, pf, po) = _bufs()
    f = lib.dsp_posterior_features_f64
    for bad in ((1, 0, 4, 2), (1, 2, 0, 2), (1, 2, 4, 0), (-1, 2, 4, 2)):           # T, L, D below 1; negative batch
        assert f(pa, pb, pf, po, None, *bad, None) == DSP_EINVAL
        assert "posterior_features_f64" in _err(lib)
    for args in ((None, pb, pf, po), (pa, None, pf, po), (pa, pb, None, po), (pa, pb, pf, None)):
        assert f(*args, None, 1, 2, 4, 3, None) == DSP_EINVAL                        # (odd D is a valid size: the null pointer is what is refused)
        assert "posterior_features_f64" in _err(lib) and "null" in _err(lib)
    assert f(pa, pb, pf, po, None, 0, 2, 4, 1, None) == DSP_OK                       # empty batch, lse NULL, D = 1
    assert f(None, None, None, None, None, 0, 2, 4, 2, None) == DSP_OK


def test_posterior_features_bwd_argument_validation(lib):
    keep, (pa, pb, pl, pg) = _bufs()
    keep2, (pd, _, _, _) = _bufs()
    f = lib.dsp_posterior_features_bwd_f64
    for bad in ((1, 0, 4, 2), (1, 2, 0, 2), (1, 2, 4, 0), (-1, 2, 4, 2)):
        assert f(pa, pb, pl, pg, pd, *bad, None) == DSP_EINVAL
        assert "posterior_features_bwd_f64" in _err(lib)
    for args in ((None, pb, pl, pg, pd), (pa, None, pl, pg, pd), (pa, pb, None, pg, pd), (pa, pb, pl, None, pd), (pa, pb, pl, pg, None)):
        assert f(*args, 1, 2, 4, 3, None) == DSP_EINVAL                              # the backward needs the row statistics: lse NULL is refused
        assert "posterior_features_bwd_f64" in _err(lib) and "null" in _err(lib)
    assert f(pa, pb, pl, pg, pd, 0, 2, 4, 1, None) == DSP_OK
    assert f(None, None, None, None, None, 0, 2, 4, 2, None) == DSP_OK


def test_operators_refuse_cpu_float64_tensors():
    import torch
    from daspeech_amd import decode_ops
    a = torch.zeros(1, 3, 5, dtype=torch.float64)
    f = torch.zeros(1, 5, 4, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="expected GPU tensors"):
        decode_ops.posterior(a, a)
    with pytest.raises(RuntimeError, match="expected GPU tensors"):
        decode_ops.posterior_features(a, a, f)
    with pytest.raises(RuntimeError, match="expected GPU tensors"):
        decode_ops.expect_features(a, a.float(), f.requires_grad_())
    assert decode_ops._PosteriorFeaturesF64Fn is not decode_ops._PosteriorFeaturesFn


def _torch_two_step(c):
    """torch's CPU double two-step and its autograd: another summation order, another exp / log"""
    import torch
    a, b = torch.from_numpy(c["alpha"]), torch.from_numpy(c["beta"])
    f = torch.from_numpy(c["features"]).requires_grad_()
    s = a + b
    p = torch.nan_to_num(torch.exp(s - torch.logsumexp(s, -1, keepdim=True)))
    out = p @ f
    (out * torch.from_numpy(c["grad_out"])).sum().backward()
    return p.numpy(), out.detach().numpy(), f.grad.numpy()


@pytest.mark.parametrize("seed,B,T,L,TR,D", CASES)
def test_reference_agrees_with_torch_cpu_double(seed, B, T, L, TR, D):
    c = make_case(seed, B, T, L, TR, D)
    p, lse, out, gf = posterior_ref(c["alpha"], c["beta"], c["features"], c["grad_out"])
    tp, tout, tgf = _torch_two_step(c)
    assert p.dtype == np.float64 and not np.isnan(p).any()
    tl = c["tgt_len"]
    for bb in range(B):
        assert (p[bb, tl[bb]:] == 0).all() and np.isneginf(lse[bb, tl[bb]:]).all() and (out[bb, tl[bb]:] == 0).all()
        np.testing.assert_allclose(p[bb, :tl[bb]].sum(-1), 1.0, rtol=0, atol=1e-12)
        assert np.isfinite(lse[bb, :tl[bb]]).all()
    print(f"max finite |alpha+beta| {max_finite_abs(c['alpha'], c['beta']):.0f}; reference vs torch CPU double: p {np.abs(p - tp).max():.2e}  "
          f"p@f {np.abs(out - tout).max():.2e}  bwd {np.abs(gf - tgf).max():.2e}")
    np.testing.assert_allclose(p, tp, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(out, tout, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(gf, tgf, rtol=1e-12, atol=1e-12)


def test_reference_agrees_with_torch_cpu_double_on_the_large_graph():
    """|alpha + beta| reaches 1.26e3: the bound follows its unit in the last place, as the GPU test's does"""
    seed, B, T, L, TR, D = LARGE
    assert (T - 1) * TR + 1 >= L
    c = make_case(seed, B, T, L, TR, D)
    M = max_finite_abs(c["alpha"], c["beta"])
    assert M > 1000
    p, lse, out, gf = posterior_ref(c["alpha"], c["beta"], c["features"], c["grad_out"])
    tp, tout, tgf = _torch_two_step(c)
    print(f"M {M:.0f}, spacing {np.spacing(M):.2e}; p {np.abs(p - tp).max():.2e}  p@f {np.abs(out - tout).max():.2e}  bwd {np.abs(gf - tgf).max():.2e}")
    np.testing.assert_allclose(p, tp, rtol=0, atol=16 * np.spacing(M))
    np.testing.assert_allclose(out, tout, rtol=0, atol=16 * np.spacing(M) * max(1.0, np.abs(c["features"]).max()))
    np.testing.assert_allclose(gf, tgf, rtol=0, atol=16 * np.spacing(M) * max(1.0, np.abs(c["grad_out"]).max()))


@pytest.mark.parametrize("seed,B,T,L,TR,D", CASES[:2])
def test_reference_agrees_with_the_fp32_oracle(seed, B, T, L, TR, D):
    """the fp32 oracle on fp32 alpha / beta / features against the double reference on their exact widening, at the tolerance
    tests/test_gpu_decode_ops.py holds the fp32 kernels to against that oracle"""
    c = make_case(seed, B, T, L, TR, D)
    a32 = orc.dag_alpha(c["match"], c["links"], c["out_len"], c["tgt_len"], np.float32)
    b32 = orc.dag_beta(c["match"], c["links"], c["out_len"], c["tgt_len"], np.float32)
    f32 = c["features"].astype(np.float32)
    score32, ex32 = orc.posterior_expect(a32, b32, f32)
    p, _, out, _ = posterior_ref(a32.astype(np.float64), b32.astype(np.float64), f32.astype(np.float64))
    np.testing.assert_allclose(score32, p, rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(ex32, out, rtol=1e-4, atol=1e-5)
