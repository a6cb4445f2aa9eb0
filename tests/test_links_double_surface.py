"""CPU-side checks of the double-precision link producer's surface (csrc/extract_links_f64.hip): the two symbols are declared with double*
for every floating pointer, exported and bound; the ABI version and the dtype codes are what they were; argument validation answers without
a device; the operators still refuse CPU tensors; and the two float64 formulations of tests/util_links_ref.py agree on every case the GPU
tests run.  No kernel is launched.

The last test prints, per GPU case, the largest disagreement of the two double formulations and the miss of the fp32 formulation (the same
band form on the inputs narrowed to fp32: what the operators computed for float64 callers before the double kernels) — the figures that
justify the GPU bounds of tests/test_gpu_links_double.py: its value bound (1e-12) must stay >= 10x the double-versus-double disagreement and
<= 1e-3 x the fp32 miss, which is asserted here for every case, the wide-window one included."""
import ctypes
import os
import re

import pytest
import torch

from tests.util_links_ref import CASES, TILED, links_band, links_loop, make_case, max_abs_diff, max_tol_ratio, reference, run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dsp_extract_links_f64", "dsp_extract_links_bwd_f64")
DSP_OK, DSP_EINVAL = 0, -1
VALUE_BOUND = 1e-12                      # rtol = atol of the GPU tests on links and stats
GRAD_RTOL, GRAD_ATOL = 1e-9, 1e-12       # of the GPU tests on dq, dk, d log_gates (the figures of tests/test_gpu_lsg_double.py)


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
        m = re.search(r"\bint\s+" + n + r"\s*\((.*?)\)\s*;", text, flags=re.S)
        assert m, f"{n} is not declared in include/daspeech_decode.h"
        assert hasattr(raw, n), f"{n} is not exported by {_lib.SO_PATH}"
        assert n in _lib.SIGNATURES
        args = [a.strip() for a in m.group(1).split(",")]
        ptrs = [a for a in args if "*" in a]
        # every floating pointer is a double*; the only other pointer is the int64 out_len
        assert [a for a in ptrs if not re.search(r"\bdouble\s*\*", a)] == ["const int64_t* out_len"], (n, ptrs)
        assert not any(re.search(r"\bfloat\b", a) for a in args), (n, args)
        assert "double scale" in args
        # the binding passes the scale as a double and as many arguments as the header declares
        res, argtypes = _lib.SIGNATURES[n]
        assert len(argtypes) == len(args) and argtypes.count(ctypes.c_double) == 1 and ctypes.c_float not in argtypes
    assert len(_lib.SIGNATURES["dsp_extract_links_f64"][1]) == 14 and len(_lib.SIGNATURES["dsp_extract_links_bwd_f64"][1]) == 18
    # additive: the ABI version and the dtype codes of the fp32 entry points are what they were (no double code)
    assert _lib.ABI_VERSION == 2 and lib.dsp_abi_version() == 2
    assert _lib.DTYPE_CODES == {"torch.float32": 0, "torch.float16": 1, "torch.bfloat16": 2}
    assert re.search(r"#define\s+DSP_ABI_VERSION\s+2\b", dag)


def _bufs(n):
    # host buffers only stand in for non-null pointers: every call below returns before a launch
    arrs = [(ctypes.c_double * 16)() for _ in range(n)]
    return arrs, [ctypes.cast(a, ctypes.c_void_p) for a in arrs]


BAD_SIZES = (
    # B, L, H, CK, TR, what the message names
    (1, 8, 4, 64, 3, "heads"),           # H != 8
    (1, 8, 16, 64, 3, "heads"),
    (1, 8, 8, 48, 3, "head width"),      # CK outside {32, 64, 128}
    (1, 8, 8, 256, 3, "head width"),
    (1, 8, 8, 64, 0, "TR"),              # TR < 1
    (1, 8, 8, 64, -2, "TR"),
    (1, 8, 8, 64, 8, "TR"),              # TR > L-1
    (1, 1, 8, 64, 1, "TR"),              # a one-vertex graph has no window
    (-1, 8, 8, 64, 3, "sizes"),
    (1, 0, 8, 64, 1, "sizes"),
)


def test_forward_argument_validation(lib):
    keep, (q, k, g, ol, bias, links, stats) = _bufs(7)
    f = lib.dsp_extract_links_f64
    for B, L, Hh, CK, TR, word in BAD_SIZES:
        assert f(q, k, g, ol, bias, links, stats, B, L, Hh, CK, TR, 0.125, None) == DSP_EINVAL, (B, L, Hh, CK, TR)
        assert "extract_links_f64" in _err(lib) and word in _err(lib), _err(lib)
    for i in (0, 1, 2, 3, 5):                                                       # q, k, log_gates, out_len, links
        args = [q, k, g, ol, None, links, None]                                     # (dist_bias and stats may be NULL: inference)
        args[i] = None
        assert f(*args, 1, 8, 8, 64, 3, 0.125, None) == DSP_EINVAL
        assert "extract_links_f64" in _err(lib) and "null" in _err(lib)
    assert f(q, k, g, ol, None, links, None, 0, 8, 8, 64, 3, 0.125, None) == DSP_OK      # empty batch: nothing to launch
    assert f(None, None, None, None, None, None, None, 0, 8, 8, 64, 7, 0.125, None) == DSP_OK


def test_backward_argument_validation(lib):
    keep, (q, k, g, ol, bias, links, G, stats, dq, dk, dg) = _bufs(11)
    f = lib.dsp_extract_links_bwd_f64
    for B, L, Hh, CK, TR, word in BAD_SIZES:
        assert f(q, k, g, ol, bias, links, G, stats, dq, dk, dg, B, L, Hh, CK, TR, 0.125, None) == DSP_EINVAL, (B, L, Hh, CK, TR)
        assert "extract_links_bwd_f64" in _err(lib) and word in _err(lib), _err(lib)
    for i in (0, 1, 2, 3, 5, 6, 7, 8, 9, 10):                                       # everything but dist_bias; the backward needs the stats
        args = [q, k, g, ol, None, links, G, stats, dq, dk, dg]
        args[i] = None
        assert f(*args, 1, 8, 8, 64, 3, 0.125, None) == DSP_EINVAL
        assert "extract_links_bwd_f64" in _err(lib) and "null" in _err(lib)
    assert f(q, k, g, ol, None, links, G, stats, dq, dk, dg, 0, 8, 8, 64, 3, 0.125, None) == DSP_OK
    assert f(*([None] * 11), 0, 8, 8, 64, 7, 0.125, None) == DSP_OK


def test_operators_refuse_cpu_float64_tensors():
    from daspeech_amd import decode_ops
    q = torch.zeros(1, 5, 8, 32, dtype=torch.float64)
    g = torch.zeros(1, 5, 8, dtype=torch.float64)
    ol = torch.tensor([5])
    with pytest.raises(RuntimeError, match="expected GPU tensors"):
        decode_ops.extract_links(q, q, g, ol, 3)
    with pytest.raises(RuntimeError, match="expected GPU tensors"):
        decode_ops.extract_links_autograd(q.clone().requires_grad_(), q.float(), g, ol, 3)
    assert decode_ops._ExtractLinksF64Fn is not decode_ops._ExtractLinksFn
    assert decode_ops._links_f64(q.float(), q, g.float()) and decode_ops._links_f64(q.float(), q.float(), g)
    assert not decode_ops._links_f64(q.float(), q.half(), g.bfloat16())


@pytest.mark.parametrize("use_bias", [False, True])
@pytest.mark.parametrize("case", CASES + [TILED], ids=lambda c: "B%d-L%d-CK%d-TR%d" % c[:4])
def test_the_two_reference_formulations_agree(case, use_bias):
    """Prints the figures the GPU bounds rest on and asserts the margins on both sides of them."""
    c, band = reference(case, use_bias)
    loop = run(links_loop, c, use_bias)
    fp32 = run(links_band, c, use_bias, torch.float32)
    assert band["links"].dtype == torch.float64 and loop["links"].dtype == torch.float64 and fp32["links"].dtype == torch.float32
    B, L, CK, TR, lens = case
    # the structure both formulations must share: -inf exactly at i+d+1 >= out_len, every row with a successor a distribution
    i = torch.arange(L).view(1, L, 1); d = torch.arange(TR).view(1, 1, TR)
    invalid = (i + d + 1) >= torch.tensor(lens).view(B, 1, 1).clamp(max=L)
    assert torch.equal(torch.isneginf(band["links"]), invalid) and torch.equal(torch.isneginf(loop["links"]), invalid)
    rows = ~invalid.all(-1)
    assert float(torch.logsumexp(band["links"][rows], -1).abs().max()) <= 1e-12
    assert torch.equal(torch.isneginf(band["stats"][..., 0]), ~rows.unsqueeze(-1).expand(-1, -1, 8))
    assert bool((band["stats"][..., 1][~rows] == 0).all())
    dd_val = max(max_abs_diff(loop["links"], band["links"]), max_abs_diff(loop["stats"], band["stats"]))
    miss_val = max_abs_diff(fp32["links"], band["links"])
    dd_grad = max(max_tol_ratio(loop[n], band[n], GRAD_RTOL, GRAD_ATOL) for n in ("dq", "dk", "dg"))
    miss_grad = max(max_tol_ratio(fp32[n], band[n], GRAD_RTOL, GRAD_ATOL) for n in ("dq", "dk", "dg"))
    dd_gabs = max(float((loop[n] - band[n]).abs().max()) for n in ("dq", "dk", "dg"))
    miss_gabs = max(float((fp32[n].double() - band[n]).abs().max()) for n in ("dq", "dk", "dg"))
    print(f"case {case} bias {use_bias}: values: double vs double {dd_val:.2e}, fp32 miss {miss_val:.2e};  gradients: double vs double "
          f"{dd_gabs:.2e} ({dd_grad:.2e} of the bound), fp32 miss {miss_gabs:.2e} ({miss_grad:.2e} of the bound)")
    assert VALUE_BOUND >= 10 * dd_val, "the GPU value bound is not 10x above the disagreement of two double formulations"
    assert VALUE_BOUND <= 1e-3 * miss_val, "the GPU value bound is not 1000x below an fp32 computation's miss"
    assert dd_grad <= 0.1, "the GPU gradient bound is not 10x above the disagreement of two double formulations"
    assert miss_grad > 1.0, "an fp32 computation would pass the GPU gradient bound"
