"""CPU-side checks of the double-precision gather's surface (csrc/logsoftmax_gather_f64.hip): the two symbols are declared, exported and
bound, their argument validation answers without a device, and the operator still refuses CPU tensors.  No kernel is launched."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dsp_logsoftmax_gather_f64", "dsp_logsoftmax_gather_bwd_f64")
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
    text = open(os.path.join(ROOT, "include", "daspeech_dag.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    raw = ctypes.CDLL(_lib.SO_PATH)
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(\s*double\s*\*", text), f"{n} is not declared in include/daspeech_dag.h"
        assert hasattr(raw, n), f"{n} is not exported by {_lib.SO_PATH}"
        assert n in _lib.SIGNATURES
    # additive: the ABI version and the dtype codes of the fp32 entry points are what they were
    assert _lib.ABI_VERSION == 2 and lib.dsp_abi_version() == 2
    assert _lib.DTYPE_CODES == {"torch.float32": 0, "torch.float16": 1, "torch.bfloat16": 2}
    assert re.search(r"#define\s+DSP_ABI_VERSION\s+2\b", text)


def _fwd(lib, logits, idx, match, stats, B, L, V, S, ws):
    return lib.dsp_logsoftmax_gather_f64(logits, idx, S, 0, 1, match, S * L, 1, L, stats, B, L, V, S, ws, None)


def _bwd(lib, inout, idx, g, stats, B, L, V, S):
    return lib.dsp_logsoftmax_gather_bwd_f64(inout, idx, S, 0, 1, g, S * L, 1, L, stats, B, L, V, S, None)


def test_forward_argument_validation(lib):
    # host buffers only stand in for non-null pointers: every call below returns before a launch
    x = (ctypes.c_double * 16)(); i = (ctypes.c_int64 * 16)(); m = (ctypes.c_double * 16)(); st = (ctypes.c_double * 16)()
    px, pi, pm, ps = (ctypes.cast(a, ctypes.c_void_p) for a in (x, i, m, st))
    assert _fwd(lib, px, pi, pm, None, 1, 2, 0, 2, 0) == DSP_EINVAL                     # V = 0
    assert "logsoftmax_gather_f64" in _err(lib)
    assert _fwd(lib, px, pi, pm, None, -1, 2, 4, 2, 0) == DSP_EINVAL
    assert _fwd(lib, None, pi, pm, None, 1, 2, 4, 2, 0) == DSP_EINVAL                   # null logits
    assert "logsoftmax_gather_f64" in _err(lib) and "null" in _err(lib)
    assert _fwd(lib, px, None, pm, None, 1, 2, 4, 2, 0) == DSP_EINVAL
    assert _fwd(lib, px, pi, None, None, 1, 2, 4, 2, 0) == DSP_EINVAL
    assert _fwd(lib, px, pi, pm, None, 0, 2, 4, 2, 1) == DSP_OK                         # empty batch: nothing to launch
    assert _fwd(lib, None, None, None, None, 3, 0, 4, 2, 0) == DSP_OK                   # L = 0
    assert _fwd(lib, px, pi, pm, ps, 1, 2, 4, 2, 1) == DSP_EINVAL                       # softmax store AND lazy statistics
    assert "logsoftmax_gather_f64" in _err(lib)
    assert _fwd(lib, px, pi, pm, ps, 0, 2, 4, 2, 1) == DSP_EINVAL                       # ... also with nothing to launch


def test_backward_argument_validation(lib):
    x = (ctypes.c_double * 16)(); i = (ctypes.c_int64 * 16)(); g = (ctypes.c_double * 16)()
    px, pi, pg = (ctypes.cast(a, ctypes.c_void_p) for a in (x, i, g))
    assert _bwd(lib, px, pi, pg, None, 1, 2, 0, 2) == DSP_EINVAL                        # V = 0
    assert "logsoftmax_gather_bwd_f64" in _err(lib)
    assert _bwd(lib, None, pi, pg, None, 1, 2, 4, 2) == DSP_EINVAL
    assert "logsoftmax_gather_bwd_f64" in _err(lib) and "null" in _err(lib)
    assert _bwd(lib, px, None, pg, None, 1, 2, 4, 2) == DSP_EINVAL
    assert _bwd(lib, px, pi, None, None, 1, 2, 4, 2) == DSP_EINVAL
    assert _bwd(lib, px, pi, pg, None, 0, 2, 4, 2) == DSP_OK
    assert _bwd(lib, None, None, None, None, 2, 0, 4, 2) == DSP_OK


def test_operator_refuses_cpu_float64_tensors():
    import torch
    from daspeech_amd import custom_ops
    x = torch.zeros(1, 3, 5, dtype=torch.float64)
    idx = torch.zeros(1, 3, 2, dtype=torch.long)
    with pytest.raises(RuntimeError, match="expected GPU tensors"):
        custom_ops.dag_logsoftmax_gather_inplace(x, idx)
    with pytest.raises(RuntimeError, match="expected GPU tensors"):
        custom_ops.dag_logsoftmax_gather_inplace(x.clone().requires_grad_().clone(), idx)


def test_float64_stays_out_of_the_fp32_launch_helpers():
    import torch
    from daspeech_amd import _lib
    import sys
    import daspeech_amd.custom_ops  # noqa: F401
    dl = sys.modules["daspeech_amd.custom_ops.dag_loss"]           # (the package attribute of that name is the function)
    assert "torch.float64" not in _lib.DTYPE_CODES
    assert callable(dl._lsg64_forward) and callable(dl._lsg64_backward)
    with pytest.raises(KeyError):                                        # the fp32 backward helper has no code for a double buffer
        dl._lsg_backward(torch.zeros(1, 2, 3, dtype=torch.float64), torch.zeros(1, 2, 1, dtype=torch.long), torch.zeros(1, 2, 1))
