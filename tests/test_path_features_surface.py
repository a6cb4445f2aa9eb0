"""CPU: the surface of the path-features operator (daspeech_amd.decode_ops) — what it declines without a GPU, and in which order it looks."""
import pytest
import torch

from tests import util_path_features_ref as U


def _case(dtype=torch.float32):
    return U.make_features(3, 20, 8, dtype, 1), U.random_path(3, 20, 2)


def test_cpu_tensors_float64_and_the_switch_are_not_served():
    from daspeech_amd import decode_ops
    x, path = _case()
    assert decode_ops.PATH_FEATURES_HIP is True
    assert decode_ops.path_features_served(x, path, 12) is False                       # CPU tensors
    assert decode_ops.path_features_served(x.double(), path, 12) is False              # float64 is refused, never narrowed
    assert "float64" in decode_ops._path_features_problem(x.double(), path, 12)
    old = decode_ops.set_path_features_hip(False)
    try:
        assert old is True and decode_ops.PATH_FEATURES_HIP is False
        assert decode_ops.path_features_served(x, path, 12) is False
    finally:
        assert decode_ops.set_path_features_hip(old) is False
    assert decode_ops.PATH_FEATURES_HIP is True


def test_raising_function_refuses_cpu_tensors():
    from daspeech_amd import decode_ops
    x, path = _case()
    with pytest.raises(RuntimeError, match="path_features_autograd") as e:
        decode_ops.path_features_autograd(x, path, 12)
    assert decode_ops._NOT_GPU in str(e.value)


def test_a_cpu_tensor_is_refused_before_its_strides_are_looked_at():
    """a layout reason would send the raising function into a dense copy first: the device comes before it"""
    from daspeech_amd import decode_ops
    x, path = _case()
    xt = x.transpose(1, 2).contiguous().transpose(1, 2)
    assert not xt.is_contiguous() and xt.stride(2) != 1
    assert decode_ops._path_features_problem(xt, path, 12) == decode_ops._NOT_GPU
    assert decode_ops._path_features_problem(xt, path.t().contiguous().t(), 12) == decode_ops._NOT_GPU


@pytest.mark.parametrize("bad,what", [
    (lambda x, p: (x[0], p, 4), "[B, L, C]"),
    (lambda x, p: (x, p[:, :5], 4), "int64 or int32"),
    (lambda x, p: (x, p.to(torch.int16), 4), "int64 or int32"),
    (lambda x, p: (x, p, -1), "width"),
    (lambda x, p: (x, p, torch.tensor(4)), "width"),
    (lambda x, p: (x[:, :, :6], p, 4), "multiple of 4"),
    (lambda x, p: (x.half()[:, :, :4], p, 4), "multiple of 8"),
])
def test_shape_and_dtype_reasons_come_before_the_device(bad, what):
    from daspeech_amd import decode_ops
    x, path = _case()
    assert what in decode_ops._path_features_problem(*bad(x, path))


def test_constants_mirror_the_header():
    import os
    import re
    from daspeech_amd import decode_ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "daspeech_decode.h")).read()
    for name in ("TILE_W", "TILE_L", "MAX_L"):
        (v,) = re.findall(rf"#define DSP_PATH_FEATURES_{name} (\d+)", text)
        assert int(v) == getattr(decode_ops, f"PATH_FEATURES_{name}")
