"""GPU: decode_ops.path_features_autograd on what torch accepts but a fresh allocation never is (tests/util_views.py): features as a column
slice of a larger NaN-filled buffer (a row pitch, and with it a batch pitch, read in place), as a row-and-column slice (two pitches) and at
an odd storage offset (both answered "not served" and settled by a dense copy inside the raising function), a transposed path (read through
its strides), an expanded (stride-0) and a row-pitched gradient (read in place).  Each view gives the bits of the dense call.  The test
registers the operator's public names in the table of tests/test_gpu_views.py (imported as pytest itself imports it, so the table filled is
the table read), where test_every_public_operator_has_a_row looks for them."""
import pytest
import torch

import test_gpu_views as TV
from tests import util_path_features_ref as U
from tests import util_views as V

pytestmark = pytest.mark.gpu

DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
B, L, C = 3, 70, 264                                             # two 64-vertex chunks, five backward tiles; C no multiple of a wave's quads


def _feature_views(x):
    """name -> (view of x, what path_features_served answers)"""
    out = {}
    wide = torch.full((B, L, C + 16), float("nan"), dtype=x.dtype, device=x.device)      # what lies around the slice is never to be read
    v = wide[:, :, :C]
    v.copy_(x)
    assert v.stride() == (L * (C + 16), C + 16, 1)
    out["column_slice_of_larger_buffer"] = (v, True)
    wide = torch.full((B, L + 3, C + 16), float("nan"), dtype=x.dtype, device=x.device)
    v = wide[:, :L, :C]
    v.copy_(x)
    assert v.stride() == ((L + 3) * (C + 16), C + 16, 1)
    out["row_and_column_slice"] = (v, False)
    v = V.at_offset(x)
    assert v.data_ptr() % 16 and v.is_contiguous()
    out["odd_storage_offset"] = (v, False)
    v = V.via_transpose(x)
    assert not v.is_contiguous()
    out["transposed_features"] = (v, False)
    return out


@TV.covers("path_features_autograd", "path_features_served", "path_features_checked", "set_path_features_hip")
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_views_agree_with_the_dense_call(dtype):
    from daspeech_amd import decode_ops
    dt = DTYPES[dtype]
    x = U.make_features(B, L, C, dt, 11, "cuda")
    path = U.random_path(B, L, 2).cuda()
    W = int((path[:, 1:] >= 0).sum(1).max()) + 2
    dy = torch.randn((1, W, C), generator=torch.Generator().manual_seed(6)).to(dt).cuda().repeat(B, 1, 1)      # constant along the batch
    ref = U.backward_of(U.reference, x, path, W, dy)
    dense = U.backward_of(decode_ops.path_features_autograd, x, path, W, dy)
    assert all(torch.equal(u, v) for u, v in zip(dense, ref))

    def same(got, name):
        for k, u, v in zip(("out", "pad", "n", "dfeatures"), got, dense):
            assert u.shape == v.shape and torch.equal(u, v), (name, k)

    for name, (v, served) in _feature_views(x).items():
        assert decode_ops.path_features_served(v, path, W) is served, name
        same(U.backward_of(decode_ops.path_features_autograd, v, path, W, dy), name)
        if served:
            with torch.no_grad():                                            # what the criterion calls after `served` said yes: the same launch
                res = decode_ops.path_features_checked(v, path, W)
            assert all(torch.equal(a, b) for a, b in zip(res, dense[:3])), name
            old = decode_ops.set_path_features_hip(False)
            try:
                assert old is True and decode_ops.path_features_served(v, path, W) is False
            finally:
                assert decode_ops.set_path_features_hip(old) is False
    pt = V.via_transpose(path)
    assert not pt.is_contiguous() and pt.stride() == (1, B)
    assert decode_ops.path_features_served(x, pt, W) is True
    same(U.backward_of(decode_ops.path_features_autograd, x, pt, W, dy), "transposed_path")
    for name, g in (("expanded_dy", V.expanded(dy, 0)), ("row_pitched_dy", V.row_pitched(dy, 16 // dy.element_size())),
                    ("row_pitched_dy_off_grid", V.row_pitched(dy, 1)), ("dy_at_odd_offset", V.at_offset(dy)),
                    ("transposed_dy", V.via_transpose(dy))):
        assert not (g.is_contiguous() and g.data_ptr() % 16 == 0), name
        same(U.backward_of(decode_ops.path_features_autograd, x, path, W, g), name)
    assert V.expanded(dy, 0).stride(0) == 0
