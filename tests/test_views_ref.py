"""tests/util_views.py on the CPU: every helper keeps the values bit for bit and has exactly the layout property it claims (data pointer
residue, strides, is_contiguous()).  CPU allocations of torch are 64-byte aligned, so the residues can be checked without a device."""
import pytest
import torch

from tests import util_views as V

DTYPES = [torch.float32, torch.float16, torch.bfloat16, torch.float64, torch.int64, torch.int32, torch.uint8, torch.bool]
SHAPES = [(7,), (3, 5), (2, 5, 8), (1, 6, 4), (2, 3, 4, 6)]


def _values(shape, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-50, 50, shape, generator=g)
    if dtype == torch.bool:
        return x > 0
    if dtype == torch.uint8:
        return x.abs().to(dtype)
    return (x.to(torch.float64) / 4).to(dtype) if dtype.is_floating_point else x.to(dtype)


def _same_bits(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype and a.device == b.device
    if a.dtype == torch.bool:
        return torch.equal(a, b)
    w = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return torch.equal(a.contiguous().view(w), b.contiguous().view(w))


def test_fresh_cpu_allocations_are_on_the_grid():
    for dtype in DTYPES:
        assert torch.empty(37, dtype=dtype).data_ptr() % 64 == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_at_offset(dtype):
    es = torch.empty((), dtype=dtype).element_size()
    for shape in SHAPES:
        t = _values(shape, dtype)
        ks = [None] + [k for k in range(1, 2 * (16 // es)) if (k * es) % 16]
        for k in ks:
            v = V.at_offset(t, k)
            kk = V.default_offset(dtype) if k is None else k
            assert v.data_ptr() % 16 == (kk * es) % 16 != 0
            assert v.data_ptr() % es == 0                                 # the element alignment holds
            assert v.is_contiguous() and v.stride() == t.contiguous().stride()
            assert _same_bits(v, t)
        for k in (0, 16 // es, -1):
            with pytest.raises(ValueError):
                V.at_offset(t, k)
    # a non-contiguous input comes back contiguous, with its values
    t = _values((4, 6), dtype).t()
    v = V.at_offset(t)
    assert v.is_contiguous() and _same_bits(v, t.contiguous()) and v.data_ptr() % 16


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_row_pitched(dtype):
    for shape in SHAPES[1:]:
        t = _values(shape, dtype, 1)
        C = shape[-1]
        for pad in (1, 4, 16 // t.element_size()):
            v = V.row_pitched(t, pad)
            assert v.stride(-1) == 1 and v.stride(-2) == C + pad
            for d in range(v.dim() - 2):                                  # the outer dimensions stay dense over the pitched rows
                assert v.stride(d) == v.stride(d + 1) * v.shape[d + 1]
            rows = t.numel() // C
            assert v.is_contiguous() == (rows == 1)
            assert v.data_ptr() % 16 == 0
            assert _same_bits(v, t)
    with pytest.raises(ValueError):
        V.row_pitched(_values((7,), dtype), 4)
    with pytest.raises(ValueError):
        V.row_pitched(_values((3, 5), dtype), 0)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_column_slice(dtype):
    for shape in SHAPES:
        t = _values(shape, dtype, 2)
        C, es = shape[-1], t.element_size()
        v = V.column_slice(t)
        assert v.stride(-1) == 1 and _same_bits(v, t)
        assert v.data_ptr() % 16 == (C * es) % 16                         # a = C columns in
        assert v.storage_offset() == C
        if t.dim() >= 2:
            assert v.stride(-2) == 3 * C
            assert v.is_contiguous() == (t.numel() // C == 1)
        v = V.column_slice(t, before=1, after=0)
        assert v.storage_offset() == 1 and v.data_ptr() % 16 == es % 16 and _same_bits(v, t)
        if t.dim() >= 2:
            assert v.stride(-2) == C + 1
        with pytest.raises(ValueError):
            V.column_slice(t, before=0, after=0)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_via_transpose(dtype):
    for shape in SHAPES[1:]:
        t = _values(shape, dtype, 3)
        v = V.via_transpose(t)
        assert _same_bits(v, t) and v.data_ptr() % 16 == 0
        assert v.stride(-2) == 1 and v.stride(-1) == shape[-2]
        assert v.is_contiguous() == (shape[-1] == 1 or shape[-2] == 1)
        assert not v.is_contiguous()                                      # every shape of this list has two long last dimensions
    t = _values((2, 5, 8), dtype, 4)
    v = V.via_transpose(t, 0, 1)
    assert v.stride() == (8, 16, 1) and not v.is_contiguous() and _same_bits(v, t)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_expanded(dtype):
    row = _values((1, 5, 8), dtype, 5)
    t = row.expand(3, 5, 8).contiguous()
    assert V.constant_dim(t) == 0
    v = V.expanded(t)
    assert v.stride() == (0, 8, 1) and not v.is_contiguous() and _same_bits(v, t)
    col = _values((3, 1, 8), dtype, 6).expand(3, 5, 8).contiguous()
    v = V.expanded(col)
    assert v.stride() == (8, 0, 1) and not v.is_contiguous() and _same_bits(v, col)
    ones = torch.ones(4, 6).to(dtype)                                     # what a plain .sum() sends back: constant everywhere
    v = V.expanded(ones, 1)
    assert v.stride() == (1, 0) and _same_bits(v, ones)
    g = torch.zeros(2, 3, requires_grad=True)
    (gr,) = torch.autograd.grad((g * 1.0).sum(), g)
    assert V.constant_dim(gr) == 0
    varying = torch.arange(24).reshape(2, 3, 4).to(torch.float32 if dtype == torch.bool else dtype)
    assert V.constant_dim(varying) is None
    with pytest.raises(ValueError):
        V.expanded(varying)
    with pytest.raises(ValueError):
        V.expanded(t, 1)                                                  # t varies along dimension 1


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_every_variant_names_and_values(dtype):
    t = _values((2, 5, 8), dtype, 7)
    got = dict(V.every_variant(t))
    assert list(got) == ["offset", "pitched", "pitched1", "colslice", "transposed"]
    for name, v in got.items():
        assert _same_bits(v, t), name
        assert not (v.is_contiguous() and v.data_ptr() % 16 == 0), name    # none of them is what a fresh allocation gives
    es = t.element_size()
    assert got["pitched"].stride(-2) == 8 + 16 // es and (got["pitched"].stride(-2) * es) % 16 == (8 * es) % 16
    assert got["pitched1"].stride(-2) == 9
    one = dict(V.every_variant(_values((7,), dtype, 8)))
    assert list(one) == ["offset", "colslice"]
    const = _values((1, 8), dtype, 9).expand(5, 8).contiguous()
    assert list(dict(V.every_variant(const))) == ["offset", "pitched", "pitched1", "colslice", "transposed", "expanded"]


def test_helpers_keep_nan_payloads_and_signed_zeros():
    t = torch.tensor([[0.0, -0.0, float("nan"), float("inf")], [1.0, -1.0, float("-inf"), 5e-324]], dtype=torch.float64)
    for name, v in V.every_variant(t):
        assert _same_bits(v, t), name
