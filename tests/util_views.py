"""The same values in another layout: pure torch helpers (tensors of any device in, tensors of that device out) for the tests that hand the
HIP operators what torch accepts but a fresh allocation never is — a contiguous tensor whose data pointer is off the 16-byte grid, rows with
a pitch, a column slice of a wider tensor, a transposed copy, a broadcast.  tests/test_views_ref.py checks on the CPU that every helper keeps
the values bit for bit and has exactly the property it claims."""
import torch

GRID = 16                    # bytes: what the vector loads of the kernels and the gates of the C ABI ask of a pointer


def default_offset(dtype) -> int:
    """elements past a 16-byte boundary that leave the pointer off the grid for this dtype while it stays element-aligned: 1 for every
    element narrower than 16 bytes"""
    es = torch.empty((), dtype=dtype).element_size()
    if es >= GRID:
        raise ValueError(f"no off-grid offset for {dtype}: one element fills the grid")
    return 1


def at_offset(t, k=None):
    """the values of t, contiguous, in a buffer whose data pointer is k elements past a 16-byte boundary (k None: default_offset)"""
    es = t.element_size()
    k = default_offset(t.dtype) if k is None else int(k)
    per = GRID // es
    if k < 0 or (k * es) % GRID == 0:
        raise ValueError(f"offset of {k} elements of {es} bytes is on the 16-byte grid")
    buf = torch.empty(t.numel() + k + per, dtype=t.dtype, device=t.device)
    lead = (-(buf.data_ptr() // es)) % per              # elements up to the first 16-byte boundary of the buffer
    v = buf[lead + k: lead + k + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def row_pitched(t, pad):
    """the values of t [..., R, C] with unit stride along the last dimension and a row stride of C + pad elements"""
    if t.dim() < 2 or pad < 1:
        raise ValueError("row_pitched needs at least two dimensions and a positive pad")
    C = t.shape[-1]
    wide = torch.empty(tuple(t.shape[:-1]) + (C + pad,), dtype=t.dtype, device=t.device)
    if wide.is_floating_point():
        wide.fill_(float("nan"))                         # the padding is never to be read
    v = wide[..., :C]
    v.copy_(t)
    return v


def column_slice(t, before=None, after=None):
    """the values of t [..., C] as wide[..., a:a+C] of a [..., a+C+b] tensor — what linear_fused returns for one of its modules (a and b
    default to C: the middle third of a fused projection)"""
    if t.dim() < 1:
        raise ValueError("column_slice needs a last dimension")
    C = t.shape[-1]
    a = C if before is None else int(before)
    b = C if after is None else int(after)
    if a + b < 1:
        raise ValueError("column_slice of the whole row is no slice")
    wide = torch.empty(tuple(t.shape[:-1]) + (a + C + b,), dtype=t.dtype, device=t.device)
    if wide.is_floating_point():
        wide.fill_(float("nan"))
    v = wide[..., a:a + C]
    v.copy_(t)
    return v


def via_transpose(t, d0=-2, d1=-1):
    """the values of t, stored with dimensions d0 and d1 exchanged: non-contiguous when both are longer than 1"""
    return t.transpose(d0, d1).contiguous().transpose(d0, d1)


def constant_dim(t):
    """the first dimension longer than 1 along which t does not vary, or None"""
    for d in range(t.dim()):
        if t.shape[d] > 1 and torch.equal(t, t.narrow(d, 0, 1).expand_as(t)):
            return d
    return None


def expanded(t, dim=None):
    """the values of t with stride 0 along `dim` (None: the first dimension along which t does not vary) — the gradient of a .sum(), a
    broadcast parameter, an index expanded over the vertices.  Only a tensor that is constant along that dimension has such a layout."""
    d = constant_dim(t) if dim is None else dim % t.dim()
    if d is None or t.shape[d] < 2 or not torch.equal(t, t.narrow(d, 0, 1).expand_as(t)):
        raise ValueError("expanded needs a dimension longer than 1 along which the tensor is constant")
    return t.narrow(d, 0, 1).contiguous().expand_as(t)


def every_variant(t):
    """yields (name, view) for every layout above that exists for t: `offset` always; `pitched` (rows stay on the 16-byte grid), `pitched1`
    (they do not) and `transposed` from two dimensions on; `colslice` from one; `expanded` where t is constant along a dimension"""
    es = t.element_size()
    yield "offset", at_offset(t)
    if t.dim() >= 2:
        yield "pitched", row_pitched(t, max(GRID // es, 1))
        yield "pitched1", row_pitched(t, 1)
    if t.dim() >= 1:
        yield "colslice", column_slice(t)
    if t.dim() >= 2 and t.shape[-1] > 1 and t.shape[-2] > 1:
        yield "transposed", via_transpose(t)
    if constant_dim(t) is not None:
        yield "expanded", expanded(t)
