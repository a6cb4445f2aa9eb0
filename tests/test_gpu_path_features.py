"""GPU: decode_ops.path_features_autograd (csrc/path_features_train.hip) against the torch lines of the criterion's argmax branch
(tests/util_path_features_ref.py, held to a vertex-by-vertex loop by tests/test_path_features_ref.py) on the same device tensors: out, pad, n
and dfeatures with torch.equal in fp32, fp16 and bf16 — a row is copied, and each source row has exactly one addend in the gradient, so the
bits are the comparison.  Shapes are the smallest at which the kernels can go wrong: L at the wave tail and at one and many 64-vertex chunks,
C of one 16-byte quad, of no multiple of a wave's quads and the released width, widths 0, 1, the widest count and past it, more than one
workgroup tile each way, counts that differ per sample with a sample that has no vertex on the path."""
import pytest
import torch

from tests import util_path_features_ref as U

pytestmark = pytest.mark.gpu

DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
B = 3


def _ops():
    from daspeech_amd import decode_ops
    return decode_ops


def _widest(path, skip_first=True):
    on = path >= 0
    if skip_first:
        on = on.clone()
        on[:, 0] = False
    return int(on.sum(1).max())


def _dy(W, C, dtype, seed=3):
    return torch.randn((B, W, C), generator=torch.Generator().manual_seed(seed)).to(dtype).cuda()


def _check(x, path, W, dtype, skip_first=True, what=""):
    """operator against the torch lines at width W: the four tensors bit for bit"""
    dy = _dy(W, x.shape[2], dtype)
    ref = U.backward_of(U.reference, x, path, W, dy, skip_first)
    got = U.backward_of(_ops().path_features_autograd, x, path, W, dy, skip_first)
    for name, r, g in zip(("out", "pad", "n", "dfeatures"), ref, got):
        assert g.dtype == r.dtype and g.shape == r.shape and g.is_contiguous(), (what, name, W)
        assert torch.equal(g, r), (what, name, W)
    return got


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("C", [8, 264, 512])
@pytest.mark.parametrize("L", [1, 2, 63, 64, 65, 257])
def test_equals_the_torch_lines(L, C, dtype):
    dt = DTYPES[dtype]
    x = U.make_features(B, L, C, dt, 1, "cuda")
    path = U.random_path(B, L, 2).cuda()
    counts = (path[:, 1:] >= 0).sum(1).tolist()
    assert counts[1] == 0 and (L < 63 or len(set(counts)) == 3)              # a sample with no vertex on the path, three different counts
    widest = _widest(path)
    for W in sorted({0, 1, widest, widest + 3}):
        out, pad, n, dx = _check(x, path, W, dt, what=(L, C, dtype))
        assert n.tolist() == [min(c, W) for c in counts]


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_more_than_one_workgroup_tile_each_way(dtype):
    """the widths of the tiles are the kernels' own constants: three backward tiles and a tail in L, two forward tiles and a tail in W"""
    D = _ops()
    L, W = 3 * D.PATH_FEATURES_TILE_L + 5, 2 * D.PATH_FEATURES_TILE_W + 3
    path = U.planted_path("every_vertex", B, L)
    path[1, 7:] = -1                                                         # six rows: inside the first forward tile
    path[2, ::2] = -1
    path = path.cuda()
    assert _widest(path) > W > D.PATH_FEATURES_TILE_W
    x = U.make_features(B, L, 264, DTYPES[dtype], 4, "cuda")
    _check(x, path, W, DTYPES[dtype])
    _check(x, path, _widest(path) + 3, DTYPES[dtype])


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("name", U.PLANTED)
def test_planted_paths(name, dtype):
    dt = DTYPES[dtype]
    L, C = 130, 264
    path = U.planted_path(name, B, L).cuda()
    x = U.make_features(B, L, C, dt, 6, "cuda")
    widest = _widest(path)
    for W in sorted({1, max(widest, 1), widest + 3, 40}):
        got = _check(x, path, W, dt, what=name)
        if name == "only_vertex_0":
            assert widest == 0 and got[1].all() and not got[0].any() and not got[2].any() and not got[3].any()
    if name == "all_fives":                                                  # only the sign of a value is read
        ranks = U.ranks_where(path >= 0)
        assert not torch.equal(ranks, path)
        a = _check(x, path, widest, dt)
        b = _check(x, ranks, widest, dt)
        assert all(torch.equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_surplus_is_dropped_and_nothing_behind_the_outputs_is_written(dtype):
    """every vertex on the path and W < L - 1: the rows beyond W are dropped; the C ABI called on buffers of the caller with a NaN row (0xff
    bytes) behind out, pad, n and dfeatures, which stays as it was"""
    D = _ops()
    from daspeech_amd import _lib
    dt = DTYPES[dtype]
    L, C, W = 70, 264, 21
    path = U.planted_path("every_vertex", B, L).cuda()
    x = U.make_features(B, L, C, dt, 7, "cuda")
    dy = _dy(W, C, dt)
    ref = U.backward_of(U.reference, x, path, W, dy)
    assert ref[2].tolist() == [W] * B and not ref[1].any()
    _check(x, path, W, dt)
    out = torch.full((B * W + 1, C), float("nan"), dtype=dt, device="cuda")
    pad = torch.full((B * W + 16,), 0xff, dtype=torch.uint8, device="cuda")
    n = torch.full((B + 1,), -7, dtype=torch.int64, device="cuda")
    dx = torch.full((B * L + 1, C), float("nan"), dtype=dt, device="cuda")
    lib = _lib.load()
    code = D._FLOAT_CODES[dt]
    D._launch(x.device, lib.dsp_path_features_fwd, x.data_ptr(), C, path.data_ptr(), L, 1, 1, 1, out.data_ptr(), pad.data_ptr(), n.data_ptr(),
              code, B, L, W, C)
    D._launch(x.device, lib.dsp_path_features_bwd, dy.data_ptr(), W * C, C, path.data_ptr(), L, 1, 1, 1, dx.data_ptr(), code, B, L, W, C)
    torch.cuda.synchronize()
    assert torch.equal(out[:-1].view(B, W, C), ref[0]) and torch.isnan(out[-1]).all()
    assert torch.equal(pad[:B * W].view(B, W).bool(), ref[1]) and (pad[:B * W] <= 1).all() and (pad[B * W:] == 0xff).all()
    assert torch.equal(n[:B], ref[2]) and int(n[B]) == -7
    assert torch.equal(dx[:-1].view(B, L, C), ref[3]) and torch.isnan(dx[-1]).all()
    assert not dx[:-1].view(B, L, C)[:, W + 1:].any()                        # the dropped vertices: exact zeros


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_nan_in_rows_that_are_not_selected_never_shows(dtype):
    dt = DTYPES[dtype]
    L, C = 65, 8
    path = U.random_path(B, L, 2).cuda()
    x = U.make_features(B, L, C, dt, 1, "cuda")
    clean = x.clone()
    x[path < 0] = float("nan")
    x[:, 0] = float("inf")
    W = _widest(path) + 3
    out, pad, n = _ops().path_features_autograd(x, path, W)
    assert torch.isfinite(out).all()
    want = U.reference(clean, path, W)
    assert torch.equal(out, want[0]) and torch.equal(pad, want[1]) and torch.equal(n, want[2])


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_skip_first_false_keeps_vertex_0(dtype):
    dt = DTYPES[dtype]
    L, C = 65, 264
    path = U.random_path(B, L, 2).cuda()
    x = U.make_features(B, L, C, dt, 1, "cuda")
    W = _widest(path, False)
    assert W == _widest(path) + 1
    got = _check(x, path, W, dt, skip_first=False)
    assert torch.equal(got[0][0, 0], x[0, 0]) and torch.equal(got[3][0, 0], _dy(W, C, dt)[0, 0])
    _check(x, path, W + 3, dt, skip_first=False)
    _check(x, path, 1, dt, skip_first=False)


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_int32_path_equals_int64(dtype):
    dt = DTYPES[dtype]
    L, C = 130, 8
    path = U.random_path(B, L, 8).cuda()
    x = U.make_features(B, L, C, dt, 1, "cuda")
    W = _widest(path)
    a = _check(x, path, W, dt)
    b = _check(x, path.to(torch.int32), W, dt)
    assert all(torch.equal(u, v) for u, v in zip(a, b))


def test_without_gradient_nothing_is_recorded():
    D = _ops()
    L, C = 65, 8
    path = U.random_path(B, L, 2).cuda()
    x = U.make_features(B, L, C, torch.float16, 1, "cuda")
    W = _widest(path)
    want = U.reference(x, path, W)
    with torch.no_grad():
        res = D.path_features_autograd(x.clone().requires_grad_(True), path, W)
    assert all(t.grad_fn is None and not t.requires_grad for t in res) and all(torch.equal(u, v) for u, v in zip(res, want))
    res = D.path_features_autograd(x, path, W)                               # no input requires grad
    assert all(t.grad_fn is None and not t.requires_grad for t in res) and all(torch.equal(u, v) for u, v in zip(res, want))
    out, pad, n = D.path_features_autograd(x.clone().requires_grad_(True), path, W)
    assert out.requires_grad and not pad.requires_grad and not n.requires_grad      # pad and n are marked non-differentiable
    out, pad, n = D.path_features_autograd(x.clone().requires_grad_(True), path, 0)
    assert out.shape == (B, 0, C) and pad.shape == (B, 0) and pad.dtype == torch.bool and n.tolist() == [0] * B and n.dtype == torch.int64


def test_gates_on_gpu_tensors():
    D = _ops()
    L, C = 65, 8
    path = U.random_path(B, L, 2).cuda()
    x = U.make_features(B, L, C, torch.float16, 1, "cuda")
    assert D.path_features_served(x, path, 12) and D.path_features_served(x, path.to(torch.int32), 0)
    with torch.autocast("cuda", dtype=torch.float16):
        assert not D.path_features_served(x, path, 12)
    old = D.set_path_features_hip(False)
    try:
        assert not D.path_features_served(x, path, 12)
    finally:
        D.set_path_features_hip(old)
    assert not D.path_features_served(x.double(), path, 12)
    assert not D.path_features_served(x, path.cpu(), 12)
    assert not D.path_features_served(x[:, :, :4], path, 12)                 # half a quad
    with pytest.raises(RuntimeError, match="float64"):
        D.path_features_autograd(x.double(), path, 12)


def test_no_host_wait_in_forward_or_backward():
    """under set_sync_debug_mode("error") the operator's forward and backward pass, and the torch lines (the host read of the widest count)
    raise"""
    D = _ops()
    L, C = 65, 264
    path = U.random_path(B, L, 2).cuda()
    x = U.make_features(B, L, C, torch.float16, 1, "cuda")
    W = _widest(path)
    dy = _dy(W, C, torch.float16)
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    control = None
    try:
        torch.cuda.set_sync_debug_mode("error")
        got = U.backward_of(D.path_features_autograd, x, path, W, dy)
        try:
            U.backward_of(lambda f, p, w, s: U.torch_lines(f, p, s), x, path, W, dy)
        except RuntimeError as e:
            control = str(e)
    finally:
        torch.cuda.set_sync_debug_mode(old)
    if control is None:
        pytest.skip("the control (int(n_on.max()) under set_sync_debug_mode('error')) does not raise on this torch build")
    assert "synchroniz" in control
    assert torch.isfinite(got[3]).all()
