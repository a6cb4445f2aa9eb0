"""CPU: the reference of the path-features tests (tests/util_path_features_ref.py) — the torch lines of the criterion's argmax branch — is the
stable compaction its operator is defined as: forward, mask, counts and gradient equal a plain Python loop over the vertices bit for bit
(each source row has exactly one addend in the gradient, so equality of bits is the right comparison in every dtype)."""
import pytest
import torch

from tests import util_path_features_ref as U

DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16, "fp64": torch.float64}


def _dy(B, W, C, dtype):
    return torch.randn((B, W, C), generator=torch.Generator().manual_seed(3)).to(dtype)


def _same(ref, want):
    out, pad, n, dx = ref
    assert torch.equal(out, want[0]) and out.dtype == want[0].dtype
    assert torch.equal(pad, want[1]) and pad.dtype == torch.bool
    assert torch.equal(n, want[2]) and n.dtype == torch.int64
    assert torch.equal(dx, want[3])


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("name", U.PLANTED + ("random",))
def test_torch_lines_equal_the_loop(name, dtype):
    B, L, C = 3, 70, 8
    path = U.random_path(B, L, 2) if name == "random" else U.planted_path(name, B, L)
    x = U.make_features(B, L, C, DTYPES[dtype], 1)
    on = path >= 0
    on[:, 0] = False
    W = int(on.sum(1).max())                                     # the width the torch lines choose themselves
    dy = _dy(B, W, C, DTYPES[dtype])
    got = U.backward_of(lambda f, p, w, s: U.torch_lines(f, p, s), x, path, W, dy)
    assert got[0].shape == (B, W, C)
    _same(got, U.loop(x, path, W, dy))


@pytest.mark.parametrize("skip_first", [True, False])
@pytest.mark.parametrize("extra", [-2, 0, 3])
def test_reference_at_another_width_equals_the_loop(extra, skip_first):
    """narrower than the widest count: the surplus is dropped; wider: zero rows and True behind it, the counts unchanged"""
    B, L, C = 3, 70, 8
    path = U.random_path(B, L, 4)
    x = U.make_features(B, L, C, torch.float32, 1)
    on = path >= 0
    if skip_first:
        on[:, 0] = False
    widest = int(on.sum(1).max())
    W = widest + extra
    dy = _dy(B, W, C, torch.float32)
    got = U.backward_of(U.reference, x, path, W, dy, skip_first)
    _same(got, U.loop(x, path, W, dy, skip_first))
    if extra > 0:
        assert got[1][:, widest:].all() and not got[0][:, widest:].any()
    assert int(got[2].max()) == min(widest, W)


def test_planted_paths_have_what_they_claim():
    B, L = 3, 70
    assert (U.planted_path("only_vertex_0", B, L) >= 0).sum() == B
    p = U.planted_path("vertices_63_64", B, L)
    assert (p[:, 63] == 1).all() and (p[:, 64] == 2).all() and (p >= 0).sum() == 3 * B
    assert (U.planted_path("last_vertex", B, L)[:, L - 1] == 1).all()
    assert (U.planted_path("every_vertex", B, L) == torch.arange(L)).all()
    p = U.planted_path("all_fives", B, L)
    assert set(p.unique().tolist()) == {-1, 5} and torch.equal(p >= 0, U.random_path(B, L, 5) >= 0)
    r = U.random_path(B, L, 2)
    counts = (r >= 0).sum(1)
    assert counts[1] == 0 and counts[0] != counts[2] and counts.min() == 0 and (r[:, 0][counts > 0] == 0).all()


def test_nan_in_rows_that_are_not_selected_never_shows():
    B, L, C = 3, 70, 8
    path = U.random_path(B, L, 2)
    x = U.make_features(B, L, C, torch.float32, 1)
    x[(path < 0)] = float("nan")
    x[:, 0] = float("nan")
    out, pad, n = U.reference(x, path, 50)
    assert torch.isfinite(out).all()
