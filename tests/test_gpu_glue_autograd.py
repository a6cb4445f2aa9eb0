"""The differentiable variance-adaptor glue (csrc/tts_glue_grad.hip, decode_ops.bucketize_embed_add_autograd / length_regulate_autograd,
VarianceAdaptor under grad) against the float64 restatements of tests/util_glue_grad_ref.py.

Forward: indices exact, the add bit-equal to torch's add in the same dtype.  Gradients: integer-valued incoming gradients make every fp32
partial sum exact in any order, so the result must be the float64 reference rounded ONCE to the dtype, bit for bit (this catches double
rounding and accumulation in half precision); normal-distributed gradients are held to the bound of a sum of m terms accumulated in fp32
and rounded once, m * 2^-24 * sum|g_i| + 2^-p * |ref| (R.sum_bound; it holds for any summation order).  Two calls on the same inputs must
give the same bits.  Where a case is about every output element being written, the C entry point is called on a NaN-filled (idx: -7)
buffer, and the padding frames of the length regulator's incoming gradient are NaN: none may reach the result.  Every case prints its
figures (`pytest -s`)."""
import copy

import numpy as np
import pytest
import torch

from tests import util_glue_grad_ref as R
from tests import util_glue_ref as G

pytestmark = pytest.mark.gpu
NAN = float("nan")
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
CHUNK = 64


def D():
    from daspeech_amd import decode_ops
    return decode_ops


def LIB():
    from daspeech_amd import _lib
    return _lib


def cu(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to("cuda")


def poisoned(shape, dtype=torch.float32):
    return torch.full(shape, -7 if dtype in (torch.int32, torch.int64) else NAN, dtype=dtype, device="cuda")


def bits_of(dtype):
    return R.SIGNIFICAND_BITS[str(dtype).split(".")[1]]


def f64(t):
    return t.detach().to(torch.float64).cpu().numpy()


def once(ref, dtype):
    """the float64 reference rounded once to dtype (exact integers survive the float64 -> float32 step, so there is one rounding)"""
    return torch.from_numpy(np.asarray(ref, np.float64)).to(torch.float32).to(dtype)


def within(name, got, ref, bound):
    err = np.abs(f64(got) - ref)
    worst = float((err - bound).max()) if err.size else 0.0
    print(f"glue-autograd {name}: max err {float(err.max()) if err.size else 0.0:.3e} max bound {float(np.max(bound)) if err.size else 0.0:.3e} "
          f"largest excess {worst:.3e}")
    assert not np.isnan(f64(got)).any(), f"{name}: NaN in the result (an element never written, or a padding frame read)"
    assert np.all(err <= bound), f"{name}: error above the derived bound by {worst:.3e}"


# ---------------------------------------------------------------- dsp_bucketize_embed_add_fwd

# (seed, n, C, nb): half rows of 520 B (the unaligned path), no bins, more rows than one trip of the 4096-row grid, the minimum
FWD_CASES = [(62, 5, 260, 2), (63, 3, 24, 0), (61, 4100, 256, 255), (64, 1, 1, 1)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", FWD_CASES)
def test_bucketize_forward_indices_exact_and_add_bit_equal_to_torch(case, dtype):
    lib = LIB()
    seed, n, C, nb = case
    x, v, bins, emb = G.bucketize_inputs(seed, n, C, nb)
    tx, tv, tb, te = cu(x, dtype), cu(v), cu(bins), cu(emb, dtype)
    out, idx = poisoned((n, C), dtype), poisoned((n,), torch.int32)
    lib.check(lib.load().dsp_bucketize_embed_add_fwd(lib.ptr(tx), lib.DTYPE_CODES[str(dtype)], lib.ptr(tv), lib.ptr(tb) if nb else None, nb,
                                                     lib.ptr(te), lib.ptr(out), lib.ptr(idx), n, C, lib.current_stream_handle()),
              "dsp_bucketize_embed_add_fwd")
    torch.cuda.synchronize()
    ref_idx = G.bucketize_ref(v, bins)
    np.testing.assert_array_equal(idx.cpu().numpy(), ref_idx)
    want = tx + te[torch.from_numpy(ref_idx).cuda()]             # torch's add in the same dtype on the device
    assert not torch.isnan(out).any()
    assert torch.equal(out, want)
    assert torch.equal(tx, cu(x, dtype))                         # out of place
    got = D().bucketize_embed_add_autograd(tx.view(1, n, C), tv.view(1, n), tb, te)
    assert got.shape == (1, n, C) and got.dtype == dtype and torch.equal(got.view(n, C), want)


# ---------------------------------------------------------------- dsp_embed_grad

def embed_grad_direct(g, idx, K):
    lib = LIB()
    n, C = g.shape
    out = poisoned((K, C), g.dtype)
    nbytes = int(lib.load().dsp_embed_grad_workspace_bytes(n, K - 1, C))
    ws = torch.full((max(nbytes, 16),), 0xAB, dtype=torch.uint8, device="cuda")
    lib.check(lib.load().dsp_embed_grad(lib.ptr(g) if n else None, lib.DTYPE_CODES[str(g.dtype)], lib.ptr(idx) if n else None, lib.ptr(out), n,
                                        K - 1, C, lib.ptr(ws) if n else None, nbytes, lib.current_stream_handle()), "dsp_embed_grad")
    torch.cuda.synchronize()
    return out


def _idx_cases():
    rng = np.random.default_rng(91)
    chunks = np.concatenate([np.full(CHUNK, 0), np.full(CHUNK + 1, 1), np.full(2 * CHUNK + 1, 3)])       # bucket 2 of 4 stays empty
    return {
        "one-bucket-4100": (np.full(4100, 37), 256, 256),          # 65 chunks of one bucket; 255 empty buckets
        "chunk-edges": (rng.permutation(chunks), 4, 20),            # one chunk, one chunk + 1, two chunks + 1; half rows of 40 B: unaligned
        "row-per-bucket": (rng.permutation(256), 256, 256),
        "one-row": (np.array([2]), 3, 8),
        "no-rows": (np.zeros(0, np.int64), 5, 8),
    }


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(_idx_cases()))
def test_embed_grad_of_integer_gradients_is_the_float64_sum_rounded_once(name, dtype):
    assert CHUNK == D().EMBED_GRAD_CHUNK
    idx, K, C = _idx_cases()[name]
    n = len(idx)
    g = np.random.default_rng(92).integers(-2, 3, (n, C)).astype(np.float32)
    got = embed_grad_direct(cu(g, dtype), cu(idx.astype(np.int32)), K)
    ref = R.embed_grad_ref(g, idx, K)
    print(f"glue-autograd embed_grad {name} {dtype}: n {n} K {K} C {C} max |ref| {np.abs(ref).max() if ref.size else 0:.0f}")
    assert not torch.isnan(got).any()
    assert torch.equal(got.cpu(), once(ref, dtype))
    empty = np.bincount(idx, minlength=K) == 0
    assert torch.all(got.cpu()[torch.from_numpy(empty)] == 0)


def _skewed_idx():
    """4100 rows: the buckets of the (61, 4100, 256, 255) values, then every second row moved to bucket 0 (the unvoiced frames' bucket)"""
    _, v, bins, _ = G.bucketize_inputs(61, 4100, 256, 255)
    idx = G.bucketize_ref(v, bins)
    idx[::2] = 0
    return idx


@pytest.mark.parametrize("dtype", DTYPES)
def test_embed_grad_of_normal_gradients_within_the_derived_bound(dtype):
    idx = _skewed_idx()
    tg = cu(np.random.default_rng(93).standard_normal((4100, 256)).astype(np.float32), dtype)
    got = embed_grad_direct(tg, cu(idx.astype(np.int32)), 256)
    g = f64(tg)
    m, a = R.embed_grad_terms(g, idx, 256)
    ref = R.embed_grad_ref(g, idx, 256)
    within(f"embed_grad normal {dtype}", got, ref, R.sum_bound(m, a, ref, bits_of(dtype)))


# ---------------------------------------------------------------- dsp_length_regulator_bwd

def lr_durations(seed, B, N):
    """0..6, a zero inside every sample, the last sample all zero, one segment of 300 frames: maxlen is far beyond the other samples' ends"""
    dur = np.random.default_rng(seed).integers(0, 7, (B, N))
    if N > 2:
        dur[:, N // 2] = 0
    dur[B - 1] = 0
    dur[0, N - 1] = 300
    return dur


def lr_cum(dur):
    lib = LIB()
    B, N = dur.shape
    td = cu(dur.astype(np.int64))
    cum, lens = poisoned((B, N), torch.int64), poisoned((B,), torch.int64)
    lib.check(lib.load().dsp_length_regulator_lens(lib.ptr(td), lib.ptr(cum), lib.ptr(lens), B, N, lib.current_stream_handle()),
              "dsp_length_regulator_lens")
    return cum, int(lens.max().item())


def lr_bwd_direct(g, cum, N):
    lib = LIB()
    B, maxlen, C = g.shape
    out = poisoned((B, N, C), g.dtype)
    lib.check(lib.load().dsp_length_regulator_bwd(lib.ptr(g), lib.DTYPE_CODES[str(g.dtype)], lib.ptr(cum), lib.ptr(out), B, N, C, maxlen,
                                                  lib.current_stream_handle()), "dsp_length_regulator_bwd")
    torch.cuda.synchronize()
    return out


def lr_grad_out(seed, dur, maxlen, C, integer):
    """[B,maxlen,C] float32 with NaN in every padding frame"""
    rng = np.random.default_rng(seed)
    B = dur.shape[0]
    g = rng.integers(-2, 3, (B, maxlen, C)).astype(np.float32) if integer else rng.standard_normal((B, maxlen, C)).astype(np.float32)
    for b in range(B):
        g[b, int(dur[b].sum()):] = np.nan
    return g


# (B, N, C, dtypes): the workload's row, the minimum, more than a wave of rows per sample, more rows than one trip of the 4096-row grid,
# half rows of 520 B (the unaligned path)
LR_CASES = [(3, 5, 256, DTYPES), (2, 1, 1, DTYPES), (2, 257, 8, DTYPES), (2, 2100, 8, DTYPES), (3, 7, 260, [torch.float16])]
LR_PARAMS = [(B, N, C, dt) for B, N, C, dts in LR_CASES for dt in dts]


@pytest.mark.parametrize("B,N,C,dtype", LR_PARAMS)
def test_length_regulator_bwd_sums_its_frames_and_never_reads_padding(B, N, C, dtype):
    dur = lr_durations(100 + N, B, N)
    cum, maxlen = lr_cum(dur)
    assert maxlen == int(dur.sum(1).max()) and maxlen >= 300
    np.testing.assert_array_equal(cum.cpu().numpy(), dur.cumsum(1))
    # integer-valued gradients: the float64 sum rounded once, bit for bit
    g = lr_grad_out(101, dur, maxlen, C, integer=True)
    got = lr_bwd_direct(cu(g, dtype), cum, N)
    ref = R.length_regulator_bwd_ref(g, dur)
    assert not torch.isnan(got).any(), "a padding frame reached grad_x, or a row was never written"
    assert torch.equal(got.cpu(), once(ref, dtype))
    assert torch.all(got.cpu()[torch.from_numpy(dur == 0)] == 0)
    # normal-distributed gradients: the derived bound
    tg = cu(lr_grad_out(102, dur, maxlen, C, integer=False), dtype)
    got = lr_bwd_direct(tg, cum, N)
    gw = f64(tg)
    m, a = R.length_regulator_bwd_terms(gw, dur)
    ref = R.length_regulator_bwd_ref(gw, dur)
    within(f"length_regulator_bwd ({B},{N},{C}) {dtype}", got, ref, R.sum_bound(m, a, ref, bits_of(dtype)))


# ---------------------------------------------------------------- reproducibility

@pytest.mark.parametrize("dtype", DTYPES)
def test_both_backwards_give_the_same_bits_twice(dtype):
    tg = cu(np.random.default_rng(94).standard_normal((4100, 256)).astype(np.float32), dtype)
    idx = cu(np.full(4100, 37, np.int32))
    a, b = embed_grad_direct(tg, idx, 256), embed_grad_direct(tg, idx, 256)
    assert not torch.isnan(a).any() and torch.equal(a, b)
    dur = lr_durations(105, 3, 5)
    cum, maxlen = lr_cum(dur)
    tg = cu(lr_grad_out(95, dur, maxlen, 256, integer=False), dtype)
    a, b = lr_bwd_direct(tg, cum, 5), lr_bwd_direct(tg, cum, 5)
    assert not torch.isnan(a).any() and torch.equal(a, b)


# ---------------------------------------------------------------- autograd plumbing

@pytest.mark.parametrize("dtype", DTYPES)
def test_autograd_through_both_ops_from_a_non_contiguous_gradient(dtype):
    ops = D()
    n, C, nb = 300, 24, 9
    x, v, bins, emb = G.bucketize_inputs(65, n, C, nb)
    tx, tw = cu(x, dtype).view(3, 100, C).requires_grad_(), cu(emb, dtype).requires_grad_()
    out = ops.bucketize_embed_add_autograd(tx, cu(v).view(3, 100), cu(bins), tw)
    assert out.requires_grad and out.shape == tx.shape
    wide = cu(np.random.default_rng(96).standard_normal((3, 100, 2 * C)).astype(np.float32), dtype)
    go = wide[:, :, :C]
    assert not go.is_contiguous()
    gx, gw = torch.autograd.grad(out, (tx, tw), go)
    assert torch.equal(gx, go)                                   # the gradient of x is the incoming gradient
    idx = G.bucketize_ref(v, bins)
    g = f64(go).reshape(n, C)
    m, a = R.embed_grad_terms(g, idx, nb + 1)
    ref = R.embed_grad_ref(g, idx, nb + 1)
    within(f"autograd embed {dtype}", gw, ref, R.sum_bound(m, a, ref, bits_of(dtype)))

    dur = lr_durations(106, 3, 7)
    tx = cu(np.random.default_rng(97).standard_normal((3, 7, C)).astype(np.float32), dtype).requires_grad_()
    out, lens = ops.length_regulate_autograd(tx, cu(dur))
    assert lens.grad_fn is None and not lens.requires_grad and lens.tolist() == dur.sum(1).tolist()
    plain, plain_lens = ops.length_regulate(tx, cu(dur))
    assert torch.equal(out.detach(), plain) and torch.equal(lens, plain_lens)
    wide = cu(np.random.default_rng(98).standard_normal((3, out.shape[1], 2 * C)).astype(np.float32), dtype)
    go = wide[:, :, C:]
    gx, = torch.autograd.grad(out, tx, go)
    g = f64(go)
    m, a = R.length_regulator_bwd_terms(g, dur)
    ref = R.length_regulator_bwd_ref(g, dur)
    within(f"autograd length_regulate {dtype}", gx, ref, R.sum_bound(m, a, ref, bits_of(dtype)))


def test_no_rows_and_no_frames_give_exact_zero_gradients():
    ops = D()
    w = torch.randn(4, 8, device="cuda", requires_grad=True)
    x = torch.zeros(0, 8, device="cuda", requires_grad=True)
    out = ops.bucketize_embed_add_autograd(x, torch.zeros(0, device="cuda"), torch.tensor([-1.0, 0.0, 1.0], device="cuda"), w)
    gx, gw = torch.autograd.grad(out.sum(), (x, w))
    assert gx.shape == (0, 8) and gw.shape == (4, 8) and torch.all(gw == 0)
    got = embed_grad_direct(torch.zeros(0, 8, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda"), 4)      # the C entry point, n = 0
    assert torch.all(got == 0)
    x = torch.randn(2, 3, 8, device="cuda", requires_grad=True)
    out, lens = ops.length_regulate_autograd(x, torch.zeros(2, 3, dtype=torch.long, device="cuda"))
    assert out.shape == (2, 0, 8) and lens.tolist() == [0, 0]
    gx, = torch.autograd.grad(out.sum(), x)
    assert gx.shape == (2, 3, 8) and torch.all(gx == 0)
    with pytest.raises(RuntimeError):
        ops.length_regulate_autograd(x.double(), torch.ones(2, 3, dtype=torch.long, device="cuda"))       # float64 is refused, not narrowed
    with pytest.raises(RuntimeError):
        ops.bucketize_embed_add_autograd(x.double(), torch.zeros(2, 3, device="cuda"), torch.tensor([0.0], device="cuda"), w[:2].double())


# ---------------------------------------------------------------- VarianceAdaptor under grad

def _adaptor(dtype):
    from daspeech_amd.models.fastspeech2 import VarianceAdaptor
    torch.manual_seed(0)
    return VarianceAdaptor(256, 256, 3, 256, -4.66, 5.7333, -4.9544, 3.2244, dropout=0.0).cuda().to(dtype).eval()


def _adaptor_inputs(dtype):
    """as tests/test_gpu_model.py::test_training_path_adaptor_matches_hip_inference_path"""
    torch.manual_seed(3)
    x = torch.randn(3, 11, 256, device="cuda")
    pmask = torch.arange(11, device="cuda").unsqueeze(0) >= torch.tensor([11, 7, 2], device="cuda").unsqueeze(1)
    dur = torch.randint(0, 5, (3, 11), device="cuda").masked_fill(pmask, 0)
    pit = torch.rand(3, 11, device="cuda") * 10 - 4.6; ene = torch.rand(3, 11, device="cuda") * 8 - 4.9
    return x.to(dtype), pmask, dur, pit.to(dtype), ene.to(dtype)


def _count_calls(monkeypatch):
    ops = D()
    calls = {"bucketize": 0, "regulate": 0}
    b0, r0 = ops.bucketize_embed_add_autograd, ops.length_regulate_autograd

    def b1(*a, **k):
        calls["bucketize"] += 1
        return b0(*a, **k)

    def r1(*a, **k):
        calls["regulate"] += 1
        return r0(*a, **k)
    monkeypatch.setattr(ops, "bucketize_embed_add_autograd", b1)
    monkeypatch.setattr(ops, "length_regulate_autograd", r1)
    return calls


def _memoise(monkeypatch, mod, stats):
    """mod(input) returns the output recorded for a bit-equal earlier input instead of computing it again"""
    seen, forward = [], mod.forward

    def fwd(inp):
        for i, o in seen:
            if i.shape == inp.shape and torch.equal(i, inp):
                stats["hit"] += 1
                return o
        stats["miss"] += 1
        seen.append((inp.detach().clone(), forward(inp)))
        return seen[-1][1]
    monkeypatch.setattr(mod, "forward", fwd)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_adaptor_under_grad_runs_the_hip_ops_and_returns_the_bits_of_the_torch_formulation(dtype, monkeypatch):
    """All five outputs of forward under grad, teacher-forced and predicted, torch.equal to the torch formulation on the same tensors.
    The three variance predictors are torch code on both sides (MIOpen convolutions, a hipBLASLt projection) and are not bit-reproducible
    from call to call on this stack — the torch formulation differs from ITSELF in log_dur / pitch / energy (seen: 3e-7 .. 6e-7 in fp32,
    1.5e-3 .. 2e-3 in fp16; printed below) — so each predictor is memoised on the bits of its input: the torch run must then find every predictor input the HIP
    run recorded (the energy predictor's is x + pitch embedding: the first glue op's output), and every output can be compared exactly."""
    va = _adaptor(dtype)
    x, pmask, dur, pit, ene = _adaptor_inputs(dtype)

    def run():
        with torch.enable_grad():
            return va(x.clone().requires_grad_(), pmask, dur, pit, ene), va(x.clone().requires_grad_(), pmask)
    names = ("x", "out_lens", "log_dur", "pitch", "energy")
    monkeypatch.setattr(va, "_forward_hip", va._forward_torch)
    t1, t2 = run(), run()
    monkeypatch.undo()
    for mode, p, q in zip(("teacher", "predicted"), t1, t2):
        print(f"glue-autograd adaptor {dtype} {mode}: the torch formulation against itself, max abs diff " +
              ", ".join(f"{n} {(a.double() - b.double()).abs().max().item() if a.numel() else 0.0:.3e}" for n, a, b in zip(names, p, q)))
    stats = {"hit": 0, "miss": 0}
    for pred in (va.duration_predictor, va.pitch_predictor, va.energy_predictor):
        _memoise(monkeypatch, pred, stats)
    calls = _count_calls(monkeypatch)
    hip = run()
    assert calls == {"bucketize": 4, "regulate": 2}
    assert stats == {"hit": 2, "miss": 4}          # the predicted pass feeds the same x to the duration and pitch predictors
    assert hip[0][0].requires_grad and hip[0][1].grad_fn is None
    monkeypatch.setattr(va, "_forward_hip", va._forward_torch)
    ref = run()
    assert calls == {"bucketize": 4, "regulate": 2}
    assert stats == {"hit": 8, "miss": 4}, "a predictor of the torch formulation saw other input bits than under the HIP ops"
    for mode, got, want in zip(("teacher", "predicted"), hip, ref):
        assert len(got) == len(want) == 5
        for name, a, b in zip(names, got, want):
            print(f"glue-autograd adaptor {dtype} {mode} {name}: shape {tuple(a.shape)} equal {torch.equal(a, b)}")
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), (mode, name)


def test_adaptor_in_float64_keeps_the_torch_formulation(monkeypatch):
    va = _adaptor(torch.float64)
    x, pmask, dur, pit, ene = _adaptor_inputs(torch.float64)
    calls = _count_calls(monkeypatch)
    with torch.enable_grad():
        out = va(x.clone().requires_grad_(), pmask, dur, pit, ene)
    assert calls == {"bucketize": 0, "regulate": 0}
    assert out[0].dtype == torch.float64 and out[0].requires_grad


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_adaptor_gradients_are_as_accurate_as_the_torch_formulation(dtype, monkeypatch):
    """Gradients w.r.t. the input and both embedding tables under a fixed random cotangent on the regulated output, against a float64 CPU
    run of _forward_torch on a double copy of the module; err = max |got - ref| / max |ref|.  The torch formulation on the same device gives
    err_t against the same reference; the HIP ops must hold err <= 8 * err_t + 4 ulps of the dtype (G.fp32_bound's rule)."""
    va = _adaptor(dtype)
    x, pmask, dur, pit, ene = _adaptor_inputs(dtype)
    params = lambda m: [m.embed_pitch.weight, m.embed_energy.weight]     # noqa: E731

    def grads(mod, xin, args, cot):
        xin = xin.clone().requires_grad_()
        with torch.enable_grad():
            out = mod(xin, *args)[0]
            return torch.autograd.grad(out, [xin] + params(mod), cot.to(device=out.device, dtype=out.dtype))

    torch.manual_seed(11)
    cot = torch.randn((3, int(dur.sum(1).max()), 256), device="cuda").to(dtype)
    calls = _count_calls(monkeypatch)
    got = grads(va, x, (pmask, dur, pit, ene), cot)
    assert calls == {"bucketize": 2, "regulate": 1}
    va64 = copy.deepcopy(va).double().cpu()
    ref = grads(va64, x.double().cpu(), (pmask.cpu(), dur.cpu(), pit.double().cpu(), ene.double().cpu()), cot.double().cpu())
    monkeypatch.setattr(va, "_forward_hip", va._forward_torch)
    tor = grads(va, x, (pmask, dur, pit, ene), cot)
    assert calls == {"bucketize": 2, "regulate": 1}
    ulp = 2.0 ** -(bits_of(dtype) - 1)
    for name, g, t, r in zip(("x", "embed_pitch.weight", "embed_energy.weight"), got, tor, ref):
        r = r.numpy()
        err, err_t = G.rel_err(f64(g), r), G.rel_err(f64(t), r)
        bound = G.fp32_bound(err_t, float("inf")) if dtype == torch.float32 else 8.0 * err_t + 4.0 * ulp
        print(f"glue-autograd adaptor {dtype} d/d{name}: err {err:.3e} err_t {err_t:.3e} bound {bound:.3e}")
        assert g.dtype == dtype and g.shape == r.shape and not torch.isnan(g).any()
        assert err <= bound, f"d/d{name}: err {err:.3e} > bound {bound:.3e} (torch formulation: {err_t:.3e})"
