"""GPU: the stride-2 channels-last Conv1d training operator (csrc/conv1d_stride2_train.hip; decode_ops.conv1d_stride2_channels_last_autograd)
against the float64 restatement of tests/util_conv1d_stride2_ref.py, by the project's 4 x rule (tests/util_4x_rule.py): for y, dx, dW and db
    max|got - ref64| / max|ref64|  <=  4 * max(the same figure for the yardstick, one rounding of the dtype),
the yardstick being torch's own F.conv1d(stride=2) under autograd in the same dtype on the transposed tensors.  A tap that reads the
neighbouring sample, a parity image read at the wrong row, a read past column Cin or a row that is never written is an error of order 1
(outputs, gradients and workspaces are NaN-filled before every call).  Shapes, with R the row tile and S the row split of the weight gradient:
T in {1, 2, 3, 4, K-1, K, 2R-1, 2R, 2R+1, 2R+2, 4R+1, 4R+2} (each T_out around the row tile reached from an odd and from an even T; the two
parities of dx with equal and with different tile counts); channel counts with a tail block of 16 (80 = 64 + 16, 16 alone, 144 = 2 x 64 + 16)
and of 48, half a column tile (64), one (128) and one and a half (192), K 1 / 3 / 5 / 15; the subsampler's real widths at T = 2R+1, 2R+2;
B * T_out one above S, and a split boundary inside a sample."""
import copy

import pytest
import torch

from tests import util_conv1d_stride2_ref as A
from tests.util_4x_rule import check_4x

pytestmark = pytest.mark.gpu
NAN = float("nan")
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
R, S = A.ROW_TILE, A.WGRAD_ROWS
BIAS_MODES = ("none", "dtype", "fp32")
GRADS = ("dx", "dw", "db")

SHAPES = [(16, 64, 1), (80, 64, 5), (48, 192, 3), (64, 128, 15), (144, 64, 5)]
REAL = [(80, 1024, 5), (512, 512, 5)]


def _cases():
    out = []
    for Cin, Cout, K in SHAPES:
        for T in sorted({1, 2, 3, 4, K - 1, K, 2 * R - 1, 2 * R, 2 * R + 1, 2 * R + 2, 4 * R + 1, 4 * R + 2} - {0}):
            for B in (1, 3):
                out += [(B, T, Cin, Cout, K, dt) for dt in (F16, BF16)]
    for Cin, Cout, K in REAL:
        out += [(B, T, Cin, Cout, K, dt) for T in (2 * R + 1, 2 * R + 2) for B in (1, 3) for dt in (F16, BF16)]
    out += [(1, 2 * S + 1, 16, 64, 3, dt) for dt in (F16, BF16)]            # B*T_out = S + 1: a split of one row
    out += [(3, 700, 80, 64, 5, dt) for dt in (F16, BF16)]                  # B*T_out = 1050: the split boundary falls inside a sample
    return out


CASES = _cases()
IDS = ["B%d-T%d-%dto%d-K%d-%s" % (c[:5] + (str(c[5]).split(".")[1],)) for c in CASES]


def D():
    from daspeech_amd import decode_ops
    return decode_ops


def LIB():
    from daspeech_amd import _lib
    return _lib


def poisoned(shape, dtype):
    return torch.full(tuple(shape), NAN, dtype=dtype, device="cuda")


def stored(case):
    """the inputs as the dtype stores them, on the GPU; bias32: the same values in fp32"""
    B, T, Cin, Cout, K, dtype = case
    t = A.inputs(100 + T + 7 * B + K + Cin, B, T, Cin, Cout, K)
    out = {n: v.to(dtype).cuda() for n, v in t.items()}
    out["bias32"] = out["bias"].float()
    return out


def _bias(t, mode):
    return {"none": None, "dtype": t["bias"], "fp32": t["bias32"]}[mode]


def hip_direct(case, t, mode="dtype", skip=(), x=None, ld_x=None, short=0):
    """the two C entry points on poisoned outputs and workspaces; short: bytes taken off the workspace sizes (returns the two codes)"""
    B, T, Cin, Cout, K, dtype = case
    To = A.t_out(T)
    lib, L = LIB(), LIB().load()
    code = lib.DTYPE_CODES[str(dtype)]
    bias = _bias(t, mode)
    bcode = lib.DTYPE_CODES[str((t["x"] if bias is None else bias).dtype)]
    st = lib.current_stream_handle()
    x = t["x"] if x is None else x
    ld_x = Cin if ld_x is None else ld_x
    y = poisoned((B, To, Cout), dtype)
    n0 = int(L.dsp_conv1d_s2_train_workspace_bytes(0, B, T, Cin, Cout, K))
    ws0 = poisoned((n0 // 4,), F32)
    rc0 = L.dsp_conv1d_s2_train_fwd(lib.ptr(x), ld_x, lib.ptr(t["w"]), lib.ptr(bias), lib.ptr(y), Cout, lib.ptr(ws0), n0 - short, code, bcode, B, T, Cin,
                                    Cout, K, st)
    shapes = dict(dx=(B, T, Cin), dw=(Cout, Cin, K), db=(Cout,))
    g = {n: (None if n in skip else poisoned(shapes[n], (F32 if mode == "fp32" else dtype) if n == "db" else dtype)) for n in GRADS}
    n1 = int(L.dsp_conv1d_s2_train_workspace_bytes(1, B, T, Cin, Cout, K))
    ws1 = poisoned((n1 // 4,), F32)
    rc1 = L.dsp_conv1d_s2_train_bwd(lib.ptr(t["dy"]), Cout, lib.ptr(x), ld_x, lib.ptr(t["w"]), lib.ptr(g["dx"]), lib.ptr(g["dw"]), lib.ptr(g["db"]),
                                    lib.ptr(ws1), n1 - short, code, bcode, B, T, Cin, Cout, K, st)
    torch.cuda.synchronize()
    if short:
        return rc0, rc1, [y, ws0, ws1] + list(g.values())
    lib.check(rc0, "fwd")
    lib.check(rc1, "bwd")
    out = dict(y=y)
    out.update({n: v for n, v in g.items() if v is not None})
    return out


def reference(t):
    """float64, without the bias in y (added per bias mode)"""
    c = {n: t[n].double().cpu() for n in ("x", "w", "bias", "dy")}
    out = {n: v.numpy() for n, v in A.backward(c["x"], c["w"], c["dy"]).items()}
    out["y0"] = A.forward(c["x"], c["w"]).numpy()
    out["bias"] = c["bias"].numpy()
    return out


_cache = {}


def results(ci):
    """inputs, float64 reference, the torch yardstick with and without bias and one HIP run of a case, computed once and left unchanged"""
    if ci not in _cache:
        t = stored(CASES[ci])
        tor = {True: A.torch_lines(t["x"], t["w"], t["bias"], t["dy"]), False: A.torch_lines(t["x"], t["w"], None, t["dy"])}
        _cache[ci] = (t, reference(t), tor, hip_direct(CASES[ci], t))
        if len(_cache) > 4:                                                  # the cases run in order: keep the device's memory small
            del _cache[next(iter(_cache))]
    return _cache[ci]


def test_constants_match_the_library():
    d, ws = D(), LIB().load().dsp_conv1d_s2_train_workspace_bytes
    assert (d.CONV1D_TRAIN_ROW_TILE, d.CONV1D_TRAIN_WGRAD_ROWS, d.CONV1D_TRAIN_MAX_K, d.CONV1D_TRAIN_MAX_C) == (A.ROW_TILE, A.WGRAD_ROWS, A.MAX_K, A.MAX_C)
    assert ws(1, 1, 2 * S + 1, 16, 64, 3) - ws(1, 1, 2 * S, 16, 64, 3) >= 4 * 3 * 16 * 64      # B*T_out = S + 1: a second split


@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_every_element_written_and_within_4x_of_torch(ci):
    """1. accuracy, for the three bias modes of each case"""
    t, ref, tor, hip = results(ci)
    B, T, Cin, Cout, K, dtype = CASES[ci]
    assert hip["y"].shape == tor[True]["y"].shape == (B, A.t_out(T), Cout)
    for mode in BIAS_MODES:
        got = hip if mode == "dtype" else hip_direct(CASES[ci], t, mode)
        with_bias = mode != "none"
        want = dict(y=ref["y0"] + ref["bias"] if with_bias else ref["y0"], dx=ref["dx"], dw=ref["dw"], db=ref["db"])
        yard = dict(tor[with_bias])
        yard.setdefault("db", tor[True]["db"])                              # db does not depend on the bias: torch's figure for it with one
        assert got["db"].dtype == (F32 if mode == "fp32" else dtype)
        for name, v in got.items():
            assert not torch.isnan(v).any(), f"{mode} {name}: NaN (an element never written)"
        check_4x(f"conv1d-s2-{IDS[ci]}-bias-{mode}", got, yard, want)
    if K == 1:
        assert not hip["dx"][:, 1::2].any()                                 # rows no tap reaches: written, as zeros
    landing = {k for k, _, _ in A.taps(T, K)}
    for k in range(K):
        assert k in landing or not hip["dw"][:, :, k].any(), k              # taps that never land inside a sample: written, as zeros


@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_two_calls_give_equal_bits(ci):
    """3. bits: a second call"""
    t, ref, tor, hip = results(ci)
    again = hip_direct(CASES[ci], t)
    for name, v in hip.items():
        assert torch.equal(v, again[name]), name


NULLABLE = [i for i, c in enumerate(CASES) if c[1] in (2, 2 * R + 1, 2 * S + 1, 700) and c[5] == F16]


@pytest.mark.parametrize("ci", NULLABLE, ids=[IDS[i] for i in NULLABLE])
def test_each_gradient_alone_has_the_bits_it_has_with_the_others(ci):
    """3. bits: dx, dW, db each requested alone and each left out"""
    t, ref, tor, hip = results(ci)
    for name in GRADS:
        alone = hip_direct(CASES[ci], t, skip=tuple(n for n in GRADS if n != name))
        assert sorted(alone) == sorted(("y", name)) and torch.equal(alone[name], hip[name]), name
        part = hip_direct(CASES[ci], t, skip=(name,))
        assert name not in part
        for n, v in part.items():
            assert torch.equal(v, hip[n]), (name, n)


@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("mode", BIAS_MODES)
def test_operator_is_the_two_entry_points(dtype, mode):
    """3. bits: the autograd operator returns what the direct C calls return; a gradient autograd does not ask for is not computed"""
    case = (3, 2 * R + 1, 80, 192, 5, dtype)
    t = stored(case)
    direct = hip_direct(case, t, mode)
    bias = _bias(t, mode)
    leaves = [t["x"].clone().requires_grad_(), t["w"].clone().requires_grad_()] + ([] if bias is None else [bias.clone().requires_grad_()])
    y = D().conv1d_stride2_channels_last_autograd(*leaves)
    grads = torch.autograd.grad(y, leaves, t["dy"])
    assert torch.equal(y, direct["y"])
    for name, g in zip(GRADS, grads):
        assert g.dtype == direct[name].dtype and torch.equal(g, direct[name]), name
    w2 = t["w"].clone().requires_grad_()
    (dw2,) = torch.autograd.grad(D().conv1d_stride2_channels_last_autograd(t["x"], w2, bias), [w2], t["dy"])
    assert torch.equal(dw2, direct["dw"])
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda s: (saved.append(s), s)[1], lambda s: s):
        D().conv1d_stride2_channels_last_autograd(*leaves)
    assert len(saved) == 2 and saved[0].shape == t["x"].shape and saved[1].shape == t["w"].shape          # x and weight, nothing else


# ---------------------------------------------------------------- 2. views

def _op(x, w, bias, dy):
    leaves = [x.detach().requires_grad_(), w.detach().requires_grad_(), bias.detach().requires_grad_()]
    y = D().conv1d_stride2_channels_last_autograd(*leaves)
    return (y.detach(),) + tuple(torch.autograd.grad(y, leaves, dy))


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_views_give_the_bits_of_the_dense_call(dtype):
    case = (3, 2 * R + 1, 80, 128, 5, dtype)
    B, T, Cin, Cout, K, _ = case
    To = A.t_out(T)
    t = stored(case)
    base = _op(t["x"], t["w"], t["bias"], t["dy"])
    direct = hip_direct(case, t)
    for got, name in zip(base, ("y",) + GRADS):
        assert torch.equal(got, direct[name]), name

    def same(tag, out):
        for got, want, name in zip(out, base, ("y",) + GRADS):
            assert got.shape == want.shape and torch.equal(got, want), (tag, name)
    # x as a column slice of a wider tensor whose other columns are NaN: read with its row stride; a read past column Cin = 64 + 16 shows
    for lo, wide_c in ((0, 2 * Cin), (Cin, 2 * Cin), (8, Cin + 16)):
        wide = poisoned((B, T, wide_c), dtype)
        wide[..., lo:lo + Cin] = t["x"]
        xs = wide[..., lo:lo + Cin]
        assert xs.stride(1) == wide_c and D()._conv1d_s2_train_problem(xs, t["w"], t["bias"]) is None
        same(f"column slice at {lo} of {wide_c}", _op(xs, t["w"], t["bias"], t["dy"]))
        sliced = hip_direct(case, t, x=xs, ld_x=wide_c)
        for name, v in direct.items():
            assert torch.equal(sliced[name], v), ("direct column slice", lo, name)
    # aligned but NOT dense: the frames 1 .. T of a longer batch, samples (T + 1) rows apart (copied)
    longer = poisoned((B, T + 1, Cin), dtype)
    longer[:, 1:] = t["x"]
    xn = longer[:, 1:]
    assert xn.data_ptr() % 16 == 0 and not xn.is_contiguous() and D()._conv1d_s2_train_problem(xn, t["w"], t["bias"]).startswith("layout")
    same("aligned, not dense", _op(xn, t["w"], t["bias"], t["dy"]))
    # an x off the 16-byte grid
    off = poisoned((1 + B * T * Cin,), dtype)[1:].view(B, T, Cin)
    off.copy_(t["x"])
    assert off.data_ptr() % 16
    same("off the grid", _op(off, t["w"], t["bias"], t["dy"]))
    # dy as a transpose
    dyt = t["dy"].transpose(1, 2).contiguous().transpose(1, 2)
    assert not dyt.is_contiguous() and torch.equal(dyt, t["dy"])
    same("dy transposed", _op(t["x"], t["w"], t["bias"], dyt))
    # dy at an odd offset of its storage
    dyo = poisoned((1 + B * To * Cout,), dtype)[1:].view(B, To, Cout)
    dyo.copy_(t["dy"])
    assert dyo.data_ptr() % 16
    same("dy off the grid", _op(t["x"], t["w"], t["bias"], dyo))
    # dy as a broadcast: what .sum() sends back, and one row repeated over the frames
    for tag, small in (("ones", torch.ones(1, 1, 1, dtype=dtype, device="cuda")), ("row", t["dy"][:1, :1])):
        dyb = small.expand(B, To, Cout)
        assert dyb.stride(0) == 0 and dyb.stride(1) == 0
        want = _op(t["x"], t["w"], t["bias"], dyb.contiguous())
        for got, w_, name in zip(_op(t["x"], t["w"], t["bias"], dyb), want, ("y",) + GRADS):
            assert torch.equal(got, w_), (tag, name)


# ---------------------------------------------------------------- 4. error codes

def test_a_workspace_one_byte_short_is_enospc_and_nothing_runs():
    case = (2, 9, 80, 64, 5, F16)
    rc0, rc1, touched = hip_direct(case, stored(case), short=1)
    assert rc0 == rc1 and rc0 not in (0, -1)
    assert b"workspace" in LIB().load().dsp_last_error()
    for v in touched:
        assert torch.isnan(v).all()


def test_zero_rows_return_empty_results():
    x = torch.zeros(0, 9, 80, dtype=F16, device="cuda", requires_grad=True)
    w = torch.randn(128, 80, 3, device="cuda").half().requires_grad_()
    b = torch.randn(128, device="cuda").half().requires_grad_()
    y = D().conv1d_stride2_channels_last_autograd(x, w, b)
    assert y.shape == (0, 5, 128) and y.dtype == F16
    dx, dw, db = torch.autograd.grad(y, [x, w, b], torch.zeros_like(y))
    assert dx.shape == x.shape and dw.shape == w.shape and not dw.any() and db.shape == b.shape and not db.any()


def test_unserved_inputs_are_refused_on_the_device_too():
    from torch import nn
    served, op = D().conv1d_stride2_channels_last_served, D().conv1d_stride2_channels_last_autograd
    conv = nn.Conv1d(80, 128, 5, stride=2, padding=2).half().cuda()
    x = torch.zeros(2, 9, 80, dtype=F16, device="cuda")
    assert served(x, conv) and served(x.bfloat16(), copy.deepcopy(conv).bfloat16())
    assert op(x, conv.weight, conv.bias).shape == (2, 5, 128)
    for dt, reason in ((torch.float64, "never narrowed"), (F32, "fp16 or bf16")):
        c = copy.deepcopy(conv).to(dt)
        assert not served(x.to(dt), c)
        with pytest.raises(RuntimeError, match=reason):
            op(x.to(dt), c.weight, c.bias)
    assert not served(x.cpu(), copy.deepcopy(conv).cpu())
    with pytest.raises(RuntimeError, match="GPU"):
        op(x.cpu(), conv.weight.cpu(), conv.bias.cpu())
    for bad in (nn.Conv1d(80, 128, 5, padding=2), nn.Conv1d(80, 128, 5, stride=2, padding=4, dilation=2), nn.Conv1d(80, 128, 5, stride=2, padding=2, groups=2),
                nn.Conv1d(80, 128, 5, stride=2, padding=1), nn.Conv1d(80, 128, 4, stride=2, padding=2), nn.Conv1d(80, 80, 5, stride=2, padding=2)):
        assert not served(x, bad.half().cuda())
    assert not served(torch.zeros(2, 9, 24, dtype=F16, device="cuda"), nn.Conv1d(24, 128, 5, stride=2, padding=2).half().cuda())
    old = D().set_conv1d_stride2_train_hip(False)
    try:
        assert not served(x, conv)
    finally:
        D().set_conv1d_stride2_train_hip(old)
    with torch.autocast("cuda", dtype=F16):
        assert not served(x, conv)


# ---------------------------------------------------------------- 5. the module

def _run_subsampler(m, x0, lens, cot, x_grad=True):
    x = x0.clone().requires_grad_(x_grad)
    out, out_lens = m(x, lens)
    named = sorted(m.named_parameters())
    grads = torch.autograd.grad(out, ([x] if x_grad else []) + [p for _, p in named], cot)
    res = dict(out=out.detach())
    if x_grad:
        res["dx"], grads = grads[0], grads[1:]
    res.update({"d." + n: g for (n, _), g in zip(named, grads)})
    return res, out_lens


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["float16", "bfloat16"])
@pytest.mark.parametrize("T", [7, 2 * R + 2])
def test_subsampler_training_with_the_operator_on_and_off(T, dtype, monkeypatch):
    from daspeech_amd.models.daspeech import Conv1dSubsampler
    torch.manual_seed(3)
    B = 3
    master = Conv1dSubsampler(80, 128, 64).double().train()
    with torch.no_grad():
        for p in master.parameters():                                       # parameters, inputs and cotangent as the dtype stores them
            p.copy_(p.to(dtype).double())
    x0 = torch.randn(B, T, 80, dtype=torch.float64).to(dtype)
    lens = torch.tensor([T, max(T - 5, 1), max(T // 2, 1)])
    To = A.t_out(A.t_out(T))
    cot = torch.randn(B, To, 64, dtype=torch.float64).to(dtype)
    ref, ref_lens = _run_subsampler(copy.deepcopy(master), x0.double(), lens, cot.double())
    ref = {k: v.detach().numpy() for k, v in ref.items()}
    assert ref["out"].shape == (B, To, 64)
    # what goes through _launch: the entries of the stride-2 operator, with the dx pointer of each backward
    launches = []
    real = D()._launch
    monkeypatch.setattr(D(), "_launch", lambda dev, entry, *a: (launches.append((entry.__name__, a[5] if len(a) > 5 else None)), real(dev, entry, *a))[1])
    s2 = lambda: [l for l in launches if l[0].startswith("dsp_conv1d_s2_train_")]
    res = {}
    for on in (True, False):
        old = D().set_conv1d_stride2_train_hip(on)
        try:
            m = copy.deepcopy(master).to(dtype).cuda()
            res[on], got_lens = _run_subsampler(m, x0.cuda(), lens.cuda(), cot.cuda())
        finally:
            D().set_conv1d_stride2_train_hip(old)
        assert res[on]["out"].shape == (B, To, 64) and torch.equal(got_lens.cpu(), ref_lens)
        # with the switch on two forwards and two backwards, each backward with a dx; none with it off
        assert [n for n, _ in s2()] == ["dsp_conv1d_s2_train_fwd"] * 2 + ["dsp_conv1d_s2_train_bwd"] * 2, (on, launches)
        assert all(dxp is not None for n, dxp in s2() if n.endswith("bwd"))
    check_4x(f"conv1d-s2-subsampler-T{T}", res[True], res[False], ref)
    # src without a gradient (the filterbank input): no dx for the first convolution, the parameter gradients keep their bits
    del launches[:]
    m = copy.deepcopy(master).to(dtype).cuda()
    old = D().set_conv1d_stride2_train_hip(True)
    try:
        nograd, _ = _run_subsampler(m, x0.cuda(), lens.cuda(), cot.cuda(), x_grad=False)
    finally:
        D().set_conv1d_stride2_train_hip(old)
    bwd = [dxp for n, dxp in s2() if n.endswith("bwd")]
    assert len(bwd) == 2 and bwd[0] is not None and bwd[1] is None          # the second layer's backward runs first
    for name, v in nograd.items():
        assert torch.equal(v, res[True][name]), name
    # eval() under no_grad: the lines from before the operator, the same bits with the switch on and off
    del launches[:]
    m.eval()
    outs = []
    for on in (True, False):
        old = D().set_conv1d_stride2_train_hip(on)
        try:
            with torch.no_grad():
                outs.append(m(x0.cuda(), lens.cuda()))
        finally:
            D().set_conv1d_stride2_train_hip(old)
    assert not s2() and torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
