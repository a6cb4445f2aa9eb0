"""GPU: the channels-last Conv1d training operator (csrc/conv1d_train.hip; decode_ops.conv1d_channels_last_autograd) against the float64
restatement of tests/util_conv1d_train_ref.py, by the project's 4 x rule (tests/util_4x_rule.py): for y, dx, dW and db
    max|got - ref64| / max|ref64|  <=  4 * max(the same figure for the yardstick, one rounding of the dtype),
the yardstick being torch's own F.conv1d under autograd in the same dtype on the transposed tensors.  A tap that reads the neighbouring sample,
a tile that spans two samples or a row that is never written is an error of order 1 (outputs, gradients and workspaces are NaN-filled before
every call).  Shapes: the smallest at which the tiling can go wrong — T around the row tile R of the forward (1, 2, K-1, R-1, R, R+1, 2R+1),
one and three samples, B*T one above the row split S of the weight gradient, channel counts that fill half a column tile (64), one and a half
(192) and one (128), every tap count from 1 to 15 in steps that matter, and the three real widths at T = R + 1."""
import copy

import numpy as np
import pytest
import torch

from tests import util_conv1d_train_ref as A
from tests.util_4x_rule import check_4x

pytestmark = pytest.mark.gpu
NAN = float("nan")
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
R, S = A.ROW_TILE, A.WGRAD_ROWS
BIAS_MODES = ("none", "dtype", "fp32")
GRADS = ("dx", "dw", "db")

SHAPES = [(64, 64, 1), (64, 64, 3), (64, 192, 9), (192, 64, 15), (128, 128, 5)]
REAL = [(256, 1024, 9), (1024, 256, 9), (256, 256, 3)]


def _cases():
    out = []
    for Cin, Cout, K in SHAPES:
        for T in sorted({1, 2, K - 1, R - 1, R, R + 1, 2 * R + 1} - {0}):
            for B in (1, 3):
                out += [(B, T, Cin, Cout, K, dt) for dt in (F16, BF16)]
    for Cin, Cout, K in REAL:
        out += [(B, R + 1, Cin, Cout, K, dt) for B in (1, 3) for dt in (F16, BF16)]
    out += [(1, S + 1, 64, 64, 3, dt) for dt in (F16, BF16)]               # B*T one above the split of the weight gradient: a split of one row
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


def hip_direct(case, t, mode="dtype", skip=(), x=None, ld_x=None):
    """the two C entry points on poisoned outputs and workspaces"""
    B, T, Cin, Cout, K, dtype = case
    lib, L = LIB(), LIB().load()
    code = lib.DTYPE_CODES[str(dtype)]
    bias = _bias(t, mode)
    bcode = lib.DTYPE_CODES[str((t["x"] if bias is None else bias).dtype)]
    st = lib.current_stream_handle()
    x = t["x"] if x is None else x
    ld_x = Cin if ld_x is None else ld_x
    y = poisoned((B, T, Cout), dtype)
    n0 = int(L.dsp_conv1d_train_workspace_bytes(0, B, T, Cin, Cout, K))
    ws0 = poisoned((n0 // 4,), F32)
    lib.check(L.dsp_conv1d_train_fwd(lib.ptr(x), ld_x, lib.ptr(t["w"]), lib.ptr(bias), lib.ptr(y), Cout, lib.ptr(ws0), n0, code, bcode, B, T, Cin, Cout, K,
                                     st), "fwd")
    shapes = dict(dx=(B, T, Cin), dw=(Cout, Cin, K), db=(Cout,))
    g = {n: (None if n in skip else poisoned(shapes[n], (F32 if mode == "fp32" else dtype) if n == "db" else dtype)) for n in GRADS}
    n1 = int(L.dsp_conv1d_train_workspace_bytes(1, B, T, Cin, Cout, K))
    ws1 = poisoned((n1 // 4,), F32)
    lib.check(L.dsp_conv1d_train_bwd(lib.ptr(t["dy"]), Cout, lib.ptr(x), ld_x, lib.ptr(t["w"]), lib.ptr(g["dx"]), lib.ptr(g["dw"]), lib.ptr(g["db"]),
                                     lib.ptr(ws1), n1, code, bcode, B, T, Cin, Cout, K, st), "bwd")
    torch.cuda.synchronize()
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
    d = D()
    assert (d.CONV1D_TRAIN_ROW_TILE, d.CONV1D_TRAIN_WGRAD_ROWS, d.CONV1D_TRAIN_MAX_K, d.CONV1D_TRAIN_MAX_C) == (A.ROW_TILE, A.WGRAD_ROWS, A.MAX_K, A.MAX_C)
    assert LIB().load().dsp_conv1d_train_workspace_bytes(1, 1, S + 1, 64, 64, 3) >= 2 * 4 * 3 * 64 * 64      # two splits


@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_every_element_written_and_within_4x_of_torch(ci):
    """1. accuracy, for the three bias modes of each case"""
    t, ref, tor, hip = results(ci)
    for mode in BIAS_MODES:
        got = hip if mode == "dtype" else hip_direct(CASES[ci], t, mode)
        with_bias = mode != "none"
        want = dict(y=ref["y0"] + ref["bias"] if with_bias else ref["y0"], dx=ref["dx"], dw=ref["dw"], db=ref["db"])
        yard = dict(tor[with_bias])
        yard.setdefault("db", tor[True]["db"])                              # db does not depend on the bias: torch's figure for it with one
        assert got["db"].dtype == (F32 if mode == "fp32" else CASES[ci][5])
        for name, v in got.items():
            assert not torch.isnan(v).any(), f"{mode} {name}: NaN (an element never written)"
        check_4x(f"conv1d-{IDS[ci]}-bias-{mode}", got, yard, want)


@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_two_calls_give_equal_bits(ci):
    """3. bits: a second call"""
    t, ref, tor, hip = results(ci)
    again = hip_direct(CASES[ci], t)
    for name, v in hip.items():
        assert torch.equal(v, again[name]), name


NULLABLE = [i for i, c in enumerate(CASES) if c[1] in (2, R + 1, S + 1) and c[5] == F16]


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
    case = (3, R + 1, 64, 192, 9, dtype)
    t = stored(case)
    direct = hip_direct(case, t, mode)
    bias = _bias(t, mode)
    leaves = [t["x"].clone().requires_grad_(), t["w"].clone().requires_grad_()] + ([] if bias is None else [bias.clone().requires_grad_()])
    y = D().conv1d_channels_last_autograd(*leaves)
    grads = torch.autograd.grad(y, leaves, t["dy"])
    assert torch.equal(y, direct["y"])
    for name, g in zip(GRADS, grads):
        assert g.dtype == direct[name].dtype and torch.equal(g, direct[name]), name
    w2 = t["w"].clone().requires_grad_()
    (dw2,) = torch.autograd.grad(D().conv1d_channels_last_autograd(t["x"], w2, bias), [w2], t["dy"])
    assert torch.equal(dw2, direct["dw"])
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda s: (saved.append(s), s)[1], lambda s: s):
        D().conv1d_channels_last_autograd(*leaves)
    assert len(saved) == 2 and saved[0].shape == t["x"].shape and saved[1].shape == t["w"].shape          # x and weight, nothing else


# ---------------------------------------------------------------- 2. views

def _op(x, w, bias, dy):
    leaves = [x.detach().requires_grad_(), w.detach().requires_grad_(), bias.detach().requires_grad_()]
    y = D().conv1d_channels_last_autograd(*leaves)
    return (y.detach(),) + tuple(torch.autograd.grad(y, leaves, dy))


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_views_give_the_bits_of_the_dense_call(dtype):
    case = (3, R + 1, 64, 128, 5, dtype)
    B, T, Cin, Cout, K, _ = case
    t = stored(case)
    base = _op(t["x"], t["w"], t["bias"], t["dy"])
    direct = hip_direct(case, t)
    for got, name in zip(base, ("y",) + GRADS):
        assert torch.equal(got, direct[name]), name

    def same(tag, out):
        for got, want, name in zip(out, base, ("y",) + GRADS):
            assert got.shape == want.shape and torch.equal(got, want), (tag, name)
    # x as a column slice of a wider tensor: read with its row stride of 2 Cin, by the operator and by the C entry points
    wide = poisoned((B, T, 2 * Cin), dtype)
    wide[..., Cin:] = t["x"]
    xs = wide[..., Cin:]
    assert xs.stride(1) == 2 * Cin and D()._conv1d_train_problem(xs, t["w"], t["bias"]) is None
    same("column slice", _op(xs, t["w"], t["bias"], t["dy"]))
    sliced = hip_direct(case, t, x=xs, ld_x=2 * Cin)
    for name, v in direct.items():
        assert torch.equal(sliced[name], v), ("direct column slice", name)
    # x at a 16-byte aligned offset of its storage, dense behind it ... (served as it is)
    buf = poisoned((8 + B * T * Cin,), dtype)
    xo = buf[8:].view(B, T, Cin)
    xo.copy_(t["x"])
    assert xo.data_ptr() % 16 == 0 and xo.storage_offset() == 8 and D()._conv1d_train_problem(xo, t["w"], t["bias"]) is None
    same("aligned offset", _op(xo, t["w"], t["bias"], t["dy"]))
    # ... and aligned but NOT dense: the frames 1 .. T of a longer batch, samples (T + 1) rows apart (copied)
    longer = poisoned((B, T + 1, Cin), dtype)
    longer[:, 1:] = t["x"]
    xn = longer[:, 1:]
    assert xn.data_ptr() % 16 == 0 and not xn.is_contiguous() and D()._conv1d_train_problem(xn, t["w"], t["bias"]).startswith("layout")
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
    # dy as a broadcast: what .sum() sends back, and one row repeated over the frames
    for tag, small in (("ones", torch.ones(1, 1, 1, dtype=dtype, device="cuda")), ("row", t["dy"][:1, :1])):
        dyb = small.expand(B, T, Cout)
        assert dyb.stride(0) == 0 and dyb.stride(1) == 0
        want = _op(t["x"], t["w"], t["bias"], dyb.contiguous())
        for got, w_, name in zip(_op(t["x"], t["w"], t["bias"], dyb), want, ("y",) + GRADS):
            assert torch.equal(got, w_), (tag, name)


# ---------------------------------------------------------------- 4. refusals

def test_bad_arguments_are_refused_before_any_launch():
    lib, L = LIB(), LIB().load()
    case = (2, 9, 64, 128, 3, F16)
    B, T, Cin, Cout, K, _ = case
    t = stored(case)
    st = lib.current_stream_handle()
    y = poisoned((B, T, Cout), F16)
    n0 = int(L.dsp_conv1d_train_workspace_bytes(0, B, T, Cin, Cout, K))
    ws0 = poisoned((n0 // 4,), F32)
    P = lib.ptr

    def fwd(x=t["x"], w=t["w"], yy=y, ws=ws0, nb=n0, ldx=Cin, ldy=Cout, act=1, par=1, B_=B, T_=T, Ci=Cin, Co=Cout, K_=K, off=0):
        xp = None if x is None else P(x).value + off
        return L.dsp_conv1d_train_fwd(xp, ldx, P(w), P(t["bias"]), P(yy), ldy, P(ws), nb, act, par, B_, T_, Ci, Co, K_, st)
    assert fwd(x=None) == -1 and fwd(w=None) == -1 and fwd(yy=None) == -1 and fwd(yy=t["x"]) == -1 and fwd(off=2) == -1
    assert fwd(ws=None) == -1 and fwd(nb=16) not in (0, -1) and fwd(ws=y) == -1
    assert fwd(ldx=Cin - 8) == -1 and fwd(ldx=Cin + 4) == -1 and fwd(ldy=Cout - 8) == -1 and fwd(ldy=Cout + 4) == -1
    assert fwd(act=0, par=0) == -1 and fwd(act=3) == -1 and fwd(act=1, par=2) == -1
    assert fwd(T_=0) == -1 and fwd(B_=-1) == -1 and fwd(B_=1 << 12, T_=(1 << 12) + 1) == -1
    assert fwd(Ci=80) == -1 and fwd(Co=80) == -1 and fwd(Ci=0) == -1 and fwd(Co=A.MAX_C + 64) == -1
    assert fwd(K_=2) == -1 and fwd(K_=0) == -1 and fwd(K_=17) == -1
    assert b"conv1d_train_fwd" in L.dsp_last_error()
    assert fwd(B_=0) == 0                                                   # zero rows: nothing to do
    torch.cuda.synchronize()
    assert torch.isnan(y).all() and torch.isnan(ws0).all()                  # nothing ran
    assert fwd() == 0
    torch.cuda.synchronize()
    assert not torch.isnan(y).any()
    dx, dw, db = poisoned((B, T, Cin), F16), poisoned((Cout, Cin, K), F16), poisoned((Cout,), F16)
    n1 = int(L.dsp_conv1d_train_workspace_bytes(1, B, T, Cin, Cout, K))
    ws1 = poisoned((n1 // 4,), F32)

    def bwd(dy=t["dy"], x=t["x"], dx_=dx, dw_=dw, db_=db, ws=ws1, nb=n1, act=1, par=1, T_=T, K_=K, ld=Cout):
        return L.dsp_conv1d_train_bwd(P(dy), ld, P(x), Cin, P(t["w"]), P(dx_), P(dw_), P(db_), P(ws), nb, act, par, B, T_, Cin, Cout, K_, st)
    assert bwd(dy=None) == -1 and bwd(x=None) == -1 and bwd(dx_=t["x"]) == -1 and bwd(dw_=t["w"]) == -1 and bwd(db_=dw) == -1
    assert bwd(ws=None) == -1 and bwd(nb=n0) not in (0, -1) and bwd(ws=dx) == -1
    assert bwd(act=0) == -1 and bwd(par=2) == -1 and bwd(T_=0) == -1 and bwd(K_=4) == -1 and bwd(ld=Cout + 4) == -1
    assert b"conv1d_train_bwd" in L.dsp_last_error()
    assert bwd(dx_=None, dw_=None, db_=None, ws=None, nb=0) == 0           # nothing asked for: nothing needed
    torch.cuda.synchronize()
    assert torch.isnan(dx).all() and torch.isnan(dw).all() and torch.isnan(db).all() and torch.isnan(ws1).all()
    assert bwd() == 0
    torch.cuda.synchronize()
    assert not torch.isnan(dx).any() and not torch.isnan(dw).any() and not torch.isnan(db).any()


def test_zero_rows_return_empty_results():
    x = torch.zeros(0, 9, 64, dtype=F16, device="cuda", requires_grad=True)
    w = torch.randn(128, 64, 3, device="cuda").half().requires_grad_()
    b = torch.randn(128, device="cuda").half().requires_grad_()
    y = D().conv1d_channels_last_autograd(x, w, b)
    assert y.shape == (0, 9, 128) and y.dtype == F16
    dx, dw, db = torch.autograd.grad(y, [x, w, b], torch.zeros_like(y))
    assert dx.shape == x.shape and dw.shape == w.shape and not dw.any() and db.shape == b.shape and not db.any()


def test_unserved_inputs_are_refused_on_the_device_too():
    from torch import nn
    served, op = D().conv1d_channels_last_served, D().conv1d_channels_last_autograd
    conv = nn.Conv1d(64, 128, 3, padding=1).half().cuda()
    x = torch.zeros(2, 9, 64, dtype=F16, device="cuda")
    assert served(x, conv) and served(x.bfloat16(), copy.deepcopy(conv).bfloat16())
    assert op(x, conv.weight, conv.bias).shape == (2, 9, 128)
    for dt, reason in ((torch.float64, "never narrowed"), (F32, "fp16 or bf16")):
        c = copy.deepcopy(conv).to(dt)
        assert not served(x.to(dt), c)
        with pytest.raises(RuntimeError, match=reason):
            op(x.to(dt), c.weight, c.bias)
    assert not served(x.cpu(), copy.deepcopy(conv).cpu())
    with pytest.raises(RuntimeError, match="GPU"):
        op(x.cpu(), conv.weight.cpu(), conv.bias.cpu())
    with pytest.raises(RuntimeError, match="one device"):
        op(x, conv.weight, conv.bias.cpu())
    for bad in (nn.Conv1d(64, 128, 3, padding=1, stride=2), nn.Conv1d(64, 128, 3, padding=2, dilation=2), nn.Conv1d(64, 128, 3, padding=1, groups=2),
                nn.Conv1d(64, 128, 5, padding=1), nn.Conv1d(64, 128, 4, padding=2), nn.Conv1d(64, 80, 3, padding=1)):
        assert not served(x, bad.half().cuda())
    assert not served(torch.zeros(2, 9, 80, dtype=F16, device="cuda"), nn.Conv1d(80, 128, 3, padding=1).half().cuda())
    off = torch.zeros(1 + x.numel(), dtype=F16, device="cuda")[1:].view(x.shape)
    assert not served(off, conv) and op(off, conv.weight, conv.bias).shape == (2, 9, 128)      # off the 16-byte grid: the layer keeps its lines, the public function copies
    old = D().set_conv1d_train_hip(False)
    try:
        assert old is True and not served(x, conv)
    finally:
        assert D().set_conv1d_train_hip(old) is False
    with torch.autocast("cuda", dtype=F16):
        assert not served(x, conv)


# ---------------------------------------------------------------- 5. the modules

LB, LT, LDIM = 3, 2 * R + 1, 256


def _module(kind, p):
    from daspeech_amd.models.fastspeech2 import FFTLayer, VariancePredictor
    torch.manual_seed(3)
    if kind == "fft":
        m = FFTLayer(LDIM, 4, 1024, 9, dropout=p, attention_dropout=0.0)
        pad = torch.arange(LT).unsqueeze(0) >= torch.tensor([LT, LT - 5, R - 3]).unsqueeze(1)          # a ragged batch
        call = lambda mod, x, pd: mod(x, pd)
    else:
        m = VariancePredictor(LDIM, 256, 3, dropout=p)
        pad = torch.zeros(LB, LT, dtype=torch.bool)
        call = lambda mod, x, pd: mod(x)
    return m.double().train(), pad, call


def _run_module(m, call, x0, pad, cot):
    x = x0.clone().requires_grad_()
    out = call(m, x, pad)
    named = sorted(m.named_parameters())
    grads = torch.autograd.grad(out, [x] + [p for _, p in named], cot)
    res = dict(out=out.detach(), dx=grads[0])
    res.update({"d." + n: g for (n, _), g in zip(named, grads[1:])})
    return res


def _count_calls(monkeypatch):
    calls = []
    real = D().conv1d_channels_last_checked                                 # the entry the layers call after conv1d_channels_last_sites_served
    monkeypatch.setattr(D(), "conv1d_channels_last_checked", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


@pytest.mark.parametrize("kind", ["fft", "predictor"])
def test_module_training_with_the_operator_on_and_off(kind, monkeypatch):
    dtype = F16
    master, pad, call = _module(kind, 0.0)
    with torch.no_grad():
        for p in master.parameters():                                       # parameters, inputs and cotangent as the dtype stores them
            p.copy_(p.to(dtype).double())
    x0 = torch.randn(LB, LT, LDIM, dtype=torch.float64).to(dtype)
    cot = torch.randn((LB, LT, LDIM) if kind == "fft" else (LB, LT), dtype=torch.float64).to(dtype)
    ref = {k: v.detach().numpy() for k, v in _run_module(copy.deepcopy(master), call, x0.double(), pad, cot.double()).items()}
    calls = _count_calls(monkeypatch)
    res = {}
    for on in (True, False):
        old = D().set_conv1d_train_hip(on)
        try:
            m = copy.deepcopy(master).to(dtype).cuda()
            res[on] = _run_module(m, call, x0.cuda(), pad.cuda(), cot.cuda())
        finally:
            D().set_conv1d_train_hip(old)
        assert len(calls) == 2, (on, calls)                                 # two sites per FFT layer and per predictor with the switch on, none with it off
    # the soft-max is invariant to a key bias: that gradient is zero in exact arithmetic, so max|ref| is no scale for it; its error is measured
    # against the scale of the key weight's gradient, which the same rounding residues feed (as tests/test_gpu_resnorm_autograd.py)
    scales = {}
    for name in ref:
        if name.endswith("k_proj.bias"):
            kw = name[:-4] + "weight"
            assert np.abs(ref[name]).max() < 1e-12 * np.abs(ref[kw]).max()
            scales[name] = np.abs(ref[kw]).max()
    check_4x(f"conv1d-module-{kind}", res[True], res[False], ref, scales=scales)


@pytest.mark.parametrize("kind", ["fft", "predictor"])
def test_module_training_with_dropout_gives_the_same_bits_under_the_same_seed(kind, monkeypatch):
    master, pad, call = _module(kind, 0.1)
    m = master.half().cuda()
    x0 = torch.randn(LB, LT, LDIM).half().cuda()
    cot = torch.randn((LB, LT, LDIM) if kind == "fft" else (LB, LT)).half().cuda()
    calls = _count_calls(monkeypatch)
    runs = []
    # The operator's own bits are pinned by test_two_calls_give_equal_bits; here the torch ops around it (the GEMMs of the projections, the
    # attention backward, F.dropout) have to repeat themselves too.  Run to run they do not unless asked to
    # (tests/test_gpu_resnorm_autograd.py explains), so they run on their deterministic algorithms, and the first run — where the libraries
    # settle on their kernels for a new shape — is not compared.
    old = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled(),
           torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark)
    torch.use_deterministic_algorithms(True, warn_only=True)
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        for seed in (20, 21, 21, 22):
            torch.manual_seed(seed)
            torch.cuda.manual_seed(seed)
            runs.append(_run_module(m, call, x0, pad.cuda(), cot))
    finally:
        torch.use_deterministic_algorithms(old[0], warn_only=old[1])
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = old[2], old[3]
    assert len(calls) == 8
    del runs[0]
    for name, v in runs[0].items():
        assert torch.isfinite(v).all(), name
        assert torch.equal(v, runs[1][name]), name
    assert not torch.equal(runs[0]["out"], runs[2]["out"])                  # another seed: other masks
