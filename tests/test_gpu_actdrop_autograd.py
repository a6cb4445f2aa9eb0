"""The bias + activation + dropout operator under autograd (csrc/act_dropout_train.hip, decode_ops.bias_act_dropout_autograd, the training
branches of ConformerLayer / NATDecoderLayer / FFNAdapter / ConformerEncoder) against the float64 restatement of tests/util_actdrop_ref.py,
evaluated on the inputs as stored (after rounding to the dtype) with the mask that decode_ops.dropout_keep_mask returns.

Accuracy: the 4 x rule of tests/util_4x_rule.py on y, dh and dbias; the yardstick is the torch lines in the same dtype on the same device with
the operator's own mask applied by a multiply.  Every case prints both figures.
Written-ness: the C entry points run on NaN-filled outputs and a NaN-filled workspace; no NaN may survive.  Two calls give equal bits; dh alone
and dbias alone have the bits they have when both are asked for.

Figures of the first run on an MI355X (highest hip / torch figure per dtype over the cases below) are in DESIGN.md §8."""
import copy
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import util_actdrop_ref as A
from tests.util_4x_rule import check_4x

pytestmark = pytest.mark.gpu
NAN = float("nan")
SEED, OFFSET = 0x9E3779B97F4A7C15, 0x1_0000_0008          # both with a high word: all six words of key and counter matter
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
CH = A.CHUNK_ROWS


def D():
    from daspeech_amd import decode_ops
    return decode_ops


def LIB():
    from daspeech_amd import _lib
    return _lib


def V(dtype):
    return 4 if dtype == F32 else 8


# (act, dtype, bias: "same" / "f32" / None, p, R, Cout or "min" for one 16-byte group).  A covering set, not the product: every activation in
# every dtype; every bias kind, every p, every R of (1, a chunk less one, a chunk, a chunk and one, two chunks and one, 200) and every width of
# (one group, 24, 264 = 33 or 66 groups: not a power of two and, in fp32, more than one slab of 64 groups, 2048) with every activation;
# glu at Cin 16 and 528.
CASES = [
    ("identity", F32, "same", 0.1, 1, "min"), ("identity", F16, None, 0.5, CH - 1, 24), ("identity", BF16, "f32", 0.0, 65, 264),
    ("identity", F16, "same", 0.1, 200, 2048), ("identity", F32, None, 0.5, CH, 264),
    ("relu", F32, None, 0.0, CH + 1, 24), ("relu", F16, "f32", 0.1, CH, "min"), ("relu", BF16, "same", 0.5, 200, 264),
    ("relu", F16, "same", 0.0, 1, 2048), ("relu", F32, "same", 0.1, 65, 264),
    ("silu", F32, "same", 0.5, CH - 1, 264), ("silu", F16, "same", 0.1, 200, 2048), ("silu", BF16, None, 0.0, CH + 1, 24),
    ("silu", F16, "f32", 0.5, 65, "min"), ("silu", F32, None, 0.1, CH, 2048), ("silu", BF16, "f32", 0.1, 1, 264),
    ("gelu", F32, "same", 0.1, 200, 24), ("gelu", F16, "same", 0.0, CH + 1, 264), ("gelu", BF16, "f32", 0.5, CH - 1, 2048),
    ("gelu", F16, None, 0.1, CH, "min"), ("gelu", F32, "same", 0.0, 65, 2048),
    ("glu", F32, "same", 0.1, CH + 1, 8), ("glu", F16, None, 0.0, 200, 264), ("glu", BF16, "same", 0.5, 1, 24),
    ("glu", F16, "f32", 0.1, 65, 8), ("glu", F32, None, 0.5, CH - 1, 264), ("glu", F16, "same", 0.5, CH, 2048),
    ("glu", BF16, None, 0.1, 200, 264),
]


def _cid(c):
    return "%s-%s-bias%s-p%s-R%d-C%s" % (c[0], str(c[1]).split(".")[1], c[2], c[3], c[4], c[5])


def poisoned(shape, dtype):
    return torch.full(tuple(shape), NAN, dtype=dtype, device="cuda")


_STORED = {}


def stored(case, layout="dense"):
    """the inputs of a case rounded to their dtypes, on the device (computed once per case and layout, never modified): h [R,Cin] dense or a
    column slice of a wider tensor, bias [Cin] or None, dy [R,Cout], the keep mask, and the float64 reference of y, dh and dbias"""
    key = (case, layout)
    if key in _STORED:
        return _STORED[key]
    act, dtype, bk, p, R, C = case
    Cout = V(dtype) if C == "min" else C
    Cin = 2 * Cout if act == "glu" else Cout
    h, bias, dy = A.inputs(7 * R + Cin, R, Cin, act)
    h, dy = h.to(dtype).cuda(), dy.to(dtype).cuda()
    bias = None if bk is None else bias.to(dtype if bk == "same" else F32).cuda()
    if layout == "slice":                                                  # pitch > Cin, the start one 16-byte group into the row
        wide = poisoned((R, Cin + 3 * V(dtype)), dtype)
        wide[:, V(dtype):V(dtype) + Cin] = h
        h = wide[:, V(dtype):V(dtype) + Cin]
        assert not h.is_contiguous() or R == 1
    keep = D().dropout_keep_mask(SEED, OFFSET, p, (R, Cout), "cuda") if p > 0 else None
    kc = None if keep is None else keep.cpu()
    ref = dict(y=A.forward(h.cpu(), None if bias is None else bias.cpu(), act, kc, p).numpy())
    dh, dbias = A.backward(h.cpu(), None if bias is None else bias.cpu(), act, dy.cpu(), kc, p)
    ref["dh"] = dh.numpy()
    if bias is not None:
        ref["dbias"] = dbias.numpy()
    out = SimpleNamespace(act=act, dtype=dtype, p=p, R=R, Cin=Cin, Cout=Cout, h=h, bias=bias, dy=dy, keep=keep, ref=ref)
    _STORED[key] = out
    return out


def hip_direct(t, skip=(), seed=SEED, offset=OFFSET):
    """both C entry points on NaN-filled outputs and a NaN-filled workspace -> dict of outputs (the entries of `skip` left out: NULL; without
    dbias the backward gets no workspace at all)"""
    lib, L = LIB(), LIB().load()
    pd = t.dtype if t.bias is None else t.bias.dtype
    codes = (lib.DTYPE_CODES[str(t.dtype)], lib.DTYPE_CODES[str(pd)])
    act = D().ACT_CODES[t.act]
    thr = D().dropout_threshold(t.p)
    scale = 1.0 / (1.0 - t.p) if thr else NAN                             # thr == 0: keep_scale is not read
    ld = D()._row_pitch(t.h)
    out = dict(y=poisoned((t.R, t.Cout), t.dtype), dh=poisoned((t.R, t.Cin), t.dtype))
    if t.bias is not None:
        out["dbias"] = poisoned((t.Cin,), pd)
    st = lib.current_stream_handle()
    lib.check(L.dsp_act_dropout_train_fwd(lib.ptr(t.h), ld, lib.ptr(t.bias), act, scale, thr, seed, offset, lib.ptr(out["y"]), codes[0], codes[1],
                                          t.R, t.Cin, st), "dsp_act_dropout_train_fwd")
    g = {k: (None if k in skip else out.get(k)) for k in ("dh", "dbias")}
    ws, nbytes = None, 0
    if g["dbias"] is not None:
        nbytes = int(L.dsp_act_dropout_train_workspace_bytes(t.R, t.Cin))
        assert nbytes > 0 and nbytes % 16 == 0
        ws = poisoned((nbytes // 4,), F32)
    lib.check(L.dsp_act_dropout_train_bwd(lib.ptr(t.dy), lib.ptr(t.h), ld, lib.ptr(t.bias), act, scale, thr, seed, offset, lib.ptr(g["dh"]),
                                          lib.ptr(g["dbias"]), lib.ptr(ws), nbytes, codes[0], codes[1], t.R, t.Cin, st), "dsp_act_dropout_train_bwd")
    torch.cuda.synchronize()
    for k in skip:
        out.pop(k, None)
    return out


def torch_lines(t):
    """the torch lines the operator replaces on the same stored inputs, in the same dtype, on the device; the mask applied by a multiply"""
    h = t.h.clone(memory_format=torch.contiguous_format).requires_grad_()
    bias = None if t.bias is None else t.bias.clone().requires_grad_()
    y = A.torch_lines(h, bias, t.act, t.keep, t.p)
    assert y.dtype == t.dtype
    grads = torch.autograd.grad(y, [h] + ([] if bias is None else [bias]), t.dy)
    out = dict(y=y.detach(), dh=grads[0])
    if bias is not None:
        out["dbias"] = grads[1]
    return out


def test_constants_match_the_library():
    assert (A.CHUNK_ROWS, A.MAX_CIN, A.ACTS) == (D().ACTDROP_CHUNK_ROWS, D().ACTDROP_MAX_CIN, tuple(D().ACT_CODES))
    seen = lambda i: {c[i] for c in CASES}
    assert seen(0) == set(A.ACTS) and seen(2) == {"same", "f32", None} and seen(3) == {0.0, 0.1, 0.5}
    assert seen(4) == {1, CH - 1, CH, CH + 1, 65, 200} and {"min", 24, 264, 2048} <= seen(5)
    assert {(c[0], c[1]) for c in CASES} == {(a, d) for a in A.ACTS for d in (F32, F16, BF16)}


@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_every_element_written_and_within_4x_of_torch(case):
    t = stored(case)
    check_4x("actdrop " + _cid(case), hip_direct(t), torch_lines(t), t.ref)


VIEWS = [("silu", F16, "same", 0.1, 65, 264), ("glu", F16, None, 0.1, CH + 1, 264), ("gelu", F32, "f32", 0.5, 33, 24),
         ("relu", BF16, "same", 0.0, 200, 2048), ("glu", F16, "same", 0.0, 33, 8), ("glu", BF16, "f32", 0.5, 33, 264)]


def _gen():
    return torch.cuda.default_generators[torch.cuda.current_device()]


def _operator(t, dy, want=("dh", "dbias"), seed=SEED, offset=OFFSET):
    """the public function under the generator state that makes it reserve (seed, offset)"""
    h = t.h.detach().requires_grad_("dh" in want)
    bias = None if t.bias is None else t.bias.detach().requires_grad_("dbias" in want)
    state = torch.cuda.get_rng_state()
    try:
        torch.cuda.manual_seed(seed)
        _gen().set_offset(offset)
        y = D().bias_act_dropout_autograd(h, bias, t.act, t.p, True)
    finally:
        torch.cuda.set_rng_state(state)
    wrt = [x for x in (h, bias) if x is not None and x.requires_grad]
    grads = torch.autograd.grad(y, wrt, dy)
    out = dict(y=y.detach())
    for x, g in zip(wrt, grads):
        out["dh" if x is h else "dbias"] = g
    return out


@pytest.mark.parametrize("case", VIEWS, ids=_cid)
def test_pitched_h_and_transposed_dy_through_the_operator(case):
    """h a column slice of a wider tensor (served with its pitch: no copy) and dy a transposed view (made dense by the operator): the 4 x
    rule, and the bits of the entry points on the dense tensors"""
    dense, t = stored(case), stored(case, "slice")
    assert D().bias_act_dropout_served(t.h, t.bias, t.act) and D()._row_pitch(t.h) > t.Cin
    direct = hip_direct(t)                                                 # the C entry points with ld_h > Cin
    for k, v in hip_direct(dense).items():
        assert torch.equal(v, direct[k]), k
    dy_t = t.dy.t().contiguous().t()
    assert not dy_t.is_contiguous() or t.R == 1 or t.Cout == 1
    got = _operator(t, dy_t)
    assert got["dh"].is_contiguous() and tuple(got["dh"].shape) == (t.R, t.Cin)
    check_4x("actdrop-view " + _cid(case), got, torch_lines(t), t.ref)
    for k, v in direct.items():
        assert torch.equal(v, got[k]), k
    # a layout the kernels do not take (rows of two pitches; a start off the grid) is copied by the public function, not by `served`
    odd = torch.zeros(t.R, t.Cin + 1, dtype=t.dtype, device="cuda")[:, 1:]
    odd.copy_(t.h)
    assert not D().bias_act_dropout_served(odd, t.bias, t.act)
    state = torch.cuda.get_rng_state()
    torch.cuda.manual_seed(SEED)
    _gen().set_offset(OFFSET)
    y = D().bias_act_dropout_autograd(odd, t.bias, t.act, t.p, True)
    torch.cuda.set_rng_state(state)
    assert torch.equal(y, direct["y"])


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("dtype", [F32, F16], ids=["float32", "float16"])
@pytest.mark.parametrize("act", ["identity", "glu"])
def test_index_rule(act, dtype, p):
    """h = 1 (glu: a gate of 30, whose sigmoid is 1 in fp32), no bias: y is dropout_keep_mask(seed, offset, p, (R, Cout)) / (1 - p) exactly"""
    R, Cout = 33, 264
    h = torch.ones(R, Cout * (2 if act == "glu" else 1), dtype=dtype, device="cuda")
    if act == "glu":
        h[:, Cout:] = 30.0
    torch.cuda.manual_seed(5)
    _gen().set_offset(16)
    y = D().bias_act_dropout_autograd(h, None, act, p, True)
    assert _gen().get_offset() == 20                                       # a masked call takes four of the stream
    keep = D().dropout_keep_mask(torch.cuda.initial_seed(), 16, p, (R, Cout), "cuda")
    scale = torch.tensor(1.0 / (1.0 - p), dtype=F32, device="cuda")       # keep_scale as the C ABI gets it
    assert torch.equal(y, (keep.to(F32) * scale).to(dtype))
    assert abs(float(keep.float().mean()) - (1 - p)) < 0.03
    other = D().dropout_keep_mask(torch.cuda.initial_seed(), 20, p, (R, Cout), "cuda")
    assert not torch.equal(y != 0, other)                                   # and no other mask explains the result
    # p = 0 and eval calls leave the generator alone, and drop nothing
    state = torch.cuda.get_rng_state()
    for kw in (dict(p=0.0, training=True), dict(p=p, training=False)):
        assert torch.equal(D().bias_act_dropout_autograd(h, None, act, **kw), torch.ones(R, Cout, dtype=dtype, device="cuda"))
    assert torch.equal(torch.cuda.get_rng_state(), state) and _gen().get_offset() == 20
    # the same generator state gives the same mask; GLAT's two passes replay it under _same_draws
    from daspeech_amd.models.daspeech import _same_draws
    with _same_draws(99, h.device, True):
        e1 = D().bias_act_dropout_autograd(h, None, act, p, True)
    with _same_draws(99, h.device, True):
        e2 = D().bias_act_dropout_autograd(h, None, act, p, True)
    assert torch.equal(e1, e2) and not torch.equal(e1, y) and torch.equal(torch.cuda.get_rng_state(), state)


BITS = [c for c in CASES if c[2] is not None and c[4] in (CH + 1, 65, 200)]


@pytest.mark.parametrize("case", BITS, ids=_cid)
def test_equal_bits_and_each_gradient_alone(case):
    t = stored(case)
    a, b = hip_direct(t), hip_direct(t)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    only_dh, only_db = hip_direct(t, skip=("dbias",)), hip_direct(t, skip=("dh",))
    assert torch.equal(only_dh["dh"], a["dh"]) and torch.equal(only_db["dbias"], a["dbias"])
    if t.p > 0:
        assert not torch.equal(hip_direct(t, offset=OFFSET + 4)["y"], a["y"])
    # the operator asks for what autograd needs, and only that
    got = _operator(t, t.dy, want=("dbias",))
    assert set(got) == {"y", "dbias"} and torch.equal(got["dbias"], a["dbias"]) and torch.equal(got["y"], a["y"])
    got = _operator(t, t.dy, want=("dh",))
    assert set(got) == {"y", "dh"} and torch.equal(got["dh"], a["dh"])


@pytest.mark.parametrize("act", ["silu", "glu"])
def test_no_rows(act):
    h = torch.zeros(0, 64, dtype=F16, device="cuda", requires_grad=True)
    bias = torch.zeros(64, dtype=F16, device="cuda", requires_grad=True)
    state = torch.cuda.get_rng_state()
    y = D().bias_act_dropout_autograd(h, bias, act, 0.0, True)
    assert tuple(y.shape) == (0, 32 if act == "glu" else 64) and y.dtype == F16
    dh, db = torch.autograd.grad(y, [h, bias], torch.zeros_like(y))
    assert tuple(dh.shape) == (0, 64) and torch.equal(db, torch.zeros_like(bias))
    assert torch.equal(torch.cuda.get_rng_state(), state)
    lib, L = LIB(), LIB().load()
    assert L.dsp_act_dropout_train_fwd(None, 64, None, 2, 1.0, 0, 0, 0, None, 1, 1, 0, 64, lib.current_stream_handle()) == 0      # nothing is read


def test_bad_arguments_are_refused_before_any_launch():
    lib, L = LIB(), LIB().load()
    t = stored(("silu", F16, "same", 0.1, 65, 264))
    y, dh, db = poisoned((t.R, t.Cout), F16), poisoned((t.R, t.Cin), F16), poisoned((t.Cin,), F16)
    ws = poisoned((int(L.dsp_act_dropout_train_workspace_bytes(t.R, t.Cin)) // 4,), F32)
    st = lib.current_stream_handle()
    P = lib.ptr

    def fwd(h=t.h, ld=t.Cin, bias=t.bias, act=2, thr=100, out=y, codes=(1, 1), R=t.R, C=t.Cin, off=0):
        return L.dsp_act_dropout_train_fwd(P(h).value + off if off else P(h), ld, P(bias), act, 1.1, thr, 1, 0, P(out), codes[0], codes[1], R, C, st)

    def bwd(dy=t.dy, h=t.h, ld=t.Cin, act=2, g=dh, b=db, w=ws, n=None, R=t.R, C=t.Cin):
        n = (0 if w is None else w.numel() * 4) if n is None else n
        return L.dsp_act_dropout_train_bwd(P(dy), P(h), ld, P(t.bias), act, 1.1, 100, 1, 0, P(g), P(b), P(w), n, 1, 1, R, C, st)

    EINVAL, ENOSPC = -1, -2
    bad = [fwd(h=None), fwd(out=None), fwd(out=t.h), fwd(act=5), fwd(act=-1), fwd(C=t.Cin + 4), fwd(C=0), fwd(C=A.MAX_CIN + 8), fwd(R=-1),
           fwd(R=(1 << 24) + 1), fwd(ld=t.Cin - 8), fwd(ld=t.Cin + 4), fwd(off=2), fwd(codes=(3, 1)), fwd(codes=(0, 1)), fwd(codes=(1, 2)),
           fwd(thr=(1 << 24) + 1), fwd(act=4, C=264, ld=264),
           bwd(dy=None), bwd(h=None), bwd(g=t.dy), bwd(g=t.h), bwd(w=None), bwd(act=7), bwd(act=4, C=264, ld=264)]
    assert all(rc == EINVAL for rc in bad), bad
    assert b"glu" in L.dsp_last_error()
    assert bwd(n=16) == ENOSPC
    assert bwd(g=None, b=None, w=None) == 0 and bwd(b=None, w=None) == 0            # nothing asked; dh alone needs no workspace
    torch.cuda.synchronize()
    assert torch.isnan(y).all() and torch.isnan(db).all() and torch.isnan(ws).all()   # the refused calls launched nothing
    assert fwd() == 0 and fwd(R=0, h=None, out=None) == 0


def test_float64_and_cpu_are_refused_on_the_device_too():
    x = torch.zeros(2, 8, device="cuda", dtype=torch.float64)
    with pytest.raises(RuntimeError, match="float64"):
        D().bias_act_dropout_autograd(x, None, "silu")
    assert not D().bias_act_dropout_served(x, None, "silu")
    xf = torch.zeros(8, 8, device="cuda")
    assert D().bias_act_dropout_served(xf, None, "silu") and not D().bias_act_dropout_served(xf.t(), None, "silu")
    assert not D().bias_act_dropout_served(xf, torch.zeros(8), "silu")                # a CPU bias
    with pytest.raises(RuntimeError, match="bias"):
        D().bias_act_dropout_autograd(xf, torch.zeros(4, device="cuda"), "silu")
    with pytest.raises(RuntimeError, match=r"\[0, 1\)"):
        D().bias_act_dropout_autograd(xf, None, "silu", p=1.0)
    with torch.autocast("cuda", dtype=F16):
        assert not D().bias_act_dropout_served(xf, None, "silu")
    old = D().set_act_dropout_hip(False)
    try:
        assert not D().bias_act_dropout_served(xf, None, "silu")
    finally:
        D().set_act_dropout_hip(old)


# ---------------------------------------------------------------- the layers in training mode, the operator on and off

B, T, DIM = 2, 9, 64


def _count_calls(monkeypatch):
    calls = []
    real = D().bias_act_dropout_checked                                    # the entry the layers call after the `served` question
    monkeypatch.setattr(D(), "bias_act_dropout_checked", lambda *a, **k: (calls.append(a[2]), real(*a, **k))[1])
    return calls


def _module(kind, p):
    """(float64 module in training mode, float64 inputs, call)"""
    from daspeech_amd.models import daspeech as M
    from daspeech_amd.models.fastspeech2 import FFNAdapter
    torch.manual_seed(3)
    if kind == "adapter":
        return FFNAdapter(DIM, 128, 48, dropout=p).double().train(), [torch.randn(B, T, DIM, dtype=torch.float64)], lambda m, x: m(x[0])
    a = SimpleNamespace(**dict(M.DEFAULT_ARGS, input_feat=16, conv_channels=32, encoder_layers=2, encoder_embed_dim=DIM, encoder_ffn_embed_dim=128,
                               encoder_attention_heads=4, depthwise_kernel=7, dropout=p))
    lens = torch.tensor([4 * T, 4 * T - 9])
    call = lambda m, x: m(x[0], lens.to(x[0].device))["encoder_out"]
    return M.ConformerEncoder(a).double().train(), [torch.randn(B, 4 * T, 16, dtype=torch.float64)], call


def _run(module, call, xs, cot):
    xs = [x.clone().requires_grad_() for x in xs]
    out = call(module, xs)
    named = sorted(module.named_parameters())
    grads = torch.autograd.grad(out, xs + [q for _, q in named], cot)
    res = dict(out=out.detach(), dx=grads[0])
    res.update({"d." + n: g for (n, _), g in zip(named, grads[len(xs):])})
    return res


@pytest.mark.parametrize("kind,sites", [("adapter", ["relu"]), ("encoder", ["silu", "glu", "silu"] * 2)])
def test_module_training_with_the_operator_on_and_off(kind, sites, monkeypatch):
    dtype = F16
    master, xs, call = _module(kind, 0.0)
    with torch.no_grad():
        for q in master.parameters():                                      # parameters, inputs and cotangent as the dtype stores them
            q.copy_(q.to(dtype).double())
    xs = [x.to(dtype) for x in xs]
    with torch.no_grad():
        shape = call(copy.deepcopy(master), [x.double() for x in xs]).shape
    assert shape[1] == T
    cot = torch.randn(shape, dtype=torch.float64).to(dtype)
    ref = {k: v.detach().numpy() for k, v in _run(copy.deepcopy(master), call, [x.double() for x in xs], cot.double()).items()}
    calls = _count_calls(monkeypatch)
    res = {}
    for on in (True, False):
        old = D().set_act_dropout_hip(on)
        try:
            res[on] = _run(copy.deepcopy(master).to(dtype).cuda(), call, [x.cuda() for x in xs], cot.cuda())
        finally:
            D().set_act_dropout_hip(old)
        assert calls == sites, (on, calls)                                 # every site went through the operator with the switch on, and only then
    # the soft-max is invariant to a key bias: that gradient is zero in exact arithmetic, so max|ref| is no scale for it; its error is measured
    # against the scale of the key weight's gradient (as tests/test_gpu_resnorm_autograd.py)
    scales = {}
    for name in ref:
        if name.endswith("linear_k.bias"):
            kw = name[:-4] + "weight"
            assert np.abs(ref[name]).max() < 1e-12 * np.abs(ref[kw]).max()
            scales[name] = np.abs(ref[kw]).max()
    check_4x(f"module-{kind}-float16", res[True], res[False], ref, scales=scales)


@pytest.mark.parametrize("kind,sites", [("conformer", ["silu", "glu", "silu"]), ("nat", ["gelu"]), ("adapter", ["relu"]),
                                        ("encoder", ["identity"] + ["silu", "glu", "silu"] * 2)])
def test_sites_per_forward_with_dropout(kind, sites, monkeypatch):
    from daspeech_amd.models.daspeech import ConformerLayer, NATDecoderLayer
    torch.manual_seed(3)
    x = torch.randn(B, T, DIM).half().cuda()
    pad = (torch.arange(T).unsqueeze(0) >= torch.tensor([T, T - 3]).unsqueeze(1)).cuda()
    if kind == "conformer":
        layer = ConformerLayer(DIM, 128, 4, 7, dropout=0.1).half().cuda().train()
        pos = torch.randn(1, 2 * T - 1, DIM).half().cuda()
        fwd = lambda: layer(x, pos, pad)
    elif kind == "nat":
        layer = NATDecoderLayer(DIM, 128, 4, 48, dropout=0.1, attention_dropout=0.0, activation_dropout=0.1).half().cuda().train()
        enc = torch.randn(B, 7, 48).half().cuda()
        enc_pad = (torch.arange(7).unsqueeze(0) >= torch.tensor([7, 5]).unsqueeze(1)).cuda()
        fwd = lambda: layer(x, pad, enc, enc_pad)
    else:
        module, xs, call = _module(kind, 0.1)
        layer = module.half().cuda()
        xs = [t.half().cuda() for t in xs]
        fwd = lambda: call(layer, xs)
    calls = _count_calls(monkeypatch)
    for on, rn in ((True, True), (True, False), (False, True)):           # both training branches of the layer classes
        old, old_rn = D().set_act_dropout_hip(on), D().set_residual_norm_hip(rn)
        try:
            del calls[:]
            off0 = _gen().get_offset()
            out = fwd()
            assert calls == (sites if on else []), (on, rn, calls)
            assert torch.isfinite(out).all() and _gen().get_offset() > off0
            grads = torch.autograd.grad(out.float().sum(), list(layer.parameters()), allow_unused=True)
            assert all(g is not None and torch.isfinite(g).all() for g in grads), (on, rn)
        finally:
            D().set_act_dropout_hip(old)
            D().set_residual_norm_hip(old_rn)
