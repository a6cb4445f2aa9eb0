"""GPU: the relative-position attention training operator (csrc/relpos_attention_train.hip; decode_ops.relpos_attention_autograd) against the
float64 restatement of tests/util_relpos_train_ref.py, by the project's 4 x rule (tests/test_gpu_resnorm_autograd.py): for o, lse and each of the
six gradients   max|got - ref64| / max|ref64|  <=  4 * max(the same figure for the yardstick, one rounding of the dtype),   the yardstick being the
module's torch training lines on the GPU in the same dtype with the operator's own keep mask applied explicitly.  A wrong mask or a wrong
shift is an error of order 1.  Shapes: the smallest at which the tiling (blocks of 32 queries / keys / position rows) can go wrong."""
import copy

import numpy as np
import pytest
import torch

from tests import util_relpos_train_ref as A
from tests.test_gpu_resnorm_autograd import ROUND, check_4x, figure      # the 4 x rule  # noqa: F401

pytestmark = pytest.mark.gpu
NAN = float("nan")
SEED, OFFSET = 1234567, 40
F16, BF16 = torch.float16, torch.bfloat16

# (T, B, H, dtype, mask, p): every T with both dtypes; B in {1, 3}, H in {1, 4}, the three masks and the three rates spread over them.
# The mask with a sample of a single valid key comes with B = 3: with that sample ALONE (B = 1) P is 1 on one key, dS = P (dP - D) is zero in
# exact arithmetic, and so are dq, dk, dpos, du and dv: max|ref64| is then float64 noise (1e-17) and no scale for a figure.
CASES = [(1, 1, 1, F16, "none", 0.0), (1, 3, 4, BF16, "single", 0.5),
         (2, 3, 1, F16, "ragged", 0.1), (2, 1, 4, BF16, "none", 0.0),
         (31, 3, 4, F16, "single", 0.5), (31, 1, 1, BF16, "ragged", 0.0),
         (32, 3, 4, F16, "none", 0.1), (32, 1, 1, BF16, "ragged", 0.5),
         (33, 1, 1, F16, "ragged", 0.0), (33, 3, 4, BF16, "none", 0.1),
         (63, 3, 1, F16, "single", 0.1), (63, 1, 4, BF16, "ragged", 0.5),
         (65, 1, 4, F16, "ragged", 0.5), (65, 3, 1, BF16, "single", 0.0),
         (129, 1, 1, F16, "none", 0.5), (129, 3, 4, BF16, "single", 0.1),
         (200, 3, 4, F16, "ragged", 0.1), (200, 1, 1, BF16, "none", 0.0), (200, 3, 4, BF16, "single", 0.5), (200, 1, 4, F16, "none", 0.0)]
IDS = ["T%d-B%d-H%d-%s-%s-p%g" % (T, B, H, str(d).split(".")[1], m, p) for T, B, H, d, m, p in CASES]
GRADS = ("dq", "dk", "dv", "dpos", "du", "dv_bias")


def D():
    from daspeech_amd import decode_ops
    return decode_ops


def LIB():
    from daspeech_amd import _lib
    return _lib


def f64(t):
    return t.detach().double().cpu().numpy()


def poisoned(shape, dtype):
    return torch.full(tuple(shape), NAN, dtype=dtype, device="cuda")


def stored(case, param_dtype=None):
    """the inputs as the dtype stores them, on the GPU"""
    T, B, H, dtype, mask, p = case
    t = A.inputs(100 + T + 7 * B + H, B, T, H)
    out = {n: v.to(dtype).cuda() for n, v in t.items()}
    for n in ("bias_u", "bias_v"):
        out[n] = t[n].to(dtype).to(param_dtype or dtype).cuda()
    pm = A.pad_masks(mask, B, T)
    out["pad"] = None if pm is None else pm.cuda()
    return out


def mask_for(case):
    T, B, H, dtype, mask, p = case
    if p == 0.0:
        return None
    return D().dropout_keep_mask(SEED, OFFSET, p, (B, H, T, A.padded(T)), "cuda")[..., :T]


def hip_direct(case, t, skip=(), seed=SEED, offset=OFFSET):
    """the two C entry points on poisoned outputs"""
    T, B, H, dtype, mask, p = case
    lib, L = LIB(), LIB().load()
    C = H * 64
    code, pcode = lib.DTYPE_CODES[str(dtype)], lib.DTYPE_CODES[str(t["bias_u"].dtype)]
    thr = D().dropout_threshold(p) if p > 0 else 0
    scale = 1.0 / (1.0 - p) if thr else 1.0
    pm = None if t["pad"] is None else t["pad"].view(torch.uint8)
    o, lse = poisoned((B, T, C), dtype), poisoned((B, H, T), torch.float32)
    st = lib.current_stream_handle()
    lib.check(L.dsp_relpos_attention_train_fwd(lib.ptr(t["q"]), lib.ptr(t["k"]), lib.ptr(t["v"]), C, lib.ptr(t["pos"]), lib.ptr(t["bias_u"]),
                                               lib.ptr(t["bias_v"]), lib.ptr(pm), scale, thr, seed, offset, lib.ptr(o), lib.ptr(lse), code, pcode, B, T, H, st),
              "fwd")
    shapes = dict(dq=(B, T, C), dk=(B, T, C), dv=(B, T, C), dpos=(2 * T - 1, C), du=(H, 64), dv_bias=(H, 64))
    g = {n: (None if n in skip else poisoned(shapes[n], t["bias_u"].dtype if n in ("du", "dv_bias") else dtype)) for n in GRADS}
    nbytes = int(L.dsp_relpos_attention_train_workspace_bytes(B, T, H))
    ws = poisoned((nbytes // 4,), torch.float32)
    lib.check(L.dsp_relpos_attention_train_bwd(lib.ptr(t["do"]), lib.ptr(t["q"]), lib.ptr(t["k"]), lib.ptr(t["v"]), C, lib.ptr(t["pos"]), lib.ptr(t["bias_u"]),
                                               lib.ptr(t["bias_v"]), lib.ptr(pm), lib.ptr(o), lib.ptr(lse), scale, thr, seed, offset,
                                               *[lib.ptr(g[n]) for n in GRADS], lib.ptr(ws), nbytes, code, pcode, B, T, H, st), "bwd")
    torch.cuda.synchronize()
    out = dict(o=o, lse=lse)
    out.update({n: v for n, v in g.items() if v is not None})
    return out


def torch_lines(case, t, keep):
    """the yardstick: the module's lines in the dtype, on the GPU, with the operator's mask"""
    T, B, H, dtype, mask, p = case
    names = ("q", "k", "v", "pos", "bias_u", "bias_v")
    leaves = [t[n].clone().requires_grad_() for n in names]
    o, lse = A.module_lines(*leaves, t["pad"], H, keep, p)
    grads = torch.autograd.grad(o, leaves, t["do"])
    out = dict(o=o.detach(), lse=lse.detach())
    out.update(dict(zip(GRADS, grads)))
    return out


def reference(case, t, keep):
    T, B, H, dtype, mask, p = case
    c = {n: t[n].double().cpu() for n in ("q", "k", "v", "pos", "bias_u", "bias_v", "do")}
    pm = None if t["pad"] is None else t["pad"].cpu()
    kp = None if keep is None else keep.cpu()
    f = A.forward(c["q"], c["k"], c["v"], c["pos"], c["bias_u"], c["bias_v"], pm, H, kp, p)
    out = dict(o=f["o"].numpy(), lse=f["lse"].numpy())
    out.update({n: v.numpy() for n, v in A.backward(c["q"], c["k"], c["v"], c["pos"], c["bias_u"], c["bias_v"], pm, H, c["do"], kp, p).items()})
    return out


_cache = {}


def results(ci):
    """inputs, mask, float64 reference, torch yardstick and one HIP run of a case, computed once and left unchanged"""
    if ci not in _cache:
        case = CASES[ci]
        t = stored(case)
        keep = mask_for(case)
        _cache[ci] = (t, keep, reference(case, t, keep), torch_lines(case, t, keep), hip_direct(case, t))
    return _cache[ci]


def test_constants_match_the_library():
    assert D().RELPOS_TRAIN_MAX_T == A.MAX_T >= 1500
    L = LIB().load()
    assert L.dsp_relpos_attention_train_workspace_bytes(1, A.MAX_T, 1) > 0


@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_every_element_written_and_within_4x_of_torch(ci):
    t, keep, ref, tor, hip = results(ci)
    for name, v in hip.items():
        assert not torch.isnan(v).any(), f"{name}: NaN (an element never written)"
    check_4x("relpos-" + IDS[ci], hip, tor, ref)


@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_two_calls_give_equal_bits(ci):
    t, keep, ref, tor, hip = results(ci)
    again = hip_direct(CASES[ci], t)
    for name, v in hip.items():
        assert torch.equal(v, again[name]), name


NULLABLE = [i for i, c in enumerate(CASES) if c[0] in (2, 33, 200) and c[3] == F16]


@pytest.mark.parametrize("ci", NULLABLE, ids=[IDS[i] for i in NULLABLE])
def test_each_gradient_can_be_left_out_without_changing_the_others(ci):
    t, keep, ref, tor, hip = results(ci)
    for left_out in GRADS:
        part = hip_direct(CASES[ci], t, skip=(left_out,))
        assert left_out not in part
        for name, v in part.items():
            assert torch.equal(v, hip[name]), (left_out, name)
    only = hip_direct(CASES[ci], t, skip=tuple(n for n in GRADS if n != "dpos"))
    assert torch.equal(only["dpos"], hip["dpos"])


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_fp32_biases_under_16_bit_data(dtype):
    case = (65, 3, 4, dtype, "ragged", 0.1)
    t = stored(case, param_dtype=torch.float32)
    keep = mask_for(case)
    hip = hip_direct(case, t)
    assert hip["du"].dtype == torch.float32 and hip["dv_bias"].dtype == torch.float32 and hip["dq"].dtype == dtype
    tt = dict(t)
    tt["bias_u"], tt["bias_v"] = t["bias_u"].to(dtype), t["bias_v"].to(dtype)          # the module adds them in the data dtype
    tor = torch_lines(case, tt, keep)
    # figures of one dtype: the yardstick's fp16 bias gradients are compared in their own precision, the operator's fp32 ones against ROUND[fp32] would
    # tighten the bound below what 16-bit operands can give — the bound is taken for the data dtype
    hip16 = {n: (v.to(dtype) if n in ("du", "dv_bias") else v) for n, v in hip.items()}
    check_4x("relpos-fp32-biases-" + str(dtype).split(".")[1], hip16, tor, reference(case, t, keep))


def test_key_row_stride_of_a_stacked_projection():
    """q, k, v as column slices of one [B,T,3C] tensor (row stride 3C) give the bits of contiguous tensors"""
    case = (33, 3, 4, F16, "ragged", 0.1)
    T, B, H = case[:3]
    C = H * 64
    t = stored(case)
    o0, lse0 = D().relpos_attention_autograd(t["q"], t["k"], t["v"], t["pos"], t["bias_u"], t["bias_v"], t["pad"], H, p=0.0, return_lse=True)
    qkv = torch.cat([t["q"], t["k"], t["v"]], dim=-1)
    o1, lse1 = D().relpos_attention_autograd(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], t["pos"], t["bias_u"], t["bias_v"], t["pad"], H, p=0.0,
                                             return_lse=True)
    assert torch.equal(o0, o1) and torch.equal(lse0, lse1)


def test_a_sample_without_a_valid_key_gives_nan_like_torch_and_harms_no_other():
    case = (33, 3, 1, F16, "none", 0.0)
    T, B, H = case[:3]
    t = stored(case)
    pad = torch.zeros(B, T, dtype=torch.bool, device="cuda")
    pad[1] = True
    o = D().relpos_attention_autograd(t["q"], t["k"], t["v"], t["pos"], t["bias_u"], t["bias_v"], pad, H)
    ref, _ = A.module_lines(t["q"], t["k"], t["v"], t["pos"], t["bias_u"], t["bias_v"], pad, H)
    assert torch.isnan(o[1]).all() and torch.isnan(ref[1]).all()
    assert torch.isfinite(o[0]).all() and torch.isfinite(o[2]).all()


def test_bad_arguments_are_refused_before_any_launch():
    lib, L = LIB(), LIB().load()
    case = (9, 2, 2, F16, "none", 0.0)
    T, B, H = case[:3]
    C = H * 64
    t = stored(case)
    o, lse = poisoned((B, T, C), F16), poisoned((B, H, T), torch.float32)
    st = lib.current_stream_handle()

    def fwd(q=t["q"], oo=o, ll=lse, ld=C, act=1, par=1, B_=B, T_=T, H_=H, thr=0, off=0):
        qp = None if q is None else lib.ptr(q).value + off
        return L.dsp_relpos_attention_train_fwd(qp, lib.ptr(t["k"]), lib.ptr(t["v"]), ld, lib.ptr(t["pos"]), lib.ptr(t["bias_u"]), lib.ptr(t["bias_v"]), None,
                                                1.0, thr, 1, 0, lib.ptr(oo), lib.ptr(ll), act, par, B_, T_, H_, st)
    assert fwd(q=None) == -1 and fwd(oo=None) == -1 and fwd(ll=None) == -1 and fwd(oo=t["q"]) == -1 and fwd(off=2) == -1
    assert fwd(ld=C - 8) == -1 and fwd(ld=C + 4) == -1 and fwd(act=0, par=0) == -1 and fwd(act=3) == -1 and fwd(act=1, par=2) == -1
    assert fwd(T_=0) == -1 and fwd(T_=A.MAX_T + 1) == -1 and fwd(H_=0) == -1 and fwd(B_=-1) == -1 and fwd(thr=(1 << 24) + 1) == -1
    assert b"relpos_attention_train_fwd" in L.dsp_last_error()
    assert fwd(B_=0) == 0
    torch.cuda.synchronize()
    assert torch.isnan(o).all() and torch.isnan(lse).all()                                      # nothing ran
    assert fwd() == 0
    torch.cuda.synchronize()
    assert not torch.isnan(o).any() and not torch.isnan(lse).any()
    dq, dpos = poisoned((B, T, C), F16), poisoned((2 * T - 1, C), F16)
    nbytes = int(L.dsp_relpos_attention_train_workspace_bytes(B, T, H))
    ws = poisoned((nbytes // 4,), torch.float32)

    def bwd(do=t["do"], dq_=dq, dp=dpos, ws_=ws, nb=nbytes, act=1, T_=T):
        return L.dsp_relpos_attention_train_bwd(lib.ptr(do), lib.ptr(t["q"]), lib.ptr(t["k"]), lib.ptr(t["v"]), C, lib.ptr(t["pos"]), lib.ptr(t["bias_u"]),
                                                lib.ptr(t["bias_v"]), None, lib.ptr(o), lib.ptr(lse), 1.0, 0, 1, 0, lib.ptr(dq_), None, None, lib.ptr(dp),
                                                None, None, lib.ptr(ws_), nb, act, 1, B, T_, H, st)
    assert bwd(do=None) == -1 and bwd(dq_=t["q"]) == -1 and bwd(dq_=t["do"]) == -1 and bwd(ws_=None) == -1 and bwd(nb=16) not in (0, -1)
    assert bwd(act=0) == -1 and bwd(T_=0) == -1 and bwd(dp=dq) == -1
    assert b"relpos_attention_train_bwd" in L.dsp_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(dq).all() and torch.isnan(dpos).all()
    assert bwd(dp=None, ws_=None, nb=0) == 0                                                    # no summed gradient asked for: no workspace needed
    assert bwd() == 0
    torch.cuda.synchronize()
    assert not torch.isnan(dq).any() and not torch.isnan(dpos).any()


def test_workspace_question():
    L = LIB().load()
    ws = L.dsp_relpos_attention_train_workspace_bytes
    assert ws(0, 9, 4) == 0 and ws(2, 0, 4) == 0 and ws(2, 9, 0) == 0
    prev = 0
    for B, T, H in [(1, 1, 1), (1, 2, 1), (1, 33, 1), (2, 33, 1), (2, 33, 4), (2, 200, 4), (32, 200, 4), (32, 1500, 4)]:
        n = ws(B, T, H)
        assert n % 16 == 0 and n >= prev and n >= B * (2 * T - 1) * H * 64 * 4
        prev = n


# ---------------------------------------------------------------- decode_ops.relpos_attention_autograd

def _gen():
    return torch.cuda.default_generators[torch.cuda.current_device()]


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_operator_is_the_two_entry_points(dtype):
    case = (65, 3, 4, dtype, "ragged", 0.1)
    T, B, H = case[:3]
    t = stored(case)
    torch.cuda.manual_seed(SEED)
    _gen().set_offset(OFFSET)
    leaves = {n: t[n].clone().requires_grad_() for n in ("q", "k", "v", "pos", "bias_u", "bias_v")}
    o, lse = D().relpos_attention_autograd(leaves["q"], leaves["k"], leaves["v"], leaves["pos"], leaves["bias_u"], leaves["bias_v"], t["pad"], H, p=0.1,
                                           return_lse=True)
    assert _gen().get_offset() == OFFSET + 4                                # a masked call takes four of the stream
    grads = torch.autograd.grad(o, list(leaves.values()), t["do"])
    direct = hip_direct(case, t)
    assert torch.equal(o, direct["o"]) and torch.equal(lse, direct["lse"])
    for name, g in zip(GRADS, grads):
        assert torch.equal(g, direct[name]), name
    # partial gradients: only what autograd asks for is computed, with the same bits
    q2 = t["q"].clone().requires_grad_()
    _gen().set_offset(OFFSET)
    o2 = D().relpos_attention_autograd(q2, t["k"], t["v"], t["pos"], t["bias_u"], t["bias_v"], t["pad"], H, p=0.1)
    (dq2,) = torch.autograd.grad(o2, [q2], t["do"])
    assert torch.equal(dq2, direct["dq"])


def test_generator_properties():
    case = (33, 3, 4, F16, "none", 0.5)
    T, B, H = case[:3]
    t = stored(case)
    call = lambda **kw: D().relpos_attention_autograd(t["q"], t["k"], t["v"], t["pos"], t["bias_u"], t["bias_v"], None, H, **kw)
    torch.cuda.manual_seed(5)
    off0 = _gen().get_offset()
    a0 = call(p=0.0)
    a1 = call(p=0.5, training=False)
    assert _gen().get_offset() == off0 and torch.equal(a0, a1)             # no dropout: the generator is left alone
    b0 = call(p=0.5)
    assert _gen().get_offset() == off0 + 4
    b1 = call(p=0.5)
    assert not torch.equal(b0, b1)                                          # successive calls: other masks
    torch.cuda.manual_seed(5)
    assert torch.equal(call(p=0.5), b0)                                     # the same seed: the same bits
    torch.cuda.manual_seed(6)
    assert not torch.equal(call(p=0.5), b0)                                 # another seed: another o
    kept = D().dropout_keep_mask(5, off0, 0.5, (B, H, T, A.padded(T)), "cuda")[..., :T]
    assert 0.45 < kept.float().mean().item() < 0.55


def test_unserved_inputs_are_refused_on_the_device_too():
    case = (9, 2, 2, F16, "none", 0.0)
    t = stored(case)
    args = lambda **r: [r.get(n, t[n]) for n in ("q", "k", "v", "pos", "bias_u", "bias_v")]
    served, op = D().relpos_attention_autograd_served, D().relpos_attention_autograd
    assert served(*args(), None, 2)
    for bad in (dict(q=t["q"].double()), dict(q=t["q"].float(), k=t["k"].float(), v=t["v"].float(), pos=t["pos"].float()), dict(pos=t["pos"][:-1]),
                dict(bias_u=t["bias_u"].to(BF16))):
        assert not served(*args(**bad), None, 2)
        with pytest.raises(RuntimeError):
            op(*args(**bad), None, 2)
    assert not served(*args(), None, 4)                                     # head width 32
    with pytest.raises(RuntimeError):
        op(*args(), None, 4)
    old = D().set_relpos_attention_hip(False)
    try:
        assert old is True and not served(*args(), None, 2)
    finally:
        assert D().set_relpos_attention_hip(old) is False
    with torch.autocast("cuda", dtype=torch.float16):
        assert not served(*args(), None, 2)


# ---------------------------------------------------------------- the layer

LB, LT, LDIM, LH = 2, 37, 256, 4


def _layer(p):
    from daspeech_amd.models.daspeech import RelPosSelfAttention
    torch.manual_seed(3)
    layer = RelPosSelfAttention(LDIM, LH, dropout=p).double().train()
    pad = torch.arange(LT).unsqueeze(0) >= torch.tensor([LT, LT - 5]).unsqueeze(1)
    pos = torch.randn(1, 2 * LT - 1, LDIM, dtype=torch.float64)
    return layer, pos, pad


def _run_layer(layer, x0, pos, pad, cot):
    x = x0.clone().requires_grad_()
    out = layer(x, pos, pad)
    named = sorted(layer.named_parameters())
    grads = torch.autograd.grad(out, [x] + [p for _, p in named], cot)
    res = dict(out=out.detach(), dx=grads[0])
    res.update({"d." + n: g for (n, _), g in zip(named, grads[1:])})
    return res


def _count_calls(monkeypatch):
    calls = []
    real = D().relpos_attention_checked                                     # the entry the layer calls after relpos_attention_autograd_served
    monkeypatch.setattr(D(), "relpos_attention_checked", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


def test_layer_training_with_the_operator_on_and_off(monkeypatch):
    dtype = F16
    master, pos, pad = _layer(0.0)
    with torch.no_grad():
        for p in master.parameters():                                       # parameters, inputs and cotangent as the dtype stores them
            p.copy_(p.to(dtype).double())
    x0 = torch.randn(LB, LT, LDIM, dtype=torch.float64).to(dtype)
    cot = torch.randn(LB, LT, LDIM, dtype=torch.float64).to(dtype)
    pos = pos.to(dtype)
    ref = {k: v.detach().numpy() for k, v in _run_layer(copy.deepcopy(master), x0.double(), pos.double(), pad, cot.double()).items()}
    calls = _count_calls(monkeypatch)
    res = {}
    for on in (True, False):
        old = D().set_relpos_attention_hip(on)
        try:
            layer = copy.deepcopy(master).to(dtype).cuda()
            res[on] = _run_layer(layer, x0.cuda(), pos.cuda(), pad.cuda(), cot.cuda())
        finally:
            D().set_relpos_attention_hip(old)
        assert len(calls) == 1, (on, calls)                                 # one call with the switch on, none with it off
    # the soft-max is invariant to a key bias: that gradient is zero in exact arithmetic, so max|ref| is no scale for it; its error is measured
    # against the scale of the key weight's gradient, which the same rounding residues feed (as tests/test_gpu_resnorm_autograd.py)
    name, kw = "d.linear_k.bias", "d.linear_k.weight"
    assert np.abs(ref[name]).max() < 1e-12 * np.abs(ref[kw]).max()
    check_4x("relpos-layer-float16", res[True], res[False], ref, scales={name: np.abs(ref[kw]).max()})


def test_layer_training_with_dropout_gives_the_same_bits_under_the_same_seed(monkeypatch):
    master, pos, pad = _layer(0.1)
    layer = master.half().cuda()
    x0 = torch.randn(LB, LT, LDIM).half().cuda()
    cot = torch.randn(LB, LT, LDIM).half().cuda()
    pos, pad = pos.half().cuda(), pad.cuda()
    calls = _count_calls(monkeypatch)
    runs = []
    # The operator's own bits are pinned by test_two_calls_give_equal_bits; here the torch GEMMs of the projections around it have to repeat
    # themselves too.  Run to run they do not unless asked to (tests/test_gpu_resnorm_autograd.py explains), so they run on their
    # deterministic algorithms, and the first run — where the libraries settle on their kernels for a new shape — is not compared.
    old = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled(),
           torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark)
    torch.use_deterministic_algorithms(True, warn_only=True)
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        for seed in (20, 21, 21, 22):
            torch.cuda.manual_seed(seed)
            runs.append(_run_layer(layer, x0, pos, pad, cot))
    finally:
        torch.use_deterministic_algorithms(old[0], warn_only=old[1])
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = old[2], old[3]
    assert len(calls) == 4
    del runs[0]
    for name, v in runs[0].items():
        assert torch.isfinite(v).all(), name
        assert torch.equal(v, runs[1][name]), name
    assert not torch.equal(runs[0]["out"], runs[2]["out"])                  # another seed: other masks
