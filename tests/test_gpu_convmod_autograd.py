"""The convolution-module operator under autograd (csrc/conformer_train.hip, decode_ops.dwconv_bn_silu_autograd, ConformerLayer's training
branch) against the float64 restatement of tests/util_convmod_ref.py, evaluated on the inputs as stored (after rounding to the dtype).

Accuracy: per tensor the figure is max|got - ref| / max|ref|.  The yardstick is the same figure for torch's own ops in the same dtype on
the same device (transpose -> conv1d(groups=C) -> batch_norm(training) -> silu -> transpose, autograd backward): the HIP figure may be at
most 4 x torch's — both are fp32 accumulations of the same terms in another order — and where torch's figure is below one rounding of the
tensor's dtype (2^-24 / 2^-11 / 2^-8) the bound is 4 x that rounding.  Nothing is skipped or masked; every case prints both figures.
Written-ness: the C entry points run on NaN-filled outputs and a NaN-filled workspace; no NaN may survive.  Two calls give equal bits;
leaving one of dx / dw / dgamma / dbeta out leaves the bits of the others."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import util_convmod_ref as R

pytestmark = pytest.mark.gpu
NAN = float("nan")
EPS, MOM = 1e-5, 0.1
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
ROUND = {torch.float32: 2.0 ** -24, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}      # one rounding of the dtype
TILE_ROWS = R.TIME_TILE * R.CHUNK_TILES
# the edge shapes, and one whose B*T spans several reduction chunks without being a multiple of one (5 x 821 = 4105 rows, 33 chunks)
SHAPES = R.EDGE_SHAPES + [(5, 6 * TILE_ROWS + 53, 64, 31)]


def D():
    from daspeech_amd import decode_ops
    return decode_ops


def LIB():
    from daspeech_amd import _lib
    return _lib


def test_constants_match_the_library():
    assert (R.TIME_TILE, R.CHUNK_TILES) == (D().CONVMOD_TIME_TILE, D().CONVMOD_CHUNK_TILES)


def served_shape(shape, dtype):
    return shape[2] % (16 // torch.empty((), dtype=dtype).element_size()) == 0


CASES = [(s, d) for s in SHAPES for d in DTYPES if served_shape(s, d)]
CASE_IDS = ["B%d-T%d-C%d-K%d-%s" % (s + (str(d).split(".")[1],)) for s, d in CASES]


def f64(t):
    return t.detach().to(torch.float64).cpu().numpy()


def poisoned(shape, dtype):
    return torch.full(tuple(shape), NAN, dtype=dtype, device="cuda")


def stored(case, bn_dtype=None):
    """the inputs rounded to their dtypes, on the device"""
    (B, T, C, K), dtype = case
    bd = dtype if bn_dtype is None else bn_dtype
    x, w, gamma, beta, gy, rm, rv = R.inputs(7 * T + K + C, B, T, C, K)
    dev = lambda a, d: torch.from_numpy(a).to(d).cuda()
    return dict(x=dev(x, dtype), w=dev(w, dtype), gy=dev(gy, dtype), gamma=dev(gamma, bd), beta=dev(beta, bd), rm=dev(rm, bd), rv=dev(rv, bd))


def hip_direct(case, t, skip=()):
    """both C entry points on NaN-filled outputs and a NaN-filled workspace -> dict of outputs (the entries of `skip` left out: NULL)"""
    (B, T, C, K), dtype = case
    lib, L = LIB(), LIB().load()
    bd = t["gamma"].dtype
    codes = (lib.DTYPE_CODES[str(dtype)], lib.DTYPE_CODES[str(bd)])
    nbytes = int(L.dsp_dwconv_bn_silu_train_workspace_bytes(B, T, C, K))
    assert nbytes > 0 and nbytes % 16 == 0
    out = dict(y=poisoned((B, T, C), dtype), save_mean=poisoned((C,), torch.float32), save_invstd=poisoned((C,), torch.float32),
               running_mean=t["rm"].clone(), running_var=t["rv"].clone(), dx=poisoned((B, T, C), dtype), dw=poisoned((C, K), dtype),
               dgamma=poisoned((C,), bd), dbeta=poisoned((C,), bd))
    ws = poisoned((nbytes // 4,), torch.float32)
    st = lib.current_stream_handle()
    lib.check(L.dsp_dwconv_bn_silu_train_fwd(lib.ptr(t["x"]), lib.ptr(t["w"]), lib.ptr(t["gamma"]), lib.ptr(t["beta"]), lib.ptr(out["running_mean"]),
                                             lib.ptr(out["running_var"]), MOM, EPS, lib.ptr(out["y"]), lib.ptr(out["save_mean"]),
                                             lib.ptr(out["save_invstd"]), lib.ptr(ws), nbytes, codes[0], codes[1], B, T, C, K, st),
              "dsp_dwconv_bn_silu_train_fwd")
    ws.fill_(NAN)
    g = {k: (None if k in skip else out[k]) for k in ("dx", "dw", "dgamma", "dbeta")}
    lib.check(L.dsp_dwconv_bn_silu_train_bwd(lib.ptr(t["x"]), lib.ptr(t["w"]), lib.ptr(t["gamma"]), lib.ptr(t["beta"]), lib.ptr(out["save_mean"]),
                                             lib.ptr(out["save_invstd"]), lib.ptr(t["gy"]), lib.ptr(g["dx"]), lib.ptr(g["dw"]), lib.ptr(g["dgamma"]),
                                             lib.ptr(g["dbeta"]), lib.ptr(ws), nbytes, codes[0], codes[1], B, T, C, K, st),
              "dsp_dwconv_bn_silu_train_bwd")
    torch.cuda.synchronize()
    for k in skip:
        del out[k]
    return out


def torch_lines(case, t):
    """the present torch lines of ConformerLayer's training branch on the same stored inputs, in the same dtype, on the device"""
    (B, T, C, K), dtype = case
    x, w = t["x"].clone().requires_grad_(), t["w"].view(C, 1, K).clone().requires_grad_()
    g, b = t["gamma"].clone().requires_grad_(), t["beta"].clone().requires_grad_()
    rm, rv = t["rm"].clone(), t["rv"].clone()
    z = F.conv1d(x.transpose(1, 2), w, None, 1, (K - 1) // 2, 1, C)
    bnout, sm, si = torch.native_batch_norm(z, g, b, rm, rv, True, MOM, EPS)      # F.batch_norm(training=True), statistics kept
    y = F.silu(bnout).transpose(1, 2)
    dx, dw, dg, db = torch.autograd.grad(y, [x, w, g, b], t["gy"])
    torch.cuda.synchronize()
    return dict(y=y, save_mean=sm, save_invstd=si, running_mean=rm, running_var=rv, dx=dx, dw=dw.view(C, K), dgamma=dg, dbeta=db)


def reference(t):
    a = {k: f64(v) for k, v in t.items()}
    f = R.forward(a["x"], a["w"], a["gamma"], a["beta"], EPS, a["rm"], a["rv"], MOM)
    g = R.backward(a["x"], a["w"], a["gamma"], a["beta"], EPS, a["gy"])
    return dict(y=f["y"], save_mean=f["mean"], save_invstd=f["invstd"], running_mean=f["running_mean"], running_var=f["running_var"], **g)


def figure(got, ref, scale=None):
    return float(np.abs(f64(got) - ref).max() / (np.abs(ref).max() if scale is None else scale))


def check_4x(tag, hip, tor, ref, scales=None):
    """the 4 x rule on every tensor of `ref`; prints both figures.  scales: max|ref| replaced for the named tensors (see its one user)"""
    bad = []
    for name, r in ref.items():
        assert not np.isnan(f64(hip[name])).any(), f"{tag} {name}: NaN in the result (an element never written)"
        sc = (scales or {}).get(name)
        fh, ft = figure(hip[name], r, sc), figure(tor[name], r, sc)
        bound = 4.0 * max(ft, ROUND[hip[name].dtype])
        print(f"convmod {tag} {name}: hip {fh:.3e} torch {ft:.3e} bound {bound:.3e}")
        if not fh <= bound:
            bad.append((name, fh, ft, bound))
    assert not bad, f"{tag}: figure above 4 x torch's (name, hip, torch, bound): {bad}"


_cache = {}


def results(case):
    """inputs, float64 reference, torch yardstick and one HIP run of a case, computed once and left unchanged"""
    if case not in _cache:
        t = stored(case)
        _cache[case] = (t, reference(t), torch_lines(case, t), hip_direct(case, t))
    return _cache[case]


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_every_element_written_and_within_4x_of_torch(case):
    t, ref, tor, hip = results(case)
    check_4x(CASE_IDS[CASES.index(case)], hip, tor, ref)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_two_calls_give_equal_bits(case):
    t, _, _, first = results(case)
    again = hip_direct(case, t)
    for name, v in first.items():
        assert torch.equal(v.view(torch.uint8), again[name].view(torch.uint8)), name


NULLABLE = [c for c in CASES if c[0] in ((2, 17, 16, 31), (2, 2 * R.TIME_TILE + 1, 8, 7), (5, 6 * TILE_ROWS + 53, 64, 31))]


@pytest.mark.parametrize("case", NULLABLE, ids=[CASE_IDS[CASES.index(c)] for c in NULLABLE])
def test_each_gradient_can_be_left_out_without_changing_the_others(case):
    t, _, _, full = results(case)
    names = ("dx", "dw", "dgamma", "dbeta")
    for skip in [(n,) for n in names] + [("dx", "dw"), ("dx", "dgamma", "dbeta"), ("dw", "dgamma", "dbeta")]:
        part = hip_direct(case, t, skip=skip)
        for n in names:
            if n not in skip:
                assert torch.equal(part[n].view(torch.uint8), full[n].view(torch.uint8)), (skip, n)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_fp32_batchnorm_tensors_under_16_bit_activations(dtype):
    case = ((3, 19, 24, 15), dtype)
    t = stored(case, bn_dtype=torch.float32)
    hip = hip_direct(case, t)
    assert hip["dgamma"].dtype == torch.float32 and hip["running_var"].dtype == torch.float32
    check_4x("fp32-bn-" + str(dtype).split(".")[1], hip, torch_lines(case, t), reference(t))


def test_bad_arguments_are_refused_before_any_launch():
    lib, L = LIB(), LIB().load()
    case = ((2, 9, 8, 7), torch.float32)
    t = stored(case)
    B, T, C, K = case[0]
    y, sm, si = poisoned((B, T, C), torch.float32), poisoned((C,), torch.float32), poisoned((C,), torch.float32)
    nbytes = int(L.dsp_dwconv_bn_silu_train_workspace_bytes(B, T, C, K))
    ws = poisoned((nbytes // 4,), torch.float32)

    def fwd(x=t["x"], yy=y, ws_=ws, nb=nbytes, act=0, bn=0, B_=B, T_=T, C_=C, K_=K, off=0):
        xp = None if x is None else lib.ptr(x).value + off
        return L.dsp_dwconv_bn_silu_train_fwd(xp, lib.ptr(t["w"]), lib.ptr(t["gamma"]), lib.ptr(t["beta"]), None, None, MOM, EPS, lib.ptr(yy), lib.ptr(sm),
                                              lib.ptr(si), lib.ptr(ws_), nb, act, bn, B_, T_, C_, K_, lib.current_stream_handle())
    assert fwd(x=None) == -1 and fwd(yy=t["x"]) == -1 and fwd(off=4) == -1 and fwd(K_=5) == -1 and fwd(C_=6) == -1 and fwd(act=3) == -1
    assert fwd(act=0, bn=1) == -1 and fwd(B_=1, T_=1) == -1 and fwd(ws_=None) == -1 and fwd(nb=16) != 0
    assert b"dwconv_bn_silu_train_fwd" in L.dsp_last_error()
    assert fwd(B_=0) == 0
    torch.cuda.synchronize()
    assert torch.isnan(y).all() and torch.isnan(sm).all()                                    # nothing ran
    assert fwd() == 0
    torch.cuda.synchronize()
    assert not torch.isnan(y).any()


# ---------------------------------------------------------------- decode_ops.dwconv_bn_silu_autograd: gradients and buffers through the module API

def _modules(case, t, track=True):
    (B, T, C, K), dtype = case
    conv = nn.Conv1d(C, C, K, padding=(K - 1) // 2, groups=C, bias=False).cuda().to(dtype)
    bn = nn.BatchNorm1d(C, eps=EPS, momentum=MOM, track_running_stats=track).cuda().to(dtype).train()
    with torch.no_grad():
        conv.weight.copy_(t["w"].view(C, 1, K)); bn.weight.copy_(t["gamma"]); bn.bias.copy_(t["beta"])
        if track:
            bn.running_mean.copy_(t["rm"]); bn.running_var.copy_(t["rv"])
    return conv, bn


@pytest.mark.parametrize("dtype", DTYPES)
def test_operator_gradients_and_buffers_after_one_and_two_steps(dtype):
    case = ((3, 2 * R.TIME_TILE + 3, 16, 15), dtype)
    (B, T, C, K), _ = case
    t = stored(case)
    direct = hip_direct(case, t)
    conv, bn = _modules(case, t)
    ref_bn = copy.deepcopy(bn)                                     # torch's module in the same dtype: the yardstick of the buffers
    assert D().dwconv_bn_silu_autograd_served(t["x"], conv, bn)
    a = {k: f64(v) for k, v in t.items()}
    rm, rv = a["rm"], a["rv"]
    for step in (1, 2):
        x = t["x"].clone().requires_grad_()
        y = D().dwconv_bn_silu_autograd(x, conv.weight, bn)
        grads = torch.autograd.grad(y, [x, conv.weight, bn.weight, bn.bias], t["gy"])
        ref_bn(F.conv1d(t["x"].transpose(1, 2), conv.weight.detach(), None, 1, (K - 1) // 2, 1, C))
        f = R.forward(a["x"], a["w"], a["gamma"], a["beta"], EPS, rm, rv, MOM)
        rm, rv = f["running_mean"], f["running_var"]
        assert int(bn.num_batches_tracked) == step == int(ref_bn.num_batches_tracked)
        if step == 1:                                              # the operator is the two entry points: the same bits
            for got, name in zip((y,) + grads, ("y", "dx", "dw", "dgamma", "dbeta")):
                assert got.dtype == direct[name].dtype and torch.equal(got.reshape(direct[name].shape), direct[name]), name
            assert grads[1].shape == conv.weight.shape
        check_4x(f"buffers-step{step}-{str(dtype).split('.')[1]}", dict(running_mean=bn.running_mean, running_var=bn.running_var),
                 dict(running_mean=ref_bn.running_mean, running_var=ref_bn.running_var), dict(running_mean=rm, running_var=rv))
    # only some gradients asked for: the others are not computed, the bits stay
    x = t["x"].clone().requires_grad_()
    y = D().dwconv_bn_silu_autograd(x, conv.weight.detach(), bn)
    gx, gb = torch.autograd.grad(y, [x, bn.bias], t["gy"])
    assert torch.equal(gx, direct["dx"]) and torch.equal(gb, direct["dbeta"])


def test_without_tracked_statistics_no_buffer_is_touched():
    case = ((2, 19, 8, 7), torch.float32)
    t = stored(case)
    conv, bn = _modules(case, t, track=False)
    assert bn.running_mean is None and bn.num_batches_tracked is None
    assert D().dwconv_bn_silu_autograd_served(t["x"], conv, bn)
    y = D().dwconv_bn_silu_autograd(t["x"].clone().requires_grad_(), conv.weight, bn)
    assert bn.running_mean is None and bn.running_var is None and bn.num_batches_tracked is None
    ref = reference(t)
    assert figure(y, ref["y"]) <= 4 * max(figure(torch_lines(case, t)["y"], ref["y"]), ROUND[torch.float32])
    with pytest.raises(RuntimeError, match="GPU tensors"):         # float64 is refused, never narrowed
        D().dwconv_bn_silu_autograd(t["x"].double(), conv.double().weight, bn.double())


# ---------------------------------------------------------------- ConformerLayer in training mode, the operator on and off

def _run_layer(layer, x0, pos, pad, cot):
    x = x0.clone().requires_grad_()
    out = layer(x, pos, pad)
    names = [n for n, _ in sorted(layer.named_parameters())]
    grads = torch.autograd.grad(out, [x] + [p for _, p in sorted(layer.named_parameters())], cot)
    res = dict(out=out, dx=grads[0])
    res.update({"d." + n: g for n, g in zip(names, grads[1:])})
    bn = layer.conv_module["batch_norm"]
    res["running_mean"], res["running_var"] = bn.running_mean.clone(), bn.running_var.clone()
    return res


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_conformer_layer_training_with_the_operator_on_and_off(dtype, monkeypatch):
    from daspeech_amd.models.daspeech import ConformerLayer
    torch.manual_seed(3)
    B, T, C = 3, 37, 64
    master = ConformerLayer(C, 128, 4, 31, dropout=0.0).double().train()
    with torch.no_grad():
        for p in master.parameters():                              # parameters, inputs and cotangent as the dtype stores them
            p.copy_(p.to(dtype).double())
    x0 = torch.randn(B, T, C, dtype=torch.float64).to(dtype)
    pos = torch.randn(1, 2 * T - 1, C, dtype=torch.float64).to(dtype)
    pad = torch.arange(T).unsqueeze(0) >= torch.tensor([T, T - 5, T - 11]).unsqueeze(1)
    cot = torch.randn(B, T, C, dtype=torch.float64).to(dtype)
    ref = {k: v.detach().numpy() for k, v in _run_layer(copy.deepcopy(master), x0.double(), pos.double(), pad, cot.double()).items()}
    calls = []
    real = D().dwconv_bn_silu_autograd
    monkeypatch.setattr(D(), "dwconv_bn_silu_autograd", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    res = {}
    for on in (True, False):
        old = D().set_conv_module_hip(on)
        try:
            layer = copy.deepcopy(master).to(dtype).cuda()
            res[on] = _run_layer(layer, x0.cuda(), pos.cuda(), pad.cuda(), cot.cuda())
            assert int(layer.conv_module["batch_norm"].num_batches_tracked) == 1
        finally:
            D().set_conv_module_hip(old)
        assert len(calls) == 1, (on, calls)                        # the operator ran with the switch on, and only then
    # the soft-max is invariant to a key bias: that gradient is zero in exact arithmetic (1e-17 in float64), so max|ref| is no scale for it;
    # its error is measured against the scale of the key weight's gradient, which the same rounding residues feed
    kb, kw = "d.self_attn.linear_k.bias", "d.self_attn.linear_k.weight"
    assert np.abs(ref[kb]).max() < 1e-12 * np.abs(ref[kw]).max()
    check_4x("layer-" + str(dtype).split(".")[1], res[True], res[False], ref, scales={kb: np.abs(ref[kw]).max()})


def test_fp16_model_takes_a_training_step_through_the_operator(monkeypatch):
    from daspeech_amd.criterions import s2s_dag_fastspeech2_loss
    from daspeech_amd.fp16_trainer import half_sample
    from daspeech_amd.synthetic import make_s2st_batch
    from tests.test_gpu_model import small_model
    calls = []
    real = D().dwconv_bn_silu_autograd
    monkeypatch.setattr(D(), "dwconv_bn_silu_autograd", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    old = D().set_conv_module_hip(True)
    try:
        model = small_model().half().train()
        batch = half_sample(make_s2st_batch(3, "cuda", seed=2, min_frames=120, max_frames=160))
        torch.manual_seed(7)
        loss, _ = s2s_dag_fastspeech2_loss(model, batch, glat_p="0.5:0.1@200k", update_num=100000)
        assert torch.isfinite(loss)
        (loss * 128.0).backward()
    finally:
        D().set_conv_module_hip(old)
    assert len(calls) >= 2                                         # the encoder's Conformer layers went through it
    missing = [n for n, p in model.named_parameters() if p.grad is None]
    assert not missing, missing[:8]
    assert all(torch.isfinite(p.grad).all() for p in model.parameters())
