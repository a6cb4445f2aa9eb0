"""The residual + dropout + LayerNorm operator under autograd (csrc/residual_norm_train.hip, decode_ops.residual_dropout_layer_norm_autograd, the
training branches of ConformerLayer / NATDecoderLayer / FFTLayer) against the float64 restatement of tests/util_resnorm_ref.py, evaluated on
the inputs as stored (after rounding to the dtype) with the mask that decode_ops.dropout_keep_mask returns.

Accuracy: per tensor the figure is max|got - ref| / max|ref|.  The yardstick is the same figure for torch's own ops in the same dtype on the
same device (add, multiply by the same mask, add, layer_norm, autograd backward): the HIP figure may be at most 4 x torch's — both are fp32
accumulations of the same terms in another order — and where torch's figure is below one rounding of the tensor's dtype (2^-24 / 2^-11 /
2^-8) the bound is 4 x that rounding.  Nothing is skipped or masked; every case prints both figures.
Written-ness: the C entry points run on NaN-filled outputs and a NaN-filled workspace; no NaN may survive.  Two calls give equal bits;
leaving one of dh / dresidual / dbias / dgamma / dbeta out leaves the bits of the others."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import util_resnorm_ref as R
from tests.util_4x_rule import ROUND, check_4x, f64, figure      # (names other test modules import from here)  # noqa: F401

pytestmark = pytest.mark.gpu
NAN = float("nan")
EPS = 1e-5
SEED, OFFSET = 0x9E3779B97F4A7C15, 0x1_0000_0008          # both with a high word: all six words of key and counter matter
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
CH = R.CHUNK_ROWS
# (leading dims, C): one row; idle lanes; a chunk less one, a chunk, a chunk and one (with a ragged number of 16-byte groups per lane);
# several chunks and not a multiple of one; the widest row; a 3-D input; and the layer tests' width, where a wave holds 8 (16-bit) or 4 rows
SHAPES = [((1,), 8), ((3,), 72), ((CH - 1,), 256), ((CH,), 512), ((CH + 1,), 520), ((6 * CH + 53,), 512), ((5,), 2048), ((2, 7), 256),
          ((2 * CH + 5,), 64)]
# every option at every shape and dtype: p, alpha, bias, h, which of (y, s) feed the backward
CONFIGS = [dict(name="pre-norm", p=0.1, alpha=0.5, bias=True, h=True, use_s=True, use_y=True),
           dict(name="post-norm", p=0.0, alpha=1.0, bias=False, h=True, use_s=False, use_y=True),
           dict(name="drop-nobias", p=0.1, alpha=1.0, bias=False, h=True, use_s=True, use_y=True),
           dict(name="plain-ln", p=0.0, alpha=1.0, bias=False, h=False, use_s=False, use_y=True),
           # y not used downstream: the backward gets ds alone, and neither s, stats nor gamma (passed as NULL through the C entry point)
           dict(name="sum-only", p=0.1, alpha=0.5, bias=True, h=True, use_s=True, use_y=False)]


def D():
    from daspeech_amd import decode_ops
    return decode_ops


def LIB():
    from daspeech_amd import _lib
    return _lib


def test_constants_match_the_library():
    assert (R.CHUNK_ROWS, R.MAX_C) == (D().RESNORM_CHUNK_ROWS, D().RESNORM_MAX_C)


def served_shape(shape, dtype):
    return shape[1] % (16 // torch.empty((), dtype=dtype).element_size()) == 0


CASES = [(s, d) for s in SHAPES for d in DTYPES if served_shape(s, d)]
CASE_IDS = ["R%s-C%d-%s" % ("x".join(map(str, s[0])), s[1], str(d).split(".")[1]) for s, d in CASES]


def poisoned(shape, dtype):
    return torch.full(tuple(shape), NAN, dtype=dtype, device="cuda")


def rows_of(shape):
    return int(np.prod(shape[0]))


def stored(case, param_dtype=None, exact_params=False):
    """the inputs rounded to their dtypes, on the device, as [R,C] / [C]; exact_params: the parameters hold values of the data dtype"""
    (lead, C), dtype = case
    Rr = rows_of((lead, C))
    pd = dtype if param_dtype is None else param_dtype
    a = R.inputs(7 * Rr + C, Rr, C)
    out = {}
    for k, v in a.items():
        is_param = k in ("bias", "gamma", "beta")
        t = torch.from_numpy(v)
        if is_param and exact_params:
            t = t.to(dtype)
        out[k] = t.to(pd if is_param else dtype).cuda()
    return out


def mask_for(cfg, Rr, C):
    """the keep mask the kernels apply for (SEED, OFFSET, p), from the library's own mask function; None without dropout"""
    if cfg["p"] == 0 or not cfg["h"]:
        return None
    return D().dropout_keep_mask(SEED, OFFSET, cfg["p"], (Rr, C), "cuda")


def hip_direct(case, cfg, t, skip=(), seed=SEED, offset=OFFSET):
    """both C entry points on NaN-filled outputs and a NaN-filled workspace -> dict of outputs (the entries of `skip` left out: NULL)"""
    (lead, C), dtype = case
    Rr = rows_of((lead, C))
    lib, L = LIB(), LIB().load()
    pd = t["gamma"].dtype
    codes = (lib.DTYPE_CODES[str(dtype)], lib.DTYPE_CODES[str(pd)])
    p, alpha = cfg["p"], cfg["alpha"]
    thr = D().dropout_threshold(p) if cfg["h"] else 0
    scale = 1.0 / (1.0 - p) if thr else 1.0
    out = dict(y=poisoned((Rr, C), dtype), stats=poisoned((Rr, 2), torch.float32), dresidual=poisoned((Rr, C), dtype),
               dgamma=poisoned((C,), pd), dbeta=poisoned((C,), pd))
    if cfg["h"]:
        out.update(s=poisoned((Rr, C), dtype), dh=poisoned((Rr, C), dtype))
        if cfg["bias"]:
            out["dbias"] = poisoned((C,), pd)
    h = t["h"] if cfg["h"] else None
    bias = t["bias"] if cfg["bias"] else None
    st = lib.current_stream_handle()
    lib.check(L.dsp_resnorm_train_fwd(lib.ptr(h), lib.ptr(t["residual"]), lib.ptr(bias), lib.ptr(t["gamma"]), lib.ptr(t["beta"]), EPS, alpha, scale,
                                      thr, seed, offset, lib.ptr(out.get("s")), lib.ptr(out["y"]), lib.ptr(out["stats"]), codes[0], codes[1], Rr, C, st),
              "dsp_resnorm_train_fwd")
    nbytes = int(L.dsp_resnorm_train_workspace_bytes(Rr, C))
    assert nbytes > 0 and nbytes % 16 == 0
    ws = poisoned((nbytes // 4,), torch.float32)
    g = {k: (None if k in skip else out.get(k)) for k in ("dh", "dresidual", "dbias", "dgamma", "dbeta")}
    saved = out["s"] if cfg["h"] else t["residual"]
    dy = t["dy"] if cfg["use_y"] else None
    ds = t["ds"] if cfg["use_s"] else None
    saved, stats, gamma = (saved, out["stats"], t["gamma"]) if dy is not None else (None, None, None)
    lib.check(L.dsp_resnorm_train_bwd(lib.ptr(dy), lib.ptr(ds), lib.ptr(saved), lib.ptr(stats), lib.ptr(gamma), alpha, scale, thr, seed, offset,
                                      lib.ptr(g["dh"]), lib.ptr(g["dresidual"]), lib.ptr(g["dbias"]), lib.ptr(g["dgamma"]), lib.ptr(g["dbeta"]),
                                      lib.ptr(ws), nbytes, codes[0], codes[1], Rr, C, st), "dsp_resnorm_train_bwd")
    torch.cuda.synchronize()
    for k in skip:
        out.pop(k, None)
    out["mean"], out["rstd"] = (out["stats"][:, i].clone(memory_format=torch.contiguous_format) for i in (0, 1))
    del out["stats"]
    return out


def torch_lines(case, cfg, t, keep):
    """the torch lines the operator replaces on the same stored inputs, in the same dtype, on the device; the mask applied by a multiply"""
    (lead, C), dtype = case
    res = t["residual"].clone().requires_grad_()
    gamma, beta = t["gamma"].to(dtype).requires_grad_(), t["beta"].to(dtype).requires_grad_()
    wrt, names = [res, gamma, beta], ["dresidual", "dgamma", "dbeta"]
    if cfg["h"]:
        h = t["h"].clone().requires_grad_()
        wrt.append(h); names.append("dh")
        z = h
        if cfg["bias"]:
            bias = t["bias"].to(dtype).requires_grad_()
            wrt.append(bias); names.append("dbias")
            z = z + bias
        if keep is not None:
            z = z * keep.to(dtype) * (1.0 / (1.0 - cfg["p"]))
        s = res + (z if cfg["alpha"] == 1.0 else cfg["alpha"] * z)
    else:
        s = res
    y = F.layer_norm(s, (C,), gamma, beta, EPS)
    outs, cots = ([y], [t["dy"]]) if cfg["use_y"] else ([], [])
    if cfg["use_s"]:
        outs.append(s); cots.append(t["ds"])
    grads = torch.autograd.grad(outs, wrt, cots, allow_unused=True)
    grads = [torch.zeros_like(w) if g is None else g for g, w in zip(grads, wrt)]      # a parameter no used output depends on
    sd = s.detach().float()
    mean = sd.mean(1)
    rstd = 1.0 / torch.sqrt(((sd - mean[:, None]) ** 2).mean(1) + EPS)        # torch keeps its statistics to itself: recomputed in fp32
    out = dict(y=y.detach(), mean=mean, rstd=rstd, **{n: g for n, g in zip(names, grads)})
    if cfg["h"]:
        out["s"] = s.detach()
    torch.cuda.synchronize()
    return out


def reference(case, cfg, t, keep):
    (lead, C), dtype = case
    a = {k: f64(v) for k, v in t.items()}
    kp = None if keep is None else keep.cpu().numpy()
    rnd = lambda s: torch.from_numpy(s).to(dtype).to(torch.float64).numpy()
    f = R.forward(a["h"] if cfg["h"] else None, a["residual"], a["bias"] if cfg["bias"] else None, a["gamma"], a["beta"], EPS, cfg["alpha"], cfg["p"],
                  kp, round_s=rnd)
    g = R.backward(f["s"], a["gamma"], EPS, cfg["alpha"], cfg["p"], kp, a["dy"] if cfg["use_y"] else None, a["ds"] if cfg["use_s"] else None,
                   has_h=cfg["h"])
    out = dict(y=f["y"], mean=f["mean"], rstd=f["rstd"], **g)
    if cfg["h"]:
        out["s"] = f["s"]
        if not cfg["bias"]:
            del out["dbias"]
    return out


_cache = {}


def results(case, ci):
    """inputs, mask, float64 reference, torch yardstick and one HIP run of a case and configuration, computed once and left unchanged"""
    if (case, ci) not in _cache:
        cfg = CONFIGS[ci]
        t = stored(case)
        keep = mask_for(cfg, rows_of(case[0]), case[0][1])
        _cache[(case, ci)] = (t, keep, reference(case, cfg, t, keep), torch_lines(case, cfg, t, keep), hip_direct(case, cfg, t))
    return _cache[(case, ci)]


# ---------------------------------------------------------------- the mask

@pytest.mark.parametrize("n", [1, 3, 4, 5, 8 * 72 + 2, 4 * 1000 + 1])
def test_keep_mask_equals_the_numpy_restatement_bit_for_bit(n):
    for seed, off, p in ((0, 0, 0.5), (SEED, OFFSET, 0.1), (0xFFFFFFFFFFFFFFFF, 4, 0.5), (12345, 1 << 40, 0.9), (7, 12, 0.0), (7, 12, 1.0 - 2.0 ** -30)):
        got = D().dropout_keep_mask(seed, off, p, (n,), "cuda")
        assert got.dtype == torch.bool and got.shape == (n,)
        assert np.array_equal(got.cpu().numpy(), R.keep_mask(seed, off, p, n)), (seed, off, p)


def test_keep_mask_of_a_poisoned_buffer_and_its_kept_share():
    lib, L = LIB(), LIB().load()
    rows, C = 400, 256                                               # N = 102400 >= 1e5
    N = rows * C
    for p in (0.1, 0.5):
        out = torch.full((N + 3,), 77, dtype=torch.uint8, device="cuda")
        lib.check(L.dsp_dropout_keep_mask(SEED, OFFSET, D().dropout_threshold(p), lib.ptr(out), N, lib.current_stream_handle()), "dsp_dropout_keep_mask")
        torch.cuda.synchronize()
        assert int(out[:N].max()) <= 1 and bool((out[N:] == 77).all())       # every element written, nothing past the end
        share = float(out[:N].double().mean())
        print(f"resnorm keep share p {p}: {share:.5f}")
        assert abs(share - (1 - p)) <= 5 * np.sqrt(p * (1 - p) / N), (p, share)
        assert torch.equal(out[:N].bool().view(rows, C), D().dropout_keep_mask(SEED, OFFSET, p, (rows, C), "cuda"))


# ---------------------------------------------------------------- the two entry points

@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_every_element_written_and_within_4x_of_torch(case):
    for ci, cfg in enumerate(CONFIGS):
        t, keep, ref, tor, hip = results(case, ci)
        assert sorted(ref) == sorted(hip) == sorted(tor), cfg["name"]
        check_4x(CASE_IDS[CASES.index(case)] + "-" + cfg["name"], hip, tor, ref)
        if keep is not None:                                        # the mask is the one the kernel applied: dropped elements pass the residual on
            dropped = ~keep
            assert torch.equal(hip["s"][dropped], t["residual"][dropped]) and not bool(hip["dh"][dropped].any())


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_two_calls_give_equal_bits(case):
    for ci in (0, 1, 4):
        t, _, _, _, first = results(case, ci)
        again = hip_direct(case, CONFIGS[ci], t)
        for name, v in first.items():
            assert torch.equal(v.view(torch.uint8), again[name].view(torch.uint8)), (CONFIGS[ci]["name"], name)


NULLABLE = [c for c in CASES if c[0] in (((3,), 72), ((CH + 1,), 520), ((6 * CH + 53,), 512))]


@pytest.mark.parametrize("case", NULLABLE, ids=[CASE_IDS[CASES.index(c)] for c in NULLABLE])
def test_each_gradient_can_be_left_out_without_changing_the_others(case):
    t, _, _, _, full = results(case, 0)
    names = ("dh", "dresidual", "dbias", "dgamma", "dbeta")
    for skip in [(n,) for n in names] + [("dh", "dresidual"), ("dbias", "dgamma", "dbeta"), ("dh", "dbias"), ("dh", "dresidual", "dgamma", "dbeta")]:
        part = hip_direct(case, CONFIGS[0], t, skip=skip)
        for n in names:
            if n not in skip:
                assert torch.equal(part[n].view(torch.uint8), full[n].view(torch.uint8)), (skip, n)


def test_without_dropout_and_scale_dh_equals_dresidual():
    case = (((CH + 1,), 520), torch.float16)
    _, _, _, _, hip = results(case, 1)
    assert torch.equal(hip["dh"], hip["dresidual"])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_fp32_parameters_under_16_bit_data(dtype):
    case = (((CH + 3,), 264), dtype)
    cfg = CONFIGS[0]
    t = stored(case, param_dtype=torch.float32, exact_params=True)
    keep = mask_for(cfg, CH + 3, 264)
    hip = hip_direct(case, cfg, t)
    assert hip["dgamma"].dtype == torch.float32 and hip["dbias"].dtype == torch.float32 and hip["dh"].dtype == dtype
    check_4x("fp32-params-" + str(dtype).split(".")[1], hip, torch_lines(case, cfg, t, keep), reference(case, cfg, t, keep))


def test_bad_arguments_are_refused_before_any_launch():
    lib, L = LIB(), LIB().load()
    case = (((5,), 8), torch.float32)
    t = stored(case)
    Rr, C = 5, 8
    s, y, stats = poisoned((Rr, C), torch.float32), poisoned((Rr, C), torch.float32), poisoned((Rr, 2), torch.float32)

    def fwd(h=t["h"], res=t["residual"], ss=s, yy=y, act=0, par=0, R_=Rr, C_=C, thr=0, off=0):
        hp = None if h is None else lib.ptr(h).value + off
        return L.dsp_resnorm_train_fwd(hp, lib.ptr(res), None, lib.ptr(t["gamma"]), lib.ptr(t["beta"]), EPS, 1.0, 1.0, thr, 1, 0, lib.ptr(ss), lib.ptr(yy),
                                       lib.ptr(stats), act, par, R_, C_, lib.current_stream_handle())
    assert fwd(res=None) == -1 and fwd(yy=t["residual"]) == -1 and fwd(ss=None) == -1 and fwd(ss=y) == -1 and fwd(off=4) == -1
    assert fwd(C_=6) == -1 and fwd(C_=2052) == -1 and fwd(act=3) == -1 and fwd(act=0, par=1) == -1 and fwd(R_=(1 << 24) + 1) == -1 and fwd(R_=-1) == -1
    assert fwd(act=1, par=1, C_=12) == -1 and fwd(thr=(1 << 24) + 1) == -1
    assert b"resnorm_train_fwd" in L.dsp_last_error()
    assert fwd(R_=0) == 0
    torch.cuda.synchronize()
    assert torch.isnan(y).all() and torch.isnan(s).all() and torch.isnan(stats).all()          # nothing ran
    assert fwd() == 0 and fwd(h=None, ss=None) == 0
    torch.cuda.synchronize()
    assert not torch.isnan(y).any() and not torch.isnan(s).any() and not torch.isnan(stats).any()
    dres, dg = poisoned((Rr, C), torch.float32), poisoned((C,), torch.float32)
    nbytes = int(L.dsp_resnorm_train_workspace_bytes(Rr, C))
    ws = poisoned((nbytes // 4,), torch.float32)

    def bwd(dy=t["dy"], ss=s, dr=dres, dgm=dg, ws_=ws, nb=nbytes, C_=C):
        return L.dsp_resnorm_train_bwd(lib.ptr(dy), None, lib.ptr(ss), lib.ptr(stats), lib.ptr(t["gamma"]), 1.0, 1.0, 0, 1, 0, None, lib.ptr(dr), None,
                                       lib.ptr(dgm), None, lib.ptr(ws_), nb, 0, 0, Rr, C_, lib.current_stream_handle())
    assert bwd(ss=None) == -1 and bwd(dr=t["dy"]) == -1 and bwd(ws_=None) == -1 and bwd(nb=16) not in (0, -1) and bwd(C_=6) == -1
    assert b"resnorm_train_bwd" in L.dsp_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(dres).all() and torch.isnan(dg).all()
    assert bwd(dgm=None, ws_=None, nb=0) == 0                                                   # no column sum asked for: no workspace needed
    assert bwd() == 0
    torch.cuda.synchronize()
    assert not torch.isnan(dres).any() and not torch.isnan(dg).any()


# ---------------------------------------------------------------- decode_ops.residual_dropout_layer_norm_autograd

def _ln(t, C, dtype):
    ln = nn.LayerNorm(C, eps=EPS).cuda().to(t["gamma"].dtype)
    with torch.no_grad():
        ln.weight.copy_(t["gamma"]); ln.bias.copy_(t["beta"])
    return ln


def _gen():
    return torch.cuda.default_generators[torch.cuda.current_device()]


@pytest.mark.parametrize("dtype", DTYPES)
def test_operator_is_the_two_entry_points(dtype):
    """a 3-D input through the operator gives the bits of the C entry points on its [R,C] view, for the generator's (seed, offset)"""
    lead, C = (2, 7), 256
    case = ((lead, C), dtype)
    t = stored(case)
    ln = _ln(t, C, dtype)
    v3 = lambda x: x.view(*lead, C)
    torch.cuda.manual_seed(1234)
    _gen().set_offset(40)
    direct = hip_direct(case, CONFIGS[0], t, seed=int(torch.cuda.initial_seed()), offset=40)
    h, res, bias = v3(t["h"]).clone().requires_grad_(), v3(t["residual"]).clone().requires_grad_(), t["bias"].clone().requires_grad_()
    assert D().residual_dropout_layer_norm_served(h, res, ln, bias=bias)
    s, y = D().residual_dropout_layer_norm_autograd(h, res, ln, bias=bias, alpha=0.5, p=0.1, training=True)
    assert _gen().get_offset() == 44
    grads = torch.autograd.grad([s, y], [h, res, bias, ln.weight, ln.bias], [v3(t["ds"]), v3(t["dy"])])
    for got, name in zip((s, y) + grads, ("s", "y", "dh", "dresidual", "dbias", "dgamma", "dbeta")):
        assert got.dtype == direct[name].dtype and torch.equal(got.reshape(direct[name].shape), direct[name]), name
    assert s.shape == (2, 7, C) and grads[0].shape == (2, 7, C)
    # training=False: no dropout, the generator untouched
    direct0 = hip_direct(case, dict(CONFIGS[0], p=0.0), t)
    s0, y0 = D().residual_dropout_layer_norm_autograd(h, res, ln, bias=bias, alpha=0.5, p=0.1, training=False)
    assert _gen().get_offset() == 44 and torch.equal(y0.reshape(-1, C), direct0["y"])


def test_operator_forms_and_partial_gradients():
    C = 72
    case = (((3,), C), torch.float32)
    t = stored(case)
    ln = _ln(t, C, torch.float32)
    op = D().residual_dropout_layer_norm_autograd
    # post-norm, no dropout, alpha 1: y alone; dh and dresidual are one tensor
    post = hip_direct(case, CONFIGS[1], t)
    h, res = t["h"].clone().requires_grad_(), t["residual"].clone().requires_grad_()
    y = op(h, res, ln, return_sum=False)
    assert isinstance(y, torch.Tensor) and torch.equal(y, post["y"])
    gh, gr, gw = torch.autograd.grad(y, [h, res, ln.weight], t["dy"])
    assert torch.equal(gh, post["dh"]) and torch.equal(gr, post["dresidual"]) and torch.equal(gw, post["dgamma"])
    assert gh.data_ptr() == gr.data_ptr()
    # h None: a plain LayerNorm under autograd, y alone whatever return_sum says
    plain = hip_direct(case, CONFIGS[3], t)
    x = t["residual"].clone().requires_grad_()
    y = op(None, x, ln, p=0.1, training=True, return_sum=True)
    assert isinstance(y, torch.Tensor) and torch.equal(y, plain["y"])
    gx, gb = torch.autograd.grad(y, [x, ln.bias], t["dy"])
    assert torch.equal(gx, plain["dresidual"]) and torch.equal(gb, plain["dbeta"])
    # pre-norm with only s used downstream: the LayerNorm parameters get zeros, h and the residual get ds
    h, res = t["h"].clone().requires_grad_(), t["residual"].clone().requires_grad_()
    s, y = op(h, res, ln, alpha=0.5)
    gh, gr, gw = torch.autograd.grad(s, [h, res, ln.weight], t["ds"], allow_unused=True)
    assert torch.equal(gr, t["ds"]) and torch.equal(gh, 0.5 * t["ds"]) and (gw is None or not bool(gw.any()))
    # a constant residual (no gradient asked for) and a parameter-free backward
    h = t["h"].clone().requires_grad_()
    y = op(h, t["residual"], ln, return_sum=False)
    (gh,) = torch.autograd.grad(y, [h], t["dy"])
    assert torch.equal(gh, post["dh"])


def test_generator_properties():
    C = 256
    case = (((CH + 1,), C), torch.float16)
    t = stored(case)
    ln = _ln(t, C, torch.float16)
    op = lambda: D().residual_dropout_layer_norm_autograd(t["h"], t["residual"], ln, bias=t["bias"], p=0.1, training=True)[0]
    torch.cuda.manual_seed(77)
    off0 = _gen().get_offset()
    a = op()
    assert _gen().get_offset() == off0 + 4                              # a masked call takes four of the stream
    b = op()
    assert not torch.equal(a, b)                                        # successive calls: different masks
    torch.cuda.manual_seed(77)
    assert torch.equal(op(), a) and torch.equal(op(), b)                # the same generator state: the same masks
    state = torch.cuda.get_rng_state()
    c = op()
    torch.cuda.set_rng_state(state)                                     # set_rng_state restores the stream
    assert torch.equal(op(), c)
    # the mask is dropout_keep_mask's for the reserved (seed, offset): dropped elements pass the residual on
    torch.cuda.manual_seed(5)
    _gen().set_offset(16)
    d = op()
    keep = D().dropout_keep_mask(torch.cuda.initial_seed(), 16, 0.1, (CH + 1, C), "cuda")
    res = t["residual"]
    assert torch.equal(d[~keep], res[~keep]) and float((d != res)[keep].float().mean()) > 0.98      # (a kept value may round away in fp16)
    other = D().dropout_keep_mask(torch.cuda.initial_seed(), 20, 0.1, (CH + 1, C), "cuda")
    assert not torch.equal(d[~other], res[~other])                      # and no other mask explains the result
    assert 0.85< float(keep.float().mean()) < 0.95
    # p = 0 and eval calls leave the generator alone
    state = torch.cuda.get_rng_state()
    D().residual_dropout_layer_norm_autograd(t["h"], t["residual"], ln, p=0.0, training=True)
    D().residual_dropout_layer_norm_autograd(t["h"], t["residual"], ln, p=0.1, training=False)
    D().residual_dropout_layer_norm_autograd(None, t["residual"], ln, p=0.1, training=True)
    assert torch.equal(torch.cuda.get_rng_state(), state)
    # both GLAT passes of the model run under _same_draws: identical masks inside, the surrounding stream untouched
    from daspeech_amd.models.daspeech import _same_draws
    dev = t["h"].device
    outer = torch.cuda.get_rng_state(dev)
    with _same_draws(99, dev, True):
        e1 = op()
    with _same_draws(99, dev, True):
        e2 = op()
    assert torch.equal(e1, e2) and torch.equal(torch.cuda.get_rng_state(dev), outer)


def test_float64_and_cpu_are_refused_on_the_device_too():
    x = torch.zeros(2, 8, device="cuda", dtype=torch.float64)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        D().residual_dropout_layer_norm_autograd(x, x, nn.LayerNorm(8).cuda().double())
    assert not D().residual_dropout_layer_norm_served(x, x, nn.LayerNorm(8).cuda().double())
    xf = torch.zeros(2, 8, device="cuda")
    assert not D().residual_dropout_layer_norm_served(xf.t(), xf.t(), nn.LayerNorm(2).cuda())          # not contiguous
    with torch.autocast("cuda", dtype=torch.float16):
        assert not D().residual_dropout_layer_norm_served(xf, xf, nn.LayerNorm(8).cuda())


# ---------------------------------------------------------------- the three layer classes in training mode, the operator on and off

B, T, DIM = 2, 9, 64


def _layer_and_call(kind, p):
    from daspeech_amd.models.daspeech import ConformerLayer, NATDecoderLayer
    from daspeech_amd.models.fastspeech2 import FFTLayer
    torch.manual_seed(3)
    pad = torch.arange(T).unsqueeze(0) >= torch.tensor([T, T - 3]).unsqueeze(1)
    if kind == "conformer":
        layer = ConformerLayer(DIM, 128, 4, 7, dropout=p)
        extra = [torch.randn(1, 2 * T - 1, DIM, dtype=torch.float64)]
        call = lambda m, x, e, pd: m(x, e[0], pd)
    elif kind == "nat":
        layer = NATDecoderLayer(DIM, 128, 4, 48, dropout=p, attention_dropout=0.0, activation_dropout=p)
        enc_pad = torch.arange(7).unsqueeze(0) >= torch.tensor([7, 5]).unsqueeze(1)
        extra = [torch.randn(B, 7, 48, dtype=torch.float64), enc_pad]
        call = lambda m, x, e, pd: m(x, pd, e[0], e[1])
    else:
        layer = FFTLayer(DIM, 4, 128, 3, dropout=p, attention_dropout=0.0)
        extra = []
        call = lambda m, x, e, pd: m(x, pd)
    return layer.double().train(), extra, pad, call


def _run_layer(layer, call, x0, extra, pad, cot):
    x = x0.clone().requires_grad_()
    out = call(layer, x, extra, pad)
    named = sorted(layer.named_parameters())
    grads = torch.autograd.grad(out, [x] + [p for _, p in named], cot)
    res = dict(out=out.detach(), dx=grads[0])
    res.update({"d." + n: g for (n, _), g in zip(named, grads[1:])})
    return res


def _to(extra, dtype, device):
    return [e.to(device) if e.dtype == torch.bool else e.to(dtype).to(device) for e in extra]


def _count_calls(monkeypatch):
    calls = []
    real = D().residual_dropout_layer_norm_checked                     # the entry the layers call after residual_dropout_layer_norm_served
    monkeypatch.setattr(D(), "residual_dropout_layer_norm_checked", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("kind,sites", [("conformer", 4), ("nat", 3), ("fft", 2)])
def test_layer_training_with_the_operator_on_and_off(kind, sites, dtype, monkeypatch):
    master, extra, pad, call = _layer_and_call(kind, 0.0)
    with torch.no_grad():
        for p in master.parameters():                                  # parameters, inputs and cotangent as the dtype stores them
            p.copy_(p.to(dtype).double())
    x0 = torch.randn(B, T, DIM, dtype=torch.float64).to(dtype)
    cot = torch.randn(B, T, DIM, dtype=torch.float64).to(dtype)
    extra = [e if e.dtype == torch.bool else e.to(dtype) for e in extra]
    ref = {k: v.detach().numpy() for k, v in _run_layer(copy.deepcopy(master), call, x0.double(), _to(extra, torch.float64, "cpu"), pad, cot.double()).items()}
    calls = _count_calls(monkeypatch)
    res = {}
    for on in (True, False):
        old = D().set_residual_norm_hip(on)
        try:
            layer = copy.deepcopy(master).to(dtype).cuda()
            res[on] = _run_layer(layer, call, x0.cuda(), _to(extra, dtype, "cuda"), pad.cuda(), cot.cuda())
        finally:
            D().set_residual_norm_hip(old)
        assert len(calls) == sites, (on, calls)                        # every site went through the operator with the switch on, and only then
    # the soft-max is invariant to a key bias: that gradient is zero in exact arithmetic, so max|ref| is no scale for it; its error is measured
    # against the scale of the key weight's gradient, which the same rounding residues feed (as tests/test_gpu_convmod_autograd.py)
    scales = {}
    for name in ref:
        if name.endswith("k_proj.bias") or name.endswith("linear_k.bias"):
            kw = name[:-4] + "weight"
            assert np.abs(ref[name]).max() < 1e-12 * np.abs(ref[kw]).max()
            scales[name] = np.abs(ref[kw]).max()
    check_4x(f"layer-{kind}-" + str(dtype).split(".")[1], res[True], res[False], ref, scales=scales)


@pytest.mark.parametrize("kind,sites", [("conformer", 4), ("nat", 3), ("fft", 2)])
def test_layer_training_with_dropout_gives_the_same_bits_under_the_same_seed(kind, sites, monkeypatch):
    master, extra, pad, call = _layer_and_call(kind, 0.1)
    layer = master.half().cuda()
    x0 = torch.randn(B, T, DIM).half().cuda()
    cot = torch.randn(B, T, DIM).half().cuda()
    extra = _to(extra, torch.float16, "cuda")
    calls = _count_calls(monkeypatch)
    runs = []
    # The operator's own bits are pinned by test_two_calls_give_equal_bits; here the torch ops of the layer around it (MIOpen's convolutions of
    # the FFT block, the attention backward) have to repeat themselves too.  Run to run they do not unless asked to (seen on an MI355X: single
    # roundings of `out` between a first and a second run, of `dx` between later ones; tests/test_gpu_glance_ops.py met the same in the
    # criterions), so they run on their deterministic algorithms, and the first run — where the libraries settle on their kernels for a new
    # shape — is not compared.
    old = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled(),
           torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark)
    torch.use_deterministic_algorithms(True, warn_only=True)
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        for seed in (20, 21, 21, 22):
            torch.cuda.manual_seed(seed)
            runs.append(_run_layer(layer, call, x0, extra, pad.cuda(), cot))
    finally:
        torch.use_deterministic_algorithms(old[0], warn_only=old[1])
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = old[2], old[3]
    assert len(calls) == 4 * sites
    del runs[0]
    for name, v in runs[0].items():
        assert torch.isfinite(v).all(), name
        assert torch.equal(v, runs[1][name]), name
    assert not torch.equal(runs[0]["out"], runs[2]["out"])              # another seed: other masks
