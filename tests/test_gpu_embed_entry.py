"""The embedding-entry operators under autograd (csrc/embed_entry_train.hip; decode_ops.embed_entry_autograd and
positional_add_dropout_autograd) against the float64 restatement of tests/util_embed_entry_ref.py, evaluated on the inputs as stored (after
rounding to the dtype) with the mask that decode_ops.dropout_keep_mask returns.

Accuracy: the 4 x rule of tests/util_4x_rule.py on y, dE, dP, dx and dalpha; the yardstick is the torch lines of the models in the same dtype
on the same device with the operator's own mask applied by a multiply (an fp32 table next to 16-bit data: torch's promoted result rounded to
the data dtype; an out-of-range token, on which torch raises: an appended zero row).  Every case prints both figures.
Written-ness: the C entry points run on NaN-filled outputs and a NaN-filled workspace; no NaN may survive; row `pad` and rows without a source
are exact zeros.  Two calls give equal bits; dE alone and dP alone (dx alone, dalpha alone) have the bits they have when both are asked for.
Views: a table that is a view into a flat parameter buffer at an odd offset is NOT served by embed_entry_served (the layer's torch lines run)
and is COPIED by the public function.

The two views tests register the operators' public names in the table of tests/test_gpu_views.py (imported as pytest itself imports it), where
test_every_public_operator_has_a_row looks for them.

Figures of the first run on an MI355X (highest hip / torch figure per dtype over the cases below) are in DESIGN.md §8."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import test_gpu_views as TV
from tests import util_embed_entry_ref as R
from tests.util_4x_rule import check_4x

pytestmark = pytest.mark.gpu
NAN = float("nan")
SEED, OFFSET = 0x9E3779B97F4A7C15, 0x1_0000_0008          # both with a high word: all six words of key and counter matter
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
PAD = R.PAD


def D():
    from daspeech_amd import decode_ops
    return decode_ops


def LIB():
    from daspeech_amd import _lib
    return _lib


def VE(dtype):
    return 4 if dtype == F32 else 8


def poisoned(shape, dtype):
    if dtype in (torch.int32, torch.uint8):
        return torch.full(tuple(shape), 0x7F if dtype == torch.uint8 else -0x55555556, dtype=dtype, device="cuda")
    return torch.full(tuple(shape), NAN, dtype=dtype, device="cuda")


def _name(dtype):
    return str(dtype).split(".")[1]


# ---------------------------------------------------------------- token entry
# (pattern or hot-key count, dtype, p, V, C or "min" for one 16-byte group, rows of P beyond L + pad + 1).  A covering set, not the product.
ENTRY_CASES = [
    ("train", F16, 0.1, 8192, 512, 0), ("left-pad", F32, 0.5, 7, "min", 5), ("interior", BF16, 0.0, 512, 24, 0),
    ("all-pad-row", F16, 0.0, 7, 264, 3), ("no-pad", F32, 0.1, 512, 24, 0), ("one", BF16, 0.5, 7, "min", 0),
    ("distinct", F16, 0.5, 8192, 24, 0), ("out-of-range", F32, 0.0, 512, 264, 2), ("out-of-range", F16, 0.1, 7, 24, 0),
    (R.SORT_MAX - 1, F16, 0.1, 512, 24, 0), (R.SORT_MAX, F32, 0.0, 7, "min", 1), (R.SORT_MAX + 1, BF16, 0.5, 8192, 24, 0),
    (2 * R.GRAD_CHUNK - 1, F32, 0.1, 512, 8, 0), (2 * R.GRAD_CHUNK, F16, 0.0, 8192, 264, 0), (2 * R.GRAD_CHUNK + 1, BF16, 0.1, 7, 24, 2),
    (2 * R.GRAD_CHUNK + 1, F32, 0.5, 512, 512, 0),
]


def _eid(c):
    return "%s-%s-p%s-V%d-C%s-NP+%d" % (c[0], _name(c[1]), c[2], c[3], c[4], c[5])


_ENTRY = {}


def entry(case):
    """the inputs of a case as stored, on the device (made once, never modified), the keep mask and the float64 reference"""
    if case in _ENTRY:
        return _ENTRY[case]
    pat, dtype, p, V, C, extra = case
    C = VE(dtype) if C == "min" else C
    tok = R.hot_key_case(pat, V) if isinstance(pat, int) else R.token_case(pat, V)
    B, L = tok.shape
    NP = L + PAD + 1 + extra
    g = torch.Generator().manual_seed(11 * L + C)
    E = (torch.randn(V, C, generator=g) * 0.5 + 0.25).to(dtype).cuda()
    P = (torch.randn(NP, C, generator=g) * 0.5 + 0.25).to(dtype).cuda()
    E[PAD] = 0; P[PAD] = 0                                                 # as nn.Embedding keeps them
    dy = torch.randn(B, L, C, generator=g).to(dtype).cuda()
    scale = float(np.sqrt(C))
    keep = D().dropout_keep_mask(SEED, OFFSET, p, (B * L, C), "cuda") if p > 0 else None
    kn = None if keep is None else keep.cpu().numpy()
    ks = 1.0 / (1.0 - p) if p > 0 else 1.0
    ref = R.embed_entry_ref(tok, R.f64(E), R.f64(P), PAD, scale, kn, ks, R.f64(dy))
    out = SimpleNamespace(tok=torch.tensor(tok).cuda(), tok_np=tok, dtype=dtype, p=p, B=B, L=L, V=V, NP=NP, C=C, E=E, P=P, dy=dy, scale=scale,
                          keep=keep, ks=ks, ref=ref)
    _ENTRY[case] = out
    return out


def hip_entry(t, skip=(), tokens=None, ld=None):
    """both C entry points on NaN-filled outputs and a NaN-filled workspace -> dict y, dE, dP, tok32, pos32 (the entries of `skip` NULL)"""
    lib, L = LIB(), LIB().load()
    code = lib.DTYPE_CODES[str(t.dtype)]
    thr = D().dropout_threshold(t.p)
    scale = t.ks if thr else NAN                                            # thr == 0: keep_scale is not read
    n = t.B * t.L
    tokens = t.tok if tokens is None else tokens
    out = dict(y=poisoned((t.B, t.L, t.C), t.dtype), dE=poisoned((t.V, t.C), t.dtype), dP=poisoned((t.NP, t.C), t.dtype),
               tok32=poisoned((n,), torch.int32), pos32=poisoned((n,), torch.int32))
    st = lib.current_stream_handle()
    lib.check(L.dsp_embed_entry_fwd(lib.ptr(tokens), t.L if ld is None else ld, lib.ptr(t.E), lib.ptr(t.P), PAD, t.scale, scale, thr, SEED, OFFSET,
                                    lib.ptr(out["y"]), lib.ptr(out["tok32"]), lib.ptr(out["pos32"]), code, t.B, t.L, t.V, t.NP, t.C, st),
              "dsp_embed_entry_fwd")
    nbytes = int(L.dsp_embed_entry_bwd_workspace_bytes(n, t.V, t.NP, t.C, thr))
    assert nbytes > 0 and nbytes % 16 == 0
    ws = poisoned((nbytes // 4,), F32)
    g = {k: (None if k in skip else out[k]) for k in ("dE", "dP")}
    lib.check(L.dsp_embed_entry_bwd(lib.ptr(t.dy), lib.ptr(out["tok32"]), lib.ptr(out["pos32"]), PAD, t.scale, scale, thr, SEED, OFFSET,
                                    lib.ptr(g["dE"]), lib.ptr(g["dP"]), lib.ptr(ws), nbytes, code, n, t.V, t.NP, t.C, st), "dsp_embed_entry_bwd")
    torch.cuda.synchronize()
    for k in skip:
        out.pop(k)
    return out


def torch_entry(t):
    """the lines of DAGDecoder.extract_features in the dtype of the tables; an out-of-range token reads an appended zero row"""
    E, P = t.E.clone().requires_grad_(), t.P.clone().requires_grad_()
    inside = (t.tok >= 0) & (t.tok < t.V)
    Ex = torch.cat([E, torch.zeros(1, t.C, dtype=t.dtype, device="cuda")])
    y = R.torch_embed_entry(torch.where(inside, t.tok, torch.full_like(t.tok, t.V)), Ex, P, PAD, t.scale, t.keep, t.ks)
    dE, dP = torch.autograd.grad(y, [E, P], t.dy)
    return dict(y=y.detach(), dE=dE, dP=dP)


@pytest.mark.parametrize("case", ENTRY_CASES, ids=_eid)
def test_token_entry_against_float64(case):
    t = entry(case)
    hip = hip_entry(t)
    # the integer outputs are exact
    inside = (t.tok_np >= 0) & (t.tok_np < t.V)
    assert np.array_equal(hip["tok32"].cpu().numpy(), np.where(inside, t.tok_np, -1).reshape(-1))
    assert np.array_equal(hip["pos32"].cpu().numpy(), R.positions(t.tok_np != PAD, PAD).reshape(-1))
    check_4x("embed_entry " + _eid(case), hip, torch_entry(t), t.ref)
    # padding_idx, rows without a source, and nothing but zeros from an out-of-range token
    dE, dP = hip["dE"].float().cpu().numpy(), hip["dP"].float().cpu().numpy()
    assert not dE[PAD].any() and not dP[PAD].any()
    used = np.zeros(t.V, bool); used[t.tok_np[inside]] = True
    assert not dE[~used].any()
    usedp = np.zeros(t.NP, bool); usedp[R.positions(t.tok_np != PAD, PAD).reshape(-1)] = True
    assert not dP[~usedp].any()


@pytest.mark.parametrize("case", [ENTRY_CASES[0], ENTRY_CASES[7], ENTRY_CASES[10], ENTRY_CASES[11], ENTRY_CASES[15]], ids=_eid)
def test_token_entry_bits_do_not_depend_on_the_call_or_on_what_is_asked_for(case):
    t = entry(case)
    a, b = hip_entry(t), hip_entry(t)
    for k in ("y", "dE", "dP"):
        assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), k
    only_e, only_p = hip_entry(t, skip=("dP",)), hip_entry(t, skip=("dE",))
    assert torch.equal(only_e["dE"].view(torch.uint8), a["dE"].view(torch.uint8))
    assert torch.equal(only_p["dP"].view(torch.uint8), a["dP"].view(torch.uint8))


def test_token_entry_through_autograd_matches_the_c_entries_and_the_random_stream():
    t = entry(ENTRY_CASES[0])
    gen = torch.cuda.default_generators[torch.cuda.current_device()]
    res = []
    for _ in range(2):
        torch.cuda.manual_seed(1234)
        seed, off = gen.initial_seed(), gen.get_offset()
        E, P = t.E.clone().requires_grad_(), t.P.clone().requires_grad_()
        y = D().embed_entry_autograd(t.tok, E, P, PAD, t.scale, p=t.p, training=True)
        assert gen.get_offset() == off + 4                                  # a masked call moves the generator by 4
        dE, dP = torch.autograd.grad(y, [E, P], t.dy)
        res.append((y.detach(), dE, dP))
    for u, v in zip(*res):                                                  # the same seed: the same bits
        assert torch.equal(u.view(torch.uint8), v.view(torch.uint8))
    # the mask applied is dropout_keep_mask's: the inputs have no zero where the token is not pad
    keep = D().dropout_keep_mask(seed, off, t.p, (t.B * t.L, t.C), "cuda").view(t.B, t.L, t.C)
    live = t.tok.ne(PAD).unsqueeze(-1).expand_as(keep)
    y0 = D().embed_entry_autograd(t.tok, t.E, t.P, PAD, t.scale)           # no mask
    assert (y0[live] != 0).all()
    assert torch.equal((res[0][0] != 0)[live], keep[live])
    off = gen.get_offset()
    D().embed_entry_autograd(t.tok, t.E, t.P, PAD, t.scale, p=0.0, training=True)
    D().embed_entry_autograd(t.tok, t.E, t.P, PAD, t.scale, p=0.3, training=False)
    assert gen.get_offset() == off                                          # unmasked calls leave the generator alone
    assert torch.equal(y0.view(torch.uint8), hip_entry(SimpleNamespace(**{**vars(t), "p": 0.0, "ks": 1.0}))["y"].view(torch.uint8))


@TV.covers("embed_entry_autograd", "embed_entry_served", "embed_entry_checked", "set_embed_entry_hip")
def test_token_entry_views():
    t = entry(ENTRY_CASES[2])                                               # bf16, p = 0: the bits of a dense call are the yardstick
    want = hip_entry(t)
    # tokens as a column slice of a wider tensor: read in place through the row stride
    wide = torch.full((t.B, t.L + 7), 5, dtype=torch.int64, device="cuda")
    wide[:, 3:3 + t.L] = t.tok
    view = wide[:, 3:3 + t.L]
    assert not view.is_contiguous()
    got = hip_entry(t, tokens=view, ld=t.L + 7)
    for k in ("y", "dE", "dP"):
        assert torch.equal(got[k].view(torch.uint8), want[k].view(torch.uint8)), k
    E, P = t.E.clone().requires_grad_(), t.P.clone().requires_grad_()
    y = D().embed_entry_autograd(view, E, P, PAD, t.scale)
    assert torch.equal(y.view(torch.uint8), want["y"].view(torch.uint8))
    # dy non-contiguous and at an odd storage offset
    buf = torch.zeros(t.B * t.L * t.C * 2 + 1, dtype=t.dtype, device="cuda")
    dyv = buf[1:].view(t.B, t.L, t.C, 2)[..., 0]
    dyv.copy_(t.dy)
    assert not dyv.is_contiguous() and dyv.data_ptr() % 16
    dE, dP = torch.autograd.grad(y, [E, P], dyv)
    assert torch.equal(dE.view(torch.uint8), want["dE"].view(torch.uint8)) and torch.equal(dP.view(torch.uint8), want["dP"].view(torch.uint8))
    # tables as views into a flat parameter buffer at an odd offset: not served where the torch lines can run, copied by the public function
    flat = torch.zeros(1 + t.V * t.C + t.NP * t.C, dtype=t.dtype, device="cuda")
    Ev, Pv = flat[1:1 + t.V * t.C].view(t.V, t.C), flat[1 + t.V * t.C:].view(t.NP, t.C)
    Ev.copy_(t.E); Pv.copy_(t.P)
    assert Ev.data_ptr() % 16
    mods = [torch.nn.Embedding(t.V, t.C, padding_idx=PAD), torch.nn.Embedding(t.NP, t.C, padding_idx=PAD)]
    mods[0].weight, mods[1].weight = torch.nn.Parameter(t.E.clone()), torch.nn.Parameter(t.P.clone())
    assert D().embed_entry_served(t.tok, *mods)
    mods[0].weight = torch.nn.Parameter(Ev)
    assert not D().embed_entry_served(t.tok, *mods)
    assert torch.equal(D().embed_entry_autograd(t.tok, Ev, Pv, PAD, t.scale).view(torch.uint8), want["y"].view(torch.uint8))


# ---------------------------------------------------------------- positional add
# (dtype, table "same" / "f32", alpha "same" / "f32", p, B, N, C or "min", NT); NT 40 and 30: below the longest row, the clamp acts
POS_CASES = [
    (F16, "same", "same", 0.1, 3, 65, 512, 200), (F32, "same", "same", 0.5, 1, 1, "min", 4), (BF16, "f32", "f32", 0.0, 3, 63, 24, 70),
    (F16, "f32", "same", 0.5, 3, 130, 264, 40), (F32, "same", "same", 0.0, 3, 64, 264, 30), (BF16, "same", "same", 0.1, 1, 130, 24, 140),
    (F16, "same", "f32", 0.0, 3, 64, "min", 100),
]


def _pid(c):
    return "%s-tab%s-alpha%s-p%s-B%d-N%d-C%s-NT%d" % (_name(c[0]), c[1], c[2], c[3], c[4], c[5], c[6], c[7])


_POS = {}


def posadd(case):
    if case in _POS:
        return _POS[case]
    dtype, tk, ak, p, B, N, C, NT = case
    C = VE(dtype) if C == "min" else C
    g = torch.Generator().manual_seed(13 * N + C)
    x = (torch.randn(B, N, C, generator=g) + 3.0).to(dtype).cuda()         # no zeros: x + alpha * tab stays away from 0
    tab = (torch.rand(NT, C, generator=g) * 0.5).to(dtype if tk == "same" else F32).cuda()
    tab[1] = 0
    alpha = torch.tensor([0.75]).to(dtype if ak == "same" else F32).cuda()
    dy = torch.randn(B, N, C, generator=g).to(dtype).cuda()
    mask = torch.zeros(B, N, dtype=torch.bool)
    if B > 1:
        mask[0, 3:5] = True; mask[1, N // 2:] = True; mask[2, :] = True     # interior pads, right padding, an all-pad row
    elif N > 1:
        mask[0, :N // 3] = True                                             # left padding
    mask = mask.cuda()
    keep = D().dropout_keep_mask(SEED, OFFSET, p, (B * N, C), "cuda") if p > 0 else None
    ks = 1.0 / (1.0 - p) if p > 0 else 1.0
    ref = R.pos_add_ref(R.f64(x), mask.cpu().numpy(), R.f64(tab), float(alpha.double().item()), None if keep is None else keep.cpu().numpy(),
                        ks, R.f64(dy))
    out = SimpleNamespace(dtype=dtype, p=p, B=B, N=N, C=C, NT=NT, x=x, tab=tab, alpha=alpha, dy=dy, mask=mask, keep=keep, ks=ks, ref=ref)
    _POS[case] = out
    return out


def hip_posadd(t, skip=(), x=None):
    lib, L = LIB(), LIB().load()
    codes = [lib.DTYPE_CODES[str(d)] for d in (t.dtype, t.tab.dtype, t.alpha.dtype)]
    thr = D().dropout_threshold(t.p)
    scale = t.ks if thr else NAN
    R_ = t.B * t.N
    x = t.x if x is None else x
    out = dict(y=poisoned((t.B, t.N, t.C), t.dtype), dx=poisoned((t.B, t.N, t.C), t.dtype), dalpha=poisoned((1,), t.alpha.dtype),
               pos32=poisoned((R_,), torch.int32))
    st = lib.current_stream_handle()
    lib.check(L.dsp_pos_add_fwd(lib.ptr(x), D()._row_pitch(x), lib.ptr(t.mask.view(torch.uint8)), lib.ptr(t.tab), lib.ptr(t.alpha), 1, scale, thr,
                                SEED, OFFSET, lib.ptr(out["y"]), lib.ptr(out["pos32"]), *codes, t.B, t.N, t.NT, t.C, st), "dsp_pos_add_fwd")
    g = {k: (None if k in skip else out[k]) for k in ("dx", "dalpha")}
    nbytes = int(L.dsp_pos_add_bwd_workspace_bytes(R_))
    ws = poisoned((nbytes // 4,), F32)
    lib.check(L.dsp_pos_add_bwd(lib.ptr(t.dy), lib.ptr(t.tab), lib.ptr(out["pos32"]), scale, thr, SEED, OFFSET, lib.ptr(g["dx"]),
                                lib.ptr(g["dalpha"]), lib.ptr(ws), nbytes, *codes, R_, t.NT, t.C, st), "dsp_pos_add_bwd")
    torch.cuda.synchronize()
    for k in skip:
        out.pop(k)
    return out


def torch_posadd(t):
    x, alpha = t.x.clone().requires_grad_(), t.alpha.clone().requires_grad_()
    y = R.torch_pos_add(x, t.mask, t.tab, alpha).to(t.dtype)                # an fp32 table or alpha: torch's promoted result, rounded
    if t.keep is not None:
        y = y * (t.keep.view_as(y).to(t.dtype) * t.ks)
    dx, da = torch.autograd.grad(y, [x, alpha], t.dy)
    return dict(y=y.detach(), dx=dx, dalpha=da)


@pytest.mark.parametrize("case", POS_CASES, ids=_pid)
def test_positional_add_against_float64(case):
    t = posadd(case)
    hip = hip_posadd(t)
    want_pos = np.minimum(R.positions(~t.mask.cpu().numpy(), 1), t.NT - 1).reshape(-1)
    assert np.array_equal(hip["pos32"].cpu().numpy(), want_pos)
    if t.N > t.NT:
        assert (want_pos == t.NT - 1).sum() > 1                             # the clamp acted
    check_4x("pos_add " + _pid(case), hip, torch_posadd(t), t.ref)
    a = hip_posadd(t)
    only_x, only_a = hip_posadd(t, skip=("dalpha",)), hip_posadd(t, skip=("dx",))
    for k in ("y", "dx", "dalpha"):
        assert torch.equal(a[k].view(torch.uint8), hip[k].view(torch.uint8)), k          # two calls: equal bits
    assert torch.equal(only_x["dx"].view(torch.uint8), hip["dx"].view(torch.uint8))
    assert torch.equal(only_a["dalpha"].view(torch.uint8), hip["dalpha"].view(torch.uint8))


@TV.covers("positional_add_dropout_autograd", "positional_add_dropout_served", "positional_add_dropout_checked")
def test_positional_add_through_autograd_random_stream_and_views():
    t = posadd(POS_CASES[0])
    gen = torch.cuda.default_generators[torch.cuda.current_device()]
    res = []
    for _ in range(2):
        torch.cuda.manual_seed(4321)
        seed, off = gen.initial_seed(), gen.get_offset()
        x, alpha = t.x.clone().requires_grad_(), t.alpha.clone().requires_grad_()
        y = D().positional_add_dropout_autograd(x, t.mask, t.tab, alpha, p=t.p, training=True)
        assert gen.get_offset() == off + 4
        dx, da = torch.autograd.grad(y, [x, alpha], t.dy)
        res.append((y.detach(), dx, da))
    for u, v in zip(*res):
        assert torch.equal(u.view(torch.uint8), v.view(torch.uint8))
    keep = D().dropout_keep_mask(seed, off, t.p, (t.B * t.N, t.C), "cuda").view(t.B, t.N, t.C)
    assert torch.equal(res[0][0] != 0, keep)                                # x + alpha * tab has no zero
    off = gen.get_offset()
    x = t.x.clone().requires_grad_()
    y0 = D().positional_add_dropout_autograd(x, t.mask, t.tab, t.alpha, p=0.0)
    D().positional_add_dropout_autograd(x, t.mask, t.tab, t.alpha, p=0.4, training=False)
    assert gen.get_offset() == off
    (dx0,) = torch.autograd.grad(y0, [x], t.dy)
    assert torch.equal(dx0, t.dy)                                           # without dropout: dx is dy
    want = hip_posadd(SimpleNamespace(**{**vars(t), "p": 0.0, "ks": 1.0}))
    assert torch.equal(y0.view(torch.uint8), want["y"].view(torch.uint8))
    # x as x[:, 1:] (two pitches: copied) and as a column slice of a wider tensor (one pitch: read in place)
    big = torch.randn(t.B, t.N + 1, t.C, device="cuda").to(t.dtype)
    big[:, 1:] = t.x
    assert D()._row_pitch(big[:, 1:]) is None and not D().positional_add_dropout_served(big[:, 1:], t.mask, t.tab, t.alpha)
    wide = torch.randn(t.B, t.N, t.C + 2 * VE(t.dtype), device="cuda").to(t.dtype)
    wide[:, :, VE(t.dtype):VE(t.dtype) + t.C] = t.x
    pitched = wide[:, :, VE(t.dtype):VE(t.dtype) + t.C]
    assert D()._row_pitch(pitched) == t.C + 2 * VE(t.dtype) and D().positional_add_dropout_served(pitched, t.mask, t.tab, t.alpha)
    assert torch.equal(hip_posadd(SimpleNamespace(**{**vars(t), "p": 0.0, "ks": 1.0}), x=pitched)["y"].view(torch.uint8), want["y"].view(torch.uint8))
    buf = torch.zeros(t.B * t.N * t.C * 2 + 1, dtype=t.dtype, device="cuda")
    dyv = buf[1:].view(t.B, t.N, t.C, 2)[..., 0]
    dyv.copy_(t.dy)
    for xv in (big[:, 1:], pitched):
        xv = xv.detach().requires_grad_()
        alpha = t.alpha.clone().requires_grad_()
        y = D().positional_add_dropout_autograd(xv, t.mask, t.tab, alpha)
        assert torch.equal(y.view(torch.uint8), want["y"].view(torch.uint8))
        dx, da = torch.autograd.grad(y, [xv, alpha], dyv)                   # dy non-contiguous and at an odd storage offset
        assert torch.equal(dx, t.dy) and torch.equal(da.view(torch.uint8), want["dalpha"].view(torch.uint8))
