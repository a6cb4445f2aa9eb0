"""GPU: the multi-head attention training operator (csrc/mha_train.hip; decode_ops.mha_attention_autograd) against the float64 restatement of
tests/util_mha_train_ref.py, by the project's 4 x rule (tests/util_4x_rule.py): for o, lse and each of the three gradients
max|got - ref64| / max|ref64|  <=  4 * max(the same figure for the yardstick, one rounding of the dtype),   the yardstick being the modules'
torch training lines on the GPU in the same dtype with the operator's own keep mask applied explicitly.  A wrong mask or a wrong tile is an
error of order 1.

Shapes: the smallest at which the tiling can go wrong.  The kernels' tile sizes (include/daspeech_decode.h):
  * a wave owns 32 rows — queries in the forward and the dq pass, keys in the dk / dv pass — so N and M at 31, 32, 33 (and 63, 65);
  * a workgroup owns DSP_MHA_TRAIN_OWN_ROWS = 128 of them (four waves, the last ones idle past the end), so N and M at 127, 128, 129;
  * the other side is streamed in tiles of DSP_MHA_TRAIN_TILE_ROWS = 32 rows — keys in the forward and the dq pass, queries in the dk / dv pass —
    with the next tile loaded ahead, so M and N at 31, 32, 33 again, and 1, 2 for a single partial tile;
  * N = 400 with M = 200 is past three whole workgroups of queries and one of keys."""
import copy

import numpy as np
import pytest
import torch

from tests import util_mha_train_ref as A
from tests.util_4x_rule import check_4x

pytestmark = pytest.mark.gpu
NAN = float("nan")
SEED, OFFSET = 1234567, 40
F16, BF16 = torch.float16, torch.bfloat16

# (N, M, B, H, dtype, mask, p): B in {1, 3}, H in {1, 4, 8}, both dtypes, the three masks and the three rates spread over the shapes.
# The mask with a sample of a single valid key comes with B = 3: with that sample ALONE (B = 1) P is 1 on one key, dS = P (dP - D) is zero in
# exact arithmetic, and so are dq and dk: max|ref64| is then float64 noise and no scale for a figure (tests/test_gpu_relpos_train.py).
CASES = [(1, 1, 1, 1, F16, "none", 0.0), (1, 1, 3, 4, BF16, "single", 0.5),
         (2, 5, 3, 1, F16, "ragged", 0.1), (2, 5, 1, 8, BF16, "none", 0.0),
         (31, 33, 3, 4, F16, "single", 0.5), (31, 33, 1, 1, BF16, "ragged", 0.0),
         (32, 32, 3, 8, F16, "none", 0.1), (32, 32, 1, 1, BF16, "ragged", 0.5),
         (33, 31, 1, 1, F16, "ragged", 0.0), (33, 31, 3, 4, BF16, "none", 0.1),
         (63, 65, 3, 1, F16, "single", 0.1), (63, 65, 1, 4, BF16, "ragged", 0.5),
         (65, 129, 1, 4, F16, "ragged", 0.5), (65, 129, 3, 1, BF16, "single", 0.0),
         (129, 64, 1, 8, F16, "none", 0.5), (129, 64, 3, 4, BF16, "single", 0.1),
         (127, 128, 3, 1, F16, "ragged", 0.1), (127, 128, 1, 4, BF16, "none", 0.5),
         (128, 127, 1, 4, F16, "none", 0.0), (128, 127, 3, 1, BF16, "ragged", 0.1),
         (200, 77, 3, 4, F16, "ragged", 0.1), (200, 77, 1, 1, BF16, "none", 0.0), (200, 77, 3, 8, BF16, "single", 0.5),
         (400, 200, 1, 4, F16, "ragged", 0.1), (400, 200, 1, 1, BF16, "none", 0.0)]
IDS = ["N%d-M%d-B%d-H%d-%s-%s-p%g" % (N, M, B, H, str(d).split(".")[1], m, p) for N, M, B, H, d, m, p in CASES]
GRADS = ("dq", "dk", "dv")


def D():
    from daspeech_amd import decode_ops
    return decode_ops


def LIB():
    from daspeech_amd import _lib
    return _lib


def poisoned(shape, dtype):
    return torch.full(tuple(shape), NAN, dtype=dtype, device="cuda")


def stored(case):
    """the inputs as the dtype stores them, on the GPU"""
    N, M, B, H, dtype, mask, p = case
    t = A.inputs(100 + N + 3 * M + 7 * B + H, B, N, M, H)
    out = {n: v.to(dtype).cuda() for n, v in t.items()}
    pm = A.pad_masks(mask, B, M)
    out["pad"] = None if pm is None else pm.cuda()
    return out


def mask_for(case, seed=SEED, offset=OFFSET):
    N, M, B, H, dtype, mask, p = case
    if p == 0.0:
        return None
    return D().dropout_keep_mask(seed, offset, p, (B, H, N, A.padded(M)), "cuda")[..., :M]


def hip_direct(case, t, skip=(), seed=SEED, offset=OFFSET):
    """the two C entry points on poisoned outputs; q, k, v are taken with the row strides they have"""
    N, M, B, H, dtype, mask, p = case
    lib, L = LIB(), LIB().load()
    C = H * 64
    code = lib.DTYPE_CODES[str(dtype)]
    thr = D().dropout_threshold(p) if p > 0 else 0
    scale = 1.0 / (1.0 - p) if thr else 1.0
    pm = None if t["pad"] is None else t["pad"].view(torch.uint8)
    o, lse = poisoned((B, N, C), dtype), poisoned((B, H, N), torch.float32)
    st = lib.current_stream_handle()
    ldq, ldkv = t["q"].stride(1), t["k"].stride(1)
    assert t["v"].stride(1) == ldkv
    lib.check(L.dsp_mha_train_fwd(lib.ptr(t["q"]), ldq, lib.ptr(t["k"]), lib.ptr(t["v"]), ldkv, lib.ptr(pm), scale, thr, seed, offset, lib.ptr(o),
                                  lib.ptr(lse), code, B, N, M, H, st), "fwd")
    shapes = dict(dq=(B, N, C), dk=(B, M, C), dv=(B, M, C))
    g = {n: (None if n in skip else poisoned(shapes[n], dtype)) for n in GRADS}
    nbytes = int(L.dsp_mha_train_workspace_bytes(B, N, M, H))
    ws = poisoned((nbytes // 4,), torch.float32)
    lib.check(L.dsp_mha_train_bwd(lib.ptr(t["do"]), lib.ptr(t["q"]), ldq, lib.ptr(t["k"]), lib.ptr(t["v"]), ldkv, lib.ptr(pm), lib.ptr(lse), scale, thr,
                                  seed, offset, *[lib.ptr(g[n]) for n in GRADS], lib.ptr(ws), nbytes, code, B, N, M, H, st), "bwd")
    torch.cuda.synchronize()
    out = dict(o=o, lse=lse)
    out.update({n: v for n, v in g.items() if v is not None})
    return out


def torch_lines(case, t, keep):
    """the yardstick: the modules' lines in the dtype, on the GPU, with the operator's mask"""
    N, M, B, H, dtype, mask, p = case
    leaves = [t[n].clone().requires_grad_() for n in ("q", "k", "v")]
    o, lse = A.module_lines(*leaves, t["pad"], H, keep, p)
    grads = torch.autograd.grad(o, leaves, t["do"])
    out = dict(o=o.detach(), lse=lse.detach())
    out.update(dict(zip(GRADS, grads)))
    return out


def reference(case, t, keep):
    N, M, B, H, dtype, mask, p = case
    c = {n: t[n].double().cpu() for n in ("q", "k", "v", "do")}
    pm = None if t["pad"] is None else t["pad"].cpu()
    kp = None if keep is None else keep.cpu()
    f = A.forward(c["q"], c["k"], c["v"], pm, H, kp, p)
    out = dict(o=f["o"].numpy(), lse=f["lse"].numpy())
    out.update({n: v.numpy() for n, v in A.backward(c["q"], c["k"], c["v"], pm, H, c["do"], kp, p).items()})
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
    assert D().MHA_TRAIN_MAX_LEN == A.MAX_LEN == 4096
    for n in ("dsp_mha_train_fwd", "dsp_mha_train_bwd", "dsp_mha_train_workspace_bytes"):
        assert hasattr(LIB().load(), n)


def test_workspace_question():
    ws = LIB().load().dsp_mha_train_workspace_bytes
    assert ws(0, 9, 5, 4) == 0 and ws(2, 0, 5, 4) == 0 and ws(2, 9, 0, 4) == 0 and ws(2, 9, 5, 0) == 0
    prev = 0
    for B, N, M, H in [(1, 1, 1, 1), (1, 2, 1, 1), (1, 33, 40, 1), (2, 33, 40, 1), (2, 33, 40, 4), (2, 200, 77, 4), (32, 400, 400, 8), (32, A.MAX_LEN, 9, 8)]:
        n = ws(B, N, M, H)
        assert n % 16 == 0 and n >= prev and n >= B * H * N * 4
        prev = n


@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_every_element_written_and_within_4x_of_torch(ci):
    t, keep, ref, tor, hip = results(ci)
    for name, v in hip.items():
        assert not torch.isnan(v).any(), f"{name}: NaN (an element never written)"
    check_4x("mha-" + IDS[ci], hip, tor, ref)


@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_two_calls_give_equal_bits(ci):
    t, keep, ref, tor, hip = results(ci)
    again = hip_direct(CASES[ci], t)
    for name, v in hip.items():
        assert torch.equal(v, again[name]), name


NULLABLE = [i for i, c in enumerate(CASES) if c[0] in (2, 33, 200) and c[4] == F16]


@pytest.mark.parametrize("ci", NULLABLE, ids=[IDS[i] for i in NULLABLE])
def test_each_gradient_can_be_left_out_without_changing_the_others(ci):
    t, keep, ref, tor, hip = results(ci)
    for left_out in GRADS:
        part = hip_direct(CASES[ci], t, skip=(left_out,))
        assert left_out not in part
        for name, v in part.items():
            assert torch.equal(v, hip[name]), (left_out, name)
    for only in GRADS:
        part = hip_direct(CASES[ci], t, skip=tuple(n for n in GRADS if n != only))
        assert torch.equal(part[only], hip[only]), only


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_views_of_stacked_projections_give_the_bits_of_dense_copies(dtype):
    """q as a view of a [B,N,3C] buffer, k and v as views of a [B,M,2C] buffer: row strides 3C and 2C"""
    case = (33, 70, 3, 4, dtype, "ragged", 0.1)
    N, M, B, H = case[:4]
    C = H * 64
    t = stored(case)
    dense = hip_direct(case, t)
    qkv = torch.cat([torch.full_like(t["q"], 7.0), t["q"], torch.full_like(t["q"], -7.0)], dim=-1)
    kv = torch.cat([t["k"], t["v"]], dim=-1)
    tv = dict(t, q=qkv[..., C:2 * C], k=kv[..., :C], v=kv[..., C:])
    assert tv["q"].stride(1) == 3 * C and tv["k"].stride(1) == 2 * C and tv["v"].stride(1) == 2 * C
    views = hip_direct(case, tv)
    for name, v in dense.items():
        assert torch.equal(v, views[name]), name
    # and through the operator, which takes the views as they are
    assert D().mha_attention_autograd_served(tv["q"], tv["k"], tv["v"], t["pad"], H)
    o0 = D().mha_attention_autograd(t["q"], t["k"], t["v"], t["pad"], H)
    o1 = D().mha_attention_autograd(tv["q"], tv["k"], tv["v"], t["pad"], H)
    assert torch.equal(o0, o1)


def test_a_sample_without_a_valid_key_gives_nan_in_its_own_rows_only():
    case = (33, 40, 3, 1, F16, "none", 0.0)
    N, M, B, H = case[:4]
    t = stored(case)
    t["pad"] = torch.zeros(B, M, dtype=torch.bool, device="cuda")
    t["pad"][1] = True
    hip = hip_direct(case, t)
    ref, _ = A.module_lines(t["q"], t["k"], t["v"], t["pad"], H)
    assert torch.isnan(ref[1]).all() and torch.isfinite(ref[0]).all()      # what torch's soft-max gives
    for name, v in hip.items():
        if name == "lse":
            assert (v[1] == float("-inf")).all()                            # log of an empty sum, as torch.logsumexp gives
        else:
            assert torch.isnan(v[1]).all(), name
        assert torch.isfinite(v[0]).all() and torch.isfinite(v[2]).all(), name


def test_bad_arguments_are_refused_before_any_launch():
    lib, L = LIB(), LIB().load()
    case = (9, 5, 2, 2, F16, "none", 0.0)
    N, M, B, H = case[:4]
    C = H * 64
    t = stored(case)
    o, lse = poisoned((B, N, C), F16), poisoned((B, H, N), torch.float32)
    st = lib.current_stream_handle()

    def fwd(q=t["q"], k=t["k"], oo=o, ll=lse, ldq=C, ldkv=C, act=1, B_=B, N_=N, M_=M, H_=H, thr=0, off=0):
        qp = None if q is None else lib.ptr(q).value + off
        return L.dsp_mha_train_fwd(qp, ldq, lib.ptr(k), lib.ptr(t["v"]), ldkv, None, 1.0, thr, 1, 0, lib.ptr(oo), lib.ptr(ll), act, B_, N_, M_, H_, st)
    assert fwd(q=None) == -1 and fwd(k=None) == -1 and fwd(oo=None) == -1 and fwd(ll=None) == -1
    assert fwd(oo=t["q"]) == -1 and fwd(oo=t["k"]) == -1                                        # an output that aliases an input
    assert fwd(off=2) == -1 and fwd(off=8) == -1                                                # misaligned
    assert fwd(ldq=C - 8) == -1 and fwd(ldq=C + 4) == -1 and fwd(ldq=C + 1) == -1 and fwd(ldkv=C - 8) == -1 and fwd(ldkv=C + 4) == -1
    assert fwd(act=0) == -1 and fwd(act=3) == -1
    assert fwd(N_=0) == -1 and fwd(M_=0) == -1 and fwd(N_=A.MAX_LEN + 1) == -1 and fwd(M_=A.MAX_LEN + 1) == -1 and fwd(H_=0) == -1 and fwd(B_=-1) == -1
    assert fwd(thr=(1 << 24) + 1) == -1
    assert b"mha_train_fwd" in L.dsp_last_error()
    assert fwd(B_=0) == 0
    torch.cuda.synchronize()
    assert torch.isnan(o).all() and torch.isnan(lse).all()                                      # nothing ran
    assert fwd() == 0
    torch.cuda.synchronize()
    assert not torch.isnan(o).any() and not torch.isnan(lse).any()
    dq, dk, dv = poisoned((B, N, C), F16), poisoned((B, M, C), F16), poisoned((B, M, C), F16)

    nbytes = int(L.dsp_mha_train_workspace_bytes(B, N, M, H))
    ws = poisoned((nbytes // 4,), torch.float32)

    def bwd(do=t["do"], dq_=dq, dk_=dk, dv_=dv, ldq=C, ldkv=C, act=1, N_=N, M_=M, off=0, ws_=ws, nb=nbytes):
        dop = None if do is None else lib.ptr(do).value + off
        return L.dsp_mha_train_bwd(dop, lib.ptr(t["q"]), ldq, lib.ptr(t["k"]), lib.ptr(t["v"]), ldkv, None, lib.ptr(lse), 1.0, 0, 1, 0,
                                   lib.ptr(dq_), lib.ptr(dk_), lib.ptr(dv_), lib.ptr(ws_), nb, act, B, N_, M_, H, st)
    assert bwd(do=None) == -1 and bwd(dq_=t["q"]) == -1 and bwd(dq_=t["do"]) == -1 and bwd(dk_=t["k"]) == -1 and bwd(dv_=lse) == -1 and bwd(dk_=dv) == -1
    assert bwd(ws_=None) == -1 and bwd(ws_=dq) == -1 and bwd(nb=nbytes - 16) not in (0, -1)        # no workspace, an aliased one, too small a one
    assert bwd(off=2) == -1 and bwd(ldq=C + 4) == -1 and bwd(ldkv=C + 12) == -1 and bwd(act=0) == -1
    assert bwd(N_=0) == -1 and bwd(M_=A.MAX_LEN + 1) == -1
    assert b"mha_train_bwd" in L.dsp_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(dq).all() and torch.isnan(dk).all() and torch.isnan(dv).all() and torch.isnan(ws).all()
    assert bwd(dq_=None, dk_=None, dv_=None) == 0                                               # nothing asked for
    assert bwd() == 0
    torch.cuda.synchronize()
    assert not torch.isnan(dq).any() and not torch.isnan(dk).any() and not torch.isnan(dv).any()


# ---------------------------------------------------------------- decode_ops.mha_attention_autograd

def _gen():
    return torch.cuda.default_generators[torch.cuda.current_device()]


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_operator_is_the_two_entry_points(dtype):
    case = (65, 129, 3, 4, dtype, "ragged", 0.1)
    N, M, B, H = case[:4]
    t = stored(case)
    torch.cuda.manual_seed(SEED)
    _gen().set_offset(OFFSET)
    leaves = [t[n].clone().requires_grad_() for n in ("q", "k", "v")]
    o, lse = D().mha_attention_autograd(*leaves, t["pad"], H, p=0.1, return_lse=True)
    assert _gen().get_offset() == OFFSET + 4                                # a masked call takes four of the stream
    assert not lse.requires_grad
    grads = torch.autograd.grad(o, leaves, t["do"])
    direct = hip_direct(case, t)
    assert torch.equal(o, direct["o"]) and torch.equal(lse, direct["lse"])
    for name, g in zip(GRADS, grads):
        assert torch.equal(g, direct[name]), name
    # partial gradients: only what autograd asks for is computed, with the same bits
    k2 = t["k"].clone().requires_grad_()
    _gen().set_offset(OFFSET)
    o2 = D().mha_attention_autograd(t["q"], k2, t["v"], t["pad"], H, p=0.1)
    (dk2,) = torch.autograd.grad(o2, [k2], t["do"])
    assert torch.equal(dk2, direct["dk"])


def test_generator_properties_and_the_mask_applied():
    case = (33, 31, 3, 4, F16, "none", 0.5)
    N, M, B, H = case[:4]
    t = stored(case)
    call = lambda **kw: D().mha_attention_autograd(t["q"], t["k"], t["v"], None, H, **kw)
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
    # the mask applied is dropout_keep_mask(...)[..., :M]: o against the reference with THAT mask (any other mask is an error of order 1)
    kept = D().dropout_keep_mask(5, off0, 0.5, (B, H, N, A.padded(M)), "cuda")[..., :M]
    assert 0.45 < kept.float().mean().item() < 0.55
    ref = A.forward(t["q"].double().cpu(), t["k"].double().cpu(), t["v"].double().cpu(), None, H, kept.cpu(), 0.5)["o"].numpy()
    tor, _ = A.module_lines(t["q"], t["k"], t["v"], None, H, kept, 0.5)
    check_4x("mha-mask-applied", dict(o=b0), dict(o=tor), dict(o=ref))


def test_unserved_inputs_are_refused_on_the_device_too():
    case = (9, 5, 2, 2, F16, "none", 0.0)
    N, M, B, H = case[:4]
    C = H * 64
    t = stored(case)
    args = lambda **r: [r.get(n, t[n]) for n in ("q", "k", "v")]
    served, op = D().mha_attention_autograd_served, D().mha_attention_autograd
    pad_m = torch.zeros(B, M, dtype=torch.bool, device="cuda")
    assert served(*args(), None, H) and served(*args(), pad_m, H)
    for bad in (dict(q=t["q"].double()), dict(q=t["q"].float(), k=t["k"].float(), v=t["v"].float()), dict(v=t["v"].to(BF16)), dict(v=t["v"][:, :-1])):
        assert not served(*args(**bad), None, H)
        with pytest.raises(RuntimeError):
            op(*args(**bad), None, H)
    assert not served(*args(), torch.zeros(B, N, dtype=torch.bool, device="cuda"), H)           # a [B,N] mask where N != M
    with pytest.raises(RuntimeError):
        op(*args(), torch.zeros(B, N, dtype=torch.bool, device="cuda"), H)
    assert not served(*args(), None, 4)                                     # head width 32
    with pytest.raises(RuntimeError):
        op(*args(), None, 4)
    # k and v with different row strides: not served as they are; the public function settles the layout with dense copies
    k3 = torch.cat([t["k"], t["k"], t["k"]], dim=-1)[..., :C]
    v2 = torch.cat([t["v"], t["v"]], dim=-1)[..., :C]
    assert not served(t["q"], k3, v2, None, H)
    assert torch.equal(op(t["q"], k3, v2, None, H), op(*args(), None, H))
    old = D().set_mha_attention_hip(False)
    try:
        assert old is True and not served(*args(), None, H)
    finally:
        assert D().set_mha_attention_hip(old) is False
    with torch.autocast("cuda", dtype=torch.float16):
        assert not served(*args(), None, H)


# ---------------------------------------------------------------- the modules

MB, MN, MM = 2, 40, 70          # cross-attention: 40 queries on a memory of 70
SN = 70                         # self-attention of the FFT layer


def _count_calls(monkeypatch):
    calls = []
    real = D().mha_attention_checked                                        # the entry the modules call after mha_attention_autograd_served
    monkeypatch.setattr(D(), "mha_attention_checked", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    import daspeech_amd.models.fastspeech2 as fs2
    assert not hasattr(fs2, "mha_attention_checked")                        # imported inside forward: the patched name is the one it finds
    return calls


def _sdpa_calls(monkeypatch):
    import torch.nn.functional as F
    calls = []
    real = F.scaled_dot_product_attention
    monkeypatch.setattr(F, "scaled_dot_product_attention", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


def _modules(p):
    """(name, float64 module, its inputs as (x, mem or None, pad)), weights, inputs and cotangent as fp16 stores them"""
    from daspeech_amd.models.daspeech import _MHA
    from daspeech_amd.models.fastspeech2 import _SelfAttention
    torch.manual_seed(3)
    mha = _MHA(512, 8, kdim=256, dropout=p).double().train()
    sa = _SelfAttention(256, 4, p).double().train()
    rn = lambda *s: torch.randn(*s, dtype=torch.float64).to(F16).double()
    with torch.no_grad():
        for mod in (mha, sa):
            for w in mod.parameters():
                w.copy_(w.to(F16).double())
    mem_pad = torch.arange(MM).unsqueeze(0) >= torch.tensor([MM, MM - 23]).unsqueeze(1)
    x_pad = torch.arange(SN).unsqueeze(0) >= torch.tensor([SN - 9, SN]).unsqueeze(1)
    return [("mha", mha, rn(MB, MN, 512), rn(MB, MM, 256), mem_pad, rn(MB, MN, 512)),
            ("self", sa, rn(MB, SN, 256), None, x_pad, rn(MB, SN, 256))]


def _heads(mod):
    return mod.h if hasattr(mod, "h") else mod.heads


def _run_module(mod, x, mem, pad, cot):
    out = mod(x, mem, pad) if mem is not None else mod(x, pad)
    named = sorted(mod.named_parameters())
    grads = torch.autograd.grad(out, [p for _, p in named], cot)
    res = dict(out=out.detach())
    res.update({"d." + n: g for (n, _), g in zip(named, grads)})
    return res


def _run_lines(mod, x, mem, pad, cot, keep, p):
    """the module by its explicit lines (A.module_lines), which take a given keep mask"""
    m = x if mem is None else mem
    q, k, v = mod.q_proj(x), mod.k_proj(m), mod.v_proj(m)
    o, _ = A.module_lines(q, k, v, pad, _heads(mod), keep, p)
    out = mod.out_proj(o)
    named = sorted(mod.named_parameters())
    grads = torch.autograd.grad(out, [w for _, w in named], cot)
    res = dict(out=out.detach())
    res.update({"d." + n: g for (n, _), g in zip(named, grads)})
    return res


def _to_gpu(mod, x, mem, pad, cot):
    return copy.deepcopy(mod).to(F16).cuda(), x.to(F16).cuda(), None if mem is None else mem.to(F16).cuda(), pad.cuda(), cot.to(F16).cuda()


def _np(res):
    return {k: v.detach().numpy() for k, v in res.items()}


def _key_bias_scale(ref):
    # the soft-max is invariant to a key bias: that gradient is zero in exact arithmetic, so max|ref| is no scale for it; its error is measured
    # against the scale of the key weight's gradient, which the same rounding residues feed (tests/test_gpu_relpos_train.py)
    name, kw = "d.k_proj.bias", "d.k_proj.weight"
    assert np.abs(ref[name]).max() < 1e-12 * np.abs(ref[kw]).max()
    return {name: np.abs(ref[kw]).max()}


@pytest.mark.parametrize("which", [0, 1], ids=["mha-cross", "self-attention"])
def test_module_training_with_the_operator_on_and_off(monkeypatch, which):
    name, mod, x, mem, pad, cot = _modules(0.0)[which]
    ref = _np(_run_module(copy.deepcopy(mod), x, mem, pad, cot))
    calls, sdpa = _count_calls(monkeypatch), _sdpa_calls(monkeypatch)
    res = {}
    for on in (True, False):
        old = D().set_mha_attention_hip(on)
        try:
            res[on] = _run_module(*_to_gpu(mod, x, mem, pad, cot))
        finally:
            D().set_mha_attention_hip(old)
        # one call of the operator and no scaled_dot_product_attention with the switch on; the reverse with it off
        assert (len(calls), len(sdpa)) == (1, 0 if on else 1), (on, calls, sdpa)
    check_4x(name + "-module-float16", res[True], res[False], ref, scales=_key_bias_scale(ref))


@pytest.mark.parametrize("which", [0, 1], ids=["mha-cross", "self-attention"])
def test_module_training_with_dropout(monkeypatch, which):
    p = 0.1
    name, mod, x, mem, pad, cot = _modules(p)[which]
    gmod, gx, gmem, gpad, gcot = _to_gpu(mod, x, mem, pad, cot)
    calls, sdpa = _count_calls(monkeypatch), _sdpa_calls(monkeypatch)
    runs, offs = [], []
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
            offs.append(_gen().get_offset())
            runs.append(_run_module(gmod, gx, gmem, gpad, gcot))
            assert _gen().get_offset() == offs[-1] + 4
    finally:
        torch.use_deterministic_algorithms(old[0], warn_only=old[1])
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = old[2], old[3]
    assert len(calls) == 4 and not sdpa
    for key, v in runs[1].items():
        assert torch.isfinite(v).all(), key
        assert torch.equal(v, runs[2][key]), key
    assert not torch.equal(runs[1]["out"], runs[3]["out"])                  # another seed: other masks
    # the rule against the float64 module with the operator's mask: the call reserved (seed 21, the offset before it)
    B, N = x.shape[:2]
    M = N if mem is None else mem.shape[1]
    H = _heads(mod)
    keep = D().dropout_keep_mask(21, offs[1], p, (B, H, N, A.padded(M)), "cuda")[..., :M]
    ref = _np(_run_lines(copy.deepcopy(mod), x, mem, pad, cot, keep.cpu(), p))
    tor = _run_lines(gmod, gx, gmem, gpad, gcot, keep, p)
    check_4x(name + "-module-dropout-float16", runs[1], tor, ref, scales=_key_bias_scale(ref))
