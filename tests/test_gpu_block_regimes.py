"""dsp_ffn_split, dsp_linear_ln_split, dsp_attention_split and dsp_relpos_attention against the float64 references of
tests/util_block_ref.py at the tile, group and mask edges the workload-shaped tests (tests/test_gpu_ffn_fused.py, tests/test_gpu_attention.py)
never execute: every (groups, chunks per group) of ff_groups(), T = 1 and T within one row of the 64-row tile, padded row strides, NULL
biases, both reduce kernels past one grid-stride trip, planted LayerNorm rows; key masks with wholly masked first tiles, holes and lone
keys, scores whose maximum rises on every key tile or never, |s| near 70, row strides that differ between q, k and v, query limits, the
relative-position variant around T = 32 / 128, both work-item orders.  tests/test_block_ref.py proves that the tables reach those regimes
and that the bound used here rejects the emulated defects on these very inputs.

Every launch goes through the C entry points on NaN-filled outputs (and a NaN-filled FFN workspace of exactly the bytes asked for), so
that stale memory of the caching allocator cannot stand in for something a kernel failed to write.  Float results must satisfy
`err <= min(8 err32 + 4 * 2^-23, cap)` (util_glue_ref.fp32_bound) on the whole tensor and on every sample (FFN) or (sample, head)
(attention), each against its own scale; err32 is the same reference evaluated in fp32 on the CPU; cap is 2e-6 for the FFN, 3e-6 for the
LayerNorm-staged linear and max(3e-6, 8 S 2^-24) for attention with S the largest finite |scaled score|.  Every case prints its figures
(`pytest -s`; profiles/block_regimes.txt)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import util_block_ref as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
C = 256


def LIB():
    from daspeech_amd import _lib
    return _lib


def OPS():
    from daspeech_amd import decode_ops
    return decode_ops


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def nans(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=DEV)


def at(t, off_floats=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + 4 * off_floats)


def pack(w, step):
    """hi / lo fp16 fragments of a [Cout, Cin] weight exactly as decode_ops.SplitConv1d packs a one-tap layer: per `step`-channel slice"""
    _lib = LIB()
    lib = _lib.load()
    Cout, Cin = w.shape
    n = lib.dsp_conv1d_split_packed_elems(1, Cout, step)
    hi = torch.empty(Cin // step * n, dtype=torch.float16, device=DEV)
    lo = torch.empty_like(hi)
    for sl in range(Cin // step):
        wt = w[:, sl * step:(sl + 1) * step].unsqueeze(-1).permute(2, 0, 1).contiguous()
        _lib.check(lib.dsp_conv1d_split_pack(_lib.ptr(wt), ctypes.c_void_p(hi.data_ptr() + 2 * sl * n), ctypes.c_void_p(lo.data_ptr() + 2 * sl * n), 1, Cout,
                                             step, _lib.current_stream_handle()), "dsp_conv1d_split_pack")
    return hi, lo


def padded(a, ld, off=0):
    """a [B,T,c] inside a NaN-filled [B,T,ld] buffer at column `off` -> (buffer, view)"""
    B, T, c = a.shape
    buf = nans(B, T, ld)
    buf[..., off:off + c] = cu(a)
    return buf, buf[..., off:off + c]


# ---------------------------------------------------------------- dsp_ffn_split

_ffn_dev = {}
GUARD = 64                   # NaN floats behind the workspace that must stay NaN


def ffn_device(tag):
    if tag not in _ffn_dev:
        d = U.ffn_inputs(tag)
        ld, off = {"c": (C, 0), "ld260": (260, 0), "slice768": (768, 256)}[d["xlay"]]
        dev = dict(x=padded(d["x"], ld, off), ldx=ld, res=padded(d["res"], d["ldr"]), w1=pack(cu(d["w1"]), 256), w2=pack(cu(d["w2"]), 512))
        for k in ("ln_w", "ln_b", "b1", "b2", "post_w", "post_b"):
            dev[k] = None if d[k] is None else cu(d[k])
        _ffn_dev.clear()                                                 # one case's tensors at a time
        _ffn_dev[tag] = dev
    return _ffn_dev[tag]


def run_ffn(tag, with_res, post=None, ws_short=0, **over):
    """one dsp_ffn_split call -> (rc, out buffer [B,T,ldo] or None, out_ln [B,T,256] or None).  post: None = as the case says.
    over: arguments replaced for the refusal tests (H, C, ldx, b1, out_ln)."""
    _lib = LIB()
    lib = _lib.load()
    d, dev = U.ffn_inputs(tag), ffn_device(tag)
    B, T, H = d["B"], d["T"], d["H"]
    post = d["post"] if post is None else post
    nws = lib.dsp_ffn_split_workspace_bytes(B, T, C, H)
    assert nws == U.ff_workspace_bytes(B, T, H)
    ws = nans(nws // 4 + GUARD)
    out = None if post == "only" else nans(B, T, d["ldo"])
    out_ln = nans(B, T, C) if post else None
    a = dict(H=H, C=C, ldx=dev["ldx"], b1=at(dev["b1"]), out_ln=at(out_ln))
    a.update(over)
    rc = lib.dsp_ffn_split(at(dev["x"][1]), a["ldx"], at(dev["ln_w"]), at(dev["ln_b"]), U.LN_EPS, at(dev["w1"][0]), at(dev["w1"][1]), a["b1"],
                           at(dev["w2"][0]), at(dev["w2"][1]), at(dev["b2"]), at(dev["res"][0]) if with_res else None, d["ldr"], U.FFN_ALPHA, at(out),
                           d["ldo"], at(ws), nws - ws_short, B, T, a["C"], a["H"], d["act"], at(dev["post_w"]) if post else None,
                           at(dev["post_b"]) if post else None, U.LN_EPS, a["out_ln"], _lib.current_stream_handle())
    torch.cuda.synchronize()
    assert torch.isnan(ws[nws // 4:]).all(), (tag, "a write behind the workspace")
    if rc == 0:
        assert not torch.isnan(ws[:nws // 4]).any(), (tag, "a partial sum the kernel did not write")
    return rc, out, out_ln


def ffn_modules(d):
    ln = post = None
    with torch.no_grad():
        if d["ln"]:
            ln = torch.nn.LayerNorm(C, eps=U.LN_EPS).to(DEV).eval()
            ln.weight.copy_(cu(d["ln_w"])); ln.bias.copy_(cu(d["ln_b"]))
        if d["post"]:
            post = torch.nn.LayerNorm(C, eps=U.LN_EPS).to(DEV).eval()
            post.weight.copy_(cu(d["post_w"])); post.bias.copy_(cu(d["post_b"]))
        l1 = torch.nn.Linear(C, d["H"], bias=d["b1"] is not None).to(DEV).eval()
        l2 = torch.nn.Linear(d["H"], C, bias=d["b2"] is not None).to(DEV).eval()
        l1.weight.copy_(cu(d["w1"])); l2.weight.copy_(cu(d["w2"]))
        if d["b1"] is not None:
            l1.bias.copy_(cu(d["b1"]))
        if d["b2"] is not None:
            l2.bias.copy_(cu(d["b2"]))
    return ln, l1, l2, post


@pytest.mark.parametrize("tag", list(U.FFN_CASES))
def test_ffn_split_regimes_match_fp64(tag):
    d = U.ffn_inputs(tag)
    for with_res in U.ffn_twins(tag):
        rc, out, out_ln = run_ffn(tag, with_res)
        assert rc == 0, LIB().load().dsp_last_error()
        o = None if out is None else out[..., :C].cpu().numpy()
        if out is not None:
            assert not np.isnan(o).any(), "every row < T is written"
            assert torch.isnan(out[..., C:]).all(), "the padding columns of out (ldo > C) stay untouched"
        if out_ln is not None:
            assert not torch.isnan(out_ln).any()
        assert U.ffn_verdict(tag, with_res, o, None if out_ln is None else out_ln.cpu().numpy())
        # the fixed-order reduction: the same bits again
        _, out2, ln2 = run_ffn(tag, with_res)
        assert (out is None or torch.equal(out[..., :C], out2[..., :C])) and (out_ln is None or torch.equal(out_ln, ln2))
        if d["post"]:
            # the other post-LayerNorm form and the plain reduction write the same bits
            _, out3, ln3 = run_ffn(tag, with_res, post="only" if d["post"] == "out" else "out")
            _, out4, _ = run_ffn(tag, with_res, post="")
            assert torch.equal(ln3, out_ln)
            for a in (out, out3):
                assert a is None or torch.equal(a[..., :C], out4[..., :C])
        if d["xlay"] == "c" and d["ldr"] == C and d["ldo"] == C and d["B"] * d["T"] >= 128:
            # decode_ops.ffn_fused serves this shape: the same bits through the wrapper
            ln, l1, l2, post = ffn_modules(d)
            dev = ffn_device(tag)
            with torch.no_grad():
                w = OPS().ffn_fused(dev["x"][0], ln, l1, l2, {0: None, 1: "relu", 2: "silu", 3: "gelu"}[d["act"]], residual=dev["res"][0] if with_res else None,
                                    alpha=U.FFN_ALPHA, post_ln=post)
            assert w is not None
            w_out, w_ln = w if post is not None else (w, None)
            assert torch.equal(w_out, out[..., :C]) and (w_ln is None or torch.equal(w_ln, out_ln))


def test_ffn_split_refuses_a_workspace_one_byte_short():
    lib = LIB().load()
    for tag in ("g2-n1-T65", "g8-n1-T1"):
        rc, out, out_ln = run_ffn(tag, False, ws_short=1)
        assert rc != 0 and b"workspace" in lib.dsp_last_error()
        assert (out is None or torch.isnan(out).all()) and (out_ln is None or torch.isnan(out_ln).all())


@pytest.mark.parametrize("what,over", [("H = 768", dict(H=768)), ("C = 128", dict(C=128)), ("ldx = 258", dict(ldx=258)), ("misaligned b1", "b1+4"),
                                       ("post-LayerNorm weight without out_ln", dict(out_ln=None))])
def test_ffn_split_refusals_leave_the_output_untouched(what, over):
    lib = LIB().load()
    tag = "g1-n2-trips-p" if "post" in what else "g1-n8-T2"              # a case with a post-LayerNorm / with a b1
    if over == "b1+4":
        over = dict(b1=at(ffn_device(tag)["b1"], 1))
    rc, out, out_ln = run_ffn(tag, True, **over)
    assert rc != 0 and len(lib.dsp_last_error()) > 0, what
    assert torch.isnan(out).all() and (out_ln is None or torch.isnan(out_ln).all()), what


# ---------------------------------------------------------------- dsp_linear_ln_split (instance <256,256,64,8,1>)

@pytest.mark.parametrize("i", range(len(U.LINEAR_LN_CASES)))
def test_linear_ln_split_planted_rows_match_fp64(i):
    _lib = LIB()
    lib = _lib.load()
    d = U.linear_ln_inputs(i)
    B, T, M = d["B"], d["T"], d["M"]
    x, ln_w, ln_b, bias = cu(d["x"]), cu(d["ln_w"]), cu(d["ln_b"]), cu(d["b"])
    hi, lo = pack(cu(d["w"]), 256)
    lens = None if d["lens"] is None else torch.tensor(d["lens"], dtype=torch.int32, device=DEV)

    def run():
        out = nans(B, T, M)
        _lib.check(lib.dsp_linear_ln_split(at(x), C, at(ln_w), at(ln_b), U.LN_EPS, at(hi), at(lo), at(bias), None, M, 1.0, at(out), M, B, T, M, d["act"],
                                           at(lens), d["slack"], _lib.current_stream_handle()), "dsp_linear_ln_split")
        torch.cuda.synchronize()
        return out
    out = run()
    assert not torch.isnan(out).any(), "every row < T is written (skipped tiles as zeros)"
    assert U.linear_ln_verdict(i, out.cpu().numpy())
    for b, n in enumerate(d["rows"]):
        assert (out[b, n:] == 0).all(), "skipped tiles are exactly zero"
    assert torch.equal(run(), out)


# ---------------------------------------------------------------- dsp_attention_split

def att_device(d):
    """q, k, v views in the case's layout (NaN in every column no operand owns) and the mask bytes"""
    Cq = d["H"] * d["dk"]
    lay = d["layout"]
    if lay == "c":
        q, k, v = cu(d["q"]), cu(d["k"]), cu(d["v"])
    elif lay == "kv2c":
        q = cu(d["q"])
        kv = torch.cat([cu(d["k"]), cu(d["v"])], -1)
        k, v = kv[..., :Cq], kv[..., Cq:]
    elif lay == "qkv3c":
        qkv = torch.cat([cu(d["q"]), cu(d["k"]), cu(d["v"])], -1)
        q, k, v = qkv[..., :Cq], qkv[..., Cq:2 * Cq], qkv[..., 2 * Cq:]
    else:                                                                # ldq = C + 8, ldk = 2 C, ldv = C + 4
        q, k, v = padded(d["q"], Cq + 8)[1], padded(d["k"], 2 * Cq)[1], padded(d["v"], Cq + 4)[1]
    mask = None if d["key_mask"] is None else cu(d["key_mask"].astype(np.uint8))
    return q, k, v, mask


def same(a, b):
    """equal bits, a NaN (the rows of a sample without a live key) equal to a NaN"""
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


def run_attention(d, q, k, v, mask, q_lens=None, q_slack=0):
    _lib = LIB()
    lib = _lib.load()
    out = nans(d["B"], d["N"], d["H"] * d["dk"])
    _lib.check(lib.dsp_attention_split(at(q), q.stride(1), at(k), k.stride(1), at(v), v.stride(1), at(mask), at(out), d["B"], d["N"], d["M"], d["H"], d["dk"],
                                       d["scale"], at(q_lens), q_slack, _lib.current_stream_handle()), "dsp_attention_split")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("tag", list(U.ATT_CASES))
def test_attention_split_regimes_match_fp64(tag):
    d = U.attention_inputs(tag)
    q, k, v, mask = att_device(d)
    Cq = d["H"] * d["dk"]
    assert (q.stride(1), k.stride(1), v.stride(1)) == {"c": (Cq, Cq, Cq), "kv2c": (Cq, 2 * Cq, 2 * Cq), "qkv3c": (3 * Cq,) * 3,
                                                       "odd": (Cq + 8, 2 * Cq, Cq + 4)}[d["layout"]]
    out = run_attention(d, q, k, v, mask)
    got = out.cpu().numpy()
    live = U.live_samples(d["key_mask"], d["B"])
    assert not np.isnan(got[live]).any(), "no NaN in a row < N of a sample with a live key"
    assert U.attention_verdict(tag, got)
    assert same(run_attention(d, q, k, v, mask), out), "the same bits again"
    if mask is not None:
        # padding rows cannot leak into a valid query: +-3e4 there and zeros there give the same bits
        z = att_device(U.attention_inputs(tag, "zero"))
        assert same(run_attention(d, *z), out)
    with torch.no_grad():
        w = OPS().attention(q, k, v, None if mask is None else mask.bool(), d["H"])
    assert w is not None and same(w, out), "decode_ops.attention: the same bits"


@pytest.mark.parametrize("slack", U.QSLACKS)
def test_attention_split_query_limits(slack):
    """q_lens in {0, 1, 31, 32, 33, N, N + 50}, one sample each: rows below the limit carry the dense call's bits, every 32-query group that
    starts at or after it is zeros, and nothing below N is left unwritten"""
    d = U.qlens_inputs()
    q, k, v, mask = cu(d["q"]), cu(d["k"]), cu(d["v"]), cu(d["key_mask"].astype(np.uint8))
    dense = run_attention(d, q, k, v, mask)
    assert not torch.isnan(dense).any()
    lens = torch.tensor(U.QLENS, dtype=torch.int32, device=DEV)
    out = run_attention(d, q, k, v, mask, lens, slack)
    assert not torch.isnan(out).any(), "no NaN survives in a row < N"
    for b, n in enumerate(U.QLENS):
        lim = min(d["N"], n + slack)
        assert torch.equal(out[b, :lim], dense[b, :lim]), (b, n)
        assert (out[b, U.q_rows_computed(n + slack, d["N"]):] == 0).all(), (b, n)
    assert (out[0, 32:] == 0).all() and bool((out[0] == 0).all()) == (slack == 0)
    with torch.no_grad():
        w = OPS().attention(q, k, v, mask.bool(), d["H"], q_lens=lens, q_slack=slack)
    assert torch.equal(w, out)


# ---------------------------------------------------------------- dsp_relpos_attention

@pytest.mark.parametrize("tag", list(U.REL_CASES))
def test_relpos_attention_regimes_match_fp64(tag):
    _lib = LIB()
    lib = _lib.load()
    d = U.relpos_inputs(tag)
    B, T, H = d["B"], d["T"], d["H"]
    Cq = H * 64
    if d["fused"]:
        qkv = torch.cat([cu(d["q"]), cu(d["k"]), cu(d["v"])], -1)
        q, k, v = qkv[..., :Cq], qkv[..., Cq:2 * Cq], qkv[..., 2 * Cq:]
    else:
        q, k, v = cu(d["q"]), cu(d["k"]), cu(d["v"])
    pos, bu, bv = cu(d["pos"]), cu(d["bias_u"]), cu(d["bias_v"])
    mask = None if d["pad_mask"] is None else cu(d["pad_mask"].astype(np.uint8))

    def run():
        out = nans(B, T, Cq)
        _lib.check(lib.dsp_relpos_attention(at(q), at(k), at(v), q.stride(1), at(pos), at(bu), at(bv), at(mask), at(out), B, T, H, 64,
                                            _lib.current_stream_handle()), "dsp_relpos_attention")
        torch.cuda.synchronize()
        return out
    out = run()
    assert not torch.isnan(out).any()
    assert U.relpos_verdict(tag, out.cpu().numpy())
    assert torch.equal(run(), out), "the same bits again"
    with torch.no_grad():
        w = OPS().relpos_attention(q, k, v, pos.unsqueeze(0), bu, bv, None if mask is None else mask.bool(), H)
    assert w is not None and torch.equal(w, out), "decode_ops.relpos_attention: the same bits"
