"""conv1d_split / ffn_split launch shapes that stage a row tile once and tile one-tap layers over the batch's rows: every output bit is
the one the launch shape before produced.  Everything goes through the C entry points.

Output-tile loop (csrc/conv1d_split.hip: a workgroup stages its rows once and runs a contiguous range of output tiles from them).
    The looped launch of a layer with M output channels == the concatenation of launches of ONE 256-channel block each (the block's
    weights packed on their own, bias / res / out pointers moved to the block's columns): bit for bit, plus the fp64 bound of this family
    in tests/test_gpu_split_addressing.py, 4e-6 of max |ref64|.  At B = 3 every launch is far below one workgroup per CU, where the plan
    gives each output tile its own workgroup; dsp_conv1d_split_plan_cus plans the looped launch as for a smaller device, so that the
    ranges are 1 (every tile in one workgroup) and 2 (a range boundary inside the row tile) — the single-block launches are planned for
    the real device.  T = 63, 65, 131: the smallest shapes with a partial row tile, a second tile of one or two rows and — ragged — a dead
    tile.  Three more cases reach the instances the workload loops in (16-wave 512-channel, 128-row 256-channel, 8-wave 512-channel
    K = 3), which cs_run picks only for wide layers.
Batch-row tiling (a dense one-tap, one-slice layer and the fused FFN tile B * T rows as one sequence).
    B = 3, T = 70 and B = 5, T = 13 put utterance boundaries inside tiles; the result == B calls with B = 1, bit for bit, and the 4 bytes
    after each output buffer stay untouched.
"""
import ctypes

import pytest
import torch

DEV = "cuda:0"
ACT = {None: 0, "relu": 1, "silu": 2, "gelu": 3}
ACT_FN = {None: lambda t: t, "relu": torch.relu, "silu": torch.nn.functional.silu, "gelu": torch.nn.functional.gelu}
CANARY = 777.0


def _lib_():
    from daspeech_amd import _lib
    lib = _lib.load()
    lib.dsp_conv1d_split_plan_cus.restype = ctypes.c_int
    lib.dsp_conv1d_split_plan_cus.argtypes = [ctypes.c_int]
    return _lib, lib


def at(t, off=0):
    """device pointer of tensor t, `off` floats in (None -> NULL)"""
    return None if t is None else ctypes.c_void_p(t.data_ptr() + 4 * off)


def pack(w, CI):
    """w [M, CI, K] fp32 -> (hi, lo) packed for one slice"""
    _lib, lib = _lib_()
    M, _, K = w.shape
    n = lib.dsp_conv1d_split_packed_elems(K, M, CI)
    hi = torch.empty(n, dtype=torch.float16, device=DEV); lo = torch.empty_like(hi)
    wt = w.permute(2, 0, 1).contiguous()
    _lib.check(lib.dsp_conv1d_split_pack(_lib.ptr(wt), _lib.ptr(hi), _lib.ptr(lo), K, M, CI, _lib.current_stream_handle()), "pack")
    return hi, lo


def out_buffer(*shape):
    """an output tensor filled with CANARY, with one more CANARY float right behind it"""
    n = 1
    for s in shape:
        n *= s
    flat = torch.full((n + 1,), CANARY, device=DEV)
    return flat, flat[:n].view(*shape)


def conv_call(x, w, bias, res, alpha, act, ln, lens, slack, out, col0, M_total):
    """One launch for the output columns col0 .. col0 + w.shape[0] of a layer M_total wide: out / res / bias moved to the columns."""
    _lib, lib = _lib_()
    B, T, CI = x.shape
    M, _, K = w.shape
    hi, lo = pack(w, CI)
    st = _lib.current_stream_handle()
    b_ = at(bias, col0); r_ = at(res, col0); o_ = at(out, col0)
    if ln is not None:
        _lib.check(lib.dsp_linear_ln_split(at(x), CI, at(ln[0]), at(ln[1]), 1e-5, at(hi), at(lo), b_, r_, M_total, alpha, o_, M_total, B, T, M, ACT[act],
                                           at(lens), slack, st), "linear_ln_split")
    elif lens is not None:
        _lib.check(lib.dsp_conv1d_split_ragged(at(x), CI, at(hi), at(lo), b_, r_, M_total, alpha, o_, M_total, B, T, CI, 1, M, K, ACT[act], at(lens), slack, st),
                   "ragged")
    elif res is not None or alpha != 1.0:
        _lib.check(lib.dsp_conv1d_split_residual(at(x), CI, at(hi), at(lo), b_, r_, M_total, alpha, o_, M_total, B, T, CI, 1, M, K, ACT[act], st), "residual")
    else:
        _lib.check(lib.dsp_conv1d_split(at(x), CI, at(hi), at(lo), b_, o_, M_total, B, T, CI, 1, M, K, ACT[act], 0, st), "conv1d_split")


def make_layer(seed, B, T, CI, M, K, with_bias, with_res, with_ln):
    torch.manual_seed(seed)
    x = torch.randn(B, T, CI, device=DEV) * 1.5 + 0.25
    w = torch.randn(M, CI, K, device=DEV) / (CI * K) ** 0.5
    bias = torch.randn(M, device=DEV) * 0.1 if with_bias else None
    res = torch.randn(B, T, M, device=DEV) if with_res else None
    ln = (torch.randn(CI, device=DEV) * 0.3 + 1.0, torch.randn(CI, device=DEV) * 0.3) if with_ln else None
    return x, w, bias, res, ln


def ref64(x, w, bias, res, alpha, act, ln):
    dt = torch.float64
    xx = x.to(dt)
    if ln is not None:
        xx = torch.nn.functional.layer_norm(xx, (x.shape[-1],), ln[0].to(dt), ln[1].to(dt), 1e-5)
    K = w.shape[-1]
    v = torch.nn.functional.conv1d(xx.transpose(1, 2), w.to(dt), None if bias is None else bias.to(dt), padding=(K - 1) // 2).transpose(1, 2)
    v = ACT_FN[act](v)
    return alpha * v if res is None else res.to(dt) + alpha * v


def check_loop_case(seed, B, T, CI, M, K, act, with_bias, with_res, alpha, with_ln, ragged, cus_list, block=256):
    _lib, lib = _lib_()
    x, w, bias, res, ln = make_layer(seed, B, T, CI, M, K, with_bias, with_res, with_ln)
    lens = slack = None
    if ragged:          # past one row tile (32 or 64 rows at these shapes) every sample has a partially valid tile and a dead one
        lens, slack = torch.tensor([T - 40, 9, T // 2 - 17][:B], device=DEV, dtype=torch.int32), 0
    # reference: one launch per 256-channel block, planned for the real device (one output tile per workgroup at these sizes)
    assert lib.dsp_conv1d_split_plan_cus(0) == 0
    flat_ref, want = out_buffer(B, T, M)
    for c0 in range(0, M, block):
        conv_call(x, w[c0:c0 + block].contiguous(), bias, res, alpha, act, ln, lens, slack or 0, want, c0, M)
    r64 = ref64(x, w, bias, res, alpha, act, ln)
    live = torch.ones(B, T, 1, device=DEV, dtype=torch.bool) if lens is None else (torch.arange(T, device=DEV)[None, :, None] < lens[:, None, None])
    scale = (r64.abs() * live).max().item()
    for cus in cus_list:
        flat, got = out_buffer(B, T, M)
        lib.dsp_conv1d_split_plan_cus(cus)
        try:
            conv_call(x, w, bias, res, alpha, act, ln, lens, slack or 0, got, 0, M)
        finally:
            lib.dsp_conv1d_split_plan_cus(0)
        case = f"B={B} T={T} CI={CI} M={M} K={K} act={act} bias={with_bias} res={with_res} alpha={alpha} ln={with_ln} ragged={ragged} cus={cus}"
        err = ((got.double() - r64).abs() * live).max().item() / scale
        print(f"\n[stage-once] {case}: err {err:.3e}")
        assert torch.isfinite(got).all(), case
        assert torch.equal(got, want), (case, "looped launch differs from the single-block launches in",
                                        int((got != want).sum().item()), "elements")
        assert err < 4e-6, (case, err)
        assert flat[-1].item() == CANARY and flat_ref[-1].item() == CANARY, (case, "the 4 bytes after the output were written")


def plan_ranges(B, T, kw, cus):
    """(ranges, output tiles) of the looped launch on a device of `cus` CUs"""
    _, lib = _lib_()
    fn = lib.dsp_conv1d_split_plan
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int] * 10 + [ctypes.POINTER(ctypes.c_int)]
    out = (ctypes.c_int * 6)()
    assert fn(B, T, kw["CI"], 1, kw["M"], kw["K"], int(kw["ragged"]), int(kw["with_ln"]), 0, cus, out) == 0
    return out[3], out[2]


# ranges: cus = 1 -> one workgroup runs every output tile of its row tile; a cus that needs two ranges puts a range boundary inside
TS = (63, 65, 131)
LOOP_CASES = []
for CI in (256, 512):
    for M in (512, 768, 1536, 2048):
        LOOP_CASES.append((f"ci{CI}-m{M}", dict(CI=CI, M=M, K=1, act="relu", with_bias=True, with_res=False, alpha=1.0, with_ln=False, ragged=False)))
LOOP_CASES += [
    ("ci256-m520-partial-tile", dict(CI=256, M=520, K=1, act="gelu", with_bias=True, with_res=True, alpha=0.5, with_ln=False, ragged=False)),
    ("ci512-m520-partial-tile", dict(CI=512, M=520, K=1, act=None, with_bias=False, with_res=False, alpha=1.0, with_ln=False, ragged=False)),
    ("ci256-m1024-k9", dict(CI=256, M=1024, K=9, act="relu", with_bias=True, with_res=False, alpha=1.0, with_ln=False, ragged=False)),
    ("ci256-m1024-k1", dict(CI=256, M=1024, K=1, act="relu", with_bias=True, with_res=False, alpha=1.0, with_ln=False, ragged=False)),
    ("ci256-m768-ln", dict(CI=256, M=768, K=1, act=None, with_bias=True, with_res=False, alpha=1.0, with_ln=True, ragged=False)),
    ("ci256-m768-ln-res-silu", dict(CI=256, M=768, K=1, act="silu", with_bias=True, with_res=True, alpha=0.5, with_ln=True, ragged=False)),
    ("ci512-m1536-nobias-alpha", dict(CI=512, M=1536, K=1, act=None, with_bias=False, with_res=False, alpha=0.5, with_ln=False, ragged=False)),
    ("ci512-m2048-res-silu", dict(CI=512, M=2048, K=1, act="silu", with_bias=True, with_res=True, alpha=0.5, with_ln=False, ragged=False)),
    ("ci256-m1024-k9-ragged", dict(CI=256, M=1024, K=9, act="relu", with_bias=True, with_res=True, alpha=1.0, with_ln=False, ragged=True)),
    ("ci512-m1536-ragged", dict(CI=512, M=1536, K=1, act="gelu", with_bias=True, with_res=False, alpha=1.0, with_ln=False, ragged=True)),
    ("ci256-m768-ln-ragged", dict(CI=256, M=768, K=1, act=None, with_bias=True, with_res=True, alpha=0.5, with_ln=True, ragged=True)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("name,kw", LOOP_CASES, ids=[c[0] for c in LOOP_CASES])
def test_output_tile_loop_bits(name, kw, T):
    B = 3
    seed = 9000 + 7 * [c[0] for c in LOOP_CASES].index(name) + T
    # the two smallest numbers of ranges the plan gives on devices of 1 .. 64 CUs: 1 (a workgroup runs every output tile of its row
    # tile) or 2, then a range boundary inside the row tile (a divisor of the tile count is needed: 3 tiles go from 1 range to 3)
    first = {}
    for cus in range(1, 65):
        r, m = plan_ranges(B, T, kw, cus)
        if r < m:
            first.setdefault(r, cus)
    assert first and min(first) <= 2, first
    check_loop_case(seed, B, T, cus_list=tuple(first[r] for r in sorted(first)[:2]), **kw)


# the instances the workload's looped launches run in; cs_run picks them from the workgroup count of a wide layer
WIDE_CASES = [
    ("cs512x16-m16384", dict(CI=512, M=16384, K=1, act="relu", with_bias=True, with_res=False, alpha=1.0, with_ln=False, ragged=False), 65, (1, 12)),
    ("cs256-128row-m11264", dict(CI=256, M=11264, K=1, act=None, with_bias=True, with_res=True, alpha=0.5, with_ln=False, ragged=False), 131, (1, 8)),
    ("cs512x8-k3-m11264", dict(CI=512, M=11264, K=3, act="silu", with_bias=True, with_res=False, alpha=1.0, with_ln=False, ragged=False), 65, (1, 24)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw,T,cus_list", WIDE_CASES, ids=[c[0] for c in WIDE_CASES])
def test_output_tile_loop_bits_in_the_wide_instances(name, kw, T, cus_list):
    from tests.test_gpu_split_addressing import cs_instance
    want = {"cs512x16-m16384": (512, 256, 64, 16), "cs256-128row-m11264": (256, 256, 128, 8), "cs512x8-k3-m11264": (512, 256, 64, 8)}[name]
    assert cs_instance(kw["CI"], 1, kw["M"], kw["K"], 3, T, "plain") == want
    for cus in cus_list:
        r, m = plan_ranges(3, T, kw, cus)
        assert m >= 44 and r == (1 if cus == 1 else r) and m // r >= 11, (cus, r, m)        # long ranges
    check_loop_case(9900 + T + kw["K"], 3, T, cus_list=cus_list, **kw)


# ------------------------------------------------------------------------------------------------------------------ batch rows
BT = [(3, 70), (5, 13)]


def check_rows_case(seed, B, T, CI, M, act, with_res, alpha, with_ln):
    x, w, bias, res, ln = make_layer(seed, B, T, CI, M, 1, True, with_res, with_ln)
    flat, got = out_buffer(B, T, M)
    conv_call(x, w, bias, res, alpha, act, ln, None, 0, got, 0, M)
    flat1, want = out_buffer(B, T, M)
    for b in range(B):
        conv_call(x[b:b + 1], w, bias, None if res is None else res[b:b + 1], alpha, act, ln, None, 0, want[b:b + 1], 0, M)
    case = f"B={B} T={T} CI={CI} M={M} act={act} res={with_res} ln={with_ln}"
    assert torch.isfinite(got).all() and not (got == CANARY).any(), case
    assert torch.equal(got, want), (case, "B * T rows as one sequence differ from B calls with B = 1 in", int((got != want).sum().item()), "elements")
    assert flat[-1].item() == CANARY and flat1[-1].item() == CANARY, (case, "the 4 bytes after the output were written")
    r64 = ref64(x, w, bias, res, alpha, act, ln)
    err = (got.double() - r64).abs().max().item() / r64.abs().max().item()
    print(f"\n[batch-rows] {case}: err {err:.3e}")
    assert err < 4e-6, (case, err)


@pytest.mark.gpu
@pytest.mark.parametrize("B,T", BT)
@pytest.mark.parametrize("CI,M", [(128, 272), (256, 256), (256, 768), (512, 512), (512, 1536)])
def test_batch_rows_conv1d_split(B, T, CI, M):
    check_rows_case(9100 + B + CI + M, B, T, CI, M, "relu", False, 1.0, False)


@pytest.mark.gpu
@pytest.mark.parametrize("B,T", BT)
@pytest.mark.parametrize("CI,M", [(128, 272), (256, 256), (512, 1536)])
def test_batch_rows_conv1d_split_residual(B, T, CI, M):
    check_rows_case(9200 + B + CI + M, B, T, CI, M, "gelu", True, 0.5, False)


@pytest.mark.gpu
@pytest.mark.parametrize("B,T", BT)
@pytest.mark.parametrize("M,with_res", [(768, False), (512, True)])
def test_batch_rows_linear_ln_split(B, T, M, with_res):
    check_rows_case(9300 + B + M, B, T, 256, M, "silu" if with_res else None, with_res, 0.5 if with_res else 1.0, True)


def ffn_call(x, ln, w1p, b1, w2p, b2, res, alpha, H, act, post, want_out):
    """dsp_ffn_split on x [B,T,256]; returns (flat out, out, flat out_ln, out_ln)"""
    _lib, lib = _lib_()
    B, T, C = x.shape
    nws = lib.dsp_ffn_split_workspace_bytes(B, T, C, H)
    assert nws > 0
    ws = torch.empty(nws // 4, device=DEV)
    flat, out = out_buffer(B, T, C) if want_out else (None, None)
    flat_ln, out_ln = out_buffer(B, T, C) if post is not None else (None, None)
    _lib.check(lib.dsp_ffn_split(at(x), C, at(ln[0]), at(ln[1]), 1e-5, at(w1p[0]), at(w1p[1]), at(b1), at(w2p[0]), at(w2p[1]), at(b2), at(res), C, alpha,
                                 at(out), C, at(ws), nws, B, T, C, H, ACT[act], at(post[0]) if post else None, at(post[1]) if post else None, 1e-5,
                                 at(out_ln), _lib.current_stream_handle()), "ffn_split")
    return flat, out, flat_ln, out_ln


@pytest.mark.gpu
@pytest.mark.parametrize("B,T", BT)
@pytest.mark.parametrize("H", [512, 2048])
@pytest.mark.parametrize("post", [False, True], ids=["plain", "postln"])
def test_batch_rows_ffn_split(B, T, H, post):
    C = 256
    torch.manual_seed(9400 + B + H + int(post))
    x = torch.randn(B, T, C, device=DEV) * 1.5 + 0.25
    res = torch.randn(B, T, C, device=DEV)
    ln = (torch.randn(C, device=DEV) * 0.3 + 1.0, torch.randn(C, device=DEV) * 0.3)
    w1 = torch.randn(H, C, 1, device=DEV) / C ** 0.5; b1 = torch.randn(H, device=DEV) * 0.1
    w2 = torch.randn(C, H, 1, device=DEV) / H ** 0.5; b2 = torch.randn(C, device=DEV) * 0.1
    w1p = pack(w1, C)
    parts = [pack(w2[:, s:s + 512].contiguous(), 512) for s in range(0, H, 512)]
    w2p = (torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts]))
    pl = (torch.randn(C, device=DEV) * 0.3 + 1.0, torch.randn(C, device=DEV) * 0.3) if post else None
    flat, got, flat_ln, got_ln = ffn_call(x, ln, w1p, b1, w2p, b2, res, 0.5, H, "silu", pl, True)
    case = f"B={B} T={T} H={H} post={post}"
    for b in range(B):
        f1, want, f1_ln, want_ln = ffn_call(x[b:b + 1].contiguous(), ln, w1p, b1, w2p, b2, res[b:b + 1].contiguous(), 0.5, H, "silu", pl, True)
        assert torch.equal(got[b:b + 1], want), (case, b, "rows differ from the B = 1 call in", int((got[b:b + 1] != want).sum().item()), "elements")
        assert f1[-1].item() == CANARY
        if post:
            assert torch.equal(got_ln[b:b + 1], want_ln), (case, b, "post-LayerNorm rows differ from the B = 1 call")
            assert f1_ln[-1].item() == CANARY
    assert torch.isfinite(got).all() and not (got == CANARY).any(), case
    assert flat[-1].item() == CANARY, (case, "the 4 bytes after out were written")
    if post:
        assert torch.isfinite(got_ln).all() and not (got_ln == CANARY).any() and flat_ln[-1].item() == CANARY, case
        # only the normalised rows (out = NULL): the same bits
        _, none_out, f2_ln, only_ln = ffn_call(x, ln, w1p, b1, w2p, b2, res, 0.5, H, "silu", pl, False)
        assert none_out is None and torch.equal(only_ln, got_ln) and f2_ln[-1].item() == CANARY, case
    # the module itself, in fp64, within the bound tests/test_gpu_ffn_fused.py holds this kernel to (2e-6 of max |ref64|)
    xn = torch.nn.functional.layer_norm(x.double(), (C,), ln[0].double(), ln[1].double(), 1e-5)
    h = torch.nn.functional.silu(xn @ w1[:, :, 0].double().T + b1.double())
    r64 = res.double() + 0.5 * (h @ w2[:, :, 0].double().T + b2.double())
    err = (got.double() - r64).abs().max().item() / r64.abs().max().item()
    print(f"\n[batch-rows] ffn {case}: err {err:.3e}")
    assert err < 2e-6, (case, err)
