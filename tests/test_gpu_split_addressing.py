"""Fragment addressing of the split-operand MFMA loops (csrc/split_frag.h: conv1d_split_kernel, hifigan_resunit_f32_kernel,
hifigan_conv_f32_kernel): every output bit is the one the kernels produced BEFORE the address arithmetic left their K steps.

tests/golden/split_addressing_parent.npz was written once by tools/split_addressing_golden.py on a build of the commit before that
change.  Inputs are a seed each (torch's device generator), so the file holds outputs only — and since the 456 outputs of the cases
below are 600 MB (the 36 unit shapes alone 400 MB) against a 1 MiB limit per committed file, it holds of each output: the SHA-256 of its
fp32 bytes (equal digests are equal bits), a CRC-32 of every block of 16 output rows, so that a failure names the rows whose bits moved,
and 16 evenly spaced elements, compared with torch.equal so that it shows values.  Every case is also held to an fp64 reference within
the bound the existing split-precision tests use for its kernel:
    conv1d_split        err < 4e-6 and err < 8 err32 + 1e-6, in units of max |ref64|; err32 = the plain fp32 evaluation beside it
                        (tests/test_gpu_decode_ops.py::test_split_precision_conv1d_is_fp32_accurate)
    hifigan fp32        _unit_case (a) / _conv_case of tests/test_gpu_hifigan_layers.py, as they stand

The shapes are the smallest at which an address can go wrong: B = 2, T one short of the time tile, one past it, and 2 tiles + 3.

conv1d_split (cs_run picks the instance; NT = its time tile; M = 272 leaves a partial 16-row output tile unless the instance needs the
workgroup count of a wide layer):
    cs128   <128,128,256,4,2>   CI 128, one slice, taps 1 / 3 / 9, residual, GELU / none / SiLU
    cs256n  <256,128,64,8,1>    CI 256, two slices, taps 9 / 3 / 1, ragged lens with slack, ReLU / GELU / SiLU
    cs256ln <256,256,64,8,1>    the LayerNorm-staged instance (dsp_linear_ln_split), one ragged
    cs256w  <256,256,128,8,1>   eight slices x eight tap groups of K = 9 (split-K fills the 256 workgroups the 128-row tile asks for)
    cs512n  <512,256,32,8,1>    CI 512, two slices, K = 3 — at T = NT + 1 as split-K with 2 tap groups
    cs512x  <512,256,64,16,1>   the 16-wave path: one tap, one slice, M = 16144 (128 workgroups), residual
    cs512w  <512,256,64,8,1>    two slices, K = 3, split-K with 2 tap groups, M = 3856
hifigan_resunit_f32: C in {32, 64, 128, 256} x k in {3, 7, 11} x dilation in {1, 3, 5}, T in {nt - 1, nt + 1, 2 nt + 3} (nt: unit_tile of
    tests/test_gpu_hifigan_tap_tiles.py), with and without per-sample lengths, STORE and ACCUM.
hifigan_conv_f32: conv_pre (80 channels padded to 96, k = 7), the 512 -> 256 upsampler at u = 8 and the 128 -> 64 one at u = 2, each two
    columns past a tile edge.
"""
import hashlib
import os
import zlib

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "split_addressing_parent.npz")
DEV = "cuda:0"
NSAMPLE = 16


def digest(t):
    """(SHA-256 of the fp32 bytes, NSAMPLE evenly spaced elements, CRC-32 of each block of 16 rows of the [rows, channels] view)"""
    a = t.detach().float().contiguous().cpu().numpy()
    idx = np.linspace(0, a.size - 1, NSAMPLE).astype(np.int64)
    rows = a.reshape(-1, a.shape[-1])
    crc = np.array([zlib.crc32(rows[r:r + 16].tobytes()) for r in range(0, rows.shape[0], 16)], dtype=np.uint32)
    return hashlib.sha256(a.tobytes()).hexdigest(), a.reshape(-1)[idx].copy(), crc


# ------------------------------------------------------------------------------------------------------------------ conv1d_split
ACT = {None: 0, "relu": 1, "silu": 2, "gelu": 3}
# tag: (CI, nslices, M, NT, per T index: (K, act, mode)); mode: plain / res / ragged / ksplit:<tap groups> / ln / lnragged
CS_CASES = {
    "cs128": (128, 1, 272, 256, [(1, "gelu", "res"), (3, None, "res"), (9, "silu", "res")]),
    "cs256n": (256, 2, 272, 64, [(9, "relu", "ragged"), (3, "gelu", "ragged"), (1, "silu", "ragged")]),
    "cs256ln": (256, 1, 272, 64, [(1, "relu", "ln"), (1, None, "lnragged"), (1, "gelu", "ln")]),
    "cs256w": (256, 8, 272, 128, [(9, "relu", "ksplit:8"), (9, None, "ksplit:8"), (9, "silu", "ksplit:8")]),
    "cs512n": (512, 2, 272, 32, [(3, None, "plain"), (3, "relu", "ksplit:2"), (3, "gelu", "res")]),
    "cs512x": (512, 1, 16144, 64, [(1, "relu", "res"), (1, None, "plain"), (1, "silu", "res")]),
    "cs512w": (512, 2, 3856, 64, [(3, "gelu", "ksplit:2"), (3, "relu", "ksplit:2"), (3, None, "ksplit:2")]),
}


def cs_instance(CI, nslices, M, K, B, T, mode):
    """cs_run's choice (csrc/conv1d_split.hip), restated: the cases above must reach the instance their tag names."""
    kmul = nslices * int(mode.split(":")[1]) if mode.startswith("ksplit") else 1
    if mode.startswith("ln"):
        return (256, 256, 64, 8)
    mt = (M + 255) // 256
    if CI == 256:
        if ((T + 127) // 128) * mt * B * kmul >= 256:
            return (256, 256, 128, 8)
        return (256, 128, 64, 8) if ((T + 63) // 64) * mt * B * kmul < 150 else (256, 256, 64, 8)
    if CI == 512:
        if K <= 9 and ((T + 63) // 64) * mt * B * kmul < 128:
            return (512, 256, 32, 8)
        return (512, 256, 64, 16) if (K == 1 and nslices == 1 and kmul == 1) else (512, 256, 64, 8)
    return (128, 128, 256, 8)


CS_WANT = {"cs128": (128, 128, 256, 8), "cs256n": (256, 128, 64, 8), "cs256ln": (256, 256, 64, 8), "cs256w": (256, 256, 128, 8),
           "cs512n": (512, 256, 32, 8), "cs512x": (512, 256, 64, 16), "cs512w": (512, 256, 64, 8)}


def cs_ts(NT):
    return (NT - 1, NT + 1, 2 * NT + 3)


def test_conv1d_split_cases_reach_the_instances_they_name():
    for tag, (CI, ns, M, NT, per_t) in CS_CASES.items():
        for T, (K, _, mode) in zip(cs_ts(NT), per_t):
            assert cs_instance(CI, ns, M, K, 2, T, mode) == CS_WANT[tag], (tag, T)


def run_cs_case(tag, ti):
    """One conv1d_split launch through the C ABI; returns (output, ref64, ref32, rows to compare per sample)."""
    from daspeech_amd import _lib
    lib = _lib.load()
    CI, ns, M, NT, per_t = CS_CASES[tag]
    K, act, mode = per_t[ti]
    B, T, Cin = 2, cs_ts(NT)[ti], CI * ns
    torch.manual_seed(40000 + 100 * sorted(CS_CASES).index(tag) + ti)
    x = torch.randn(B, T, Cin, device=DEV) * 1.5 + 0.25
    w = torch.randn(M, Cin, K, device=DEV) / (Cin * K) ** 0.5
    bias = torch.randn(M, device=DEV) * 0.1
    res = torch.randn(B, T, M, device=DEV) if mode in ("res", "ragged", "lnragged") or mode.startswith("ksplit") else None
    alpha = 0.5 if res is not None else 1.0
    ln_w = ln_b = None
    if mode.startswith("ln"):
        ln_w, ln_b = torch.randn(CI, device=DEV) * 0.3 + 1.0, torch.randn(CI, device=DEV) * 0.3
    lens = slack = None
    if mode in ("ragged", "lnragged"):
        lens, slack = torch.tensor([T, max(T - NT - 9, 3)], device=DEV, dtype=torch.int32), 5
    st = _lib.current_stream_handle()
    n = lib.dsp_conv1d_split_packed_elems(K, M, CI)
    hi = torch.empty(ns * n, dtype=torch.float16, device=DEV); lo = torch.empty_like(hi)
    for sl in range(ns):
        wt = w[:, sl * CI:(sl + 1) * CI, :].permute(2, 0, 1).contiguous()
        _lib.check(lib.dsp_conv1d_split_pack(_lib.ptr(wt), hi.data_ptr() + 2 * sl * n, lo.data_ptr() + 2 * sl * n, K, M, CI, st), "pack")
    out = torch.full((B, T, M), 777.0, device=DEV)
    p = _lib.ptr
    if mode.startswith("ln"):
        _lib.check(lib.dsp_linear_ln_split(p(x), Cin, p(ln_w), p(ln_b), 1e-5, p(hi), p(lo), p(bias), p(res), M, alpha, p(out), M, B, T, M, ACT[act],
                                           p(lens), slack or 0, st), "linear_ln_split")
    elif mode.startswith("ksplit"):
        tg = int(mode.split(":")[1])
        nws = lib.dsp_conv1d_split_ksplit_workspace_bytes(B, T, M, ns, tg)
        ws = torch.empty(nws // 4, device=DEV)
        _lib.check(lib.dsp_conv1d_split_ksplit(p(x), Cin, p(hi), p(lo), p(bias), p(res), M, alpha, p(out), M, B, T, CI, ns, M, K, ACT[act], tg, p(ws), nws,
                                               None, 0, st), "ksplit")
    elif mode == "ragged":
        _lib.check(lib.dsp_conv1d_split_ragged(p(x), Cin, p(hi), p(lo), p(bias), p(res), M, alpha, p(out), M, B, T, CI, ns, M, K, ACT[act], p(lens), slack, st), "ragged")
    elif mode == "res":
        _lib.check(lib.dsp_conv1d_split_residual(p(x), Cin, p(hi), p(lo), p(bias), p(res), M, alpha, p(out), M, B, T, CI, ns, M, K, ACT[act], st), "residual")
    else:
        _lib.check(lib.dsp_conv1d_split(p(x), Cin, p(hi), p(lo), p(bias), p(out), M, B, T, CI, ns, M, K, ACT[act], 0, st), "conv1d_split")

    def ref(dt):
        xx = x.to(dt)
        if ln_w is not None:
            xx = torch.nn.functional.layer_norm(xx, (CI,), ln_w.to(dt), ln_b.to(dt), 1e-5)
        v = torch.nn.functional.conv1d(xx.transpose(1, 2), w.to(dt), bias.to(dt), padding=(K - 1) // 2).transpose(1, 2)
        v = {None: lambda t: t, "relu": torch.relu, "silu": torch.nn.functional.silu, "gelu": torch.nn.functional.gelu}[act](v)
        return alpha * v if res is None else res.to(dt) + alpha * v
    # rows computed: every tile that starts below lens[b] + slack; the tiles after it come back as zeros
    rows = [T] * B if lens is None else [min(T, -(-(int(n) + slack) // NT) * NT) for n in lens.tolist()]
    return out, ref(torch.float64), ref(torch.float32), rows


def check_cs_fp64(out, ref64, ref32, rows, case):
    assert torch.isfinite(out).all(), case
    live = torch.arange(out.shape[1], device=DEV)[None, :, None] < torch.tensor(rows, device=DEV)[:, None, None]
    scale = (ref64.abs() * live).max().item()
    err = ((out.double() - ref64).abs() * live).max().item() / scale
    err32 = ((ref32.double() - ref64).abs() * live).max().item() / scale
    print(f"\n[split-addressing] {case}: err {err:.3e}  err32 {err32:.3e}")
    assert err < 4e-6 and err < 8 * err32 + 1e-6, (case, err, err32)
    for b, n in enumerate(rows):
        assert (out[b, n:] == 0).all(), (case, "skipped tiles must be zeros", b)


# ------------------------------------------------------------------------------------------------------------------ hifigan fp32
UNITS = [(C, K, d) for C in (32, 64, 128, 256) for K in (3, 7, 11) for d in (1, 3, 5)]
CONVS = {"conv_pre": (96, 512, 1, 128), "up8": (512, 256, 8, 64), "up2": (128, 64, 2, 256)}        # CI, Cout, u, NT of hgs_conv_one


def run_unit_cases(C, K, dil):
    """[(key, output)] of one (C, K, dilation): 3 T x (dense, ragged) x (STORE, ACCUM), each inside _unit_case's fp64 bound."""
    from tests.test_gpu_hifigan_layers import Worst, _unit_case
    from tests.test_gpu_hifigan_tap_tiles import unit_tile
    h1, h2 = dil * (K - 1) // 2, (K - 1) // 2
    nt = unit_tile(C, K, dil)[1]
    worst, outs, n = Worst(f"split addressing unit C={C} K={K} dil={dil} (nt {nt})"), [], 0
    for T in (nt - 1, nt + 1, 2 * nt + 3):
        for ragged in (0, 1):
            for accumulate in (0, 1):
                kw = dict(lens=torch.tensor([T, T - h1 - h2 - 1], device=DEV, dtype=torch.int32), T0=T) if ragged else {}
                out = _unit_case(21000 + 17 * n + C + K, False, 2, T, C, K, dil, accumulate, worst, chain_too=False, **kw)
                if ragged:                       # rows past a sample's length are unspecified (whole tiles are skipped)
                    out = torch.cat([out[0], out[1, :T - h1 - h2 - 1]])
                outs.append((f"unit-{C}-{K}-{dil}-T{T}-r{ragged}-a{accumulate}", out))
                n += 1
    worst.report()
    return outs


def run_conv_case(tag):
    from tests.test_gpu_hifigan_layers import Worst, _conv_case
    from tests.util_hifigan_ref import OUT_STORE, OUT_UPSAMPLE, conv_shifts
    CI, Cout, u, NT = CONVS[tag]
    worst = Worst(f"split addressing {tag}")
    T = NT + 2
    if u == 1:
        out = _conv_case(31000, False, 2, T, CI, Cout, conv_shifts(7, 1), 1.0, True, False, OUT_STORE, 1.0, worst)
    else:
        out = _conv_case(31000 + u, False, 2, T, CI, Cout, [0, -1], 0.1, True, False, OUT_UPSAMPLE, 1.0, worst, u=u, pad=u // 2)
    worst.report()
    return [(f"conv-{tag}-T{T}", out)]


# ------------------------------------------------------------------------------------------------------------------ golden
_golden = None


def golden():
    global _golden
    if _golden is None:
        z = np.load(GOLDEN)
        off, crc = z["crc_offsets"], z["crc16rows"]
        _golden = {k: (d, s, crc[off[i]:off[i + 1]]) for i, (k, d, s) in enumerate(zip(z["keys"].tolist(), z["sha256"].tolist(), z["samples"]))}
    return _golden


def assert_parent_bits(key, out):
    d, s, crc = digest(out)
    want_d, want_s, want_crc = golden()[key]
    assert torch.equal(torch.from_numpy(s), torch.from_numpy(want_s)), (key, s, want_s)
    assert crc.shape == want_crc.shape, (key, tuple(out.shape))
    moved = np.nonzero(crc != want_crc)[0]
    assert moved.size == 0, (key, tuple(out.shape), "16-row blocks of the [rows, channels] view whose bits differ from the parent build's", moved[:20].tolist())
    assert d == want_d, (key, "SHA-256 of the output differs from the parent build's")


CS_IDS = [(tag, ti) for tag in CS_CASES for ti in range(3)]


@pytest.mark.gpu
@pytest.mark.parametrize("tag,ti", CS_IDS, ids=[f"{t}-{i}" for t, i in CS_IDS])
def test_conv1d_split_bits_of_the_parent(tag, ti):
    out, ref64, ref32, rows = run_cs_case(tag, ti)
    check_cs_fp64(out, ref64, ref32, rows, f"{tag} T index {ti}")
    assert_parent_bits(f"{tag}-{ti}", out)


@pytest.mark.gpu
@pytest.mark.parametrize("C,K,dil", UNITS, ids=[f"{c}-{k}-{d}" for c, k, d in UNITS])
def test_resunit_f32_bits_of_the_parent(C, K, dil):
    for key, out in run_unit_cases(C, K, dil):
        assert_parent_bits(key, out)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(CONVS))
def test_conv_f32_bits_of_the_parent(tag):
    for key, out in run_conv_case(tag):
        assert_parent_bits(key, out)
