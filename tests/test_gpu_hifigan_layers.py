"""Every HiFi-GAN HIP layer kernel (csrc/hifigan_conv_f32.hip, csrc/hifigan_conv.hip) as ONE layer record against the plain fp64
reference of tests/util_hifigan_ref.py, at the tile edges of each compiled instance.

Error scale: A = the layer's sum over magnitudes (ref_abs_layer).  Comparator: e32 = max |plain fp32 evaluation - fp64| / A of the same
layer on the same data, measured in the same test.

    fp32 (split) path   max |got - ref64| / A <= 3 * 2^-22 + 3 * max(e32, 2^-24)
                        3 * 2^-22: two operand splits and the dropped wl.xl product, <= 2^-22 each (tests/test_hifigan_layer_ref.py shows
                        the emulated split inside it and an emulation without a correction product 50x outside); the second term is the
                        fp32 accumulation and output rounding, order dependent, with the 3x margin of tests/test_gpu_ffn_fused.py
    fp16-storage path   |got - ref64| <= 2^-11 |ref64| + 3 * max(e32, 2^-24) * A      on fp16-exact inputs: one fp16 rounding of the output
                        (single records: the reference starts from the operand as the kernel stages it, leaky_relu applied in fp16)

Compiled instance -> case that launches it:
    hgs_launch<512,256,64,8,1> / <256,256,64,8,1> / <128,128,256,4,2> / <96,256,128,8,1> / <64,64,512,2,4> / <32,32,512,1,8>
        test_conv_store_f32[CI] (and the ACCUM, UPSAMPLE, partial-M, lens cases at the same CI)
    hgs_unit_launch<256,48,8,1>   test_unit_f32[256-*]        hgs_unit_launch<64,240,2,4>   test_unit_f32[64-*]
    hgs_unit_launch<32,496,1,8>   test_unit_f32[32-*]         hgs_unit_launch<128,112,8,1>  test_unit_f32[128-K-dil], h1 <= 16
    hgs_unit_launch<128,96,8,1>   test_unit_f32[128-11-4], [128-9-5] (h1 = 20)              hgs_unit_launch<128,80,8,1>  test_unit_f32[128-11-5] (h1 = 25)
Every test prints its worst normalised error, e32 and bound (pytest -s).  Measured on an MI355X (worst case of each family, in units of A):
    family                 err        e32        bound          family                 err        e32        bound
    conv STORE fp32        1.5e-07    6.7e-08    9.2e-07        conv STORE fp16        9.5e-05    1.7e-07    1.2e-04
    conv ACCUM fp32        1.7e-07    1.3e-07    1.1e-06        UPSAMPLE fp16          2.4e-04    1.8e-07    2.7e-04
    UPSAMPLE fp32          1.4e-07    1.7e-07    1.2e-06        partial M fp16         2.7e-04    1.3e-07    3.7e-04
    partial M fp32         1.4e-07    9.8e-08    1.0e-06        unit fp16 (a)          3.4e-04    2.1e-07    9.3e-04
    unit fp32, per step    1.6e-07    6.1e-08    9.0e-07        lens fp16              4.2e-04    2.8e-07    1.0e-03
    unit fp32 (a)          1.9e-07    1.8e-07    2.2e-05        post fp32 / fp16       1.2e-07    5.1e-08    8.9e-07
    lens fp32              1.6e-07    2.1e-07    1.3e-06        long rows fp32         1.8e-07    1.4e-07    1.1e-06
A split kernel without one correction product sits at 5e-5 .. 9e-5 on the single-record cases (tried once on a scratch build: every fp32
conv, upsample, partial-M, unit, lens and long-row case fails); a valid length one row short fails the lens and post cases.
"""
import pytest
import torch

from tests.util_hifigan_ref import (OUT_ACCUM, OUT_STORE, OUT_UPSAMPLE, conv_shifts, ref_abs_layer, ref_layer, ref_post,
                                    valid_lens)

pytestmark = pytest.mark.gpu

# the comparator has to be a true fp32 evaluation
torch.backends.cuda.matmul.allow_tf32 = False

DEV = "cuda:0"
SPLIT = 3 * 2.0 ** -22          # derived: see the module docstring
FLOOR = 2.0 ** -24
HALF_ULP16 = 2.0 ** -11
EINVAL = -1

F32_NT = {512: 64, 256: 64, 128: 256, 96: 128, 64: 512, 32: 512}        # hgs_conv_one
F32_MT = {512: 256, 256: 256, 128: 128, 96: 256, 64: 64, 32: 32}
F16_NT = {512: 128, 256: 128, 128: 256, 96: 128, 64: 512, 32: 512}       # hg_conv_one
CONV_KD = [(1, 1), (3, 1), (7, 3), (11, 5)]


def _ops():
    from daspeech_amd import hifigan_ops
    return hifigan_ops


def _last_error():
    from daspeech_amd import _lib
    return _lib.load().dsp_last_error().decode("utf-8", "replace")


def _rand(*shape, s=1.0):
    return torch.randn(*shape, device=DEV) * s


def _q(t, f16):
    """fp16 path: make the data fp16-exact first (kept in fp32 for the references)."""
    return t.half().float() if (f16 and t is not None) else t


def _dev(t, f16):
    return None if t is None else (t.half() if f16 else t).contiguous()


def _pack(w, f16):
    ops = _ops()
    return ops.pack_weights(w.half()) if f16 else ops.pack_weights_f32(w)


def _d(t):
    return None if t is None else t.double()


class Worst:
    """Worst normalised error of a family, with the comparator and bound of that case."""

    def __init__(self, family):
        self.family, self.n, self.e32, self.bound, self.case = family, -1.0, 0.0, 0.0, None

    def add(self, n, e32, bound, case):
        if n > self.n:
            self.n, self.e32, self.bound, self.case = n, e32, bound, case

    def report(self):
        print(f"\n[hifigan-layers] {self.family}: worst err/A {self.n:.3e}  e32 {self.e32:.3e}  bound {self.bound:.3e}  case {self.case}")


def _row_mask(B, Tout, vl_out):
    return (torch.arange(Tout, device=DEV)[None, :, None] < torch.tensor(vl_out, device=DEV)[:, None, None])


def _check(got, ref64, A, ref32, f16, case, worst, mask=None):
    """The tolerance of the module docstring, element-wise over the rows of `mask` (default: all)."""
    assert torch.isfinite(got).all(), case
    live = torch.ones_like(A, dtype=torch.bool) if mask is None else mask.expand_as(A)
    if not live.any():
        return
    An = A.clamp_min(1e-300)
    e32 = float(((ref32.double() - ref64).abs() / An)[live].max())
    acc = 3 * max(e32, FLOOR)
    err = (got.double() - ref64).abs()
    if f16:
        allow = HALF_ULP16 * ref64.abs() + acc * A
        n, bound = float((err / An)[live].max()), float((allow / An)[live].max())
        worst.add(n, e32, bound, case)
        bad = (err > allow) & live
        assert not bad.any(), (case, "worst err/allow", float((err / allow.clamp_min(1e-300))[live].max()), "e32", e32)
    else:
        n, bound = float((err / An)[live].max()), SPLIT + acc
        worst.add(n, e32, bound, case)
        assert n <= bound, (case, "err/A", n, "e32", e32, "bound", bound, "at", _where(err / An * live, got.shape))


def _where(t, shape):
    i = int(t.reshape(-1).argmax())
    out = []
    for s in reversed(shape):
        out.append(i % s); i //= s
    return tuple(reversed(out))


def _conv_case(seed, f16, B, T, CI, Cout, shifts, slope, use_bias, use_res, mode, scale, worst, u=1, pad=0, lens=None, T0=0, tag=""):
    """One single-layer record against fp64; returns (got, launch arguments) for the bit-identity checks of the lens cases."""
    ops = _ops()
    torch.manual_seed(seed)
    M = Cout * u
    K = len(shifts)
    Tout = T * u
    x = _q(_rand(B, T, CI, s=1.5), f16)
    w = _q(_rand(K, M, CI, s=1.0 / (CI * K) ** 0.5), f16)
    bias = _rand(Cout, s=0.1) if use_bias else None
    res = _q(_rand(B, Tout, Cout), f16) if use_res else None
    prev = _q(_rand(B, Tout, Cout), f16) if mode == OUT_ACCUM else None
    out = _dev(prev.clone() if prev is not None else torch.full((B, Tout, Cout), 777.0, device=DEV), f16)
    len_mul = T // T0 if lens is not None else 1
    ops.launch_layer(_dev(x, f16), _pack(w, f16), bias, _dev(res, f16), out, shifts, slope, scale, mode, u, pad, lens=lens, T0=T0)
    args = (shifts, slope, scale, mode, u, pad, Tout, Cout, None if lens is None else lens.tolist(), len_mul)
    if f16 and slope != 1.0:
        # fp16 storage: the MFMA operand is the staged fp16 tile, and hg_stage_tile applies the leaky_relu in fp16 (x * fp16(slope), rounded
        # to fp16).  That rounding is the storage format's, not the layer arithmetic's, so the reference starts from the staged operand,
        # as it starts from fp16-exact x and w (and as the unit's reference rounds the intermediate the unit stores in fp16).
        xh = x.half()
        x = torch.where(xh > 0, xh, xh * torch.tensor(slope, device=DEV).half()).float()
        args = (shifts, 1.0) + args[2:]
    ref64 = ref_layer(_d(x), _d(w), _d(bias), _d(res), _d(prev), *args)
    A = ref_abs_layer(_d(x), _d(w), _d(bias), _d(res), _d(prev), *args)
    ref32 = ref_layer(x, w, bias, res, prev, *args)
    mask = None if lens is None else _row_mask(B, Tout, [v * u for v in valid_lens(B, T, lens.tolist(), len_mul)])
    case = f"{tag} {'f16' if f16 else 'f32'} B={B} T={T} CI={CI} Cout={Cout} K={K} shifts={shifts[0]}..{shifts[-1]} slope={slope} bias={use_bias} res={use_res} mode={mode} u={u}"
    _check(out.float(), ref64, A, ref32, f16, case, worst, mask)
    return out


def _t_list(NT, halo):
    return sorted({1, 2, max(halo, 1), NT - 1, NT, NT + 1, 2 * NT + 3, 5 * NT + 7})


def _admitted(CI, NT, halo, esz):
    return (NT + halo) * CI * esz <= 160 * 1024


# ---------------------------------------------------------------------------------------------------------------- single conv, STORE
@pytest.mark.parametrize("CI", [512, 256, 128, 96, 64, 32])
def test_conv_store_f32(CI):
    """hgs_launch<CI, ...> at (K, dil) x T around its time tile; slope 0.1 / none, with and without bias / res, B 1 and 3."""
    worst, n = Worst(f"conv STORE fp32 CI={CI}"), 0
    NT = F32_NT[CI]
    for K, dil in CONV_KD:
        halo = dil * (K - 1)
        if not _admitted(CI, NT, halo, 4):
            continue
        for T in _t_list(NT, halo):
            _conv_case(1000 + n, False, (1, 3)[n % 2], T, CI, CI, conv_shifts(K, dil), (0.1, 1.0)[(n // 2) % 2], (n // 4) % 2 == 0, (n // 8 + n) % 2 == 0,
                       OUT_STORE, 1.0, worst)
            n += 1
    assert n >= 14
    worst.report()


@pytest.mark.parametrize("CI", [512, 256, 128, 96, 64, 32])
def test_conv_store_f16(CI):
    """The fp16-storage twin (hg_launch<CI, ...>) where its output is rounded once: STORE, scale 1, no residual (with a residual, a scale
    or ACCUM the kernel rounds acc + bias to fp16 before the epilogue arithmetic: that path is pinned through the fused-unit cases)."""
    worst, n = Worst(f"conv STORE fp16 CI={CI}"), 0
    NT = F16_NT[CI]
    for K, dil in [(3, 1), (11, 5)]:
        halo = dil * (K - 1)
        if not _admitted(CI, NT, halo, 2):
            continue
        for T in sorted({1, max(halo, 1), NT - 1, NT + 1, 2 * NT + 3}):
            _conv_case(1500 + n, True, (1, 3)[n % 2], T, CI, CI, conv_shifts(K, dil), (0.1, 1.0)[(n // 2) % 2], (n // 4) % 2 == 0, False,
                       OUT_STORE, 1.0, worst)
            n += 1
    assert n >= 5
    worst.report()


# ---------------------------------------------------------------------------------------------------------------- ACCUM
@pytest.mark.parametrize("CI", [512, 256, 128, 96, 64, 32])
def test_conv_accum_f32(CI):
    worst, n = Worst(f"conv ACCUM fp32 CI={CI}"), 0
    NT = F32_NT[CI]
    for K, dil in [(3, 1), (7, 3)]:
        if not _admitted(CI, NT, dil * (K - 1), 4):
            continue
        for T in (1, NT - 1, NT + 1, 2 * NT + 3):
            _conv_case(2000 + n, False, (3, 1)[n % 2], T, CI, CI, conv_shifts(K, dil), 0.1, True, n % 3 != 0, OUT_ACCUM, 1.0 / 3, worst)
            n += 1
    worst.report()


# ---------------------------------------------------------------------------------------------------------------- UPSAMPLE
@pytest.mark.parametrize("CI,Cout,u", [(512, 256, 8), (256, 128, 8), (128, 64, 2), (64, 32, 2)])
@pytest.mark.parametrize("f16", [False, True])
def test_upsample(CI, Cout, u, f16):
    """The four V1 upsamplers (two taps, shifts {0, -1}, M = u * Cout phase-major rows, ncol = T + 1 columns) against the
    conv_transpose1d semantics of ref_layer (tests/test_hifigan_layer_ref.py pins those to torch's conv_transpose1d in fp64)."""
    worst, n = Worst(f"UPSAMPLE {'fp16' if f16 else 'fp32'} {CI}->{Cout} u={u}"), 0
    NT = (F16_NT if f16 else F32_NT)[CI]
    for T in (1, NT - 1, NT, NT + 1):
        _conv_case(3000 + n, f16, (1, 3)[n % 2], T, CI, Cout, [0, -1], 0.1, n != 1, False, OUT_UPSAMPLE, 1.0, worst, u=u, pad=u // 2)
        n += 1
    worst.report()


# ---------------------------------------------------------------------------------------------------------------- partial M tiles
@pytest.mark.parametrize("CI", [256, 32, 128])
def test_conv_partial_output_row_tiles_f32(CI):
    """Cout not a multiple of the M tile (nor of 16): the zero rows of the weight packer and the M edge of the epilogue."""
    worst, n = Worst(f"partial M fp32 CI={CI}"), 0
    NT = F32_NT[CI]
    for Cout in (4, 20, F32_MT[CI] + 16):
        for T in (3, NT + 1):
            _conv_case(4000 + n, False, (3, 1)[n % 2], T, CI, Cout, conv_shifts(3, 1), 0.1, True, n % 2 == 0, OUT_STORE, 1.0, worst)
            _conv_case(4100 + n, False, 1, T, CI, Cout, conv_shifts(7, 3), 1.0, n % 2 == 1, True, OUT_ACCUM, 0.5, worst)
            n += 1
    worst.report()


def test_conv_partial_output_row_tiles_f16():
    worst, n = Worst("partial M fp16"), 0
    for CI in (256, 32):
        for Cout in (8, 24, F32_MT[CI] + 16):
            _conv_case(4500 + n, True, 2, F16_NT[CI] + 1, CI, Cout, conv_shifts(3, 1), 0.1, True, False, OUT_STORE, 1.0, worst)
            n += 1
    worst.report()


# ---------------------------------------------------------------------------------------------------------------- fused units
def _unit_data(seed, f16, B, T, C, K):
    torch.manual_seed(seed)
    s = 1.0 / (C * K) ** 0.5
    return dict(x=_q(_rand(B, T, C, s=1.5), f16), w1=_q(_rand(K, C, C, s=s), f16), w2=_q(_rand(K, C, C, s=s), f16),
                b1=_rand(C, s=0.1), b2=_rand(C, s=0.1), prev=_q(_rand(B, T, C), f16))


def _unit_bound(d, K, dil, slope, scale, accumulate, f16, lens, len_mul):
    """(ref64, element-wise absolute bound, A2, e32 of the two convs).  The first conv's allowance tol1 (per element of the intermediate)
    is carried through the second conv's |w2| (leaky_relu is 1-Lipschitz), the second conv adds its own, all times scale."""
    B, T, C = d["x"].shape
    x, w1, w2, b1, b2 = d["x"], d["w1"], d["w2"], d["b1"], d["b2"]
    prev = d["prev"] if accumulate else None
    a1 = (conv_shifts(K, dil), slope, 1.0, OUT_STORE, 1, 0, T, C, lens, len_mul)
    a2 = (conv_shifts(K, 1), slope, scale, OUT_ACCUM if accumulate else OUT_STORE, 1, 0, T, C, lens, len_mul)
    h64 = ref_layer(_d(x), _d(w1), _d(b1), None, None, *a1)
    A1 = ref_abs_layer(_d(x), _d(w1), _d(b1), None, None, *a1)
    e1 = float(((ref_layer(x, w1, b1, None, None, *a1).double() - h64).abs() / A1.clamp_min(1e-300)).max())
    if f16:
        h64 = h64.half().double()                       # the intermediate is stored in fp16 (LDS)
        tol1 = HALF_ULP16 * h64.abs() + 3 * max(e1, FLOOR) * A1
    else:
        tol1 = (SPLIT + 3 * max(e1, FLOOR)) * A1
    hin = h64.float()                                   # the second conv's comparator starts from the same intermediate
    ref64 = ref_layer(h64, _d(w2), _d(b2), _d(x), _d(prev), *a2)
    A2 = ref_abs_layer(h64, _d(w2), _d(b2), _d(x), _d(prev), *a2)
    r2 = ref_layer(hin, w2, b2, x, prev, *a2).double() - ref_layer(hin.double(), _d(w2), _d(b2), _d(x), _d(prev), *a2)
    e2 = float((r2.abs() / A2.clamp_min(1e-300)).max())
    carried = abs(scale) * ref_layer(tol1, _d(w2).abs(), None, None, None, conv_shifts(K, 1), 1.0, 1.0, OUT_STORE, 1, 0, T, C, lens, len_mul)
    own = (HALF_ULP16 * ref64.abs() + 3 * max(e2, FLOOR) * A2) if f16 else (SPLIT + 3 * max(e2, FLOOR)) * A2
    return ref64, carried + own, A2, max(e1, e2)


def _unit_case(seed, f16, B, T, C, K, dil, accumulate, worst, lens=None, T0=0, chain_too=True):
    ops = _ops()
    d = _unit_data(seed, f16, B, T, C, K)
    slope, scale = 0.1, 1.0 / 3
    W1, W2 = _pack(d["w1"], f16), _pack(d["w2"], f16)
    x = _dev(d["x"], f16)
    out = _dev(d["prev"].clone(), f16)
    sh1, sh2 = conv_shifts(K, dil), conv_shifts(K, 1)
    ops.launch_layer(x, W1, d["b1"], None, out, sh1, slope, scale, OUT_ACCUM if accumulate else OUT_STORE, w2=W2, bias2=d["b2"], lens=lens, T0=T0)
    case = f"unit {'f16' if f16 else 'f32'} B={B} T={T} C={C} K={K} dil={dil} accumulate={accumulate} lens={None if lens is None else lens.tolist()}"
    if chain_too:       # (b) bit-identical to the two one-record launches it replaces
        h = torch.zeros_like(x)
        o2 = _dev(d["prev"].clone(), f16)
        ops.launch_layer(x, W1, d["b1"], None, h, sh1, slope, 1.0, OUT_STORE, lens=lens, T0=T0)
        ops.launch_layer(h, W2, d["b2"], x, o2, sh2, slope, scale, OUT_ACCUM if accumulate else OUT_STORE, lens=lens, T0=T0)
        vl = valid_lens(B, T, None if lens is None else lens.tolist(), T // T0 if lens is not None else 1)
        for b in range(B):
            assert torch.equal(out[b, :vl[b]], o2[b, :vl[b]]), (case, "fused != chain", b, (out[b, :vl[b]].float() - o2[b, :vl[b]].float()).abs().max().item())
    ll = None if lens is None else lens.tolist()
    len_mul = T // T0 if lens is not None else 1
    if chain_too and not f16:
        # The worst-case bound of (a) carries the first conv's whole allowance through |w2| and ends far above what the kernels do.  The
        # chain the unit equals bit for bit can be held to the single-record tolerance at each of its two steps (the second from the
        # intermediate the first one wrote), which pins the unit as tightly as a single layer.
        a1 = (sh1, slope, 1.0, OUT_STORE, 1, 0, T, C, ll, len_mul)
        a2 = (sh2, slope, scale, OUT_ACCUM if accumulate else OUT_STORE, 1, 0, T, C, ll, len_mul)
        mrow = _row_mask(B, T, valid_lens(B, T, ll, len_mul))
        prev = d["prev"] if accumulate else None
        _check(h, ref_layer(_d(d["x"]), _d(d["w1"]), _d(d["b1"]), None, None, *a1), ref_abs_layer(_d(d["x"]), _d(d["w1"]), _d(d["b1"]), None, None, *a1),
               ref_layer(d["x"], d["w1"], d["b1"], None, None, *a1), False, case + " [first conv]", worst, mrow)
        _check(o2, ref_layer(_d(h), _d(d["w2"]), _d(d["b2"]), _d(d["x"]), _d(prev), *a2), ref_abs_layer(_d(h), _d(d["w2"]), _d(d["b2"]), _d(d["x"]), _d(prev), *a2),
               ref_layer(h, d["w2"], d["b2"], d["x"], prev, *a2), False, case + " [second conv]", worst, mrow)
    # (a) against fp64
    ref64, bound, A2, e32 = _unit_bound(d, K, dil, slope, scale, accumulate, f16, ll, len_mul)
    mask = _row_mask(B, T, valid_lens(B, T, ll, len_mul)).expand_as(ref64)
    assert torch.isfinite(out).all(), case
    err = (out.double() - ref64).abs()
    if mask.any():
        An = A2.clamp_min(1e-300)
        worst.add(float((err / An)[mask].max()), e32, float((bound / An)[mask].max()), case)
        assert not ((err > bound) & mask).any(), (case, "worst err/bound", float((err / bound.clamp_min(1e-300))[mask].max()), "e32", e32)
    return out


V1_KD = [(K, d) for K in (3, 7, 11) for d in (1, 3, 5)]
UNIT_F32 = [(C, K, d) for C in (32, 64, 128, 256) for K, d in V1_KD] + [(128, 11, 4), (128, 9, 5)]


def _unit_nt_f32(C, h1):
    if C == 128:
        return 112 if h1 <= 16 else 96 if h1 <= 24 else 80
    return {32: 496, 64: 240, 256: 48}[C]


@pytest.mark.parametrize("C,K,dil", UNIT_F32, ids=[f"{c}-{k}-{d}" for c, k, d in UNIT_F32])
def test_unit_f32(C, K, dil):
    """The fused ResBlock unit record of dsp_hifigan_conv_chain_f32 around its instance's tile: (a) fp64, (b) == its two layers."""
    from daspeech_amd import _lib
    assert _lib.load().dsp_hifigan_resunit_f32_supported(C, K, dil)
    h1 = dil * (K - 1) // 2
    NT = _unit_nt_f32(C, h1)
    worst, n = Worst(f"unit fp32 C={C} K={K} dil={dil} (NT {NT})"), 0
    for T in sorted({1, h1, NT - 1, NT, NT + 1, 3 * NT + h1}):
        for accumulate in (0, 1):
            _unit_case(5000 + 7 * n + C, False, (1, 3)[n % 2], T, C, K, dil, accumulate, worst)
            n += 1
    worst.report()


@pytest.mark.parametrize("C,K,dil,T", [(32, 11, 5, 1000), (32, 3, 1, 497), (64, 7, 3, 481), (64, 11, 5, 7), (128, 11, 5, 250), (128, 3, 1, 239),
                                       (32, 7, 3, 258111), (64, 11, 5, 127003), (64, 3, 1, 126976), (256, 11, 5, 300), (256, 3, 1, 111),
                                       (256, 7, 3, 113), (256, 7, 3, 22403)])
def test_unit_f16(C, K, dil, T):
    """dsp_hifigan_resunit's kernels through a one-record table at the shapes of test_hifigan_fused_resblock_unit_bit_identical_to_layer_chain
    (the long rows select the wide tiles by workgroup count), against ref_unit in fp64 with the intermediate rounded to fp16."""
    worst = Worst(f"unit fp16 C={C} K={K} dil={dil} T={T}")
    for accumulate in (0, 1):
        _unit_case(6000 + C + K + accumulate, True, 2, T, C, K, dil, accumulate, worst, chain_too=T < 5000)
        if T > 5000:
            torch.cuda.empty_cache()
    worst.report()


# ---------------------------------------------------------------------------------------------------------------- per-utterance lengths
@pytest.mark.parametrize("len_mul", [1, 8])
@pytest.mark.parametrize("f16", [False, True])
def test_lens_rows_equal_the_utterance_alone(len_mul, f16):
    """B = 4, lens = [T0, T0-1, 1, 0]: the rows below each utterance's length are within tolerance of the fp64 reference of the truncated
    utterance (ref_layer masks exactly so: tests/test_hifigan_layer_ref.py) and equal the single-utterance launch without lens bit for bit."""
    ops = _ops()
    worst = Worst(f"lens len_mul={len_mul} {'fp16' if f16 else 'fp32'}")
    T0 = 70
    T = T0 * len_mul
    lens = torch.tensor([T0, T0 - 1, 1, 0], device=DEV, dtype=torch.int32)
    # single conv (CI 128: 256-column tiles, CI 256: 64 / 128), upsampler, fused unit
    for seed, (CI, K, dil) in enumerate([(128, 7, 3), (256, 3, 1), (32, 11, 5)]):
        sh = conv_shifts(K, dil)
        out = _conv_case(7000 + seed, f16, 4, T, CI, CI, sh, 0.1, True, not f16, OUT_STORE, 1.0, worst, lens=lens, T0=T0, tag="lens")
        torch.manual_seed(7000 + seed)                        # the same draws as _conv_case
        x = _q(_rand(4, T, CI, s=1.5), f16); w = _q(_rand(K, CI, CI, s=1.0 / (CI * K) ** 0.5), f16); bias = _rand(CI, s=0.1)
        res = None if f16 else _rand(4, T, CI)
        for b, n in enumerate(valid_lens(4, T, lens.tolist(), len_mul)):
            if n == 0:
                continue
            alone = torch.empty(1, n, CI, device=DEV, dtype=out.dtype)
            ops.launch_layer(_dev(x[b:b + 1, :n], f16), _pack(w, f16), bias, None if res is None else res[b:b + 1, :n].contiguous(), alone, sh, 0.1, 1.0, OUT_STORE)
            assert torch.equal(alone[0], out[b, :n]), ("conv", CI, b, n)
    for seed, (CI, Cout, u) in enumerate([(128, 64, 2), (256, 128, 8)]):
        out = _conv_case(7100 + seed, f16, 4, T, CI, Cout, [0, -1], 0.1, True, False, OUT_UPSAMPLE, 1.0, worst, u=u, pad=u // 2, lens=lens, T0=T0, tag="lens")
        torch.manual_seed(7100 + seed)
        x = _q(_rand(4, T, CI, s=1.5), f16); w = _q(_rand(2, Cout * u, CI, s=1.0 / (CI * 2) ** 0.5), f16); bias = _rand(Cout, s=0.1)
        for b, n in enumerate(valid_lens(4, T, lens.tolist(), len_mul)):
            if n == 0:
                continue
            alone = torch.empty(1, n * u, Cout, device=DEV, dtype=out.dtype)
            ops.launch_layer(_dev(x[b:b + 1, :n], f16), _pack(w, f16), bias, None, alone, [0, -1], 0.1, 1.0, OUT_UPSAMPLE, u, u // 2)
            assert torch.equal(alone[0], out[b, :n * u]), ("upsample", CI, b, n)
    for seed, (C, K, dil) in enumerate([(128, 11, 5), (64, 7, 3), (256, 3, 1)]):
        for accumulate in (0, 1):
            out = _unit_case(7200 + seed, f16, 4, T, C, K, dil, accumulate, worst, lens=lens, T0=T0)
            d = _unit_data(7200 + seed, f16, 4, T, C, K)
            for b, n in enumerate(valid_lens(4, T, lens.tolist(), len_mul)):
                if n == 0:
                    continue
                alone = _dev(d["prev"][b:b + 1, :n].clone(), f16)
                ops.launch_layer(_dev(d["x"][b:b + 1, :n], f16), _pack(d["w1"], f16), d["b1"], None, alone, conv_shifts(K, dil), 0.1, 1.0 / 3,
                                 OUT_ACCUM if accumulate else OUT_STORE, w2=_pack(d["w2"], f16), bias2=d["b2"])
                assert torch.equal(alone[0], out[b, :n]), ("unit", C, b, n)
    worst.report()


# ---------------------------------------------------------------------------------------------------------------- conv_post, input packing
def _post(x, w, bias, slope, f16, lens=None, len_mul=1):
    from daspeech_amd import _lib
    lib = _lib.load()
    B, T, C = x.shape
    wav = torch.full((B, T), 777.0, device=DEV)
    st = _lib.current_stream_handle()
    xd = _dev(x, f16)
    if not f16:
        rc = lib.dsp_hifigan_post_f32(_lib.ptr(xd), _lib.ptr(w), bias, _lib.ptr(wav), B, T, C, w.shape[0], slope, _lib.ptr(lens), len_mul, st)
    elif lens is None:
        rc = lib.dsp_hifigan_post(_lib.ptr(xd), _lib.ptr(w), bias, _lib.ptr(wav), B, T, C, w.shape[0], slope, st)
    else:
        rc = lib.dsp_hifigan_post_lens(_lib.ptr(xd), _lib.ptr(w), bias, _lib.ptr(wav), B, T, C, w.shape[0], slope, _lib.ptr(lens), len_mul, st)
    _lib.check(rc, "dsp_hifigan_post*")
    return wav


def _check_post(wav, x, w, bias, slope, lens, len_mul, worst, case):
    """tanh is 1-Lipschitz: the fp32-path tolerance on the sum before it, plus one fp32 ulp of the result."""
    ll = None if lens is None else lens.tolist()
    s64, A = ref_post(_d(x), _d(w), bias, slope, ll, len_mul, pre_tanh=True)
    s32, _ = ref_post(x, w, bias, slope, ll, len_mul, pre_tanh=True)
    ref = ref_post(_d(x), _d(w), bias, slope, ll, len_mul)
    live = A > 0
    e32 = float(((s32.double() - s64).abs() / A.clamp_min(1e-300))[live].max()) if live.any() else 0.0
    tol = SPLIT + 3 * max(e32, FLOOR)
    err = (wav.double() - ref).abs()
    allow = tol * A + 2.0 ** -23 * ref.abs()
    if live.any():
        worst.add(float((err / A.clamp_min(1e-300))[live].max()), e32, tol, case)
    assert not (err > allow).any(), (case, float((err / allow.clamp_min(1e-300)).max()), e32)
    B, T = wav.shape
    for b, n in enumerate(valid_lens(B, T, ll, len_mul)):
        assert (wav[b, n:] == 0).all(), (case, "non-zero past the valid length", b)


@pytest.mark.parametrize("f16", [False, True])
def test_post(f16):
    """dsp_hifigan_post_f32 (256-step tiles with a K - 1 halo) / dsp_hifigan_post[_lens]: C = 32, K = 7."""
    worst = Worst(f"post {'fp16' if f16 else 'fp32'}")
    C, K = 32, 7
    for n, T in enumerate((1, 255, 256, 257, 1000)):
        torch.manual_seed(8000 + n)
        B = (1, 3)[n % 2]
        x = _q(_rand(B, T, C, s=1.5), f16); w = _rand(K, C, s=1.0 / (C * K) ** 0.5); bias = 0.05 * (n - 2)
        _check_post(_post(x, w, bias, 0.01, f16), x, w, bias, 0.01, None, 1, worst, f"post T={T} B={B}")
    for len_mul in (1, 8):
        T0 = 66
        T = T0 * len_mul
        lens = torch.tensor([T0, T0 - 1, 1, 0], device=DEV, dtype=torch.int32)
        torch.manual_seed(8100 + len_mul)
        x = _q(_rand(4, T, C, s=1.5), f16); w = _rand(K, C, s=1.0 / (C * K) ** 0.5)
        wav = _post(x, w, -0.1, 0.01, f16, lens, len_mul)
        _check_post(wav, x, w, -0.1, 0.01, lens, len_mul, worst, f"post lens len_mul={len_mul}")
        for b, m in enumerate(valid_lens(4, T, lens.tolist(), len_mul)):
            if m:
                assert torch.equal(_post(x[b:b + 1, :m].contiguous(), w, -0.1, 0.01, f16)[0], wav[b, :m]), (b, m)
    worst.report()


@pytest.mark.parametrize("B,T,C,Cpad", [(3, 37, 80, 96), (1, 1, 80, 96), (2, 300, 80, 128), (2, 5, 32, 32)])
def test_pad_and_pack_input_are_exact(B, T, C, Cpad):
    from daspeech_amd import _lib
    lib = _lib.load()
    torch.manual_seed(B * T)
    x = _rand(B, T, C, s=3.0)
    want = torch.nn.functional.pad(x, (0, Cpad - C))
    o32 = torch.full((B, T, Cpad), 777.0, device=DEV)
    _lib.check(lib.dsp_hifigan_pad_input_f32(_lib.ptr(x), _lib.ptr(o32), B, T, C, Cpad, _lib.current_stream_handle()), "pad_input_f32")
    assert torch.equal(o32, want)
    o16 = torch.full((B, T, Cpad), 777.0, device=DEV, dtype=torch.float16)
    _lib.check(lib.dsp_hifigan_pack_input(_lib.ptr(x), _lib.ptr(o16), B, T, C, Cpad, _lib.current_stream_handle()), "pack_input")
    assert torch.equal(o16, want.half())


# ---------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("f16", [False, True])
def test_refusals_return_einval_and_leave_out_untouched(f16):
    """Host-side argument checks: each returns DSP_EINVAL with a message before anything is launched."""
    ops = _ops()
    dt = torch.float16 if f16 else torch.float32

    def refused(what, x, w, out, shifts, **kw):
        before = out.clone()
        rc = ops.launch_layer(x, w, None, None, out, shifts, 0.1, 1.0, check=False, **kw)
        msg = _last_error()
        torch.cuda.synchronize()
        assert rc == EINVAL and msg, (what, rc, msg)
        assert torch.equal(out, before), what
        with pytest.raises(Exception):
            ops.launch_layer(x, w, None, None, out, shifts, 0.1, 1.0, **kw)
        return msg

    T = 8
    x512 = torch.zeros(1, T, 512, device=DEV, dtype=dt)
    w512 = _pack(torch.zeros(11, 512, 512, device=DEV), f16)
    assert "LDS" in refused("CI=512 with halo 50", x512, w512, torch.full((1, T, 512), 5.0, device=DEV, dtype=dt), conv_shifts(11, 5))
    x32 = torch.zeros(1, T, 32, device=DEV, dtype=dt)
    refused("Cout % 4 != 0", x32, _pack(torch.zeros(3, 6, 32, device=DEV), f16), torch.full((1, T, 6), 5.0, device=DEV, dtype=dt), conv_shifts(3, 1))
    if f16:             # 16-byte (8-half) output chunks: Cout % 8 == 4 would spill into the next row
        refused("fp16 Cout % 8 != 0", x32, _pack(torch.zeros(3, 12, 32, device=DEV), f16), torch.full((1, T, 12), 5.0, device=DEV, dtype=dt), conv_shifts(3, 1))
    refused("M != up_u * Cout", x32, _pack(torch.zeros(2, 64, 32, device=DEV), f16), torch.full((1, 2 * T, 16), 5.0, device=DEV, dtype=dt), [0, -1],
            out_mode=OUT_UPSAMPLE, up_u=2, up_pad=1, M=64)
    lens = torch.tensor([4], device=DEV, dtype=torch.int32)
    w32 = _pack(torch.zeros(3, 32, 32, device=DEV), f16)
    refused("lens with T0 = 0", x32, w32, torch.full((1, T, 32), 5.0, device=DEV, dtype=dt), conv_shifts(3, 1), lens=lens, T0=0)
    xu = torch.full((1, T, 32), 5.0, device=DEV, dtype=dt)
    refused("unit with x == out", xu, w32, xu, conv_shifts(3, 1), w2=w32)


# ---------------------------------------------------------------------------------------------------------------- long rows
def test_long_rows_f32():
    """C = 32, T = 329 frames x 256 (the benchmark's last stage), B = 2: one fused unit and one conv."""
    worst = Worst("long rows fp32 C=32 T=84224")
    T = 329 * 256
    _unit_case(9000, False, 2, T, 32, 11, 5, 1, worst)
    _conv_case(9001, False, 2, T, 32, 32, conv_shifts(7, 3), 0.1, True, True, OUT_STORE, 1.0, worst)
    worst.report()
