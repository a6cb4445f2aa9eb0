"""Float64 restatements of the three launches that carry the eval-mode acoustic stage, the seeded inputs and case tables their tests share,
restatements of the dispatch arithmetic the cases must reach, and CPU emulations of the kernels' arithmetic with switchable defects.

    dsp_ffn_split          csrc/ffn_split.hip        out = res + alpha * (W2 . act(W1 . LN(x) + b1) + b2)
                                                     (fairseq/modules/conformer_layer.py:140-146 FeedForwardModule, called as
                                                     x + 0.5 * ffn(x) by ConformerEncoderLayer.forward :254-281)
    dsp_linear_ln_split    csrc/conv1d_split.hip     act(W . LN(x) + b), the LayerNorm-staged instance <256,256,64,8,1>
    dsp_attention_split    csrc/attention_split.hip  softmax(q k^T * scale + key padding) v per head
                                                     (fairseq/modules/multihead_attention.py, eval mode)
    dsp_relpos_attention   csrc/attention_split.hip  score(i, j) = (q_i + u) . k_j + (q_i + v) . pos[T-1 - i + j]
                                                     (fairseq/modules/espnet_multihead_attention.py:172-254)

tests/test_block_ref.py (CPU) pins each reference to an independent torch formulation, proves that every row of the case tables reaches
the regime it names, and shows that the bound of the GPU test holds the unmutated emulation on every case input and rejects every
mutant on the cases named for it.  tests/test_gpu_block_regimes.py runs the kernels on the same arrays.

Everything here is CPU torch / numpy.  Inputs come from numpy.random.default_rng(seed), so the CPU and GPU tests see the same arrays.

Not covered: a sweep over input scales.  The split x = hi + lo * 2^-11 keeps 22 bits only while lo is a normal fp16 number; for tensors
whose largest entries are near 1e-6 lo falls into fp16's subnormal range and the relative accuracy degrades.  Inputs beyond the fp16
range (65504) are outside the kernels' contract (include/daspeech_decode.h)."""
import functools
import math

import numpy as np
import torch

from tests.util_glue_ref import fp32_bound, rel_err

NEG_INF = float("-inf")
F32, F64 = torch.float32, torch.float64
C_FF = 256                  # the one instance of ffn_split / the LayerNorm-staged linear
FFN_CAP = 2e-6              # tests/test_gpu_ffn_fused.py::test_ffn_fused_matches_fp64_and_the_two_gemm_path
LINEAR_LN_CAP = 3e-6        # tests/test_gpu_ffn_fused.py::test_linear_with_staged_layer_norm_matches_layer_norm_then_linear
ATT_CAP = 3e-6              # tests/test_gpu_attention.py::test_attention_split_matches_fp64
PAD_JUNK = 3.0e4            # what masked key / value rows hold: inside the fp16 range, far above every live entry


def t_(a, dtype):
    return None if a is None else torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).to(dtype)


def _act(v, act):
    """dsp_conv1d_split's activation codes: 0 none, 1 ReLU, 2 SiLU, 3 GELU (erf form)"""
    if act == 1:
        return torch.clamp_min(v, 0.0)
    if act == 2:
        return v / (1.0 + torch.exp(-v))
    if act == 3:
        return 0.5 * v * (1.0 + torch.erf(v * (1.0 / math.sqrt(2.0))))
    return v


def _layer_norm(x, w, b, eps):
    """biased variance, eps inside the square root (torch.nn.LayerNorm's definition), in x's dtype"""
    mu = x.mean(-1, keepdim=True)
    d = x - mu
    return d / torch.sqrt((d * d).mean(-1, keepdim=True) + eps) * w + b


# ---------------------------------------------------------------- float64 references (dtype=torch.float32: the fp32 comparator)

def ffn_ref(x, ln_w, ln_b, eps, w1, b1, w2, b2, act, res, alpha, post_w=None, post_b=None, post_eps=1e-5, dtype=F64):
    """conformer_layer.py:140-146 (layer_norm - w_1 - activation - w_2) as :254-281 calls it: out = res + alpha * ffn(x).
    x [..., C], w1 [H, C], w2 [C, H]; ln_w / b1 / b2 / res / post_w may be None.  -> (out, LayerNorm(out) or None)"""
    xx = t_(x, dtype)
    if ln_w is not None:
        xx = _layer_norm(xx, t_(ln_w, dtype), t_(ln_b, dtype), eps)
    h = xx @ t_(w1, dtype).T
    if b1 is not None:
        h = h + t_(b1, dtype)
    y = _act(h, act) @ t_(w2, dtype).T
    if b2 is not None:
        y = y + t_(b2, dtype)
    out = alpha * y if res is None else t_(res, dtype) + alpha * y
    out_ln = None if post_w is None else _layer_norm(out, t_(post_w, dtype), t_(post_b, dtype), post_eps)
    return out, out_ln


def linear_ln_ref(x, ln_w, ln_b, eps, w, b, act, dtype=F64):
    """act(W . LayerNorm(x) + b): what dsp_linear_ln_split computes without a residual"""
    xx = _layer_norm(t_(x, dtype), t_(ln_w, dtype), t_(ln_b, dtype), eps)
    return _act(xx @ t_(w, dtype).T + t_(b, dtype), act)


def attention_ref(q, k, v, key_mask, heads, scale, dtype=F64):
    """multihead_attention.py, eval mode: softmax_j(scale * q_i . k_j; key_mask[b, j] -> -inf) v_j per head.  key_mask [B, M] bool, any
    pattern, or None.  -> (out [B, N, C], scaled scores [B, H, N, M] with -inf at masked keys).  A sample without a live key: NaN rows."""
    q, k, v = t_(q, dtype), t_(k, dtype), t_(v, dtype)
    B, N, C = q.shape
    M, dk = k.shape[1], C // heads
    out = torch.empty(B, N, C, dtype=dtype)
    scores = torch.empty(B, heads, N, M, dtype=dtype)
    for b in range(B):
        for h in range(heads):
            sl = slice(h * dk, (h + 1) * dk)
            s = (q[b, :, sl] @ k[b, :, sl].T) * scale
            if key_mask is not None:
                s = torch.where(t_(key_mask[b], torch.bool)[None, :], torch.full_like(s, NEG_INF), s)
            scores[b, h] = s
            e = torch.exp(s - s.max(-1, keepdim=True).values)            # an all -inf row: -inf - -inf = NaN, as torch's soft-max
            out[b, :, sl] = (e / e.sum(-1, keepdim=True)) @ v[b, :, sl]
    return out, scores


def relpos_attention_ref(q, k, v, pos, bias_u, bias_v, pad_mask, heads, dtype=F64):
    """espnet_multihead_attention.py:172-254 with rel_shift written as the gather it amounts to:
    score(i, j) = ((q_i + u) . k_j + (q_i + v) . pos[T-1 - i + j]) / sqrt(dk).  pos [2T-1, C].  -> (out, scaled scores)"""
    q, k, v, pos = t_(q, dtype), t_(k, dtype), t_(v, dtype), t_(pos, dtype)
    bu, bv = t_(bias_u, dtype), t_(bias_v, dtype)
    B, T, C = q.shape
    dk = C // heads
    idx = (T - 1) - torch.arange(T)[:, None] + torch.arange(T)[None, :]                 # [i, j] -> row of pos
    out = torch.empty(B, T, C, dtype=dtype)
    scores = torch.empty(B, heads, T, T, dtype=dtype)
    for b in range(B):
        for h in range(heads):
            sl = slice(h * dk, (h + 1) * dk)
            ac = (q[b, :, sl] + bu[h]) @ k[b, :, sl].T
            bd = torch.gather((q[b, :, sl] + bv[h]) @ pos[:, sl].T, 1, idx)
            s = (ac + bd) / math.sqrt(dk)
            if pad_mask is not None:
                s = torch.where(t_(pad_mask[b], torch.bool)[None, :], torch.full_like(s, NEG_INF), s)
            scores[b, h] = s
            e = torch.exp(s - s.max(-1, keepdim=True).values)
            out[b, :, sl] = (e / e.sum(-1, keepdim=True)) @ v[b, :, sl]
    return out, scores


# ---------------------------------------------------------------- the bound

def att_cap(scores):
    """max(3e-6, 8 S 2^-24), S the largest finite |scaled score|: rounding a score of size S to fp32 moves its weight by S 2^-24
    relatively, in torch's fp32 path and in the kernel alike"""
    s = np.asarray(scores, np.float64)
    fin = np.isfinite(s)
    S = float(np.abs(s[fin]).max()) if fin.any() else 0.0
    return max(ATT_CAP, 8.0 * S * 2.0 ** -24)


def judge(got, ref, ref32, cap):
    """-> (err, err32, bound, ok): util_glue_ref.rel_err of the result and of the fp32 comparator against the float64 reference, and
    err <= util_glue_ref.fp32_bound(err32, cap).  A NaN anywhere in `got` fails."""
    got, ref, ref32 = (np.asarray(a, np.float64) for a in (got, ref, ref32))
    err, err32 = rel_err(got, ref), rel_err(ref32, ref)
    bound = fp32_bound(err32, cap)
    return err, err32, bound, bool(err <= bound)


def judge_slices(got, ref, ref32, cap, slices):
    """judge() on the whole tensor and on every slice of `slices` ((name, index) pairs), each against its own slice's scale.
    -> [(name, err, err32, bound, ok)]"""
    rows = [("all",) + judge(got, ref, ref32, cap)]
    for name, ix in slices:
        rows.append((name,) + judge(np.asarray(got)[ix], np.asarray(ref)[ix], np.asarray(ref32)[ix], cap))
    return rows


# ---------------------------------------------------------------- dispatch arithmetic, restated (csrc/ffn_split.hip, csrc/attention_split.hip)

def ff_groups(B, T, H):
    """ff_groups(): hidden-channel groups G in {1, 2, 4, 8}"""
    tiles = ((T + 63) // 64) * B
    G = 1
    while tiles * G < 224 and G < 8 and (H // 256) % (2 * G) == 0:
        G *= 2
    return G


def ff_regime(B, T, H):
    """-> (G, chunks per group)"""
    G = ff_groups(B, T, H)
    return G, (H // 256) // G


def ff_reduce_trips(B, T):
    """trips of ffn_reduce_kernel's grid-stride loop (256 threads x float4, at most 2048 workgroups)"""
    n4 = B * T * C_FF // 4
    grid = min((n4 + 255) // 256, 2048)
    return -(-n4 // (grid * 256))


def ff_reduce_ln_trips(B, T):
    """trips of ffn_reduce_ln_kernel's loop (4 rows per workgroup, at most 4096 workgroups)"""
    rows = B * T
    grid = min((rows + 3) // 4, 4096)
    return -(-rows // (grid * 4))


def ff_workspace_bytes(B, T, H):
    return ff_groups(B, T, H) * B * T * C_FF * 4


def at_ntq(N):
    return (N + 127) // 128


def at_nt(mask_row, M):
    """key tiles of one sample: up to the last key that is not padding; 1 when every key is masked"""
    if mask_row is None:
        return (M - 1 + 32) // 32
    live = np.nonzero(~np.asarray(mask_row, bool))[0]
    return 1 if live.size == 0 else (int(live.max()) + 32) // 32


def at_nwork(B, N, H):
    return at_ntq(N) * H * B


def at_remap(B, N, H):
    """the XCD remap of work items is on when the grid is a multiple of 8"""
    return at_nwork(B, N, H) % 8 == 0


def at_leading_masked_tiles(mask_row):
    """number of wholly masked key tiles before the first live key (the m_new == -inf branch on a live sample)"""
    if mask_row is None:
        return 0
    live = np.nonzero(~np.asarray(mask_row, bool))[0]
    return 0 if live.size == 0 else int(live.min()) // 32


def q_rows_computed(lim, N):
    """rows written by live waves under a query limit: every 32-query group that starts below the limit"""
    lim = max(0, min(lim, N))
    return min(N, -(-lim // 32) * 32)


# ---------------------------------------------------------------- FFN cases and inputs

# tag: B, T, H, (G, nch) it names, act, ln (None | "plain" | "mean300": the first 64-row tile has mean 300, spread 1 | "const": one exactly
# constant row beside ordinary ones), b1, b2 (False: NULL), res (False: NULL, judged as alpha * branch), x layout ("c" | "ld260" |
# "slice768"), ldr, ldo, post ("" | "out": post-LayerNorm beside out | "only": out = NULL as well).  alpha = 0.5 throughout.
FFN_CASES = {
    "g1-n2-T3":      (224, 3, 512, (1, 2), 0, None, False, True, True, "c", 256, 256, ""),
    "g1-n8-T2":      (224, 2, 2048, (1, 8), 2, "plain", True, False, True, "ld260", 256, 256, ""),
    "g1-n2-trips":   (257, 64, 512, (1, 2), 1, "mean300", True, True, True, "c", 256, 256, ""),
    "g1-n2-trips-p": (257, 64, 512, (1, 2), 3, "const", True, True, True, "c", 256, 256, "out"),
    "g2-n1-T65":     (2, 65, 512, (2, 1), 3, "plain", False, False, True, "c", 264, 272, "out"),
    "g2-n3-T63":     (1, 63, 1536, (2, 3), 2, "mean300", True, True, True, "slice768", 256, 256, "only"),
    "g2-n4-T1":      (112, 1, 2048, (2, 4), 1, None, True, True, False, "c", 256, 256, ""),
    "g2-n2-T2":      (112, 2, 1024, (2, 2), 0, "const", True, True, True, "c", 256, 256, ""),
    "g4-n2-T64":     (56, 64, 2048, (4, 2), 3, "plain", True, True, True, "c", 256, 256, ""),
    "g4-n1-T1":      (1, 1, 1024, (4, 1), 2, "plain", False, True, True, "c", 256, 256, "out"),
    "g4-n3-T65":     (2, 65, 3072, (4, 3), 1, "plain", True, True, True, "ld260", 256, 272, ""),
    "g8-n1-T1":      (1, 1, 2048, (8, 1), 0, None, True, False, False, "c", 256, 256, "only"),
    "g8-n2-T129":    (3, 129, 4096, (8, 2), 3, "const", True, True, True, "c", 264, 256, "out"),
}
FFN_FIELDS = ("B", "T", "H", "regime", "act", "ln", "b1", "b2", "res", "xlay", "ldr", "ldo", "post")
FFN_ALPHA, LN_EPS, RES_SCALE = 0.5, 1e-5, 0.2
CONST_ROW_VALUE = 3.0        # every partial sum of 256 copies is exact in fp32: the row normalises to exactly the LayerNorm bias

# the cases on which each defect of emulate_ffn_split must show
FFN_MUTANT_CASES = {
    "lo_w1x": ("g2-n1-T65", "g4-n3-T65"),
    "lo_w2h": ("g2-n1-T65", "g4-n3-T65"),
    "drop_chunk": ("g2-n3-T63", "g8-n2-T129"),
    "w2_half": ("g2-n3-T63", "g4-n1-T1"),
    "ln_onepass": ("g1-n2-trips", "g2-n3-T63"),
}


def ffn_case(tag):
    return dict(zip(FFN_FIELDS, FFN_CASES[tag]), tag=tag)


def mean300_rows(rng, n, C):
    return (300.0 + np.round(rng.standard_normal((n, C)) * 128.0) / 128.0).astype(np.float32)


def planted_rows(rng, rows, C, ln):
    """x [rows, C] float32: ordinary rows 0.2 + 1.7 normal; "mean300": rows 0..63 are 300 + normal; "const": row min(5, rows - 1) holds
    CONST_ROW_VALUE in every channel.

    The mean-300 rows lie on a grid of 2^-7.  Every partial sum of such a row is then exact in fp32 in any order (below 2^17 in steps of
    2^-7: 24 bits), so the row mean is exact and what is left is the question the rows are planted for: does the variance survive a mean
    300 times the spread (a one-pass E[x^2] - mean^2 does not: emulate_ffn_split's ln_onepass).  Off the grid the fp32 rounding of the
    row sum (ulp 2^-7 at 76800) shifts the mean by ~1e-5 of the spread in ANY fp32 LayerNorm: measured on the CPU at (257, 64, 512),
    torch's fp32 evaluation sits at err32 = 6.9e-6 (9.8e-6 on the planted sample) and the emulation at the same figure, ratio 1.00 —
    above the 2e-6 cap by the conditioning of the input, with no difference between implementations left to test."""
    x = (0.2 + 1.7 * rng.standard_normal((rows, C))).astype(np.float32)
    if ln == "mean300":
        n = min(64, rows)
        x[:n] = mean300_rows(rng, n, C)
    if ln == "const":
        x[min(5, rows - 1)] = CONST_ROW_VALUE
    return x


@functools.lru_cache(maxsize=None)
def ffn_inputs(tag):
    """the arrays of one FFN case (float32 numpy; None where the case passes NULL): weights at the 1 / sqrt(fan_in) scale of
    tests/test_gpu_split_addressing.py, |res| no larger than alpha * branch (tests/test_block_ref.py checks it per case)"""
    c = ffn_case(tag)
    B, T, H = c["B"], c["T"], c["H"]
    rng = np.random.default_rng(7000 + sorted(FFN_CASES).index(tag))
    f = lambda a: a.astype(np.float32)                                   # noqa: E731
    d = dict(c)
    d["x"] = planted_rows(rng, B * T, C_FF, c["ln"]).reshape(B, T, C_FF)
    d["ln_w"] = f(1.0 + 0.2 * rng.standard_normal(C_FF)) if c["ln"] else None
    d["ln_b"] = f(0.2 * rng.standard_normal(C_FF)) if c["ln"] else None
    d["w1"] = f(rng.standard_normal((H, C_FF)) / math.sqrt(C_FF))
    d["w2"] = f(rng.standard_normal((C_FF, H)) / math.sqrt(H))
    d["b1"] = f(0.1 * rng.standard_normal(H)) if c["b1"] else None
    d["b2"] = f(0.1 * rng.standard_normal(C_FF)) if c["b2"] else None
    d["res"] = f(RES_SCALE * rng.standard_normal((B, T, C_FF)))          # used only when the case has a residual
    d["post_w"] = f(1.0 + 0.2 * rng.standard_normal(C_FF)) if c["post"] else None
    d["post_b"] = f(0.2 * rng.standard_normal(C_FF)) if c["post"] else None
    return d


def ffn_twins(tag):
    """the residual settings a case is judged at: as the table says, and always without a residual, so a large residual cannot hide the
    branch"""
    return (True, False) if FFN_CASES[tag][FFN_FIELDS.index("res")] else (False,)


@functools.lru_cache(maxsize=None)
def ffn_refs(tag, with_res):
    """((out64, out_ln64), (out32, out_ln32)) as float64 / float32 numpy, computed once per case"""
    d = ffn_inputs(tag)
    args = (d["x"], d["ln_w"], d["ln_b"], LN_EPS, d["w1"], d["b1"], d["w2"], d["b2"], d["act"], d["res"] if with_res else None, FFN_ALPHA,
            d["post_w"], d["post_b"], LN_EPS)
    n = lambda pair: tuple(None if a is None else a.numpy() for a in pair)          # noqa: E731
    return n(ffn_ref(*args, dtype=F64)), n(ffn_ref(*args, dtype=F32))


# dsp_linear_ln_split (instance cs256ln): (T, M, ln planting, ragged).  B = 2; ragged: lens = [T, 9], slack 5
LINEAR_LN_CASES = [(63, 128, "mean300", False), (65, 272, "const", True), (131, 768, "mean300", True), (131, 272, "const", False)]
LINEAR_LN_TILE = 64


@functools.lru_cache(maxsize=None)
def linear_ln_inputs(i):
    T, M, ln, ragged = LINEAR_LN_CASES[i]
    rng = np.random.default_rng(7100 + i)
    f = lambda a: a.astype(np.float32)                                   # noqa: E731
    d = dict(T=T, M=M, B=2, ragged=ragged, act=(0, 3, 2, 1)[i])
    d["x"] = planted_rows(rng, 2 * T, C_FF, ln).reshape(2, T, C_FF)
    if ln == "mean300":
        d["x"][1, :min(T, 64)] = mean300_rows(rng, min(T, 64), C_FF)
    d["ln_w"], d["ln_b"] = f(1.0 + 0.3 * rng.standard_normal(C_FF)), f(0.3 * rng.standard_normal(C_FF))
    d["w"], d["b"] = f(rng.standard_normal((M, C_FF)) / math.sqrt(C_FF)), f(0.1 * rng.standard_normal(M))
    d["lens"], d["slack"] = ([T, 9], 5) if ragged else (None, 0)
    d["rows"] = [T, T] if not ragged else [min(T, -(-(n + 5) // LINEAR_LN_TILE) * LINEAR_LN_TILE) for n in d["lens"]]
    return d


# ---------------------------------------------------------------- attention cases and inputs

# tag: B, N, M, H, dk, mask, score shape, layout.
#   masks (per sample, see key_masks): none | suffix | lead40 | lead64 | holes | lone | dead
#   score shapes (see attention_inputs): flat | peaked | rising | falling | hot
#   layouts: c (contiguous) | kv2c (k, v as slices of [B,M,2C]) | qkv3c (all three slices of [B,N,3C]; N = M) | odd (ldq != ldk != ldv)
ATT_CASES = {
    "N1-M1":         (2, 1, 1, 4, 64, "none", "flat", "c"),
    "N31-M31-w9":    (3, 31, 31, 3, 64, "suffix", "flat", "qkv3c"),
    "N33-M32":       (2, 33, 32, 4, 64, "none", "peaked", "c"),
    "N33-M33-3c":    (2, 33, 33, 4, 64, "holes", "flat", "qkv3c"),
    "N127-M33-lone": (4, 127, 33, 2, 64, "lone", "flat", "c"),
    "N129-M64-rise": (2, 129, 64, 4, 64, "suffix", "rising", "kv2c"),
    "N257-M65-lead": (1, 257, 65, 3, 64, "lead40", "peaked", "c"),
    "N257-M97-lead": (2, 257, 97, 4, 64, "lead64", "rising", "c"),
    "N257-M161-w15": (1, 257, 161, 5, 64, "holes", "falling", "c"),
    "N33-M161-hot":  (3, 33, 161, 5, 64, "suffix", "hot", "odd"),
    "N65-M97-hot":   (2, 65, 97, 2, 64, "suffix", "hot", "c"),
    "N65-M97-flat":  (2, 65, 97, 2, 64, "suffix", "flat", "c"),
    "N33-M97-rise":  (2, 33, 97, 4, 64, "none", "rising", "c"),
    "N31-M161-fall": (2, 31, 161, 4, 64, "none", "falling", "c"),
    "N65-M161-dead": (3, 65, 161, 1, 64, "dead", "rising", "c"),
    "d128-holes":    (2, 127, 161, 2, 128, "holes", "rising", "kv2c"),
    "d128-dead":     (4, 33, 65, 2, 128, "dead", "flat", "c"),
    "d128-lead":     (2, 129, 97, 2, 128, "lead40", "falling", "c"),
    "d128-lone":     (2, 1, 65, 2, 128, "lone", "peaked", "odd"),
}
ATT_FIELDS = ("B", "N", "M", "H", "dk", "mask", "scores", "layout")

ATT_MUTANT_CASES = {
    "lo_kq": ("N65-M97-flat", "N65-M97-hot", "d128-dead"),
    "lo_vp": ("N65-M97-flat", "N33-M32", "d128-dead"),
    "no_rescale": ("N129-M64-rise", "N33-M97-rise", "d128-holes"),
    "neg_inf_max": ("N257-M65-lead", "N257-M97-lead", "d128-lead"),
    "nt_early": ("N127-M33-lone", "d128-lone"),
}
# Counting key tiles from M instead of from the last live key is NOT a defect of the values: the extra tiles hold masked keys only, whose
# weights are exp(-inf) = 0 exactly (the kernel's header says so: "exact: their weights are 0").  The CPU test shows that on these cases
# the mutant's output has the bits of the unmutated emulation, junk-filled padding rows included.
ATT_EQUIVALENT_MUTANT_CASES = {"nt_from_m": ("N33-M161-hot", "N129-M64-rise", "N65-M97-flat")}


def att_case(tag):
    return dict(zip(ATT_FIELDS, ATT_CASES[tag]), tag=tag)


def key_masks(kind, B, M):
    """[B, M] bool (True: padding) or None.
    suffix  sample 0 full, then shorter and shorter (one sample: M - 11 keys, at least 1)
    lead40 / lead64  sample 0: the first 40 / 64 keys masked (one / two wholly masked first tiles); the others a suffix mask
    holes   every third key masked and a 33-key gap from key 20 (across a tile edge); sample 1 also loses its last 3 keys
    lone    even samples: only key M-1 live (M-1 = 32 t: a tile's first slot); sample 1: only key 0 live; sample 3: only key 31 (a tile's
            last slot)
    dead    sample 1 wholly masked, the others a suffix mask"""
    if kind == "none":
        return None
    j = np.arange(M)
    m = np.zeros((B, M), bool)
    suffix = [M if B > 1 else max(1, M - 11)] + [max(1, (M * (B - b)) // B - 1) for b in range(1, B)]
    if kind in ("suffix", "lead40", "lead64", "dead"):
        for b in range(B):
            m[b] = j >= suffix[b]
    if kind in ("lead40", "lead64"):
        m[0] = j < int(kind[4:])
    if kind == "holes":
        m[:] = (j % 3 == 1) | ((j >= 20) & (j < 53))
        if B > 1:
            m[1, max(1, M - 3):] = True
    if kind == "lone":
        m[:] = True
        m[0::2, M - 1] = False
        m[1::4, 0] = False
        m[3::4, min(31, M - 1)] = False
    if kind == "dead":
        m[1] = True
    return m


def _unit_dirs(rng, H, dk):
    u = rng.standard_normal((H, dk))
    return u / np.linalg.norm(u, axis=1, keepdims=True)


def _set_component(x, u, value):
    """x [..., H, dk]: replace every row's component along u[h] by value (array broadcastable to x[..., 0])"""
    comp = np.einsum("...hd,hd->...h", x, u)
    return x + (np.asarray(value) - comp)[..., None] * u


@functools.lru_cache(maxsize=None)
def attention_inputs(tag, pad="junk"):
    """q [B,N,C], k, v [B,M,C] float32, mask [B,M] bool or None.  Score shapes (s = q . k / sqrt(dk), per head a unit direction u):
    flat     q, k = 1.5 normal: |s| up to ~ 11
    peaked   q x 6
    rising   q . u = 3 exactly, k_j . u = 2 sqrt(dk) (tile(j) + 1), small noise: every query's maximum rises by ~ 6 on every key tile
    falling  the same with -2 sqrt(dk) (tile(j) + 1): the maximum of every query is in its first live tile, no later tile rescales
    hot      q . u = k . u = sqrt(62 sqrt(dk)): s = 62 + a flat spread, |s| up to ~ 72
    Masked key / value rows hold pad: "junk" +-3e4, "zero" zeros, "keep" ordinary values."""
    c = att_case(tag)
    B, N, M, H, dk = c["B"], c["N"], c["M"], c["H"], c["dk"]
    rng = np.random.default_rng(8000 + sorted(ATT_CASES).index(tag))
    u = _unit_dirs(rng, H, dk)
    qn, kn = rng.standard_normal((B, N, H, dk)), rng.standard_normal((B, M, H, dk))
    tile = (np.arange(M) // 32 + 1).astype(np.float64)[None, :, None]
    kind = c["scores"]
    if kind == "flat":
        q, k = 1.5 * qn, 1.5 * kn
    elif kind == "peaked":
        q, k = 9.0 * qn, 1.5 * kn
    elif kind in ("rising", "falling"):
        sign = 1.0 if kind == "rising" else -1.0
        q = _set_component(0.7 * qn, u, 3.0)
        k = _set_component(0.7 * kn, u, sign * 2.0 * math.sqrt(dk) * tile)
    else:
        g = math.sqrt(62.0 * math.sqrt(dk))
        q, k = _set_component(1.5 * qn, u, g), _set_component(1.5 * kn, u, g)
    v = 2.0 * rng.standard_normal((B, M, H, dk)) + 0.3
    sgn = np.where(rng.random((B, M, H * dk)) < 0.5, -1.0, 1.0)
    q, k, v = (a.reshape(a.shape[0], a.shape[1], H * dk).astype(np.float32) for a in (q, k, v))
    mask = key_masks(c["mask"], B, M)
    if mask is not None and pad != "keep":
        fill = (PAD_JUNK * sgn if pad == "junk" else 0.0 * sgn).astype(np.float32)
        k = np.where(mask[:, :, None], fill, k)
        v = np.where(mask[:, :, None], -fill if pad == "junk" else fill, v)
    return dict(c, q=q, k=k, v=v, key_mask=mask, scale=float(dk) ** -0.5)


@functools.lru_cache(maxsize=None)
def attention_refs(tag):
    """(out64, scores64, out32) as numpy, computed once per case (junk-filled padding rows: they cannot reach a valid query)"""
    d = attention_inputs(tag)
    o64, s64 = attention_ref(d["q"], d["k"], d["v"], d["key_mask"], d["H"], d["scale"], dtype=F64)
    o32, _ = attention_ref(d["q"], d["k"], d["v"], d["key_mask"], d["H"], d["scale"], dtype=F32)
    return o64.numpy(), s64.numpy(), o32.numpy()


def live_samples(mask, B):
    return [b for b in range(B) if mask is None or not mask[b].all()]


def head_slices(B, H, dk, samples):
    return [(f"b{b}h{h}", (b, slice(None), slice(h * dk, (h + 1) * dk))) for b in samples for h in range(H)]


def tile_maxima(scores_bh, nt):
    """[N, nt] maxima of the scaled scores over each key tile (-inf: no live key in the tile)"""
    N, M = scores_bh.shape
    out = np.full((N, nt), NEG_INF)
    for t in range(nt):
        out[:, t] = scores_bh[:, t * 32:min(M, (t + 1) * 32)].max(1)
    return out


# q_lens / q_slack: one sample per limit
QLENS_SHAPE = dict(B=7, N=129, M=65, H=2, dk=64)
QLENS = (0, 1, 31, 32, 33, 129, 179)
QSLACKS = (0, 5)


@functools.lru_cache(maxsize=None)
def qlens_inputs():
    s = QLENS_SHAPE
    rng = np.random.default_rng(8500)
    C = s["H"] * s["dk"]
    f = lambda a: a.astype(np.float32)                                   # noqa: E731
    return dict(s, q=f(1.5 * rng.standard_normal((s["B"], s["N"], C))), k=f(1.5 * rng.standard_normal((s["B"], s["M"], C))),
                v=f(2.0 * rng.standard_normal((s["B"], s["M"], C)) + 0.3), key_mask=key_masks("suffix", s["B"], s["M"]), scale=0.125)


# relative-position attention (dk = 64): tag: B, T, H, nonzero biases, fused [B,T,3C] layout, suffix mask
REL_CASES = {
    "T1":      (2, 1, 4, False, False, False),
    "T31-w9":  (3, 31, 3, True, True, True),
    "T32":     (2, 32, 4, True, False, True),
    "T33":     (1, 33, 3, False, True, False),
    "T127":    (2, 127, 2, True, False, True),
    "T128":    (4, 128, 2, True, True, True),
    "T129":    (2, 129, 2, False, False, True),
    "T161":    (1, 161, 3, True, True, True),
    "T257":    (2, 257, 4, True, False, True),
    "T257-w9": (1, 257, 3, True, True, False),
}
REL_MUTANT_CASES = {"rel_shift1": ("T33", "T129", "T257-w9"), "lo_kq": ("T127",), "lo_vp": ("T127",)}


@functools.lru_cache(maxsize=None)
def relpos_inputs(tag):
    B, T, H, biased, fused, masked = REL_CASES[tag]
    rng = np.random.default_rng(9000 + sorted(REL_CASES).index(tag))
    C = H * 64
    f = lambda a: a.astype(np.float32)                                   # noqa: E731
    q, k, v = (f(1.2 * rng.standard_normal((B, T, C))) for _ in range(3))
    pos = f(rng.standard_normal((2 * T - 1, C)))
    bu, bv = f(0.5 * rng.standard_normal((H, 64))), f(0.5 * rng.standard_normal((H, 64)))
    if not biased:
        bu, bv = np.zeros_like(bu), np.zeros_like(bv)
    mask = key_masks("suffix", B, T) if masked else None
    if mask is not None:
        sgn = np.where(rng.random((B, T, C)) < 0.5, -1.0, 1.0).astype(np.float32)
        k = np.where(mask[:, :, None], PAD_JUNK * sgn, k)
        v = np.where(mask[:, :, None], -PAD_JUNK * sgn, v)
    return dict(tag=tag, B=B, T=T, H=H, fused=fused, q=q, k=k, v=v, pos=pos, bias_u=bu, bias_v=bv, pad_mask=mask)


@functools.lru_cache(maxsize=None)
def relpos_refs(tag):
    d = relpos_inputs(tag)
    a = (d["q"], d["k"], d["v"], d["pos"], d["bias_u"], d["bias_v"], d["pad_mask"], d["H"])
    o64, s64 = relpos_attention_ref(*a, dtype=F64)
    o32, _ = relpos_attention_ref(*a, dtype=F32)
    return o64.numpy(), s64.numpy(), o32.numpy()


# ---------------------------------------------------------------- emulation of the kernels' arithmetic

def split16(x):
    """x = hi + lo * 2^-11 with hi, lo fp16 (returned widened to fp32): the split of every MFMA operand"""
    hi = x.to(torch.float16).to(F32)
    lo = ((x - hi) * 2048.0).to(torch.float16).to(F32)
    return hi, lo


def split_products(a, b, drop_lo=False):
    """a [m,k] x b [k,n] as the kernels form it: (main, correction) = (ah.bh, ah.bl + al.bh) accumulated in fp32; the caller folds the
    correction with 2^-11.  drop_lo: the defect of a missing pair of correction MFMAs (correction = 0)."""
    ah, al = split16(a)
    bh, bl = split16(b)
    main = ah @ bh
    return main, (torch.zeros_like(main) if drop_lo else ah @ bl + al @ bh)


def _ln32(x, w, b, eps, onepass=False):
    mean = x.sum(-1, keepdim=True) * (1.0 / x.shape[-1])
    d = x - mean
    if onepass:                                                          # the defect: variance as E[x^2] - mean^2
        var = torch.clamp_min((x * x).sum(-1, keepdim=True) * (1.0 / x.shape[-1]) - mean * mean, 0.0)
        return d * (1.0 / torch.sqrt(var + eps)) * w + b
    rstd = 1.0 / torch.sqrt((d * d).sum(-1, keepdim=True) * (1.0 / x.shape[-1]) + eps)
    return d * rstd * w + b


def emulate_ffn_split(x, ln_w, ln_b, eps, w1, b1, w2, b2, act, res, alpha, post_w=None, post_b=None, post_eps=1e-5, G=1, mutant=None):
    """ffn_split_kernel + ffn_reduce(_ln)_kernel in fp32 torch: LayerNorm in fp32, per group g and 256-channel chunk of it
    h = act(W1[chunk] . x + b1) with split operands, h split again, y0 / y1 accumulated over the group's chunks, partial = y0 + y1 2^-11,
    the G partials added in order, then bias, alpha, residual and the post-LayerNorm.
    mutant: lo_w1x | lo_w2h (no correction products in that GEMM) | drop_chunk (the last chunk of the last group is never accumulated) |
    w2_half (W2's 512-slice indexed by chunk >> 1 without the (chunk & 1) half offset: odd chunks read the even chunk's columns) |
    ln_onepass (the staged LayerNorm's variance as E[x^2] - mean^2)"""
    x = t_(x, F32)
    lead = x.shape[:-1]
    xx = x.reshape(-1, C_FF)
    if ln_w is not None:
        xx = _ln32(xx, t_(ln_w, F32), t_(ln_b, F32), eps, onepass=mutant == "ln_onepass")
    w1, w2 = t_(w1, F32), t_(w2, F32)
    H = w1.shape[0]
    nch = (H // 256) // G
    total = None
    for g in range(G):
        y0 = torch.zeros(xx.shape[0], C_FF)
        y1 = torch.zeros_like(y0)
        for c in range(nch):
            ch = g * nch + c
            if mutant == "drop_chunk" and g == G - 1 and c == nch - 1:
                continue
            cs = slice(ch * 256, (ch + 1) * 256)
            h0, h1 = split_products(xx, w1[cs].T, drop_lo=mutant == "lo_w1x")
            h = h0 + h1 * (1.0 / 2048.0)
            if b1 is not None:
                h = h + t_(b1, F32)[cs]
            h = _act(h, act)
            ws = slice((ch & ~1) * 256, ((ch & ~1) + 1) * 256) if mutant == "w2_half" else cs
            a0, a1 = split_products(h, w2[:, ws].T, drop_lo=mutant == "lo_w2h")
            y0, y1 = y0 + a0, y1 + a1
        part = y0 + y1 * (1.0 / 2048.0)
        total = part if total is None else total + part
    if b2 is not None:
        total = total + t_(b2, F32)
    out = alpha * total if res is None else t_(res, F32).reshape(-1, C_FF) + alpha * total
    out_ln = None if post_w is None else _ln32(out, t_(post_w, F32), t_(post_b, F32), post_eps).reshape(*lead, C_FF)
    return out.reshape(*lead, C_FF), out_ln


def emulate_linear_ln_split(x, ln_w, ln_b, eps, w, b, act):
    """the LayerNorm-staged split GEMM: fp32 LayerNorm, split operands, bias, activation"""
    xx = _ln32(t_(x, F32), t_(ln_w, F32), t_(ln_b, F32), eps)
    m, c = split_products(xx.reshape(-1, C_FF), t_(w, F32).T)
    return _act(m + c * (1.0 / 2048.0) + t_(b, F32), act).reshape(*x.shape[:-1], w.shape[0])


def emulate_attention_split(q, k, v, key_mask, heads, scale, pos=None, bias_u=None, bias_v=None, mutant=None):
    """attention_split_kernel in fp32 torch: key tiles of 32 up to the last live key, S = K . Q with split operands, the running maximum
    and sum, the accumulator rescale, P = exp(s - m) split into fp16 pairs, O += V . P, out = (O0 + O1 2^-11) / l.  pos / bias_u /
    bias_v: the relative-position variant ((q + u) . k + (q + v) . pos[T-1 - i + j], summed before the scale).
    mutant: lo_kq | lo_vp (no correction products) | no_rescale (accumulators keep their old maximum) | neg_inf_max (an all-masked
    prefix's -inf maximum used as a maximum: no m_use = 0) | nt_from_m (tiles counted from M) | nt_early (tiles = ceil(last / 32): one
    short when the last live key is a tile's first slot) | rel_shift1 (pos[T - i + j])"""
    q, k, v = t_(q, F32), t_(k, F32), t_(v, F32)
    B, N, C = q.shape
    M, dk = k.shape[1], C // heads
    rel = pos is not None
    out = torch.empty(B, N, C)
    for b in range(B):
        mk = torch.zeros(M, dtype=torch.bool) if key_mask is None else t_(key_mask[b], torch.bool)
        live = torch.nonzero(~mk).flatten()
        last = int(live.max()) if live.numel() else -1
        nt = 1 if last < 0 else (last + 32) // 32
        if mutant == "nt_from_m" and last >= 0:
            nt = (M + 31) // 32
        if mutant == "nt_early" and last >= 0:
            nt = max(1, (last + 31) // 32)
        for h in range(heads):
            sl = slice(h * dk, (h + 1) * dk)
            Q = q[b, :, sl]
            Qc = Q + t_(bias_u, F32)[h] if rel else Q
            if rel:
                g0, g1 = split_products(Q + t_(bias_v, F32)[h], t_(pos, F32)[:, sl].T, drop_lo=mutant == "lo_kq")
                Gm = torch.cat([g0 + g1 * (1.0 / 2048.0), torch.zeros(N, 64)], 1)       # rows past 2T-2 read as zeros
            m_run = torch.full((N,), NEG_INF)
            l_run = torch.zeros(N)
            o0, o1 = torch.zeros(N, dk), torch.zeros(N, dk)
            for t in range(nt):
                j = torch.arange(t * 32, t * 32 + 32)
                jc = torch.clamp(j, max=M - 1)
                bias = torch.where((j >= M) | mk[jc], torch.tensor(NEG_INF), torch.tensor(0.0))
                s0, s1 = split_products(Qc, k[b, jc, sl].T, drop_lo=mutant == "lo_kq")
                s = s0 + s1 * (1.0 / 2048.0)
                if rel:
                    r = (N - 1) - torch.arange(N)[:, None] + j[None, :] + (1 if mutant == "rel_shift1" else 0)
                    s = s + torch.gather(Gm, 1, torch.clamp(r, max=Gm.shape[1] - 1))
                s = s * scale + bias
                m_new = torch.maximum(m_run, s.max(1).values)
                m_use = m_new if mutant == "neg_inf_max" else torch.where(m_new == NEG_INF, torch.zeros_like(m_new), m_new)
                alpha = torch.exp(m_run - m_use)
                e = torch.exp(s - m_use[:, None])
                l_run = l_run * alpha + e.sum(1)
                m_run = m_new
                if mutant != "no_rescale":
                    o0, o1 = o0 * alpha[:, None], o1 * alpha[:, None]
                a0, a1 = split_products(e, v[b, jc, sl], drop_lo=mutant == "lo_vp")
                o0, o1 = o0 + a0, o1 + a1
            out[b, :, sl] = (o0 + o1 * (1.0 / 2048.0)) * (1.0 / l_run)[:, None]
    return out


# ---------------------------------------------------------------- verdicts shared by the CPU (emulation) and GPU (kernel) tests

def report(kind, case, rows):
    """print the whole-tensor figures and the worst slice of judge_slices' rows; -> True when every row is inside its bound"""
    worst = max(rows[1:], key=lambda r: (not r[4], r[1] / r[3] if r[1] == r[1] else float("inf")), default=None)
    for name, err, err32, bound, ok in [rows[0]] + ([worst] if worst else []):
        ratio = err / err32 if err32 > 0 else (0.0 if err == 0 else float("inf"))
        print(f"block-regimes {kind} {case} [{name}]: err {err:.3e} err32 {err32:.3e} ratio {ratio:.2f} bound {bound:.3e}{'' if ok else '  OUTSIDE'}")
    return all(r[4] for r in rows)


def ffn_verdict(tag, with_res, out, out_ln, kind="ffn"):
    """out / out_ln [B,T,256] (either may be None) against ffn_refs: whole tensor and every sample, FFN_CAP"""
    (o64, l64), (o32, l32) = ffn_refs(tag, with_res)
    sl = [(f"b{b}", (b,)) for b in range(FFN_CASES[tag][0])]
    ok = True
    if out is not None:
        ok &= report(kind, f"{tag} res={int(with_res)} out", judge_slices(out, o64, o32, FFN_CAP, sl))
    if out_ln is not None:
        ok &= report(kind, f"{tag} res={int(with_res)} out_ln", judge_slices(out_ln, l64, l32, FFN_CAP, sl))
    return ok


def linear_ln_refs(i):
    d = linear_ln_inputs(i)
    a = (d["x"], d["ln_w"], d["ln_b"], LN_EPS, d["w"], d["b"], d["act"])
    return linear_ln_ref(*a, dtype=F64).numpy(), linear_ln_ref(*a, dtype=F32).numpy()


def linear_ln_verdict(i, got, kind="linear_ln"):
    """the rows below each sample's computed bound (LINEAR_LN_CAP), whole and per sample"""
    d = linear_ln_inputs(i)
    r64, r32 = linear_ln_refs(i)
    keep = np.concatenate([np.arange(n) + b * d["T"] for b, n in enumerate(d["rows"])])
    flat = lambda a: np.asarray(a).reshape(2 * d["T"], -1)[keep]                       # noqa: E731
    sl = [(f"b{b}", (slice(sum(d["rows"][:b]), sum(d["rows"][:b + 1])),)) for b in range(2)]
    return report(kind, f"T={d['T']} M={d['M']} ragged={int(d['ragged'])}", judge_slices(flat(got), flat(r64), flat(r32), LINEAR_LN_CAP, sl))


def _att_verdict(kind, tag, got, o64, s64, o32, mask, B, H, dk):
    live = live_samples(mask, B)
    got = np.asarray(got)
    for b in range(B):
        if b not in live:
            assert np.isnan(got[b]).all(), (tag, b, "a sample without a live key gets NaN rows, as torch's soft-max gives")
    cap = att_cap(s64[live])
    sl = head_slices(len(live), H, dk, range(len(live)))
    return report(kind, tag, judge_slices(got[live], o64[live], o32[live], cap, sl))


def attention_verdict(tag, got, kind="attention"):
    d = attention_inputs(tag)
    o64, s64, o32 = attention_refs(tag)
    return _att_verdict(kind, tag, got, o64, s64, o32, d["key_mask"], d["B"], d["H"], d["dk"])


def relpos_verdict(tag, got, kind="relpos"):
    d = relpos_inputs(tag)
    o64, s64, o32 = relpos_refs(tag)
    return _att_verdict(kind, tag, got, o64, s64, o32, d["pad_mask"], d["B"], d["H"], 64)
