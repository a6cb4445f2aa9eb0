"""numpy float64 restatements of the decode / TTS glue steps (csrc/decode_tts.hip, csrc/conformer_ops.hip) and the seeded inputs the
glue tests share.  Each function cites the reference lines its kernel cites; tests/test_glue_ref.py pins each one to an independent
statement (torch CPU float64 modules, torch.bucketize, the C oracle), tests/test_gpu_glue_regimes.py compares the kernels with them.

Path follow keeps its C oracle (oracle.dag_oracle.follow_path / argmax_logp / lookahead_next)."""
import numpy as np

from tests.util_posterior_ref import posterior_ref  # noqa: F401  (s2s_dag_fastspeech2_loss.py:259-262)

FP32_ULP = 2.0 ** -23


# ---------------------------------------------------------------- references

def argmax_logp_ref(x):
    """tok = first maximum over the last axis, score = log_softmax at it = -log sum_v exp(x_v - max)
    (s2s_conformer_dag_fastspeech2.py:207-208), on the input widened to float64.  -> (tok int32, score float64)"""
    x = np.asarray(x, np.float64)
    tok = x.argmax(-1)                                        # numpy: the first of equal maxima
    m = np.take_along_axis(x, tok[..., None], -1)
    with np.errstate(invalid="ignore"):
        s = np.exp(x - m).sum(-1)
    return tok.astype(np.int32), -np.log(s)


def dwconv_bn_silu_ref(x, w, bn_w, bn_b, mean, var, eps):
    """SiLU(BatchNorm_eval(depthwise_conv1d(x))) on channels-last x [B,T,C], w [C,K], zero padding (K-1)/2 — the middle of fairseq's
    ConvolutionModule (conformer_layer.py: depthwise_conv -> batch_norm -> activation) in eval mode.  bn_w / bn_b None: 1 / 0."""
    x = np.asarray(x, np.float64)
    w = np.asarray(w, np.float64)
    B, T, C = x.shape
    K = w.shape[1]
    P = (K - 1) // 2
    xp = np.zeros((B, T + K - 1, C))
    xp[:, P:P + T] = x
    y = np.zeros((B, T, C))
    for k in range(K):                                        # cross-correlation, as torch's Conv1d
        y += xp[:, k:k + T] * w[:, k]
    g = np.ones(C) if bn_w is None else np.asarray(bn_w, np.float64)
    be = np.zeros(C) if bn_b is None else np.asarray(bn_b, np.float64)
    y = (y - np.asarray(mean, np.float64)) / np.sqrt(np.asarray(var, np.float64) + eps) * g + be
    return y / (1.0 + np.exp(-y))


def layer_norm_ref(x, w, b, eps):
    """LayerNorm over the last axis: biased variance, eps inside the sqrt (torch.nn.LayerNorm's definition).  w / b None: 1 / 0."""
    x = np.asarray(x, np.float64)
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    y = (x - mu) / np.sqrt(var + eps)
    if w is not None:
        y = y * np.asarray(w, np.float64)
    if b is not None:
        y = y + np.asarray(b, np.float64)
    return y


def gather_rows_ref(features, keep_idx, n_feat, fmax):
    """out[b,k] = features[b, keep_idx[b,k]] for k < n_feat[b] (and a keep index inside the graph), zero rows elsewhere — the
    _collate_frames of the kept hidden states (s2s_conformer_dag_fastspeech2.py:219-243).  Keeps the features' dtype: a pure copy."""
    features = np.asarray(features)
    B, L, D = features.shape
    cap = keep_idx.shape[1]
    out = np.zeros((B, fmax, D), features.dtype)
    for b in range(B):
        for k in range(min(int(n_feat[b]), cap, fmax)):
            j = int(keep_idx[b, k])
            if 0 <= j < L:
                out[b, k] = features[b, j]
    return out


def bucketize_ref(values, bins):
    """first index with bins[idx] >= value (torch.bucketize, right=False), compared in float64; no bins: 0"""
    return np.searchsorted(np.asarray(bins, np.float64), np.asarray(values, np.float64), side="left").astype(np.int64)


def bucketize_embed_add_ref(x, values, bins, emb):
    """x + Embedding(bucketize(values, bins))  (fastspeech2.py:169-177,207-210).  The indices come from float64 comparisons, the add is the
    one fp32 add the kernel does, so the result can be compared bit for bit."""
    idx = bucketize_ref(values, bins)
    return np.asarray(x, np.float32) + np.asarray(emb, np.float32)[idx]


# ---------------------------------------------------------------- errors and bounds

def rel_err(got, ref):
    """max |got - ref| over the largest reference magnitude"""
    ref = np.asarray(ref, np.float64)
    scale = float(np.abs(ref).max())
    return float(np.abs(np.asarray(got, np.float64) - ref).max()) / (scale if scale > 0 else 1.0)


def fp32_bound(err32, cap):
    """"as accurate as an fp32 implementation": 8 x the error of torch's own fp32 result against the same float64 reference (the factor of
    test_split_precision_conv1d_is_fp32_accurate) + 4 fp32 ulps of the output scale (the __expf / __logf / rsqrtf intrinsics, which torch's
    path does not use), never beyond `cap`, the tolerance the older tests of the kernel already hold."""
    return min(8.0 * err32 + 4.0 * FP32_ULP, cap)


# ---------------------------------------------------------------- inputs (np.random.default_rng seeds; dtype float32 unless stated)

# (seed, B, T, L): one vertex, a partial wave, a wave + 1, exactly one trip of the 256-thread loops, one trip + 1; each at both scales
POSTERIOR_SMALL = [(41, 1, 3, 1), (42, 1, 3, 63), (43, 1, 3, 65), (44, 1, 3, 256), (45, 1, 3, 257)]
POSTERIOR_SCALES = (1.0, 300.0)
POSTERIOR_STRIDE = (47, 5, 820, 5)          # 4100 rows: 4 more than the 4096-workgroup grid


def posterior_inputs(seed, B, T, L, scale, dead_rows=()):
    """synthetic alpha, beta [B,T,L] float32: normal * scale with ~15 % -inf entries each (not DP outputs); every row keeps one finite sum
    unless listed in dead_rows (flat row indices), whose alpha is all -inf"""
    rng = np.random.default_rng(seed)
    a = (rng.standard_normal((B, T, L)) * scale).astype(np.float32)
    b = (rng.standard_normal((B, T, L)) * scale).astype(np.float32)
    a[rng.random((B, T, L)) < 0.15] = -np.inf
    b[rng.random((B, T, L)) < 0.15] = -np.inf
    keep = rng.integers(0, L, (B, T))                         # one live vertex per row
    bi, ti = np.meshgrid(np.arange(B), np.arange(T), indexing="ij")
    a[bi, ti, keep] = (rng.standard_normal((B, T)) * scale).astype(np.float32)
    b[bi, ti, keep] = (rng.standard_normal((B, T)) * scale).astype(np.float32)
    af = a.reshape(B * T, L)
    for r in dead_rows:
        af[r] = -np.inf
    return a, b


def stride_dead_rows(nrows=4100, grid=4096):
    """dead-row pattern of the grid-stride case: rows r and r + grid are handled by the same workgroup; for r in {0, 2} row r is live and
    row r + grid dead, for r in {1, 3} the other way round; elsewhere every 7th row is dead"""
    dead = {r for r in range(4, grid) if r % 7 == 0}
    dead |= {0 + grid, 2 + grid, 1, 3}
    return sorted(r for r in dead if r < nrows)


def ragged_posterior_inputs(seed, B, T, L, scale=1.0):
    """posterior_inputs with ragged target lengths: T_0 = T, the others shorter; rows t >= T_b are dead.  -> (alpha, beta, tgt_len)"""
    rng = np.random.default_rng(seed + 1000)
    tl = np.array([T] + [int(rng.integers(max(1, T // 2), T)) if T > 1 else 1 for _ in range(B - 1)], np.int64)
    dead = [b * T + t for b in range(B) for t in range(int(tl[b]), T)]
    a, b = posterior_inputs(seed, B, T, L, scale, dead)
    return a, b, tl


def features_inputs(seed, B, L, T, D):
    """features [B,L,D] and grad_out [B,T,D] float32"""
    rng = np.random.default_rng(seed + 2000)
    return rng.standard_normal((B, L, D)).astype(np.float32), rng.standard_normal((B, T, D)).astype(np.float32)


# planted bit-equal maxima of the (2, 7, 600) argmax case: (row, first position, second position)
TIES = [(0, 70, 200),        # different waves: thread 0's merge of the per-wave results
        (1, 5, 261),         # one thread, two trips of its stride-256 loop: the strict >
        (2, 63, 64)]         # the last lane of wave 0 and the first of wave 1


def argmax_inputs(seed, B, L, V, ties=()):
    """logits [B,L,V] float32; ties = (flat row, v1, v2): both set to a small integer above the row maximum, which fp16 and bf16 hold
    exactly and no other entry of the row can round up to"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((B, L, V)) * 3).astype(np.float32)
    xf = x.reshape(B * L, V)
    for r, v1, v2 in ties:
        xf[r, v1] = xf[r, v2] = np.float32(np.ceil(xf[r].max()) + 1.0)
    return x


def decode_inputs(seed, B, L, V, TR, D, out_len, pad, all_pad=False):
    """logits [B,L,V], links [B,L,TR] (log-softmax over the valid successors, -inf outside graph / window), features [B,L,D] float32.
    Some vertices emit <pad>, some repeat the token of their neighbour; all_pad: every vertex emits <pad>."""
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((B, L, V)) * 2).astype(np.float32)
    if all_pad:
        logits[:, :, pad] += 40.0
    else:
        logits[:, ::5, pad] += 20.0
        logits[:, 1::7, 7 % V] += 20.0
        logits[:, 2::7, 7 % V] += 20.0
    raw = rng.standard_normal((B, L, TR))
    i = np.arange(L)[None, :, None]; d = np.arange(TR)[None, None, :]
    valid = (i + d + 1) < np.asarray(out_len)[:, None, None]
    raw = np.where(valid, raw, -np.inf)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = raw.max(-1, keepdims=True)
        m = np.where(np.isfinite(m), m, 0.0)
        links = raw - m - np.log(np.exp(raw - m).sum(-1, keepdims=True))
    links = np.where(valid, links, -np.inf).astype(np.float32)
    feats = rng.standard_normal((B, L, D)).astype(np.float32)
    return logits, links, feats


# (seed, n, C, nb)
BUCKETIZE_CASES = [(61, 4100, 256, 255), (62, 5, 260, 2), (63, 3, 24, 0)]


def bucketize_inputs(seed, n, C, nb):
    """x [n,C], values [n], bins [nb] (sorted), emb [nb+1,C] float32; the first values sit on bin edges, below the first bin, above the last
    one and at -inf / +inf"""
    rng = np.random.default_rng(seed)
    bins = np.sort(rng.standard_normal(nb)).astype(np.float32)
    v = (rng.standard_normal(n) * 2).astype(np.float32)
    special = [-np.inf, np.inf]
    if nb:
        special += [bins[0], bins[0] - 1.0, bins[-1] + 1.0, bins[-1], bins[nb // 2], np.nextafter(bins[0], np.float32(-np.inf)),
                    np.nextafter(bins[-1], np.float32(np.inf))]
    for k, s in enumerate(special[:n]):
        v[k] = s
    if n > 4096:                                              # the rows a second grid-stride trip serves
        v[4096] = special[2 % len(special)]; v[n - 1] = np.inf
    emb = rng.standard_normal((nb + 1, C)).astype(np.float32)
    x = rng.standard_normal((n, C)).astype(np.float32)
    return x, v, bins, emb


# (seed, B, T, C, K)
DWCONV_CASES = [(71, 1, 1, 4, 31), (72, 2, 9, 4, 3), (73, 1, 17, 260, 15), (74, 3, 8, 64, 7), (75, 2, 40, 256, 31)]


def dwconv_inputs(seed, B, T, C, K):
    """x [B,T,C], w [C,K], bn weight, bias, running mean, running var [C] float32"""
    rng = np.random.default_rng(seed)
    f = lambda a: a.astype(np.float32)
    return (f(rng.standard_normal((B, T, C))), f(rng.standard_normal((C, K)) / np.sqrt(K)), f(rng.uniform(0.5, 1.5, C)), f(rng.normal(0, 0.3, C)),
            f(rng.normal(0, 0.5, C)), f(rng.uniform(0.3, 2.0, C)))


# (seed, rows, C, mean, spread)
LAYER_NORM_CASES = [(81, 1, 4, 1.5, 3.0), (82, 5, 260, 1.5, 3.0), (83, 3, 2048, 1.5, 3.0), (84, 9, 256, 1.5, 3.0), (85, 9, 256, 100.0, 0.01)]


def layer_norm_inputs(seed, rows, C, mean, spread):
    """x [rows,C] = mean + spread * normal, weight, bias [C] float32"""
    rng = np.random.default_rng(seed)
    x = (mean + spread * rng.standard_normal((rows, C))).astype(np.float32)
    return x, rng.uniform(0.5, 1.5, C).astype(np.float32), rng.normal(0, 0.2, C).astype(np.float32)
