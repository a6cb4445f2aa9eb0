"""float64 restatement of the two embedding-entry operators (include/daspeech_decode.h: dsp_embed_entry_fwd / _bwd, dsp_pos_add_fwd / _bwd),
forward and backward, on the inputs AS STORED (already rounded to their dtype) and with an explicit keep mask, plus the token patterns and the
torch lines of the models that the CPU and GPU tests share."""
import numpy as np
import torch

PAD, BOS, EOS, UNK = 1, 0, 2, 3
SORT_MAX = 64          # DSP_EMBED_ENTRY_SORT_MAX
GRAD_CHUNK = 64        # DSP_EMBED_GRAD_CHUNK


def f64(t):
    return t.detach().to(torch.float64).cpu().numpy()


def positions(keep, pad):
    """pad + keep * cumsum(keep) along the last axis (DAGDecoder.positions, positions_from_padding_mask)"""
    keep = keep.astype(np.int64)
    return pad + keep * np.cumsum(keep, axis=1)


def embed_entry_ref(tokens, E, P, pad, scale, keep_mask=None, keep_scale=1.0, dy=None):
    """tokens [B,L] int64 array, E [V,C] / P [NP,C] float64 arrays as stored, keep_mask None or a bool [B*L,C] array, dy None or [B,L,C].
    -> dict y [B,L,C] (and dE, dP with dy).  A token outside [0, V) contributes a zero row and counts as non-pad; row `pad` of dE and dP is
    zero (padding_idx)."""
    B, L = tokens.shape
    V, C = E.shape
    pos = positions(tokens != pad, pad)
    inside = (tokens >= 0) & (tokens < V)
    emb = np.where(inside[..., None], E[np.where(inside, tokens, 0)], 0.0)
    m = np.ones((B, L, C)) if keep_mask is None else keep_mask.reshape(B, L, C).astype(np.float64) * keep_scale
    out = {"y": m * (float(scale) * emb + P[pos])}
    if dy is not None:
        g = (np.asarray(dy, np.float64) * m).reshape(B * L, C)
        dE, dP = np.zeros_like(E), np.zeros_like(P)
        tk, ps = tokens.reshape(-1), pos.reshape(-1)
        ok = inside.reshape(-1)
        np.add.at(dE, tk[ok], g[ok])
        np.add.at(dP, ps, g)
        dE *= float(scale)
        dE[pad] = 0.0
        dP[pad] = 0.0
        out.update(dE=dE, dP=dP)
    return out


def pos_add_ref(x, mask, tab, alpha, keep_mask=None, keep_scale=1.0, dy=None, pad=1):
    """x [B,N,C], mask [B,N] bool (True: padding), tab [NT,C], alpha a float, all float64 as stored -> dict y (and dx, dalpha with dy)"""
    B, N, C = x.shape
    pos = np.minimum(positions(~mask, pad), tab.shape[0] - 1)
    m = np.ones((B, N, C)) if keep_mask is None else keep_mask.reshape(B, N, C).astype(np.float64) * keep_scale
    out = {"y": m * (x + float(alpha) * tab[pos])}
    if dy is not None:
        g = np.asarray(dy, np.float64) * m
        out.update(dx=g, dalpha=np.array([(g * tab[pos]).sum()]))
    return out


# ---------------------------------------------------------------- the models' own lines (the parent commit's), any dtype and device
def torch_embed_entry(tokens, E, P, pad, scale, keep=None, keep_scale=1.0):
    """DAGDecoder.extract_features' entry lines with the mask applied by a multiply"""
    k = tokens.ne(pad).int()
    pos = (torch.cumsum(k, dim=1) * k).long() + pad
    x = scale * torch.nn.functional.embedding(tokens, E, padding_idx=pad) + torch.nn.functional.embedding(pos, P, padding_idx=pad)
    return x if keep is None else x * (keep.view_as(x).to(x.dtype) * keep_scale)


def torch_pos_add(x, mask, tab, alpha, keep=None, keep_scale=1.0, pad=1):
    """FastSpeech2NoEmb.forward's positional lines (positions_from_padding_mask, the clamp of _pos) with the mask applied by a multiply"""
    k = (~mask).int()
    idx = ((torch.cumsum(k, dim=1) * k).long() + pad).clamp(max=tab.shape[0] - 1)
    y = x + alpha * tab[idx]
    return y if keep is None else y * (keep.view_as(y).to(y.dtype) * keep_scale)


# ---------------------------------------------------------------- token patterns
def token_case(name, V, seed=0):
    """-> tokens [B,L] int64 numpy array for a named pattern (see TOKEN_CASES)"""
    rng = np.random.default_rng(seed)
    if name == "train":                       # [bos, unk..., eos, pad...] of three lengths
        L, lens = 65, (65, 40, 3)
        t = np.full((3, L), PAD, np.int64)
        for b, n in enumerate(lens):
            t[b, :n] = UNK; t[b, 0] = BOS; t[b, n - 1] = EOS
        return t
    if name == "left-pad":
        t = np.full((3, 63), PAD, np.int64)
        for b, n in enumerate((63, 20, 1)):
            t[b, 63 - n:] = rng.integers(4, V, n)
        return t
    if name == "interior":
        t = rng.integers(4, V, (3, 130)).astype(np.int64)
        t[:, ::3] = PAD; t[1, 40:90] = PAD; t[2, 0] = PAD; t[2, -1] = PAD
        return t
    if name == "all-pad-row":
        t = rng.integers(4, V, (3, 64)).astype(np.int64)
        t[1, :] = PAD
        return t
    if name == "no-pad":
        return rng.integers(4, V, (1, 64)).astype(np.int64)
    if name == "one":
        return np.array([[UNK]], np.int64)
    if name == "distinct":                    # every token another key
        assert V >= 130 + 4
        return (4 + rng.permutation(V - 4)[:130]).reshape(1, 130).astype(np.int64)
    if name == "out-of-range":
        t = rng.integers(4, V, (3, 24)).astype(np.int64)
        t[0, 5] = V; t[1, 0] = -1; t[2, 23] = V + 1000; t[2, 3:6] = PAD
        return t
    raise KeyError(name)


def hot_key_case(count, V, L=130, seed=0):
    """B = 3 rows of L in which key UNK appears exactly `count` times (the other vertices distinct tokens >= 4 where V allows, else spread
    evenly over the few keys there are), one pad at the end of each row"""
    rng = np.random.default_rng(seed + count)
    n = 3 * L
    assert count <= n - 3
    flat = np.empty(n, np.int64)
    others = n - count
    if V - 4 >= others:
        flat[:others] = 4 + rng.permutation(V - 4)[:others]
    else:
        flat[:others] = np.array([0, 2] + list(range(4, V)))[np.arange(others) % (V - 2)]
    flat[others:] = UNK
    rng.shuffle(flat)
    t = flat.reshape(3, L)
    for b in range(3):                      # a pad at each row's end, the displaced token is dropped unless it is a hot one
        if t[b, -1] == UNK:
            j = int(np.flatnonzero(t[b] != UNK)[0])
            t[b, j] = UNK
        t[b, -1] = PAD
    assert (t == UNK).sum() == count
    return t


TOKEN_CASES = ("train", "left-pad", "interior", "all-pad-row", "no-pad", "one", "distinct", "out-of-range")
# one below, at and one above the threshold between the sorted fill and the ballot compaction, which is also the chunk of the sums, and two chunks
HOT_COUNTS = (SORT_MAX - 1, SORT_MAX, SORT_MAX + 1, 2 * GRAD_CHUNK - 1, 2 * GRAD_CHUNK, 2 * GRAD_CHUNK + 1)
