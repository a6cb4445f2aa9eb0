"""float64 references of the link producer (DAGDecoder.extract_links, s2t_conformer_dag.py:171-212, banded branch) for the tests of
csrc/extract_links_f64.hip: two independent formulations, both torch on CPU tensors, inputs seeded by a torch.Generator, gradients by CPU
autograd.

  links_band   the band-gather form of tests/test_gpu_decode_ops.py::test_fused_extract_links_backward_direct_q_k_gates: the dense
               [B,L,L,H] content, the band gathered out of it, log_softmax over the window, logsumexp over the heads (log space);
  links_loop   one source vertex at a time in exp space: the successors' rows in reversed order, channels summed in reversed order,
               p = exp(s - max) / sum, links = log(sum_h p * gate probability) — another summation order, no log_softmax / logsumexp.

`reference(case, use_bias)` computes the band form with its stats and gradients ONCE per process and hands the same (read-only) tensors to
every test that asks."""
import functools
import math

import torch

H = 8
NEG = float("-inf")

# (B, L, CK, TR, out_len): L off the 4-vertex tile, a graph of 2 vertices, rows without a successor, TR just past one 32-lane chunk, the
# full window, the smallest graph
CASES = [
    (3, 70, 64, 7, (70, 51, 2)),
    (3, 70, 64, 32, (70, 51, 2)),
    (2, 45, 32, 33, (45, 30)),
    (3, 70, 128, 69, (70, 51, 2)),
    (1, 6, 32, 1, (6,)),
]
TILED = (2, 700, 64, 699, (700, 333))           # a window beyond one LDS tile of the double kernels


def make_case(case, scale=0.5):
    """q, k [B,L,H,CK], log_gates [B,L,H], out_len [B], loss weights w [B,L,TR], dist_bias [TR]: float64 CPU tensors"""
    B, L, CK, TR, lens = case
    g = torch.Generator().manual_seed(100000 + 1000 * L + 10 * TR + CK)
    q = torch.randn(B, L, H, CK, dtype=torch.float64, generator=g) * scale
    k = torch.randn(B, L, H, CK, dtype=torch.float64, generator=g) * scale
    lg = torch.log_softmax(torch.randn(B, L, H, dtype=torch.float64, generator=g), -1)
    w = torch.randn(B, L, TR, dtype=torch.float64, generator=g)
    bias = -0.02 * torch.arange(TR, dtype=torch.float64) + 0.05 * torch.randn(TR, dtype=torch.float64, generator=g)
    return {"q": q, "k": k, "lg": lg, "olen": torch.tensor(lens, dtype=torch.long), "w": w, "bias": bias, "TR": TR}


def links_band(q, k, lg, olen, TR, bias=None):
    """(links [B,L,TR], stats [B,L,H,2] detached) in the dtype of q"""
    B, L, _, CK = q.shape
    content = torch.einsum("bicf,bjcf->bijc", q, k) / (CK ** 0.5)
    idx = torch.arange(L).unsqueeze(1) + torch.arange(TR).unsqueeze(0) + 1
    invalid = idx.unsqueeze(0) >= olen.view(B, 1, 1)
    band = content.gather(2, idx.unsqueeze(0).masked_fill(invalid, 0).unsqueeze(-1).expand(-1, -1, -1, H))
    if bias is not None:
        band = band + bias.to(band).view(1, 1, TR, 1)
    nouse = invalid.all(-1)
    masked = band.masked_fill(invalid.unsqueeze(-1), NEG)
    with torch.no_grad():
        mx = masked.max(2).values                                                   # [B,L,H]
        ls = (masked - mx.masked_fill(nouse.unsqueeze(-1), 0.0).unsqueeze(2)).exp().sum(2).masked_fill(nouse.unsqueeze(-1), 1.0).log()
        stats = torch.stack([mx, ls], -1)
    ls_band = torch.log_softmax(masked.masked_fill(nouse.view(B, L, 1, 1), 0.0), 2).masked_fill(invalid.unsqueeze(-1), -1e30)
    out = torch.logsumexp(ls_band + lg.unsqueeze(2), -1)
    return out.masked_fill(invalid, NEG), stats


def links_loop(q, k, lg, olen, TR, bias=None):
    """the same (links, stats) vertex by vertex in exp space"""
    B, L, _, CK = q.shape
    scale = 1.0 / math.sqrt(CK)
    gp = lg.exp()
    stats = torch.zeros(B, L, H, 2, dtype=q.dtype)
    stats[..., 0] = NEG
    rows = []
    for b in range(B):
        Lb = min(L, int(olen[b]))
        for i in range(L):
            n = min(Lb - i - 1, TR)
            if n <= 0:
                rows.append(torch.full((TR,), NEG, dtype=q.dtype))
                continue
            kk = k[b, i + 1:i + 1 + n].flip(0)                                      # successors in reversed order [n,H,CK]
            s = (kk * q[b, i].unsqueeze(0)).flip(-1).sum(-1) * scale               # [n,H]
            if bias is not None:
                s = s + bias[:n].to(s).flip(0).unsqueeze(1)
            m = s.detach().max(0).values
            e = (s - m).exp()
            z = e.sum(0)
            stats[b, i, :, 0] = m
            stats[b, i, :, 1] = z.detach().log()
            val = ((e / z) * gp[b, i]).sum(-1).log().flip(0)
            rows.append(torch.cat([val, torch.full((TR - n,), NEG, dtype=q.dtype)]))
    return torch.stack(rows).view(B, L, TR), stats


def masked_loss(links, w):
    """weights the links unevenly and ignores the -inf entries (as dag_loss's gradient does)"""
    fin = torch.isfinite(links)
    return (links.masked_fill(~fin, 0.0) * w.to(links)).sum()


def run(form, c, use_bias, dtype=torch.float64):
    """{links, stats, dq, dk, dg} of one formulation on the case's inputs cast to `dtype`"""
    q, k, lg = (c[n].to(dtype).clone().requires_grad_() for n in ("q", "k", "lg"))
    links, stats = form(q, k, lg, c["olen"], c["TR"], c["bias"].to(dtype) if use_bias else None)
    masked_loss(links, c["w"]).backward()
    return {"links": links.detach(), "stats": stats, "dq": q.grad, "dk": k.grad, "dg": lg.grad}


@functools.lru_cache(maxsize=None)
def _reference(case, use_bias):
    c = make_case(case)
    return c, run(links_band, c, use_bias)


def reference(case, use_bias):
    """(inputs, band-form results) of a case — computed once, shared, not to be modified"""
    return _reference(tuple(case), bool(use_bias))


def max_abs_diff(a, b):
    """largest |a - b| over the entries finite in b (0 for none); the -inf patterns must agree"""
    assert torch.equal(torch.isneginf(a), torch.isneginf(b))
    f = torch.isfinite(b)
    return float((a[f].double() - b[f].double()).abs().max()) if f.any() else 0.0


def max_tol_ratio(a, b, rtol, atol):
    """largest |a - b| / (atol + rtol |b|): <= 1 is what assert_allclose(a, b, rtol, atol) accepts"""
    return float(((a.double() - b.double()).abs() / (atol + rtol * b.double().abs())).max())
