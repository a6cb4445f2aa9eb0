"""Case table, float64 references and CPU emulations for the fp32 link kernels (csrc/extract_links.hip: one-image and tiled fp32-FMA kernels;
csrc/extract_links_mfma.hip: split-fp16 scores on the matrix cores, exact-fp32 or bf16-triple contractions) at the launch and score regimes
the older link tests do not reach.  tests/test_links_regimes_ref.py checks all of this on the CPU, tests/test_gpu_links_regimes.py holds the
kernels to it.

References (float64, torch on CPU tensors, gradients by CPU autograd through an explicit grad_links tensor):
  links_bandc   the band form of tests/util_links_ref.links_band chunked over source rows (no [L,L,H] tensor): the reference of the GPU tests
  links_loop    tests/util_links_ref.links_loop, vertex by vertex in exp space: the second formulation
Both run on the fp32 inputs WIDENED, so the rounding of the inputs is no part of any error.

Emulation (`emulate`): the same operation computed the way a kernel family computes it, in fp32 —
  FMA family    four fp32 FMA chains per dot product ((a0 + a1) + (a2 + a3)), natural-log soft-max state over the whole window
  matrix cores  q scale log2(e) and k cut into fp16 hi / lo pieces, score = hh + (hl + lh) / 2048 accumulated in fp32 per 16 channels, base-2
                online soft-max state per lane half, merged across the 32-partner tiles walked from the far end of the window, the two halves
                merged last; contraction 0 = fp32 products, contraction 1 = bf16 triples (8 + 8 + 8 bits by truncation), six products
Its error against float64 is the `err_ref` of the bound; with a `mutant` it computes a subtly wrong kernel instead.

Bound, per slice on the slice's own scale (links, dgate: per sample; stats, dq, dk: per (sample, head)):
    err <= min(8 err_ref + 4 2^-23 scale, 2e-5 scale),   scale = the slice's largest |float64 reference|
(the form of tests/util_glue_ref.fp32_bound; the cap is what test_matrix_core_extract_links_at_baseline_graph_size holds, without its floor
of 1).  A slice of zeros has scale 0: the kernels must write exact zeros there (the one exception, dq and dk at TR = 1: `void_gradients`).

One departure from the lengths first proposed for the B = 6 table, (160, 33, 32, 31, 2, 1): the graph of two vertices has seventeen here.
Two vertices are one soft-max row with one slot: its probability is 1 whatever the score, so dq and dk are identically zero and the one link
is log(sum of the gate probabilities) = 0 — float64 leaves rounding noise of 1e-17 there and a relative bound has no scale to refer to.  A
graph of three vertices is hardly better: one row with two slots carries the whole gradient of a (sample, head) slice, next to a one-slot row
whose ds = A - p SA is A times the rounding of p = 1; what such a slice holds the kernel to is a single rounding event of the emulation, not
the error of fp32 arithmetic (and under peaked or steep scores the two-slot soft-max is one-hot to 1e-8 and the slice is rounding alone: the
fp32 evaluation of the reference is then outside 2e-5 of the slice's scale, which the cap rules out for a row).  Seventeen vertices give
every head a dozen rows whose gradient survives, and keep what the short graph is in the table for: a single live tile, a one-slot row,
rows without a successor, dead tiles.  Graphs of two and three vertices stay covered by tests/util_links_ref.CASES and the FMA rows here."""
import functools
import math
from collections import namedtuple

import torch

from tests.util_links_ref import H, NEG, links_loop  # noqa: F401

F32, F64 = torch.float32, torch.float64
ULP = 2.0 ** -23
CAP = 2e-5
LOG2E, LN2 = 1.4426950408889634, 0.6931471805599453
NAMES = ("links", "stats", "dq", "dk", "dg")

# fam: "mfma" (csrc/extract_links_mfma.hip), "one" / "tiled" (csrc/extract_links.hip);  contract: the xl_contract pins the backward runs
# with (None = unset: the library's default by size);  tile: the xl_tile pin;  reach: what tests/test_links_regimes_ref.py asserts of the row
Row = namedtuple("Row", "id fam B L CK TR lens score grad contract tile reach")

B6 = (160, 33, 32, 31, 17, 1)         # (see the module's docstring)


def _lens(B, L, step):
    return tuple(L - step * b for b in range(B))


def _m(id, B, L, TR, lens, score="flat", grad="unit", contract=(0, 1), reach=()):
    return Row(id, "mfma", B, L, 64, TR, tuple(lens), score, grad, tuple(contract), 0, tuple(reach))


def _f(id, fam, B, L, CK, TR, lens, score="flat", grad="unit", tile=0, reach=()):
    return Row(id, fam, B, L, CK, TR, tuple(lens), score, grad, (), tile, tuple(reach))


ROWS = [
    # ---- matrix cores.  B % 8 == 0: workgroups go round the XCDs, sample = XCD + 8 n; all lengths differ, NQ = 3 owner tiles
    _m("mc-B8-L70-TR7", 8, 70, 7, _lens(8, 70, 7), reach=("xcd", "nq3", "partial")),
    _m("mc-B8-L70-TR69", 8, 70, 69, _lens(8, 70, 7), reach=("xcd", "nq3", "full")),
    _m("mc-B16-L70-TR7", 16, 70, 7, _lens(16, 70, 4), reach=("xcd", "xcd_round2", "nq3")),
    _m("mc-B16-L70-TR69", 16, 70, 69, _lens(16, 70, 4), reach=("xcd", "xcd_round2", "nq3", "full")),
    # B = 6: live tile counts 1..5, odd and even step counts, EMIT's dead tiles, FULL and partial blocks, rows without a successor
    _m("mc-B6-L160-TR1", 6, 160, 1, B6, reach=("nlive1", "nlive2", "nosucc", "dead", "partial")),
    _m("mc-B6-L160-TR31", 6, 160, 31, B6, reach=("nlive1", "nlive2", "dead", "live_odd", "live_even")),
    _m("mc-B6-L160-TR32", 6, 160, 32, B6, reach=("nlive2", "dead", "partial")),
    _m("mc-B6-L160-TR33", 6, 160, 33, B6, reach=("nlive3", "dead", "step_odd")),
    _m("mc-B6-L160-TR64", 6, 160, 64, B6, reach=("nlive3", "dead", "full", "step_odd")),
    _m("mc-B6-L160-TR159", 6, 160, 159, B6, reach=("nlive1", "nlive2", "nlive3", "nlive4", "nlive5", "dead", "full", "partial", "nosucc")),
    # graph lengths at 32 k - 1, 32 k, 32 k + 1
    _m("mc-L65-TR33", 3, 65, 33, (65, 64, 63), reach=("len32k-1", "len32k", "len32k+1")),
    _m("mc-L95-TR33", 3, 95, 33, (95, 65, 31), reach=("len32k-1", "len32k+1")),
    _m("mc-L97-TR33", 3, 97, 33, (97, 96, 64), reach=("len32k", "len32k+1")),
    # the dispatch boundary: the last graph on 32-owner tiles, then 64-owner tiles (QG = 2) and the bf16-triple contraction by default
    _m("mc-L1536-TR33", 1, 1536, 33, (1536,), reach=("qg1", "nlive3")),
    _m("mc-L1570-TR40", 2, 1570, 40, (1570, 1500), reach=("qg2", "nlive4", "partial", "step_even")),
    _m("mc-L1570-TR97-default", 2, 1570, 97, (1570, 1500), contract=(None,), reach=("qg2", "triple_by_default", "full")),
    # score regimes on the B = 6 table
    _m("mc-B6-TR33-peaked", 6, 160, 33, B6, score="peaked", reach=("score",)),
    _m("mc-B6-TR64-steep", 6, 160, 64, B6, score="steep", reach=("score",)),
    _m("mc-B6-TR159-rise", 6, 160, 159, B6, score="rise", reach=("score", "nlive5")),
    _m("mc-B6-TR159-fall", 6, 160, 159, B6, score="fall", reach=("score", "nlive5")),
    _m("mc-B6-TR33-bias_steep", 6, 160, 33, B6, score="bias_steep", reach=("score",)),
    _m("mc-B6-TR64-bias_none", 6, 160, 64, B6, score="bias_none"),
    _m("mc-B6-TR31-gate_off", 6, 160, 31, B6, score="gate_off", reach=("gate_off",)),
    # gradient regimes
    _m("mc-B6-TR159-ranged", 6, 160, 159, B6, grad="ranged", reach=("ranged",)),
    _m("mc-B6-TR159-sparse", 6, 160, 159, B6, grad="sparse", reach=("sparse",)),
    _m("mc-B6-TR159-planted", 6, 160, 159, B6, grad="planted", reach=("planted",)),
    _m("mc-L1570-TR40-ranged", 2, 1570, 40, (1570, 1500), grad="ranged", reach=("qg2", "ranged")),
    _m("mc-L1570-TR40-sparse", 2, 1570, 40, (1570, 1500), grad="sparse", reach=("qg2", "sparse")),
    _m("mc-L1570-TR40-planted", 2, 1570, 40, (1570, 1500), grad="planted", reach=("qg2", "planted")),
    # ---- fp32 FMA, one image per workgroup: every head width, L off the 4-vertex tile, TR round one 32-lane chunk and the full window
    _f("one-CK32-L5-TR4", "one", 2, 5, 32, 4, (5, 3), reach=("nosucc",)),
    _f("one-CK32-L70-TR31", "one", 3, 70, 32, 31, (70, 51, 3)),
    _f("one-CK64-L70-TR32-sparse", "one", 3, 70, 64, 32, (70, 51, 3), grad="sparse", reach=("sparse",)),
    _f("one-CK64-L70-TR33", "one", 3, 70, 64, 33, (70, 51, 3)),
    _f("one-CK64-L5-TR4", "one", 2, 5, 64, 4, (5, 3)),
    _f("one-CK128-L70-TR69", "one", 3, 70, 128, 69, (70, 51, 3)),
    _f("one-CK128-L5-TR4", "one", 2, 5, 128, 4, (5, 3)),
    _f("one-CK64-L70-TR69-steep-planted", "one", 3, 70, 64, 69, (70, 51, 17), score="steep", grad="planted", reach=("score", "planted")),
    _f("one-CK32-L70-TR33-fall-ranged", "one", 3, 70, 32, 33, (70, 51, 3), score="fall", grad="ranged", reach=("score", "ranged")),
    # ---- fp32 FMA, window walked in tiles of TW slots: windows of k TW - 1, k TW and k TW + 1 slots
    _f("tiled32-L70-TR63", "tiled", 3, 70, 64, 63, (70, 51, 3), tile=32),
    _f("tiled32-L70-TR64", "tiled", 3, 70, 64, 64, (70, 51, 3), tile=32),
    _f("tiled32-L70-TR65-peaked-planted", "tiled", 3, 70, 64, 65, (70, 51, 17), score="peaked", grad="planted", tile=32, reach=("score", "planted")),
    _f("tiled64-L131-TR127", "tiled", 2, 131, 64, 127, (131, 77), tile=64),
    _f("tiled64-L131-TR128-rise-sparse", "tiled", 2, 131, 32, 128, (131, 77), score="rise", grad="sparse", tile=64, reach=("score", "sparse")),
    _f("tiled64-L131-TR129-ranged", "tiled", 2, 131, 128, 129, (131, 77), grad="ranged", tile=64, reach=("ranged",)),
    # the library's own choice: a one-image LDS above 150 KB, three tiles of 512 slots
    _f("tiled-auto-L1160-TR1159", "tiled", 1, 1160, 64, 1159, (1160,), reach=("auto_tiled",)),
]
ROW = {r.id: r for r in ROWS}
IDS = [r.id for r in ROWS]

# largest window maximum (natural-log scores, over samples, vertices and heads) per score regime: asserted by the CPU companion
SCORE_INTERVAL = {"flat": (0.4, 2.5), "peaked": (8.0, 30.0), "steep": (30.0, 80.0), "rise": (8.0, 40.0), "fall": (8.0, 40.0),
                  "bias_steep": (0.3, 2.5), "bias_none": (0.4, 2.5), "gate_off": (0.4, 2.5)}
SLOPE = 0.15          # rise / fall: score difference of neighbouring successors; the other channels (scale 0.1) add noise of ~0.01, so the
                      # ramp orders ANY two successors — a tile the window touches with one slot included
GATE_OFF_HEAD = 3


# ---------------------------------------------------------------------------------------------------------------- inputs

def _seed(row):
    return 7000003 + 1000 * row.L + 10 * row.TR + row.CK + 17 * row.B + 100003 * sorted(SCORE_INTERVAL).index(row.score)


@functools.lru_cache(maxsize=None)
def _inputs(row):
    B, L, CK, TR = row.B, row.L, row.CK, row.TR
    g = torch.Generator().manual_seed(_seed(row))
    s = {"peaked": 2.0, "steep": 3.5, "rise": 0.1, "fall": 0.1}.get(row.score, 0.5)
    q = torch.randn(B, L, H, CK, dtype=F64, generator=g) * s
    k = torch.randn(B, L, H, CK, dtype=F64, generator=g) * s
    logit = torch.randn(B, L, H, dtype=F64, generator=g)
    w = torch.randn(B, L, TR, dtype=F64, generator=g)
    d = torch.arange(TR, dtype=F64)
    bias = -0.02 * d + 0.05 * torch.randn(TR, dtype=F64, generator=g)
    if row.score in ("rise", "fall"):
        # channel 0 carries a ramp over the successors: q0 k0 / sqrt(CK) = -+ SLOPE j
        q[..., 0] = math.sqrt(CK)
        k[..., 0] = (SLOPE if row.score == "fall" else -SLOPE) * torch.arange(L, dtype=F64).view(1, L, 1)
        bias = -0.02 * d                                         # (no jitter: it would reorder neighbours)
    if row.score == "bias_steep":
        bias = -0.5 * d
    if row.score == "bias_none":
        bias = None
    if row.score == "gate_off":
        logit[:, ::3, GATE_OFF_HEAD] -= 80.0
    lg = torch.log_softmax(logit, -1)
    if TR == 1:
        # one slot per window: every soft-max is 1 and the link is the gates' mass, log(sum_h gate_h) — which is 0 for normalised gates and
        # would leave the links without a scale; the mass varies per vertex here
        lg = lg + 0.5 * torch.randn(B, L, 1, dtype=F64, generator=g)
    olen = torch.tensor(row.lens, dtype=torch.long)
    i = torch.arange(L).view(1, L, 1)
    invalid = (i + torch.arange(TR).view(1, 1, TR) + 1) >= olen.view(B, 1, 1).clamp(max=L)
    if row.grad == "ranged":
        w = w * torch.tensor([2.0 ** (40 * (b % 3 - 1)) for b in range(B)], dtype=F64).view(B, 1, 1)
    if row.grad == "sparse":
        w[:, 1::3] = 0.0
    w = w.to(F32)
    if row.grad == "planted":
        bad = torch.tensor([float("nan"), float("inf"), float("-inf")], dtype=F32)
        n = int(invalid.sum())
        w[invalid] = bad[torch.arange(n) % 3]
    c = {"q": q.to(F32), "k": k.to(F32), "lg": lg.to(F32), "olen": olen, "G": w, "bias": None if bias is None else bias.to(F32),
         "TR": TR, "invalid": invalid}
    return c


def inputs(row):
    """q, k [B,L,H,CK], lg [B,L,H], G = grad_links [B,L,TR], bias [TR] or None: the fp32 tensors the kernels get (drawn in float64 from a
    seeded CPU generator, then narrowed); olen [B]; invalid [B,L,TR] = the slots beyond the sample's graph.  Shared: not to be modified."""
    return _inputs(row)


# ---------------------------------------------------------------------------------------------------------------- float64 references

def links_bandc(q, k, lg, olen, TR, bias=None, chunk=None):
    """tests/util_links_ref.links_band over chunks of source rows: (links [B,L,TR], stats [B,L,H,2] detached)"""
    B, L, _, CK = q.shape
    chunk = chunk or (L if L <= 256 else 128)
    outs, stats = [], []
    for i0 in range(0, L, chunk):
        i1 = min(L, i0 + chunk)
        j0, j1 = min(i0 + 1, L - 1), min(L, i1 + TR)                               # successors j0 .. j1-1 serve the chunk
        content = torch.einsum("bicf,bjcf->bijc", q[:, i0:i1], k[:, j0:j1]) / (CK ** 0.5)
        idx = torch.arange(i0, i1).unsqueeze(1) + torch.arange(TR).unsqueeze(0) + 1
        invalid = idx.unsqueeze(0) >= olen.view(B, 1, 1).clamp(max=L)
        loc = (idx - j0).unsqueeze(0).masked_fill(invalid, 0).unsqueeze(-1).expand(-1, -1, -1, H)
        band = content.gather(2, loc)
        if bias is not None:
            band = band + bias.to(band).view(1, 1, TR, 1)
        nouse = invalid.all(-1)
        masked = band.masked_fill(invalid.unsqueeze(-1), NEG)
        with torch.no_grad():
            mx = masked.max(2).values
            ls = (masked - mx.masked_fill(nouse.unsqueeze(-1), 0.0).unsqueeze(2)).exp().sum(2).masked_fill(nouse.unsqueeze(-1), 1.0).log()
            stats.append(torch.stack([mx, ls], -1))
        ls_band = torch.log_softmax(masked.masked_fill(nouse.view(B, -1, 1, 1), 0.0), 2).masked_fill(invalid.unsqueeze(-1), -1e30)
        outs.append(torch.logsumexp(ls_band + lg[:, i0:i1].unsqueeze(2), -1).masked_fill(invalid, NEG))
    return torch.cat(outs, 1), torch.cat(stats, 1)


def _fwd_key(row):
    return row._replace(id="", grad="", contract=(), tile=0, reach=(), fam="")


@functools.lru_cache(maxsize=None)
def _forward64(key, form):
    c = _inputs(key._replace(grad="unit"))
    q, k, lg = (c[n].to(F64).clone().requires_grad_() for n in ("q", "k", "lg"))
    links, stats = form(q, k, lg, c["olen"], c["TR"], None if c["bias"] is None else c["bias"].to(F64))
    return (q, k, lg), links, stats


def run64(row, form=links_bandc):
    """{links, stats, dq, dk, dg} of a float64 formulation on the row's inputs widened; grad_links is applied as it stands — a NaN or an
    infinity at a slot beyond the graph meets the constant -inf the formulation wrote there and never reaches q, k or the gates"""
    leaves, links, stats = _forward64(_fwd_key(row), form)
    dq, dk, dg = torch.autograd.grad(links, leaves, inputs(row)["G"].to(F64), retain_graph=True)
    return {"links": links.detach(), "stats": stats, "dq": dq, "dk": dk, "dg": dg}


@functools.lru_cache(maxsize=None)
def reference(row):
    """the chunked band form on the row — computed once per process, shared, not to be modified"""
    return run64(row)


# ---------------------------------------------------------------------------------------------------------------- launch geometry

def mfma_tiles(L, TR, Lb, OT, transposed=False):
    """per owner tile of csrc/extract_links_mfma.hip: (o0, t0, t1, te) — live partner tiles [t0, t1), EMIT walks on to te"""
    out = []
    Lb = min(Lb, L)
    for ot in range((L + OT - 1) // OT):
        o0 = ot * OT
        pbeg = max(0, o0 - TR) if transposed else o0 + 1
        pend = min(o0 + OT - 1, Lb) if transposed else min(Lb, o0 + OT + TR)
        t0 = pbeg >> 5
        t1 = ((pend + 31) >> 5) if pend > pbeg else t0
        out.append((o0, t0, t1, max(t1, (o0 + OT + TR + 31) >> 5)))
    return out


def mfma_facts(row):
    """what the row reaches in the matrix-core kernels, from the launch arithmetic of xl_mfma_kernel restated"""
    L, TR = row.L, row.TR
    OT = 32 if L <= 1536 else 64
    facts = {"qg1" if OT == 32 else "qg2", "nq%d" % ((L + OT - 1) // OT)}
    if L > 1536:
        facts.add("triple_by_default")
    for Lb in row.lens:
        Lb = min(Lb, L)
        facts |= {"len32k-1"} if Lb % 32 == 31 else ({"len32k"} if Lb % 32 == 0 else ({"len32k+1"} if Lb % 32 == 1 else set()))
        for o0, t0, t1, te in mfma_tiles(L, TR, Lb, OT):
            nlive, nstep = t1 - t0, te - t0
            if nlive:
                facts |= {"nlive%d" % nlive, "live_odd" if nlive & 1 else "live_even"}
            facts.add("step_odd" if nstep & 1 else "step_even")
            if te > t1:
                facts.add("dead")
            for t in range(t0, t1):
                for grp in range(OT // 32):
                    omin, pmin = o0 + 32 * grp, 32 * t
                    dmin, dmax = pmin - (omin + 31) - 1, pmin + 31 - omin - 1
                    if dmax < 0 or dmin >= TR:
                        continue
                    facts.add("full" if dmin >= 0 and dmax < TR and pmin + 31 < Lb and omin + 31 < L else "partial")
        # the backward always runs 32-owner tiles; DK's partners are the sources
        for tr in (False, True):
            for o0, t0, t1, te in mfma_tiles(L, TR, Lb, 32, tr):
                if t1 - t0:
                    facts.add(("bwdT_" if tr else "bwd_") + ("odd" if (t1 - t0) & 1 else "even"))
    return facts


def xcd_map(B, L, OT):
    """workgroup id -> (XCD, sample, owner tile index) as xl_mfma_kernel maps them"""
    NQ = (L + OT - 1) // OT
    out = []
    for wg in range(NQ * B):
        if B % 8 == 0:
            c, sl = wg & 7, wg >> 3
            out.append((wg & 7, c + 8 * (sl // NQ), sl % NQ))
        else:
            out.append((wg & 7, wg // NQ, wg % NQ))
    return out


# ---------------------------------------------------------------------------------------------------------------- emulation

MUTANTS = ("lo_dropped", "first_tile_dropped", "last_tile_dropped", "band_edge", "mask_by_L", "bias_shift", "half_missing", "no_rescale",
           "three_products", "no_sa_term", "swap_b8", "g_leak")


def _f32(x):
    return torch.tensor(x, dtype=F32)


def _fma(a, b, c):
    """fp32 fma(a, b, c): the product of two fp32 is exact in double"""
    return (a.double() * b.double() + c.double()).to(F32)


def _exp2(x):
    return torch.exp2(x)


def _split16(x):
    hi = x.to(torch.float16)
    lo = ((x - hi.to(F32)) * 2048.0).to(torch.float16)
    return hi.to(F32), lo.to(F32)


def _trunc_bf16(x):
    return (x.contiguous().view(torch.int32) & -65536).view(F32)


def _triple(x):
    x1 = _trunc_bf16(x)
    r1 = x - x1
    x2 = _trunc_bf16(r1)
    x3 = _trunc_bf16(r1 - x2)
    return x1, x2, x3


SIX = ((0, 0), (1, 0), (0, 1), (2, 0), (1, 1), (0, 2))       # (piece of the partner row, piece of ds) in the kernel's order


def _scores(fam, qc, kb, bias_d, scale, mutant, owner="q"):
    """band scores [n,S,H] fp32 of source rows qc [n,H,CK] against their successors' rows kb [n,S,H,CK]; bias_d [S] or None.
    FMA family: natural-log scores; matrix cores: scores log2(e), the OWNER rows pre-multiplied by scale log2(e) before they are split
    (q in STATS / EMIT / SA / DQ, k in DK: the two differ in the last bits)"""
    n, S, _, CK = kb.shape
    if fam != "mfma":
        acc = torch.zeros(n, S, H, 4, dtype=F32)
        qd, kd = qc.double().unsqueeze(1), kb.double()
        for c in range(CK // 4):
            acc = (qd[..., 4 * c:4 * c + 4] * kd[..., 4 * c:4 * c + 4] + acc.double()).to(F32)
        s = ((acc[..., 0] + acc[..., 1]) + (acc[..., 2] + acc[..., 3])) * _f32(scale)
        return s if bias_d is None else s + bias_d.view(1, S, 1)
    sc2 = _f32(scale) * _f32(LOG2E)
    qh, ql = _split16(qc * sc2 if owner == "q" else qc)
    kh, kl = _split16(kb if owner == "q" else kb * sc2)
    qh, ql = qh.unsqueeze(1).double(), ql.unsqueeze(1).double()
    shh = torch.zeros(n, S, H, dtype=F32)
    slo = torch.zeros(n, S, H, dtype=F32)
    for c in range(CK // 16):                                    # one MFMA step = 16 channels, fp32 accumulators
        sl = slice(16 * c, 16 * c + 16)
        shh = ((kh[..., sl].double() * qh[..., sl]).sum(-1) + shh.double()).to(F32)
        slo = ((kl[..., sl].double() * qh[..., sl]).sum(-1) + slo.double()).to(F32)
        slo = ((kh[..., sl].double() * ql[..., sl]).sum(-1) + slo.double()).to(F32)
    s = shh if mutant == "lo_dropped" else _fma(slo, _f32(1.0 / 2048.0), shh)
    return s if bias_d is None else _fma(bias_d.view(1, S, 1), _f32(LOG2E), s)


def _state_fma(s, valid):
    """(max, log-sum) [n,H] over the valid slots, natural logarithms; (-inf, 0) without one"""
    sm = s.masked_fill(~valid.unsqueeze(-1), NEG)
    mx = sm.max(1).values
    dead = mx == NEG
    sm_ = (sm - mx.masked_fill(dead, 0.0).unsqueeze(1)).exp().sum(1)
    return mx, torch.where(dead, torch.zeros_like(mx), sm_.clamp_min(1e-38).log())


def _state_mfma(s2, valid, i0, mutant):
    """the STATS kernel: per lane half (partner bit 2) an online base-2 (max, sum) over the partner tiles of 32 walked from the far end,
    the halves merged at the end.  -> (max, log-sum) [n,H] in natural logarithms"""
    n, S, _ = s2.shape
    pp = torch.arange(i0, i0 + n).view(n, 1) + torch.arange(S).view(1, S) + 1
    tile, half = pp >> 5, (pp >> 2) & 1
    sm = s2.masked_fill(~valid.unsqueeze(-1), NEG)
    tv = tile.masked_fill(~valid, -1)
    tmax = tv.max(1).values                                      # the first tile walked, per source row
    tmin = tile.masked_fill(~valid, 1 << 30).min(1).values
    if mutant == "first_tile_dropped":
        sm = sm.masked_fill(((tile == tmax.view(n, 1)) & (tmax != tmin).view(n, 1)).unsqueeze(-1), NEG)
    if mutant == "last_tile_dropped":
        sm = sm.masked_fill(((tile == tmin.view(n, 1)) & (tmax != tmin).view(n, 1)).unsqueeze(-1), NEG)
    m = torch.full((2, n, H), NEG, dtype=F32)
    l = torch.zeros(2, n, H, dtype=F32)
    lo, hi = int(tile.min()), int(tile.max())
    for t in range(hi, lo - 1, -1):
        for g in (0, 1):
            sel = ((tile == t) & (half == g)).unsqueeze(-1)
            st = sm.masked_fill(~sel, NEG)
            m_new = torch.maximum(m[g], st.max(1).values)
            m_use = m_new.masked_fill(m_new == NEG, 0.0)
            ps = _exp2(st - m_use.unsqueeze(1)).sum(1)
            resc = torch.ones_like(l[g]) if mutant == "no_rescale" else _exp2(m[g] - m_use)
            l[g] = l[g] * resc + ps
            m[g] = m_new
    mm = torch.maximum(m[0], m[1])
    mu = mm.masked_fill(mm == NEG, 0.0)
    lt = l[0] * _exp2(m[0] - mu)
    if mutant != "half_missing":
        lt = lt + l[1] * _exp2(m[1] - mu)
    dead = mm == NEG
    return mm * _f32(LN2), torch.where(dead, torch.zeros_like(mm), lt.clamp_min(1e-38).log())


def emulate(row, contract=0, mutant=None):
    """{links, stats, dq, dk, dg} fp32 as the row's kernel family computes them (contract: 0 fp32 products, 1 bf16 triples; None = by size)"""
    c = inputs(row)
    fam, B, L, CK, TR = row.fam, row.B, row.L, row.CK, row.TR
    if contract is None:
        contract = 1 if L > 1536 else 0
    mf = fam == "mfma"
    scale = float(_f32(float(CK) ** -0.5))
    S = TR + 1 if mutant == "band_edge" else TR                   # band_edge: the window takes d <= TR into its soft-max
    links = torch.full((B, L, TR), NEG, dtype=F32)
    stats = torch.zeros(B, L, H, 2, dtype=F32)
    dq, dk, dg = torch.zeros(B, L, H, CK, dtype=F32), torch.zeros(B, L, H, CK, dtype=F32), torch.zeros(B, L, H, dtype=F32)
    bias = c["bias"]
    bias_d = None
    if bias is not None:
        di = torch.arange(S).clamp(max=TR - 1)
        if mutant == "bias_shift":
            di = (di + 1).clamp(max=TR - 1)
        bias_d = bias[di]
    nrow = max(1, 8192 // S)
    for b in range(B):
        Lb = L if mutant == "mask_by_L" else min(L, int(c["olen"][b]))
        q, k, lg, G = c["q"][b], c["k"][b], c["lg"][b], c["G"][b]
        for i0 in range(0, L, nrow):
            i1 = min(L, i0 + nrow)
            n = i1 - i0
            j = torch.arange(i0, i1).view(n, 1) + torch.arange(S).view(1, S) + 1
            valid = j < Lb
            jc = j.clamp(max=L - 1)
            kb = k[jc]                                           # [n,S,H,CK]
            s = _scores(fam, q[i0:i1], kb, bias_d, scale, mutant)
            mx, ls = _state_mfma(s, valid, i0, mutant) if mf else _state_fma(s, valid)
            stats[b, i0:i1, :, 0], stats[b, i0:i1, :, 1] = mx, ls
            dead = (mx == NEG).unsqueeze(1)
            gt = lg[i0:i1]
            vT = valid[:, :TR].unsqueeze(-1)
            if mf:
                ca = (((gt - mx) - ls) * _f32(LOG2E)).masked_fill(dead.squeeze(1), 0.0).unsqueeze(1)
                cp = (-(mx + ls) * _f32(LOG2E)).masked_fill(dead.squeeze(1), 0.0).unsqueeze(1)
                v = (s[:, :TR] + ca).masked_fill(~vT, NEG)
                m2 = v.max(-1).values
                e = _exp2(v - m2.masked_fill(m2 == NEG, 0.0).unsqueeze(-1)).sum(-1)
                lk = torch.where(m2 == NEG, m2, (m2 + e.clamp_min(1e-38).log2()) * _f32(LN2))
            else:
                lsm = ((s[:, :TR] - mx.unsqueeze(1)) - ls.unsqueeze(1))
                v = (lsm + gt.unsqueeze(1)).masked_fill(~vT, NEG)
                m2 = v.max(-1).values
                e = (v - m2.masked_fill(m2 == NEG, 0.0).unsqueeze(-1)).exp().sum(-1)
                lk = torch.where(m2 == NEG, m2, m2 + e.clamp_min(1e-38).log())
            links[b, i0:i1] = lk
            # ---- backward: A = G exp(ls + gate - links), SA = sum_d A, ds = A - exp(ls) SA
            Gc = G[i0:i1]
            if mf:
                w = _exp2(((s[:, :TR] + ca) - (lk * _f32(LOG2E)).unsqueeze(-1)).masked_fill(~vT, NEG))
                p = _exp2((s[:, :TR] + cp).masked_fill(~vT, NEG))
            else:
                w = ((lsm + gt.unsqueeze(1)) - lk.unsqueeze(-1)).masked_fill(~vT, NEG).exp()
                p = lsm.masked_fill(~vT, NEG).exp()
            if mutant == "g_leak":
                A = Gc.unsqueeze(-1) * w                          # 0 x NaN at a masked slot
            else:
                A = torch.where(vT, Gc.masked_fill(~valid[:, :TR], 0.0).unsqueeze(-1) * w, torch.zeros_like(w))
            sa = A.sum(1)
            ds = A if mutant == "no_sa_term" else (A.double() - p.double() * sa.unsqueeze(1).double()).to(F32)
            dg[b, i0:i1] = sa
            dsT = ds
            if mf:
                # DK recomputes the scores with k as the owner and takes SA from the first pass
                sT = _scores(fam, q[i0:i1], kb[:, :TR], None if bias_d is None else bias_d[:TR], scale, mutant, owner="k")
                wT = _exp2(((sT + ca) - (lk * _f32(LOG2E)).unsqueeze(-1)).masked_fill(~vT, NEG))
                pT = _exp2((sT + cp).masked_fill(~vT, NEG))
                AT = Gc.unsqueeze(-1) * wT if mutant == "g_leak" else torch.where(vT, Gc.masked_fill(~valid[:, :TR], 0.0).unsqueeze(-1) * wT, torch.zeros_like(wT))
                dsT = AT if mutant == "no_sa_term" else (AT.double() - pT.double() * sa.unsqueeze(1).double()).to(F32)
            kbT, jT = kb[:, :TR], jc[:, :TR].reshape(-1)
            qc = q[i0:i1]
            if mf and contract:
                pairs = SIX[:3] if mutant == "three_products" else SIX
                d3, dT3, k3, q3 = _triple(ds), _triple(dsT), _triple(kbT), _triple(qc)
                accq = torch.zeros(n, H, CK, dtype=F32)
                T = torch.zeros(n, TR, H, CK, dtype=F32)
                for px, pd in pairs:
                    accq = accq + torch.einsum("ndh,ndhc->nhc", d3[pd], k3[px])
                    T = T + dT3[pd].unsqueeze(-1) * q3[px].unsqueeze(1)
            else:
                accq = torch.einsum("ndh,ndhc->nhc", ds, kbT)
                T = dsT.unsqueeze(-1) * qc.unsqueeze(1)
            dq[b, i0:i1] = accq * _f32(scale)
            dk[b].index_add_(0, jT, T.reshape(n * TR, H, CK))
        dk[b] *= _f32(scale)
    out = {"links": links, "stats": stats, "dq": dq, "dk": dk, "dg": dg}
    if mutant == "swap_b8":
        perm = torch.arange(B) ^ 8
        out = {n: t[perm] for n, t in out.items()}
    return out


@functools.lru_cache(maxsize=None)
def emulation(row, contract):
    """the unmutated emulation of the row — computed once per process, shared, not to be modified"""
    return emulate(row, contract)


# ---------------------------------------------------------------------------------------------------------------- errors and the bound

def slices(name, t):
    """the tensor as [slices, elements]: links, dg per sample; stats, dq, dk per (sample, head)"""
    B = t.shape[0]
    if name in ("links", "dg"):
        return t.reshape(B, -1)
    return t.transpose(1, 2).reshape(B * H, -1)                  # [B,L,H,..] -> [B,H,L,..]


def slice_errors(name, got, ref):
    """(err, scale) [slices] float64: largest |got - ref| over the entries finite in ref and the slice's largest |ref|; a slice whose -inf
    pattern differs from the reference's, or that holds a NaN or an infinity where the reference is finite, has err = inf"""
    g, r = slices(name, got.double()), slices(name, ref.double())
    fin = torch.isfinite(r)
    bad = ((torch.isneginf(g) != torch.isneginf(r)) | (fin & ~torch.isfinite(g))).any(1)
    z = torch.zeros_like(r)
    err = torch.where(fin, (g - r).abs(), z).nan_to_num(nan=math.inf, posinf=math.inf).max(1).values
    scale = torch.where(fin, r.abs(), z).max(1).values
    return err.masked_fill(bad, math.inf), scale


def bound(err_ref, scale):
    """min(8 err_ref + 4 2^-23 scale, 2e-5 scale) per slice"""
    return torch.minimum(8.0 * err_ref + 4.0 * ULP * scale, CAP * scale)


def void_gradients(row):
    """TR = 1: every window has one slot, its soft-max is 1 whatever q and k are, so dq and dk are identically zero (the float64 reference
    gives exact zeros).  The kernels form ds = A - p SA from A = G exp(..) and p = exp2(score - state) = 1 +- a few ulps, so what they
    leave is rounding of size ulp |A| |partner row| and no reference magnitude exists to hold it against.  For these two tensors of such a
    row the scale is that of the terms instead: the largest |grad_links| times the largest |q| or |k| entry times 1 / sqrt(CK)."""
    return ("dq", "dk") if row.TR == 1 else ()


def term_scale(row):
    c = inputs(row)
    G = c["G"][~c["invalid"]]
    return float(G.abs().max()) * max(float(c["q"].abs().max()), float(c["k"].abs().max())) * float(row.CK) ** -0.5


def judge(name, got, emu, ref, void_scale=None):
    """(ok, worst err / bound, err, bound, scale, err_ref) of one output tensor against the bound its emulation's error allows"""
    err, scale = slice_errors(name, got, ref)
    err_ref, _ = slice_errors(name, emu, ref)
    if void_scale is not None:
        assert not ref.any()
        scale = torch.full_like(scale, void_scale)
    bd = bound(err_ref, scale)
    ratio = torch.where(err <= bd, err / bd.clamp_min(1e-300), torch.full_like(err, math.inf))
    ratio = torch.where((err == 0) & (bd == 0), torch.zeros_like(err), ratio)
    return bool((err <= bd).all()), float(ratio.max()), err, bd, scale, err_ref


def figures(name, got, emu, ref, void_scale=None):
    """one line for the record: the worst slice of the tensor"""
    ok, ratio, err, bd, scale, err_ref = judge(name, got, emu, ref, void_scale)
    r = torch.where(bd > 0, err / bd.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    w = int(torch.argmax(r.nan_to_num(nan=math.inf)))            # the slice that uses most of its bound (or misses it by most)
    return (f"{name}: worst slice {w}: err {float(err[w]):.3e} scale {float(scale[w]):.3e} err_ref {float(err_ref[w]):.3e} bound {float(bd[w]):.3e}"
            f"  (largest err / bound {ratio:.3f}){'' if ok else '  OUTSIDE'}")
