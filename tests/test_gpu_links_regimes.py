"""The fp32 link kernels — csrc/extract_links.hip (one-image and tiled fp32-FMA kernels) and csrc/extract_links_mfma.hip (matrix cores, both
owner-tile sizes, both contraction modes) — against the float64 reference of tests/util_links_regimes.py, row by row of its case table,
launched through the C entry points alone (dsp_extract_links, _train, _bwd; dsp_extract_links_ws, _bwd_ws with the workspace
dsp_extract_links_workspace asks for).

Every output buffer starts NaN-filled, the workspace has exactly the bytes asked for with a NaN guard behind it, the pins are restored in
`finally`, and dsp_extract_links_debug_ran() must name exactly the family of the row after every call.

Patterns: the -inf pattern of the links is the reference's, no NaN anywhere, stats are (-inf, 0) on rows without a successor, dq / dk / dgate
are exact zeros at and beyond the sample's length, inference and training forward are bit-equal, a second identical call is bit-equal.
Accuracy, per slice on the slice's own scale (links, dgate per sample; stats, dq, dk per (sample, head)):
    err <= min(8 err_ref + 4 2^-23 scale, 2e-5 scale)
with err_ref the error of the CPU emulation of the family's arithmetic against the same reference — nothing in the allowance comes from a
kernel.  tests/test_links_regimes_ref.py shows on the CPU that this bound holds a right kernel and rejects a subtly wrong one on these rows.
`planted` rows carry NaN, +inf and -inf in grad_links at the slots beyond the graph: the gradients must not see them.
Figures: `pytest -s`; one full run is kept in profiles/links_regimes.txt."""
import ctypes

import pytest
import torch

from tests import util_links_regimes as U

pytestmark = pytest.mark.gpu

FWD_BIT = {"one": 1, "tiled": 2, "mfma": 4}
BWD_BIT = {"one": 8, "tiled": 16}
GUARD = 1024                                      # floats behind the workspace
_DEVICE_ERROR = []                                # a launch or a synchronisation that raised: nothing of this module touches the device after it


def dev():
    return torch.device("cuda:0")


def _L():
    from daspeech_amd import _lib
    return _lib


def _ran():
    torch.cuda.synchronize()
    return int(_L().load().dsp_extract_links_debug_ran())


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev())


def _bits(t):
    return t.view(torch.int32)


def _workspace(row, phase):
    """(buffer of exactly the bytes dsp_extract_links_workspace asks for + a guard, NaN-filled; the byte count)"""
    n = ctypes.c_size_t(0)
    _L().check(_L().load().dsp_extract_links_workspace(row.B, row.L, U.H, row.CK, row.TR, phase, ctypes.byref(n)), "dsp_extract_links_workspace")
    if row.fam != "mfma":
        assert n.value == 0, "xl_mfma 0: the fp32-FMA kernels serve the call, no workspace"
        return None, 0
    assert n.value > 0 and n.value % 4 == 0
    return _nan(n.value // 4 + GUARD), n.value


def _guard_intact(ws, n):
    return bool(torch.isnan(ws[n // 4:]).all())


class _Device:
    """the row's tensors on the device and the launches of its family"""

    def __init__(self, row):
        self.row = row
        c = U.inputs(row)
        self.q, self.k, self.lg, self.G = (c[n].to(dev()).contiguous() for n in ("q", "k", "lg", "G"))
        self.olen = c["olen"].to(dev())
        self.bias = None if c["bias"] is None else c["bias"].to(dev())
        self.dims = (row.B, row.L, U.H, row.CK, row.TR, float(row.CK) ** -0.5)

    def forward(self, training):
        """links (and stats) from NaN-filled buffers; asserts the family that ran and the workspace guard"""
        row, lib, P, L_ = self.row, _L().load(), _L().ptr, _L()
        B, L = row.B, row.L
        links = _nan(B, L, row.TR)
        stats = _nan(B, L, U.H, 2) if training else None
        ws, n = _workspace(row, 1 if training else 0)
        st = L_.current_stream_handle()
        _ran()
        if row.fam == "mfma":
            L_.check(lib.dsp_extract_links_ws(P(self.q), P(self.k), P(self.lg), P(self.olen), P(self.bias), P(links), P(stats), *self.dims, P(ws), n, st),
                     "dsp_extract_links_ws")
        elif training:
            L_.check(lib.dsp_extract_links_train(P(self.q), P(self.k), P(self.lg), P(self.olen), P(self.bias), P(links), P(stats), *self.dims, st),
                     "dsp_extract_links_train")
        else:
            L_.check(lib.dsp_extract_links(P(self.q), P(self.k), P(self.lg), P(self.olen), P(self.bias), P(links), *self.dims, st), "dsp_extract_links")
        bits = _ran()
        assert bits == FWD_BIT[row.fam], f"forward: families {bits:#b} ran, the row names {FWD_BIT[row.fam]:#b}"
        assert ws is None or _guard_intact(ws, n), "the forward wrote behind its workspace"
        return links, stats

    def backward(self, links, stats, contract):
        row, lib, P, L_ = self.row, _L().load(), _L().ptr, _L()
        dq, dk, dg = _nan(*self.q.shape), _nan(*self.k.shape), _nan(*self.lg.shape)
        ws, n = _workspace(row, 2)
        st = L_.current_stream_handle()
        _ran()
        if row.fam == "mfma":
            L_.check(lib.dsp_extract_links_bwd_ws(P(self.q), P(self.k), P(self.lg), P(self.olen), P(self.bias), P(links), P(self.G), P(stats),
                                                  P(dq), P(dk), P(dg), *self.dims, P(ws), n, st), "dsp_extract_links_bwd_ws")
            triple = contract == 1 or (contract is None and row.L > 1536)
            want = 64 if triple else 32
        else:
            L_.check(lib.dsp_extract_links_bwd(P(self.q), P(self.k), P(self.lg), P(self.olen), P(self.bias), P(links), P(self.G), P(stats),
                                               P(dq), P(dk), P(dg), *self.dims, st), "dsp_extract_links_bwd")
            want = BWD_BIT[row.fam]
        bits = _ran()
        assert bits == want, f"backward: families {bits:#b} ran, the row names {want:#b}"
        assert ws is None or _guard_intact(ws, n), "the backward wrote behind its workspace"
        return dq, dk, dg


def _patterns(row, ref, links, inf_links, stats, links2, stats2):
    neg = torch.isneginf(ref["links"])
    lk, st = links.cpu(), stats.cpu()
    assert not torch.isnan(lk).any() and not torch.isnan(st).any(), "a cell the forward did not write (or a NaN it computed)"
    assert torch.equal(torch.isneginf(lk), neg) and torch.isfinite(lk[~neg]).all(), "the -inf pattern of the links"
    assert torch.equal(_bits(inf_links), _bits(links)), "inference and training forward differ"
    assert torch.equal(_bits(links2), _bits(links)) and torch.equal(_bits(stats2), _bits(stats)), "a second identical forward differs"
    dead = torch.isneginf(ref["stats"][..., 0])
    assert torch.equal(torch.isneginf(st[..., 0]), dead) and torch.isfinite(st[..., 0][~dead]).all() and torch.isfinite(st[..., 1]).all()
    assert bool((st[..., 1][dead] == 0).all()), "stats of a row without a successor are (-inf, 0)"


def _judge(row, contract, ref, got, tag):
    emu = U.emulation(row, contract)
    bad = []
    for n in U.NAMES:
        if n not in got:
            continue
        vs = U.term_scale(row) if n in U.void_gradients(row) else None
        ok = U.judge(n, got[n], emu[n], ref[n], vs)[0]
        print(f"{row.id} {tag}: {U.figures(n, got[n], emu[n], ref[n], vs)}")
        if not ok:
            bad.append(n)
    return bad


@pytest.mark.parametrize("rid", U.IDS)
def test_link_kernels_against_float64(rid):
    row = U.ROW[rid]
    ref = U.reference(row)
    L_ = _L()
    bad = []
    assert not _DEVICE_ERROR, f"not run: the device reported an error in {_DEVICE_ERROR[0]}"
    try:
        L_.set_option("xl_mfma", 1 if row.fam == "mfma" else 0)
        L_.set_option("xl_tile", row.tile)
        L_.set_option("xl_contract", -1)
        d = _Device(row)
        inf_links, _ = d.forward(False)
        links, stats = d.forward(True)
        links2, stats2 = d.forward(True)
        _patterns(row, ref, links, inf_links, stats, links2, stats2)
        fwd = {"links": links.cpu(), "stats": stats.cpu()}
        contracts = row.contract if row.fam == "mfma" else (0,)
        bad += [("forward", n) for n in _judge(row, contracts[0], ref, fwd, "forward")]
        for ct in contracts:
            L_.set_option("xl_contract", -1 if ct is None else ct)
            dq, dk, dg = d.backward(links, stats, ct)
            again = d.backward(links, stats, ct)
            got = {"dq": dq.cpu(), "dk": dk.cpu(), "dg": dg.cpu()}
            tag = "backward" + (f" (contraction {'by size' if ct is None else ct})" if row.fam == "mfma" else "")
            for n, t in got.items():
                assert not torch.isnan(t).any() and torch.isfinite(t).all(), f"{tag}: {n} holds a NaN or an infinity"
            for (n, t), t2 in zip(got.items(), again):
                assert torch.equal(_bits(t), _bits(t2.cpu())), f"{tag}: a second identical call differs in {n}"
            for b, m in enumerate(row.lens):
                assert not got["dq"][b, m:].any() and not got["dk"][b, m:].any() and not got["dg"][b, m:].any(), \
                    f"{tag}: a gradient at or beyond the length of sample {b}"
            bad += [(tag, n) for n in _judge(row, ct, ref, got, tag)]
    except AssertionError:
        raise
    except Exception:
        _DEVICE_ERROR.append(rid)
        raise
    finally:
        L_.set_option("xl_mfma", -1)
        L_.set_option("xl_tile", 0)
        L_.set_option("xl_contract", -1)
    assert not bad, f"outside the bound: {bad}"


def test_planted_gradients_through_the_double_kernels():
    """csrc/extract_links_f64.hip on a `planted` row, at that family's tolerances (tests/test_gpu_links_double.py): NaN and infinities in
    grad_links beyond the graph reach no gradient"""
    from daspeech_amd import decode_ops as D
    row = U.ROW["mc-B6-TR159-planted"]
    assert not _DEVICE_ERROR, f"not run: the device reported an error in {_DEVICE_ERROR[0]}"
    c, ref = U.inputs(row), U.reference(row)
    bias = None if c["bias"] is None else c["bias"].double().to(dev())
    _ran()
    qd, kd, gd, ol, bias, links, stats = D._links_f64_forward(c["q"].double().to(dev()), c["k"].double().to(dev()), c["lg"].double().to(dev()),
                                                               c["olen"].to(dev()), row.TR, bias, True)
    G = c["G"].to(dev())
    assert not torch.isfinite(G[c["invalid"].to(dev())]).any()
    dq, dk, dg = D._links_f64_backward(qd, kd, gd, ol, bias, links, stats, G, row.TR)
    assert _ran() == (1 << 7) | (1 << 8)
    assert torch.equal(torch.isneginf(links).cpu(), torch.isneginf(ref["links"]))
    fin = torch.isfinite(ref["links"])
    torch.testing.assert_close(links.cpu()[fin], ref["links"][fin], rtol=1e-12, atol=1e-12)
    for n, t in (("dq", dq), ("dk", dk), ("dg", dg)):
        assert torch.isfinite(t).all(), n
        print(f"double kernels, planted: {n} max abs error {float((t.cpu() - ref[n]).abs().max()):.3e} (largest value {float(ref[n].abs().max()):.3e})")
        torch.testing.assert_close(t.cpu(), ref[n], rtol=1e-9, atol=1e-12, msg=lambda m: f"{n}: {m}")
    for b, m in enumerate(row.lens):
        assert not dq[b, m:].any() and not dk[b, m:].any() and not dg[b, m:].any()
