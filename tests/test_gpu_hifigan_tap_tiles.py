"""The fp32 fused ResBlock unit (csrc/hifigan_conv_f32.hip, hifigan_resunit_f32_kernel) at the edges of its TAP-AWARE time tile.

A unit computes c1 over NTI intermediate columns (the compiled instance) and stores NT <= NTI - 2 h2 of them, h2 = (ntaps - 1) / 2.  The rule
of hgs_unit_tile, restated in unit_tile() below: every instance offers NT = NTI - 2 h2 and, where one wave column spans the tile
(C >= 128), NT = NTI - 16 with one 16-column c2 step fewer; the tile is the one with the fewest (c1 + c2) steps per stored column among
those whose LDS keeps the stage's residency (80 KB at C = 128 and C = 32, 160 KB elsewhere), the wider instance on a tie.

For every V1 (C, ntaps, dilation): B = 2, T in {NT - 1, NT, NT + 1, 2 NT + 3}, with and without per-sample lengths [T, T - h1 - h2 - 1], STORE and
ACCUM at scale 1/3, through _unit_case of tests/test_gpu_hifigan_layers.py — its assertions and its tolerance, unchanged:
  (b) torch.equal with the two one-record launches the unit replaces (rows below each sample's length), and each of those two steps
      within SPLIT + 3 max(e32, 2^-24) of the fp64 reference of tests/util_hifigan_ref.py;
  (a) the unit against the fp64 reference within the bound _unit_bound carries through both convolutions.
"""
import pytest
import torch

from tests.test_gpu_hifigan_layers import DEV, Worst, _unit_case

KS, DILS, CS = (3, 7, 11), (1, 3, 5), (32, 64, 128, 256)
INSTANCES = {256: (64,), 128: (128, 112, 96), 64: (256,), 32: (512,)}        # NTI of the compiled instances, widest first
RESIDENT = {256: 160 * 1024, 128: 80 * 1024, 64: 160 * 1024, 32: 80 * 1024}


def unit_lds(C, nti, nt, h1):
    return max((nti + 2 * h1) * C * 4, (nti + 16) * C * 4, nt * (C + 4) * 4)


def unit_tile(C, K, dil):
    """(NTI, NT) by the documented rule."""
    h1, h2 = dil * (K - 1) // 2, (K - 1) // 2
    for budget in (RESIDENT[C], 160 * 1024):
        best = None
        for nti in INSTANCES[C]:
            for trim in ((0, 1) if C >= 128 else (0,)):
                nt = nti - 16 if trim else nti - 2 * h2
                steps = 2 * (nti // 16) - trim
                if nt < 1 or nt + 2 * h2 > nti or unit_lds(C, nti, nt, h1) > budget:
                    continue
                if best is None or steps * best[1] < best[2] * nt:
                    best = (nti, nt, steps)
        if best:
            return best[:2]
    return None


def test_rule_gives_the_documented_v1_tiles():
    """The widths the kernel's comment and DESIGN name: k = 11 keeps the tap-blind tile where one wave column spans it."""
    for d in DILS:
        assert [unit_tile(256, k, d) for k in KS] == [(64, 62), (64, 58), (64, 48)]
        assert [unit_tile(128, k, d) for k in KS] == [(128, 126), (128, 122), (128, 112) if d < 5 else (96, 80)]
        assert [unit_tile(64, k, d) for k in KS] == [(256, 254), (256, 250), (256, 246)]
        assert [unit_tile(32, k, d) for k in KS] == [(512, 510), (512, 506), (512, 502)]
    assert unit_tile(128, 11, 4) == (112, 96) and unit_tile(128, 9, 5) == (112, 104)


CASES = [(C, K, d) for C in CS for K in KS for d in DILS]


@pytest.mark.gpu
@pytest.mark.parametrize("C,K,dil", CASES, ids=[f"{c}-{k}-{d}" for c, k, d in CASES])
def test_unit_f32_at_tap_tile_edges(C, K, dil):
    from daspeech_amd import _lib
    assert _lib.load().dsp_hifigan_resunit_f32_supported(C, K, dil)
    h1, h2 = dil * (K - 1) // 2, (K - 1) // 2
    NT = unit_tile(C, K, dil)[1]
    worst, n = Worst(f"unit fp32 tap tile C={C} K={K} dil={dil} (NT {NT})"), 0
    for T in (NT - 1, NT, NT + 1, 2 * NT + 3):
        short = T - h1 - h2 - 1
        assert short > 0
        for accumulate in (0, 1):
            _unit_case(11000 + 13 * n + C + K, False, 2, T, C, K, dil, accumulate, worst)
            _unit_case(12000 + 13 * n + C + K, False, 2, T, C, K, dil, accumulate, worst,
                       lens=torch.tensor([T, short], device=DEV, dtype=torch.int32), T0=T)
            n += 1
    worst.report()
