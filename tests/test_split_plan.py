"""Launch plan of the split-operand Conv1d / Linear kernel (csrc/conv1d_split.hip: cs_plan, asked through dsp_conv1d_split_plan — host
arithmetic, no device call): how many rows one launch tiles, how many row tiles and output-channel tiles it has, and into how many
contiguous ranges a row tile's output tiles are divided (one workgroup per range: it stages the rows once and runs its tiles from them).

Pinned here, for a device of 256 CUs:
  * the plan of the S2ST workload's launches (B = 32; T = 200 Conformer encoder, 394 NAT decoder, 483 FastSpeech2 decoder);
  * ranges partition the output tiles: equal lengths, every tile in exactly one range; their number is the one with the fewest K-steps
    on a CU's critical path — rounds of resident workgroups x (1 for staging + tiles per range x taps) — and among equals the largest;
  * only a dense one-tap, one-slice launch without split-K is tiled over the B * T rows, and only where that fits one round of resident
    workgroups or saves a round (never in the <256,128,64> instance); multi-slice, split-K and `lens` launches keep one launch row per
    (sample, frame) and — multi-slice, split-K — one output tile per workgroup;
  * the instance (output-tile width, row-tile height) is the one cs_run has always chosen from the caller's (B, T): tiling the rows
    as one sequence does not change it.
"""
import ctypes

import pytest

CUS = 256


@pytest.fixture(scope="module")
def plan():
    from daspeech_amd import _lib, build
    build.build()
    fn = _lib.load().dsp_conv1d_split_plan
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int] * 10 + [ctypes.POINTER(ctypes.c_int)]

    def ask(B, T, CI, nslices, M, ntaps, has_lens=0, has_ln=0, tap_groups=0, n_cus=CUS):
        out = (ctypes.c_int * 6)()
        rc = fn(B, T, CI, nslices, M, ntaps, has_lens, has_ln, tap_groups, n_cus, out)
        assert rc == 0, (B, T, CI, nslices, M, ntaps, has_lens, has_ln, tap_groups, n_cus)
        return dict(rows=out[0], row_tiles=out[1], m_tiles=out[2], ranges=out[3], MT=out[4], NT=out[5])
    return ask


def ceil_div(a, b):
    return -(-a // b)


# (name, arguments, rows per launch, row tiles, output tiles, ranges, MT, NT)
WORKLOAD = [
    # NAT decoder, T = 394: 12 608 rows = 197 tiles of 64 (224 tiled per sample)
    ("decoder fc1 512->2048, lens", dict(B=32, T=394, CI=512, nslices=1, M=2048, ntaps=1, has_lens=1), 394, 224, 8, 1, 256, 64),
    ("decoder q|k|v 512->1536, lens", dict(B=32, T=394, CI=512, nslices=1, M=1536, ntaps=1, has_lens=1), 394, 224, 6, 1, 256, 64),
    ("decoder 512->512, lens", dict(B=32, T=394, CI=512, nslices=1, M=512, ntaps=1, has_lens=1), 394, 224, 2, 1, 256, 64),
    ("decoder fc1 512->2048, dense", dict(B=32, T=394, CI=512, nslices=1, M=2048, ntaps=1), 12608, 197, 8, 1, 256, 64),
    ("decoder 512->512, dense", dict(B=32, T=394, CI=512, nslices=1, M=512, ntaps=1), 12608, 197, 2, 1, 256, 64),
    ("decoder fc2 2048->512 (4 slices)", dict(B=32, T=394, CI=512, nslices=4, M=512, ntaps=1), 394, 224, 2, 2, 256, 64),
    # Conformer encoder, T = 200: 6 400 rows = 100 tiles of 64 (128 tiled per sample)
    ("encoder q|k|v 256->768, LayerNorm staged", dict(B=32, T=200, CI=256, nslices=1, M=768, ntaps=1, has_ln=1), 200, 128, 3, 3, 256, 64),
    ("encoder pointwise_conv1 256->512, LayerNorm staged", dict(B=32, T=200, CI=256, nslices=1, M=512, ntaps=1, has_ln=1), 6400, 100, 2, 2, 256, 64),
    ("encoder 256->256", dict(B=32, T=200, CI=256, nslices=1, M=256, ntaps=1), 200, 128, 2, 2, 128, 64),
    # FastSpeech2 decoder, T = 483, ragged (lens): rows stay per sample
    ("FFT conv 256->1024 K=9, lens", dict(B=32, T=483, CI=256, nslices=1, M=1024, ntaps=9, has_lens=1), 483, 128, 4, 2, 256, 128),
    ("FFT conv 256->1024 K=9, dense", dict(B=32, T=483, CI=256, nslices=1, M=1024, ntaps=9), 483, 128, 4, 2, 256, 128),
    ("FFT conv 1024->256 K=9 (2 slices), lens", dict(B=32, T=483, CI=512, nslices=2, M=256, ntaps=9, has_lens=1), 483, 256, 1, 1, 256, 64),
    ("FFT q|k|v 256->768, lens", dict(B=32, T=483, CI=256, nslices=1, M=768, ntaps=1, has_lens=1), 483, 128, 3, 3, 256, 128),
]


@pytest.mark.parametrize("name,kw,rows,row_tiles,m_tiles,ranges,MT,NT", WORKLOAD, ids=[w[0] for w in WORKLOAD])
def test_workload_launch_plans(plan, name, kw, rows, row_tiles, m_tiles, ranges, MT, NT):
    got = plan(**kw)
    assert got == dict(rows=rows, row_tiles=row_tiles, m_tiles=m_tiles, ranges=ranges, MT=MT, NT=NT), (name, got)


SWEEP = [dict(B=B, T=T, CI=CI, nslices=ns, M=M, ntaps=K, has_lens=hl, tap_groups=tg)
         for B in (1, 3, 32) for T in (13, 63, 65, 200, 394, 483) for CI in (128, 256, 512) for ns in (1, 2, 4)
         for M in (256, 512, 520, 768, 1024, 1536, 2048) for K in (1, 3, 9) for hl in (0, 1) for tg in (0, 1, 3) if tg <= K and not (tg == 1 and ns == 1)]


def resident(kw, g, cus):
    """workgroups the device holds at once: two per CU in <256,128,64> (4 waves per SIMD) while the LDS tiles allow, else one"""
    lds = 2 * (g["NT"] + kw["ntaps"] - 1) * kw["CI"] * 2
    return cus * (2 if (g["MT"], g["NT"]) == (128, 64) and 2 * lds <= 160 * 1024 else 1)


def best_ranges(row_tiles, m_tiles, ntaps, res):
    """(ranges, rounds): fewest K-steps on a CU's critical path, among equals the most ranges"""
    cost = {r: ceil_div(row_tiles * r, res) * (1 + (m_tiles // r) * ntaps) for r in range(1, m_tiles + 1) if m_tiles % r == 0}
    r = max(r for r in cost if cost[r] == min(cost.values()))
    return r, ceil_div(row_tiles * r, res)


def test_ranges_cover_every_output_tile_exactly_once(plan):
    for kw in SWEEP:
        for cus in (1, 64, 256, 304):
            g = plan(n_cus=cus, **kw)
            assert g["m_tiles"] == ceil_div(kw["M"], g["MT"]), (kw, g)
            assert 1 <= g["ranges"] <= g["m_tiles"] and g["m_tiles"] % g["ranges"] == 0, (kw, cus, g)      # equal lengths
            per = g["m_tiles"] // g["ranges"]
            owned = [m for r in range(g["ranges"]) for m in range(r * per, min((r + 1) * per, g["m_tiles"]))]
            assert owned == list(range(g["m_tiles"])), (kw, cus, g)
            if kw["nslices"] > 1 or kw["tap_groups"] > 0:            # the staged rows are not the whole reduction: one tile per workgroup
                assert g["ranges"] == g["m_tiles"], (kw, cus, g)
            else:
                assert g["ranges"] == best_ranges(g["row_tiles"], g["m_tiles"], kw["ntaps"], resident(kw, g, cus))[0], (kw, cus, g)
    # a pure function of its arguments
    assert plan(**SWEEP[7]) == plan(**SWEEP[7])


def test_only_dense_one_tap_one_slice_launches_tile_the_batch_rows(plan):
    for kw in SWEEP:
        g = plan(**kw)
        flat = kw["ntaps"] == 1 and kw["nslices"] == 1 and not kw["has_lens"] and kw["tap_groups"] == 0 and (g["MT"], g["NT"]) != (128, 64)
        if flat:
            res = resident(kw, g, CUS)
            rounds_flat = best_ranges(ceil_div(kw["B"] * kw["T"], g["NT"]), g["m_tiles"], 1, res)[1]
            rounds = best_ranges(kw["B"] * ceil_div(kw["T"], g["NT"]), g["m_tiles"], 1, res)[1]
            flat = rounds_flat == 1 or rounds_flat < rounds
        if flat:
            assert g["rows"] == kw["B"] * kw["T"] and g["row_tiles"] == ceil_div(kw["B"] * kw["T"], g["NT"]), (kw, g)
        else:
            assert g["rows"] == kw["T"] and g["row_tiles"] == kw["B"] * ceil_div(kw["T"], g["NT"]), (kw, g)


def test_instance_choice_is_the_callers_b_and_t(plan):
    """(MT, NT) against cs_run's rule as tests/test_gpu_split_addressing.py restates it: from the caller's (B, T), whether or not the rows
    are then tiled as one sequence."""
    from tests.test_gpu_split_addressing import cs_instance
    for kw in SWEEP:
        mode = "ksplit:%d" % kw["tap_groups"] if kw["tap_groups"] else "plain"
        want = cs_instance(kw["CI"], kw["nslices"], kw["M"], kw["ntaps"], kw["B"], kw["T"], mode)
        g = plan(**kw)
        assert (g["MT"], g["NT"]) == (want[1], want[2]), (kw, g, want)
    for B, T, M in ((3, 70, 768), (32, 200, 768), (1, 6400, 768)):
        g = plan(B=B, T=T, CI=256, nslices=1, M=M, ntaps=1, has_ln=1)
        assert (g["MT"], g["NT"]) == (256, 64), (B, T, g)                # the LayerNorm-staged instance, always
    # same rows, different batch shape: the instance follows (B, T), the rows per launch do not
    a = plan(B=32, T=200, CI=256, nslices=1, M=1024, ntaps=1)          # 2 x 4 x 32 = 256 workgroups at 128 rows: the 128-row tiles
    b = plan(B=1, T=6400, CI=256, nslices=1, M=1024, ntaps=1)          # 50 x 4 = 200: the 64-row tiles
    assert a["rows"] == b["rows"] == 6400 and (a["MT"], a["NT"]) == (256, 128) and (b["MT"], b["NT"]) == (256, 64)
    assert a["row_tiles"] == 50                                         # 6 400 rows as one sequence, in the instance of (32, 200)


def test_plan_refuses_what_the_kernel_does_not_serve(plan):
    from daspeech_amd import _lib
    fn = _lib.load().dsp_conv1d_split_plan
    out = (ctypes.c_int * 6)()
    assert fn(2, 10, 96, 1, 256, 1, 0, 0, 0, CUS, out) != 0            # slice width
    assert fn(2, 10, 512, 1, 256, 1, 0, 1, 0, CUS, out) != 0           # the staged LayerNorm is a 256-channel one-tap layer
    assert fn(2, 10, 256, 1, 256, 1, 0, 0, 0, 0, out) != 0             # no CUs
    assert fn(2, 10, 256, 1, 256, 1, 0, 0, 0, CUS, None) != 0
