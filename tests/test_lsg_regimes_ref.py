"""CPU-side checks of tests/util_lsg_regimes.py, the table tests/test_gpu_lsg_regimes.py holds csrc/logsoftmax_gather.hip to:
  * every row reaches the kernel instance it names (asked through dsp_logsoftmax_gather_plan: host arithmetic, no device call), and the rows
    together name every instance launch_fwd / launch_bwd can select;
  * the register kernel with global gathers (family 1) is reached only by L below the 16-row tile of the LDS-gather kernel, over the whole
    domain of its instances: its former 32-row variant (write_softmax, L >= 32) could not be selected and is gone;
  * for every row and layout the largest element offset the strides reach lies inside the buffer the GPU test allocates (same arithmetic);
  * the inputs have the planted properties;
  * the float32 comparator holds every older tolerance (`cap`) on these inputs, so no row falls back to 8 err32 + 4 ulp alone;
  * seven emulated kernel defects, applied to the float64 reference on these very inputs, are each at least 10 x outside the bound."""
import numpy as np
import pytest

from tests import util_lsg_regimes as U


@pytest.fixture(scope="module", autouse=True)
def built():
    from daspeech_amd import build
    build.build()


@pytest.mark.parametrize("case", U.CASES, ids=lambda c: c.tag)
def test_row_reaches_the_instance_it_names(case):
    for lazy in (0, 1):
        f, b = U.case_plan(case, 0, lazy), U.case_plan(case, 1, lazy)
        assert (f if f == U.EINVAL else f[:4]) == (case.fwd if case.fwd == U.EINVAL else tuple(case.fwd)), (case.tag, f)
        assert (b if b == U.EINVAL else b[:4]) == (case.bwd if case.bwd == U.EINVAL else tuple(case.bwd)), (case.tag, b)
    for p in (U.case_plan(case, 0), U.case_plan(case, 1)):
        if p != U.EINVAL:
            fam, vec, nv, rt, grid, lds = p
            ntiles = case.B * -(-case.L // rt)
            cap = 4096 if fam in (U.FWD_REGL, U.FWD_REGL_WIDE, U.BWD_REG, U.BWD_REG_WIDE) else 2048
            assert grid == min(ntiles, cap) and 0 < lds <= 160 * 1024, (case.tag, p)
            assert vec == int(U.is_vec(case))


def test_rows_name_every_instance_and_regime():
    named = set()
    for c in U.CASES:
        for p in (c.fwd, c.bwd):
            if p != U.EINVAL:
                named.add((p[0], c.dtype, p[1], p[2]))
    missing = [i for i in U.INSTANCES if i not in named]
    assert not missing, missing
    tiles = {(c.fwd[0], c.fwd[3]) for c in U.CASES if c.fwd != U.EINVAL}
    assert {(U.FWD_REGL, 16), (U.FWD_REGL, 8), (U.FWD_REG, 1), (U.FWD_REG, 2), (U.FWD_REG, 4), (U.FWD_REG, 8), (U.FWD_REGL_WIDE, 4),
            (U.FWD_REGL_WIDE, 1), (U.FWD_GENERIC, 1), (U.FWD_GENERIC, 2), (U.FWD_GENERIC, 4), (U.FWD_GENERIC, 8)} <= tiles
    assert {(U.BWD_REG_WIDE, 4), (U.BWD_REG_WIDE, 1)} <= {(c.bwd[0], c.bwd[3]) for c in U.CASES if c.bwd != U.EINVAL}
    # a second grid-stride trip of each capped grid: 4096 (register kernels) and 2048 (generic, forward tiles and backward rows)
    trips = {(p[0], p[4]) for c in U.CASES for p in (U.case_plan(c, 0), U.case_plan(c, 1)) if p != U.EINVAL and c.L > 1000}
    assert {(U.FWD_REGL, 4096), (U.BWD_REG, 4096), (U.FWD_GENERIC, 2048), (U.BWD_GENERIC, 2048)} <= trips
    assert any(c.S > 256 for c in U.CASES) and any(c.S > 2048 for c in U.CASES) and any("off1" in c.flags for c in U.CASES)


def test_plan_refuses_what_the_launch_refuses():
    assert U.plan(0, "f32", 1, 2, 64, 38400) != U.EINVAL and U.plan(0, "f32", 1, 2, 64, 38401) == U.EINVAL
    assert U.plan(1, "f32", 2, 50, 40944, 9) != U.EINVAL and U.plan(1, "f32", 2, 50, 40948, 9) == U.EINVAL
    assert U.plan(1, "f16", 2, 50, 40952, 9) == U.EINVAL
    assert U.plan(0, "f32", 0, 5, 64, 3)[0] == -1 and U.plan(1, "f32", 5, 0, 64, 3)[0] == -1          # nothing is launched
    assert U.plan(0, "f32", 1, 1, 0, 3) == U.EINVAL and U.plan(0, "f32", -1, 1, 8, 3) == U.EINVAL
    from daspeech_amd import _lib
    assert b"logsoftmax_gather" in _lib.load().dsp_last_error()


def test_register_kernel_with_global_gathers_is_reached_only_below_sixteen_rows():
    """Over the domain of lsg_fwd_reg_kernel's instances — aligned rows of at most 8 vectors per lane, S <= 2048 —: the row image is at most
    32 KB, so the LDS-gather kernel keeps a tile of 4 rows or more, S * tile is a multiple of 4, and only L below that tile (<= 16) is left
    to family 1.  `write_softmax && L >= 32`, the condition of the 32-row variant launch_fwd once had, is therefore never true there."""
    from daspeech_amd import _lib
    import ctypes
    fn = _lib.load().dsp_logsoftmax_gather_plan
    out = (ctypes.c_int * 6)()
    reached = 0
    for dtype, n in (("f32", 4), ("f16", 8), ("bf16", 8)):
        code = U.CODES[dtype]
        for V in [n] + [256 * n * nv for nv in range(1, 9)]:
            for L in (1, 2, 3, 4, 7, 8, 15, 16, 17, 31, 32, 33, 64):
                for S in range(0, 2049):
                    assert fn(0, code, 2, L, V, S, 1, 1, 0, out) == 0
                    fam, rt = out[0], out[3]
                    assert fam in (U.FWD_REG, U.FWD_REGL), (dtype, V, L, S, fam)
                    if fam == U.FWD_REG:
                        reached += 1
                        assert L < 16 and rt <= 8 and rt <= L, (dtype, V, L, S, rt)
                    else:
                        assert rt >= 4 and L >= rt and (S * rt) % 4 == 0, (dtype, V, L, S, rt)
    assert reached > 0


IDX_LAYOUTS = ("expand", "dense_bls", "stored_bsl")
OUT_LAYOUTS = ("pitched", "dense_bls")
GRAD_LAYOUTS = ("bsl", "dense_bls")


@pytest.mark.parametrize("case", U.CASES, ids=lambda c: c.tag)
def test_strides_stay_inside_the_buffers(case):
    n, first, guard = U.logits_layout(case)
    es = U.ESIZE[case.dtype]
    assert guard >= case.V and first + case.B * case.L * case.V + guard == n
    assert (first * es) % 16 == (es if "off1" in case.flags else 0)
    for name in OUT_LAYOUTS:
        numel, st, ld = U.out_layout(case, name)
        assert 0 <= U.max_offset(case, st) < numel - U.GUARD_FLOATS, (case.tag, name)
        if ld:
            assert ld > case.L and ld % 4 == 0
        # distinct (b, j, s) -> distinct elements
        assert len({st[0], st[1], st[2]}) == 3 or min(case.B, case.L, case.S) == 1 or case.L == case.S
    for name in IDX_LAYOUTS:
        numel, st = U.idx_layout(case, name)
        assert 0 <= U.max_offset(case, st) < numel, (case.tag, name)
    for name in GRAD_LAYOUTS:
        numel, st = U.grad_layout(case, name)
        assert 0 <= U.max_offset(case, st) < numel, (case.tag, name)
    # place / view_bls are inverse on a small probe of the row's own strides
    if case.B * case.L * case.S <= 20000:
        v = np.arange(case.B * case.L * case.S, dtype=np.float32).reshape(case.B, case.L, case.S)
        for numel, st in (U.out_layout(case, "pitched")[:2], U.grad_layout(case, "dense_bls"), U.idx_layout(case, "stored_bsl")):
            assert np.array_equal(U.view_bls(U.place(v, numel, st, np.nan, np.float32), case, st), v)


def _ratio(got, ref, bound):
    return U.worst(got, ref, bound)[0]


@pytest.mark.parametrize("case", [c for c in U.CASES if c.fwd != U.EINVAL], ids=lambda c: c.tag)
def test_inputs_comparator_and_defects(case):
    inp, ref = U.make_inputs(case.tag), U.references(case.tag)
    B, L, V, S = case.B, case.L, case.V, case.S
    x = inp.x
    # ---- the inputs are what the table claims
    assert np.array_equal(U.to_dtype(x, case.dtype), x), "logits are values of the case's dtype"
    assert np.isfinite(x).any(axis=-1).all(), "no row is entirely -inf"
    if L > 1 and V > 1:
        assert (inp.idx[:, 1:] != inp.idx[:, :-1]).any(axis=-1).mean() > 0.9, "rows have targets of their own"
    if S >= 3:
        assert any(np.bincount(inp.idxc[0, j]).max() >= 3 for j in range(min(L, 4))), "a token three times in a row"
    if L >= 9 and (S >= 8 or V > 1):
        assert (inp.idx < 0).any() and (inp.idx >= V).any() and (inp.idxc == 0).any() and (inp.idxc == V - 1).any()
    rows = x.reshape(B * L, V)
    for name, lanes in (("lane_inf", [5]), ("wave_inf", range(64, 128))):
        if name in inp.plants:
            cols = U.lane_columns(case, U.is_vec(case), inp.plants[name], lanes)
            if 0 < len(cols) < V:
                r = rows[inp.plants[name]]
                assert np.isneginf(r[cols]).all() and np.isfinite(np.delete(r, cols)).all(), name
                if U.is_vec(case):
                    n = 16 // U.ESIZE[case.dtype]
                    want = [c for k in range(0, V, 256 * n) for t in lanes for c in range(k + t * n, min(k + t * n + n, V))]
                    assert sorted(want) == list(cols)
    if np.isneginf(x).any() and S > 0:
        assert np.isneginf(ref.match64).any(), "a -inf logit is gathered"
    assert not np.isnan(ref.match64).any() and not np.isnan(ref.sm64).any()
    m = x.max(axis=-1)
    if "max_first" in inp.plants and V > 1:
        assert rows[inp.plants["max_first"]].argmax() == 0
    if "max_last" in inp.plants:
        assert rows[inp.plants["max_last"]].argmax() == V - 1 or V == 1 or rows[inp.plants["max_last"]][V - 1] == m.reshape(-1)[inp.plants["max_last"]]

    # ---- the float32 comparator holds every cap: no row of the table needs the bound without its cap
    sm_start = U.to_dtype(ref.sm64.astype(np.float32), case.dtype)          # what an eager forward leaves behind, up to its rounding
    geager64, geager32 = U.backward_refs(sm_start, inp.idxc, inp.g)
    gscale_e, gscale_l = U.grad_scale_rows(sm_start, inp.idxc, inp.g), U.grad_scale_rows(ref.sm64, inp.idxc, inp.g)
    bounds = {
        "match": U.match_bound(case, ref.match64, ref.match32, inp.row_scale),
        "softmax": U.softmax_bound(case, ref.sm64, ref.sm32),
        "grad_eager": U.grad_bound(case, geager64, geager32, gscale_e),
        "grad_lazy": U.grad_bound(case, ref.glazy64, ref.glazy32, gscale_l),
    }
    for name, (r64, r32, cap) in {"match": (ref.match64, ref.match32, U.match_cap(ref.match64, inp.row_scale)),
                                  "softmax": (ref.sm64, ref.sm32, U.softmax_cap(ref.sm64)),
                                  "grad_eager": (geager64, geager32, U.grad_cap(geager64)),
                                  "grad_lazy": (ref.glazy64, ref.glazy32, U.grad_cap(ref.glazy64))}.items():
        assert _ratio(r32, r64, cap) <= 1.0, (name, "the float32 comparator misses the cap")
        assert _ratio(r32, r64, bounds[name]) <= 1.0, name
    assert _ratio(ref.inv32, ref.inv64, U.inv_bound(ref.inv64, ref.inv32)) <= 1.0

    # ---- emulated defects, each at least 10 x outside the bound (None: the defect cannot show at this shape)
    if B * L * V > 2_500_000:
        return
    caught = 0
    for name in U.MATCH_DEFECTS:
        bad = U.defect_match(name, case, inp)
        if bad is not None:
            r = _ratio(bad, ref.match64, bounds["match"])
            print(f"{case.tag}: match defect {name}: {r:.3g} x the bound")
            assert r >= 10.0, (name, r)
            caught += 1
    for name in U.GRAD_DEFECTS:
        for mode, sm, gref in (("grad_eager", sm_start, geager64), ("grad_lazy", ref.sm64, ref.glazy64)):
            bad = U.defect_grad(name, case, inp, sm, gref)
            if bad is not None:
                r = _ratio(bad, gref, bounds[mode])
                print(f"{case.tag}: {mode} defect {name}: {r:.3g} x the bound")
                assert r >= 10.0, (name, mode, r)
                caught += 1
    assert caught >= (6 if L >= 2 and V >= 8 and S >= 8 else 1)
