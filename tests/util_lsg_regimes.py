"""Case table, inputs, float64 references and bounds for the fp32 / fp16 / bf16 logsoftmax-gather kernels (csrc/logsoftmax_gather.hip) at every
launch regime of launch_fwd / launch_bwd.  tests/test_lsg_regimes_ref.py checks all of this on the CPU (the table against
dsp_logsoftmax_gather_plan, the buffer extents, the planted inputs, the rejection of emulated defects); tests/test_gpu_lsg_regimes.py holds
the kernels to it.

Families (out[0] of dsp_logsoftmax_gather_plan): 0 forward generic, 1 forward registers (gathers from global memory), 2 forward registers +
LDS gather, 3 the same for wide fp32 rows, 4 backward generic, 5 backward registers, 6 backward registers for wide fp32 rows.

References
  float64   oracle.dag_oracle.logsoftmax_gather / logsoftmax_gather_bwd on the logits AS ROUNDED to the case's dtype (the rounding of the
            inputs is no part of any error) and on the CLAMPED indices.  The eager backward's reference starts from the softmax the forward
            stored (the device's own, or on the CPU the float64 softmax rounded to the dtype), the lazy one from the logits.
  float32   the same formulas evaluated in float32 on the CPU (forward32 / backward32: numpy, whose pairwise sums are the closest the CPU has
            to the kernels' tree reductions; the oracle's own float32 instantiation sums a row left to right and is 6 - 170 x outside the
            older tolerances at V >= 8192) on the same inputs: `err32` is its error against the float64 reference.

Bounds (none is measured on the kernels), per vertex row on the row's own scale = its largest finite |float64 reference| (match: at least 1,
see match_bound; gradients: the size of the terms that cancel, see grad_scale_rows):
  fp32 quantities (match, fp32 softmax, fp32 gradients, 1/s):  err <= min(8 err32 + 4 2^-23 scale, cap)   (tests/util_glue_ref.fp32_bound),
      cap = what the kernel's older tests hold:  match 2e-6 |ref| + 2e-6 max(1, logit scale of the row);  softmax 1e-6 |ref| + 1e-7;
      gradients 4e-6 max(1, max |gref|) (the maximum over the whole tensor, as in test_oracle_logsoftmax_gather);  1/s is the softmax of the
      row's largest logit and takes the softmax cap.
  fp16 / bf16 softmax and gradients: the fp32 bound + one rounding of the stored value, 2^-11 |ref| + 2^-25 (fp16) or 2^-8 |ref| (bf16),
      never beyond the older 1e-3 / 8e-3 relative + a tenth of it absolute (gradients: 4x, on max(1, max |gref|)).
  The row maximum m of the statistics is exact; the -inf sets of `match` are equal; NaN and +inf appear nowhere."""
import ctypes
import functools
import zlib
from collections import namedtuple

import numpy as np
import torch

from oracle import dag_oracle as orc
from tests.util_glue_ref import fp32_bound

FWD_GENERIC, FWD_REG, FWD_REGL, FWD_REGL_WIDE, BWD_GENERIC, BWD_REG, BWD_REG_WIDE = range(7)
FAMILY_NAMES = ("fwd_generic", "fwd_reg", "fwd_regl", "fwd_regl_wide", "bwd_generic", "bwd_reg", "bwd_reg_wide")
EINVAL = "EINVAL"
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
CODES = {"f32": 0, "f16": 1, "bf16": 2}
ESIZE = {"f32": 4, "f16": 2, "bf16": 2}
ULP = 2.0 ** -23

# fwd / bwd: the instance the row must reach, (family, VEC, NV, row tile), or EINVAL.  flags: "off1" the [B,L,V] buffer starts one element
# past a 16-byte boundary;  "ops" the row also runs through custom_ops.dag_logsoftmax_gather_inplace under autograd.
Case = namedtuple("Case", "tag dtype B L V S flags fwd bwd")


def _c(tag, dtype, B, L, V, S, fwd, bwd, flags=()):
    return Case(tag, dtype, B, L, V, S, tuple(flags), fwd, bwd)


G0, G1 = (FWD_GENERIC, 0, 0), (FWD_GENERIC, 1, 0)
BG0, BG1 = (BWD_GENERIC, 0, 0, 1), (BWD_GENERIC, 1, 0, 1)

CASES = [
    # ---- fp32, LDS-gather register kernel, NV = 2, 4, 6, 8 (1024 logits per vector slot), 16-row tiles; S = 300, 512: second tk[] slot
    _c("f32-regl2", "f32", 3, 50, 512, 17, (FWD_REGL, 1, 2, 16), (BWD_REG, 1, 2, 16), ["ops"]),
    _c("f32-regl4", "f32", 2, 50, 2052, 17, (FWD_REGL, 1, 4, 16), (BWD_REG, 1, 4, 16)),
    _c("f32-regl6-S300", "f32", 2, 50, 4100, 300, (FWD_REGL, 1, 6, 16), (BWD_REG, 1, 6, 16)),
    _c("f32-regl8-S512", "f32", 2, 50, 8192, 512, (FWD_REGL, 1, 8, 16), (BWD_REG, 1, 8, 16)),
    _c("f32-regl8-tile8", "f32", 2, 12, 8192, 1024, (FWD_REGL, 1, 8, 8), BG1),
    # ---- fp32, register kernel with global gathers: L below the LDS-gather tile; tiles of 2, 4, 8, 1 and (S = 1024) 4 rows
    _c("f32-reg2-tile2", "f32", 3, 3, 512, 17, (FWD_REG, 1, 2, 2), BG1, ["ops"]),
    _c("f32-reg4-tile4", "f32", 2, 7, 3000, 17, (FWD_REG, 1, 4, 4), BG1),
    _c("f32-reg6-tile8", "f32", 2, 15, 5000, 17, (FWD_REG, 1, 6, 8), BG1),
    _c("f32-reg8-tile1", "f32", 2, 1, 8192, 17, (FWD_REG, 1, 8, 1), BG1),
    _c("f32-reg8-S1024-tile4", "f32", 2, 5, 8192, 1024, (FWD_REG, 1, 8, 4), BG1),
    # ---- fp32 wide rows: NV = 10, 12, 14 (tile 4), 16 (tile 1); fall-through by S * tile % 4; L under the tile
    _c("f32-wide10", "f32", 2, 50, 8196, 17, (FWD_REGL_WIDE, 1, 10, 16), (BWD_REG_WIDE, 1, 10, 16), ["ops"]),
    _c("f32-wide12-S512", "f32", 2, 50, 10244, 512, (FWD_REGL_WIDE, 1, 12, 16), (BWD_REG_WIDE, 1, 12, 16)),
    _c("f32-wide14-S1024-tile4", "f32", 2, 50, 12292, 1024, (FWD_REGL_WIDE, 1, 14, 4), (BWD_REG_WIDE, 1, 14, 4)),
    _c("f32-wide16-S2048-tile1", "f32", 2, 50, 16384, 2048, (FWD_REGL_WIDE, 1, 16, 1), (BWD_REG_WIDE, 1, 16, 1)),
    _c("f32-wide16-S2047-fallthrough", "f32", 2, 50, 16384, 2047, G1 + (4,), (BWD_REG_WIDE, 1, 16, 1)),
    _c("f32-wide16-L9", "f32", 2, 9, 16384, 17, G1 + (8,), BG1),
    # ---- fp32 generic VEC past the wide range; the last V the backward serves, and one past it
    _c("f32-generic-V16388", "f32", 2, 50, 16388, 9, G1 + (16,), BG1, ["ops"]),
    _c("f32-generic-V40944", "f32", 2, 50, 40944, 9, G1 + (16,), BG1),
    _c("f32-generic-V40948-bwd-refused", "f32", 2, 50, 40948, 9, G1 + (16,), EINVAL),
    # ---- generic by S (> 2048): row tiles 4, 2, 1 (the last S the forward serves), and one past it
    _c("f32-S2049-tile4", "f32", 2, 20, 64, 2049, G1 + (4,), BG1),
    _c("f32-S4000-tile2", "f32", 2, 20, 64, 4000, G1 + (2,), BG1),
    _c("f32-S38400-tile1", "f32", 1, 2, 64, 38400, G1 + (1,), BG1),
    _c("f32-S38401-fwd-refused", "f32", 1, 2, 64, 38401, EINVAL, BG1),
    # ---- scalar head / tail (Peel): odd V, V = 1..5 (head > V, nb = 0), a base pointer off the 16-byte grid at an aligned V
    _c("f32-V37", "f32", 3, 50, 37, 17, G0 + (16,), BG0, ["ops"]),
    _c("f32-V10001", "f32", 2, 50, 10001, 17, G0 + (16,), BG0),
    _c("f32-V1", "f32", 2, 50, 1, 17, G0 + (16,), BG0),
    _c("f32-V2", "f32", 2, 50, 2, 17, G0 + (16,), BG0),
    _c("f32-V3", "f32", 2, 50, 3, 17, G0 + (16,), BG0),
    _c("f32-V4", "f32", 2, 50, 4, 17, (FWD_REGL, 1, 2, 16), (BWD_REG, 1, 2, 16)),
    _c("f32-V5", "f32", 2, 50, 5, 17, G0 + (16,), BG0),
    _c("f32-V512-off1", "f32", 2, 50, 512, 17, G0 + (16,), BG0, ["off1"]),
    _c("f16-V6004", "f16", 2, 50, 6004, 17, G0 + (16,), BG0),
    _c("f16-V1000-off1", "f16", 2, 50, 1000, 17, G0 + (16,), BG0, ["off1"]),
    _c("bf16-V1003", "bf16", 2, 50, 1003, 17, G0 + (16,), BG0),
    _c("bf16-V264-off1", "bf16", 2, 50, 264, 17, G0 + (16,), BG0, ["off1"]),
    # ---- fp16 (2048 logits per vector slot): regl 2, 4, 6, 8; reg 2, 4, 6, 8; the backward's LDS boundary; generic VEC
    _c("f16-regl2", "f16", 2, 50, 1000, 17, (FWD_REGL, 1, 2, 16), (BWD_REG, 1, 2, 16)),
    _c("f16-regl4", "f16", 2, 50, 4104, 17, (FWD_REGL, 1, 4, 16), (BWD_REG, 1, 4, 16)),
    _c("f16-regl6", "f16", 2, 50, 9000, 17, (FWD_REGL, 1, 6, 16), (BWD_REG, 1, 6, 16)),
    _c("f16-regl8", "f16", 2, 50, 16384, 17, (FWD_REGL, 1, 8, 16), (BWD_REG, 1, 8, 16), ["ops"]),
    _c("f16-regl8-S191", "f16", 2, 50, 16384, 191, (FWD_REGL, 1, 8, 16), (BWD_REG, 1, 8, 16)),
    _c("f16-regl8-S192", "f16", 2, 50, 16384, 192, (FWD_REGL, 1, 8, 16), BG1),
    _c("f16-reg2", "f16", 2, 3, 1000, 17, (FWD_REG, 1, 2, 2), BG1),
    _c("f16-reg4", "f16", 2, 5, 4104, 17, (FWD_REG, 1, 4, 4), BG1),
    _c("f16-reg6", "f16", 2, 9, 9000, 17, (FWD_REG, 1, 6, 8), BG1),
    _c("f16-reg8", "f16", 2, 3, 16384, 17, (FWD_REG, 1, 8, 2), BG1),
    _c("f16-generic-V16392", "f16", 2, 50, 16392, 17, G1 + (16,), BG1),
    # ---- bf16: regl 2, 4, 6, 8; reg 2, 4, 6, 8; generic VEC
    _c("bf16-regl2", "bf16", 2, 50, 264, 17, (FWD_REGL, 1, 2, 16), (BWD_REG, 1, 2, 16)),
    _c("bf16-regl4", "bf16", 2, 50, 4104, 17, (FWD_REGL, 1, 4, 16), (BWD_REG, 1, 4, 16)),
    _c("bf16-regl6", "bf16", 2, 50, 8200, 17, (FWD_REGL, 1, 6, 16), (BWD_REG, 1, 6, 16), ["ops"]),
    _c("bf16-regl8", "bf16", 2, 50, 12296, 17, (FWD_REGL, 1, 8, 16), (BWD_REG, 1, 8, 16)),
    _c("bf16-reg2", "bf16", 2, 3, 264, 17, (FWD_REG, 1, 2, 2), BG1),
    _c("bf16-reg4", "bf16", 2, 7, 4104, 17, (FWD_REG, 1, 4, 4), BG1),
    _c("bf16-reg6", "bf16", 2, 9, 8200, 17, (FWD_REG, 1, 6, 8), BG1),
    _c("bf16-reg8", "bf16", 2, 15, 12296, 17, (FWD_REG, 1, 8, 8), BG1),
    _c("bf16-generic-V16392", "bf16", 2, 20, 16392, 17, G1 + (16,), BG1),
    # ---- a second grid-stride trip: 4126 tiles of 16 rows against caps of 4096 (registers) and 2048 (generic), 66000 rows against 2048
    _c("bf16-stride-V8", "bf16", 2, 33000, 8, 3, (FWD_REGL, 1, 2, 16), (BWD_REG, 1, 2, 16)),
    _c("f32-stride-V5", "f32", 2, 33000, 5, 3, G0 + (16,), BG0),
]
BY_TAG = {c.tag: c for c in CASES}
assert len(BY_TAG) == len(CASES)

# every instance launch_fwd / launch_bwd can select: (family, dtype, VEC, NV); each backward one exists with LAZY = false and true, and every
# case runs both backward entry points
INSTANCES = ([(FWD_GENERIC, d, v, 0) for d in DTYPES for v in (0, 1)] + [(BWD_GENERIC, d, v, 0) for d in DTYPES for v in (0, 1)]
             + [(f, d, 1, nv) for f in (FWD_REG, FWD_REGL, BWD_REG) for d in DTYPES for nv in (2, 4, 6, 8)]
             + [(f, "f32", 1, nv) for f in (FWD_REGL_WIDE, BWD_REG_WIDE) for nv in (10, 12, 14, 16)])


# ------------------------------------------------------------------------------------------------------------ the plan

def plan(backward, dtype, B, L, V, S, aligned16=1, write_softmax=0, lazy=0):
    """dsp_logsoftmax_gather_plan -> (family, VEC, NV, row tile, grid, LDS bytes), or EINVAL."""
    from daspeech_amd import _lib
    out = (ctypes.c_int * 6)()
    rc = _lib.load().dsp_logsoftmax_gather_plan(int(backward), CODES[dtype], B, L, V, S, aligned16, write_softmax, lazy, out)
    return EINVAL if rc != 0 else tuple(out)


def case_plan(case, backward, lazy=0):
    return plan(backward, case.dtype, case.B, case.L, case.V, case.S, 0 if "off1" in case.flags else 1, 0, lazy)


# ------------------------------------------------------------------------------------------------------------ layouts and extents

def round4(n):
    return (n + 3) // 4 * 4


GUARD_FLOATS = 64


def logits_layout(case):
    """(elements allocated, first element of the [B,L,V] block, guard elements on either side).  The guards are whole rows, rounded up so
    that the block starts on a 16-byte boundary before the "off1" displacement."""
    n = 16 // ESIZE[case.dtype]
    guard = (2 * case.V + n - 1) // n * n
    off = 1 if "off1" in case.flags else 0
    return 2 * guard + off + case.B * case.L * case.V, guard + off, guard


def out_layout(case, name):
    """match buffer: (floats allocated incl. the guard, strides (b, j, s), row pitch or 0)."""
    B, L, S = case.B, case.L, case.S
    if name == "pitched":                       # [B,S,ld], ld > L always: there are pitch columns to watch
        ld = round4(L) + 4
        return B * S * ld + GUARD_FLOATS, (S * ld, 1, ld), ld
    assert name == "dense_bls"                  # the reference's [B,L,S]
    return B * L * S + GUARD_FLOATS, (L * S, S, 1), 0


def idx_layout(case, name):
    """index tensor: (int64 elements allocated, strides (b, j, s))."""
    B, L, S = case.B, case.L, case.S
    if name == "expand":
        return B * S, (S, 0, 1)
    if name == "dense_bls":
        return B * L * S, (L * S, S, 1)
    assert name == "stored_bsl"
    return B * S * L, (S * L, 1, L)


def grad_layout(case, name):
    """gradient tensor: (floats allocated, strides (b, j, s))."""
    B, L, S = case.B, case.L, case.S
    if name == "bsl":                           # gsj == 1
        return B * S * L, (S * L, 1, L)
    assert name == "dense_bls"
    return B * L * S, (L * S, S, 1)


def max_offset(case, strides):
    sb, sj, ss = strides
    return (case.B - 1) * sb + (case.L - 1) * sj + (case.S - 1) * ss


def place(values_bls, numel, strides, fill, dtype):
    """A flat numpy buffer of `numel` elements filled with `fill`, holding values_bls[b,j,s] at b*sb + j*sj + s*ss."""
    B, L, S = values_bls.shape
    buf = np.full(numel, fill, dtype)
    sb, sj, ss = strides
    off = (np.arange(B)[:, None, None] * sb + np.arange(L)[None, :, None] * sj + np.arange(S)[None, None, :] * ss)
    buf[off.ravel()] = values_bls.ravel()      # sj == 0 (expand): the rows agree, the last write is as good as the first
    return buf


def view_bls(buf, case, strides):
    sb, sj, ss = strides
    off = (np.arange(case.B)[:, None, None] * sb + np.arange(case.L)[None, :, None] * sj + np.arange(case.S)[None, None, :] * ss)
    return buf[off]


# ------------------------------------------------------------------------------------------------------------ inputs

def to_dtype(x32, dtype):
    """float32 array -> the values after rounding to `dtype`, as float32."""
    if dtype == "f32":
        return np.ascontiguousarray(x32, np.float32)
    return torch.from_numpy(np.ascontiguousarray(x32, np.float32)).to(DTYPES[dtype]).float().numpy()


def is_vec(case):
    """16-byte accesses over whole rows: V a multiple of the vector and the buffer on the 16-byte grid."""
    return case.V % (16 // ESIZE[case.dtype]) == 0 and "off1" not in case.flags


def peel(addr_mod16, V, esize):
    """Peel of csrc/logsoftmax_gather.hip: (head, nb, tail0, nscalar) of a row whose first byte is at addr_mod16 (mod 16)."""
    n = 16 // esize
    h = ((16 - addr_mod16) & 15) // esize
    head = min(h, V)
    nb = (V - head) // n
    tail0 = head + nb * n
    return head, nb, tail0, head + (V - tail0)


def lane_columns(case, vec, rowflat, lanes):
    """The columns of row `rowflat` that the given lanes of the 256-thread workgroup read in pass A (the online max / sum)."""
    V, es = case.V, ESIZE[case.dtype]
    n = 16 // es
    cols = []
    if vec:
        for t in lanes:
            for v0 in range(t * n, V, 256 * n):
                cols += range(v0, min(v0 + n, V))
        return np.array(sorted(cols), np.int64)
    off = 1 if "off1" in case.flags else 0
    head, nb, tail0, nscalar = peel(((off + rowflat * V) * es) % 16, V, es)
    for t in lanes:
        for e in range(t, nscalar, 256):
            cols.append(e if e < head else tail0 + (e - head))
        for i in range(t, nb, 256):
            cols += range(head + i * n, head + i * n + n)
    return np.array(sorted(cols), np.int64)


PLANTS = ("max_first", "max_last", "ascending", "descending", "scatter_inf", "lane_inf", "wave_inf", "single_finite", "span")
Inputs = namedtuple("Inputs", "x idx idxc g row_scale plants shared shared_c")


@functools.lru_cache(maxsize=2)
def make_inputs(tag):
    """x [B,L,V] float32 holding values of the case's dtype; idx [B,L,S] int64 with its own targets per (b, j), out-of-range values included,
    idxc its clamped copy; g [B,L,S] float32; row_scale [B,L] the logit scale of each row; plants {name: flat row}; shared / shared_c [B,1,S]
    the targets of row 0 of each sample (for the stride-0 expand layout)."""
    case = BY_TAG[tag]
    B, L, V, S = case.B, case.L, case.V, case.S
    rng = np.random.default_rng(zlib.crc32(tag.encode()))
    R = B * L
    scales = np.array([0.5, 3.0, 20.0])[np.arange(R) % 3]
    x = (rng.standard_normal((R, V)) * scales[:, None]).astype(np.float32)
    span = 6e4 if case.dtype == "f16" else 80.0
    vec = is_vec(case)
    # planted rows: spread over the tiles when there are rows enough, else the first rows, starting at a plant that depends on the case
    first = zlib.crc32(tag.encode()) % len(PLANTS)
    names = [PLANTS[(first + i) % len(PLANTS)] for i in range(min(len(PLANTS), R))]
    plants = {}
    for i, name in enumerate(names):
        r = (3 + 7 * i) % R if R >= 64 else i
        row = x[r]
        if name == "max_first":
            row[0] = row.max() + 5.0
        elif name == "max_last":
            row[V - 1] = row.max() + 5.0
        elif name == "ascending":
            row[:] = np.sort(row)
        elif name == "descending":
            row[:] = np.sort(row)[::-1]
        elif name == "scatter_inf":
            hit = rng.random(V) < 0.1
            hit[int(rng.integers(0, V))] = False
            row[hit] = -np.inf
        elif name in ("lane_inf", "wave_inf"):
            cols = lane_columns(case, vec, r, [5] if name == "lane_inf" else range(64, 128))
            if 0 < len(cols) < V:
                row[cols] = -np.inf
        elif name == "single_finite":
            keep = int(rng.integers(0, V))
            v = row[keep]
            row[:] = -np.inf
            row[keep] = v
        elif name == "span":
            row[:] = rng.uniform(-span, span, V)
            scales[r] = span
        plants[name] = r
    x = to_dtype(x, case.dtype).reshape(B, L, V)
    assert np.isfinite(x).any(axis=-1).all() and not np.isnan(x).any() and not np.isposinf(x).any()

    idx = rng.integers(0, V, (B, L, S)).astype(np.int64)
    special = [0, V - 1, min(1, V - 1), max(V - 2, 0), -1, -7, V, V + 9, min(3, V - 1)]
    for b in range(B):
        for j in range(L if L <= 64 else 64):          # the planted structure covers the first 64 rows of a sample; the rest are random
            if S >= 8:
                idx[b, j, [0, S // 2, S - 1]] = idx[b, j, 0]                  # a token three times, the last two in later slots
                for q in range(3):                                            # (S >= 8: slots 1..3 are none of 0, S // 2, S - 1, S - 2)
                    idx[b, j, 1 + q] = special[(3 * j + q) % len(special)]
            elif j % 3 == 0:
                idx[b, j, :] = idx[b, j, 0]                                   # S < 8: a row of one token ...
            else:
                for q in range(S):
                    idx[b, j, q] = special[(S * j + q) % len(special)]        # ... or of special columns
    for name, r in plants.items():                      # a gathered -inf wherever -inf was planted
        dead = np.flatnonzero(np.isneginf(x.reshape(R, V)[r]))
        if len(dead) and S > 0:
            idx[r // L, r % L, (S - 2 if S >= 8 else S - 1)] = dead[len(dead) // 2]
    idxc = np.clip(idx, 0, V - 1)
    g = rng.standard_normal((B, L, S)).astype(np.float32)
    shared = np.ascontiguousarray(idx[:, :1, :])
    return Inputs(x, idx, idxc, g, scales.reshape(B, L), plants, shared, np.clip(shared, 0, V - 1))


# ------------------------------------------------------------------------------------------------------------ references

def row_stats64(x):
    x64 = x.astype(np.float64)
    m = x64.max(axis=-1)
    with np.errstate(invalid="ignore"):
        s = np.exp(x64 - m[..., None]).sum(axis=-1)
    return m, 1.0 / s


def row_stats32(x):
    x32 = x.astype(np.float32)
    m = x32.max(axis=-1)
    s = np.exp(x32 - m[..., None], dtype=np.float32).sum(axis=-1, dtype=np.float32)
    return m, (np.float32(1.0) / s).astype(np.float32)


def forward32(x, idxc):
    """The forward's formulas in float32 (numpy: pairwise sums, as close to a tree reduction as the CPU offers) -> (match32, softmax32)."""
    x32 = np.ascontiguousarray(x, np.float32)
    m = x32.max(axis=-1, keepdims=True)
    e = np.exp(x32 - m, dtype=np.float32)
    s = e.sum(axis=-1, keepdims=True, dtype=np.float32)
    ls = np.log(s, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        match = (np.take_along_axis(x32, np.broadcast_to(idxc, x.shape[:2] + idxc.shape[2:]), axis=-1) - m) - ls
    return match.astype(np.float32), (e / s).astype(np.float32)


def backward32(sm, idxc, g):
    """The backward's formulas in float32: softmax * -(sum g), then the scatter-add."""
    B, L, S = idxc.shape
    g32 = np.ascontiguousarray(g, np.float32)
    out = (np.ascontiguousarray(sm, np.float32) * -g32.sum(axis=-1, keepdims=True, dtype=np.float32)).astype(np.float32)
    bb = np.broadcast_to(np.arange(B)[:, None, None], idxc.shape)
    jj = np.broadcast_to(np.arange(L)[None, :, None], idxc.shape)
    np.add.at(out, (bb, jj, idxc), g32)
    return out


def forward_refs(x, idxc):
    """-> (match64, softmax64, match32, softmax32), all [B,L,*]."""
    idxc = np.ascontiguousarray(np.broadcast_to(idxc, (x.shape[0], x.shape[1], idxc.shape[2])))
    m64, s64 = orc.logsoftmax_gather(x.astype(np.float64), idxc, np.float64, want_softmax=True)
    m32, s32 = forward32(x, idxc)
    return m64, s64, m32, s32


def backward_refs(sm, idxc, g):
    """sm: the softmax the backward starts from (any float array) -> (gref64, gref32)."""
    g64 = orc.logsoftmax_gather_bwd(sm.astype(np.float64), idxc, g.astype(np.float64), np.float64)
    return g64, backward32(sm, idxc, g)


Refs = namedtuple("Refs", "match64 sm64 match32 sm32 m64 inv64 inv32 glazy64 glazy32")


@functools.lru_cache(maxsize=2)
def references(tag):
    inp = make_inputs(tag)
    match64, sm64, match32, sm32 = forward_refs(inp.x, inp.idxc)
    m64, inv64 = row_stats64(inp.x)
    _, inv32 = row_stats32(inp.x)
    glazy64 = orc.logsoftmax_gather_bwd(sm64, inp.idxc, inp.g.astype(np.float64), np.float64)
    glazy32 = backward32(sm32, inp.idxc, inp.g)                  # the fp32 path end to end: fp32 softmax, fp32 backward
    return Refs(match64, sm64, match32, sm32, m64, inv64, inv32, glazy64, glazy32)


# ------------------------------------------------------------------------------------------------------------ bounds

def _rows(a):
    return a.reshape(-1, a.shape[-1])


def _row_err32_scale(ref64, ref32):
    fin = np.isfinite(ref64)
    d = np.where(fin, np.abs(np.where(fin, ref32, 0.0).astype(np.float64) - np.where(fin, ref64, 0.0)), 0.0)
    return d.max(axis=-1, keepdims=True), np.where(fin, np.abs(np.where(fin, ref64, 0.0)), 0.0).max(axis=-1, keepdims=True)


def fp32_bound_rows(ref64, ref32, cap, use_cap=True, scale=None):
    """Elementwise min(8 err32 + 4 ulp scale, cap) with err32 and scale per row (tests/util_glue_ref.fp32_bound on the row's scale)."""
    err32, own = _row_err32_scale(ref64, ref32)
    scale = own if scale is None else np.maximum(own, scale)
    safe = np.where(scale > 0, scale, 1.0)
    b = np.vectorize(lambda e, s: fp32_bound(e / s, np.inf) * s)(err32, safe) * (scale > 0)
    b = np.broadcast_to(b, ref64.shape)
    return np.minimum(b, cap) if use_cap else b.copy()


def match_cap(ref64, row_scale):
    fin = np.isfinite(ref64)
    return 2e-6 * np.where(fin, np.abs(np.where(fin, ref64, 0.0)), 0.0) + 2e-6 * np.maximum(1.0, row_scale)[..., None]


def softmax_cap(ref64):
    return 1e-6 * np.abs(ref64) + 1e-7


def grad_cap(gref64):
    return np.full(gref64.shape, 4e-6 * max(1.0, float(np.abs(gref64).max())))


def stored_rounding(ref64, dtype):
    if dtype == "f16":
        return 2.0 ** -11 * np.abs(ref64) + 2.0 ** -25
    if dtype == "bf16":
        return 2.0 ** -8 * np.abs(ref64)
    return np.zeros_like(ref64)


OLD_EPS = {"f16": 1e-3, "bf16": 8e-3}


def match_bound(case, ref64, ref32, row_scale):
    """scale = max(1, the row's largest |reference|): match = (x - m) - log s with s >= 1 held in fp32, so log s carries the rounding of s,
    2^-24 relative = up to 2^-24 absolute, however small log s itself is (a peaked row: s = 1 + tiny) — the floor the cap has as well."""
    return fp32_bound_rows(ref64, ref32, match_cap(ref64, row_scale), scale=1.0)


def softmax_bound(case, ref64, ref32):
    b = fp32_bound_rows(ref64, ref32, softmax_cap(ref64))
    if case.dtype == "f32":
        return b
    eps = OLD_EPS[case.dtype]
    return np.minimum(b + stored_rounding(ref64, case.dtype), eps * np.abs(ref64) + 0.1 * eps)


def inv_bound(ref64, ref32):
    return fp32_bound_rows(ref64[..., None], ref32[..., None], softmax_cap(ref64[..., None]))[..., 0]


def grad_scale_rows(sm, idxc, g):
    """[B,L,1]: the scale of a gradient row.  gx[v] = sm[v] (-sum_s g[s]) + sum_{s: idx[s] = v} g[s] is a sum whose terms cancel (exactly, at
    V = 1), so fp32 rounding is relative to the terms and not to the result: scale = max_v (sm[v] sum_s |g[s]| + sum_{s: idx[s] = v} |g[s]|)."""
    B, L, S = idxc.shape
    a = np.abs(g.astype(np.float64))
    t = np.abs(sm.astype(np.float64)) * a.sum(axis=-1, keepdims=True)
    bb = np.broadcast_to(np.arange(B)[:, None, None], idxc.shape)
    jj = np.broadcast_to(np.arange(L)[None, :, None], idxc.shape)
    np.add.at(t, (bb, jj, idxc), a)
    return t.max(axis=-1, keepdims=True)


def grad_bound(case, gref64, gref32, scale):
    b = fp32_bound_rows(gref64, gref32, grad_cap(gref64), scale=scale)
    if case.dtype == "f32":
        return b
    eps = 4 * OLD_EPS[case.dtype]
    return np.minimum(b + stored_rounding(gref64, case.dtype), eps * np.abs(gref64) + eps * max(1.0, float(np.abs(gref64).max())))


def worst(got, ref64, bound):
    """(largest err / bound, err there, bound there) over the finite reference entries; inf when a -inf / NaN / +inf is out of place."""
    got = np.asarray(got, np.float64)
    if np.isnan(got).any() or np.isposinf(got).any() or not np.array_equal(np.isneginf(got), np.isneginf(ref64)):
        return np.inf, np.inf, 0.0
    fin = np.isfinite(ref64)
    if not fin.any():
        return 0.0, 0.0, 0.0
    err = np.abs(np.where(fin, got, 0.0) - np.where(fin, ref64, 0.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(fin, np.where(err == 0, 0.0, err / bound), 0.0)
    k = np.unravel_index(np.argmax(ratio), ratio.shape)
    return float(ratio[k]), float(err[k]), float(bound[k])


# ------------------------------------------------------------------------------------------------------------ emulated defects

def _lse64(x):
    m, inv = row_stats64(x)
    return m - np.log(inv)


def defect_match(name, case, inp):
    """float64 `match` [B,L,S] of a subtly wrong forward kernel, or None where the defect cannot show in this case."""
    x = inp.x.astype(np.float64)
    B, L, V, S = case.B, case.L, case.V, case.S
    lse = _lse64(inp.x)[..., None]
    take = lambda xx, ii: np.take_along_axis(xx, ii, axis=-1)       # noqa: E731
    if name == "idx_of_next_row":
        return None if L < 2 or V < 2 else take(x, np.roll(inp.idxc, -1, axis=1)) - lse
    if name == "stale_row_image":
        return None if L < 2 else take(np.roll(x, 1, axis=1), inp.idxc) - lse
    if name == "last_vector_dropped":
        n = 16 // ESIZE[case.dtype]
        drop = n if is_vec(case) else 1
        if V <= drop:
            return None
        xs = x[..., :V - drop]
        if not np.isfinite(xs).any(axis=-1).all():
            return None
        return take(x, inp.idxc) - _lse64(xs)[..., None]
    if name == "no_clamp_wraps":
        if np.array_equal(inp.idx % V, inp.idxc):
            return None
        return take(x, inp.idx % V) - lse
    raise KeyError(name)


def defect_grad(name, case, inp, sm, gref):
    """float64 gradient [B,L,V] of a subtly wrong backward kernel started from the softmax `sm`, or None."""
    B, L, V, S = case.B, case.L, case.V, case.S
    g = inp.g.astype(np.float64)
    bb, jj = np.arange(B)[:, None, None], np.arange(L)[None, :, None]
    if name == "scatter_overwrites":
        out = sm.astype(np.float64) * -g.sum(axis=-1, keepdims=True)
        base = out.copy()
        for s in range(S):                                           # the last writer wins
            out[bb[..., 0], jj[..., 0], inp.idxc[:, :, s]] = base[bb[..., 0], jj[..., 0], inp.idxc[:, :, s]] + g[:, :, s]
        return out
    if name == "delta_not_rezeroed":
        if L < 2:
            return None
        sc = np.zeros((B, L, V))
        np.add.at(sc, (np.broadcast_to(bb, inp.idxc.shape), np.broadcast_to(jj, inp.idxc.shape), inp.idxc), g)
        out = gref.copy()
        out[:, 1:] += sc[:, :-1]                                     # row j still carries row j-1's scatter image
        return out
    if name == "sum_over_first_256":
        if S <= 256:
            return None
        return gref + sm.astype(np.float64) * g[:, :, 256:].sum(axis=-1, keepdims=True)
    if name == "no_clamp_wraps":
        if np.array_equal(inp.idx % V, inp.idxc):
            return None
        return orc.logsoftmax_gather_bwd(sm.astype(np.float64), inp.idx % V, g, np.float64)
    if name == "idx_of_next_row":
        return None if L < 2 or V < 2 else orc.logsoftmax_gather_bwd(sm.astype(np.float64), np.ascontiguousarray(np.roll(inp.idxc, -1, axis=1)), g, np.float64)
    raise KeyError(name)


MATCH_DEFECTS = ("idx_of_next_row", "stale_row_image", "last_vector_dropped", "no_clamp_wraps")
GRAD_DEFECTS = ("scatter_overwrites", "delta_not_rezeroed", "sum_over_first_256", "no_clamp_wraps", "idx_of_next_row")
