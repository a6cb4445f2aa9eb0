"""decode_ops._row_pitch against its definition, on the CPU: pitch p is valid iff the element (r, c) of the tensor flattened to rows [R, C]
sits at storage_offset + r * p + c for every r, c; no valid pitch -> None.  With one row every pitch is valid and the function may report C.
Inputs: as_strided views of one 4 096-element buffer (bounds-checked), over shapes, strides (zero, overlapping and non-unit ones included)
and storage offsets."""
import itertools

import torch

BUF = 4096
SHAPES_3D = list(itertools.product((1, 2, 3), (1, 2, 5), (1, 4, 8)))
STRIDES_3D = list(itertools.product((0, 1, 4, 8, 10, 16, 20, 24, 40, 48, 80, 120), (0, 1, 4, 8, 10, 16, 24), (0, 1, 2)))
OTHER_SHAPES = [(1, 8), (5, 4), (3, 1), (2, 1, 3, 4), (1, 2, 1, 8), (2, 3, 1, 1), (1, 1, 1, 4)]
OFFSETS = (0, 3)


def _element_offsets(shape, strides):
    """storage offsets (relative to the view's own) of the elements, as a [R, C] tensor in row-major order of the leading dimensions"""
    off = torch.zeros(shape, dtype=torch.long)
    for d, (n, s) in enumerate(zip(shape, strides)):
        view = [1] * len(shape)
        view[d] = n
        off = off + (torch.arange(n) * s).view(view)
    return off.reshape(-1, shape[-1])


def _brute_force(shape, strides):
    """(pitch, rows): the pitch by the definition above (None: there is none; with one row: the columns alone decide, reported as C)"""
    off = _element_offsets(shape, strides)
    R, C = off.shape
    p = C if R == 1 else int(off[1, 0] - off[0, 0])
    want = torch.arange(R).unsqueeze(1) * p + torch.arange(C).unsqueeze(0)
    return (p if torch.equal(off, want) else None), R


def _cases():
    for shape in SHAPES_3D:
        for strides in STRIDES_3D:
            yield shape, strides
    for shape in OTHER_SHAPES:
        pool = [(0, 1, 4, 8, 24, 40)] * (len(shape) - 1) + [(0, 1, 2)]
        for strides in itertools.product(*pool):
            yield shape, strides


def test_row_pitch_is_the_brute_force_pitch_on_strided_views():
    from daspeech_amd import decode_ops
    buf = torch.arange(BUF, dtype=torch.float32)
    n = some = none = 0
    for shape, strides in _cases():
        span = sum((k - 1) * s for k, s in zip(shape, strides))
        for offset in OFFSETS:
            assert offset + span < BUF, (shape, strides, offset)                 # the view stays inside the buffer
            t = buf.as_strided(shape, strides, offset)
            want, R = _brute_force(shape, strides)
            got = decode_ops._row_pitch(t)
            assert got == want, (shape, strides, offset, got, want)
            if got is not None:                                                 # and the elements are where the pitch says
                rows = t.reshape(-1, shape[-1])
                assert rows[R - 1, shape[-1] - 1] == offset + (R - 1) * got + shape[-1] - 1
                some += 1
            else:
                none += 1
            n += 1
    assert n == 2 * (len(SHAPES_3D) * len(STRIDES_3D) + sum(6 ** (len(s) - 1) * 3 for s in OTHER_SHAPES))
    assert some > 500 and none > 5000                                           # both answers are exercised
