"""The dropout state of the training operators on the device: DropoutState, its draws() scope, the registry of active scopes and
the questions decode_ops asks it (_active_dropout_state, _capture_ok) — everything the state needs, in one module that depends on the C
binding alone.  decode_ops imports from here and re-exports DropoutState: that is where its users find it, next to the operators it serves."""
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _lib

_DRAWS = {}                  # device index -> the DropoutState whose draws() scope is active on that device (empty: every call asks the generator)
_NOT_GPU_DEVICE = "expected a GPU device (HIP op, no CPU path)"


def _capturing() -> bool:
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


def _device_index(device) -> int:
    return device.index if device.index is not None else torch.cuda.current_device()


def _state_tensor(device, seed: int, offset: int) -> Tensor:
    """the int64[2] device tensor {seed, offset} of a DropoutState (the 64 bits of the seed as they are: a seed above 2^63 is stored negative)"""
    seed &= 0xFFFFFFFFFFFFFFFF
    return torch.tensor([seed - (1 << 64) if seed >> 63 else seed, int(offset)], dtype=torch.int64, device=device)


def _advance(state, by: int) -> None:
    """state[1] += by: dsp_dropout_state_advance on the current stream of the state's device — under capture the node draws() records last"""
    with torch.cuda.device(state.device):
        _lib.check(_lib.load().dsp_dropout_state_advance(state.tensor.data_ptr(), int(by), _lib.current_stream_handle()), "dsp_dropout_state_advance")


class _StateDraws:
    """What _dropout_call hands out in place of a host seed inside DropoutState.draws(): the state, and the generation of the scope that
    reserved the call.  An autograd.Function keeps it in ctx (which keeps the state tensor alive) and asks it for the pointer at every launch."""
    __slots__ = ("state", "generation")

    def __init__(self, state, generation):
        self.state, self.generation = state, generation

    def pointer(self) -> int:
        st = self.state
        if st._generation != self.generation or st._intra is None:
            raise RuntimeError("DropoutState: this call was reserved in a draws() scope that has exited — its advance has moved the offset on, and "
                               "the mask of the forward cannot be drawn again; run the backward before the scope exits")
        return st.tensor.data_ptr()


class DropoutState:
    """The dropout state of the training operators ON THE DEVICE: one int64[2] tensor {seed, offset} (`tensor`), for launches that are recorded
    into a graph (torch.cuda.graph), where no host integer can name the offset of a replay.

        state = DropoutState(device)                 # seed / offset default to the device's default generator: (initial_seed(), get_offset()),
                                                     # read on the host here — construct it OUTSIDE a capture
        with torch.cuda.graph(g), state.draws():     # or eagerly, without a graph: the same kernels, the same masks
            loss = layer(x).sum(); loss.backward()

    Inside draws() every masked call of a training operator on that device (residual_dropout_layer_norm, bias_act_dropout, embed_entry,
    positional_add_dropout, relpos_attention, mha_attention; `training and p > 0`) takes (state tensor, intra) in place of the host pair
    (seed, offset): intra is a host counter, 0 at entry and 4 more per masked call — the steps _reserve_dropout_stream moves the generator by;
    calls with p == 0 or training=False reserve nothing — and the kernels read seed = state[0], offset = state[1] + intra on the device
    (the ..._state entries of include/daspeech_decode.h).  The default generator is not touched.  On a clean exit draws() enqueues ONE
    launch on the current stream, state[1] += the intra reached (dsp_dropout_state_advance): under capture it is the graph's last node, so
    every replay draws new masks and leaves the state advanced as one eager pass leaves the generator, without host work between replays.
    The masks are those of the host form for the same numbers: an eager call with the generator at (seed, offset + intra).

    THE BACKWARD OF A FORWARD THAT RAN INSIDE draws() HAS TO RUN BEFORE THAT SCOPE EXITS — the advance moves state[1], and the backward
    recomputes its mask from the state.  Inside one captured graph that holds by construction; eagerly, call backward() inside the `with`.
    A backward that comes later is detected on the host (a generation counter) and raises; it never draws another mask silently.
    Scopes do not nest on a device.  set / get are host calls for use outside a capture (get synchronises); mark / rewind read and set the
    host counter, for code that needs two passes with the same masks (models/daspeech.py: _same_draws)."""

    def __init__(self, device, seed: Optional[int] = None, offset: Optional[int] = None):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"DropoutState: {_NOT_GPU_DEVICE}")
        if _capturing():
            raise RuntimeError("DropoutState: construct the state outside a graph capture (seed and offset are written from the host)")
        idx = _device_index(device)
        if seed is None or offset is None:
            gen = torch.cuda.default_generators[idx]
            seed = int(gen.initial_seed()) if seed is None else seed
            offset = int(gen.get_offset()) if offset is None else offset
        self.device = torch.device("cuda", idx)
        self.tensor = _state_tensor(self.device, int(seed), int(offset))
        self._intra = None           # None: no draws() scope is active
        self._high = 0
        self._generation = 0
        self._seed_marks = {}

    def set(self, seed: int, offset: int) -> None:
        """state = {seed, offset}, from the host: outside a capture and outside draws()"""
        if _capturing() or self._intra is not None:
            raise RuntimeError("DropoutState.set: a host call, for use outside a graph capture and outside draws()")
        self.tensor.copy_(_state_tensor("cpu", int(seed), int(offset)))

    def get(self) -> Tuple[int, int]:
        """(seed, offset) as the device holds them now; synchronises.  Outside a capture."""
        if _capturing():
            raise RuntimeError("DropoutState.get: a host read, for use outside a graph capture")
        seed, offset = self.tensor.tolist()
        return seed & 0xFFFFFFFFFFFFFFFF, offset

    def _reserve(self) -> Tuple[_StateDraws, int]:
        intra = self._intra
        self._intra = intra + 4
        if self._intra > self._high:
            self._high = self._intra
        return _StateDraws(self, self._generation), intra

    def mark(self) -> int:
        """the host counter `intra` of the active draws() scope"""
        if self._intra is None:
            raise RuntimeError("DropoutState.mark: no draws() scope is active")
        return self._intra

    def rewind(self, mark: int) -> None:
        """intra = mark (a value mark() gave in this scope): the masked calls that follow draw the masks of the calls that followed the mark.
        The advance at exit is the highest intra reached, so a rewound pass does not count twice."""
        if self._intra is None:
            raise RuntimeError("DropoutState.rewind: no draws() scope is active")
        if mark < 0 or mark % 4 or mark > self._high:
            raise ValueError(f"DropoutState.rewind: {mark} is not a mark of this scope")
        self._intra = int(mark)

    def _catch_up(self) -> None:
        """intra = the highest intra this scope has reached: what ends a rewound pass, so that a pass that drew fewer masks than the one it
        repeats leaves no spent offset to the calls behind it"""
        if self._intra is not None and self._intra < self._high:
            self._intra = self._high

    def draws(self):
        """the scope described above; yields the state"""
        return _DrawsScope(self)


class _DrawsScope:
    """DropoutState.draws(): a plain context manager (no generator frame: it is entered once per captured layer or step)"""
    __slots__ = ("state",)

    def __init__(self, state):
        self.state = state

    def __enter__(self):
        st = self.state
        idx = st.device.index
        if idx in _DRAWS:
            raise RuntimeError("DropoutState.draws: a draws() scope is already active on this device (scopes do not nest)")
        st._intra, st._high = 0, 0
        st._seed_marks = {}          # models/daspeech.py _same_draws: seed -> the mark of the first pass under it
        _DRAWS[idx] = st
        return st

    def __exit__(self, exc_type, exc, tb):
        st = self.state
        del _DRAWS[st.device.index]
        total = st._high
        st._intra, st._high = None, 0
        st._generation += 1
        if exc_type is None and total:               # a pass that raised is not advanced over: nothing of it is replayed
            _advance(st, total)
        return False


def _active_dropout_state(device) -> Optional[DropoutState]:
    """the DropoutState whose draws() scope is active on `device`, or None"""
    if not _DRAWS:
        return None
    device = torch.device(device)
    return _DRAWS.get(_device_index(device)) if device.type == "cuda" else None


def _capture_ok(device, masked: bool = True) -> bool:
    """the last question of the ..._served rules of the masked operators: the current stream is not capturing a graph, or the call draws no
    mask, or a draws() scope on the device hands out the state in place of host integers"""
    if not _capturing():
        return True
    return not masked or (bool(_DRAWS) and _device_index(device) in _DRAWS)
