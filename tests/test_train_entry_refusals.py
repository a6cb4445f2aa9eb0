"""CPU: the argument gates of the training operators' C entries (csrc/host_gates.h and what stays at each site) answer every call of
tests/util_train_entry_refusal_calls.py with the return code and, byte for byte, the dsp_last_error() text that the build before the gates
were shared gave: tests/golden/train_entry_refusals.json, recorded once by tests/golden/make_train_entry_refusals.py.  The pointers are
made-up addresses; every call is answered before any device call, so no GPU is needed."""
import json
import os

import pytest

from daspeech_amd import _lib
from tests import util_train_entry_refusal_calls as U


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def recorded(golden_dir):
    with open(os.path.join(golden_dir, "train_entry_refusals.json")) as f:
        return {(sym, case): (rc, msg) for sym, case, rc, msg in json.load(f)}


CALLS = U.calls()


def test_the_fixture_holds_exactly_the_calls(recorded):
    assert set(recorded) == {(sym, case) for sym, case, _, _ in CALLS}
    assert all((rc == 0) == ok for (rc, _), ok in ((recorded[(s, c)], ok) for s, c, ok, _ in CALLS))


@pytest.mark.parametrize("sym", sorted({s for s, _, _, _ in CALLS}))
def test_every_call_gives_the_recorded_code_and_message(lib, recorded, sym):
    for s, case, ok, args in CALLS:
        if s != sym:
            continue
        rc, msg = recorded[(s, case)]
        assert getattr(lib, s)(*args) == rc, (s, case)
        if not ok:
            assert lib.dsp_last_error().decode("utf-8") == msg, (s, case)


# the outputs of the entries that refuse two equal ones (an entry that is not here does not look: such a call would reach a launch)
TWO_OUTPUTS = {
    "dsp_act_dropout_train_bwd": ("dh", "dbias"), "dsp_resnorm_train_fwd": ("s", "y"), "dsp_resnorm_train_bwd": ("dh", "dresidual"),
    "dsp_dwconv_bn_silu_train_fwd": ("save_mean", "save_invstd"), "dsp_conv1d_train_bwd": ("dx", "dw", "db"),
    "dsp_conv1d_s2_train_bwd": ("dx", "dw", "db"), "dsp_mha_train_fwd": ("out", "lse"), "dsp_mha_train_bwd": ("dq", "dk", "dv"),
    "dsp_relpos_attention_train_bwd": ("dq", "dk", "dv", "dpos", "dbias_u", "dbias_v"), "dsp_embed_entry_bwd": ("dE", "dP"),
    "dsp_tts_loss_fwd": ("losses", "inv_counts"), "dsp_tts_loss_bwd": ("d_feat_out", "d_feat_post", "d_log_dur", "d_pitch", "d_energy"),
}


def test_the_table_covers_what_each_entry_gates():
    """per fwd / bwd entry, read off the ARGUMENTS of its refused cases and not off their names: a pointer of the base call made null; a pointer
    made equal to another pointer of the base call; two outputs made equal where the entry looks; a pointer moved off the 16-byte grid (by
    less than 16 bytes, the workspace and rng_state apart); the three workspace refusals where the entry takes a workspace; a nothing-to-do
    call.  The twins run the same cases (util_train_entry_refusal_calls.calls) plus the misaligned rng_state."""
    for name, e in U.ENTRIES.items():
        if not name.endswith(("_fwd", "_bwd")):
            continue
        base = dict(e["base"])
        ptrs = {k: v for k, v in base.items() if isinstance(v, int) and v >= U.a(0)}
        refused = [over for _, over in e["cases"]]
        one = [(k, v) for over in refused if len(over) == 1 for k, v in over.items() if k in ptrs and k != "workspace"]
        assert any(v is None for _, v in one), name
        assert any(v is not None and v != ptrs[k] and v in ptrs.values() for k, v in one), name
        assert any(v is not None and v % 16 and 0 < v - ptrs[k] < 16 for k, v in one), name
        if name in TWO_OUTPUTS:
            outs = TWO_OUTPUTS[name]
            assert any(k in outs and v in [ptrs[o] for o in outs if o != k] for k, v in one), name
        assert e["ok"], name
        if "workspace" in base:
            assert {"null workspace", "short workspace", "workspace at +2 bytes"} <= {c for c, _ in e["cases"]}, name
    for s in {s for s, _, _, _ in CALLS if s.endswith("_state")}:
        assert (s, "rng_state at +4 bytes") in {(x, c) for x, c, _, _ in CALLS}, s


def test_short_and_misplaced_workspaces_differ_in_their_code(recorded):
    for (s, case), (rc, _) in recorded.items():
        if case == "short workspace":
            assert rc == -2, s
        if case in ("null workspace", "workspace at +2 bytes"):
            assert rc == -1, s
