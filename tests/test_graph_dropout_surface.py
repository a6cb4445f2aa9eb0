"""CPU-side checks of the dropout state on the device (decode_ops.DropoutState): the names and their documentation, the refusal of CPU
devices, the host bookkeeping of draws() — intra 0, 4, 8 for the masked calls, nothing for an unmasked one, the advance at exit, mark /
rewind, nesting, a backward after its scope — with the launch replaced, and the C ABI of the ..._state entries.  No device call."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASKED = ("dsp_resnorm_train_fwd", "dsp_resnorm_train_bwd", "dsp_act_dropout_train_fwd", "dsp_act_dropout_train_bwd", "dsp_embed_entry_fwd",
          "dsp_embed_entry_bwd", "dsp_pos_add_fwd", "dsp_pos_add_bwd", "dsp_relpos_attention_train_fwd", "dsp_relpos_attention_train_bwd",
          "dsp_mha_train_fwd", "dsp_mha_train_bwd")
NEW_SYMBOLS = tuple(n + "_state" for n in MASKED) + ("dsp_dropout_keep_mask_state", "dsp_dropout_state_advance")
DEV = torch.device("cuda", 0)


@pytest.fixture
def host_state(monkeypatch):
    """a DropoutState for cuda:0 whose tensor lives on the host and whose launches are recorded instead of made: (state, launches)"""
    from daspeech_amd import decode_ops, dropout_state
    launches = []
    monkeypatch.setattr(dropout_state, "_state_tensor", lambda device, seed, offset: torch.tensor([seed, offset], dtype=torch.int64))
    monkeypatch.setattr(dropout_state, "_advance", lambda st, by: launches.append(("dsp_dropout_state_advance", (st.tensor.data_ptr(), by))))
    monkeypatch.setattr(decode_ops, "_launch", lambda dev, entry, *args: launches.append((entry.__name__, args)))
    return decode_ops.DropoutState(DEV, seed=7, offset=(1 << 32) + 8), launches


def test_the_names_exist_and_are_documented():
    from daspeech_amd import decode_ops
    st = decode_ops.DropoutState
    for name in ("set", "get", "draws", "mark", "rewind"):
        assert callable(getattr(st, name)) and getattr(st, name).__doc__, name
    doc = st.__doc__
    for word in ("int64[2]", "draws()", "intra", "dsp_dropout_state_advance", "BEFORE THAT SCOPE EXITS", "generation", "nest"):
        assert word in doc, word
    assert callable(decode_ops._active_dropout_state) and "DropoutState" in decode_ops.dropout_keep_mask.__doc__
    for served in ("residual_dropout_layer_norm_served", "bias_act_dropout_served", "embed_entry_served", "positional_add_dropout_served",
                   "relpos_attention_autograd_served", "mha_attention_autograd_served"):
        assert "DropoutState.draws()" in getattr(decode_ops, served).__doc__, served
    assert "DropoutState.draws()" in decode_ops.__doc__


def test_cpu_devices_are_refused():
    from daspeech_amd import decode_ops
    with pytest.raises(RuntimeError, match=r"^DropoutState: expected a GPU device \(HIP op, no CPU path\)$"):
        decode_ops.DropoutState("cpu")
    with pytest.raises(RuntimeError, match=r"^DropoutState: expected a GPU device \(HIP op, no CPU path\)$"):
        decode_ops.DropoutState(torch.device("cpu"), seed=1, offset=0)
    with pytest.raises(RuntimeError, match=r"^dropout_keep_mask: expected a GPU device \(HIP op, no CPU path\)$"):
        decode_ops.dropout_keep_mask(1, 0, 0.5, (4,), "cpu")
    assert decode_ops._active_dropout_state("cpu") is None


def test_masked_calls_take_intra_0_4_8_and_the_exit_advances_by_12(host_state):
    from daspeech_amd import decode_ops
    st, launches = host_state
    with st.draws() as inside:
        assert inside is st and decode_ops._active_dropout_state(DEV) is st
        got = [decode_ops._dropout_call(0.3, True, DEV), decode_ops._dropout_call(0.1, True, DEV),
               decode_ops._dropout_call(0.0, True, DEV), decode_ops._dropout_call(0.3, False, DEV),       # unmasked: p == 0, not training
               decode_ops._dropout_call(0.5, True, DEV)]
        assert [g[0] for g in got] == [0.3, 0.1, 0.0, 0.0, 0.5]
        assert [g[2] for g in got] == [0, 4, 0, 0, 8]
        for g in (got[0], got[1], got[4]):
            assert g[1].state is st and g[1].pointer() == st.tensor.data_ptr()
        assert got[2][1:] == (0, 0) and got[3][1:] == (0, 0)                    # the host form of "no mask": nothing reserved
        assert st.mark() == 12 and launches == []
        lib = decode_ops._lib.load()
        entry, seed, offset, tail = decode_ops._masked(lib, "dsp_mha_train_fwd", got[4][1], got[4][2])
        assert entry.__name__ == "dsp_mha_train_fwd_state" and (seed, offset) == (0, 8) and tail == (st.tensor.data_ptr(),)
        entry, seed, offset, tail = decode_ops._masked(lib, "dsp_mha_train_fwd", 5, 16)
        assert entry.__name__ == "dsp_mha_train_fwd" and (seed, offset, tail) == (5, 16, ())
    assert decode_ops._active_dropout_state(DEV) is None
    assert launches == [("dsp_dropout_state_advance", (st.tensor.data_ptr(), 12))]
    with st.draws():                                                            # a scope without a masked call enqueues nothing
        decode_ops._dropout_call(0.0, True, DEV)
    assert len(launches) == 1


def test_mark_and_rewind_replay_0_4(host_state):
    from daspeech_amd import decode_ops
    st, launches = host_state
    with pytest.raises(RuntimeError, match="no draws"):
        st.mark()
    with st.draws():
        m = st.mark()
        first = [decode_ops._dropout_call(0.3, True, DEV)[2] for _ in range(2)]
        st.rewind(m)
        second = [decode_ops._dropout_call(0.3, True, DEV)[2] for _ in range(2)]
        assert m == 0 and first == [0, 4] and second == [0, 4] and st.mark() == 8
        with pytest.raises(ValueError):
            st.rewind(12)                                                       # beyond what this scope has reached
    assert launches == [("dsp_dropout_state_advance", (st.tensor.data_ptr(), 8))]    # the rewound pass does not count twice


def test_same_draws_marks_then_rewinds_inside_a_scope(host_state):
    from daspeech_amd import decode_ops
    from daspeech_amd.models import daspeech
    st, _ = host_state
    seen = []
    with st.draws():
        decode_ops._dropout_call(0.3, True, DEV)                                # a masked call before the pair (the encoder)
        for _ in range(2):
            with daspeech._same_draws(1234, DEV, True):
                seen.append([decode_ops._dropout_call(0.3, True, DEV)[2] for _ in range(3)])
        assert seen == [[4, 8, 12], [4, 8, 12]] and st.mark() == 16
        with daspeech._same_draws(1234, DEV, True):                             # a third pass under the seed starts a pair of its own
            assert decode_ops._dropout_call(0.3, True, DEV)[2] == 16
        with daspeech._same_draws(1234, DEV, True):                             # its partner draws FEWER masks (none) ...
            pass
        assert st.mark() == 20                                                  # ... and leaves no spent offset to the calls behind it


def test_the_capture_question_of_the_served_rules(host_state, monkeypatch):
    """under capture a masked call is served only inside a scope on that device, an unmasked one always; no capture: always"""
    from daspeech_amd import dropout_state
    st, _ = host_state
    ok = dropout_state._capture_ok
    assert ok(DEV, True) and ok(DEV, False)
    monkeypatch.setattr(dropout_state, "_capturing", lambda: True)
    assert not ok(DEV, True) and ok(DEV, False)
    with st.draws():
        assert ok(DEV, True) and ok(DEV, False) and not ok(torch.device("cuda", 1), True)
    assert not ok(DEV, True)


def test_nesting_raises_and_a_raising_pass_is_not_advanced_over(host_state, monkeypatch):
    from daspeech_amd import decode_ops
    st, launches = host_state
    other = decode_ops.DropoutState(DEV, seed=1, offset=0)
    with st.draws():
        with pytest.raises(RuntimeError, match="do not nest"):
            with other.draws():
                pass
        with pytest.raises(RuntimeError, match="do not nest"):
            with st.draws():
                pass
        assert decode_ops._active_dropout_state(DEV) is st                      # the refused scope left the active one in place
    with pytest.raises(KeyError):
        with st.draws():
            decode_ops._dropout_call(0.3, True, DEV)
            raise KeyError("a pass that fails")
    assert decode_ops._active_dropout_state(DEV) is None and launches == []


def test_a_backward_after_its_scope_raises(host_state):
    """_BiasActDropoutTrainFn on host tensors with the launch replaced: the backward inside the scope launches the ..._state entry with the
    forward's intra, the backward of a forward whose scope has exited raises instead of drawing another mask"""
    from daspeech_amd import decode_ops
    st, launches = host_state
    fn = decode_ops._BiasActDropoutTrainFn
    h = torch.zeros(4, 8, requires_grad=True)
    with st.draws():
        decode_ops._dropout_call(0.3, True, DEV)
        y = fn.apply(h, None, decode_ops.ACT_CODES["relu"], 8, *decode_ops._dropout_call(0.3, True, DEV))
        y.backward(torch.ones_like(y))
    names = [n for n, _ in launches]
    assert names == ["dsp_act_dropout_train_fwd_state", "dsp_act_dropout_train_bwd_state", "dsp_dropout_state_advance"]
    fwd, bwd = launches[0][1], launches[1][1]
    assert fwd[6:8] == (0, 4) and fwd[-1] == st.tensor.data_ptr()             # seed unused, offset = intra, the state before the stream
    assert bwd[7:9] == (0, 4) and bwd[-1] == st.tensor.data_ptr()
    with st.draws():
        y = fn.apply(h, None, decode_ops.ACT_CODES["relu"], 8, *decode_ops._dropout_call(0.3, True, DEV))
    with pytest.raises(RuntimeError, match="scope that has exited"):
        y.backward(torch.ones_like(y))
    with st.draws():                                                            # nor inside a LATER scope of the same state
        with pytest.raises(RuntimeError, match="scope that has exited"):
            y.backward(torch.ones_like(y))


def test_outside_a_scope_the_generator_form_is_untouched(monkeypatch):
    from daspeech_amd import decode_ops
    monkeypatch.setattr(decode_ops, "_reserve_dropout_stream", lambda device: (11, 40))
    assert decode_ops._dropout_call(0.3, True, DEV) == (0.3, 11, 40)
    assert decode_ops._dropout_call(0.3, False, DEV) == (0.0, 0, 0) and decode_ops._dropout_call(0.0, True, DEV) == (0.0, 0, 0)


def test_the_new_symbols_are_declared_bound_and_exported():
    from daspeech_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "daspeech_decode.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(dsp_[a-z0-9_]+)\s*\(", text))
    build.build()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    for name in MASKED + ("dsp_dropout_keep_mask",):                          # the old entry's arguments, then rng_state, then the stream
        old, new = _lib.SIGNATURES[name], _lib.SIGNATURES[name + "_state"]
        assert new[0] is old[0] and new[1][:-2] == old[1][:-1] and len(new[1]) == len(old[1]) + 1, name
        decl = re.search(r"\b%s_state\s*\(([^;]*)\);" % name, text).group(1)
        assert re.search(r"const uint64_t\*\s*rng_state,\s*dsp_stream_t stream$", " ".join(decl.split())), name
        assert decl.count(",") + 1 == len(new[1]), name
    assert lib.dsp_abi_version() == _lib.ABI_VERSION
