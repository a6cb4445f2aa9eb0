"""Whole layers, forward and backward to every parameter, captured inside DropoutState.draws() and replayed: the HIP training operators — not
the torch lines — run under capture, every replay draws new masks, and replay r gives the BITS of an eager run of the same layer with the
default generator at (S, O + r n), n the offset one pass reserves.  FFTLayer, ConformerLayer and NATDecoderLayer in training mode with
padding masks, and the FFNAdapter and the VariancePredictor, fp16 and bf16; an fp32 FFTLayer, whose convolution and attention sites keep
their torch lines, with and without a scope; and the two-pass rule of models/daspeech.py _same_draws inside a scope."""
import pytest
import torch

pytestmark = pytest.mark.gpu

S, O = 0x5EED_0000_1234, (1 << 32) + 8
DT = {"fp16": torch.float16, "bf16": torch.bfloat16}


def dops():
    from daspeech_amd import decode_ops
    return decode_ops


def _rand(gen, shape, dtype, scale=1.0):
    return (torch.randn(shape, generator=gen, dtype=torch.float32) * scale).to(dtype).cuda()


def _pad(B, T, lens):
    return (torch.arange(T).unsqueeze(0) >= torch.tensor(lens).unsqueeze(1)).cuda()


def _fft(dtype):
    from daspeech_amd.models.fastspeech2 import FFTLayer
    g = torch.Generator().manual_seed(1)
    layer = FFTLayer(128, 2, 128, 9, 0.1, 0.1).to(device="cuda", dtype=dtype).train()
    x, pad = _rand(g, (2, 40, 128), dtype).requires_grad_(), _pad(2, 40, [40, 29])
    return layer, [x], lambda: layer(x, pad)


def _conformer(dtype):
    from daspeech_amd.models.daspeech import ConformerLayer, rel_positional_encoding
    g = torch.Generator().manual_seed(2)
    layer = ConformerLayer(128, 256, 2, 31, 0.1).to(device="cuda", dtype=dtype).train()
    x, pad = _rand(g, (2, 40, 128), dtype).requires_grad_(), _pad(2, 40, [33, 40])
    pos = rel_positional_encoding(40, 128, x.device, dtype)
    return layer, [x], lambda: layer(x, pos, pad)


def _nat(dtype):
    from daspeech_amd.models.daspeech import NATDecoderLayer
    g = torch.Generator().manual_seed(3)
    layer = NATDecoderLayer(128, 256, 2, 128, 0.1, 0.1, 0.1).to(device="cuda", dtype=dtype).train()
    x, enc = _rand(g, (2, 24, 128), dtype).requires_grad_(), _rand(g, (2, 40, 128), dtype).requires_grad_()
    self_pad, enc_pad = _pad(2, 24, [24, 17]), _pad(2, 40, [31, 40])
    return layer, [x, enc], lambda: layer(x, self_pad, enc, enc_pad)


def _adapter(dtype):
    from daspeech_amd.models.fastspeech2 import FFNAdapter
    g = torch.Generator().manual_seed(5)
    layer = FFNAdapter(128, 256, 128, 0.1).to(device="cuda", dtype=dtype).train()
    x = _rand(g, (2, 40, 128), dtype).requires_grad_()
    return layer, [x], lambda: layer(x)


def _predictor(dtype):
    from daspeech_amd.models.fastspeech2 import VariancePredictor
    g = torch.Generator().manual_seed(6)
    layer = VariancePredictor(128, 128, 3, 0.5).to(device="cuda", dtype=dtype).train()
    x = _rand(g, (2, 40, 128), dtype).requires_grad_()
    return layer, [x], lambda: layer(x)


LAYERS = {"fft": _fft, "conformer": _conformer, "nat": _nat, "adapter": _adapter, "predictor": _predictor}
# the ..._state entries a captured pass has to contain (forward and backward of each)
EXPECTED = {"fft": {"dsp_resnorm_train_state", "dsp_mha_train_state"}, "conformer": {"dsp_resnorm_train_state", "dsp_relpos_attention_train_state",
                                                                                    "dsp_act_dropout_train_state"},
            "nat": {"dsp_resnorm_train_state", "dsp_mha_train_state", "dsp_act_dropout_train_state"}, "adapter": {"dsp_act_dropout_train_state"},
            "predictor": {"dsp_act_dropout_train_state"}}


def _recorded(monkeypatch):
    """(names, undo): every launch of the host layer and the advance of a scope's exit, by entry name, in order"""
    from daspeech_amd import dropout_state
    d = dops()
    names, launch, advance = [], d._launch, dropout_state._advance
    monkeypatch.setattr(d, "_launch", lambda dev, entry, *a: (names.append(entry.__name__), launch(dev, entry, *a))[1])
    monkeypatch.setattr(dropout_state, "_advance", lambda st, by: (names.append("dsp_dropout_state_advance"), advance(st, by))[1])
    return names, lambda: (monkeypatch.setattr(d, "_launch", launch), monkeypatch.setattr(dropout_state, "_advance", advance))


def _warm(once):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            once()                                                  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)


def _build(kind, dtype):
    torch.manual_seed(11)                                           # the parameters' initial values
    layer, inputs, call = LAYERS[kind](dtype)
    leaves = inputs + [p for p in layer.parameters()]
    go = _rand(torch.Generator().manual_seed(4), tuple(call().shape), dtype)

    def step():
        y = call()
        return [y.detach()] + list(torch.autograd.grad(y, leaves, go))
    return layer, step


def _eager_reference(step, offset):
    gen = torch.cuda.default_generators[torch.cuda.current_device()]
    old = torch.cuda.get_rng_state()
    torch.cuda.manual_seed(S); gen.set_offset(offset)
    res = [t.clone() for t in step()]
    used = gen.get_offset() - offset
    torch.cuda.set_rng_state(old)
    return res, used


@pytest.mark.parametrize("dtype", list(DT))
@pytest.mark.parametrize("kind", list(LAYERS))
def test_a_captured_layer_runs_the_hip_operators_and_replays_the_eager_bits(kind, dtype, monkeypatch):
    d = dops()
    layer, step = _build(kind, DT[dtype])
    state = d.DropoutState("cuda", S, O)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            with state.draws():
                step()                                              # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    state.set(S, O)
    launched, undo = _recorded(monkeypatch)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        with state.draws():
            out = step()
            n = state.mark()
    undo()
    masked = [e for e in launched if e.endswith("_state")]
    # the feature: under capture the layer's dropout sites are the project's kernels drawing from the device state, forward and backward
    assert n >= 4 and len(masked) == 2 * (n // 4), (n, launched)
    assert launched[-1] == "dsp_dropout_state_advance"              # the graph's last node
    assert {e.replace("_fwd", "").replace("_bwd", "") for e in masked} == EXPECTED[kind]
    replays = []
    for r in range(3):
        g.replay()
        torch.cuda.synchronize()
        replays.append([t.clone() for t in out])
    assert state.get() == (S, O + 3 * n)
    for r in range(3):
        want, used = _eager_reference(step, O + r * n)
        assert used == n                                            # the eager pass reserves what the captured one did: no torch dropout beside it
        assert len(want) == len(replays[r])
        for i, (a, b) in enumerate(zip(replays[r], want)):
            assert torch.equal(a, b), f"replay {r}: result {i} differs from the eager run at offset O + {r} n"
    assert not torch.equal(replays[0][0], replays[1][0]) and not torch.equal(replays[1][0], replays[2][0])
    assert not torch.equal(replays[0][0], replays[2][0])


def test_without_a_scope_a_captured_layer_keeps_the_torch_lines(monkeypatch):
    """today's behaviour of a masked call under capture without draws(): not served"""
    d = dops()
    layer, step = _build("nat", torch.float16)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    launched, undo = _recorded(monkeypatch)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    undo()
    g.replay()
    torch.cuda.synchronize()
    assert not [e for e in launched if "resnorm" in e or "mha" in e or "act_dropout" in e], launched


@pytest.mark.parametrize("scope", [True, False], ids=["draws", "no-scope"])
def test_an_fp32_fft_layer_whose_convolutions_stay_on_torch_captures_with_and_without_a_scope(scope, monkeypatch):
    """fp32: the convolutions and the attention keep their torch lines, and _ConvFFN asks the residual site's question BEFORE its h is dense
    (with h = None as a stand-in) although the call that follows draws a mask.  Without a scope that call must not be served under capture —
    nothing may reserve from the host generator on a capturing stream —; inside a scope it is the HIP operator on the device state."""
    d = dops()
    layer, step = _build("fft", torch.float32)
    state = d.DropoutState("cuda", S, O)

    def once():
        if not scope:
            return step()
        with state.draws():
            return step()
    _warm(once)
    state.set(S, O)
    reserved, reserve = [], d._reserve_dropout_stream
    monkeypatch.setattr(d, "_reserve_dropout_stream", lambda device: (reserved.append(1), reserve(device))[1])
    launched, undo = _recorded(monkeypatch)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = once()
    undo()
    assert not reserved                                             # no host reservation while the stream was capturing
    masked = [e for e in launched if e.endswith("_state")]
    resnorm = [e for e in launched if e.startswith("dsp_resnorm_train")]
    if scope:
        assert masked == ["dsp_resnorm_train_fwd_state", "dsp_resnorm_train_bwd_state"] and launched[-1] == "dsp_dropout_state_advance"
    else:
        # the attention's residual site draws nothing (p = 0 there) and may stay on the operator; the masked site behind the convolutions may not
        assert not masked and len(resnorm) == 2, launched
    seen = []
    for r in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.isfinite(t).all() for t in out)
        seen.append(out[0].clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])      # new masks on every replay, either way
    assert state.get() == (S, O + (3 * 4 if scope else 0))


def test_same_draws_inside_a_scope_gives_both_passes_the_same_masks():
    from daspeech_amd.models.daspeech import _same_draws
    d = dops()
    layer, step = _build("nat", torch.float16)
    state = d.DropoutState("cuda", S, O)
    gen = torch.cuda.default_generators[torch.cuda.current_device()]
    before = (gen.initial_seed(), gen.get_offset())
    dev = torch.device("cuda", torch.cuda.current_device())
    with state.draws():
        with _same_draws(77, dev, True):
            first = step()
        n = state.mark()
        with _same_draws(77, dev, True):
            second = step()
        assert state.mark() == n                                    # the second pass drew the first one's offsets again
        third = step()
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    assert not torch.equal(first[0], third[0])
    assert (gen.initial_seed(), gen.get_offset()) == before         # the generator was not reseeded, nor moved
    assert state.get() == (S, O + 2 * n)                            # two distinct passes' worth, not three
    want, used = _eager_reference(step, O)
    assert used == n
    for a, b in zip(first, want):
        assert torch.equal(a, b)
