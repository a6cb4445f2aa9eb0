"""The six masked training operators with the dropout state on the device (decode_ops.DropoutState), eagerly and in a captured graph.

The reference of every case is the operator's host-integer form, eagerly, with the default generator set to (S, O + 4k): inside
state.draws() with the state at (S, O) the k-th masked call has to give the SAME BITS, outputs and every gradient — eagerly, and captured
once and replayed three times (each replay k of the step's n / 4 masked calls against O + r n + 4k), after which the state holds
(S, O + 3n).  O has bit 32 set, so that a dropped high word of state[1] + intra shows.  Shapes are the smallest that cross each kernel's
internal boundaries (several workgroups, a C that is no power of two, T no multiple of 4, the long-list path of the embedding backward)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

S, O, P = 0x1234_5678_9ABC, (1 << 32) + 8, 0.3
CALLS = 2                                          # masked calls of one step: intra 0 and 4, n = 8
DT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}


def dops():
    from daspeech_amd import decode_ops
    return decode_ops


def _rand(gen, shape, dtype, scale=1.0):
    return (torch.randn(shape, generator=gen, dtype=torch.float32) * scale).to(dtype).cuda()


def _resnorm(shape, dtype):
    g = torch.Generator().manual_seed(sum(shape))
    C = shape[-1]
    ln = torch.nn.LayerNorm(C).to(device="cuda", dtype=dtype)
    with torch.no_grad():
        ln.weight.copy_(_rand(g, (C,), dtype, 0.5) + 1); ln.bias.copy_(_rand(g, (C,), dtype, 0.1))
    leaves = [_rand(g, shape, dtype).requires_grad_(), _rand(g, shape, dtype).requires_grad_(), _rand(g, (C,), dtype, 0.3).requires_grad_(),
              ln.weight, ln.bias]
    return leaves, lambda: dops().residual_dropout_layer_norm_autograd(leaves[0], leaves[1], ln, bias=leaves[2], alpha=0.5, p=P, training=True)


def _actdrop(shape, act, dtype):
    g = torch.Generator().manual_seed(sum(shape))
    leaves = [_rand(g, shape, dtype).requires_grad_(), _rand(g, shape[-1:], dtype, 0.3).requires_grad_()]
    return leaves, lambda: (dops().bias_act_dropout_autograd(leaves[0], leaves[1], act, p=P, training=True),)


def _embed(L, dtype):
    g = torch.Generator().manual_seed(L)
    V, C, pad = 11, 16, 1
    tok = torch.full((2, L), pad, dtype=torch.int64)
    if L == 9:
        tok[0, 4:] = torch.tensor([0, 3, 3, 7, 2])            # a left-padded row; row 1 stays all pad
    else:
        tok[0, 3:] = 3; tok[1, :5] = torch.tensor([0, 3, 10, 3, 2])      # 67 rows of one token: the long-list path of the backward
    tok = tok.cuda()
    leaves = [_rand(g, (V, C), dtype).requires_grad_(), _rand(g, (L + pad + 1, C), dtype).requires_grad_()]
    return leaves, lambda: (dops().embed_entry_autograd(tok, leaves[0], leaves[1], pad, 4.0, p=P, training=True),)


def _posadd(dtype):
    g = torch.Generator().manual_seed(3)
    mask = torch.zeros(2, 9, dtype=torch.bool); mask[0, 6:] = True; mask[1, :2] = True
    mask, table = mask.cuda(), _rand(g, (12, 16), dtype)
    leaves = [_rand(g, (2, 9, 16), dtype).requires_grad_(), torch.tensor([0.7], dtype=dtype, device="cuda").requires_grad_()]
    return leaves, lambda: (dops().positional_add_dropout_autograd(leaves[0], mask, table, leaves[1], p=P, training=True),)


def _relpos(dtype):
    g = torch.Generator().manual_seed(5)
    B, T, H = 2, 37, 2
    mask = torch.zeros(B, T, dtype=torch.bool); mask[1, 30:] = True
    mask = mask.cuda()
    leaves = [_rand(g, (B, T, H * 64), dtype, 0.5).requires_grad_() for _ in range(3)]
    leaves += [_rand(g, (2 * T - 1, H * 64), dtype, 0.5).requires_grad_(), _rand(g, (H, 64), dtype, 0.3).requires_grad_(),
               _rand(g, (H, 64), dtype, 0.3).requires_grad_()]
    return leaves, lambda: (dops().relpos_attention_autograd(*leaves, mask, H, p=P, training=True),)


def _mha(dtype):
    g = torch.Generator().manual_seed(6)
    B, N, M, H = 2, 5, 70, 2
    mask = torch.zeros(B, M, dtype=torch.bool); mask[0, 61:] = True
    mask = mask.cuda()
    leaves = [_rand(g, (B, N, H * 64), dtype, 0.5).requires_grad_(), _rand(g, (B, M, H * 64), dtype, 0.5).requires_grad_(),
              _rand(g, (B, M, H * 64), dtype, 0.5).requires_grad_()]
    return leaves, lambda: (dops().mha_attention_autograd(*leaves, mask, H, p=P, training=True),)


CASES = {}
for _d in ("fp32", "fp16", "bf16"):
    CASES[f"resnorm-3x5x24-{_d}"] = lambda d=_d: _resnorm((3, 5, 24), DT[d])
    CASES[f"resnorm-2x70x512-{_d}"] = lambda d=_d: _resnorm((2, 70, 512), DT[d])
    CASES[f"actdrop-glu-67x80-{_d}"] = lambda d=_d: _actdrop((67, 80), "glu", DT[d])
    CASES[f"actdrop-silu-130x64-{_d}"] = lambda d=_d: _actdrop((130, 64), "silu", DT[d])
for _d in ("fp16", "bf16"):
    CASES[f"embed-L9-{_d}"] = lambda d=_d: _embed(9, DT[d])
    CASES[f"embed-L70-{_d}"] = lambda d=_d: _embed(70, DT[d])
    CASES[f"posadd-{_d}"] = lambda d=_d: _posadd(DT[d])
    CASES[f"relpos-T37-{_d}"] = lambda d=_d: _relpos(DT[d])
    CASES[f"mha-5x70-{_d}"] = lambda d=_d: _mha(DT[d])

_BUILT = {}


def case(name):
    """(leaves, step, reference): step() runs CALLS masked calls, forward and backward to every leaf, and returns all results; reference(r)
    is what the eager host-integer step gives with the generator at (S, O + 4 CALLS r), computed once per r and kept unchanged"""
    if name in _BUILT:
        return _BUILT[name]
    leaves, call = CASES[name]()
    probe = call()
    gen = torch.Generator().manual_seed(99)
    gos = [_rand(gen, tuple(o.shape), o.dtype) for o in probe]

    def step():
        res = []
        for _ in range(CALLS):
            outs = call()
            res += [o.detach() for o in outs] + list(torch.autograd.grad(outs, leaves, gos))
        return res
    refs = {}

    def reference(r):
        if r not in refs:
            gen_ = torch.cuda.default_generators[torch.cuda.current_device()]
            old = torch.cuda.get_rng_state()
            torch.cuda.manual_seed(S); gen_.set_offset(O + 4 * CALLS * r)
            assert dops()._active_dropout_state("cuda") is None
            refs[r] = [t.clone() for t in step()]
            assert gen_.get_offset() == O + 4 * CALLS * (r + 1)
            torch.cuda.set_rng_state(old)
        return refs[r]
    _BUILT[name] = (leaves, step, reference)
    return _BUILT[name]


def same(got, want, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), f"{what}: result {i} differs"


@pytest.mark.parametrize("name", list(CASES))
def test_eager_calls_inside_draws_equal_the_host_integer_calls(name):
    _, step, reference = case(name)
    state = dops().DropoutState("cuda", S, O)
    gen = torch.cuda.default_generators[torch.cuda.current_device()]
    before = gen.get_offset()
    for r in range(2):                                              # the second scope starts where the first one's advance left the state
        with state.draws():
            got = step()
        same(got, reference(r), f"scope {r}")
    assert state.get() == (S, O + 2 * 4 * CALLS) and gen.get_offset() == before
    want = reference(0)
    per = len(want) // CALLS
    assert not torch.equal(want[0], want[per])                      # the k-th call of a scope has a mask of its own


@pytest.mark.parametrize("name", list(CASES))
def test_captured_and_replayed_calls_equal_the_host_integer_calls(name):
    _, step, reference = case(name)
    state = dops().DropoutState("cuda", S, O + 400)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            with state.draws():
                step()                                              # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    state.set(S, O)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        with state.draws():
            out = step()
    assert state.get() == (S, O)                                    # recorded, not run
    for r in range(3):
        g.replay()
        torch.cuda.synchronize()
        same(out, reference(r), f"replay {r}")
    assert state.get() == (S, O + 3 * 4 * CALLS)


def test_the_device_form_of_the_keep_mask_equals_the_host_form():
    d = dops()
    state = d.DropoutState("cuda", S, O)
    for shape, intra in (((3, 5, 24), 0), ((2, 2, 37, 40), 4), ((1030,), 8)):
        assert torch.equal(d.dropout_keep_mask(state, intra, P, shape), d.dropout_keep_mask(S, O + intra, P, shape, "cuda"))
    state.set((1 << 64) - 3, O)                                     # a seed with its top bit set goes through the int64 tensor unharmed
    assert state.get() == ((1 << 64) - 3, O)
    assert torch.equal(d.dropout_keep_mask(state, 4, P, (9, 16)), d.dropout_keep_mask((1 << 64) - 3, O + 4, P, (9, 16), "cuda"))
    frac = d.dropout_keep_mask(state, 0, P, (1 << 16,)).float().mean().item()
    assert abs(frac - (1 - P)) < 0.01
