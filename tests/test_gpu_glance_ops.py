"""The glancing kernels (csrc/glance.hip) behind decode_ops.force_emit / decode_ops.glance_select and their use by the criteria.  The reference of
every check is the torch formulation the criteria used before, run in the same process with decode_ops.set_glance_hip(False); every comparison
is torch.equal — the kernels copy and select values, they compute none."""
from contextlib import contextmanager

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NINF = float("-inf")
FE_SHAPES = [(1, 1, 1), (2, 3, 5), (3, 7, 6), (2, 5, 7), (2, 4, 64), (2, 9, 259), (1, 33, 1030)]            # (B, T, L)
GS_SHAPES = [(1, 1, 1), (2, 5, 3), (3, 64, 9), (2, 257, 40), (2, 1030, 130), (1, 4100, 300)]              # (B, L, T)


@contextmanager
def torch_formulation():
    from daspeech_amd import decode_ops
    old = decode_ops.set_glance_hip(False)
    try:
        yield
    finally:
        decode_ops.set_glance_hip(old)


def _gen(*key):
    return torch.Generator(device="cuda").manual_seed(sum(int(k) * 1000 ** i for i, k in enumerate(key)) + 17)


def _path_and_masks(B, T, L, gen):
    """path [B,L] in [-1, T) and the three reveal masks; vertex L-1 of sample 0 has no alignment and is revealed in `all` and `random`"""
    path = torch.randint(-1, T, (B, L), device="cuda", generator=gen)
    path[0, L - 1] = -1
    rnd = torch.rand(B, L, device="cuda", generator=gen) < 0.4
    rnd[0, L - 1] = True
    return path, {"none": torch.zeros(B, L, dtype=torch.bool, device="cuda"), "all": torch.ones(B, L, dtype=torch.bool, device="cuda"), "random": rnd}


def _match_input(kind, B, T, L, gen):
    """[B,T,L] emission scores, some cells already -inf, in the layout `kind`"""
    from daspeech_amd import custom_ops
    if kind == "gather":                     # the real gather's output: an fp32 view with rows pitched to a multiple of 4
        V = 11
        logits = torch.randn(B, L, V, device="cuda", generator=gen) * 2
        logits[:, ::3, 4] = NINF             # token 4 is impossible at every third vertex: -inf cells in the match
        tgt = torch.randint(0, V, (B, T), device="cuda", generator=gen)
        tgt[:, 0] = 4
        with torch.no_grad():
            m = custom_ops.dag_logsoftmax_gather_inplace(logits, tgt.unsqueeze(1).expand(-1, L, -1))[1].transpose(1, 2)
        assert torch.isneginf(m).any()
        return m
    x = torch.randn(B * T * L + 1, device="cuda", generator=gen) * 2 - 3
    x[torch.rand(x.shape, device="cuda", generator=gen) < 0.1] = NINF
    x[1] = NINF
    if kind == "dense":
        return x[:-1].view(B, T, L).clone()
    if kind == "offset1":                    # storage offset 1: a base no 16-byte access can take
        m = x[1:].view(B, T, L)
        assert m.data_ptr() % 16 == 4
        return m
    assert kind == "f64"
    return x[:-1].view(B, T, L).double()


@pytest.mark.parametrize("kind", ["gather", "dense", "offset1", "f64"])
@pytest.mark.parametrize("shape", FE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_force_emit_forward_equals_the_torch_expression(shape, kind):
    from daspeech_amd import decode_ops
    from daspeech_amd.custom_ops.dag_loss import _round4, _row_pitch
    B, T, L = shape
    gen = _gen(B, T, L, len(kind))
    m = _match_input(kind, B, T, L, gen)
    path, masks = _path_and_masks(B, T, L, gen)
    if kind == "gather" and L % 4:
        assert _row_pitch(m) == _round4(L) and (B * T == 1 or not m.is_contiguous())
    snapshot = m.clone()
    for name, revealed in masks.items():
        assert decode_ops.force_emit_served(m, path, revealed), name
        out = decode_ops.force_emit(m, path, revealed)
        with torch_formulation():
            assert not decode_ops.force_emit_served(m, path, revealed)
            want = decode_ops.force_emit(m, path, revealed)
        assert out.dtype == m.dtype and out.shape == m.shape
        assert torch.equal(out, want), (name, int((out != want).sum()))
        assert torch.equal(m, snapshot)                                            # out of place
        if name != "none":
            assert torch.isneginf(out[0, :, L - 1]).all()                          # revealed, path = -1: a column of -inf
        if m.dtype == torch.float32:
            assert _row_pitch(out) == _round4(L), (name, out.stride())             # what the DP ops take without a copy, for every L
        else:
            assert out.is_contiguous()


def _grad_out(kind, B, T, L, dtype, gen):
    if kind == "dense":
        return torch.randn(B, T, L, device="cuda", generator=gen).to(dtype)
    if kind == "transposed":
        return torch.randn(B, L, T, device="cuda", generator=gen).to(dtype).transpose(1, 2)
    if kind == "pitched":
        return torch.randn(B, T, L + 5, device="cuda", generator=gen).to(dtype)[:, :, 2:L + 2]
    assert kind == "broadcast"               # what sum().backward() hands down: every stride zero
    return torch.randn((), device="cuda", generator=gen).to(dtype).expand(B, T, L)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", FE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_force_emit_backward_equals_autograd_of_the_torch_expression(shape, dtype):
    from daspeech_amd import decode_ops
    B, T, L = shape
    gen = _gen(B, T, L, 5)
    m = (torch.randn(B, T, L, device="cuda", generator=gen) * 2 - 3).to(dtype)
    path, masks = _path_and_masks(B, T, L, gen)
    assert decode_ops.force_emit_served(m, path, masks["all"])
    for name, revealed in masks.items():
        for gk in ("dense", "transposed", "pitched", "broadcast"):
            g = _grad_out(gk, B, T, L, dtype, gen)
            a = m.clone().requires_grad_()
            decode_ops.force_emit(a, path, revealed).backward(g)
            b = m.clone().requires_grad_()
            with torch_formulation():
                decode_ops.force_emit(b, path, revealed).backward(g)
            assert torch.equal(a.grad, b.grad), (name, gk)
            assert torch.equal(a.grad, g.masked_fill(revealed.unsqueeze(1), 0)), (name, gk)


# ---------------------------------------------------------------------------------------------------------------- chain
def _chain(logits0, links0, tgt, ol, tl, path, revealed):
    """gather -> force_emit -> dag_loss -> backward: (loss, d logits, d links)"""
    from daspeech_amd import custom_ops, decode_ops
    leaf = logits0.clone().requires_grad_()
    links = links0.clone().requires_grad_()
    L = leaf.shape[1]
    _, match = custom_ops.dag_logsoftmax_gather_inplace(leaf.clone(), tgt.unsqueeze(1).expand(-1, L, -1))
    m = decode_ops.force_emit(match.transpose(1, 2), path, revealed)
    loss = custom_ops.dag_loss(m, links, ol, tl)
    (loss / tl).sum().backward()
    return loss.detach(), leaf.grad, links.grad


@pytest.mark.parametrize("L,TR", [(30, 8), (32, 8), (259, 32)])
def test_chain_gather_force_emit_dag_loss_backward(L, TR):
    """The gradients reaching the logits and the links through force_emit against the same chain on the torch expression.  The parent chain
    is run twice first: it is bit-stable (every kernel on it is a HIP kernel of this library with a fixed summation order; measured on an
    MI355X: zero difference between the two parent runs in loss, logits gradient and links gradient for all three shapes), so the
    comparison is torch.equal."""
    from daspeech_amd import custom_ops
    from tests.util_inputs import make_dag_inputs
    B, T, V = 3, 16, 40                                  # (the shortest target still reaches the last vertex within its window)
    _, links, ol, tl = make_dag_inputs(L, B, T, L, TR)
    gen = _gen(L, TR)
    logits = torch.randn(B, L, V, device="cuda", generator=gen) * 2
    tgt = torch.randint(2, V, (B, T), device="cuda", generator=gen)
    links, ol, tl = torch.from_numpy(links).cuda(), torch.from_numpy(ol).cuda(), torch.from_numpy(tl).cuda()
    with torch.no_grad():
        match = custom_ops.dag_logsoftmax_gather_inplace(logits.clone(), tgt.unsqueeze(1).expand(-1, L, -1))[1].transpose(1, 2)
        path = custom_ops.dag_best_alignment(match, links, ol, tl)
    revealed = (torch.rand(B, L, device="cuda", generator=gen) < 0.5) & (path >= 0)
    assert revealed.any()
    with torch_formulation():
        p1 = _chain(logits, links, tgt, ol, tl, path, revealed)
        p2 = _chain(logits, links, tgt, ol, tl, path, revealed)
    new = _chain(logits, links, tgt, ol, tl, path, revealed)
    assert torch.isfinite(p1[0]).all() and p1[1].abs().sum() > 0 and p1[2].abs().sum() > 0
    for name, a, b, c in zip(("loss", "grad_logits", "grad_links"), p1, p2, new):
        d_parent = float((a - b).abs().nan_to_num(0).max())
        print(f"chain L={L} TR={TR} {name}: parent vs parent {d_parent:.3e}, new vs parent {float((c - a).abs().nan_to_num(0).max()):.3e}")
        assert torch.equal(a, b), f"{name}: the parent chain is not bit-stable ({d_parent:.3e})"
        assert torch.equal(c, a), name


# ---------------------------------------------------------------------------------------------------------------- reveal selection
def _alignment(B, L, T, n_tgt, gen, dead_sample):
    """a valid alignment per sample: n_tgt[b] vertices, in order, carry targets 0 .. n_tgt[b]-1; `dead_sample` has none (all -1)"""
    path = torch.full((B, L), -1, dtype=torch.long, device="cuda")
    for b in range(B):
        if b == dead_sample:
            continue
        n = int(n_tgt[b])
        pos = torch.randperm(L, device="cuda", generator=gen)[:n].sort().values
        path[b, pos] = torch.arange(n, device="cuda")
    return path


def _select_inputs(B, L, T, guess_mode, dead_sample):
    gen = _gen(B, L, T, len(guess_mode), dead_sample + 2)
    V = 50
    n_tgt = torch.randint(max(1, min(T, L) - 3), min(T, L) + 1, (B,), device="cuda", generator=gen)
    tgt = torch.randint(4, V, (B, T), device="cuda", generator=gen)
    path = _alignment(B, L, T, n_tgt, gen, dead_sample)
    oracle = tgt.gather(-1, path.clip(min=0))
    guess = torch.randint(4, V, (B, L), device="cuda", generator=gen)
    if guess_mode == "half":
        guess = torch.where(torch.rand(B, L, device="cuda", generator=gen) < 0.5, oracle, guess)
    else:
        guess = oracle + 1                                                         # nothing right: counts reach the number of aligned vertices
    prev = torch.randint(0, 4, (B, L), device="cuda", generator=gen)
    levels = torch.tensor([-1.0, -0.0, 0.0, 0.5, 1.0], device="cuda")               # ties straddle every threshold
    noise = levels[torch.randint(0, 5, (B, L), device="cuda", generator=gen)]
    unif = torch.rand(B, L, device="cuda", generator=gen)
    return tgt, path, guess, prev, n_tgt, noise, unif


def _both(*args, **kw):
    from daspeech_amd import decode_ops
    got = decode_ops.glance_select(*args, **kw)
    with torch_formulation():
        want = decode_ops.glance_select(*args, **kw)
    for key in ("oracle", "n_right", "keep_prob", "revealed", "glanced"):
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, key
        assert torch.equal(got[key], want[key]), (key, int((got[key] != want[key]).sum()))
    return got


@pytest.mark.parametrize("shape", GS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_glance_select_equals_the_torch_formulation(shape):
    from daspeech_amd import decode_ops
    B, L, T = shape
    for guess_mode, dead in (("half", -1), ("none", -1), ("half", 0)):
        tgt, path, guess, prev, n_tgt, noise, unif = _select_inputs(B, L, T, guess_mode, dead)
        assert decode_ops._glance_served(tgt, path, guess, prev, unif)
        aligned = (path >= 0).sum(1)
        # counts of number-random = int((n_tgt - n_right) * p + 0.5): p = 0 gives 0; p = 1 with nothing right gives the number of aligned
        # vertices; p_beyond pushes them past it, up to the row length (the torch formulation cannot index beyond L)
        p_beyond = min(3.0, L / int(n_tgt.max()))
        for p in (0.0, 0.5, 1.0, p_beyond):
            got = _both(tgt, path, guess, prev, n_tgt, p, "number-random", noise=noise, unif=unif)
            counts = ((n_tgt - got["n_right"]) * p + 0.5).long()
            assert int(counts.max()) <= L
            kept = got["keep_prob"].sum(1).long()
            assert bool(((kept >= counts) | (counts > aligned)).all())
            if p == 0.0:
                assert not got["keep_prob"].any() and not got["revealed"].any() and torch.equal(got["glanced"], prev)
            if p == 1.0 and guess_mode == "none" and dead < 0:
                assert torch.equal(counts, aligned) and torch.equal(got["keep_prob"], (path >= 0).float())
            if p == p_beyond and dead == 0:
                assert bool(got["keep_prob"][0].all())                             # no alignment: every score is the fill, the whole row is kept
        for unif_n in (torch.zeros(B, device="cuda"), torch.rand(B, device="cuda", generator=_gen(B, L, 3)), torch.full((B,), 0.999, device="cuda")):
            _both(tgt, path, guess, prev, n_tgt, 0.5, "cmlm", noise=noise, unif=unif, unif_n=unif_n)
        for p in (0.0, 0.3, 1.0):
            _both(tgt, path, guess, prev, n_tgt, p, None, unif=unif)


def test_glat_function_keeps_its_contract_on_the_hip_ops():
    """signature, return value and glat_info keys of criterions.glat_function do not depend on the switch; nor do the values"""
    from types import SimpleNamespace
    from daspeech_amd.criterions import glat_function
    from tests.util_inputs import make_dag_inputs
    B, L, T, TR, V, PAD = 4, 61, 13, 16, 40, 1
    rng = np.random.default_rng(5)
    _, links, ol, tl = make_dag_inputs(9, B, T, L, TR)
    logits = (rng.standard_normal((B, L, V)) * 2).astype(np.float32)
    prev = np.full((B, L), 3, np.int64); prev[np.arange(L)[None] >= ol[:, None]] = PAD
    tgt = rng.integers(4, V, (B, T)); tgt[np.arange(T)[None] >= tl[:, None]] = PAD
    t = lambda a: torch.from_numpy(a).cuda()
    noise, unif = torch.randn(B, L, device="cuda", generator=_gen(1)), torch.rand(B, L, device="cuda", generator=_gen(2))
    run = lambda: glat_function(SimpleNamespace(pad=PAD), t(logits), t(tgt), t(prev), {"context_p": 0.5}, links=t(links),
                                glance_strategy="number-random", noise=noise, unif=unif)
    got = run()
    with torch_formulation():
        want = run()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and sorted(got[2]) == sorted(want[2])
    for key, v in want[2].items():
        assert (torch.equal(got[2][key], v) if torch.is_tensor(v) else got[2][key] == v), key
    assert got[2]["keep_word_mask"].any()


# ---------------------------------------------------------------------------------------------------------------- criteria
# With torch's layers on their default algorithms the model around the DAG ops is not bit-reproducible on the GPU: two runs of the PARENT
# formulation differed in the last bit of the loss and in the gradients, so the step runs under deterministic_torch() below.  Measured on an
# MI355X: with it, 8 parent runs of each criterion agree bit for bit (28 pairs) and the test demands torch.equal.  Should the parent runs of
# the test itself ever differ, the bound is the largest difference seen between parent runs WITHOUT deterministic_torch() on that machine,
# every pair of 8 runs plus the pair of an earlier process, in the measure of _spread — (relative loss difference, gradient difference):
# nat 7.5e-8 (203.78855895996094 against 203.78857421875), 4.77e-4; s2s 8.8e-8 (348.2511901855469 against 348.251220703125), 1.19e-3.
PARENT_SPREAD = {"nat": (7.5e-8, 4.77e-4), "s2s": (8.8e-8, 1.19e-3)}
PARENT_RUNS = 8


def _spread(a, b):
    """(relative loss difference, largest gradient difference over the parameters: per parameter, relative to its own largest entry plus
    1e-3 of the largest entry of the whole gradient — a parameter whose gradient is mathematically zero holds rounding noise on both sides)"""
    (la, ga), (lb, gb) = a, b
    gscale = max(float(g.abs().max()) for g in ga.values())
    worst = max(float((ga[n] - gb[n]).abs().max()) / (float(ga[n].abs().max()) + 1e-3 * gscale) for n in ga)
    return abs(float(la) - float(lb)) / abs(float(la)), worst


@contextmanager
def deterministic_torch(on=True):
    """torch's own layers on their deterministic algorithms where they have one (embedding / index / scatter backwards, convolution
    algorithms): takes most of the run-to-run noise out of the model around the DAG ops"""
    old = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled(),
           torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark)
    if on:
        torch.use_deterministic_algorithms(True, warn_only=True)
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(old[0], warn_only=old[1])
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = old[2], old[3]


def _criterion_runs(kind, parents=2, deterministic=True):
    """-> ([parent runs], new run), a run = (loss, {parameter: gradient})"""
    with deterministic_torch(deterministic):
        return _criterion_runs_inner(kind, parents)


def _criterion_runs_inner(kind, parents):
    from daspeech_amd.criterions import NATDAGLoss, S2SDAGFastSpeech2Loss
    from daspeech_amd.models.daspeech import S2SConformerDAGFastSpeech2Model, S2TConformerDAGModel
    from daspeech_amd.synthetic import make_s2st_batch
    torch.manual_seed(0)
    if kind == "nat":
        m = S2TConformerDAGModel(encoder_layers=2, decoder_layers=1).cuda().eval()            # eval: no dropout -> the draws below are the only ones
        s = make_s2st_batch(3, "cuda", seed=6, min_frames=100, max_frames=150)
        s["target"] = s["target_text"]
        crit = NATDAGLoss(glat_p="0.5", glance_strategy="number-random")
    else:
        m = S2SConformerDAGFastSpeech2Model(encoder_layers=2, decoder_layers=1, tts=dict(enc_layers=1, dec_layers=1)).cuda().eval()
        s = make_s2st_batch(3, "cuda", seed=1, min_frames=120, max_frames=200)
        crit = S2SDAGFastSpeech2Loss(glat_p="0.5", glance_strategy="number-random", tts_loss_weight=5.0)
    s["update_num"] = 1000
    crit.train()
    shape = m.initialize_output_tokens_by_tokens(s["net_input"]["src_tokens"], s["net_input"]["src_lengths"]).shape
    crit.glat_draws = {"noise": torch.randn(shape, device="cuda", generator=_gen(3)), "unif": torch.rand(shape, device="cuda", generator=_gen(4))}
    seen = {}
    fwd = m.forward

    def spy(*a, **k):
        out = fwd(*a, **k)
        seen["revealed"] = int(out["keep_word_mask"].sum())
        return out
    m.forward = spy

    def run():
        torch.manual_seed(123)
        m.zero_grad(set_to_none=True)
        loss, _, log = crit(m, s)
        loss.backward()
        assert torch.isfinite(loss) and seen["revealed"] > 0
        return loss.detach(), {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
    with torch_formulation():
        olds = [run() for _ in range(parents)]
    return olds, run()


@pytest.mark.parametrize("kind", ["nat", "s2s"])
def test_criterion_step_equals_the_parent_formulation(kind):
    """One NATDAGLoss / S2SDAGFastSpeech2Loss step (glat on, number-random, fixed draws): loss and every parameter gradient, switch on against
    switch off.  Rule as in the chain test: torch.equal where the parent is bit-stable (it is under deterministic_torch(), see PARENT_SPREAD),
    else the recorded parent-vs-parent spread."""
    (p1, p2), new = _criterion_runs(kind)
    assert p1[1].keys() == p2[1].keys() == new[1].keys() and len(p1[1]) > 50
    parent, got = _spread(p1, p2), _spread(p1, new)
    print(f"criterion {kind}: loss parent {float(p1[0])!r} {float(p2[0])!r} new {float(new[0])!r}; (loss, gradient) spread parent vs parent "
          f"{parent[0]:.3e} {parent[1]:.3e}, new vs parent {got[0]:.3e} {got[1]:.3e}")
    if torch.equal(p1[0], p2[0]) and all(torch.equal(p1[1][n], p2[1][n]) for n in p1[1]):
        assert torch.equal(new[0], p1[0])
        for n in p1[1]:
            assert torch.equal(new[1][n], p1[1][n]), n
    else:
        assert got[0] <= PARENT_SPREAD[kind][0] and got[1] <= PARENT_SPREAD[kind][1], (got, parent, PARENT_SPREAD[kind])
