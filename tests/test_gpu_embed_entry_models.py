"""DAGDecoder.extract_features, FastSpeech2NoEmb.forward and VariancePredictor.forward in train() mode with the embedding-entry operators
(csrc/embed_entry_train.hip) and the VariancePredictor's LayerNorm -> dropout on the project's operators: switch on against switch off by the
4 x rule of tests/util_4x_rule.py against a float64 copy of the module (dropout 0), equal bits under the same seed and a gradient for every
parameter with the released dropout rates, no F.dropout call left in the three modules, and eval mode without gradient untouched by the switch."""
import copy
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.util_4x_rule import check_4x

pytestmark = pytest.mark.gpu
F16, F32 = torch.float16, torch.float32
KINDS = ("decoder", "tts", "predictor")


def D():
    from daspeech_amd import decode_ops
    return decode_ops


def _switch(kind, on):
    """the switches behind the wiring this file is about -> a function that puts them back"""
    if kind == "predictor":
        old = (D().set_residual_norm_hip(on), D().set_act_dropout_hip(on))
        return lambda: (D().set_residual_norm_hip(old[0]), D().set_act_dropout_hip(old[1]))
    old = D().set_embed_entry_hip(on)
    return lambda: D().set_embed_entry_hip(old)


def _module(kind, released):
    """(module in float64 on the CPU in train() mode, inputs, call, cotangent shapes' maker); dropout 0 unless `released`"""
    from daspeech_amd.models import daspeech as M
    from daspeech_amd.models import fastspeech2 as FS
    torch.manual_seed(3)
    if kind == "decoder":
        rates = {} if released else dict(dropout=0.0, attention_dropout=0.0, activation_dropout=0.0)
        a = SimpleNamespace(**{**M.DEFAULT_ARGS, "decoder_layers": 2, "decoder_embed_dim": 256, "decoder_ffn_embed_dim": 512,
                               "decoder_attention_heads": 4, "encoder_embed_dim": 256, "max_target_positions": 64, **rates})
        m = M.DAGDecoder(a)
        B, L, T = 3, 40, 12
        tok = torch.full((B, L), M.PAD, dtype=torch.long)
        for b, n in enumerate((40, 27, 3)):
            tok[b, :n] = M.UNK; tok[b, 0] = M.BOS; tok[b, n - 1] = M.EOS
        tok[1, 5:9] = torch.tensor([7, 9, 7, 11])                          # glanced vertices
        enc_pad = torch.arange(T).unsqueeze(0) >= torch.tensor([12, 9, 4]).unsqueeze(1)
        inputs = dict(tok=tok, enc=torch.randn(B, T, 256, dtype=torch.float64), enc_pad=enc_pad)
        call = lambda mod, i: (mod.extract_features(i["tok"], {"encoder_out": i["enc"], "encoder_padding_mask": i["enc_pad"]}),)   # noqa: E731
        used = lambda n: n.startswith(("embed_tokens", "embed_positions", "layers"))                                            # noqa: E731
    elif kind == "tts":
        rates = {} if released else dict(dropout=0.0, attention_dropout=0.0, var_pred_dropout=0.0)
        m = FS.FastSpeech2NoEmb(enc_layers=2, dec_layers=2, max_positions=200, **rates)
        B, N = 3, 30
        mask = torch.arange(N).unsqueeze(0) >= torch.tensor([30, 21, 5]).unsqueeze(1)
        dur = torch.randint(1, 4, (B, N)).masked_fill(mask, 0)
        inputs = dict(x=torch.randn(B, N, 256, dtype=torch.float64), mask=mask, dur=dur, pit=torch.randn(B, N, dtype=torch.float64),
                      ene=torch.randn(B, N, dtype=torch.float64))
        with torch.no_grad():
            m.pos_emb_alpha.fill_(0.75); m.dec_pos_emb_alpha.fill_(1.25)

        def call(mod, i):
            mel, _, _, log_dur, pitch, energy = mod(i["x"], i["mask"], i["dur"], i["pit"], i["ene"])
            return mel, log_dur, pitch, energy
        used = lambda n: True                                                                                                   # noqa: E731
    else:
        m = FS.VariancePredictor(256, 256, 3, dropout=0.5 if released else 0.0)
        inputs = dict(x=torch.randn(3, 30, 256, dtype=torch.float64))
        call = lambda mod, i: (mod(i["x"]),)                                                                                    # noqa: E731
        used = lambda n: True                                                                                                   # noqa: E731
    return m.double().train(), inputs, call, used


def _to(inputs, dtype, dev):
    return {k: (v.to(dtype) if v.is_floating_point() else v).to(dev) for k, v in inputs.items()}


def _run(m, call, inputs, used, cots=None):
    outs = call(m, inputs)
    if cots is None:
        g = torch.Generator().manual_seed(5)
        cots = [torch.randn(o.shape, generator=g, dtype=torch.float64) for o in outs]
    named = [(n, p) for n, p in sorted(m.named_parameters()) if used(n)]
    grads = torch.autograd.grad(outs, [p for _, p in named], [c.to(o.dtype).to(o.device) for c, o in zip(cots, outs)], allow_unused=True)
    res = {f"out{i}": o.detach() for i, o in enumerate(outs)}
    res.update({"d." + n: g for (n, _), g in zip(named, grads)})
    return res, cots


@pytest.mark.parametrize("dtype", [F16, F32], ids=["float16", "float32"])
@pytest.mark.parametrize("kind", KINDS)
def test_training_with_the_operators_on_and_off(kind, dtype):
    master, inputs, call, used = _module(kind, released=False)
    with torch.no_grad():
        for p in master.parameters():                                       # parameters and inputs as the dtype stores them
            p.copy_(p.to(dtype).double())
    inputs = {k: (v.to(dtype).double() if v.is_floating_point() else v) for k, v in inputs.items()}
    ref, cots = _run(copy.deepcopy(master), call, inputs, used)
    cots = [c.to(dtype).double() for c in cots]
    ref, _ = _run(copy.deepcopy(master), call, inputs, used, cots)
    assert all(v is not None for v in ref.values())                         # every parameter of the path receives a gradient
    ref = {k: v.detach().numpy() for k, v in ref.items()}
    res = {}
    for on in (True, False):
        back = _switch(kind, on)
        try:
            m = copy.deepcopy(master).to(dtype).cuda()
            res[on], _ = _run(m, call, _to(inputs, dtype, "cuda"), used, cots)
        finally:
            back()
    # the soft-max is invariant to a key bias: that gradient is zero in exact arithmetic, so max|ref| is no scale for it; its error is measured
    # against the scale of the key weight's gradient, which the same rounding residues feed (as tests/test_gpu_resnorm_autograd.py)
    scales = {}
    for name in ref:
        if name.endswith("k_proj.bias"):
            kw = name[:-4] + "weight"
            assert np.abs(ref[name]).max() < 1e-12 * np.abs(ref[kw]).max()
            scales[name] = np.abs(ref[kw]).max()
    for need in {"decoder": ("d.embed_tokens.weight", "d.embed_positions.weight"), "tts": ("d.pos_emb_alpha", "d.dec_pos_emb_alpha"),
                 "predictor": ("d.ln1.weight",)}[kind]:
        assert need in ref
    check_4x(f"embed-entry-module-{kind}", res[True], res[False], ref, scales=scales)


@pytest.mark.parametrize("kind", KINDS)
def test_released_dropout_rates_same_seed_same_bits_and_no_torch_dropout(kind, monkeypatch):
    import torch.nn.functional as F
    master, inputs, call, used = _module(kind, released=True)
    m = master.half().cuda()
    inputs = _to(inputs, F16, "cuda")

    def no_dropout(*a, **k):
        raise AssertionError("F.dropout was called")
    monkeypatch.setattr(F, "dropout", no_dropout)
    runs = []
    # the torch ops around the operators (GEMMs, embedding gradients of the variance adaptor) run on their deterministic algorithms, and the
    # first run — where the libraries settle on their kernels for a new shape — is not compared (tests/test_gpu_resnorm_autograd.py explains)
    old = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled(),
           torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark)
    torch.use_deterministic_algorithms(True, warn_only=True)
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    cots = None
    try:
        for seed in (20, 21, 21, 22):
            torch.manual_seed(seed)
            torch.cuda.manual_seed(seed)
            r, cots = _run(m, call, inputs, used, cots)
            runs.append(r)
    finally:
        torch.use_deterministic_algorithms(old[0], warn_only=old[1])
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = old[2], old[3]
    for name, v in runs[1].items():
        assert v is not None, f"{name}: no gradient"
        assert torch.isfinite(v).all(), name
        assert torch.equal(v, runs[2][name]), name                          # the same seed: the same bits
    assert any(not torch.equal(runs[2][n], runs[3][n]) for n in runs[2] if n.startswith("out"))       # another seed: another mask


@pytest.mark.parametrize("kind", KINDS)
def test_eval_without_gradient_does_not_see_the_switch(kind):
    master, inputs, call, used = _module(kind, released=True)
    m = master.float().cuda().eval()
    inputs = _to(inputs, F32, "cuda")
    outs = {}
    for on in (True, False):
        back = _switch(kind, on)
        try:
            with torch.no_grad():
                outs[on] = call(m, inputs)
        finally:
            back()
    for a, b in zip(outs[True], outs[False]):
        assert torch.equal(a, b)
