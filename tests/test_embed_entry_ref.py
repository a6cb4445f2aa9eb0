"""CPU: the float64 restatement of the embedding-entry operators (tests/util_embed_entry_ref.py) against torch autograd of the models' own
lines in float64, and the surface of the operators — the decode_ops names, what the `served` questions decline, what the public functions
refuse, the header's constants, and that DAGDecoder.extract_features, FastSpeech2NoEmb.forward and VariancePredictor.forward on CPU compute the
bits of the lines they had before the operators were wired in (the operators are a GPU path)."""
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from daspeech_amd import _lib, decode_ops
from daspeech_amd.models import daspeech as M
from daspeech_amd.models import fastspeech2 as FS
from tests import util_embed_entry_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12


def _close(a, b):
    sc = max(np.abs(b).max(), 1.0)
    assert np.abs(a - b).max() <= TOL * sc, np.abs(a - b).max() / sc


def _token_cases():
    for name in R.TOKEN_CASES:
        yield name, (lambda V, name=name: R.token_case(name, V))
    for c in R.HOT_COUNTS:
        yield f"hot-{c}", (lambda V, c=c: R.hot_key_case(c, V))


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("name,make", list(_token_cases()))
def test_token_entry_restatement_against_torch_autograd(name, make, masked):
    V, C, scale = 512, 8, math.sqrt(8)
    tok = make(V)
    B, L = tok.shape
    NP = L + R.PAD + 1 + (3 if B > 1 else 0)
    rng = np.random.default_rng(1)
    E, P = rng.standard_normal((V, C)), rng.standard_normal((NP, C))
    dy = rng.standard_normal((B, L, C))
    keep = rng.random((B * L, C)) >= 0.5 if masked else None
    ks = 2.0 if masked else 1.0
    ref = R.embed_entry_ref(tok, E, P, R.PAD, scale, keep, ks, dy)
    # torch: an out-of-range token reads an extra zero row appended to the table (torch itself raises on such a token)
    inside = (tok >= 0) & (tok < V)
    Et = torch.tensor(E, requires_grad=True)
    Pt = torch.tensor(P, requires_grad=True)
    Ex = torch.cat([Et, torch.zeros(1, C, dtype=torch.float64)])
    y = R.torch_embed_entry(torch.tensor(np.where(inside, tok, V)), Ex, Pt, R.PAD, scale, None if keep is None else torch.tensor(keep), ks)
    dE, dP = torch.autograd.grad(y, [Et, Pt], torch.tensor(dy))
    _close(ref["y"], y.detach().numpy()); _close(ref["dE"], dE.numpy()); _close(ref["dP"], dP.numpy())
    assert not ref["dE"][R.PAD].any() and not ref["dP"][R.PAD].any()


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("B,N,NT", [(1, 1, 4), (3, 63, 70), (3, 65, 40), (3, 130, 200)])
def test_positional_add_restatement_against_torch_autograd(B, N, NT, masked):
    C = 8
    rng = np.random.default_rng(2)
    x, tab, dy = rng.standard_normal((B, N, C)), rng.standard_normal((NT, C)), rng.standard_normal((B, N, C))
    tab[1] = 0.0
    mask = np.zeros((B, N), bool)
    if B > 1:
        mask[1, N // 2:] = True; mask[2, :] = True; mask[0, 3:5] = True
    keep = rng.random((B * N, C)) >= 0.1 if masked else None
    ks = 1.0 / 0.9 if masked else 1.0
    ref = R.pos_add_ref(x, mask, tab, 0.75, keep, ks, dy)
    xt, at = torch.tensor(x, requires_grad=True), torch.tensor([0.75], dtype=torch.float64, requires_grad=True)
    y = R.torch_pos_add(xt, torch.tensor(mask), torch.tensor(tab), at, None if keep is None else torch.tensor(keep), ks)
    dx, da = torch.autograd.grad(y, [xt, at], torch.tensor(dy))
    _close(ref["y"], y.detach().numpy()); _close(ref["dx"], dx.numpy()); _close(ref["dalpha"], da.numpy())


def test_hot_key_cases_hold_the_counts_they_name():
    for V in (7, 512, 8192):
        for c in R.HOT_COUNTS:
            t = R.hot_key_case(c, V)
            assert (t == R.UNK).sum() == c and t.shape == (3, 130) and (t[:, -1] == R.PAD).all() and t.max() < V


# ---------------------------------------------------------------- the surface
def test_names_constants_and_header():
    for n in ("set_embed_entry_hip", "embed_entry_served", "embed_entry_checked", "embed_entry_autograd", "positional_add_dropout_served",
              "positional_add_dropout_checked", "positional_add_dropout_autograd"):
        assert callable(getattr(decode_ops, n)), n
    assert decode_ops.EMBED_ENTRY_HIP is True
    text = open(os.path.join(ROOT, "include", "daspeech_decode.h")).read()
    for macro, val in (("DSP_EMBED_ENTRY_MAX_C", decode_ops.EMBED_ENTRY_MAX_C), ("DSP_EMBED_ENTRY_SORT_MAX", decode_ops.EMBED_ENTRY_SORT_MAX),
                       ("DSP_POS_ADD_CHUNK_ROWS", decode_ops.POS_ADD_CHUNK_ROWS), ("DSP_EMBED_ENTRY_SORT_MAX", R.SORT_MAX),
                       ("DSP_EMBED_GRAD_CHUNK", R.GRAD_CHUNK)):
        assert int(re.search(rf"#define {macro} (\d+)", text).group(1)) == val, macro
    for n in ("dsp_embed_entry_fwd", "dsp_embed_entry_bwd", "dsp_embed_entry_bwd_workspace_bytes", "dsp_pos_add_fwd", "dsp_pos_add_bwd",
              "dsp_pos_add_bwd_workspace_bytes"):
        assert n in _lib.SIGNATURES and re.search(rf"\b{n}\s*\(", text), n
    assert _lib.ABI_VERSION == 2
    assert "embed_entry_autograd" in decode_ops.__doc__ and "positional_add_dropout_autograd" in decode_ops.__doc__


def test_workspace_questions_are_host_arithmetic():
    lib = _lib.load()
    ws = lib.dsp_embed_entry_bwd_workspace_bytes
    assert ws(0, 512, 70, 64, 0) == 0
    a, b, c = ws(100, 512, 70, 64, 0), ws(100, 512, 70, 64, 1), ws(200, 512, 70, 64, 0)
    assert 0 < a < b and a < c and a % 16 == 0 and b % 16 == 0
    assert b - a == 100 * 64 * 4                                            # g, written once as fp32, only with a mask
    assert lib.dsp_pos_add_bwd_workspace_bytes(0) == 0 and lib.dsp_pos_add_bwd_workspace_bytes(33) == 16


def _emb(V=16, NP=12, C=8, dtype=torch.float16):
    a = torch.nn.Embedding(V, C, padding_idx=1).to(dtype)
    b = torch.nn.Embedding(NP, C, padding_idx=1).to(dtype)
    return a, b


def test_served_declines_what_the_kernels_do_not_take():
    tok = torch.full((2, 5), 3, dtype=torch.int64)
    for dtype in (torch.float16, torch.bfloat16, torch.float32, torch.float64):
        assert not decode_ops.embed_entry_served(tok, *_emb(dtype=dtype))                                  # CPU tensors
        x = torch.zeros(2, 5, 8, dtype=dtype)
        assert not decode_ops.positional_add_dropout_served(x, torch.zeros(2, 5, dtype=torch.bool), torch.zeros(9, 8, dtype=dtype),
                                                            torch.ones(1, dtype=dtype))
    why = decode_ops._embed_entry_problem
    e, p = _emb(dtype=torch.float64)
    assert "float64" in why(tok, e.weight, p.weight, 1)                     # by its own reason, before the question about the device
    e, p = _emb()
    assert "GPU" in why(tok, e.weight, p.weight, 1)
    assert "int64" in why(tok.int(), e.weight, p.weight, 1)
    assert "not served" in why(torch.full((2, 11), 3), e.weight, p.weight, 1)                   # L + pad + 1 > NP
    assert "not served" in why(tok, *(m.weight for m in _emb(C=12)), 1)                         # a width off the 16-byte grid
    pw = decode_ops._posadd_problem
    x, m = torch.zeros(2, 5, 8, dtype=torch.float16), torch.zeros(2, 5, dtype=torch.bool)
    assert "float64" in pw(x.double(), torch.zeros(9, 8, dtype=torch.float64), m, torch.ones(1, dtype=torch.float64))
    assert "GPU" in pw(x, torch.zeros(9, 8), m, torch.ones(1))                                  # an fp32 table and alpha are taken
    assert "table" in pw(x, torch.zeros(9, 8, dtype=torch.bfloat16), m, torch.ones(1))
    assert "table" in pw(x, torch.zeros(9, 8, requires_grad=True), m, torch.ones(1))
    assert "alpha" in pw(x, torch.zeros(9, 8), m, torch.ones(2))
    assert "padding_mask" in pw(x, torch.zeros(9, 8), m[:, :4], torch.ones(1))
    with torch.autocast("cpu", dtype=torch.bfloat16):
        assert not decode_ops.embed_entry_served(tok, e, p)
        assert not decode_ops.positional_add_dropout_served(x, m, torch.zeros(9, 8), torch.ones(1))
    old = decode_ops.set_embed_entry_hip(False)
    try:
        assert old is True and decode_ops.EMBED_ENTRY_HIP is False
        assert not decode_ops.embed_entry_served(tok, e, p)
        assert not decode_ops.positional_add_dropout_served(x, m, torch.zeros(9, 8), torch.ones(1))
    finally:
        assert decode_ops.set_embed_entry_hip(old) is False
    assert decode_ops.EMBED_ENTRY_HIP is True


def test_public_functions_raise_on_cpu_tensors():
    tok = torch.full((2, 5), 3, dtype=torch.int64)
    e, p = _emb()
    with pytest.raises(RuntimeError, match="GPU"):
        decode_ops.embed_entry_autograd(tok, e.weight, p.weight, 1, 2.0)
    with pytest.raises(RuntimeError, match="float64"):
        decode_ops.embed_entry_autograd(tok, *(m.weight for m in _emb(dtype=torch.float64)), 1, 2.0)
    x, m = torch.zeros(2, 5, 8, dtype=torch.float16), torch.zeros(2, 5, dtype=torch.bool)
    with pytest.raises(RuntimeError, match="GPU"):
        decode_ops.positional_add_dropout_autograd(x, m, torch.zeros(9, 8), torch.ones(1))
    with pytest.raises(RuntimeError, match="float64"):
        decode_ops.positional_add_dropout_autograd(x.double(), m, torch.zeros(9, 8, dtype=torch.float64), torch.ones(1, dtype=torch.float64))


# ---------------------------------------------------------------- the models on CPU keep the bits of the parent's lines
def _drop(x, p, training):
    return F.dropout(x, p, training) if training and p > 0 else x


def _decoder_args(dropout):
    return SimpleNamespace(decoder_embed_dim=16, vocab_size=20, max_target_positions=40, decoder_ffn_embed_dim=32, decoder_attention_heads=2,
                           encoder_embed_dim=16, dropout=dropout, attention_dropout=0.0, activation_dropout=0.0, decoder_layers=0,
                           max_transition_length=8)


@pytest.mark.parametrize("training,dropout", [(False, 0.0), (True, 0.0), (True, 0.3)])
def test_decoder_entry_on_cpu_has_the_bits_of_the_torch_lines(training, dropout):
    torch.manual_seed(0)
    dec = M.DAGDecoder(_decoder_args(dropout)).train(training)               # no layers: extract_features is its entry lines
    tok = torch.tensor(R.token_case("interior", 20)[:, :30])
    enc = {"encoder_out": torch.zeros(4, 3, 16), "encoder_padding_mask": torch.zeros(3, 4, dtype=torch.bool)}
    torch.manual_seed(5)
    got = dec.extract_features(tok, enc)
    torch.manual_seed(5)
    want = dec.embed_scale * dec.embed_tokens(tok) + dec.embed_positions(dec.positions(tok))
    want = _drop(want, dropout, training)
    assert torch.equal(got, want)


@pytest.mark.parametrize("training,dropout", [(False, 0.0), (True, 0.0), (True, 0.2)])
def test_tts_positional_sites_and_predictor_on_cpu_have_the_bits_of_the_torch_lines(training, dropout):
    torch.manual_seed(0)
    tts = FS.FastSpeech2NoEmb(embed_dim=16, heads=2, fft_hidden_dim=32, fft_kernel_size=3, enc_layers=0, dec_layers=0, var_pred_hidden_dim=16,
                              var_pred_kernel_size=3, var_pred_n_bins=8, dropout=dropout, var_pred_dropout=dropout, out_dim=4,
                              max_positions=50).train(training)
    with torch.no_grad():
        tts.pos_emb_alpha.fill_(0.7); tts.dec_pos_emb_alpha.fill_(1.3)
    B, N = 2, 9
    x = torch.randn(B, N, 16)
    mask = torch.zeros(B, N, dtype=torch.bool); mask[1, 6:] = True
    dur = torch.randint(1, 4, (B, N)).masked_fill(mask, 0)
    pit, ene = torch.randn(B, N), torch.randn(B, N)
    torch.manual_seed(7)
    mel = tts(x, mask, dur, pit, ene)[0]
    torch.manual_seed(7)
    h = _drop(x + tts.pos_emb_alpha * tts._pos(mask), dropout, training)
    h, out_lens, _, _, _ = tts.var_adaptor(h, mask, dur, pit, ene)
    dec_mask = torch.arange(h.shape[1]).unsqueeze(0) >= out_lens.unsqueeze(1)
    h = h + tts.dec_pos_emb_alpha * tts._pos(dec_mask)
    assert torch.equal(mel, tts.out_proj(h))
    vp = tts.var_adaptor.duration_predictor
    torch.manual_seed(9)
    got = vp(x)
    torch.manual_seed(9)
    w = _drop(vp.ln1(vp.conv1(x.transpose(1, 2)).transpose(1, 2)), vp.p, training)
    w = _drop(vp.ln2(vp.conv2(w.transpose(1, 2)).transpose(1, 2)), vp.p, training)
    assert torch.equal(got, vp.proj(w).squeeze(2))
