"""CPU: the surface of the TTS-loss operator — names and constants, the header's declarations and #defines against decode_ops and
_lib.SIGNATURES, the workspace question (host arithmetic), what tts_losses_served declines and tts_losses_autograd raises, and the criterion on
CPU tensors, which keeps the bits of its torch lines."""
import os
import re

import pytest
import torch

from tests import util_tts_loss_ref as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("dsp_tts_loss_workspace_bytes", "dsp_tts_loss_fwd", "dsp_tts_loss_bwd")


def test_names_and_constants():
    from daspeech_amd import decode_ops
    assert decode_ops.TTS_LOSS_HIP is True
    for name in ("set_tts_loss_hip", "_tts_loss_problem", "tts_losses_served", "tts_losses_checked", "tts_losses_autograd"):
        assert callable(getattr(decode_ops, name)), name
    assert "tts_losses_autograd" in decode_ops.__doc__ and "tts_loss_train.hip" in decode_ops.__doc__
    assert decode_ops.set_tts_loss_hip(False) is True and decode_ops.TTS_LOSS_HIP is False
    assert decode_ops.set_tts_loss_hip(True) is False and decode_ops.TTS_LOSS_HIP is True
    d = U.header_defines()
    assert d["DSP_TTSLOSS_CHUNK_ROWS"] == decode_ops.TTSLOSS_CHUNK_ROWS and d["DSP_TTSLOSS_CHUNK_ELEMS"] == decode_ops.TTSLOSS_CHUNK_ELEMS


def test_header_and_binding():
    from daspeech_amd import _lib
    text = open(os.path.join(ROOT, "include", "daspeech_decode.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES, name
    assert re.search(r"#define\s+DSP_TTSLOSS_CHUNK_ROWS\s+\d+", code) and re.search(r"#define\s+DSP_TTSLOSS_CHUNK_ELEMS\s+\d+", code)
    assert _lib.ABI_VERSION == 2
    assert os.path.exists(os.path.join(ROOT, "daspeech_amd", "csrc", "tts_loss_train.hip"))


def test_workspace_question_is_host_arithmetic():
    from daspeech_amd import _lib
    lib = _lib.load()
    ws = lib.dsp_tts_loss_workspace_bytes
    assert ws(0, 528, 62) == 0 and ws(-1, 528, 62) == 0 and ws(4, 0, 0) == 0 and ws(0, 0, 0) == 0
    d = U.header_defines()
    R, E = d["DSP_TTSLOSS_CHUNK_ROWS"], d["DSP_TTSLOSS_CHUNK_ELEMS"]
    assert ws(1, 1, 1) == 32                                   # 2 mel partials + 3 variance partials, fp32, rounded up to 16 bytes
    for B, F_, N in ((1, 1, 1), (3, 7, 5), (32, 528, 62), (2, R + 1, 65), (2, 3 * R - 1, E + 1), (64, 1200, 200)):
        a = ws(B, F_, N)
        assert a > 0 and a % 16 == 0
        need = 4 * (2 * -(-B * F_ // R) + 3 * -(-B * N // E))
        assert need <= a < need + 16
        assert ws(B + 1, F_, N) >= a and ws(B, F_ + 1, N) >= a and ws(B, F_, N + 1) >= a
        assert ws(B, F_ + 2 * R, N) > a and ws(B, F_, N + 2 * E) > a              # two more chunks are at least 16 more bytes


def _cpu_case(**kw):
    return U.make_case(2, 6, 6, 8, 5, **kw)


def _declined(case, why):
    """served says no, and the raising function raises under its own name with `why` in the message"""
    from daspeech_amd import decode_ops
    assert decode_ops.tts_losses_served(*U.args_of(case)) is False
    with pytest.raises(RuntimeError, match=r"^tts_losses_autograd: .*" + why):
        decode_ops.tts_losses_autograd(*U.args_of(case))


def test_served_declines_and_autograd_raises():
    from daspeech_amd import decode_ops
    _declined(_cpu_case(), "GPU tensors")
    case = _cpu_case()
    case["pitches"] = case["pitches"].to(torch.float16)
    _declined(case, "one floating dtype")
    _declined(_cpu_case(dtype=torch.float64), "never narrowed")
    for key, shape in (("target_audio", (3, 6, 8)), ("target_audio", (2, 6, 4)), ("feat_post", (2, 5, 8)), ("energies", (2, 4)),
                       ("durations", (2, 6)), ("audio_lens", (3,)), ("src_lens", (2, 1))):
        case = _cpu_case()
        case[key] = torch.zeros(shape, dtype=case[key].dtype)
        _declined(case, "")
    case = _cpu_case()
    case["durations"] = case["durations"].to(torch.float32)
    _declined(case, "int64 or int32")
    for key in ("target_audio", "pitches", "energies"):
        case = _cpu_case()
        case[key].requires_grad_(True)
        _declined(case, "must not require grad")
    # the two gates in front of the rule: the switch and autocast (asked on tensors that fail the rule anyway: the answer is False either way,
    # and the raising function still names the rule's reason)
    old = decode_ops.set_tts_loss_hip(False)
    try:
        _declined(_cpu_case(), "GPU tensors")
    finally:
        decode_ops.set_tts_loss_hip(old)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        assert decode_ops.tts_losses_served(*U.args_of(_cpu_case())) is False


def test_problem_function_orders_its_reasons():
    """the layout reasons come last and begin with _LAYOUT, so that a dense copy is tried only on tensors that are otherwise served"""
    from daspeech_amd import decode_ops
    case = _cpu_case()
    case["pitch_out"] = case["pitch_out"].t().contiguous().t()
    why = decode_ops._tts_loss_problem(*U.args_of(case))
    assert why == decode_ops._NOT_GPU                           # not the layout: a CPU tensor is refused before its strides are looked at
    assert decode_ops._tts_loss_problem(*U.args_of(_cpu_case(dtype=torch.float64))).startswith("the data has to be fp32, fp16 or bf16")


class _CpuCriterion:
    """S2SDAGFastSpeech2Loss with the alpha / beta of the HIP DAG loss taken out (they feed the `expect` strategy only): the torch DAG loss,
    the torch gather and the torch alignment serve CPU tensors, so `argmax` runs the whole forward there"""

    @staticmethod
    def make():
        from daspeech_amd.criterions import S2SDAGFastSpeech2Loss

        class Crit(S2SDAGFastSpeech2Loss):
            def _compute_dag_loss_with_alpha_beta(self, *a, **k):
                self.dag = self._dag_loss_core(*a[:5], k["name"], k["factor"], k["matchmask"], k["keep_word_mask"], k["model"], False,
                                               path=k["path"])[0]
                return self.dag, None, None
        return Crit(glat_p="0", tts_loss_weight=5.0, training_strategy="argmax", torch_dag_loss=True, torch_dag_logsoftmax_gather=True,
                    torch_dag_best_alignment=True)


@pytest.mark.parametrize("postnet", [False, True])
def test_criterion_on_cpu_keeps_the_bits_of_its_torch_lines(postnet):
    from daspeech_amd.models.daspeech import S2SConformerDAGFastSpeech2Model
    from daspeech_amd.synthetic import make_s2st_batch
    torch.manual_seed(0)
    tts = dict(enc_layers=1, dec_layers=1, add_postnet=True) if postnet else dict(enc_layers=1, dec_layers=1)
    m = S2SConformerDAGFastSpeech2Model(encoder_layers=1, decoder_layers=1, tts=tts).eval()
    s = make_s2st_batch(2, "cpu", seed=3, min_frames=60, max_frames=90)
    s["update_num"] = 10
    crit = _CpuCriterion.make()
    crit.train()
    seen = {}
    tts_fwd = m.tts.forward

    def spy(*a, **k):
        seen["out"] = tts_fwd(*a, **k)
        return seen["out"]
    m.tts.forward = spy
    loss, _, log = crit(m, s)
    fo, fp, _, ld, po, eo = seen["out"]
    assert (fp is not None) == postnet
    l1, dur, pitch, energy = U.torch_lines(fo, fp, s["target_audio"], s["target_audio_lengths"], ld, po, eo, s["durations"], s["pitches"],
                                           s["energies"], s["target_text_lengths"] - 1)
    tts_loss = l1 + dur + pitch + energy
    want = crit.dag["loss"] + tts_loss * 5.0
    assert torch.isfinite(loss) and loss.dtype == torch.float32
    assert torch.equal(loss.detach(), want.detach())
    for key, val in (("tts-loss", tts_loss), ("l1-loss", l1), ("dur-loss", dur), ("pitch-loss", pitch), ("energy-loss", energy), ("loss", want)):
        assert torch.equal(log[key], val.detach()), key
    params = [p for p in m.parameters() if p.requires_grad]
    got = torch.autograd.grad(loss, params, retain_graph=True, allow_unused=True)
    ref = torch.autograd.grad(want, params, allow_unused=True)
    assert sum(g is not None for g in got) > 20
    for p, a, b in zip(params, got, ref):
        assert (a is None) == (b is None) and (a is None or torch.equal(a, b))
