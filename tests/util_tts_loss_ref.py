"""What the tests of the TTS-loss operator (decode_ops.tts_losses_autograd, csrc/tts_loss_train.hip) share: the float64 reference written from
the lengths, the criterion's torch lines as they stand in S2SDAGFastSpeech2Loss.forward, the case builder, and the kernel's chunking restated
from the header's #defines (the number of fp32 additions between a term and a result, which bounds the forward's error)."""
import math
import os
import re

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("feat_out", "feat_post", "target_audio", "audio_lens", "log_dur_out", "pitch_out", "energy_out", "durations", "pitches", "energies",
         "src_lens")
GRAD_NAMES = ("feat_out", "feat_post", "log_dur_out", "pitch_out", "energy_out")
LOSSES = ("l1", "dur", "pitch", "energy")


def header_defines():
    text = open(os.path.join(ROOT, "include", "daspeech_decode.h")).read()
    return {k: int(v) for k, v in re.findall(r"#define\s+(DSP_TTSLOSS_CHUNK_[A-Z]+)\s+(\d+)", text)}


def additions_on_longest_path(B, F_, C, N):
    """fp32 additions between a term and a result of dsp_tts_loss_fwd, the longest chain over the data dtypes and both access forms: a lane
    adds its elements of the chunk one by one (16-byte form: V = 4 or 8 elements per group, the groups l, l + 64, ... of the chunk's
    rows * C / V; scalar form: the elements l, l + 64, ...), 6 butterfly steps fold the wave; in the tail thread t adds the partials t, t + 256,
    ..., 6 steps fold the wave and 3 additions the four waves; the postnet term is one more addition."""
    d = header_defines()
    rows, elems = d["DSP_TTSLOSS_CHUNK_ROWS"], d["DSP_TTSLOSS_CHUNK_ELEMS"]

    def tail(n_items, per):
        return math.ceil(math.ceil(n_items / per) / 256) + 6 + 3

    r = min(rows, B * F_)
    lane = max(V * math.ceil(r * C / V / 64) for V in (1, 4, 8) if C % V == 0)
    mel = lane + 6 + tail(B * F_, rows) + 1
    src = math.ceil(min(elems, B * N) / 64) + 6 + tail(B * N, elems)
    return max(mel, src)


def forward_bound(B, F_, C, N):
    """relative error of a loss against float64 on the same inputs: every partial is a sum of non-negative terms, so each of the `path`
    additions and the 4 roundings of a term (subtraction, log, square or abs, division) costs at most 2^-24"""
    return (additions_on_longest_path(B, F_, C, N) + 4) * 2.0 ** -24


def make_case(B, F, Fa, C, N, audio_lens=None, src_lens=None, dtype=torch.float32, device="cpu", seed=0, post=True):
    """random inputs of one problem as a dict keyed by NAMES; lengths None: full"""
    g = torch.Generator().manual_seed(seed)
    F_ = min(F, Fa)

    def rnd(*shape):
        return torch.randn(*shape, generator=g).to(dtype).to(device)
    case = {
        "feat_out": rnd(B, F, C), "feat_post": rnd(B, F, C) if post else None, "target_audio": rnd(B, Fa, C),
        "audio_lens": torch.tensor([F_] * B if audio_lens is None else audio_lens, dtype=torch.int64, device=device),
        "log_dur_out": rnd(B, N), "pitch_out": rnd(B, N), "energy_out": rnd(B, N),
        "durations": torch.randint(0, 20, (B, N), generator=g).to(device), "pitches": rnd(B, N), "energies": rnd(B, N),
        "src_lens": torch.tensor([N] * B if src_lens is None else src_lens, dtype=torch.int64, device=device),
    }
    return case


def args_of(case):
    return tuple(case[k] for k in NAMES)


def torch_lines(feat_out, feat_post, target_audio, audio_lens, log_dur_out, pitch_out, energy_out, durations, pitches, energies, src_lens):
    """(l1, dur, pitch, energy) by the torch lines of S2SDAGFastSpeech2Loss.forward, copied (src_lens is target_text_lengths - 1 there)"""
    from daspeech_amd.criterions import _lengths_to_mask
    _feat_out, _feat_out_post = feat_out, feat_post
    sample = {"target_audio": target_audio, "target_audio_lengths": audio_lens, "durations": durations, "pitches": pitches, "energies": energies}
    src_mask = _lengths_to_mask(src_lens, log_dur_out.shape[1])
    F_ = min(_feat_out.shape[1], sample["target_audio"].shape[1])
    tgt_mask = _lengths_to_mask(sample["target_audio_lengths"].clamp(max=F_), F_)
    feat_out, feat = _feat_out[:, :F_][tgt_mask], sample["target_audio"][:, :F_][tgt_mask]
    l1_loss = F.l1_loss(feat_out, feat, reduction="mean")
    if _feat_out_post is not None:
        l1_loss = l1_loss + F.l1_loss(_feat_out_post[:, :F_][tgt_mask], feat, reduction="mean")
    pitch_loss = F.mse_loss(pitch_out[src_mask], sample["pitches"][src_mask], reduction="mean")
    energy_loss = F.mse_loss(energy_out[src_mask], sample["energies"][src_mask], reduction="mean")
    log_dur = torch.log(sample["durations"].to(log_dur_out.dtype) + 1)[src_mask]
    dur_loss = F.mse_loss(log_dur_out[src_mask], log_dur, reduction="mean")
    return l1_loss, dur_loss, pitch_loss, energy_loss


def reference_f64(case):
    """the four losses in float64 from the formulas of include/daspeech_decode.h, utterance by utterance from the lengths (no mask); NaN for
    an empty selection"""
    c = {k: (v.detach().cpu() if v is not None else None) for k, v in case.items()}
    fo, fp, tg = c["feat_out"].double(), None if c["feat_post"] is None else c["feat_post"].double(), c["target_audio"].double()
    B, F_, C, N = fo.shape[0], min(fo.shape[1], tg.shape[1]), fo.shape[2], c["log_dur_out"].shape[1]
    s = [0.0] * 5
    n_mel = n_src = 0
    for b in range(B):
        m = min(max(int(c["audio_lens"][b]), 0), F_)
        k = min(max(int(c["src_lens"][b]), 0), N)
        n_mel += C * m
        n_src += k
        s[0] += float((fo[b, :m] - tg[b, :m]).abs().sum())
        if fp is not None:
            s[4] += float((fp[b, :m] - tg[b, :m]).abs().sum())
        s[1] += float((c["log_dur_out"][b, :k].double() - torch.log(c["durations"][b, :k].double() + 1)).pow(2).sum())
        s[2] += float((c["pitch_out"][b, :k].double() - c["pitches"][b, :k].double()).pow(2).sum())
        s[3] += float((c["energy_out"][b, :k].double() - c["energies"][b, :k].double()).pow(2).sum())

    def div(a, n):
        return a / n if n else float("nan")
    return [div(s[0], n_mel) + (div(s[4], n_mel) if fp is not None else 0.0), div(s[1], n_src), div(s[2], n_src), div(s[3], n_src)]


def with_grad(case, names=GRAD_NAMES, dtype=None):
    """a copy of the case whose tensors of `names` are fresh leaves that require grad (dtype: the floating tensors converted first)"""
    out = {}
    for k, v in case.items():
        if v is not None and v.is_floating_point():
            v = v.detach().clone() if dtype is None else v.detach().to(dtype)
            v.requires_grad_(k in names)
        out[k] = v
    return out


def backward_of(fn, case, g):
    """(losses, {name: grad}) of sum_i g[i] * fn(case)[i]"""
    losses = fn(*args_of(case))
    if not isinstance(losses, torch.Tensor):
        losses = torch.stack([x.to(torch.float32) if x.dtype != torch.float64 else x for x in losses])
    (losses * g.to(losses.dtype)).sum().backward()
    return losses.detach(), {k: case[k].grad for k in GRAD_NAMES if case[k] is not None and case[k].requires_grad}
