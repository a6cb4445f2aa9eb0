#!/usr/bin/env python3
"""Forward + backward of one channels-last convolution site of the FastSpeech2 half alone, at the three site shapes of a C5 step: the torch
lines the operator replaces (transpose -> nn.Conv1d with its bias -> transpose -> .contiguous(); autograd backward) against
decode_ops.conv1d_channels_last_autograd with the bias — same process, same tensors, the two legs INTERLEAVED round by round.  Per leg: GPU
time by HIP events and host time (perf_counter around the calls, no sync inside) of forward and of forward + backward with all three
gradients, warm-up then median and the 10 % .. 90 % spread; the FLOPs of the three products (2 B T Cin Cout K each).  Then
torch.cuda.max_memory_allocated over one forward + backward of the TTS half (FastSpeech2NoEmb, B 32, 62 tokens -> 530 frames) with the switch
on and off.  `--only hip|torch --rounds N` runs one leg N times and nothing else: the run a kernel trace is taken of.  GPU box only; a plain
tool, not a test.  The table is printed and written.

usage: conv1d_train_bench.py [--batch B] [--iters N] [--warmup N] [--out FILE] [--only hip|torch --rounds N]
default: B 32, fp16; default file: profiles/conv1d_train_bench.txt"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                                                   # noqa: E402
from torch import nn                                           # noqa: E402
from daspeech_amd import decode_ops                            # noqa: E402
from daspeech_amd.models.fastspeech2 import FastSpeech2NoEmb   # noqa: E402

SITES = [("FFT conv 1", 530, 256, 1024, 9), ("FFT conv 2", 530, 1024, 256, 9), ("predictor conv", 62, 256, 256, 3)]      # name, T, Cin, Cout, K


def _opt(name, default, conv=int):
    return conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def one(fn):
    """(GPU ms by events, host ms until the last call returned)"""
    a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record(); fn(); b.record()
    host = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    return a.elapsed_time(b), host


def interleaved(fns, iters, warmup):
    """every leg once per round, in turn -> per leg ((median, 10 %, 90 %) GPU ms, the same for host ms)"""
    ts = [([], []) for _ in fns]
    for i in range(warmup + iters):
        for k, fn in enumerate(fns):
            g, h = one(fn)
            if i >= warmup:
                ts[k][0].append(g); ts[k][1].append(h)
    stat = lambda t: (sorted(t)[len(t) // 2], sorted(t)[len(t) // 10], sorted(t)[(9 * len(t)) // 10])
    return [(stat(g), stat(h)) for g, h in ts]


def site(B, T, Cin, Cout, K, dev, dtype):
    gen = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(s, device=dev, generator=gen).to(dtype)
    conv = nn.Conv1d(Cin, Cout, K, padding=(K - 1) // 2).to(dev, dtype)
    x = rnd(B, T, Cin).requires_grad_()
    cot = rnd(B, T, Cout)
    wrt = [x, conv.weight, conv.bias]
    assert decode_ops.conv1d_channels_last_served(x, conv)
    torch_lines = lambda: conv(x.transpose(1, 2)).transpose(1, 2).contiguous()
    hip_op = lambda: decode_ops.conv1d_channels_last_autograd(x, conv.weight, conv.bias)
    both = lambda fwd: torch.autograd.grad(fwd(), wrt, cot)
    return torch_lines, hip_op, both


def tts_peak(B, dev, dtype):
    """peak memory (MiB above the resident tensors) of one forward + backward of the TTS half, switch off / on"""
    torch.manual_seed(0)
    model = FastSpeech2NoEmb().to(dev, dtype).train()
    N, per = 62, 9
    x = torch.randn(B, N, 256, device=dev).to(dtype)
    pad = torch.zeros(B, N, dtype=torch.bool, device=dev)
    dur = torch.full((B, N), per, device=dev)
    dur[:, -1] = 530 - per * (N - 1)                                       # 530 frames a sample
    pitch, energy = torch.randn(B, N, device=dev).to(dtype), torch.randn(B, N, device=dev).to(dtype)
    peaks = {}
    for on in (False, True):
        old = decode_ops.set_conv1d_train_hip(on)
        try:
            for rep in range(2):                                            # the second run: allocator and libraries warm
                torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                mel, _, _, log_dur, p_out, e_out = model(x, pad, durations=dur, pitches=pitch, energies=energy)
                (mel.float().pow(2).mean() + log_dur.float().pow(2).mean() + p_out.float().pow(2).mean() + e_out.float().pow(2).mean()).backward()
                torch.cuda.synchronize()
                peaks[on] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
                model.zero_grad(set_to_none=True)
                del mel, log_dur, p_out, e_out
        finally:
            decode_ops.set_conv1d_train_hip(old)
    return peaks


def main():
    B = _opt("--batch", 32)
    iters, warmup = _opt("--iters", 200), _opt("--warmup", 20)
    out_path = _opt("--out", os.path.join(ROOT, "profiles", "conv1d_train_bench.txt"), str)
    only, rounds = _opt("--only", None, str), _opt("--rounds", 20)
    dev, dtype = torch.device("cuda:0"), torch.float16
    if only:                                                               # one leg alone, for a kernel trace
        for name, T, Cin, Cout, K in SITES:
            torch_lines, hip_op, both = site(B, T, Cin, Cout, K, dev, dtype)
            for _ in range(rounds):
                both(hip_op if only == "hip" else torch_lines)
            torch.cuda.synchronize()
        return
    lines = []

    def say(t):
        print(t, flush=True)
        lines.append(t)

    say(f"one channels-last convolution site alone, B {B} fp16; device {torch.cuda.get_device_name(0)}; median (10 % .. 90 %) of {iters} rounds after "
        f"{warmup} warm-up, legs interleaved; forward, and forward + backward (gradients of x, weight, bias)")
    fmt = lambda m: f"{m[0]:7.3f} ({m[1]:.3f} .. {m[2]:.3f})"
    for name, T, Cin, Cout, K in SITES:
        torch_lines, hip_op, both = site(B, T, Cin, Cout, K, dev, dtype)
        (tf, hf) = interleaved([torch_lines, hip_op], iters, warmup)
        (tb, hb) = interleaved([lambda: both(torch_lines), lambda: both(hip_op)], iters, warmup)
        gf = 2.0 * B * T * Cin * Cout * K / 1e9
        say(f"{name}: B {B} x T {T}, {Cin} -> {Cout}, K {K}; {gf:.2f} GFLOP per product, {3 * gf:.2f} forward + backward")
        say(f"    torch lines   forward GPU {fmt(tf[0])} ms host {fmt(tf[1])} ms   forward + backward GPU {fmt(tb[0])} ms host {fmt(tb[1])} ms")
        say(f"    HIP operator  forward GPU {fmt(hf[0])} ms host {fmt(hf[1])} ms   forward + backward GPU {fmt(hb[0])} ms host {fmt(hb[1])} ms"
            f"   ratio torch / HIP: GPU {tb[0][0] / hb[0][0]:.2f} host {tb[1][0] / hb[1][0]:.2f}")
        say(f"    by the events: torch {3 * gf / tb[0][0]:.0f} TFLOP/s, HIP {3 * gf / hb[0][0]:.0f} TFLOP/s forward + backward "
            f"({100 * 3 * gf / hb[0][0] / 2500:.1f} % of the 2.5 PF fp16 peak)")
    peaks = tts_peak(B, dev, dtype)
    say(f"TTS half (FastSpeech2NoEmb, B {B}, 62 tokens -> 530 frames) forward + backward, peak memory above the resident tensors: torch lines "
        f"{peaks[False]:.1f} MiB, HIP operator {peaks[True]:.1f} MiB  (difference {peaks[False] - peaks[True]:.1f} MiB)")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(f"written: {out_path}")


if __name__ == "__main__":
    main()
