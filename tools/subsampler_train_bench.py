#!/usr/bin/env python3
"""Forward, and forward + backward, of the encoder's Conv1dSubsampler alone (80 -> 1024 -> GLU -> 512 -> 512 -> GLU -> 256, K 5, stride 2) at the
frame counts daspeech_amd/synthetic.py gives the C5 step (the two batches bench.py's train workload alternates): the torch lines (transpose ->
nn.Conv1d stride 2 through MIOpen -> F.glu -> transpose; autograd backward) against the training branch on the HIP stride-2 operator
(decode_ops.set_conv1d_stride2_train_hip) — same process, same module and tensors, the two legs INTERLEAVED round by round.  The input does not
require a gradient (the filterbank features of the step), so the backward is the two weight / bias gradients and the input gradient of the
second layer.  Per leg: GPU time by HIP events and host time (perf_counter around the calls, no sync inside), warm-up then median and the
10 % .. 90 % spread.  `--only hip|torch --rounds N` runs one leg N times and nothing else: the run a kernel trace is taken of.  GPU box only; a
plain tool, not a test.  The table is printed and written.

usage: subsampler_train_bench.py [--batch B] [--iters N] [--warmup N] [--out FILE] [--only hip|torch --rounds N]
default: B 32, fp16; default file: profiles/subsampler_train.txt"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                                                   # noqa: E402
from daspeech_amd import decode_ops                            # noqa: E402
from daspeech_amd.models.daspeech import DEFAULT_ARGS, Conv1dSubsampler   # noqa: E402
from daspeech_amd.synthetic import make_s2st_batch             # noqa: E402


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


def frame_counts(B):
    """the padded frame counts of the two batches the C5 step alternates (bench.py: make_s2st_batch(B, dev, seed=i), i = 0, 1)"""
    return [int(make_s2st_batch(B, "cpu", seed=i)["net_input"]["src_tokens"].shape[1]) for i in range(2)]


def legs(module, B, T, dev, dtype):
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((B, T, DEFAULT_ARGS["input_feat"]), device=dev, generator=gen).to(dtype)
    lens = torch.full((B,), T, device=dev)
    T4 = int(module.out_lengths(torch.tensor([T]))[0])
    cot = torch.randn((B, T4, DEFAULT_ARGS["encoder_embed_dim"]), device=dev, generator=gen).to(dtype)
    params = list(module.parameters())
    assert decode_ops.conv1d_stride2_channels_last_sites_served(x, module.conv_layers)

    def leg(on):
        def forward():
            old = decode_ops.set_conv1d_stride2_train_hip(on)
            try:
                return module(x, lens)[0]
            finally:
                decode_ops.set_conv1d_stride2_train_hip(old)
        return forward, lambda: torch.autograd.grad(forward(), params, cot)
    return leg(False), leg(True)


def flops(B, T):
    """(forward, forward + backward) GFLOP: one product per layer forward, dW for both, dx for the second only"""
    a = DEFAULT_ARGS
    K1, K2 = a["conv_kernels"]
    T2 = (T - 1) // 2 + 1
    T4 = (T2 - 1) // 2 + 1
    p1 = 2.0 * B * T2 * a["input_feat"] * a["conv_channels"] * K1 / 1e9
    p2 = 2.0 * B * T4 * (a["conv_channels"] // 2) * (2 * a["encoder_embed_dim"]) * K2 / 1e9
    return p1 + p2, 2 * p1 + 3 * p2


def main():
    B = _opt("--batch", 32)
    iters, warmup = _opt("--iters", 200), _opt("--warmup", 20)
    out_path = _opt("--out", os.path.join(ROOT, "profiles", "subsampler_train.txt"), str)
    only, rounds = _opt("--only", None, str), _opt("--rounds", 20)
    dev, dtype = torch.device("cuda:0"), torch.float16
    a = DEFAULT_ARGS
    torch.manual_seed(0)
    module = Conv1dSubsampler(a["input_feat"], a["conv_channels"], a["encoder_embed_dim"], a["conv_kernels"]).to(dev, dtype).train()
    Ts = frame_counts(B)
    if only:                                                               # one leg alone, for a kernel trace
        for T in Ts:
            (tf, tb), (hf, hb) = legs(module, B, T, dev, dtype)
            for _ in range(rounds):
                (hb if only == "hip" else tb)()
            torch.cuda.synchronize()
        return
    lines = []

    def say(t):
        print(t, flush=True)
        lines.append(t)

    say(f"Conv1dSubsampler alone in train(), B {B} fp16, input without a gradient; device {torch.cuda.get_device_name(0)}; median (10 % .. 90 %) of "
        f"{iters} rounds after {warmup} warm-up, legs interleaved; forward, and forward + backward (gradients of the four parameters)")
    fmt = lambda m: f"{m[0]:7.3f} ({m[1]:.3f} .. {m[2]:.3f})"
    for T in Ts:
        (tf, tb), (hf, hb) = legs(module, B, T, dev, dtype)
        (rtf, rhf) = interleaved([tf, hf], iters, warmup)
        (rtb, rhb) = interleaved([tb, hb], iters, warmup)
        gf, gb = flops(B, T)
        say(f"T {T} frames -> {int(module.out_lengths(torch.tensor([T]))[0])}: {gf:.2f} GFLOP forward, {gb:.2f} forward + backward")
        say(f"    torch lines   forward GPU {fmt(rtf[0])} ms host {fmt(rtf[1])} ms   forward + backward GPU {fmt(rtb[0])} ms host {fmt(rtb[1])} ms")
        say(f"    HIP operator  forward GPU {fmt(rhf[0])} ms host {fmt(rhf[1])} ms   forward + backward GPU {fmt(rhb[0])} ms host {fmt(rhb[1])} ms"
            f"   ratio torch / HIP: GPU {rtb[0][0] / rhb[0][0]:.2f} host {rtb[1][0] / rhb[1][0]:.2f}")
        say(f"    by the events: torch {gb / rtb[0][0]:.0f} TFLOP/s, HIP {gb / rhb[0][0]:.0f} TFLOP/s forward + backward "
            f"({100 * gb / rhb[0][0] / 2500:.1f} % of the 2.5 PF fp16 peak)")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(f"written: {out_path}")


if __name__ == "__main__":
    main()
