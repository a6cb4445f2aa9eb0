#!/usr/bin/env python3
"""The tail of the released objective alone — the l1 (+ postnet), duration, pitch and energy losses from the TTS outputs — at the shapes of a
C5 batch: the criterion's torch lines (masks from the lengths, boolean selections, F.l1_loss / F.mse_loss) against
decode_ops.tts_losses_autograd, forward and forward + backward.  Per call: the time between two HIP events around it and the time the host
spends issuing it (the queue is empty when a call starts; the host clock stops when the call returns, before any synchronisation of the
tool's own) — warm-up, then the median.  Every leg is a process of its own under its own `timeout`, torch and HIP alternating; a leg that
fails ends the tool.  GPU box only; a plain tool, not a test.  The table is printed and written.

usage: tts_loss_bench.py [--batch B] [--src N] [--frames F] [--target-frames Fa] [--channels C] [--dtype fp16|fp32|bf16] [--postnet 0|1]
                         [--iters N] [--warmup N] [--timeout SECONDS] [--out FILE]
default: B 32, N 62, F 528, Fa 528, C 80, fp16, no postnet (the C5 shape), 200 iterations after 20; default file: profiles/tts_loss_bench.txt"""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _opt(name, default, conv=int):
    return conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def leg(which):
    import torch
    import torch.nn.functional as F
    from daspeech_amd import decode_ops
    B, N, Fo, Fa, C = _opt("--batch", 32), _opt("--src", 62), _opt("--frames", 528), _opt("--target-frames", 528), _opt("--channels", 80)
    iters, warmup, post = _opt("--iters", 200), _opt("--warmup", 20), bool(_opt("--postnet", 0))
    dtype = {"fp16": torch.float16, "fp32": torch.float32, "bf16": torch.bfloat16}[_opt("--dtype", "fp16", str)]
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)

    def rnd(*shape, grad=False):
        return torch.randn(shape, device=dev, generator=gen).to(dtype).requires_grad_(grad)
    feat_out, feat_post, target = rnd(B, Fo, C, grad=True), rnd(B, Fo, C, grad=True) if post else None, rnd(B, Fa, C)
    log_dur_out, pitch_out, energy_out = rnd(B, N, grad=True), rnd(B, N, grad=True), rnd(B, N, grad=True)
    pitches, energies = rnd(B, N), rnd(B, N)
    durations = torch.randint(0, 20, (B, N), device=dev, generator=gen)
    audio_lens = torch.randint(min(Fo, Fa) // 2, min(Fo, Fa) + 1, (B,), device=dev, generator=gen)
    src_lens = torch.randint(N // 2, N + 1, (B,), device=dev, generator=gen)
    leaves = [t for t in (feat_out, feat_post, log_dur_out, pitch_out, energy_out) if t is not None]
    weights = torch.tensor([1.0, 1.0, 1.0, 1.0], device=dev)

    def torch_lines():
        src_mask = torch.arange(N, device=dev).unsqueeze(0) < src_lens.unsqueeze(1)
        F_ = min(Fo, Fa)
        tgt_mask = torch.arange(F_, device=dev).unsqueeze(0) < audio_lens.clamp(max=F_).unsqueeze(1)
        fo, feat = feat_out[:, :F_][tgt_mask], target[:, :F_][tgt_mask]
        l1 = F.l1_loss(fo, feat, reduction="mean")
        if feat_post is not None:
            l1 = l1 + F.l1_loss(feat_post[:, :F_][tgt_mask], feat, reduction="mean")
        pitch = F.mse_loss(pitch_out[src_mask], pitches[src_mask], reduction="mean")
        energy = F.mse_loss(energy_out[src_mask], energies[src_mask], reduction="mean")
        log_dur = torch.log(durations.to(dtype) + 1)[src_mask]
        dur = F.mse_loss(log_dur_out[src_mask], log_dur, reduction="mean")
        return l1 + dur + pitch + energy

    def hip_op():
        return (decode_ops.tts_losses_autograd(feat_out, feat_post, target, audio_lens, log_dur_out, pitch_out, energy_out, durations, pitches,
                                               energies, src_lens) * weights).sum()
    fwd = torch_lines if which == "torch" else hip_op

    def both():
        return torch.autograd.grad(fwd(), leaves)

    def timed(fn):
        dev_ms, host_ms = [], []
        for i in range(warmup + iters):
            a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record(); fn(); b.record()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            if i >= warmup:
                dev_ms.append(a.elapsed_time(b)); host_ms.append((t1 - t0) * 1e3)
        return statistics.median(dev_ms), min(dev_ms), statistics.median(host_ms), min(host_ms)
    f, fb = timed(fwd), timed(both)
    name = "torch lines" if which == "torch" else "HIP operator"
    print(f"LEG {name:<13s} forward: events {f[0]:7.3f} ms (min {f[1]:7.3f}) host {f[2]:7.3f} ms (min {f[3]:7.3f})   "
          f"forward + backward: events {fb[0]:7.3f} ms (min {fb[1]:7.3f}) host {fb[2]:7.3f} ms (min {fb[3]:7.3f})   "
          f"loss {float(fwd()):.6f}", flush=True)
    if which == "torch":
        print(f"HEAD TTS losses alone, B {B} N {N} F {Fo} Fa {Fa} C {C} postnet {int(post)} ({int(audio_lens.clamp(max=min(Fo, Fa)).sum())} valid "
              f"frames, {int(src_lens.sum())} valid source positions), {dtype}; device {torch.cuda.get_device_name(0)}; median (min) of {iters} "
              f"after {warmup} warm-up", flush=True)


def main():
    if "--leg" in sys.argv:
        return leg(_opt("--leg", "torch", str))
    out_path = _opt("--out", os.path.join(ROOT, "profiles", "tts_loss_bench.txt"), str)
    limit = _opt("--timeout", 180)
    passed = [a for a in sys.argv[1:]]
    head, rows = None, []
    for which in ("torch", "hip", "torch", "hip"):
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--leg", which] + passed
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            print(r.stdout)
            print(f"leg {which} ended with status {r.returncode}: nothing more is started")
            return r.returncode
        for line in r.stdout.splitlines():
            if line.startswith("LEG "):
                rows.append(line[4:])
                print(line[4:], flush=True)
            elif line.startswith("HEAD ") and head is None:
                head = line[5:]
    lines = [head] + rows
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(head)
    print(f"written: {out_path}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
