#!/usr/bin/env python3
"""Forward + backward of the Conformer convolution module's inner half alone (depthwise conv -> batch-statistics BatchNorm -> SiLU) at the
shape of a C5 encoder layer: the torch lines of ConformerLayer's training branch (transpose -> Conv1d(groups=C) -> BatchNorm1d -> SiLU ->
transpose, autograd backward) against decode_ops.dwconv_bn_silu_autograd — same process, same tensors, HIP events around each leg, warm-up
then median.  GPU box only; a plain tool, not a test.  The table is printed and written.

usage: convmod_bench.py [--batch B] [--frames T] [--dim C] [--kernel K] [--iters N] [--warmup N] [--out FILE]
default: B 32, T 200 (800 fbank frames after the 4x subsampler: the longest utterances of bench.py --workload train), C 256, K 31;
fp16 and fp32; default file: profiles/convmod_bench.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                                                   # noqa: E402
import torch.nn as nn                                          # noqa: E402
import torch.nn.functional as F                                # noqa: E402
from daspeech_amd import decode_ops                            # noqa: E402


def _opt(name, default, conv=int):
    return conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def timed(fn, iters, warmup):
    ts = []
    for i in range(warmup + iters):
        a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def main():
    B, T, C, K = _opt("--batch", 32), _opt("--frames", 200), _opt("--dim", 256), _opt("--kernel", 31)
    iters, warmup = _opt("--iters", 200), _opt("--warmup", 20)
    out_path = _opt("--out", os.path.join(ROOT, "profiles", "convmod_bench.txt"), str)
    dev = torch.device("cuda:0")
    lines = []

    def say(t):
        print(t, flush=True)
        lines.append(t)

    say(f"convolution module inner half alone, B {B} T {T} C {C} K {K}; device {torch.cuda.get_device_name(0)}; median (min) of {iters} after "
        f"{warmup} warm-up, HIP events around forward + backward (gradients of x, conv weight, BN weight and bias)")
    for dtype in (torch.float16, torch.float32):
        gen = torch.Generator(device=dev).manual_seed(0)
        conv = nn.Conv1d(C, C, K, padding=(K - 1) // 2, groups=C, bias=False).to(dev, dtype)
        bn = nn.BatchNorm1d(C).to(dev, dtype).train()
        x = torch.randn((B, T, C), device=dev, generator=gen).to(dtype).requires_grad_()
        cot = torch.randn((B, T, C), device=dev, generator=gen).to(dtype)
        params = [x, conv.weight, bn.weight, bn.bias]
        assert decode_ops.dwconv_bn_silu_autograd_served(x, conv, bn)

        def torch_lines():
            return F.silu(bn(conv(x.transpose(1, 2)))).transpose(1, 2)

        def hip_op():
            return decode_ops.dwconv_bn_silu_autograd(x, conv.weight, bn)

        def both(fwd):
            return torch.autograd.grad(fwd(), params, cot)

        res = {}
        for name, fwd in (("torch lines", torch_lines), ("HIP operator", hip_op), ("torch lines (again)", torch_lines), ("HIP operator (again)", hip_op)):
            f_ms, f_mn = timed(fwd, iters, warmup)
            fb_ms, fb_mn = timed(lambda: both(fwd), iters, warmup)
            res[name] = both(fwd)
            say(f"{str(dtype):<14s} {name:<22s} forward {f_ms:7.3f} ms (min {f_mn:7.3f})   forward + backward {fb_ms:7.3f} ms (min {fb_mn:7.3f})")
        gt, gh = res["torch lines"], res["HIP operator"]
        say("    HIP vs torch gradients, max abs diff: " + ", ".join(
            f"{n} {(a.float() - b.float()).abs().max().item():.3e} (scale {b.float().abs().max().item():.3e})"
            for n, a, b in zip(("x", "conv weight", "BN weight", "BN bias"), gh, gt)))
        say("    HIP gradients bit-equal on a second call: " + str(all(torch.equal(a, b) for a, b in zip(gh, both(hip_op)))))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(f"written: {out_path}")


if __name__ == "__main__":
    main()
