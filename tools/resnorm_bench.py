#!/usr/bin/env python3
"""Forward + backward of one residual site of the training step alone — s = residual + alpha * dropout(h [+ bias]); y = LayerNorm(s) — at
the site shapes of a C5 step: the torch lines of the training branches (add bias -> F.dropout -> scale -> add -> LayerNorm, autograd
backward, the bias gradient a column sum) against decode_ops.residual_dropout_layer_norm_autograd — same process, same tensors, the two
legs INTERLEAVED round by round, HIP events around each leg, warm-up then median and the 10 % .. 90 % spread.  GPU box only; a plain tool,
not a test.  The table is printed and written.

usage: resnorm_bench.py [--batch B] [--iters N] [--warmup N] [--out FILE]
default: B 32; rows B x 200 at C 256 (Conformer encoder: 800 fbank frames after the 4x subsampler), B x 400 at C 512 (NAT decoder: the
graph of 0.5 x 800 vertices), B x 800 at C 256 (FastSpeech2 decoder: mel frames); fp16 and fp32; default file: profiles/resnorm_bench.txt"""
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


def one(fn):
    a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def interleaved(fns, iters, warmup):
    """every leg once per round, in turn -> per leg (median, 10 %, 90 %) in ms"""
    ts = [[] for _ in fns]
    for i in range(warmup + iters):
        for k, fn in enumerate(fns):
            t = one(fn)
            if i >= warmup:
                ts[k].append(t)
    out = []
    for t in ts:
        t.sort()
        out.append((t[len(t) // 2], t[len(t) // 10], t[(9 * len(t)) // 10]))
    return out


def main():
    B = _opt("--batch", 32)
    iters, warmup = _opt("--iters", 200), _opt("--warmup", 20)
    out_path = _opt("--out", os.path.join(ROOT, "profiles", "resnorm_bench.txt"), str)
    dev = torch.device("cuda:0")
    lines = []

    def say(t):
        print(t, flush=True)
        lines.append(t)

    say(f"one residual + dropout + LayerNorm site alone, B {B}; device {torch.cuda.get_device_name(0)}; median (10 % .. 90 %) of {iters} rounds after "
        f"{warmup} warm-up, legs interleaved, HIP events around forward + backward (gradients of h, residual, bias, LayerNorm weight and bias)")
    sites = [("conformer ffn -> next norm (pre-norm, alpha 0.5, bias, s and y)", 200, 256, dict(alpha=0.5, bias=True, pre=True, p=0.1)),
             ("conformer block -> next norm (pre-norm, no bias, s and y)", 200, 256, dict(alpha=1.0, bias=False, pre=True, p=0.1)),
             ("conformer first norm (h None: LayerNorm alone)", 200, 256, dict(alpha=1.0, bias=False, pre=False, p=0.0, plain=True)),
             ("NAT decoder site (post-norm, bias)", 400, 512, dict(alpha=1.0, bias=True, pre=False, p=0.1)),
             ("FastSpeech2 FFT attention site (post-norm, no dropout)", 800, 256, dict(alpha=1.0, bias=False, pre=False, p=0.0)),
             ("FastSpeech2 FFT conv site (post-norm, h a transposed view: copied first)", 800, 256, dict(alpha=1.0, bias=False, pre=False, p=0.1, tview=True))]
    for dtype in (torch.float16, torch.float32):
        for name, T, C, o in sites:
            gen = torch.Generator(device=dev).manual_seed(0)
            ln = nn.LayerNorm(C).to(dev, dtype)
            rnd = lambda *s: torch.randn(s, device=dev, generator=gen).to(dtype)
            res = rnd(B, T, C).requires_grad_()
            h = (rnd(B, C, T).transpose(1, 2) if o.get("tview") else rnd(B, T, C)).requires_grad_()
            bias = rnd(C).requires_grad_() if o["bias"] else None
            cy, cs = rnd(B, T, C), rnd(B, T, C)
            plain = o.get("plain", False)
            wrt = [res, ln.weight, ln.bias] + ([] if plain else [h]) + ([bias] if bias is not None else [])
            assert decode_ops.residual_dropout_layer_norm_served(None if plain else h.contiguous(), res, ln, bias=bias)

            def torch_lines():
                if plain:
                    return (ln(res),)
                z = h if bias is None else h + bias
                z = F.dropout(z, o["p"], True) if o["p"] > 0 else z
                s = res + (z if o["alpha"] == 1.0 else o["alpha"] * z)
                return (ln(s), s) if o["pre"] else (ln(s),)

            def hip_op():
                if plain:
                    return (decode_ops.residual_dropout_layer_norm_autograd(None, res, ln),)
                r = decode_ops.residual_dropout_layer_norm_autograd(h.contiguous() if o.get("tview") else h, res, ln, bias=bias, alpha=o["alpha"],
                                                                    p=o["p"], training=True, return_sum=o["pre"])
                return (r[1], r[0]) if o["pre"] else (r,)

            def both(fwd):
                outs = fwd()
                return torch.autograd.grad(outs, wrt, [cy, cs][:len(outs)])

            (tf, hf) = interleaved([torch_lines, hip_op], iters, warmup)
            (tb, hb) = interleaved([lambda: both(torch_lines), lambda: both(hip_op)], iters, warmup)
            fmt = lambda m: f"{m[0]:7.3f} ({m[1]:.3f} .. {m[2]:.3f})"
            say(f"{str(dtype):<14s} rows {B * T:6d} C {C:4d}  {name}")
            say(f"    torch lines   forward {fmt(tf)} ms   forward + backward {fmt(tb)} ms")
            say(f"    HIP operator  forward {fmt(hf)} ms   forward + backward {fmt(hb)} ms   ratio torch / HIP {tb[0] / hb[0]:.2f}"
                + ("   (inside the spread)" if hb[1] <= tb[0] <= hb[2] or tb[1] <= hb[0] <= tb[2] else ""))
            if o["p"] == 0:
                gt, gh = both(torch_lines), both(hip_op)
                say("    HIP vs torch gradients, max abs diff: " + ", ".join(
                    f"{(a.float() - b.float()).abs().max().item():.2e} (scale {b.float().abs().max().item():.2e})" for a, b in zip(gh, gt)))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(f"written: {out_path}")


if __name__ == "__main__":
    main()
