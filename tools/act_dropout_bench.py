#!/usr/bin/env python3
"""Forward + backward of ONE activation site alone — the element-wise pass between the two GEMMs of a feed-forward block, with the bias of
the Linear in front of it — at the shapes of a C5 step: the torch lines (activation, F.dropout on the GEMM's output with its bias added; autograd
backward and the row reduction of the bias gradient) against decode_ops.bias_act_dropout_autograd — same process, same tensors, the two legs INTERLEAVED round by round.
Per leg: GPU time by HIP events and host time (perf_counter around the calls, no sync inside) of forward + backward, warm-up then median
and the 10 % .. 90 % spread.  Then torch.cuda.max_memory_allocated over one forward + backward of a 12-layer Conformer encoder stack each
way (set_act_dropout_hip on / off).  GPU box only; a plain tool, not a test.  The table is printed and written.

usage: act_dropout_bench.py [--batch B] [--frames T] [--graph-len L] [--iters N] [--warmup N] [--out FILE]
default: B 32, T 200 (encoder frames of an 800-frame utterance), L 400 (its graph: src_upsample_scale 0.5 x 800), fp16, p 0.1;
default file: profiles/act_dropout_bench.txt"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                                                   # noqa: E402
import torch.nn.functional as F                                # noqa: E402
from daspeech_amd import decode_ops                            # noqa: E402
from daspeech_amd.models.daspeech import ConformerLayer, rel_positional_encoding      # noqa: E402


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


def main():
    B, T, L = _opt("--batch", 32), _opt("--frames", 200), _opt("--graph-len", 400)
    iters, warmup = _opt("--iters", 200), _opt("--warmup", 20)
    out_path = _opt("--out", os.path.join(ROOT, "profiles", "act_dropout_bench.txt"), str)
    dev, dtype, p = torch.device("cuda:0"), torch.float16, 0.1
    lines = []

    def say(t):
        print(t, flush=True)
        lines.append(t)

    say(f"one activation site alone, fp16 p {p}; device {torch.cuda.get_device_name(0)}; median (10 % .. 90 %) of {iters} rounds after {warmup} "
        f"warm-up, legs interleaved; forward + backward (gradients of h and of the bias)")
    fmt = lambda m: f"{m[0]:7.3f} ({m[1]:.3f} .. {m[2]:.3f})"
    acts = {"silu": F.silu, "gelu": F.gelu, "glu": lambda t: F.glu(t, dim=-1)}
    # (site, rows, Cin, act, bias, p)
    sites = [("encoder FFN   w_1 -> SiLU -> dropout", B * T, 2048, "silu", True, p),
             ("encoder conv  pointwise_conv1 -> GLU", B * T, 512, "glu", False, 0.0),
             ("decoder FFN   fc1 -> GELU -> dropout", B * L, 2048, "gelu", True, p)]
    for name, R, Cin, act, with_bias, ps in sites:
        gen = torch.Generator(device=dev).manual_seed(0)
        rnd = lambda *s: torch.randn(s, device=dev, generator=gen).to(dtype)
        h = rnd(R, Cin).requires_grad_()
        bias = (0.5 * rnd(Cin)).requires_grad_() if with_bias else None
        cot = rnd(R, Cin // 2 if act == "glu" else Cin)
        wrt = [h] + ([bias] if with_bias else [])
        assert decode_ops.bias_act_dropout_served(h, bias, act)

        # torch's Linear adds its bias in the GEMM epilogue, so the torch leg starts from h + bias as the GEMM leaves it and pays for the
        # bias only where the step does: the row reduction of the gradient in the backward
        hb_ = (h + bias).detach().requires_grad_() if with_bias else h

        def torch_lines():
            y = acts[act](hb_)
            return F.dropout(y, ps, True) if ps > 0 else y

        def torch_both():
            (g,) = torch.autograd.grad(torch_lines(), [hb_], cot)
            return (g, g.sum(0)) if with_bias else (g,)

        def hip_op():
            return decode_ops.bias_act_dropout_autograd(h, bias, act, ps, True)

        (tf, hf) = interleaved([torch_lines, hip_op], iters, warmup)
        (tb, hb) = interleaved([torch_both, lambda: torch.autograd.grad(hip_op(), wrt, cot)], iters, warmup)
        say(f"{name}   R {R} Cin {Cin} p {ps}")
        say(f"    torch lines   forward GPU {fmt(tf[0])} ms host {fmt(tf[1])} ms   forward + backward GPU {fmt(tb[0])} ms host {fmt(tb[1])} ms")
        say(f"    HIP operator  forward GPU {fmt(hf[0])} ms host {fmt(hf[1])} ms   forward + backward GPU {fmt(hb[0])} ms host {fmt(hb[1])} ms"
            f"   ratio torch / HIP: GPU {tb[0][0] / hb[0][0]:.2f} host {tb[1][0] / hb[1][0]:.2f}")
    # activation memory of an encoder stack: 12 layers, one forward + backward each way
    C, H = 256, 4
    torch.manual_seed(0)
    gen = torch.Generator(device=dev).manual_seed(0)
    layers = torch.nn.ModuleList(ConformerLayer(C, 2048, H, 31, dropout=p) for _ in range(12)).to(dev, dtype).train()
    x = torch.randn((B, T, C), device=dev, generator=gen).to(dtype)
    table = rel_positional_encoding(T, C, dev, dtype)
    pad = torch.zeros(B, T, dtype=torch.bool, device=dev)
    peaks = {}
    for on in (False, True):
        old = decode_ops.set_act_dropout_hip(on)
        try:
            for rep in range(2):                                        # the second run: allocator and libraries warm
                torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                y = x
                for layer in layers:
                    y = layer(y, table, pad)
                y.float().pow(2).mean().backward()
                torch.cuda.synchronize()
                peaks[on] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
                layers.zero_grad(set_to_none=True)
                del y
        finally:
            decode_ops.set_act_dropout_hip(old)
    say(f"12-layer encoder (dim {C}, ffn 2048, B {B} T {T}) forward + backward, peak memory above the resident tensors: torch lines "
        f"{peaks[False]:.1f} MiB, HIP operator {peaks[True]:.1f} MiB  (saved {peaks[False] - peaks[True]:.1f} MiB, "
        f"{(peaks[False] - peaks[True]) / 12:.1f} MiB per layer)")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(f"written: {out_path}")


if __name__ == "__main__":
    main()
