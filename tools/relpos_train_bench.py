#!/usr/bin/env python3
"""Forward + backward of the Conformer relative-position attention of one encoder layer alone — between the q / k / v / position projections
and linear_out — at the shapes of a C5 step: the torch lines of RelPosSelfAttention's training branch (bias adds, two batched GEMMs,
rel_shift, scale, masked_fill, soft-max, dropout, the value GEMM; autograd backward) against decode_ops.relpos_attention_autograd — same
process, same tensors, the two legs INTERLEAVED round by round.  Per leg: GPU time by HIP events and host time (perf_counter around the
calls, no sync inside) of forward + backward, warm-up then median and the 10 % .. 90 % spread.  Then torch.cuda.max_memory_allocated over
one forward + backward of a 12-layer Conformer encoder stack each way (set_relpos_attention_hip on / off).  GPU box only; a plain tool, not
a test.  The table is printed and written.

usage: relpos_train_bench.py [--batch B] [--heads H] [--iters N] [--warmup N] [--out FILE]
default: B 32, H 4, T 75 and 200, fp16, p 0.1; default file: profiles/relpos_train_bench.txt"""
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                                                   # noqa: E402
import torch.nn.functional as F                                # noqa: E402
from daspeech_amd import decode_ops                            # noqa: E402
from daspeech_amd.models.daspeech import ConformerLayer, RelPosSelfAttention, rel_positional_encoding      # noqa: E402


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
    B, H = _opt("--batch", 32), _opt("--heads", 4)
    iters, warmup = _opt("--iters", 200), _opt("--warmup", 20)
    out_path = _opt("--out", os.path.join(ROOT, "profiles", "relpos_train_bench.txt"), str)
    dev, dtype, p, C = torch.device("cuda:0"), torch.float16, 0.1, H * 64
    lines = []

    def say(t):
        print(t, flush=True)
        lines.append(t)

    say(f"relative-position attention of one Conformer layer alone, B {B} H {H} fp16 p {p}; device {torch.cuda.get_device_name(0)}; median (10 % .. 90 %) "
        f"of {iters} rounds after {warmup} warm-up, legs interleaved; forward + backward (gradients of q, k, v, pos, bias_u, bias_v)")
    fmt = lambda m: f"{m[0]:7.3f} ({m[1]:.3f} .. {m[2]:.3f})"
    for T in (75, 200):
        gen = torch.Generator(device=dev).manual_seed(0)
        rnd = lambda *s: torch.randn(s, device=dev, generator=gen).to(dtype)
        q, k, v = (rnd(B, T, C).requires_grad_() for _ in range(3))
        pos = rnd(2 * T - 1, C).requires_grad_()
        bu, bv = (0.5 * rnd(H, 64)).requires_grad_(), (0.5 * rnd(H, 64)).requires_grad_()
        lens = torch.randint(max(1, T // 2), T + 1, (B,), device=dev, generator=gen)
        lens[0] = T
        pad = torch.arange(T, device=dev).unsqueeze(0) >= lens.unsqueeze(1)
        cot = rnd(B, T, C)
        wrt = [q, k, v, pos, bu, bv]
        assert decode_ops.relpos_attention_autograd_served(q, k, v, pos, bu, bv, pad, H)

        def torch_lines():
            qh = q.view(B, T, H, 64)
            kh, vh = k.view(B, T, H, 64).transpose(1, 2), v.view(B, T, H, 64).transpose(1, 2)
            ph = pos.view(1, -1, H, 64).transpose(1, 2)
            ac = torch.matmul((qh + bu).transpose(1, 2), kh.transpose(-2, -1))
            bd = RelPosSelfAttention.rel_shift(torch.matmul((qh + bv).transpose(1, 2), ph.transpose(-2, -1)))
            scores = ((ac + bd) / math.sqrt(64)).masked_fill(pad.view(B, 1, 1, T), float("-inf"))
            att = F.dropout(torch.softmax(scores, dim=-1), p, True)
            return torch.matmul(att, vh).transpose(1, 2).reshape(B, T, C)

        def hip_op():
            return decode_ops.relpos_attention_autograd(q, k, v, pos, bu, bv, pad, H, p=p, training=True)

        both = lambda fwd: torch.autograd.grad(fwd(), wrt, cot)
        (tf, hf) = interleaved([torch_lines, hip_op], iters, warmup)
        (tb, hb) = interleaved([lambda: both(torch_lines), lambda: both(hip_op)], iters, warmup)
        say(f"T {T:4d}")
        say(f"    torch lines   forward GPU {fmt(tf[0])} ms host {fmt(tf[1])} ms   forward + backward GPU {fmt(tb[0])} ms host {fmt(tb[1])} ms")
        say(f"    HIP operator  forward GPU {fmt(hf[0])} ms host {fmt(hf[1])} ms   forward + backward GPU {fmt(hb[0])} ms host {fmt(hb[1])} ms"
            f"   ratio torch / HIP: GPU {tb[0][0] / hb[0][0]:.2f} host {tb[1][0] / hb[1][0]:.2f}")
        # activation memory of an encoder stack: 12 layers, one forward + backward each way
        torch.manual_seed(0)
        layers = torch.nn.ModuleList(ConformerLayer(C, 4 * C, H, 31, dropout=p) for _ in range(12)).to(dev, dtype).train()
        x = rnd(B, T, C)
        table = rel_positional_encoding(T, C, dev, dtype)
        peaks = {}
        for on in (False, True):
            old = decode_ops.set_relpos_attention_hip(on)
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
                decode_ops.set_relpos_attention_hip(old)
        say(f"    12-layer encoder forward + backward, peak memory above the resident tensors: torch lines {peaks[False]:.1f} MiB, HIP operator "
            f"{peaks[True]:.1f} MiB  (saved {peaks[False] - peaks[True]:.1f} MiB, {(peaks[False] - peaks[True]) / 12:.1f} MiB per layer)")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(f"written: {out_path}")


if __name__ == "__main__":
    main()
