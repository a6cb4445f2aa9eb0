#!/usr/bin/env python3
"""Forward + backward of the variance-adaptor glue alone (bucketize + embedding add twice, length regulator) at the shapes of a C5 batch:
the differentiable torch formulation (VarianceAdaptor._forward_torch's ops) against decode_ops.bucketize_embed_add_autograd /
length_regulate_autograd — same process, same tensors, HIP events around each leg, warm-up then median.  The energy predictor between the
two adds is left out: it is the same torch code on both sides.  GPU box only; a plain tool, not a test.  The table is printed and written.

usage: glue_autograd_bench.py [--batch B] [--dtype fp16|fp32|bf16] [--iters N] [--warmup N] [--out FILE]
default: B 32 (synthetic.make_s2st_batch, seed 0: the durations / pitches / energies bench.py --workload train draws), fp16;
default file: profiles/glue_autograd_bench.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                                                   # noqa: E402
import torch.nn.functional as F                                # noqa: E402
from daspeech_amd import decode_ops                            # noqa: E402
from daspeech_amd.synthetic import make_s2st_batch             # noqa: E402


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
    B, iters, warmup = _opt("--batch", 32), _opt("--iters", 200), _opt("--warmup", 20)
    dtype = {"fp16": torch.float16, "fp32": torch.float32, "bf16": torch.bfloat16}[_opt("--dtype", "fp16", str)]
    out_path = _opt("--out", os.path.join(ROOT, "profiles", "glue_autograd_bench.txt"), str)
    dev = torch.device("cuda:0")
    s = make_s2st_batch(B, dev, seed=0)
    dur, pit, ene = s["durations"], s["pitches"].to(dtype), s["energies"].to(dtype)
    N, C, nbins = dur.shape[1], 256, 256
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((B, N, C), device=dev, generator=gen).to(dtype).requires_grad_()
    wp = torch.randn((nbins, C), device=dev, generator=gen).to(dtype).requires_grad_()
    we = torch.randn((nbins, C), device=dev, generator=gen).to(dtype).requires_grad_()
    pbins = torch.linspace(-4.66, 5.7333, nbins - 1, device=dev).to(dtype)
    ebins = torch.linspace(-4.9544, 3.2244, nbins - 1, device=dev).to(dtype)
    maxlen = int(dur.sum(1).max())
    cot = torch.randn((B, maxlen, C), device=dev, generator=gen).to(dtype)

    def torch_glue():
        h = x + F.embedding(torch.bucketize(pit, pbins), wp)
        h = h + F.embedding(torch.bucketize(ene, ebins), we)
        out_lens = dur.sum(1)
        ml = int(out_lens.max())
        cum = dur.cumsum(1)
        frames = torch.arange(ml, device=dev).unsqueeze(0).expand(B, -1)
        src = torch.searchsorted(cum, frames.contiguous(), right=True).clamp(max=max(N - 1, 0))
        return h.gather(1, src.unsqueeze(-1).expand(-1, -1, C)) * (frames < out_lens.unsqueeze(1)).unsqueeze(-1).to(h.dtype)

    def hip_glue():
        h = decode_ops.bucketize_embed_add_autograd(x, pit, pbins, wp)
        h = decode_ops.bucketize_embed_add_autograd(h, ene, ebins, we)
        return decode_ops.length_regulate_autograd(h, dur)[0]

    def both(glue):
        return torch.autograd.grad(glue(), [x, wp, we], cot)

    lines = []

    def say(t):
        print(t, flush=True)
        lines.append(t)

    say(f"variance-adaptor glue alone, B {B} N {N} C {C} bins {nbins} frames {maxlen} ({int(dur.sum())} valid), {dtype}; device "
        f"{torch.cuda.get_device_name(0)}; median (min) of {iters} after {warmup} warm-up, HIP events around forward + backward")
    res = {}
    for name, glue in (("torch formulation", torch_glue), ("HIP autograd ops", hip_glue), ("torch formulation (again)", torch_glue),
                       ("HIP autograd ops (again)", hip_glue)):
        f_ms, f_mn = timed(glue, iters, warmup)
        fb_ms, fb_mn = timed(lambda: both(glue), iters, warmup)
        res[name] = both(glue)
        say(f"{name:<28s} forward {f_ms:7.3f} ms (min {f_mn:7.3f})   forward + backward {fb_ms:7.3f} ms (min {fb_mn:7.3f})")
    gt, gh = res["torch formulation"], res["HIP autograd ops"]
    say("    HIP vs torch gradients, max abs diff: " + ", ".join(
        f"{n} {(a.float() - b.float()).abs().max().item():.3e} (scale {b.float().abs().max().item():.3e})" for n, a, b in zip(("x", "pitch table", "energy table"), gh, gt)))
    again = both(hip_glue)
    say("    HIP gradients bit-equal on a second call: " + str(all(torch.equal(a, b) for a, b in zip(gh, again))))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(f"written: {out_path}")


if __name__ == "__main__":
    main()
