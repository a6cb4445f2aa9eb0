#!/usr/bin/env python3
"""decode_ops.posterior_features on float64 alpha / beta / features (csrc/posterior_f64.hip) against the only alternative a float64 caller
has, torch's own double two-step `nan_to_num(exp(a + b - logsumexp)) @ f` and its autograd — same process, same tensors, HIP events around
each leg, warm-up then median — with torch's peak memory (it holds [B,T,L] doubles) beside the fused call's.  The fp32 kernels' times on the
same shape are printed for scale.  GPU box only; a plain tool, not a test.  The table is printed and written to a file.

usage: posterior_f64_bench.py [B T L D] [--iters N] [--warmup N] [--no-torch] [--only-new] [--out FILE]
default shape: C2's, B 32, T 512, L 4096, D 512 (alpha and beta 537 MB each in double; 68.7 GFLOP per direction);
default file: profiles/posterior_f64_bench.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                                                   # noqa: E402
from daspeech_amd import decode_ops                            # noqa: E402

FP64_FMA_TFLOPS = 78.6      # MI355X vector fp64: 256 CUs x 4 SIMDs x 16 lanes x 2 FLOP x 2.4 GHz (half the 157.3 TF fp32 vector rate)


def _opt(name, default, conv=int):
    return conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def timed(fn, prep, iters, warmup):
    """median / min HIP-event time (ms) of fn(); prep() runs before every call, outside the event bracket."""
    ts = []
    for i in range(warmup + iters):
        if prep is not None:
            prep()
        a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def peak_of(fn):
    """rise of the peak of allocated device memory across fn(), MB"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    keep = fn()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    del keep
    return rise / 1e6


def main():
    flags = ("--iters", "--warmup", "--out")
    pos = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith("--") and sys.argv[i - 1] not in flags]
    B, T, L, D = [int(v) for v in pos[:4]] if len(pos) >= 4 else (32, 512, 4096, 512)
    iters, warmup = _opt("--iters", 9), _opt("--warmup", 2)
    out_path = _opt("--out", os.path.join(ROOT, "profiles", "posterior_f64_bench.txt"), str)
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    # alpha + beta of a DP are large negative numbers with a narrow live band; what the kernels cost does not depend on the values
    a = torch.randn((B, T, L), dtype=torch.float64, device=dev, generator=gen) * 4 - 300
    b = torch.randn((B, T, L), dtype=torch.float64, device=dev, generator=gen) * 4 - 300
    a[:, T - 2:, :] = float("-inf")                                 # two dead rows per sample
    f = torch.randn((B, L, D), dtype=torch.float64, device=dev, generator=gen)
    g = torch.randn((B, T, D), dtype=torch.float64, device=dev, generator=gen)
    flop = 2.0 * B * T * L * D
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"shape B {B} T {T} L {L} D {D}: alpha, beta {B * T * L * 8 / 1e6:.0f} MB each (double), features {B * L * D * 8 / 1e6:.0f} MB, "
        f"{flop / 1e9:.1f} GFLOP per direction; device {torch.cuda.get_device_name(0)}; median (min) of {iters} after {warmup} warm-up, HIP events")

    def report(name, ms, mn, against=None, peak=None, rate=True):
        s = f"{name:<52s} {ms:9.3f} ms  (min {mn:8.3f})"
        if rate:
            tf = flop / (ms * 1e-3) / 1e12
            s += f"  {tf:6.2f} TFLOP/s = {tf / FP64_FMA_TFLOPS:5.3f} of the {FP64_FMA_TFLOPS} TF fp64 FMA rate"
        if against is not None:
            s += f"  = {ms / against:5.3f} x torch's leg"
        if peak is not None:
            s += f"  peak memory + {peak:8.1f} MB"
        say(s)
        return ms

    t_f = t_b = None
    ref_out = ref_gf = None
    if "--no-torch" not in sys.argv:
        fr = f.detach().clone().requires_grad_()
        keep = {}

        def torch_fwd():
            s = a + b
            keep["out"] = torch.nan_to_num(torch.exp(s - torch.logsumexp(s, -1, keepdim=True))) @ fr
            return keep["out"]

        def torch_bwd():
            keep["gf"] = torch.autograd.grad(keep["out"], [fr], grad_outputs=g)[0]
            return keep["gf"]

        def torch_both():
            torch_fwd()
            return torch_bwd()
        pk_f = peak_of(torch_fwd)
        keep.clear()
        pk_fb = peak_of(torch_both)
        t_f = report("torch f64 two-step forward (with grad)", *timed(torch_fwd, None, iters, warmup), peak=pk_f)
        t_b = report("torch f64 autograd backward", *timed(torch_bwd, torch_fwd, iters, warmup), peak=pk_fb)
        ref_out, ref_gf = keep["out"].detach().clone(), keep["gf"].clone()
        keep.clear()
        del fr
        torch.cuda.empty_cache()

    fd = f.detach().clone().requires_grad_()
    keep = {}

    def fused_fwd():
        keep["out"] = decode_ops.posterior_features(a, b, fd)
        return keep["out"]

    def fused_bwd():
        keep["gf"] = torch.autograd.grad(keep["out"], [fd], grad_outputs=g)[0]
        return keep["gf"]

    def fused_both():
        fused_fwd()
        return fused_bwd()
    fused_fwd(); keep.clear()
    pk_f = peak_of(fused_fwd)
    keep.clear()
    pk_fb = peak_of(fused_both)
    n_f = report("f64 fused posterior_features forward", *timed(fused_fwd, None, iters, warmup), t_f, pk_f)
    n_b = report("f64 fused posterior_features backward", *timed(fused_bwd, fused_fwd, iters, warmup), t_b, pk_fb)
    report("f64 posterior (the [B,T,L] score itself)", *timed(lambda: decode_ops.posterior(a, b), None, iters, warmup), rate=False)
    if ref_out is not None:
        say(f"    fused vs torch f64: out max abs diff {(keep['out'].detach() - ref_out).abs().max().item():.3e}, "
            f"gradient max abs diff {(keep['gf'] - ref_gf).abs().max().item():.3e}")
        for leg, n, t in (("forward", n_f, t_f), ("backward", n_b, t_b)):
            say(f"    {leg}: the fused double call is {'slower' if n > t else 'faster'} than torch's two-step ({n:.3f} vs {t:.3f} ms)")
    keep.clear()
    del ref_out, ref_gf

    if "--only-new" not in sys.argv:
        a32, b32, g32 = a.float(), b.float(), g.float()
        f32 = f.float().requires_grad_()
        del a, b
        torch.cuda.empty_cache()
        k32 = {}

        def f32_fwd():
            k32["out"] = decode_ops.posterior_features(a32, b32, f32)

        def f32_bwd():
            k32["gf"] = torch.autograd.grad(k32["out"], [f32], grad_outputs=g32)[0]
        report("fp32 fused posterior_features forward", *timed(f32_fwd, None, iters, warmup), rate=False)
        report("fp32 fused posterior_features backward", *timed(f32_bwd, f32_fwd, iters, warmup), rate=False)

    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(f"written: {out_path}")


if __name__ == "__main__":
    main()
