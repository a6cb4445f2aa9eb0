#!/usr/bin/env python3
"""decode_ops.extract_links_autograd on float64 q / k / log_gates (csrc/extract_links_f64.hip) against the only alternative a float64 caller
has, torch's dense double formulation (the [B,L,L,H] content tensor, the band gathered out of it, log_softmax, logsumexp) and its autograd —
same process, same tensors, HIP events around each leg, warm-up then median — with torch's peak memory beside the fused call's.  The fp32
kernels' times on the same shape are printed for scale.  GPU box only; a plain tool, not a test.  The table is printed and written to a file.

usage: links_f64_bench.py [B L CK] [--tr N ...] [--iters N] [--warmup N] [--no-torch] [--only-new] [--out FILE]
default shape: B 4, L 1024, CK 64 (torch's [B,L,L,H] doubles: 268 MB, and several of them under autograd), windows 32 and L-1;
default file: profiles/links_f64_bench.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                                                   # noqa: E402
from daspeech_amd import decode_ops                            # noqa: E402

H = 8


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


def torch_links(q, k, lg, olen, TR):
    """the dense formulation (DAGDecoder.extract_links with fused_links off) in the dtype of q"""
    B, L, _, CK = q.shape
    content = torch.einsum("bicf,bjcf->bijc", q, k) / (CK ** 0.5)
    idx = torch.arange(L, device=q.device).unsqueeze(1) + torch.arange(TR, device=q.device).unsqueeze(0) + 1
    invalid = idx.unsqueeze(0) >= olen.view(B, 1, 1)
    band = content.gather(2, idx.unsqueeze(0).masked_fill(invalid, 0).unsqueeze(-1).expand(-1, -1, -1, H))
    nouse = invalid.all(-1)
    band = band.masked_fill(invalid.unsqueeze(-1), float("-inf")).masked_fill(nouse.view(B, L, 1, 1), 0.0)
    band = torch.log_softmax(band, 2).masked_fill(invalid.unsqueeze(-1), -1e30)
    return torch.logsumexp(band + lg.unsqueeze(2), -1).masked_fill(invalid, float("-inf"))


def main():
    flags = ("--iters", "--warmup", "--out", "--tr")
    pos = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith("--") and sys.argv[i - 1] not in flags]
    B, L, CK = [int(v) for v in pos[:3]] if len(pos) >= 3 else (4, 1024, 64)
    iters, warmup = _opt("--iters", 9), _opt("--warmup", 2)
    windows = [int(sys.argv[i + 1]) for i, a in enumerate(sys.argv) if a == "--tr"] or [32, L - 1]
    out_path = _opt("--out", os.path.join(ROOT, "profiles", "links_f64_bench.txt"), str)
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    q = torch.randn((B, L, H, CK), dtype=torch.float64, device=dev, generator=gen) * 0.5
    k = torch.randn((B, L, H, CK), dtype=torch.float64, device=dev, generator=gen) * 0.5
    lg = torch.log_softmax(torch.randn((B, L, H), dtype=torch.float64, device=dev, generator=gen), -1)
    olen = torch.full((B,), L, dtype=torch.long, device=dev)
    olen[-1] = (2 * L) // 3
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"shape B {B} L {L} H {H} CK {CK}: q, k {B * L * H * CK * 8 / 1e6:.1f} MB each (double), torch's [B,L,L,H] content {B * L * L * H * 8 / 1e6:.0f} MB; "
        f"device {torch.cuda.get_device_name(0)}; median (min) of {iters} after {warmup} warm-up, HIP events")

    def report(name, ms, mn, against=None, peak=None):
        s = f"{name:<52s} {ms:9.3f} ms  (min {mn:8.3f})"
        if against is not None:
            s += f"  = {ms / against:6.3f} x torch's leg"
        if peak is not None:
            s += f"  peak memory + {peak:8.1f} MB"
        say(s)
        return ms

    for TR in windows:
        w = torch.randn((B, L, TR), dtype=torch.float64, device=dev, generator=gen)
        say(f"-- window TR {TR}: score FLOPs {2.0 * B * L * min(TR, L) * H * CK / 1e9:.2f} G (band, one pass)")

        def legs(fn, qq, kk, gg, ww):
            keep = {}
            leaves = [t.detach().clone().requires_grad_() for t in (qq, kk, gg)]

            def fwd():
                keep["links"] = fn(*leaves)
                return keep["links"]

            def bwd():
                lk = keep["links"]
                keep["g"] = torch.autograd.grad((lk.masked_fill(~torch.isfinite(lk), 0.0) * ww).sum(), leaves)
                return keep["g"]

            def both():
                fwd()
                return bwd()
            return keep, fwd, bwd, both

        t_f = t_b = None
        ref = None
        if "--no-torch" not in sys.argv:
            keep, fwd, bwd, both = legs(lambda a, b, c: torch_links(a, b, c, olen, TR), q, k, lg, w)
            pk_f = peak_of(fwd); keep.clear()
            pk_fb = peak_of(both); keep.clear()
            t_f = report("torch f64 dense formulation forward (with grad)", *timed(fwd, None, iters, warmup), peak=pk_f)
            t_b = report("torch f64 autograd backward (incl. the loss)", *timed(bwd, fwd, iters, warmup), peak=pk_fb)
            ref = (keep["links"].detach().clone(), [g.clone() for g in keep["g"]])
            keep.clear()
            torch.cuda.empty_cache()
        keep, fwd, bwd, both = legs(lambda a, b, c: decode_ops.extract_links_autograd(a, b, c, olen, TR), q, k, lg, w)
        fwd(); keep.clear()
        pk_f = peak_of(fwd); keep.clear()
        pk_fb = peak_of(both); keep.clear()
        n_f = report("f64 extract_links_autograd forward", *timed(fwd, None, iters, warmup), t_f, pk_f)
        n_b = report("f64 extract_links_autograd backward (incl. the loss)", *timed(bwd, fwd, iters, warmup), t_b, pk_fb)
        if ref is not None:
            fin = torch.isfinite(ref[0])
            say(f"    fused vs torch f64: links max abs diff {(keep['links'].detach()[fin] - ref[0][fin]).abs().max().item():.3e}, gradient max abs diff "
                f"{max((a - b).abs().max().item() for a, b in zip(keep['g'], ref[1])):.3e}")
            for leg, n, t in (("forward", n_f, t_f), ("backward", n_b, t_b)):
                say(f"    {leg}: the double kernels are {'slower' if n > t else 'faster'} than torch's dense formulation ({n:.3f} vs {t:.3f} ms)")
        keep.clear()
        ref = None
        if "--only-new" not in sys.argv:
            keep, fwd, bwd, both = legs(lambda a, b, c: decode_ops.extract_links_autograd(a, b, c, olen, TR), q.float(), k.float(), lg.float(), w.float())
            report("fp32 extract_links_autograd forward", *timed(fwd, None, iters, warmup))
            report("fp32 extract_links_autograd backward (incl. the loss)", *timed(bwd, fwd, iters, warmup))
            keep.clear()
        torch.cuda.empty_cache()

    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(f"written: {out_path}")


if __name__ == "__main__":
    main()
