#!/usr/bin/env python3
"""dag_logsoftmax_gather_inplace on float64 logits (csrc/logsoftmax_gather_f64.hip) against the only alternative a float64 caller has,
torch's own double path `x.log_softmax(-1).gather(-1, idx)` and its autograd backward — same process, same tensors, HIP events around each
leg, warm-up then median (as bench.py's `dag` leg times gather_fwd / gather_bwd, through the launch wrappers the autograd Function uses).
The fp32 kernels' times on the same shape are printed for scale.  GPU box only; a plain tool, not a test.

usage: lsg_f64_bench.py [B L V S] [--iters N] [--warmup N] [--no-torch] [--only-new]
default shape: C2's K1 shape in double, B 32, L 4096, V 8192, S 512 (8.6 GB of logits)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                   # noqa: E402
import daspeech_amd.custom_ops                                 # noqa: E402,F401

dl = sys.modules["daspeech_amd.custom_ops.dag_loss"]


def _opt(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


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


def main():
    pos = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith("--") and not sys.argv[i - 1] in ("--iters", "--warmup")]
    B, L, V, S = [int(v) for v in pos[:4]] if len(pos) >= 4 else (32, 4096, 8192, 512)
    iters, warmup = _opt("--iters", 9), _opt("--warmup", 2)
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    master = torch.randn((B, L, V), dtype=torch.float64, device=dev, generator=gen) * 3
    tgt = torch.randint(0, V, (B, S), device=dev, generator=gen)
    idx = tgt.unsqueeze(1).expand(-1, L, -1)
    g = torch.randn((B, S, L), dtype=torch.float64, device=dev, generator=gen).transpose(1, 2)        # [B,L,S] view, runs along the vertex axis
    x = master.clone()
    BLV, BSL = float(B) * L * V, float(B) * S * L
    print(f"shape B {B} L {L} V {V} S {S}: logits {BLV * 8 / 1e9:.2f} GB (double), match {BSL * 8 / 1e9:.3f} GB; "
          f"device {torch.cuda.get_device_name(0)}; median (min) of {iters} after {warmup} warm-up, HIP events")
    rows = []

    def report(name, ms, mn, nbytes=None, against=None):
        s = f"{name:<44s} {ms:9.3f} ms  (min {mn:8.3f})"
        if nbytes is not None:
            s += f"  {nbytes / 1e9:6.2f} GB algorithmic -> {nbytes / (ms * 1e-3) / 1e12:5.2f} TB/s"
        if against is not None:
            s += f"  = {ms / against:5.3f} x torch's leg"
        print(s, flush=True)
        rows.append((name, ms))
        return ms

    def restore():
        x.copy_(master)

    # ---- torch's double path first (the yardstick): forward without / with autograd, backward
    t_fwd_ng = t_fwd_g = t_bwd = None
    if "--no-torch" not in sys.argv:
        def torch_fwd_nograd():
            with torch.no_grad():
                return x.log_softmax(-1).gather(-1, idx)
        t_fwd_ng = report("torch f64 log_softmax.gather, no grad", *timed(torch_fwd_nograd, None, iters, warmup))
        xr = x.detach().requires_grad_()
        keep = {}

        def torch_fwd_grad():
            keep["m"] = xr.log_softmax(-1).gather(-1, idx)
        t_fwd_g = report("torch f64 log_softmax.gather, with grad", *timed(torch_fwd_grad, None, iters, warmup))

        def torch_bwd():
            keep["gx"] = torch.autograd.grad(keep["m"], [xr], grad_outputs=g)[0]
        t_bwd = report("torch f64 autograd backward", *timed(torch_bwd, torch_fwd_grad, iters, warmup))
        ref_match = keep["m"].detach()
        ref_gx = keep.pop("gx")
        keep.clear()
        del xr

    # ---- the double kernels
    f_bytes, fw_bytes, b_bytes = BLV * 8 + BSL * 8, 2 * BLV * 8 + BSL * 8, 2 * BLV * 8 + BSL * 8
    out = {}

    def fwd_nograd():
        out["m"], _ = dl._lsg64_forward(x, idx, False, False)

    def fwd_eager():
        out["m"], _ = dl._lsg64_forward(x, idx, True, False)

    def fwd_lazy():
        out["m"], out["st"] = dl._lsg64_forward(x, idx, False, True)

    def bwd_eager():
        dl._lsg64_backward(x, idx, g)

    def bwd_lazy():
        dl._lsg64_backward(x, idx, g, out["st"])

    def prep_bwd_eager():
        restore(); fwd_eager()

    report("f64 (a) forward, no gradient", *timed(fwd_nograd, None, iters, warmup), f_bytes, t_fwd_ng)
    report("f64 (b) forward, softmax stored (eager)", *timed(fwd_eager, restore, iters, warmup), fw_bytes, t_fwd_g)
    restore()
    report("f64 (c) forward, lazy (row statistics)", *timed(fwd_lazy, None, iters, warmup), f_bytes, t_fwd_g)
    if t_fwd_ng is not None:
        d = (out["m"].transpose(1, 2) - ref_match)
        print(f"    match vs torch f64: max abs diff {d[torch.isfinite(d)].abs().max().item():.3e}")
    report("f64 (d) backward from the softmax (eager)", *timed(bwd_eager, prep_bwd_eager, iters, warmup), b_bytes, t_bwd)
    if t_bwd is not None:
        print(f"    gradient vs torch f64 autograd: max abs diff {(x - ref_gx).abs().max().item():.3e}")
    restore(); fwd_lazy()
    report("f64 (d) backward from the logits (lazy)", *timed(bwd_lazy, restore, iters, warmup), b_bytes, t_bwd)
    if t_bwd is not None:
        print(f"    gradient vs torch f64 autograd: max abs diff {(x - ref_gx).abs().max().item():.3e}")
        del ref_gx, ref_match

    # ---- the fp32 kernels on the same shape, for scale
    if "--only-new" not in sys.argv:
        del x
        m32 = master.float()
        del master
        torch.cuda.empty_cache()
        x32 = m32.clone()
        g32 = g.float()
        o32 = {}

        def restore32():
            x32.copy_(m32)

        def f32_eager():
            dl._lsg_forward(x32, idx, True)

        def f32_lazy():
            o32["m"], o32["st"] = dl._lsg_forward_lazy(x32, idx)

        def prep32():
            restore32(); f32_eager()
        f32b, f32wb = BLV * 4 + BSL * 4, 2 * BLV * 4 + BSL * 4
        report("fp32 forward, no gradient", *timed(lambda: dl._lsg_forward(x32, idx, False), None, iters, warmup), f32b)
        report("fp32 forward, softmax stored (eager)", *timed(f32_eager, restore32, iters, warmup), f32wb)
        restore32()
        report("fp32 forward, lazy", *timed(f32_lazy, None, iters, warmup), f32b)
        report("fp32 backward from the softmax (eager)", *timed(lambda: dl._lsg_backward(x32, idx, g32), prep32, iters, warmup), f32wb)
        restore32(); f32_lazy()
        report("fp32 backward from the logits (lazy)", *timed(lambda: dl._lsg_backward(x32, idx, g32, o32["st"]), restore32, iters, warmup), f32wb)


if __name__ == "__main__":
    main()
