#!/usr/bin/env python3
"""The optimizer half of the fp16 training step alone, at the released model's parameter list: FP16FlatOptimizer on the torch path
(hip_step=False: _foreach_copy_, mul_, vector_norm, mul_, fused AdamW, _foreach_copy_) against the HIP step (csrc/fp16_optim.hip), alternating in
one process, HIP events around each step() (the step's one sync included), warm-up then median / min / max.  The parameter sizes come from
the released model built on the `meta` device; parameters and gradients are random fp16.  Two segments: gradients whose norm stays below
clip_norm (no clip pass on the torch path) and gradients above it.  GB/s is against the derived byte counts per element — torch path 52 (60
when clipping), HIP step 30 — to be read against the measured copy ceiling of the device (about 6.3 TB/s on MI355X), not its spec.
torch.cuda.max_memory_allocated of each path is taken in a pass of its own, one optimizer alive at a time.

usage: fp16_optim_bench.py [--rounds N] [--warmup N] [--chunk C [C ...]] [--shares] [--out FILE]
  --chunk   work-item sizes of the HIP step to time (default: fp16_trainer.HIP_STEP_CHUNK)
  --shares  print which share of the elements takes which access path of the kernels and exit (no GPU needed)
default file: profiles/fp16_optim_bench.txt.  GPU box only (but for --shares); a plain tool, not a test."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                                                   # noqa: E402
from daspeech_amd import fp16_trainer as F                     # noqa: E402

TORCH_BYTES, TORCH_BYTES_CLIP, HIP_BYTES = 52, 60, 30


def _opt(name, default, conv=int):
    return conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def _opts(name, default):
    if name not in sys.argv:
        return default
    out = []
    for a in sys.argv[sys.argv.index(name) + 1:]:
        if a.startswith("--"):
            break
        out.append(int(a))
    return out


def released_sizes():
    from daspeech_amd.models.daspeech import S2SConformerDAGFastSpeech2Model
    with torch.device("meta"):
        m = S2SConformerDAGFastSpeech2Model()
    return [p.numel() for p in m.parameters() if p.requires_grad]


def path_shares(sizes, chunk):
    """Share of the elements per access path, for tensors that start on a 16-byte boundary (what the allocator hands out): the Adam pass (fp32
    as float4 with the 16-bit side in 8- / 4- / 2-byte pieces, or one element at a time in an item's head and tail) and the sum of squares
    (groups of eight from the item's first element in 16- / 8- / 4- / 2-byte pieces, or the tail one at a time)."""
    adam = {"float4 + 8 B": 0, "float4 + 4 B": 0, "float4 + 2 B": 0, "element-wise": 0}
    ssq = {"16 B": 0, "8 B": 0, "4 B": 0, "2 B": 0, "element-wise": 0}
    off = [0]
    for n in sizes:
        off.append(off[-1] + n)
    for ti, first, cnt in F.build_work_items(sizes, chunk):
        f0 = off[ti] + first
        head = min(cnt, (4 - f0 % 4) % 4)
        nvec = (cnt - head) // 4
        a = (2 * (first + head)) % 8
        adam["float4 + 8 B" if a == 0 else ("float4 + 4 B" if a % 4 == 0 else "float4 + 2 B")] += 4 * nvec
        adam["element-wise"] += cnt - 4 * nvec
        a = (2 * first) % 16
        ssq["16 B" if a == 0 else ("8 B" if a % 8 == 0 else ("4 B" if a % 4 == 0 else "2 B"))] += cnt // 8 * 8
        ssq["element-wise"] += cnt % 8
    return adam, ssq


def _time(fn):
    a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
    a.record(); r = fn(); b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), r


def alternate(legs, rounds, warmup):
    ts = {n: [] for n in legs}
    for i in range(warmup + rounds):
        for n, fn in legs.items():
            t, ok = _time(fn)
            assert ok is True, f"{n}: step() skipped"
            if i >= warmup:
                ts[n].append(t)
    return {n: (sorted(v)[len(v) // 2], min(v), max(v)) for n, v in ts.items()}


def make_optimizer(sizes, dev, hip, chunk=None, seed=0):
    gen = torch.Generator(device=dev).manual_seed(seed)
    params = [torch.nn.Parameter(torch.randn(n, device=dev, generator=gen).half()) for n in sizes]
    old = F.HIP_STEP_CHUNK
    if chunk:
        F.HIP_STEP_CHUNK = chunk
    try:
        opt = F.FP16FlatOptimizer(params, lr=1e-4, betas=(0.9, 0.999), weight_decay=0.01, clip_norm=1.0, init_scale=2.0 ** 7, hip_step=hip)
    finally:
        F.HIP_STEP_CHUNK = old
    return opt


def set_grads(opt, std, seed=1):
    gen = torch.Generator(device=opt.master.device).manual_seed(seed)
    for p in opt.params:
        p.grad = (torch.randn(p.shape, device=p.device, generator=gen) * std).half()


def main():
    rounds, warmup = max(100, _opt("--rounds", 100)), _opt("--warmup", 10)
    chunks = _opts("--chunk", [F.HIP_STEP_CHUNK])
    out_path = _opt("--out", os.path.join(ROOT, "profiles", "fp16_optim_bench.txt"), str)
    lines = []

    def say(t):
        print(t, flush=True)
        lines.append(t)

    sizes = released_sizes()
    n = sum(sizes)
    say(f"released parameter list: {len(sizes)} trainable tensors, {n} elements, sizes {min(sizes)} .. {max(sizes)}, "
        f"{sum(1 for s in sizes if s == 1)} of one element")
    for chunk in chunks:
        adam, ssq = path_shares(sizes, chunk)
        say(f"  chunk {chunk}: {len(F.build_work_items(sizes, chunk))} work items; Adam pass: "
            + ", ".join(f"{k} {100.0 * v / n:.4f} %" for k, v in adam.items()))
        say("    sum of squares: " + ", ".join(f"{k} {100.0 * v / n:.4f} %" for k, v in ssq.items()))
    if "--shares" in sys.argv:
        return
    dev = torch.device("cuda:0")
    say(f"device {torch.cuda.get_device_name(0)}; median (min .. max) of {rounds} alternations after {warmup} warm-up rounds, HIP events around step()")

    # memory: one optimizer alive at a time, parameters and gradients included
    for name, hip in (("torch", False), ("hip", True)):
        torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
        opt = make_optimizer(sizes, dev, hip)
        set_grads(opt, 1.0)
        for _ in range(2):
            assert opt.step() is True
        torch.cuda.synchronize()
        say(f"  max_memory_allocated {name:5s} {torch.cuda.max_memory_allocated() / 1e9:.3f} GB (allocated now {torch.cuda.memory_allocated() / 1e9:.3f} GB)")
        del opt
    torch.cuda.empty_cache()

    opts = {"torch": make_optimizer(sizes, dev, False)}
    for chunk in chunks:
        opts[f"hip chunk {chunk}"] = make_optimizer(sizes, dev, True, chunk)
    for label, std, tbytes in (("norm below clip_norm", 1e-3, TORCH_BYTES), ("norm above clip_norm (the torch path clips in a pass of its own)", 1.0, TORCH_BYTES_CLIP)):
        for o in opts.values():
            set_grads(o, std)
        res = alternate({k: o.step for k, o in opts.items()}, rounds, warmup)
        say(f"{label}: gradient norm {opts['torch'].last_grad_norm:.4g} (torch) {list(opts.values())[1].last_grad_norm:.4g} (hip)")
        for k, (med, lo, hi) in res.items():
            b = tbytes if k == "torch" else HIP_BYTES
            say(f"  {k:16s} {med:8.3f} ms (min {lo:8.3f} .. max {hi:8.3f})   {b} B/element -> {b * n / med / 1e9:6.2f} TB/s at the median")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(f"written: {out_path}")


if __name__ == "__main__":
    main()
