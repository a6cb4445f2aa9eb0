#!/usr/bin/env python3
"""The optimizer half of the fp16 training step alone, at the released model's parameter list: FP16FlatOptimizer on the torch path
(hip_step=False: _foreach_copy_, mul_, vector_norm, mul_, fused AdamW, _foreach_copy_) against the HIP step (csrc/fp16_optim.hip), alternating in
one process, HIP events around each step() (the step's one sync included), warm-up then median / min / max.  The parameter sizes come from
the released model built on the `meta` device; parameters and gradients are random fp16.  Two segments: gradients whose norm stays below
clip_norm (no clip pass on the torch path) and gradients above it.  GB/s is against the derived byte counts per element — torch path 52 (60
when clipping), HIP step 30 — to be read against the measured copy ceiling of the device (about 6.3 TB/s on MI355X), not its spec.
torch.cuda.max_memory_allocated of each path is taken in a pass of its own, one optimizer alive at a time.

--device-scaler: the HIP step's two modes instead — the host reading the norm (device_scaler=False, the default) against the decisions made
on the device (device_scaler=True: three launches, no wait) — in alternating rounds: the time until the GPU is idle by events around step(),
the host time of step() with the GPU idle before it, and the C5 training step of daspeech_amd/synthetic.py (bench.py's --workload train) with
each optimizer in alternating pairs, the host-sync runs' own spread beside the medians.

usage: fp16_optim_bench.py [--rounds N] [--warmup N] [--chunk C [C ...]] [--shares] [--out FILE]
       fp16_optim_bench.py --device-scaler [--rounds N] [--warmup N] [--pairs N] [--steps N] [--out FILE]
  --chunk   work-item sizes of the HIP step to time (default: fp16_trainer.HIP_STEP_CHUNK)
  --shares  print which share of the elements takes which access path of the kernels and exit (no GPU needed)
  --pairs, --steps   C5 leg of --device-scaler: alternating pairs of runs of --steps training steps each (default 5 pairs of 20)
default file: profiles/fp16_optim_bench.txt (profiles/fp16_optim_device_scaler.txt with --device-scaler).  GPU box only (but for --shares); a
plain tool, not a test."""
import os
import sys
import time

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


def make_optimizer(sizes, dev, hip, chunk=None, seed=0, device_scaler=False):
    gen = torch.Generator(device=dev).manual_seed(seed)
    params = [torch.nn.Parameter(torch.randn(n, device=dev, generator=gen).half()) for n in sizes]
    old = F.HIP_STEP_CHUNK
    if chunk:
        F.HIP_STEP_CHUNK = chunk
    try:
        opt = F.FP16FlatOptimizer(params, lr=1e-4, betas=(0.9, 0.999), weight_decay=0.01, clip_norm=1.0, init_scale=2.0 ** 7, hip_step=hip,
                                  device_scaler=device_scaler)
    finally:
        F.HIP_STEP_CHUNK = old
    return opt


def set_grads(opt, std, seed=1):
    gen = torch.Generator(device=opt.master.device).manual_seed(seed)
    for p in opt.params:
        p.grad = (torch.randn(p.shape, device=p.device, generator=gen) * std).half()


def _median(v):
    return sorted(v)[len(v) // 2]


def device_scaler_site(sizes, dev, rounds, warmup, say):
    """host-sync against device mode at the site: events around step() (launch to GPU idle) and the host's own time inside step()"""
    opts = {"host-sync": make_optimizer(sizes, dev, True), "device": make_optimizer(sizes, dev, True, device_scaler=True)}
    for label, std in (("norm below clip_norm", 1e-3), ("norm above clip_norm", 1.0)):
        for o in opts.values():
            set_grads(o, std)
        gpu, host = {n: [] for n in opts}, {n: [] for n in opts}
        for i in range(warmup + rounds):
            for n, o in opts.items():
                a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record(); t0 = time.perf_counter(); r = o.step(); t1 = time.perf_counter(); b.record()
                torch.cuda.synchronize()
                assert int(r) == 1, f"{n}: step() skipped"
                if i >= warmup:
                    gpu[n].append(a.elapsed_time(b)); host[n].append(1e3 * (t1 - t0))
        say(f"{label}: gradient norm {float(opts['host-sync'].last_grad_norm):.4g} (host-sync) {float(opts['device'].last_grad_norm):.4g} (device)")
        for n in opts:
            say(f"  {n:10s} to GPU idle {_median(gpu[n]):7.3f} ms (min {min(gpu[n]):7.3f} .. max {max(gpu[n]):7.3f})   "
                f"host time of step() {_median(host[n]):7.3f} ms (min {min(host[n]):7.3f} .. max {max(host[n]):7.3f})")
    say("  (the same gradient tensors every step: the device mode uploads no pointer table; the host-sync mode uploads it every step)")


def device_scaler_c5(dev, pairs, steps, warmup, say):
    """the C5 training step as bench.py --workload train builds it, once per optimizer mode, in alternating pairs"""
    from daspeech_amd.criterions import s2s_dag_fastspeech2_loss
    from daspeech_amd.models.daspeech import S2SConformerDAGFastSpeech2Model
    from daspeech_amd.synthetic import calibrate_synthetic_weights, make_s2st_batch
    legs = {}
    for name, mode in (("host-sync", False), ("device", True)):
        torch.manual_seed(1234)
        model = calibrate_synthetic_weights(S2SConformerDAGFastSpeech2Model()).to(dev).half().train()
        hb = [F.half_sample(make_s2st_batch(32, dev, seed=i)) for i in range(2)]
        opt = F.FP16FlatOptimizer(model.parameters(), lr=1e-4, betas=(0.9, 0.999), weight_decay=0.01, clip_norm=1.0, init_scale=2.0 ** 7,
                                  hip_step=True, device_scaler=mode)

        def step(i, model=model, hb=hb, opt=opt):
            opt.zero_grad()
            loss, _ = s2s_dag_fastspeech2_loss(model, hb[i % len(hb)], glat_p="0.5:0.1@200k", update_num=100000 + i)
            opt.backward(loss)
            opt.step()
        legs[name] = step
    for fn in legs.values():
        for i in range(warmup):
            fn(i)
    ms = {n: [] for n in legs}
    for _ in range(pairs):
        for n, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(steps):
                fn(i)
            torch.cuda.synchronize()
            ms[n].append(1e3 * (time.perf_counter() - t0) / steps)
    say(f"C5 training step (B 32, fp16 model), {pairs} alternating pairs of {steps} steps after {warmup} warm-up steps each, host-sync first, ms per step:")
    for n, v in ms.items():
        say(f"  {n:10s} " + " / ".join(f"{x:.2f}" for x in v) + f"   median {_median(v):.2f}, {max(v) - min(v):.2f} apart")
    d = _median(ms["device"]) - _median(ms["host-sync"])
    spread = max(ms["host-sync"]) - min(ms["host-sync"])
    say(f"  device - host-sync at the medians: {d:+.2f} ms; the host-sync runs are {spread:.2f} ms apart: "
        + ("inside the host-sync mode's own spread" if abs(d) <= spread else "beyond the host-sync mode's own spread"))


def main():
    if "--device-scaler" in sys.argv:
        rounds, warmup = max(20, _opt("--rounds", 100)), _opt("--warmup", 10)
        out_path = _opt("--out", os.path.join(ROOT, "profiles", "fp16_optim_device_scaler.txt"), str)
        lines = []

        def say(t):
            print(t, flush=True)
            lines.append(t)

        dev = torch.device("cuda:0")
        sizes = released_sizes()
        say(f"released parameter list: {len(sizes)} trainable tensors, {sum(sizes)} elements; device {torch.cuda.get_device_name(0)}; "
            f"median (min .. max) of {rounds} alternations after {warmup} warm-up rounds")
        device_scaler_site(sizes, dev, rounds, warmup, say)
        device_scaler_c5(dev, _opt("--pairs", 5), _opt("--steps", 20), warmup, say)
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            fh.write("\n".join(lines) + "\n")
        print(f"written: {out_path}")
        return
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
