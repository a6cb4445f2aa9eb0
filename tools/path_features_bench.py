#!/usr/bin/env python3
"""The argmax strategy's features_on_path site alone, and a training step of the argmax criterion.

Site (default): the torch lines of S2SDAGFastSpeech2Loss's argmax branch (clone, path[:, 0] = -1, mask, sum, stable argsort, the host read of
the widest count, lengths-to-mask, gather, masked_fill) against decode_ops.path_features_checked, forward and forward + backward, at the C5
shape (B 32, L 400, W 64, C 512, fp16) and a stress shape (L 1 024, W 256): HIP events around 50 calls, median (min, max) of 7 such blocks
after 20 calls of warm-up, microseconds per call, and the device activities of one call under torch.profiler.  On a checkout without the
operator only the torch lines are measured.

--step: the C5 batch of bench.py's train workload (make_s2st_batch, B 32, fp16 model and batch, FP16FlatOptimizer, dropout as released) with
S2SDAGFastSpeech2Loss(training_strategy="argmax") — forward + backward + optimizer, the criterion taken as the checkout has it —, one JSON
line with ms_per_step.  bench.py itself measures the `expect` strategy.

GPU box only; a plain tool, not a test.

usage: path_features_bench.py [--step] [--steps K] [--warmup W] [--batch B] [--out FILE]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = (("C5", 32, 400, 64, 512), ("stress", 32, 1024, 256, 512))


def _opt(name, default, conv=int):
    return conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def torch_lines(features, path):
    import torch
    with torch.no_grad():
        path = path.clone()
        path[:, 0] = -1
        features_mask = path >= 0
        n_on = features_mask.sum(-1)
        order = torch.argsort((~features_mask).to(torch.int8), dim=1, stable=True)[:, : int(n_on.max())]
        features_padding_mask = ~(torch.arange(order.shape[1], device=n_on.device).unsqueeze(0) < n_on.unsqueeze(1))
    out = features.gather(1, order.unsqueeze(-1).expand(-1, -1, features.shape[-1])).masked_fill(features_padding_mask.unsqueeze(-1), 0)
    return out, features_padding_mask


def _path(B, L, W, gen):
    """a path as the alignment gives it: vertex 0 on, then between W / 2 and W vertices in random places (the first sample: W), ranks as values"""
    import torch
    on = torch.zeros((B, L), dtype=torch.bool)
    on[:, 0] = True
    for b in range(B):
        k = W if b == 0 else int(torch.randint(W // 2, W + 1, (1,), generator=gen))
        on[b, 1 + torch.randperm(L - 1, generator=gen)[:k]] = True
    return torch.where(on, on.to(torch.int64).cumsum(1) - 1, torch.full((B, L), -1, dtype=torch.int64))


def site(out_path):
    import torch
    from daspeech_amd import decode_ops
    dev = torch.device("cuda:0")
    have_op = hasattr(decode_ops, "path_features_checked")
    lines = []
    for name, B, L, W, C in SHAPES:
        gen = torch.Generator().manual_seed(0)
        x = torch.randn((B, L, C), generator=gen).half().to(dev).requires_grad_(True)
        path = _path(B, L, W, gen).to(dev)
        dy = torch.randn((B, W, C), generator=gen).half().to(dev)
        legs = [("torch", lambda: torch_lines(x, path)[0])]
        if have_op:
            assert decode_ops.path_features_served(x, path, W)
            legs.append(("hip", lambda: decode_ops.path_features_checked(x, path, W)[0]))
            a, b = torch_lines(x, path), decode_ops.path_features_checked(x, path, W)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])

        def blocks(fn):
            for _ in range(20):
                fn()
            per = []
            for _ in range(7):
                a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                for _ in range(50):
                    fn()
                b.record()
                torch.cuda.synchronize()
                per.append(a.elapsed_time(b) * 1e3 / 50)
            return statistics.median(per), min(per), max(per)

        def activities(fn):
            from torch.profiler import ProfilerActivity, profile
            fn()
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)      # kernels, memsets and copies

        for which, fwd in legs:
            def both():
                x.grad = None
                fwd().backward(dy)
            f, fb = blocks(fwd), blocks(both)
            line = (f"path features {name:<6s} B={B} L={L} W={W} C={C} fp16 | {which:<6s} | fwd us median {f[0]:8.1f} (min {f[1]:.1f} max {f[2]:.1f}) | "
                    f"fwd+bwd us median {fb[0]:8.1f} (min {fb[1]:.1f} max {fb[2]:.1f}) | launches fwd {activities(fwd)} fwd+bwd {activities(both)}")
            print(line, flush=True)
            lines.append(line)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            fh.write("\n".join(lines) + "\n")


def step():
    import torch
    from daspeech_amd import decode_ops
    from daspeech_amd.criterions import S2SDAGFastSpeech2Loss
    from daspeech_amd.fp16_trainer import FP16FlatOptimizer, half_sample
    from daspeech_amd.models.daspeech import S2SConformerDAGFastSpeech2Model
    from daspeech_amd.synthetic import calibrate_synthetic_weights, make_s2st_batch
    steps, warmup, B = _opt("--steps", 40), _opt("--warmup", 10), _opt("--batch", 32)
    dev = torch.device("cuda:0")
    torch.manual_seed(1234)
    model = calibrate_synthetic_weights(S2SConformerDAGFastSpeech2Model()).to(dev)
    model.train()
    model.half()
    batches = [half_sample(make_s2st_batch(B, dev, seed=i)) for i in range(2)]
    opt = FP16FlatOptimizer(model.parameters(), lr=1e-4, betas=(0.9, 0.999), weight_decay=0.01, clip_norm=1.0, init_scale=2.0 ** 7)
    crit = S2SDAGFastSpeech2Loss(glat_p="0.5:0.1@200k", glance_strategy="number-random", tts_loss_weight=5.0, training_strategy="argmax")
    crit.train()
    loss = None

    def one(i):
        nonlocal loss
        opt.zero_grad()
        s = dict(batches[i % len(batches)])
        s["update_num"] = 100000 + i
        loss, _, _ = crit(model, s)
        opt.backward(loss)
        opt.step()
    for i in range(warmup):
        one(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(warmup, warmup + steps):
        one(i)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    print(json.dumps({"workload": "C5 training step, argmax strategy: forward + backward + optimizer, fp16 model", "ms_per_step": ms,
                      "utt_per_s": B * 1e3 / ms, "steps": steps, "warmup": warmup, "batch": B, "loss": float(loss),
                      "path_features_operator": bool(getattr(decode_ops, "PATH_FEATURES_HIP", False)),
                      "peak_memory_GB": torch.cuda.max_memory_allocated() / 2 ** 30}), flush=True)


if __name__ == "__main__":
    if "--step" in sys.argv:
        step()
    else:
        site(_opt("--out", None, str))
