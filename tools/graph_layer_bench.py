#!/usr/bin/env python3
"""Forward + backward of ONE layer of the C5 training step — eager against a captured graph (torch.cuda.graph) that is replayed — per layer
type, at the step's sizes: ConformerLayer 512 / 2048 / 8 heads / K 31 at T = 200, NATDecoderLayer 512 / 2048 / 8 heads at L = 400 (encoder
memory T = 200), FFTLayer 256 / 4 heads / 1024 / K 9 at F = 330; B = 32, fp16, training mode, ragged padding masks, the released dropout
rates (0.1 everywhere).  Three variants, same process, same tensors:

  (a) eager            the layer as the step calls it: the HIP training operators, (seed, offset) reserved on the host per masked call
  (b) graph, draws()   captured inside decode_ops.DropoutState.draws() and replayed: the same HIP operators drawing from the state on the
                       device, new masks every replay, no host work between replays
  (c) graph, torch     captured WITHOUT a draws() scope and replayed: a masked call under capture is not served, the layer's torch lines run
                       — what a captured layer was before the state lived on the device

Per variant: wall time per iteration (perf_counter around call + synchronize) and GPU time by events, median of 40 iterations after 10; the
three variants are timed in turn and the whole turn is REPEATED (default 3 rounds), so every variant has a spread over its own repeated runs
(max - min of its round medians).  The comparison that matters is (b) against (a) in wall time, read next to the spread of (a): by the
rule of DESIGN.md a difference counts when it is more than three times that spread.  Differences are printed as (b) minus the other variant
(negative: (b) is faster).  Every iteration is synchronised, so "wall" is GPU time plus a constant — what a graph saves in host issue time of
an unsynchronised step is not what this tool measures.  GPU box only; a plain tool, not a test.  The table is
printed and written.

usage: graph_layer_bench.py [--batch B] [--iters N] [--warmup N] [--rounds N] [--out FILE]      default file: profiles/graph_dropout.txt"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                                                   # noqa: E402
from daspeech_amd import decode_ops                            # noqa: E402


def _opt(name, default, conv=int):
    return conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def _pad(B, T, gen):
    lens = torch.randint(int(0.6 * T), T + 1, (B,), generator=gen)
    lens[0] = T
    return (torch.arange(T).unsqueeze(0) >= lens.unsqueeze(1)).cuda()


def layers(B, dtype):
    """name -> (module, leaves, call)"""
    from daspeech_amd.models.daspeech import ConformerLayer, NATDecoderLayer, rel_positional_encoding
    from daspeech_amd.models.fastspeech2 import FFTLayer
    g = torch.Generator().manual_seed(7)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dtype).cuda().requires_grad_()      # noqa: E731
    out = {}
    conf = ConformerLayer(512, 2048, 8, 31, 0.1).to(device="cuda", dtype=dtype).train()
    x, pad = rnd(B, 200, 512), _pad(B, 200, g)
    pos = rel_positional_encoding(200, 512, x.device, dtype)
    out["ConformerLayer 512/2048/8/K31 T=200"] = (conf, [x], lambda x=x, pad=pad: conf(x, pos, pad))
    nat = NATDecoderLayer(512, 2048, 8, 512, 0.1, 0.1, 0.1).to(device="cuda", dtype=dtype).train()
    y, enc, ypad, epad = rnd(B, 400, 512), rnd(B, 200, 512), _pad(B, 400, g), _pad(B, 200, g)
    out["NATDecoderLayer 512/2048/8 L=400"] = (nat, [y, enc], lambda: nat(y, ypad, enc, epad))
    fft = FFTLayer(256, 4, 1024, 9, 0.1, 0.1).to(device="cuda", dtype=dtype).train()
    f, fpad = rnd(B, 330, 256), _pad(B, 330, g)
    out["FFTLayer 256/4/1024/K9 F=330"] = (fft, [f], lambda: fft(f, fpad))
    return out


def capture(step, state):
    """step captured after two warm-up calls on a side stream; inside state.draws() when a state is given"""
    def once():
        if state is None:
            return step()
        with state.draws():
            return step()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            once()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    launched, launch = [], decode_ops._launch
    decode_ops._launch = lambda dev, entry, *a: (launched.append(entry.__name__), launch(dev, entry, *a))[1]
    try:
        with torch.cuda.graph(g):
            once()
    finally:
        decode_ops._launch = launch
    return g, launched


def timed(fn, iters, warmup):
    """(median wall ms per iteration, median GPU ms by events)"""
    wall, gpu = [], []
    for i in range(warmup + iters):
        a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            wall.append((time.perf_counter() - t0) * 1e3); gpu.append(a.elapsed_time(b))
    med = lambda t: sorted(t)[len(t) // 2]                     # noqa: E731
    return med(wall), med(gpu)


def main():
    B, iters, warmup, rounds = _opt("--batch", 32), _opt("--iters", 40), _opt("--warmup", 10), _opt("--rounds", 3)
    path = _opt("--out", os.path.join(ROOT, "profiles", "graph_dropout.txt"), str)
    torch.manual_seed(1234)
    lines = [f"graph_layer_bench: forward + backward of one layer, B = {B}, fp16, training mode, dropout 0.1, {torch.cuda.get_device_name(0)}",
             f"median of {iters} iterations after {warmup}, {rounds} rounds in turn; ms: wall (call + synchronize) / GPU (events); "
             "spread = max - min of a variant's round medians",
             "(a) eager   (b) graph captured inside DropoutState.draws(), replayed   (c) graph captured without a scope (torch lines), replayed",
             "differences are (b) minus the other variant: negative = (b) is faster.  Every iteration is synchronised, so wall is GPU time plus a "
             "constant: the host issue time of an unsynchronised step is NOT measured here", ""]
    for name, (layer, leaves, call) in layers(B, torch.float16).items():
        leaves = leaves + list(layer.parameters())
        go = torch.randn_like(call())

        def step():
            return torch.autograd.grad(call(), leaves, go)
        state = decode_ops.DropoutState("cuda")
        gb, lb = capture(step, state)
        gc, lc = capture(step, None)
        nb = sum(e.endswith("_state") for e in lb)
        variants = (("a", step), ("b", gb.replay), ("c", gc.replay))
        res = {k: [] for k, _ in variants}
        for _ in range(rounds):
            for k, fn in variants:
                res[k].append(timed(fn, iters, warmup))
        lines.append(f"{name}   [(b) recorded {nb} launches of the ..._state entries and {len(lb)} HIP-operator launches in all; (c) {len(lc)}, "
                     f"{sum(e.endswith('_state') for e in lc)} of them ..._state]")
        stat = {}
        for k, _ in variants:
            w, g = sorted(r[0] for r in res[k]), sorted(r[1] for r in res[k])
            stat[k] = (w[len(w) // 2], w[-1] - w[0], g[len(g) // 2], g[-1] - g[0])
            lines.append(f"  ({k})  wall {stat[k][0]:8.3f} ms (spread {stat[k][1]:.3f})   GPU {stat[k][2]:8.3f} ms (spread {stat[k][3]:.3f})   "
                         f"rounds wall {' '.join(f'{r[0]:.3f}' for r in res[k])}")
        d, s = stat["b"][0] - stat["a"][0], stat["a"][1]             # every difference below is (b) minus the other: negative = (b) is faster
        lines.append(f"  (b) - (a), wall: {d:+.3f} ms ((b) / (a) = {stat['b'][0] / stat['a'][0]:.2f}), {abs(d) / s if s > 0 else float('inf'):.1f} x the spread "
                     f"of (a): {'beyond' if abs(d) > 3 * s else 'inside'} three times that spread;  (b) - (c), wall: {stat['b'][0] - stat['c'][0]:+.3f} ms, "
                     f"GPU: {stat['b'][2] - stat['c'][2]:+.3f} ms")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
