#!/usr/bin/env python3
"""The glancing step alone at the DAG benchmark's shape: the torch formulation (decode_ops.set_glance_hip(False) — what the criteria ran
before csrc/glance.hip) against the HIP ops, alternating in one process on the same tensors, HIP events around each leg, warm-up then
median / min / max over the alternations.  Three segments:
  force-emit forward    from the gather's [B,T,L] output (fp32 view, rows pitched to 4) to the tensor dag_loss launches on — for the torch
                        formulation that includes the copy into a pitched buffer that dag_loss makes when L is no multiple of 4
  force-emit backward   from dag_loss's grad_match (pitched) to the gradient the gather's backward receives
  reveal selection      decode_ops.glance_select (oracle tokens, count of right vertices, number-random threshold, reveal, glanced
                        tokens) — glat_function without its arg-max, gather, alignment and emission mask, which are the same code on both sides
Results are compared with torch.equal at the timed size.  GPU box only; a plain tool, not a test.  The table is printed and written.

usage: glance_bench.py [--batch B] [--tgt-len T] [--graph-len L [L ...]] [--rounds N] [--warmup N] [--out FILE]
default: B 32, T 512, L 4096 and 4095 (C2 and a graph length off the 4 grid); default file: profiles/glance_bench.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import importlib                                               # noqa: E402
import torch                                                   # noqa: E402
from daspeech_amd import decode_ops                            # noqa: E402

dl = importlib.import_module("daspeech_amd.custom_ops.dag_loss")      # (the package attribute of that name is the operator)


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


def _time(fn):
    a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
    a.record(); r = fn(); b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), r


def alternate(legs, rounds, warmup):
    """legs: {name: fn}; -> {name: (median, min, max)} over `rounds` alternations after `warmup` untimed ones"""
    ts = {n: [] for n in legs}
    for i in range(warmup + rounds):
        for n, fn in legs.items():
            t, _ = _time(fn)
            if i >= warmup:
                ts[n].append(t)
    return {n: (sorted(v)[len(v) // 2], min(v), max(v)) for n, v in ts.items()}


def with_switch(on, fn):
    def run():
        old = decode_ops.set_glance_hip(on)
        try:
            return fn()
        finally:
            decode_ops.set_glance_hip(old)
    return run


def main():
    B, T, rounds, warmup = _opt("--batch", 32), _opt("--tgt-len", 512), _opt("--rounds", 20), _opt("--warmup", 3)
    Ls = _opts("--graph-len", [4096, 4095])
    out_path = _opt("--out", os.path.join(ROOT, "profiles", "glance_bench.txt"), str)
    dev = torch.device("cuda:0")
    lines = []

    def say(t):
        print(t, flush=True)
        lines.append(t)

    say(f"glancing step alone, B {B} T {T}; device {torch.cuda.get_device_name(0)}; median (min .. max) of {rounds} alternations torch / HIP "
        f"after {warmup} warm-up rounds, HIP events")
    for L in Ls:
        gen = torch.Generator(device=dev).manual_seed(L)
        V = 8192
        tgt = torch.randint(4, V, (B, T), device=dev, generator=gen)
        n_tgt = torch.full((B,), T, dtype=torch.long, device=dev)
        path = torch.full((B, L), -1, dtype=torch.long, device=dev)
        for b in range(B):                                      # a valid alignment: T vertices in order
            pos = torch.randperm(L, device=dev, generator=gen)[:T].sort().values
            path[b, pos] = torch.arange(T, device=dev)
        oracle = tgt.gather(-1, path.clip(min=0))
        guess = torch.where(torch.rand(B, L, device=dev, generator=gen) < 0.5, oracle, oracle + 1)
        prev = torch.randint(0, 4, (B, L), device=dev, generator=gen)
        noise = torch.randn(B, L, device=dev, generator=gen)
        unif = torch.rand(B, L, device=dev, generator=gen)

        def select():
            return decode_ops.glance_select(tgt, path, guess, prev, n_tgt, 0.5, "number-random", noise=noise, unif=unif)
        sel_t, sel_h = with_switch(False, select)(), with_switch(True, select)()
        same_sel = all(torch.equal(sel_t[k], sel_h[k]) for k in sel_t)
        revealed = sel_h["revealed"]
        matchmask = decode_ops.emission_mask(path, T)

        match = dl._pitched_empty(B, T, L, dev)
        match.copy_(torch.randn(B, T, L, device=dev, generator=gen) * 2 - 5)
        match = match.detach().requires_grad_()
        grad = dl._pitched_empty(B, T, L, dev)
        grad.copy_(torch.randn(B, T, L, device=dev, generator=gen))

        def fwd_torch():                                        # the criterion's expression, then dag_loss's own layout step
            glat_prev_mask = revealed.unsqueeze(1)
            out = match.masked_fill(glat_prev_mask, 0) + match.masked_fill(~matchmask, float("-inf")).masked_fill(~glat_prev_mask, 0).detach()
            return out, dl._as_pitched(out)[0]

        def fwd_hip():
            out = decode_ops.force_emit(match, path, revealed)
            return out, dl._as_pitched(out)[0]
        assert decode_ops.force_emit_served(match, path, revealed)
        (o_t, p_t), (o_h, p_h) = fwd_torch(), fwd_hip()
        same_fwd = torch.equal(o_t, o_h) and torch.equal(p_t, p_h) and p_h.data_ptr() == o_h.data_ptr()
        g_t, = torch.autograd.grad(o_t, match, grad, retain_graph=True)
        g_h, = torch.autograd.grad(o_h, match, grad, retain_graph=True)
        same_bwd = torch.equal(g_t, g_h)

        nbytes = B * T * L * 4
        say(f"L {L}: one [B,T,L] fp32 tensor = {nbytes / 2 ** 20:.0f} MiB; results torch.equal: select {same_sel}, forward {same_fwd}, backward {same_bwd}")
        res = alternate({"torch": fwd_torch, "hip": fwd_hip}, rounds, warmup)
        for n in ("torch", "hip"):
            say("  force-emit forward   %-6s %8.3f ms (%8.3f .. %8.3f)" % (n, *res[n]))
        say(f"    (the HIP pass reads and writes {nbytes / 2 ** 20:.0f} MiB once each: {2 * nbytes / res['hip'][0] / 1e9:.2f} TB/s at the median)")
        res = alternate({"torch": lambda: torch.autograd.grad(o_t, match, grad, retain_graph=True),
                         "hip": lambda: torch.autograd.grad(o_h, match, grad, retain_graph=True)}, rounds, warmup)
        for n in ("torch", "hip"):
            say("  force-emit backward  %-6s %8.3f ms (%8.3f .. %8.3f)" % (n, *res[n]))
        say(f"    (the HIP pass: {2 * nbytes / res['hip'][0] / 1e9:.2f} TB/s at the median)")
        res = alternate({"torch": with_switch(False, select), "hip": with_switch(True, select)}, rounds, warmup)
        for n in ("torch", "hip"):
            say("  reveal selection     %-6s %8.3f ms (%8.3f .. %8.3f)" % (n, *res[n]))
        del o_t, p_t, o_h, p_h, g_t, g_h, match, grad, matchmask
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(f"written: {out_path}")


if __name__ == "__main__":
    main()
