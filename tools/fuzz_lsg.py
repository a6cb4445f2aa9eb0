#!/usr/bin/env python3
"""Randomised parity sweep of dag_logsoftmax_gather_inplace (K1 forward + backward, eager and lazy state) against the fp64 oracle.
usage: fuzz_lsg.py [n_cases] [seed]   (GPU box only)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from oracle import dag_oracle as orc
from daspeech_amd import custom_ops as ops
n = int(sys.argv[1]) if len(sys.argv) > 1 else 60
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
dev = torch.device("cuda"); bad = 0
for case in range(n):
    B = int(rng.integers(1, 5)); L = int(rng.integers(1, 300)); T = int(rng.integers(1, 70))
    if rng.random() < 0.15: T = int(rng.integers(257, 601))                               # now and then past the first 256 gather slots
    V = int(rng.choice([int(rng.integers(2, 3000)), 8192, 512, 1000, 37, 4096, 6000, 10000]))
    dtype = [torch.float32, torch.float16, torch.bfloat16][int(rng.integers(0, 3))]
    scale = float(rng.choice([0.5, 3.0, 20.0]))
    lazy = case % 2 == 1                                                                  # backward state: stored softmax / row statistics
    per_row = (case // 2) % 2 == 1                                                        # targets of its own per vertex / one row expanded
    logits = torch.from_numpy((rng.standard_normal((B, L, V)) * scale).astype(np.float32)).to(dtype)
    tgt = rng.integers(0, V, (B, L, T) if per_row else (B, 1, T))
    if rng.random() < 0.5 and T > 3: tgt[..., T // 2:] = tgt[..., : T - T // 2]        # duplicate targets: the backward scatter must add
    tag = f"case {case}: B={B} L={L} V={V} T={T} {str(dtype)[6:]} scale={scale} {'lazy' if lazy else 'eager'} {'per-row' if per_row else 'expanded'} targets"
    prev = ops.set_lazy_softmax(lazy)
    try:
        lf = logits.float().numpy(); idx = np.ascontiguousarray(np.broadcast_to(tgt, (B, L, T)))
        ref, sm = orc.logsoftmax_gather(lf, idx, np.float64, want_softmax=True)
        x = logits.to(dev).requires_grad_(); work = x.clone(); tg = torch.from_numpy(tgt).to(dev)
        out_x, match = ops.dag_logsoftmax_gather_inplace(work, tg if per_row else tg.expand(-1, L, -1))
        np.testing.assert_allclose(match.detach().cpu().numpy(), ref, rtol=2e-6, atol=2e-6 * max(1.0, scale))
        eps = {torch.float32: 1e-6, torch.float16: 1e-3, torch.bfloat16: 8e-3}[dtype]
        held = out_x.detach().float().cpu().numpy()
        if lazy:
            assert np.array_equal(held, lf), "the lazy forward changed the logits"
            sm_dev = sm                                                                   # the backward recomputes the softmax from the logits
        else:
            sm_dev = held
            np.testing.assert_allclose(sm_dev, sm, rtol=eps, atol=eps * 0.1)
        w = rng.standard_normal((B, L, T)).astype(np.float32)
        (gx,) = torch.autograd.grad((match * torch.from_numpy(w).to(dev)).sum(), [x])
        gref = orc.logsoftmax_gather_bwd(sm_dev, idx, w, np.float64)
        np.testing.assert_allclose(gx.float().cpu().numpy(), gref, rtol=4 * eps, atol=4 * eps * max(1.0, float(np.abs(gref).max())))
    except Exception as e:       # noqa
        bad += 1
        print("FAIL", tag, "->", " | ".join(l.strip() for l in str(e).splitlines() if l.strip())[:300])
    finally:
        ops.set_lazy_softmax(prev)
print(f"{n} cases, {bad} failures")
