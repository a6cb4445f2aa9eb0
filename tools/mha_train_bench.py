#!/usr/bin/env python3
"""Forward and forward + backward of the multi-head attention sites of a C5 training step alone — between the q / k / v projections and
out_proj — at the shapes the step produces: the torch lines of the training branches of _MHA / _SelfAttention (three view().transpose()
reshapes, the zeros + masked_fill additive mask, F.scaled_dot_product_attention with dropout, the transpose(1, 2).reshape copy; autograd
backward) against decode_ops.mha_attention_autograd — same process, same tensors, the two legs INTERLEAVED round by round.  Per leg: GPU time
by HIP events and host time (perf_counter around the calls, no sync inside), warm-up then median and the 10 % .. 90 % spread.

The shapes are FOUND, not assumed: one loss evaluation of the C5 model (fp16, synthetic.make_s2st_batch(32), as bench.py --workload train
builds it) with the operator's entry counted gives every (B, N, M, H) the step calls it with; they fall into four classes — decoder
self-attention (H 8, N = M), decoder encoder-attention (H 8, N != M), FFT encoder and FFT decoder (H 4; the decoder runs over mel frames and
is the longer one) — and each class is timed at the shape it has in that batch.  GPU box only; a plain tool, not a test.  The table is
printed and written.

usage: mha_train_bench.py [--batch B] [--iters N] [--warmup N] [--out FILE]
default: B 32, fp16, p 0.1, ragged masks; default file: profiles/mha_train_bench.txt"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                                                   # noqa: E402
import torch.nn.functional as F                                # noqa: E402
from daspeech_amd import decode_ops                            # noqa: E402


def _opt(name, default, conv=int):
    return conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def one(fn):
    """(GPU ms by events, host ms until the last call returned)"""
    a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record(); fn(); b.record()
    host = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    return a.elapsed_time(b), host


def interleaved(fns, iters, warmup):
    """every leg once per round, in turn -> per leg ((median, 10 %, 90 %) GPU ms, the same for host ms)"""
    ts = [([], []) for _ in fns]
    for i in range(warmup + iters):
        for k, fn in enumerate(fns):
            g, h = one(fn)
            if i >= warmup:
                ts[k][0].append(g); ts[k][1].append(h)
    stat = lambda t: (sorted(t)[len(t) // 2], sorted(t)[len(t) // 10], sorted(t)[(9 * len(t)) // 10])
    return [(stat(g), stat(h)) for g, h in ts]


def step_shapes(B, dev):
    """{(B, N, M, H): calls} of one loss evaluation of the C5 model on make_s2st_batch(B), and the valid key counts per sample of each shape"""
    from daspeech_amd.criterions import s2s_dag_fastspeech2_loss
    from daspeech_amd.fp16_trainer import half_sample
    from daspeech_amd.models.daspeech import S2SConformerDAGFastSpeech2Model
    from daspeech_amd.synthetic import calibrate_synthetic_weights, make_s2st_batch
    torch.manual_seed(1234)
    model = calibrate_synthetic_weights(S2SConformerDAGFastSpeech2Model()).to(dev).half().train()
    batch = half_sample(make_s2st_batch(B, dev, seed=0))
    seen, lens = {}, {}
    real = decode_ops.mha_attention_checked

    def counted(q, k, v, pad_mask, heads, **kw):
        key = (q.shape[0], q.shape[1], k.shape[1], heads)
        seen[key] = seen.get(key, 0) + 1
        if pad_mask is not None:
            lens[key] = (~pad_mask.bool()).sum(1)
        return real(q, k, v, pad_mask, heads, **kw)
    decode_ops.mha_attention_checked = counted
    try:
        loss, _ = s2s_dag_fastspeech2_loss(model, batch, glat_p="0.5:0.1@200k", update_num=100000)
        loss.backward()
        torch.cuda.synchronize()
    finally:
        decode_ops.mha_attention_checked = real
    del model
    torch.cuda.empty_cache()
    return seen, lens


def classes(seen):
    """the four shape classes, each at its most frequent (then longest) shape"""
    pick = lambda c: max(c, key=lambda s: (seen[s], s[1])) if c else None
    h8s = [s for s in seen if s[3] == 8 and s[1] == s[2]]
    h8x = [s for s in seen if s[3] == 8 and s[1] != s[2]]
    h4 = sorted((s for s in seen if s[3] == 4), key=lambda s: s[1])
    short = [s for s in h4 if s[1] == h4[0][1]] if h4 else []
    long_ = [s for s in h4 if s[1] == h4[-1][1]] if len(h4) > 1 else []
    return [("decoder self-attention", pick(h8s)), ("decoder encoder-attention", pick(h8x)), ("FFT encoder", pick(short)), ("FFT decoder (mel frames)", pick(long_))]


def main():
    B = _opt("--batch", 32)
    iters, warmup = _opt("--iters", 200), _opt("--warmup", 20)
    out_path = _opt("--out", os.path.join(ROOT, "profiles", "mha_train_bench.txt"), str)
    dev, dtype, p = torch.device("cuda:0"), torch.float16, 0.1
    lines = []

    def say(t):
        print(t, flush=True)
        lines.append(t)

    say(f"multi-head attention sites of a C5 training step alone, B {B} fp16 p {p}, ragged masks; device {torch.cuda.get_device_name(0)}; median "
        f"(10 % .. 90 %) of {iters} rounds after {warmup} warm-up, legs interleaved; backward: gradients of q, k, v")
    seen, lens = step_shapes(B, dev)
    say("shapes of one loss evaluation (forward + backward) of the C5 model on synthetic.make_s2st_batch(%d), (B, N, M, H): calls of the operator" % B)
    for s in sorted(seen, key=lambda s: (-s[3], s[1], s[2])):
        say(f"    {s}: {seen[s]}")
    fmt = lambda m: f"{m[0]:7.3f} ({m[1]:.3f} .. {m[2]:.3f})"
    for name, shape in classes(seen):
        if shape is None:
            say(f"{name}: no such call in the step")
            continue
        Bn, N, M, H = shape
        C = H * 64
        gen = torch.Generator(device=dev).manual_seed(0)
        rnd = lambda *s: torch.randn(s, device=dev, generator=gen).to(dtype)
        q = rnd(Bn, N, C).requires_grad_()
        k, v = rnd(Bn, M, C).requires_grad_(), rnd(Bn, M, C).requires_grad_()
        if shape in lens:
            kl = lens[shape].to(dev)
        else:
            kl = torch.randint(max(1, M // 2), M + 1, (Bn,), device=dev, generator=gen)
            kl[0] = M
        pad = torch.arange(M, device=dev).unsqueeze(0) >= kl.unsqueeze(1)
        cot = rnd(Bn, N, C)
        wrt = [q, k, v]
        assert decode_ops.mha_attention_autograd_served(q, k, v, pad, H)

        def torch_lines():
            qh = q.view(Bn, N, H, 64).transpose(1, 2)
            kh = k.view(Bn, M, H, 64).transpose(1, 2)
            vh = v.view(Bn, M, H, 64).transpose(1, 2)
            mask = torch.zeros(Bn, 1, 1, M, dtype=dtype, device=dev).masked_fill(pad.view(Bn, 1, 1, M), float("-inf"))
            o = F.scaled_dot_product_attention(qh, kh, vh, attn_mask=mask, dropout_p=p)
            return o.transpose(1, 2).reshape(Bn, N, C)

        def hip_op():
            return decode_ops.mha_attention_autograd(q, k, v, pad, H, p=p, training=True)

        both = lambda fwd: torch.autograd.grad(fwd(), wrt, cot)
        (tf, hf) = interleaved([torch_lines, hip_op], iters, warmup)
        (tb, hb) = interleaved([lambda: both(torch_lines), lambda: both(hip_op)], iters, warmup)
        say(f"{name}: B {Bn} N {N} M {M} H {H}, valid keys {int(kl.min())} .. {int(kl.max())}, {seen[shape]} calls a step")
        say(f"    torch lines   forward GPU {fmt(tf[0])} ms host {fmt(tf[1])} ms   forward + backward GPU {fmt(tb[0])} ms host {fmt(tb[1])} ms")
        say(f"    HIP operator  forward GPU {fmt(hf[0])} ms host {fmt(hf[1])} ms   forward + backward GPU {fmt(hb[0])} ms host {fmt(hb[1])} ms"
            f"   ratio torch / HIP, forward + backward: GPU {tb[0][0] / hb[0][0]:.2f} host {tb[1][0] / hb[1][0]:.2f}")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(f"written: {out_path}")


if __name__ == "__main__":
    main()
