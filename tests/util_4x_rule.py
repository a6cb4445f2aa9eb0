"""The 4 x rule of the training operators' GPU tests (tests/test_gpu_resnorm_autograd.py states it): per tensor the figure is
max|got - ref| / max|ref| against the float64 reference; the HIP figure may be at most 4 x the figure of torch's own ops in the same dtype, and
where torch's figure is below one rounding of the tensor's dtype the bound is 4 x that rounding."""
import numpy as np
import torch

ROUND = {torch.float32: 2.0 ** -24, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}      # one rounding of the dtype


def f64(t):
    return t.detach().to(torch.float64).cpu().numpy()


def figure(got, ref, scale=None):
    """max|got - ref| / max|ref|; where the reference is zero throughout (dgamma / dbeta when y was not used) the absolute figure: the bound of
    check_4x then admits next to nothing but the zeros themselves"""
    sc = np.abs(ref).max() if scale is None else scale
    return float(np.abs(f64(got) - ref).max() / (sc if sc > 0 else 1.0))


def check_4x(tag, hip, tor, ref, scales=None):
    """the 4 x rule on every tensor of `ref`; prints both figures.  scales: max|ref| replaced for the named tensors (see its users)"""
    bad = []
    for name, r in ref.items():
        assert not np.isnan(f64(hip[name])).any(), f"{tag} {name}: NaN in the result (an element never written)"
        sc = (scales or {}).get(name)
        fh, ft = figure(hip[name], r, sc), figure(tor[name], r, sc)
        bound = 4.0 * max(ft, ROUND[hip[name].dtype])
        print(f"resnorm {tag} {name}: hip {fh:.3e} torch {ft:.3e} bound {bound:.3e}")
        if not fh <= bound:
            bad.append((name, fh, ft, bound))
    assert not bad, f"{tag}: figure above 4 x torch's (name, hip, torch, bound): {bad}"
