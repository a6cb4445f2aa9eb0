"""The row of the stride-2 channels-last Conv1d training operator in the view contract of tests/test_gpu_views.py: x, the weight, the
bias and the incoming gradient through every layout of util_views.every_variant, one at a time, then all at once.  The row uses that module's
own machinery (sweep, same_bits, expanded_gradients) and registers the operator's public names in its table, so that
test_every_public_operator_has_a_row finds them: the module is imported here as pytest itself imports it (tests/ is no package; its
directory is on sys.path during a run), so the table filled is the table read."""
import pytest
import torch
from torch import nn

import test_gpu_views as TV
from tests import util_conv1d_stride2_ref as A
from tests.util_4x_rule import check_4x

pytestmark = pytest.mark.gpu


@TV.covers("conv1d_stride2_channels_last_autograd", "conv1d_stride2_channels_last_served", "conv1d_stride2_channels_last_sites_served",
           "conv1d_stride2_channels_last_checked", "set_conv1d_stride2_train_hip")
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["float16", "bfloat16"])
def test_conv1d_stride2_channels_last_autograd(dtype):
    """x, weight, bias and the incoming gradient in every layout, B 2, T 33 -> 17, 80 -> 128 channels, K 5: the public operator reads a pitched x or a
    column slice with its row stride and copies what the kernels do not take (bits of the fresh call, which holds the 4 x rule against the torch
    lines in float64); the two predicates decide between `checked` and the torch lines as the layers do; with the switch off both say no"""
    d = TV.D()
    B, T, Cin, Cout, K = 2, 33, 80, 128, 5
    t = A.inputs(5, B, T, Cin, Cout, K)
    args = {n: TV.cu(t[n], dtype) for n in ("x", "w", "bias", "dy")}
    names = ("y", "dx", "dw", "db")

    def lines(a, dt, device="cuda"):
        r = A.torch_lines(*(a[n].to(dt).to(device) for n in ("x", "w", "bias", "dy")))
        return tuple(r[n] for n in names)

    def op(a, ask):
        x, w, b = TV.leaf(a["x"]), TV.leaf(a["w"]), TV.leaf(a["bias"])
        if ask:
            conv = nn.Conv1d(Cin, Cout, K, stride=2, padding=(K - 1) // 2)
            conv.weight, conv.bias = nn.Parameter(a["w"]), nn.Parameter(a["bias"])        # a Parameter keeps the layout of its tensor
            ok = d.conv1d_stride2_channels_last_served(x, conv) if ask == "served" else d.conv1d_stride2_channels_last_sites_served(x, (conv,))
            if not ok:
                return lines(a, dtype), False
        fn = d.conv1d_stride2_channels_last_checked if ask else d.conv1d_stride2_channels_last_autograd
        y = fn(x, w, b)
        return (y.detach(),) + tuple(TV._grads(y, [x, w, b], a["dy"])), True
    ref = dict(zip(names, (TV.f64(v) for v in lines(args, torch.float64, "cpu"))))
    tor = dict(zip(names, lines(args, dtype)))
    base, _ = op(args, None)
    check_4x(f"views conv1d stride 2 {dtype}", dict(zip(names, base)), tor, ref)
    TV.same_bits("checked", op(args, "served")[0], base)
    vary = ("x", "w", "bias", "dy")
    TV.sweep(args, vary, lambda a: op(a, None)[0], base=base)
    TV.expanded_gradients(args, ("dy",), lambda a: op(a, None)[0])
    for ask in ("served", "sites"):
        hips = []

        def call(a):
            out, hip = op(a, ask)
            hips.append(hip)
            return out
        TV.sweep(args, vary, call, lambda tag, out: check_4x(f"{ask} {tag} {dtype}", dict(zip(names, out)), tor, ref))
        assert any(hips) and not all(hips), ask
    old = d.set_conv1d_stride2_train_hip(False)
    try:
        assert old is True
        for ask in ("served", "sites"):
            out, hip = op(args, ask)
            assert not hip
            # the torch lines ran: MIOpen's kernels do not repeat their bits from call to call, so they are held to the rule, not to `tor`
            check_4x(f"off {ask} {dtype}", dict(zip(names, out)), tor, ref)
    finally:
        assert d.set_conv1d_stride2_train_hip(old) is False
