"""The row of the bias + activation + dropout operator in the view contract of tests/test_gpu_views.py: h, the bias and the
incoming gradient through every layout of util_views.every_variant, one at a time, then all at once.  The row uses that module's own
machinery (sweep, same_bits, expanded_gradients) and registers the operator's public names in its table, so that
test_every_public_operator_has_a_row finds them: the module is imported here as pytest itself imports it (tests/ is no package; its
directory is on sys.path during a run), so the table filled is the table read."""
import pytest
import torch

import test_gpu_views as TV
from tests import util_actdrop_ref as A
from tests.util_4x_rule import check_4x

pytestmark = pytest.mark.gpu


@TV.covers("bias_act_dropout_autograd", "bias_act_dropout_served", "bias_act_dropout_sites_served", "bias_act_dropout_checked", "set_act_dropout_hip")
@pytest.mark.parametrize("act", ["silu", "glu"])
@pytest.mark.parametrize("dtype", TV.TRAIN_DTYPES, ids=TV.TRAIN_IDS)
def test_bias_act_dropout_autograd(dtype, act):
    """h, the bias and the incoming gradient in every layout, p = 0, R = 33 (a chunk and one row), Cin = 144 (a ragged number of 16-byte
    groups per wave): the public operator serves a pitched h with its pitch and copies what the kernels do not take (bits of the fresh call,
    which holds the 4 x rule against the torch lines in float64); the two predicates decide between `checked` and the torch lines as the
    layers do; with the switch off both say no"""
    d = TV.D()
    R, Cin = 33, 144
    h, bias, dy = A.inputs(5, R, Cin, act)
    args = dict(h=TV.cu(h, dtype), bias=TV.cu(bias, dtype), dy=TV.cu(dy, dtype))
    names = ("y", "dh", "dbias")

    def lines(a, dt):
        x, b = TV.leaf(a["h"].to(dt)), TV.leaf(a["bias"].to(dt))
        y = A.torch_lines(x, b, act)
        return (y.detach(),) + tuple(TV._grads(y, [x, b], a["dy"].to(dt)))

    def op(a, ask):
        x, b = TV.leaf(a["h"]), TV.leaf(a["bias"])
        if ask == "served" and not d.bias_act_dropout_served(x, b, act):
            return lines(a, dtype), False
        if ask == "sites" and not d.bias_act_dropout_sites_served(x, ((Cin, b, act),)):      # asked of the layer input; `checked` copies a view
            return lines(a, dtype), False
        fn = d.bias_act_dropout_checked if ask else d.bias_act_dropout_autograd
        y = fn(x, b, act, 0.0, True)
        return (y.detach(),) + tuple(TV._grads(y, [x, b], a["dy"])), True
    ref = dict(zip(names, (TV.f64(x) for x in lines(args, torch.float64))))
    tor = dict(zip(names, lines(args, dtype)))
    base, _ = op(args, None)
    check_4x(f"views actdrop {act} {dtype}", dict(zip(names, base)), tor, ref)
    TV.same_bits("checked", op(args, "served")[0], base)
    vary = ("h", "bias", "dy")
    TV.sweep(args, vary, lambda a: op(a, None)[0], base=base)
    TV.expanded_gradients(args, ("dy",), lambda a: op(a, None)[0])
    for ask in ("served", "sites"):
        hips = []

        def call(a):
            out, hip = op(a, ask)
            hips.append(hip)
            return out
        TV.sweep(args, vary, call, lambda tag, out: check_4x(f"{ask} {tag} {act} {dtype}", dict(zip(names, out)), tor, ref))
        assert any(hips) and not all(hips), ask
    old = d.set_act_dropout_hip(False)
    try:
        assert old is True
        for ask in ("served", "sites"):
            out, hip = op(args, ask)
            assert not hip
            TV.same_bits(f"off {ask}", out, tuple(tor[n] for n in names))
    finally:
        assert d.set_act_dropout_hip(old) is False
