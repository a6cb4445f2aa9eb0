"""The row of the multi-head attention training operator in the view contract of tests/test_gpu_views.py: q, k, v, the mask and
the incoming gradient through every layout of util_views.every_variant, one at a time, then all at once.  The row uses that module's own
machinery (sweep, same_bits, expanded_gradients) and registers the operator's public names in its table, so that
test_every_public_operator_has_a_row finds them: the module is imported here as pytest itself imports it (tests/ is no package; its
directory is on sys.path during a run), so the table filled is the table read."""
import pytest
import torch

import test_gpu_views as TV
from tests import util_mha_train_ref as A
from tests.util_4x_rule import check_4x

pytestmark = pytest.mark.gpu


@TV.covers("mha_attention_autograd", "mha_attention_autograd_served", "mha_attention_checked", "set_mha_attention_hip")
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["float16", "bfloat16"])
def test_mha_attention_autograd(dtype):
    """q, k, v, the mask and the incoming gradient in every layout, p = 0, N = 33 queries on M = 40 keys (a wave's 32 rows and one, a tile and a
    part), B = 3, H = 2: the public operator reads a column slice with its row stride and copies what the kernels do not take (bits of the fresh
    call, which holds the 4 x rule against the modules' torch lines in float64); the predicate decides between `checked` and the torch lines as
    _MHA and _SelfAttention do; with the switch off it says no"""
    d = TV.D()
    N, M, B, H = 33, 40, 3, 2
    t = A.inputs(1000 * N + 10 * M + B + H, B, N, M, H)
    args = {n: TV.cu(v, dtype) for n, v in t.items()}
    args["pad"] = TV.cu(A.pad_masks("ragged", B, M))
    names = ("o", "dq", "dk", "dv")
    ins = ("q", "k", "v")

    def lines(a, dt):
        x = [TV.leaf(a[n].to(dt).contiguous()) for n in ins]
        o = A.module_lines(*x, a["pad"].contiguous(), H)[0]
        return (o.detach(),) + tuple(TV._grads(o, x, a["do"].to(dt)))

    def op(a, ask):
        x = [TV.leaf(a[n]) for n in ins]
        if ask and not d.mha_attention_autograd_served(*x, a["pad"], H):
            return lines(a, dtype), False
        fn = d.mha_attention_checked if ask else d.mha_attention_autograd
        o = fn(*x, a["pad"], H, p=0.0, training=True)
        return (o.detach(),) + tuple(TV._grads(o, x, a["do"])), True
    ref = dict(zip(names, (TV.f64(x) for x in lines(args, torch.float64))))
    tor = dict(zip(names, lines(args, dtype)))
    base, _ = op(args, False)
    check_4x(f"views mha {dtype}", dict(zip(names, base)), tor, ref)
    TV.same_bits("checked", op(args, True)[0], base)
    vary = ins + ("pad", "do")
    TV.sweep(args, vary, lambda a: op(a, False)[0], base=base)
    TV.expanded_gradients(args, ("do",), lambda a: op(a, False)[0])
    hips = []

    def call(a):
        out, hip = op(a, True)
        hips.append(hip)
        return out
    TV.sweep(args, vary, call, lambda tag, out: check_4x(f"{tag} {dtype}", dict(zip(names, out)), tor, ref))
    assert any(hips) and not all(hips)
    # fp32 is not served by this operator (fp32 layers keep their torch lines): the predicate says no and the public operator keeps its
    # documented error
    a32 = [args[n].float() for n in ins]
    assert not d.mha_attention_autograd_served(*a32, args["pad"], H)
    with pytest.raises(RuntimeError, match="have to be fp16 or bf16, got torch.float32"):
        d.mha_attention_autograd(*a32, args["pad"], H)
    old = d.set_mha_attention_hip(False)
    try:
        assert old is True
        out, hip = op(args, True)
        assert not hip
        check_4x(f"off {dtype}", dict(zip(names, out)), tor, ref)
    finally:
        assert d.set_mha_attention_hip(old) is False
