"""CPU-side checks of the helpers the training operators' raising functions share (decode_ops._settled): a layout reason is settled by a dense
copy of the data tensors and asked about once more, every other reason raises under the operator's name, and the dropout probability is
checked AFTER the copy — a strided input does not get a bad p past the check and on to the generator."""
import pytest
import torch


def _problem(h, tag):
    """a stand-in for a _..._problem() function: a layout reason for a tensor that is not contiguous, another reason for tag 'bad'"""
    from daspeech_amd import decode_ops
    if tag == "bad":
        return "tag is not served"
    if not h.is_contiguous():
        return decode_ops._LAYOUT + ": h needs unit column stride"
    return None


def test_a_layout_reason_is_settled_by_a_dense_copy_and_anything_else_raises():
    from daspeech_amd import decode_ops
    dense, strided = torch.arange(24.0).reshape(4, 6), torch.arange(48.0).reshape(4, 12)[:, ::2]
    h, tag = decode_ops._settled("op", _problem, (dense, "ok"), 1, 0.1)
    assert h is dense and tag == "ok"                                           # nothing in the way: the arguments themselves
    h, tag = decode_ops._settled("op", _problem, (strided, "ok"), 1, 0.0)
    assert h is not strided and h.is_contiguous() and torch.equal(h, strided) and tag == "ok"
    with pytest.raises(RuntimeError, match="^op: tag is not served$"):
        decode_ops._settled("op", _problem, (dense, "bad"), 1)
    with pytest.raises(RuntimeError, match="^op: tag is not served$"):          # the reason left after the copy, not the layout one
        decode_ops._settled("op", lambda h, tag: _problem(h, "ok" if not h.is_contiguous() else tag), (strided, "bad"), 1)
    with pytest.raises(RuntimeError, match="^op: layout"):                      # a copy that does not settle it: asked once more, then raised
        decode_ops._settled("op", lambda h, tag: decode_ops._LAYOUT + ": never", (strided, "ok"), 1)


@pytest.mark.parametrize("p", [1.0, 1.5, -0.1])
def test_a_bad_dropout_probability_raises_with_and_without_a_layout_problem(p):
    from daspeech_amd import decode_ops
    dense, strided = torch.arange(24.0).reshape(4, 6), torch.arange(48.0).reshape(4, 12)[:, ::2]
    for h in (dense, strided):
        with pytest.raises(RuntimeError, match=r"^op: dropout probability has to be in \[0, 1\)"):
            decode_ops._settled("op", _problem, (h, "ok"), 1, p)
    with pytest.raises(RuntimeError, match="^op: tag is not served$"):          # the problem's own reason comes first
        decode_ops._settled("op", _problem, (dense, "bad"), 1, p)
