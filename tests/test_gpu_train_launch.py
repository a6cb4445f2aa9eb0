"""decode_ops._launch on its own — the one launch path of the training operators: the entry is called with the current raw stream of the
tensor's device as its last argument and that device current, the device that was current before is current again afterwards (also when the
entry raises), and a non-zero return code raises through _lib.check under the entry's name.  The entries here are Python functions: no
kernel of the project is launched."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _ops():
    from daspeech_amd import decode_ops
    return decode_ops


def test_entry_gets_its_arguments_and_the_current_raw_stream():
    seen = []

    def entry(*args):
        seen.append(args)
        return 0
    dev = torch.device("cuda", torch.cuda.current_device())
    before = torch.cuda.current_device()
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        assert _ops()._launch(dev, entry, 7, None, 2.5) is None
    assert _ops()._launch(torch.device("cuda"), entry, 1) is None               # no index: the current device
    assert seen[0] == (7, None, 2.5, s.cuda_stream)
    assert seen[1] == (1, torch.cuda.current_stream(before).cuda_stream) and seen[1][1] != s.cuda_stream
    assert torch.cuda.current_device() == before


def test_nonzero_return_code_raises_under_the_entrys_name():
    from daspeech_amd import _lib

    def dsp_made_up_entry(*args):
        return -22
    dev = torch.device("cuda", torch.cuda.current_device())
    before = torch.cuda.current_device()
    with pytest.raises(_lib.DaspeechHipError, match=r"dsp_made_up_entry failed \(rc=-22\)"):
        _ops()._launch(dev, dsp_made_up_entry, 1, 2)
    assert torch.cuda.current_device() == before


def test_check_is_reached_through_the_module(monkeypatch):
    calls = []
    monkeypatch.setattr(_ops()._lib, "check", lambda rc, what: calls.append((rc, what)))
    dev = torch.device("cuda", torch.cuda.current_device())
    _ops()._launch(dev, lambda *a: 0, 1)
    assert calls == []                                                          # only a non-zero code goes to _lib.check

    def named(*a):
        return 5
    _ops()._launch(dev, named, 1)
    assert calls == [(5, "named")]


def test_another_device_is_current_inside_and_the_previous_one_afterwards():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    torch.cuda.set_device(0)
    try:
        t = torch.zeros(1, device="cuda:1")
        inside = []

        def entry(*args):
            inside.append((torch.cuda.current_device(), args[-1]))
            return 0
        _ops()._launch(t.device, entry, 3)
        assert inside == [(1, torch.cuda.current_stream(1).cuda_stream)] and torch.cuda.current_device() == 0

        def raising(*args):
            assert torch.cuda.current_device() == 1
            raise ValueError("from the entry")
        with pytest.raises(ValueError, match="from the entry"):
            _ops()._launch(t.device, raising, 3)
        assert torch.cuda.current_device() == 0
    finally:
        torch.cuda.set_device(0)


def test_bad_p_with_a_strided_input_raises_before_the_generator_is_touched():
    """the public functions check p after the dense copy that settles a layout: a strided h (q, k, v) with p outside [0, 1) raises the
    RuntimeError of the dense case and reserves nothing from the generator"""
    D = _ops()
    torch.cuda.init()
    dev = torch.device("cuda", torch.cuda.current_device())
    gen = torch.cuda.default_generators[dev.index]
    before = gen.get_offset()
    h = torch.zeros(4, 128, dtype=torch.float16, device=dev)[:, ::2]
    assert D._actdrop_problem(h, None, "silu").startswith(D._LAYOUT) and D._actdrop_problem(h.contiguous(), None, "silu") is None
    q = torch.zeros(2, 5, 128, dtype=torch.float16, device=dev).transpose(0, 1)
    pos, u = torch.zeros(3, 128, dtype=torch.float16, device=dev), torch.zeros(2, 64, dtype=torch.float16, device=dev)
    assert D._relpos_train_problem(q, q, q, pos, u, u, None, 2).startswith(D._LAYOUT)
    for p in (1.0, 1.5):
        with pytest.raises(RuntimeError, match="bias_act_dropout_autograd: dropout probability"):
            D.bias_act_dropout_autograd(h, None, "silu", p=p, training=True)
        with pytest.raises(RuntimeError, match="relpos_attention_autograd: dropout probability"):
            D.relpos_attention_autograd(q, q, q, pos, u, u, None, 2, p=p, training=True)
    assert gen.get_offset() == before
