"""GPU: the parameter gradients whose last step is a fixed-order merge of fp32 partials (csrc/partial_merge.h: the bias gradients of
bias_act_dropout and conv1d, resnorm's dgamma / dbeta / dbias, the weight gradients of the two Conv1d operators and of the Conformer
depthwise convolution, relpos attention's dpos / dbias_u / dbias_v) give, bit for bit, what the build before those tails were shared gave:
tests/golden/train_merge_parent.npz, recorded once by tests/golden/make_train_merge_parent.py.  The order of addition is part of the
operators' contract (bit-reproducible backward), so the comparison is torch.equal, with no tolerance.  The cases and what each one exercises
are in tests/util_train_merge_cases.py, shared with the recorder."""
import os

import numpy as np
import pytest
import torch

from tests import util_train_merge_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def parent(golden_dir):
    with np.load(os.path.join(golden_dir, "train_merge_parent.npz")) as z:
        return {k: z[k] for k in z.files}


def test_the_fixture_holds_exactly_the_cases(parent):
    assert {k.split("/")[0] for k in parent} == set(C.CASES)


@pytest.mark.parametrize("name", list(C.CASES))
def test_parameter_gradients_are_the_parents_bits(parent, name):
    got = C.run(name)
    assert {f"{name}/{k}" for k in got} == {k for k in parent if k.startswith(name + "/")}
    for key, t in got.items():
        want = torch.from_numpy(parent[f"{name}/{key}"])
        assert t.dtype == want.dtype and t.shape == want.shape, (name, key)
        assert torch.equal(t.cpu(), want), (name, key, float((t.cpu().float() - want.float()).abs().max()))
