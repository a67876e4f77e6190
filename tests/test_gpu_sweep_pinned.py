"""The table optimizers' sweeps give the bits they gave when tests/golden/sweep_pinned.json was recorded: SGD, Adagrad, RMSprop,
SGDM (plain, Nesterov), FTRL and Adam at the smallest shapes at which every loop of the sweep runs (dense, marked with and
without an L2 term, the rate from the device, one block and the built-in cap), an unaligned tensor, 66 tensors in two launches,
Adam's lazy, deferred and co-launched steps and the three paths of row-wise Adagrad.  tests/golden/make_sweep_pinned.py holds the
cases and says how the file was made.  Nothing here has a tolerance: the kernels' element updates are correctly rounded as
written, so a digest moves only when an edit changes a result bit -- or, after a toolchain change alone, when the compiler no
longer rounds the updates as written, which is worth knowing."""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_sweep_pinned", os.path.join(_GOLDEN, "make_sweep_pinned.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

with open(G.JSON) as _f:
    PINNED = json.load(_f)


def test_the_file_holds_every_case():
    assert sorted(PINNED) == sorted(G.cases())


@pytest.mark.parametrize("name", sorted(PINNED))
def test_pinned_bits(name):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    want = PINNED[name]
    got = G.cases()[name](torch.device("cuda:0"))
    assert got["inputs"] == want["inputs"], (
        "%s: the INPUTS moved, not the kernels (the case builders or numpy's generator changed): nothing is known about the sweep" % name)
    moved = sorted(k for k in want if got.get(k) != want[k])
    assert not moved and sorted(got) == sorted(want), (
        "%s: %s differ from the recorded bits.  After an edit of the sweep: the edit changed a result.  After a toolchain change "
        "alone: the element updates are no longer rounded as written (csrc/opt_math.h, csrc/adam_math.h)" % (name, ", ".join(moved)))
