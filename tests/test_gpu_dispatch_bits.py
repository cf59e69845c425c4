"""Every dispatch path of the library hands its caller the bits it handed before the host interface was tidied (csrc/host.h).

The host side picks the schedule a shape runs and carves the caller's scratch; none of that may move a result bit.  For each
path -- the short- and long-series one-launch steps, the batched one-launch step with both hand-off protocols, the
launch-per-column schedule as one and as two stream groups, the table-free and forward-only steps, alpha's refinement, the
factorisation entries, the inverses, and the fp64 twins -- the smallest shape that takes it is run and the sha256 of what
comes back (out, alpha, info and the factor left in the workspace; A, Winv, Y for the factorisation entries) is compared
with the digest recorded on an MI355X before the change: tests/golden/dispatch_bits.json, written by
tests/golden/make_golden_dispatch_bits.py, which also confirms the path each shape takes.  Only cases that two separate
processes reproduced are in the table; what was left out is listed there under `omitted`."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_golden_dispatch_bits", os.path.join(GOLDEN, "make_golden_dispatch_bits.py"))
maker = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(maker)

with open(os.path.join(GOLDEN, "dispatch_bits.json")) as _fh:
    TABLE = json.load(_fh)


def test_the_table_covers_the_cases():
    assert set(TABLE["cases"]) | set(TABLE["omitted"]) == set(maker.CASES)
    assert not set(TABLE["cases"]) & set(TABLE["omitted"])
    # only the K-sliced paths sum in arrival order: nothing else may be left out
    assert set(TABLE["omitted"]) <= {"f32_step_no_tables"}


@pytest.mark.parametrize("name", sorted(TABLE["cases"]))
def test_same_bits_as_before(name):
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("needs a GPU")
    got, want = maker.run_case(name), TABLE["cases"][name]
    assert got["inputs"] == want["inputs"], "the test's own inputs differ from the recorded ones"
    for what in want:
        print(name, what, got[what], "recorded", want[what])
    assert got == want
