"""The workspace-size queries answer what they answered before the host interface was tidied (csrc/host.h): the sizes are
the sums the regions inside a workspace are carved by, so a layout that moved shows here.  Held against
tests/golden/workspace_bytes.json (tests/golden/make_golden_workspace_bytes.py), once for the full chip and once for a faked
64-CU / 2-XCD device, where the topology guard switches the one-launch steps (and their state regions) off.  No GPU."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_golden_workspace_bytes", os.path.join(GOLDEN, "make_golden_workspace_bytes.py"))
maker = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(maker)

with open(os.path.join(GOLDEN, "workspace_bytes.json")) as _fh:
    TABLE = json.load(_fh)


def test_the_table_is_for_this_grid():
    g = TABLE["grid"]
    assert (tuple(g["B"]), tuple(g["N"]), tuple(g["want_grad"]), tuple(g["T"])) == (maker.BS, maker.NS, maker.GRADS, maker.TASKS)
    assert maker.BS == (1, 2, 3, 7, 8, 9, 10, 16, 24, 31, 32, 40, 64, 65, 96)
    assert maker.NS == (100, 128, 256, 399, 1000, 1024, 1536, 2048, 3072, 4096)
    assert (tuple(g["Kc_cv"]), tuple(g["Kc_bm"])) == (maker.CV_KCS, maker.BM_KCS) == ((1, 8), (0, 3))


@pytest.mark.parametrize("topology", list(maker.TOPOLOGIES))
def test_workspace_bytes_are_the_recorded_ones(topology):
    # (the knobs are read once per process: the full chip is this process, the reduced device a child)
    got, want = maker.collect() if topology == "full_chip" else maker.collect_in_child(topology), TABLE[topology]
    assert set(got) == set(want) and len(want) == 9
    for q in want:
        assert got[q] == want[q], q
    # the guard's effect is in the table: no state of a one-launch step on the reduced device
    if topology != "full_chip":
        assert got != TABLE["full_chip"]
        assert all(v == 0 for row in got["volt_potrf_workspace_bytes_f64"] for v in row)
