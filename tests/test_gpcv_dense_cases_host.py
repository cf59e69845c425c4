"""CPU checks of the dense GPCV step's edge cases (tests/gpcv_dense_cases.py), before a GPU is involved:

  * the conditions on the inputs -- properties of the case list, not of the kernel: the designated rows of a "floored" case
    have an fp64 variance below min_var / 2 and every other row of every case one above 2 min_var; a "clamped" case has at
    least 5 % of every series' nodes under the clamp; and no node of any case lies within 1e-4 of the clamp (|f - log min_scale|
    for "exp", |s - min_scale| / min_scale for "cv"), where fp32 could legitimately take the other branch;
  * the restatement of the step in fp64 is the oracle, and in float32 it meets the GPU test's bounds on every case outside
    LONG: the bounds are reachable in that precision;
  * the negative controls: each deliberately wrong fp64 result FAILS the comparison on the case named for it.

No device is needed."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gpcv_dense_cases as D  # noqa: E402
import spd_families  # noqa: E402

IDS = [D.case_id(c) for c in D.ALL_CASES]


def find(**kw):
    got = [c for c in D.ALL_CASES if all(getattr(c, k) == v for k, v in kw.items())]
    assert got, kw
    return got


def test_the_case_list_is_what_it_says():
    assert len(IDS) == len(set(IDS))
    counts = {g: len(find(group=g)) for g in ("SIZES", "LONG", "KINDS", "WEIGHTS", "QUAD", "KC")}
    print("dense GPCV cases:", counts, "total", len(D.ALL_CASES))
    assert counts == dict(SIZES=49, LONG=2, KINDS=12, WEIGHTS=8, QUAD=14, KC=8)
    assert {c.n for c in find(group="SIZES", Kc=0, prior="bm", B=1)} == set(D.EDGE_N)
    assert {c.Kc for c in D.ALL_CASES} == set(range(9))
    assert {0, 127, 128, 129} <= set(D.floored_rows(130))
    for c in D.ALL_CASES:
        we, wk = D.weights(c)
        assert c.group == "WEIGHTS" or (we != wk and we > 0 and wk > 0)           # a swap of the weights shows everywhere


@pytest.mark.parametrize("c", D.ALL_CASES, ids=IDS)
def test_conditions_on_the_inputs(c):
    for b, s in enumerate(D.inputs(c)):
        for k in ("y", "m", "Lq", "c", "K") + (("abc",) if c.Kc else ()):
            assert torch.equal(s[k], D.r32(s[k])), (b, k)                         # both sides read the same numbers
        var = D.variances(s["Lq"])
        rows = torch.zeros(c.n, dtype=torch.bool)
        rows[s["floored"]] = True
        assert (c.kind == "floored") == bool(rows.any())
        assert bool((var[rows] < D.MIN_VAR / 2).all()), (b, var[rows])
        assert bool((var[~rows] > 2 * D.MIN_VAR).all()), (b, float(var[~rows].min()))
        share, margin = D.node_margins(s, c)
        assert margin >= D.CLAMP_MARGIN, (b, margin)
        if c.kind == "clamped":
            assert share >= 0.05, (b, share)
        if c.kind == "all_clamped":
            assert share == 1.0
        assert not torch.equal(s["Lq"], s["Lq"].tril()) or c.n == 1               # junk above the diagonal


@pytest.mark.parametrize("c", D.SHORT_CASES, ids=[D.case_id(c) for c in D.SHORT_CASES])
def test_restatement_is_the_oracle_and_fp32_meets_the_bounds(c):
    ref = D.oracle(c)
    r64 = D.ratios(D.restated(c), ref)
    assert max(r64.values()) <= 1e-3, r64                                         # (fp64 round-off against bounds of 5e-5 .. 5e-3)
    r32 = D.ratios(D.restated(c, torch.float32), ref)
    print("DENSE-FP32", D.case_id(c), D.fmt(r32))
    assert D.passes(r32), r32
    assert D.passes(D.ratios(D.stack(ref), ref))


def test_all_clamped_ell_has_its_closed_form():
    """m = -30: every node is clamped, ell = -sum_i (y_i^2 / (2 min_scale^2) + log min_scale + log sqrt(2 pi)), and the
    likelihood has no gradient at all."""
    for c in find(kind="all_clamped"):
        for s, r in zip(D.inputs(c), D.oracle(c)):
            want = D.all_clamped_ell(s, c)
            assert abs(r["out"]["ell"] - want) <= 1e-12 * abs(want)
            if c.Kc:
                assert not r["grad_abc"].any()
            we0 = D.restate(s, c._replace(group="WEIGHTS", weights="0,1"))        # the same inputs without the likelihood
            wk = D.weights(c)[1]
            for k in ("grad_m", "grad_Lq"):
                assert float((r[k] - wk * we0[k]).abs().max()) <= 1e-12 * float(r[k].abs().max()), k


def test_zero_weights_have_exactly_zero_gradients():
    for c in find(group="WEIGHTS", weights="0,1"):
        for r in D.oracle(c):
            assert float(r["grad_m"].sum() + r["grad_mu"]) == pytest.approx(0.0, abs=1e-9 * float(r["grad_m"].abs().max()))
            assert c.Kc == 0 or not r["grad_abc"].any()
    for c in find(group="WEIGHTS", weights="1,0"):
        for r in D.oracle(c):
            assert r["grad_mu"] == 0.0 and not r["grad_K"].any()


# ------------------------------------------------------------------------------------------------ negative controls
def _broken(c, broken):
    r = D.ratios(D.restated(c, broken=broken), D.oracle(c))
    print("DENSE-CONTROL", broken, D.case_id(c), "passes" if D.passes(r) else "fails", D.fmt(r))
    return r


def test_control_swapped_weights():
    """w_ell and w_kl exchanged: seen at (1/n, 0.25/n) -- and not at (1, 1), which is why that pair alone was not enough."""
    for c in find(group="WEIGHTS", weights="1/n,0.25/n"):
        assert not D.passes(_broken(c, "swap"))
    for c in find(group="WEIGHTS", weights="1,1"):
        assert D.passes(_broken(c, "swap"))
    for c in find(group="SIZES", n=65):                                           # the default weights are unequal too
        assert not D.passes(_broken(c, "swap"))


def test_control_floor_ignored():
    for c in find(kind="floored"):
        assert not D.passes(_broken(c, "nofloor"))
    for c in find(kind="clamped"):                                                # (nothing to ignore where no row is floored)
        assert D.passes(_broken(c, "nofloor"))


def test_control_clamped_nodes_keep_their_gradient():
    for c in find(kind="clamped"):
        assert not D.passes(_broken(c, "clampgrad"))


def test_control_f_instead_of_log_min_scale():
    for c in find(kind="clamped", Kc=0):
        r = _broken(c, "logf")
        assert not D.passes(r) and r["out"] > 1.0 and r["grad_m"] > 1.0


def test_control_permuted_rows_of_an_off_diagonal_block():
    """The rows of the off-diagonal 128-block of grad_Lq in reverse order, at n = 257.  Seen on "wishart".  It was expected
    to go unseen on "bm", whose Cholesky factor has rank-one blocks -- but the block of grad_Lq is the block of K^-1 Lq, and
    Lq's rows are random whatever the prior: measured, the control fails on "bm" as well (by more: the Brownian prior's K^-1
    is larger), and that is what is asserted."""
    perm = np.arange(128)[::-1].copy()
    for prior in ("wishart", "bm"):
        (c,) = find(group="SIZES", n=257, B=1, prior=prior, Kc=0)
        ref = D.oracle(c)
        got = D.stack(ref)
        got["grad_Lq"] = torch.as_tensor(spd_families.permute_block_rows(got["grad_Lq"].numpy(), slice(128, 256), slice(0, 128),
                                                                         perm))
        r = D.ratios(got, ref)
        print("DENSE-CONTROL permuted rows", D.case_id(c), D.fmt(r))
        assert r["grad_Lq"] > 1.0 and all(v < 1.0 for k, v in r.items() if k != "grad_Lq")


def test_control_one_pass_of_the_abc_reduction():
    """cv_abc_reduce_kernel stopped after one pass: the row blocks 256 .. ceil(N/4) - 1 (here the one block of row 1024) left
    out of grad_abc."""
    (c,) = find(group="LONG", Kc=5)
    s, ref = D.inputs(c)[0], D.oracle(c)
    nblk = (c.n + 3) // 4
    assert nblk > 256
    part = D.restate(s, c, rows=torch.arange(min(c.n, 4 * 256)))
    got = D.stack(ref)
    got["grad_abc"] = part["grad_abc"][None]
    r = D.ratios(got, ref)
    print("DENSE-CONTROL one pass of abc", D.case_id(c), D.fmt(r))
    assert min(r["grad_a"], r["grad_b"], r["grad_c"]) > 1.0


def test_control_one_pass_of_the_tile_sums():
    """gpcv_scalars_kernel stopped after one pass: the tile sums 256 .. 288 of the 17 x 17 left out of tr(K^-1 S) (and of
    |K^-1 Lq|_F^2, which no bound covers).  Tile (tm, tn) of T' = Lq' L^-T holds the block (tn, tm) of T = L^-1 Lq."""
    (c,) = find(group="LONG", Kc=0)
    s, ref = D.inputs(c)[0], D.oracle(c)
    nt = (c.n + 127) // 128
    assert nt * nt - 256 == 33
    Lk = torch.linalg.cholesky(s["K"] + D.JITTER * torch.eye(c.n, dtype=torch.float64))
    T = torch.linalg.solve_triangular(Lk, s["Lq"].tril(), upper=False)
    assert abs(float(T.pow(2).sum()) - ref[0]["out"]["trace"]) <= 1e-9 * ref[0]["out"]["trace"]
    lost = sum(float(T[128 * (t % nt):128 * (t % nt + 1), 128 * (t // nt):128 * (t // nt + 1)].pow(2).sum())
               for t in range(256, nt * nt))
    got = D.stack(ref)
    wk = D.weights(c)[1]
    got["out"][0, 5] -= lost
    got["out"][0, 1] -= 0.5 * lost
    got["out"][0, 9] += 0.5 * wk * lost
    r = D.ratios(got, ref)
    print("DENSE-CONTROL one pass of tile sums", D.case_id(c), f"lost {lost:.4g} of {ref[0]['out']['trace']:.6g}", D.fmt(r))
    assert r["out"] > 1.0
