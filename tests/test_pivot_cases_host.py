"""The planted matrices of tests/pivot_cases.py fail where they are said to (CPU only).

For every shape tests/test_gpu_failed_pivot.py runs, every series it plants in and every (i, kind) it plants there:
  * the fp64 restatement of include/volt_hip.h's definition, `first_failed_pivot`, gives i + 1 on plant(...) + s2 I;
  * for the kinds without a NaN so does LAPACK (torch.linalg.cholesky_ex);
  * the margins that make i + 1 the answer in fp32 as well are CONDITIONS here, not measurements: a `neg` or `schur` pivot is
    at least 1e-4 from zero (four orders above the fp32 rounding of a sum of at most 1700 terms of size at most 1e-3), a `zero`
    pivot is exactly 0, and every clean pivot before the planted one is >= 1;
  * only row i of the lower triangle differs from the clean matrix, so the rows above keep the clean factor -- which is what lets
    `first_failed_pivot` start at row i (`known`); a sample of cases per shape is also run from row 0.
A shape that misses a condition is replaced, not the bound."""
import numpy as np
import pytest
import torch

import pivot_cases as pc

SHAPES = sorted(pc.shapes().items())
ALL_PATHS = {**pc.PATHS, **{k: v[:6] for k, v in pc.TUNED_PATHS.items()}}


def _noisy(Kp, s2):
    return Kp.astype(np.float64) + float(s2) * np.eye(Kp.shape[0])


def test_row_by_row_and_column_by_column_are_the_same_factor():
    """`clean_factor` loops by columns for speed; `factor` is the row-by-row reference.  Same entries to fp64 round-off, and
    LAPACK's."""
    K, _r, s2 = pc.clean(2, 300)
    A = _noisy(K[1], s2[1])
    L, piv = pc.factor(A)
    Lc, pivc = pc.clean_factor(2, 300, 1)
    assert np.abs(L - Lc).max() <= 1e-14 and np.abs(piv - pivc).max() <= 1e-14
    assert np.abs(L - np.linalg.cholesky(A)).max() <= 1e-14
    assert pc.first_failed_pivot(A) == (0, None)


def test_the_paths_take_the_dispatch_tables_shapes():
    """Every fp32 step / factorisation case of tests/golden/make_golden_dispatch_bits.py -- the smallest shape that takes one
    path, confirmed there -- is a path here, with its shape, options and schedule."""
    entry_of = {"mll": "mll", "potrf": "potrf", "potrf_two_call": "two_call"}
    have = {(e, B, N, tuple(sorted(opt.items()))): sched for e, B, N, opt, sched, _f in pc.PATHS.values()}
    seen = 0
    for name, (kind, B, N, opt, path) in pc.maker.CASES.items():
        if kind in entry_of:
            assert have.get((entry_of[kind], B, N, tuple(sorted(opt.items())))) == path, name
            seen += 1
    assert seen == 12


def test_positions_cover_the_phase_and_tile_borders():
    for N in sorted({n for (_b, n), _s in SHAPES}):
        p = pc.positions(N)
        assert p == sorted(set(p)) and p[0] == 0 and p[-1] == N - 1
        assert {0, 31, 32, 63, 64, 95, 96, 127, 128} <= set(p)
        last = 128 * ((N - 1) // 128)
        assert last in p                                     # first row of the last tile
        for t in ((N // 128) // 2, N // 128 - 1):            # a middle tile and the last complete one
            assert {128 * t + o for o in (31, 32, 63, 64, 95, 96, 127)} <= set(p)
        got = pc.cases(N)
        assert len(got) == len(set(got))
        assert all(not (k == "schur" and i < 31) and not (k == "nan_off" and i < 1) for i, k in got)
        assert {k for _i, k in got} == set(pc.KINDS)


def test_calls_plant_in_at_most_half_the_series_and_leave_the_ends_clean_once():
    for name, (_entry, B, N, _opt, _sched, full) in ALL_PATHS.items():
        calls = pc.calls(B, N, full)
        seen = {(i, k) for call in calls for _b, i, k in call}
        assert seen == set(pc.cases(N)), name                # every case runs on every path
        for call in calls:
            ser = [b for b, _i, _k in call]
            assert len(ser) == len(set(ser)) and len(ser) <= max(1, B // 2), name
            if len(ser) > 1:
                assert len({(i, k) for _b, i, k in call}) == len(ser), name     # different cases side by side
        if B >= 6:
            for end in (0, B - 1):
                assert any(end in [b for b, _i, _k in c] for c in calls), name
                assert any(end not in [b for b, _i, _k in c] for c in calls), name
            assert any(len(c) > 1 for c in calls), name


@pytest.mark.parametrize("B,N", [s for s, _ in SHAPES])
def test_every_planted_case_fails_first_at_its_pivot(B, N):
    K, _r, s2 = pc.clean(B, N)
    series = pc.shapes()[(B, N)]
    todo = {}
    for name, (_entry, b_, n_, _opt, _sched, full) in ALL_PATHS.items():
        if (b_, n_) == (B, N):
            for call in pc.calls(B, N, full):
                for b, i, kind in call:
                    todo.setdefault(b, set()).add((i, kind))
    assert set(todo) == series
    worst = {"neg": np.inf, "schur": np.inf}
    full_runs = 0
    for b in sorted(todo):
        L, piv = pc.clean_factor(B, N, b)
        assert piv.min() >= 1.0, (b, piv.min())              # every clean pivot, so every pivot before a planted one
        for i, kind in sorted(todo[b]):
            Kp = pc.plant(K[b], s2[b], i, kind, L)
            diff = np.argwhere(np.tril(Kp) != np.tril(K[b]))
            assert len(diff) and (diff[:, 0] == i).all(), (b, i, kind)          # (NaN != NaN: the NaN kinds show up too)
            if kind != "zero":
                assert len(diff) == 1
            A = _noisy(Kp, s2[b])
            at, d = pc.first_failed_pivot(A, known=(L, i))
            assert at == i + 1, (b, i, kind, at, d)
            if kind in ("neg", "schur"):
                assert d <= -1e-4, (b, i, kind, d)
                worst[kind] = min(worst[kind], -d)
                if kind == "schur":
                    assert A[i, i] > 0                       # the diagonal of K + s2 I stays positive: only the sum fails it
            elif kind == "zero":
                assert d == 0.0 and float(np.float32(Kp[i, i]) + np.float32(s2[b])) == 0.0
            else:
                assert np.isnan(d)
            if kind not in pc.NAN_KINDS:
                assert int(torch.linalg.cholesky_ex(torch.from_numpy(A)).info) == i + 1, (b, i, kind)
            # from row 0, without `known`: the first case of each kind on the first series, where that is cheap
            if N <= 512 and b == min(todo) and full_runs < 2 * len(pc.KINDS) and i <= 128:
                assert pc.first_failed_pivot(A)[0] == i + 1
                full_runs += 1
    print(f"({B}, {N}): {sum(len(v) for v in todo.values())} planted matrices on {len(todo)} series; smallest |pivot| neg "
          f"{worst['neg']:.3g}, schur {worst['schur']:.3g}")


@pytest.mark.parametrize("B,N", [s for s, _ in SHAPES])
def test_two_failures_in_one_matrix_fail_at_the_first(B, N):
    K, _r, s2 = pc.clean(B, N)
    b = B // 2
    L, _piv = pc.clean_factor(B, N, b)
    for pair in pc.doubles(N):
        (i0, _k0), (i1, _k1) = pair
        assert i0 < i1 < N
        A = _noisy(pc.plant_double(K[b], s2[b], pair, L), s2[b])
        assert pc.first_failed_pivot(A, known=(L, i0))[0] == i0 + 1
        assert int(torch.linalg.cholesky_ex(torch.from_numpy(np.nan_to_num(A, nan=0.0))).info) == i0 + 1
