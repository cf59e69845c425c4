"""Matrices whose Cholesky factorisation fails at a known pivot, and the reference that says which (host only, numpy).

include/volt_hip.h: `info[b]` is 0, or the 1-based index of the first non-positive / NaN pivot.  `first_failed_pivot` is that
sentence as code -- an unblocked fp64 Cholesky of the lower triangle, row by row -- and is the reference of
tests/test_pivot_cases_host.py (which checks every case below against it, on the CPU) and of tests/test_gpu_failed_pivot.py
(which runs the same cases through every fp32 dispatch path).  LAPACK is only a cross-check: a vendor potrf need not test for NaN.

The clean matrices are `inputs(B, N)` of tests/golden/make_golden_dispatch_bits.py: integers scaled by powers of two, identical
on every machine, off-diagonal +-1/32 under a diagonal in [3, 4).  `plant` edits ONE row of the lower triangle so that pivot i
fails, in one of five ways (KINDS).  Rows < i of a factor depend on rows < i of the matrix alone, so every pivot before i is the
clean matrix's (>= 1: tests/test_pivot_cases_host.py) and i + 1 is the first failed pivot in any precision as long as the
failed pivot's own sign is beyond rounding: `neg` and `schur` keep |d| >= 1e-4, `zero` is exact, the NaN kinds need no margin."""
import functools
import importlib.util
import os

import numpy as np

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_golden_dispatch_bits", os.path.join(_GOLDEN, "make_golden_dispatch_bits.py"))
maker = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(maker)

KINDS = ("neg", "schur", "zero", "nan_diag", "nan_off")
NAN_KINDS = ("nan_diag", "nan_off")


def first_failed_pivot(A, known=None):
    """(j + 1, d_j) for the first pivot d_j = A[j,j] - sum_{m<j} L[j,m]^2 with not (d_j > 0), or (0, None): an unblocked fp64
    Cholesky of the lower triangle of A, row by row (row j: L[j,m] = (A[j,m] - sum_{c<m} L[j,c] L[m,c]) / L[m,m], m < j, then d_j).
    `known` = (L, r): rows < r of the factor are taken from L instead of being worked out again -- they depend on rows < r of
    A alone, so this is the same arithmetic for a matrix that equals L's above row r."""
    return _cholesky(A, known)[:2]


def factor(A):
    """(L, pivots) of the same row-by-row fp64 Cholesky; raises if a pivot fails."""
    j, d, L, piv = _cholesky(A, None)
    if j:
        raise ValueError(f"pivot {j} = {d}")
    return L, piv


def _cholesky(A, known):
    A = np.asarray(A, dtype=np.float64)
    n = A.shape[0]
    L = np.zeros((n, n))
    piv = np.zeros(n)
    r0 = 0
    if known is not None:
        L0, r0 = known
        L[:r0] = L0[:r0]
        piv[:r0] = np.diagonal(L0)[:r0] ** 2
    for j in range(r0, n):
        row = L[j]
        a = A[j]
        for m in range(j):                                   # forward substitution against the rows above
            row[m] = (a[m] - row[:m] @ L[m, :m]) / L[m, m]
        d = a[j] - row[:j] @ row[:j]
        if not d > 0:
            return j + 1, d, L, piv
        piv[j] = d
        row[j] = np.sqrt(d)
    return 0, None, L, piv


@functools.lru_cache(maxsize=None)
def clean(B, N):
    """inputs(B, N) in fp32: (K [B,N,N], resid [B,N], sigma2 [B]); read-only."""
    K, r, s2 = maker.inputs(B, N)
    for x in (K, r, s2):
        x.setflags(write=False)
    return K, r, s2


@functools.lru_cache(maxsize=None)
def clean_factor(B, N, b):
    """(L, pivots) of series b of inputs(B, N) plus its noise (`_by_columns`).  Worked out once and shared."""
    K, _r, s2 = clean(B, N)
    L, piv = _by_columns(K[b].astype(np.float64) + float(s2[b]) * np.eye(N))
    L.setflags(write=False)
    piv.setflags(write=False)
    return L, piv


def _by_columns(A):
    """`factor` with its loops the other way round: entry (j, m) is the same (A[j,m] - sum_{c<m} L[j,c] L[m,c]) / L[m,m], worked
    out for all rows j > m at once -- a matrix-vector product per column instead of a Python loop per entry (0.3 s instead of
    minutes at N = 1280).  tests/test_pivot_cases_host.py compares the two."""
    n = A.shape[0]
    L = np.zeros((n, n))
    piv = np.zeros(n)
    for m in range(n):
        col = A[m:, m] - L[m:, :m] @ L[m, :m]
        d = col[0]
        if not d > 0:
            raise ValueError(f"pivot {m + 1} = {d}")
        piv[m] = d
        L[m, m] = np.sqrt(d)
        L[m + 1:, m] = col[1:] / L[m, m]
    return L, piv


def plant(K, s2, i, kind, Lref=None):
    """A copy of K (one fp32 matrix of `inputs`) whose factorisation with noise s2 fails first at pivot i (0-based); only row i of
    the lower triangle is edited.  Lref: the fp64 factor of the clean K + s2 I (`schur` only; worked out here when not given)."""
    N = K.shape[0]
    assert 0 <= i < N and kind in KINDS
    Kp = np.array(K, dtype=np.float32, copy=True)
    s2 = np.float32(s2)
    if kind == "neg":
        Kp[i, i] = -1.0
    elif kind == "schur":
        assert i >= 31, "below 31 terms the sum is too small for the margin"
        if Lref is None:
            Lref = factor(K.astype(np.float64) + float(s2) * np.eye(N))[0]
        Kp[i, i] = np.float32(0.5 * float(Lref[i, :i] @ Lref[i, :i])) - s2
    elif kind == "zero":
        Kp[i, :i] = 0.0
        Kp[i, i] = -s2
    elif kind == "nan_diag":
        Kp[i, i] = np.nan
    else:
        assert i >= 1, "row 0 has nothing below the diagonal"
        Kp[i, i // 2] = np.nan
    return Kp


def positions(N):
    """Where a 32-pivot phase, a 128-tile or the matrix begins and ends: 0, 31, 32, 63, 64, 95, 96, 127, 128; the same eight
    offsets inside a middle tile and inside the last complete tile; the first row of the last tile; N - 1."""
    off = (31, 32, 63, 64, 95, 96, 127, 128)
    full = N // 128                                          # complete tiles
    p = {0, *off, 128 * ((N - 1) // 128), N - 1}
    for t in (full // 2, full - 1):
        if t >= 0:
            p |= {128 * t + o for o in off}
    return sorted(x for x in p if 0 <= x < N)


def cases(N):
    """Every (i, kind) of positions(N) x KINDS that is a case (`schur` needs i >= 31, `nan_off` i >= 1): position-major, so
    that neighbours in the list differ in kind."""
    return [(i, k) for i in positions(N) for k in KINDS if not (k == "schur" and i < 31) and not (k == "nan_off" and i < 1)]


# Two failures in one matrix: ((first, kind), (second, kind)); info names the smaller index.  Same 32-pivot phase; different
# tiles (the second clipped to the matrix); a NaN below the diagonal of a later row than a negative diagonal.
def doubles(N):
    return [((40, "schur"), (45, "neg")), ((100, "neg"), (min(300, N - 1), "schur")), ((150, "neg"), (200, "nan_off"))]


def plant_double(K, s2, pair, Lref=None):
    (i0, k0), (i1, k1) = pair
    Kp = plant(K, s2, i0, k0, Lref)
    Kq = plant(K, s2, i1, k1, Lref)
    Kp[i1, :i1 + 1] = Kq[i1, :i1 + 1]                        # rows i0 != i1: the two edits do not meet
    return Kp


def calls(B, N, full=None):
    """The calls of one path: a list of calls, each a list of (series, i, kind) planted together.
    B <= 2: one series per call, the series taking turns.  B >= 6: at most half the series per call -- even series in one call, odd
    ones in the next, so that series 0 and B - 1 are each clean in one call and planted in another -- and every series of a call
    with a different case.  full = a series: the two launch-per-column shapes carry every case on that series alone (one per
    call) and the even / odd pattern once."""
    cs = cases(N)
    if B <= 2:
        return [[(c % B, i, k)] for c, (i, k) in enumerate(cs)]
    half = B // 2
    sets = ([b for b in range(0, B, 2)][:half], [b for b in range(1, B, 2)][:half])
    if full is not None:
        out = [[(full, i, k)] for (i, k) in cs]
        for s, ser in enumerate(sets):
            out.append([(b, *cs[(7 * x + 3 * s) % len(cs)]) for x, b in enumerate(ser)])
        return out
    out, c = [], 0
    while c < len(cs):
        ser = sets[len(out) % 2]
        out.append([(b, *cs[c + x]) for x, b in enumerate(ser) if c + x < len(cs)])
        c += len(ser)
    if len(out) < 2:
        out.append([(b, *cs[x % len(cs)]) for x, b in enumerate(sets[1])])
    return out


# ---- the fp32 dispatch paths.  name: (entry, B, N, options, schedule, series that carries every case alone or None).
# entry: "mll" ops.mll_step; "potrf" ops.potrf (volt_potrf_k_f32); "two_call" volt_prepare_f32 + volt_potrf_ws_f32 with its
# workspace; "plain" volt_prepare_f32 + volt_potrf_f32.  schedule: "small" / "long" / "batch" the one-launch steps, "columns" a
# launch per block column, "split" the launch per block column with every long product in K-slices (fewer than 3 matrices
# with scratch).  The shapes are make_golden_dispatch_bits.CASES' where it has the path (tests/test_pivot_cases_host.py checks);
# N = 1200 is the ragged twin of the one-launch paths whose table shape is a multiple of 128 (the identity padding begins inside
# a 32-pivot phase of the last tile).
PATHS = {
    "step_short_series": ("mll", 2, 300, {}, "small", None),
    "step_long_series": ("mll", 1, 500, {}, "long", None),
    "step_batched_local": ("mll", 8, 1280, {}, "batch", None),
    "step_batched_agent": ("mll", 6, 1280, {}, "batch", None),
    "step_columns_one_group": ("mll", 72, 384, {}, "columns", 36),
    "step_columns_two_groups": ("mll", 144, 512, {}, "columns", 72),
    "step_no_tables": ("mll", 2, 300, {"tables": False}, "columns", None),
    "step_forward_only_batched": ("mll", 8, 1280, {"want_grad": False}, "batch", None),
    "step_forward_only_short": ("mll", 2, 300, {"want_grad": False}, "columns", None),
    "step_refine_alpha": ("mll", 2, 300, {"refine_alpha": True}, "small", None),
    "potrf_tables": ("potrf", 8, 1280, {}, "batch", None),
    "potrf_no_tables": ("potrf", 8, 1280, {"tables": False}, "columns", None),
    "potrf_two_call": ("two_call", 8, 1280, {}, "batch", None),
    "potrf_plain": ("plain", 2, 300, {}, "columns", None),
    "potrf_split_k": ("potrf", 2, 500, {}, "split", None),
    "step_batched_local_ragged": ("mll", 8, 1200, {}, "batch", None),
    "step_batched_agent_ragged": ("mll", 6, 1200, {}, "batch", None),
    "step_forward_only_batched_ragged": ("mll", 8, 1200, {"want_grad": False}, "batch", None),
    "potrf_tables_ragged": ("potrf", 8, 1200, {}, "batch", None),
    "potrf_two_call_ragged": ("two_call", 8, 1200, {}, "batch", None),
}
# A schedule the full chip never reaches by itself: with scratch and its tables, 3 .. 64 matrices run the late block columns
# (from column 12 on for the factorisation alone, where more than one such column is left: chol.hip run_factor_groups,
# sched_build) from the host-balanced piece list of csrc/sched.h -- but every shape that gets there is taken by the batched one
# launch first (batch_step.hip volt_internal_batch_applies).  A device that is not the full MI355X has the one-launch steps off
# and runs it; here a child process started with ENV does.  name: (entry, B, N, options, schedule, full, ENV).  N = 1700: 14 block
# columns, the last complete tile (12) and the ragged last one (13) are the two scheduled columns.
TUNED_PATHS = {
    "potrf_columns_balanced": ("potrf", 8, 1700, {}, "columns", None, {"VOLT_TUNE": "1", "VOLT_BATCH": "0"}),
}


def shapes():
    """{(B, N): the series that get a planted matrix on some path}."""
    out = {}
    for _entry, B, N, _opt, _sched, full in list(PATHS.values()) + [v[:6] for v in TUNED_PATHS.values()]:
        for call in calls(B, N, full):
            out.setdefault((B, N), set()).update(b for b, _i, _k in call)
    return out
