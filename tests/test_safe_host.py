"""The internal-error fall-back of the failure policy (volt_amd/safe.py: `rerun_table_free`, shared by `_safe_factor` and
gp._ExactMLL) on the host: ops.potrf / ops.mll_step are replaced by torch.linalg.cholesky_ex on the CPU with the library's
internal code written into ``info`` on a schedule the case chooses, so the sequence -- which calls with which ``tables``, which
warnings, which error text -- is pinned without a device and without trampling a workspace (the device-side cover stays
tests/test_gpu_contract.py::test_internal_errors_are_not_reported_as_not_positive_definite)."""
import warnings

import pytest
import torch

INT_MIN = -(2 ** 31)
WARN = "A not p.d., added jitter of {:.1e} to the diagonal"


class Factor:
    def __init__(self, L, info):
        self.L, self.info = L, info


@pytest.fixture
def fake(monkeypatch):
    """fake(internal): installs the two entries; ``internal(call number, tables, jitter)`` says when info is the internal code.
    Returns the list of (entry, jitter, tables) of every call."""
    from volt_amd import ops
    calls = []

    def install(internal):
        del calls[:]

        def info_of(A, jitter, tables):
            L, info = torch.linalg.cholesky_ex(A + jitter * torch.eye(A.shape[-1], dtype=A.dtype))
            info = info.to(torch.int32)
            return L, torch.full_like(info, INT_MIN) if internal(len(calls), tables, jitter) else info

        def potrf(A3, sigma2=None, jitter=0.0, tables=True):
            calls.append(("potrf", jitter, tables))
            return Factor(*info_of(A3, jitter, tables))

        def mll_step(K, resid, sigma2, ws=None, want_grad=True, jitter=0.0, refine_alpha=False, tables=True):
            calls.append(("mll_step", jitter, tables))
            L, info = info_of(K + sigma2.reshape(-1, 1, 1) * torch.eye(K.shape[-1], dtype=K.dtype), jitter, tables)
            out = torch.zeros(K.shape[0], 8, dtype=K.dtype)
            out[:, 0] = torch.diagonal(L, dim1=-2, dim2=-1).log().sum(-1)
            return out, torch.zeros_like(resid), info
        monkeypatch.setattr(ops, "potrf", potrf)
        monkeypatch.setattr(ops, "mll_step", mll_step)
        return calls
    return install


def observe(fn):
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        try:
            out, err = fn(), None
        except Exception as e:                                     # noqa: BLE001 -- the exception is what is looked at
            out, err = None, e
    return out, err, [(w.category, str(w.message)) for w in rec]


def matrix(c, dtype=torch.float32, B=2):
    """I [B,4,4] with A[1,2,2] = -c (c None: the identity)."""
    A = torch.eye(4, dtype=dtype).repeat(B, 1, 1)
    if c is not None:
        A[1, 2, 2] = -c
    return A


POTRF_WARNING = ("volt_potrf reported an internal error (info = [-2147483648, -2147483648] ...) on its one-launch schedule; "
                 "re-run on the launch-per-column schedule")


def test_safe_factor_falls_back_once_and_stays_table_free(fake):
    from volt_amd import _lib, gp
    calls = fake(lambda n, tables, jitter: tables)                  # the one-launch schedule always reports the internal code
    (f, used), err, warned = observe(lambda: gp._safe_factor(matrix(None)))
    assert err is None and used == 0.0 and not f.info.any() and warned == [(_lib.VoltHipWarning, POTRF_WARNING)]
    assert calls == [("potrf", 0.0, True), ("potrf", 0.0, False)]
    del calls[:]
    (f, used), err, warned = observe(lambda: gp._safe_factor(matrix(3e-6)))          # a real pivot failure behind it: rung 1
    assert err is None and used == 1e-6 * (10 ** 1) and not f.info.any()
    assert warned == [(_lib.VoltHipWarning, POTRF_WARNING), (gp.NumericalWarning, WARN.format(1e-5))]
    assert calls == [("potrf", 0.0, True), ("potrf", 0.0, False), ("potrf", 1e-6, False), ("potrf", 1e-6 * (10 ** 1), False)]
    del calls[:]
    _, err, warned = observe(lambda: gp._safe_factor(matrix(float("nan"))))           # NaN is looked for after the fall-back
    assert type(err) is gp.NanError and str(err) == "cholesky_cpu: 1 of 32 elements of the (2, 4, 4) tensor are NaN."
    assert calls == [("potrf", 0.0, True), ("potrf", 0.0, False)] and warned == [(_lib.VoltHipWarning, POTRF_WARNING)]


def test_safe_factor_raises_on_a_second_internal_code(fake):
    from volt_amd import _lib, gp
    calls = fake(lambda n, tables, jitter: True)
    _, err, warned = observe(lambda: gp._safe_factor(matrix(None)))
    assert type(err) is _lib.VoltHipError and str(err) == f"volt_potrf: internal error on both schedules, info = {[INT_MIN] * 2}"
    assert calls == [("potrf", 0.0, True), ("potrf", 0.0, False)] and warned == [(_lib.VoltHipWarning, POTRF_WARNING)]
    calls = fake(lambda n, tables, jitter: jitter > 0)               # a pivot failure first, the internal code inside the ladder
    _, err, warned = observe(lambda: gp._safe_factor(matrix(3e-6)))
    assert type(err) is _lib.VoltHipError and str(err) == f"volt_potrf: internal error, info = {[INT_MIN] * 2}" and warned == []
    assert calls == [("potrf", 0.0, True), ("potrf", 1e-6, True)]


class Holder:
    def workspace(self, *a):
        return None


def mll(A):
    from volt_amd import gp
    B, n = A.shape[:2]
    zeros, noise = torch.zeros(B, n, dtype=A.dtype), torch.full((B,), 1e-4, dtype=A.dtype)
    return observe(lambda: gp._ExactMLL.apply(A - 1e-4 * torch.eye(n, dtype=A.dtype), zeros, noise, zeros, Holder(), None))


MLL_WARNING = ("volt_mll_step_f32 reported an internal error (info = ['0x80000000']) on its one-launch schedule; the step was "
               "re-run on the launch-per-column schedule")


def test_the_mll_falls_back_once_and_its_rungs_return_to_the_one_launch_schedule(fake):
    from volt_amd import _lib, gp
    calls = fake(lambda n, tables, jitter: n == 1)                   # the first call only
    val, err, warned = mll(matrix(None))
    assert err is None and bool(torch.isfinite(val).all()) and warned == [(_lib.VoltHipWarning, MLL_WARNING)]
    assert calls == [("mll_step", 0.0, True), ("mll_step", 0.0, False)]
    fake(lambda n, tables, jitter: n == 1)
    val, err, warned = mll(matrix(3e-6))
    assert err is None and warned == [(_lib.VoltHipWarning, MLL_WARNING), (gp.NumericalWarning, WARN.format(1e-5))]
    assert calls == [("mll_step", 0.0, True), ("mll_step", 0.0, False), ("mll_step", 1e-6, True), ("mll_step", 1e-6 * (10 ** 1), True)]


def test_the_mll_raises_on_a_second_internal_code_and_at_once_in_fp64(fake):
    from volt_amd import _lib
    calls = fake(lambda n, tables, jitter: True)
    _, err, warned = mll(matrix(None))
    assert type(err) is _lib.VoltHipError and warned == [(_lib.VoltHipWarning, MLL_WARNING)]
    assert str(err) == f"volt_mll_step_f32: internal error on both schedules, info = {[INT_MIN] * 2}"
    assert calls == [("mll_step", 0.0, True), ("mll_step", 0.0, False)]
    calls = fake(lambda n, tables, jitter: jitter > 0)
    _, err, warned = mll(matrix(3e-6))
    assert type(err) is _lib.VoltHipError and str(err) == f"volt_mll_step: internal error, info = {[INT_MIN] * 2}" and warned == []
    assert calls == [("mll_step", 0.0, True), ("mll_step", 1e-6, True)]
    calls = fake(lambda n, tables, jitter: True)                     # the fp64 step has no table-free schedule
    _, err, warned = mll(matrix(None, torch.float64))
    assert type(err) is _lib.VoltHipError and str(err) == "volt_mll_step_f64: internal error, info = ['0x80000000']" and warned == []
    assert calls == [("mll_step", 0.0, True)]
