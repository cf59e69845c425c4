"""The failure policy of every factorising route through ONE rung table: psd_safe_cholesky / `_safe_factor` (ops.potrf),
ExactMarginalLogLikelihood (ops.mll_step), `_safe_forms` (ops.vk_forms), `_safe_draw` (ops.markov_draw) and `_chol_1x1`.

The inputs put one pivot at -c and every other pivot far from zero, so with first rung s the route must succeed
    plain for the clean input,   at s for c = 0.3 s,   at 10 s for c = 3 s,   at 100 s for c = 30 s,   never for c = 1,
whatever the rounding: the nearest miss is 0.3 s against s.  s is gpytorch's default (1e-6 fp32, 1e-8 fp64) and a given 1e-4.
The dense routes take A = I with A[k,k] = -c (the table is first checked against the oracle's psd_safe_cholesky on the host);
the chain routes take the grids of their own ladder tests with one step of -c (checked against the fp64 restatements, on the
numbers the device sees).  Per case: the jitter used, the ONE NumericalWarning and its text (or none), the exception's type and
full text, and every (jitter, tables) the ops entry was called with -- a clean input calls it exactly once."""
import inspect
import warnings

import numpy as np
import pytest
import torch

import chain_draw_ref as chain
import vk_chain_ref as vk
import vk_forms_ref as forms
from oracle import volt_oracle as vo

gpu = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
DENSE = [(8, 5), (130, 129)]                    # (N, k): one padded tile; two block columns, ragged, the pivot in the second
FIRST = [(F32, None), (F64, None), (F32, 1e-4), (F64, 1e-4)]
IDS = ["f32-default", "f64-default", "f32-1e-4", "f64-1e-4"]
EXHAUSTED = 3
WARN = "A not p.d., added jitter of {:.1e} to the diagonal"
GPYTORCH = "Matrix not positive definite after repeatedly adding jitter up to {:.1e}."
NAN_COUNT = "cholesky_cpu: 1 of {} elements of the {} tensor are NaN."


def first_rung(dtype, given):
    return given if given is not None else (1e-6 if dtype == F32 else 1e-8)


def table(s):
    """(case, c, the rung that works: None = the plain attempt, EXHAUSTED = none)."""
    return [("clean", None, None), ("rung0", 0.3 * s, 0), ("rung1", 3 * s, 1), ("rung2", 30 * s, 2), ("exhausted", 1.0, EXHAUSTED)]


def expect(rung, s, tables):
    """(the jitter used, the warning's text or None, the calls of the entry)."""
    if rung is None:
        return 0.0, None, [(0.0, tables)]
    tried = [s * (10 ** i) for i in range(min(rung, 2) + 1)]
    calls = [(0.0, tables)] + [(j, tables) for j in tried]
    return (None, None, calls) if rung == EXHAUSTED else (tried[-1], WARN.format(tried[-1]), calls)


def observe(fn):
    """(result, exception, [(category, text)] of the numerical and library warnings)."""
    from volt_amd import _lib, gp
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        try:
            out, err = fn(), None
        except Exception as e:                                     # noqa: BLE001 -- the exception is what is looked at
            out, err = None, e
    return out, err, [(w.category, str(w.message)) for w in rec if issubclass(w.category, (gp.NumericalWarning, _lib.VoltHipWarning))]


def check(got, rung, s, calls, tables, exhausted, what):
    """One case against the table; returns (result, jitter used)."""
    from volt_amd import gp
    out, err, warned = got
    used, text, want = expect(rung, s, tables)
    print(f"{what}: calls {calls}, warned {warned}, raised {err!r}")
    assert calls == want, what
    if rung == EXHAUSTED:
        assert type(err) is gp.NotPSDError and str(err) == exhausted and warned == [], what
    else:
        assert err is None and warned == ([] if text is None else [(gp.NumericalWarning, text)]), what
    return out, used


def check_nan(got, calls, tables, text, what):
    from volt_amd import gp
    _, err, warned = got
    print(f"{what}: calls {calls}, warned {warned}, raised {err!r}")
    assert type(err) is gp.NanError and str(err) == text and warned == [] and calls == [(0.0, tables)], what


@pytest.fixture
def counted(monkeypatch):
    """counted(name): wraps ops.<name>; the list it returns gets the (jitter, tables) of every call (tables None: no such argument)."""
    def wrap(name):
        from volt_amd import ops
        real, calls = getattr(ops, name), []
        sig = inspect.signature(real)

        def entry(*a, **kw):
            bound = sig.bind(*a, **kw)
            bound.apply_defaults()
            calls.append((float(bound.arguments["jitter"]), bound.arguments.get("tables")))
            return real(*a, **kw)
        monkeypatch.setattr(ops, name, entry)
        return calls
    return wrap


def dense(N, k, c, B, dtype, device="cuda"):
    """A = I [B,N,N] with A[B // 2, k, k] = -c (c None: the identity)."""
    A = torch.eye(N, dtype=dtype, device=device).repeat(B, 1, 1)
    if c is not None:
        A[B // 2, k, k] = -c
    return A


# ------------------------------------------------------------------------------------------------ the table itself, on the host
@pytest.mark.parametrize("N,k", DENSE)
@pytest.mark.parametrize("dtype,given", FIRST, ids=IDS)
def test_the_oracle_lands_every_dense_case_on_its_rung(N, k, dtype, given):
    s = first_rung(dtype, given)
    for case, c, rung in table(s):
        A = dense(N, k, c, 1, dtype, "cpu")[0].numpy()
        used = expect(rung, s, True)[0]
        if rung == EXHAUSTED:
            with pytest.raises(np.linalg.LinAlgError):
                vo.psd_safe_cholesky(A, given)
        else:
            L, got = vo.psd_safe_cholesky(A, given)
            assert got == used and L.dtype == A.dtype, (case, got, used)
            assert abs(L[k, k] ** 2 - (1.0 if c is None else used - c)) <= 1e-5 * (1.0 if c is None else used - c), case
    A[2, 2] = np.nan
    with pytest.raises(FloatingPointError):
        vo.psd_safe_cholesky(A, given)


# ------------------------------------------------------------------------------------------------ ops.potrf
@gpu
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N,k", DENSE)
@pytest.mark.parametrize("dtype,given", FIRST, ids=IDS)
def test_safe_factor_walks_the_table(counted, N, k, B, dtype, given):
    from volt_amd import gp
    calls, s = counted("potrf"), first_rung(dtype, given)
    for case, c, rung in table(s):
        A = dense(N, k, c, B, dtype)
        del calls[:]
        got = observe(lambda: gp._safe_factor(A, given))
        out, used = check(got, rung, s, calls, True, GPYTORCH.format(s * (10 ** 2)), f"_safe_factor {case}")
        if rung != EXHAUSTED:
            f, jit = out
            assert jit == used and f.L.dtype == dtype and not f.info.any()
            pivot = 1.0 if c is None else used - c                 # L = I but for L[k,k]^2 = jitter - c (I + jitter elsewhere)
            assert abs(float(f.L[B // 2, k, k]) ** 2 - pivot) <= 1e-5 * pivot, case
    # psd_safe_cholesky is the same route: dense L in A's shape and dtype
    A = dense(N, k, 3 * s, B, dtype)
    del calls[:]
    got = observe(lambda: gp.psd_safe_cholesky(A[0] if B == 1 else A, jitter=given))
    L, _ = check(got, 1, s, calls, True, None, "psd_safe_cholesky rung1")
    assert L.dtype == dtype and L.shape == (A[0] if B == 1 else A).shape
    A[B // 2, 2, 2] = float("nan")
    del calls[:]
    check_nan(observe(lambda: gp._safe_factor(A, given)), calls, True, NAN_COUNT.format(A.numel(), tuple(A.shape)), "_safe_factor NaN")


# ------------------------------------------------------------------------------------------------ ops.mll_step
@gpu
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N,k", DENSE)
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_the_mll_walks_the_table(counted, N, k, B, dtype):
    """K = A - sigma^2 I with the likelihood's noise at its floor, so that the step factors A (the cancellation leaves the bad
    pivot at -c to 2^-23 of the floor 1e-4, 7e-12, against a nearest miss of 0.7 s >= 7e-9).  The step has no given first rung."""
    from volt_amd import gp
    calls, s = counted("mll_step"), first_rung(dtype, None)
    lh = gp.GaussianLikelihood().cuda().to(dtype)
    lh.noise_covar.raw_noise.data.fill_(-30.0)
    floor = lh.noise.detach().to(dtype).reshape(()) * torch.eye(N, dtype=dtype, device="cuda")
    mll = gp.ExactMarginalLogLikelihood(lh, None)
    zeros = torch.zeros((B, N) if B > 1 else (N,), dtype=dtype, device="cuda")

    def run(A):
        return mll(gp.MultivariateNormal(zeros, (A if B > 1 else A[0]) - floor), zeros)
    for case, c, rung in table(s):
        A = dense(N, k, c, B, dtype)
        del calls[:]
        val, _ = check(observe(lambda: run(A)), rung, s, calls, True,
                       f"K + sigma^2 I not positive definite for 1 of {B} series after jitter (first failing pivot {k + 1})", f"mll {case}")
        if rung != EXHAUSTED:
            assert val.dtype == dtype and bool(torch.isfinite(val).all()), case
    A = dense(N, k, None, B, dtype)
    A[B // 2, 2, 2] = float("nan")
    del calls[:]
    check_nan(observe(lambda: run(A)), calls, True, "cholesky: NaN in the covariance, the noise or the residual", "mll NaN")


# ------------------------------------------------------------------------------------------------ ops.vk_forms
@gpu
@pytest.mark.parametrize("dtype,given", FIRST, ids=IDS)
def test_safe_forms_walks_the_table(counted, dtype, given):
    """The three increasing grids of test_gpu_predict_linear's ladder test; grid 1 steps down by c at point 41."""
    from volt_amd import gp
    calls, s = counted("vk_forms"), first_rung(dtype, given)
    V, _, r = vk.mixed_case(130, 70, 0)
    keep = [b for b in range(12) if (np.diff(V[b], prepend=0.0) > 0).all()][:3]
    V3, r3 = torch.tensor(V[keep]).to(dtype), torch.tensor(r[keep]).to(dtype)
    for case, c, rung in table(s):
        Vc = V3.clone()
        if c is not None:
            Vc[1, 41] = Vc[1, 40] - c
        ok = [not forms.forms_ref(Vc.double().numpy(), j, r3.double().numpy())[1].any() for j in [0.0] + [s * (10 ** i) for i in range(3)]]
        assert ok == [rung is None] + [rung is None or i >= rung for i in range(3)], (case, ok)      # the restatement, first
        del calls[:]
        got = observe(lambda: gp._safe_forms(Vc.cuda(), r3.cuda(), given))
        out, used = check(got, rung, s, calls, None, GPYTORCH.format(s * (10 ** 2)), f"_safe_forms {case}")
        if rung != EXHAUSTED:
            assert out[1] == used and out[0].dtype == F64 and tuple(out[0].shape) == (3, 4) and bool(torch.isfinite(out[0]).all())
    Vn = V3.clone()
    Vn[0, 5] = float("nan")
    del calls[:]
    check_nan(observe(lambda: gp._safe_forms(Vn.cuda(), r3.cuda(), given)), calls, None, NAN_COUNT.format(Vn.numel(), tuple(Vn.shape)),
              "_safe_forms NaN")


# ------------------------------------------------------------------------------------------------ ops.markov_draw
@gpu
@pytest.mark.parametrize("dtype,given", FIRST, ids=IDS)
def test_safe_draw_walks_the_table(counted, dtype, given):
    """test_gpu_chain_draw's crafted chain (g = 1, c_k = 0.01 (k + 1)) with a step of -c at point 32; the default rung goes by
    ``f64``, the model's dtype, here the dtype of z."""
    from volt_amd import gp, ops
    calls, s = counted("markov_draw"), first_rung(dtype, given)
    H, i, S = 65, 32, 9
    z = torch.tensor(np.random.default_rng(3).standard_normal((1, S, H))).to(dtype).cuda()
    mean = torch.zeros(1, H, dtype=F64, device="cuda")

    def run(diag):
        d = torch.tensor(diag[None]).cuda()
        return gp._safe_draw(lambda j: ops.markov_draw(mean, d, d, z, j), (d, d, mean, z), given, f64=dtype == F64)
    for case, c, rung in table(s):
        diag = 0.01 * (1.0 + np.arange(H))
        if c is not None:
            diag[i] = diag[i - 1] - c
        cg = chain.markov_cg(diag, diag)
        piv = [chain.chain_pivots_ref(*cg, j) for j in [0.0] + [s * (10 ** n) for n in range(3)]]
        ok = [len(t) == H and bool((t > 0).all()) for t in piv]
        assert ok == [rung is None] + [rung is None or n >= rung for n in range(3)], (case, ok)        # the restatement, first
        del calls[:]
        out, used = check(observe(lambda: run(diag)), rung, s, calls, None, GPYTORCH.format(s * (10 ** 2)), f"_safe_draw {case}")
        if rung != EXHAUSTED:
            assert out[1] == used and out[0].dtype == dtype and tuple(out[0].shape) == (1, S, H) and bool(torch.isfinite(out[0]).all())
    diag = 0.01 * (1.0 + np.arange(H))
    diag[7] = np.nan
    del calls[:]
    check_nan(observe(lambda: run(diag)), calls, None, NAN_COUNT.format(H, (1, H)), "_safe_draw NaN")


# ------------------------------------------------------------------------------------------------ the 1x1 covariance (host)
@pytest.mark.parametrize("dtype,given", FIRST, ids=IDS)
def test_chol_1x1_walks_the_table(dtype, given):
    """No ops entry: the ladder runs on the tensor.  Its default first rung is 1e-6 whatever the dtype."""
    from volt_amd import gp
    from volt_amd.rollout_utils import _chol_1x1
    s = given if given is not None else 1e-6
    for case, c, rung in table(s):
        pc = torch.tensor([1.0, 1.0 if c is None else -c, 2.0], dtype=dtype).reshape(3, 1, 1)
        out, err, warned = observe(lambda: _chol_1x1(pc, given))
        used, text, _ = expect(rung, s, None)
        if rung == EXHAUSTED:
            assert type(err) is gp.NotPSDError and str(err) == "predictive covariance not positive definite after adding jitter" and warned == []
        else:
            assert err is None and warned == ([] if text is None else [(gp.NumericalWarning, text)]), case
            assert out.dtype == dtype and torch.equal(out, (pc + used).sqrt() if used else pc.sqrt()), case
    _, err, warned = observe(lambda: _chol_1x1(torch.tensor([[[float("nan")]]], dtype=dtype), given))
    assert type(err) is gp.NanError and str(err) == "cholesky: NaN in the predictive covariance" and warned == []


# ------------------------------------------------------------------------------------------------ a quirk that is kept
@gpu
def test_safe_factor_starts_a_half_precision_input_at_the_fp64_rung(counted):
    """`_safe_factor` factors a half-precision input in fp32 but picks its default rung by ``A.dtype == float32``: 1e-8.  With
    c = 2^-24 (a half-precision number) the fp64 ladder succeeds at 1e-7; the fp32 ladder would have at 1e-6."""
    from volt_amd import gp
    calls = counted("potrf")
    A = dense(8, 5, 2.0 ** -24, 1, torch.float16)
    (f, jit), _ = check(observe(lambda: gp._safe_factor(A)), 1, 1e-8, calls, True, None, "_safe_factor half")
    assert jit == 1e-8 * (10 ** 1) and f.L.dtype == F32
