"""The failure policy of every factorising route, once: gpytorch's ``psd_safe_cholesky``.  Try the route plain;
on a failed pivot look for NaN (`check_nan`); retry with jitter * 10^i from `default_jitter`, warn at the first rung that works,
NotPSDError when they run out (`jitter_ladder`).  An internal code of the library is no pivot failure: `rerun_table_free`.  The
routes below and gp._ExactMLL are an attempt, NaN inputs and texts on top of these; what one does differently is written at it."""
import warnings

import torch

from . import ops


class NotPSDError(RuntimeError):
    pass


class deferred_checks:
    """Context in which the factorisation's per-matrix ``info`` is NOT read back on the host after every step (that
    read is a device synchronisation, and it makes a training iteration impossible to capture in a hipGraph) but
    OR-ed into a device-side accumulator; ``any_bad()`` / ``raise_if_bad()`` read it when the caller chooses.  The
    training loops of train_utils use it (graph-captured loops, and the batched eager loops, which check every few
    iterations and replay from a snapshot with gpytorch's jitter ladder when a step failed).

    ``immediate = True`` keeps the per-step host check (and the ladder) while still sizing the accumulators: one
    accumulator per (length, device) of ``info``, so an iteration that factors batches of different shapes (an MLL
    step and a GPCV step, two models) keeps every flag, and nothing is allocated -- or re-zeroed on replay -- inside
    a graph capture: run one iteration with ``immediate = True`` under the context first."""
    _active = None

    def __init__(self, immediate=False):
        self.immediate = immediate
        self._acc = {}

    def __enter__(self):
        self._prev = deferred_checks._active
        deferred_checks._active = self
        return self

    def __exit__(self, *exc):
        deferred_checks._active = self._prev
        return False

    @classmethod
    def deferring(cls):
        """The active context if it is deferring the check, else None."""
        a = cls._active
        return a if a is not None and not a.immediate else None

    def _slot(self, info):
        flat = info.reshape(-1)
        key = (flat.shape[0], flat.device)
        acc = self._acc.get(key)
        if acc is None:
            if flat.is_cuda and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("deferred_checks: no accumulator for this info shape yet -- run one iteration with "
                                   "immediate=True under the context before capturing")
            acc = self._acc[key] = torch.zeros_like(flat)
        return acc, flat

    def reserve(self, info):
        self._slot(info)

    def note(self, info):
        acc, flat = self._slot(info)
        acc.bitwise_or_(flat)                            # one launch per step; non-zero once any step failed

    @classmethod
    def settle(cls, *infos) -> bool:
        """The protocol every step follows once its ``info`` words are on the device.  While deferring: OR each into its
        accumulator and return False -- no allocation and no host read, so the step can be captured.  Otherwise: size the
        accumulators if a context is active (``immediate``) and return True -- the caller reads ``info`` on the host now."""
        chk = cls._active
        if chk is not None:
            for info in infos:
                (chk.reserve if chk.immediate else chk.note)(info)
        return chk is None or chk.immediate

    def clear(self):
        for acc in self._acc.values():
            acc.zero_()

    def any_bad(self) -> int:
        """Number of matrices with a failed factorisation since the last clear() -- ONE host read."""
        if not self._acc:
            return 0
        return int(torch.stack([(a != 0).sum() for a in self._acc.values()]).sum().item())

    def raise_if_bad(self):
        nbad = self.any_bad()
        if nbad and any(bool((a < 0).any().item()) for a in self._acc.values()):
            # (the accumulators OR the steps' info words: a negative one holds an internal code -- INT_MIN, INT_MIN + 1 --, not a pivot)
            raise ops._lib.VoltHipError("a factorisation reported an INTERNAL error (hand-off time-out / workspace table) while "
                                        "the check was deferred; rerun without deferral: the step is then re-run on the "
                                        "launch-per-column schedule")
        if nbad:
            raise NotPSDError(f"{nbad} matrices failed a factorisation while the check was deferred (not positive "
                              "definite); rerun without deferral to get gpytorch's jitter-retry behaviour")


class NanError(RuntimeError):
    pass


class NumericalWarning(RuntimeWarning):
    pass


# ------------------------------------------------------------------------------------ the policy
def default_jitter(f64: bool, given=None) -> float:
    """The first rung: the caller's (``given``), else gpytorch's 1e-6 for an fp32 route and 1e-8 for an fp64 one, by ITS test."""
    return given if given is not None else 1e-8 if f64 else 1e-6


def info_failed(info: torch.Tensor, internal=None) -> bool:
    """Whether any entry of a route's ``info`` is non-zero -- the ONE host read of an attempt.  ``internal``: the text of the
    VoltHipError that an internal code in it raises first (one more read), for the rungs of a route that has such codes."""
    if internal is not None and ops.info_internal(info):
        raise ops._lib.VoltHipError(internal(info))
    return bool((info != 0).any().item())


def check_nan(tensors, message=None, shape=None):
    """NanError for the first of ``tensors`` that holds a NaN (non-tensors are skipped; one host read per tensor looked at),
    with the caller's ``message``, else gpytorch's count of the NaNs (``shape``: the shape it names, if not the tensor's)."""
    for t in tensors:
        if torch.is_tensor(t) and torch.isnan(t).any():
            raise NanError(message or f"cholesky_cpu: {int(torch.isnan(t).sum())} of {t.numel()} elements of the "
                                      f"{tuple(t.shape if shape is None else shape)} tensor are NaN.")


def jitter_ladder(attempt, failed, first, max_tries=3, exhausted=None):
    """``attempt(first * 10^i)`` for i = 0 .. max_tries - 1 until ``failed(result)`` is False: warns with the rung that worked
    and returns (result, that rung); NotPSDError with ``exhausted`` (default: gpytorch's text, naming the last rung) otherwise."""
    for i in range(max_tries):
        jitter_new = first * (10 ** i)
        result = attempt(jitter_new)
        if not failed(result):
            warnings.warn(f"A not p.d., added jitter of {jitter_new:.1e} to the diagonal", NumericalWarning)
            return result, jitter_new
    raise NotPSDError(exhausted or f"Matrix not positive definite after repeatedly adding jitter up to {jitter_new:.1e}.")


def rerun_table_free(run, info_of, warning, error):
    """For a result whose info holds an internal code, which never enters the ladder: warn, return ``run(tables=False)`` -- the
    launch-per-column schedule of the same entry point --, and raise VoltHipError(``error(info)``) if that has one too."""
    warnings.warn(warning, ops._lib.VoltHipWarning)
    result = run(tables=False)
    if ops.info_internal(info_of(result)):
        raise ops._lib.VoltHipError(error(info_of(result)))
    return result


def _plain_then_ladder(attempt, failed, nan_inputs, nan_text, first, max_tries=3, exhausted=None):
    """The whole policy of a route without internal codes: (result, the jitter used), 0.0 where the plain attempt worked."""
    result = attempt(0.0)
    if not failed(result):
        return result, 0.0
    check_nan(nan_inputs, nan_text)
    return jitter_ladder(attempt, failed, first, max_tries, exhausted)


# ------------------------------------------------------------------------------------ the routes
def psd_safe_cholesky(A, upper=False, out=None, jitter=None, max_tries=3):
    """gpytorch.utils.cholesky.psd_safe_cholesky on the HIP potrf (`_safe_factor`).  Returns dense L."""
    L = _safe_factor(A, jitter, max_tries)[0].L.reshape(A.shape)
    return L.transpose(-1, -2) if upper else L


def _safe_factor(A, jitter=None, max_tries=3):
    """The policy around the HIP potrf, in A's dtype (fp32 or fp64; anything else is computed in fp32): (ops.CholeskyFactor, the
    jitter used).  Kept as they are: the default rung goes by ``A.dtype == float32``, so a half-precision input, factored in
    fp32, starts at the fp64 rung; and after a fall-back to the launch-per-column schedule the rungs of this call stay on it."""
    A3 = A.reshape(-1, A.shape[-1], A.shape[-1])
    if A3.dtype != torch.float64:
        A3 = A3.to(torch.float32)
    f = ops.potrf(A3)
    if not info_failed(f.info):
        return f, 0.0
    tables = not ops.info_internal(f.info)
    if not tables:
        f = rerun_table_free(lambda tables: ops.potrf(A3, tables=tables), lambda f: f.info,
                             f"volt_potrf reported an internal error (info = {f.info.tolist()[:4]} ...) on its one-launch "
                             "schedule; re-run on the launch-per-column schedule",
                             lambda info: f"volt_potrf: internal error on both schedules, info = {info.tolist()[:8]}")
        if not info_failed(f.info):
            return f, 0.0
    check_nan((A3,), shape=A.shape)
    internal = lambda info: f"volt_potrf: internal error, info = {info.tolist()[:8]}"
    return jitter_ladder(lambda j: ops.potrf(A3, jitter=j, tables=tables), lambda f: info_failed(f.info, internal),
                         default_jitter(A.dtype != torch.float32, jitter), max_tries)


def _safe_draw(draw, inputs=(), jitter=None, max_tries=3, f64=False):
    """The policy around a chain draw (ops.markov_draw / ops.vk_draw): ``draw(j) -> (out, info)``, plain first (j = 0), then
    one jitter for the whole batch; the default rung is the fp32 one unless ``f64`` (an fp64 model).  ``inputs``: the tensors
    looked at for NaN on a failure.  Returns (out, the jitter used)."""
    (out, _), used = _plain_then_ladder(draw, lambda res: info_failed(res[1]), inputs, None, default_jitter(f64, jitter), max_tries)
    return out, used


def _safe_forms(V, resid, jitter=None, max_tries=3):
    """`_safe_draw` around ops.vk_forms: the conditioning scalars of the train block A = V[min(i,j)] + j I that the dense
    route gets from a factorisation, in O(N).  The default rung goes by resid's dtype; only V is looked at for NaN.  V [N] or
    [G,N], resid [G,N].  Returns (out [G,4] fp64 = V'A^-1 V, V'A^-1 r, r'A^-1 r, logdet A; the jitter used)."""
    return _safe_draw(lambda j: ops.vk_forms(V, j, resid), (V,), jitter, max_tries, resid.dtype == torch.float64)


def _chol_1x1(pc: torch.Tensor, jitter):
    """psd_safe_cholesky of a [...,1,1] matrix (rollout_utils.py:46): sqrt, with the ladder on the host.  Kept as they are:
    the default rung is the fp32 one whatever pc's dtype, and both errors have texts of their own."""
    pj, _ = _plain_then_ladder(lambda j: pc + j if j else pc, lambda p: not bool((p > 0).all()), (pc,),
                               "cholesky: NaN in the predictive covariance", default_jitter(False, jitter),
                               exhausted="predictive covariance not positive definite after adding jitter")
    return pj.sqrt()
