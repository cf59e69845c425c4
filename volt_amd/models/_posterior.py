"""What the posteriors of BMGP and MultitaskBMGP share: both condition T independent chains over one grid.
The models differ in where the chain inputs come from (`Chains`: the kernel and the likelihood, or the Kronecker prologue)
and in how the per-chain result m_j [T,H], C_j [T,H,H] is assembled (the posterior itself, or scaled by kappa_j and mixed
through V); the option check, the failure report, the sweep and the dense factor-and-product sequence are here, once."""
from typing import NamedTuple

import torch

from .. import ops
from ..gp import _MarkovCov, check_grid
from ..safe import NanError, NotPSDError, _safe_factor

SOLVERS = ("dense", "linear")
POSTERIORS = ("solve", "sweep", "chain")


class Chains(NamedTuple):
    """The chains to condition on: K_j = vol_j min(x, x') + sigma2_j I with residual resid_j, and what a failure report says."""
    x: torch.Tensor                           # [N] the grid, fp64
    vol: torch.Tensor                         # [T]
    sigma2: torch.Tensor                      # [T]
    resid: torch.Tensor                       # [T,N] fp64
    who: str                                  # the model's name
    params: tuple                             # tensors looked at only on failure
    nan: str                                  # what a NaN / inf among them is called
    not_psd: str                              # what a failed pivot is called


def check_options(who, solver, posterior, grid=None, kernel="bm"):
    """``posterior`` against ``solver``; with ``grid`` (a model's constructor: the drivers, which check before any model is
    built, pass none) also the solver's name and what solver="linear" needs of the kernel and the training grid -- 1-D,
    x_0 >= 0, strictly increasing (ONE host read)."""
    if grid is not None and solver not in SOLVERS:
        raise ValueError(f"{who}: solver must be one of {SOLVERS}, got {solver!r}")
    if posterior not in POSTERIORS:
        raise ValueError(f"{who}: posterior must be one of {POSTERIORS}, got {posterior!r}")
    if posterior != "solve" and solver != "linear":
        raise ValueError(f"{who}: posterior={posterior!r} needs solver='linear' (the dense solver has one posterior)")
    if grid is not None and solver == "linear":
        if kernel != "bm":
            raise ValueError(f"{who}: solver='linear' needs kernel='bm' (Brownian motion is Markov; kernel {kernel!r} is not)")
        if grid.ndim != 1:
            raise ValueError(f"{who}(solver='linear'): the grid must be 1-D [N], got shape {tuple(grid.shape)}")
        check_grid(grid, f"{who}(solver='linear')")


def _sort_order(xs, order):
    """``order`` (the permutation that sorted xs), or None where xs was ascending already (ONE host read): the chain draw then
    skips the gather of z and the scatter of the result."""
    if xs.shape[0] < 2 or bool((xs[1:] >= xs[:-1]).all()):
        return None
    return order


def check_info(info, ch, order=None):
    """ONE host read of a chain launch's info (ops.bm_step, ops.bm_post).  NaN / inf parameters (``ch.params``) are a NanError
    before a failed pivot is a NotPSDError; a negative code of ops.bm_post names the offending test point by its index in the
    caller's order (``order``: the sort's permutation)."""
    info = info.tolist()
    if not any(info):
        return
    if not all(bool(torch.isfinite(p).all()) for p in ch.params):
        raise NanError(f"{ch.who} posterior: {ch.nan}")
    code = next(i for i in info if i)
    if code < 0 and order is not None:
        raise ValueError(f"{ch.who} posterior: test point {int(order[-code - 1])} is NaN / inf or negative "
                         "(Brownian motion starts at x = 0)")
    raise NotPSDError(f"{ch.who} posterior: {ch.not_psd}")


def sweep(ch, xs, lazy, dtype, scale=None, batched=True):
    """posterior="sweep" / "chain": ONE ops.bm_post launch over the sorted test points (any order and duplicates accepted: sorted
    on the device, the order restored on the way out) and one host read of its info; var = v xi_h - p_h, cov of neighbours
    = v xi_h - q_h, the rest by gp._MarkovCov (times ``scale`` [T]), fp64 throughout and rounded once to ``dtype``.  Returns
    (m [T,H] fp64 in the caller's order, the covariance): ``lazy`` leaves it a _MarkovCov (one more host read, `_sort_order`),
    else the same object evaluated.  Not ``batched``: the covariance of the one chain, [H,H]."""
    xs64, order = torch.sort(xs.double())
    out, info = ops.bm_post(ch.x, xs64, ch.vol, ch.sigma2, ch.resid)
    check_info(info, ch, order)
    prior = ch.vol.double().reshape(-1, 1) * xs64
    diag, off = prior - out[:, 1], prior - out[:, 2]
    m = torch.empty_like(diag)
    m[:, order] = out[:, 0]
    if not batched:
        diag, off = diag[0], off[0]
    cov = _MarkovCov(diag, off, _sort_order(xs, order) if lazy else order, scale=scale, dtype=dtype)
    return m, cov if lazy else cov.evaluate()


def dense_products(A, Kst, r):
    """The dense posterior's products from A = L L' [T,N,N] on the HIP potrf (psd_safe_cholesky's ladder), L^-1 from the HIP
    triangular inverse and the library GEMM: G = K_*t L^-T, w = (L^-1 r)' -> (G w [T,H,1] = K_*t A^-1 r, G G' = K_*t A^-1 K_t*)."""
    f, _ = _safe_factor(A)
    Linv = ops.trtri(f).mT.contiguous()                                                # L^-1, rows K-contiguous
    G = ops.gemm_nt(Kst, Linv, uplo_b=1)
    w = ops.gemm_nt(r, Linv, uplo_b=1)
    return ops.gemm_nt(G, w), ops.gemm_nt(G, G)
