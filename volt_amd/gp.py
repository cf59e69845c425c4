"""Minimal stand-ins for the four gpytorch types the hot path touches, backed by the HIP library.

The reference's call sites are unchanged:

    likelihood = GaussianLikelihood()                               # train_utils.py:100,195
    mll = ExactMarginalLogLikelihood(likelihood, model)             # train_utils.py:127,240
    output = model(train_x)                                         # ExactGP.__call__ -> forward
    loss = -mll(output, train_y); loss.backward()                   # train_utils.py:249-250

gpytorch itself is third-party and absent from /root/reference; what is restated here (from its
published behaviour, gpytorch >= 1.0.1 per setup.py:19) is only the plumbing: parameter names and
registration order (the reference freezes parameters *positionally*, train_utils.py:226-227), the
``softplus + 1e-4`` noise constraint, input unsqueezing in ``ExactGP.__call__`` and the
``psd_safe_cholesky`` jitter policy.  The arithmetic -- K + sigma^2 I, Cholesky, solves, log-det,
gradient -- runs in libvolt_hip.so through one ``torch.autograd.Function``; there is no CPU path.
"""
from __future__ import annotations

import math
import threading

import torch
import torch.nn.functional as F
from torch import nn

from . import ops, safe
from .safe import (NanError, NotPSDError, NumericalWarning, deferred_checks,                  # noqa: F401 -- re-exported: the
                   psd_safe_cholesky, _safe_draw, _safe_factor, _safe_forms)                  # failure policy lives in safe.py


def same_values(a: torch.Tensor, b: torch.Tensor) -> bool:
    """``torch.equal(a, b)`` without its device synchronisation when the answer is known from the host side: two views
    of the same memory with the same layout hold the same values.  The reference's loops pass the stored training
    inputs back into ``model(train_x)`` on every iteration (train_utils.py:246), where each ``torch.equal`` on GPU
    tensors (VoltMagpie.py:122, EWMA.py:49) costs a full host-device round trip."""
    if (a.shape == b.shape and a.dtype == b.dtype and a.device == b.device and a.stride() == b.stride()
            and a.data_ptr() == b.data_ptr()):
        return True
    return a.shape == b.shape and torch.equal(a, b)


class EqualMemo:
    """Remembers that one particular tensor OBJECT compared equal to a stored tensor; valid while both version counters
    (bumped by any in-place write through any view) are unchanged.  Keyed on identity through a weak reference, never
    on addresses, so a new tensor that happens to reuse freed memory is always compared for real."""

    def __init__(self):
        self._ref, self._ver = None, None

    def equal(self, x: torch.Tensor, stored: torch.Tensor, compare) -> bool:
        held = self._ref() if self._ref is not None else None
        if held is x and self._ver == (x._version, stored._version):
            return True
        ok = bool(compare())
        if ok:
            import weakref
            self._ref, self._ver = weakref.ref(x), (x._version, stored._version)
        return ok


# ------------------------------------------------------------------------------------ modules
class Module(nn.Module):
    """gpytorch.Module stand-in: nn.Module plus ``register_prior`` (train_utils.py:158-159 puts a NormalPrior on the
    log-linear mean's slope; ExactMarginalLogLikelihood adds the log-priors / N like gpytorch does)."""

    def register_prior(self, name, prior, param_or_closure, setting_closure=None):
        if not hasattr(self, "_priors"):
            object.__setattr__(self, "_priors", {})
        if isinstance(param_or_closure, str) and not hasattr(self, param_or_closure):
            raise AttributeError(f"Unknown parameter {param_or_closure} for {type(self).__name__}")
        self._priors[name] = (prior, param_or_closure)

    def named_priors(self, prefix=""):
        for name, (prior, target) in getattr(self, "_priors", {}).items():
            closure = (lambda m, t=target: getattr(m, t)) if isinstance(target, str) else target
            yield prefix + name, self, prior, closure
        for cname, child in self.named_children():
            if isinstance(child, Module):
                yield from child.named_priors(prefix + cname + ".")


class NormalPrior:
    """gpytorch.priors.NormalPrior(loc, scale): log-density evaluated on the parameter's own device."""

    def __init__(self, loc, scale, validate_args=None, transform=None):
        self.loc, self.scale = float(loc), float(scale)

    def log_prob(self, x):
        return -0.5 * ((x - self.loc) / self.scale) ** 2 - math.log(self.scale) - 0.5 * math.log(2 * math.pi)


class Kernel(Module):
    """gpytorch.kernels.Kernel stand-in: ``kernel(x1, x2)`` calls ``forward`` and wraps the result
    so that ``.evaluate()`` (rollout_utils.py:26) works."""
    has_lengthscale = False

    def __init__(self, **kwargs):
        super().__init__()

    def __call__(self, *args, **kwargs):
        return _Evaluated(self.forward(*args, **kwargs))


class _Evaluated:
    """Already-dense "lazy tensor", and the base of the lazy ones: a subclass defines `_build(detach=False)` -- the dense
    tensor, from detached parameters when asked -- and ``shape``; ``tensor`` (read-only), ``evaluate``, ``to_dense`` and
    ``detach`` all come from that one hook, so nothing is formed before one of them is asked for."""

    def __init__(self, t):
        self._t = t

    def _build(self, detach=False):
        return self._t.detach() if detach else self._t

    @property
    def tensor(self):
        return self._build()

    @tensor.setter
    def tensor(self, v):
        raise AttributeError("read-only")

    def evaluate(self):
        return self._build()

    def to_dense(self):
        return self._build()

    def detach(self):
        return self._build(detach=True)

    @property
    def shape(self):
        return self._build().shape


class _ScaledDense(_Evaluated):
    """K = scale * base with a trainable scalar `scale` and a constant dense `base` (BMKernel: vol *
    min(x, x')).  Keeping the factorisation lets the MLL return d mll / d scale from the quantities
    the fused step already has (see _ExactMLL.backward) instead of a dense d mll / d K."""

    def __init__(self, scale, base):
        self.scale, self.base = scale, base

    def _build(self, detach=False):
        scale = self.scale.detach() if detach else self.scale
        # a batched kernel carries scale [T,1] over one shared base [N,N]
        return (scale.unsqueeze(-1) if scale.ndim > 1 else scale) * self.base

    @property
    def shape(self):
        return self.base.shape


class _BrownianPrior(_ScaledDense):
    """Lazy prior covariance of BMGP(solver="linear"): K = scale * min(x, x') over the 1-D grid ``x``, never formed --
    ExactMarginalLogLikelihood hands (scale, x) to the linear-time step (_ChainMLL, csrc/bm.hip).  min(x, x') is
    materialised only when ``.evaluate()`` / ``.to_dense()`` (or ``.base``) is asked for."""

    def __init__(self, scale, x):
        self.scale, self.x = scale, x

    @property
    def base(self):
        return torch.minimum(self.x.unsqueeze(-1), self.x.unsqueeze(-2))

    @property
    def shape(self):
        n = self.x.shape[-1]
        return torch.Size((n, n))


class _BrownianLevelPrior(_BrownianPrior):
    """Lazy prior of SingleTaskVariationalGP(prior_solver="markov"): Brownian motion started from an N(0, level) level,
    K_M = scale * min(x, x') + level 1 1' (increments of variance q_0 = scale x_0 + level, q_i = scale (x_i - x_{i-1})), never
    formed -- VariationalELBO hands (scale, x) to the O(N) step of csrc/gpcv_markov.hip.  NOT K + level I: a jitter on the
    starting level keeps K_M^-1 exactly tridiagonal.  Dense only when ``.evaluate()`` / ``.to_dense()`` is asked for."""

    def __init__(self, scale, x, level):
        self.scale, self.x, self.level = scale, x, level

    def _build(self, detach=False):
        return super()._build(detach) + self.level


def _markov_cov(diag, off):
    """The covariance [..,H,H] of a Markov process over H ordered points from its diagonal ``diag`` [..,H] and its first
    off-diagonal ``off`` [..,H] (off[.., j] = cov(j, j+1); the last entry is not read): cov(a, c) = diag_a prod_{a <= j < c} g_j
    with g_j = off_j / diag_j -- what the posterior of a Markov prior under independent noise is (BMGP(posterior="sweep")).
    fp64; the product is exp(L_c - L_a) over L = cumsum log g, never a ratio of cumulative products (which underflow).
    Where diag_j <= 0 (a point of zero variance: f(0) = 0) g_j := 0: that row and column are zero and nothing couples
    across it -- the zeros are counted beside L, not sent through the logarithm.  Symmetric by construction."""
    diag, off = diag.double(), off.double()
    H = diag.shape[-1]
    g = torch.where(diag > 0, off / torch.where(diag > 0, diag, torch.ones_like(diag)), torch.zeros_like(diag))
    g = g.clamp_min(0.0)[..., :H - 1]
    zero = g <= 0
    pad = torch.zeros_like(diag[..., :1])
    L = torch.cat([pad, torch.where(zero, torch.ones_like(g), g).log().cumsum(-1)], -1)           # L_0 = 0
    Z = torch.cat([pad, zero.to(torch.float64).cumsum(-1)], -1)                                   # zeros of g before each point
    dL = L.unsqueeze(-2) - L.unsqueeze(-1)                                                        # [a, c] = L_c - L_a
    upper = diag.clamp_min(0.0).unsqueeze(-1) * torch.exp(dL) * (Z.unsqueeze(-2) == Z.unsqueeze(-1))
    upper = torch.triu(upper)
    return upper + torch.triu(upper, 1).mT


class _MarkovCov(_Evaluated):
    """Lazy covariance of a Markov posterior over H points (BMGP / MultitaskBMGP(posterior="chain")):
    ``scale`` * _markov_cov(diag, off) over the points in ASCENDING order, with ``order`` the permutation that sorted the
    caller's points (None: they were ascending) -- what posterior="sweep" evaluates at once.  diag, off [..,H] fp64; scale None
    or [T] (the eigen-directions' kappa_j).  The [..,H,H] matrix is formed, through `_markov_cov`, only when ``.evaluate()`` /
    ``.to_dense()`` / ``.tensor`` is asked for, and rounded to ``dtype``; draws go through `draw`, which never forms it.

    Unsorted points: the chain runs over the sorted points, the N(0,1) number at the caller's position i drives the point at
    position i, and the result comes back in the caller's order: mean + P L_sorted P' z with P the sort's permutation.  For
    ascending points (what every driver passes) that is the dense route's mean + chol(C) z path by path; for other orders
    it has the same distribution but is a different root of C than chol(C) of the unsorted matrix."""

    def __init__(self, diag, off, order=None, scale=None, dtype=torch.float32, mean=None):
        self.diag, self.off, self.order, self.scale, self.dtype = diag, off, order, scale, dtype
        self.mean = mean                  # the posterior mean before its rounding to ``dtype`` (fp64, the caller's order), or None

    def _build(self, detach=False):                # (formed under no_grad from detached forms: nothing to detach)
        cov = _markov_cov(self.diag, self.off)
        if self.scale is not None:
            cov = self.scale.reshape(-1, 1, 1) * cov
        if self.order is not None:
            full = torch.empty_like(cov)
            full[..., self.order.unsqueeze(-1), self.order.unsqueeze(0)] = cov
            cov = full
        return cov.to(self.dtype)

    @property
    def shape(self):
        H = self.diag.shape[-1]
        return torch.Size((*self.diag.shape[:-1], H, H))

    def draw(self, mean, z, exp=False):
        """mean + L z for z [G,S,H] (G = the number of chains, 1 for an unbatched posterior) and mean [G,H] or None, both in
        the CALLER's order of the points, on ops.markov_draw under `_safe_draw`'s jitter ladder; [G,S,H] in z's dtype."""
        H = self.diag.shape[-1]
        diag, off = self.diag.reshape(-1, H), self.off.reshape(-1, H)
        if self.scale is not None:
            diag, off = self.scale.reshape(-1, 1) * diag, self.scale.reshape(-1, 1) * off
        mean = torch.zeros_like(diag) if mean is None else mean.reshape(-1, H).to(torch.float64)
        if self.order is not None:
            mean, z = mean[:, self.order], z[..., self.order]
        out, _ = _safe_draw(lambda j: ops.markov_draw(mean, diag, off, z, j, exp=exp), (diag, off, mean, z),
                            f64=self.dtype == torch.float64)
        if self.order is not None:
            back = torch.empty_like(out)
            back[..., self.order] = out
            out = back
        return out


def check_grid(x, who):
    """What the linear-time solvers (csrc/bm.hip, csrc/gpcv_bm.hip) need of their 1-D grid ``x``, checked once with ONE host
    read: x[0] >= 0 and strictly increasing.  ``who`` names the caller in the message."""
    if x.shape[0] > 1:
        first_ok, increasing = torch.stack([x[0] >= 0, (x[1:] > x[:-1]).all()]).tolist()
    else:
        first_ok, increasing = bool(x[0] >= 0), True
    if not first_ok:
        raise ValueError(f"{who}: the grid must start at x[0] >= 0")
    if not increasing:
        raise ValueError(f"{who}: the grid must be strictly increasing")


class _VolPrior(_Evaluated):
    """Lazy covariance of the data model with ``data_solver="linear"`` (models/_base.py): K[.., i, j] = V[.., min(i, j)] over
    the integrated squared vol path ``x`` = V ([N] or [B,N]), never formed -- ExactMarginalLogLikelihood hands V to the
    linear-time step (_ChainMLL, csrc/bm.hip).  K is filled only when ``.evaluate()`` / ``.to_dense()`` is asked for."""

    def __init__(self, V):
        self.x = V

    def _build(self, detach=False):
        return ops.fill(self.x.detach() if detach else self.x)

    @property
    def shape(self):
        n = self.x.shape[-1]
        return torch.Size((*self.x.shape[:-1], n, n))


def _dense(c):
    return c.evaluate() if isinstance(c, _Evaluated) else c


class Mean(Module):
    def __call__(self, x):
        if x.ndimension() == 1:          # gpytorch.means.Mean.__call__ adds the feature dimension to 1-D inputs
            x = x.unsqueeze(1)
        res = self.forward(x)
        return res


class ConstantMean(Mean):
    def __init__(self, batch_shape=torch.Size(), **kwargs):
        super().__init__()
        self.batch_shape = batch_shape
        self.register_parameter("constant", nn.Parameter(torch.zeros(*batch_shape, 1)))

    def forward(self, x):
        if x.shape[:-2] == self.batch_shape:
            return self.constant.expand(x.shape[:-1])
        if len(self.batch_shape) and x.ndim == 2:              # batched constant over shared inputs [N,1]
            return self.constant.expand(*self.batch_shape, x.shape[-2])
        return self.constant.expand(*x.shape[:-1]) if x.ndim > 1 else self.constant.expand(x.shape)


class LinearMean(Mean):
    def __init__(self, input_size, batch_shape=torch.Size(), bias=True):
        super().__init__()
        self.register_parameter("weights", nn.Parameter(torch.randn(*batch_shape, input_size, 1)))
        if bias:
            self.register_parameter("bias", nn.Parameter(torch.randn(*batch_shape, 1)))
        else:
            self.bias = None

    def forward(self, x):
        if x.ndim == 1:
            x = x.unsqueeze(-1)
        res = (x * self.weights.squeeze(-1).unsqueeze(-2)).sum(-1)     # x w over the (tiny) feature axis: elementwise, no BLAS
        if self.bias is not None:
            res = res + self.bias
        return res


class MultitaskMean(Mean):
    """gpytorch.means.MultitaskMean(base_means, num_tasks): one mean per task, stacked on a trailing task axis ([N,T]).
    A single base mean is deep-copied ``num_tasks - 1`` times (parameters ``base_means.<t>.*``), as gpytorch does."""

    def __init__(self, base_means, num_tasks):
        super().__init__()
        if isinstance(base_means, Mean):
            import copy
            base_means = [base_means] + [copy.deepcopy(base_means) for _ in range(num_tasks - 1)]
        if len(base_means) != num_tasks:
            raise RuntimeError("MultitaskMean: one base mean, or one per task")
        self.base_means = nn.ModuleList(base_means)
        self.num_tasks = num_tasks

    def forward(self, x):
        return torch.cat([m(x).unsqueeze(-1) for m in self.base_means], dim=-1)


class MultivariateNormal:
    """gpytorch.distributions.MultivariateNormal stand-in (VoltMagpie.py:127)."""

    def __init__(self, mean, covariance_matrix):
        self.loc = mean
        self._covar = covariance_matrix

    @property
    def mean(self):
        return self.loc

    @property
    def covariance_matrix(self):
        return _dense(self._covar)

    @property
    def lazy_covariance_matrix(self):
        return self._covar if isinstance(self._covar, _Evaluated) else _Evaluated(self._covar)

    @property
    def variance(self):
        return torch.diagonal(self.covariance_matrix, dim1=-2, dim2=-1)

    def _base_samples(self, sample_shape, base_samples):
        """``base_samples`` as given, else N(0, I) draws of shape sample_shape + loc.shape."""
        if base_samples is None:
            base_samples = torch.randn(torch.Size(sample_shape) + self.loc.shape, dtype=self.loc.dtype, device=self.loc.device)
        return base_samples

    def rsample(self, sample_shape=torch.Size(), base_samples=None):
        base_samples = self._base_samples(sample_shape, base_samples)
        if isinstance(self._covar, _MarkovCov):             # posterior="chain": O(S H), no H x H matrix (ops.markov_draw)
            H = self.loc.shape[-1]
            G = self.loc.numel() // H
            zb = base_samples.reshape(-1, G, H).transpose(0, 1).to(self.loc.dtype)         # [G,S,H] (a view when G = 1)
            out = self._covar.draw(self.loc if self._covar.mean is None else self._covar.mean, zb)   # (fp64 mean: ONE rounding, the output's)
            return out.transpose(0, 1).reshape(base_samples.shape)
        cov = self.covariance_matrix
        L = psd_safe_cholesky(cov)
        # loc + L z on the library GEMM: rows of z times L' (batched covariances: the batch leads the GEMM)
        H = L.shape[-1]
        if L.ndim == 2:
            lz = ops.gemm_nt(base_samples.reshape(-1, H), L, uplo_b=1).reshape(base_samples.shape)
        else:
            nb = L.numel() // (H * H)
            zb = base_samples.reshape(-1, nb, H).transpose(0, 1).contiguous()              # [T,S,H]
            lz = ops.gemm_nt(zb, L.reshape(nb, H, H), uplo_b=1).transpose(0, 1).reshape(base_samples.shape)
        return self.loc + lz.to(self.loc.dtype)

    def sample(self, sample_shape=torch.Size(), base_samples=None):
        with torch.no_grad():
            return self.rsample(sample_shape, base_samples)


class _KroneckerPrior:
    """Lazy prior covariance of MultitaskBMGP (training mode): K_x (x) K_t with K_x = vol * M, M = min(x_i, x_k) and
    K_t = F F' + diag(var) of ``covar_module`` (a MultitaskKernel over a BMKernel).  Element (n, t) of vec Y sits at n*T + t
    (gpytorch's interleaved order).  ExactMarginalLogLikelihood reads the raw parameters from it (the Kronecker step,
    _KronMLL); the dense matrix is built only on request.  ``M`` None (MultitaskBMGP(solver="linear")): M is never handed to
    the step -- the MLL runs on the linear-time chain (ops.kron_bm_step) over the grid ``x`` -- and min(x, x') is formed only
    when ``.evaluate()`` / ``.to_dense()`` (or ``.M`` itself) is asked for."""

    def __init__(self, covar_module, x, M=None):
        self.covar_module, self.x, self._M = covar_module, x, M

    @property
    def linear(self):
        return self._M is None

    @property
    def M(self):
        return torch.minimum(self.x.unsqueeze(-1), self.x.unsqueeze(-2)) if self._M is None else self._M

    def evaluate(self):
        vol = self.covar_module.data_covar_module.vol.reshape(())
        Kt = self.covar_module.task_covar_module.covar_matrix.evaluate()
        return torch.kron(vol * self.M.to(Kt.dtype), Kt)

    to_dense = evaluate

    @property
    def shape(self):
        n = self.x.shape[-1] * self.covar_module.num_tasks
        return torch.Size((n, n))


class MultitaskMultivariateNormal:
    """gpytorch.distributions.MultitaskMultivariateNormal stand-in for MultitaskBMGP (VoltMagpie.py:101-118 take
    ``.sample()`` / ``.mean`` of it).  ``mean`` is [n, T]; the joint covariance is over vec(mean) in gpytorch's interleaved
    order (element (n, t) at n*T + t).  Two forms:
      * a prior (``covariance_matrix`` a _KroneckerPrior or a dense [nT, nT] tensor): what ExactMarginalLogLikelihood takes;
      * a Kronecker posterior (``blocks=(V, C)``): cov = (I (x) V) blockdiag_j(C_j) (I (x) V'), V [T,T] = D^1/2 Q, C [T,n,n]
        (MultitaskBMGP.posterior_call).  A draw is mean + (L_j z_j)_j V' with L_j L_j' = C_j (HIP potrf), i.e. the root
        R[(h,t), (h',j)] = V[t,j] L_j[h,h'].
    ``base_samples`` (sample_shape + [n, T]): element [..., h, j] is the N(0,1) draw of block j at point h (posterior form);
    of vec position h*T + j of the dense root (prior form).  The dense ``covariance_matrix`` is built only when asked for."""

    def __init__(self, mean, covariance_matrix=None, blocks=None):
        self.loc = mean
        self._covar = covariance_matrix
        self._blocks = blocks
        self._root = None

    @property
    def mean(self):
        return self.loc

    @property
    def num_tasks(self):
        return self.loc.shape[-1]

    @property
    def event_shape(self):
        return self.loc.shape

    @property
    def lazy_covariance_matrix(self):
        return self._covar

    @property
    def covariance_matrix(self):
        if self._blocks is not None:
            V, C = self._dense_blocks()
            n, T = self.loc.shape
            return torch.einsum("tj,sj,jhk->htks", V, V, C).reshape(n * T, n * T)
        return _dense(self._covar)

    @property
    def variance(self):
        if self._blocks is not None:
            V, C = self._dense_blocks()
            return torch.einsum("jh,tj->ht", torch.diagonal(C, dim1=-2, dim2=-1), V * V)
        return torch.diagonal(self.covariance_matrix).reshape(self.loc.shape)

    def _dense_blocks(self):
        """(V, C [T,n,n]): a lazy C (gp._MarkovCov, posterior="chain") is densified here, on request only."""
        V, C = self._blocks
        return V, _dense(C)

    def root_blocks(self):
        """(V [T,T], L [T,n,n]) of the posterior form: L_j L_j' = C_j from the HIP potrf (psd_safe_cholesky's jitter policy)."""
        if self._blocks is None:
            raise ValueError("root_blocks: not a Kronecker posterior")
        if self._root is None:
            V, C = self._dense_blocks()
            self._root = (V, psd_safe_cholesky(C))
        return self._root

    def rsample(self, sample_shape=torch.Size(), base_samples=None):
        n, T = self.loc.shape
        shape = torch.Size(sample_shape) + self.loc.shape
        if base_samples is None:
            base_samples = torch.randn(shape, dtype=self.loc.dtype, device=self.loc.device)
        if tuple(base_samples.shape[-2:]) != (n, T):
            raise ValueError(f"base_samples must end in the mean's shape {tuple(self.loc.shape)}")
        if self._blocks is None:                                  # prior form: the dense root, on the HIP factorisation
            flat = MultivariateNormal(self.loc.reshape(-1), self.covariance_matrix)
            return flat.rsample(base_samples=base_samples.reshape(*base_samples.shape[:-2], n * T)).reshape(base_samples.shape)
        z = base_samples.reshape(-1, n, T).to(torch.float32)
        S = z.shape[0]
        if isinstance(self._blocks[1], _MarkovCov):          # posterior="chain": every L_j z_j from ONE ops.markov_draw launch, G = T
            lz = self._blocks[1].draw(None, z.permute(2, 0, 1).to(torch.float64))             # [T,S,n], kept in fp64 ...
            out = ops.markov_mix(lz, self._blocks[0], self.loc)                               # ... through V': ONE rounding, the output's
            return out.to(self.loc.dtype).reshape(base_samples.shape)
        V, L = self.root_blocks()
        lz = ops.gemm_nt(z.permute(2, 0, 1).contiguous(), L.to(torch.float32), uplo_b=1)      # [T,S,n]: (L_j z_j)'
        lz = lz.permute(1, 2, 0).reshape(S * n, T)
        out = self.loc + ops.gemm_nt(lz, V.to(torch.float32)).reshape(S, n, T).to(self.loc.dtype)
        return out.reshape(base_samples.shape)

    def sample(self, sample_shape=torch.Size(), base_samples=None):
        with torch.no_grad():
            return self.rsample(sample_shape, base_samples)


# --------------------------------------------------------------------------------- likelihood
class _NoiseCovar(Module):
    def __init__(self, batch_shape):
        super().__init__()
        self.register_parameter("raw_noise", nn.Parameter(torch.zeros(*batch_shape, 1)))


class GaussianLikelihood(Module):
    """noise = softplus(raw_noise) + 1e-4  (gpytorch default GreaterThan(1e-4) constraint).
    ``likelihood.raw_noise.data = torch.tensor([1e-5])`` (train_utils.py:222) => noise ~= 0.6933."""
    NOISE_FLOOR = 1e-4

    def __init__(self, batch_shape=torch.Size(), **kwargs):
        super().__init__()
        self.noise_covar = _NoiseCovar(batch_shape)

    @property
    def raw_noise(self):
        return self.noise_covar.raw_noise

    @raw_noise.setter
    def raw_noise(self, value):
        self.noise_covar.raw_noise = value

    @property
    def noise(self):
        return F.softplus(self.noise_covar.raw_noise) + self.NOISE_FLOOR

    @noise.setter
    def noise(self, value):
        value = torch.as_tensor(value, dtype=self.raw_noise.dtype, device=self.raw_noise.device)
        v = (value - self.NOISE_FLOOR).clamp_min(1e-12).expand_as(self.raw_noise)
        with torch.no_grad():
            self.noise_covar.raw_noise.copy_(v + torch.log(-torch.expm1(-v)))    # inverse softplus

    def forward(self, function_dist):
        """p(y|f): add the noise to the diagonal (dense; used outside the fused MLL only)."""
        cov = function_dist.covariance_matrix
        n = cov.shape[-1]
        noise = self.noise.reshape(*self.noise.shape[:-1], 1, 1)
        return MultivariateNormal(function_dist.mean, cov + noise * torch.eye(n, dtype=cov.dtype, device=cov.device))



def _inv_softplus_floor(value, like, floor):
    value = torch.as_tensor(value, dtype=like.dtype, device=like.device)
    v = (value - floor).clamp_min(1e-12).expand_as(like)
    return v + torch.log(-torch.expm1(-v))


class MultitaskGaussianLikelihood(Module):
    """gpytorch.likelihoods.MultitaskGaussianLikelihood(num_tasks, rank=0) stand-in (VoltMagpie.py:51-55 build it beside
    MultitaskBMGP).  Restated from gpytorch's published behaviour (not executed here; gpytorch is not installed):
    ``raw_task_noises`` [T] then ``raw_noise`` [1] are registered, both zeros, each through GreaterThan(1e-4), i.e.
    softplus(raw) + 1e-4; the noise covariance is I_n (x) diag(task_noises + noise).  ``likelihood.noise = v`` sets
    raw_noise to the constraint's inverse (VoltMagpie.py:54: 1e-3).  Only rank 0 with both noise terms is provided."""
    NOISE_FLOOR = 1e-4

    def __init__(self, num_tasks, rank=0, batch_shape=torch.Size(), task_prior=None, noise_prior=None, noise_constraint=None,
                 has_global_noise=True, has_task_noise=True):
        super().__init__()
        if rank != 0 or not (has_global_noise and has_task_noise) or task_prior is not None or noise_prior is not None:
            raise NotImplementedError("MultitaskGaussianLikelihood: rank 0 with task and global noise, no priors, is what "
                                      "the reference builds; nothing else is provided")
        self.register_parameter("raw_task_noises", nn.Parameter(torch.zeros(*batch_shape, num_tasks)))
        self.register_parameter("raw_noise", nn.Parameter(torch.zeros(*batch_shape, 1)))
        self.num_tasks, self.rank = num_tasks, rank

    @property
    def noise(self):
        return F.softplus(self.raw_noise) + self.NOISE_FLOOR

    @noise.setter
    def noise(self, value):
        with torch.no_grad():
            self.raw_noise.copy_(_inv_softplus_floor(value, self.raw_noise, self.NOISE_FLOOR))

    @property
    def task_noises(self):
        return F.softplus(self.raw_task_noises) + self.NOISE_FLOOR

    @task_noises.setter
    def task_noises(self, value):
        with torch.no_grad():
            self.raw_task_noises.copy_(_inv_softplus_floor(value, self.raw_task_noises, self.NOISE_FLOOR))

    def forward(self, function_dist):
        """p(y|f): I_n (x) diag(d) added to the dense covariance (outside the Kronecker MLL only)."""
        cov = function_dist.covariance_matrix
        n = function_dist.mean.shape[0]
        d = (self.task_noises + self.noise).to(cov.dtype)
        return MultitaskMultivariateNormal(function_dist.mean, cov + torch.diag(d.repeat(n)))


# -------------------------------------------------------------------------------------- model
class ExactGP(Module):
    """gpytorch.models.ExactGP stand-in.  Registers ``likelihood`` first (so it is parameter 0 for
    the positional grad_flags of train_utils.py:226), stores 1-D inputs as [N,1] and passes
    unsqueezed inputs to ``forward`` exactly like gpytorch does."""

    def __init__(self, train_inputs, train_targets, likelihood):
        super().__init__()
        self.likelihood = likelihood
        if train_inputs is not None and torch.is_tensor(train_inputs):
            train_inputs = (train_inputs,)
        self.train_inputs = None if train_inputs is None else tuple(
            t.unsqueeze(-1) if t.ndimension() == 1 else t for t in train_inputs)
        self.train_targets = train_targets

    def __call__(self, *args, **kwargs):
        inputs = [a.unsqueeze(-1) if torch.is_tensor(a) and a.ndimension() == 1 else a for a in args]
        if self.training:
            return self.forward(*inputs, **kwargs)
        return self.posterior_call(*inputs, **kwargs)

    def posterior_call(self, *inputs, **kwargs):
        raise NotImplementedError(
            f"{type(self).__name__}: eval-mode model(x) (generic gpytorch posterior) is outside the accelerated path; "
            "use GeneratePrediction / Rollouts (voltron/rollout_utils.py) which this package does implement")


# --------------------------------------------------------------------------------------- MLL
class refine_alpha:
    """Opt-in context (``with gp.refine_alpha(): loss = -mll(model(x), y)``): the fp32 MLL step refines alpha = K_s^-1 (y - m)
    by one step of iterative refinement against K itself (VOLT_REFINE_ALPHA) -- for models whose mean has trainable
    parameters (d mll / d mean = alpha / N; voltron/train_utils.py:213-220) and that train to the noise floor, where any
    fp32 factorisation leaves alpha at cond * eps (the reference's own path included).  Default off: the step then does
    what the reference's fp32 path does.  Costs one more pass over K and two triangular solves per step.

    REQUIREMENT: the residual r - K_s alpha is formed against whole rows of the caller's K, so BOTH triangles of every K
    that passes through an MLL inside the context must hold the symmetric matrix (everywhere else the library reads the
    lower triangle only); the kernels of this package return full symmetric matrices.  fp32 only (an fp64 step ignores
    it: its alpha is at cond * eps64 already).  The switch is per THREAD (threading.local) and re-entrant: a context
    entered on one thread does not change what another thread's steps do."""
    _tls = threading.local()

    def __init__(self, on=True):
        self.on = on

    @staticmethod
    def active():
        return bool(getattr(refine_alpha._tls, "on", False))

    def __enter__(self):
        self._prev = refine_alpha.active()
        refine_alpha._tls.on = self.on
        return self

    def __exit__(self, *exc):
        refine_alpha._tls.on = self._prev
        return False


class _ExactMLL(torch.autograd.Function):
    """mll[b] = log N(y_b; m_b, K_b + s2_b I) / N  with analytic backward:
    d/d s2 = 1/2 (a'a - tr K_s^-1)/N,  d/d m = a/N,  d/d y = -a/N,  a = K_s^-1 (y - m)."""

    @staticmethod
    def forward(ctx, K, mean, noise, target, holder, scale=None):
        B, n = mean.shape
        want_dk = bool(ctx.needs_input_grad[0])       # kernels with trainable parameters (Matern / SM / FBM baselines)
        K = K.detach()
        need_grad = want_dk or any(ctx.needs_input_grad[1:4]) or (scale is not None and ctx.needs_input_grad[5])
        if K.dtype != torch.float64:                  # the caller's dtype is kept (VolKernel.py:28-33): fp32 or fp64 step
            K = K.to(torch.float32)
        dt = K.dtype
        if want_dk and dt != torch.float32:
            raise NotImplementedError("the dense d mll / d K path (FBM kernel) is fp32 only")
        ws = holder.workspace(B, n, need_grad, K.device, dt)
        resid = (target - mean).to(dt)
        noise = noise.to(dt)
        # gpytorch factors through psd_safe_cholesky: plain first, then its jitter ladder (safe.py), the jitter added inside
        # the fused step.  Unlike `_safe_factor`, the rungs go back to the one-launch schedule after a table-free re-run.
        run = lambda jitter=0.0, **kw: ops.mll_step(K, resid, noise, ws, want_grad=need_grad, jitter=jitter,
                                                    refine_alpha=refine_alpha.active(), **kw)
        out, alpha, info = run()
        bad = int((info != 0).sum().item()) if deferred_checks.settle(info) else 0
        if bad and ops.info_internal(info):
            # an internal code (include/volt_hip.h), not a pivot.  The fp64 step has no table-free schedule to re-run on.
            codes = sorted({int(v) & 0xffffffff for v in info[info <= ops._lib.INFO_INTERNAL_MAX].tolist()})
            if dt != torch.float32:
                raise ops._lib.VoltHipError(f"volt_mll_step_f64: internal error, info = {[hex(c) for c in codes]}")
            out, alpha, info = safe.rerun_table_free(
                run, lambda res: res[2],
                f"volt_mll_step_f32 reported an internal error (info = {[hex(c) for c in codes]}) on its one-launch "
                "schedule; the step was re-run on the launch-per-column schedule",
                lambda info: f"volt_mll_step_f32: internal error on both schedules, info = {info.tolist()}")
            bad = int((info != 0).sum().item())
        if bad:
            safe.check_nan((K, resid, noise), "cholesky: NaN in the covariance, the noise or the residual")
            internal = lambda info: f"volt_mll_step: internal error, info = {info.tolist()}"
            (out, alpha, info), _ = safe.jitter_ladder(
                run, lambda res: safe.info_failed(res[2], internal), safe.default_jitter(dt != torch.float32),
                exhausted=f"K + sigma^2 I not positive definite for {bad} of {B} series after jitter "
                          f"(first failing pivot {int(info[info != 0][0].item())})")
        ctx.n = n
        ctx.has_scale = scale is not None
        ctx.want_dk = want_dk
        if need_grad:
            # the step's outputs live in the workspace, which the next forward overwrites: ONE packed copy of what backward
            # needs ([B, 8 + N]: the scalars and alpha) instead of a clone per tensor -- the iteration of a short series is
            # launch-bound (profiles/r06/pipeline_kernel_stats.csv: ~45 tiny kernels beside a 0.13 ms step), every copy is one
            pk = torch.cat((out, alpha), dim=1)
            keep = lambda t: t.detach().clone() if t.is_leaf else t.detach()     # (computed tensors are fresh already)
            extra = (pk[:, 2:6], keep(noise), keep(scale)) if scale is not None else ()
            gk = (ops.mll_grad_k(ws),) if want_dk else ()       # 1/2 (a a' - K_s^-1) / N from the step's own Y = L^-T
            ctx.save_for_backward(pk[:, 1], pk[:, 8:], *gk, *extra)
            return pk[:, 0]
        return out[:, 0].clone()

    @staticmethod
    def backward(ctx, g):
        dsig, alpha = ctx.saved_tensors[:2]
        gm = g.unsqueeze(-1) * alpha / ctx.n
        gscale = gK = None
        rest = ctx.saved_tensors[2:]
        if ctx.want_dk:
            gK, rest = g.reshape(-1, 1, 1) * rest[0], rest[1:]
        if ctx.has_scale:
            gscale = _scale_grad(g, *rest, ctx.n)
        return gK, gm, g * dsig, -gm, None, gscale


def _scale_grad(g, q, noise, c, n):
    """g * d mll / d c for K = c M from the step's scalars q = (quad, logdet, tr K_s^-1, a'a) [B,4]:
    a'Ma = (r'a - s2 a'a)/c  and  tr(K_s^-1 M) = (N - s2 tr K_s^-1)/c."""
    quad, tr, aa = q[:, 0], q[:, 2], q[:, 3]
    gscale = (g * 0.5 * ((quad - noise * aa) - (n - noise * tr)) / (n * c.reshape(-1))).reshape(c.shape)
    if gscale.shape != c.shape:
        gscale = gscale.sum().reshape(c.shape)
    return gscale


class _ChainMLL(torch.autograd.Function):
    """_ExactMLL without K, on the linear-time step of csrc/bm.hip (fp64 arithmetic, two O(N) sweeps), for the two covariances
    that are Markov chains over a grid:
      * ``scale`` given: the Brownian-motion prior K_b = scale_b min(x, x'), ``grid`` = x [N] (ops.bm_step);
      * ``scale`` None: the volatility-kernel data model K_b = V_b[min(i, j)], ``grid`` = V, [N] or [B,N] (ops.vk_step); the vol
        path is frozen (no gradient with respect to V, no scale).
    Same value, same gradients -- d/d mean = a/N, d/d target = -a/N, d/d s2, and d/d scale from the closed form shared with
    _ExactMLL (_scale_grad).  No jitter ladder: the tridiagonal the step factors is SPD whenever s2 > 0, so a failed pivot is
    a NaN (NanError) or a non-positive noise (NotPSDError)."""

    @staticmethod
    def forward(ctx, mean, noise, target, holder, grid, scale):
        B, n = mean.shape
        need_grad = any(ctx.needs_input_grad[:3]) or ctx.needs_input_grad[5]
        dt = torch.float64 if mean.dtype == torch.float64 else torch.float32
        ws = holder.bm_workspace(B, n, grid.device, dt)
        resid = (target - mean).to(dt)
        noise = noise.to(dt)
        if scale is None:
            out, alpha, info = ops.vk_step(grid.detach(), noise, resid, ws, want_grad=need_grad)
        else:
            out, alpha, info = ops.bm_step(grid, scale.detach(), noise, resid, ws, want_grad=need_grad)
        if deferred_checks.settle(info):
            bad = int((info != 0).sum().item())
            if bad:
                if scale is None:
                    what, K, inputs = "volatility-kernel", "V[min(i, j)]", "the integrated vol path"
                else:
                    what, K, inputs = "Brownian-motion", "vol min(x, x')", "the grid, the scale"
                safe.check_nan((resid, noise, grid, scale), f"{what} MLL: NaN in {inputs}, the noise or the residual")
                raise NotPSDError(f"{K} + sigma^2 I not positive definite for {bad} of {B} series "
                                  f"(first failing pivot {int(info[info != 0][0].item())}): the noise must be positive")
        ctx.n = n
        if need_grad:
            pk = torch.cat((out, alpha), dim=1)          # the ONE saved tensor: [B, 8 + N], the scalars and alpha
            ctx.save_for_backward(pk)
            if scale is not None:
                ctx.scale_shape = scale.shape if scale.numel() == B else torch.Size((B,))
            return pk[:, 0]
        return out[:, 0].clone()

    @staticmethod
    def backward(ctx, g):
        (pk,) = ctx.saved_tensors                    # out[:, 6] = the noise, out[:, 7] = the scale the step used
        gm = g.unsqueeze(-1) * pk[:, 8:] / ctx.n
        gscale = _scale_grad(g, pk[:, 2:6], pk[:, 6], pk[:, 7].reshape(ctx.scale_shape), ctx.n) if ctx.needs_input_grad[5] else None
        return gm, g * pk[:, 1], -gm, None, None, gscale


class _KronMLL(torch.autograd.Function):
    """mll = log N(vec Y; vec mu, K_x (x) K_t + I (x) D) / (N T) of MultitaskBMGP and its gradient wrt the five raw
    parameters, from ONE prologue -> batched step (B = T over the shared M) -> epilogue sequence (ops.kron_mll_step,
    include/volt_hip.h; ``M`` None: ops.kron_bm_step, the same sequence around the linear-time chain step, which has no
    internal error codes).  No host read when the check is deferred, so the iteration captures into a hipGraph.
    Unlike _ExactMLL there is no jitter ladder: gpytorch would add jitter to the NT x NT matrix, which this path never
    forms; a failed factorisation (each M + sigma_j^2 I has sigma_j^2 = 1 / (vol lambda_j) > 0) raises NotPSDError."""

    @staticmethod
    def forward(ctx, raw_vol, covar_factor, raw_var, raw_task_noises, raw_noise, x, target, M, holder):
        params = (raw_vol, covar_factor, raw_var, raw_task_noises, raw_noise)
        n, T = target.shape
        if M is None:
            ws = holder.kron_workspace(n, T, target.device, target.dtype, "linear")
            res, info, eig_info, _ = ops.kron_bm_step(params, x, target, ws)
        else:
            ws = holder.kron_workspace(n, T, M.device, M.dtype)
            res, info, eig_info, _ = ops.kron_mll_step(params, x, target, M, ws)
        eig_bad = eig_info.clamp(max=0)                       # sweeps used >= 0; -1: the eigensolver hit its sweep cap
        if deferred_checks.settle(info, eig_bad):
            nbad, ebad, internal = torch.stack([(info != 0).sum(), (eig_bad != 0).sum(),
                                                (info <= ops._lib.INFO_INTERNAL_MAX).sum()]).tolist()
            if ebad:
                raise ops._lib.VoltHipError("volt_kron_prologue: the eigensolver of the task covariance did not converge")
            if internal:
                raise ops._lib.VoltHipError(f"volt_mll_step: internal error, info = {info.tolist()}")
            if nbad:
                if not bool(torch.isfinite(target).all()) or not all(bool(torch.isfinite(p).all()) for p in params):
                    raise NanError("Kronecker MLL: NaN / inf in the targets or the parameters")
                raise NotPSDError(f"M + sigma_j^2 I not positive definite for {nbad} of {T} eigen-directions")
        res = res.clone()                                     # the workspace is overwritten by the next forward
        ctx.save_for_backward(res)
        ctx.meta = [(p.shape, p.dtype) for p in params]
        return res[0].to(raw_vol.dtype)

    @staticmethod
    def backward(ctx, g):
        (res,) = ctx.saved_tensors
        T = (res.numel() - 3) // 3
        parts = (res[1:2], res[3:3 + T], res[3 + T:3 + 2 * T], res[3 + 2 * T:], res[2:3])
        grads = tuple((g * p).reshape(shape).to(dt) for p, (shape, dt) in zip(parts, ctx.meta))
        return (*grads, None, None, None, None)


class ExactMarginalLogLikelihood(Module):
    """gpytorch.mlls.ExactMarginalLogLikelihood stand-in: ``mll(model(x), y)`` returns the marginal
    log likelihood divided by the number of data points (a scalar, or [T] for a batched model)."""

    def __init__(self, likelihood, model):
        super().__init__()
        # plain attributes: gpytorch registers both as submodules, but nobody iterates mll.parameters()
        object.__setattr__(self, "likelihood", likelihood)
        object.__setattr__(self, "model", model)
        self._ws = None

    def workspace(self, B, n, want_grad, device, dtype=torch.float32):
        return ops.cached_workspace(self, "_ws", ops.MllWorkspace, B, n, want_grad, device, dtype)

    def bm_workspace(self, B, n, device, dtype=torch.float32):
        return ops.cached_workspace(self, "_bws", ops.BmWorkspace, B, n, device, dtype)

    def kron_workspace(self, n, T, device, dtype=torch.float32, solver="dense"):
        return ops.cached_workspace(self, "_kws", ops.KronWorkspace, n, T, device, dtype, solver)

    def _add_log_priors(self, res, num_data):
        """gpytorch: + sum log p(theta) / num_data over the model's registered priors."""
        priors = self.model.named_priors() if isinstance(self.model, Module) else ()
        for _, module, prior, closure in priors:
            res = res + prior.log_prob(closure(module)).sum() / num_data
        return res

    def _kron_forward(self, function_dist, target):
        """MultitaskBMGP's prior: the Kronecker step (_KronMLL).  ``target`` has the model's layout, [N, T]."""
        prior = function_dist.lazy_covariance_matrix
        if tuple(target.shape) != tuple(function_dist.mean.shape):
            raise ValueError(f"ExactMarginalLogLikelihood: target {tuple(target.shape)} does not have the multitask mean's "
                             f"shape {tuple(function_dist.mean.shape)} ([N, T], the layout the model was built with)")
        if not prior.x.is_cuda or not target.is_cuda:
            raise ops._lib.VoltHipError("ExactMarginalLogLikelihood: tensors must live on the MI355X; no CPU fallback")
        task, data = prior.covar_module.task_covar_module, prior.covar_module.data_covar_module
        lh = self.likelihood
        params = (data.raw_vol, task.covar_factor, task.raw_var, lh.raw_task_noises, lh.raw_noise)
        f64 = any(t.dtype == torch.float64 for t in (prior.x, target, *params))
        dt = torch.float64 if f64 else torch.float32           # torch's promotion of the reference's own arithmetic
        res = _KronMLL.apply(*params, prior.x, target.to(dt), None if prior.linear else prior.M.to(dt), self)
        return self._add_log_priors(res, target.numel())       # gpytorch: the MultitaskMultivariateNormal's event size

    def forward(self, function_dist, target):
        lazy = function_dist.lazy_covariance_matrix
        if isinstance(function_dist, MultitaskMultivariateNormal) and isinstance(lazy, _KroneckerPrior):
            return self._kron_forward(function_dist, target)
        mean = function_dist.mean
        n = mean.shape[-1]
        mean2, t2 = mean.reshape(-1, n), target.reshape(-1, n)
        B = mean2.shape[0]
        # the three priors differ in what stands for the covariance, the function applied to it and the dtype rule
        if isinstance(lazy, _VolPrior):
            # the data model with data_solver="linear": the linear-time step on per-series grids, in the integrated vol
            # path's dtype (the dense step computes in the covariance's, which is V's)
            V = lazy.x.reshape(-1, n)
            cov = V = V[0] if V.shape[0] == 1 else V         # [N]: one grid for all series
            if V.ndim == 2 and V.shape[0] != B:
                raise ValueError(f"ExactMarginalLogLikelihood: {V.shape[0]} vol paths for {B} series")
            f64 = V.dtype == torch.float64
            step = lambda *mean_noise_target: _ChainMLL.apply(*mean_noise_target, self, V, None)
        elif isinstance(lazy, _BrownianPrior):
            # BMGP(solver="linear"): the linear-time step, in the mean's dtype
            cov = lazy.x
            scale = lazy.scale.expand(B) if lazy.scale.numel() == 1 and B > 1 else lazy.scale
            f64 = mean.dtype == torch.float64
            step = lambda *mean_noise_target: _ChainMLL.apply(*mean_noise_target, self, lazy.x, scale)
        else:
            scale = None
            if isinstance(lazy, _ScaledDense):
                scale = lazy.scale
                K = lazy.detach()
            else:
                K = function_dist.covariance_matrix
            cov = K.reshape(-1, n, n)
            f64 = cov.dtype == torch.float64                 # computed in the covariance's dtype
            step = lambda *mean_noise_target: _ExactMLL.apply(cov, *mean_noise_target, self, scale)
        if not cov.is_cuda or not target.is_cuda:
            raise ops._lib.VoltHipError("ExactMarginalLogLikelihood: tensors must live on the MI355X; no CPU fallback")
        noise = self.likelihood.noise.reshape(-1)
        noise = noise.expand(B) if noise.numel() == 1 else noise
        dt = torch.float64 if f64 else torch.float32
        res = step(mean2.to(dt), noise.to(dt), t2.to(dt))
        res = res.reshape(mean.shape[:-1]) if mean.ndim > 1 else res.reshape(())
        return self._add_log_priors(res, n)


LOG_2PI = math.log(2 * math.pi)
