"""Variational-GP plumbing of the GPCV stage, backed by volt_gpcv_step_f32 ("exp" likelihood),
volt_gpcv_cv_step_f32 ("cv"), volt_gpcv_bm_step_f32 (either likelihood under the lazy Brownian-motion prior of
``SingleTaskVariationalGP(prior_solver="linear")``), volt_gpcv_markov_step_f32 (either likelihood, the Markov variational
family of ``prior_solver="markov"``: O(N) time and memory), volt_gpcv_mt_step_f32 (the multi-task model, "exp") and
volt_gpcv_mt_cv_step_f32 (the multi-task model, "cv" with one warp per task) and volt_gpcv_mt_markov_step_f32 (the multi-task
model with the Markov family of ``MultitaskVariationalGP(prior_solver="markov")``, either likelihood: O(N T)).
The two Markov models also answer AWAY from the inducing grid (``MarkovPredictiveLatent``, ``MultitaskMarkovPredictiveLatent``:
volt_markov_predict_plan_f32 / volt_markov_predict_draw_f32, O(N + S H)).

The reference builds this stage from gpytorch parts (voltron/train_utils.py:20-44,
voltron/models/single_task_variational_gp.py:69-122): ``CholeskyVariationalDistribution`` +
``UnwhitenedVariationalStrategy`` with the inducing points fixed at the training inputs, and
``VariationalELBO(likelihood, model, num_data, combine_terms=True)`` evaluated under
``num_gauss_hermite_locs(75)``.  gpytorch is third-party and absent from /root/reference; restated here
(from its published behaviour) is only what those call sites need:

* ``model(x)`` with ``x`` equal to the inducing points returns q(u) = N(m, Lq Lq') itself (the strategy's
  ``torch.equal(x, inducing_points)`` short cut); other inputs are outside the accelerated path;
* ``elbo = E_q[log p(y|f)].sum() / N - beta KL(q(u) || N(mean(Z), K(Z,Z) + 1e-3 I)) / num_data``;
* parameter names: ``variational_strategy._variational_distribution.{variational_mean,chol_variational_covar}``.

The arithmetic -- quadrature, Cholesky of the prior, the two triangular products behind tr(K^-1 S) and
K^-1 Lq, all gradients -- runs in libvolt_hip.so through one ``torch.autograd.Function``; no CPU path.
"""
from __future__ import annotations

import functools
import inspect
import math

import numpy as np
import torch
from torch import nn

from . import ops
from .gp import Module, MultivariateNormal, _BrownianLevelPrior, _BrownianPrior, _ScaledDense, _dense
from .safe import NotPSDError, check_nan, deferred_checks

PRIOR_JITTER = 1e-3        # LazyTensor.add_jitter() default on the inducing prior
MIN_VARIANCE = 1e-6        # gpytorch.settings.min_variance for fp32


class num_gauss_hermite_locs:
    """gpytorch.settings.num_gauss_hermite_locs (default 20): ``with num_gauss_hermite_locs(75): ...``."""
    _value = 20

    def __init__(self, value):
        self._new, self._old = int(value), None

    @classmethod
    def value(cls):
        return cls._value

    def __enter__(self):
        self._old, num_gauss_hermite_locs._value = num_gauss_hermite_locs._value, self._new
        return self

    def __exit__(self, *exc):
        num_gauss_hermite_locs._value = self._old
        return False


_GH_CACHE = {}


def _gauss_hermite(n, device, dtype=torch.float32):
    """GaussHermiteQuadrature1D's nodes and weights (numpy hermgauss), weights pre-divided by sqrt(pi)."""
    key = (n, str(device), dtype)
    if key not in _GH_CACHE:
        x, w = np.polynomial.hermite.hermgauss(n)
        _GH_CACHE[key] = (torch.tensor(x, dtype=dtype, device=device),
                          torch.tensor(w / math.sqrt(math.pi), dtype=dtype, device=device))
    return _GH_CACHE[key]


class CholeskyVariationalDistribution(Module):
    """q(u) = N(variational_mean, L L'), L = tril(chol_variational_covar); gpytorch initialises 0 / I."""

    def __init__(self, num_inducing_points, batch_shape=torch.Size(), **kwargs):
        super().__init__()
        self.variational_mean = nn.Parameter(torch.zeros(*batch_shape, num_inducing_points))
        self.chol_variational_covar = nn.Parameter(torch.eye(num_inducing_points).repeat(*batch_shape, 1, 1))


class UnwhitenedVariationalStrategy(Module):
    def __init__(self, model, inducing_points, variational_distribution, learn_inducing_locations=True):
        super().__init__()
        object.__setattr__(self, "model", model)
        if inducing_points.dim() == 1:
            inducing_points = inducing_points.unsqueeze(-1)
        if learn_inducing_locations:
            raise NotImplementedError("learn_inducing_locations=True is outside the accelerated path: LearnGPCV fixes "
                                      "the inducing points at the training inputs (train_utils.py:30)")
        self.register_buffer("inducing_points", inducing_points.detach().clone())
        self._variational_distribution = variational_distribution
        self.register_buffer("variational_params_initialized", torch.tensor(0))


class VariationalLatent(MultivariateNormal):
    """What ``model(train_x)`` returns: q(u) itself, tied to its model so the ELBO can reach the prior."""

    def __init__(self, model):
        dist = model.variational_strategy._variational_distribution
        self.model = model
        self.loc = dist.variational_mean
        self._chol = dist.chol_variational_covar

    @property
    def chol(self):
        return self._chol.tril()

    @property
    def _covar(self):
        L = self.chol.detach()
        return ops.gemm_nt(L, L, uplo_a=1, uplo_b=1)                 # S = L L'

    @property
    def variance(self):
        return self.chol.pow(2).sum(-1).clamp_min(MIN_VARIANCE)

    def rsample(self, sample_shape=torch.Size(), base_samples=None):
        """m + L eps, eps ~ N(0, I) of shape sample_shape + [N] (one series) -- CholLazyTensor's root is L itself."""
        base_samples = self._base_samples(sample_shape, base_samples)
        eps = base_samples.reshape(-1, self.loc.shape[-1]) if self.loc.ndim == 1 else base_samples
        if self.loc.ndim == 1:
            f = ops.gemm_nt(eps, self.chol.detach(), uplo_b=1)       # [S,N] = eps L'
            return self.loc.detach() + f.reshape(base_samples.shape)
        S = eps.reshape(-1, *self.loc.shape)                          # [S,B,N]
        f = ops.gemm_nt(S.transpose(0, 1).contiguous(), self.chol.detach(), uplo_b=1)   # [B,S,N]
        return self.loc.detach() + f.transpose(0, 1).reshape(base_samples.shape)


class MarkovVariationalDistribution(Module):
    """q(u) = N(variational_mean, P^-1) with a TRIDIAGONAL precision P = Lp Lp', Lp lower bidiagonal: diagonal
    exp(log_diag_precision_root), entry (i+1, i) coupling_i exp(log_diag_precision_root_i) -- 3 N numbers instead of the
    Cholesky family's N^2 / 2.  Under a Brownian prior and a likelihood that factorises over points the optimal Gaussian q has
    precision K^-1 + diag(lambda), which is tridiagonal: the family contains it.  No positivity constraint, no sign ambiguity,
    no pivot.  ``coupling`` is stored [.., N]; its last entry is unused and never read.  Initialised 0 / I like gpytorch."""

    def __init__(self, num_inducing_points, batch_shape=torch.Size(), **kwargs):
        super().__init__()
        self.variational_mean = nn.Parameter(torch.zeros(*batch_shape, num_inducing_points))
        self.log_diag_precision_root = nn.Parameter(torch.zeros(*batch_shape, num_inducing_points))
        self.coupling = nn.Parameter(torch.zeros(*batch_shape, num_inducing_points))

    def natural_sites(self):
        """(lam1, lam2) [B,N] fp64: the sites of ``VariationalELBO.natural_gradient_step`` (the optimal q has precision
        K_M^-1 + diag(lam2) and mean mu + P^-1 lam1).  Non-persistent buffers made at the first call, zeros
        (q = prior), on the parameters' device: a ``state_dict`` never holds them."""
        m = self.variational_mean
        n = m.shape[-1]
        for name in ("_natural_lam1", "_natural_lam2"):
            t = getattr(self, name, None)
            if t is None or t.device != m.device or t.numel() != m.numel() or t.dtype != torch.float64:
                self.register_buffer(name, torch.zeros(m.numel() // n, n, dtype=torch.float64, device=m.device), persistent=False)
        return self._natural_lam1, self._natural_lam2


class MarkovVariationalLatent(MultivariateNormal):
    """What ``SingleTaskVariationalGP(prior_solver="markov")(train_x)`` returns: q(u) of ``MarkovVariationalDistribution``,
    tied to its model.  ``variance`` and ``rsample`` are O(N) recurrences on the device (csrc/gpcv_markov.hip); the dense
    covariance is built only when ``_covar`` is asked for."""

    def __init__(self, model):
        dist = model.variational_strategy._variational_distribution
        self.model = model
        self.loc = dist.variational_mean
        self._rho, self._gamma = dist.log_diag_precision_root, dist.coupling

    def _flat(self):
        n = self.loc.shape[-1]
        return (t.detach().reshape(-1, n) for t in (self.loc, self._rho, self._gamma))

    @property
    def precision_root(self):
        """Lp [.., N, N], dense (tests and small problems only)."""
        d = self._rho.detach().double().exp()
        Lp = torch.diag_embed(d)
        if d.shape[-1] > 1:
            Lp = Lp + torch.diag_embed(self._gamma.detach().double()[..., :-1] * d[..., :-1], offset=-1)
        return Lp

    @property
    def _covar(self):
        Lp = self.precision_root
        return torch.linalg.inv(Lp @ Lp.mT).to(self.loc.dtype)

    @property
    def variance(self):
        """diag P^-1, clamped at MIN_VARIANCE.  DETACHED: unlike ``VariationalLatent.variance`` it carries no gradient to
        log_diag_precision_root / coupling (the recurrence runs in the HIP library) -- a direct caller of
        ``likelihood.expected_log_prob(y, latent)`` differentiates through the mean only; the gradients of the variational
        parameters come from ``VariationalELBO``, which is what the trainers use."""
        _, rho, gamma = self._flat()
        return ops.markov_root_var(rho, gamma).to(self.loc.dtype).reshape(self.loc.shape).clamp_min(MIN_VARIANCE)

    def rsample(self, sample_shape=torch.Size(), base_samples=None):
        """m + Lp^-T eps, eps ~ N(0, I) of shape sample_shape + loc.shape: one backward recurrence per draw."""
        base_samples = self._base_samples(sample_shape, base_samples)
        m, rho, gamma = self._flat()
        B, n = m.shape
        eps = base_samples.reshape(-1, B, n).transpose(0, 1)                                   # [B,S,N]
        f = ops.markov_root_draw(m, rho, gamma, eps)
        return f.transpose(0, 1).reshape(base_samples.shape).to(self.loc.dtype)


def _predict_points(x, who):
    """The test points of a prediction away from the grid as a flat [H] tensor: [H] or [H,1], finite, >= 0, any order."""
    if not torch.is_tensor(x) or x.ndim not in (1, 2) or (x.ndim == 2 and x.shape[-1] != 1) or x.numel() < 1:
        raise ValueError(f"{who}: test points must be [H] or [H,1] with H >= 1, got shape "
                         f"{tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}")
    xs = x.detach().reshape(-1)
    if not bool((torch.isfinite(xs) & (xs >= 0)).all()):
        raise ValueError(f"{who}: test points must be finite and >= 0 (the Brownian prior lives on x >= 0)")
    return xs


class MarkovPredictiveLatent(MultivariateNormal):
    """What ``SingleTaskVariationalGP(prior_solver="markov")(x)`` returns for ``x`` other than the inducing grid: q(f(x)), the
    Gauss-Markov q(u) carried through the Brownian prior's conditional -- a bridge between the neighbouring knots, free Brownian
    motion beyond the last one (csrc/markov_predict.hip).  ``loc`` / ``variance`` [.., H] come from ONE O(N + H)
    launch made here; ``rsample`` draws joint paths in O(H) each.  No N x N or H x H array exists unless ``_covar`` is asked for
    (tests and small H).  NO autograd: everything is detached -- the parameters' gradients come from ``VariationalELBO``."""

    def __init__(self, model, xs):
        latent = MarkovVariationalLatent(model)
        m, rho, gamma = latent._flat()
        Z = model.variational_strategy.inducing_points
        B = m.shape[0]
        mu = model.mean_module.constant.detach().reshape(-1)
        vol = model.covar_module.vol.detach().reshape(-1)
        if mu.numel() not in (1, B) or vol.numel() not in (1, B):
            raise ValueError("MarkovPredictiveLatent: the mean constant and the kernel's vol must be one value or one per series")
        self.model, self._batch, self._xs = model, latent.loc.shape[:-1], xs
        self.plan = ops.markov_predict_plan(Z.reshape(-1), xs, vol, mu, m, rho, gamma, jitter=PRIOR_JITTER)
        self._dtype = latent.loc.dtype
        self.loc = self.plan.mean.to(self._dtype).reshape(*self._batch, -1)

    @property
    def variance(self):
        """var_q + var_p, clamped at MIN_VARIANCE; detached, like ``MarkovVariationalLatent.variance``."""
        v = self.plan.var_q + self.plan.var_p
        return v.to(self._dtype).reshape(self.loc.shape).clamp_min(MIN_VARIANCE)

    @property
    def _covar(self):
        """Dense [.., H, H] from the dense definition A P^-1 A' + K** - A K_uu A' in fp64 (tests and small H only)."""
        model = self.model
        x = model.variational_strategy.inducing_points.reshape(-1).double()
        xs = self._xs.double()
        S = MarkovVariationalLatent(model)._covar.double().reshape(-1, x.shape[0], x.shape[0])
        vol = model.covar_module.vol.detach().double().reshape(-1, 1, 1)
        k = lambda a, b: vol * torch.minimum(a.unsqueeze(-1), b.unsqueeze(-2)) + PRIOR_JITTER
        Kuu, Ksu, Kss = k(x, x), k(xs, x), k(xs, xs)
        A = torch.linalg.solve(Kuu, Ksu.mT).mT
        C = A @ S @ A.mT + Kss - A @ Kuu @ A.mT
        return C.reshape(*self._batch, self.plan.H, self.plan.H).to(self._dtype)

    def rsample(self, sample_shape=torch.Size(), base_samples=None):
        """Joint draws of f(x), shape sample_shape + loc.shape.  ``base_samples``: N(0, 1) of shape sample_shape + [.., E],
        E = plan.E <= 3 H + 1 numbers per path (NOT H: a path is the image of the knot chain's and the bridges' innovations).
        E is read from the device at the first use (ops.MarkovPredictPlan.E: one host synchronisation), so
        ``model(x).rsample(..)`` as a whole cannot be captured in a graph; with ``plan.E`` read beforehand and ``base_samples``
        given, the draw alone can (ops.markov_predict_draw makes no host read)."""
        E = self.plan.E
        if base_samples is None:
            base_samples = torch.randn(*torch.Size(sample_shape), *self._batch, E, dtype=torch.float32, device=self.loc.device)
        elif base_samples.shape[-1] < E or tuple(base_samples.shape[base_samples.ndim - 1 - len(self._batch):-1]) != tuple(self._batch):
            raise ValueError(f"base_samples must be sample_shape + {tuple(self._batch) + (E,)}, got {tuple(base_samples.shape)}")
        lead = base_samples.shape[:base_samples.ndim - 1 - len(self._batch)]
        eps = base_samples.reshape(-1, self.plan.B, base_samples.shape[-1]).transpose(0, 1)            # [B,S,E]
        f = ops.markov_predict_draw(self.plan, eps)                                                    # [B,S,H]
        return f.transpose(0, 1).reshape(*lead, *self._batch, self.plan.H).to(self._dtype)


def _dkl_dscale_grad(o, c, n, w_kl, g):
    """dF/dc for K = c M + j I from the step's scalars o = out[:, 2:9]:
    tr(K^-1 M) = (N - j tr K^-1)/c,  tr(G'MG) = (tr(K^-1 S) - j |G|^2)/c,  beta'M beta = (r'K^-1 r - j |beta|^2)/c;
    dKL/dc = 1/2 (first - second - third)."""
    quad, tr_s, tr_inv, gg, bb = o[:, 0], o[:, 3], o[:, 4], o[:, 5], o[:, 6]
    j = PRIOR_JITTER
    dkl = 0.5 * ((n - j * tr_inv) - (tr_s - j * gg) - (quad - j * bb)) / c.reshape(-1)
    return (-w_kl * g * dkl).reshape(c.shape) if c.numel() == g.numel() else (-w_kl * g * dkl).sum().reshape(c.shape)


def _cv_transform(raw_a, raw_b, raw_c, B):
    """The "cv" likelihood's constraints, a = softplus(raw_a), b = 3 sigmoid(raw_b), c = 6 sigmoid(raw_c) - 3
    (volatility_likelihood.py:24-26), as the step's abc [B,3,Kc], and their Jacobian [..., 3, Kc]:
    d a / d raw_a = sigmoid(raw_a);  d b / d raw_b = 3 s (1 - s);  d c / d raw_c = 6 s (1 - s)."""
    sa, sb, sc = torch.sigmoid(raw_a.detach()), torch.sigmoid(raw_b.detach()), torch.sigmoid(raw_c.detach())
    abc = torch.stack([torch.nn.functional.softplus(raw_a.detach()), 3.0 * sb, 6.0 * sc - 3.0], -2)     # [..., 3, Kc]
    jac = torch.stack([sa, 3.0 * sb * (1.0 - sb), 6.0 * sc * (1.0 - sc)], -2)
    return abc.to(torch.float32).expand(B, 3, raw_a.shape[-1]), jac


def _cv_raw_grads(g2, graw, raw_shape):
    """The gradients of raw_a, raw_b, raw_c from graw = dF/d(a,b,c) * Jacobian [B,3,Kc]: raws of shape [Kc] are one
    likelihood for every series (the gradient sums over them), [B,Kc] one per series."""
    graw = g2 * graw                                                   # [B,3,Kc]
    graw = graw.sum(0) if len(raw_shape) == 1 else graw.transpose(0, 1)     # [3,Kc] / [3,B,Kc]
    return tuple(graw[i].reshape(raw_shape) for i in range(3))


@functools.lru_cache(maxsize=None)
def _inputs(function):
    """The names of ``function.forward``'s inputs, in order: ``backward`` returns one gradient (or None) for each."""
    return tuple(inspect.signature(function.forward).parameters)[1:]


def _elbo_forward(ctx, ws, device, num_gh, raws, lead, step, failed, grad_fields, keep, value):
    """The forward all four ELBO functions share, around one ops step into the workspace ``ws``.
    ``raws``: (raw_a, raw_b, raw_c) of the "cv" likelihood, or three None ("exp"); ``lead``: B or T of the step's abc.
    ``step(gh_x, gh_w, abc)`` runs the family's step; ``failed(abc)`` raises for a nonzero ``ws.info``.
    ``grad_fields``: input name -> the workspace field that is dF/d(that input); a field the workspace lacks is skipped.
    ``keep``: name -> a further tensor ``backward`` needs; ``value``: the view of ``ws.out`` that holds F (views of the
    workspace are cloned AFTER the step; the next step overwrites it).  What ``backward`` reads is saved under its name: the
    gradients under their inputs', ``keep`` under its own, dF/d(a,b,c) * Jacobian under "graw"."""
    gh_x, gh_w = _gauss_hermite(num_gh, device)
    cv = raws[0] is not None
    abc, jac = _cv_transform(*raws, lead) if cv else (None, None)
    step(gh_x, gh_w, abc)
    if deferred_checks.settle(ws.info) and bool((ws.info != 0).any().item()):
        failed(abc)
    saved = {name: getattr(ws, field).clone() for name, field in grad_fields.items() if getattr(ws, field) is not None}
    ctx.grad_names = tuple(saved)
    saved.update((name, t.clone()) for name, t in keep.items())
    if cv:
        ctx.raw_shape = raws[0].shape
        saved["graw"] = ws.grad_abc * jac
    ctx.saved_names = tuple(saved)
    ctx.save_for_backward(*saved.values())
    return value.clone()


def _elbo_backward(ctx, g):
    """The backward all four share.  Returns ({input name: g * its saved gradient, g broadcast over the leading (series)
    dimension; raw_a, raw_b, raw_c with the "cv" likelihood}, {name: saved tensor}): the caller adds its scale rule."""
    sv = dict(zip(ctx.saved_names, ctx.saved_tensors))
    grads = {name: g.reshape((-1,) + (1,) * (sv[name].ndim - 1)) * sv[name] for name in ctx.grad_names}
    if "graw" in sv:
        grads["raw_a"], grads["raw_b"], grads["raw_c"] = _cv_raw_grads(g.reshape(-1, 1, 1), sv["graw"], ctx.raw_shape)
    return grads, sv


class _GPCVElbo(torch.autograd.Function):
    """F[b] = w_ell ell_b - w_kl KL_b over a dense prior K, with the analytic gradient the HIP step returns.  raw_a, raw_b,
    raw_c None: the "exp" likelihood (ops.gpcv_step); given ([Kc] or [B,Kc]): the copula-process ("cv") likelihood,
    scale(f) = sum_k a_k softplus(b_k f + c_k) (ops.gpcv_cv_step) -- the step returns dF/d(a,b,c), the constraints' chain
    rule is applied here."""

    @staticmethod
    def forward(ctx, m, Lq, mean, K, y, raw_a, raw_b, raw_c, holder, scale, num_gh, w_ell, w_kl):
        B, n = m.shape
        want_dk = bool(ctx.needs_input_grad[_inputs(_GPCVElbo).index("K")])
        cv = raw_a is not None
        ws = holder.workspace(ops.GpcvWorkspace, B, n, want_dk, m.device, raw_a.shape[-1] if cv else 0)

        def step(gh_x, gh_w, abc):
            fn, lik = (ops.gpcv_cv_step, (abc,)) if cv else (ops.gpcv_step, ())
            fn(K.detach(), (m - mean).detach(), m.detach(), Lq.detach(), y, *lik, gh_x, gh_w, ws=ws, want_dk=want_dk,
               jitter=PRIOR_JITTER, min_var=MIN_VARIANCE, w_ell=w_ell, w_kl=w_kl)

        def failed(abc):
            _raise_step_failure("GPCV cv step" if cv else "GPCV step", ws.info, (K, m, Lq) + ((abc,) if cv else ()),
                                "prior covariance K + 1e-3 I")
        ctx.n, ctx.w_kl = n, w_kl
        keep = {"o": ws.out[:, 2:9], "prior_scale": scale.detach()} if scale is not None else {}
        return _elbo_forward(ctx, ws, m.device, num_gh, (raw_a, raw_b, raw_c), B, step, failed,
                             {"m": "grad_m", "Lq": "grad_Lq", "mean": "grad_mu", "K": "grad_K"}, keep, ws.out[:, 9])

    @staticmethod
    def backward(ctx, g):
        grads, sv = _elbo_backward(ctx, g)
        if "prior_scale" in sv:
            grads["scale"] = _dkl_dscale_grad(sv["o"], sv["prior_scale"], ctx.n, ctx.w_kl, g)
        return tuple(grads.get(name) for name in _inputs(_GPCVElbo))


class _GPCVBmElbo(torch.autograd.Function):
    """``_GPCVElbo`` (either likelihood: raw_a, raw_b, raw_c None or given) under the lazy Brownian-motion prior
    K = scale min(x, x'): the O(N^2) step of csrc/gpcv_bm.hip.  No dense K and no dF/dK: the prior's only parameter is
    ``scale``, whose gradient is the closed form the dense function uses (``_dkl_dscale_grad``).  A function of its own
    because its inputs differ in kind (a grid and a scale for a matrix), not only in data."""

    @staticmethod
    def forward(ctx, m, Lq, mean, scale, x, y, raw_a, raw_b, raw_c, holder, num_gh, w_ell, w_kl):
        B, n = m.shape
        ws = holder.workspace(ops.GpcvBmWorkspace, B, n, m.device, raw_a.shape[-1] if raw_a is not None else 0)

        def step(gh_x, gh_w, abc):
            ops.gpcv_bm_step(x, scale.detach(), (m - mean).detach(), m.detach(), Lq.detach(), y, gh_x, gh_w, ws, abc=abc,
                             jitter=PRIOR_JITTER, min_var=MIN_VARIANCE, w_ell=w_ell, w_kl=w_kl)

        def failed(abc):
            _raise_step_failure("GPCV step (linear prior)", ws.info, (scale, m, Lq) + ((abc,) if abc is not None else ()),
                                "prior covariance K + 1e-3 I")
        ctx.n, ctx.w_kl = n, w_kl
        return _elbo_forward(ctx, ws, m.device, num_gh, (raw_a, raw_b, raw_c), B, step, failed,
                             {"m": "grad_m", "Lq": "grad_Lq", "mean": "grad_mu"},
                             {"o": ws.out[:, 2:9], "prior_scale": scale.detach()}, ws.out[:, 9])

    @staticmethod
    def backward(ctx, g):
        grads, sv = _elbo_backward(ctx, g)
        grads["scale"] = _dkl_dscale_grad(sv["o"], sv["prior_scale"], ctx.n, ctx.w_kl, g)
        return tuple(grads.get(name) for name in _inputs(_GPCVBmElbo))


class _GPCVMarkovElbo(torch.autograd.Function):
    """F[b] = w_ell ell_b - w_kl KL_b for the Markov family (m, rho, gamma) under the level-jitter Brownian prior
    K_M = scale min(x, x') + j 1 1' (csrc/gpcv_markov.hip: one launch, O(N)).  The step returns dF/dscale itself
    (out[:, 6]); scale = sigmoid(raw_vol) stays in the graph, so its chain rule is autograd's."""

    @staticmethod
    def forward(ctx, m, rho, gamma, mean, scale, x, y, raw_a, raw_b, raw_c, holder, num_gh, w_ell, w_kl):
        B, n = m.shape
        ws = holder.workspace(ops.GpcvMarkovWorkspace, B, n, m.device, raw_a.shape[-1] if raw_a is not None else 0)

        def step(gh_x, gh_w, abc):
            ops.gpcv_markov_step(x, scale.detach(), (m - mean).detach(), m.detach(), rho.detach(), gamma.detach(), y, gh_x,
                                 gh_w, ws, abc=abc, jitter=PRIOR_JITTER, min_var=MIN_VARIANCE, w_ell=w_ell, w_kl=w_kl)

        def failed(abc):
            # info = 1: F is not finite.  There is no pivot in this family: a NaN input, or parameters whose variances overflow
            _raise_step_failure("GPCV step (markov family)", ws.info,
                                (scale, m, rho, gamma[..., :-1], mean, y) + ((abc,) if abc is not None else ()), None,
                                message="F is not finite although no input is NaN (info = "
                                        f"{ws.info.tolist()[:8]}): the variances exp(-2 log_diag_precision_root) or the products "
                                        "of coupling^2 overflow, or the prior's increments are not positive")
        ctx.scale_shape = scale.shape
        return _elbo_forward(ctx, ws, m.device, num_gh, (raw_a, raw_b, raw_c), B, step, failed,
                             {"m": "grad_m", "rho": "grad_rho", "gamma": "grad_gamma", "mean": "grad_mu"},
                             {"dF_dscale": ws.out[:, 6]}, ws.out[:, 9])

    @staticmethod
    def backward(ctx, g):
        grads, sv = _elbo_backward(ctx, g)
        gscale = g * sv["dF_dscale"]
        grads["scale"] = gscale.reshape(ctx.scale_shape) if gscale.numel() == math.prod(ctx.scale_shape) else \
            gscale.sum().reshape(ctx.scale_shape)
        return tuple(grads.get(name) for name in _inputs(_GPCVMarkovElbo))


class MultitaskVariationalLatent(MultivariateNormal):
    """What ``MultitaskVariationalGP(inducing_points)`` returns: q(F) = N(M, S_x (x) S_t) itself (event shape [N,T]), tied
    to its model so the ELBO can reach the prior."""

    def __init__(self, model):
        self.model = model
        self.loc = model.variational_mean

    @property
    def num_tasks(self):
        return self.loc.shape[-1]

    @property
    def event_shape(self):
        return self.loc.shape

    @property
    def _roots(self):
        return self.model.variational_covar_root.tril(), self.model.variational_task_covar_root.tril()

    @property
    def _covar(self):
        Lx, Lt = (r.detach() for r in self._roots)
        return torch.kron(ops.gemm_nt(Lx, Lx, uplo_a=1, uplo_b=1), ops.gemm_nt(Lt, Lt, uplo_a=1, uplo_b=1))

    @property
    def variance(self):
        Lx, Lt = self._roots
        return (Lx.pow(2).sum(-1).unsqueeze(-1) * Lt.pow(2).sum(-1).unsqueeze(-2)).clamp_min(MIN_VARIANCE)

    def rsample(self, sample_shape=torch.Size(), base_samples=None):
        """M + Lx E Lt', E ~ N(0, I) of shape sample_shape + [N,T] (the Kronecker root applied factor by factor)."""
        n, T = self.loc.shape
        base_samples = self._base_samples(sample_shape, base_samples)
        Lx, Lt = (r.detach() for r in self._roots)
        E = base_samples.reshape(-1, n, T)
        S = E.shape[0]
        X = ops.gemm_nt(E.reshape(S * n, T), Lt, uplo_b=1).reshape(S, n, T)                    # E Lt'
        Z = ops.gemm_nt(X.transpose(1, 2).reshape(S * T, n), Lx, uplo_b=1).reshape(S, T, n)    # (Lx X)'
        return self.loc.detach() + Z.transpose(1, 2).reshape(base_samples.shape)


def _raise_step_failure(what, info, tensors, which, message=None):
    """``message``: what NotPSDError says where the step has no factorisation to blame (the Markov family)."""
    if ops.info_internal(info):
        raise ops._lib.VoltHipError(f"{what}: internal error, info = {info.tolist()[:8]}")
    check_nan(tensors, f"{what}: NaN in the prior covariance or the variational parameters")
    raise NotPSDError(f"{what}: {message}" if message else f"{what}: {which} is not positive definite")


def mt_dkl_dscale(out, scale, n, T, jitter=PRIOR_JITTER):
    """dKL/ds of the multi-task step for K_x = s M0 (BMKernel: s = vol), from the scalars in the step's ``out``:
    [T (N - j tr K^-1) - tau_t (tau_x - j |G|_F^2) - (q - j tr(K_t^-1 A'A))] / (2 s),  K = s M0 + j I."""
    q, tau_x, tau_t, tr_inv, gg, tr_aa = out[2], out[7], out[8], out[9], out[10], out[11]
    return 0.5 * (T * (n - jitter * tr_inv) - tau_t * (tau_x - jitter * gg) - (q - jitter * tr_aa)) / scale.reshape(())


class _GPCVMtElbo(torch.autograd.Function):
    """F = w_ell ell - w_kl KL of the multi-task model with the analytic gradients the HIP step returns.  raw_a, raw_b, raw_c
    None: the "exp" likelihood; given ([T,Kc]): the copula-process ("cv") likelihood, one warp per task -- the step returns
    dF/d(a,b,c), the constraints' chain rule is applied here, as in ``_GPCVElbo``."""

    @staticmethod
    def forward(ctx, M, Lx, Lt, c, cf, rv, K, y, raw_a, raw_b, raw_c, holder, scale, num_gh, w_ell, w_kl):
        n, T = M.shape
        want_dk = bool(ctx.needs_input_grad[_inputs(_GPCVMtElbo).index("K")])
        cv = raw_a is not None
        ws = holder.workspace(ops.GpcvMtWorkspace, n, T, want_dk, M.device, raw_a.shape[-1] if cv else 0)

        def step(gh_x, gh_w, abc):
            ops.gpcv_mt_step(K.detach(), M, c, Lx, Lt, cf, rv, y, gh_x, gh_w, ws, want_dk=want_dk, jitter=PRIOR_JITTER,
                             min_var=MIN_VARIANCE, w_ell=w_ell, w_kl=w_kl, abc=abc)

        def failed(abc):
            info = ws.info.cpu()
            # info[0]: K_x + jitter I (LAPACK-style or an internal code);  info[1]: a pivot of K_t;  info[2]: F not finite
            which = "prior covariance K_x + 1e-3 I" if int(info[0]) != 0 else "task covariance K_t"
            _raise_step_failure("multi-task GPCV cv step" if cv else "multi-task GPCV step", info[:1],
                                (K, M, Lx, Lt, c, cf, rv, y) + ((abc,) if cv else ()), which)
        ctx.n, ctx.T, ctx.w_kl, ctx.cf_shape = n, T, w_kl, cf.shape
        keep = {"out": ws.out, "prior_scale": scale.detach()} if scale is not None else {}
        return _elbo_forward(ctx, ws, M.device, num_gh, (raw_a, raw_b, raw_c), T, step, failed,
                             {"M": "grad_M", "Lx": "grad_Lx", "Lt": "grad_Lt", "c": "grad_c", "cf": "grad_covar_factor",
                              "rv": "grad_raw_var", "K": "grad_K"}, keep, ws.out[12])

    @staticmethod
    def backward(ctx, g):
        grads, sv = _elbo_backward(ctx, g)
        grads["cf"] = grads["cf"].reshape(ctx.cf_shape)
        if "prior_scale" in sv:
            dkl = mt_dkl_dscale(sv["out"], sv["prior_scale"], ctx.n, ctx.T)
            grads["scale"] = (-ctx.w_kl * g * dkl).reshape(sv["prior_scale"].shape)
        return tuple(grads.get(name) for name in _inputs(_GPCVMtElbo))


class MultitaskMarkovVariationalLatent(MultitaskVariationalLatent):
    """What ``MultitaskVariationalGP(prior_solver="markov")(inducing_points)`` returns: q(F) = N(M, P^-1 (x) S_t) with the
    tridiagonal P = Lp Lp' of (log_diag_precision_root, coupling).  ``variance`` and ``rsample`` are O(N T) recurrences on the
    device (csrc/gpcv_markov.hip's root kernels); the dense covariance is built only when ``_covar`` is asked for."""

    def _root(self):
        m = self.model
        return m.log_diag_precision_root.detach().reshape(1, -1), m.coupling.detach().reshape(1, -1)

    @property
    def _covar(self):
        rho, gamma = self._root()
        d = rho[0].double().exp()
        Lp = torch.diag_embed(d)
        if d.shape[-1] > 1:
            Lp = Lp + torch.diag_embed(gamma[0].double()[:-1] * d[:-1], offset=-1)
        Lt = self.model.variational_task_covar_root.detach().tril().double()
        return torch.kron(torch.linalg.inv(Lp @ Lp.mT).contiguous(), (Lt @ Lt.mT).contiguous()).to(self.loc.dtype)

    @property
    def variance(self):
        """clamp(s_n st_t), s = diag P^-1 from the step's own scan, st = diag S_t.  DETACHED, like
        ``MarkovVariationalLatent.variance``: the gradients of the variational parameters come from ``VariationalELBO``."""
        s = ops.markov_root_var(*self._root())[0]                                              # [N] fp64
        st = self.model.variational_task_covar_root.detach().tril().double().pow(2).sum(-1)
        return (s.unsqueeze(-1) * st.unsqueeze(-2)).to(self.loc.dtype).clamp_min(MIN_VARIANCE)

    def rsample(self, sample_shape=torch.Size(), base_samples=None):
        """M + (Lp^-T E) Lt', E ~ N(0, I) of shape sample_shape + [N,T]: one backward recurrence per draw and task column
        (ops.markov_root_draw over the S T columns), then the T x T product."""
        n, T = self.loc.shape
        base_samples = self._base_samples(sample_shape, base_samples)
        rho, gamma = self._root()
        E = base_samples.reshape(-1, n, T)
        S = E.shape[0]
        cols = E.transpose(1, 2).reshape(1, S * T, n)                                          # a column of E per draw
        U = ops.markov_root_draw(torch.zeros_like(rho), rho, gamma, cols).reshape(S, T, n)     # (Lp^-T E)'
        Lt = self.model.variational_task_covar_root.detach().tril().to(torch.float32)
        F = torch.matmul(U.transpose(1, 2), Lt.mT)                                             # [S,N,T]
        return (self.loc.detach() + F.reshape(base_samples.shape)).to(self.loc.dtype)


class MultitaskMarkovPredictiveLatent(MultitaskVariationalLatent):
    """What ``MultitaskVariationalGP(prior_solver="markov")(x)`` returns for ``x`` other than the inducing grid: q(F(x)) over
    [H,T], covariance (A P^-1 A') (x) S_t + (K** - A K_uu A') (x) K_t with K_t = f f' + diag softplus(raw_var) as the step
    defines it.  The x side is csrc/markov_predict.hip: one plan over the T columns of M (the mean: task t's
    constant is the level before x_0) and one over a single zero-mean series (the variances and the draws: exact deviations,
    no mean to subtract) -- so the three N-length scans, which do not depend on the mean, run T + 1 times instead of once, in
    two launches; the two T x T products of ``rsample`` stay in torch.  NO autograd, like ``MarkovPredictiveLatent``."""

    def __init__(self, model, xs):
        self.model, self._xs = model, xs
        M = model.variational_mean.detach()
        n, T = M.shape
        rho, gamma = model.log_diag_precision_root.detach().reshape(1, n), model.coupling.detach().reshape(1, n)
        c, cf, rv = (t.detach().reshape(-1) for t in model._task_params())
        x, vol = model.inducing_points.reshape(-1), model.data_kernel.vol.detach().reshape(-1)
        self._mean_plan = ops.markov_predict_plan(x, xs, vol, c, M.mT, rho.expand(T, n), gamma.expand(T, n), jitter=PRIOR_JITTER)
        zero = torch.zeros(1, n, dtype=torch.float32, device=M.device)
        self.plan = ops.markov_predict_plan(x, xs, vol, zero[:, 0], zero, rho, gamma, jitter=PRIOR_JITTER)
        self._dtype = M.dtype
        self.loc = self._mean_plan.mean.mT.to(self._dtype).contiguous()                       # [H,T]
        Lt = model.variational_task_covar_root.detach().tril().double()
        self._St = Lt @ Lt.mT
        self._Kt = torch.outer(cf.double(), cf.double()) + torch.diag(torch.nn.functional.softplus(rv.double()))
        self._Lt = Lt

    @property
    def variance(self):
        """var_q diag S_t + var_p diag K_t [H,T], clamped at MIN_VARIANCE; detached."""
        v = torch.outer(self.plan.var_q[0], self._St.diagonal()) + torch.outer(self.plan.var_p[0], self._Kt.diagonal())
        return v.to(self._dtype).clamp_min(MIN_VARIANCE)

    @property
    def _covar(self):
        """Dense (H T) x (H T), element (h, t) at h T + t, from the dense definition in fp64 (tests and small H only)."""
        m = self.model
        x, xs = m.inducing_points.reshape(-1).double(), self._xs.double()
        n = x.shape[0]
        d = m.log_diag_precision_root.detach().double().exp()
        Lp = torch.diag_embed(d)
        if n > 1:
            Lp = Lp + torch.diag_embed(m.coupling.detach().double()[:-1] * d[:-1], offset=-1)
        S = torch.linalg.inv(Lp @ Lp.mT)
        vol = m.data_kernel.vol.detach().double().reshape(())
        k = lambda a, b: vol * torch.minimum(a.unsqueeze(-1), b.unsqueeze(-2)) + PRIOR_JITTER
        Kuu, Ksu, Kss = k(x, x), k(xs, x), k(xs, xs)
        A = torch.linalg.solve(Kuu, Ksu.mT).mT
        C = torch.kron((A @ S @ A.mT).contiguous(), self._St) + torch.kron((Kss - A @ Kuu @ A.mT).contiguous(), self._Kt)
        return C.to(self._dtype)

    def rsample(self, sample_shape=torch.Size(), base_samples=None):
        """Joint draws of F(x), shape sample_shape + [H,T]: T unit chains mixed by Lt' plus T unit bridges mixed by chol(K_t)'.
        ``base_samples``: N(0, 1) of shape sample_shape + [T, E], E = plan.E <= 3 H + 1 -- the chain and the bridge steps read
        disjoint columns of a row, so one row serves both.  E is read from the device at the first use (one host synchronisation:
        see ``MarkovPredictiveLatent.rsample``)."""
        H, T = self.loc.shape
        E = self.plan.E
        if base_samples is None:
            base_samples = torch.randn(*torch.Size(sample_shape), T, E, dtype=torch.float32, device=self.loc.device)
        elif base_samples.ndim < 2 or base_samples.shape[-2] != T or base_samples.shape[-1] < E:
            raise ValueError(f"base_samples must be sample_shape + {(T, E)}, got {tuple(base_samples.shape)}")
        lead = base_samples.shape[:-2]
        eps = base_samples.reshape(1, -1, base_samples.shape[-1])                                      # [1, S T, E]
        Uc = ops.markov_predict_draw(self.plan, eps, part="chain").reshape(-1, T, H)                   # (zero mean: the parts alone)
        Ub = ops.markov_predict_draw(self.plan, eps, part="bridge").reshape(-1, T, H)
        Ck = torch.linalg.cholesky(self._Kt).to(torch.float32)
        F = torch.matmul(Uc.transpose(1, 2), self._Lt.to(torch.float32).mT) + torch.matmul(Ub.transpose(1, 2), Ck.mT)   # [S,H,T]
        return (self.loc + F).reshape(*lead, H, T).to(self._dtype)


class _GPCVMtMarkovElbo(torch.autograd.Function):
    """F = w_ell ell - w_kl KL of the multi-task model with the Markov family (M, rho, gamma, Lt) under the prior
    K_M (x) K_t, K_M = scale min(x, x') + j 1 1' (csrc/gpcv_mt_markov.hip: O(N T)).  The step returns dF/dscale itself
    (out[9]); scale = sigmoid(raw_vol) stays in the graph, so its chain rule is autograd's, as in ``_GPCVMarkovElbo``."""

    @staticmethod
    def forward(ctx, M, rho, gamma, Lt, c, cf, rv, scale, x, y, raw_a, raw_b, raw_c, holder, num_gh, w_ell, w_kl):
        n, T = M.shape
        cv = raw_a is not None
        ws = holder.workspace(ops.GpcvMtMarkovWorkspace, n, T, M.device, raw_a.shape[-1] if cv else 0)

        def step(gh_x, gh_w, abc):
            ops.gpcv_mt_markov_step(x, scale.detach(), M.detach(), c.detach(), rho.detach(), gamma.detach(), Lt.detach(),
                                    cf.detach(), rv.detach(), y, gh_x, gh_w, ws, abc=abc, jitter=PRIOR_JITTER,
                                    min_var=MIN_VARIANCE, w_ell=w_ell, w_kl=w_kl)

        def failed(abc):
            info = ws.info.cpu()
            # info[0]: F is not finite;  info[1]: a pivot of K_t.  There is no pivot on the x side
            tensors = (scale, M, rho, gamma[..., :-1], Lt, c, cf, rv, y) + ((abc,) if cv else ())
            what = "multi-task GPCV cv step (markov family)" if cv else "multi-task GPCV step (markov family)"
            if int(info[1]) != 0:
                _raise_step_failure(what, info[1:], tensors, "task covariance K_t")
            _raise_step_failure(what, info[:1], tensors, None,
                                message="F is not finite although no input is NaN: the variances exp(-2 log_diag_precision_root) "
                                        "or the products of coupling^2 overflow, the prior's increments are not positive, or the "
                                        "task root has a zero on its diagonal")
        ctx.cf_shape, ctx.scale_shape = cf.shape, scale.shape
        return _elbo_forward(ctx, ws, M.device, num_gh, (raw_a, raw_b, raw_c), T, step, failed,
                             {"M": "grad_M", "rho": "grad_rho", "gamma": "grad_gamma", "Lt": "grad_Lt", "c": "grad_c",
                              "cf": "grad_covar_factor", "rv": "grad_raw_var"}, {"dF_dscale": ws.out[9]}, ws.out[10])

    @staticmethod
    def backward(ctx, g):
        grads, sv = _elbo_backward(ctx, g)
        grads["cf"] = grads["cf"].reshape(ctx.cf_shape)
        grads["scale"] = (g * sv["dF_dscale"]).reshape(ctx.scale_shape)
        return tuple(grads.get(name) for name in _inputs(_GPCVMtMarkovElbo))


class VariationalELBO(Module):
    """gpytorch.mlls.VariationalELBO(likelihood, model, num_data, beta=1.0, combine_terms=True) stand-in
    (train_utils.py:44): ``mll(model(train_x), yy)`` -> scalar ELBO (or [T] for a batched model)."""

    def __init__(self, likelihood, model, num_data, beta=1.0, combine_terms=True):
        super().__init__()
        if not combine_terms:
            raise NotImplementedError("combine_terms=False is not used on this path (train_utils.py:44)")
        param = getattr(likelihood, "param", "exp")
        if param not in ("exp", "cv"):
            raise NotImplementedError(f"unknown volatility likelihood parameterisation {param!r}")
        if param == "cv" and hasattr(model, "variational_task_covar_root"):      # MultitaskVariationalGP: one warp per task
            T = model.num_tasks
            if likelihood.raw_a.ndim != 2:
                raise NotImplementedError('the multi-task model has an accelerated "cv" ELBO with one warp per task only: '
                                          f"build the likelihood with batch_shape=[num_tasks] = [{T}]")
            if likelihood.raw_a.shape[0] != T:
                raise ValueError(f"VariationalELBO: the likelihood's batch shape {tuple(likelihood.raw_a.shape[:-1])} does "
                                 f"not match the model's num_tasks = {T}")
        if param == "cv" and not 1 <= likelihood.raw_a.shape[-1] <= ops.GPCV_CV_K_MAX:
            raise NotImplementedError(f'the accelerated "cv" ELBO takes 1 <= K <= {ops.GPCV_CV_K_MAX} warp terms')
        object.__setattr__(self, "likelihood", likelihood)
        object.__setattr__(self, "model", model)
        self.num_data, self.beta = float(num_data), float(beta)
        for attr in self._WS_ATTR.values():
            setattr(self, attr, None)

    # one workspace of each kind lives from iteration to iteration (a captured graph holds their addresses)
    _WS_ATTR = {ops.GpcvWorkspace: "_ws", ops.GpcvMtWorkspace: "_mt_ws", ops.GpcvBmWorkspace: "_bm_ws",
                ops.GpcvMarkovWorkspace: "_markov_ws", ops.GpcvMtMarkovWorkspace: "_mt_markov_ws"}

    def workspace(self, cls, *key):
        """The cached workspace of class ``cls`` if it fits ``key`` (the constructor's arguments), else a new one."""
        return ops.cached_workspace(self, self._WS_ATTR[cls], cls, *key)

    @staticmethod
    def _need_cuda(t):
        if not t.is_cuda:
            raise ops._lib.VoltHipError("VariationalELBO: tensors must live on the MI355X; no CPU fallback")

    def _weights(self, n):                               # (num_gh, w_ell, w_kl): the likelihood term / N, the KL / (num_data / beta)
        return num_gauss_hermite_locs.value(), 1.0 / n, self.beta / self.num_data

    def _likelihood_raws(self, lead, m):
        """(raw_a, raw_b, raw_c) of a "cv" likelihood as the ELBO functions take them, three None for "exp".  A batched
        likelihood (one parameter set per series or task) must match the model's ``lead`` = B series (batch shape
        m.shape[:-1]) or T tasks."""
        lik = self.likelihood
        if getattr(lik, "param", "exp") != "cv":
            return [None, None, None]
        Kc = lik.raw_a.shape[-1]
        raws = [lik.raw_a, lik.raw_b, lik.raw_c]
        if lik.raw_a.ndim > 1:
            if lik.raw_a.numel() != lead * Kc:
                raise ValueError(f"VariationalELBO: the likelihood's batch shape {tuple(lik.raw_a.shape[:-1])} does not "
                                 f"match the model's {tuple(m.shape[:-1])}")
            raws = [r.reshape(lead, Kc) for r in raws]
        return raws

    def _forward_multitask(self, latent, target):
        """VariationalELBO over a MultitaskMultivariateNormal (event shape [N,T]): the likelihood term is summed over
        tasks and divided by N, the KL by num_data / beta."""
        model = latent.model
        M = model.variational_mean
        self._need_cuda(M)
        n, T = M.shape
        if tuple(target.shape) != (n, T):
            raise ValueError(f"VariationalELBO: the multi-task target must be [N,T] = [{n},{T}] (got {tuple(target.shape)})")
        lazy = model.data_kernel(model.inducing_points)
        scale = None
        if isinstance(lazy, _ScaledDense) and lazy.scale.numel() == 1:
            scale = lazy.scale
            K = scale.detach().reshape(()) * lazy.base
        else:
            K = _dense(lazy)
        c, cf, rv = model._task_params()
        return _GPCVMtElbo.apply(M, model.variational_covar_root, model.variational_task_covar_root, c, cf, rv,
                                 K.to(torch.float32), target.to(torch.float32), *self._likelihood_raws(T, M), self, scale,
                                 *self._weights(n))

    def _forward_multitask_markov(self, latent, target):
        """``_forward_multitask`` for prior_solver="markov": the O(N T) step over (M, rho, gamma, Lt); nothing N x N is formed."""
        model = latent.model
        M = model.variational_mean
        self._need_cuda(M)
        n, T = M.shape
        if tuple(target.shape) != (n, T):
            raise ValueError(f"VariationalELBO: the multi-task target must be [N,T] = [{n},{T}] (got {tuple(target.shape)})")
        c, cf, rv = model._task_params()
        return _GPCVMtMarkovElbo.apply(M, model.log_diag_precision_root, model.coupling, model.variational_task_covar_root, c,
                                       cf, rv, model.data_kernel.vol, model.inducing_points.reshape(-1),
                                       target.to(torch.float32), *self._likelihood_raws(T, M), self, *self._weights(n))

    def _forward_markov(self, latent, target):
        """prior_solver="markov": the O(N) step over (m, rho, gamma); nothing N x N is formed."""
        model = latent.model
        m = latent.loc
        self._need_cuda(m)
        prior = model.forward(model.variational_strategy.inducing_points)
        lazy = prior.lazy_covariance_matrix
        if not isinstance(lazy, _BrownianLevelPrior):
            raise TypeError("VariationalELBO: the Markov variational family needs the prior of prior_solver='markov'")
        n = m.shape[-1]
        f32 = lambda t: t.reshape(-1, n).to(torch.float32)
        B = m.numel() // n
        res = _GPCVMarkovElbo.apply(f32(m), f32(latent._rho), f32(latent._gamma), f32(prior.mean.expand(m.shape)), lazy.scale,
                                    lazy.x, f32(target), *self._likelihood_raws(B, m), self, *self._weights(n))
        return res.reshape(m.shape[:-1]) if m.ndim > 1 else res.reshape(())

    def natural_gradient_step(self, target, step=1.0):
        """One natural-gradient (conjugate-computation VI) update of q for ``SingleTaskVariationalGP(prior_solver="markov")``:
        ONE launch, O(N), no host read (ops.gpcv_markov_natgrad).  The weights, the likelihood's transformed
        a, b, c, the prior mean and the vol are what ``forward`` hands the ELBO step.  The sites live on the
        ``MarkovVariationalDistribution`` (``natural_sites``: fp64, zeros at first use, not in the ``state_dict``); the three
        variational parameters are overwritten IN PLACE, under ``no_grad``.  ``step`` in (0, 1]: 1 jumps to the q the current
        sites' targets define (the "exp" likelihood converges in about ten such updates); the "cv" likelihood is not
        log-concave -- its negative lam2 targets are clamped at 0 and F need not rise monotonically: use a step of 0.5.
        Returns ``out`` [B,4] fp64: the number of clamped sites and max |change| of the mean, log_diag_precision_root and
        coupling -- a convergence measure; ``info`` stays on the workspace (1: a non-finite series, now NaN)."""
        model = self.model
        strategy = getattr(model, "variational_strategy", None)
        dist = getattr(strategy, "_variational_distribution", None)
        if not isinstance(dist, MarkovVariationalDistribution):
            raise ValueError('VariationalELBO.natural_gradient_step needs SingleTaskVariationalGP(prior_solver="markov"): only '
                             f"the Markov variational family contains the optimal q (got {type(model).__name__}"
                             f"(prior_solver={getattr(model, 'prior_solver', None)!r}))")
        m = dist.variational_mean
        self._need_cuda(m)
        with torch.no_grad():
            prior = model.forward(strategy.inducing_points)
            lazy = prior.lazy_covariance_matrix
            if not isinstance(lazy, _BrownianLevelPrior):
                raise TypeError("VariationalELBO: the Markov variational family needs the prior of prior_solver='markov'")
            n = m.shape[-1]
            B = m.numel() // n
            q = [p.data.view(B, n) for p in (m, dist.log_diag_precision_root, dist.coupling)]
            if any(t.dtype != torch.float32 or not t.is_contiguous() for t in q):
                raise ValueError("VariationalELBO.natural_gradient_step: the variational parameters must be contiguous fp32")
            num_gh, w_ell, w_kl = self._weights(n)
            gh_x, gh_w = _gauss_hermite(num_gh, m.device)
            raws = self._likelihood_raws(B, m)
            abc = _cv_transform(*raws, B)[0] if raws[0] is not None else None
            lam1, lam2 = dist.natural_sites()
            # (the update's workspace is no ELBO step's: it lives beside the five of `_WS_ATTR`, kept the same way)
            ws = ops.cached_workspace(self, "_markov_ng_ws", ops.GpcvMarkovNgWorkspace, B, n, m.device,
                                      abc.shape[-1] if abc is not None else 0)
            ops.gpcv_markov_natgrad(lazy.x, lazy.scale, prior.mean.expand(m.shape).reshape(B, n), *q,
                                    target.reshape(B, n).to(torch.float32), gh_x, gh_w, lam1, lam2, ws, abc=abc, into=tuple(q),
                                    jitter=PRIOR_JITTER, min_var=MIN_VARIANCE, w_ell=w_ell, w_kl=w_kl, step=step)
        return ws.out

    def forward(self, approximate_dist_f, target):
        if isinstance(approximate_dist_f, MultitaskMarkovVariationalLatent):
            return self._forward_multitask_markov(approximate_dist_f, target)
        if isinstance(approximate_dist_f, MultitaskVariationalLatent):
            return self._forward_multitask(approximate_dist_f, target)
        if isinstance(approximate_dist_f, MarkovVariationalLatent):
            return self._forward_markov(approximate_dist_f, target)
        if not isinstance(approximate_dist_f, VariationalLatent):
            raise TypeError("VariationalELBO expects the output of SingleTaskVariationalGP(train_x)")
        model = approximate_dist_f.model
        m, Lq = approximate_dist_f.loc, approximate_dist_f._chol
        self._need_cuda(m)
        Z = model.variational_strategy.inducing_points
        prior = model.forward(Z)
        n = m.shape[-1]
        batched = m.ndim > 1
        m2, L3, y2 = m.reshape(-1, n), Lq.reshape(-1, n, n), target.reshape(-1, n).to(torch.float32)
        B = m2.shape[0]
        mean2 = prior.mean.expand(m.shape).reshape(-1, n)
        lazy = prior.lazy_covariance_matrix
        raws, weights = self._likelihood_raws(B, m), self._weights(n)
        if isinstance(lazy, _BrownianPrior):                           # prior_solver="linear": no dense K anywhere
            res = _GPCVBmElbo.apply(m2.to(torch.float32), L3.to(torch.float32), mean2.to(torch.float32), lazy.scale, lazy.x, y2,
                                    *raws, self, *weights)
        else:
            scale = None
            if isinstance(lazy, _ScaledDense):
                scale = lazy.scale
                K3 = (scale.detach().reshape(-1, 1, 1) * lazy.base).expand(B, n, n)
            else:
                K3 = _dense(lazy).expand(B, n, n) if _dense(lazy).ndim == 2 else _dense(lazy).reshape(-1, n, n)
            res = _GPCVElbo.apply(m2.to(torch.float32), L3.to(torch.float32), mean2.to(torch.float32), K3, y2, *raws, self,
                                  scale, *weights)
        return res.reshape(m.shape[:-1]) if batched else res.reshape(())
