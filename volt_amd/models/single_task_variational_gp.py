"""SingleTaskVariationalGP, voltron/models/single_task_variational_gp.py:69-236 -- SURVEY 8(f) row 4.

The variational GP LearnGPCV fits to the scaled returns (train_utils.py:26-31): inducing points fixed at the
training inputs, unwhitened strategy, Cholesky variational distribution.  Only that configuration is on the
accelerated path; the whitened strategy / learned inducing locations / botorch posterior interface of the
reference class are not (they are never reached from LearnGPCV).  The dense algebra -- here the start-up
factorisations of ``initialize_variational_parameters`` -- runs through the HIP library (potrf, trtri, gemm)."""
import torch

from .. import ops
from ..gp import ConstantMean, EqualMemo, Module, MultivariateNormal, _BrownianLevelPrior, _BrownianPrior, _dense, check_grid
from ..safe import _safe_factor
from ..kernels.BMKernel import BMKernel
from ..likelihoods import VolatilityGaussianLikelihood  # noqa: F401  (re-exported like the reference's module namespace)
from ..variational import (PRIOR_JITTER, CholeskyVariationalDistribution, MarkovVariationalDistribution,
                           MarkovPredictiveLatent, MarkovVariationalLatent, UnwhitenedVariationalStrategy, VariationalLatent,
                           _predict_points)


class SingleTaskVariationalGP(Module):
    """``prior_solver="dense"`` (default): the prior is ``covar_module(x)`` and the ELBO step factors it (csrc/gpcv.hip).
    ``prior_solver="linear"`` (``covar_module`` a BMKernel only): ``forward`` returns the lazy ``gp._BrownianPrior`` and
    VariationalELBO runs the O(N^2) step of csrc/gpcv_bm.hip.  The inducing grid is validated ONCE here (one
    host read): x_0 >= 0, strictly increasing.  The start-up values (``initialize_variational_parameters``) are dense
    either way.
    ``prior_solver="markov"`` (BMKernel only, grid validated the same way): O(N) time and memory (csrc/gpcv_markov.hip; DESIGN
    4.19).  The variational family is ``MarkovVariationalDistribution`` (tridiagonal precision; parameters
    ``variational_mean``, ``log_diag_precision_root``, ``coupling``) and the prior is Brownian motion started from an
    N(0, 1e-3) LEVEL, K_M = vol min(x, x') + 1e-3 1 1' -- not the other solvers' K + 1e-3 I, whose diagonal jitter destroys the
    Markov structure; a jitter on the starting level keeps the precision exactly tridiagonal and x_0 = 0 valid.  The
    start-up values take an O(N) route (``_initialize_markov``); no N x N tensor exists anywhere on this route.
    Only this solver answers AWAY from the inducing grid: ``model(x)`` for any x [H] or [H,1] >= 0, in any order, returns
    ``MarkovPredictiveLatent`` (mean, variance, joint draws in O(N + S H); csrc/markov_predict.hip) -- between
    two observations or beyond the last one.  "dense" and "linear" raise NotImplementedError there."""
    PRIOR_SOLVERS = ("dense", "linear", "markov")

    def __init__(self, init_points=None, likelihood=None, learn_inducing_locations=True, covar_module=None,
                 mean_module=None, use_piv_chol_init=True, num_inducing=None, use_whitened_var_strat=True,
                 init_targets=None, train_inputs=None, train_targets=None, outcome_transform=None,
                 input_transform=None, *, prior_solver="dense"):
        super().__init__()
        if prior_solver not in self.PRIOR_SOLVERS:
            raise ValueError(f"SingleTaskVariationalGP: prior_solver must be one of {self.PRIOR_SOLVERS}, got {prior_solver!r}")
        if use_whitened_var_strat:
            raise NotImplementedError("use_whitened_var_strat=True is outside the accelerated path: LearnGPCV uses the "
                                      "unwhitened strategy (train_utils.py:30)")
        if outcome_transform is not None or input_transform is not None:
            raise NotImplementedError("botorch input/outcome transforms are not used by LearnGPCV")
        if covar_module is None:
            raise NotImplementedError("pass covar_module (BMKernel / FBMKernel, train_utils.py:22-25)")
        if prior_solver != "dense" and not isinstance(covar_module, BMKernel):
            raise ValueError(f"SingleTaskVariationalGP: prior_solver={prior_solver!r} needs covar_module=BMKernel (Brownian "
                             f"motion is Markov; {type(covar_module).__name__} is not)")
        inducing_points = init_points.detach().clone()
        if prior_solver != "dense":
            if inducing_points.ndim > 2 or (inducing_points.ndim == 2 and inducing_points.shape[-1] != 1):
                raise ValueError(f"SingleTaskVariationalGP(prior_solver={prior_solver!r}): the inducing grid must be [N] or "
                                 f"[N,1], got shape {tuple(inducing_points.shape)}")
            check_grid(inducing_points.reshape(-1), f"SingleTaskVariationalGP(prior_solver={prior_solver!r})")
        self.prior_solver = prior_solver
        family = MarkovVariationalDistribution if prior_solver == "markov" else CholeskyVariationalDistribution
        variational_distribution = family(inducing_points.shape[-2])
        self.variational_strategy = UnwhitenedVariationalStrategy(
            self, inducing_points, variational_distribution, learn_inducing_locations=learn_inducing_locations)
        self.mean_module = ConstantMean() if mean_module is None else mean_module
        self.covar_module = covar_module
        self.likelihood = likelihood
        self.train_inputs = [train_inputs] if train_inputs is not None else [init_points]
        self.train_targets = train_targets if train_targets is not None else init_targets
        self.condition_into_exact = True
        object.__setattr__(self, "_eq_memo", EqualMemo())
        self.to(init_points.device)

    @property
    def num_outputs(self):
        return 1

    def forward(self, x):
        """The prior at x (single_task_variational_gp.py:117-121); prior_solver="linear": lazily, over the inducing grid."""
        if self.prior_solver != "dense":
            Z = self.variational_strategy.inducing_points
            if x is not Z and not (x.numel() == Z.numel() and torch.equal(x.reshape(-1), Z.reshape(-1))):
                raise ValueError(f"SingleTaskVariationalGP(prior_solver={self.prior_solver!r}): the prior is over the inducing "
                                 "grid validated at construction")
            if self.prior_solver == "markov":
                return MultivariateNormal(self.mean_module(x), _BrownianLevelPrior(self.covar_module.vol, Z[:, 0], PRIOR_JITTER))
            return MultivariateNormal(self.mean_module(x), _BrownianPrior(self.covar_module.vol, Z[:, 0]))
        return MultivariateNormal(self.mean_module(x), self.covar_module(x))

    def __call__(self, x):
        arg = x
        if x.ndim == 1:
            x = x.unsqueeze(-1)
        Z = self.variational_strategy.inducing_points
        # LearnGPCV passes the same train_x object on every iteration (train_utils.py:51): compare once, not 1000 times
        if x.shape == Z.shape and self._eq_memo.equal(arg, Z, lambda: torch.equal(x, Z)):
            return MarkovVariationalLatent(self) if self.prior_solver == "markov" else VariationalLatent(self)
        if self.prior_solver == "markov":                             # away from the grid: O(N + H), csrc/markov_predict.hip
            return MarkovPredictiveLatent(self, _predict_points(arg, 'SingleTaskVariationalGP(prior_solver="markov")'))
        raise NotImplementedError("SingleTaskVariationalGP(x) away from the inducing points is outside the accelerated "
                                  "path: LearnGPCV only evaluates the model at train_x (train_utils.py:51,60)")

    def initialize_variational_parameters(self, likelihood, x, f=None, y=None):
        """single_task_variational_gp.py:204-254: covariance S = L (L'HL + I)^-1 L' with H the inverse Hessian of the
        likelihood, stored as 10 * chol(S); the mean constant is the log of the mean running std of y.
        "exp": mean = log running std, H clamped to [1e-4, 1000] (off-diagonal zeros included).
        "cv" (:227-238, K = 1 only) with the reference's quirks kept: ``y = f.t()`` replaces the returns by the log running
        std, so H sees the data only through it; mean = ((y/a).exp() - 1 - c)/b; no clamp on this branch.  The reference's
        ``y / trans_a`` broadcasts [N] against [K], which works for K = 1 only: K > 1 raises here.
        y [N], or [T,N] for T series sharing the inducing points (batched parameters)."""
        param = getattr(likelihood, "param", "exp")
        if param not in ("exp", "cv"):
            raise NotImplementedError(f"unknown volatility likelihood parameterisation {param!r}")
        if param == "cv" and likelihood.raw_a.shape[-1] != 1:
            raise NotImplementedError('the "cv" initialisation divides y [N] by trans_a [K] (single_task_variational_gp.py:229: '
                                      '`y / likelihood.trans_a`), a broadcast that only works for K = 1; K = '
                                      f'{likelihood.raw_a.shape[-1]} has no start-up values')
        with torch.no_grad():
            Z = self.variational_strategy.inducing_points
            if self.prior_solver != "markov":
                kuu = _dense(self.covar_module(Z)).to(torch.float32)
            y2 = y.reshape(-1, y.shape[-1]).to(torch.float32)
            T, N = y2.shape
            # running std of y[:i] (unbiased), one prefix-sum pass instead of the reference's N slices
            idx = torch.arange(N, device=y2.device, dtype=torch.float64)
            c1 = torch.cumsum(y2.double(), -1)
            c2 = torch.cumsum(y2.double() ** 2, -1)
            s1 = torch.cat([torch.zeros(T, 1, dtype=torch.float64, device=y2.device), c1[:, :-1]], -1)
            s2 = torch.cat([torch.zeros(T, 1, dtype=torch.float64, device=y2.device), c2[:, :-1]], -1)
            var = (s2 - s1 * s1 / idx.clamp_min(1)) / (idx - 1).clamp_min(1)
            running_std = var.clamp_min(0).sqrt().to(torch.float32)
            running_std[:, :10] = running_std[:, 10:11]
            if f is None:
                f = running_std.clamp(min=1e-4).log()
            f = f.reshape(T, N)
            markov = self.prior_solver == "markov"
            if param == "exp":
                # torch.diag_embed(...).clamp(min=1e-4, max=1000.): the clamp also lifts the off-diagonal zeros to 1e-4
                h = (0.5 * y2.pow(-2.0) * (f * 2.0).exp()).clamp(min=1e-4, max=1000.0)
                ih = None if markov else torch.full((T, N, N), 1e-4, device=y2.device)
            else:
                a, b, c = (p.detach().to(y2.device, torch.float32).reshape(-1, 1)
                           for p in (likelihood.trans_a, likelihood.trans_b, likelihood.trans_c))      # [1,1] or [T,1]
                yl = f                                                                       # `y = f.t()`: the returns are gone
                f = ((yl / a).exp() - 1 - c) / b
                sigma = ((b * f + c).exp() + 1).log().mul(a).clamp(min=likelihood.MIN_SCALE)  # likelihood(f).scale, K = 1
                scaling = ((2 + 3 * yl.pow(2.0)) * (a * b.pow(2.0) / 2)).pow(-1.0)
                h = scaling * sigma.pow(2.0) * (1 + torch.cosh(b * yl + c))
                ih = None if markov else torch.zeros((T, N, N), device=y2.device)
            if markov:
                return self._initialize_markov(h.expand(T, N), f, running_std, y.ndim == 1)
            ih.diagonal(dim1=-2, dim2=-1).copy_(h)
            L = _safe_factor(kuu.reshape(-1, N, N))[0].L.expand(T, N, N)                 # kuu.cholesky()
            Lt = L.mT.contiguous()
            HL = ops.gemm_nt(ih, Lt, uplo_b=2)                                           # H L
            inner = ops.gemm_nt(Lt, HL.mT.contiguous(), uplo_a=2)                        # L' H L
            inner = inner + torch.eye(N, device=y2.device)
            fi = _safe_factor(inner)[0]
            Yi = ops.trtri(fi)                                                           # chol(inner)^-T
            R = ops.gemm_nt(L.contiguous(), Yi.mT.contiguous(), uplo_a=1, uplo_b=1)        # L chol(inner)^-1 ... R R' = S
            S = ops.gemm_nt(R, R)
            S_root = _safe_factor(S)[0].L * 10.0
            dist = self.variational_strategy._variational_distribution
            squeeze = y.ndim == 1
            dist.variational_mean.data = f[0] if squeeze else f
            dist.chol_variational_covar.data = S_root[0] if squeeze else S_root
            self.variational_strategy.variational_params_initialized.fill_(1)
            const = running_std.mean(-1).log()
            self.mean_module.constant.data = const[0] if squeeze else const.unsqueeze(-1)

    def _initialize_markov(self, h, f, running_std, squeeze):
        """The start-up values of prior_solver="markov" in O(N).  The reference's S = L (L'HL + I)^-1 L' equals (K^-1 + H)^-1 for
        a diagonal H, so under the Markov prior K_M its precision is tridiagonal: P0 = (K_M^-1 + diag(h)) / 100 (the / 100 is the
        reference's 10 * chol(S)), and (log_diag_precision_root, coupling) is the bidiagonal Cholesky factor of P0 -- one fp64
        host loop over N, vectorised over the series, once.  h, f [T,N]: what ``initialize_variational_parameters`` computed.
        One quirk cannot be carried: the "exp" branch's clamp lifts the OFF-diagonal zeros of H to 1e-4, a dense rank-one term;
        here H is its clamped diagonal only."""
        Z = self.variational_strategy.inducing_points
        x = Z.reshape(-1).double().cpu().numpy()
        vol = self.covar_module.vol.detach().double().reshape(-1).cpu().numpy()           # [1] or [T]
        rho, gamma = markov_startup_factor(x, vol, PRIOR_JITTER, h.double().cpu().numpy())
        dev, dist = Z.device, self.variational_strategy._variational_distribution
        put = lambda a: torch.as_tensor(a[0] if squeeze else a, dtype=torch.float32).to(dev)
        dist.variational_mean.data = f[0] if squeeze else f
        dist.log_diag_precision_root.data = put(rho)
        dist.coupling.data = put(gamma)
        self.variational_strategy.variational_params_initialized.fill_(1)
        const = running_std.mean(-1).log()
        self.mean_module.constant.data = const[0] if squeeze else const.unsqueeze(-1)


def markov_startup_factor(x, vol, jitter, h, scale=100.0):
    """(rho, gamma) [T,N] of the bidiagonal Cholesky factor Lp (diagonal e^rho, sub-diagonal gamma e^rho) of the tridiagonal
    P0 = (K_M^-1 + diag(h)) / scale, K_M = vol min(x, x') + jitter 1 1': K_M^-1 has diagonal 1/q_i + 1/q_{i+1} (1/q_{N-1} at the
    end) and off-diagonal -1/q_{i+1}.  numpy fp64: x [N], vol [1] or [T], h [T,N].  O(T N) time and memory; gamma[:, N-1] = 0."""
    import numpy as np
    T, N = h.shape
    q = np.empty((np.size(vol), N))
    q[:, 0] = vol * x[0] + jitter
    q[:, 1:] = vol[:, None] * np.diff(x)[None, :]
    iq = 1.0 / q
    diag = (iq + h) / scale                                                                # [T,N]
    diag[:, :-1] += iq[:, 1:] / scale
    off = np.broadcast_to(-iq[:, 1:] / scale, (T, N - 1))                                  # P0[i+1, i]
    rho, gamma = np.zeros((T, N)), np.zeros((T, N))
    l2 = diag[:, 0].copy()                                                                 # Lp_ii^2
    for i in range(N):
        rho[:, i] = 0.5 * np.log(l2)
        if i + 1 < N:
            g = off[:, i] / l2
            gamma[:, i] = g
            l2 = diag[:, i + 1] - g * g * l2
    return rho, gamma
