"""MultitaskVariationalGP, voltron/models/multi_task_variational_gp.py:11-146 -- the joint GPCV model of T series that
share one time grid: q(F) = N(M, S_x (x) S_t) against the Kronecker prior N(mu, K_x (x) K_t), inducing points fixed at
the inputs.  Parameter names, shapes, registration order and start values are the reference's; the ELBO and all of its
gradients come from ONE HIP step that factors K_x once for all T series: volt_gpcv_mt_step_f32 for the "exp" likelihood,
volt_gpcv_mt_cv_step_f32 for the copula-process ("cv") one with one warp per task (a likelihood built with
``batch_shape=[num_tasks]``).

Stated differences from the reference file (README, quirk table):
* ``model(x)`` is defined at the inducing points only, where the reference's three-term covariance (:113-146) collapses
  to S_x (x) S_t and its mean to M (K_uu^-1 K_ux = I); anything else raises NotImplementedError.
* the prior's data block carries the single-task path's jitter 1e-3 (variational.PRIOR_JITTER); the reference adds none
  (:95-111) and leans on gpytorch's jitter ladder when x[0] = 0 makes K_x[0,0] = 0.
* rank=1, fp32; param="cv" with one warp per task only (an unbatched "cv" likelihood, one warp shared by all tasks, has no
  accelerated ELBO), and its start-up values for K = 1 only, as for SingleTaskVariationalGP.
* ``prior_solver="markov"`` (keyword-only; the default "dense" is everything above, unchanged): the joint model in
  O(N T (Q + T) + T^3) time and O(N T) memory (csrc/gpcv_mt_markov.hip, volt_gpcv_mt_markov_step_f32).  The data
  kernel must be a BMKernel over a grid 0 <= x_0 < x_1 < .. (validated once); the prior's data block is Brownian motion
  started from an N(0, 1e-3) LEVEL, K_M = vol min(x, x') + 1e-3 1 1' (not K_x + 1e-3 I, whose diagonal jitter destroys the
  Markov structure), and the variational family is q(F) = N(M, P^-1 (x) S_t) with a TRIDIAGONAL precision P = Lp Lp':
  parameters ``variational_mean`` [N,T], ``log_diag_precision_root`` [N], ``coupling`` [N] (its last entry is never read),
  ``variational_task_covar_root`` [T,T] -- there is no ``variational_covar_root``.  The start-up values take an O(N T) route
  (``_initialize_markov``); no N x N tensor exists anywhere on this route.  This solver alone also answers AWAY from the
  inducing grid: ``model(x)`` for any x [H] or [H,1] >= 0 returns ``MultitaskMarkovPredictiveLatent`` over [H,T] (mean,
  variance, joint draws; csrc/markov_predict.hip); ``prior_solver="dense"`` keeps raising there.
The reference has no trainer for this class; train_utils.FitGPCVMultitask is LearnGPCV's loop over it.  gpytorch is not
installed here; both branches of ``initialize_variational_parameters`` are pinned to the reference's own code, executed
over stand-ins, by tests/golden/mt_gpcv_cv.npz."""
import torch
from torch import nn

from .. import ops
from ..gp import ConstantMean, EqualMemo, Module, MultitaskMean, _dense, check_grid
from ..safe import _safe_factor
from ..kernels.BMKernel import BMKernel
from ..kernels.MultitaskKernel import IndexKernel
from ..variational import (MIN_VARIANCE, PRIOR_JITTER, MultitaskMarkovPredictiveLatent, MultitaskMarkovVariationalLatent,
                           MultitaskVariationalLatent, _gauss_hermite, _predict_points)
from .single_task_variational_gp import markov_startup_factor


class MultitaskVariationalGP(Module):
    PRIOR_SOLVERS = ("dense", "markov")

    def __init__(self, inducing_points, num_tasks, covar_module=None, rank=1, *, prior_solver="dense", **kwargs):
        super().__init__()
        if prior_solver not in self.PRIOR_SOLVERS:
            raise ValueError(f"MultitaskVariationalGP: prior_solver must be one of {self.PRIOR_SOLVERS}, got {prior_solver!r}")
        if rank != 1:
            raise NotImplementedError("MultitaskVariationalGP: only the rank-1 IndexKernel has an accelerated ELBO")
        if covar_module is None:
            raise NotImplementedError("pass covar_module (BMKernel / FBMKernel): the data kernel of the Kronecker prior")
        ops._check_tasks(num_tasks)
        n = inducing_points.shape[-1]
        if prior_solver == "markov":
            if not isinstance(covar_module, BMKernel):
                raise ValueError(f"MultitaskVariationalGP: prior_solver='markov' needs covar_module=BMKernel (Brownian motion "
                                 f"is Markov; {type(covar_module).__name__} is not)")
            if inducing_points.ndim != 1:
                raise ValueError("MultitaskVariationalGP(prior_solver='markov'): the inducing grid must be [N], got shape "
                                 f"{tuple(inducing_points.shape)}")
            check_grid(inducing_points, "MultitaskVariationalGP(prior_solver='markov')")
        self.prior_solver = prior_solver
        # registration and draw order of the reference's __init__ (:15-36): the mean's randn comes before IndexKernel's two
        self.register_parameter("variational_mean", nn.Parameter(0.01 * torch.randn(n, num_tasks), requires_grad=True))
        if prior_solver == "markov":                             # the tridiagonal precision root, 0 / I like the dense one
            self.register_parameter("log_diag_precision_root", nn.Parameter(torch.zeros(n), requires_grad=True))
            self.register_parameter("coupling", nn.Parameter(torch.zeros(n), requires_grad=True))
        else:
            self.register_parameter("variational_covar_root", nn.Parameter(torch.eye(n), requires_grad=True))
        self.register_parameter("variational_task_covar_root", nn.Parameter(torch.eye(num_tasks), requires_grad=True))
        self.index_kernel = IndexKernel(num_tasks=num_tasks, rank=rank, **kwargs)
        self.data_kernel = covar_module
        self.inducing_points = inducing_points
        self.num_tasks = num_tasks
        self.mean_module = MultitaskMean(ConstantMean(), num_tasks=num_tasks)
        object.__setattr__(self, "_eq_memo", EqualMemo())
        object.__setattr__(self, "_kl_ws", None)
        self.to(inducing_points.device)

    @property
    def variational_strategy(self):
        return self                                              # "hacky af for now" (:90-93): the ELBO asks it for the KL

    def _task_params(self):
        c = torch.cat([m.constant.reshape(1) for m in self.mean_module.base_means])
        return c, self.index_kernel.covar_factor, self.index_kernel.raw_var

    def kl_divergence(self):
        """KL(q || p) (:95-111), from the HIP step (no likelihood term: one quadrature node, y = 0)."""
        M = self.variational_mean
        if not M.is_cuda:
            raise ops._lib.VoltHipError("MultitaskVariationalGP.kl_divergence: tensors must live on the MI355X; no CPU fallback")
        n, T = M.shape
        if self.prior_solver == "markov":
            with torch.no_grad():
                c, cf, rv = self._task_params()
                gx, gw = _gauss_hermite(1, M.device)
                ws = self._kl_ws
                if ws is None or not ws.fits(n, T, M.device):
                    ws = ops.GpcvMtMarkovWorkspace(n, T, M.device)
                    object.__setattr__(self, "_kl_ws", ws)
                ops.gpcv_mt_markov_step(self.inducing_points, self.data_kernel.vol, M, c, self.log_diag_precision_root,
                                        self.coupling, self.variational_task_covar_root, cf, rv, torch.zeros_like(M), gx, gw,
                                        ws, jitter=PRIOR_JITTER, min_var=MIN_VARIANCE)
                return ws.out[1].clone()
        with torch.no_grad():
            K = _dense(self.data_kernel(self.inducing_points)).to(torch.float32)
            c, cf, rv = self._task_params()
            gx, gw = _gauss_hermite(1, M.device)
            ws = self._kl_ws
            if ws is None or ws.N != n or ws.T != T or ws.buf.device != M.device:
                ws = ops.GpcvMtWorkspace(n, T, False, M.device)
                object.__setattr__(self, "_kl_ws", ws)
            ops.gpcv_mt_step(K, M, c, self.variational_covar_root, self.variational_task_covar_root, cf, rv,
                             torch.zeros_like(M), gx, gw, ws, jitter=PRIOR_JITTER, min_var=MIN_VARIANCE)
            return ws.out[1].clone()

    def forward(self, x, **kwargs):
        raise NotImplementedError("MultitaskVariationalGP.forward(x) away from the inducing points (:113-146) is outside "
                                  "the accelerated path; call model(inducing_points)")

    def __call__(self, x, **kwargs):
        Z = self.inducing_points
        xs = x.reshape(Z.shape) if x.numel() == Z.numel() else x
        if xs.shape == Z.shape and self._eq_memo.equal(x, Z, lambda: torch.equal(xs, Z)):
            return MultitaskMarkovVariationalLatent(self) if self.prior_solver == "markov" else MultitaskVariationalLatent(self)
        if self.prior_solver == "markov":                        # away from the grid: O(N + H) on the x side
            return MultitaskMarkovPredictiveLatent(self, _predict_points(x, "MultitaskVariationalGP(prior_solver='markov')"))
        return self.forward(x, **kwargs)

    def initialize_variational_parameters(self, likelihood, x, f=None, y=None):
        """:38-88.  y [N,T]: S_root = L C^-T with L = chol(K_uu), C = chol(L' H L + I), H the mean over tasks of the inverse
        Hessians; stored as the reference stores it -- 10 * S_root, a FULL matrix of which only tril() is ever used.
        (gpytorch's root_inv_decomposition is taken on its Cholesky route.)
        "exp": mean = log running std of each column, H clamped to [1e-4, 1000] AFTER diag_embed, so its off-diagonal 1e-4
        survives the mean.
        "cv" (:58-69, one warp per task, K = 1 only) with the reference's quirks kept: ``y = f.t()`` replaces the returns by
        the log running std, mean = ((y/a).exp() - 1 - c)/b, sigma from the likelihood's own forward, and NO clamp on the
        diag_embed-ed inverse Hessian, so the mean over tasks keeps zeros off the diagonal.  The reference's ``y / trans_a``
        divides [T,N] by [T,K], a broadcast that only works for K = 1: K > 1 raises here."""
        param = getattr(likelihood, "param", "exp")
        if param not in ("exp", "cv"):
            raise NotImplementedError(f"unknown volatility likelihood parameterisation {param!r}")
        if param == "cv":
            if tuple(likelihood.raw_a.shape[:-1]) != (self.num_tasks,):
                raise NotImplementedError('the multi-task "cv" start-up needs one warp per task: build the likelihood with '
                                          f"batch_shape=[num_tasks] = [{self.num_tasks}]")
            if likelihood.raw_a.shape[-1] != 1:
                raise NotImplementedError('the "cv" initialisation divides y [T,N] by trans_a [T,K] '
                                          "(multi_task_variational_gp.py:60: `y / likelihood.trans_a`), a broadcast that only "
                                          f"works for K = 1; K = {likelihood.raw_a.shape[-1]} has no start-up values")
        assert y is not None
        markov = self.prior_solver == "markov"
        with torch.no_grad():
            if not markov:
                kuu = _dense(self.data_kernel(self.inducing_points)).to(torch.float32)
            y2 = y.to(torch.float32)
            N, T = y2.shape
            # running std of y[:i] (unbiased) per column, one prefix-sum pass instead of the reference's N slices
            idx = torch.arange(N, device=y2.device, dtype=torch.float64).unsqueeze(-1)
            zero = torch.zeros(1, T, dtype=torch.float64, device=y2.device)
            s1 = torch.cat([zero, torch.cumsum(y2.double(), 0)[:-1]], 0)
            s2 = torch.cat([zero, torch.cumsum(y2.double() ** 2, 0)[:-1]], 0)
            var = (s2 - s1 * s1 / idx.clamp_min(1)) / (idx - 1).clamp_min(1)
            running_std = var.clamp_min(0).sqrt().to(torch.float32)
            running_std[:10] = running_std[10]
            if f is None:
                f = running_std.clamp(min=1e-4).log()
            if param == "exp":
                # torch.diag_embed(...).clamp(min=1e-4, max=1000.).mean(0): diagonal = mean of the clamped entries, elsewhere 1e-4
                h = (0.5 * y2.pow(-2.0) * (f * 2.0).exp()).T.clamp(min=1e-4, max=1000.0).mean(0)
                ih = None if markov else torch.full((N, N), 1e-4, device=y2.device)
            else:
                a, b, c = (p.detach().to(y2.device, torch.float32) for p in
                           (likelihood.trans_a, likelihood.trans_b, likelihood.trans_c))     # [T,1]
                yl = f.t()                                                                   # `y = f.t()`: the returns are gone
                ft = ((yl / a).exp() - 1 - c) / b                                            # [T,N]
                sigma = likelihood(ft).scale                         # plain-tensor forward: parameter set t meets row t
                scaling = ((2 + 3 * yl.pow(2.0)) * (a * b.pow(2.0) / 2)).pow(-1.0)
                h = (scaling * sigma.pow(2.0) * (1 + torch.cosh(b * yl + c))).mean(0)       # diag of diag_embed(.).mean(0)
                ih = None if markov else torch.zeros(N, N, device=y2.device)
                f = ft.t()
            if markov:
                return self._initialize_markov(h, f, running_std)
            ih.diagonal().copy_(h)
            L = _safe_factor(kuu.reshape(1, N, N))[0].L[0]                                   # kuu.cholesky()
            Lt = L.mT.contiguous()
            HL = ops.gemm_nt(ih, Lt, uplo_b=2)                                               # H L
            inner = ops.gemm_nt(Lt, HL.mT.contiguous(), uplo_a=2)                            # L' H L
            inner = inner + torch.eye(N, device=y2.device)                                   # .add_jitter(1.0)
            Yi = ops.trtri(_safe_factor(inner.reshape(1, N, N))[0])[0]                       # C^-T
            S_root = ops.gemm_nt(L.contiguous(), Yi.mT.contiguous(), uplo_a=1, uplo_b=1)     # L C^-T
            self.variational_covar_root.data = (S_root * 10.0).contiguous()
            self._initialize_mean_and_task_kernel(f, running_std)

    def _initialize_mean_and_task_kernel(self, f, running_std):
        """What both start-up routes share (:80-88): the variational mean, the mean constants, covar_factor / 10."""
        self.variational_mean.data = f.to(torch.float32).contiguous()
        log_means = running_std.clamp(min=1e-4).mean(0).log()
        for i, m in enumerate(self.mean_module.base_means):
            m.constant.data.add_(log_means[i])
        if type(self.index_kernel) is IndexKernel:
            # (`index_kernel.var.data /= 10.` at :87 divides a temporary, as in BMGP.py:39: a no-op)
            self.index_kernel.covar_factor.data /= 10.

    def _initialize_markov(self, h, f, running_std):
        """The start-up values of prior_solver="markov" in O(N T).  The dense route stores 10 * S_root with S_root S_root' =
        L (L'HL + I)^-1 L' = (K^-1 + H)^-1 for a diagonal H, so under the Markov prior K_M the precision of S_x is tridiagonal:
        P0 = (K_M^-1 + diag h) / 100, and (log_diag_precision_root, coupling) is its bidiagonal Cholesky factor
        (single_task_variational_gp.markov_startup_factor: one fp64 host loop over N).  h [N]: the mean over tasks that
        ``initialize_variational_parameters`` computed.  One quirk cannot be carried: the "exp" branch's clamp leaves 1e-4 OFF the
        diagonal of H, a dense rank-one term; here H is its diagonal only (DESIGN 4.19 says the same of the single-task model)."""
        Z = self.inducing_points
        x = Z.reshape(-1).double().cpu().numpy()
        vol = self.data_kernel.vol.detach().double().reshape(-1).cpu().numpy()            # [1]
        rho, gamma = markov_startup_factor(x, vol, PRIOR_JITTER, h.double().reshape(1, -1).cpu().numpy())
        put = lambda a: torch.as_tensor(a[0], dtype=torch.float32).to(Z.device)
        self.log_diag_precision_root.data = put(rho)
        self.coupling.data = put(gamma)
        self._initialize_mean_and_task_kernel(f, running_std)
