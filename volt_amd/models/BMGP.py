"""Brownian-motion GP over the log-volatility path -- voltron/models/BMGP.py:9-28.

SURVEY 8(f) row 1: it supplies ``pred_vol`` at voltron/rollout_utils.py:66 through
``model.vol_model(test_x).sample(...)``.  Training-mode call -> prior MVN (for an MLL); eval-mode
call -> exact-GP posterior at the test points, computed with the same HIP Cholesky / triangular
inverse as the data model (K_s^-1 = Y Y^T, Y = L^-T), the products on the library's own MFMA GEMM (ops.gemm_nt).
MultitaskBMGP (:30-56, botorch's KroneckerMultiTaskGP) is below: the vol forecaster of the batched models when they are
built with ``multitask_vol=True``; its MLL runs on the Kronecker step (gp._KronMLL, csrc/kron.hip; ``solver="linear"``: around
the linear-time chain step, csrc/kron_chain.hip).

Addition: ``train_y`` [T,N] builds T independent vol models over shared inputs in one object (batched kernel
parameter, noise and posterior) -- what the batched forecast driver trains instead of looping over tickers.
"""
import torch

from .. import ops
from ..gp import (ExactGP, MultitaskMultivariateNormal, MultivariateNormal, _BrownianPrior, _dense, _KroneckerPrior,
                  same_values)
from ..kernels.BMKernel import BMKernel
from ..kernels.FBMKernel import FBMKernel
from ..kernels.MultitaskKernel import MultitaskKernel
from ._posterior import POSTERIORS, SOLVERS, Chains, check_info, check_options, dense_products, sweep


class BMGP(ExactGP):
    """``solver="dense"`` (default): the N x N machinery of the data model.  ``solver="linear"`` (kernel "bm" only): Brownian
    motion is Markov, so the MLL step and the posterior solve run in O(N) on csrc/bm.hip (fp64 arithmetic, no N x N matrix
    anywhere) -- ``forward`` returns a lazy prior, ``posterior_call`` goes through ops.bm_step / ops.bm_solve.
    The training grid is validated ONCE here (one host read): 1-D, x_0 >= 0, strictly increasing.
    ``posterior`` (solver="linear" only): "solve" (default) conditions through ops.bm_step / ops.bm_solve on K_t* [T,N,H];
    "sweep" through ONE forward sweep (ops.bm_post) that forms the clipped increments of K_t* on the fly and
    rebuilds the H x H covariance from its diagonal and first off-diagonal (the posterior is Markov): nothing is N x H;
    "chain" is the same sweep with the covariance left lazy (gp._MarkovCov): samples come from ops.markov_draw in O(S H) and
    the H x H matrix is built only when ``.covariance_matrix`` / ``.variance`` is asked for."""
    SOLVERS = SOLVERS
    POSTERIORS = POSTERIORS
    _POST_CHUNK = 4096                        # rows of K_t* per fp64 product of the linear posterior (bounds its temporaries)

    def __init__(self, train_x, train_y, likelihood, kernel="bm", solver="dense", posterior="solve"):
        check_options("BMGP", solver, posterior, train_x, kernel)
        super().__init__(train_x, train_y, likelihood)
        kw = {"batch_shape": train_y.shape[:-1]} if train_y.ndim > 1 else {}
        if kernel == "bm":
            self.covar_module = BMKernel(**kw).to(train_x.device)
        elif kernel == "fbm":
            self.covar_module = FBMKernel(**kw).to(train_x.device)      # BMGP.py:15-16; dense d mll / d K path
        self.solver = solver
        self.posterior = posterior
        self.scaling = (train_x[1] - train_x[0])

    def mean_module(self, x):
        return -0.5 * self.covar_module.vol.pow(2.0) * x.squeeze()        # BMGP.py:20-21

    def forward(self, x):
        if self.solver == "linear":
            stored = self.train_inputs[0]
            if not same_values(x, stored) and not (x.ndim >= 2 and x.shape[-2:] == stored.shape
                                                   and torch.equal(x, stored.expand_as(x))):
                raise ValueError("BMGP(solver='linear'): the prior is over the training grid validated at construction")
            return MultivariateNormal(self.mean_module(x), _BrownianPrior(self.covar_module.vol, self.train_inputs[0][:, 0]))
        return MultivariateNormal(self.mean_module(x), self.covar_module(x))

    def _chains(self):
        """The T series as chains (models/_posterior.py): the kernel's vol, the likelihood's noise, the residual in fp64."""
        xt = self.train_inputs[0][:, 0]
        y = self.train_targets
        T = y.shape[0] if y.ndim > 1 else 1
        vol = self.covar_module.vol.reshape(-1).expand(T)
        noise = self.likelihood.noise.reshape(-1).expand(T)
        resid = (y - self.mean_module(xt)).reshape(T, xt.shape[0])
        if self.posterior == "solve":             # (this route looks at the parameters only, and says so)
            looked, nan = (vol, noise), "NaN / inf in the kernel's vol or the noise"
        else:
            looked, nan = (vol, noise, y), "NaN / inf in the targets or the parameters"
        return Chains(xt.double(), vol, noise, resid.double(), "BMGP", looked, nan,
                      "vol min(x, x') + sigma^2 I is not positive definite (the noise must be positive)")

    def _solve(self, x, ch, dt):
        """mean* = m(x*) + K_*t alpha and cov = K_** - K_*t A^-1 K_t* with alpha from the linear-time step (fp64: the residual
        upcast) and A^-1 K_t* from the linear-time solve in the model's dtype (R = K_t* [T,N,H]); the two products over N are
        accumulated in fp64, a block of rows at a time."""
        xt = self.train_inputs[0][:, 0]
        xs = x[:, 0] if x.ndim > 1 else x
        (T, n), H = ch.resid.shape, xs.shape[0]
        # alpha in fp64 and K_*t rebuilt in fp64 block by block below: K_*t alpha sums N terms of either sign, so an fp32
        # rounding of alpha or of K_*t would come back multiplied by sum |alpha_i| K_i
        x64, xs64, vol64 = ch.x, xs.double(), ch.vol.double().reshape(T, 1, 1)
        # (the workspaces, (1 + H) T N doubles, live for this call only: a forecast takes one posterior per fit)
        _, alpha, info = ops.bm_step(x64, ch.vol, ch.sigma2, ch.resid)
        check_info(info, ch)
        Kts = ch.vol.to(dt).reshape(T, 1, 1) * torch.minimum(xt.to(dt).unsqueeze(-1), xs.to(dt).unsqueeze(-2))     # [T,N,H]
        X, _ = ops.bm_solve(xt, ch.vol, ch.sigma2, Kts)
        mean_c = torch.zeros(T, H, dtype=torch.float64, device=xt.device)
        S = torch.zeros(T, H, H, dtype=torch.float64, device=xt.device)
        for lo in range(0, n, self._POST_CHUNK):
            Kc = vol64 * torch.minimum(x64[lo:lo + self._POST_CHUNK].unsqueeze(-1), xs64.unsqueeze(-2))    # [T,c,H]
            mean_c += torch.einsum("tnh,tn->th", Kc, alpha[:, lo:lo + self._POST_CHUNK])
            S += Kc.mT @ X[:, lo:lo + self._POST_CHUNK].double()
        Kss = vol64 * torch.minimum(xs64.unsqueeze(-1), xs64.unsqueeze(-2))
        return (self.mean_module(x).double().reshape(T, H) + mean_c).to(dt), (Kss - S).to(dt)

    def _posterior_dense(self, x, ch):
        """K_s = L L' on the HIP potrf, K_s^-1 = Y Y' with Y = L^-T from the HIP triangular inverse, every product on the library
        GEMM (_posterior.dense_products)."""
        xt = self.train_inputs[0]
        (T, n), H = ch.resid.shape, x.shape[0]
        A = _dense(self.covar_module(xt, xt)).reshape(T, n, n) + ch.sigma2.reshape(T, 1, 1) * torch.eye(n, device=xt.device)
        Kst = _dense(self.covar_module(x, xt)).reshape(T, H, n)
        m, S = dense_products(A, Kst, ch.resid.to(torch.float32).reshape(T, 1, n))
        return self.mean_module(x).reshape(T, H) + m.reshape(T, H), _dense(self.covar_module(x, x)).reshape(T, H, H) - S

    def posterior_call(self, x):
        """Exact-GP posterior at the test points.  One series -> MultivariateNormal(mean [H], cov [H,H]); T series over the
        shared grid -> (mean [T,H], cov [T,H,H]).  solver="dense": `_posterior_dense`; solver="linear": `_solve`, or with
        posterior="sweep" / "chain" _posterior.sweep -- mean* = m(x*) + m_h in fp64 (the upcasts of `_solve`), rounded once to the
        model's dtype."""
        with torch.no_grad():
            ch = self._chains()
            batched = self.train_targets.ndim > 1
            dt = torch.float64 if self.train_targets.dtype == torch.float64 else torch.float32
            if self.solver == "linear" and self.posterior != "solve":
                xs64 = (x[:, 0] if x.ndim > 1 else x).double()
                lazy = self.posterior == "chain"
                m, cov = sweep(ch, xs64, lazy, dt, batched=batched)
                mean = self.mean_module(xs64).reshape(m.shape) + m
                if not batched:
                    mean = mean[0]
                if lazy:
                    cov.mean = mean               # (fp64: a chain draw rounds once, at its output)
                return MultivariateNormal(mean.to(dt), cov)
            mean, cov = self._solve(x, ch, dt) if self.solver == "linear" else self._posterior_dense(x, ch)
            if not batched:
                mean, cov = mean[0], cov[0]
            return MultivariateNormal(mean, cov)


class MultitaskBMGP(ExactGP):
    """voltron/models/BMGP.py:30-56: train_x [N], train_y [N,T], a MultitaskGaussianLikelihood(T).  Covariance
    K_x (x) K_t (MultitaskKernel(BMKernel(), T), rank-1 IndexKernel), element (n, t) at n*T + t; mean
    mu[n,t] = -1/2 vol^2 x_n K_t[t,t] -- inter-task correlation left out of the mean on purpose, as the reference's comment
    says (:44-49).

    The reference subclasses botorch's KroneckerMultiTaskGP and then replaces its covariance module and deletes its mean
    module; what is left of botorch is ExactGP's plumbing.  Restated from botorch's published (2022-era, unpinned in
    setup.py) behaviour, not executed here: the inputs are stored as [N,1], the targets as [N,T], no outcome transform, no
    priors remain (botorch's own modules, which carried them, are replaced).  Parameters, in registration order:
    likelihood.raw_task_noises [T], likelihood.raw_noise [1], covar_module.task_covar_module.covar_factor [T,1],
    .task_covar_module.raw_var [T], covar_module.data_covar_module.raw_vol [1].

    Initial values: botorch builds (and the reference discards) modules of its own first, and those draw from the
    generator, so the reference's draws cannot be reproduced.  Here ``covar_factor = randn(T,1)`` then ``raw_var =
    randn(T)`` from torch's default generator, in that order; then, as in the reference (:38-40), ``covar_factor /= 10``
    while ``task_covar_module.var.data /= 10.`` divides a computed temporary and changes nothing.

    ``solver="dense"`` (default): M = min(x, x') is filled once and every eigen-direction is an N x N dense step.
    ``solver="linear"``: each direction's M + sigma_j^2 I is the tridiagonal chain of BMGP(solver="linear"), so the MLL step
    (ops.kron_bm_step) and the posterior run in O(T N + T^2 N) with no N x N matrix anywhere; ``forward`` returns
    the lazy prior over the training grid, which is validated ONCE here (one host read): 1-D, x_0 >= 0, strictly increasing.
    ``posterior`` (solver="linear" only): "solve" (default) or "sweep", as for BMGP -- one ops.bm_post launch for all
    eigen-directions instead of a chain solve per group of test points -- or "chain": the sweep with the blocks
    C_j left lazy, every L_j z_j of a draw from one ops.markov_draw launch."""
    SOLVERS = SOLVERS
    POSTERIORS = POSTERIORS
    _POST_CHUNK = BMGP._POST_CHUNK
    _POST_SOLVE_ELEMS = 1 << 19               # directions x N x points per solve of the linear posterior (bounds its three buffers)

    def __init__(self, train_x, train_y, likelihood, base_mean=None, solver="dense", posterior="solve", **kwargs):
        check_options("MultitaskBMGP", solver, posterior, train_x)
        super().__init__(train_x, train_y, likelihood)
        if train_y.ndim != 2:
            raise ValueError("MultitaskBMGP: train_y must be [N, T]")
        ops._check_tasks(train_y.shape[-1])
        self.covar_module = MultitaskKernel(BMKernel(), num_tasks=train_y.shape[-1], **kwargs).to(train_x.device)
        self.covar_module.task_covar_module.var.data /= 10.              # a computed property: no effect (BMGP.py:39)
        self.covar_module.task_covar_module.covar_factor.data /= 10.
        self.solver = solver
        self.posterior = posterior
        if solver == "dense":
            x = train_x.reshape(-1)
            self._base = torch.minimum(x.unsqueeze(-1), x.unsqueeze(-2))  # M = min(x_i, x_k): K_x = vol M, filled once
        self._post_ws = None

    def mean_module(self, x):
        if x.ndim == 1:
            x = x.unsqueeze(-1)
        scaled_mean = -0.5 * self.covar_module.data_covar_module.vol.pow(2.0) * x.repeat(1, self.covar_module.num_tasks)
        return scaled_mean * self.covar_module.task_covar_module.covar_matrix.evaluate().diag()

    def forward(self, x):
        xs = x[..., 0] if x.ndim > 1 else x
        if self.solver == "linear":
            stored = self.train_inputs[0]
            if not same_values(x, stored) and not (xs.shape == stored.shape[:1] and torch.equal(xs, stored[:, 0])):
                raise ValueError("MultitaskBMGP(solver='linear'): the prior is over the training grid validated at construction")
            return MultitaskMultivariateNormal(self.mean_module(xs), _KroneckerPrior(self.covar_module, stored[:, 0]))
        if same_values(x, self.train_inputs[0]):
            M = self._base
        else:
            M = torch.minimum(xs.unsqueeze(-1), xs.unsqueeze(-2))
        return MultitaskMultivariateNormal(self.mean_module(xs), _KroneckerPrior(self.covar_module, xs, M))

    def _chains(self):
        """The cold fp64 prologue on the model's cached workspace -> (the workspace: d, Q; kappa [T] fp64; the T
        eigen-directions as chains (models/_posterior.py): unit vol -- the linear workspace's ones --, sigma_j^2, r_j)."""
        xt = self.train_inputs[0][:, 0]
        Y = self.train_targets
        n, T = Y.shape
        if self._post_ws is None or not self._post_ws.fits(n, T, xt.device, torch.float64, self.solver):
            self._post_ws = ops.KronWorkspace(n, T, xt.device, torch.float64, self.solver)
        ws = self._post_ws
        task, data = self.covar_module.task_covar_module, self.covar_module.data_covar_module
        params = (data.raw_vol, task.covar_factor, task.raw_var, self.likelihood.raw_task_noises, self.likelihood.raw_noise)
        ops.kron_prologue(params, xt, Y, ws)
        ones = ws.ones if self.solver == "linear" else None                   # (the dense blocks fill M themselves)
        return ws, ws.state[0] * ws.lam(), Chains(xt.double(), ones, ws.sigma2, ws.resid, "MultitaskBMGP", params + (Y,),
                                                  "NaN / inf in the targets or the parameters",
                                                  "M + sigma_j^2 I is not positive definite")

    def _solve(self, xs, ws, ch):
        """Without any N x N matrix: alpha_j from the linear-time step in fp64; X_j = (M + sigma_j^2 I)^-1 M_x* from the
        linear-time solve; m_j = M_*x alpha_j and M_** - M_*x X_j, the two products over N accumulated in fp64 over blocks of
        rows as BMGP._solve does."""
        (T, n), H = ch.resid.shape, xs.shape[0]
        x64, xs64 = ch.x, xs.double()
        _, alpha, info = ops.bm_step(x64, ch.vol, ch.sigma2, ch.resid, ws.bm, want_grad=True)
        check_info(info, ch)
        mt = torch.zeros(T, H, dtype=torch.float64, device=x64.device)
        S = torch.zeros(T, H, H, dtype=torch.float64, device=x64.device)
        m_sx = lambda lo, hi, h0=0, h1=H: torch.minimum(xs64[h0:h1].unsqueeze(-1), x64[lo:hi].unsqueeze(-2))   # M_*x block
        for lo in range(0, n, self._POST_CHUNK):
            mt += alpha[:, lo:lo + self._POST_CHUNK] @ m_sx(lo, lo + self._POST_CHUNK).t()
        # the solve in groups of test points (at a large T, of directions too): its right-hand sides, X and workspace are
        # each [directions, N, points] doubles, and a solve costs the length of the chain however many columns ride on it
        jb = max(1, min(T, self._POST_SOLVE_ELEMS // n))
        hb = max(1, min(H, self._POST_SOLVE_ELEMS // (n * jb)))
        for j in range(0, T, jb):
            for h in range(0, H, hb):
                rhs = m_sx(0, n, h, h + hb).t().unsqueeze(0).expand(min(jb, T - j), n, min(hb, H - h))
                X, _ = ops.bm_solve(x64, ch.vol[j:j + jb], ch.sigma2[j:j + jb], rhs)
                for lo in range(0, n, self._POST_CHUNK):
                    S[j:j + jb, :, h:h + hb] += m_sx(lo, lo + self._POST_CHUNK).unsqueeze(0) @ X[:, lo:lo + self._POST_CHUNK]
                del X
        return mt, torch.minimum(xs64.unsqueeze(-1), xs64.unsqueeze(-2)).unsqueeze(0) - S

    def posterior_call(self, x):
        """Exact latent posterior at x [H] (gpytorch's eval-mode ExactGP call): a MultitaskMultivariateNormal with mean [H,T].
        Block by block in the eigenbasis of the task covariance: the prologue (fp64) gives W, Lambda and
        r_j; then per block m~_j = sqrt(kappa_j) M_*x (M + sigma_j^2 I)^-1 r_j and C_j = kappa_j [M_** - M_*x (M +
        sigma_j^2 I)^-1 M_x*]; finally mean = mu_* + m~ V' and cov = (I (x) V) blockdiag(C_j) (I (x) V'), V = D^1/2 Q.
        solver="dense": the blocks in fp32 on the HIP potrf / triangular inverse / GEMM (_posterior.dense_products), as
        BMGP's.  solver="linear": in fp64 from `_solve`, or with posterior="sweep" / "chain" from ONE ops.bm_post launch for all
        directions (_posterior.sweep; "chain": the blocks C_j left lazy), rounded once to fp32 like the dense posterior."""
        with torch.no_grad():
            xs = x[..., 0] if x.ndim > 1 else x
            ws, kap, ch = self._chains()
            (T, n), H = ch.resid.shape, xs.shape[0]
            V = ws.d().sqrt().unsqueeze(-1) * ws.Q()                                       # D^1/2 Q, fp64
            if self.solver == "linear":
                if self.posterior == "solve":
                    m, C = self._solve(xs, ws, ch)
                    C = (kap.reshape(T, 1, 1) * C).to(torch.float32)
                else:
                    m, C = sweep(ch, xs, self.posterior == "chain", torch.float32, scale=kap)
                mt = kap.sqrt().reshape(T, 1) * m                                          # m~_j
                mean = (self.mean_module(xs).double() + mt.t() @ V.t()).to(torch.float32)
                return MultitaskMultivariateNormal(mean, blocks=(V.to(torch.float32), C))
            kap, V = kap.to(torch.float32), V.to(torch.float32)
            s32 = ch.sigma2.to(torch.float32).reshape(T, 1, 1)
            A = self._base.to(torch.float32).unsqueeze(0) + s32 * torch.eye(n, device=xs.device)
            xs32, xt32 = xs.to(torch.float32), self.train_inputs[0][:, 0].to(torch.float32)
            Mst = torch.minimum(xs32.unsqueeze(-1), xt32.unsqueeze(-2)).expand(T, H, n).contiguous()
            m, S = dense_products(A, Mst, ch.resid.to(torch.float32).reshape(T, 1, n))
            mt = kap.sqrt().reshape(T, 1) * m.reshape(T, H)                                # m~_j
            Mss = torch.minimum(xs32.unsqueeze(-1), xs32.unsqueeze(-2))
            C = kap.reshape(T, 1, 1) * (Mss.unsqueeze(0) - S)
            mean = self.mean_module(xs).to(torch.float32) + ops.gemm_nt(mt.t().contiguous(), V)
            return MultitaskMultivariateNormal(mean, blocks=(V, C))
