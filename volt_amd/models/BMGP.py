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
from ..gp import (ExactGP, MultitaskMultivariateNormal, MultivariateNormal, NanError, NotPSDError, _BrownianPrior, _KroneckerPrior,
                  _MarkovCov, _markov_cov, _safe_factor, check_grid, same_values)
from ..kernels.BMKernel import BMKernel
from ..kernels.FBMKernel import FBMKernel
from ..kernels.MultitaskKernel import MultitaskKernel


def _check_posterior(who, posterior, solver):
    if posterior not in BMGP.POSTERIORS:
        raise ValueError(f"{who}: posterior must be one of {BMGP.POSTERIORS}, got {posterior!r}")
    if posterior != "solve" and solver != "linear":
        raise ValueError(f"{who}: posterior={posterior!r} needs solver='linear' (the dense solver has one posterior)")


def _sort_order(xs, order):
    """``order`` (the permutation that sorted xs), or None where xs was ascending already (ONE host read): the chain draw then
    skips the gather of z and the scatter of the result."""
    if xs.shape[0] < 2 or bool((xs[1:] >= xs[:-1]).all()):
        return None
    return order


def _check_post_info(info, order, who, params, not_psd):
    """ONE host read of ops.bm_post's info.  NaN / inf parameters (``params``: tensors looked at only on failure) are a
    NanError before a failed pivot is a NotPSDError; a negative code names the offending test point by its index in the
    caller's order (``order``: the sort's permutation)."""
    info = info.tolist()
    if not any(info):
        return
    if not all(bool(torch.isfinite(p).all()) for p in params):
        raise NanError(f"{who} posterior: NaN / inf in the targets or the parameters")
    code = next(i for i in info if i)
    if code < 0:
        raise ValueError(f"{who} posterior: test point {int(order[-code - 1])} is NaN / inf or negative "
                         "(Brownian motion starts at x = 0)")
    raise NotPSDError(f"{who} posterior: {not_psd}")


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
    SOLVERS = ("dense", "linear")
    POSTERIORS = ("solve", "sweep", "chain")
    _POST_CHUNK = 4096                        # rows of K_t* per fp64 product of the linear posterior (bounds its temporaries)

    def __init__(self, train_x, train_y, likelihood, kernel="bm", solver="dense", posterior="solve"):
        if solver not in self.SOLVERS:
            raise ValueError(f"BMGP: solver must be one of {self.SOLVERS}, got {solver!r}")
        _check_posterior("BMGP", posterior, solver)
        if solver == "linear" and kernel != "bm":
            raise ValueError(f"BMGP: solver='linear' needs kernel='bm' (Brownian motion is Markov; kernel {kernel!r} is not)")
        if solver == "linear":
            if train_x.ndim != 1:
                raise ValueError(f"BMGP(solver='linear'): the grid must be 1-D [N], got shape {tuple(train_x.shape)}")
            check_grid(train_x, "BMGP(solver='linear')")
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

    def _posterior_linear(self, x):
        """mean* = m(x*) + K_*t alpha and cov = K_** - K_*t A^-1 K_t* with alpha from the linear-time step (fp64) and
        A^-1 K_t* from the linear-time solve in the model's dtype (R = K_t* [T,N,H]); the two products over N are
        accumulated in fp64, a block of rows at a time.  Returned in the model's dtype."""
        with torch.no_grad():
            xt = self.train_inputs[0][:, 0]
            y = self.train_targets
            batched = y.ndim > 1
            T = y.shape[0] if batched else 1
            n = xt.shape[0]
            xs = x[:, 0] if x.ndim > 1 else x
            H = xs.shape[0]
            dt = torch.float64 if y.dtype == torch.float64 else torch.float32
            vol = self.covar_module.vol.reshape(-1).expand(T)
            noise = self.likelihood.noise.reshape(-1).expand(T)
            resid = (y - self.mean_module(xt)).reshape(T, n)
            # alpha in fp64 (the residual upcast) and K_*t rebuilt in fp64 block by block below: K_*t alpha sums N terms of
            # either sign, so an fp32 rounding of alpha or of K_*t would come back multiplied by sum |alpha_i| K_i
            x64, xs64, vol64 = xt.double(), xs.double(), vol.double().reshape(T, 1, 1)
            # (the workspaces, (1 + H) T N doubles, live for this call only: a forecast takes one posterior per fit)
            _, alpha, info = ops.bm_step(x64, vol, noise, resid.double())
            if int((info != 0).sum().item()):
                if not bool(torch.isfinite(vol).all()) or not bool(torch.isfinite(noise).all()):
                    raise NanError("BMGP posterior: NaN / inf in the kernel's vol or the noise")
                raise NotPSDError("BMGP posterior: vol min(x, x') + sigma^2 I is not positive definite (the noise must be positive)")
            Kts = vol.to(dt).reshape(T, 1, 1) * torch.minimum(xt.to(dt).unsqueeze(-1), xs.to(dt).unsqueeze(-2))     # [T,N,H]
            X, _ = ops.bm_solve(xt, vol, noise, Kts)
            mean_c = torch.zeros(T, H, dtype=torch.float64, device=xt.device)
            S = torch.zeros(T, H, H, dtype=torch.float64, device=xt.device)
            for lo in range(0, n, self._POST_CHUNK):
                Kc = vol64 * torch.minimum(x64[lo:lo + self._POST_CHUNK].unsqueeze(-1), xs64.unsqueeze(-2))    # [T,c,H]
                mean_c += torch.einsum("tnh,tn->th", Kc, alpha[:, lo:lo + self._POST_CHUNK])
                S += Kc.mT @ X[:, lo:lo + self._POST_CHUNK].double()
            Kss = vol64 * torch.minimum(xs64.unsqueeze(-1), xs64.unsqueeze(-2))
            mean = (self.mean_module(x).double().reshape(T, H) + mean_c).to(dt)
            cov = (Kss - S).to(dt)
            if not batched:
                mean, cov = mean[0], cov[0]
            return MultivariateNormal(mean, cov)

    def _posterior_sweep(self, x):
        """The same posterior from ONE ops.bm_post launch over the sorted test points (any order and duplicates accepted:
        sorted on the device, the order restored on the way out) and one host read of its info: mean* = m(x*) + m_h,
        var = v xi_h - p_h, cov of neighbours = v xi_h - q_h, the rest by gp._markov_cov; fp64 throughout (the upcasts of
        `_posterior_linear`), rounded once to the model's dtype."""
        with torch.no_grad():
            xt = self.train_inputs[0][:, 0]
            y = self.train_targets
            batched = y.ndim > 1
            T = y.shape[0] if batched else 1
            n = xt.shape[0]
            xs = x[:, 0] if x.ndim > 1 else x
            H = xs.shape[0]
            dt = torch.float64 if y.dtype == torch.float64 else torch.float32
            vol = self.covar_module.vol.reshape(-1).expand(T)
            noise = self.likelihood.noise.reshape(-1).expand(T)
            resid = (y - self.mean_module(xt)).reshape(T, n)
            xs64, order = torch.sort(xs.double())
            out, info = ops.bm_post(xt.double(), xs64, vol, noise, resid.double())
            _check_post_info(info, order, "BMGP", (vol, noise, y),
                             "vol min(x, x') + sigma^2 I is not positive definite (the noise must be positive)")
            prior = vol.double().reshape(T, 1) * xs64
            mean_s = self.mean_module(xs64).reshape(T, H) + out[:, 0]
            if self.posterior == "chain":                      # the same forms, the covariance left lazy
                mean = torch.empty_like(mean_s)
                mean[:, order] = mean_s
                diag, off = prior - out[:, 1], prior - out[:, 2]
                if not batched:
                    mean, diag, off = mean[0], diag[0], off[0]
                return MultivariateNormal(mean.to(dt), _MarkovCov(diag, off, _sort_order(xs, order), dtype=dt, mean=mean))
            cov_s = _markov_cov(prior - out[:, 1], prior - out[:, 2])
            mean = torch.empty_like(mean_s)
            mean[:, order] = mean_s
            cov = torch.empty_like(cov_s)
            cov[:, order.unsqueeze(-1), order.unsqueeze(0)] = cov_s
            mean, cov = mean.to(dt), cov.to(dt)
            if not batched:
                mean, cov = mean[0], cov[0]
            return MultivariateNormal(mean, cov)

    def posterior_call(self, x):
        """Exact-GP posterior at the test points: K_s = L L' on the HIP potrf, K_s^-1 = Y Y' with Y = L^-T from the HIP
        triangular inverse, every product on the library GEMM.  One series -> MultivariateNormal(mean [H], cov [H,H]);
        T series over the shared grid -> (mean [T,H], cov [T,H,H]).  solver="linear": _posterior_linear, or _posterior_sweep
        with posterior="sweep" / "chain"."""
        if self.solver == "linear":
            return self._posterior_linear(x) if self.posterior == "solve" else self._posterior_sweep(x)
        with torch.no_grad():
            from ..gp import _dense
            xt = self.train_inputs[0]
            y = self.train_targets
            batched = y.ndim > 1
            T = y.shape[0] if batched else 1
            n, H = xt.shape[0], x.shape[0]
            Ktt = _dense(self.covar_module(xt, xt)).reshape(T, n, n)
            noise = self.likelihood.noise.reshape(-1).expand(T)
            A = Ktt + noise.reshape(T, 1, 1) * torch.eye(n, device=xt.device)
            f, _ = _safe_factor(A)
            Linv = ops.trtri(f).mT.contiguous()                                            # L^-1, rows K-contiguous
            Kst = _dense(self.covar_module(x, xt)).reshape(T, H, n)
            G = ops.gemm_nt(Kst, Linv, uplo_b=1)                                           # K_*t L^-T
            r = (y - self.mean_module(xt)).to(torch.float32).reshape(T, 1, n)
            w = ops.gemm_nt(r, Linv, uplo_b=1)                                             # (L^-1 r)'
            mean = self.mean_module(x).reshape(T, H) + ops.gemm_nt(G, w).reshape(T, H)
            cov = _dense(self.covar_module(x, x)).reshape(T, H, H) - ops.gemm_nt(G, G)
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
    SOLVERS = BMGP.SOLVERS
    POSTERIORS = BMGP.POSTERIORS
    _POST_CHUNK = BMGP._POST_CHUNK
    _POST_SOLVE_ELEMS = 1 << 19               # directions x N x points per solve of the linear posterior (bounds its three buffers)

    def __init__(self, train_x, train_y, likelihood, base_mean=None, solver="dense", posterior="solve", **kwargs):
        if solver not in self.SOLVERS:
            raise ValueError(f"MultitaskBMGP: solver must be one of {self.SOLVERS}, got {solver!r}")
        _check_posterior("MultitaskBMGP", posterior, solver)
        if solver == "linear":
            if train_x.ndim != 1:
                raise ValueError(f"MultitaskBMGP(solver='linear'): the grid must be 1-D [N], got shape {tuple(train_x.shape)}")
            check_grid(train_x, "MultitaskBMGP(solver='linear')")
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

    def _posterior_linear(self, x):
        """`posterior_call` without any N x N matrix: the cold fp64 prologue as there; alpha_j from the linear-time step in
        fp64; X_j = (M + sigma_j^2 I)^-1 M_x* from the linear-time solve; m~_j = sqrt(kappa_j) M_*x alpha_j and
        C_j = kappa_j (M_** - M_*x X_j), the two products over N accumulated in fp64 over blocks of rows as
        BMGP._posterior_linear does.  Returned in fp32, like the dense posterior."""
        with torch.no_grad():
            xt = self.train_inputs[0][:, 0]
            Y = self.train_targets
            n, T = Y.shape
            xs = x[..., 0] if x.ndim > 1 else x
            H = xs.shape[0]
            dev = xt.device
            if self._post_ws is None or not self._post_ws.fits(n, T, dev, torch.float64, "linear"):
                self._post_ws = ops.KronWorkspace(n, T, dev, torch.float64, "linear")
            ws = self._post_ws
            task, data = self.covar_module.task_covar_module, self.covar_module.data_covar_module
            params = (data.raw_vol, task.covar_factor, task.raw_var, self.likelihood.raw_task_noises, self.likelihood.raw_noise)
            x64, xs64 = xt.double(), xs.double()
            ops.kron_prologue(params, x64, Y, ws)
            kap = ws.state[0] * ws.lam()                                                   # [T], fp64
            _, alpha, info = ops.bm_step(x64, ws.ones, ws.sigma2, ws.resid, ws.bm, want_grad=True)
            if int((info != 0).sum().item()):
                if not all(bool(torch.isfinite(p).all()) for p in params) or not bool(torch.isfinite(Y).all()):
                    raise NanError("MultitaskBMGP posterior: NaN / inf in the targets or the parameters")
                raise NotPSDError("MultitaskBMGP posterior: M + sigma_j^2 I is not positive definite")
            mt = torch.zeros(T, H, dtype=torch.float64, device=dev)
            S = torch.zeros(T, H, H, dtype=torch.float64, device=dev)
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
                    X, _ = ops.bm_solve(x64, ws.ones[j:j + jb], ws.sigma2[j:j + jb], rhs)
                    for lo in range(0, n, self._POST_CHUNK):
                        S[j:j + jb, :, h:h + hb] += m_sx(lo, lo + self._POST_CHUNK).unsqueeze(0) @ X[:, lo:lo + self._POST_CHUNK]
                    del X
            mt = kap.sqrt().reshape(T, 1) * mt                                             # m~_j
            Mss = torch.minimum(xs64.unsqueeze(-1), xs64.unsqueeze(-2))
            C = (kap.reshape(T, 1, 1) * (Mss.unsqueeze(0) - S)).to(torch.float32)
            V64 = ws.d().sqrt().unsqueeze(-1) * ws.Q()                                     # D^1/2 Q
            mean = (self.mean_module(xs).double() + mt.t() @ V64.t()).to(torch.float32)
            return MultitaskMultivariateNormal(mean, blocks=(V64.to(torch.float32), C))

    def _posterior_sweep(self, x):
        """`_posterior_linear` with the T chain solves and the products over N replaced by ONE ops.bm_post launch over the
        sorted test points (unit vol, the directions' sigma_j^2 and residuals of the cold fp64 prologue) and one host read of
        its info: m~_j = sqrt(kappa_j) m_j and C_j = kappa_j markov_cov(xi - p_j, xi - q_j); the assembly is unchanged."""
        with torch.no_grad():
            xt = self.train_inputs[0][:, 0]
            Y = self.train_targets
            n, T = Y.shape
            xs = x[..., 0] if x.ndim > 1 else x
            dev = xt.device
            if self._post_ws is None or not self._post_ws.fits(n, T, dev, torch.float64, "linear"):
                self._post_ws = ops.KronWorkspace(n, T, dev, torch.float64, "linear")
            ws = self._post_ws
            task, data = self.covar_module.task_covar_module, self.covar_module.data_covar_module
            params = (data.raw_vol, task.covar_factor, task.raw_var, self.likelihood.raw_task_noises, self.likelihood.raw_noise)
            x64 = xt.double()
            ops.kron_prologue(params, x64, Y, ws)
            kap = ws.state[0] * ws.lam()                                                   # [T], fp64
            xs64, order = torch.sort(xs.double())
            out, info = ops.bm_post(x64, xs64, ws.ones, ws.sigma2, ws.resid)
            _check_post_info(info, order, "MultitaskBMGP", params + (Y,), "M + sigma_j^2 I is not positive definite")
            mt_s = kap.sqrt().reshape(T, 1) * out[:, 0]                                    # m~_j over the sorted points
            V64 = ws.d().sqrt().unsqueeze(-1) * ws.Q()                                     # D^1/2 Q
            if self.posterior == "chain":                      # the same forms, the blocks C_j left lazy
                mt = torch.empty_like(mt_s)
                mt[:, order] = mt_s
                mean = (self.mean_module(xs).double() + mt.t() @ V64.t()).to(torch.float32)
                C = _MarkovCov(xs64 - out[:, 1], xs64 - out[:, 2], _sort_order(xs, order), scale=kap, dtype=torch.float32)
                return MultitaskMultivariateNormal(mean, blocks=(V64.to(torch.float32), C))
            C_s = kap.reshape(T, 1, 1) * _markov_cov(xs64 - out[:, 1], xs64 - out[:, 2])
            mt = torch.empty_like(mt_s)
            mt[:, order] = mt_s
            C = torch.empty_like(C_s)
            C[:, order.unsqueeze(-1), order.unsqueeze(0)] = C_s
            mean = (self.mean_module(xs).double() + mt.t() @ V64.t()).to(torch.float32)
            return MultitaskMultivariateNormal(mean, blocks=(V64.to(torch.float32), C.to(torch.float32)))

    def posterior_call(self, x):
        """Exact latent posterior at x [H] (gpytorch's eval-mode ExactGP call): a MultitaskMultivariateNormal with mean [H,T].
        Block by block in the eigenbasis of the task covariance: the prologue (fp64) gives W, Lambda and
        r_j; then per block m~_j = sqrt(kappa_j) M_*x (M + sigma_j^2 I)^-1 r_j and C_j = kappa_j [M_** - M_*x (M +
        sigma_j^2 I)^-1 M_x*] on the HIP potrf / triangular inverse / GEMM, as BMGP.posterior_call does; finally
        mean = mu_* + m~ V' and cov = (I (x) V) blockdiag(C_j) (I (x) V'), V = D^1/2 Q.  solver="linear": _posterior_linear, or
        _posterior_sweep with posterior="sweep" / "chain"."""
        if self.solver == "linear":
            return self._posterior_linear(x) if self.posterior == "solve" else self._posterior_sweep(x)
        with torch.no_grad():
            xt = self.train_inputs[0][:, 0]
            Y = self.train_targets
            n, T = Y.shape
            xs = x[..., 0] if x.ndim > 1 else x
            H = xs.shape[0]
            dev = xt.device
            if self._post_ws is None or self._post_ws.state.device != dev:
                self._post_ws = ops.KronWorkspace(n, T, dev, torch.float64)
            ws = self._post_ws
            task, data = self.covar_module.task_covar_module, self.covar_module.data_covar_module
            params = (data.raw_vol, task.covar_factor, task.raw_var, self.likelihood.raw_task_noises, self.likelihood.raw_noise)
            ops.kron_prologue(params, xt, Y, ws)
            kap = (ws.state[0] * ws.lam()).to(torch.float32)                               # [T]
            M = self._base.to(torch.float32)
            A = M.unsqueeze(0) + ws.sigma2.to(torch.float32).reshape(T, 1, 1) * torch.eye(n, device=dev)
            f, _ = _safe_factor(A)
            Linv = ops.trtri(f).mT.contiguous()                                            # L_j^-1
            xs32, xt32 = xs.to(torch.float32), xt.to(torch.float32)
            Mst = torch.minimum(xs32.unsqueeze(-1), xt32.unsqueeze(-2)).expand(T, H, n).contiguous()
            G = ops.gemm_nt(Mst, Linv, uplo_b=1)                                           # M_*x L^-T
            w = ops.gemm_nt(ws.resid.to(torch.float32).reshape(T, 1, n), Linv, uplo_b=1)   # (L^-1 r)'
            mt = kap.sqrt().reshape(T, 1) * ops.gemm_nt(G, w).reshape(T, H)               # m~_j
            Mss = torch.minimum(xs32.unsqueeze(-1), xs32.unsqueeze(-2))
            C = kap.reshape(T, 1, 1) * (Mss.unsqueeze(0) - ops.gemm_nt(G, G))
            V = (ws.d().sqrt().unsqueeze(-1) * ws.Q()).to(torch.float32)                   # D^1/2 Q
            mean = self.mean_module(xs).to(torch.float32) + ops.gemm_nt(mt.t().contiguous(), V)
            return MultitaskMultivariateNormal(mean, blocks=(V, C))
