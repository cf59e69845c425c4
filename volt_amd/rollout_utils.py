"""Posterior conditionals and sequential rollouts -- drop-in for voltron/rollout_utils.py.

``GeneratePrediction`` / ``Rollouts`` keep the reference's signatures, shapes, CPU-resident
``samples`` result and the in-place mutation of ``model`` between horizon steps
(rollout_utils.py:80-86; callers defend with copy.deepcopy, experiments/weather/GPGenerator.py:79).

Two engines compute the same conditional:

* ``engine="dense"`` -- the reference's algorithm line by line, on the device: at every horizon step
  fill S matrices of size (N+idx+1)^2, Cholesky-factor every train block, two solves, one draw
  (rollout_utils.py:26-48).  O(H S N^3); kept as the on-device restatement used by the parity tests.
* ``engine="bordered"`` (default) -- volt_rollout_* HIP kernels: the train block of every sample's
  matrix is identical (``train_stack_vol = log_vol_path.repeat(S,1)``, :72), so it is factored once
  and each sample only extends its own <= H x H bordered factor.  See DESIGN.md "Rollouts".

Extra keyword-only arguments (``pred_vol``, ``z``, ``engine``) let tests inject the vol-path
sample and the N(0,1) draws the reference takes from ``model.vol_model`` and ``torch.randn``.
``solver="linear"`` (or a model built with ``predict_solver="linear"``) conditions on the train block in
O(N) instead: `_posterior_draw_linear`, ``train_block_terms(solve="chain")`` -- DESIGN 4.15.
"""
from __future__ import annotations

import os

import torch

from . import ops
from .safe import _chol_1x1, _safe_draw, _safe_factor, _safe_forms, default_jitter


def _posterior_draw(covar_module, full_x, full_vol, idx_cut, train_diffs, test_mean_term, z, jitter,
                    latent_mean=None, theta=0.5):
    """rollout_utils.py:26-53 on the device.  full_x [N+T] or [S,N+T]; full_vol [S,N+T] (or [N+T]);
    train_diffs [S,N,1] (or broadcastable); test_mean_term broadcastable to [S,T,1]; z [S,T,n].
    Returns samples + pred_mean, shape [S,T,n]."""
    cov_mat = covar_module(full_x.unsqueeze(-1), full_vol.unsqueeze(-1)).evaluate()        # :26  (HIP fill)
    if cov_mat.ndim == 2:
        cov_mat = cov_mat.unsqueeze(0)
    S = cov_mat.shape[0]
    T = cov_mat.shape[-1] - idx_cut
    K_tr = cov_mat[..., :idx_cut, :idx_cut]                                                # :27
    K_te_tr = cov_mat[..., idx_cut:, :idx_cut]                                             # :28, transposed: rows = test points
    K_te = cov_mat[..., idx_cut:, idx_cut:]                                                # :29
    f, _ = _safe_factor(K_tr, jitter)                                                      # :35  (HIP potrf)
    td = train_diffs.reshape(-1, idx_cut) if train_diffs.ndim > 1 else train_diffs.reshape(1, idx_cut)
    td = td.expand(S, idx_cut)
    sol = ops.cholesky_solve(f, td)                                                        # :36
    # every product below runs on the library's own MFMA GEMM (volt_gemm_nt_f32), not on a vendor BLAS
    dt = cov_mat.dtype
    pred_mean = ops.gemm_nt(K_te_tr, sol.unsqueeze(1)).to(dt)                              # [S,T,1] = K_te,tr sol
    pred_mean = pred_mean + test_mean_term                                                 # :39
    if latent_mean is not None:
        pred_mean = pred_mean - theta * (pred_mean - latent_mean)                          # :41-42
    if T == 1:
        sol2 = ops.cholesky_solve(f, K_te_tr[..., 0, :])                                   # :44
        pred_cov = K_te - (K_te_tr[..., 0, :] * sol2).sum(-1).reshape(S, 1, 1)
        pred_cov_L = _chol_1x1(pred_cov, jitter)                                           # :46
        return pred_cov_L * z + pred_mean                                                  # :48,:53 (1x1 "matmul")
    Linv = ops.trtri(f).mT.contiguous()                                                    # L^-1 (lower), rows K-contiguous
    G = ops.gemm_nt(K_te_tr, Linv, uplo_b=1)                                               # K_te,tr L^-T   [S,T,N]
    pred_cov = K_te - ops.gemm_nt(G, G).to(dt)
    fc, _ = _safe_factor(pred_cov, jitter)
    return ops.gemm_nt(fc.L, z.mT.contiguous(), uplo_a=1).to(dt) + pred_mean               # :48,:53


SOLVERS = ("dense", "linear")


def _resolve_solver(solver, model=None):
    """``solver=None`` reads the model's ``predict_solver`` ("dense" for a model without one)."""
    if solver is None:
        solver = getattr(model, "predict_solver", "dense")
    if solver not in SOLVERS:
        raise ValueError(f"solver must be one of {SOLVERS}, got {solver!r}")
    return solver


DRAWS = ("factor", "chain")


def _resolve_draw(draw, solver, model=None):
    """``draw=None`` reads the model's ``predict_draw`` ("factor" for a model without one).  "chain" (ops.vk_draw, DESIGN
    4.17) exists on the linear route only."""
    if draw is None:
        draw = getattr(model, "predict_draw", "factor")
    if draw not in DRAWS:
        raise ValueError(f"draw must be one of {DRAWS}, got {draw!r}")
    if draw == "chain" and solver != "linear":
        raise ValueError("draw='chain' needs solver='linear' (predict_solver='linear'): the dense route factors its own blocks")
    return draw


def _rows_shared(t):
    """Whether the rows of t [S,n] are one row (an expanded view, or equal values: one device read)."""
    return t.shape[0] == 1 or t.stride(0) == 0 or bool((t == t[:1]).all())


def _linear_draw(rho, tau, V_last, V_te, test_mean_term, z, jitter, latent_mean, theta, dt, draw="factor", test_vol=None):
    """The draw from the conditional whose train block enters through rho = u'A^-1 u and tau = u'A^-1 r (fp64, [G] each with
    G = S or 1) -- every appended point has the same cross-covariance u = V with the train block, so
        mean_t = tau + m(x_t),     cov_st = V_te[min(s,t)] - rho = (V_te[min(s,t)] - V_last) + (V_last - rho),
    the sum of the test increments plus what the jitter rung leaves of the last train entry, in fp64 (the two terms of the
    second bracket agree to rounding at rung 0).  V_te [S,T] fp64, z [S,T,n].  Returns samples + pred_mean [S,T,n] in ``dt``.
    ``draw="chain"``: the same draw from ONE ops.vk_draw launch in O(T) per path -- no [S,T,T] array, no
    factorisation; T = 1 is the chain's first step.  It forms W itself from ``test_vol`` = (vol_last [G], pred_vol [S,T], dx
    [G] or a number): the last train vol, the test vols and the uniform grid step; ``V_te`` is not read (pass None)."""
    f64 = torch.float64
    if draw == "chain":
        vol_last, pred_vol, dx = test_vol
        S, T = pred_vol.shape
        n = z.shape[-1]
        pred_mean = tau.reshape(-1, 1, 1) + test_mean_term.to(f64)
        if latent_mean is not None:
            pred_mean = pred_mean - theta * (pred_mean - torch.as_tensor(latent_mean, device=pred_vol.device).to(f64))
        vlr = (V_last - rho).reshape(-1)
        shared = pred_mean.shape[0] == 1 and all(not torch.is_tensor(t) or t.numel() == 1 for t in (vlr, vol_last, dx))
        G, Sg = (1, S) if shared else (S, 1)                                             # one series of S paths, or S series of one
        mean = pred_mean.expand(G, T, 1).reshape(G, T)
        zc = z.to(dt).mT.reshape(G, Sg * n, T)                                             # [S,n,T]: the n columns are `reps`
        pv = pred_vol.to(dt).reshape(G, Sg, T)
        jitter = default_jitter(False) if T == 1 and jitter is None else jitter           # `_chol_1x1`'s first rung, whatever the dtype
        out, _ = _safe_draw(lambda j: ops.vk_draw(pv, vol_last, vlr, dx, mean, zc, j, reps=n), (pv, vlr, mean, zc), jitter,
                            f64=dt == f64)
        return out.reshape(S, n, T).mT
    S, T = V_te.shape
    pred_mean = tau.reshape(-1, 1, 1) + test_mean_term.to(f64)                            # [S,T,1] (or broadcastable)
    if latent_mean is not None:
        pred_mean = pred_mean - theta * (pred_mean - torch.as_tensor(latent_mean, device=V_te.device).to(f64))
    W = (V_te - V_last.reshape(-1, 1)) + (V_last - rho).reshape(-1, 1)                  # [S,T]: the diagonal of the T x T block
    if T == 1:
        pred_cov_L = _chol_1x1(W.reshape(S, 1, 1), jitter)
        return (pred_cov_L * z.to(f64) + pred_mean).to(dt)
    idx = torch.arange(T, device=V_te.device)
    pred_cov = W[:, torch.minimum(idx[:, None], idx[None, :])]                           # [S,T,T]
    fc, _ = _safe_factor(pred_cov.to(dt), jitter)
    noise = ops.gemm_nt(fc.L.to(torch.float32), z.to(torch.float32).mT.contiguous(), uplo_a=1)
    return (noise.to(f64) + pred_mean).to(dt)


def _posterior_draw_linear(covar_module, full_x, full_vol, idx_cut, train_diffs, test_mean_term, z, jitter,
                           latent_mean=None, theta=0.5, draw="factor"):
    """`_posterior_draw` without any N x N or N x T array (solver="linear"): same arguments, same result to
    rounding.  The stacked integrated path V comes from ops.cumtrapz in fp64; its first N entries are the train block
    K = V[min(i,j)] (they do not depend on the test vols: CumTrapz's halved last weight sits on the last test point), and the
    train block enters only through the two scalars of safe._safe_forms (volt_vk_forms_*, one O(N) sweep per grid, the
    project's jitter ladder around it).  One grid serves all S samples when their train rows are shared; per-sample histories
    (the dense Rollouts engine after its first step) run as S grids in one launch.
    ``draw="chain"``: the integrated path is formed over the train part alone (the same products in the same order: its N
    entries are bit for bit those of the stacked path) and the test part inside ops.vk_draw -- `_linear_draw`."""
    from .kernels import VolatilityKernel
    if not isinstance(covar_module, VolatilityKernel):
        raise TypeError("solver='linear' conditions on the volatility kernel's min structure; "
                        f"got {type(covar_module).__name__} (use solver='dense')")
    f64 = torch.float64
    dt = torch.float64 if full_vol.dtype == torch.float64 else torch.float32
    N = idx_cut
    vol = full_vol.reshape(-1, full_vol.shape[-1])
    x = full_x.reshape(-1, full_x.shape[-1])
    S, T = vol.shape[0], vol.shape[-1] - N
    td = train_diffs.reshape(-1, N) if train_diffs.ndim > 1 else train_diffs.reshape(1, N)
    one_x = _rows_shared(x)
    G = 1 if one_x and _rows_shared(vol[:, :N]) and _rows_shared(td) else S              # grids: one for all samples, or one each
    first = default_jitter(dt == f64, jitter)                       # by what came in: the forms are fp64 whatever the input
    if draw == "chain":
        xg = (x[0] if one_x else x[:G]).to(f64)
        U = ops.cumtrapz(torch.cat((vol[:G, :N], vol[:G, N - 1:N]), -1).to(f64), xg[..., :N + 1], square=True)[:, :N]   # [G,N]
        out, _ = _safe_forms(U, td.to(f64).expand(S, N)[:G], first)
        return _linear_draw(out[:, 0], out[:, 1], U[:, N - 1], None, test_mean_term, z, jitter, latent_mean, theta, dt, "chain",
                            (vol[:G, N - 1], vol[:, N:], xg[..., 1] - xg[..., 0]))
    V = ops.cumtrapz(vol.to(f64), (x[0] if one_x else x).to(f64), square=True)             # [S,N+T]
    out, _ = _safe_forms(V[:G, :N], td.to(f64).expand(S, N)[:G], first)
    return _linear_draw(out[:, 0], out[:, 1], V[:, N - 1], V[:, N:], test_mean_term, z, jitter, latent_mean, theta, dt)


def GeneratePrediction(train_x, train_y, test_x, pred_vol, model, latent_mean=None, theta=0.5, *, z=None, solver=None,
                       draw=None):
    """voltron/rollout_utils.py:6-53.  Reads model.{log_vol_path, train_x, train_y, mean_module,
    covar_module}; returns [S, T] (T = test_x.shape[0]).  ``solver``: "dense" (the reference's route) or "linear"
    (`_posterior_draw_linear`, no N x N array); None reads ``model.predict_solver``.  ``draw`` (solver="linear" only):
    "factor" or "chain" (ops.vk_draw: no T x T array either); None reads ``model.predict_draw``."""
    solver = _resolve_solver(solver, model)
    how = _resolve_draw(draw, solver, model)
    draw = _posterior_draw_linear if solver == "linear" else _posterior_draw
    kw = {"draw": how} if solver == "linear" else {}
    vol = model.log_vol_path.exp()
    if model.train_x.ndim != test_x.ndim:
        test_x_for_stack = test_x.unsqueeze(0).repeat(model.train_x.shape[0], 1)
    else:
        test_x_for_stack = test_x
    if vol.ndim == 1:
        vol_for_stack = vol.unsqueeze(0).repeat(pred_vol.shape[0], 1)
    else:
        vol_for_stack = vol
    full_x = torch.cat((model.train_x, test_x_for_stack), dim=-1)
    full_vol = torch.cat((vol_for_stack, pred_vol), dim=-1)
    idx_cut = model.train_x.shape[-1]

    train_mean = model.mean_module(model.train_x)
    train_diffs = model.train_y.unsqueeze(-1) - train_mean.unsqueeze(-1)
    test_mean_term = model.mean_module(test_x).detach().T.unsqueeze(-1)                    # :39
    S, T = full_vol.shape[0], test_x.shape[0]
    if z is None:
        z = torch.randn(S, T, 1).to(test_x.device)                                         # :47
    out = draw(model.covar_module, full_x, full_vol, idx_cut, train_diffs, test_mean_term,
               z.reshape(S, T, 1), 1e-4, latent_mean, theta, **kw)
    return out.squeeze(-1)


def _model_generate_prediction(model, test_x, pred_vol, n_sample=1):
    """The model-method twins, VoltronGP.py:62-95 / VoltMagpie.py:67-99 (default jitter, n_sample
    draws per test point, mean from model.train_inputs).  A model built with ``predict_solver="linear"`` conditions through
    `_posterior_draw_linear`."""
    if model.train_x.ndim != test_x.ndim:
        test_x_for_stack = test_x.unsqueeze(0).repeat(model.train_x.shape[0], 1)
    else:
        test_x_for_stack = test_x
    full_x = torch.cat((model.train_x, test_x_for_stack), dim=-1)
    full_vol = torch.cat((model.log_vol_path.exp(), pred_vol), dim=-1)
    idx_cut = model.train_x.shape[-1]
    train_mean = model.mean_module(*model.train_inputs).detach()
    train_diffs = model.train_y.unsqueeze(-1) - train_mean.reshape(model.train_y.shape).unsqueeze(-1)
    test_mean_term = model.mean_module(test_x).detach().unsqueeze(-1)
    batch = full_vol.shape[:-1]
    T = test_x.shape[0]
    z = torch.randn(*batch, T, n_sample).to(test_x.device)
    S = 1 if len(batch) == 0 else batch[0]
    solver = _resolve_solver(None, model)
    draw = _posterior_draw_linear if solver == "linear" else _posterior_draw
    kw = {"draw": _resolve_draw(None, solver, model)} if solver == "linear" else {}
    out = draw(model.covar_module, full_x, full_vol, idx_cut, train_diffs, test_mean_term, z.reshape(S, T, n_sample), None, **kw)
    out = out.reshape(*batch, T, n_sample)
    return out.squeeze(-1)                                  # (samples + pred_mean).squeeze(-1), VoltMagpie.py:96-99: [T] for n_sample = 1


def rollout_engine_max_h():
    from .rollout_engine import MAX_H
    return MAX_H


def Rollouts(train_x, train_y, test_x, model, nsample=50, method="volt", theta=None, *, pred_vol=None, z=None,
             engine=None, solver=None, draw=None):
    """voltron/rollout_utils.py:57-93.  train_x [N], train_y [N+1] raw prices, test_x [H] ->
    samples [nsample, H] on the CPU (log-price units).  Mutates ``model`` like the reference.
    ``solver``: "dense" or "linear" (None: ``model.predict_solver``) -- with "linear" the bordered engine conditions on the
    train block through the O(N) chain (train_block_terms(solve="chain")) and the dense engine draws every step with
    `_posterior_draw_linear`; no N x N array either way.  ``draw`` (solver="linear" only; None: ``model.predict_draw``):
    "chain" draws every step of the dense engine through ops.vk_draw; the bordered engine has one recursion of
    its own and is not changed by it."""
    if method != "volt":
        return nonvol_rollouts(train_x, train_y, test_x, model, nsample=nsample)
    solver = _resolve_solver(solver, model)
    draw = _resolve_draw(draw, solver, model)
    engine = engine or os.environ.get("VOLT_ROLLOUT_ENGINE", "bordered")
    if theta is None:
        latent_mean = None
    else:
        latent_mean = train_y.log().mean()
    ntest = test_x.numel()
    if pred_vol is None:
        pred_vol = model.vol_model(test_x).sample(torch.Size((nsample,))).exp()           # :66
    pred_vol = pred_vol.to(train_x.device)
    if z is not None:
        z = z.to(train_x.device)
    if engine == "bordered" and ntest > rollout_engine_max_h():
        engine = "dense"                         # the bordered kernel holds <= 1024 appended points per sample
    if engine == "bordered":
        from .rollout_engine import rollouts_bordered
        out = rollouts_bordered(train_x, train_y, test_x, model, pred_vol, z, latent_mean, theta,
                                solve="chain" if solver == "linear" else "factor")
        if out is not None:
            return out
        engine = "dense"                         # a mean module the bordered kernel has no mode for: the general route
    if engine != "dense":
        raise ValueError(f"unknown rollout engine {engine!r}")

    samples = torch.zeros(nsample, ntest)                                                  # on the CPU, :65
    th = 0.5 if theta is None else theta
    samples[:, 0] = GeneratePrediction(train_x, train_y, test_x[0].unsqueeze(0), pred_vol[:, 0].unsqueeze(1),
                                       model, latent_mean, th, z=None if z is None else z[:, 0:1],
                                       solver=solver, draw=draw).squeeze().cpu()
    train_stack_y = train_y[1:].log().repeat(nsample, 1)
    train_stack_vol = model.log_vol_path.repeat(nsample, 1)

    for idx in range(1, ntest):
        stack_y = torch.cat((train_stack_y, samples[:, :idx].to(train_stack_y.device)), -1)
        stack_vol = torch.cat((train_stack_vol, pred_vol[:, :idx].to(train_stack_vol.device).log()), -1)
        rolling_x = torch.cat((train_x, test_x[:idx]))
        model.mean_module.train_y = stack_y
        model.mean_module.train_x = rolling_x
        model.train_x = rolling_x
        model.train_y = stack_y
        model.log_vol_path = stack_vol
        samples[:, idx] = GeneratePrediction(train_x, train_y, test_x[idx].unsqueeze(0),
                                             pred_vol[:, idx].unsqueeze(-1), model, latent_mean, th,
                                             z=None if z is None else z[:, idx:idx + 1], solver=solver,
                                             draw=draw).squeeze().cpu()
    return samples


def nonvol_rollouts(train_x, train_y, test_x, model, nsample=50, *, z=None):
    """voltron/rollout_utils.py:95-115 -- SURVEY 8(f) row 2: sequential rollouts of a baseline GP (generic kernel,
    usually a moving-average mean).  The reference conditions ``nsample`` stacked series on one more point per step
    through botorch's ``model.posterior``; here one shared factorisation + one GEMM + the mean recursion
    (rollout_engine.rollouts_shared) produce the same draws.  The model is left in the state the reference leaves it
    in (:106-111); samples come back on the CPU, log-price units.  ``z`` [nsample, H] optionally fixes the N(0,1) draws."""
    from . import rollout_engine
    ntest = test_x.numel()
    samples = rollout_engine.rollouts_shared(train_x, train_y, test_x, model, nsample, z=z)
    if ntest > 1:
        stack_y = torch.cat((train_y.log().repeat(nsample, 1), samples[:, :ntest - 1]), -1)
        rolling_x = torch.cat((train_x, test_x[:ntest - 1]))
        model.mean_module.train_y = stack_y
        model.mean_module.train_x = rolling_x
        model.train_inputs = (rolling_x.view(-1, 1),)
        model.train_targets = stack_y
        model.train()
    return samples.cpu()
