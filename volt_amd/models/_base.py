"""What VoltronGP, VoltMagpie and Volt share (voltron/models/{VoltronGP,VoltMagpie,Volt}.py): an exact GP whose
covariance is the volatility kernel of a stored vol path, filled ONCE on the device (``train_cov``) and reused by every
training step (``data_solver="linear"``: kept as its integrated vol path V, gp._VolPrior, and never filled), plus a Brownian-motion GP over the log-vol path that forecasts it.  Attribute names are the reference's
(rollout_utils.py:7-32,81-86 and train_utils.py:222-224 read and write them); the subclasses only choose the mean."""
import torch

from .. import ops
from ..gp import (ExactGP, ExactMarginalLogLikelihood, GaussianLikelihood, MultitaskGaussianLikelihood, MultivariateNormal,
                  _VolPrior, same_values)
from ..kernels import VolatilityKernel
from ._posterior import check_options
from .BMGP import BMGP, MultitaskBMGP


class VolGP(ExactGP):
    def _init_vol_state(self, x, y, vol_path, multitask_vol=False, vol_solver="dense", data_solver="dense",
                        predict_solver="dense", vol_posterior="solve", predict_draw="factor"):
        """x [N], y [N] or [T,N] (batched layout: one shared input grid, T target / vol rows), vol_path like y or None.
        Call after ``mean_module`` is set so that the modules register in the reference's order.  ``multitask_vol`` (batched
        models only): the reference's own vol forecaster, a MultitaskBMGP over the [N,T] log-vol paths with a
        MultitaskGaussianLikelihood(T) at noise 1e-3 (VoltMagpie.py:51-55) -- the T forecasts are then jointly drawn and
        correlated; without it T independent BM-GPs (the batched BMGP).  ``data_solver="linear"``: ``train_cov`` is the lazy
        _VolPrior over V = CumTrapz(vol^2, x) instead of the N x N fill, and the MLL of the training inputs runs on the linear-time
        step (gp._ChainMLL, csrc/bm.hip); the default "dense" is the filled matrix and the dense step.
        ``predict_solver="linear"``: GeneratePrediction / SamplePrediction / MeanPrediction, rollout_utils.GeneratePrediction
        and Rollouts condition on the train block through the O(N) chain (volt_vk_forms_*) instead of filling
        and factoring it; independent of ``data_solver`` (a dense-trained model may predict linearly), and "dense" changes
        nothing.  ``vol_posterior`` (with ``vol_solver="linear"``): the vol forecaster's ``posterior``, "solve", "sweep" or "chain"
        (BMGP / MultitaskBMGP).  ``predict_draw`` (with ``predict_solver="linear"``): "factor" (default) fills
        and factors the T x T predictive block of a joint draw, "chain" draws it in O(T) per path (ops.vk_draw)."""
        if predict_solver not in BMGP.SOLVERS:
            raise ValueError(f"predict_solver must be one of {BMGP.SOLVERS}, got {predict_solver!r}")
        self.predict_solver = predict_solver
        from ..rollout_utils import _resolve_draw
        self.predict_draw = _resolve_draw(predict_draw, predict_solver)
        if data_solver not in BMGP.SOLVERS:
            raise ValueError(f"data_solver must be one of {BMGP.SOLVERS}, got {data_solver!r}")
        self.data_solver = data_solver        # Volt.Train fits the data model with the solver the model was built with
        dev = x.device
        batch_shape = y.shape[:-1]
        self.covar_module = VolatilityKernel().to(dev)
        self.train_x = x.unsqueeze(0).repeat(*batch_shape, 1) if len(batch_shape) else x
        self.train_y = y
        self.log_vol_path = vol_path.log() if vol_path is not None else -torch.ones(x.shape[0], device=dev)
        if data_solver == "linear":
            self.train_cov = self._vol_prior(self.train_x.squeeze(), self.log_vol_path.exp().squeeze())   # (the kernel's squeeze()s)
        else:
            self.train_cov = self.covar_module(self.train_x.unsqueeze(-1), self.log_vol_path.exp().unsqueeze(-1)).detach()
        # vol forecaster: one BM-GP per series by default.  (The reference's batched models use botorch's Kronecker multitask
        # GP there: MultitaskBMGP, opt-in with multitask_vol=True; the default batched BMGP -- T independent vol models over
        # the shared grid -- leaves out the cross-series correlation.)  ``vol_solver="linear"``: that BM-GP on the linear-time
        # solver (BMGP(solver="linear"), csrc/bm.hip), and MultitaskBMGP on the linear-time Kronecker step (csrc/kron_chain.hip).
        if vol_solver not in BMGP.SOLVERS:
            raise ValueError(f"vol_solver must be one of {BMGP.SOLVERS}, got {vol_solver!r}")
        check_options("vol_posterior", vol_solver, vol_posterior)
        self.vol_solver = vol_solver          # Volt.Train refits the vol forecaster: with the solver the model was built with
        self.vol_posterior = vol_posterior    # ... and with the same posterior
        if multitask_vol:
            if not len(batch_shape) or self.log_vol_path.shape[:-1] != batch_shape:
                raise ValueError("multitask_vol=True needs a batched model with a [T,N] vol_path")
            self.vol_lh = MultitaskGaussianLikelihood(num_tasks=batch_shape[0]).to(dev)
            self.vol_lh.noise = 1e-3
            self.vol_model = MultitaskBMGP(x, self.log_vol_path.t(), self.vol_lh, solver=vol_solver, posterior=vol_posterior)   # [N] inputs, [N,T] targets
            return
        self.vol_lh = GaussianLikelihood(batch_shape=batch_shape).to(dev)
        self.vol_model = (BMGP(x, self.log_vol_path, self.vol_lh, solver=vol_solver, posterior=vol_posterior)
                          if self.log_vol_path.shape[:-1] == batch_shape else None)

    @staticmethod
    def _vol_prior(x, vol):
        """The linear data solver's covariance: V = CumTrapz(vol^2, x) as VolatilityKernel.forward forms it, not filled."""
        return _VolPrior(ops.cumtrapz(vol, x, square=True).detach())

    def UpdateVolPath(self, vol_path):
        self.log_vol_path = vol_path.log()
        if self.data_solver == "linear":
            self.train_cov = self._vol_prior(self.train_inputs[0].squeeze(-1) if self.train_x.ndim == 1 else self.train_x,
                                             self.log_vol_path.exp())
            return
        self.train_cov = self.covar_module(self.train_inputs[0].squeeze(-1) if self.train_x.ndim == 1 else self.train_x,
                                           self.log_vol_path.exp())

    def VolMLL(self):
        vol_mll = ExactMarginalLogLikelihood(self.vol_lh, self.vol_model)
        if isinstance(self.vol_model, MultitaskBMGP):
            # the reference passes the [T,N] inputs and targets (VoltMagpie.py:62-65) to a model built on [N] / [N,T]; the
            # layouts the model was built with are passed here
            return vol_mll(self.vol_model(self.vol_model.train_inputs[0]), self.log_vol_path.t())
        return vol_mll(self.vol_model(self.train_x), self.log_vol_path)

    def GeneratePrediction(self, test_x, pred_vol, n_sample=1):
        from ..rollout_utils import _model_generate_prediction
        return _model_generate_prediction(self, test_x, pred_vol, n_sample)

    def _predict_with(self, pred_vol, test_x, n_sample, return_vol):
        prediction = self.GeneratePrediction(test_x, pred_vol, n_sample)
        return (prediction, pred_vol) if return_vol else prediction

    def _vol_layout(self, v):
        # a MultitaskBMGP forecasts [H,T]: the reference transposes to [T,H] (VoltMagpie.py:103,113)
        return v.transpose(-1, -2) if isinstance(self.vol_model, MultitaskBMGP) else v

    def SamplePrediction(self, test_x, n_sample=1, return_vol=False):
        self.vol_model.eval()
        return self._predict_with(self._vol_layout(self.vol_model(test_x).sample().exp()), test_x, n_sample, return_vol)

    def MeanPrediction(self, test_x, n_sample=1, return_vol=False):
        self.vol_model.eval()
        return self._predict_with(self._vol_layout(self.vol_model(test_x).mean.exp()), test_x, n_sample, return_vol)

    def forward(self, x):
        mean_x = self.mean_module(x)
        if same_values(x, self.train_inputs[0]):          # torch.equal without the device sync when aliased
            covar_x = self.train_cov                      # the cached fill (data_solver="linear": the lazy _VolPrior)
        else:
            covar_x = self.covar_module(x, self.log_vol_path.exp())
        return MultivariateNormal(mean_x, covar_x)
