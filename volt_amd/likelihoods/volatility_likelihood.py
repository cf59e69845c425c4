"""Volatility likelihood of the GPCV stage, voltron/likelihoods/volatility_likelihood.py:8-58 -- SURVEY 8(f) row 4.

``y | f ~ N(0, scale(f))`` with ``scale = clamp(exp f, 1e-3)`` ("exp", what LearnGPCV uses, train_utils.py:20) or the
copula-process warp ``sum_k a_k log(1 + exp(b_k f + c_k))`` ("cv").  ``forward`` is elementwise and stays in torch; the
expectation under q(f) that the ELBO needs (75-node Gauss-Hermite, train_utils.py:50) runs in the HIP step for both:
volt_gpcv_step_f32 for "exp", volt_gpcv_cv_step_f32 for "cv" (K <= 8 terms; it also returns the gradients for a, b, c,
and VariationalELBO applies the constraints' chain rule).  "cv" is accelerated for SingleTaskVariationalGP latents,
unbatched and batched, and for the multi-task model with one warp per task (``batch_shape=[num_tasks]``:
volt_gpcv_mt_cv_step_f32); one unbatched warp shared by all tasks is not offered there.

``batch_shape=[T]`` stores [T,K] parameters, one set per series.  The reference's ``forward`` multiplies them against
samples [...,X,1] as they are, which lines T up with the samples' LAST axis: that is the multi-task layout [...,N,T]
(multi_task_variational_gp.py:62), and fails for batched single-task samples [...,T,N] unless N = T.  Here ``forward`` on a
plain tensor broadcasts them as [T,1,K] against samples [...,T,N], so series t of the samples meets parameter set t;
``marginal`` and ``expected_log_prob`` on a ``MultitaskVariationalLatent`` (event [N,T]) line parameter set t up with
column t and answer in the latent's own [...,N,T] layout."""
import torch
import torch.nn.functional as F
from torch import nn
from torch.distributions import Normal

from ..gp import Module, MultivariateNormal

NUM_LIKELIHOOD_SAMPLES = 10       # gpytorch.settings.num_likelihood_samples default, used by Likelihood.marginal


class VolatilityGaussianLikelihood(Module):
    MIN_SCALE = 1e-3              # volatility_likelihood.py:50

    def __init__(self, K=5, batch_shape=torch.Size(), param="cv", *args, **kwargs):
        super().__init__()
        if param == "cv":
            self.raw_a = nn.Parameter(torch.rand(*batch_shape, K))
            self.raw_b = nn.Parameter(0.1 * torch.rand(*batch_shape, K))
            self.raw_c = nn.Parameter(torch.rand(*batch_shape, K))
        self.param = param

    # constraints of volatility_likelihood.py:24-26: Positive (softplus), Interval(0,3), Interval(-3,3) (sigmoid)
    @property
    def trans_a(self):
        return F.softplus(self.raw_a)

    @property
    def trans_b(self):
        return 3.0 * torch.sigmoid(self.raw_b)

    @property
    def trans_c(self):
        return 6.0 * torch.sigmoid(self.raw_c) - 3.0

    def forward(self, function_samples, *args, **kwargs):
        if self.param == "cv":
            a, b, c = self.trans_a, self.trans_b, self.trans_c
            if a.ndim > 1:                                        # [T,K] -> [T,1,K]: one parameter set per series
                a, b, c = a.unsqueeze(-2), b.unsqueeze(-2), c.unsqueeze(-2)
            transform = ((b * function_samples.unsqueeze(-1) + c).exp() + 1).log() * a
            summed_transform = transform.sum(-1)
        else:
            summed_transform = function_samples.exp()
        return Normal(torch.zeros_like(summed_transform), summed_transform.clamp(min=self.MIN_SCALE))

    def _per_task(self, input):
        """Is ``input`` the multi-task latent (event [N,T]) under [T,K] parameters?  Then column t takes parameter set t."""
        from ..variational import MultitaskVariationalLatent
        return self.param == "cv" and self.raw_a.ndim > 1 and isinstance(input, MultitaskVariationalLatent)

    def _forward_columns(self, function_samples, *args, **kwargs):
        """``forward`` for samples [...,N,T] with parameter set t on column t; the result keeps that layout."""
        d = self.forward(function_samples.transpose(-1, -2), *args, **kwargs)
        return Normal(d.loc.transpose(-1, -2), d.scale.transpose(-1, -2))

    def expected_log_prob(self, target, input, *params, **kwargs):
        """volatility_likelihood.py:52-57 (gpytorch ``_OneDimensionalLikelihood.expected_log_prob``): E_{q(f_i)} log p(y_i|f_i)
        per point by Gauss-Hermite quadrature with ``num_gauss_hermite_locs`` nodes.  O(N Q) elementwise, kept in
        torch for direct callers; LearnGPCV's loop gets the same numbers (and their gradients) from the fused HIP step."""
        import math
        from ..variational import _gauss_hermite, num_gauss_hermite_locs
        mean, var = input.mean, input.variance
        gx, gw = _gauss_hermite(num_gauss_hermite_locs.value(), target.device, mean.dtype)      # nodes in q(f)'s precision
        locs = torch.sqrt(2.0 * var).unsqueeze(-1) * gx + mean.unsqueeze(-1)
        fwd = self._forward_columns if self._per_task(input) else self.forward
        logp = fwd(locs.movedim(-1, 0)).log_prob(target)                        # [Q, ..., N]  ([Q, N, T] for the multi-task latent)
        res = (logp * gw.reshape(-1, *([1] * (logp.ndim - 1)))).sum(0)
        return res

    def marginal(self, function_dist, *args, **kwargs):
        """gpytorch Likelihood.marginal: push ``num_likelihood_samples`` joint draws of f through ``forward``."""
        samples = function_dist.rsample(torch.Size([NUM_LIKELIHOOD_SAMPLES]))
        if self._per_task(function_dist):
            return self._forward_columns(samples, *args, **kwargs)
        return self.forward(samples, *args, **kwargs)

    def __call__(self, input, *args, **kwargs):
        if isinstance(input, MultivariateNormal):
            return self.marginal(input, *args, **kwargs)
        return self.forward(input, *args, **kwargs)
