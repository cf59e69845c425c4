"""IndexKernel and MultitaskKernel -- the task half of the reference's MultitaskBMGP (voltron/models/BMGP.py:35:
``MultitaskKernel(BMKernel(), num_tasks=T)``).  gpytorch's classes, restated from their published behaviour (gpytorch is
not installed here, so none of this is pinned by executing it):

* IndexKernel(num_tasks, rank=1) registers ``covar_factor`` = randn(T, rank) and then ``raw_var`` = randn(T) (two draws
  from torch's default generator, in that order), ``var = softplus(raw_var)`` (Positive constraint) and
  ``covar_matrix = covar_factor covar_factor' + diag(var)``.  ``var`` is computed, so the reference's
  ``task_covar_module.var.data /= 10.`` (BMGP.py:39) divides a temporary and changes nothing.
* MultitaskKernel(data_covar_module, num_tasks, rank=1) registers ``task_covar_module`` (an IndexKernel) and then
  ``data_covar_module``; ``K(x1, x2) = data(x1, x2) (x) K_t`` with element (n, t) at n*T + t.

Elementwise and tiny, kept in torch; the MLL over this kernel runs on the Kronecker step (gp._KronMLL)."""
import torch
import torch.nn.functional as F
from torch import nn

from ..gp import Kernel, _dense, _Evaluated


class IndexKernel(Kernel):
    def __init__(self, num_tasks, rank=1, batch_shape=torch.Size(), prior=None, var_constraint=None, **kwargs):
        super().__init__(**kwargs)
        if prior is not None or var_constraint is not None:
            raise NotImplementedError("IndexKernel: priors and custom constraints are not provided (the reference uses neither)")
        self.num_tasks, self.rank, self.batch_shape = num_tasks, rank, batch_shape
        self.register_parameter("covar_factor", nn.Parameter(torch.randn(*batch_shape, num_tasks, rank)))
        self.register_parameter("raw_var", nn.Parameter(torch.randn(*batch_shape, num_tasks)))

    @property
    def var(self):
        return F.softplus(self.raw_var)

    @var.setter
    def var(self, value):
        value = torch.as_tensor(value, dtype=self.raw_var.dtype, device=self.raw_var.device).expand_as(self.raw_var)
        with torch.no_grad():
            self.raw_var.copy_(value + torch.log(-torch.expm1(-value)))

    @property
    def covar_matrix(self):
        f = self.covar_factor
        return _Evaluated(f @ f.transpose(-1, -2) + torch.diag_embed(self.var))

    def forward(self, i1, i2=None, **kwargs):
        """K_t at integer task indices i1 [n1] (or [n1,1]), i2 [n2]."""
        i2 = i1 if i2 is None else i2
        Kt = self.covar_matrix.evaluate()
        return Kt[i1.reshape(-1).long()][:, i2.reshape(-1).long()]


class MultitaskKernel(Kernel):
    def __init__(self, data_covar_module, num_tasks, rank=1, task_covar_prior=None, **kwargs):
        super().__init__(**kwargs)
        self.task_covar_module = IndexKernel(num_tasks=num_tasks, rank=rank, prior=task_covar_prior)
        self.data_covar_module = data_covar_module
        self.num_tasks = num_tasks

    def forward(self, x1, x2=None, **kwargs):
        """Dense data(x1, x2) (x) K_t, [n1 T, n2 T] (interleaved order)."""
        x2 = x1 if x2 is None else x2
        Kx = _dense(self.data_covar_module(x1, x2))
        Kt = self.task_covar_module.covar_matrix.evaluate()
        dt = torch.promote_types(Kx.dtype, Kt.dtype)
        return torch.kron(Kx.to(dt), Kt.to(dt))
