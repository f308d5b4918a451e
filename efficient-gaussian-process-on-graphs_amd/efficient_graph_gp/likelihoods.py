"""Likelihoods for ``efficient_graph_gp.models.SVGP``: mirrors of ``gpflow.likelihoods.MultiClass`` with the
``RobustMax`` inverse link (what the reference's Cora notebooks build: ``gpflow.likelihoods.MultiClass(num_classes=7)``)
and of ``gpflow.likelihoods.Gaussian``.

MultiClass's expectations are a 20-point Gauss-Hermite quadrature of a product of normal CDFs per data point
(GPflow's likelihoods/multiclass.py: ``RobustMax.prob_is_largest``, ``MultiClass._variational_expectations``,
``_predict_non_logged_density``, ``_predict_mean_and_var``); they and their gradient run in one launch of the engine
(``grf_robustmax_ve_f64``, include/grf_svgp.h).  The Gaussian's have a closed form, written in torch:
``-1/2 log 2 pi s2 - 1/2 ((y - mu)^2 + v) / s2``.
"""
from typing import Optional

import numpy as np
import torch

VARIANCE_LOWER_BOUND = 1e-6  # gpflow.likelihoods.Gaussian's DEFAULT_VARIANCE_LOWER_BOUND
_LOG_2PI = float(np.log(2.0 * np.pi))


class RobustMax:
    """GPflow's RobustMax inverse link: the largest latent wins with probability 1 - epsilon.  ``epsilon`` is a
    constant (GPflow's is ``trainable=False``)."""

    def __init__(self, num_classes: int, epsilon: float = 1e-3):
        if int(num_classes) < 2:
            raise ValueError("RobustMax: num_classes must be at least 2")
        if not 0.0 < float(epsilon) < 1.0:
            raise ValueError("RobustMax: epsilon must lie in (0, 1)")
        self.num_classes = int(num_classes)
        self.epsilon = float(epsilon)

    @property
    def eps_k1(self) -> float:
        return self.epsilon / (self.num_classes - 1.0)


class MultiClass(torch.nn.Module):
    """``gpflow.likelihoods.MultiClass(num_classes, invlink=RobustMax(num_classes))``, 20 quadrature points."""
    num_gauss_hermite_points = 20

    def __init__(self, num_classes: int, invlink: Optional[RobustMax] = None):
        super().__init__()
        if invlink is None:
            invlink = RobustMax(num_classes)
        if not isinstance(invlink, RobustMax):
            raise NotImplementedError("MultiClass: only the RobustMax inverse link is supported")
        if invlink.num_classes != int(num_classes):
            raise ValueError("MultiClass: the inverse link's num_classes differs")
        self.num_classes = int(num_classes)
        self.invlink = invlink
        self.latent_dim = self.num_classes

    def parameter(self):
        return None

    def targets(self, Y, n: int, device) -> torch.Tensor:
        """The labels as a device int32 vector, validated on the host: integers in [0, num_classes)."""
        Yh = Y.detach().cpu().numpy() if torch.is_tensor(Y) else np.asarray(Y)
        Yh = Yh.reshape(-1)
        if Yh.size != n:
            raise ValueError(f"MultiClass: {n} labels expected, one per node")
        Yi = Yh.astype(np.int64)
        if not np.all(Yi == Yh) or (Yi.size and (Yi.min() < 0 or Yi.max() >= self.num_classes)):
            raise ValueError(f"MultiClass: labels must be integers in [0, {self.num_classes})")
        return torch.from_numpy(Yi.astype(np.int32)).to(device)

    def variational_expectations(self, eng, fmean, fvar, Y, par=None, with_grad=True):
        ve, gmu, gvar = eng.robustmax_ve(fmean, fvar, Y, with_grad=with_grad, epsilon=self.invlink.epsilon)
        return ve, gmu, gvar, None

    def predict_mean_and_var(self, eng, fmean, fvar):
        ps = eng.robustmax_predict(fmean, fvar, epsilon=self.invlink.epsilon)
        return ps, ps - ps * ps

    def predict_log_density(self, eng, fmean, fvar, Y):
        ps = eng.robustmax_predict(fmean, fvar, epsilon=self.invlink.epsilon)
        return torch.log(ps.gather(1, Y.long()[:, None])[:, 0])


class Gaussian(torch.nn.Module):
    """``gpflow.likelihoods.Gaussian(variance)``: the variance is a softplus parameter with the 1e-6 lower bound."""

    def __init__(self, variance: float = 1.0, *, device=None):
        super().__init__()
        v = float(variance) - VARIANCE_LOWER_BOUND
        if not v > 0.0:
            raise ValueError(f"Gaussian: variance must exceed the lower bound {VARIANCE_LOWER_BOUND}")
        raw = v + np.log(-np.expm1(-v))  # softplus^-1
        self.raw_variance = torch.nn.Parameter(torch.tensor(raw, dtype=torch.float64, device=device))
        self.latent_dim = None

    @property
    def variance(self) -> torch.Tensor:
        return torch.nn.functional.softplus(self.raw_variance) + VARIANCE_LOWER_BOUND

    def parameter(self):
        return self.variance

    def targets(self, Y, n: int, device) -> torch.Tensor:
        Yt = Y.detach() if torch.is_tensor(Y) else torch.as_tensor(np.asarray(Y, dtype=np.float64))
        if Yt.dim() == 1:
            Yt = Yt[:, None]
        if Yt.dim() != 2 or Yt.shape[0] != n:
            raise ValueError(f"Gaussian: Y must be ({n} x P), one row per node")
        return Yt.to(device, torch.float64).contiguous()

    def variational_expectations(self, eng, fmean, fvar, Y, par, with_grad=True):
        """(ve (n,), d/dmu, d/dvar, d sum(ve)/d variance), summed over the P columns."""
        s2 = par.reshape(())
        r = Y - fmean
        q = r * r + fvar
        ve = (-0.5 * (_LOG_2PI + torch.log(s2)) - 0.5 * q / s2).sum(dim=1)
        if not with_grad:
            return ve, None, None, None
        gpar = (-0.5 / s2 + 0.5 * q / (s2 * s2)).sum()
        return ve, r / s2, torch.full_like(fvar, -0.5) / s2, gpar

    def predict_mean_and_var(self, eng, fmean, fvar):
        return fmean, fvar + self.variance.detach()

    def predict_log_density(self, eng, fmean, fvar, Y):
        v = fvar + self.variance.detach()
        return (-0.5 * (_LOG_2PI + torch.log(v) + (Y - fmean) ** 2 / v)).sum(dim=1)
