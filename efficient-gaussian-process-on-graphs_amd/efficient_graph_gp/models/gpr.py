"""Dense exact GP regression: mirror of ``gpflow.models.GPR`` as the reference uses it
(experiments/sparse/scaling_exp/run_scaling_experiment.py:687-730, ``DenseGPModel``: ``GPR(data=(X, Y), kernel=...,
noise_variance=...)``, ``-log_marginal_likelihood()`` minimised, ``predict_f`` reported; the Cora, traffic and
mesh-ablation notebooks do the same).

Everything runs on the engine's fp64 Cholesky (``grf_potrf_f64``) and triangular solves (``grf_trsm_f64``), with no
host read of device data: ``log_marginal_likelihood`` is ``grf_amd.features.gpr_log_marginal_likelihood`` on
``kernel.K_torch(X, X)`` (so the kernel's own backward carries the gradient to its parameters), the predictions are

    A = L^-1 K[X, X*]   (one solve, the test nodes as right-hand-side rows),
    mean = A^T L^-1 Y,   var = K_diag[X*] - sum A^2,   cov = K[X*, X*] - A^T A   (the symmetric product).

The class is a ``torch.nn.Module``: its parameters are the kernel's plus the likelihood variance, stored through a
softplus with GPflow's 1e-6 lower bound.  Node sets are integer node ids (any shape, flattened: GPflow's (n, 1)
float arrays of ids are accepted); values come back as fp64 tensors on the device.  The predictions are not
differentiable.
"""
from typing import Optional, Tuple

import numpy as np
import torch

from grf_amd.engine import get_engine
from grf_amd.features import _LOG_2PI, gpr_factor, gpr_log_marginal_likelihood

VARIANCE_LOWER_BOUND = 1e-6  # gpflow.likelihoods.Gaussian's DEFAULT_VARIANCE_LOWER_BOUND


def _nodes(X) -> torch.Tensor:
    if torch.is_tensor(X):
        return X.detach().reshape(-1).long()
    return torch.from_numpy(np.asarray(X).reshape(-1).astype(np.int64))


class GPR(torch.nn.Module):
    def __init__(self, data: Tuple, kernel, noise_variance: float = 1.0, mean_function=None, *, device=None):
        super().__init__()
        if mean_function is not None:
            raise NotImplementedError("GPR: only the zero mean function (mean_function=None) is supported")
        if not hasattr(kernel, "K_torch"):
            raise TypeError("GPR: the kernel must expose K_torch(X1, X2)")
        X, Y = data
        self.engine = get_engine(device)
        self.kernel = kernel
        self.X = _nodes(X).to(self.engine.device)
        Yt = Y.detach() if torch.is_tensor(Y) else torch.as_tensor(np.asarray(Y, dtype=np.float64))
        if Yt.dim() == 1:
            Yt = Yt[:, None]
        if Yt.dim() != 2 or Yt.shape[0] != self.X.numel() or Yt.shape[0] < 1 or Yt.shape[1] < 1:
            raise ValueError("GPR: data = (X, Y) needs Y of shape (n, p) with one row per node of X")
        self.Y = Yt.to(self.engine.device, torch.float64).contiguous()
        v = float(noise_variance) - VARIANCE_LOWER_BOUND
        if not v > 0.0:
            raise ValueError(f"GPR: noise_variance must exceed the lower bound {VARIANCE_LOWER_BOUND}")
        raw = v + np.log(-np.expm1(-v))  # softplus^-1
        self.raw_likelihood_variance = torch.nn.Parameter(
            torch.tensor(raw, dtype=torch.float64, device=self.engine.device))
        self._factor_key = None
        self._factor = None
        self._info = None

    # ------------------------------------------------------------ parameters and the cached factor
    @property
    def likelihood_variance(self) -> torch.Tensor:
        """sigma^2 = softplus(raw) + 1e-6, a differentiable fp64 scalar on the device."""
        return torch.nn.functional.softplus(self.raw_likelihood_variance) + VARIANCE_LOWER_BOUND

    @property
    def cholesky_info(self) -> Optional[torch.Tensor]:
        """The device int32 of the last factorisation (0: positive definite), None before the first."""
        return self._info

    def check(self) -> None:
        """Reads ``cholesky_info`` (one host read) and raises as GPflow's Cholesky does when it is not 0."""
        if self._info is not None:
            info = int(self._info.item())
            if info != 0:
                raise ValueError("Cholesky decomposition was not successful: the leading minor of order "
                                 f"{info} of K + sigma^2 I is not positive definite")

    def invalidate(self) -> None:
        """Drop the cached factor (and the kernel's cached K): needed only after a parameter write that bypasses
        the version counters, e.g. ``p.data.copy_(...)``."""
        self._factor_key, self._factor = None, None
        if hasattr(self.kernel, "invalidate"):
            self.kernel.invalidate()

    def _key(self):
        ps = [p for p in self.kernel.parameters()] if isinstance(self.kernel, torch.nn.Module) else []
        ps.append(self.raw_likelihood_variance)
        return tuple((p.data_ptr(), p._version) for p in ps)

    def _factored(self, K: Optional[torch.Tensor] = None):
        """(F, logdet, info) of K[X, X] + sigma^2 I, cached per (kernel parameter versions, noise version)."""
        key = self._key()
        if self._factor is None or key != self._factor_key:
            with torch.no_grad():
                if K is None:
                    K = self.kernel.K_torch(self.X, self.X)
                self._factor = gpr_factor(K, self.likelihood_variance, self.engine)
            self._factor_key = key
            self._info = self._factor[2]
        return self._factor

    # ------------------------------------------------------------ training
    def log_marginal_likelihood(self) -> torch.Tensor:
        """log p(Y | X) summed over Y's columns: a differentiable fp64 scalar (NaN when ``cholesky_info`` != 0)."""
        K = self.kernel.K_torch(self.X, self.X)
        lml, info = gpr_log_marginal_likelihood(K, self.likelihood_variance, self.Y, factor=self._factored(K),
                                                engine=self.engine)
        self._info = info
        return lml

    def training_loss(self) -> torch.Tensor:
        return -self.log_marginal_likelihood()

    # ------------------------------------------------------------ prediction
    PREDICT_CHUNK = 2048  # test nodes per K_torch call of the variance path

    def _blocks(self, xs: torch.Tensor):
        """(K[xs, xs], K[xs, X]) as fresh fp64 matrices with contiguous rows, from ONE K_torch call.  They are
        copies: the solves and the product below work in place, and a kernel may hand out its own storage."""
        Kb = self.kernel.K_torch(xs, torch.cat([xs, self.X]))
        Kb = Kb.detach().to(self.engine.device, torch.float64, copy=True)
        m = xs.numel()
        return Kb[:, :m].contiguous(), Kb[:, m:].contiguous()

    @torch.no_grad()
    def predict_f(self, Xnew, full_cov: bool = False):
        """(mean, var) of the latent function at ``Xnew``: (n*, p) and (n*, p), or the covariance (p, n*, n*) with
        ``full_cov`` (GPflow's shapes).  The model's data and the kernel's matrices are not modified."""
        eng = self.engine
        xs = _nodes(Xnew).to(eng.device)
        p = int(self.Y.shape[1])
        F = self._factored()[0]
        Yt = self.Y.t().clone(memory_format=torch.contiguous_format)                 # p x n, a copy of the targets
        V = eng.cholesky_solve(F, Yt, transposed=False, inplace=True)                # (L^-1 Y)^T
        if full_cov:
            Kss, Ksx = self._blocks(xs)
            A = eng.cholesky_solve(F, Ksx, transposed=False, inplace=True)           # n* x n: rows L^-1 k_*
            mean = eng.gemm_nt_f64(A, V)                                             # n* x p
            cov = eng.gemm_nt_f64(A, A, alpha=-1.0, gamma=1.0, Z=Kss, out=Kss, symmetric=True)
            return mean, cov[None].expand(p, -1, -1).contiguous()
        means, variances = [], []
        for c in range(0, max(xs.numel(), 1), self.PREDICT_CHUNK):
            Kss, Ksx = self._blocks(xs[c:c + self.PREDICT_CHUNK])
            A = eng.cholesky_solve(F, Ksx, transposed=False, inplace=True)
            means.append(eng.gemm_nt_f64(A, V))
            variances.append(Kss.diagonal() - (A * A).sum(dim=1))
        mean, var = torch.cat(means), torch.cat(variances)
        return mean, var[:, None].expand(-1, p).contiguous()

    @torch.no_grad()
    def predict_y(self, Xnew, full_cov: bool = False):
        """``predict_f`` with the likelihood variance added to the variances (the covariance's diagonal)."""
        mean, var = self.predict_f(Xnew, full_cov=full_cov)
        s2 = self.likelihood_variance
        if full_cov:
            var.diagonal(dim1=-2, dim2=-1).add_(s2)
            return mean, var
        return mean, var + s2

    @torch.no_grad()
    def predict_log_density(self, data: Tuple) -> torch.Tensor:
        """log N(Ynew | mean, var + sigma^2) under ``predict_y``'s marginals, summed over the columns: (n*,)."""
        Xnew, Ynew = data
        mean, var = self.predict_y(Xnew)
        Yn = Ynew.detach() if torch.is_tensor(Ynew) else torch.as_tensor(np.asarray(Ynew, dtype=np.float64))
        Yn = Yn.to(mean.device, torch.float64).reshape(mean.shape)
        return (-0.5 * (_LOG_2PI + torch.log(var) + (Yn - mean) ** 2 / var)).sum(dim=1)
