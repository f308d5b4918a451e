"""Sparse variational GP: mirror of ``gpflow.models.SVGP`` as the reference's headline dense experiment uses it
(experiments/dense/cora/classification_multiple_{GRF,GRF_small,diff,diff_small}.ipynb):

    likelihood = gpflow.likelihoods.MultiClass(num_classes=7)
    model = gpflow.models.SVGP(kernel=graph_kernel, likelihood=likelihood, inducing_variable=Z,
                               num_latent_gps=7, whiten=True)

trained by Adam on ``model.training_loss((X, Y))`` and reported as ``argmax(model.predict_y(x_test)[0])``.

Everything runs on the engine with no host read of device data: ``elbo`` is ``grf_amd.features.svgp_elbo`` (the fp64
Cholesky factor of K[Z, Z] + jitter I, the whitened conditional by one triangular solve and two products, the
likelihood's expectations with their gradient in one launch, the backward of the factor by products and solves), so
the kernel's own backward carries the gradient on to its parameters.  The inducing variable is a fixed set of node
ids (in the reference its gradient through ``tf.gather`` is None and the notebooks filter it out).  Node sets are
integer node ids in the forms ``GPR`` accepts; values come back as fp64 tensors on the device.  The predictions are
not differentiable.
"""
from typing import Optional, Tuple

import torch

from grf_amd.engine import get_engine
from grf_amd.features import svgp_conditional, svgp_elbo, svgp_factor

from ..likelihoods import Gaussian, MultiClass
from .gpr import _nodes


class SVGP(torch.nn.Module):
    def __init__(self, kernel, likelihood, inducing_variable, *, mean_function=None, num_latent_gps: int = 1,
                 q_diag: bool = False, q_mu=None, q_sqrt=None, whiten: bool = True, num_data: Optional[int] = None,
                 jitter: float = 1e-6, device=None):
        super().__init__()
        if mean_function is not None:
            raise NotImplementedError("SVGP: only the zero mean function (mean_function=None) is supported")
        if q_diag:
            raise NotImplementedError("SVGP: only a full q_sqrt (q_diag=False) is supported")
        if not whiten:
            raise NotImplementedError("SVGP: only the whitened parameterisation (whiten=True) is supported")
        if not hasattr(kernel, "K_torch"):
            raise TypeError("SVGP: the kernel must expose K_torch(X1, X2)")
        if not isinstance(likelihood, (MultiClass, Gaussian)):
            raise NotImplementedError("SVGP: the likelihood must be MultiClass (RobustMax) or Gaussian")
        self.engine = get_engine(device)
        dev = self.engine.device
        self.kernel = kernel
        self.likelihood = likelihood.to(dev)
        self.Z = _nodes(inducing_variable).to(dev)
        M, P = int(self.Z.numel()), int(num_latent_gps)
        if M < 1 or P < 1:
            raise ValueError("SVGP: at least one inducing node and one latent GP are needed")
        if isinstance(likelihood, MultiClass) and likelihood.num_classes != P:
            raise ValueError("SVGP: MultiClass needs num_latent_gps == num_classes")
        self.num_latent_gps, self.num_data, self.jitter = P, num_data, float(jitter)
        qm = torch.zeros((M, P), dtype=torch.float64) if q_mu is None else torch.as_tensor(q_mu, dtype=torch.float64)
        qs = torch.eye(M, dtype=torch.float64).repeat(P, 1, 1) if q_sqrt is None \
            else torch.as_tensor(q_sqrt, dtype=torch.float64)
        if tuple(qm.shape) != (M, P) or tuple(qs.shape) != (P, M, M):
            raise ValueError(f"SVGP: q_mu must be ({M} x {P}) and q_sqrt ({P} x {M} x {M})")
        self.q_mu = torch.nn.Parameter(qm.detach().clone().to(dev))
        self.q_sqrt = torch.nn.Parameter(torch.tril(qs.detach().clone()).to(dev))
        self._factor_key = None
        self._factor = None
        self._info = None
        self._data = None

    # ------------------------------------------------------------ the cached factor of K[Z, Z] + jitter I
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
                                 f"{info} of K[Z, Z] + jitter I is not positive definite")

    def invalidate(self) -> None:
        """Drop the cached factor (and the kernel's cached K): needed only after a parameter write that bypasses
        the version counters."""
        self._factor_key, self._factor = None, None
        if hasattr(self.kernel, "invalidate"):
            self.kernel.invalidate()

    def _key(self):
        ps = [p for p in self.kernel.parameters()] if isinstance(self.kernel, torch.nn.Module) else []
        return tuple((p.data_ptr(), p._version) for p in ps)

    def _factored(self, Kmm: Optional[torch.Tensor] = None):
        """(F, logdet, info) of K[Z, Z] + jitter I, cached per kernel parameter versions."""
        key = self._key()
        if self._factor is None or key != self._factor_key:
            with torch.no_grad():
                if Kmm is None:
                    Kmm = self.kernel.K_torch(self.Z, self.Z)
                self._factor = svgp_factor(Kmm, self.jitter, self.engine)
            self._factor_key = key
            self._info = self._factor[2]
        return self._factor

    # ------------------------------------------------------------ training
    def _on_device(self, data: Tuple):
        """(node ids, targets) of ``data = (X, Y)`` on the device.  The labels are validated on the host at the call
        (integers in [0, num_classes)) and uploaded; the result is kept for the next call with the same two
        objects (tensors: at the same version), so that a training loop's steps read nothing back.  A host array
        changed in place after its first use is not seen: pass a new one."""
        X, Y = data
        key = tuple((id(t), t._version if torch.is_tensor(t) else None) for t in (X, Y))
        if self._data is None or self._data[0] != key:
            xs = _nodes(X).to(self.engine.device)
            Yd = self.likelihood.targets(Y, int(xs.numel()), self.engine.device)
            if Yd.dim() == 2 and Yd.shape[1] != self.num_latent_gps:
                raise ValueError(f"SVGP: Y must have {self.num_latent_gps} columns")
            self._data = (key, (X, Y), xs, Yd)      # (X and Y are held: their ids stay theirs)
        return self._data[2], self._data[3]

    def prior_kl(self) -> torch.Tensor:
        """KL(q(v) || N(0, I)) summed over the latents (gauss_kl, whitened): a differentiable fp64 scalar."""
        Lq = torch.tril(self.q_sqrt)
        P, M = int(Lq.shape[0]), int(Lq.shape[1])
        return 0.5 * ((self.q_mu * self.q_mu).sum() - float(P * M)
                      - torch.log(Lq.diagonal(dim1=1, dim2=2) ** 2).sum() + (Lq * Lq).sum())

    def elbo(self, data: Tuple) -> torch.Tensor:
        """The evidence lower bound of ``data = (X, Y)``: a differentiable fp64 scalar (NaN when ``cholesky_info``
        != 0); the expectation term is scaled by num_data / batch when ``num_data`` was given."""
        xs, Yd = self._on_device(data)
        n = int(xs.numel())
        Kb = self.kernel.K_torch(torch.cat([self.Z, xs]), self.Z)
        M = int(self.Z.numel())
        Kmm, Knm = Kb[:M], Kb[M:]
        Knn = self.kernel.K_torch(xs, xs).diagonal()
        scale = 1.0 if self.num_data is None else float(self.num_data) / n
        elbo, info = svgp_elbo(Kmm, Knm, Knn, self.q_mu, self.q_sqrt, Yd, self.likelihood, scale=scale,
                               jitter=self.jitter, factor=self._factored(Kmm), engine=self.engine)
        self._info = info
        return elbo

    def training_loss(self, data: Tuple) -> torch.Tensor:
        return -self.elbo(data)

    # ------------------------------------------------------------ prediction
    PREDICT_CHUNK = 2048  # test nodes per K_torch call

    def _blocks(self, xs: torch.Tensor):
        """(K[xs, xs], K[xs, Z]) as fresh fp64 matrices with contiguous rows, from ONE K_torch call.  They are
        copies: the solve below works in place, and a kernel may hand out its own storage."""
        Kb = self.kernel.K_torch(xs, torch.cat([xs, self.Z]))
        Kb = Kb.detach().to(self.engine.device, torch.float64, copy=True)
        m = xs.numel()
        return Kb[:, :m].contiguous(), Kb[:, m:].contiguous()

    def _q(self):
        return self.q_mu.detach().to(torch.float64), torch.tril(self.q_sqrt.detach().to(torch.float64))

    @torch.no_grad()
    def predict_f(self, Xnew, full_cov: bool = False):
        """(mean, var) of the latent functions at ``Xnew``: (n*, P) and (n*, P), or the covariances (P, n*, n*)
        with ``full_cov`` (GPflow's shapes): K** - A^T A, computed once, plus T_p T_p^T per latent (symmetric products;
        the whole (P, n*, n*) result must fit the device: it is not chunked)."""
        eng = self.engine
        xs = _nodes(Xnew).to(eng.device)
        F = self._factored()[0]
        qm, Lq = self._q()
        P, M = int(Lq.shape[0]), int(Lq.shape[1])
        if full_cov:
            Kss, Ksz = self._blocks(xs)
            AT, T, mean, _ = svgp_conditional(eng, F, Ksz, Kss.diagonal(), qm, Lq)
            ns = int(xs.numel())
            eng._dense_memory_guard("predict_f(full_cov=True)", ns, (P + 1) * ns * ns * 8)
            C = eng.gemm_nt_f64(AT, AT, alpha=-1.0, gamma=1.0, Z=Kss, out=Kss, symmetric=True)   # K** - A^T A, once
            cov = torch.empty((P, ns, ns), dtype=torch.float64, device=eng.device)
            for p in range(P):
                Tp = T[:, p * M:(p + 1) * M]
                eng.gemm_nt_f64(Tp, Tp, gamma=1.0, Z=C, out=cov[p], symmetric=True)
            return mean, cov
        means, variances = [], []
        for c in range(0, max(xs.numel(), 1), self.PREDICT_CHUNK):
            Kss, Ksz = self._blocks(xs[c:c + self.PREDICT_CHUNK])
            _, _, mean, var = svgp_conditional(eng, F, Ksz, Kss.diagonal(), qm, Lq)
            means.append(mean)
            variances.append(var)
        return torch.cat(means), torch.cat(variances)

    @torch.no_grad()
    def predict_y(self, Xnew):
        """MultiClass: (ps, ps - ps^2), the class probabilities (n*, P); Gaussian: (mean, var + sigma^2)."""
        mean, var = self.predict_f(Xnew)
        return self.likelihood.predict_mean_and_var(self.engine, mean, var)

    @torch.no_grad()
    def predict_log_density(self, data: Tuple) -> torch.Tensor:
        """log p(Ynew | q) under ``predict_f``'s marginals: (n*,)."""
        Xnew, Ynew = data
        mean, var = self.predict_f(Xnew)
        Yd = self.likelihood.targets(Ynew, int(mean.shape[0]), self.engine.device)
        return self.likelihood.predict_log_density(self.engine, mean, var, Yd)
