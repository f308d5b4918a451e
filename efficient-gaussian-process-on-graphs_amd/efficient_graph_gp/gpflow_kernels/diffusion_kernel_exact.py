"""Exact diffusion kernel: mirror of gpflow_kernels/diffusion_kernel_exact.py:6-46.

K = sigma_f^2 exp(-beta L), the closed form the diffusion GRF and PoFM kernels approximate.  The reference calls
``tf.linalg.expm``; here E = exp(-beta L) comes from scaling and squaring on the fp64 matrix cores
(``GRFEngine.diffusion_expm``: 17 + s dense products, bitwise symmetric) and stays on the device, cached per value
of ``beta``.  ``beta`` and ``sigma_f`` are learnable positive parameters (raw ``torch.nn.Parameter``s under a
softplus, as in the sibling kernels).  ``K`` / ``K_diag`` / ``__call__`` return numpy; ``K_torch`` is
differentiable:
    d<G, K>/dbeta    = -sigma_f^2 <G, (L E)[x1, x2]>   one contraction-mode product with the rows x1 of L and x2 of
                                                       E (E is symmetric: E[:, x2] = E[x2, :]^T), never written,
    d<G, K>/dsigma_f = 2 sigma_f <G, E[x1, x2]>.
"""
import numpy as np
import torch

from grf_amd import api
from grf_amd.engine import get_engine

from .diffusion_kernel_fast_grf import _softplus_inverse
from .general_kernel_fast_grf import _indices


class _ExactKernelFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, beta, sigma_f, kernel, i1, i2):
        E = kernel.expm(float(beta))
        ctx.kernel, ctx.E, ctx.i1, ctx.i2 = kernel, E, i1, i2
        ctx.save_for_backward(sigma_f)
        return sigma_f.detach() ** 2 * E[i1][:, i2]

    @staticmethod
    def backward(ctx, g):
        (sigma_f,) = ctx.saved_tensors
        kernel, E, i1, i2 = ctx.kernel, ctx.E, ctx.i1, ctx.i2
        g = g.contiguous()
        g_beta = g_sigma = None
        if g.numel() == 0:
            zero = torch.zeros((), dtype=torch.float64, device=g.device)
            return zero, zero.clone(), None, None, None
        if ctx.needs_input_grad[0]:
            le = kernel.engine.gemm_nt_f64(kernel.L, E, ra=i1, rb=i2, W=g)
            g_beta = -(sigma_f ** 2) * le[0]
        if ctx.needs_input_grad[1]:
            g_sigma = 2.0 * sigma_f * (g * E[i1][:, i2]).sum()
        return g_beta, g_sigma, None, None, None


class GraphDiffusionKernel(torch.nn.Module):
    def __init__(self, adjacency_matrix, beta=None, sigma_f=None, normalize_laplacian=True, *, device=None, **kwargs):
        super().__init__()
        adjacency_matrix = np.asarray(adjacency_matrix, dtype=np.float64)
        assert adjacency_matrix.ndim == 2 and adjacency_matrix.shape[0] == adjacency_matrix.shape[1], \
            "Adjacency matrix must be square."
        beta, sigma_f = float(beta or 2.0), float(sigma_f or 1.0)
        if beta <= 0 or sigma_f <= 0:
            raise ValueError("beta and sigma_f must be positive")
        self.adjacency_matrix = adjacency_matrix
        self.normalize_laplacian = normalize_laplacian
        self.engine = get_engine(device)
        self.device = self.engine.device
        # the dense Laplacian and the bound on its spectral radius, once per graph
        self.L, self.radius = api.dense_laplacian_device(adjacency_matrix, normalize_laplacian, device)
        self.raw_beta = torch.nn.Parameter(torch.tensor(_softplus_inverse(beta), dtype=torch.float64,
                                                        device=self.device))
        self.raw_sigma_f = torch.nn.Parameter(torch.tensor(_softplus_inverse(sigma_f), dtype=torch.float64,
                                                           device=self.device))
        self._cache = None  # (beta, E)
        self.expm_count = 0  # how many times E was computed (the cache's misses)

    @property
    def beta(self) -> torch.Tensor:
        return torch.nn.functional.softplus(self.raw_beta)

    @property
    def sigma_f(self) -> torch.Tensor:
        return torch.nn.functional.softplus(self.raw_sigma_f)

    @property
    def laplacian(self) -> np.ndarray:
        return self.L.cpu().numpy()

    def expm(self, beta: float) -> torch.Tensor:
        """E = exp(-beta L) on the device, cached for the last value of beta."""
        beta = float(beta)
        if self._cache is None or self._cache[0] != beta:
            self._cache = (beta, self.engine.diffusion_expm(self.L, beta, beta * self.radius))
            self.expm_count += 1
        return self._cache[1]

    def invalidate(self) -> None:
        """Drop the cached E."""
        self._cache = None

    def diffusion_kernel(self, adj_matrix=None, beta=None, sigma_f=None) -> np.ndarray:
        """The whole K (reference :26-32) for this kernel's graph, fp64 numpy."""
        b = float(self.beta.detach()) if beta is None else float(beta)
        s = float(self.sigma_f.detach()) if sigma_f is None else float(sigma_f)
        return s ** 2 * self.expm(b).cpu().numpy()

    def _index_pair(self, X1, X2):
        n = self.L.shape[0]
        i1 = _indices(X1)
        i2 = i1 if X2 is None else _indices(X2)
        for i in (i1, i2):
            if i.numel() and (int(i.min()) < 0 or int(i.max()) >= n):
                raise IndexError(f"node indices must lie in [0, {n})")
        return i1.to(self.device), i2.to(self.device)

    def K_torch(self, X1, X2=None) -> torch.Tensor:
        i1, i2 = self._index_pair(X1, X2)
        return _ExactKernelFunction.apply(self.beta, self.sigma_f, self, i1, i2)

    def _scaled(self) -> torch.Tensor:
        return float(self.sigma_f.detach()) ** 2 * self.expm(float(self.beta.detach()))

    def K(self, X1, X2=None) -> np.ndarray:
        i1, i2 = self._index_pair(X1, X2)
        return self._scaled()[i1][:, i2].cpu().numpy()

    def K_diag(self, X) -> np.ndarray:
        i, _ = self._index_pair(X, None)
        return self._scaled().diagonal()[i].cpu().numpy()

    def __call__(self, X1, X2=None, full_cov=True):
        return self.K(X1, X2) if full_cov else self.K_diag(X1)
