"""Diffusion exact walk-power (PoFM) kernel: mirror of gpflow_kernels/diffusion_kernel_pofm.py:7-40.

K = sigma_f^2 K_f K_f^T with K_f = sum_i (-beta / 2)^i / i! L^i, i = 0 .. max_expansion: the truncated
series of exp(-beta L / 2) the diffusion fast-GRF kernel estimates.  The exact powers [I, L, ..., L^max_expansion]
come from the device SpGEMM (``GRFEngine.exact_steps``) and stay on the device as the dense step tensor; the
learnable positive ``beta`` / ``sigma_f``, the modulator formula, the cached MFMA Gram, ``K`` / ``K_diag`` /
``__call__`` / ``K_torch`` and its gradients are GraphDiffusionFastGRFKernel's (with max_expansion + 1 steps).
"""
import numpy as np

from grf_amd import _lib as C
from grf_amd import api

from .diffusion_kernel_fast_grf import GraphDiffusionFastGRFKernel


class GraphDiffusionPoFMKernel(GraphDiffusionFastGRFKernel):
    def __init__(self, adjacency_matrix, beta: float = 2.0, max_expansion: int = 5, sigma_f: float = 1.0,
                 normalize_laplacian: bool = True, *, device=None, **kwargs):
        adjacency_matrix = np.asarray(adjacency_matrix, dtype=np.float64)
        assert adjacency_matrix.ndim == 2 and adjacency_matrix.shape[0] == adjacency_matrix.shape[1], \
            "Adjacency matrix must be square."
        if beta <= 0 or sigma_f <= 0:
            raise ValueError("beta and sigma_f must be positive")
        mode = C.LAP_NUMPY_SAFE if normalize_laplacian else C.LAP_COMBINATORIAL
        F = api.exact_step_tensor_device(adjacency_matrix, max_expansion + 1, laplacian_mode=mode, device=device)
        super().__init__(adjacency_matrix, max_walk_length=max_expansion + 1, beta=beta, sigma_f=sigma_f,
                         normalize_laplacian=normalize_laplacian, device=device, step_matrices=F)
        self.max_expansion = max_expansion
        self.normalize_laplacian = normalize_laplacian
        del self.walks_per_node, self.p_halt  # (no walks here)

    def compute_diffusion_kernel(self, adj_matrix=None, beta=None, max_expansion=None) -> np.ndarray:
        """The whole K (reference :30-39) for this kernel's graph, fp64 numpy."""
        if max_expansion is not None and max_expansion != self.max_expansion:
            raise ValueError("max_expansion is fixed at construction (the powers are precomputed)")
        b = self.beta.detach() if beta is None else beta
        return self.grf_kernel(float(b), float(self.sigma_f.detach()))
