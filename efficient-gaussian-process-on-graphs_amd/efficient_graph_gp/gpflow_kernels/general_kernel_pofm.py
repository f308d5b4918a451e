"""General-modulator exact walk-power (PoFM) kernel: mirror of gpflow_kernels/general_kernel_pofm.py:45-96.

The kernel the fast-GRF kernels estimate: its (N, N, L) step tensor is the exact [I, L, L^2, ...]
(the reference's ``compute_pstep_walk_matrix``, :7-42) instead of a random-walk estimate of it.  The powers
are chained on the device SpGEMM (``GRFEngine.exact_steps``, fp64, scipy's summation order) on the
safe-degree normalised Laplacian (``normalize_laplacian=False``: the combinatorial one), densified there and
kept on the device.  Everything after that -- the learnable fp64 ``modulator_vector``, Phi = F f, the cached
MFMA Gram, ``K`` / ``K_diag`` / ``__call__`` / ``K_torch`` and its gradient -- is GraphGeneralFastGRFKernel's.
"""
import numpy as np

from grf_amd import _lib as C
from grf_amd import api

from .general_kernel_fast_grf import GraphGeneralFastGRFKernel


class GraphGeneralPoFMKernel(GraphGeneralFastGRFKernel):
    def __init__(self, adjacency_matrix, max_walk_length: int = 10, modulator_vector: np.ndarray = None,
                 normalize_laplacian: bool = True, *, device=None, **kwargs):
        adjacency_matrix = np.asarray(adjacency_matrix, dtype=np.float64)
        assert adjacency_matrix.ndim == 2 and adjacency_matrix.shape[0] == adjacency_matrix.shape[1], \
            "Adjacency matrix must be square."
        if modulator_vector is not None and len(modulator_vector) != max_walk_length:
            raise ValueError("The length of the modulator vector must be equal to the max_walk_length.")
        mode = C.LAP_NUMPY_SAFE if normalize_laplacian else C.LAP_COMBINATORIAL
        F = api.exact_step_tensor_device(adjacency_matrix, max_walk_length, laplacian_mode=mode, device=device)
        super().__init__(adjacency_matrix, max_walk_length=max_walk_length, modulator_vector=modulator_vector,
                         step_matrices=F, device=device)
        self._lap_mode = mode
        del self.walks_per_node, self.p_halt  # (no walks here)

    def pofm_kernel(self, modulator_vector) -> np.ndarray:
        """The whole K (reference :94-96), fp64 numpy."""
        return self.grf_kernel(modulator_vector)
