"""GRF kernel for GPyTorch: mirror of gptorch_kernels_sparse/sparse_grf_kernel.py:5-61.

K[x1, x2] = Phi[x1] Phi[x2]^T with Phi = sum_l f_l M_l and a learnable modulator f.  The step
matrices stay on the GPU; Phi, the row selections, K (the exact fixed-point sparse Gram) and the
gradient w.r.t. f run on the HIP kernels behind ``grf_amd.features.GRFKernelFunction`` -- Phi is
never densified.  Subclasses ``gpytorch.kernels.Kernel`` when gpytorch is installed, else
``torch.nn.Module`` with the same ``forward(x1_idx, x2_idx, diag)`` signature.
"""
import torch

from grf_amd.features import StepMatrices, WalkPolynomial, feature_matrix, grf_kernel

try:
    import gpytorch
    _Base = gpytorch.kernels.Kernel
except ImportError:  # pragma: no cover - depends on the environment
    _Base = torch.nn.Module


class SparseGRFKernel(_Base):
    def __init__(self, max_walk_length, step_matrices_torch, **kwargs):
        super().__init__(**kwargs) if _Base is not torch.nn.Module else super().__init__()
        self.register_parameter("raw_modulator_vector",
                                torch.nn.Parameter(torch.randn(max_walk_length)))
        self.step_matrices = step_matrices_torch
        self._steps = None

    @property
    def modulator_vector(self):
        return self.raw_modulator_vector

    def _operator(self):
        """The WalkPolynomial this kernel was built on (``step_matrices_torch=<WalkPolynomial>``), else None."""
        return self.step_matrices if isinstance(self.step_matrices, WalkPolynomial) else None

    def _no_blocks(self, what: str):
        return NotImplementedError(
            f"SparseGRFKernel.{what} needs step matrices: on a WalkPolynomial Phi is never formed; use "
            "SparseGraphGP.predict and SparseGraphGP.marginal_log_likelihood, which run on the operator, and "
            "SparseWalkOperatorKernel.forward or grf_amd.features.grf_kernel for K blocks and diagonals")

    def _step_set(self):
        """The StepMatrices of the kernel's step matrices, or its WalkPolynomial."""
        if self._operator() is not None:
            return self.step_matrices
        if self._steps is None:
            self._steps = StepMatrices(self.step_matrices)
        return self._steps

    def forward(self, x1_idx=None, x2_idx=None, diag=False, **params):
        """K[x1, x2] (or its diagonal) = Phi[x1] Phi[x2]^T (reference :24-49)."""
        if self._operator() is not None:
            raise self._no_blocks("forward")
        return grf_kernel(self.modulator_vector, self._step_set(), x1_idx, x2_idx, diag)

    def _get_feature_matrix(self):
        """Phi as a torch sparse CSR tensor on the device (reference :51-61; not differentiable:
        gradients flow through ``forward``)."""
        if self._operator() is not None:
            raise self._no_blocks("_get_feature_matrix")
        return feature_matrix(self.modulator_vector, self._step_set())


class SparseWalkOperatorKernel(SparseGRFKernel):
    """SparseGRFKernel on a ``WalkPolynomial`` (``step_matrices_torch=<WalkPolynomial>``): ``forward`` returns
    blocks and diagonals of the exact K = p(G) p(G)^T from the operator itself (fp64 chains with the walk matrix,
    the result in the modulator's dtype), differentiable in the modulator.  Phi is still never formed, so
    ``_get_feature_matrix`` keeps raising."""

    def __init__(self, max_walk_length, step_matrices_torch, **kwargs):
        if not isinstance(step_matrices_torch, WalkPolynomial):
            raise TypeError("SparseWalkOperatorKernel needs a WalkPolynomial (GraphPreprocessor.walk_operator())")
        super().__init__(max_walk_length, step_matrices_torch, **kwargs)

    def forward(self, x1_idx=None, x2_idx=None, diag=False, **params):
        """K[x1, x2], or with ``diag`` (x1 and x2 the same tensor) diag K[x1]."""
        return grf_kernel(self.modulator_vector, self.step_matrices, x1_idx, x2_idx, diag)
