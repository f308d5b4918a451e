from .sparse_diffusion_kernel import SparseDiffusionKernel
from .sparse_grf_kernel import SparseGRFKernel, SparseWalkOperatorKernel

__all__ = ["SparseGRFKernel", "SparseWalkOperatorKernel", "SparseDiffusionKernel"]
