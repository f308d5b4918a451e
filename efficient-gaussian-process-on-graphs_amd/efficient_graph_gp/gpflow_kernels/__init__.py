"""GPflow-style GRF kernels (mirror of efficient_graph_gp/gpflow_kernels/__init__.py).

GPflow / TensorFlow are not installed in this image, so the two fast-GRF kernels
are provided with the same constructor and ``K`` / ``K_diag`` / ``grf_kernel`` API
backed by the GPU engine (numpy in, numpy out), and so are the two exact walk-power
(PoFM) kernels they estimate, on the device SpGEMM's exact step matrices.  The
package-level names GraphDiffusionKernel and GraphDiffusionGRFKernel raise NotImplementedError;
the closed-form kernel sigma_f^2 exp(-beta L) is in the submodule ``diffusion_kernel_exact``
(the reference's module path), the TF-walker kernel is outside the GRF hot path.
"""
from .diffusion_kernel_fast_grf import GraphDiffusionFastGRFKernel
from .diffusion_kernel_pofm import GraphDiffusionPoFMKernel
from .general_kernel_fast_grf import GraphGeneralFastGRFKernel
from .general_kernel_pofm import GraphGeneralPoFMKernel


def _out_of_scope(name):
    class _Stub:
        def __init__(self, *a, **k):
            raise NotImplementedError(f"{name} is outside the GRF hot path this engine implements (see DESIGN.md)")
    _Stub.__name__ = name
    return _Stub


GraphDiffusionKernel = _out_of_scope("GraphDiffusionKernel")
GraphDiffusionGRFKernel = _out_of_scope("GraphDiffusionGRFKernel")

__all__ = ["GraphDiffusionKernel", "GraphDiffusionPoFMKernel", "GraphDiffusionGRFKernel",
           "GraphDiffusionFastGRFKernel", "GraphGeneralPoFMKernel", "GraphGeneralFastGRFKernel"]
