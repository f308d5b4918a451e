"""Dense GP models on the kernels of ``efficient_graph_gp.gpflow_kernels`` (the reference's users put them into
``gpflow.models.GPR`` and ``gpflow.models.SVGP``; GPflow / TensorFlow are not installed, so the models are provided
here on the engine's fp64 Cholesky)."""
from .gpr import GPR
from .svgp import SVGP

__all__ = ["GPR", "SVGP"]
