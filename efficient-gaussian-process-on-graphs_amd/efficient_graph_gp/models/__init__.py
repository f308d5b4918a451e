"""Dense exact GP models on the kernels of ``efficient_graph_gp.gpflow_kernels`` (the reference's users put them
into ``gpflow.models.GPR``; GPflow / TensorFlow are not installed, so the model is provided here on the engine's
fp64 Cholesky)."""
from .gpr import GPR

__all__ = ["GPR"]
