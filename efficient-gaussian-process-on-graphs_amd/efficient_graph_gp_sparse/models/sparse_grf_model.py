"""SparseGraphGP: mirror of efficient_graph_gp_sparse/models/sparse_grf_model.py:10-45.

``predict`` is the pathwise-conditioning step after the GRF path:
    f_test  = eps1 Phi_test^T,  f_train = eps1 Phi_train^T,
    V       = linear_cg(K_train_train + s2 I, y - f_train - eps2)
    samples = f_test + (K_test_train V)^T
Here K is never formed: every product is Phi[rows] (Phi[cols]^T X) on the GPU
(``grf_spmm_csr`` / ``grf_cg_gram_solve*`` in libgrf_amd.so), and the CG runs the
same linear_cg rule (per-column normalisation, eps guards, stop at k >= 10 once the
mean residual < ``gpytorch.settings.cg_tolerance`` = 1) in fp64 by default
(``cg_dtype=torch.float32`` keeps the reference's fp32 recurrence).

The random draws are taken exactly as the reference takes them (same shapes, same
order, on the test inputs' device), so a seeded torch generator gives the same eps.
Subclasses ``gpytorch.models.ExactGP`` when gpytorch is installed; otherwise a
``torch.nn.Module`` whose ``forward`` returns (mean, covariance).
"""
import torch

from grf_amd.engine import DeviceCSR, WalkPolynomial, get_engine, preconditioner_name  # noqa: F401
from grf_amd.features import grf_marginal_log_likelihood, resolve_cg_tolerance

from ..gptorch_kernels_sparse.sparse_grf_kernel import SparseGRFKernel

try:
    import gpytorch
    _Base = gpytorch.models.ExactGP
except ImportError:  # pragma: no cover - depends on the environment
    gpytorch = None
    _Base = torch.nn.Module


EVAL_CG_TOLERANCE = 1e-2  # gpytorch.settings.eval_cg_tolerance: the solves of a prediction


def _noise_value(likelihood) -> float:
    noise = likelihood.noise if hasattr(likelihood, "noise") else likelihood
    return float(noise.item() if torch.is_tensor(noise) else noise)


class SparseGraphGP(_Base):
    def __init__(self, x_train, y_train, likelihood, step_matrices, max_walk_length):
        if gpytorch is not None:
            super().__init__(x_train, y_train, likelihood)
            self.mean_module = gpytorch.means.ZeroMean()
        else:
            super().__init__()
            self.likelihood = likelihood
        self.x_train, self.y_train = x_train, y_train
        self.covar_module = SparseGRFKernel(max_walk_length=max_walk_length, step_matrices_torch=step_matrices)
        # (step_matrices may be a WalkPolynomial: predict and marginal_log_likelihood then run on the exact
        # kernel Phi = p(G) as a matrix-free operator)
        self.num_nodes = (step_matrices if isinstance(step_matrices, WalkPolynomial) else step_matrices[0]).shape[0]

    def forward(self, x):
        if gpytorch is not None:
            return gpytorch.distributions.MultivariateNormal(self.mean_module(x), self.covar_module(x))
        K = self.covar_module(x, x)
        return torch.zeros(K.shape[0], dtype=K.dtype, device=K.device), K

    def _phi_csr(self, device) -> DeviceCSR:
        """Phi = sum_l f_l M_l (current modulator) as a device CSR (rows ascending, columns
        ascending within a row, fp32 values; grf_phi_steps_csr on the kernel's step matrices)."""
        phi = self.covar_module._step_set().phi(self.covar_module.modulator_vector)
        if phi.ptr.device != torch.device(device):
            raise ValueError("predict: the step matrices live on another device than x_test")
        return phi

    def marginal_log_likelihood(self, probes=None, n_probes=64, generator=None, tolerance=None, max_iter=1000,
                                per_datum=True, preconditioner=None):
        """The training objective the reference evaluates as ``mll(model(x_train), y_train)`` under
        ``max_cholesky_size(0)``: the marginal log-likelihood of ``y_train`` (zero mean) by CG and stochastic
        Lanczos quadrature, K never formed (``grf_amd.features.grf_marginal_log_likelihood``).  A
        differentiable fp64 scalar: ``backward()`` fills the modulator's gradient and, when the likelihood's
        noise is a tensor, the noise's (a float noise is a constant).  ``per_datum`` divides by the number
        of training points, as ``ExactMarginalLogLikelihood`` does.  ``preconditioner="jacobi"`` preconditions the
        solve by diag(K^) (None, the default: the reference's unpreconditioned solve)."""
        noise = self.likelihood.noise if hasattr(self.likelihood, "noise") else self.likelihood
        info = {}
        out = grf_marginal_log_likelihood(
            self.covar_module.modulator_vector, noise, self.covar_module._step_set(), self.x_train.int().flatten(),
            self.y_train, probes=probes, n_probes=n_probes, generator=generator, tolerance=tolerance,
            max_iter=max_iter, per_datum=per_datum, info=info, preconditioner=preconditioner)
        self.last_cg_iterations = info["cg_iterations"]
        return out

    @torch.no_grad()
    def predict(self, x_test, n_samples=64, cg_dtype=torch.float64, max_iter=1000, tolerance=None,
                preconditioner=None):
        """(n_samples x n_test) posterior samples (float32, like the reference).  ``preconditioner="jacobi"``
        preconditions the solve by diag(K^) (fp64 only: with ``cg_dtype=torch.float32`` a ValueError)."""
        preconditioner_name(preconditioner, "predict")
        if preconditioner is not None and cg_dtype != torch.float64:
            raise ValueError("predict: preconditioner=\"jacobi\" needs cg_dtype=torch.float64")
        dev = x_test.device
        train_indices = self.x_train.int().flatten()
        test_indices = x_test.int().flatten()
        eng = get_engine(dev if dev.type == "cuda" else None)
        op = self.covar_module._operator()
        if op is not None and op.engine.device != eng.device:
            raise ValueError("predict: the walk operator lives on another device than x_test")
        phi = op if op is not None else self._phi_csr(eng.device)

        noise_variance = _noise_value(self.likelihood)
        noise_std = torch.sqrt(torch.tensor(noise_variance, device=dev))
        # the reference's draws, same shapes and order (sparse_grf_model.py:36-37)
        eps1_batch = torch.randn(n_samples, self.num_nodes, device=dev)
        eps2_batch = noise_std * torch.randn(n_samples, len(train_indices), device=dev)
        tolerance = resolve_cg_tolerance(tolerance)
        out, self.last_cg_iterations = eng.pathwise_predict(
            phi, train_indices.to(eng.device), test_indices.to(eng.device), self.y_train, noise_variance,
            eps1_batch, eps2_batch, tolerance=tolerance, max_iter=max_iter, dtype=cg_dtype,
            f=self.covar_module.modulator_vector if op is not None else None, preconditioner=preconditioner)
        return out.to(torch.float32)

    def _moments(self, x_test, full_cov, tolerance, max_iter, add_noise, preconditioner=None):
        preconditioner_name(preconditioner, "predict_f")
        dev = x_test.device
        eng = get_engine(dev if dev.type == "cuda" else None)
        op = self.covar_module._operator()
        if op is not None and op.engine.device != eng.device:
            raise ValueError("predict_f: the walk operator lives on another device than x_test")
        phi = op if op is not None else self._phi_csr(eng.device)
        info = {}
        out = eng.posterior_moments(
            phi, self.x_train.int().flatten().to(eng.device), x_test.int().flatten().to(eng.device), self.y_train,
            _noise_value(self.likelihood), f=self.covar_module.modulator_vector if op is not None else None,
            full_cov=full_cov, tolerance=EVAL_CG_TOLERANCE if tolerance is None else float(tolerance),
            max_iter=max_iter, info=info, add_noise=add_noise, preconditioner=preconditioner)
        self.last_cg_iterations = max(info["cg_iterations"] + [info["alpha_iterations"]])
        return out

    @torch.no_grad()
    def predict_f(self, x_test, full_cov=False, tolerance=None, max_iter=1000, preconditioner=None):
        """The exact posterior mean and variance of the latent function at ``x_test``: (mean, var), fp64
        tensors of shape (n_test,), or with ``full_cov`` (mean, cov) with cov (n_test x n_test) -- what the
        reference's dense baseline returns from ``model.predict_f`` (run_scaling_experiment.py:729) and its
        sparse model can only estimate from pathwise samples (``predict(...).mean(0) / .std(0)``).

        K is never formed: the test nodes go through batched CG solves of 256 columns on the walk's Phi or on
        the WalkPolynomial operator, whichever the model was built on (``GRFEngine.posterior_moments``).
        ``tolerance`` defaults to gpytorch's eval_cg_tolerance (1e-2), not the training default of 1.

        Variances are returned as computed, never clamped.  What makes that safe is a property of CG: from a
        zero start, b^T x_k increases monotonically to b^T K^-1 b, so a solve that stops early over-estimates
        the variance and never under-estimates it, up to rounding.  In floating point that holds for b^T x_k
        only while CG keeps its residual orthogonal to the Krylov space (b^T K^-1 b - b^T x_k =
        ||x - x_k||^2_K + x_k^T r_k, and on the walk's ill-conditioned Phi the last term put a stopped solve
        1e-4 of the prior below the truth), so the variance is formed from the energy form
        x_k^T (2 b - K^ x_k) = b^T K^-1 b - ||x - x_k||^2_K, which is below b^T K^-1 b for any x_k at the cost of
        one more operator product per chunk.
        ``last_cg_iterations`` is the largest iteration count over the chunks' solves and the solve for the
        mean.  ``preconditioner="jacobi"`` preconditions every solve by diag(K^), built once per call; the
        energy form's bound holds for any iterate, so the statement on the variances is unchanged."""
        return self._moments(x_test, full_cov, tolerance, max_iter, False, preconditioner)

    @torch.no_grad()
    def predict_y(self, x_test, full_cov=False, tolerance=None, max_iter=1000, preconditioner=None):
        """``predict_f`` for the noisy observation: the noise variance added to the variances, or to the
        covariance's diagonal."""
        return self._moments(x_test, full_cov, tolerance, max_iter, True, preconditioner)

    @torch.no_grad()
    def nlpd(self, x_test, y_test, tolerance=None, max_iter=1000, preconditioner=None):
        """The negative log predictive density of ``y_test`` under ``predict_y``'s marginals, by the reference's
        formula (wind_experiment.py:319-324): an fp64 scalar tensor."""
        mean, var = self.predict_y(x_test, tolerance=tolerance, max_iter=max_iter, preconditioner=preconditioner)
        y = y_test.to(mean.device, torch.float64).flatten()
        std = var.sqrt()
        z = (y - mean) / std
        return (0.5 * torch.log(2.0 * torch.pi * std * std) + 0.5 * z * z).mean()
