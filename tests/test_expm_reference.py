"""CPU: the numpy restatement of grf_expm_sym_f64 (tests/expm_reference.py) against the eigendecomposition truth,
scipy.linalg.expm (the reference's own function) and the golden fixture made by the reference's diffusion_kernel;
its analytic gradients against central differences.  The bounds are 10x the errors measured and recorded in
tests/expm_reference.py."""
import math

import numpy as np
import pytest
import scipy.linalg

import expm_reference as R


def test_squarings_rule():
    assert [R.squarings(r) for r in (0.0, 0.3, 1.0, 1.0000001, 2.0, 2.5, 4.0, 800.0, 1024.0, 1025.0)] == \
        [0, 0, 0, 1, 1, 2, 2, 10, 10, 11]
    assert R.squarings(float("inf")) == -1 and R.squarings(float("nan")) == -1
    assert R.product_count(4.0) == 19
    # theta = 1: the scaled matrix's bound is at most 1, and the degree-18 remainder is below 1e-17
    for rho in (0.5, 1.0, 3.0, 4.0, 239200.0):
        assert rho / 2 ** R.squarings(rho) <= 1.0
    assert 1.0 / math.factorial(19) < 1e-17


@pytest.mark.parametrize("key,g,normalize,beta", list(R.cases()))
def test_restatement_against_truth_and_scipy(key, g, normalize, beta):
    W, L, rho, T = R.case_data(g, normalize, beta)
    E = R.expm_restated(L, beta, rho)
    err = float(np.abs(E - T).max())
    S = scipy.linalg.expm(-beta * L)
    err_scipy = float(np.abs(E - S).max())
    scipy_truth = float(np.abs(S - T).max())
    print(f"{key}: s = {R.squarings(rho)}, |E - truth| = {err:.2e} (recorded {R.MEASURED[key]:.2e}), "
          f"|E - scipy| = {err_scipy:.2e}, |scipy - truth| = {scipy_truth:.2e}")
    assert np.array_equal(E, E.T)
    assert err <= 10 * R.MEASURED[key]
    # scipy against the restatement: within the restatement's bound plus scipy's own distance from the truth
    assert err_scipy <= 10 * R.MEASURED[key] + scipy_truth


def test_s_zero_and_large_s_are_both_reached():
    s = [R.squarings(R.case_data(g, nz, b)[2]) for _, g, nz, b in R.cases()]
    assert min(s) == 0 and max(s) >= 10


@pytest.mark.parametrize("key,g,normalize,beta", list(R.grad_cases()))
def test_analytic_gradients_against_central_differences(key, g, normalize, beta):
    W, L, rho, _ = R.case_data(g, normalize, beta)
    x1, x2, G = R.grad_inputs()
    E = R.expm_restated(L, beta, rho)
    d_beta, d_sigma, scale_beta, scale_sigma = R.kernel_grads(L, E, R.GRAD_SIGMA, x1, x2, G)
    fd_beta, fd_sigma = R.fd_grads(g, normalize, beta, R.GRAD_SIGMA, x1, x2, G)
    e_beta, e_sigma = abs(d_beta - fd_beta) / scale_beta, abs(d_sigma - fd_sigma) / scale_sigma
    print(f"{key}: d/dbeta {d_beta:.6e} (fd {fd_beta:.6e}, rel {e_beta:.2e}), "
          f"d/dsigma {d_sigma:.6e} (fd {fd_sigma:.6e}, rel {e_sigma:.2e}); recorded {R.MEASURED_GRAD[key]}")
    assert e_beta <= 10 * R.MEASURED_GRAD[key][0]
    assert e_sigma <= 10 * R.MEASURED_GRAD[key][1]


def test_restatement_against_the_reference_fixture(golden):
    d = golden("expm")
    for name in ("toy", "isolated"):
        W = d[name + "_adj"]
        L = R.laplacian(W, True)
        if name == "isolated":
            assert W[7].sum() == 0 and L[7, 7] == 1.0 and np.count_nonzero(L[7]) == 1
        for beta in d["betas"]:
            K = d[f"{name}_K_{beta:g}"]
            E = R.expm_restated(L, float(beta), R.rho_bound(W, L, float(beta), True))
            # n <= 40, s <= 2: 19 products of rows whose absolute sums are at most sqrt(n), each within
            # (n + 4) 2^-53 of its exact value, doubled twice by the squarings -- well below 1e-13; scipy's Pade
            # approximant is held to the same figure
            assert np.abs(E - K).max() <= 1e-13, (name, beta, np.abs(E - K).max())


def test_small_and_degenerate_inputs():
    assert np.allclose(R.expm_restated(np.array([[0.7]]), 2.0, 1.4), [[math.exp(-1.4)]], rtol=0, atol=1e-15)
    L2 = np.array([[1.0, -1.0], [-1.0, 1.0]])
    assert np.abs(R.expm_restated(L2, 3.0, 6.0) - R.expm_truth(L2, 3.0)).max() <= 1e-15
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            R.expm_restated(L2, bad, 1.0)
    with pytest.raises(ValueError):
        R.expm_restated(L2, 1.0, float("inf"))
