"""CPU: the numpy restatement of the dense exact GPR (tests/gpr_reference.py) meets its np.longdouble truth within
the bounds the GPU tests use, and numpy.linalg.cholesky stays inside the same bounds.

Bounds (u = 2^-53, gamma_k = k u / (1 - k u)), compared, never divided:
    |A - L L^T| <= gamma_{n+1} |L| |L^T| on the lower triangle (Higham Thm 10.3),
    |b - T x| <= gamma_n |T| |x| for T = L and L^T (Thm 8.5),
    logdet against the header's statement restated in fp64 (the terms RN(2 log F_ii) added in ascending i; on the
    CPU that is the restatement's own loop, so the check pins the helper the GPU test compares the device with),
    the GPR quantities against the longdouble truth to n u kappa(K^) |value|.
"""
import numpy as np
import pytest

import gpr_reference as R

SIZES = [1, 2, 65, 129, 300]


@pytest.fixture(scope="module")
def cases():
    out = {}
    for n in SIZES:
        A = R.spd_matrix(n, seed=n)
        out[n] = (A, R.potrf(A))
    return out


@pytest.mark.parametrize("n", SIZES)
def test_factorisation_residual_mirror_and_logdet(cases, n):
    A, (F, logdet, info) = cases[n]
    assert info == 0
    assert np.array_equal(F, F.T)
    assert R.factor_residual_excess(A, F) <= 0
    ref = R.LD(R.logdet_ascending(F))
    assert abs(R.LD(logdet) - ref) <= n * R.U * abs(ref)
    Lnp = np.linalg.cholesky(A)
    assert R.factor_residual_excess(A, Lnp) <= 0
    # the factor itself against the truth: the bound's forward form through the condition number
    Lt = R.potrf_truth(A)
    kappa = np.linalg.cond(A)
    assert np.abs(np.tril(F) - Lt).max() <= 4 * n * float(R.U) * kappa * np.abs(Lt).max()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("nrhs", [1, 3, 65])
def test_solve_residuals(cases, n, nrhs):
    A, (F, _, _) = cases[n]
    L = np.tril(F)
    B = np.random.default_rng(100 * n + nrhs).standard_normal((nrhs, n))
    X = R.trsm(F, B, False)
    assert R.solve_residual_excess(L, X, B) <= 0
    Xt = R.trsm(F, B, True)
    assert R.solve_residual_excess(L.T, Xt, B) <= 0
    # numpy's factor with the same substitution stays inside the bound too
    Lnp = np.linalg.cholesky(A)
    Fnp = Lnp + np.tril(Lnp, -1).T
    assert R.solve_residual_excess(Lnp, R.trsm(Fnp, B, False), B) <= 0
    # the truth's own residual is far inside
    assert R.solve_residual_excess(L, R.trsm_truth(L, B, False), B) <= 0


def test_block_edge_does_not_change_the_contract():
    A = R.spd_matrix(37, seed=5)
    for nb in (1, 4, 16, 37, 128):
        F, logdet, info = R.potrf(A, nb=nb)
        assert info == 0 and R.factor_residual_excess(A, F) <= 0
        B = np.random.default_rng(nb).standard_normal((5, 37))
        assert R.solve_residual_excess(np.tril(F), R.trsm(F, B, False, nb=nb), B) <= 0
        assert R.solve_residual_excess(np.tril(F).T, R.trsm(F, B, True, nb=nb), B) <= 0


@pytest.mark.parametrize("n,k", [(5, 0), (5, 4), (140, 3), (140, 128), (140, 139)])
def test_not_positive_definite_sets_info(n, k):
    r = np.random.default_rng(n + k)
    L0 = np.tril(r.standard_normal((n, n))) + 3.0 * np.eye(n)
    A = L0 @ L0.T
    A = np.tril(A) + np.tril(A, -1).T
    A[k, k] -= L0[k, k] ** 2 + 1.0
    F, logdet, info = R.potrf(A)
    assert info == k + 1 and np.isnan(logdet)


def test_gpr_formulas_against_the_truth_and_finite_differences():
    r = np.random.default_rng(7)
    n, ns, p, noise = 40, 20, 2, 0.1
    Phi = r.standard_normal((n + ns, 30))
    Kall = Phi @ Phi.T
    K, Ksx, Kss = Kall[:n, :n], Kall[n:, :n], Kall[n:, n:]
    Y = r.standard_normal((n, p))
    got = R.gpr(K, noise, Y, Ksx, Kss)
    tru = R.gpr(K, noise, Y, Ksx, Kss, dtype=np.longdouble)
    kappa = np.linalg.cond(K + noise * np.eye(n))
    for name in ("lml", "dK", "dnoise", "mean", "var", "cov"):
        t = np.asarray(tru[name])
        err = np.abs(np.asarray(got[name], dtype=R.LD) - t).max()
        assert err <= n * float(R.U) * kappa * np.abs(t).max(), name
    # the formulas themselves: numpy's dense algebra
    Kh = K + noise * np.eye(n)
    a = np.linalg.solve(Kh, Y)
    lml = -0.5 * (Y * a).sum() - 0.5 * p * np.linalg.slogdet(Kh)[1] - 0.5 * n * p * np.log(2 * np.pi)
    assert abs(got["lml"] - lml) <= 1e-9 * abs(lml)
    assert np.allclose(got["mean"], Ksx @ a, rtol=1e-9, atol=1e-9)
    assert np.allclose(got["cov"], Kss - Ksx @ np.linalg.solve(Kh, Ksx.T), rtol=1e-8, atol=1e-8)
    assert np.allclose(got["var"], np.diag(got["cov"]), rtol=1e-9, atol=1e-9)
    # gradients by central differences on the longdouble value
    h = 1e-6
    d = (R.gpr(K, noise + h, Y, dtype=np.longdouble)["lml"] - R.gpr(K, noise - h, Y, dtype=np.longdouble)["lml"]) / (2 * h)
    assert abs(float(d) - got["dnoise"]) <= 1e-6 * abs(got["dnoise"])
    E = np.zeros((n, n))
    E[3, 7] = E[7, 3] = 1.0
    d = (R.gpr(K + h * E, noise, Y, dtype=np.longdouble)["lml"] - R.gpr(K - h * E, noise, Y, dtype=np.longdouble)["lml"]) / (2 * h)
    assert abs(float(d) - 2 * got["dK"][3, 7]) <= 1e-6 * abs(2 * got["dK"][3, 7])
