"""CPU: the numpy restatement of the matrix-free marginal likelihood (tests/mll_reference.py).

* Its CG is oracle/cg.py's linear_cg with the coefficients recorded: same solutions, same counts.
* With identity probes Z = sqrt(n) I the Hutchinson traces are exact and stochastic Lanczos
  quadrature is exact once Lanczos has run out, so the restatement must meet the dense truth
  (Cholesky log det, K^-1, exact traces).  What is left is linear_cg's own floor: its
  ``p.Ap < 1e-10`` guard stops every (normalised) column at a relative residual near 1e-5, after 4 to
  9 iterations on these systems (condition numbers below 40; an isolated training node's column after
  one), which is why max_iter = 48 lets every column reach its stall.  The solutions are then off by
  ~1e-5 relative.  Measured against the truth on the four cases below: log det 1.4e-12 to 2.0e-11
  relative (a Gauss quadrature, exact to twice the Krylov depth), value 8.6e-14 to 1.2e-11, noise
  gradient 2.1e-11 to 3.5e-9, modulator gradient 3.5e-8 to 2.9e-7 (set by the guard, not by rounding).
  The bounds asserted are those figures with a margin for another BLAS's summation order.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import mll_reference as R
from oracle import cg as OCG


def system(N, n_train, noise, seed, f=(1.0, -0.45, 0.2)):
    """Three step matrices of a random graph (M_0 = I, M_l = W^l with W the degree-normalised
    adjacency, values rounded to fp32 like the preprocessor's), Phi_T, the M_l[T], y."""
    r = np.random.default_rng(seed)
    m = 3 * N
    u, v = r.integers(0, N, m), r.integers(0, N, m)
    keep = u != v
    A = sp.coo_matrix((np.ones(keep.sum()), (u[keep], v[keep])), shape=(N, N)).tocsr()
    A = (A + A.T).tocsr()
    A.data[:] = 1.0
    d = np.maximum(np.asarray(A.sum(1)).ravel(), 1.0)
    W = sp.diags(1.0 / np.sqrt(d)) @ A @ sp.diags(1.0 / np.sqrt(d))
    mats = [sp.identity(N, format="csr")]
    for _ in range(len(f) - 1):
        mats.append(sp.csr_matrix((mats[-1] @ W).astype(np.float32).astype(np.float64)))
    T = np.sort(r.permutation(N)[:n_train])
    phi = R.phi_from_steps(mats, f)
    y = r.standard_normal(n_train)
    return phi[T], [M[T] for M in mats], y, noise


CASES = [(200, 64, 0.05, 1), (300, 96, 0.3, 2), (400, 128, 1.0, 3), (300, 128, 0.05, 4)]


def test_cg_lanczos_is_linear_cg():
    Pt, Ms, y, noise = system(300, 96, 0.3, 7)
    mm = R._khat_matmul(Pt, noise)
    B = np.random.default_rng(0).standard_normal((96, 7))
    B[:, 3] = 0.0
    for tol, mi in ((1.0, 1000), (1e-2, 1000), (1e-12, 48), (1.0, 3)):
        X, k, al, be = R.cg_lanczos(mm, B, tolerance=tol, max_iter=mi)
        Xo, ko = OCG.linear_cg(mm, B, tolerance=tol, max_iter=mi)
        assert k == ko and np.array_equal(X, Xo)
        assert not al[k:].any() and not be[k:].any() and al[0, [0, 1, 2, 4, 5, 6]].all()
        assert not al[:, 3].any()                       # the zero column never moves


def test_tridiagonal_is_lanczos_of_khat():
    """The CG coefficients' tridiagonal is the Lanczos matrix of K^ started at z / ||z||: its
    eigenvalues lie in K^'s spectrum and e1^T T e1 = z^T K^ z / z^T z."""
    Pt, Ms, y, noise = system(200, 64, 0.3, 5)
    K = (Pt @ Pt.T).toarray() + noise * np.eye(64)
    z = np.random.default_rng(1).standard_normal((64, 1))
    _, k, al, be = R.cg_lanczos(lambda v: K @ v, z, tolerance=1e-12, max_iter=6)
    T = R.tridiagonal(al[:, 0], be[:, 0], k)
    assert T.shape == (6, 6)
    np.testing.assert_allclose(T[0, 0], (z.T @ K @ z).item() / (z.T @ z).item(), rtol=1e-12)
    lam, lamK = np.linalg.eigvalsh(T), np.linalg.eigvalsh(K)
    assert lamK[0] * (1 - 1e-12) <= lam[0] and lam[-1] <= lamK[-1] * (1 + 1e-12)


@pytest.mark.parametrize("N,n_train,noise,seed", CASES)
def test_identity_probes_meet_the_dense_truth(N, n_train, noise, seed):
    Pt, Ms, y, s2 = system(N, n_train, noise, seed)
    K = (Pt @ Pt.T).toarray() + s2 * np.eye(n_train)
    assert np.linalg.cond(K) < 40
    est = R.estimate(Pt, Ms, y, s2, R.identity_probes(n_train), tolerance=1e-12, max_iter=48)
    tru = R.dense_truth(Pt, Ms, y, s2)
    # every column has stalled (alpha = 0) well before max_iter (an isolated training node's e_i is an
    # eigenvector of K^: its column is solved, and its Lanczos run out, after one iteration)
    stall = [R.lanczos_length(est["alpha"][:, c], est["iters"]) for c in range(1 + n_train)]
    assert est["iters"] == 48 and 1 <= min(stall) and max(stall) <= 30
    rel = lambda a, b: np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(np.asarray(b)))
    e_logdet = rel(est["logdet"], tru["logdet"])
    e_value = rel(est["value"], tru["value"])
    e_f = rel(est["grad_f"], tru["grad_f"])
    e_noise = rel(est["grad_noise"], tru["grad_noise"])
    print(f"N={N} n={n_train} s2={s2}: stall {min(stall)}..{max(stall)} logdet {e_logdet:.2e} value {e_value:.2e} "
          f"grad_f {e_f:.2e} grad_noise {e_noise:.2e}")
    assert e_logdet <= 1e-9
    assert e_value <= 1e-9
    assert e_f <= 1e-5
    assert e_noise <= 1e-7


def test_random_probes_estimate_the_truth():
    """t = 64 Gaussian probes: an unbiased estimate -- within a few of its own standard errors."""
    Pt, Ms, y, s2 = system(300, 96, 0.3, 2)
    Z = np.random.default_rng(9).standard_normal((96, 64))
    est = R.estimate(Pt, Ms, y, s2, Z, tolerance=1e-12, max_iter=48)
    tru = R.dense_truth(Pt, Ms, y, s2)
    assert abs(est["logdet"] - tru["logdet"]) <= 0.05 * abs(tru["logdet"]) + 2.0
    assert np.all(np.abs(est["grad_f"] - tru["grad_f"]) <= 0.25 * np.abs(tru["grad_f"]).max() + 1.0)


def test_engine_host_quadrature_is_the_restatements():
    """GRFEngine.slq_logdet (the product's host step: tridiagonals + eigh) on the restatement's coefficients."""
    from grf_amd.engine import GRFEngine
    Pt, Ms, y, s2 = system(300, 96, 0.3, 2)
    Z = np.random.default_rng(3).standard_normal((96, 9))
    Z[:, 4] = 0.0                                       # a zero probe: m_c = 0, contributes nothing
    for tol, mi in ((1e-12, 48), (1e-2, 1000), (1.0, 3)):
        est = R.estimate(Pt, Ms, y, s2, Z, tolerance=tol, max_iter=mi)
        coef = np.concatenate([est["alpha"][:, 1:], est["beta"][:, 1:]], axis=0)
        got = GRFEngine.slq_logdet(coef, est["iters"], np.sum(Z * Z, axis=0))
        assert abs(got - est["logdet"]) <= 1e-13 * abs(est["logdet"])
