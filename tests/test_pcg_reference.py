"""CPU: the numpy restatement of the diagonally preconditioned linear_cg (tests/pcg_reference.py).

* With dinv = 1 it is oracle/cg.py's linear_cg bit for bit (solutions, counts) and mll_reference's
  coefficients.
* Run to its floor it meets numpy.linalg.solve (the bound of tests/test_cg_oracle.py).
* The preconditioned MLL restatement with exact probes g = sqrt(n) I meets the dense truth at the
  tolerances of tests/test_mll_reference.py: D^1/2 g spans the space, E[z z^T] = D exactly, and every
  column's Lanczos of D^-1/2 K^ D^-1/2 runs out.
* On the golden Cora features the Jacobi count is at most half the plain count.
"""
import numpy as np
import pytest

import mll_reference as R
import pcg_reference as P
from oracle import cg as OCG
from test_cg_oracle import _spd
from test_mll_reference import CASES, system


def test_unit_diagonal_is_linear_cg():
    Pt, Ms, y, noise = system(300, 96, 0.3, 7)
    mm = R._khat_matmul(Pt, noise)
    B = np.random.default_rng(0).standard_normal((96, 7))
    B[:, 3] = 0.0
    one = np.ones(96)
    for tol, mi in ((1.0, 1000), (1e-2, 1000), (1e-12, 48), (1.0, 3), (1.0, 1)):
        X, k, al, be, _ = P.pcg_lanczos(mm, B, one, tolerance=tol, max_iter=mi)
        Xo, ko = OCG.linear_cg(mm, B, tolerance=tol, max_iter=mi)
        assert k == ko and np.array_equal(X, Xo)
        _, kr, alr, ber = R.cg_lanczos(mm, B, tolerance=tol, max_iter=mi)
        assert kr == k and np.array_equal(al, alr) and np.array_equal(be, ber)
    Z, k, _, _, res = P.pcg_lanczos(mm, np.zeros((96, 2)), one)
    assert k == 0 and not Z.any() and not res.any()


def test_converges_to_solve():
    phi, A, r = _spd(60, 1)
    B = r.standard_normal((60, 5))
    dinv = 1.0 / np.diag(A)
    X, k, _, _, _ = P.pcg_lanczos(lambda v: A @ v, B, dinv, tolerance=1e-12, max_iter=1000)
    want = np.linalg.solve(A, B)
    assert np.linalg.norm(A @ X - B, axis=0).max() <= 1e-4 * np.linalg.norm(B, axis=0).min()
    np.testing.assert_allclose(X, want, rtol=2e-3, atol=1e-4 * np.abs(want).max())
    assert k == 1000                                  # linear_cg's stall floor (~1e-5) never meets 1e-12


def test_first_iterates_are_textbook_pcg():
    phi, A, r = _spd(50, 4)
    B = r.standard_normal((50, 3))
    dinv = r.uniform(0.2, 5.0, 50)
    X, k, _, _, _ = P.pcg_lanczos(lambda v: A @ v, B, dinv, max_iter=6)
    assert k == 6
    for c in range(3):
        x, res = np.zeros(50), B[:, c].copy()
        z = dinv * res
        p, rz = z.copy(), res @ z
        for _ in range(6):
            ap = A @ p
            a = rz / (p @ ap)
            x, res = x + a * p, res - a * ap
            z = dinv * res
            rz_new = res @ z
            p, rz = z + (rz_new / rz) * p, rz_new
        np.testing.assert_allclose(X[:, c], x, rtol=1e-10, atol=1e-12)


def test_jacobi_dinv_order_and_guards():
    import scipy.sparse as sp
    rows = [[0.5, -3.0, 1e-4], [], [2.0]]
    phi = sp.csr_matrix((np.array([v for r in rows for v in r], np.float32), np.array([0, 2, 3, 1], np.int32),
                         np.array([0, 3, 3, 4])), shape=(3, 4))
    d = P.jacobi_dinv(phi, 0.0, rows=[2, 1, 0, 0])
    assert d[1] == 1.0 and d[0] == 0.25 and d[2] == d[3]
    v = np.float32(rows[0]).astype(np.float64)
    assert d[2] == 1.0 / (((0.0 + v[0] * v[0]) + v[1] * v[1]) + v[2] * v[2])
    assert P.jacobi_dinv(phi, 0.5)[1] == 2.0


@pytest.mark.parametrize("N,n_train,noise,seed", CASES)
def test_identity_probes_meet_the_dense_truth(N, n_train, noise, seed):
    Pt, Ms, y, s2 = system(N, n_train, noise, seed)
    est = P.estimate(Pt, Ms, y, s2, R.identity_probes(n_train), tolerance=1e-12, max_iter=48)
    tru = R.dense_truth(Pt, Ms, y, s2)
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


@pytest.mark.parametrize("N,n_train,noise,seed", CASES)
def test_noise_gradient_needs_the_second_order_form(N, n_train, noise, seed):
    """a_k.a_k alone is of first order in the preconditioned iterate's error (measured against the dense truth's
    a.a: 1.5e-8, 3.4e-9, 5.9e-9, 5.8e-8, which put the noise gradient up to 3.7e-7 off); a_k.a_k + 2 w.r_k is of
    second order (2.4e-10, 6.5e-11, 1.4e-11, 1.3e-10; noise gradient at most 1.7e-9 off).  Held here: the corrected
    form is at least ten times closer on every case."""
    Pt, Ms, y, s2 = system(N, n_train, noise, seed)
    est = P.estimate(Pt, Ms, y, s2, R.identity_probes(n_train), tolerance=1e-12, max_iter=48)
    K = (Pt @ Pt.T).toarray() + s2 * np.eye(n_train)
    at = np.linalg.solve(K, y)
    a = est["X"][:, 0]
    t = len(y)
    U, V = est["X"][:, 1:], R.identity_probes(n_train) * np.sqrt(1.0 / np.diag(K))[:, None]
    aa = 2.0 * (est["grad_noise"] + 0.5 / t * float(np.sum(U * V)))
    e_plain, e_corr = abs(a @ a - at @ at) / (at @ at), abs(aa - at @ at) / (at @ at)
    print(f"N={N} n={n_train} s2={s2}: a.a error, a_k.a_k {e_plain:.2e}, corrected {e_corr:.2e}")
    assert 10.0 * e_corr <= e_plain


def test_jacobi_halves_the_iterations_on_cora(golden):
    """Golden Cora m16 Phi (4 steps, f_l = (-1)^l / (2^l l!)), all 2708 rows, noise 0.01, tolerance 1e-2, 8
    Gaussian columns from default_rng(0): a condition on the restatement alone.  Measured with these columns: plain 60, Jacobi 21."""
    phi = P.cora_phi(golden)
    n = phi.shape[0]
    assert n == 2708
    mm = R._khat_matmul(phi, 0.01)
    B = np.random.default_rng(0).standard_normal((n, 8))
    _, k_plain = OCG.linear_cg(mm, B, tolerance=1e-2)
    X, k_jac, _, _, res = P.pcg_lanczos(mm, B, P.jacobi_dinv(phi, 0.01), tolerance=1e-2)
    print(f"cora: plain {k_plain} iterations, jacobi {k_jac}")
    assert res.mean() < 1e-2
    assert 2 * k_jac <= k_plain
