"""CPU: the numpy restatement of the exact posterior moments (tests/posterior_reference.py).

* Its solves are oracle/cg.py's linear_cg.  Run to the stall (tolerance 1e-12, max_iter >= n: linear_cg's
  ``p.Ap < 1e-10`` guard stops every normalised column at a relative residual near 1e-5) the chunked moments
  meet the dense truth (fp64 Phi Phi^T, Cholesky).  A solution that is off by delta puts the mean and the
  covariance's off-diagonal entries off by O(delta), but a variance by O(delta^2) only: b^T K^-1 b - b^T x_k is
  the squared energy norm of the error.
* Stopped early, the variances err on the safe side: from a zero start b^T x_k increases monotonically to
  b^T K^-1 b.
* Phi = f0 I has a closed form.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import mll_reference as M
import posterior_reference as R


def phi_system(N, seed, f=(1.0, -0.45, 0.2)):
    """Phi of three step matrices of a random graph (M_0 = I, M_l = W^l with W the degree-normalised adjacency,
    values rounded to fp32 like the preprocessor's): all N rows."""
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
    return M.phi_from_steps(mats, f)


def case(N, n_train, n_test, seed):
    """Sorted training nodes, test nodes that include training nodes and a repeat, targets."""
    r = np.random.default_rng(seed + 100)
    train = np.sort(r.permutation(N)[:n_train])
    test = r.integers(0, N, n_test)
    test[:3] = train[:3]
    test[5] = test[4]
    return train, test, r.standard_normal(n_train)


# (N, n_train, n_test, noise, seed): 257 and 300 test nodes cross a chunk boundary
CASES = [(200, 64, 65, 0.05, 1), (300, 96, 257, 0.3, 2), (400, 128, 300, 1.0, 3), (300, 128, 65, 0.05, 4)]

_truth = {}


def _case(N, n_train, n_test, noise, seed):
    key = (N, n_train, n_test, noise, seed)
    if key not in _truth:
        P = phi_system(N, seed)
        train, test, y = case(N, n_train, n_test, seed)
        _truth[key] = (P, train, test, y, R.dense_truth(P, train, test, y, noise))
    return _truth[key]


@pytest.mark.parametrize("N,n_train,n_test,noise,seed", CASES)
def test_stalled_solves_meet_the_dense_truth(N, n_train, n_test, noise, seed):
    """Measured here (max error relative to the largest prior variance), over the four cases:
      mean 1.6e-6 to 1.6e-5, var 1.8e-11 to 5.3e-11, cov 6.2e-7 to 1.4e-6
    -- linear_cg's stall floor (solutions ~1e-5 off), entering the variances squared.  The bounds asserted are
    those figures with two decades of margin for another BLAS's summation order."""
    P, train, test, y, tru = _case(N, n_train, n_test, noise, seed)
    est = R.moments(P, train, test, y, noise, tolerance=1e-12, max_iter=max(n_train, 48), full_cov=True)
    assert len(est["iters"]) == (n_test + 255) // 256
    e = R.errors(est, tru, full_cov=True)
    print(f"N={N} n={n_train} n*={n_test} s2={noise}: " + "  ".join(f"{q} {v:.2e}" for q, v in e.items()))
    assert e["mean"] <= 2e-3 and e["var"] <= 5e-9 and e["cov"] <= 2e-4
    assert np.array_equal(est["cov"], est["cov"].T)
    assert np.max(np.abs(np.diag(est["cov"]) - est["var"])) <= 5e-9 * tru["prior"].max()
    # repeated test nodes give repeated results; training nodes are ordinary test nodes
    assert est["var"][5] == est["var"][4] and est["mean"][5] == est["mean"][4]
    # without full_cov: the same mean and var
    plain = R.moments(P, train, test, y, noise, tolerance=1e-12, max_iter=max(n_train, 48))
    assert plain["cov"] is None and np.array_equal(plain["var"], est["var"]) and np.array_equal(plain["mean"], est["mean"])
    noisy = R.moments(P, train, test, y, noise, tolerance=1e-12, max_iter=max(n_train, 48), full_cov=True,
                      add_noise=True)
    assert np.array_equal(noisy["var"], est["var"] + noise)
    assert np.array_equal(np.diag(noisy["cov"]), np.diag(est["cov"]) + noise)


@pytest.mark.parametrize("N,n_train,n_test,noise,seed", CASES)
def test_a_stopped_solve_never_underestimates_a_variance(N, n_train, n_test, noise, seed):
    """tolerance = 1: linear_cg stops after its minimum of iterations (k = 10, the eleventh).  Measured on these
    cases: var - truth lies in [-1.2e-16, 5.9e-11] x prior."""
    P, train, test, y, tru = _case(N, n_train, n_test, noise, seed)
    est = R.moments(P, train, test, y, noise, tolerance=1.0)
    assert est["iters"] == [11] * len(est["iters"])
    assert np.all(est["var"] >= tru["var"] - 1e-12 * tru["prior"])
    # ... and a solve cut much shorter over-estimates visibly, still never under
    short = R.moments(P, train, test, y, noise, tolerance=1.0, max_iter=2)
    assert short["iters"] == [2] * len(short["iters"])
    assert np.all(short["var"] >= tru["var"] - 1e-12 * tru["prior"])
    assert np.max(short["var"] - tru["var"]) > 1e-6 * tru["prior"].max()
    assert np.all(short["var"] >= est["var"] - 1e-12 * tru["prior"])


@pytest.mark.parametrize("f0,noise", [(1.0, 0.1), (0.75, 2.0), (-1.5, 0.01)])
def test_identity_features_closed_form(f0, noise):
    """max_walk_length = 1: Phi = f0 I, K = f0^2 I."""
    N = 50
    P = sp.identity(N, format="csr") * f0
    train, test, y = case(N, 20, 70, 9)
    est = R.moments(P, train, test, y, noise, tolerance=1e-12, max_iter=48, full_cov=True)
    mean, var = R.identity_closed_form(f0, noise, train, test, y)
    assert np.max(np.abs(est["var"] - var)) <= 1e-14 * f0 * f0
    assert np.max(np.abs(est["mean"] - mean)) <= 1e-14 * np.max(np.abs(y))
    tru = R.dense_truth(P, train, test, y, noise)
    assert np.max(np.abs(tru["var"] - var)) <= 1e-14 * f0 * f0


def test_nlpd_is_the_gaussian_log_density():
    r = np.random.default_rng(0)
    y, m, s = r.standard_normal(9), r.standard_normal(9), r.uniform(0.5, 2.0, 9)
    from scipy.stats import norm
    assert abs(R.nlpd(y, m, s) - float(-np.mean(norm.logpdf(y, m, s)))) <= 1e-14
