"""CPU: the numpy restatement of the SVGP classification (tests/svgp_reference.py) against its truths.

1. RobustMax.prob_is_largest in fp64 against the mpmath truth on random rows and on the edge rows (mu = +-50, var in
   {0, 1e-12, 1e3}, the label first and last), P in {2, 3, 7, 64}, n_gh in {1, 20}: error <= 4 (P + n_gh) u max|p|
   (P - 1 factors of one erf, documented at no more than 2 ulp, and two roundings each; an n_gh-term sum).
   Measured: 1.9e-16 (P = 7, n_gh = 20, bound 1.2e-14), 5.2e-16 (P = 64).  The analytic gradients of the variational
   expectations (n_gh = 20, the same P) equal the torch expression's autograd within the same bound scaled by the
   gradient's magnitude, and every row's equal the mpmath formulas within it; the mpmath formulas themselves
   equal mpmath central differences.  "The gradient's magnitude" is read as the bound is stated for p, relative to
   the largest magnitude over the rows (max|p| there, max|gradient| here).  Measured, worst over P: restatement
   against autograd 0.056 of the bound, restatement against the truth 0.033, autograd against the truth 0.042.
   Relative to each ROW's own largest entry, which is stricter than the issue and is printed but not asserted, the
   restatement and autograd still differ by at most 1.37 x 4 (P + n_gh) u (dvar, P = 2), but both miss the truth by
   up to 29 x (P = 3, the rows with var = 1e3): there x_i = mu_y + gh_x[i] sqrt(2 var_y) reaches 290 and cancels
   against mu_c to a d_ic of order 1, so d_ic inherits an absolute error of 290 u / s_c, several hundred u, which
   the count of roundings behind 4 (P + n_gh) u does not contain.  It is the conditioning of GPflow's formula at
   those rows, the same for any fp64 evaluation of it (torch's autograd: 28 x), not an error of the restatement.
2. Gaussian likelihood at the analytic optimum: the restated ELBO equals the collapsed bound (np.longdouble) within
   N u kappa(Kmm) |value|, and any perturbation of m lowers it.
3. The restated Cholesky backward equals torch autograd of the torch expression.
"""
import mpmath
import numpy as np
import pytest

import svgp_reference as R

U = float(R.U)


def _rows(P, seed):
    mu, var, y = R.random_rows(12, P, seed)
    emu, evar, ey = R.edge_rows(P)
    return np.vstack([mu, emu]), np.vstack([var, evar]), np.concatenate([y, ey])


@pytest.mark.parametrize("n_gh", [1, 20])
@pytest.mark.parametrize("P", [2, 3, 7, 64])
def test_probability_against_mpmath(P, n_gh):
    gh_x, gh_w = R.hermgauss(n_gh)
    mu, var, y = _rows(P, 10 * P + n_gh)
    p = R.prob_is_largest(mu, var, y, gh_x, gh_w)
    truth = [R.prob_truth(mu[k], var[k], int(y[k]), gh_x, gh_w) for k in range(len(y))]
    err = max(abs(R.mp(p[k]) - truth[k]) for k in range(len(y)))
    scale = float(max(abs(t) for t in truth))
    bound = R.floor_p(P, n_gh, scale)
    print(f"P={P} n_gh={n_gh}: |p - truth| {float(err):.3e}, bound {bound:.3e} (max|p| {scale:.3e})")
    assert err <= bound
    ps = R.predict_probabilities(mu[:4], var[:4], gh_x, gh_w)
    for k in range(4 if P <= 7 else 1):
        t = R.predict_truth(mu[k], var[k], gh_x, gh_w)
        assert max(abs(R.mp(ps[k, c]) - t[c]) for c in range(P)) <= R.floor_p(P, n_gh, 1.0)
    if n_gh == 20:
        assert np.abs(ps.sum(axis=1) - 1.0).max() < 0.2   # (the quadrature's probabilities nearly sum to one)


@pytest.mark.parametrize("P", [2, 3, 7, 64])
def test_gradients_against_torch_autograd_and_mpmath(P):
    import torch
    n_gh = 20
    gh_x, gh_w = R.hermgauss(n_gh)
    mu, var, y = _rows(P, 77 + P)
    n = len(y)
    ve, dmu, dvar = R.variational_expectations(mu, var, y, gh_x, gh_w)
    tm = torch.tensor(mu, requires_grad=True)
    tv = torch.tensor(var, requires_grad=True)
    tve = R.ve_torch(torch, tm, tv, y, gh_x, gh_w)
    tve.sum().backward()
    dve = np.log(1.0 - R.EPSILON) - np.log(R.EPSILON / (P - 1))
    truths = [R.ve_truth(mu[k], var[k], int(y[k]), gh_x, gh_w) for k in range(n)]        # every row
    for j, (name, got, want) in enumerate((("ve", ve, tve.detach().numpy()), ("dmu", dmu, tm.grad.numpy()),
                                           ("dvar", dvar, tv.grad.numpy()))):
        # the issue's bound, as it is stated for p (relative to max|p| over the rows): 4 (P + n_gh) u times the
        # quantity's largest magnitude over the rows; for ve that of dve = d ve / d p (|p| <= 1)
        truth = [[t[0]] if j == 0 else t[j] for t in truths]
        mag = abs(dve) if j == 0 else float(max(abs(g) for t in truth for g in t))
        bound = R.floor_p(P, n_gh, mag)
        got2, want2 = got.reshape(n, -1), want.reshape(n, -1)
        diff = np.abs(got2 - want2).max()
        err = float(max(abs(R.mp(g) - t) for k in range(n) for g, t in zip(got2[k], truth[k])))
        err_torch = float(max(abs(R.mp(g) - t) for k in range(n) for g, t in zip(want2[k], truth[k])))
        # a figure only: the same errors relative to each row's own largest entry
        rowmag = np.array([max(float(max(abs(g) for g in truth[k])), 1e-300) for k in range(n)])
        row_err = np.array([float(max(abs(R.mp(g) - t) for g, t in zip(got2[k], truth[k]))) for k in range(n)])
        row_diff = np.abs(got2 - want2).max(axis=1)
        print(f"P={P} {name}: |restatement - autograd| {diff:.3e}, |restatement - truth| {err:.3e}, |autograd - truth| "
              f"{err_torch:.3e}, bound {bound:.3e} (magnitude {mag:.3e})")
        if j:
            print(f"    relative to each row's own magnitude, in units of 4 (P + n_gh) u: restatement - autograd "
                  f"{np.max(row_diff / R.floor_p(P, n_gh, rowmag)):.3g}, restatement - truth "
                  f"{np.max(row_err / R.floor_p(P, n_gh, rowmag)):.3g}")
        assert diff <= bound, name                 # against the torch expression's autograd
        assert err <= bound, name                  # every row against the mpmath formulas
    # a clipped variance gets gradient 0
    clipped = var < R.CLIP
    assert clipped.any() and np.all(dvar[clipped] == 0.0) and np.all(tv.grad.numpy()[clipped] == 0.0)
    if P == 64:                                    # (the central differences below: P <= 7 is enough)
        return
    h = mpmath.mpf(10) ** -15
    for k in (0, 1):
        _, tdmu, tdvar = R.ve_truth(mu[k], var[k], int(y[k]), gh_x, gh_w)
        for c in range(P):
            for which, grad in (("mu", tdmu), ("var", tdvar)):
                lo, hi = [[R.mp(v) for v in mu[k]], [R.mp(v) for v in var[k]]], None
                hi = [list(lo[0]), list(lo[1])]
                j = 0 if which == "mu" else 1
                lo[j][c] -= h
                hi[j][c] += h
                fd = (R.ve_truth(hi[0], hi[1], int(y[k]), gh_x, gh_w)[0]
                      - R.ve_truth(lo[0], lo[1], int(y[k]), gh_x, gh_w)[0]) / (2 * h)
                assert abs(fd - grad[c]) <= mpmath.mpf(10) ** -20 * (1 + abs(grad[c])), (k, c, which)


def _problem(N=40, M=17, P=2, seed=4):
    r = np.random.default_rng(seed)
    Phi = r.standard_normal((N, 30)) / np.sqrt(30)
    K = Phi @ Phi.T + 0.05 * np.eye(N)
    K = np.tril(K) + np.tril(K, -1).T
    z = np.sort(r.permutation(N)[:M])
    return K, z, r.standard_normal((N, P)), r


def test_gaussian_elbo_at_the_optimum_is_the_collapsed_bound():
    N, M, P, s2, jitter = 40, 17, 2, 0.1, 1e-6
    K, z, Y, r = _problem(N, M, P)
    Kmm, Knm, Knn = K[np.ix_(z, z)], K[:, z], np.diag(K).copy()
    m, Ls = R.gaussian_optimum(Kmm, Knm, Y, s2, jitter)
    q_mu, q_sqrt = np.asarray(m, np.float64), np.asarray(Ls, np.float64)
    want = R.collapsed_bound(Kmm, Knm, Knn, Y, s2, jitter)
    got = R.elbo_gaussian(Kmm, Knm, Knn, q_mu, q_sqrt, Y, s2, jitter)
    ev = np.linalg.eigvalsh(Kmm + jitter * np.eye(M))
    kappa = ev[-1] / ev[0]
    bound = N * U * kappa * abs(float(want))
    print(f"ELBO {got:.6f}, collapsed bound {float(want):.6f}, |diff| {abs(float(R.LD(got) - want)):.3e}, "
          f"bound {bound:.3e} (kappa {kappa:.3e})")
    assert abs(float(R.LD(got) - want)) <= bound
    # the longdouble ELBO at the longdouble optimum agrees far below the fp64 bound
    assert abs(float(R.elbo_gaussian(Kmm, Knm, Knn, m, Ls, Y, s2, jitter, dtype=R.LD) - want)) <= 1e-3 * bound
    # any perturbation of m gives a smaller value
    for k in range(5):
        dm = r.standard_normal(q_mu.shape) * 10.0 ** (-k)
        assert R.elbo_gaussian(Kmm, Knm, Knn, q_mu + dm, q_sqrt, Y, s2, jitter) < got
    # the minibatch scale multiplies the expectation term and not the KL
    kl = R.gauss_kl(q_mu, q_sqrt)
    scaled = R.elbo_gaussian(Kmm, Knm, Knn, q_mu, q_sqrt, Y, s2, jitter, scale=4.0)
    assert abs(scaled - (4.0 * (got + kl) - kl)) <= 1e-9 * abs(scaled)


def test_cholesky_backward_equals_torch_autograd():
    import torch
    N, M, P, jitter = 40, 17, 3, 1e-6
    K, z, _, r = _problem(N, M, P, seed=8)
    y = r.integers(0, P, N)
    q_mu = r.standard_normal((M, P))
    q_sqrt = np.tril(r.standard_normal((P, M, M)) * 0.2) + np.eye(M)[None]
    Kmm = torch.tensor(K[np.ix_(z, z)], requires_grad=True)
    Knm = torch.tensor(K[:, z], requires_grad=True)
    Knn = torch.tensor(np.diag(K).copy())
    elbo = R.elbo_torch(torch, Kmm, Knm, Knn, torch.tensor(q_mu), torch.tensor(q_sqrt), y, jitter)
    elbo.backward()
    # the restatement: dL/dAT from the likelihood's analytic gradients, then the Cholesky backward
    Lm, AT = R.whitened_A(K[np.ix_(z, z)], K[:, z], jitter)
    fmean, fvar = R.conditional(AT, np.diag(K), q_mu, q_sqrt)
    gh_x, gh_w = R.hermgauss()
    ve, gmu, gvar = R.variational_expectations(fmean, fvar, y, gh_x, gh_w)
    assert abs(ve.sum() - R.gauss_kl(q_mu, q_sqrt) - elbo.item()) <= 1e-12 * abs(elbo.item())
    Lq = np.tril(q_sqrt)
    ATbar = gmu @ q_mu.T - 2.0 * gvar.sum(axis=1)[:, None] * AT
    for p in range(P):
        ATbar += (2.0 * gvar[:, p, None] * (AT @ Lq[p])) @ Lq[p].T
    Knm_bar, Kmm_bar = R.cholesky_backward(Lm, AT, ATbar)
    ev = np.linalg.eigvalsh(K[np.ix_(z, z)] + jitter * np.eye(M))
    kappa = ev[-1] / ev[0]
    for name, got, want in (("Knm", Knm_bar, Knm.grad.numpy()), ("Kmm", Kmm_bar, Kmm.grad.numpy())):
        err, scale = np.abs(got - want).max(), np.abs(want).max()
        print(f"d/d{name}: |restatement - autograd| {err:.3e}, bound {2 * M * U * kappa * scale:.3e}")
        assert err <= 2 * M * U * kappa * scale, name
    assert np.array_equal(Kmm_bar, Kmm_bar.T)
