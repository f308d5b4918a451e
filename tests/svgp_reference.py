"""numpy restatement of the sparse variational GP classification of include/grf_svgp.h and
efficient_graph_gp.models.SVGP: GPflow's RobustMax.prob_is_largest, MultiClass._variational_expectations with its
analytic gradients, the predictive class probabilities, the whitened conditional (base_conditional), gauss_kl, the
ELBO and the backward of the Cholesky factor.

Three levels:
  * the fp64 restatement follows the library's order rule (products over c in ascending c from 1 with the label's
    factor 1; sums over the quadrature nodes as the pairwise tree over the next power of two of lanes; the
    leave-one-out product as the full product divided by C_ic);
  * everything that passes through erf has an mpmath truth at 40 digits, evaluated from the same fp64 inputs; the linear algebra takes a ``dtype`` switch and is a
    truth in np.longdouble (tests/gpr_reference.py's potrf_truth / trsm_truth);
  * the same ELBO as a plain torch expression (torch.linalg.cholesky, solve_triangular, torch.special.erf), an
    autograd reference for the gradients.
"""
import mpmath
import numpy as np
import scipy.linalg
import scipy.special

import gpr_reference as G

U, LD = G.U, G.LD
CLIP = 1e-10
CDF_SCALE, CDF_SHIFT = 1.0 - 2e-4, 1e-4
EPSILON = 1e-3
N_GH = 20
mpmath.mp.dps = 40


def hermgauss(n_gh=N_GH):
    return np.polynomial.hermite.hermgauss(n_gh)


# ------------------------------------------------------------------ the fp64 restatement of the likelihood
def tree_sum(v):
    """The pairwise tree over the last axis, padded with zeros to a power of two."""
    v = np.asarray(v, dtype=np.float64)
    g = 1
    while g < v.shape[-1]:
        g *= 2
    pad = np.zeros(v.shape[:-1] + (g - v.shape[-1],))
    v = np.concatenate([v, pad], axis=-1)
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def _clip(v):
    return np.where(v < CLIP, CLIP, v)


def _cdf(d):
    return (0.5 * (1.0 + scipy.special.erf(d / np.sqrt(2.0)))) * CDF_SCALE + CDF_SHIFT


def _nodes(mu, var, y, gh_x):
    rows = np.arange(mu.shape[0])
    sx = np.sqrt(_clip(2.0 * var[rows, y]))
    return mu[rows, y][:, None] + gh_x[None, :] * sx[:, None], sx


def _product(mu, var, y, x):
    prod = np.ones_like(x)
    for c in range(mu.shape[1]):
        C = _cdf((x - mu[:, c, None]) / np.sqrt(_clip(var[:, c]))[:, None])
        prod = prod * np.where((y == c)[:, None], 1.0, C)
    return prod


def prob_is_largest(mu, var, y, gh_x, gh_w):
    """p (n,) of RobustMax.prob_is_largest in fp64, in the library's order."""
    mu, var, y = np.asarray(mu, np.float64), np.asarray(var, np.float64), np.asarray(y)
    x, _ = _nodes(mu, var, y, gh_x)
    return tree_sum(_product(mu, var, y, x) * (gh_w / np.sqrt(np.pi))[None, :])


def variational_expectations(mu, var, y, gh_x, gh_w, epsilon=EPSILON):
    """(ve (n,), dve/dmu (n, P), dve/dvar (n, P)) in fp64, in the library's order."""
    mu, var, y = np.asarray(mu, np.float64), np.asarray(var, np.float64), np.asarray(y)
    n, P = mu.shape
    rows = np.arange(n)
    w = (gh_w / np.sqrt(np.pi))[None, :]
    x, sx = _nodes(mu, var, y, gh_x)
    prod = _product(mu, var, y, x)
    p = tree_sum(prod * w)
    log_hit, log_miss = np.log(1.0 - epsilon), np.log(epsilon / (P - 1))
    ve = p * log_hit + (1.0 - p) * log_miss
    dve = log_hit - log_miss
    dmu, dvar = np.zeros((n, P)), np.zeros((n, P))
    own, sum_mu = np.zeros_like(x), np.zeros(n)
    for c in range(P):
        vc = var[:, c]
        s = np.sqrt(_clip(vc))[:, None]
        d = (x - mu[:, c, None]) / s
        t = w * (prod / _cdf(d)) * CDF_SCALE * (np.exp(-0.5 * (d * d)) / np.sqrt(2.0 * np.pi))
        other = (y != c)
        ts = t / s
        g_mu = -tree_sum(np.where(other[:, None], ts, 0.0))
        td = tree_sum(np.where(other[:, None], t * d, 0.0))
        with np.errstate(divide="ignore", invalid="ignore"):
            g_var = np.where(vc < CLIP, 0.0, -td / (2.0 * vc))
        own = own + np.where(other[:, None], ts, 0.0)
        sum_mu = sum_mu + np.where(other, g_mu, 0.0)
        dmu[:, c] = np.where(other, dve * g_mu, 0.0)
        dvar[:, c] = np.where(other, dve * g_var, 0.0)
    up = tree_sum(own * gh_x[None, :] / sx[:, None])
    dmu[rows, y] = dve * (-sum_mu)
    dvar[rows, y] = dve * np.where(2.0 * var[rows, y] < CLIP, 0.0, up)
    return ve, dmu, dvar


def predict_probabilities(mu, var, gh_x, gh_w, epsilon=EPSILON):
    """ps (n, P) of MultiClass._predict_mean_and_var in fp64."""
    mu = np.asarray(mu, np.float64)
    n, P = mu.shape
    ps = np.empty((n, P))
    for c in range(P):
        p = prob_is_largest(mu, var, np.full(n, c), gh_x, gh_w)
        ps[:, c] = p * (1.0 - epsilon) + (1.0 - p) * (epsilon / (P - 1))
    return ps


def rows_sqsum(T, groups, base=None):
    """grf_rows_sqsum_f64 in its order: lane l of 64 chains RN(t t) over j = l, l + 64, ... ascending, the
    pairwise tree over the lanes, then base[r] + the sum.  No transcendental: the library's bits."""
    T = np.asarray(T, np.float64)
    n, length = T.shape[0], T.shape[1] // groups
    k = -(-max(length, 1) // 64)
    out = np.empty((n, groups))
    for g in range(groups):
        seg = np.zeros((n, k * 64))
        seg[:, :length] = T[:, g * length:(g + 1) * length]
        seg = seg.reshape(n, k, 64)
        s = np.zeros((n, 64))
        for q in range(k):
            s = s + seg[:, q] * seg[:, q]
        out[:, g] = tree_sum(s)
    return out if base is None else np.asarray(base, np.float64)[:, None] + out


# ------------------------------------------------------------------ the mpmath truth of the likelihood
def mp(x):
    """An fp64 or np.longdouble number as an exact mpf."""
    if isinstance(x, mpmath.mpf):
        return x
    hi = float(x)
    if not np.isfinite(hi):
        return mpmath.mpf(hi)
    return mpmath.mpf(hi) + mpmath.mpf(float(x - LD(hi)))


def _mp_cdf(d):
    return mpmath.mpf(CDF_SCALE) * (1 + mpmath.erf(d / mpmath.sqrt(2))) / 2 + mpmath.mpf(CDF_SHIFT)


def _mp_row(mu, var, y, gh_x, gh_w):
    P = len(mu)
    mu, var = [mp(v) for v in mu], [mp(v) for v in var]
    clip = mpmath.mpf(CLIP)
    s = [mpmath.sqrt(max(v, clip)) for v in var]
    sx = mpmath.sqrt(max(2 * var[y], clip))
    w = [mp(v) / mpmath.sqrt(mpmath.pi) for v in gh_w]
    x = [mu[y] + mp(g) * sx for g in gh_x]
    d = [[(xi - mu[c]) / s[c] for c in range(P)] for xi in x]
    return mu, var, s, sx, w, x, d


def prob_truth(mu, var, y, gh_x, gh_w):
    """p of one row (mu, var: length P) as an mpf."""
    _, _, _, _, w, x, d = _mp_row(mu, var, y, gh_x, gh_w)
    total = mpmath.mpf(0)
    for i in range(len(x)):
        prod = mpmath.mpf(1)
        for c in range(len(mu)):
            if c != y:
                prod *= _mp_cdf(d[i][c])
        total += w[i] * prod
    return total


def ve_truth(mu, var, y, gh_x, gh_w, epsilon=EPSILON):
    """(ve, dve/dmu [P], dve/dvar [P]) of one row as mpf numbers: the formulas of include/grf_svgp.h."""
    P = len(mu)
    mu_, var_, s, sx, w, x, d = _mp_row(mu, var, y, gh_x, gh_w)
    clip = mpmath.mpf(CLIP)
    others = [c for c in range(P) if c != y]
    p = mpmath.mpf(0)
    dmu, dvar = [mpmath.mpf(0)] * P, [mpmath.mpf(0)] * P
    up = mpmath.mpf(0)
    for i in range(len(x)):
        C = [_mp_cdf(d[i][c]) for c in range(P)]
        prod = mpmath.mpf(1)
        for c in others:
            prod *= C[c]
        p += w[i] * prod
        for c in others:
            loo = prod / C[c]                      # (C >= 1e-4: at 40 digits the quotient is the product without c)
            t = w[i] * loo * mpmath.mpf(CDF_SCALE) * mpmath.exp(-d[i][c] ** 2 / 2) / mpmath.sqrt(2 * mpmath.pi)
            dmu[c] -= t / s[c]
            if var_[c] >= clip:
                dvar[c] -= t * d[i][c] / (2 * var_[c])
            up += (t / s[c]) * mp(gh_x[i]) / sx
    dmu[y] = -sum(dmu[c] for c in others)
    dvar[y] = up if 2 * var_[y] >= clip else mpmath.mpf(0)
    eps = mp(epsilon)
    log_hit, log_miss = mpmath.log(1 - eps), mpmath.log(eps / (P - 1))
    ve = p * log_hit + (1 - p) * log_miss
    dve = log_hit - log_miss
    return ve, [dve * g for g in dmu], [dve * g for g in dvar]


def predict_truth(mu, var, gh_x, gh_w, epsilon=EPSILON):
    """ps [P] of one row as mpf numbers."""
    P = len(mu)
    eps = mp(epsilon)
    out = []
    for c in range(P):
        p = prob_truth(mu, var, c, gh_x, gh_w)
        out.append(p * (1 - eps) + (1 - p) * eps / (P - 1))
    return out


def floor_p(P, n_gh, scale):
    """The rounding floor of the quadrature: P - 1 factors of one erf (at most 2 ulp) and two roundings each, and
    an n_gh-term sum: 4 (P + n_gh) u |value|."""
    return 4 * (P + n_gh) * float(U) * scale


def edge_rows(P):
    """mu = +-50, var in {0, 1e-12, 1e3}, the label first and last: (mu, var, y)."""
    mus, vs, ys = [], [], []
    for k, (m0, v0) in enumerate([(50.0, 0.0), (-50.0, 0.0), (50.0, 1e-12), (-50.0, 1e-12), (50.0, 1e3),
                                  (-50.0, 1e3)]):
        for y in (0, P - 1):
            for where in ("label", "other", "all"):
                mu = np.linspace(-1.0, 1.0, P) * 0.5
                var = np.full(P, 0.7)
                idx = {"label": [y], "other": [(y + 1) % P], "all": list(range(P))}[where]
                for j in idx:
                    mu[j] = m0 if where != "all" else m0 + 0.25 * j
                    var[j] = v0
                mus.append(mu), vs.append(var), ys.append(y)
    return np.array(mus), np.array(vs), np.array(ys, dtype=np.int32)


def random_rows(n, P, seed):
    r = np.random.default_rng(seed)
    mu = r.standard_normal((n, P)) * 1.5
    var = np.exp(r.standard_normal((n, P)))
    return mu, var, r.integers(0, P, n).astype(np.int32)


# ------------------------------------------------------------------ the whitened conditional, the KL, the ELBO
def _dt(dtype):
    return LD if dtype in (LD, np.longdouble) else np.float64


def whitened_A(Kmm, Knm, jitter, dtype=np.float64):
    """(Lm, AT): the lower factor of Kmm + jitter I and AT (N x M) whose row n is Lm^-1 k_n."""
    dt = _dt(dtype)
    Kh = np.asarray(Kmm, dtype=dt) + dt(jitter) * np.eye(Kmm.shape[0], dtype=dt)
    if dt is LD:
        L = G.potrf_truth(Kh)
        return L, G.trsm_truth(L, np.asarray(Knm, dtype=dt), False)
    F, _, info = G.potrf(Kh)
    assert info == 0
    return np.tril(F), G.trsm(F, Knm, False)


def conditional(AT, Knn, q_mu, q_sqrt, dtype=np.float64):
    """(fmean, fvar), both N x P, of GPflow's whitened base_conditional with a full q_sqrt (P x M x M, lower)."""
    dt = _dt(dtype)
    AT, Knn, q_mu = np.asarray(AT, dtype=dt), np.asarray(Knn, dtype=dt), np.asarray(q_mu, dtype=dt)
    Lq = np.tril(np.asarray(q_sqrt, dtype=dt))
    fmean = AT @ q_mu
    base = Knn - (AT * AT).sum(axis=1)
    fvar = np.stack([base + ((AT @ Lq[p]) ** 2).sum(axis=1) for p in range(Lq.shape[0])], axis=1)
    return fmean, fvar


def gauss_kl(q_mu, q_sqrt, dtype=np.float64):
    """KL(q(v) || N(0, I)) summed over the P latents (gauss_kl with K = None)."""
    dt = _dt(dtype)
    q_mu, Lq = np.asarray(q_mu, dtype=dt), np.tril(np.asarray(q_sqrt, dtype=dt))
    P, M = Lq.shape[0], Lq.shape[1]
    logdet = sum(np.log(np.diag(Lq[p]) ** 2).sum() for p in range(P))
    return dt(0.5) * ((q_mu * q_mu).sum() - dt(P * M) - logdet + (Lq * Lq).sum())


def gaussian_ve(Y, fmean, fvar, s2, dtype=np.float64):
    dt = _dt(dtype)
    Y, s2 = np.asarray(Y, dtype=dt), dt(s2)
    two_pi = dt(8) * np.arctan(dt(1))
    return (-dt(0.5) * np.log(two_pi * s2) - dt(0.5) * ((Y - fmean) ** 2 + fvar) / s2).sum(axis=1)


def elbo_gaussian(Kmm, Knm, Knn, q_mu, q_sqrt, Y, s2, jitter, scale=1.0, dtype=np.float64):
    dt = _dt(dtype)
    _, AT = whitened_A(Kmm, Knm, jitter, dt)
    fmean, fvar = conditional(AT, Knn, q_mu, q_sqrt, dt)
    return dt(scale) * gaussian_ve(Y, fmean, fvar, s2, dt).sum() - gauss_kl(q_mu, q_sqrt, dt)


def elbo_multiclass(Kmm, Knm, Knn, q_mu, q_sqrt, y, jitter, scale=1.0, epsilon=EPSILON, n_gh=N_GH):
    """The fp64 restatement of the MultiClass ELBO."""
    gh_x, gh_w = hermgauss(n_gh)
    _, AT = whitened_A(Kmm, Knm, jitter)
    fmean, fvar = conditional(AT, Knn, q_mu, q_sqrt)
    ve, _, _ = variational_expectations(fmean, fvar, y, gh_x, gh_w, epsilon)
    return scale * ve.sum() - gauss_kl(q_mu, q_sqrt)


def elbo_multiclass_truth(Kmm, Knm, Knn, q_mu, q_sqrt, y, jitter, scale=1.0, epsilon=EPSILON, n_gh=N_GH):
    """The truth: the conditional and the KL in np.longdouble, the expectations in mpmath."""
    gh_x, gh_w = hermgauss(n_gh)
    _, AT = whitened_A(Kmm, Knm, jitter, LD)
    fmean, fvar = conditional(AT, Knn, q_mu, q_sqrt, LD)
    total = mpmath.mpf(0)
    for n in range(fmean.shape[0]):
        total += ve_truth(list(fmean[n]), list(fvar[n]), int(y[n]), gh_x, gh_w, epsilon)[0]
    return mp(scale) * total - mp(gauss_kl(q_mu, q_sqrt, LD))


def gaussian_optimum(Kmm, Knm, Y, s2, jitter, dtype=LD):
    """The analytic optimum of the whitened variational distribution under a Gaussian likelihood:
    S = (I + A A^T / s2)^-1, m = S A Y / s2; returns (q_mu (M x P), q_sqrt (P x M x M))."""
    dt = _dt(dtype)
    _, AT = whitened_A(Kmm, Knm, jitter, dt)
    M = AT.shape[1]
    Y = np.asarray(Y, dtype=dt)
    B = np.eye(M, dtype=dt) + (AT.T @ AT) / dt(s2)
    Lb = G.potrf_truth(B)
    Linv = G.trsm_truth(Lb, np.eye(M, dtype=dt), False).T          # Lb^-1
    S = Linv.T @ Linv
    m = S @ (AT.T @ Y) / dt(s2)
    Ls = G.potrf_truth(S)
    return m, np.stack([Ls] * Y.shape[1])


def collapsed_bound(Kmm, Knm, Knn, Y, s2, jitter):
    """Titsias' bound log N(Y | 0, A^T A + s2 I) - P tr(Knn - A^T A) / (2 s2) in np.longdouble, the jitter in A."""
    _, AT = whitened_A(Kmm, Knm, jitter, LD)
    Y, s2 = np.asarray(Y, dtype=LD), LD(s2)
    N, P = Y.shape
    Q = AT @ AT.T
    L = G.potrf_truth(Q + s2 * np.eye(N, dtype=LD))
    V = G.trsm_truth(L, Y.T, False)                                 # P x N
    two_pi = LD(8) * np.arctan(LD(1))
    lml = -LD(0.5) * (V * V).sum() - LD(P) * np.log(np.diag(L)).sum() - LD(0.5 * N * P) * np.log(two_pi)
    return lml - LD(P) * (np.asarray(Knn, dtype=LD).sum() - np.trace(Q)) / (LD(2) * s2)


# ------------------------------------------------------------------ the backward of the Cholesky factor
def cholesky_backward(Lm, AT, ATbar):
    """Given Lm = chol(Kmm), AT (N x M) with rows Lm^-1 k_n and dL/dAT (N x M): (dL/dKnm (N x M), dL/dKmm (M x M))
    by  Kmn_bar = Lm^-T A_bar,  L_bar = -tril(Kmn_bar A^T),  Kmm_bar = sym(Lm^-T Phi(Lm^T L_bar) Lm^-1),
    Phi the lower triangle with the diagonal halved."""
    Knm_bar = scipy.linalg.solve_triangular(Lm, ATbar.T, lower=True, trans="T").T
    L_bar = -np.tril(Knm_bar.T @ AT)
    S = Lm.T @ L_bar
    Phi = np.tril(S)
    Phi[np.diag_indices_from(Phi)] *= 0.5
    X = scipy.linalg.solve_triangular(Lm, Phi, lower=True, trans="T")           # Lm^-T Phi
    R = scipy.linalg.solve_triangular(Lm, X.T, lower=True, trans="T").T         # (Lm^-T X^T)^T = X Lm^-1
    return Knm_bar, 0.5 * (R + R.T)


# ------------------------------------------------------------------ the same ELBO as a plain torch expression
def ve_torch(torch, mu, var, y, gh_x, gh_w, epsilon=EPSILON):
    """MultiClass._variational_expectations on torch.special.erf and torch.clamp (n,)."""
    P = mu.shape[1]
    gx = torch.as_tensor(gh_x, dtype=mu.dtype, device=mu.device)
    w = torch.as_tensor(gh_w / np.sqrt(np.pi), dtype=mu.dtype, device=mu.device)
    y = torch.as_tensor(np.asarray(y), device=mu.device).long()
    mu_y = mu.gather(1, y[:, None])
    var_y = var.gather(1, y[:, None])
    x = mu_y + gx[None, :] * torch.sqrt(torch.clamp(2.0 * var_y, min=CLIP))           # n x n_gh
    d = (x[:, None, :] - mu[:, :, None]) / torch.sqrt(torch.clamp(var, min=CLIP))[:, :, None]
    cdfs = 0.5 * (1.0 + torch.special.erf(d / np.sqrt(2.0))) * CDF_SCALE + CDF_SHIFT
    on = torch.nn.functional.one_hot(y, P).to(mu.dtype)[:, :, None]
    cdfs = cdfs * (1.0 - on) + on
    p = torch.prod(cdfs, dim=1) @ w
    return p * np.log(1.0 - epsilon) + (1.0 - p) * np.log(epsilon / (P - 1))


def elbo_torch(torch, Kmm, Knm, Knn, q_mu, q_sqrt, Y, jitter, scale=1.0, noise=None, epsilon=EPSILON, n_gh=N_GH):
    """The ELBO on torch.linalg.cholesky / solve_triangular autograd; ``noise`` (a tensor): the Gaussian likelihood
    with Y (N x P) real, else MultiClass with Y integer labels."""
    M = Kmm.shape[0]
    Lm = torch.linalg.cholesky(Kmm + jitter * torch.eye(M, dtype=Kmm.dtype, device=Kmm.device))
    A = torch.linalg.solve_triangular(Lm, Knm.t(), upper=False)                      # M x N
    Lq = torch.tril(q_sqrt)
    fmean = A.t() @ q_mu
    base = Knn - (A * A).sum(dim=0)
    fvar = torch.stack([base + ((A.t() @ Lq[p]) ** 2).sum(dim=1) for p in range(Lq.shape[0])], dim=1)
    if noise is not None:
        ve = (-0.5 * torch.log(2.0 * np.pi * noise) - 0.5 * ((Y - fmean) ** 2 + fvar) / noise).sum(dim=1)
    else:
        gh_x, gh_w = hermgauss(n_gh)
        ve = ve_torch(torch, fmean, fvar, Y, gh_x, gh_w, epsilon)
    P = Lq.shape[0]
    kl = 0.5 * ((q_mu * q_mu).sum() - P * M - torch.log(torch.diagonal(Lq, dim1=1, dim2=2) ** 2).sum()
                + (Lq * Lq).sum())
    return scale * ve.sum() - kl
