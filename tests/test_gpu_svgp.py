"""GPU: the sparse variational GP -- grf_amd.features.svgp_elbo and efficient_graph_gp.models.SVGP.

The graph is the N = 60 ring with chords of tests/test_gpu_gpr.py; the step matrices are given (powers of the
normalised adjacency, no walk is run); 40 training nodes, 17 of them inducing, 20 test nodes, jitter 1e-6.

Truths are evaluated on the K read back from the device and widened to fp64, which isolates the model from the fp32
Gram: the linear algebra in np.longdouble, everything that passes through erf in mpmath (tests/svgp_reference.py).
Rule: the GPU's error against the truth <= max(10 x the fp64 restatement's own error, floor).  The floor of the
conditional, the KL and the Gaussian bound is N u kappa(K[Z, Z] + jitter I) |value| (u = 2^-53, N = 40); a quantity
that passes through the quadrature adds the quadrature's own floor 4 (P + n_gh) u |value|
(tests/test_svgp_reference.py), once per data point for the ELBO's sum.  Gradients are compared with the autograd of
the same expression on torch.linalg.cholesky / solve_triangular / torch.special.erf from the same K_torch output:
that is an fp64 computation of the same class, not a truth, so the difference is held to the sum of the two
floors, 2 N u kappa |value| (as tests/test_gpu_gpr.py's end-to-end test does).

  (a) Gaussian, P = 2: the ELBO at the analytic optimum equals the collapsed bound.
  (b) MultiClass, P = 3, random q_mu and lower q_sqrt: elbo, predict_f, predict_y, predict_log_density.
  (c) training_loss(...).backward() under torch.cuda.set_sync_debug_mode("error"); the gradients of q_mu, q_sqrt,
      the kernel's modulator_vector and the Gaussian's variance.
  (d) a minibatch of 10 rows with num_data = 40 scales the expectation term and not the KL.
  (e) 30 Adam steps at lr 0.05 on a three-community planted-partition graph, N = 90.
  (f) an indefinite K[Z, Z]: info != 0, a NaN loss, no exception until check().

The figures are printed; measured on an MI355X (kappa = 2.4), GPU error (restatement's error, floor): Gaussian ELBO
against the collapsed bound 1.6e-13 (4.2e-14, 6.1e-12); MultiClass ELBO 1.7e-15 (1.7e-15, 5.5e-12); predict_f mean
1.5e-16 (9.8e-17, 7.0e-15), variance 1.9e-16 (1.8e-16, 1.3e-14), covariance 2.1e-16 (2.1e-16, 1.3e-14); predict_y 1.2e-16
(1.1e-16, 2.1e-14); predict_log_density 3.4e-16 (3.4e-16, 1.3e-13).  Gradients against torch autograd, |diff| (bound):
MultiClass q_mu 1.3e-15 (1.3e-13), q_sqrt 6.7e-16 (5.1e-14), modulator 8.0e-15 (3.1e-13); Gaussian q_mu 4.4e-15 (2.9e-14),
q_sqrt 2.7e-15 (3.6e-14), modulator 2.8e-14 (1.1e-11), likelihood variance 1.7e-13 (1.0e-11); both losses equal bit for
bit.  Adam: ELBO -304.07 -> -39.12, all 30 test nodes as the restatement classifies them.
"""
import numpy as np
import pytest

import svgp_reference as R

pytestmark = pytest.mark.gpu

N, L, N_TRAIN, M, JITTER, NOISE = 60, 4, 40, 17, 1e-6, 0.1
U = float(R.U)


def _adjacency():
    A = np.zeros((N, N))
    for i in range(N):
        for d in (1, 7, 13):
            A[i, (i + d) % N] = A[(i + d) % N, i] = 1.0
    return A


def _steps(A, length=L):
    n = A.shape[0]
    W = A / np.sqrt(np.outer(A.sum(1), A.sum(1)))
    S = np.empty((n, n, length))
    Mat = np.eye(n)
    for l in range(length):
        S[:, :, l] = Mat
        Mat = Mat @ W
    return S


@pytest.fixture(scope="module")
def world():
    import torch
    from efficient_graph_gp.gpflow_kernels import GraphGeneralFastGRFKernel
    from efficient_graph_gp.likelihoods import Gaussian, MultiClass
    from efficient_graph_gp.models import SVGP
    A = _adjacency()
    kernel = GraphGeneralFastGRFKernel(A, max_walk_length=L, modulator_vector=np.array([1.0, 0.5, 0.25, 0.125]),
                                       step_matrices=_steps(A))
    r = np.random.default_rng(3)
    perm = r.permutation(N)
    tr, te = np.sort(perm[:N_TRAIN]), np.sort(perm[N_TRAIN:])
    z = np.sort(r.permutation(tr)[:M])
    with torch.no_grad():
        K = kernel.K_torch(np.arange(N), np.arange(N)).cpu().numpy().astype(np.float64)
    Kmm, Knm, Knn = K[np.ix_(z, z)], K[np.ix_(tr, z)], np.diag(K)[tr].copy()
    ev = np.linalg.eigvalsh(Kmm + JITTER * np.eye(M))
    kappa = ev[-1] / ev[0]
    Y2 = r.standard_normal((N_TRAIN, 2))
    y3 = r.integers(0, 3, N_TRAIN).astype(np.int32)
    q_mu3 = r.standard_normal((M, 3))
    q_sqrt3 = np.tril(r.standard_normal((3, M, M)) * 0.2) + np.eye(M)[None]
    return dict(torch=torch, kernel=kernel, tr=tr, te=te, z=z, K=K, Kmm=Kmm, Knm=Knm, Knn=Knn, kappa=kappa, Y2=Y2,
                y3=y3, q_mu3=q_mu3, q_sqrt3=q_sqrt3, SVGP=SVGP, Gaussian=Gaussian, MultiClass=MultiClass,
                floor=N_TRAIN * U * kappa, r=r)


def _held(name, got, rest, truth, floor):
    """The rule: GPU error <= max(10 x restatement error, floor); arrays of np.longdouble or lists of mpf."""
    if isinstance(np.ravel(truth)[0], R.mpmath.mpf):
        err = float(max(abs(R.mp(g) - t) for g, t in zip(np.ravel(got), np.ravel(truth))))
        own = float(max(abs(R.mp(g) - t) for g, t in zip(np.ravel(rest), np.ravel(truth))))
    else:
        t = np.asarray(truth, dtype=R.LD)
        err = float(np.abs(np.asarray(got, dtype=R.LD) - t).max())
        own = float(np.abs(np.asarray(rest, dtype=R.LD) - t).max())
    print(f"{name}: gpu error {err:.3e}, restatement error {own:.3e}, floor {floor:.3e}")
    assert err <= max(10 * own, floor), name


def _gaussian_model(world):
    torch = world["torch"]
    lik = world["Gaussian"](NOISE)
    s2 = float(lik.variance.item())
    assert abs(s2 - NOISE) <= 1e-12
    m, Ls = R.gaussian_optimum(world["Kmm"], world["Knm"], world["Y2"], s2, JITTER)
    q_mu, q_sqrt = np.asarray(m, np.float64), np.asarray(Ls, np.float64)
    model = world["SVGP"](world["kernel"], lik, world["z"], num_latent_gps=2, q_mu=q_mu, q_sqrt=q_sqrt,
                          jitter=JITTER)
    return model, s2, q_mu, q_sqrt


def test_a_gaussian_elbo_at_the_analytic_optimum_is_the_collapsed_bound(world):
    model, s2, q_mu, q_sqrt = _gaussian_model(world)
    elbo = model.elbo((world["tr"], world["Y2"]))
    assert elbo.dtype == world["torch"].float64 and elbo.dim() == 0
    model.check()
    want = R.collapsed_bound(world["Kmm"], world["Knm"], world["Knn"], world["Y2"], s2, JITTER)
    rest = R.elbo_gaussian(world["Kmm"], world["Knm"], world["Knn"], q_mu, q_sqrt, world["Y2"], s2, JITTER)
    print(f"ELBO {elbo.item():.6f}, collapsed bound {float(want):.6f}, kappa {world['kappa']:.3e}")
    _held("Gaussian ELBO against the collapsed bound", elbo.item(), rest, want, world["floor"] * abs(float(want)))
    # a perturbed m gives a smaller value
    with world["torch"].no_grad():
        model.q_mu.add_(1e-3)
    assert model.elbo((world["tr"], world["Y2"])).item() < elbo.item()
    # predict_y adds the likelihood's variance
    mf, vf = model.predict_f(world["te"])
    my, vy = model.predict_y(world["te"])
    assert np.array_equal(my.cpu().numpy(), mf.cpu().numpy())
    assert np.abs(vy.cpu().numpy() - (vf.cpu().numpy() + s2)).max() <= 4 * U * (np.abs(vf.cpu().numpy()).max() + s2)
    ld = model.predict_log_density((world["te"], np.zeros((N - N_TRAIN, 2)))).cpu().numpy()
    m_, v_ = my.cpu().numpy(), vy.cpu().numpy()
    ref = (-0.5 * (np.log(2 * np.pi) + np.log(v_) + m_ ** 2 / v_)).sum(axis=1)
    assert ld.shape == (N - N_TRAIN,) and np.allclose(ld, ref, rtol=1e-12, atol=1e-12)


def _multiclass_model(world, **kw):
    return world["SVGP"](world["kernel"], world["MultiClass"](3), world["z"], num_latent_gps=3, q_mu=world["q_mu3"],
                         q_sqrt=world["q_sqrt3"], jitter=JITTER, **kw)


def test_b_multiclass_elbo_and_predictions(world):
    model = _multiclass_model(world)
    q_mu, q_sqrt, y = world["q_mu3"], world["q_sqrt3"], world["y3"]
    P, n_gh = 3, R.N_GH
    log_miss = abs(np.log(R.EPSILON / (P - 1)))
    elbo = model.elbo((world["tr"], y))
    model.check()
    truth = R.elbo_multiclass_truth(world["Kmm"], world["Knm"], world["Knn"], q_mu, q_sqrt, y, JITTER)
    rest = R.elbo_multiclass(world["Kmm"], world["Knm"], world["Knn"], q_mu, q_sqrt, y, JITTER)
    floor = world["floor"] * abs(float(truth)) + N_TRAIN * R.floor_p(P, n_gh, log_miss)
    print(f"ELBO {elbo.item():.6f}")
    _held("MultiClass ELBO", [elbo.item()], [rest], [truth], floor)
    kl = model.prior_kl().item()
    assert abs(kl - float(R.gauss_kl(q_mu, q_sqrt, R.LD))) <= world["floor"] * abs(kl)
    # predict_f against the np.longdouble conditional
    te, z = world["te"], world["z"]
    Ksz, Kss = world["K"][np.ix_(te, z)], np.diag(world["K"])[te]
    Lt, ATt = R.whitened_A(world["Kmm"], Ksz, JITTER, R.LD)
    tmean, tvar = R.conditional(ATt, Kss, q_mu, q_sqrt, R.LD)
    _, ATr = R.whitened_A(world["Kmm"], Ksz, JITTER)
    rmean, rvar = R.conditional(ATr, Kss, q_mu, q_sqrt)
    mean, var = model.predict_f(te)
    assert tuple(mean.shape) == (N - N_TRAIN, P) and tuple(var.shape) == (N - N_TRAIN, P)
    _held("predict_f mean", mean.cpu().numpy(), rmean, tmean, world["floor"] * float(np.abs(tmean).max()))
    _held("predict_f variance", var.cpu().numpy(), rvar, tvar, world["floor"] * float(np.abs(tvar).max()))
    # the full covariance: its diagonal is the variance, each latent's matrix is symmetric
    mean_c, cov = model.predict_f(te, full_cov=True)
    assert tuple(cov.shape) == (P, N - N_TRAIN, N - N_TRAIN)
    cov = cov.cpu().numpy()
    assert np.array_equal(mean_c.cpu().numpy(), mean.cpu().numpy())
    tcov = np.stack([np.asarray(world["K"][np.ix_(te, te)], R.LD) - ATt @ ATt.T
                     + (ATt @ np.tril(q_sqrt[p]).astype(R.LD)) @ (ATt @ np.tril(q_sqrt[p]).astype(R.LD)).T
                     for p in range(P)])
    rcov = np.stack([world["K"][np.ix_(te, te)] - ATr @ ATr.T
                     + (ATr @ np.tril(q_sqrt[p])) @ (ATr @ np.tril(q_sqrt[p])).T for p in range(P)])
    _held("predict_f covariance", cov, rcov, tcov, world["floor"] * float(np.abs(tcov).max()))
    for p in range(P):
        assert np.array_equal(cov[p], cov[p].T)
    # predict_y and predict_log_density against mpmath on the np.longdouble conditional
    gh_x, gh_w = R.hermgauss()
    tps = [R.predict_truth(list(tmean[k]), list(tvar[k]), gh_x, gh_w) for k in range(len(te))]
    rps = R.predict_probabilities(rmean, rvar, gh_x, gh_w)
    ps, pv = model.predict_y(te)
    ps = ps.cpu().numpy()
    qfloor = world["floor"] + R.floor_p(P, n_gh, 1.0)
    _held("predict_y", ps, rps, tps, qfloor)
    assert np.abs(pv.cpu().numpy() - (ps - ps ** 2)).max() <= 4 * U
    ynew = world["r"].integers(0, P, len(te)).astype(np.int32)
    ld = model.predict_log_density((te, ynew)).cpu().numpy()
    tld = [R.mpmath.log(tps[k][int(ynew[k])]) for k in range(len(te))]
    rld = np.log(rps[np.arange(len(te)), ynew])
    scale = float(max(1 / tps[k][int(ynew[k])] for k in range(len(te))))       # d log p = dp / p
    _held("predict_log_density", ld, rld, tld, qfloor * scale + 2 * U * float(max(abs(v) for v in tld)))
    # labels are validated on the host
    with pytest.raises(ValueError, match="labels must be integers"):
        model.elbo((world["tr"], np.full(N_TRAIN, 3)))
    with pytest.raises(ValueError, match="labels must be integers"):
        model.elbo((world["tr"], y + 0.5))


def _grads(model, kernel, extra=()):
    out = [model.q_mu.grad.clone(), model.q_sqrt.grad.clone(), kernel.modulator_vector.grad.clone()]
    out += [p.grad.clone() for p in extra]
    model.zero_grad()
    kernel.zero_grad()
    return out


@pytest.mark.parametrize("which", ["multiclass", "gaussian"])
def test_c_gradients_without_a_host_synchronisation(world, which):
    torch, kernel = world["torch"], world["kernel"]
    if which == "gaussian":
        model, _, _, _ = _gaussian_model(world)
        with torch.no_grad():
            model.q_mu.add_(0.05)                         # (away from the optimum, where both gradients vanish:
            model.q_sqrt.mul_(1.25)                       # there they are rounding noise without a magnitude)
        data = (torch.from_numpy(world["tr"]).cuda(), torch.from_numpy(world["Y2"]).cuda())
        extra = [model.likelihood.raw_variance]
    else:
        model = _multiclass_model(world)
        data = (torch.from_numpy(world["tr"]).cuda(), torch.from_numpy(world["y3"]).cuda())
        extra = []
    model.zero_grad()
    kernel.zero_grad()
    model.training_loss(data)                             # (the labels are validated and kept at the first call)
    with torch.no_grad():
        kernel.modulator_vector.mul_(1.0)                 # (a new version, as after an optimiser step: K and the
    torch.cuda.synchronize()                              # factor of K[Z, Z] are computed again under the check)
    assert model._key() != model._factor_key
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = model.training_loss(data)
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(model.cholesky_info.item()) == 0
    got = [loss.detach().reshape(1)] + _grads(model, kernel, extra)
    # the same expression on torch.linalg.cholesky and torch.special.erf, from the same K_torch output
    z, tr = torch.from_numpy(world["z"]).cuda(), data[0]
    Kb = kernel.K_torch(torch.cat([z, tr]), z).to(torch.float64)
    Knn = kernel.K_torch(tr, tr).diagonal().to(torch.float64)
    noise = model.likelihood.variance if which == "gaussian" else None
    Y = data[1] if which == "gaussian" else world["y3"]
    ref = -R.elbo_torch(torch, Kb[:M], Kb[M:], Knn, model.q_mu, model.q_sqrt, Y, JITTER, noise=noise)
    ref.backward()
    want = [ref.detach().reshape(1)] + _grads(model, kernel, extra)
    assert np.array_equal(np.triu(got[2].cpu().numpy(), 1), np.zeros_like(got[2].cpu().numpy()))
    bound = 2 * world["floor"]
    if which == "multiclass":                             # (the quadrature's floor on both sides as well)
        bound += 2 * R.floor_p(3, R.N_GH, 1.0)
    names = ["loss", "q_mu", "q_sqrt", "modulator"] + ["likelihood variance"] * len(extra)
    for name, g, w in zip(names, got, want):
        g, w = g.cpu().numpy(), w.cpu().numpy()
        err, scale = np.abs(g - w).max(), np.abs(w).max()
        print(f"{which} {name}: |diff| {err:.3e}, bound {bound * scale:.3e} (|value| {scale:.3e})")
        assert np.all(np.isfinite(g)) and scale > 0
        assert err <= bound * scale, name


def test_d_a_minibatch_scales_the_expectation_term_and_not_the_kl(world):
    rows = np.arange(0, N_TRAIN, 4)
    assert len(rows) == 10
    tr, y = world["tr"][rows], world["y3"][rows]
    plain = _multiclass_model(world).elbo((tr, y)).item()
    model = _multiclass_model(world, num_data=N_TRAIN)
    scaled = model.elbo((tr, y)).item()
    kl = model.prior_kl().item()
    want = 4.0 * (plain + kl) - kl
    print(f"minibatch: elbo {scaled:.6f}, 4 (sum ve) - KL {want:.6f}, KL {kl:.6f}")
    assert abs(scaled - want) <= 16 * U * (4 * abs(plain + kl) + 5 * abs(kl))
    assert abs(model.training_loss((tr, y)).item() + scaled) == 0.0


def test_e_adam_steps_raise_the_elbo_and_the_predicted_classes_are_the_restatements(world):
    torch = world["torch"]
    from efficient_graph_gp.gpflow_kernels import GraphGeneralFastGRFKernel
    n, P = 90, 3
    r = np.random.default_rng(11)
    comm = np.repeat(np.arange(P), n // P)
    prob = np.where(comm[:, None] == comm[None, :], 0.3, 0.02)
    A = np.triu((r.random((n, n)) < prob).astype(np.float64), 1)
    A = A + A.T
    for i in range(n):                                     # (no isolated node)
        A[i, (i + 1) % n] = A[(i + 1) % n, i] = 1.0
    kernel = GraphGeneralFastGRFKernel(A, max_walk_length=L, modulator_vector=np.array([1.0, 0.5, 0.25, 0.125]),
                                       step_matrices=_steps(A))
    perm = r.permutation(n)
    tr, te = np.sort(perm[:60]), np.sort(perm[60:])
    z = np.sort(r.permutation(tr)[:30])
    model = world["SVGP"](kernel, world["MultiClass"](P), z, num_latent_gps=P)
    data = (tr, comm[tr])
    first = model.elbo(data).item()
    opt = torch.optim.Adam(model.parameters(), lr=0.05)
    for _ in range(30):
        opt.zero_grad()
        loss = model.training_loss(data)
        loss.backward()
        opt.step()
    last = model.elbo(data).item()
    model.check()
    print(f"Adam: ELBO {first:.4f} -> {last:.4f}")
    assert np.isfinite(last) and last > first
    ps = model.predict_y(te)[0].cpu().numpy()
    with torch.no_grad():
        K = kernel.K_torch(np.arange(n), np.arange(n)).cpu().numpy().astype(np.float64)
    _, AT = R.whitened_A(K[np.ix_(z, z)], K[np.ix_(te, z)], model.jitter)
    fmean, fvar = R.conditional(AT, np.diag(K)[te], model.q_mu.detach().cpu().numpy(),
                                model.q_sqrt.detach().cpu().numpy())
    rps = R.predict_probabilities(fmean, fvar, *R.hermgauss())
    top = np.sort(rps, axis=1)
    clear = top[:, -1] - top[:, -2] >= 1e-9
    acc = float((ps.argmax(axis=1) == comm[te]).mean())
    print(f"test accuracy {acc:.3f}, {int(clear.sum())} of {len(te)} nodes with a clear winner, "
          f"max |ps - restatement| {np.abs(ps - rps).max():.3e}")
    assert clear.sum() >= len(te) // 2
    assert np.array_equal(ps.argmax(axis=1)[clear], rps.argmax(axis=1)[clear])


def test_f_failure_path(world):
    torch = world["torch"]
    from efficient_graph_gp.gpflow_kernels import GraphGeneralFastGRFKernel
    r = np.random.default_rng(5)
    S = np.zeros((N, N, L))
    S[:, :, 0] = r.standard_normal((N, 3)) @ r.standard_normal((3, N))      # Phi of rank 3: K is rank-deficient
    kernel = GraphGeneralFastGRFKernel(_adjacency(), max_walk_length=L,
                                       modulator_vector=np.array([2.0, 0.0, 0.0, 0.0]), step_matrices=S)
    tr = world["tr"]
    with torch.no_grad():
        K = kernel.K_torch(tr, tr).cpu().numpy().astype(np.float64)
    assert np.linalg.eigvalsh(K + JITTER * np.eye(N_TRAIN))[0] < -1e-5, \
        "the fp32 Gram's rounding leaves K[Z, Z] + jitter I indefinite"
    model = world["SVGP"](kernel, world["MultiClass"](3), tr, num_latent_gps=3, jitter=JITTER)
    assert model.cholesky_info is None
    loss = model.training_loss((tr, world["y3"]))
    loss.backward()                                                          # (no exception)
    assert np.isnan(loss.item())
    assert int(model.cholesky_info.item()) != 0
    with pytest.raises(ValueError, match="Cholesky decomposition was not successful"):
        model.check()
    ok = world["SVGP"](kernel, world["MultiClass"](3), tr, num_latent_gps=3, jitter=1.0)
    assert np.isfinite(ok.elbo((tr, world["y3"])).item())
    ok.check()
    for kw in (dict(mean_function=lambda x: x), dict(q_diag=True), dict(whiten=False)):
        with pytest.raises(NotImplementedError):
            world["SVGP"](kernel, world["MultiClass"](3), tr, num_latent_gps=3, **kw)
