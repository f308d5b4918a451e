"""GPU: the dense exact GPR -- grf_amd.features.gpr_log_marginal_likelihood and efficient_graph_gp.models.GPR.

The graph is an N = 60 ring with chords; the step matrices are given (step_matrices=: powers of the normalised
adjacency, no walk is run); 40 training nodes, 20 test nodes, Y with two columns, sigma^2 = 0.1.

Function level.  The truth is tests/gpr_reference.py in np.longdouble on the K read back from the device and
widened to fp64, which isolates the solver from the fp32 Gram.  lml, dL/dK, dL/dsigma^2, the mean, the variance and
the full covariance are held to the project's usual rule (tests/test_gpu_mll.py): the GPU's error against the
truth <= 10 x the restatement's own error against that truth, with a floor of n u kappa(K^) |value| (u = 2^-53,
kappa from numpy.linalg.eigvalsh; |value| the quantity's largest magnitude).  The figures are printed; measured on
an MI355X (kappa = 4.9): lml 1.6e-14 (restatement 1.6e-14, floor 2.6e-12), dL/dK 1.5e-15 (1.5e-15, 7.3e-14), dL/dsigma^2
5.2e-15 (5.2e-15, 1.5e-13), mean 2.7e-16 (1.2e-16, 1.2e-14), variance 1.2e-16 (1.5e-16, 2.3e-14), covariance 1.2e-16
(1.2e-16, 2.3e-14); end to end the modulator gradient differs by 7.1e-15 (bound 4.8e-13), the noise gradient by 5.6e-16.

End to end.  GPR(...).log_marginal_likelihood().backward() fills kernel.modulator_vector.grad and the noise
gradient; both equal the gradients of the same expression evaluated with torch.linalg.cholesky on the same K_torch
output.  That reference is itself an fp64 computation of the same error class, not a truth, so the difference is
held to the sum of the two floors, 2 n u kappa |value|.  Forward and backward run under
torch.cuda.set_sync_debug_mode("error").
"""
import numpy as np
import pytest

import gpr_reference as R

pytestmark = pytest.mark.gpu

N, L, N_TRAIN, P, NOISE = 60, 4, 40, 2, 0.1
U = float(R.U)


def _adjacency():
    A = np.zeros((N, N))
    for i in range(N):
        for d in (1, 7, 13):
            A[i, (i + d) % N] = A[(i + d) % N, i] = 1.0
    return A


def _steps(A):
    W = A / np.sqrt(np.outer(A.sum(1), A.sum(1)))
    S = np.empty((N, N, L))
    M = np.eye(N)
    for l in range(L):
        S[:, :, l] = M
        M = M @ W
    return S


@pytest.fixture(scope="module")
def world():
    import torch
    from efficient_graph_gp.gpflow_kernels import GraphGeneralFastGRFKernel
    from efficient_graph_gp.models import GPR
    A = _adjacency()
    kernel = GraphGeneralFastGRFKernel(A, max_walk_length=L, modulator_vector=np.array([1.0, 0.5, 0.25, 0.125]),
                                       step_matrices=_steps(A))
    r = np.random.default_rng(3)
    perm = r.permutation(N)
    tr, te = np.sort(perm[:N_TRAIN]), np.sort(perm[N_TRAIN:])
    Y = r.standard_normal((N_TRAIN, P))
    model = GPR(data=(tr[:, None].astype(np.float64), Y), kernel=kernel, noise_variance=NOISE)
    with torch.no_grad():
        K = kernel.K_torch(tr, tr).cpu().numpy().astype(np.float64)
        Ksx = kernel.K_torch(te, tr).cpu().numpy().astype(np.float64)
        Kss = kernel.K_torch(te, te).cpu().numpy().astype(np.float64)
        noise = float(model.likelihood_variance.item())
    assert abs(noise - NOISE) <= 1e-12
    ev = np.linalg.eigvalsh(K + noise * np.eye(N_TRAIN))
    kappa = ev[-1] / ev[0]
    truth = R.gpr(K, noise, Y, Ksx, Kss, dtype=np.longdouble)
    rest = R.gpr(K, noise, Y, Ksx, Kss)
    return dict(torch=torch, kernel=kernel, model=model, tr=tr, te=te, Y=Y, K=K, Ksx=Ksx, Kss=Kss, noise=noise,
                kappa=kappa, truth=truth, rest=rest, GPR=GPR)


def _held(world, name, got):
    """The rule: GPU error <= max(10 x restatement error, n u kappa |value|), all in np.longdouble."""
    t = np.asarray(world["truth"][name], dtype=R.LD)
    err = np.abs(np.asarray(got, dtype=R.LD) - t).max()
    own = np.abs(np.asarray(world["rest"][name], dtype=R.LD) - t).max()
    floor = N_TRAIN * R.U * R.LD(world["kappa"]) * np.abs(t).max()
    print(f"{name}: gpu error {float(err):.3e}, restatement error {float(own):.3e}, floor {float(floor):.3e} "
          f"(kappa {world['kappa']:.3e}, |value| {float(np.abs(t).max()):.3e})")
    assert err <= max(10 * own, floor), name


def test_function_value_and_gradients(world):
    torch = world["torch"]
    from grf_amd.features import gpr_log_marginal_likelihood
    Kd = torch.from_numpy(world["K"]).cuda().requires_grad_(True)
    noise = torch.tensor(world["noise"], dtype=torch.float64, device="cuda", requires_grad=True)
    Yd = torch.from_numpy(world["Y"]).cuda()
    lml, info = gpr_log_marginal_likelihood(Kd, noise, Yd)
    assert lml.dtype == torch.float64 and lml.dim() == 0 and info.dtype == torch.int32
    lml.backward()
    assert int(info.item()) == 0
    _held(world, "lml", lml.item())
    _held(world, "dK", Kd.grad.cpu().numpy())
    _held(world, "dnoise", noise.grad.item())
    # an fp32 K (as K_torch may return it) is widened: the value is that of the widened matrix
    lml32, _ = gpr_log_marginal_likelihood(Kd.detach().float(), noise.detach(), Yd)
    _held(world, "lml", lml32.item())


def test_predictions(world):
    model = world["model"]
    mean, var = model.predict_f(world["te"])
    assert tuple(mean.shape) == (N - N_TRAIN, P) and tuple(var.shape) == (N - N_TRAIN, P)
    _held(world, "mean", mean.cpu().numpy())
    var = var.cpu().numpy()
    assert np.array_equal(var[:, 0], var[:, 1])
    _held(world, "var", var[:, 0])
    mean_c, cov = model.predict_f(world["te"], full_cov=True)
    assert tuple(cov.shape) == (P, N - N_TRAIN, N - N_TRAIN)
    cov = cov.cpu().numpy()
    assert np.array_equal(mean_c.cpu().numpy(), mean.cpu().numpy()) and np.array_equal(cov[0], cov[1])
    assert np.array_equal(cov[0], cov[0].T)
    _held(world, "cov", cov[0])
    # the covariance's diagonal is the variance to n u kappa
    scale = np.abs(np.diag(world["Kss"])).max()
    assert np.abs(np.diag(cov[0]) - var[:, 0]).max() <= N_TRAIN * U * world["kappa"] * scale
    # predict_y adds the noise to the variances
    my, vy = model.predict_y(world["te"])
    assert np.array_equal(my.cpu().numpy(), mean.cpu().numpy())
    assert np.abs(vy.cpu().numpy() - (var + world["noise"])).max() <= 4 * U * (scale + world["noise"])
    _, cy = model.predict_y(world["te"], full_cov=True)
    off = ~np.eye(N - N_TRAIN, dtype=bool)
    assert np.array_equal(cy.cpu().numpy()[0][off], cov[0][off])
    assert np.abs(np.diag(cy.cpu().numpy()[0]) - (np.diag(cov[0]) + world["noise"])).max() <= 4 * U * (scale + 1)
    # the log density under predict_y's marginals
    Yn = np.random.default_rng(9).standard_normal((N - N_TRAIN, P))
    ld = model.predict_log_density((world["te"], Yn)).cpu().numpy()
    m, v = my.cpu().numpy(), vy.cpu().numpy()
    ref = (-0.5 * (np.log(2 * np.pi) + np.log(v) + (Yn - m) ** 2 / v)).sum(axis=1)
    assert ld.shape == (N - N_TRAIN,) and np.allclose(ld, ref, rtol=1e-12, atol=1e-12)


def test_variance_at_a_training_node_with_almost_no_noise(world):
    torch = world["torch"]
    model = world["GPR"](data=(world["tr"], world["Y"]), kernel=world["kernel"], noise_variance=1e-6 + 1e-9)
    node = world["tr"][:5]
    _, var = model.predict_f(node)
    model.check()
    with torch.no_grad():
        prior = world["kernel"].K_torch(node, node).diagonal().cpu().numpy().astype(np.float64)
    var = var.cpu().numpy()[:, 0]
    assert np.all(var < prior)


def test_end_to_end_gradients_without_a_host_synchronisation(world):
    torch = world["torch"]
    model, kernel = world["model"], world["kernel"]
    model.zero_grad()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        lml = model.log_marginal_likelihood()
        lml.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(model.cholesky_info.item()) == 0
    model.check()
    g_f, g_n = kernel.modulator_vector.grad.clone(), model.raw_likelihood_variance.grad.clone()
    assert abs(float(model.training_loss().item()) + float(lml.item())) == 0.0
    model.zero_grad()
    # the same expression on torch.linalg.cholesky, from the same K_torch output
    K = kernel.K_torch(world["tr"], world["tr"]).to(torch.float64)
    Kh = K + model.likelihood_variance * torch.eye(N_TRAIN, dtype=torch.float64, device=K.device)
    Lt = torch.linalg.cholesky(Kh)
    a = torch.cholesky_solve(model.Y, Lt)
    ref = -0.5 * (model.Y * a).sum() - P * torch.log(Lt.diagonal()).sum() - 0.5 * N_TRAIN * P * np.log(2 * np.pi)
    ref.backward()
    r_f, r_n = kernel.modulator_vector.grad.clone(), model.raw_likelihood_variance.grad.clone()
    model.zero_grad()
    bound = 2 * N_TRAIN * U * world["kappa"]
    for name, got, want in (("lml", lml.detach().reshape(1), ref.detach().reshape(1)), ("modulator", g_f, r_f),
                            ("noise", g_n.reshape(1), r_n.reshape(1))):
        got, want = got.cpu().numpy(), want.cpu().numpy()
        err, scale = np.abs(got - want).max(), np.abs(want).max()
        print(f"end to end {name}: |diff| {err:.3e}, bound {bound * scale:.3e} (|value| {scale:.3e})")
        assert np.all(np.isfinite(got)) and scale > 0
        assert err <= bound * scale, name


def test_failure_path(world):
    torch = world["torch"]
    from efficient_graph_gp.gpflow_kernels import GraphGeneralFastGRFKernel
    r = np.random.default_rng(5)
    S = np.zeros((N, N, L))
    S[:, :, 0] = r.standard_normal((N, 3)) @ r.standard_normal((3, N))      # Phi of rank 3: K is rank-deficient
    kernel = GraphGeneralFastGRFKernel(_adjacency(), max_walk_length=L,
                                       modulator_vector=np.array([2.0, 0.0, 0.0, 0.0]), step_matrices=S)
    model = world["GPR"](data=(world["tr"], world["Y"]), kernel=kernel, noise_variance=NOISE)
    assert np.isfinite(model.log_marginal_likelihood().item()) and int(model.cholesky_info.item()) == 0
    model.check()                                                            # K + 0.1 I is fine
    model.raw_likelihood_variance.data.fill_(-40.0)                          # sigma^2 -> the 1e-6 lower bound
    model.invalidate()
    with torch.no_grad():
        K = kernel.K_torch(world["tr"], world["tr"]).cpu().numpy().astype(np.float64)
    floor = float(model.likelihood_variance.item())
    assert abs(floor - 1e-6) < 1e-12
    assert np.linalg.eigvalsh(K + floor * np.eye(N_TRAIN))[0] < -1e-5, "the fp32 Gram's rounding leaves K^ indefinite"
    lml = model.log_marginal_likelihood()
    assert np.isnan(lml.item())
    assert int(model.cholesky_info.item()) != 0
    with pytest.raises(ValueError, match="Cholesky decomposition was not successful"):
        model.check()
    with pytest.raises(NotImplementedError):
        world["GPR"](data=(world["tr"], world["Y"]), kernel=kernel, mean_function=lambda x: x)


def test_lbfgs_steps_do_not_increase_the_loss(world):
    torch = world["torch"]
    from efficient_graph_gp.gpflow_kernels import GraphGeneralFastGRFKernel
    A = _adjacency()
    kernel = GraphGeneralFastGRFKernel(A, max_walk_length=L, modulator_vector=np.array([1.0, 0.5, 0.25, 0.125]),
                                       step_matrices=_steps(A))
    model = world["GPR"](data=(world["tr"], world["Y"]), kernel=kernel, noise_variance=NOISE)
    opt = torch.optim.LBFGS(model.parameters(), lr=1.0, max_iter=5, line_search_fn="strong_wolfe")

    def closure():
        opt.zero_grad()
        loss = model.training_loss()
        loss.backward()
        return loss

    losses = [float(model.training_loss().item())]
    for _ in range(3):
        opt.step(closure)
        losses.append(float(model.training_loss().item()))
    print("LBFGS losses:", losses)
    assert all(np.isfinite(losses))
    assert all(b <= a for a, b in zip(losses, losses[1:])) and losses[-1] < losses[0]
    model.check()


def test_one_column_targets_survive_predictions(world):
    """The DenseGPModel case, Y of shape (n, 1): predictions leave the model's data and values unchanged (a
    transposed one-column Y shares its storage with Y, so nothing derived from it may be solved in place)."""
    torch = world["torch"]
    y = world["Y"][:, :1].copy()
    model = world["GPR"](data=(world["tr"], y), kernel=world["kernel"], noise_variance=NOISE)
    before = float(model.log_marginal_likelihood().item())
    m1, v1 = model.predict_f(world["te"])
    assert np.array_equal(model.Y.cpu().numpy(), y), "predict_f changed the training targets"
    model.predict_y(world["te"], full_cov=True)
    model.predict_log_density((world["te"], np.zeros((N - N_TRAIN, 1))))
    m2, v2 = model.predict_f(world["te"])
    assert np.array_equal(model.Y.cpu().numpy(), y), "the predictions changed the training targets"
    assert np.array_equal(m1.cpu().numpy(), m2.cpu().numpy()) and np.array_equal(v1.cpu().numpy(), v2.cpu().numpy())
    assert float(model.log_marginal_likelihood().item()) == before
    # the one-column values are the first column's of the two-column truth's formulas
    tru = R.gpr(world["K"], world["noise"], y, world["Ksx"], world["Kss"], dtype=np.longdouble)
    floor = N_TRAIN * U * world["kappa"]
    assert abs(before - float(tru["lml"])) <= floor * abs(float(tru["lml"]))
    assert np.abs(m1.cpu().numpy() - np.asarray(tru["mean"], dtype=np.float64)).max() <= floor * np.abs(tru["mean"]).max()
    # the kernel's matrices are untouched as well: the same blocks come back bit for bit
    with torch.no_grad():
        K = world["kernel"].K_torch(world["tr"], world["tr"]).cpu().numpy().astype(np.float64)
    assert np.array_equal(K, world["K"])
