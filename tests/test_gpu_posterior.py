"""GPU: the exact posterior mean and variance -- grf_posterior_reduce_f64 and grf_posterior_rhs_f64 called
directly (csrc/grf_posterior.hip), GRFEngine.posterior_moments on the walk's Phi and on the WalkPolynomial
operator, SparseGraphGP.predict_f / predict_y / nlpd -- against numpy, the restatement
(tests/posterior_reference.py) and the dense truth computed on the CPU.

The graph has N = 300 nodes of degree ~6; the step matrices come from the engine's own walk (8 walks,
p_halt = 0.2, L = 4), as in tests/test_gpu_mll.py.  Phi is read back from the device so that restatement and truth
see the engine's own fp32 values widened to fp64; on the operator path the truth is the dense p(G) p(G)^T.

Tolerances
  * reduce kernel: |err| <= 1e-12 * sum |terms| against numpy fp64 (the project's bound for steps_frob); a second
    call and a column permutation give the same bits; NaN pad lanes do not leak.
  * rhs kernel: E equals the dense Phi[x]^T exactly (fp32 widens exactly), nothing outside the pitch window is
    written, prior within nnz_row * 2^-53 * sum v^2 of numpy's sum.
  * engine / model at the stall tolerance (1e-12, max_iter >= n): GPU error against the dense truth <= 10 x the
    restatement's own error on that case, computed inside the test (the rule of test_gpu_mll.py), never below
    the reduce kernel's own 1e-12 * prior; errors relative to the largest prior variance.
  * at tolerance = 1: var >= truth - 1e-12 * prior for every node (CG's monotone b^T x_k).
"""
import numpy as np
import pytest
import scipy.sparse as sp

import poly_reference as PR
import posterior_reference as R

pytestmark = pytest.mark.gpu

N, F = 300, [1.0, -0.5, 0.25, -0.125]
U53 = 2.0 ** -53


def _graph(n, deg, seed):
    r = np.random.default_rng(seed)
    m = int(n * deg / 2)
    u, v = r.integers(0, n, m), r.integers(0, n, m)
    keep = u != v
    A = sp.coo_matrix((np.ones(keep.sum()), (u[keep], v[keep])), shape=(n, n)).tocsr()
    A = (A + A.T).tocsr()
    A.data[:] = 1.0
    return A


def _phi_scipy(phi):
    P = phi.to_scipy().astype(np.float64)
    P.data = phi.val32[:phi.nnz].cpu().numpy().astype(np.float64)
    return P


@pytest.fixture(scope="module")
def world():
    """Engine, the walk's step matrices, Phi(F) on the device and as scipy; the walk operator p(G) and its dense
    matrix."""
    import torch
    from efficient_graph_gp_sparse.preprocessor import GraphPreprocessor
    from grf_amd.engine import GRFEngine, WalkPolynomial
    from grf_amd.features import StepMatrices

    eng = GRFEngine("cuda:0")
    A = _graph(N, 6, 11)
    pre = GraphPreprocessor(A, walks_per_node=8, p_halt=0.2, max_walk_length=4, random_walk_seed=3, use_tqdm=False)
    ops = pre.preprocess_graph()
    steps = StepMatrices(ops, eng)
    f = torch.tensor(F, dtype=torch.float32)
    phi = steps.phi(f)
    G = eng.laplacian(A)
    op = WalkPolynomial(G, 4, engine=eng)
    return dict(eng=eng, ops=ops, steps=steps, f=f, phi=phi, P=_phi_scipy(phi), op=op,
                Pop=PR.dense_poly(G.to_scipy(), F, 4))


def _nan(shape):
    import torch
    return torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")


# ------------------------------------------------------------------------------------ 1. the reduce kernel
def _reduce_raw(eng, Bp, Xp, S, alpha, prior, add_noise=0.0):
    """grf_posterior_reduce_f64 itself on padded blocks; (var, mean) as numpy after checking that nothing past the
    S results or past the workspace was written and that the ticket is zero again."""
    import torch
    from grf_amd.engine import _p
    n = Bp.shape[0]
    need = eng.lib.grf_posterior_reduce_workspace_bytes(n, S)
    ws = _nan((need // 8 + 64,))
    var, mean = _nan((S + 8,)), _nan((S + 8,))
    rc = eng.lib.grf_posterior_reduce_f64(n, S, _p(Bp), Bp.stride(0), _p(Xp), Xp.stride(0), _p(alpha), _p(prior),
                                          float(add_noise), _p(var), _p(mean) if alpha is not None else None, _p(ws),
                                          need, eng.stream)
    torch.cuda.synchronize()
    assert rc == 0, eng.lib.grf_last_error()
    assert int(ws[:1].view(torch.int32)[0].item()) == 0, "the ticket is not zero afterwards"
    assert torch.isnan(ws[need // 8:]).all(), "wrote past the workspace"
    assert torch.isnan(var[S:]).all() and torch.isnan(mean[S:]).all(), "wrote past the results"
    if alpha is None:
        assert torch.isnan(mean).all(), "mean written without alpha"
    return var[:S].cpu().numpy(), (mean[:S].cpu().numpy() if alpha is not None else None)


@pytest.mark.parametrize("S", [1, 5, 64, 65, 256])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1025, 70001])
def test_reduce_kernel_vs_numpy(world, n, S):
    import torch
    eng = world["eng"]
    g = torch.Generator(device="cuda").manual_seed(1000 * S + n)
    Bp, Xp = _nan((n, S + 3)), _nan((n, S + 5))                      # pitches > S, the pad lanes NaN
    Bp[:, :S] = torch.randn((n, S), generator=g, dtype=torch.float64, device="cuda")
    Xp[:, :S] = torch.randn((n, S), generator=g, dtype=torch.float64, device="cuda")
    alpha = torch.randn(n, generator=g, dtype=torch.float64, device="cuda")
    prior = torch.randn(S, generator=g, dtype=torch.float64, device="cuda").abs() * n
    B, X, a, p = (t.cpu().numpy() for t in (Bp[:, :S], Xp[:, :S], alpha, prior))
    noise = 0.375
    var, mean = _reduce_raw(eng, Bp, Xp, S, alpha, prior, noise)
    q = np.sum(B * X, axis=0)
    q_mag = np.sum(np.abs(B * X), axis=0)
    assert np.all(np.isfinite(var)) and np.all(np.isfinite(mean))    # no NaN pad lane leaked
    assert np.all(np.abs(var - ((p - q) + noise)) <= 1e-12 * (p + q_mag + noise))
    assert np.all(np.abs(mean - B.T @ a) <= 1e-12 * (np.abs(B).T @ np.abs(a)) + 1e-300)
    var2, mean2 = _reduce_raw(eng, Bp, Xp, S, alpha, prior, noise)
    assert np.array_equal(var, var2) and np.array_equal(mean, mean2)  # fixed summation order
    # alpha and mean NULL: the same variances, no mean
    var3, none = _reduce_raw(eng, Bp, Xp, S, None, prior, noise)
    assert none is None and np.array_equal(var, var3)
    # a column permutation permutes the results bit for bit
    perm = torch.from_numpy(np.random.default_rng(S + n).permutation(S)).cuda()
    Bq, Xq = _nan((n, S + 3)), _nan((n, S + 5))
    Bq[:, :S], Xq[:, :S] = Bp[:, :S][:, perm], Xp[:, :S][:, perm]
    var4, mean4 = _reduce_raw(eng, Bq, Xq, S, alpha, prior[perm].contiguous(), noise)
    pn = perm.cpu().numpy()
    assert np.array_equal(var4, var[pn]) and np.array_equal(mean4, mean[pn])


def test_reduce_kernel_without_rows_and_engine_wrapper(world):
    import torch
    eng = world["eng"]
    S = 5
    prior = torch.arange(1.0, S + 1, dtype=torch.float64, device="cuda")
    one = torch.ones(1, dtype=torch.float64, device="cuda")          # (a valid alpha pointer; no row is read)
    empty = torch.zeros((0, S), dtype=torch.float64, device="cuda")
    var, mean = _reduce_raw(eng, empty, empty, S, one, prior, 0.25)
    assert np.array_equal(var, prior.cpu().numpy() + 0.25) and not mean.any()
    # the engine's wrapper: column windows of wider buffers, results into slices
    r = np.random.default_rng(5)
    B, X, a = r.standard_normal((130, 70)), r.standard_normal((130, 70)), r.standard_normal(130)
    Bd, Xd = torch.from_numpy(B).cuda(), torch.from_numpy(X).cuda()
    pr = torch.from_numpy(np.abs(r.standard_normal(70))).cuda()
    var, mean = eng.posterior_reduce(Bd[:, 3:68], Xd[:, 3:68], pr[3:68], torch.from_numpy(a).cuda())
    assert np.all(np.abs(var.cpu().numpy() - (pr[3:68].cpu().numpy() - np.sum(B * X, 0)[3:68]))
                  <= 1e-12 * (pr[3:68].cpu().numpy() + np.sum(np.abs(B * X), 0)[3:68]))
    assert np.all(np.abs(mean.cpu().numpy() - (B.T @ a)[3:68]) <= 1e-12 * (np.abs(B).T @ np.abs(a))[3:68])
    var2, none = eng.posterior_reduce(Bd[:, 3:68], Xd[:, 3:68], pr[3:68])
    assert none is None and torch.equal(var, var2)
    with pytest.raises(NotImplementedError):
        z = torch.zeros((4, 257), dtype=torch.float64, device="cuda")
        eng.posterior_reduce(z, z, torch.zeros(257, dtype=torch.float64, device="cuda"))


# ------------------------------------------------------------------------------------ 2. the rhs kernel
def _rows_matrix():
    """A 40 x 260 Phi with rows of 0, 1, 63, 64, 65 and 200 entries among ordinary ones (fp32 values)."""
    r = np.random.default_rng(8)
    n_rows, n_cols = 40, 260
    lens = list(r.integers(2, 30, n_rows))
    lens[:6] = [0, 1, 63, 64, 65, 200]
    rows = []
    for ln in lens:
        row = np.zeros(n_cols)
        row[np.sort(r.permutation(n_cols)[:ln])] = r.standard_normal(ln).astype(np.float32)
        rows.append(row)
    M = sp.csr_matrix(np.array(rows))
    assert list(np.diff(M.indptr)) == lens
    return M


@pytest.mark.parametrize("S", [1, 64, 65, 256])
def test_rhs_kernel(world, S):
    import torch
    from grf_amd.engine import DeviceCSR, _p
    eng = world["eng"]
    M = _rows_matrix()
    n_rows, n_cols = M.shape
    dev = DeviceCSR(n_rows, n_cols, torch.from_numpy(M.indptr.astype(np.int64)).cuda(),
                    torch.from_numpy(M.indices.astype(np.int32)).cuda(), None,
                    torch.from_numpy(M.data.astype(np.float32)).cuda(), int(M.nnz))
    r = np.random.default_rng(S)
    nodes = r.integers(0, n_rows, S)
    nodes[0] = 1                                                     # the row with a single entry
    if S >= 64:
        nodes[1:7] = [0, 2, 3, 4, 5, 1]                              # every special row; node 1 repeated
        nodes[40] = nodes[20]
    lde = S + 3
    Ebuf, prior = _nan((n_cols * lde + 64,)), _nan((S + 8,))
    nd = torch.from_numpy(nodes.astype(np.int32)).cuda()
    rc = eng.lib.grf_posterior_rhs_f64(n_rows, _p(dev.ptr), _p(dev.idx), _p(dev.val32), n_cols, _p(nd), S, _p(Ebuf),
                                       lde, _p(prior), eng.stream)
    torch.cuda.synchronize()
    assert rc == 0, eng.lib.grf_last_error()
    out = Ebuf.cpu().numpy()
    body = out[:n_cols * lde].reshape(n_cols, lde)
    assert np.isnan(body[:, S:]).all() and np.isnan(out[n_cols * lde:]).all(), "wrote outside the pitch window"
    assert np.isnan(prior[S:].cpu().numpy()).all()
    D = M.toarray()
    assert np.array_equal(body[:, :S], D[nodes].T)                   # exact, zeros included
    got = prior[:S].cpu().numpy()
    sq = D[nodes] ** 2
    assert np.all(np.abs(got - sq.sum(1)) <= np.diff(M.indptr)[nodes] * U53 * sq.sum(1))
    assert got[0] == D[1].max() ** 2 or got[0] == D[1].min() ** 2    # the single entry's square, exactly
    # the engine's wrapper gives the same bits
    E2, p2 = eng.posterior_rhs(dev, nd)
    assert np.array_equal(E2.cpu().numpy(), body[:, :S]) and np.array_equal(p2.cpu().numpy(), got)


def test_rhs_kernel_on_the_walks_phi(world):
    import torch
    eng, phi, P = world["eng"], world["phi"], world["P"]
    nodes = np.random.default_rng(2).integers(0, N, 65)
    E, prior = eng.posterior_rhs(phi, torch.from_numpy(nodes))
    D = P.toarray()
    assert np.array_equal(E.cpu().numpy(), D[nodes].T)
    sq = D[nodes] ** 2
    assert np.all(np.abs(prior.cpu().numpy() - sq.sum(1)) <= np.diff(P.indptr)[nodes] * U53 * sq.sum(1))


# ------------------------------------------------------------------------------------ 3. engine
def _nodes(n_train, n_test, seed):
    """Sorted training nodes, test nodes that include training nodes and repeats, targets."""
    r = np.random.default_rng(seed)
    train = np.sort(r.permutation(N)[:n_train])
    test = r.integers(0, N, n_test)
    if n_test >= 1:
        test[0] = train[0]
    if n_test >= 65:
        test[7] = test[6]
        test[8:8 + min(n_train, 12)] = train[:12]
        test[-1] = test[0]
    return train, test, r.standard_normal(n_train)


NOISE = 0.1
_cases = {}


def _case(world, path, n_train, n_test):
    """Truth, and the restatement at the stall tolerance with its own errors (computed once, left unchanged)."""
    key = (path, n_train, n_test)
    if key not in _cases:
        train, test, y = _nodes(n_train, n_test, 31 * n_train + n_test)
        P = world["P"] if path == "csr" else world["Pop"]
        full = n_test == 65
        tru = R.dense_truth(P, train, test, y, NOISE)
        est = R.moments(P, train, test, y, NOISE, tolerance=1e-12, max_iter=max(n_train, 48), full_cov=full)
        err = R.errors(est, tru, full)
        tol = {q: max(10.0 * e, 1e-12) for q, e in err.items()}
        _cases[key] = dict(train=train, test=test, y=y, tru=tru, est=est, err=err, tol=tol, full=full)
    return _cases[key]


def _moments(world, path, c, **kw):
    import torch
    eng = world["eng"]
    phi, f = (world["phi"], None) if path == "csr" else (world["op"], torch.tensor(F, dtype=torch.float64))
    return eng.posterior_moments(phi, torch.from_numpy(c["train"]), torch.from_numpy(c["test"]),
                                 torch.from_numpy(c["y"]), NOISE, f=f, **kw)


@pytest.mark.parametrize("n_test", [0, 1, 65, 257])
@pytest.mark.parametrize("n_train", [1, 64, 200])
@pytest.mark.parametrize("path", ["csr", "operator"])
def test_engine_meets_the_dense_truth(world, path, n_train, n_test):
    """Measured on an MI355X (this test's own printed figures, `pytest -m gpu -s tests/test_gpu_posterior.py`;
    error against the dense truth relative to the largest prior variance, GPU / restatement):
      csr 64/65:        mean 9.0e-7 / 9.7e-7, var 1.0e-9 / 1.0e-9,   cov 1.3e-6 / 1.3e-6
      csr 200/65:       mean 5.9e-8 / 1.5e-7, var 4.2e-12 / 1.9e-12, cov 5.1e-8 / 3.6e-8
      csr 200/257:      mean 5.5e-7 / 2.4e-7, var 3.8e-10 / 3.8e-10
      operator 200/65:  mean 4.4e-5 / 4.4e-5, var 1.1e-10 / 1.1e-10, cov 1.4e-6 / 1.4e-6
      operator 200/257: mean 3.2e-5 / 3.2e-5, var 1.3e-10 / 1.3e-10
    (linear_cg's stall floor, not rounding; n_train = 1 is at 1e-15 on both sides).  The narrowest rows are
    csr 200/65 (var 2.2 x the restatement) and csr 200/257 (mean 2.3 x); the bound is 10 x.  At tolerance 1 (11
    iterations) (var - truth) / prior lies in [4e-10, 2.3e-2] on the csr path and [-4e-16, 2.8e-10] on the operator.
    DESIGN.md section 15 has the full table."""
    import torch
    c = _case(world, path, n_train, n_test)
    info = {}
    mean, var = _moments(world, path, c, tolerance=1e-12, max_iter=max(n_train, 48), info=info)
    assert mean.shape == var.shape == (n_test,) and mean.dtype == var.dtype == torch.float64 and var.is_cuda
    assert len(info["cg_iterations"]) == (n_test + 255) // 256
    if n_test == 0:
        mean, cov = _moments(world, path, c, full_cov=True)
        assert cov.shape == (0, 0) and mean.shape == (0,)
        return
    tru, prior = c["tru"], c["tru"]["prior"]
    got = dict(mean=mean.cpu().numpy(), var=var.cpu().numpy())
    if c["full"]:
        mean_c, cov = _moments(world, path, c, tolerance=1e-12, max_iter=max(n_train, 48), full_cov=True)
        assert cov.shape == (n_test, n_test) and cov.dtype == torch.float64
        assert torch.equal(cov, cov.t()) and torch.equal(mean_c, mean)             # exactly symmetric
        got["cov"] = cov.cpu().numpy()
        assert np.max(np.abs(np.diag(got["cov"]) - got["var"])) <= c["tol"]["var"] * prior.max()
    e = R.errors(got, tru, c["full"])
    for q in e:
        print(f"{path} n={n_train} n*={n_test} {q}: gpu vs truth {e[q]:.3e}  restatement vs truth {c['err'][q]:.3e}  "
              f"tolerance {c['tol'][q]:.3e}")
    for q in e:
        assert e[q] <= c["tol"][q], q
    # repeated test nodes repeat their results
    if n_test >= 65:
        assert got["var"][7] == got["var"][6] and got["mean"][7] == got["mean"][6]
    # stopped at tolerance 1: never below the truth
    info = {}
    mean1, var1 = _moments(world, path, c, tolerance=1.0, info=info)
    slack = (var1.cpu().numpy() - tru["var"]) / prior
    print(f"{path} n={n_train} n*={n_test} tolerance 1: iterations {info['cg_iterations']}  "
          f"(var - truth) / prior in [{slack.min():.3e}, {slack.max():.3e}]")
    assert np.all(var1.cpu().numpy() >= tru["var"] - 1e-12 * prior)
    # add_noise: the same solve, the noise added last
    mean_y, var_y = _moments(world, path, c, tolerance=1.0, add_noise=True)
    assert torch.equal(mean_y, mean1) and torch.equal(var_y, var1 + NOISE)


def test_engine_argument_errors(world):
    import torch
    c = _case(world, "csr", 64, 65)
    with pytest.raises(ValueError):
        world["eng"].posterior_moments(world["op"], torch.from_numpy(c["train"]), torch.from_numpy(c["test"]),
                                       torch.from_numpy(c["y"]), NOISE)                       # no modulator
    with pytest.raises(ValueError):
        world["eng"].posterior_moments(world["phi"], torch.from_numpy(c["train"]), torch.from_numpy(c["test"]),
                                       torch.from_numpy(c["y"][:-1]), NOISE)


# ------------------------------------------------------------------------------------ 4. model
class _Lik:
    noise = NOISE


def _model(world, path, n_train, seed, L=4, steps=None):
    import torch
    from efficient_graph_gp_sparse.models import SparseGraphGP
    train, test, y = _nodes(n_train, 65, seed)
    x_train = torch.tensor(train, dtype=torch.float32, device="cuda").unsqueeze(1)
    y_train = torch.tensor(y, dtype=torch.float32, device="cuda")
    x_test = torch.tensor(test, dtype=torch.float32, device="cuda").unsqueeze(1)
    if steps is None:
        steps = world["ops"] if path == "csr" else world["op"]
    gp = SparseGraphGP(x_train, y_train, _Lik(), steps, L).cuda()
    with torch.no_grad():
        gp.covar_module.raw_modulator_vector.copy_(torch.tensor(F[:L]))
    return gp, train, test, y_train.cpu().numpy().astype(np.float64), x_test


@pytest.mark.parametrize("path", ["csr", "operator"])
def test_model_predict_f_predict_y_and_nlpd(world, path):
    import torch
    gp, train, test, y, x_test = _model(world, path, 200, 77)
    P = world["P"] if path == "csr" else world["Pop"]
    tru = R.dense_truth(P, train, test, y, NOISE)
    # predict is untouched: the same bits for a seeded generator before and after predict_f
    torch.manual_seed(9)
    before = gp.predict(x_test, n_samples=64)
    mean, var = gp.predict_f(x_test)
    assert gp.last_cg_iterations >= 11
    torch.manual_seed(9)
    after = gp.predict(x_test, n_samples=64)
    assert torch.equal(before, after)
    assert mean.dtype == var.dtype == torch.float64 and mean.shape == var.shape == (65,)
    # the default tolerance (eval_cg_tolerance = 1e-2): on the truth's safe side, and within what a solve stopped
    # by that rule can be off by (posterior_reference.stopped_solve_bounds)
    m, v = mean.cpu().numpy(), var.cpu().numpy()
    mean_bound, var_bound = R.stopped_solve_bounds(tru["B"], y, NOISE, 1e-2)
    print(f"{path}: default tolerance, {gp.last_cg_iterations} iterations: max |mean - truth| "
          f"{np.max(np.abs(m - tru['mean'])):.3e} (largest bound {mean_bound.max():.3e}), max (var - truth) / prior "
          f"{np.max((v - tru['var']) / tru['prior']):.3e}")
    # (the variance's quadratic form is the energy form x^T (2 b - K^ x) = b^T K^-1 b - ||x - x_k||^2, below
    # b^T K^-1 b for any x.  b^T x_k alone, which the first version used, differs from it by x_k^T r_k, zero only
    # while CG keeps r_k orthogonal to its Krylov space: on this very case it stopped 1.07e-4 x prior BELOW the
    # truth at node 213.  The floor is the rounding floor, or ten times what the restatement itself dips.)
    slack = (v - tru["var"]) / tru["prior"]
    est = R.moments(P, train, test, y, NOISE, tolerance=1e-2)
    est_slack = (est["var"] - tru["var"]) / tru["prior"]
    floor = min(-1e-12, 10.0 * float(est_slack.min()))
    worst = int(np.argmin(slack))
    print(f"{path}: (var - truth) / prior: gpu min {slack.min():.3e} (node {int(test[worst])}), restatement min "
          f"{est_slack.min():.3e}, floor {floor:.3e}; iterations gpu {gp.last_cg_iterations} restatement {est['iters']}")
    assert np.all(slack >= floor), (worst, slack[worst], v[worst], tru["var"][worst], tru["prior"][worst],
                                    np.sort(slack)[:5], float(est_slack.min()))
    assert np.all(v - tru["var"] <= var_bound + 1e-12 * tru["prior"])
    assert np.all(np.abs(m - tru["mean"]) <= mean_bound + 1e-12 * np.abs(tru["mean"]).max())
    # predict_y: the noise variance added, to the bit
    mean_y, var_y = gp.predict_y(x_test)
    assert torch.equal(mean_y, mean) and torch.equal(var_y, var + NOISE)
    mean_c, cov = gp.predict_f(x_test, full_cov=True)
    mean_cy, cov_y = gp.predict_y(x_test, full_cov=True)
    assert torch.equal(cov, cov.t()) and torch.equal(mean_c, mean) and torch.equal(mean_cy, mean)
    assert torch.equal(cov_y - torch.diag(cov_y.diagonal()), cov - torch.diag(cov.diagonal()))
    assert torch.equal(cov_y.diagonal(), cov.diagonal() + NOISE)
    # |cov_ij - truth| = |b_i^T K^-1 r_j| <= ||b_i|| (S tolerance ||b_j||) / s2, the same for (j, i)
    nb = np.linalg.norm(tru["B"], axis=0)
    assert np.all(np.abs(cov.cpu().numpy() - tru["cov"]) <= 65 * 1e-2 * np.outer(nb, nb) / NOISE
                  + 1e-12 * tru["prior"].max())
    # nlpd: the reference's formula on predict_y's moments
    y_test = torch.from_numpy(np.random.default_rng(4).standard_normal(65)).cuda()
    got = gp.nlpd(x_test, y_test)
    assert got.dtype == torch.float64 and got.dim() == 0
    want = R.nlpd(y_test.cpu().numpy(), mean_y.cpu().numpy(), np.sqrt(var_y.cpu().numpy()))
    assert abs(got.item() - want) <= 1e-13 * abs(want)
    # the pathwise samples' spread agrees with the exact standard deviation: a sample standard deviation of 64
    # draws has the standard error sigma / sqrt(2 * 63)
    # (that is the error of exact posterior draws, so predict's solve is run to its stall here: stopped at its
    # default tolerance of 1, after 11 iterations on the walk's ill-conditioned Phi, its samples' spread was
    # measured 5.9 standard errors off on average; the operator path's 0.7)
    torch.manual_seed(9)
    drawn = gp.predict(x_test, n_samples=64, tolerance=1e-10, max_iter=200).double()
    std = np.sqrt(tru["var"])
    z = np.abs(drawn.std(0).cpu().numpy() - np.sqrt(v)) / (std / np.sqrt(2.0 * 63.0))
    zm = np.abs(drawn.mean(0).cpu().numpy() - m) / (std / 8.0)
    print(f"{path}: sample std vs sqrt(var): mean |z| {z.mean():.2f} max {z.max():.2f};  sample mean: mean |z| "
          f"{zm.mean():.2f}")
    assert z.mean() <= 5.0 and zm.mean() <= 5.0


@pytest.mark.parametrize("path", ["csr", "operator"])
def test_identity_features_closed_form(world, path):
    """max_walk_length = 1: Phi = f0 I."""
    import torch
    f0 = F[0] * 0.75
    steps = world["ops"][:1] if path == "csr" else None
    if path == "operator":
        from grf_amd.engine import WalkPolynomial
        steps = WalkPolynomial(world["op"].G, 1, engine=world["eng"])
    gp, train, test, y, x_test = _model(world, path, 64, 5, L=1, steps=steps)
    with torch.no_grad():
        gp.covar_module.raw_modulator_vector.fill_(f0)
    mean, var = gp.predict_f(x_test, tolerance=1e-12, max_iter=48)
    want_mean, want_var = R.identity_closed_form(f0, NOISE, train, test, y)
    assert np.max(np.abs(var.cpu().numpy() - want_var)) <= 1e-14 * f0 * f0
    assert np.max(np.abs(mean.cpu().numpy() - want_mean)) <= 1e-14 * np.max(np.abs(y))
