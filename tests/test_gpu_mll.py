"""GPU: the matrix-free marginal likelihood -- CG with its Lanczos coefficients
(grf_cg_gram_solve_lanczos_f64), the modulator gradient's contraction (grf_steps_frob_f64), the engine's
value + gradients, the autograd function and SparseGraphGP.marginal_log_likelihood -- against the numpy
restatement (tests/mll_reference.py) and the dense truth computed on the CPU.

The graph has N = 300 nodes of degree ~6; the step matrices come from the engine's own walk (8 walks,
p_halt = 0.2, L = 4).  Phi (pre-existing code: grf_phi_steps_csr) is read back from the device so that
the restatement and the truth see the engine's own fp32 values widened to fp64.

Tolerances
  * coefficients: x and the count bit-identical to the plain solve; alpha / beta of iterations 0..4
    to 1e-10 relative (the bound test_gpu_cg.py uses for early iterates); rows not run are zero.
  * steps_frob: |err| <= 1e-12 * sum |terms| against numpy fp64; a second call gives the same bits.
  * exactness (identity probes, tolerance 1e-12, max_iter 48: every column runs to linear_cg's stall):
    the GPU's relative error against the dense truth <= 10 x the error the CPU restatement itself
    shows against the truth on that case, computed inside the test (the margin covers summation-order
    differences in a recurrence that stops by a threshold); test_exactness's docstring has the measured
    figures.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import mll_reference as R

pytestmark = pytest.mark.gpu

N, F = 300, [1.0, -0.5, 0.25, -0.125]


def _graph(n, deg, seed):
    r = np.random.default_rng(seed)
    m = int(n * deg / 2)
    u, v = r.integers(0, n, m), r.integers(0, n, m)
    keep = u != v
    A = sp.coo_matrix((np.ones(keep.sum()), (u[keep], v[keep])), shape=(n, n)).tocsr()
    A = (A + A.T).tocsr()
    A.data[:] = 1.0
    return A


@pytest.fixture(scope="module")
def world():
    """Engine, the walk's step matrices (device operators + fp32-valued scipy), Phi(F) as scipy."""
    import torch
    from efficient_graph_gp_sparse.preprocessor import GraphPreprocessor
    from grf_amd.engine import GRFEngine
    from grf_amd.features import StepMatrices

    eng = GRFEngine("cuda:0")
    pre = GraphPreprocessor(_graph(N, 6, 11), walks_per_node=8, p_halt=0.2, max_walk_length=4, random_walk_seed=3,
                            use_tqdm=False)
    ops = pre.preprocess_graph()
    mats = [sp.csr_matrix(M.astype(np.float32).astype(np.float64)) for M in pre.step_matrices_scipy]
    assert len(ops) == 4
    steps = StepMatrices(ops, eng)
    f = torch.tensor(F, dtype=torch.float32)
    return dict(eng=eng, ops=ops, mats=mats, steps=steps, f=f, P=_phi_scipy(steps.phi(f)))


def _phi_scipy(phi):
    P = phi.to_scipy().astype(np.float64)
    P.data = phi.val32[:phi.nnz].cpu().numpy().astype(np.float64)
    return P


def _train(n_train, seed):
    r = np.random.default_rng(seed)
    return np.sort(r.permutation(N)[:n_train]), r.standard_normal(n_train)


# ---------------------------------------------------------------- 1. coefficients
@pytest.mark.parametrize("S", [1, 5, 65, 130])
def test_cg_coefficients(world, S):
    import torch
    eng, steps = world["eng"], world["steps"]
    tr, _ = _train(64, 1)
    noise, max_iter = 0.1, 20
    B = np.random.default_rng(S).standard_normal((64, S))
    Bd = torch.from_numpy(B).cuda()
    rows = torch.from_numpy(tr)
    phi = steps.phi(world["f"])
    X0, it0, res0 = eng.cg_solve(phi, Bd, noise, rows, max_iter=max_iter, return_residuals=True)
    X1, it1, res1, coef = eng.cg_solve(phi, Bd, noise, rows, max_iter=max_iter, return_residuals=True,
                                       return_lanczos=True)
    assert it0 == it1 == 11 and torch.equal(X0, X1) and np.array_equal(res0, res1)
    assert coef.shape == (2 * max_iter, S) and coef.dtype == torch.float64
    coef = coef.cpu().numpy()
    al, be = coef[:max_iter], coef[max_iter:]
    assert not al[it1:].any() and not be[it1:].any()
    assert al[:5].all() and be[:5].all()
    Pt = world["P"][tr]
    _, k, ral, rbe = R.cg_lanczos(R._khat_matmul(Pt, noise), B, max_iter=max_iter)
    assert k == it1
    for i in range(5):
        assert np.abs(al[i] - ral[i]).max() <= 1e-10 * np.abs(ral[i]).max(), i
        assert np.abs(be[i] - rbe[i]).max() <= 1e-10 * np.abs(rbe[i]).max(), i
    # the plain entry points are untouched by a solve that recorded coefficients before them
    X2, it2 = eng.cg_solve(phi, Bd, noise, rows, max_iter=max_iter)
    assert it2 == it1 and torch.equal(X2, X1)
    with pytest.raises(ValueError):
        eng.cg_solve(phi, Bd.float(), noise, rows, max_iter=3, return_lanczos=True)


# ---------------------------------------------------------------- 2. steps_frob
def _frob_reference(mats, rows, A, WA, B, WB, wt):
    out, bound = np.zeros(len(mats)), np.zeros(len(mats))
    for l, M in enumerate(mats):
        Mr = M if rows is None else M[rows]
        out[l] = np.sum(wt * (A * (Mr @ WB) + B * (Mr @ WA)))
        bound[l] = np.sum(np.abs(wt) * (np.abs(A) * (abs(Mr) @ np.abs(WB)) + np.abs(B) * (abs(Mr) @ np.abs(WA))))
    return out, bound


def _frob_case(world, steps, mats, rows, n_sel, S, L, seed):
    import torch
    eng = world["eng"]
    r = np.random.default_rng(seed)
    A, B = r.standard_normal((n_sel, S)), r.standard_normal((n_sel, S))
    WA, WB = r.standard_normal((N, S)), r.standard_normal((N, S))
    wt = r.standard_normal(S)
    dev = [torch.from_numpy(x).cuda() for x in (A, WA, B, WB, wt)]
    rt = None if rows is None else torch.from_numpy(rows)
    out = eng.steps_frob(steps, rt, *dev, n_steps=L)
    assert out.shape == (L,) and out.dtype == torch.float64 and out.is_cuda
    want, bound = _frob_reference(mats[:L], rows, A, WA, B, WB, wt)
    got = out.cpu().numpy()
    assert np.all(np.abs(got - want) <= 1e-12 * bound + 1e-300), (got, want, bound)
    again = eng.steps_frob(steps, rt, *dev, n_steps=L)
    assert torch.equal(out, again)                                   # fixed summation order


@pytest.mark.parametrize("S", [1, 5, 65, 130, 256])
@pytest.mark.parametrize("n_sel", [1, 3, 64, 257])
def test_steps_frob_vs_numpy(world, n_sel, S):
    r = np.random.default_rng(1000 * n_sel + S)
    rows = r.integers(0, N, n_sel)
    if n_sel >= 3:
        rows[2] = rows[0]                                            # a repeated row
    for L in (1, 4):
        _frob_case(world, world["steps"], world["mats"], rows, n_sel, S, L, S + n_sel + L)


def test_steps_frob_identity_map_and_empty_rows(world):
    import torch
    from efficient_graph_gp_sparse.preprocessor import GraphPreprocessor
    from grf_amd.features import StepMatrices
    # NULL row map: all N rows in order
    _frob_case(world, world["steps"], world["mats"], None, N, 65, 4, 5)
    # step matrices with empty rows (every third row of every step, and the whole of step 2)
    mats = []
    for l, M in enumerate(world["mats"]):
        M = M.tolil(copy=True)
        for r in range(0, N, 3):
            M.rows[r], M.data[r] = [], []
        M = sp.csr_matrix(M)
        mats.append(sp.csr_matrix((N, N)) if l == 2 else M)
    steps = StepMatrices([GraphPreprocessor.from_scipy_csr(M).cuda() for M in mats], world["eng"])
    rows = np.random.default_rng(3).integers(0, N, 64)
    rows[:4] = [0, 3, 3, 1]
    _frob_case(world, steps, mats, rows, 64, 5, 4, 6)
    _frob_case(world, steps, mats, None, N, 130, 4, 7)
    # a single-step set
    one = StepMatrices(world["ops"][:1], world["eng"])
    _frob_case(world, one, world["mats"][:1], rows, 64, 65, 1, 8)
    z = torch.zeros((0, 5), dtype=torch.float64, device="cuda")
    w = torch.zeros((N, 5), dtype=torch.float64, device="cuda")
    out = world["eng"].steps_frob(world["steps"], torch.empty(0, dtype=torch.int32), z, w, z, w,
                                  torch.ones(5, dtype=torch.float64))
    assert not out.cpu().numpy().any()


def test_steps_frob_too_many_columns(world):
    import torch
    a = torch.zeros((4, 257), dtype=torch.float64, device="cuda")
    w = torch.zeros((N, 257), dtype=torch.float64, device="cuda")
    with pytest.raises(NotImplementedError):
        world["eng"].steps_frob(world["steps"], torch.arange(4), a, w, a, w, torch.ones(257, dtype=torch.float64))


# ---------------------------------------------------------------- 3. exactness
def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))) / np.max(np.abs(b)))


_cases = {}


def _exact_case(world, n_train, noise):
    """Restatement and dense truth with identity probes (computed once per case, left unchanged)."""
    key = (n_train, noise)
    if key not in _cases:
        tr, y = _train(n_train, 7 + n_train)
        Pt = world["P"][tr]
        Ms = [M[tr] for M in world["mats"]]
        Z = R.identity_probes(n_train)
        est = R.estimate(Pt, Ms, y, noise, Z, tolerance=1e-12, max_iter=48)
        tru = R.dense_truth(Pt, Ms, y, noise)
        tol = {q: 10.0 * _rel(est[q], tru[q]) for q in ("value", "grad_f", "grad_noise")}
        # the floor on the value (see test_exactness)
        tol["value"] = max(tol["value"], VALUE_FLOOR)
        _cases[key] = dict(tr=tr, y=y, Pt=Pt, Ms=Ms, Z=Z, est=est, tru=tru, tol=tol)
    return _cases[key]


# relative floor of the value's tolerance; see test_exactness's docstring (0: none needed)
VALUE_FLOOR = 0.0


def _gpu_mll(world, c, noise, Z, tolerance=1e-12, max_iter=48):
    import torch
    value, g_f, g_noise, iters = world["eng"].marginal_log_likelihood(
        world["steps"], world["f"], torch.from_numpy(c["tr"]), torch.from_numpy(c["y"]), noise,
        torch.from_numpy(np.ascontiguousarray(Z)).cuda(), tolerance, max_iter)
    return dict(value=value, grad_f=g_f.cpu().numpy(), grad_noise=g_noise, iters=iters)


@pytest.mark.parametrize("noise", [0.05, 1.0])
@pytest.mark.parametrize("n_train", [64, 128])
def test_exactness(world, n_train, noise):
    """Identity probes Z = sqrt(n) I: Hutchinson's traces are exact and SLQ is exact once Lanczos has run
    out, so value, d/df and d/ds2 must meet the dense truth as closely as the CPU restatement does (x 10).

    Measured on an MI355X (this test's own printed figures: `pytest -m gpu -s tests/test_gpu_mll.py`), relative
    error against the dense truth, GPU / CPU restatement:
      n = 64,  s2 = 0.05: value 6.8e-08 / 1.1e-07, d/df 2.6e-04 / 2.6e-04, d/ds2 1.3e-07 / 2.2e-07
      n = 64,  s2 = 1.0:  value 2.3e-10 / 1.6e-10, d/df 7.1e-08 / 1.0e-07, d/ds2 1.8e-10 / 5.8e-10
      n = 128, s2 = 0.05: value 2.0e-06 / 2.3e-06, d/df 3.3e-04 / 5.8e-05, d/ds2 1.5e-06 / 2.5e-06
      n = 128, s2 = 1.0:  value 2.6e-12 / 1.3e-10, d/df 1.2e-07 / 2.0e-07, d/ds2 5.3e-11 / 4.6e-10
    (linear_cg's stall floor on the walk's Phi, not rounding).  The restatement's value error is nowhere
    near 1e-12 on these systems and the GPU stays within its tenfold everywhere, so the relative floor the
    value would get in that event (4 x the GPU error measured against the truth) is not needed:
    VALUE_FLOOR stays 0.  One row has little margin: d/df at n = 128, s2 = 0.05, where the GPU is 5.7 x the
    restatement (bound 10 x); everywhere else it is at or below it.  The cause was not isolated; the likely
    one is a column whose `p.Ap < 1e-10` guard fires one iteration earlier under the GPU's summation
    order, which leaves that column's solution at a residual near 1e-5 instead of below it.  On the
    noise-0.05 systems (the ill-conditioned ones: the walk's Phi with 8 walks) linear_cg's stall floor
    itself puts the restatement 6e-5 to 3e-4 from the truth, so the tenfold bound there is loose in
    absolute terms (up to 2.6e-3); the noise-1.0 cases hold d/df to 1e-6 and 2e-6."""
    c = _exact_case(world, n_train, noise)
    got = _gpu_mll(world, c, noise, c["Z"])
    assert got["iters"] == c["est"]["iters"] == 48
    for q in ("value", "grad_f", "grad_noise"):
        e_gpu, e_cpu = _rel(got[q], c["tru"][q]), _rel(c["est"][q], c["tru"][q])
        print(f"exactness n={n_train} s2={noise} {q}: gpu vs truth {e_gpu:.3e}  restatement vs truth {e_cpu:.3e}  "
              f"tolerance {c['tol'][q]:.3e}")
    for q in ("value", "grad_f", "grad_noise"):
        assert _rel(got[q], c["tru"][q]) <= c["tol"][q], q


# ---------------------------------------------------------------- 4. random probes
def test_random_probes_match_restatement_and_repeat(world):
    import torch
    from grf_amd.features import grf_marginal_log_likelihood
    n_train, noise = 64, 0.05
    c = _exact_case(world, n_train, noise)
    Z = torch.randn(n_train, 7, generator=torch.Generator().manual_seed(5))
    est = R.estimate(c["Pt"], c["Ms"], c["y"], noise, Z.numpy().astype(np.float64), tolerance=1e-12, max_iter=48)
    got = _gpu_mll(world, c, noise, Z.numpy().astype(np.float64))
    for q in ("value", "grad_f", "grad_noise"):
        e = _rel(got[q], est[q])
        print(f"random probes {q}: gpu vs restatement {e:.3e}  tolerance {c['tol'][q]:.3e}")
    for q in ("value", "grad_f", "grad_noise"):
        assert _rel(got[q], est[q]) <= c["tol"][q], q

    def run():
        f = world["f"].clone().requires_grad_(True)
        s2 = torch.tensor([noise], dtype=torch.float64, requires_grad=True)
        v = grf_marginal_log_likelihood(f, s2, world["steps"], torch.from_numpy(c["tr"]), torch.from_numpy(c["y"]),
                                        n_probes=7, generator=torch.Generator().manual_seed(5), tolerance=1e-12,
                                        max_iter=48, per_datum=False)
        v.backward()
        return v.detach(), f.grad, s2.grad

    a, b = run(), run()
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    # the wrapper drew the same probes: the same numbers as the engine call above (f's gradient in f's fp32)
    assert a[0].item() == got["value"] and a[2].item() == got["grad_noise"]
    assert np.array_equal(a[1].numpy(), got["grad_f"].astype(np.float32))
    v = grf_marginal_log_likelihood(world["f"], noise, world["steps"], torch.from_numpy(c["tr"]),
                                    torch.from_numpy(c["y"]), probes=Z, tolerance=1e-12, max_iter=48)
    assert v.item() == got["value"] / n_train                        # per_datum (the default)


# ---------------------------------------------------------------- 5. model
class _Likelihood:
    def __init__(self, raw):
        self.raw_noise = raw

    @property
    def noise(self):
        import torch
        return torch.nn.functional.softplus(self.raw_noise)


def test_model_training_raises_the_true_mll(world):
    import torch
    from efficient_graph_gp_sparse.models import SparseGraphGP
    n_train = 64
    tr, y = _train(n_train, 21)
    x_train = torch.tensor(tr, dtype=torch.float32, device="cuda").unsqueeze(1)
    y_train = torch.tensor(y, dtype=torch.float32, device="cuda")
    raw = torch.tensor([-1.0], dtype=torch.float64, requires_grad=True)
    torch.manual_seed(4)
    gp = SparseGraphGP(x_train, y_train, _Likelihood(raw), world["ops"], 4).cuda()
    Z = torch.from_numpy(R.identity_probes(n_train))

    def truth():
        P = _phi_scipy(gp._phi_csr(world["eng"].device))
        Ms = [M[tr] for M in world["mats"]]
        s2 = float(torch.nn.functional.softplus(raw).item())
        return R.dense_truth(P[tr], Ms, y_train.cpu().numpy().astype(np.float64), s2)

    t0 = truth()
    mll = gp.marginal_log_likelihood(probes=Z, tolerance=1e-6)
    assert mll.dim() == 0 and mll.dtype == torch.float64
    mll.backward()
    assert gp.last_cg_iterations >= 11
    gf, gn = gp.covar_module.raw_modulator_vector.grad, raw.grad
    assert gf is not None and gf.shape == (4,) and torch.isfinite(gf).all() and gf.abs().max() > 0
    assert gn is not None and torch.isfinite(gn).all() and gn.abs().max() > 0
    # per datum, against the dense truth (CG run to 1e-6: a loose check that the pieces are the right ones)
    assert abs(mll.item() - t0["value"] / n_train) <= 1e-3 * abs(t0["value"] / n_train)
    assert _rel(gf.cpu().numpy() * n_train, t0["grad_f"]) <= 1e-2
    opt = torch.optim.Adam([gp.covar_module.raw_modulator_vector, raw], lr=0.05)
    for _ in range(20):
        opt.zero_grad()
        loss = -gp.marginal_log_likelihood(probes=Z, tolerance=1e-2)
        loss.backward()
        opt.step()
    t1 = truth()
    print(f"dense-truth MLL before {t0['value']:.4f} after 20 Adam steps {t1['value']:.4f}")
    assert t1["value"] > t0["value"]
    # a float noise is a constant: only the modulator gets a gradient
    class Fixed:
        noise = 0.1
    gp2 = SparseGraphGP(x_train, y_train, Fixed(), world["ops"], 4).cuda()
    gp2.marginal_log_likelihood(n_probes=7, generator=torch.Generator().manual_seed(1)).backward()
    assert torch.isfinite(gp2.covar_module.raw_modulator_vector.grad).all()


# ---------------------------------------------------------------- 6. argument errors
def test_argument_errors(world):
    import torch
    from grf_amd.features import grf_marginal_log_likelihood
    tr, y = _train(64, 1)
    args = (world["f"], 0.1, world["steps"], torch.from_numpy(tr), torch.from_numpy(y))
    with pytest.raises(ValueError):
        grf_marginal_log_likelihood(*args, probes=torch.zeros(64, 256))
    with pytest.raises(ValueError):
        grf_marginal_log_likelihood(*args, n_probes=256)
    with pytest.raises(ValueError):
        grf_marginal_log_likelihood(*args, probes=torch.zeros(63, 7))
    with pytest.raises(ValueError):
        grf_marginal_log_likelihood(*args, probes=torch.zeros(64))
    with pytest.raises(ValueError):
        world["eng"].marginal_log_likelihood(world["steps"], world["f"], torch.from_numpy(tr), torch.from_numpy(y),
                                             0.1, torch.zeros(64, 256), 1.0, 10)
