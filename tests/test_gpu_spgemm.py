"""GPU: the device SpGEMM (grf_spgemm_csr_count / _fill, csrc/grf_spgemm.hip) through the C ABI at edge
shapes, ``GRFEngine.spgemm`` / ``exact_steps``, and the surfaces built on the exact step matrices
(``GraphPreprocessor(exact=True)`` into SparseGRFKernel and SparseGraphGP, the two PoFM mirrors).

The kernel is held to the bit against the numpy restatement of its rule (tests/spgemm_reference.py, pinned
against scipy on the CPU by tests/test_spgemm_reference.py): row pointers and columns exact, the bits of
c_val and c_val32 identical.  Output buffers carry SLACK extra entries and are pre-filled with sentinels /
NaN: nothing may be written past c_ptr[-1].  The cases put A rows of 0 ... 200 entries over B rows of
0 ... 1000 entries, rows whose product count and distinct-column count sit at GRF_SPGEMM_SORT_PRODUCTS and
GRF_SPGEMM_ACC_SLOTS - 1 / + 0 / + 1, a hub row of ~48 000 distinct columns at n_cols = 70 000, full and no
overlap, integer-valued cancelling inputs (stored +0.0, -0.0 products), n_cols = 2^31 - 1 with more large
rows than the big path's smallest wave count, rectangular shapes throughout and n_rows in {1, 5, 257}.

Tolerances of the surfaces (none measured): the exact chain against tests/golden/pstep.npz within
2 ((1 + gamma_n)^l - 1) (|L|^l)_ij; K and diag of SparseGRFKernel within DESIGN.md section 2's
3e-5 (|Phi||Phi|^T)_ij + 1e-12 rowmax_i max|Phi|; the marginal likelihood within 10 x the CPU restatement's own
error against the dense truth (tests/test_gpu_mll.py's rule) and the model's value / gradient within its 1e-3 /
1e-2; predict within test_gpu_cg.py's 1e-5 at 3 CG iterations; the PoFM mirrors within rtol 3e-5, atol 1e-6
(K, K_diag) and rtol 1e-4, atol 1e-6 (modulator gradient), what tests/test_gpu_api.py holds
GraphGeneralFastGRFKernel to.

Measured on an MI355X (information, not asserted; the likelihood test prints its own): every product case bit-equal;
the marginal likelihood's relative error against the dense truth, GPU and restatement alike to the digits printed,
value 4.8e-11 / 4.4e-12, d/df 7.9e-08 / 8.8e-08, d/ds2 2.1e-09 / 3.5e-10 at s2 = 0.05 / 1.0 (48 iterations both).
The whole file runs in under 5 s, its slowest test (the PoFM mirrors on the 4-node graph, first use of the
dense kernels) in 0.8 s.
"""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import mll_reference as MR
import spgemm_reference as R
from golden_util import csr
from oracle import cg as OCG

pytestmark = pytest.mark.gpu

SLACK, SENT_I = 11, -77
NULL = ctypes.c_void_p(0)


@pytest.fixture(scope="module")
def eng():
    from grf_amd.engine import GRFEngine
    return GRFEngine("cuda:0")


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _thresholds():
    from grf_amd import _lib
    return (_lib.SPGEMM_SORT_PRODUCTS, _lib.SPGEMM_ACC_SLOTS)


CASES = {
    "mixed1": lambda: R.case_mixed(1),
    "mixed5": lambda: R.case_mixed(5),
    "mixed257": lambda: R.case_mixed(257),
    "thresholds": lambda: R.case_thresholds(_thresholds())[:2],
    "hub": R.case_hub,
    "full_overlap": R.case_full_overlap,
    "no_overlap": R.case_no_overlap,
    "cancelling": R.case_cancelling,
    "wide": R.case_wide,
}
_refs = {}


def _case(name):
    """(A, B, restatement's C), computed once and left unchanged."""
    if name not in _refs:
        A, B = CASES[name]()
        _refs[name] = (A, B, R.spgemm(A, B))
    return _refs[name]


def _device_product(eng, A, B, want32=True, ws_short=0):
    """count -> grf_scan_counts -> fill through the C ABI, output buffers with SLACK sentinel entries.
    Returns (status of count, status of fill, ptr, idx, val, val32) with the whole buffers as numpy."""
    lib = eng.lib
    n, n_mid, n_cols = A.shape[0], A.shape[1], B.shape[1]
    ap, ai, av = _dev(A.indptr, np.int64), _dev(A.indices, np.int32), _dev(A.data, np.float64)
    bp, bi, bv = _dev(B.indptr, np.int64), _dev(B.indices, np.int32), _dev(B.data, np.float64)
    need = lib.grf_spgemm_workspace_bytes(n, n_mid, n_cols)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    cnt = torch.full((n + SLACK,), SENT_I, dtype=torch.int32, device="cuda")
    rc_count = lib.grf_spgemm_csr_count(n, n_mid, n_cols, _p(ap), _p(ai), _p(bp), _p(bi), _p(cnt), _p(ws),
                                        need - ws_short, eng.stream)
    if rc_count != 0:
        torch.cuda.synchronize()
        return rc_count, None, cnt.cpu().numpy(), None, None, None
    assert np.all(cnt[n:].cpu().numpy() == SENT_I)
    ptr = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    sws = torch.empty(max(lib.grf_scan_workspace_bytes(n), 16), dtype=torch.uint8, device="cuda")
    assert lib.grf_scan_counts(n, _p(cnt), _p(ptr), _p(sws), sws.numel(), eng.stream) == 0
    nnz = int(ptr[-1].item())
    idx = torch.full((nnz + SLACK,), SENT_I, dtype=torch.int32, device="cuda")
    val = torch.full((nnz + SLACK,), float("nan"), dtype=torch.float64, device="cuda")
    val32 = torch.full((nnz + SLACK,), float("nan"), dtype=torch.float32, device="cuda")
    rc_fill = lib.grf_spgemm_csr_fill(n, n_mid, n_cols, _p(ap), _p(ai), _p(av), _p(bp), _p(bi), _p(bv), _p(ptr),
                                      _p(idx), _p(val), _p(val32) if want32 else NULL, _p(ws), need, eng.stream)
    torch.cuda.synchronize()
    return rc_count, rc_fill, ptr.cpu().numpy(), idx.cpu().numpy(), val.cpu().numpy(), val32.cpu().numpy()


def _assert_equal_to(ref, ptr, idx, val, val32, want32=True):
    nnz = ref.nnz
    assert np.array_equal(ptr, np.asarray(ref.indptr, np.int64))
    assert np.array_equal(idx[:nnz], np.asarray(ref.indices, np.int32))
    assert np.array_equal(val[:nnz].view(np.uint64), ref.data.view(np.uint64))
    # nothing past c_ptr[-1]
    assert len(idx) == nnz + SLACK and np.all(idx[nnz:] == SENT_I)
    assert np.isnan(val[nnz:]).all() and np.isnan(val32[nnz:]).all()
    if want32:
        assert np.array_equal(val32[:nnz].view(np.uint32), ref.data.astype(np.float32).view(np.uint32))
    else:
        assert np.isnan(val32).all()


@pytest.mark.parametrize("name", sorted(CASES))
def test_product_is_the_restatement_to_the_bit(eng, name):
    A, B, ref = _case(name)
    rc_count, rc_fill, ptr, idx, val, val32 = _device_product(eng, A, B)
    assert rc_count == 0 and rc_fill == 0, eng.lib.grf_last_error()
    _assert_equal_to(ref, ptr, idx, val, val32)


def test_case_shapes_are_what_the_names_say():
    from grf_amd import _lib
    A, B, want = R.case_thresholds(_thresholds())
    assert sorted({c for _, c in want}) == sorted(t + d for t in _thresholds() for d in (-1, 0, 1))
    ref = _case("thresholds")[2]
    for r, (what, count) in enumerate(want):
        if what == "distinct":
            assert ref.indptr[r + 1] - ref.indptr[r] == count
    A, B, ref = _case("hub")
    assert B.shape[1] == 70000 and np.diff(ref.indptr).max() > 8 * _lib.SPGEMM_ACC_SLOTS
    A, B, ref = _case("no_overlap")
    products = np.array([sum(B.indptr[k + 1] - B.indptr[k] for k in A.indices[A.indptr[r]:A.indptr[r + 1]])
                         for r in range(A.shape[0])])
    assert np.array_equal(products, np.diff(ref.indptr)) and products.max() > _lib.SPGEMM_ACC_SLOTS
    A, B, ref = _case("full_overlap")
    assert set(np.diff(ref.indptr)) == {0, 64}
    A, B, ref = _case("cancelling")
    zero = ref.data == 0.0
    assert zero.any() and not np.signbit(ref.data[zero]).any()
    A, B, ref = _case("wide")
    assert B.shape[1] == 2 ** 31 - 1
    big = sum(1 for r in range(A.shape[0])
              if sum(B.indptr[k + 1] - B.indptr[k] for k in A.indices[A.indptr[r]:A.indptr[r + 1]])
              > _lib.SPGEMM_SORT_PRODUCTS)
    assert big > _lib.SPGEMM_BIG_MIN_WAVES


def test_null_val32_and_a_second_call_gives_the_same_bits(eng):
    A, B, ref = _case("mixed5")
    rc_count, rc_fill, ptr, idx, val, val32 = _device_product(eng, A, B, want32=False)
    assert rc_count == 0 and rc_fill == 0
    _assert_equal_to(ref, ptr, idx, val, val32, want32=False)
    A, B, ref = _case("mixed257")
    first = _device_product(eng, A, B)
    again = _device_product(eng, A, B)
    for x, y in zip(first[2:], again[2:]):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))


def test_workspace_one_byte_short_launches_nothing(eng):
    from grf_amd import _lib
    A, B, _ = _case("mixed5")
    rc, _, cnt, *_ = _device_product(eng, A, B, ws_short=1)
    assert rc == _lib.GRF_EINVAL and b"workspace" in eng.lib.grf_last_error()
    assert np.all(cnt == SENT_I)  # the count buffer is untouched
    # the fill pass: the same check, its outputs untouched
    n, n_mid, n_cols = A.shape[0], A.shape[1], B.shape[1]
    need = eng.lib.grf_spgemm_workspace_bytes(n, n_mid, n_cols)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    ap, ai, av = _dev(A.indptr, np.int64), _dev(A.indices, np.int32), _dev(A.data, np.float64)
    bp, bi, bv = _dev(B.indptr, np.int64), _dev(B.indices, np.int32), _dev(B.data, np.float64)
    ref = _case("mixed5")[2]
    ptr = _dev(ref.indptr, np.int64)
    idx = torch.full((ref.nnz,), SENT_I, dtype=torch.int32, device="cuda")
    val = torch.full((ref.nnz,), float("nan"), dtype=torch.float64, device="cuda")
    rc = eng.lib.grf_spgemm_csr_fill(n, n_mid, n_cols, _p(ap), _p(ai), _p(av), _p(bp), _p(bi), _p(bv), _p(ptr), _p(idx),
                                     _p(val), NULL, _p(ws), need - 1, eng.stream)
    torch.cuda.synchronize()
    assert rc == _lib.GRF_EINVAL
    assert bool((idx == SENT_I).all()) and bool(torch.isnan(val).all())


# ------------------------------------------------------------------------------------ engine level
def _same_device_csr(M, ref):
    nnz = ref.nnz
    assert M.nnz == nnz and (M.n_rows, M.n_cols) == ref.shape
    assert np.array_equal(M.ptr.cpu().numpy(), np.asarray(ref.indptr, np.int64))
    assert np.array_equal(M.idx[:nnz].cpu().numpy(), np.asarray(ref.indices, np.int32))
    assert np.array_equal(M.val[:nnz].cpu().numpy().view(np.uint64), ref.data.view(np.uint64))
    assert np.array_equal(M.val32[:nnz].cpu().numpy().view(np.uint32),
                          ref.data.astype(np.float32).view(np.uint32))


def test_engine_spgemm_rectangular(eng):
    from grf_amd.engine import DeviceCSR
    A, B, ref = _case("mixed5")
    C = eng.spgemm(DeviceCSR.from_scipy(A, eng.device), DeviceCSR.from_scipy(B, eng.device))
    _same_device_csr(C, ref)
    with pytest.raises(ValueError):
        eng.spgemm(DeviceCSR.from_scipy(B, eng.device), DeviceCSR.from_scipy(A, eng.device))


@pytest.mark.parametrize("graph", ["grid12", "er40", "iso25"])
def test_exact_steps_chain(eng, golden, graph):
    d, sg = golden("pstep"), golden("small_graphs")
    A = R.grid_adjacency(12, 12) if graph == "grid12" else sp.csr_matrix(sg[f"{graph}_A"])
    if graph == "iso25":
        assert (np.asarray(A.sum(axis=1)).ravel() == 0).any()  # the isolated node
    A.sort_indices()
    G = eng.laplacian(A)
    Ls = G.to_scipy()
    steps = eng.exact_steps(G, 5)
    ref = R.exact_steps(Ls, 5)
    assert len(steps) == 5
    for M, want in zip(steps, ref):
        _same_device_csr(M, want)
    if graph != "grid12":
        n = A.shape[0]
        Lfix = csr(sg, f"{graph}_Lsp", n)
        assert np.array_equal(Ls.toarray(), Lfix.toarray())
        T = d[f"{graph}_pstep"]
        for l, M in enumerate(steps):
            err = np.abs(M.to_scipy().toarray() - T[:, :, l])
            bound = R.chain_bound(Lfix.toarray(), l) if l else np.zeros((n, n))
            assert np.all(err <= bound), (graph, l)
    # max_nnz one below a power's nnz: refused before that power is allocated, naming the step and the nnz
    sizes = [M.nnz for M in ref]
    top = int(np.argmax(sizes))  # (the first step with the most entries: every earlier one fits)
    assert top >= 2
    with pytest.raises(ValueError, match=rf"step {top} .*{sizes[top]}"):
        eng.exact_steps(G, 5, max_nnz=sizes[top] - 1)
    assert len(eng.exact_steps(G, 5, max_nnz=sizes[top])) == 5


# ---------------------------------------------------------------------------------------- surfaces
def _graph(n, deg, seed):
    r = np.random.default_rng(seed)
    m = int(n * deg / 2)
    u, v = r.integers(0, n, m), r.integers(0, n, m)
    keep = u != v
    A = sp.coo_matrix((np.ones(keep.sum()), (u[keep], v[keep])), shape=(n, n)).tocsr()
    A = (A + A.T).tocsr()
    A.data[:] = 1.0
    A.sort_indices()
    return A


N = 300


@pytest.fixture(scope="module")
def world(eng):
    """The exact step matrices of a 300-node graph through GraphPreprocessor(exact=True)."""
    from efficient_graph_gp_sparse.preprocessor import GraphPreprocessor
    A = _graph(N, 6, 11)
    pre = GraphPreprocessor(A, walks_per_node=3, p_halt=0.9, max_walk_length=4, random_walk_seed=1, use_tqdm=False,
                            exact=True)
    ops = pre.preprocess_graph()
    mats64 = pre.step_matrices_scipy
    mats = [sp.csr_matrix(M.astype(np.float32).astype(np.float64)) for M in mats64]  # the operators' fp32 values
    return dict(A=A, pre=pre, ops=ops, mats64=mats64, mats=mats)


def test_preprocessor_exact_steps(eng, world):
    from efficient_graph_gp_sparse.preprocessor import GraphPreprocessor
    pre, ops = world["pre"], world["ops"]
    assert "exact_4" in pre.cache_filename and "_3_0.9_" not in pre.cache_filename
    walk = GraphPreprocessor(world["A"], walks_per_node=3, p_halt=0.9, max_walk_length=4, random_walk_seed=1)
    assert walk.cache_filename != pre.cache_filename and "exact" not in walk.cache_filename
    other = GraphPreprocessor(world["A"], walks_per_node=50, p_halt=0.1, max_walk_length=4, random_walk_seed=9,
                              exact=True)
    assert other.cache_filename == pre.cache_filename  # walks, p_halt and the seed do not enter
    ref = R.exact_steps(eng.laplacian(world["A"]).to_scipy(), 4)
    assert len(ops) == 4
    for op, M64, want in zip(ops, world["mats64"], ref):
        assert R.same_bits(M64, want)
        t = op.sparse_csr_tensor
        assert t.is_sparse_csr and t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == (N, N)
        assert np.array_equal(t.crow_indices().cpu().numpy(), want.indptr)
        assert np.array_equal(t.col_indices().cpu().numpy(), want.indices)
        assert np.array_equal(t.values().cpu().numpy().view(np.uint32), want.data.astype(np.float32).view(np.uint32))


def test_sparse_grf_kernel_on_exact_steps(world):
    from efficient_graph_gp_sparse.gptorch_kernels_sparse import SparseGRFKernel
    torch.manual_seed(0)
    kern = SparseGRFKernel(4, world["ops"]).cuda()
    f = kern.modulator_vector.detach().cpu().numpy().astype(np.float64)
    Phi = sum(fl * M.toarray() for fl, M in zip(f, world["mats"]))
    aPhi = np.abs(Phi)
    rowmax, top = aPhi.max(axis=1), aPhi.max()

    def close(got, ref, absbound, rows):
        err = np.abs(np.asarray(got, np.float64) - ref)
        tol = 3e-5 * absbound + 1e-12 * (rowmax[rows] * top).reshape((-1,) + (1,) * (err.ndim - 1))
        return bool(np.all(err <= tol)), float((err / tol).max())

    i1, i2 = [0, 3, 5, 17, 299, 3], [1, 3, 20]
    x1, x2 = torch.tensor(i1, device="cuda"), torch.tensor(i2, device="cuda")
    ok, e = close(kern(x1, x2).detach().cpu().numpy(), Phi[i1] @ Phi[i2].T, aPhi[i1] @ aPhi[i2].T, i1)
    assert ok, e
    ok, e = close(kern(x1, x1, diag=True).detach().cpu().numpy(), np.einsum("ij,ij->i", Phi[i1], Phi[i1]),
                  np.einsum("ij,ij->i", aPhi[i1], aPhi[i1]), i1)
    assert ok, e
    Kfull = kern()
    ok, e = close(Kfull.detach().cpu().numpy(), Phi @ Phi.T, aPhi @ aPhi.T, np.arange(N))
    assert ok, e
    assert torch.equal(Kfull, Kfull.t())


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))) / np.max(np.abs(b)))


@pytest.mark.parametrize("noise", [0.05, 1.0])
def test_marginal_likelihood_on_exact_steps(eng, world, noise):
    """Identity probes (Hutchinson's traces exact, SLQ exact once Lanczos has run out): value, d/df and d/ds2
    meet the dense truth as closely as the CPU restatement does (x 10), tests/test_gpu_mll.py's rule."""
    from grf_amd.features import StepMatrices
    n_train = 64
    r = np.random.default_rng(71)
    tr, y = np.sort(r.permutation(N)[:n_train]), r.standard_normal(n_train)
    steps = StepMatrices(world["ops"], eng)
    f = torch.tensor([1.0, -0.5, 0.25, -0.125], dtype=torch.float32)
    phi = steps.phi(f)
    P = phi.to_scipy().astype(np.float64)
    P.data = phi.val32[:phi.nnz].cpu().numpy().astype(np.float64)
    Pt, Ms, Z = P[tr], [M[tr] for M in world["mats"]], MR.identity_probes(n_train)
    est = MR.estimate(Pt, Ms, y, noise, Z, tolerance=1e-12, max_iter=48)
    tru = MR.dense_truth(Pt, Ms, y, noise)
    value, g_f, g_noise, iters = eng.marginal_log_likelihood(
        steps, f, torch.from_numpy(tr), torch.from_numpy(y), noise, torch.from_numpy(np.ascontiguousarray(Z)).cuda(),
        1e-12, 48)
    got = dict(value=value, grad_f=g_f.cpu().numpy(), grad_noise=g_noise)
    for q in ("value", "grad_f", "grad_noise"):
        print(f"exact steps s2={noise} {q}: gpu vs truth {_rel(got[q], tru[q]):.3e}  restatement vs truth "
              f"{_rel(est[q], tru[q]):.3e}  iterations {iters} / {est['iters']}")
    for q in ("value", "grad_f", "grad_noise"):
        assert _rel(got[q], tru[q]) <= 10.0 * _rel(est[q], tru[q]), q


class _Likelihood:
    noise = torch.tensor([0.05])


def test_model_on_exact_steps(eng, world):
    from efficient_graph_gp_sparse.models import SparseGraphGP
    r = np.random.default_rng(0)
    perm = r.permutation(N)
    tr, te = perm[:200], perm[200:260]
    x_train = torch.tensor(tr, dtype=torch.float32, device="cuda").unsqueeze(1)
    y_train = torch.tensor(r.standard_normal(200), dtype=torch.float32, device="cuda")
    x_test = torch.tensor(te, dtype=torch.float32, device="cuda").unsqueeze(1)
    torch.manual_seed(4)
    gp = SparseGraphGP(x_train, y_train, _Likelihood(), world["ops"], 4).cuda()
    f = gp.covar_module.modulator_vector.detach().cpu().numpy().astype(np.float64)
    Phi = sum(float(np.float32(fl)) * M for fl, M in zip(f, world["mats"]))
    Phi = sp.csr_matrix(Phi.astype(np.float32).astype(np.float64))
    # predict: the same draws replayed through the oracle, 3 CG iterations (the rounding-determined window)
    torch.manual_seed(123)
    out = gp.predict(x_test, n_samples=32, max_iter=3)
    assert out.shape == (32, 60) and gp.last_cg_iterations == 3
    torch.manual_seed(123)
    e1 = torch.randn(32, N, device="cuda")
    e2 = torch.sqrt(torch.tensor(0.05, device="cuda")) * torch.randn(32, 200, device="cuda")
    want, it = OCG.pathwise_predict(Phi, tr, te, y_train.cpu().numpy(), 0.05, e1.cpu().numpy(), e2.cpu().numpy(),
                                    max_iter=3)
    rel = np.linalg.norm(out.cpu().numpy() - want) / np.linalg.norm(want)
    assert it == 3 and rel <= 1e-5, rel
    # the marginal likelihood per datum and its modulator gradient against the dense truth
    Z = torch.from_numpy(MR.identity_probes(200))
    mll = gp.marginal_log_likelihood(probes=Z, tolerance=1e-6)
    mll.backward()
    Ms = [M[tr] for M in world["mats"]]
    t0 = MR.dense_truth(Phi[tr], Ms, y_train.cpu().numpy().astype(np.float64), 0.05)
    assert abs(mll.item() - t0["value"] / 200) <= 1e-3 * abs(t0["value"] / 200)
    gf = gp.covar_module.raw_modulator_vector.grad
    assert gf is not None and _rel(gf.cpu().numpy() * 200, t0["grad_f"]) <= 1e-2


def _np_laplacian(A):
    d = A.sum(axis=1)
    return np.eye(len(A)) - A / np.sqrt(np.outer(d, d))


@pytest.mark.parametrize("graph", ["readme", "er40"])
def test_pofm_mirrors(golden, graph):
    from efficient_graph_gp.gpflow_kernels import GraphDiffusionPoFMKernel, GraphGeneralPoFMKernel
    A = np.asarray(golden("small_graphs")[f"{graph}_A"], np.float64)
    n = len(A)
    L = _np_laplacian(A)
    F = np.stack([np.linalg.matrix_power(L, l) for l in range(4)], axis=-1)
    r = np.random.default_rng(8)
    f = np.array([0.9, -0.4, 0.2, 0.05])
    k = GraphGeneralPoFMKernel(A, max_walk_length=4, modulator_vector=f)
    assert isinstance(k, torch.nn.Module) and isinstance(k.modulator_vector, torch.nn.Parameter)
    np.testing.assert_allclose(k.feature_matrices, F, rtol=1e-12, atol=1e-13)
    P = F @ f
    Kref = P @ P.T
    xs, ys = [0, n - 1, 2], [1, 2, 3, n - 1, 0]
    X, Y = np.array(xs)[:, None], np.array(ys)
    np.testing.assert_allclose(k.K(np.arange(n)), Kref, rtol=3e-5, atol=1e-6)
    np.testing.assert_allclose(k.K(X, Y), Kref[np.ix_(xs, ys)], rtol=3e-5, atol=1e-6)
    np.testing.assert_allclose(k(X), Kref[np.ix_(xs, xs)], rtol=3e-5, atol=1e-6)
    np.testing.assert_allclose(k.K_diag(X), np.diag(Kref)[xs], rtol=3e-5, atol=1e-6)
    np.testing.assert_allclose(k(X, full_cov=False), np.diag(Kref)[xs], rtol=3e-5, atol=1e-6)
    W = r.standard_normal((3, 5))
    (k.K_torch(X, Y) * torch.tensor(W, device=k.device)).sum().backward()
    gref = [np.sum(W * (F[xs, :, l] @ P[ys].T + P[xs] @ F[ys, :, l].T)) for l in range(4)]
    np.testing.assert_allclose(k.modulator_vector.grad.cpu().numpy(), gref, rtol=1e-4, atol=1e-6)
    # the default modulator is the reference's seeded draw
    kd = GraphGeneralPoFMKernel(A, max_walk_length=3)
    np.random.seed(42)
    np.testing.assert_array_equal(kd.modulator_vector.detach().cpu().numpy(), np.random.randn(3))
    # the combinatorial Laplacian
    kc = GraphGeneralPoFMKernel(A, max_walk_length=3, modulator_vector=[1.0, 0.5, 0.25], normalize_laplacian=False)
    Lc = np.diag(A.sum(axis=1)) - A
    Pc = np.eye(n) + 0.5 * Lc + 0.25 * Lc @ Lc
    np.testing.assert_allclose(kc.K(np.arange(n)), Pc @ Pc.T, rtol=3e-5, atol=1e-6 * np.abs(Pc @ Pc.T).max())

    # diffusion: coefficients (-beta / 2)^i / i!, i = 0 .. max_expansion; K = sigma_f^2 K_f K_f^T
    dk = GraphDiffusionPoFMKernel(A, beta=2.0, max_expansion=5, sigma_f=1.5)
    np.testing.assert_allclose([float(dk.beta), float(dk.sigma_f)], [2.0, 1.5], rtol=1e-12)

    def k_f(beta):
        out, term = np.zeros((n, n)), np.eye(n)
        for i in range(6):
            out = out + (-beta / 2.0) ** i / float(np.prod(np.arange(1, i + 1))) * term
            term = term @ L
        return out

    Kd = 2.25 * k_f(2.0) @ k_f(2.0).T
    np.testing.assert_allclose(dk.K(np.arange(n)), Kd, rtol=3e-5, atol=1e-6)
    np.testing.assert_allclose(dk.K_diag(X), np.diag(Kd)[xs], rtol=3e-5, atol=1e-6)
    np.testing.assert_allclose(dk(X, Y), Kd[np.ix_(xs, ys)], rtol=3e-5, atol=1e-6)
    (dk.K_torch(np.arange(n)) * torch.tensor(np.eye(n), device=dk.device)).sum().backward()

    def trace(beta, sig):
        return sig ** 2 * np.trace(k_f(beta) @ k_f(beta).T)

    h = 1e-6
    gb = (trace(2.0 + h, 1.5) - trace(2.0 - h, 1.5)) / (2 * h) * (1 - np.exp(-2.0))  # d softplus = sigmoid
    gs = (trace(2.0, 1.5 + h) - trace(2.0, 1.5 - h)) / (2 * h) * (1 - np.exp(-1.5))
    np.testing.assert_allclose([dk.raw_beta.grad.item(), dk.raw_sigma_f.grad.item()], [gb, gs], rtol=1e-4)


def test_pofm_errors_and_remaining_stubs():
    import efficient_graph_gp.gpflow_kernels as gk
    A = np.array([[0.0, 1.0, 1.0], [1.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    with pytest.raises(AssertionError):
        gk.GraphGeneralPoFMKernel(np.ones((3, 4)))
    with pytest.raises(AssertionError):
        gk.GraphDiffusionPoFMKernel(np.ones((3, 4)))
    with pytest.raises(ValueError):
        gk.GraphGeneralPoFMKernel(A, max_walk_length=4, modulator_vector=[1.0, 2.0])
    for stub in (gk.GraphDiffusionKernel, gk.GraphDiffusionGRFKernel):
        with pytest.raises(NotImplementedError):
            stub(A)
