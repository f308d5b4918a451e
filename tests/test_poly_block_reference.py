"""CPU: pins tests/poly_block_reference.py, the restatement the GPU tests of the walk operator's K blocks compare
against -- block and diagonal against dense p(G) p(G)^T from numpy's matrix powers on a non-symmetric G (exactly
on integer cases, within the restatement's own bound on real ones), the block and diagonal gradients against the
dense formula and against central differences of <g, K(f)>."""
import numpy as np
import pytest

import poly_block_reference as BR
import poly_reference as PR


@pytest.mark.parametrize("n_f", [1, 2, 3, 8])
@pytest.mark.parametrize("n", [1, 5, 12])
def test_block_and_diagonal_are_exact_on_integers(n, n_f):
    G = PR.directed_graph(n, 10 * n + n_f, integer=True, weights=(-1.0, 1.0))
    f = PR.modulator(n_f, n, integer=True)
    x1, x2 = BR.index_list(n, 7, 1), BR.index_list(n, 9, 2)
    K, _ = BR.kernel_block(G, f, n_f, x1, x2)
    want = BR.dense_block(G, f, n_f, x1, x2)
    assert np.abs(want).max() < 2.0 ** 53 and np.array_equal(K, want)
    d, _ = BR.kernel_diag(G, f, n_f, x2)
    assert np.array_equal(d, np.diag(BR.dense_block(G, f, n_f, x2, x2)))
    if n_f == 1:
        assert np.array_equal(K, f[0] ** 2 * (x1[:, None] == x2[None, :]))
        assert np.array_equal(d, np.full(x2.size, f[0] ** 2))


@pytest.mark.parametrize("n_f", [1, 2, 3, 8])
def test_block_and_diagonal_meet_matrix_powers_within_their_bound(n_f):
    n = 300
    G = PR.directed_graph(n, 50 + n_f, integer=False)
    assert abs(G - G.T).max() > 0.05  # (directed: a mix-up of G and G^T would show)
    f = PR.modulator(n_f, 3, integer=False)
    x1, x2 = BR.index_list(n, 40, 3), BR.index_list(n, 70, 4)
    K, bound = BR.kernel_block(G, f, n_f, x1, x2)
    want = BR.dense_block(G, f, n_f, x1, x2)
    assert np.all(np.abs(K - want) <= bound + 1e-300)
    assert bound.max() <= 1e-11 * max(np.abs(want).max(), 1.0)
    d, dbound = BR.kernel_diag(G, f, n_f, x2)
    dwant = np.diag(BR.dense_block(G, f, n_f, x2, x2))
    assert np.all(np.abs(d - dwant) <= dbound) and dbound.max() <= 1e-11 * max(dwant.max(), 1.0)
    # None means every node
    Kall, _ = BR.kernel_block(G, f, n_f, None, x2)
    assert Kall.shape == (n, x2.size) and np.array_equal(Kall[x1], K)


def test_gradients_match_dense_formula_and_central_differences():
    n, L = 60, 5
    G = PR.directed_graph(n, 77, integer=False, long_rows=())
    assert abs(G - G.T).max() > 0.05
    f = PR.modulator(L, 9, integer=False)
    x1, x2 = BR.index_list(n, 11, 5), BR.index_list(n, 17, 6)
    assert len(set(x1.tolist())) < x1.size and len(set(x2.tolist())) < x2.size   # (repeats)
    r = np.random.default_rng(12)
    g, gd = r.standard_normal((11, 17)), r.standard_normal(17)
    got, bound, _ = BR.kernel_grad(G, f, L, g, x1, x2)
    want = BR.dense_grad(G, f, L, g, x1, x2)
    assert np.all(np.abs(got - want) <= bound + 1e-12 * np.abs(want).max())
    dgot, dbound, _ = BR.kernel_diag_grad(G, f, L, gd, x2)
    dwant = BR.dense_diag_grad(G, f, L, gd, x2)
    assert np.all(np.abs(dgot - dwant) <= dbound + 1e-12 * np.abs(dwant).max())

    def block(fv):
        return float(np.sum(g * BR.dense_block(G, fv, L, x1, x2)))

    def diag(fv):
        return float(np.sum(gd * np.diag(BR.dense_block(G, fv, L, x2, x2))))

    h = 1e-5
    for l in range(L):
        e = np.zeros(L)
        e[l] = h
        for fun, val in ((block, got), (diag, dgot)):
            cd = (fun(f + e) - fun(f - e)) / (2 * h)
            assert abs(cd - val[l]) <= 1e-8 * max(abs(val[l]), np.abs(val).max()), l


def test_integer_gradients_are_exact():
    n, L = 12, 3
    G = PR.directed_graph(n, 5, integer=True)
    f = PR.modulator(L, 2, integer=True)
    x1, x2 = np.array([7, 2, 9, 0, 2]), np.array([3, 3, 11])
    g = PR.block(5, 3, 5, integer=True)
    got, _, mag = BR.kernel_grad(G, f, L, g, x1, x2)
    assert mag < 2.0 ** 53 and np.array_equal(got, BR.dense_grad(G, f, L, g, x1, x2))
    gd = np.array([1.0, -2.0, 1.0])
    dgot, _, dmag = BR.kernel_diag_grad(G, f, L, gd, x2)
    assert dmag < 2.0 ** 53 and np.array_equal(dgot, BR.dense_diag_grad(G, f, L, gd, x2))
