"""CPU: the numpy restatement of the device SpGEMM's rule (tests/spgemm_reference.py) is pinned against scipy
and against the reference's own exact walk tensors.

* Non-cancelling cases: bit-equal to scipy's ``A @ B`` (after ``sort_indices``) -- pattern and value bits.
* An integer-valued cancelling case: scipy's product with the stored zeros added back (scipy keeps or drops
  them depending on its version; the rule keeps them, as +0.0).
* The chain [I, L, L^2, ...] against ``tests/golden/pstep.npz`` (the reference's dense
  ``compute_pstep_walk_matrix``, a differently ordered fp64 product chain) for every fixture graph, elementwise
  within 2 ((1 + gamma_n)^l - 1) (|L|^l)_ij, gamma_n = n 2^-53 / (1 - n 2^-53): the textbook bound, nothing in
  it measured.  Measured: the largest error / bound ratio over all fixture graphs and steps is 0.056
  (cycle4, step 4).
"""
import numpy as np
import pytest
import scipy.sparse as sp

import spgemm_reference as R
from golden_util import csr


def _scipy_product(A, B):
    C = (sp.csr_matrix(A) @ sp.csr_matrix(B)).tocsr()
    C.sort_indices()
    return C


def _er_laplacian(n=300, p=0.03, seed=11):
    return R.normalized_laplacian(R.er_adjacency(n, p, seed))


NON_CANCELLING = {
    "mixed5": lambda: R.case_mixed(5),
    "mixed257": lambda: R.case_mixed(257),
    "thresholds": lambda: R.case_thresholds((1024, 4096))[:2],
    "full_overlap": R.case_full_overlap,
    "no_overlap": R.case_no_overlap,
}


@pytest.mark.parametrize("name", sorted(NON_CANCELLING))
def test_bit_equal_to_scipy(name):
    A, B = NON_CANCELLING[name]()
    C, S = R.spgemm(A, B), _scipy_product(A, B)
    assert np.count_nonzero(C.data == 0.0) == 0  # (a non-cancelling case: scipy has nothing to drop)
    S.eliminate_zeros()
    assert R.same_bits(C, S)


def test_wide_case_is_the_narrow_one_shifted():
    """n_cols = 2^31 - 1 (scipy's product would need scratch arrays of n_cols entries): the rule does not
    depend on where the columns lie, so the case equals scipy's product of the columns shifted down."""
    A, B = R.case_wide()
    shift = B.shape[1] - 5001
    Bn = sp.csr_matrix((B.data, B.indices - shift, B.indptr), shape=(B.shape[0], 5001))
    C, S = R.spgemm(A, B), _scipy_product(A, Bn)
    assert C.shape[1] == 2 ** 31 - 1 and C.indices.max() == 2 ** 31 - 2
    Cn = sp.csr_matrix((C.data, C.indices - shift, C.indptr), shape=S.shape)
    assert R.same_bits(Cn, S)


@pytest.mark.parametrize("graph", ["er300", "grid12"])
def test_laplacian_powers_bit_equal_to_scipy(graph):
    L = _er_laplacian() if graph == "er300" else R.normalized_laplacian(R.grid_adjacency(12, 12))
    M = sp.identity(L.shape[0], format="csr")
    for l, mine in enumerate(R.exact_steps(L, 6)):
        if l:
            M = _scipy_product(M, L)
        keep = mine.copy()
        keep.eliminate_zeros()
        ref = M.copy()
        ref.eliminate_zeros()
        assert R.same_bits(keep, ref), (graph, l)


def test_threshold_case_hits_its_counts():
    A, B, want = R.case_thresholds((1024, 4096))
    C = R.spgemm(A, B)
    for r, (what, count) in enumerate(want):
        products = int(sum(B.indptr[k + 1] - B.indptr[k] for k in A.indices[A.indptr[r]:A.indptr[r + 1]]))
        distinct = int(C.indptr[r + 1] - C.indptr[r])
        assert (products if what == "products" else distinct) == count, (r, what, products, distinct)


def test_cancelling_case_keeps_zeros():
    A, B = R.case_cancelling()
    C = R.spgemm(A, B)
    S = _scipy_product(A, B)
    # integer values: every sum is exact, so the dense products agree exactly ...
    np.testing.assert_array_equal(C.toarray(), S.toarray())
    # ... and the rule's pattern is the structural one: scipy's entries plus the exact-zero sums
    A1, B1 = sp.csr_matrix(A).copy(), sp.csr_matrix(B).copy()
    A1.data[:], B1.data[:] = 1.0, 1.0
    pat = (A1 @ B1).tocsr()
    pat.sort_indices()
    assert np.array_equal(C.indptr, pat.indptr) and np.array_equal(C.indices, pat.indices)
    zeros = C.data == 0.0
    assert zeros.any() and not np.signbit(C.data[zeros]).any()  # stored zeros are +0.0
    assert C.nnz > np.count_nonzero(S.toarray())
    last = C.data[C.indptr[-2]:]
    assert len(last) == 6 and not np.signbit(last).any() and (last == 0.0).all()  # only -0.0 products


def test_chain_within_bound_of_reference_tensor(golden):
    d, sg = golden("pstep"), golden("small_graphs")
    p_max = int(d["p_max"][0])
    worst = (0.0, None)
    for name in d["names"]:
        n = sg[f"{name}_A"].shape[0]
        L = csr(sg, f"{name}_Lsp", n)
        L.sort_indices()
        Ld = L.toarray()
        T = d[f"{name}_pstep"]
        for l, M in enumerate(R.exact_steps(L, p_max)):
            err = np.abs(M.toarray() - T[:, :, l])
            if l == 0:
                assert not err.any()
                continue
            bound = R.chain_bound(Ld, l)
            assert np.all(err <= bound), (name, l, float((err - bound).max()))
            ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
            if ratio > worst[0]:
                worst = (ratio, (str(name), l))
    print("largest error / bound:", worst)
