"""GPU: the record-triple transpose (csrc/grf_sparse.hip, tr_place_self_triples_kernel) and the whole-K Gram that
reads it (csrc/grf_gram.hip, gram_sparse_kernel<..., 16>).

* decode round trip: t_rec read back through the descriptors by the numpy decoder below -- written from
  include/grf.h's description of the format, not from the kernel -- must hold exactly Phi's (row, column, value
  bits), padding only as (row c0, +0.0) in trailing places, buckets inside the slabs and disjoint;
* K bit for bit: triples against pairs (the integer sums do not depend on the records' grouping, padding adds 0),
  and against tests/gram_reference.py's fixed-point restatement where it is cheap;
* the refusals of include/grf.h (band wider than 4096, split, slots, the planned fills): ValueError = GRF_EINVAL.

Shapes: W = 4096 with 4096 + 70 rows (two bands, a ragged last one, empty rows); buckets of 0, 1, 2, 3, 4, 23,
24, 25 entries (triple and line boundaries: 8 triples per line); one block only; one entry in each of blocks
0, 2, 4, 6 -- every triple closes early, the slab bound's worst case -- over a whole region of 128 columns; band
rows 0 and 4095; the same Phi at W = 256 and 1024 (fewer than 8 blocks); an oversized region (image > 48 KiB).
"""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import gram_reference as G

pytestmark = pytest.mark.gpu

BLOCK = 512
N_A = 4096 + 70


@pytest.fixture(scope="module")
def eng():
    from grf_amd.engine import GRFEngine
    return GRFEngine("cuda:0")


def _values(rng, size):
    v = rng.standard_normal(size).astype(np.float32) * np.float32(0.37)
    v[v == 0] = np.float32(0.5)
    return v


def _csr(mask, rng):
    P = sp.csr_matrix(mask.astype(np.float32))
    P.sort_indices()
    P.data = _values(rng, P.nnz)
    return P


_PHI = {}


def phi_a():
    """The hand-built square Phi of the module docstring (columns past 300 empty)."""
    if "a" in _PHI:
        return _PHI["a"]
    rng = np.random.default_rng(11)
    n = N_A
    mask = np.zeros((n, n), bool)
    free_rows = np.ones(n, bool)
    free_rows[[7, 100, 2047, 2048, 4100]] = False                # empty rows (kept empty below)

    def put(col, rows):
        rows = np.asarray(rows)
        assert free_rows[rows].all()
        mask[rows, col] = True

    def pick(lo, hi, c):
        pool = np.nonzero(free_rows[lo:hi])[0] + lo
        return rng.choice(pool, size=c, replace=False)

    for col, c in enumerate((0, 1, 2, 3, 4, 23, 24, 25)):          # columns 0..7: sizes in band 0
        put(col, pick(0, 4096, c))
    put(8, pick(3 * BLOCK, 4 * BLOCK, 30))                          # one block only
    put(9, [1, 4094])
    put(10, [0, 4095])                                              # the band's first and last row
    for col in range(11, 128):                                      # a spread of ordinary buckets
        put(col, pick(0, 4096, int(rng.integers(0, 40))))
    for col in range(128, 256):                                     # a whole region of worst-case buckets
        put(col, [int(pick(b * BLOCK, (b + 1) * BLOCK, 1)[0]) for b in (0, 2, 4, 6)])
    for col in range(256, 300):
        put(col, pick(0, 4096, int(rng.integers(0, 12))))
    for col in range(0, 300, 3):                                    # the ragged last band
        put(col, pick(4096, n, int(rng.integers(1, 9))))
    assert mask[0, 10] and mask[4095, 10] and not mask[[7, 100, 2047, 2048, 4100]].any()
    _PHI["a"] = _csr(mask, rng)
    return _PHI["a"]


def phi_oversized():
    """W = 1024, one band: 128 columns of ~80 entries (one region whose image exceeds 48 KiB), the rest sparse."""
    if "c" not in _PHI:
        rng = np.random.default_rng(12)
        n = 1024
        mask = rng.random((n, n)) < 0.004
        for col in range(128):
            mask[:, col] = False
            mask[rng.choice(n, size=int(rng.integers(76, 85)), replace=False), col] = True
        _PHI["c"] = _csr(mask, rng)
    return _PHI["c"]


def phi_skewed():
    """n = 1500, W = 512: a few columns in most rows (hubs), the others sparse."""
    if "s" not in _PHI:
        rng = np.random.default_rng(13)
        n = 1500
        mask = rng.random((n, n)) < 0.006
        for col in range(0, 40):
            mask[:, col] = rng.random(n) < (0.9 if col < 8 else 0.3)
        _PHI["s"] = _csr(mask, rng)
    return _PHI["s"]


def dev_csr(eng, P):
    from grf_amd.engine import DeviceCSR
    d = DeviceCSR.from_scipy(P, eng.device)
    d.val32 = torch.from_numpy(np.asarray(P.data, np.float32)).to(eng.device)
    return d


# ------------------------------------------------------------------------------------------------ the decoder
def decode_triples(tr):
    """(rows, cols, value bits) of every entry of a triple transpose, checking the format on the way."""
    W, n_cols, n = tr.band_width, tr.n_cols, tr.n_rows
    nb = -(-n // W)
    nbk = nb * n_cols
    d = tr.t_desc.cpu().numpy().view(np.uint32).astype(np.int64)
    desc, total = d[:2 * nbk].reshape(nbk, 2), int(d[2 * nbk] + (d[2 * nbk + 1] << 32))
    rec = tr.t_rec.cpu().numpy()
    assert total * 128 <= rec.size
    first, T = desc[:, 0], desc[:, 1]
    lines = (T + 7) // 8
    # buckets in (band, column) order inside the slabs' total, none overlapping the next
    ne = np.nonzero(T)[0]
    assert np.all(first[ne] + lines[ne] <= total)
    assert np.all(first[ne][1:] >= (first[ne] + lines[ne])[:-1])
    R, Cc, V = [], [], []
    words = rec[:total * 128].view(np.uint32).reshape(-1, 4)       # one 16-byte record per row
    for b in ne:
        band, col = divmod(int(b), n_cols)
        r = words[first[b] * 8: first[b] * 8 + T[b]]
        cols = r[:, 0].astype(np.int64)
        c0 = cols & 0xfff
        base = c0 & ~511
        rows = np.stack([c0, base + ((cols >> 12) & 0x3ff), base + (cols >> 22)], 1)
        vals = r[:, 1:4]
        pad = np.zeros(rows.shape, bool)
        pad[:, 1:] = rows[:, 1:] == c0[:, None]                      # a bucket holds a row once: place 0 owns c0
        assert np.all(vals[pad] == 0), "padding must be +0.0"
        assert not np.any(pad[:, 1] & ~pad[:, 2]), "padding trails the entries of a triple"
        blk = rows // BLOCK
        assert np.all((blk[~pad] >= 0)) and np.all(blk[:, 1:] - blk[:, :1] <= 1) and np.all(blk[:, 1:] >= blk[:, :1])
        assert np.all(np.diff(blk[:, 0]) >= 0), "triples in block order"
        keep = ~pad
        rr = rows[keep] + band * W
        assert np.all(rows[keep] < W) and np.all(rr < n)
        R.append(rr)
        Cc.append(np.full(rr.shape, col, np.int64))
        V.append(vals[keep].astype(np.int64))
    cat = lambda x: np.concatenate(x) if x else np.zeros(0, np.int64)  # noqa: E731
    return cat(R), cat(Cc), cat(V)


def assert_round_trip(tr, P):
    from grf_amd import _lib as C
    assert tr.rec_kind == C.REC_TRIPLES and tr.rec_unit == C.REC_LINE and tr.t_split is None
    r, c, v = decode_triples(tr)
    Pc = P.tocoo()
    want = np.stack([Pc.row.astype(np.int64), Pc.col.astype(np.int64),
                     np.asarray(Pc.data, np.float32).view(np.uint32).astype(np.int64)], 1)
    got = np.stack([r, c, v], 1)
    assert got.shape == want.shape
    order = lambda a: a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))]  # noqa: E731
    assert np.array_equal(order(got), order(want))


def whole_k(eng, phi, tr):
    K = torch.full((tr.n_rows, eng.leading_dim(tr.n_rows)), float("nan"), dtype=torch.float32, device=eng.device)
    return eng.gram_sparse_sym(phi, tr, out=K).cpu().numpy()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("W", [4096, 1024, 256])
def test_decode_round_trip(eng, W):
    P = phi_a()
    tr = eng.transpose_banded(dev_csr(eng, P), W, triples=True)
    assert_round_trip(tr, P)
    if W == 4096:
        # band 0: the worst-case region's 128 buckets of 4 one-entry triples, the one-block bucket's 30 entries as
        # 10 full triples, rows 0 and 4095 as two triples
        T = tr.t_desc.cpu().numpy().view(np.uint32)[:2 * P.shape[1]].reshape(-1, 2)[:, 1]
        assert np.all(T[128:256] == 4) and T[0] == 0 and T[8] == 10 and T[10] == 2


def test_triple_counts_match_the_model(eng):
    """Every descriptor's triple count = tools/triple_model.py's count from the bucket's block counts."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import triple_model as M
    P = phi_a()
    for W in (4096, 1024):
        tr = eng.transpose_banded(dev_csr(eng, P), W, triples=True)
        nb = -(-P.shape[0] // W)
        T = tr.t_desc.cpu().numpy().view(np.uint32)[:2 * nb * P.shape[1]].reshape(nb, P.shape[1], 2)[:, :, 1]
        blk = M.block_counts(torch.from_numpy(P.indptr.astype(np.int64)), torch.from_numpy(P.indices), P.shape[0],
                             P.shape[1], W)
        assert np.array_equal(T.astype(np.int64), M.triples(blk).numpy())


def test_whole_k_bits_triples_pairs_reference(eng):
    P = phi_a()
    phi = dev_csr(eng, P)
    Kt = whole_k(eng, phi, eng.transpose_banded(phi, 4096, triples=True))
    Kp = whole_k(eng, phi, eng.transpose_banded(phi, 4096))
    assert not np.isnan(Kt).any() and same_bits(Kt, Kp)
    assert same_bits(Kt, G.sym_ref(P, G.rowshift_ref(P)[0]))
    # the row Gram reads triples too (rows across the band boundary)
    tr = eng.transpose_banded(phi, 4096, triples=True)
    rows = eng.gram_sparse(phi, tr, 4000, 4166).cpu().numpy()
    assert same_bits(rows, eng.gram_sparse(phi, eng.transpose_banded(phi, 4096), 4000, 4166).cpu().numpy())
    for W in (1024, 256):
        assert same_bits(whole_k(eng, phi, eng.transpose_banded(phi, W, triples=True)), Kt), W


def test_kernel_step_bits_env_switch(eng, monkeypatch):
    """The benchmarked path (pipeline.kernel_step, symmetric mode) with GRF_REC_TRIPLES 1 against 0."""
    from grf_amd import _lib as C
    from grf_amd import pipeline as P
    from grf_amd.engine import DeviceCSR
    from grf_amd.graphs import er_graph_exact_edges
    n, m, L, p = 5003, 16, 6, 0.1
    A = DeviceCSR.from_scipy(er_graph_exact_edges(n, 10 * n, seed=3), eng.device)
    f = np.array([1.0, -0.5, 0.125, -0.02, 0.003, -0.0004])
    out = {}
    for flag, kind in (("1", C.REC_TRIPLES), ("0", C.REC_PAIRS)):
        monkeypatch.setenv("GRF_REC_TRIPLES", flag)
        pl = P.plan_step(n, m, L, p, f)
        assert pl.mode == "sym"
        K, fr = P.kernel_step(eng, A, pl)
        torch.cuda.synchronize()
        assert fr.tr.rec_kind == kind
        out[flag] = P.k_view(K, pl).cpu().numpy()
        if flag == "1":
            assert_round_trip(fr.tr, fr.phi.to_scipy().astype(np.float32))
    assert same_bits(out["1"], out["0"])
    assert np.array_equal(out["1"], out["1"].T)


def test_row_cuts_and_hub_split_bits(eng):
    P = phi_skewed()
    phi = dev_csr(eng, P)
    n, W = P.shape[0], 512
    ref = G.sym_ref(P, G.rowshift_ref(P)[0])
    Ks = {}
    for triples in (True, False):
        tr = eng.transpose_banded(phi, W, triples=triples)
        cuts = eng.row_cuts(phi, tr, skewed=True)
        assert cuts is not None
        K = torch.full((n, eng.leading_dim(n)), float("nan"), dtype=torch.float32, device=eng.device)
        eng.gram_sparse_upper(phi, tr, out=K, cuts=cuts)
        Ks[triples] = eng.gram_mirror(K, n).cpu().numpy()
    assert same_bits(Ks[True], Ks[False]) and same_bits(Ks[True], ref)
    Kh = {}
    for triples in (True, False):
        tr = eng.transpose_banded(phi, W, triples=triples)
        Kh[triples] = eng.gram_sparse_sym_hubs(phi, tr, 32, skewed=True).cpu().numpy()
    assert not np.isnan(Kh[True]).any() and same_bits(Kh[True], Kh[False])


def test_oversized_region(eng):
    P = phi_oversized()
    phi = dev_csr(eng, P)
    tr = eng.transpose_banded(phi, 1024, triples=True)
    d = tr.t_desc.cpu().numpy().view(np.uint32)[:2 * 128].reshape(128, 2).astype(np.int64)
    assert int(((d[:, 1] + 7) // 8).sum()) * 128 > 48 * 1024, "the first region's image must exceed the LDS cap"
    assert_round_trip(tr, P)
    Kt = whole_k(eng, phi, tr)
    assert same_bits(Kt, whole_k(eng, phi, eng.transpose_banded(phi, 1024)))
    assert same_bits(Kt, G.sym_ref(P, G.rowshift_ref(P)[0]))


def test_refusals(eng):
    phi = dev_csr(eng, phi_oversized())
    with pytest.raises(ValueError):
        eng.transpose_banded(phi, 8192, triples=True)
    with pytest.raises(ValueError):
        eng.transpose_banded(phi, 1024, triples=True, split=True)
    with pytest.raises(ValueError):
        eng.transpose_banded(phi, 1024, triples=True, slots=True)
    with pytest.raises(ValueError):
        eng.transpose_banded(phi, 1024, triples=True, self_count=False)
    with pytest.raises(ValueError):
        eng.transpose_banded(phi, 1024, triples=True, staged=False)
    torch.cuda.synchronize()
    # ... and nothing is left broken: the same call without the refused option works
    assert_round_trip(eng.transpose_banded(phi, 1024, triples=True), phi_oversized())
