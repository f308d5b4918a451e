"""GPU: the whole-K Gram tiles through the plain instantiation (csrc/grf_gram.hip, gram_plain_tile: tile
coordinates from 32-bit host constants, csrc/grf_gram_tiles.h) and the generic one beside it.

Seeded sparse Phi with n in {1, 64, 65, 130, 200} at W = 64 -- one to four bands, a last band of 1, 64, 1, 2 and
8 columns -- and n = 4097 at W = 4096 (two bands, the last one column wide; two rows of 700 and 1300 nonzeros, so a
wave's share takes a second and a third batch of 128), as record triples and as record pairs.  Every case,
symmetric upper tiles + mirror:

* bit-equal (uint32 view) to tests/gram_reference.py's fixed-point restatement at the shifts the transpose left;
* its upper triangle bit-equal to the row-mode entry (grf_gram_sparse_rec, the generic tile) on the same
  transpose -- row i of both is summed at row i's shift;
* the same K from three launches of grf_gram_sparse_upper_rec (parts 0, 1, 2 of 3);
* K lies inside a larger buffer of sentinel words (rows before and after, columns behind every row), which must
  be untouched.

One case with row cuts and one with the hub add (onto a prior K of known floats) take the generic instantiation and
must keep their bits.
"""
import numpy as np
import pytest
import torch

import gram_reference as G

pytestmark = pytest.mark.gpu

SENT = 0x7FC12345  # a NaN no kernel produces
PAD_ROWS, PAD_COLS = 3, 4

SHAPES = [(1, 64), (64, 64), (65, 64), (130, 64), (200, 64), (4097, 4096)]


@pytest.fixture(scope="module")
def eng():
    from grf_amd.engine import GRFEngine
    return GRFEngine("cuda:0")


_CASES = {}


def case(n, W):
    """(Phi, the restated whole K or None until the shifts are known)."""
    if (n, W) in _CASES:
        return _CASES[(n, W)]
    rng = np.random.default_rng(1000 + n)
    density = min(1.0, 6.0 / n + 0.05) if n < 1000 else 0.003
    long_rows = {0: 700, n - 1: 1300} if n > 1000 else {}
    rows = []
    for r in range(n):
        if r == 2 and n > 5:
            rows.append(([], []))  # an empty row
            continue
        if r in long_rows:
            c = np.sort(rng.choice(n, long_rows[r], replace=False)).astype(np.int32)
        else:
            c = np.flatnonzero(rng.random(n) < density).astype(np.int32)
        rows.append((c, G._values(rng, len(c))))
    _CASES[(n, W)] = {"P": G.csr(n, n, rows), "ref": None, "sh": None}
    return _CASES[(n, W)]


def dev_csr(eng, P):
    from grf_amd.engine import DeviceCSR
    d = DeviceCSR.from_scipy(P, eng.device)
    d.val32 = torch.from_numpy(np.asarray(P.data, np.float32)).to(eng.device)
    return d


def reference(c, tr):
    """The restated K at the transpose's own shifts (the same for both record kinds), computed once per case."""
    sh = tr.t_rowshift.cpu().numpy()[:c["P"].shape[0]]
    if c["ref"] is None:
        c["sh"], c["ref"] = sh, G.sym_ref(c["P"], sh)
    assert np.array_equal(sh, c["sh"])
    return c["ref"]


class Framed:
    """K inside a buffer of sentinel words: PAD_ROWS rows before and after, PAD_COLS columns behind every row."""

    def __init__(self, eng, n, fill=None):
        self.n, self.ld = n, eng.leading_dim(n)
        self.big = torch.full((n + 2 * PAD_ROWS, self.ld + PAD_COLS), SENT, dtype=torch.int32,
                              device=eng.device).view(torch.float32)
        self.K = self.big[PAD_ROWS:PAD_ROWS + n, :self.ld]
        if fill is not None:
            self.K[:, :n] = torch.from_numpy(fill).to(eng.device)

    def body(self):
        """K's n x n bits, after checking that every word around them still holds the sentinel."""
        w = self.big.cpu().numpy().view(np.uint32)
        frame = np.ones(w.shape, bool)
        frame[PAD_ROWS:PAD_ROWS + self.n, :self.n] = False
        assert np.all(w[frame] == SENT), "a word outside K was written"
        return w[PAD_ROWS:PAD_ROWS + self.n, :self.n].copy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("kind", ["triples", "pairs"])
@pytest.mark.parametrize("n,W", SHAPES)
def test_whole_k_bits(eng, n, W, kind):
    c = case(n, W)
    phi = dev_csr(eng, c["P"])
    tr = eng.transpose_banded(phi, W, triples=kind == "triples")
    assert tr.t_split is None
    ref = reference(c, tr)
    one = Framed(eng, n)
    eng.gram_sparse_upper(phi, tr, out=one.K)
    eng.gram_mirror(one.K, n)
    got = one.body()
    assert np.array_equal(got, bits(ref))
    # the row-mode entry on the same transpose: its rows are summed at their own shifts, as the upper triangle is
    rows = Framed(eng, n)
    eng.gram_sparse(phi, tr, 0, n, out=rows.K)
    iu = np.triu_indices(n)
    assert np.array_equal(rows.body()[iu], got[iu])
    # three launches
    three = Framed(eng, n)
    for p in range(3):
        eng.gram_sparse_upper(phi, tr, out=three.K, parts=(p, p + 1, 3))
    eng.gram_mirror(three.K, n)
    assert np.array_equal(three.body(), got)


@pytest.mark.parametrize("kind", ["triples", "pairs"])
def test_row_cuts_keep_the_bits(eng, kind):
    n, W = 200, 64
    c = case(n, W)
    phi = dev_csr(eng, c["P"])
    tr = eng.transpose_banded(phi, W, triples=kind == "triples")
    cuts = eng.row_cuts(phi, tr, skewed=True)
    assert cuts is not None
    k = Framed(eng, n)
    eng.gram_sparse_upper(phi, tr, out=k.K, cuts=cuts)
    eng.gram_mirror(k.K, n)
    assert np.array_equal(k.body(), bits(reference(c, tr)))


@pytest.mark.parametrize("kind", ["triples", "pairs"])
def test_hub_add_keeps_the_bits(eng, kind):
    """The add launch onto a prior K of known floats: float32(sum) + prior on the tiles' entries (row r: the
    columns from its band's first one on), the prior everywhere else."""
    n, W = 200, 64
    c = case(n, W)
    phi = dev_csr(eng, c["P"])
    tr = eng.transpose_banded(phi, W, triples=kind == "triples")
    reference(c, tr)
    rng = np.random.default_rng(5)
    prior = (rng.standard_normal((n, n)) * np.exp2(rng.integers(-6, 3, (n, n)))).astype(np.float32)
    own = np.arange(n)[None, :] >= (np.arange(n)[:, None] // W) * W
    want = np.where(own, G.add_ref(G.gram_fx_ref(c["P"], c["sh"])[0], prior), prior)
    k = Framed(eng, n, fill=prior)
    eng._gram_upper_cuts(phi, tr, k.K, None, (0, 1, 1), True)
    assert np.array_equal(k.body(), bits(want))
