"""GPU: the sparse Gram kernels (csrc/grf_gram.hip) called directly through the C ABI, bit for bit against the
numpy restatement of tests/gram_reference.py (pinned on the CPU by tests/test_gram_reference.py).

include/grf.h promises that a K entry is a pure function of (Phi, row shifts): the int64 sum of the terms
rint(Phi[i,k] Phi[j,k] 2^sh_i), converted by fx_to_float.  So every value assertion here is BITWISE against
``gram_reference.gram_fx_ref``; nothing is compared within a tolerance and nothing measured is asserted.  The
transposes are built on the host (line, packed and slot buckets, with and without the sub-band split, two entry
orders inside the buckets, unused bytes 0xFF), so a bug shared by the device transpose and the Gram cannot hide;
the device transposes are then held to the host-built ones bucket by bucket.  The test owns the leading
dimensions, shifts, buffers and NULLs: K buffers are NaN-filled with PAD elements past their end; padding columns,
the tail and every entry a call does not own must stay NaN, and a second call must return the same bits.

Found by this file and tests/test_gram_reference.py (fixed in the same change, csrc/grf_gram.hip):
  * fx_to_float converted the low word as unsigned, so a small negative sum (hi = -1, lo just below 2^32) took
    lo's float rounding of up to 2^7 units, far above the sum's own ulp: the derived bound of
    test_gram_reference.py failed and the ``ties`` case's K[0, j] = -2 * 2^-10 came out as +0.  The low word now
    counts as signed and hi takes its sign bit back.
  * with a split and ldk % 4 != 0 a diagonal tile's scalar write-out started at the band's first column instead
    of the row's sub-band (``test_gram_upper_parts_mirror_sym_bitwise[n65_W64-line-True]``).
Measured on an MI355X (information, not asserted): 99 cases in under 10 s, the slowest (41 bands, n = 2600) 0.9 s.
"""
import ctypes

import numpy as np
import pytest
import torch

import gram_reference as G

pytestmark = pytest.mark.gpu

PAD = 11
NULL = ctypes.c_void_p(0)
UNIT = {"line": G.REC_LINE, "packed": G.REC_PACKED, "slot": G.REC_SLOT}
BUILD = {"line": G.transpose_line_ref, "packed": G.transpose_packed_ref, "slot": G.transpose_slot_ref}


@pytest.fixture(scope="module")
def eng():
    from grf_amd.engine import GRFEngine
    return GRFEngine("cuda:0")


def _t(a, eng):
    return torch.as_tensor(np.ascontiguousarray(a)).to(eng.device)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else NULL


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _check(eng, rc, what):
    from grf_amd import _lib as C
    C.check(rc, what)


def _nan_k(rows, ldk, eng):
    return torch.full((rows * ldk + PAD,), float("nan"), dtype=torch.float32, device=eng.device)


def _body(buf, rows, ldk, cols, what):
    """The (rows x cols) block of a K buffer; the padding columns and the PAD tail must still be NaN."""
    host = buf.cpu().numpy()
    body = host[:rows * ldk].reshape(rows, ldk)
    assert np.all(np.isnan(body[:, cols:])) and np.all(np.isnan(host[rows * ldk:])), f"{what}: padding overwritten"
    return body[:, :cols].copy()


class Dev:
    """Phi (CSR) and one host-built transpose of PB (default Phi) on the device."""

    def __init__(self, eng, P, W, layout, seed=None, split=False, PB=None, shifts=None):
        PB = P if PB is None else PB
        kw = {"split": split} if layout != "slot" else {}
        desc, rec, t_split = BUILD[layout](PB, W, seed=seed, **kw)
        self.n, self.n_cols, self.t_rows, self.W, self.unit = P.shape[0], P.shape[1], PB.shape[0], W, UNIT[layout]
        self.nb = -(-PB.shape[0] // W)
        self.ptr = _t(np.asarray(P.indptr, np.int64), eng)
        # (64 slack entries: the pipelined kernel's lanes address past a short last row before masking)
        self.idx = _t(np.concatenate([np.asarray(P.indices, np.int32), np.zeros(64, np.int32)]), eng)
        self.val = _t(np.concatenate([np.asarray(P.data, np.float32), np.zeros(64, np.float32)]), eng)
        self.desc_host = desc
        self.desc = _t(desc.view(np.int32), eng)
        self.rec = _t(rec, eng)
        assert self.rec.device.type != "cuda" or self.rec.data_ptr() % 128 == 0
        self.split = _t(t_split.view(np.int16), eng) if t_split is not None else None
        self.split_host = t_split
        sh = G.rowshift_ref(P)[0] if shifts is None else shifts
        self.sh_host = np.asarray(sh, np.int32)
        self.sh = _t(self.sh_host, eng)


_CASES = {}


def _case(name):
    if not _CASES:
        for c in G.geometry_cases() + [G.tie_case(), G.hub_case(), G.probe_case(4096), G.probe_case(8192),
                                       G.bands41_case(), G.dense128_case()]:
            _CASES[c.name] = c
    return _CASES[name]


_REF = {}


def _ref_rows(c, sh, key):
    """gram_fx_ref of the case's probe rows, computed once per (case, shifts)."""
    k = (c.name, key)
    if k not in _REF:
        _REF[k] = G.gram_fx_ref(c.P, sh, rows=np.arange(c.row_begin, c.row_end))[0]
    return _REF[k]


def _gram_sparse(eng, d, rb, re, ldk, K=None):
    K = _nan_k(re - rb, ldk, eng) if K is None else K
    _check(eng, eng.lib.grf_gram_sparse(d.n, rb, re, _p(d.ptr), _p(d.idx), _p(d.val), d.W, d.unit, _p(d.desc),
                                        _p(d.rec), _p(d.sh), _p(K), ldk, NULL, 0, eng.stream), "grf_gram_sparse")
    return K


# --------------------------------------------------------------------------------------- grf_gram_sparse: row blocks
ROW_CASES = ["n1_W64", "n5_W64", "n63_W64", "n64_W64", "n65_W64", "n130_W64", "n400_W192", "n130_up40", "n130_down40",
             "ties", "hub4100", "probe_W4096", "probe_W8192"]


@pytest.mark.parametrize("layout", ["line", "packed", "slot"])
@pytest.mark.parametrize("name", ROW_CASES)
def test_gram_sparse_rows_bitwise(eng, name, layout):
    """K[row_begin:row_end] of every case from host-built transposes in two entry orders: ldk = n (odd n: the
    scalar write-out) and ldk rounded up to 4 plus a padding group (the vector write-out and its scalar tail).
    Line / packed buckets run the 4-wave tiles (8 waves at W = 8192), slot buckets the 8-wave tiles at every W."""
    c = _case(name)
    sh = np.full(c.n, c.tie_shift, np.int32) if name == "ties" else c.shifts[0]
    ref = _ref_rows(c, sh, "rule")
    rb, re = c.row_begin, c.row_end
    print(f"{name}/{layout}: n = {c.n} W = {c.W} rows [{rb}, {re}) edges {c.edges.get('probes', '')}")
    if name == "ties":
        assert np.array_equal(ref[0, 1:].astype(np.float64) * 1024, c.tie_expect.astype(np.float64))
    for seed, ldk in ((1, c.n), (2, -(-c.n // 4) * 4 + 4)):
        d = Dev(eng, c.P, c.W, layout, seed=seed, shifts=sh)
        K = _gram_sparse(eng, d, rb, re, ldk)
        got = _body(K, re - rb, ldk, c.n, name)
        bad = np.argwhere(_bits(got) != _bits(ref))
        assert len(bad) == 0, (name, layout, seed, ldk, len(bad), bad[:5].tolist(),
                               [(got[i, j], ref[i, j]) for i, j in bad[:5]])
        again = _body(_gram_sparse(eng, d, rb, re, ldk), re - rb, ldk, c.n, name)
        assert _same(again, got)


@pytest.mark.parametrize("name", ["n130_W64", "probe_W4096"])
def test_gram_sparse_follows_the_given_shifts(eng, name):
    """Shifts of the rule minus 3: K must be the fixed-point sum at the shifts it is given."""
    c = _case(name)
    sh = c.shifts[0] - 3
    ref = _ref_rows(c, sh, "minus3")
    assert not _same(ref, _ref_rows(c, c.shifts[0], "rule"))
    d = Dev(eng, c.P, c.W, "packed", seed=3, shifts=sh)
    got = _body(_gram_sparse(eng, d, c.row_begin, c.row_end, c.n), c.row_end - c.row_begin, c.n, c.n, name)
    assert _same(got, ref)


# ------------------------------------------------------------------------------------------------------ k-slices
def test_gram_sparse_kslice_bitwise(eng):
    c = _case("n130_W64")
    sh = c.shifts[0]
    r = int(np.argmax(G.row_lengths(c.P)))
    ks = c.P.indices[c.P.indptr[r]:c.P.indptr[r + 1]]
    k = int(ks[len(ks) // 2])
    n = c.n
    d = Dev(eng, c.P, c.W, "line", seed=4)
    total = np.zeros((n, n), np.int64)
    for k0, k1 in ((0, k), (k, k + 1), (k + 1, n), (0, n), (k, k), (0, 0), (n, n)):
        ref, _, _, S = G.gram_fx_ref(c.P, sh, k_slice=(k0, k1))
        K = _nan_k(n, n, eng)
        _check(eng, eng.lib.grf_gram_sparse_kslice(n, 0, n, k0, k1, _p(d.ptr), _p(d.idx), _p(d.val), d.W, d.unit,
                                                   _p(d.desc), _p(d.rec), _p(d.sh), _p(K), n, NULL, 0, eng.stream),
               "grf_gram_sparse_kslice")
        got = _body(K, n, n, n, "kslice")
        print(f"kslice [{k0}, {k1}) of row {r}'s column {k}: {int((ref != 0).sum())} nonzero entries")
        assert _same(got, ref), (k0, k1)
        if (k0, k1) in ((0, k), (k, k + 1), (k + 1, n)):
            total += S
    assert np.array_equal(total, G.gram_fx_ref(c.P, sh)[3])      # the disjoint slices' integer sums add up


# -------------------------------------------------------------------------- symmetric entry points, parts, the split
def _upper(eng, d, K, ldk, pb, pe, np_, fn="upper", cuts=None, add=0, split=None):
    sp_ = d.split if split is None else split
    a = (d.n, _p(d.ptr), _p(d.idx), _p(d.val), d.W, d.unit, _p(d.desc), _p(d.rec), _p(sp_), _p(d.sh))
    if fn == "upper":
        rc = eng.lib.grf_gram_sparse_upper(*a, _p(K), ldk, pb, pe, np_, NULL, 0, eng.stream)
    elif fn == "add":
        rc = eng.lib.grf_gram_sparse_upper_add(*a, _p(K), ldk, pb, pe, np_, NULL, 0, eng.stream)
    else:
        rc = eng.lib.grf_gram_sparse_upper_ex(*a, _p(cuts), _p(K), ldk, pb, pe, np_, add, eng.stream)
    _check(eng, rc, "grf_gram_sparse_" + fn)


def _owned(c, tiles, split):
    own = np.zeros((c.n, c.n), bool)
    for t in tiles:
        c0, c1 = G.written_cols_ref(t, c.W, c.n, True, split)
        own[t[1], c0:c1] = True
    return own


SYM = [("n1_W64", "line", False), ("n5_W64", "packed", True), ("n65_W64", "line", True), ("n130_W64", "line", True),
       ("n130_W64", "packed", False), ("n130_W64", "packed", True), ("n400_W192", "line", True),
       ("n2600_W64", "packed", True)]


@pytest.mark.parametrize("name,layout,split", SYM)
def test_gram_upper_parts_mirror_sym_bitwise(eng, name, layout, split):
    """grf_gram_sparse_upper / _upper_ex in parts: every part writes exactly the columns of its tiles (a diagonal
    tile from its row's sub-band on with a split), with row i's bits; all parts + grf_gram_mirror and
    grf_gram_sparse_sym are sym_ref."""
    c = _case(name)
    n, sh = c.n, c.shifts[0]
    full = G.gram_fx_ref(c.P, sh)[0]
    symk = G.mirror_ref(full)
    nb = -(-n // c.W)
    tiles = G.tiles_ref(n, c.W, nb, True)
    ldk = n if name != "n2600_W64" else n + 4
    d = Dev(eng, c.P, c.W, layout, seed=6, split=split)
    if split:
        assert (d.split_host & 1).any() or n < 8
    print(f"{name}/{layout} split={split}: {len(tiles)} tiles in {nb} bands")
    parts = [(0, 1, 3), (1, 2, 3), (2, 3, 3)] + [(p, p + 1, len(tiles) + 2) for p in range(min(len(tiles) + 2, 9))]
    if name == "n2600_W64":
        parts = parts[:3]
    for fn in ("upper", "ex"):
        for pb, pe, np_ in parts:
            K = _nan_k(n, ldk, eng)
            _upper(eng, d, K, ldk, pb, pe, np_, fn)
            got = _body(K, n, ldk, n, name)
            t0, t1 = G.part_tiles_ref(len(tiles), pb, pe, np_)
            own = _owned(c, tiles[t0:t1], split)
            assert np.array_equal(~np.isnan(got), own), (fn, pb, pe, np_)
            assert np.array_equal(_bits(got)[own], _bits(full)[own]), (fn, pb, pe, np_)
    # all parts of a count above the tile count cover K once; then the mirror
    K = _nan_k(n, ldk, eng)
    np_ = 3 if name == "n2600_W64" else len(tiles) + 2
    for p in range(np_):
        _upper(eng, d, K, ldk, p, p + 1, np_)
    _check(eng, eng.lib.grf_gram_mirror(n, _p(K), ldk, 0, eng.stream), "grf_gram_mirror")
    assert _same(_body(K, n, ldk, n, name), symk)
    K = _nan_k(n, ldk, eng)
    _check(eng, eng.lib.grf_gram_sparse_sym(n, _p(d.ptr), _p(d.idx), _p(d.val), d.W, d.unit, _p(d.desc), _p(d.rec),
                                            _p(d.split), _p(d.sh), _p(K), ldk, NULL, 0, eng.stream), "grf_gram_sparse_sym")
    assert _same(_body(K, n, ldk, n, name), symk)
    if split:   # an all-zero split (a region too large for the transpose's LDS image): nothing is skipped
        z = torch.zeros_like(d.split)
        K = _nan_k(n, ldk, eng)
        _upper(eng, d, K, ldk, 0, 1, 1, split=z)
        got = _body(K, n, ldk, n, name)
        own = _owned(c, tiles, True)
        assert np.array_equal(~np.isnan(got), own) and np.array_equal(_bits(got)[own], _bits(full)[own])


@pytest.mark.parametrize("ldk_pad", [0, 2])
@pytest.mark.parametrize("split", [False, True])
def test_gram_upper_add_bitwise(eng, ldk_pad, split):
    """The add path onto a prior K of known floats: ldk = 130 takes the scalar write-out, ldk = 132 the vector one
    with its scalar tail (the last band is 2 wide)."""
    c = _case("n130_W64")
    n, sh = c.n, c.shifts[0]
    ldk = n + ldk_pad
    full = G.gram_fx_ref(c.P, sh)[0]
    rng = np.random.default_rng(12)
    prior = (rng.standard_normal((n, n)) * np.exp2(rng.integers(-6, 3, (n, n)))).astype(np.float32)
    tiles = G.tiles_ref(n, c.W, 3, True)
    own = _owned(c, tiles, split)
    want = np.where(own, G.add_ref(full, prior), prior)
    d = Dev(eng, c.P, c.W, "line", seed=7, split=split)
    for fn in ("add", "ex"):
        host = np.full(n * ldk + PAD, np.nan, np.float32)
        host[:n * ldk].reshape(n, ldk)[:, :n] = prior
        K = _t(host, eng)
        for p in range(3):
            _upper(eng, d, K, ldk, p, p + 1, 3, fn, add=1)
        got = _body(K, n, ldk, n, "upper_add")
        print(f"upper_add/{fn} ldk={ldk} split={split}: {int(own.sum())} entries added")
        assert _same(got, want), fn
    assert not _same(want, np.where(own, full, prior))


# -------------------------------------------------------------------------------------------------- the row cuts
def _cuts_case():
    rng = np.random.default_rng(21)
    lens = [0, 1, 7, 8, 9, 64, 65, 129] + [int(x) for x in rng.integers(0, 12, 122)]
    n = len(lens)
    rows = []
    for ln in lens:
        cc = np.sort(rng.choice(n, ln, replace=False)).astype(np.int32)
        rows.append((cc, G._values(rng, ln)))
    return G.Case("cuts130", G.csr(n, n, rows), 64)


def _row_cuts(eng, d, desc):
    col_w = torch.full((d.n_cols + PAD,), -5, dtype=torch.int32, device=eng.device)
    cuts = torch.full((8 * d.n + PAD,), -5, dtype=torch.int32, device=eng.device)
    _check(eng, eng.lib.grf_gram_row_cuts(d.n, _p(d.ptr), _p(d.idx), d.nb, d.n_cols, _p(desc), _p(col_w), _p(cuts),
                                          eng.stream), "grf_gram_row_cuts")
    cw, cu = col_w.cpu().numpy(), cuts.cpu().numpy()
    assert np.all(cw[d.n_cols:] == -5) and np.all(cu[8 * d.n:] == -5)
    return cw[:d.n_cols], cuts, cu[:8 * d.n]


def test_row_cuts_exact_and_k_unchanged(eng):
    c = _cuts_case()
    assert n_has(G.row_lengths(c.P), (0, 1, 7, 8, 9, 64, 65, 129))
    n = c.n
    d = Dev(eng, c.P, c.W, "line", seed=8)
    nbk = d.nb * n
    descs = {"real": d.desc_host.copy()}
    z = d.desc_host.copy()
    z[1:2 * nbk:2] = 0
    descs["all-zero weights"] = z
    long_row = int(np.argmax(G.row_lengths(c.P)))
    ks = c.P.indices[c.P.indptr[long_row]:c.P.indptr[long_row + 1]]
    for tag, k in (("dominant first", ks[0]), ("dominant last", ks[-1])):
        w = d.desc_host.copy()
        w[2 * (1 * n + int(k)) + 1] = 1 << 20
        descs[tag] = w
    for tag, desc in descs.items():
        cw, cuts_dev, cu = _row_cuts(eng, d, _t(desc.view(np.int32), eng))
        ref_w = G.col_pairs_ref(desc, d.nb, n)
        ref_c = G.row_cuts_ref(c.P, ref_w)
        print(f"row cuts / {tag}: row {long_row} cuts {cu.reshape(n, 8)[long_row].tolist()}")
        assert np.array_equal(cw, ref_w), tag
        assert np.array_equal(cu, ref_c), tag
        lens = G.row_lengths(c.P)
        assert np.all(cu.reshape(n, 8) <= lens[:, None]) and np.all(np.diff(cu.reshape(n, 8), axis=1) >= 0)
        # K with these (valid, monotone, in-row) cuts is the plain call's
        full = G.gram_fx_ref(c.P, c.shifts[0])[0]
        own = _owned(c, G.tiles_ref(n, c.W, d.nb, True), False)
        K = _nan_k(n, n, eng)
        _upper(eng, d, K, n, 0, 1, 1, "ex", cuts=cuts_dev)
        got = _body(K, n, n, n, tag)
        assert np.array_equal(~np.isnan(got), own) and np.array_equal(_bits(got)[own], _bits(full)[own]), tag


def n_has(lens, want):
    return set(want) <= set(int(x) for x in lens)


# ------------------------------------------------------------------------------------------------- column blocks
def _cols_case():
    """Phi 1200 x 640; Phi_B = Phi[10:580] (570 rows: 9 bands of 64, a ragged last one, t_rows != n_cols).  Rows
    0 .. 9 hold the round-robin edge counts, an empty row and a share past 64 nonzeros per wave of 8."""
    rng = np.random.default_rng(31)
    n_rows, n_cols = 1200, 640
    lens = [127, 128, 129, 512, 513, 0, 600, 63, 64, 65] + [int(x) for x in rng.integers(0, 14, n_rows - 10)]
    lens[700] = 0
    rows = []
    for ln in lens:
        cc = np.sort(rng.choice(n_cols, ln, replace=False)).astype(np.int32)
        rows.append((cc, G._values(rng, ln)))
    return G.csr(n_rows, n_cols, rows)


def _gram_cols(eng, d, rb, re, sym0, ldk):
    K = _nan_k(re - rb, ldk, eng)
    _check(eng, eng.lib.grf_gram_sparse_cols(d.n_cols, rb, re, _p(d.ptr), _p(d.idx), _p(d.val), _p(d.sh), d.t_rows, sym0,
                                             d.W, d.unit, _p(d.desc), _p(d.rec), _p(d.split), _p(K), ldk, NULL, 0,
                                             eng.stream), "grf_gram_sparse_cols")
    return K


@pytest.fixture(scope="module")
def cols_ref():
    P = _cols_case()
    sh = G.rowshift_ref(P)[0]
    PB = P[10:580]
    return P, PB, sh, G.gram_fx_ref(P, sh, t_rows_block=PB)[0]


@pytest.mark.parametrize("layout", ["line", "packed"])
def test_gram_cols_round_robin_bitwise(eng, cols_ref, layout):
    P, PB, sh, ref = cols_ref
    assert n_has(G.row_lengths(P), G.NNZ_RR)
    d = Dev(eng, P, 64, layout, seed=9, PB=PB, shifts=sh)
    for rb, re, ldk in ((0, 40, 570), (3, 700, 572), (699, 702, 571)):
        got = _body(_gram_cols(eng, d, rb, re, -1, ldk), re - rb, ldk, 570, layout)
        print(f"cols/{layout}: rows [{rb}, {re}) ldk {ldk}")
        assert _same(got, ref[rb:re]), (rb, re)
    # the symmetric square K[B, B] with rows before and after it: the lower triangle carries the upper's bits
    for split in (False, True):
        ds = Dev(eng, P, 64, layout, seed=10, PB=PB, shifts=sh, split=split)
        got = _body(_gram_cols(eng, ds, 2, 600, 10, 572), 598, 572, 570, layout)
        want = ref[2:600].copy()
        want[8:578] = G.mirror_ref(ref[10:580])
        assert _same(got, want), split


@pytest.mark.parametrize("pipe", ["0", "1"])
def test_gram_cols_slot_bitwise(eng, cols_ref, pipe, monkeypatch):
    """Slot buckets: the tile-per-workgroup kernel (GRF_GRAM_PIPE=0) and the persistent pipelined one, whose
    workgroups own 1, 1 .. 2 and >= 4 tiles (grid = CUs x workgroups per CU by the kernel's LDS size)."""
    P, PB, sh, ref = cols_ref
    monkeypatch.setenv("GRF_GRAM_PIPE", pipe)
    d = Dev(eng, P, 64, "slot", seed=11, PB=PB, shifts=sh)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    lds = 64 * 8 + 8 * (G.CHUNK + 2 * 64 * 8)
    grid = cus * max(1, 160 * 1024 // lds)
    owned = set()
    for rb, re, ldk in ((5, 25, 570), (100, 100 + -(-3 * grid // 18), 572), (0, 1200, 571)):
        tiles = (re - rb) * 9
        owned |= {tiles // min(grid, tiles), -(-tiles // min(grid, tiles))}
        got = _body(_gram_cols(eng, d, rb, re, -1, ldk), re - rb, ldk, 570, "slot")
        print(f"cols/slot pipe={pipe}: rows [{rb}, {re}) = {tiles} tiles on {min(grid, tiles)} workgroups")
        assert _same(got, ref[rb:re]), (rb, re)
    if cus <= 256:
        assert {1, 2} <= owned and max(owned) >= 4, owned


@pytest.mark.parametrize("pipe", ["0", "1"])
def test_gram_cols_slot_long_streams_bitwise(eng, pipe, monkeypatch):
    """probe_W8192 through the column-block entry (PB = P, rows [0, row_end), no symmetric square): its 8 waves of
    equal contiguous shares are the pipelined kernel's share rule, so that kernel -- otherwise run on streams of a
    few pairs -- meets the 512 and 1024 chunks, the carry across chunks and every tail window count.  Same
    reference rows as test_gram_sparse_rows_bitwise[probe_W8192-slot]; ldk % 4 == 0 (vector write-out) and != 0."""
    c = _case("probe_W8192")
    sh = c.shifts[0]
    ref = _ref_rows(c, sh, "rule")
    rb, re, n = c.row_begin, c.row_end, c.n
    assert rb == 0 and c.edges["waves"] == 8
    monkeypatch.setenv("GRF_GRAM_PIPE", pipe)
    d = Dev(eng, c.P, c.W, "slot", seed=13, PB=c.P, shifts=sh)
    for ldk in (n + 4, n + 1):
        got = _body(_gram_cols(eng, d, rb, re, -1, ldk), re - rb, ldk, n, "probe_W8192 cols")
        bad = np.argwhere(_bits(got) != _bits(ref))
        print(f"cols/slot probe_W8192 pipe={pipe} ldk={ldk}: rows [{rb}, {re}) x {n} columns, {len(bad)} differ")
        assert len(bad) == 0, (pipe, ldk, len(bad), bad[:5].tolist(), [(got[i, j], ref[i, j]) for i, j in bad[:5]])


def test_gram_cols_padded_bitwise(eng, cols_ref):
    """Padded rows (cnt = 0 and cnt == cap among them) give the CSR path's bits."""
    P, PB, sh, ref = cols_ref
    cap = int(G.row_lengths(P).max())
    cnt, idx, val = G.to_padded(P, cap)
    assert (cnt == 0).any() and (cnt == cap).any()
    d = Dev(eng, P, 64, "slot", seed=12, PB=PB, shifts=sh)
    slack = 128
    idx_d = _t(np.concatenate([idx, np.zeros(slack, np.int32)]), eng)
    val_d = _t(np.concatenate([val, np.zeros(slack, np.float32)]), eng)
    cnt_d = _t(cnt, eng)
    for rb, re, ldk in ((0, 1200, 570), (6, 7, 572)):
        K = _nan_k(re - rb, ldk, eng)
        _check(eng, eng.lib.grf_gram_sparse_cols_padded(640, rb, re, cap, _p(cnt_d), _p(idx_d), _p(val_d), _p(d.sh), 570,
                                                        64, _p(d.desc), _p(d.rec), _p(K), ldk, eng.stream),
               "grf_gram_sparse_cols_padded")
        assert _same(_body(K, re - rb, ldk, 570, "padded"), ref[rb:re]), (rb, re)


# ---------------------------------------------------------------------------------------------------- the mirror
@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 129, 200])
def test_gram_mirror_alone(eng, n):
    rng = np.random.default_rng(n)
    for ldk in (n, -(-n // 4) * 4 + (4 if n % 4 == 0 else 0)):
        for wgs in (0, 1, 3, 10 ** 6):
            src = rng.standard_normal((n, n)).astype(np.float32)
            src[np.triu_indices(n)] = (np.arange(n * (n + 1) // 2) + 1).astype(np.float32)   # distinct upper values
            host = np.full(n * ldk + PAD, np.nan, np.float32)
            host[:n * ldk].reshape(n, ldk)[:, :n] = src
            K = _t(host, eng)
            _check(eng, eng.lib.grf_gram_mirror(n, _p(K), ldk, wgs, eng.stream), "grf_gram_mirror")
            got = _body(K, n, ldk, n, "mirror")
            assert _same(got, G.mirror_ref(src)), (n, ldk, wgs)
    print(f"mirror n={n}: {(-(-n // 64)) * (-(-n // 64) + 1) // 2} blocks")


# ------------------------------------------------------------------------------------ hub panel, drop, densify
def _small_case():
    rng = np.random.default_rng(41)
    lens = [0, 1, 64, 65, 130, 300] + [int(x) for x in rng.integers(0, 9, 20)]
    n_cols = 320
    rows = []
    for ln in lens:
        cc = np.sort(rng.choice(n_cols, ln, replace=False)).astype(np.int32)
        rows.append((cc, G._values(rng, ln)))
    return G.csr(len(lens), n_cols, rows)


def test_hub_panel_and_drop_columns(eng):
    P = _small_case()
    n, n_cols = P.shape
    ptr, idx, val = _t(np.asarray(P.indptr, np.int64), eng), _t(P.indices.astype(np.int32), eng), _t(P.data, eng)
    rng = np.random.default_rng(42)
    for tag, hubs in (("no hubs", []), ("some", sorted(rng.choice(n_cols, 37, replace=False).tolist())),
                      ("all hubs", list(range(n_cols)))):
        hub_pos = np.full(n_cols, -1, np.int32)
        hub_pos[hubs] = rng.permutation(len(hubs)).astype(np.int32)
        ldp = len(hubs) + 3
        Pn = torch.full((n * ldp + PAD,), float("nan"), dtype=torch.float32, device=eng.device)
        pos_d = _t(hub_pos, eng)
        _check(eng, eng.lib.grf_hub_panel(n, _p(ptr), _p(idx), _p(val), _p(pos_d), _p(Pn), ldp, eng.stream),
               "grf_hub_panel")
        host = Pn.cpu().numpy()
        want = G.hub_panel_ref(P, hub_pos, ldp, fill=np.nan)
        assert np.array_equal(_bits(host[:n * ldp].reshape(n, ldp)), _bits(want)) and np.all(np.isnan(host[n * ldp:])), tag
        # drop: 37 columns x 7 bands = 259 items (not a multiple of 256), none, all
        nb = 7
        desc = rng.integers(1, 1000, 2 * (nb * n_cols + 1)).astype(np.uint32)
        dd = _t(np.concatenate([desc, np.full(PAD, 77, np.uint32)]).view(np.int32), eng)
        cols = _t(np.asarray(hubs, np.int32), eng) if hubs else None
        _check(eng, eng.lib.grf_transpose_drop_columns(nb, n_cols, _p(dd), _p(cols), len(hubs), eng.stream),
               "grf_transpose_drop_columns")
        got = dd.cpu().numpy().view(np.uint32)
        assert np.array_equal(got[:len(desc)], G.drop_columns_ref(desc, nb, n_cols, hubs)), tag
        assert np.all(got[len(desc):] == 77)
        print(f"hub panel / drop: {tag}: {len(hubs)} columns x {nb} bands")


def test_densify_and_padded(eng):
    P = _small_case()
    n, n_cols = P.shape
    ptr, idx, val = _t(np.asarray(P.indptr, np.int64), eng), _t(P.indices.astype(np.int32), eng), _t(P.data, eng)
    for lda in (n_cols, n_cols + 5):
        out = torch.full((n * lda + PAD,), float("nan"), dtype=torch.float32, device=eng.device)
        _check(eng, eng.lib.grf_densify(n, _p(ptr), _p(idx), _p(val), _p(out), lda, eng.stream), "grf_densify")
        host = out.cpu().numpy()
        assert np.array_equal(_bits(host[:n * lda].reshape(n, lda)), _bits(G.densify_ref(P, lda)))
        assert np.all(np.isnan(host[n * lda:]))
    cap = 300
    cnt, pidx, pval = G.to_padded(P, cap)
    assert (cnt == 0).any() and (cnt == cap).any() and (cnt > 256).any()
    pidx[pidx < 0] = 0
    cnt_d, idx_d, val_d = _t(cnt, eng), _t(pidx, eng), _t(pval, eng)      # (held: the launch reads them)
    for lda in (n_cols, n_cols + 8):
        out = torch.full((n * lda + PAD,), float("nan"), dtype=torch.float32, device=eng.device)
        _check(eng, eng.lib.grf_densify_padded(n, cap, n_cols, _p(cnt_d), _p(idx_d), _p(val_d), _p(out), lda, eng.stream),
               "grf_densify_padded")
        host = out.cpu().numpy()
        assert np.array_equal(_bits(host[:n * lda].reshape(n, lda)), _bits(G.densify_padded_ref(cnt, pidx, pval, cap, lda)))
        assert np.all(np.isnan(host[n * lda:]))
    print(f"densify: rows {G.row_lengths(P)[:6].tolist()} lda {n_cols}, {n_cols + 5}, {n_cols + 8}")


# ------------------------------------------------------------------------------------------ the device transposes
def _decode_device(tr, nb, n_cols):
    desc = tr.t_desc.cpu().numpy().view(np.uint32).copy()
    rec = tr.t_rec.cpu().numpy()
    nbk = nb * n_cols
    if tr.rec_unit == G.REC_SLOT:       # the slots carry the pair counts
        desc[1:2 * nbk:2] = rec[:32 * nbk].view(np.uint32).reshape(nbk, 8)[:, 0]
    return G.decode_transpose(desc, rec, tr.rec_unit, nb, n_cols, tr.band_width), desc


MODES = {"atomic": dict(staged=False, self_count=False), "staged": dict(staged=True, self_count=False),
         "self": dict(self_count=True), "self+split": dict(self_count=True, split=True),
         "slot": dict(self_count=True, rec_unit=G.REC_SLOT)}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ["n1_W64", "n65_W64", "n130_W64", "n400_W192", "n130_down40", "hub4100",
                                  "dense128_W128"])
def test_device_transposes_match_host_built(eng, name, mode):
    """engine.transpose_banded in every fill: the same pairs and the same multiset of (row offset, value bits) per
    bucket as the host-built transpose, t_split equal where it is non-zero, the rule's shifts on decided rows
    (grf_phi_row_shifts and _padded too), and K from it bit-equal to the reference."""
    from grf_amd.engine import DeviceCSR, PaddedRows
    c = _case(name)
    n = c.n
    sh, decided, mx = c.shifts
    phi = DeviceCSR(n, n, _t(np.asarray(c.P.indptr, np.int64), eng), _t(c.P.indices.astype(np.int32), eng),
                    None, _t(c.P.data, eng), _nnz=int(c.P.nnz))
    for unit in ((G.REC_LINE, G.REC_PACKED) if mode != "slot" else (G.REC_SLOT,)):
        kw = dict(MODES[mode])
        kw["rec_unit"] = unit
        tr = eng.transpose_banded(phi, c.W, **kw)
        nb = -(-n // c.W)
        got, desc = _decode_device(tr, nb, n)
        layout = {G.REC_LINE: "line", G.REC_PACKED: "packed", G.REC_SLOT: "slot"}[unit]
        kwh = {"split": True} if mode == "self+split" else {}
        hdesc, hrec, hsplit = BUILD[layout](c.P, c.W, **kwh)
        want = G.decode_transpose(hdesc, hrec, unit, nb, n, c.W)
        coo = c.P.tocoo()
        n_ent = dict(zip(*np.unique((coo.row // c.W).astype(np.int64) * n + coo.col, return_counts=True)))
        assert np.array_equal(desc[1:2 * nb * n:2], hdesc[1:2 * nb * n:2]), (mode, unit)
        assert set(got) == set(want)
        for b in want:
            assert sorted(got[b]) == sorted(want[b]), (mode, unit, b)
        if mode == "self+split":
            ds = tr.t_split.cpu().numpy().view(np.uint16).reshape(-1, 8)
            nz = ds.any(axis=1)
            assert np.array_equal(ds[nz], hsplit[nz])
            for b in np.flatnonzero(nz):      # laid out by sub-band (an odd bucket's last record is the pad)
                sub = np.array([e[0] for e in got[int(b)][:n_ent[int(b)]]]) * G.K_SUB // c.W
                assert np.all(np.diff(sub) >= 0), (mode, unit, int(b))
        dsh = tr.t_rowshift.cpu().numpy()[:n]
        assert np.array_equal(dsh[decided], sh[decided]), (mode, unit)
        assert _bits(tr.t_maxabs.cpu().numpy())[0] == _bits(np.array([mx], np.float32))[0]
        rb, re = c.row_begin, c.row_end
        K = _nan_k(re - rb, n, eng)
        _check(eng, eng.lib.grf_gram_sparse(n, rb, re, _p(phi.ptr), _p(phi.idx), _p(phi.val32), c.W, unit, _p(tr.t_desc),
                                            _p(tr.t_rec), _p(tr.t_rowshift), _p(K), n, NULL, 0, eng.stream),
               "grf_gram_sparse")
        ref = G.gram_fx_ref(c.P, dsh, rows=np.arange(rb, re))[0]
        assert _same(_body(K, re - rb, n, n, name), ref), (mode, unit)
    s1 = eng.phi_row_shifts(phi).cpu().numpy()[:n]
    cap = max(1, int(G.row_lengths(c.P).max()))
    cnt, pidx, pval = G.to_padded(c.P, cap)
    s2 = eng.phi_row_shifts(PaddedRows(_t(cnt, eng), _t(np.maximum(pidx, 0), eng), None, _t(pval, eng), cap, n)).cpu().numpy()[:n]
    assert np.array_equal(s1[decided], sh[decided]) and np.array_equal(s1, s2) and np.array_equal(s1, dsh)
    print(f"device transpose {mode} / {name}: {int(decided.sum())} of {n} rows decided")
