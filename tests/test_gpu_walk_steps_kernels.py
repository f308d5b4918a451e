"""GPU: the walk, step, Phi and compaction kernels (grf_walk.hip, grf_philox.h, grf_steps.hip and the scan,
compaction and concat parts of grf_sparse.hip) called through their C entry points on hand-built inputs at
the shapes where their branches change, against the restatements of tests/walk_steps_reference.py (pinned
on the CPU by tests/test_walk_steps_reference.py).

Every comparison is bitwise, on the uint views of the values (NaN results by position only): the references
restate the kernels' arithmetic operation by operation in the orders the kernels promise -- loads in walk
order from 0.0, Phi terms in step order from 0.0 + first, one IEEE division or one multiplication by
RN(1 / m).  Output buffers are longer than what the call owns and pre-filled (-77 / NaN); the pad, and in
a padded row everything past cnt[s], must come back untouched.

Held here: grf_steps up to m = 16384 (131,200 B of dynamic LDS per workgroup), every (positions per
thread, threads) pair grf_phi_fused's host plan reaches, 32- and 64-bit keys on both sides of the switch,
runs that cross a thread's block / end on a block edge / reach the last key, the Divisor's fast window and
its IEEE fall-back over every exponent, L = 1 and 2 walks, zero-degree sources, overflowing loads, both
augmented record formats, empty PCG64 chunks, the bucket counts, the three scan levels, the compaction's
row-group tails and the concat's grid-stride loop.

Deliberately not held: the Lemire rejection tail (philox_lemire_retry and the while loop of
Pcg64::integers fire with probability < deg / 2^32 per step: out of reach at testable degrees), and the
experiment switches GRF_PHI_THREADS, GRF_PHI_SORT_LDS and GRF_PHI_LDS_PAD (read once per process; unset).
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import walk_steps_reference as R

pytestmark = pytest.mark.gpu

SENT_I, PAD = -77, 9
NULL = ctypes.c_void_p(0)
NORMS = (R.NORM_DIV, R.NORM_MUL_RECIP)
KINDS = ("int", "real")


@pytest.fixture(scope="module")
def eng():
    from grf_amd.engine import GRFEngine
    return GRFEngine("cuda:0")


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else NULL


def _t(a, eng, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(eng.device)


def _ints(n, eng, dtype=torch.int32):
    return torch.full((int(n),), SENT_I, dtype=dtype, device=eng.device)


def _nans(n, eng, dtype=torch.float64):
    return torch.full((int(n),), float("nan"), dtype=dtype, device=eng.device)


def _host(t):
    return None if t is None else t.cpu().numpy()


def _same(got, ref):
    """Bitwise equality of two arrays of one dtype and shape; NaNs are compared by position only."""
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    if got.dtype != ref.dtype or got.shape != ref.shape:
        return False
    if got.dtype.kind != "f":
        return bool(np.array_equal(got, ref))
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    gn, rn = np.isnan(got), np.isnan(ref)
    return bool(np.array_equal(gn, rn) and np.array_equal(got.view(u)[~gn], ref.view(u)[~rn]))


def _rc(eng, name, *args):
    return int(getattr(eng.lib, name)(*args))


def _ok(eng, name, *args):
    from grf_amd import _lib as C
    C.check(_rc(eng, name, *args), name)


def _padded_rows(cnt, idx, vals, cap, n_src, dtypes):
    """The padded buffers a Phi call must leave: row s holds its first cnt[s] entries, -77 / NaN elsewhere
    (the PAD tail included)."""
    oi = np.full(n_src * cap + PAD, SENT_I, np.int32)
    ov = [np.full(n_src * cap + PAD, np.nan, dt) for dt in dtypes]
    for s in range(n_src):
        k = int(cnt[s])
        oi[s * cap:s * cap + k] = idx[s][:k]
        for o, v in zip(ov, vals):
            o[s * cap:s * cap + k] = v[s][:k]
    return oi, ov


# ------------------------------------------------------------------------------------------- grf_steps
def _steps(eng, node, load, norm):
    ns, L, m = node.shape
    cnt = _ints(ns * L + PAD, eng)
    idx = _ints(ns * L * m + PAD, eng)
    val = _nans(ns * L * m + PAD, eng)
    dn, dl = _t(node, eng), _t(load, eng)          # (held in names: the inputs outlive the call)
    _ok(eng, "grf_steps", ns, m, L, norm, _p(dn), _p(dl), _p(cnt), _p(idx), _p(val), eng.stream)
    return _host(cnt), _host(idx), _host(val)


@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 255, 256, 257, 4096, 4097, 8192, 8193, 16384])
def test_steps_exact(eng, m):
    """Counts, indices and values of every (source, step) row bit-equal to steps_ref for both norms, L in
    {1, 3}, n_src in {1, 5} and both kinds of load; nothing past cnt in a row, nothing past the buffers.
    Above m = 4096 the workgroup takes more than 64 KiB of dynamic LDS (131,200 B at m = 16384)."""
    for kind in KINDS:
        for L in (1, 3):
            for n_src in (1, 5):
                node, load = R.slots_case(m, L, n_src, kind)
                for norm in NORMS:
                    rcnt, ridx, rval = R.pack_steps(R.steps_ref(node, load, norm), m)
                    cnt, idx, val = _steps(eng, node, load, norm)
                    tag = (kind, L, n_src, norm)
                    g = n_src * L
                    assert np.array_equal(cnt[:g], rcnt) and np.all(cnt[g:] == SENT_I), tag
                    assert np.array_equal(idx[:g * m], ridx) and np.all(idx[g * m:] == SENT_I), tag
                    assert _same(val[:g * m], rval) and np.all(np.isnan(val[g * m:])), tag


def test_steps_argument_edges(eng):
    """m = 16385 is refused (GRF_EUNSUPPORTED) before any launch; n_src = 0 is OK and writes nothing."""
    from grf_amd import _lib as C
    buf_i, buf_f = _ints(16385 + PAD, eng), _nans(16385 + PAD, eng)
    node, load = _t(np.zeros(16385, np.int32), eng), _t(np.ones(16385), eng)
    assert _rc(eng, "grf_steps", 1, 16385, 1, R.NORM_DIV, _p(node), _p(load), _p(buf_i), _p(buf_i), _p(buf_f),
               eng.stream) == C.GRF_EUNSUPPORTED
    assert _rc(eng, "grf_steps", 0, 7, 3, R.NORM_DIV, _p(node), _p(load), _p(buf_i), _p(buf_i), _p(buf_f),
               eng.stream) == C.GRF_OK
    assert _rc(eng, "grf_steps", 1, 7, 3, 2, _p(node), _p(load), _p(buf_i), _p(buf_i), _p(buf_f),
               eng.stream) == C.GRF_EINVAL
    torch.cuda.synchronize()
    assert np.all(_host(buf_i) == SENT_I) and np.all(np.isnan(_host(buf_f)))


# ----------------------------------------------------------------------------------- grf_steps_densify
@pytest.mark.parametrize("n_src,L", [(1, 1), (1, 3), (3, 1), (2, 2), (4, 1), (5, 1), (1, 5)])
def test_steps_densify_exact(eng, n_src, L):
    """Rows of 0, 1, 64, 65 and 130 entries scattered into a zero-filled [n_src, n_cols, L] array: the
    written cells equal the step values, every other cell (and the pad) stays zero."""
    m, n_cols = 130, 300
    rng = np.random.default_rng(11 + n_src * 7 + L)
    lens = [0, 1, 64, 65, 130]
    g_n = n_src * L
    cnt = np.array([lens[(g + L) % 5] for g in range(g_n)], np.int32)
    idx = np.full(g_n * m, SENT_I, np.int32)
    val = np.full(g_n * m, np.nan)
    want = np.zeros(n_src * n_cols * L + PAD)
    for g in range(g_n):
        k = int(cnt[g])
        cols = np.sort(rng.choice(200, size=k, replace=False))
        v = R.loads(rng, (k,), "real", m)
        idx[g * m:g * m + k], val[g * m:g * m + k] = cols, v
        s, l = divmod(g, L)
        want[(s * n_cols + cols) * L + l] = v
    out = torch.zeros(n_src * n_cols * L + PAD, dtype=torch.float64, device=eng.device)
    d_cnt, d_idx, d_val = _t(cnt, eng), _t(idx, eng), _t(val, eng)
    _ok(eng, "grf_steps_densify", n_src, m, L, n_cols, _p(d_cnt), _p(d_idx), _p(d_val), _p(out), eng.stream)
    assert _same(_host(out), want)


# --------------------------------------------------------------------------------------------- grf_phi
def _caps(row_len):
    return sorted({1, max(1, row_len - 1), max(1, row_len), row_len + 5})


def _phi(eng, packed, n_src, m, L, f, n_f, cap, want32):
    cnt = _ints(n_src + PAD, eng)
    idx = _ints(n_src * cap + PAD, eng)
    v64 = _nans(n_src * cap + PAD, eng)
    v32 = _nans(n_src * cap + PAD, eng, torch.float32) if want32 else None
    ft = None if f is None else _t(np.asarray(f, np.float64), eng)
    _ok(eng, "grf_phi", n_src, m, L, _p(packed[0]), _p(packed[1]), _p(packed[2]), _p(ft), n_f, cap, _p(cnt), _p(idx),
        _p(v64), _p(v32), eng.stream)
    return _host(cnt), _host(idx), _host(v64), _host(v32)


def _check_rows(out, ref, cap, n_src, tag):
    cnt, idx, v64, v32 = out
    rcnt, ridx, r64, r32 = ref
    assert np.array_equal(cnt[:n_src], rcnt) and np.all(cnt[n_src:] == SENT_I), tag
    wi, (w64, w32) = _padded_rows(rcnt, ridx, (r64, r32), cap, n_src, (np.float64, np.float32))
    assert np.array_equal(idx, wi), tag
    if v64 is not None:
        assert _same(v64, w64), tag
    if v32 is not None:
        assert _same(v32, w32), tag


@pytest.mark.parametrize("L", [1, 2, 63, 64])
def test_phi_merge_exact(eng, L):
    """grf_phi on step rows from steps_ref (not from the GPU): every modulator (real, with zeros,
    (1, -1, 0, ...), n_f = 0 with f = NULL, L - 1, L + 3), phi_cap in {1, row length - 1, row length,
    row length + 5}, with and without the fp32 output; L = 64 is the merge's lane limit."""
    m, n_src = 7, 5
    for kind in KINDS:
        node, load = R.slots_case(m, L, n_src, kind, seed=2)
        for norm in NORMS:
            rows = R.steps_ref(node, load, norm)
            packed = [_t(a, eng) for a in R.pack_steps(rows, m)]
            for name, f, n_f in R.modulators(L, kind):
                row_len = int(R.phi_ref(rows, f, n_f, m * L + 9)[0].max())
                for cap in _caps(row_len):
                    ref = R.phi_ref(rows, f, n_f, cap)
                    for want32 in (True, False):
                        _check_rows(_phi(eng, packed, n_src, m, L, f, n_f, cap, want32), ref, cap, n_src,
                                    (kind, norm, name, cap, want32))


def test_phi_merge_argument_edges(eng):
    from grf_amd import _lib as C
    bi, bf = _ints(65 * 8 + PAD, eng), _nans(65 * 8 + PAD, eng)
    cnt = torch.zeros(65, dtype=torch.int32, device=eng.device)
    f = _t(np.ones(65), eng)
    args = lambda L, nf, cap, fp: (1, 8, L, _p(cnt), _p(bi), _p(bf), fp, nf, cap, _p(bi), _p(bi), _p(bf), NULL, eng.stream)
    assert _rc(eng, "grf_phi", *args(65, 65, 8, _p(f))) == C.GRF_EUNSUPPORTED
    assert _rc(eng, "grf_phi", *args(3, 3, 0, _p(f))) == C.GRF_EINVAL
    assert _rc(eng, "grf_phi", *args(3, 3, 8, NULL)) == C.GRF_EINVAL
    torch.cuda.synchronize()
    assert np.all(_host(bi) == SENT_I) and np.all(np.isnan(_host(bf)))


# --------------------------------------------------------------------------------------- grf_phi_fused
def _phi_fused(eng, node, load, norm, f, n_f, cap, want32):
    n_src, L, m = node.shape
    cnt = _ints(n_src + PAD, eng)
    idx = _ints(n_src * cap + PAD, eng)
    v64 = _nans(n_src * cap + PAD, eng)
    v32 = _nans(n_src * cap + PAD, eng, torch.float32) if want32 else None
    ft = None if f is None else _t(np.asarray(f, np.float64), eng)
    _ok(eng, "grf_phi_fused", n_src, m, L, norm, _p(node), _p(load), _p(ft), n_f, cap, _p(cnt), _p(idx), _p(v64),
        _p(v32), eng.stream)
    return _host(cnt), _host(idx), _host(v64), _host(v32)


FULL_MATRIX = [(13, 5), (64, 8)]  # the shapes that run every modulator, cap and NULL combination


@pytest.mark.parametrize("shape", [s for s, _ in R.FUSED_SHAPES], ids=lambda s: f"m{s[0]}_L{s[1]}")
def test_phi_fused_exact(eng, shape):
    """Every (positions per thread, threads) pair of the host plan against phi_ref(steps_ref(...)) on the
    planted rows (all empty, one node, all distinct, runs of kPer - 1 .. 2 kPer + 3 across and on block
    edges, full rows, node ids at 2^31 - 1), both kinds of load and both norms; two shapes run every
    modulator, cap and NULL output."""
    m, L = shape
    for kind in KINDS:
        node, load, _ = R.fused_case(m, L, kind)
        n_src = node.shape[0]
        dn, dl = _t(node, eng), _t(load, eng)
        for norm in NORMS:
            rows = R.steps_ref(node, load, norm)
            mods = R.modulators(L, kind)
            for name, f, n_f in (mods if shape in FULL_MATRIX else mods[:1]):
                row_len = int(R.phi_ref(rows, f, n_f, m * L + 9)[0].max())
                for cap in (_caps(row_len) if shape in FULL_MATRIX else [max(1, m * L)]):
                    ref = R.phi_ref(rows, f, n_f, cap)
                    for want32 in ((True, False) if shape in FULL_MATRIX else (True,)):
                        _check_rows(_phi_fused(eng, dn, dl, norm, f, n_f, cap, want32), ref, cap, n_src,
                                    (kind, norm, name, cap, want32))


@pytest.mark.parametrize("m", [1, 3, 7, 100])
def test_phi_fused_divisor_every_exponent(eng, m):
    """NORM_DIV through the fused kernel's Divisor: loads at every biased exponent 0..2046 (four mantissas,
    both signs), +-0, subnormals and +-inf, each alone in its run, so an entry is (0.0 + load) / m -- the
    fast window, both of its edges and the IEEE fall-back -- against numpy's division."""
    node, load, L = R.divisor_case(m)
    n_src, cap = node.shape[0], m * L
    f = np.ones(L)
    ref = R.phi_ref(R.steps_ref(node, load, R.NORM_DIV), f, L, cap)
    flat = np.concatenate(ref[2])
    with np.errstate(all="ignore"):
        want = (0.0 + load.reshape(n_src, -1)) / np.float64(m)
    assert _same(flat, want[want != 0.0])                           # (the restatement is numpy's acc / m)
    assert np.isinf(flat).sum() >= 2 and int(ref[0].sum()) < load.size
    _check_rows(_phi_fused(eng, _t(node, eng), _t(load, eng), R.NORM_DIV, f, L, cap, True), ref, cap, n_src, m)


def test_phi_fused_argument_edges(eng):
    from grf_amd import _lib as C
    bi, bf = _ints(4097 + PAD, eng), _nans(4097 + PAD, eng)
    node, load = _t(np.zeros(4097, np.int32), eng), _t(np.ones(4097), eng)
    f = _t(np.ones(1), eng)
    assert _rc(eng, "grf_phi_fused", 1, 4097, 1, R.NORM_DIV, _p(node), _p(load), _p(f), 1, 4097, _p(bi), _p(bi),
               _p(bf), NULL, eng.stream) == C.GRF_EUNSUPPORTED
    assert _rc(eng, "grf_phi_fused", 1, 17, 241, R.NORM_DIV, _p(node), _p(load), _p(f), 1, 4097, _p(bi), _p(bi),
               _p(bf), NULL, eng.stream) == C.GRF_EUNSUPPORTED
    assert _rc(eng, "grf_phi_fused", 0, 8, 8, R.NORM_DIV, _p(node), _p(load), _p(f), 1, 64, _p(bi), _p(bi), _p(bf),
               NULL, eng.stream) == C.GRF_OK
    torch.cuda.synchronize()
    assert np.all(_host(bi) == SENT_I) and np.all(np.isnan(_host(bf)))


# ------------------------------------------------------------------------------ grf_walk / grf_walk_ex
class _Graph:
    """A walk matrix on the device (the index and value arrays hold one element when nnz = 0: the entry
    points refuse NULL)."""

    def __init__(self, eng, ptr, idx, val):
        self.n, self.nnz = len(ptr) - 1, len(idx)
        self.ptr = _t(np.asarray(ptr, np.int64), eng)
        self.idx = _t(np.asarray(idx, np.int32) if len(idx) else np.zeros(1, np.int32), eng)
        self.val = _t(np.asarray(val, np.float64) if len(idx) else np.zeros(1), eng)


def _params(m, p, L, rule, rng, n_chunks=1, seed=42):
    from grf_amd import _lib as C
    return C.GrfWalkParams(m, float(p), L, rule, rng, 0, n_chunks, seed)


def _aug(eng, G, allow16):
    """grf_walk_aug in the 16-byte (allow16) or 32-byte record format; checks the header words and that
    nothing is written past the records."""
    nbytes = int(eng.lib.grf_walk_aug_bytes(G.nnz))
    assert nbytes == 32 + 32 * G.nnz
    aug = torch.full((nbytes + 32,), 0xAB, dtype=torch.uint8, device=eng.device)
    assert aug.data_ptr() % 32 == 0
    old = os.environ.get("GRF_WALK_AUG16")
    os.environ["GRF_WALK_AUG16"] = "1" if allow16 else "0"
    try:
        _ok(eng, "grf_walk_aug", G.n, _p(G.ptr), _p(G.idx), _p(G.val), _p(aug), eng.stream)
    finally:
        if old is None:
            del os.environ["GRF_WALK_AUG16"]
        else:
            os.environ["GRF_WALK_AUG16"] = old
    host = _host(aug)
    fmt, tb, rb = R.aug_header(G.n, G.nnz, allow16)
    assert tuple(host[:12].view(np.int32)) == (fmt, tb, rb), (G.n, G.nnz, allow16)
    assert np.all(host[32 + (16 if fmt else 32) * G.nnz:] == 0xAB)
    return aug


def _walk(eng, G, aug, prm, b, e, expect=None):
    from grf_amd import _lib as C
    m, L = prm.walks_per_node, prm.max_walk_length
    size = (e - b) * L * m
    node, load = _ints(size + PAD, eng), _nans(size + PAD, eng)
    rc = _rc(eng, "grf_walk_ex", G.n, _p(G.ptr), _p(G.idx), _p(G.val), _p(aug), ctypes.byref(prm), b, e, _p(node),
             _p(load), eng.stream) if aug is not None else \
        _rc(eng, "grf_walk", G.n, _p(G.ptr), _p(G.idx), _p(G.val), ctypes.byref(prm), b, e, _p(node), _p(load), eng.stream)
    if expect is not None:
        assert rc == expect
    else:
        C.check(rc, "grf_walk")
    node, load = _host(node), _host(load)
    assert np.all(node[size:] == SENT_I) and np.all(np.isnan(load[size:]))
    return node[:size].reshape(e - b, L, m), load[:size].reshape(e - b, L, m)


@pytest.mark.parametrize("mode", ["plain", "aug16", "aug32"])
@pytest.mark.parametrize("rng", [0, 1], ids=["pcg64", "philox"])
def test_walk_deterministic_graphs(eng, rng, mode):
    """Weighted directed cycles, paths into a sink, empty graphs (n in {1, 2, 5}) and a cycle whose weights
    overflow the load: L in {1, 2, 3, 4, 7} (both ends of the pair-wise step loop), m in {1, 3, 65}, the
    three load rules, against det_walk_ref -- visits, the -1 fill, and the loads wherever a node was
    recorded."""
    for name, ptr, idx, val in R.det_graphs():
        G = _Graph(eng, ptr, idx, val)
        aug = None if mode == "plain" else _aug(eng, G, mode == "aug16")
        for L in (1, 2, 3, 4, 7):
            for m in (1, 3, 65):
                for rule in (0, 1, 2):
                    want_n, want_l = R.det_walk_ref(ptr, idx, val, m, 0.0, L, rule)
                    node, load = _walk(eng, G, aug, _params(m, 0.0, L, rule, rng), 0, G.n)
                    tag = (name, L, m, rule)
                    assert np.array_equal(node, want_n), tag
                    live = want_n >= 0
                    assert _same(load[live], want_l[live]), tag
                    if name == "huge5" and rule == 0 and L >= 3:
                        assert np.isinf(load[live]).any()


def _small_graph(n, seed):
    """A random directed graph with out-degree 1..3 (no node stops a walk early), random weights."""
    rng = np.random.default_rng(seed)
    rows = [np.sort(rng.choice(n, size=int(rng.integers(1, min(n, 3) + 1)), replace=False)) for _ in range(n)]
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    idx = np.concatenate(rows).astype(np.int32)
    return ptr, idx, rng.uniform(0.2, 3.0, idx.size)


def test_walk_pcg64_chunks(eng):
    """The PCG64 replay against the oracle at n = 5 with n_chunks in {1, 5, 8} (8 > n: empty chunks, the
    bisection's ties), over all sources and over a proper union of chunks; a range that splits a chunk is
    GRF_EINVAL and writes nothing."""
    from grf_amd import _lib as C
    from oracle import oracle as O
    ptr, idx, val = _small_graph(5, 3)
    G = _Graph(eng, ptr, idx, val)
    m, p, L = 3, 0.3, 4
    for n_chunks, ranges in ((1, [(0, 5)]), (5, [(0, 5), (1, 3), (4, 5)]), (8, [(0, 5), (2, 5), (0, 1), (5, 5)])):
        want_n, want_l = O.walk_slots(ptr, idx, val, m, p, L, rng=O.RNG_PCG64, n_chunks=n_chunks, seed=9)
        for aug in (None, _aug(eng, G, True), _aug(eng, G, False)):
            for b, e in ranges:
                node, load = _walk(eng, G, aug, _params(m, p, L, 0, C.RNG_PCG64, n_chunks, 9), b, e)
                assert np.array_equal(node, want_n[b:e]), (n_chunks, b, e)
                live = node >= 0
                assert _same(load[live], want_l[b:e][live]), (n_chunks, b, e)
    assert (want_n[:, 1:] >= 0).any() and (want_n == -1).any()
    for b, e in ((1, 3), (0, 2), (4, 5), (2, 3)):               # n = 5 in two chunks: [0, 3) and [3, 5)
        node, load = _walk(eng, G, None, _params(m, p, L, 0, C.RNG_PCG64, 2, 9), b, e, expect=C.GRF_EINVAL)
        assert np.all(node == SENT_I) and np.all(np.isnan(load))


# ---------------------------------------------------------------------------------------- grf_walk_phi
def _cluster(c, seed):
    """A connected undirected cluster of c nodes: a ring plus random chords, symmetric random weights."""
    rng = np.random.default_rng(seed)
    W = np.zeros((c, c))
    for i in range(c):
        W[i, (i + 1) % c] = W[(i + 1) % c, i] = rng.uniform(0.2, 2.0)
    for _ in range(2 * c):
        i, j = rng.integers(0, c, size=2)
        if i != j:
            W[i, j] = W[j, i] = rng.uniform(0.2, 2.0)
    rows, cols = np.nonzero(W)
    ptr = np.concatenate([[0], np.cumsum((W != 0).sum(axis=1))]).astype(np.int64)
    return ptr, cols.astype(np.int32), W[rows, cols]


class _TopCluster:
    """n nodes, all isolated but a connected cluster on the c top node ids; ptr is built on the device."""

    def __init__(self, eng, n, c=64, seed=5):
        ptr, idx, val = _cluster(c, seed)
        self.n, self.nnz, self.first = n, len(idx), n - c
        self.ptr = torch.zeros(n + 1, dtype=torch.int64, device=eng.device)
        self.ptr[n - c:] = _t(ptr, eng)
        self.idx = _t(idx + np.int32(n - c), eng)
        self.val = _t(val, eng)


def _walk_phi(eng, G, aug, prm, b, e, norm, f, n_f, cap, want64=True, want32=True, t_count=None, bw=0, row0=0,
              expect=None):
    from grf_amd import _lib as C
    ns = e - b
    cnt = _ints(ns + PAD, eng)
    idx = _ints(ns * cap + PAD, eng)
    v64 = _nans(ns * cap + PAD, eng) if want64 else None
    v32 = _nans(ns * cap + PAD, eng, torch.float32) if want32 else None
    ft = None if f is None else _t(np.asarray(f, np.float64), eng)
    rc = _rc(eng, "grf_walk_phi", G.n, _p(G.ptr), _p(G.idx), _p(G.val), _p(aug), ctypes.byref(prm), b, e, norm, _p(ft),
             n_f, cap, _p(cnt), _p(idx), _p(v64), _p(v32), _p(t_count), bw, row0, eng.stream)
    if expect is not None:
        assert rc == expect
    else:
        C.check(rc, "grf_walk_phi")
    return _host(cnt), _host(idx), _host(v64), _host(v32)


def _walk_phi_against_walk(eng, G, m, L, p, b, e, rule=0, full=False):
    """grf_walk_phi on sources [b, e) against phi_ref(steps_ref(the slots grf_walk writes for them)), without
    and with the augmented matrix, both norms; ``full``: also phi_val = NULL, no fp32 copy, a cap that cuts."""
    from grf_amd import _lib as C
    prm = _params(m, p, L, rule, C.RNG_PHILOX, 1, 1234567 + m)
    node, load = _walk(eng, G, None, prm, b, e)
    assert (node[:, 0, :] == np.arange(b, e)[:, None]).all()
    kind = "real"
    mods = R.modulators(L, kind)
    augs = (None, _aug(eng, G, True), _aug(eng, G, False)) if G.n < 4096 else (None, _aug(eng, G, True))
    cap = max(1, min(m * L, G.n))
    for norm in NORMS:
        rows = R.steps_ref(node, load, norm)
        for name, f, n_f in (mods if full else mods[:1]):
            ref = R.phi_ref(rows, f, n_f, cap)
            for aug in augs:
                _check_rows(_walk_phi(eng, G, aug, prm, b, e, norm, f, n_f, cap), ref, cap, e - b, (m, L, norm, name))
            if full:
                _check_rows(_walk_phi(eng, G, None, prm, b, e, norm, f, n_f, cap, want64=False), ref, cap, e - b, name)
                _check_rows(_walk_phi(eng, G, None, prm, b, e, norm, f, n_f, cap, want32=False), ref, cap, e - b, name)
                small = max(1, int(ref[0].max()) - 1)
                _check_rows(_walk_phi(eng, G, None, prm, b, e, norm, f, n_f, small), R.phi_ref(rows, f, n_f, small),
                            small, e - b, (name, "cut"))
    return node


@pytest.fixture(scope="module")
def cluster200(eng):
    return _Graph(eng, *_cluster(200, 1))


@pytest.mark.parametrize("shape", [s for s, _ in R.FUSED_SHAPES], ids=lambda s: f"m{s[0]}_L{s[1]}")
def test_walk_phi_fused_shapes(eng, cluster200, shape):
    """The walking kernel at every plan of FUSED_SHAPES on a connected cluster of 200 nodes with p_halt > 0
    (32-bit keys; the unrolled variants at (128, 8) and (64, 8)): the step-0 shortcut, real runs and halted
    walks all occur."""
    m, L = shape
    node = _walk_phi_against_walk(eng, cluster200, m, L, 0.15, 17, 23, full=shape in FULL_MATRIX)
    if L >= 3:
        assert (node[:, -1, :] == -1).any() and (node[:, -1, :] >= 0).any()      # halted and full-length walks


@pytest.mark.parametrize("m,L,n", [(4096, 1, 2 ** 19 - 1), (4096, 1, 2 ** 19), (128, 8, 2 ** 22 - 1), (128, 8, 2 ** 22)])
def test_walk_phi_key_width_boundary(eng, m, L, n):
    """n_cols << (wbits + lbits) on both sides of 2^32: the last graph with 32-bit keys and the first with
    64-bit keys, the walked cluster on the top node ids (the keys next to the sentinel)."""
    wb, lb = R.key_bits(m, L)
    assert ((n << (wb + lb)) <= 0xffffffff) == (n % 2 == 1) and (((n + 1) // 2 * 2) << (wb + lb)) == 2 ** 32
    G = _TopCluster(eng, n)
    node = _walk_phi_against_walk(eng, G, m, L, 0.1, n - 6, n, full=True)
    assert node.max() == n - 1 and node[node >= 0].min() >= G.first


@pytest.mark.parametrize("shape", [s for s, _ in R.FUSED_SHAPES if sum(R.key_bits(*s)) >= 10],
                         ids=lambda s: f"m{s[0]}_L{s[1]}")
def test_walk_phi_wide_keys_shapes(eng, shape):
    """The walking kernel with 64-bit keys at the other plans: n = 2^22 nodes put every shape whose walk and
    step bits reach 10 past the 32-bit limit."""
    m, L = shape
    n = 2 ** 22
    assert (n << sum(R.key_bits(m, L))) > 0xffffffff
    _walk_phi_against_walk(eng, _TopCluster(eng, n), m, L, 0.15, n - 5, n)


@pytest.mark.parametrize("row0", [0, 17])
@pytest.mark.parametrize("bw", [1, 50, 8192])
def test_walk_phi_bucket_counts(eng, cluster200, row0, bw):
    """t_count equals the histogram of ((row - count_row0) // band_width, col) over the entries returned,
    and nothing else is touched."""
    from grf_amd import _lib as C
    G, m, L, b, e = cluster200, 16, 4, 17, 137
    cap = min(m * L, G.n)
    n_bands = (e - 1 - row0) // bw + 1
    t_count = _ints(n_bands * G.n + PAD, eng)
    t_count[:n_bands * G.n] = 0
    f = R.modulators(L, "real")[0][1]
    prm = _params(m, 0.2, L, 0, C.RNG_PHILOX, 1, 77)
    cnt, idx, _, _ = _walk_phi(eng, G, None, prm, b, e, R.NORM_MUL_RECIP, f, L, cap, t_count=t_count, bw=bw, row0=row0)
    want = np.zeros(n_bands * G.n + PAD, np.int32)
    want[n_bands * G.n:] = SENT_I
    for s in range(e - b):
        cols = idx[s * cap:s * cap + cnt[s]]
        np.add.at(want, ((b + s - row0) // bw) * G.n + cols, 1)
    assert cnt[:e - b].min() >= 2 and np.array_equal(_host(t_count), want)


def test_walk_phi_argument_edges(eng, cluster200):
    """With t_count: a cap that could cut a row, and count_row0 > src_begin, are GRF_EINVAL; PCG64 is
    GRF_EUNSUPPORTED; nothing is written."""
    from grf_amd import _lib as C
    G, m, L = cluster200, 16, 4
    f = np.ones(L)
    t_count = torch.zeros(G.n * 200, dtype=torch.int32, device=eng.device)
    prm = _params(m, 0.2, L, 0, C.RNG_PHILOX)
    outs = [_walk_phi(eng, G, None, prm, 17, 30, 0, f, L, m * L - 1, t_count=t_count, bw=50, row0=0, expect=C.GRF_EINVAL),
            _walk_phi(eng, G, None, prm, 17, 30, 0, f, L, m * L, t_count=t_count, bw=50, row0=18, expect=C.GRF_EINVAL),
            _walk_phi(eng, G, None, prm, 17, 30, 0, f, L, m * L, t_count=t_count, bw=0, row0=0, expect=C.GRF_EINVAL),
            _walk_phi(eng, G, None, _params(m, 0.2, L, 0, C.RNG_PCG64), 17, 30, 0, f, L, m * L,
                      expect=C.GRF_EUNSUPPORTED)]
    for cnt, idx, v64, v32 in outs:
        assert np.all(cnt == SENT_I) and np.all(idx == SENT_I) and np.all(np.isnan(v64)) and np.all(np.isnan(v32))
    assert int(t_count.abs().sum().item()) == 0


# ------------------------------------------------------------------------------------- grf_scan_counts
def _scan(eng, cnt, n, short=0):
    ptr = _ints(n + 1 + PAD, eng, torch.int64)
    nbytes = int(eng.lib.grf_scan_workspace_bytes(n))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=eng.device)
    rc = _rc(eng, "grf_scan_counts", n, _p(cnt), _p(ptr), _p(ws), nbytes - short, eng.stream)
    return rc, ptr, nbytes


@pytest.mark.parametrize("n", [0, 1, 4095, 4096, 4097, 4096 ** 2, 4096 ** 2 + 1])
def test_scan_counts_exact(eng, n):
    """One, two and three levels of 4096-element tiles against torch.cumsum in int64; ptr[n] is written for
    n = 0; nothing past ptr[n]."""
    from grf_amd import _lib as C
    g = torch.Generator(device=eng.device)
    g.manual_seed(n + 1)
    cnt = torch.randint(0, 9, (max(n, 1),), dtype=torch.int32, device=eng.device, generator=g)
    rc, ptr, nbytes = _scan(eng, cnt, n)
    assert rc == C.GRF_OK
    levels = 0 if n <= 4096 else (1 if n <= 4096 ** 2 else 2)
    assert (nbytes > 0) == (levels > 0)
    assert int(ptr[0].item()) == 0
    assert torch.equal(ptr[1:n + 1], torch.cumsum(cnt[:n].to(torch.int64), 0))
    assert bool((ptr[n + 1:] == SENT_I).all())


def test_scan_counts_large_totals_and_short_workspace(eng):
    """Counts near 2^31 - 1 carry the total past 2^32 (and past 2^43 over two levels); a workspace one byte
    short is GRF_EINVAL and writes nothing."""
    from grf_amd import _lib as C
    for n in (5, 4097):
        cnt = (2 ** 31 - 1) - torch.arange(n, dtype=torch.int32, device=eng.device) % 7
        rc, ptr, _ = _scan(eng, cnt, n)
        assert rc == C.GRF_OK
        want = torch.cumsum(cnt.to(torch.int64), 0)
        assert int(want[-1].item()) > 2 ** 32 and torch.equal(ptr[1:n + 1], want) and int(ptr[0].item()) == 0
    rc, ptr, nbytes = _scan(eng, cnt, 4097, short=1)
    assert nbytes > 0 and rc == C.GRF_EINVAL and bool((ptr == SENT_I).all())


# --------------------------------------------------------- grf_compact_rows / grf_compact_rows_stats
COUNTS = [0, 1, 63, 64, 65, 127, 128, 129, 300]


def _padded_input(n_rows, cap, seed):
    rng = np.random.default_rng(seed)
    cnt = np.array([COUNTS[(r + n_rows) % len(COUNTS)] for r in range(n_rows)], np.int32)
    idx = rng.integers(0, 2 ** 31 - 1, size=n_rows * cap).astype(np.int32)
    v64 = R.loads(rng, (n_rows * cap,), "real", 1)
    v32 = v64.astype(np.float32)
    ptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    take = np.concatenate([r * cap + np.arange(cnt[r]) for r in range(n_rows)]).astype(np.int64)
    return cnt, ptr, idx, v64, v32, take


@pytest.mark.parametrize("n_rows", [1, 3, 4, 5, 15, 16, 17])
def test_compact_rows_exact(eng, n_rows):
    """Rows of 0 / 1 / 63 / 64 / 65 / 127 / 128 / 129 / 300 entries (cap = 300; four rows per wave, 128
    entries per trip; the last group of rows is short) gathered into the CSR at out_ptr for every allowed
    combination of NULL value outputs; the two refused combinations are GRF_EINVAL."""
    from grf_amd import _lib as C
    cap = 300
    cnt, ptr, idx, v64, v32, take = _padded_input(n_rows, cap, 40 + n_rows)
    total = int(ptr[-1])
    d = [_t(a, eng) for a in (cnt, ptr, idx, v64, v32)]
    for want64 in (True, False):
        for want32 in (True, False):
            oi, o64, o32 = _ints(total + PAD, eng), _nans(total + PAD, eng), _nans(total + PAD, eng, torch.float32)
            _ok(eng, "grf_compact_rows", n_rows, cap, _p(d[0]), _p(d[1]), _p(d[2]), _p(d[3]), _p(d[4]), _p(oi),
                _p(o64) if want64 else NULL, _p(o32) if want32 else NULL, eng.stream)
            oi, o64, o32 = _host(oi), _host(o64), _host(o32)
            assert np.array_equal(oi[:total], idx[take]) and np.all(oi[total:] == SENT_I)
            assert _same(o64[:total], v64[take]) if want64 else np.all(np.isnan(o64[:total]))
            assert _same(o32[:total], v32[take]) if want32 else np.all(np.isnan(o32[:total]))
            assert np.all(np.isnan(o64[total:])) and np.all(np.isnan(o32[total:]))
    oi, o64, o32 = _ints(total + PAD, eng), _nans(total + PAD, eng), _nans(total + PAD, eng, torch.float32)
    assert _rc(eng, "grf_compact_rows", n_rows, cap, _p(d[0]), _p(d[1]), _p(d[2]), NULL, _p(d[4]), _p(oi), _p(o64),
               _p(o32), eng.stream) == C.GRF_EINVAL
    assert _rc(eng, "grf_compact_rows", n_rows, cap, _p(d[0]), _p(d[1]), _p(d[2]), _p(d[3]), NULL, _p(oi), _p(o64),
               _p(o32), eng.stream) == C.GRF_EINVAL
    assert np.all(_host(oi) == SENT_I) and np.all(np.isnan(_host(o64))) and np.all(np.isnan(_host(o32)))


@pytest.mark.parametrize("n_rows", [1, 3, 4, 5, 15, 16, 17])
def test_compact_rows_stats_exact(eng, n_rows):
    """The same gather with the row statistics: row_max bit-equal to numpy's max |v| (0 for an empty row),
    and the shifts grf_phi_row_shifts_stats derives from them bit-equal to grf_phi_row_shifts on the
    compacted matrix."""
    cap = 300
    cnt, ptr, idx, v64, v32, take = _padded_input(n_rows, cap, 60 + n_rows)
    total = int(ptr[-1])
    d = [_t(a, eng) for a in (cnt, ptr, idx, v64, v32)]
    sbytes = int(eng.lib.grf_phi_row_shifts_workspace_bytes(n_rows))
    for want64 in (True, False):
        oi, o64, o32 = _ints(total + PAD, eng), _nans(total + PAD, eng), _nans(total + PAD, eng, torch.float32)
        stats = torch.full((sbytes + 256,), 0xAB, dtype=torch.uint8, device=eng.device)
        _ok(eng, "grf_compact_rows_stats", n_rows, cap, _p(d[0]), _p(d[1]), _p(d[2]), _p(d[3]) if want64 else NULL,
            _p(d[4]), _p(oi), _p(o64) if want64 else NULL, _p(o32), _p(stats), sbytes, eng.stream)
        assert np.array_equal(_host(oi)[:total], idx[take]) and np.all(_host(oi)[total:] == SENT_I)
        assert _same(_host(o32)[:total], v32[take]) and np.all(np.isnan(_host(o32)[total:]))
        assert _same(_host(o64)[:total], v64[take]) if want64 else np.all(np.isnan(_host(o64)))
        # (the statistics block is opaque in grf.h; row_stats_layout of grf_sparse.hip puts the n_rows fp32
        #  row maxima first, then, each 256-byte aligned, the fp64 row sums and the per-wave maxima)
        row_max = _host(stats)[:4 * n_rows].view(np.float32)
        want = np.array([np.abs(v32[r * cap:r * cap + cnt[r]]).max() if cnt[r] else 0.0 for r in range(n_rows)],
                        np.float32)
        assert _same(row_max, want)
        assert np.all(_host(stats)[sbytes:] == 0xAB)
        ma, sh = _nans(1 + PAD, eng, torch.float32), _ints(n_rows + PAD, eng)
        _ok(eng, "grf_phi_row_shifts_stats", n_rows, _p(stats), _p(ma), _p(sh), eng.stream)
        mb, sb = _nans(1 + PAD, eng, torch.float32), _ints(n_rows + PAD, eng)
        ws = torch.empty(sbytes, dtype=torch.uint8, device=eng.device)
        _ok(eng, "grf_phi_row_shifts", n_rows, _p(d[1]), _p(o32), _p(mb), _p(sb), _p(ws), sbytes, eng.stream)
        assert _same(_host(ma), _host(mb)) and np.array_equal(_host(sh), _host(sb))
        assert np.all(_host(sh)[n_rows:] == SENT_I) and _same(_host(ma)[:1], want.max(keepdims=True))
    from grf_amd import _lib as C
    assert _rc(eng, "grf_compact_rows_stats", n_rows, cap, _p(d[0]), _p(d[1]), _p(d[2]), NULL, _p(d[4]), _p(oi),
               _p(o64), _p(o32), _p(stats), sbytes, eng.stream) == C.GRF_EINVAL
    assert _rc(eng, "grf_compact_rows_stats", n_rows, cap, _p(d[0]), _p(d[1]), _p(d[2]), _p(d[3]), _p(d[4]), _p(oi),
               _p(o64), _p(o32), _p(stats), sbytes - 1, eng.stream) == C.GRF_EINVAL


# --------------------------------------------------------------------------------- grf_concat_segments
@pytest.mark.parametrize("stride", [0, 1, 300, 2048 * 256 + 5])
@pytest.mark.parametrize("n_seg", [0, 1, 3])
def test_concat_segments_exact(eng, n_seg, stride):
    """Segments of length 0, 1 and stride (the grid-stride loop runs past 2048 * 256 elements) copied to
    offsets with gaps between them: equal to numpy's concatenation, the gaps and the pad untouched."""
    rng = np.random.default_rng(5 + n_seg + stride)
    lens = np.array([[stride, 0, min(1, stride)][r % 3] for r in range(n_seg)], np.int64)
    off = (np.concatenate([[0], np.cumsum(lens + 3)])[:n_seg] + 2).astype(np.int64)
    src = rng.integers(0, 2 ** 31 - 1, size=max(n_seg * stride, 1)).astype(np.int32)
    size = int(lens.sum()) + 3 * n_seg + 2 + PAD
    want = np.full(size, SENT_I, np.int32)
    for r in range(n_seg):
        want[off[r]:off[r] + lens[r]] = src[r * stride:r * stride + lens[r]]
    dst = _ints(size, eng)
    if n_seg == 0:
        _ok(eng, "grf_concat_segments", 0, stride, NULL, NULL, NULL, NULL, eng.stream)
    else:
        d_src, d_len, d_off = _t(src, eng), _t(lens, eng), _t(off, eng)
        _ok(eng, "grf_concat_segments", n_seg, stride, _p(d_src), _p(d_len), _p(d_off), _p(dst), eng.stream)
    assert np.array_equal(_host(dst), want)
