"""GPU: what the C entry points do around their argument checks, on real buffers.

Every buffer handed to an entry lies between 64 sentinel words, outputs are pre-filled with the sentinel, and every
bad argument used here would stay inside the buffers even if its check were missing (a byte count one short of a
full-size workspace, a workspace moved by 128 bytes inside a buffer 128 bytes longer, a leading dimension of
width - 1 on a full-width buffer, an enum out of range, a t_rec_bytes one unit short of a full-size t_rec): no NULL
and no made-up pointer (those are tests/test_abi_contracts.py's, in a process without a device).

* test_refused_call_writes_nothing_and_poisons_nothing -- after each refused call every word of every buffer
  (inputs, outputs, workspaces, sentinels) is what it was; the valid call that follows on the same workspace gives
  the bits of the same call on buffers prepared afresh.  (The banded transposes leave the record order inside a
  bucket unspecified, so their records are compared through the row-mode Gram of them, an order-free integer sum.)
  grf_scan_counts needs no workspace up to 4096 counts, so its case alone has n = 5000.
* test_empty_call -- n = 0 (and n_rhs = 0, nnz = 0, n_drop = 0 where allowed) returns GRF_OK and writes only
  what include/grf.h says: l_ptr[0] = 0 (Laplacians), out[0] = 0 (scan), t_ptr[0 .. n_cols] = 0 (CSR transpose),
  the total 0 in t_desc and max |Phi| = 0 (transposes, row shifts), grad = 0 (dense step gradient), else nothing.
* test_laplacian_*_cap_too_small -- the data-dependent cap l_cap in {0, 1, nnz - 1, nnz}: nothing at or past
  l_cap is written, the entries below it are the oracle's prefix bit for bit, l_ptr is the oracle's full row
  pointer (so l_ptr[n] > l_cap tells the caller).

The header's `*_cap` arguments and their tests:
  l_cap    grf_laplacian_csr / grf_laplacian_dense          here (test_laplacian_csr_cap_too_small, _dense_)
  phi_cap  grf_phi / grf_phi_fused / grf_walk_phi            tests/test_gpu_walk_steps_kernels.py (the phi_cap cuts)
(`cap` of grf_compact_rows*, grf_phi_row_shifts_padded, grf_densify_padded*, grf_gram_sparse_cols_padded is the
row pitch of an input, not an output cap.)
"""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import torch

pytestmark = pytest.mark.gpu

SENT = 0x7FC12345  # a NaN no kernel produces
PAD = 64           # sentinel words before and after every buffer (256 bytes: the payload keeps its alignment)
OK, EINVAL, ECAPACITY, EUNSUPPORTED = 0, -1, -3, -4
REFUSALS = (EINVAL, ECAPACITY, EUNSUPPORTED)
_T = {np.dtype(np.int32): torch.int32, np.dtype(np.int64): torch.int64, np.dtype(np.float32): torch.float32,
      np.dtype(np.float64): torch.float64, np.dtype(np.uint8): torch.uint8}


@pytest.fixture(scope="module")
def eng():
    from grf_amd.engine import GRFEngine
    return GRFEngine("cuda:0")


class Buf:
    """`nbytes` of device memory between sentinel words, holding `init` (a numpy array), `fill` bytes or sentinels."""

    def __init__(self, eng, nbytes=0, init=None, zero=False):
        if init is not None:
            init = np.ascontiguousarray(init)
            nbytes = max(nbytes, init.nbytes)
        self.nw = max(2, (int(nbytes) + 7) // 8 * 2)
        self.raw = torch.full((PAD + self.nw + PAD,), SENT, dtype=torch.int32, device=eng.device)
        assert self.raw.data_ptr() % 256 == 0
        if zero:
            self.raw[PAD:PAD + self.nw] = 0
        if init is not None and init.size:
            self.raw[PAD:PAD + self.nw].view(_T[init.dtype])[:init.size] = torch.from_numpy(init.ravel()).to(eng.device)

    def p(self, off=0):
        return ctypes.c_void_p(self.raw.data_ptr() + 4 * PAD + off)

    def words(self):
        return self.raw.cpu().numpy().view(np.uint32).copy()

    def get(self, dtype, count):
        w = self.words()
        assert np.all(w[:PAD] == SENT) and np.all(w[PAD + self.nw:] == SENT), "a word outside the buffer was written"
        return w[PAD:PAD + self.nw].view(dtype)[:count].copy()


def rest_is_sentinel(buf, n_bytes_written):
    w = buf.words()
    k = (n_bytes_written + 3) // 4
    return bool(np.all(w[:PAD] == SENT) and np.all(w[PAD + k:] == SENT))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32 if a.dtype.itemsize == 4 else np.uint8)


# ---------------------------------------------------------------------- shared inputs (built once, never changed)
_SHARED = {}


def shared(name, make):
    if name not in _SHARED:
        _SHARED[name] = make()
    return _SHARED[name]


def phi_csr():
    """Phi: 130 x 130, float32 values, an empty row, rows of 1 .. 40 entries (two bands of 64 and a last one of 2)."""
    def make():
        r = np.random.default_rng(5)
        n = 130
        ptr, idx = [0], []
        for i in range(n):
            k = 0 if i == 3 else int(r.integers(1, 41))
            idx.extend(np.sort(r.choice(n, k, replace=False)).tolist())
            ptr.append(len(idx))
        val = r.uniform(-1.0, 1.0, len(idx)).astype(np.float32)
        return n, np.asarray(ptr, np.int64), np.asarray(idx, np.int32), val
    return shared("phi", make)


def lap_csr_case():
    """n = 72, rows of 0, 1, 7, 63, 64, 65 and 70 entries: group rows and whole-wave rows together."""
    def make():
        from oracle import oracle as O
        r = np.random.default_rng(7)
        n, lengths = 72, [0, 1, 7, 63, 64, 65, 70]
        ptr, idx = [0], []
        for i in range(n):
            idx.extend(np.sort(r.choice(n, lengths[i % len(lengths)], replace=False)).tolist())
            ptr.append(len(idx))
        val = r.uniform(0.1, 2.0, len(idx))
        A = sp.csr_matrix((val, np.asarray(idx, np.int32), np.asarray(ptr, np.int64)), shape=(n, n))
        L, _ = O.laplacian_sparse(A)
        return A, L
    return shared("lap_csr", make)


def lap_dense_case():
    """n = 130, rows with 0, 1, 126, 127, 128 and 129 nonzeros: staged rows and rows re-read from W."""
    def make():
        from oracle import oracle as O
        r = np.random.default_rng(8)
        n, lengths = 130, [0, 1, 126, 127, 128, 129]
        W = np.zeros((n, n))
        for i in range(n):
            k = lengths[i % len(lengths)]
            W[i, r.choice(n, k, replace=False)] = r.uniform(0.1, 2.0, k)
        ip, ix, dx = O.dense_to_walk_csr(O.laplacian_dense(W, 1))   # GRF_LAP_NUMPY_SAFE = the oracle's mode 1
        return W, ip, ix, dx
    return shared("lap_dense", make)


# ---------------------------------------------------------------------- refused calls
class Setup:
    """One entry on fresh buffers: call(**changes) -> status, result() -> {name: bits}, bads: the refused changes,
    named: the buffers by argument name."""
    bufs = ()
    named = {}
    bads = ()


def setup_laplacian_csr(eng):
    A, _ = lap_csr_case()
    n, cap = A.shape[0], A.nnz + A.shape[0]
    need = eng.lib.grf_laplacian_csr_workspace_bytes(n)
    s = Setup()
    b = dict(a_ptr=Buf(eng, init=A.indptr.astype(np.int64)), a_idx=Buf(eng, init=A.indices.astype(np.int32)),
             a_val=Buf(eng, init=A.data), l_ptr=Buf(eng, 8 * (n + 1)), l_idx=Buf(eng, 4 * cap), l_val=Buf(eng, 8 * cap),
             deg=Buf(eng, 8 * n), dinv=Buf(eng, 8 * n), ws=Buf(eng, need))
    s.bufs, s.named = list(b.values()), b

    def call(mode=0, ws_bytes=need):
        return eng.lib.grf_laplacian_csr(n, b["a_ptr"].p(), b["a_idx"].p(), b["a_val"].p(), mode, b["l_ptr"].p(),
                                         b["l_idx"].p(), b["l_val"].p(), cap, b["deg"].p(), b["dinv"].p(), b["ws"].p(),
                                         ws_bytes, eng.stream)
    s.call = call
    s.result = lambda: {k: b[k].words() for k in ("l_ptr", "l_idx", "l_val", "deg", "dinv")}
    s.bads = [dict(ws_bytes=need - 1), dict(mode=1), dict(mode=7), dict(mode=-1)]
    return s


def setup_laplacian_dense(eng):
    W = lap_dense_case()[0]
    n, cap = W.shape[0], W.shape[0] ** 2
    need = eng.lib.grf_laplacian_dense_workspace_bytes(n)
    s = Setup()
    b = dict(W=Buf(eng, init=W), l_ptr=Buf(eng, 8 * (n + 1)), l_idx=Buf(eng, 4 * cap), l_val=Buf(eng, 8 * cap),
             deg=Buf(eng, 8 * n), ws=Buf(eng, need + 128))
    s.bufs, s.named = list(b.values()), b

    def call(mode=2, ws_off=0, ws_bytes=need):
        return eng.lib.grf_laplacian_dense(n, b["W"].p(), mode, b["l_ptr"].p(), b["l_idx"].p(), b["l_val"].p(), cap,
                                           b["deg"].p(), b["ws"].p(ws_off), ws_bytes, eng.stream)
    s.call = call
    s.result = lambda: {k: b[k].words() for k in ("l_ptr", "l_idx", "l_val", "deg")}
    s.bads = [dict(ws_bytes=need - 1), dict(ws_off=128), dict(mode=0), dict(mode=9)]
    return s


def setup_scan_counts(eng):
    n = 5000
    cnt = shared("scan_cnt", lambda: np.random.default_rng(9).integers(0, 50, n).astype(np.int32))
    need = eng.lib.grf_scan_workspace_bytes(n)
    assert need > 0
    s = Setup()
    b = dict(cnt=Buf(eng, init=cnt), out=Buf(eng, 8 * (n + 1)), ws=Buf(eng, need))
    s.bufs, s.named = list(b.values()), b
    s.call = lambda ws_bytes=need: eng.lib.grf_scan_counts(n, b["cnt"].p(), b["out"].p(), b["ws"].p(), ws_bytes,
                                                           eng.stream)
    s.result = lambda: {"out": b["out"].words()}
    s.bads = [dict(ws_bytes=need - 1), dict(ws_bytes=0)]
    s.check = lambda: np.array_equal(b["out"].get(np.int64, n + 1), np.concatenate([[0], np.cumsum(cnt, dtype=np.int64)]))
    return s


def setup_transpose_self(eng, rec):
    n, ptr, idx, val = phi_csr()
    bw, unit, nnz = 64, 128, len(idx)
    nbk = -(-n // bw) * n
    lib = eng.lib
    need, stg = lib.grf_transpose_self_workspace_bytes(n, n, bw), lib.grf_transpose_staging_bytes(n, n, bw, nnz)
    kind = 1 if rec else 0   # (the _rec entry is exercised on record triples)
    units = (lib.grf_transpose_self_triples_lines_bound(n, n, bw, nnz) if rec else
             lib.grf_transpose_self_units_bound(n, n, bw, unit, nnz))
    s = Setup()
    b = dict(ptr=Buf(eng, init=ptr), idx=Buf(eng, init=idx), val=Buf(eng, init=val), t_desc=Buf(eng, 8 * (nbk + 1)),
             t_rec=Buf(eng, units * unit), t_max=Buf(eng, 4), t_shift=Buf(eng, 4 * n), ws=Buf(eng, need),
             stg=Buf(eng, stg), K=Buf(eng, 4 * n * n))
    s.bufs, s.named = list(b.values()), b

    def call(rec_kind=kind, rec_unit=unit, t_rec_bytes=units * unit, ws_bytes=need, stg_bytes=stg):
        args = (n, n, bw, rec_unit, b["ptr"].p(), b["idx"].p(), b["val"].p(), b["t_desc"].p(), None, b["t_rec"].p(),
                t_rec_bytes, b["t_max"].p(), b["t_shift"].p(), b["ws"].p(), ws_bytes, nnz, b["stg"].p(), stg_bytes,
                eng.stream)
        return lib.grf_transpose_banded_self_rec(rec_kind, *args) if rec else lib.grf_transpose_banded_self(*args)
    s.call = call

    def result():
        # the records through the row-mode Gram of them (their order inside a bucket is unspecified)
        rc = lib.grf_gram_sparse_rec(kind, n, 0, n, b["ptr"].p(), b["idx"].p(), b["val"].p(), bw, unit, b["t_desc"].p(),
                                     b["t_rec"].p(), b["t_shift"].p(), b["K"].p(), n, eng.stream)
        assert rc == OK, lib.grf_last_error()
        torch.cuda.synchronize()
        return {"t_desc": b["t_desc"].words(), "t_max": b["t_max"].words(), "t_shift": b["t_shift"].words(),
                "K": b["K"].words()}
    s.result = result
    s.bads = [dict(ws_bytes=need - 1), dict(stg_bytes=stg - 1), dict(t_rec_bytes=units * unit - unit), dict(rec_unit=7)]
    if rec:
        s.bads += [dict(rec_kind=2), dict(rec_kind=-1), dict(rec_unit=12)]
    s.check = lambda: bool(np.all(np.isfinite(b["K"].get(np.float32, n * n))))
    return s


def setup_gram_sparse_upper(eng):
    from grf_amd.engine import DeviceCSR
    n, ptr, idx, val = phi_csr()
    P = sp.csr_matrix((val.astype(np.float64), idx, ptr), shape=(n, n))
    phi = DeviceCSR.from_scipy(P, eng.device)
    phi.val32 = torch.from_numpy(val).to(eng.device)
    tr = eng.transpose_banded(phi, 64)
    assert tr.rec_kind == 0
    s = Setup()
    s.keep = (phi, tr)
    ld = n + 2
    b = dict(K=Buf(eng, 4 * n * ld))
    s.bufs = [b["K"]]

    def call(ldk=ld, rec_unit=tr.rec_unit, band_width=64, n_parts=1):
        from grf_amd.engine import _p
        return eng.lib.grf_gram_sparse_upper(n, _p(phi.ptr), _p(phi.idx), _p(phi.val32), band_width, rec_unit,
                                             _p(tr.t_desc), _p(tr.t_rec), _p(tr.t_split), _p(tr.t_rowshift), b["K"].p(),
                                             ldk, 0, 1, n_parts, None, 0, eng.stream)
    s.call = call
    s.result = lambda: {"K": b["K"].words()}
    s.bads = [dict(ldk=n - 1), dict(rec_unit=7), dict(band_width=100), dict(n_parts=0)]
    return s


def dense_operand():
    def make():
        r = np.random.default_rng(11)
        n, k, lda = 130, 40, 48
        A = np.zeros((n, lda), np.float32)
        A[:, :k] = r.uniform(-1.0, 1.0, (n, k)).astype(np.float32)
        return n, k, lda, A
    return shared("dense_A", make)


def setup_gram_dense(eng, planes):
    n, k, lda, A = dense_operand()
    lib = eng.lib
    need = lib.grf_gram_dense_split_workspace_bytes(n, k)
    ldk, ldp = 132, int(lib.grf_planes_row_bytes(k))
    s = Setup()
    b = dict(A=Buf(eng, init=A), K=Buf(eng, 4 * n * ldk), ws=Buf(eng, need + 128, zero=True), P=Buf(eng, n * ldp))
    if planes:
        assert lib.grf_split_planes(n, k, b["A"].p(), lda, b["P"].p(), ldp, eng.stream) == OK, lib.grf_last_error()
        torch.cuda.synchronize()
    s.bufs, s.named = list(b.values()), b

    def call(ld_in=None, ld_k=ldk, ws_off=0, ws_bytes=need):
        if planes:
            return lib.grf_gram_dense_planes(n, k, b["P"].p(), ldp if ld_in is None else ld_in, b["K"].p(), ld_k,
                                             b["ws"].p(ws_off), ws_bytes, eng.stream)
        return lib.grf_gram_dense_split(n, k, b["A"].p(), lda if ld_in is None else ld_in, b["K"].p(), ld_k,
                                        b["ws"].p(ws_off), ws_bytes, eng.stream)
    s.call = call
    s.result = lambda: {"K": b["K"].words()}
    s.bads = [dict(ws_bytes=need - 1), dict(ws_off=128), dict(ld_k=n - 1), dict(ld_in=(ldp - 16) if planes else 32)]

    def check():
        K = b["K"].get(np.float32, n * ldk).reshape(n, ldk)[:, :n].astype(np.float64)
        ref = A.astype(np.float64) @ A.astype(np.float64).T
        return bool(np.all(np.abs(K - ref) <= 1e-5 * (np.abs(A).astype(np.float64) @ np.abs(A).astype(np.float64).T)
                           + 1e-30))
    s.check = check
    return s


def setup_csr_transpose(eng):
    n, ptr, idx, val = phi_csr()
    nnz = len(idx)
    need = eng.lib.grf_csr_transpose_workspace_bytes(n, n, nnz)
    s = Setup()
    b = dict(ptr=Buf(eng, init=ptr), idx=Buf(eng, init=idx), val=Buf(eng, init=val), t_ptr=Buf(eng, 8 * (n + 1)),
             t_idx=Buf(eng, 4 * nnz), t_val=Buf(eng, 4 * nnz), ws=Buf(eng, need))
    s.bufs, s.named = list(b.values()), b
    s.call = lambda ws_bytes=need: eng.lib.grf_csr_transpose(n, b["ptr"].p(), b["idx"].p(), b["val"].p(), None, n, nnz,
                                                             b["t_ptr"].p(), b["t_idx"].p(), b["t_val"].p(),
                                                             b["ws"].p(), ws_bytes, eng.stream)
    s.result = lambda: {k: b[k].words() for k in ("t_ptr", "t_idx", "t_val")}
    s.bads = [dict(ws_bytes=need - 1), dict(ws_bytes=0)]

    def check():
        T = sp.csr_matrix((val, idx, ptr), shape=(n, n)).T.tocsr()
        T.sort_indices()
        return (np.array_equal(b["t_ptr"].get(np.int64, n + 1), T.indptr) and
                np.array_equal(b["t_idx"].get(np.int32, nnz), T.indices) and
                np.array_equal(bits(b["t_val"].get(np.float32, nnz)), bits(T.data.astype(np.float32))))
    s.check = check
    return s


def setup_spmm_f64(eng):
    n, ptr, idx, val = phi_csr()
    S, ld = 7, 8
    X = shared("spmm_X", lambda: np.random.default_rng(12).uniform(-1.0, 1.0, (n, ld)))
    s = Setup()
    b = dict(ptr=Buf(eng, init=ptr), idx=Buf(eng, init=idx), val=Buf(eng, init=val), X=Buf(eng, init=X),
             Y=Buf(eng, 8 * n * ld))
    s.bufs, s.named = list(b.values()), b
    s.call = lambda ldx=ld, ldy=ld: eng.lib.grf_spmm_csr_f64(n, b["ptr"].p(), b["idx"].p(), b["val"].p(), None,
                                                             b["X"].p(), ldx, S, b["Y"].p(), ldy, eng.stream)
    s.result = lambda: {"Y": b["Y"].words()}
    s.bads = [dict(ldy=S - 1), dict(ldx=S - 1)]

    def check():
        Y = b["Y"].get(np.float64, n * ld).reshape(n, ld)
        ref = sp.csr_matrix((val.astype(np.float64), idx, ptr), shape=(n, n)) @ X[:, :S]
        tail = bits(Y[:, S:])
        return bool(np.allclose(Y[:, :S], ref, rtol=1e-12, atol=1e-13)) and bool(np.all(tail == (SENT | SENT << 32)))
    s.check = check
    return s


SETUPS = {
    "grf_laplacian_csr": setup_laplacian_csr,
    "grf_laplacian_dense": setup_laplacian_dense,
    "grf_scan_counts": setup_scan_counts,
    "grf_transpose_banded_self": lambda e: setup_transpose_self(e, False),
    "grf_transpose_banded_self_rec": lambda e: setup_transpose_self(e, True),
    "grf_gram_sparse_upper": setup_gram_sparse_upper,
    "grf_gram_dense_split": lambda e: setup_gram_dense(e, False),
    "grf_gram_dense_planes": lambda e: setup_gram_dense(e, True),
    "grf_csr_transpose": setup_csr_transpose,
    "grf_spmm_csr_f64": setup_spmm_f64,
}


@pytest.mark.parametrize("entry", list(SETUPS))
def test_refused_call_writes_nothing_and_poisons_nothing(eng, entry):
    s = SETUPS[entry](eng)
    torch.cuda.synchronize()
    for bad in s.bads:
        before = [b.words() for b in s.bufs]
        rc = s.call(**bad)
        err = eng.lib.grf_last_error()
        torch.cuda.synchronize()
        assert rc in REFUSALS and err, (bad, rc, err)
        for b, w in zip(s.bufs, before):
            assert np.array_equal(b.words(), w), (bad, "a refused call wrote to a buffer")
    assert s.call() == OK, eng.lib.grf_last_error()
    torch.cuda.synchronize()
    got = s.result()
    fresh = SETUPS[entry](eng)                          # buffers prepared as for a first call
    assert fresh.call() == OK, eng.lib.grf_last_error()
    torch.cuda.synchronize()
    want = fresh.result()
    for name in want:
        assert np.array_equal(got[name], want[name]), name
    assert any(np.any(w[PAD:-PAD] != SENT) for w in got.values())       # (the valid call did write)
    if hasattr(s, "check"):
        assert s.check()


def test_refused_laplacians_then_the_oracle_bits(eng):
    """The valid Laplacian calls after the refused ones are the oracle's, on the two cap cases' inputs."""
    for setup, case in ((setup_laplacian_csr, "csr"), (setup_laplacian_dense, "dense")):
        s = setup(eng)
        assert s.call(ws_bytes=0) == EINVAL
        assert s.call() == OK
        torch.cuda.synchronize()
        if case == "csr":
            _, L = lap_csr_case()
            ip, ix, dx = L.indptr.astype(np.int64), L.indices.astype(np.int32), L.data
        else:
            _, ip, ix, dx = lap_dense_case()
        n, nnz = len(ip) - 1, len(ix)
        assert np.array_equal(s.named["l_ptr"].get(np.int64, n + 1), ip), case
        li, lv = s.named["l_idx"], s.named["l_val"]
        assert np.array_equal(li.get(np.int32, nnz), ix) and np.array_equal(bits(lv.get(np.float64, nnz)), bits(dx)), case


# ---------------------------------------------------------------------- data-dependent caps
def _cap_cases(nnz):
    return sorted({0, 1, nnz - 1, nnz})


def _assert_truncated(l_ptr, l_idx, l_val, cap_words, l_cap, ip, ix, dx):
    n, nnz = len(ip) - 1, len(ix)
    assert np.array_equal(l_ptr.get(np.int64, n + 1), ip)               # the FULL row pointer: l_ptr[n] > l_cap tells
    k = min(l_cap, nnz)
    gi, gv = l_idx.get(np.int32, cap_words), l_val.get(np.float64, cap_words)
    assert np.array_equal(gi[:k], ix[:k]) and np.array_equal(bits(gv[:k]), bits(dx[:k]))
    assert np.all(gi[k:].view(np.uint32) == SENT), "a word at or past l_cap was written"
    assert np.all(bits(gv[k:]) == (SENT | SENT << 32)), "a word at or past l_cap was written"


def test_laplacian_csr_cap_too_small(eng):
    A, L = lap_csr_case()
    ip, ix, dx = L.indptr.astype(np.int64), L.indices.astype(np.int32), L.data
    n, nnz = A.shape[0], L.nnz
    assert nnz > 2 and ip[-1] == nnz
    need = eng.lib.grf_laplacian_csr_workspace_bytes(n)
    a_ptr, a_idx, a_val = Buf(eng, init=A.indptr.astype(np.int64)), Buf(eng, init=A.indices.astype(np.int32)), Buf(eng, init=A.data)
    full = A.nnz + n                                                     # the buffers hold the documented capacity
    for l_cap in _cap_cases(nnz):
        l_ptr, l_idx, l_val = Buf(eng, 8 * (n + 1)), Buf(eng, 4 * full), Buf(eng, 8 * full)
        deg, dinv, ws = Buf(eng, 8 * n), Buf(eng, 8 * n), Buf(eng, need)
        rc = eng.lib.grf_laplacian_csr(n, a_ptr.p(), a_idx.p(), a_val.p(), 0, l_ptr.p(), l_idx.p(), l_val.p(), l_cap,
                                       deg.p(), dinv.p(), ws.p(), need, eng.stream)
        torch.cuda.synchronize()
        assert rc == OK, (l_cap, eng.lib.grf_last_error())
        _assert_truncated(l_ptr, l_idx, l_val, full, l_cap, ip, ix, dx)


def test_laplacian_dense_cap_too_small(eng):
    W, ip, ix, dx = lap_dense_case()
    n, nnz = W.shape[0], len(ix)
    assert nnz > 2 and ip[-1] == nnz
    need = eng.lib.grf_laplacian_dense_workspace_bytes(n)
    Wb = Buf(eng, init=W)
    full = nnz + 8
    for l_cap in _cap_cases(nnz):
        l_ptr, l_idx, l_val = Buf(eng, 8 * (n + 1)), Buf(eng, 4 * full), Buf(eng, 8 * full)
        deg, ws = Buf(eng, 8 * n), Buf(eng, need)
        rc = eng.lib.grf_laplacian_dense(n, Wb.p(), 2, l_ptr.p(), l_idx.p(), l_val.p(), l_cap, deg.p(), ws.p(), need,
                                         eng.stream)
        torch.cuda.synchronize()
        assert rc == OK, (l_cap, eng.lib.grf_last_error())
        _assert_truncated(l_ptr, l_idx, l_val, full, l_cap, ip, ix, dx)


# ---------------------------------------------------------------------- empty calls
def _empty_cases(eng):
    """name -> (call(B) -> status, {buffer index: bytes the header says are written (all zero)}); B(i): the i-th of
    a pool of small sentinel buffers (pointer arguments that an empty call must not touch)."""
    from grf_amd import _lib
    lib = eng.lib
    st = eng.stream
    WPm = _lib.GrfWalkParams(8, 0.1, 4, 0, 1, 0, 1, 42)
    wp = ctypes.pointer(WPm)
    steps = [Buf(eng, 4096) for _ in range(3)]      # (three step matrices' device pointers in a host array)
    hp = (ctypes.c_void_p * 3)(*[b.p().value for b in steps])
    tr_need = lib.grf_csr_transpose_workspace_bytes(0, 5, 0)
    tr_ws = Buf(eng, tr_need)

    _empty_cases.kept = steps + [tr_ws]

    def cases(B):
        return {
            "grf_laplacian_csr": (lambda: lib.grf_laplacian_csr(0, B(0), B(1), B(2), 0, B(3), B(4), B(5), 0, B(6), B(7),
                                                                B(8), 4096, st), {3: 8}),
            "grf_laplacian_dense": (lambda: lib.grf_laplacian_dense(0, B(0), 1, B(3), B(4), B(5), 0, B(6), B(8), 4096,
                                                                    st), {3: 8}),
            "grf_walk": (lambda: lib.grf_walk(0, B(0), B(1), B(2), wp, 0, 0, B(3), B(4), st), {}),
            "grf_walk_ex": (lambda: lib.grf_walk_ex(0, B(0), B(1), B(2), B(5), wp, 0, 0, B(3), B(4), st), {}),
            "grf_walk(no sources)": (lambda: lib.grf_walk(300, B(0), B(1), B(2), wp, 7, 7, B(3), B(4), st), {}),
            "grf_walk_phi": (lambda: lib.grf_walk_phi(0, B(0), B(1), B(2), None, wp, 0, 0, 0, B(3), 4, 32, B(4), B(5),
                                                      B(6), None, None, 64, 0, st), {}),
            "grf_walk_aug": (lambda: lib.grf_walk_aug(0, B(0), B(1), B(2), B(3), st), {}),
            "grf_steps": (lambda: lib.grf_steps(0, 8, 4, 0, B(0), B(1), B(2), B(3), B(4), st), {}),
            "grf_steps_densify": (lambda: lib.grf_steps_densify(0, 8, 4, 50, B(0), B(1), B(2), B(3), st), {}),
            "grf_phi": (lambda: lib.grf_phi(0, 8, 4, B(0), B(1), B(2), B(3), 4, 32, B(4), B(5), B(6), B(7), st), {}),
            "grf_phi(n_f = 0)": (lambda: lib.grf_phi(0, 8, 4, B(0), B(1), B(2), None, 0, 32, B(4), B(5), B(6), None, st), {}),
            "grf_phi_fused": (lambda: lib.grf_phi_fused(0, 8, 4, 0, B(0), B(1), B(3), 4, 32, B(4), B(5), B(6), B(7), st), {}),
            "grf_scan_counts": (lambda: lib.grf_scan_counts(0, B(0), B(1), B(2), 4096, st), {1: 8}),
            "grf_compact_rows": (lambda: lib.grf_compact_rows(0, 16, B(0), B(1), B(2), B(3), B(4), B(5), B(6), B(7), st), {}),
            "grf_compact_rows_stats": (lambda: lib.grf_compact_rows_stats(0, 16, B(0), B(1), B(2), B(3), B(4), B(5), B(6),
                                                                          B(7), B(8), 4096, st), {}),
            "grf_concat_segments": (lambda: lib.grf_concat_segments(0, 100, B(0), B(1), B(2), B(3), st), {}),
            "grf_concat_segments(stride = 0)": (lambda: lib.grf_concat_segments(3, 0, B(0), B(1), B(2), B(3), st), {}),
            "grf_transpose_banded_plan": (lambda: lib.grf_transpose_banded_plan(0, 5, 64, 128, B(0), B(1), B(2), 0, B(8),
                                                                                4096, st), {2: 8}),
            "grf_transpose_banded_fill": (lambda: lib.grf_transpose_banded_fill(0, 5, 64, 128, B(0), B(1), B(2), B(3),
                                                                                B(4), 4096, B(5), B(6), B(8), 4096, st),
                                          {5: 4}),
            "grf_transpose_banded_self": (lambda: lib.grf_transpose_banded_self(0, 5, 64, 128, B(0), B(1), B(2), B(3),
                                                                                None, B(4), 4096, B(5), B(6), B(8), 4096,
                                                                                0, B(9), 4096, st), {3: 8, 5: 4}),
            "grf_transpose_banded_self_rec": (lambda: lib.grf_transpose_banded_self_rec(1, 0, 5, 64, 128, B(0), B(1), B(2),
                                                                                        B(3), None, B(4), 4096, B(5), B(6),
                                                                                        B(8), 4096, 0, B(9), 4096, st),
                                              {3: 8, 5: 4}),
            "grf_gram_sparse": (lambda: lib.grf_gram_sparse(0, 0, 0, B(0), B(1), B(2), 64, 128, B(3), B(4), B(5), B(6), 0,
                                                            None, 0, st), {}),
            "grf_gram_sparse(no rows)": (lambda: lib.grf_gram_sparse(300, 9, 9, B(0), B(1), B(2), 64, 128, B(3), B(4),
                                                                     B(5), B(6), 300, None, 0, st), {}),
            "grf_gram_sparse_rec": (lambda: lib.grf_gram_sparse_rec(1, 0, 0, 0, B(0), B(1), B(2), 64, 128, B(3), B(4), B(5),
                                                                    B(6), 0, st), {}),
            "grf_gram_sparse_kslice": (lambda: lib.grf_gram_sparse_kslice(0, 0, 0, 0, 0, B(0), B(1), B(2), 64, 128, B(3),
                                                                          B(4), B(5), B(6), 0, None, 0, st), {}),
            "grf_gram_sparse_sym": (lambda: lib.grf_gram_sparse_sym(0, B(0), B(1), B(2), 64, 128, B(3), B(4), None, B(5),
                                                                    B(6), 0, None, 0, st), {}),
            "grf_gram_sparse_upper": (lambda: lib.grf_gram_sparse_upper(0, B(0), B(1), B(2), 64, 128, B(3), B(4), None,
                                                                        B(5), B(6), 0, 0, 1, 1, None, 0, st), {}),
            "grf_gram_sparse_upper(no parts)": (lambda: lib.grf_gram_sparse_upper(300, B(0), B(1), B(2), 64, 128, B(3),
                                                                                  B(4), None, B(5), B(6), 300, 2, 2, 3,
                                                                                  None, 0, st), {}),
            "grf_gram_sparse_upper_add": (lambda: lib.grf_gram_sparse_upper_add(0, B(0), B(1), B(2), 64, 128, B(3), B(4),
                                                                                None, B(5), B(6), 0, 0, 1, 1, None, 0, st),
                                          {}),
            "grf_gram_sparse_upper_ex": (lambda: lib.grf_gram_sparse_upper_ex(0, B(0), B(1), B(2), 64, 128, B(3), B(4),
                                                                              None, B(5), B(7), B(6), 0, 0, 1, 1, 0, st), {}),
            "grf_gram_sparse_upper_rec": (lambda: lib.grf_gram_sparse_upper_rec(1, 0, B(0), B(1), B(2), 64, 128, B(3), B(4),
                                                                                None, B(5), None, B(6), 0, 0, 1, 1, 0, st),
                                          {}),
            "grf_gram_sparse_cols(no rows)": (lambda: lib.grf_gram_sparse_cols(300, 9, 9, B(0), B(1), B(2), B(5), 80, -1,
                                                                               64, 128, B(3), B(4), None, B(6), 80, None,
                                                                               0, st), {}),
            "grf_gram_sparse_cols(t_rows = 0)": (lambda: lib.grf_gram_sparse_cols(300, 0, 100, B(0), B(1), B(2), B(5), 0,
                                                                                  -1, 64, 128, B(3), B(4), None, B(6), 0,
                                                                                  None, 0, st), {}),
            "grf_gram_sparse_cols_padded(no rows)": (lambda: lib.grf_gram_sparse_cols_padded(300, 9, 9, 16, B(0), B(1),
                                                                                             B(2), B(5), 80, 64, B(3), B(4),
                                                                                             B(6), 80, st), {}),
            "grf_gram_row_cuts": (lambda: lib.grf_gram_row_cuts(0, B(0), B(1), 2, 300, B(3), B(4), B(5), st), {}),
            "grf_hub_panel": (lambda: lib.grf_hub_panel(0, B(0), B(1), B(2), B(3), B(4), 16, st), {}),
            "grf_transpose_drop_columns(n_drop = 0)": (lambda: lib.grf_transpose_drop_columns(4, 300, B(3), B(4), 0, st), {}),
            "grf_transpose_drop_columns(no bands)": (lambda: lib.grf_transpose_drop_columns(0, 300, B(3), B(4), 5, st), {}),
            "grf_gram_mirror": (lambda: lib.grf_gram_mirror(0, B(6), 0, 0, st), {}),
            "grf_phi_row_shifts": (lambda: lib.grf_phi_row_shifts(0, B(0), B(1), B(2), B(3), B(8), 4096, st), {2: 4}),
            "grf_phi_row_shifts_padded": (lambda: lib.grf_phi_row_shifts_padded(0, 16, B(0), B(1), B(2), B(3), B(8), 4096,
                                                                                st), {2: 4}),
            "grf_phi_row_shifts_stats": (lambda: lib.grf_phi_row_shifts_stats(0, B(0), B(2), B(3), st), {2: 4}),
            "grf_gram_dense": (lambda: lib.grf_gram_dense(0, 64, B(0), 64, B(6), 0, st), {}),
            "grf_gram_dense(k_dim = 0)": (lambda: lib.grf_gram_dense(0, 0, B(0), 0, B(6), 0, st), {}),
            "grf_gram_dense_upper": (lambda: lib.grf_gram_dense_upper(0, 64, B(0), 64, B(6), 0, st), {}),
            "grf_gram_dense_ws": (lambda: lib.grf_gram_dense_ws(0, 64, B(0), 64, B(6), 0, B(8), 4096, st), {}),
            "grf_split_planes": (lambda: lib.grf_split_planes(0, 64, B(0), 64, B(1), 384, st), {}),
            "grf_split_planes(k_dim = 0)": (lambda: lib.grf_split_planes(100, 0, B(0), 0, B(1), 0, st), {}),
            "grf_densify": (lambda: lib.grf_densify(0, B(0), B(1), B(2), B(3), 300, st), {}),
            "grf_densify_padded": (lambda: lib.grf_densify_padded(0, 16, 300, B(0), B(1), B(2), B(3), 300, st), {}),
            "grf_densify_padded_planes": (lambda: lib.grf_densify_padded_planes(0, 16, 60, B(0), B(1), B(2), B(3), 384, st),
                                          {}),
            "grf_dense_steps_phi": (lambda: lib.grf_dense_steps_phi(0, 4, B(0), B(1), B(2), B(3), 0, st), {}),
            "grf_dense_steps_grad": (lambda: lib.grf_dense_steps_grad(0, 4, B(0), B(1), B(2), 0, B(3), B(8), 4096, st),
                                     {3: 32}),
            "grf_csr_transpose": (lambda: lib.grf_csr_transpose(0, B(0), B(1), B(2), None, 5, 0, B(3), B(4), B(5), tr_ws.p(),
                                                                tr_need, st), {3: 48}),
            "grf_spmm_csr": (lambda: lib.grf_spmm_csr(0, B(0), B(1), B(2), None, B(3), 8, 8, B(4), 8, st), {}),
            "grf_spmm_csr(n_rhs = 0)": (lambda: lib.grf_spmm_csr(100, B(0), B(1), B(2), None, B(3), 0, 0, B(4), 0, st), {}),
            "grf_spmm_csr_f64": (lambda: lib.grf_spmm_csr_f64(0, B(0), B(1), B(2), None, B(3), 8, 8, B(4), 8, st), {}),
            "grf_spmm_csr_f64(n_rhs = 0)": (lambda: lib.grf_spmm_csr_f64(100, B(0), B(1), B(2), None, B(3), 0, 0, B(4), 0,
                                                                         st), {}),
            "grf_phi_steps_csr_count": (lambda: lib.grf_phi_steps_csr_count(0, 3, hp, hp, hp, B(0), 3, B(1), st), {}),
            "grf_phi_steps_csr_fill": (lambda: lib.grf_phi_steps_csr_fill(0, 3, hp, hp, hp, B(0), 3, B(1), B(2), B(3), None,
                                                                          st), {}),
            "grf_csr_row_lengths": (lambda: lib.grf_csr_row_lengths(0, B(0), None, B(1), st), {}),
            "grf_csr_gather_rows": (lambda: lib.grf_csr_gather_rows(0, B(0), B(1), B(2), B(3), B(4), B(5), B(6), st), {}),
            "grf_csr_rowdot": (lambda: lib.grf_csr_rowdot(0, B(0), B(1), B(2), None, B(3), B(4), B(5), None, B(6), st), {}),
            "grf_csr_rows_dot_cols": (lambda: lib.grf_csr_rows_dot_cols(0, B(0), B(1), B(2), None, B(3), 0, B(4), st), {}),
            "grf_dense_to_csr_count": (lambda: lib.grf_dense_to_csr_count(0, 300, B(0), 300, B(1), st), {}),
            "grf_dense_to_csr_fill": (lambda: lib.grf_dense_to_csr_fill(0, 300, B(0), 300, B(1), B(2), B(3), st), {}),
        }
    return cases


def test_empty_calls(eng):
    """Every family at n = 0 (and the other empty sizes it allows): GRF_OK, and only the words the header names
    change -- to zero.  The pool buffers are 4 KiB between sentinels; the workspace (index 8) and the staging
    buffer (9) are scratch and may be written inside their 4 KiB."""
    pool = {}

    def B(i):
        if i not in pool:
            pool[i] = Buf(eng, 4096)
        return pool[i].p()

    cases = _empty_cases(eng)(B)
    scratch = (8, 9)
    for name, (call, written) in cases.items():
        pool.clear()
        rc = call()
        torch.cuda.synchronize()
        assert rc == OK, (name, rc, eng.lib.grf_last_error())
        for i, buf in pool.items():
            if i in scratch:
                buf.get(np.uint8, 1)                                    # (the sentinels around it)
                continue
            k = written.get(i, 0)
            assert rest_is_sentinel(buf, k), (name, i, "written beyond what the header says")
            assert np.all(buf.get(np.uint8, max(k, 1))[:k] == 0), (name, i)
    assert all(rest_is_sentinel(b, 0) for b in _empty_cases.kept[:3]) and _empty_cases.kept[3].get(np.uint8, 1) is not None
