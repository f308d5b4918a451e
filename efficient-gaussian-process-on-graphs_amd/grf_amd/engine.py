"""Device-resident GRF pipeline on one MI355X: thin Python over the C ABI.

Every stage is one call into ``libgrf_amd.so`` on the current torch stream of
the engine's device; buffers are torch tensors (device memory plumbing only).
Nothing here computes on the host: the only host reads are sizes
(``DeviceCSR.nnz``) needed to allocate an output exactly.

Pipeline (re-designed for gfx950)::

    A (CSR) --laplacian--> L (CSR) --walk--> visit slots [n][L][m]
      --steps--> per-step rows (sampler API)   --phi--> Phi rows
      --phi_fused (m*L <= 4096)-----------------------> Phi rows
      --compact--> Phi CSR --transpose_banded--> Phi^T buckets --gram_sparse--> K (fp32)
                           --densify--> dense Phi --gram_dense (MFMA)-----------> K (fp32)
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np
import scipy.sparse as sp
import torch

from . import _lib as C

DEFAULT_BAND_WIDTH = 4096  # transpose band = one Gram tile (32 KB int64 LDS accumulator per workgroup)
# row-mode Grams (row blocks: multi-GPU, K row ranges) are 6 % faster on 8192-wide bands with 8-wave
# tiles (C4: 25.9 vs 27.5 ms); the symmetric whole-K mode stays at 4096 (21.9 vs 22.7 ms: with 13
# bands the diagonal band tiles' lower halves cost more than the wider buckets save)
ROWS_BAND_WIDTH = 8192
# hub-column split: columns in at least this share of Phi's rows go to the dense MFMA panel (hub_count)
HUB_SHARE = 0.13
# ... and once a graph has such columns, with the split panel (bf16 products: 3/8 of the fp32 MFMA's cost per
# multiply-add) the columns down to this share as well: Enron 96 -> 192 columns, 7.52 -> 7.38 ms per K; 128 /
# 256 columns 7.47 / 7.50 (profiles/r05_hub_sweep_split.txt); Facebook's 20 columns above 0.13 stay unsplit
HUB_EXTEND_SHARE = 0.105
# gram(method="auto"): the dense MFMA path up to this many rows, the sparse path above
DENSE_GRAM_MAX_N = 4500  # measured crossover, profiles/r03_gram_crossover.txt (split Gram: r05_gram_crossover.txt)
# the banded transpose counts its buckets itself (grf_transpose_banded_self: no count atomics in the
# walk, no scan over every bucket); GRF_TRANSPOSE_SELF=0 restores the walk-counted plan (A/B)
SELF_COUNT_TRANSPOSE = os.environ.get("GRF_TRANSPOSE_SELF", "1") != "0"
# the whole-K Gram's waves take shares of about equal record pairs (grf_gram_row_cuts) instead of equal
# nonzero counts: "auto" (default) when Phi's column counts are skewed (column_stats), "1" always, "0" never
ROW_CUTS = os.environ.get("GRF_GRAM_CUTS", "auto")
# skewed: the densest column of Phi holds at least this many times the mean column's entries (C4's
# Erdos-Renyi Phi: ~1.2; Facebook / Enron: > 20)
SKEW_RATIO = 4.0
# the C solves by (family, float64, Lanczos coefficients, preconditioned) and their workspace sizes by
# (family, preconditioned); "gram": Phi as a CSR, "poly": the walk operator
CG_ENTRIES = {
    ("gram", False, False, False): "grf_cg_gram_solve",
    ("gram", True, False, False): "grf_cg_gram_solve_f64", ("gram", True, False, True): "grf_pcg_gram_solve_f64",
    ("gram", True, True, False): "grf_cg_gram_solve_lanczos_f64",
    ("gram", True, True, True): "grf_pcg_gram_solve_lanczos_f64",
    ("poly", True, False, False): "grf_cg_poly_solve_f64", ("poly", True, False, True): "grf_pcg_poly_solve_f64",
    ("poly", True, True, False): "grf_cg_poly_solve_lanczos_f64",
    ("poly", True, True, True): "grf_pcg_poly_solve_lanczos_f64",
}
CG_WORKSPACES = {("gram", False): "grf_cg_workspace_bytes", ("gram", True): "grf_pcg_workspace_bytes",
                 ("poly", False): "grf_cg_poly_workspace_bytes", ("poly", True): "grf_pcg_poly_workspace_bytes"}


def _p(t: Optional[torch.Tensor]):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def preconditioner_name(preconditioner, what: str) -> bool:
    """True for "jacobi", False for None; anything else is refused (``what``: the caller, for the message)."""
    if preconditioner is None:
        return False
    if isinstance(preconditioner, str) and preconditioner == "jacobi":
        return True
    raise ValueError(f"{what}: preconditioner must be None or \"jacobi\", not {preconditioner!r}")


@dataclass
class DeviceCSR:
    """CSR matrix in device memory (int64 row pointers, int32 columns)."""

    n_rows: int
    n_cols: int
    ptr: torch.Tensor
    idx: torch.Tensor
    val: Optional[torch.Tensor] = None    # float64
    val32: Optional[torch.Tensor] = None  # float32
    _nnz: Optional[int] = None
    nnz_bound: Optional[int] = None  # an upper bound of nnz known without a host read (buffers sized by it)
    row_bound: Optional[int] = None  # an upper bound of the entries of any one row

    @property
    def nnz(self) -> int:
        if self._nnz is None:
            self._nnz = int(self.ptr[-1].item())
        return self._nnz

    # a row selection's entry buffers are sized by rows x row_bound only while that stays within this factor
    # of the matrix's own entries (repeats allowed) or ROWS_BOUND_FLOOR entries; past it (a hub row makes
    # row_bound ~ n_cols) the exact count is read back instead
    ROWS_BOUND_FACTOR = 4
    ROWS_BOUND_FLOOR = 1 << 22

    def rows_entry_bound(self, n_sel: int) -> Optional[int]:
        """An upper bound of the entries of n_sel selected rows that is known without a host read and
        not wasteful (None: count them exactly)."""
        if self.row_bound is None:
            return None
        bound = n_sel * self.row_bound
        total = self.nnz_or_bound() if (self._nnz is not None or self.nnz_bound is not None) else None
        if total is None:
            return None
        reps = -(-max(n_sel, 1) // max(self.n_rows, 1))  # (a selection longer than the matrix repeats rows)
        return bound if bound <= max(self.ROWS_BOUND_FACTOR * reps * total, self.ROWS_BOUND_FLOOR) else None

    def nnz_or_bound(self) -> int:
        """nnz when it is known on the host, else the bound (no device->host read), else nnz (read)."""
        if self._nnz is not None:
            return self._nnz
        return self.nnz_bound if self.nnz_bound is not None else self.nnz

    @classmethod
    def from_scipy(cls, A, device) -> "DeviceCSR":
        A = sp.csr_matrix(A)
        if A.shape[0] > 0x7FFFFFFF or A.shape[1] > 0x7FFFFFFF:
            raise ValueError("graphs with more than 2^31-1 nodes are not supported")
        ptr = torch.from_numpy(np.asarray(A.indptr, dtype=np.int64)).to(device)
        idx = torch.from_numpy(np.asarray(A.indices, dtype=np.int32)).to(device)
        val = torch.from_numpy(np.asarray(A.data, dtype=np.float64)).to(device)
        return cls(A.shape[0], A.shape[1], ptr, idx, val, None, int(A.nnz))

    def to_scipy(self) -> sp.csr_matrix:
        nnz = self.nnz
        ptr = self.ptr.cpu().numpy()
        idx = self.idx[:nnz].cpu().numpy()
        val = (self.val if self.val is not None else self.val32)[:nnz].cpu().numpy()
        if ptr[-1] <= np.iinfo(np.int32).max:
            ptr = ptr.astype(np.int32)
        return sp.csr_matrix((val, idx, ptr), shape=(self.n_rows, self.n_cols))


@dataclass
class Slots:
    node: torch.Tensor  # int32 [n_src, L, m], -1 = no visit
    load: torch.Tensor  # float64 [n_src, L, m]
    src_begin: int
    n: int              # nodes of the graph (columns)

    @property
    def n_src(self):
        return self.node.shape[0]

    @property
    def L(self):
        return self.node.shape[1]

    @property
    def m(self):
        return self.node.shape[2]


@dataclass
class StepRows:
    cnt: torch.Tensor  # int32 [n_src * L]
    idx: torch.Tensor  # int32 [n_src * L * m]
    val: torch.Tensor  # float64 [n_src * L * m]
    n_src: int
    L: int
    m: int
    n: int


@dataclass
class PaddedRows:
    cnt: torch.Tensor             # int32 [n_rows]
    idx: torch.Tensor             # int32 [n_rows * cap]
    val: torch.Tensor             # float64 [n_rows * cap]
    val32: Optional[torch.Tensor]  # float32 [n_rows * cap]
    cap: int
    n_cols: int

    @property
    def n_rows(self):
        return self.cnt.shape[0]


@dataclass
class Banded:
    t_desc: torch.Tensor  # int32 [2 * (n_bands * n_cols + 1)]: per bucket {first unit, pairs}
    t_rec: torch.Tensor   # uint8 [units * rec_unit]: 12-byte record pairs {u16 j0 | u16 j1, f32 v0, f32 v1}
    t_maxabs: torch.Tensor  # float32 [1], max |Phi|
    t_rowshift: torch.Tensor  # int32 [n_rows], Gram fixed-point scale exponent per row
    band_width: int
    n_rows: int
    n_cols: int
    rec_unit: int = C.REC_LINE  # bucket alignment: 128-byte lines or packed 12-byte pairs
    # per bucket 8 uint16 entry offsets of its sub-bands (buckets laid out by sub-band; the symmetric
    # Gram's diagonal tiles start there), or None (records in arbitrary order within a bucket)
    t_split: Optional[torch.Tensor] = None
    # C.REC_PAIRS, or C.REC_TRIPLES: line buckets of 16-byte triples {u32 c0 | o1 << 12 | o2 << 22, 3 x f32}
    # (include/grf.h grf_rec_kind; t_desc then holds {first line, triples}); the whole-K and row Gram read both
    rec_kind: int = C.REC_PAIRS


def cols_band_width(rows: int, max_width: int = ROWS_BAND_WIDTH) -> int:
    """Band width of a rank's own-rows transpose (column-block Gram): the rows in the fewest bands
    of at most ``max_width``, split evenly and rounded up to a multiple of 64."""
    nb = max(1, -(-rows // max_width))
    return max(64, -(-(-(-rows // nb)) // 64) * 64)


def choose_rec_unit(nnz: int, n_rows: int, n_cols: int, band_width: int) -> int:
    """Line-aligned buckets when a bucket averages >= 8 entries (C4: ~18 at W = 4096), packed
    pairs below that (C5: ~1.4 at W = 8192, where a 128-byte line per bucket would be ~15x
    the records' bytes)."""
    per_bucket = nnz / max(1, n_rows) * band_width / max(1, n_cols)
    return C.REC_LINE if per_bucket >= 8.0 else C.REC_PACKED


def _phi_rec_unit(phi, nnz_bound, band_width: int) -> int:
    """choose_rec_unit for a Phi whose nnz may not be on the host yet: its known nnz, else the caller's bound."""
    nnz = phi.nnz if phi._nnz is not None or nnz_bound is None else nnz_bound
    return choose_rec_unit(nnz, phi.n_rows, phi.n_cols, band_width)


class DensePlanes:
    """The dense Phi as the split Gram's three bf16 planes (include/grf.h grf_split_planes): ``P`` uint8
    [n x row bytes] on the device, ``n`` rows, ``k_dim`` columns."""

    def __init__(self, P: torch.Tensor, n: int, k_dim: int):
        self.P, self.n, self.k_dim = P, int(n), int(k_dim)

    @property
    def shape(self):
        return (self.n, self.k_dim)

    def record_stream(self, stream):
        self.P.record_stream(stream)


class WalkPolynomial:
    """The exact walk-power kernel's feature matrix Phi = p(G) = sum_l f_l G^l as a matrix-free operator: the
    walk matrix ``G`` (a DeviceCSR with fp64 values, as ``GRFEngine.laplacian`` returns it, or a scipy matrix)
    and its transpose, built once here with torch (a stable sort by column).  Nothing is assumed symmetric; for
    a symmetric G the transpose aliases G.  A modulator f enters with its first ``min(len(f), L)`` entries, as
    in ``StepMatrices.phi``.  ``GRFEngine.poly_apply`` / ``poly_gram_matvec`` / ``cg_solve_poly`` /
    ``marginal_log_likelihood`` / ``pathwise_predict`` run on it; the powers of G are never formed."""

    def __init__(self, G, max_walk_length: int, engine: Optional["GRFEngine"] = None):
        if int(max_walk_length) < 1:
            raise ValueError("WalkPolynomial: max_walk_length must be at least 1")
        self.engine = engine or get_engine(G.ptr.device if isinstance(G, DeviceCSR) else None)
        G = self.engine.to_device(G)
        if G.n_rows != G.n_cols:
            raise ValueError("WalkPolynomial: the walk matrix must be square")
        if G.val is None:
            raise ValueError("WalkPolynomial: the walk matrix needs float64 values")
        self.G = G
        self.L = int(max_walk_length)
        self.shape = (G.n_rows, G.n_cols)
        n, nnz = G.n_rows, G.nnz
        cols = G.idx[:nnz].long()
        rows = torch.repeat_interleave(torch.arange(n, device=G.ptr.device), G.ptr[1:] - G.ptr[:-1])
        order = torch.sort(cols, stable=True)[1]  # (every column lists its rows in ascending order)
        t_ptr = torch.zeros(n + 1, dtype=torch.int64, device=G.ptr.device)
        t_ptr[1:] = torch.cumsum(torch.bincount(cols, minlength=n), 0)
        t_idx = rows[order].to(torch.int32)
        t_val = G.val[:nnz][order].contiguous()
        if bool(torch.equal(t_ptr, G.ptr)) and bool(torch.equal(t_idx, G.idx[:nnz])) and \
                bool(torch.equal(t_val, G.val[:nnz])):
            self.Gt = G
        else:
            self.Gt = DeviceCSR(n, n, t_ptr, t_idx, t_val, None, nnz)

    def n_terms(self, f) -> int:
        return min(int(f.numel()), self.L)


class GRFEngine:
    """All device work for one GPU.  ``device`` is a torch device (``cuda:N``)."""

    def __init__(self, device=None):
        if not torch.cuda.is_available():
            raise RuntimeError("grf_amd needs a ROCm GPU (MI355X / gfx950); none is visible")
        self.lib = C.load()
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        C.check(self.lib.grf_set_device(self.device.index), "grf_set_device")
        # the Gram kernels' tile work counter (calls on this engine's stream are ordered)
        self._gram_ws = self._ws(self.lib.grf_gram_workspace_bytes())
        # the dense Gram's arithmetic (gram_dense): the exact three-plane bf16 'split' on the bf16 matrix
        # cores (fp32-class error, 1.3-1.4x faster: profiles/r05_split_gram_error.txt, AB_LOG "split Gram") or
        # the 'fp32' matrix instruction
        self.dense_precision = os.environ.get("GRF_GRAM_DENSE_PRECISION", "split")
        if self.dense_precision not in ("split", "fp32"):
            raise ValueError(f"GRF_GRAM_DENSE_PRECISION must be 'split' or 'fp32', got {self.dense_precision!r}")

    # ------------------------------------------------------------ utilities
    @property
    def stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _empty(self, n, dtype):
        return torch.empty(int(max(n, 0)), dtype=dtype, device=self.device)

    def _ws(self, nbytes: int) -> torch.Tensor:
        return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=self.device)

    def _set_device(self):
        C.check(self.lib.grf_set_device(self.device.index), "grf_set_device")

    def to_device(self, A) -> DeviceCSR:
        return A if isinstance(A, DeviceCSR) else DeviceCSR.from_scipy(A, self.device)

    # ----------------------------------------------------------- Laplacians
    def laplacian(self, A) -> DeviceCSR:
        """scipy-semantics normalised Laplacian (utils_sparse/graph_utils.py:5-30)."""
        A = self.to_device(A)
        if A.n_rows != A.n_cols:
            raise ValueError("Adjacency matrix must be square.")
        n = A.n_rows
        cap = A.nnz + n
        lp, li, lv = self._empty(n + 1, torch.int64), self._empty(cap, torch.int32), self._empty(cap, torch.float64)
        deg, dinv = self._empty(n, torch.float64), self._empty(n, torch.float64)
        ws = self._ws(self.lib.grf_laplacian_csr_workspace_bytes(n))
        C.check(self.lib.grf_laplacian_csr(n, _p(A.ptr), _p(A.idx), _p(A.val), C.LAP_SCIPY, _p(lp), _p(li), _p(lv),
                                           cap, _p(deg), _p(dinv), _p(ws), ws.numel(), self.stream),
                "grf_laplacian_csr")
        G = DeviceCSR(n, n, lp, li, lv)
        G.nnz_bound = cap  # (sizes the augmented walk matrix without reading nnz back)
        return G

    def walk_matrix_dense(self, W, mode: int, nnz_w: Optional[int] = None) -> DeviceCSR:
        """Dense-input walk matrix (numpy Laplacian variants or the matrix itself) as CSR.

        Its capacity (and the augmented walk matrix sized from it, cached on the result) is nnz(W) + n
        (the Laplacian adds at most the diagonal).  nnz(W) is counted on the host for a host W, taken
        from ``nnz_w`` when the caller knows it (the bench counts its resident W once, at setup), else
        bounded by n^2 while that is small (<= 2^26 entries: 0.8 GB of CSR) or counted on the device
        (a torch reduction and a host round trip: 0.64 ms of C2's front, profiles/r05_c2_kernel_alone.txt)."""
        host = not torch.is_tensor(W)
        Wn = np.ascontiguousarray(W, dtype=np.float64) if host else None
        Wt = torch.as_tensor(Wn) if host else W
        Wt = Wt.to(self.device, torch.float64).contiguous()
        n = Wt.shape[0]
        if Wt.dim() != 2 or Wt.shape[1] != n:
            raise ValueError("Adjacency matrix must be square.")
        if nnz_w is not None:
            cap = min(int(nnz_w) + n, n * n)
        elif host:
            cap = int(np.count_nonzero(Wn)) + n
        elif n * n <= (1 << 26):
            cap = n * n
        else:
            cap = int(torch.count_nonzero(Wt).item()) + n
        cap = max(cap, 1)
        lp, li, lv = self._empty(n + 1, torch.int64), self._empty(cap, torch.int32), self._empty(cap, torch.float64)
        deg = self._empty(n, torch.float64)
        ws = self._ws(self.lib.grf_laplacian_dense_workspace_bytes(n))
        C.check(self.lib.grf_laplacian_dense(n, _p(Wt), mode, _p(lp), _p(li), _p(lv), cap, _p(deg), _p(ws),
                                             ws.numel(), self.stream), "grf_laplacian_dense")
        G = DeviceCSR(n, n, lp, li, lv)
        G.nnz_bound = cap
        return G

    # ---------------------------------------------------------------- walks
    def walk(self, G: DeviceCSR, walks_per_node: int, p_halt: float, max_walk_length: int, *, rng: int = C.RNG_PHILOX,
             seed: int = 42, n_chunks: int = 1, load_rule: int = C.LOAD_CUMULATIVE, src_begin: int = 0,
             src_end: Optional[int] = None, use_aug: bool = True) -> Slots:
        """Visit slots of the walks from sources [src_begin, src_end).  use_aug: step through the
        augmented walk matrix (one dependent round trip per step; the same slots bit for bit)."""
        n = G.n_rows
        src_end = n if src_end is None else src_end
        m, L = int(walks_per_node), int(max_walk_length)
        if m < 1 or L < 1:
            raise ValueError("walks_per_node and max_walk_length must be >= 1")
        ns = src_end - src_begin
        node = torch.empty((ns, L, m), dtype=torch.int32, device=self.device)
        load = torch.empty((ns, L, m), dtype=torch.float64, device=self.device)
        prm = C.GrfWalkParams(m, float(p_halt), L, int(load_rule), int(rng), 0, int(n_chunks),
                              int(seed) & 0xFFFFFFFFFFFFFFFF)
        aug = self.walk_aug(G) if use_aug else None
        C.check(self.lib.grf_walk_ex(n, _p(G.ptr), _p(G.idx), _p(G.val), _p(aug), ctypes.byref(prm), src_begin,
                                     src_end, _p(node), _p(load), self.stream), "grf_walk_ex")
        return Slots(node, load, src_begin, n)

    def chunk_bounds(self, n: int, n_chunks: int) -> list[int]:
        return [int(self.lib.grf_chunk_bounds(n, n_chunks, c)) for c in range(n_chunks)] + [n]

    # ----------------------------------------------------- steps / features
    def steps(self, slots: Slots, norm: int = C.NORM_MUL_RECIP) -> StepRows:
        ns, L, m = slots.n_src, slots.L, slots.m
        cnt = self._empty(ns * L, torch.int32)
        idx = self._empty(ns * L * m, torch.int32)
        val = self._empty(ns * L * m, torch.float64)
        C.check(self.lib.grf_steps(ns, m, L, norm, _p(slots.node), _p(slots.load), _p(cnt), _p(idx), _p(val),
                                   self.stream), "grf_steps")
        return StepRows(cnt, idx, val, ns, L, m, slots.n)

    def _f(self, f) -> torch.Tensor:
        """The modulator on the device.  Host values are uploaded once per distinct vector (a pageable
        host-to-device copy per call stalled the issuing thread ~0.2 ms inside every pipelined step)."""
        if torch.is_tensor(f):
            return f.to(self.device, torch.float64).reshape(-1)
        host = np.asarray(f, dtype=np.float64).reshape(-1)
        key = host.tobytes()
        cache = self.__dict__.setdefault("_f_cache", {})
        t = cache.get(key)
        if t is None:
            if len(cache) > 64:
                cache.clear()
            t = cache[key] = torch.from_numpy(host.copy()).to(self.device)
        return t

    def phi(self, st: StepRows, f, want32: bool = True) -> PaddedRows:
        ft = self._f(f)
        cap = max(1, min(st.m * st.L, st.n))
        cnt = self._empty(st.n_src, torch.int32)
        idx = self._empty(st.n_src * cap, torch.int32)
        val = self._empty(st.n_src * cap, torch.float64)
        v32 = self._empty(st.n_src * cap, torch.float32) if want32 else None
        C.check(self.lib.grf_phi(st.n_src, st.m, st.L, _p(st.cnt), _p(st.idx), _p(st.val), _p(ft), ft.numel(), cap,
                                 _p(cnt), _p(idx), _p(val), _p(v32), self.stream), "grf_phi")
        return PaddedRows(cnt, idx, val, v32, cap, st.n)

    def phi_fused(self, slots: Slots, f, norm: int = C.NORM_MUL_RECIP, want32: bool = True) -> PaddedRows:
        ft = self._f(f)
        ns, L, m = slots.n_src, slots.L, slots.m
        cap = max(1, min(m * L, slots.n))
        cnt = self._empty(ns, torch.int32)
        idx = self._empty(ns * cap, torch.int32)
        val = self._empty(ns * cap, torch.float64)
        v32 = self._empty(ns * cap, torch.float32) if want32 else None
        C.check(self.lib.grf_phi_fused(ns, m, L, norm, _p(slots.node), _p(slots.load), _p(ft), ft.numel(), cap,
                                       _p(cnt), _p(idx), _p(val), _p(v32), self.stream), "grf_phi_fused")
        return PaddedRows(cnt, idx, val, v32, cap, slots.n)

    def walk_phi(self, G: DeviceCSR, walks_per_node: int, p_halt: float, max_walk_length: int, f, *,
                 seed: int = 42, load_rule: int = C.LOAD_CUMULATIVE, norm: int = C.NORM_MUL_RECIP,
                 src_begin: int = 0, src_end: Optional[int] = None, want32: bool = True,
                 count_ws: Optional[torch.Tensor] = None, band_width: int = 0, use_aug: bool = True,
                 count_origin: int = 0, want64: bool = True) -> PaddedRows:
        """Philox walks straight to Phi rows (one kernel; identical to walk + features).

        count_ws: a zeroed transpose workspace (``transpose_workspace``) in which the kernel also
        counts the banded transpose's buckets, for ``transpose_banded(..., counted_ws=...)``;
        count_origin: the transposed matrix's first row (0: all of Phi; src_begin: these rows alone)."""
        n = G.n_rows
        src_end = n if src_end is None else src_end
        m, L = int(walks_per_node), int(max_walk_length)
        if m < 1 or L < 1:
            raise ValueError("walks_per_node and max_walk_length must be >= 1")
        ft = self._f(f)
        ns = src_end - src_begin
        cap = max(1, min(m * L, n))
        cnt = self._empty(ns, torch.int32)
        idx = self._empty(ns * cap, torch.int32)
        if not (want64 or want32):
            raise ValueError("walk_phi: want64 or want32")
        val = self._empty(ns * cap, torch.float64) if want64 else None  # (want64=False: f32 values only)
        v32 = self._empty(ns * cap, torch.float32) if want32 else None
        prm = C.GrfWalkParams(m, float(p_halt), L, int(load_rule), C.RNG_PHILOX, 0, 1, int(seed) & 0xFFFFFFFFFFFFFFFF)
        aug = self.walk_aug(G) if use_aug else None
        C.check(self.lib.grf_walk_phi(n, _p(G.ptr), _p(G.idx), _p(G.val), _p(aug), ctypes.byref(prm), src_begin,
                                      src_end,
                                      norm, _p(ft), ft.numel(), cap, _p(cnt), _p(idx), _p(val), _p(v32),
                                      _p(count_ws), int(band_width), int(count_origin), self.stream),
                "grf_walk_phi")
        return PaddedRows(cnt, idx, val, v32, cap, n)

    def walk_aug(self, G: DeviceCSR) -> Optional[torch.Tensor]:
        """The augmented walk matrix of G (grf_walk_aug), built once per DeviceCSR; None when
        nnz >= 2^32 (the walk then reads the row bounds per step)."""
        aug = getattr(G, "_aug", None)
        if aug is not None:
            return aug
        nnz = G.nnz_bound if getattr(G, "nnz_bound", None) is not None else G.nnz
        if nnz >= 2 ** 32:
            return None
        aug = torch.empty(max(int(self.lib.grf_walk_aug_bytes(nnz)), 32), dtype=torch.uint8, device=self.device)
        C.check(self.lib.grf_walk_aug(G.n_rows, _p(G.ptr), _p(G.idx), _p(G.val), _p(aug), self.stream), "grf_walk_aug")
        G._aug = aug
        return aug

    def features(self, slots: Slots, f, norm: int = C.NORM_MUL_RECIP) -> PaddedRows:
        """Phi rows; the fused kernel when m*L fits LDS, else steps + merge (bit-identical)."""
        if slots.m * slots.L <= 4096:
            return self.phi_fused(slots, f, norm)
        return self.phi(self.steps(slots, norm), f)

    # ------------------------------------------------------ sparse utilities
    def compact(self, rows: PaddedRows, want64: bool = True, want32: bool = True,
                sync_free: bool = False, stats: bool = False) -> DeviceCSR:
        """Compact CSR of padded rows.  sync_free: size the outputs by the padded capacity instead of
        reading nnz back (no host synchronisation; nnz is read lazily if asked for).  stats: also keep
        the rows' Gram shift statistics (``phi_row_shifts`` then skips its pass over the values)."""
        n = rows.n_rows
        ptr = self._empty(n + 1, torch.int64)
        ws = self._ws(self.lib.grf_scan_workspace_bytes(n))
        C.check(self.lib.grf_scan_counts(n, _p(rows.cnt), _p(ptr), _p(ws), ws.numel(), self.stream),
                "grf_scan_counts")
        nnz = n * rows.cap if sync_free else int(ptr[-1].item())
        idx = self._empty(nnz, torch.int32)
        v64 = self._empty(nnz, torch.float64) if want64 else None
        v32 = self._empty(nnz, torch.float32) if (want32 and rows.val32 is not None) else None
        st = None
        if stats and v32 is not None:
            st = torch.empty(int(self.lib.grf_phi_row_shifts_workspace_bytes(n)), dtype=torch.uint8,
                             device=self.device)
            C.check(self.lib.grf_compact_rows_stats(n, rows.cap, _p(rows.cnt), _p(ptr), _p(rows.idx),
                                                    _p(rows.val if want64 else None), _p(rows.val32), _p(idx),
                                                    _p(v64), _p(v32), _p(st), st.numel(), self.stream),
                    "grf_compact_rows_stats")
        else:
            C.check(self.lib.grf_compact_rows(n, rows.cap, _p(rows.cnt), _p(ptr), _p(rows.idx),
                                              _p(rows.val if want64 else None),
                                              _p(rows.val32 if v32 is not None else None), _p(idx), _p(v64),
                                              _p(v32), self.stream), "grf_compact_rows")
        out = DeviceCSR(n, rows.n_cols, ptr, idx, v64, v32, None if sync_free else nnz)
        out.row_stats = st
        out.nnz_bound = nnz
        return out

    def dense_to_scipy_csr(self, K: torch.Tensor):
        """K (dense fp32, on the device) as the scipy CSR the reference's sparse entry point returns
        (``Phi @ Phi.T``: float64 values, sorted int32 columns, exact zeros absent), built on the device
        (``grf_dense_to_csr_count`` / ``_fill``) and copied to the host once: indptr, indices, data."""
        import scipy.sparse as sp
        n_rows, n_cols = K.shape
        if K.dtype != torch.float32 or K.device != self.device or K.stride(1) != 1:
            raise ValueError("dense_to_scipy_csr: K must be a row-major float32 tensor on the engine's device")
        cnt = self._empty(n_rows, torch.int32)
        C.check(self.lib.grf_dense_to_csr_count(n_rows, n_cols, _p(K), K.stride(0), _p(cnt), self.stream),
                "grf_dense_to_csr_count")
        ptr = self._empty(n_rows + 1, torch.int64)
        ws = self._ws(self.lib.grf_scan_workspace_bytes(n_rows))
        C.check(self.lib.grf_scan_counts(n_rows, _p(cnt), _p(ptr), _p(ws), ws.numel(), self.stream),
                "grf_scan_counts")
        nnz = int(ptr[-1].item())
        idx, val = self._empty(nnz, torch.int32), self._empty(nnz, torch.float64)
        if nnz:
            C.check(self.lib.grf_dense_to_csr_fill(n_rows, n_cols, _p(K), K.stride(0), _p(ptr), _p(idx), _p(val),
                                                   self.stream), "grf_dense_to_csr_fill")
        out = sp.csr_matrix((val.cpu().numpy(), idx.cpu().numpy(), ptr.cpu().numpy()), shape=(n_rows, n_cols),
                            copy=False)
        out.has_sorted_indices = True  # (columns ascending within every row by construction)
        return out

    def step_matrices(self, st: StepRows) -> list[DeviceCSR]:
        """Per-step CSR matrices (rows = the sources of this step block)."""
        out = []
        cnt2 = st.cnt.view(st.n_src, st.L)
        for l in range(st.L):
            rows = PaddedRows(cnt2[:, l].contiguous(), st.idx[l * st.m:], st.val[l * st.m:], None, st.L * st.m, st.n)
            out.append(self.compact(rows, want64=True, want32=False))
        return out

    def steps_dense(self, st: StepRows, n_cols: Optional[int] = None) -> torch.Tensor:
        n_cols = st.n if n_cols is None else n_cols
        out = torch.zeros((st.n_src, n_cols, st.L), dtype=torch.float64, device=self.device)
        C.check(self.lib.grf_steps_densify(st.n_src, st.m, st.L, n_cols, _p(st.cnt), _p(st.idx), _p(st.val), _p(out),
                                           self.stream), "grf_steps_densify")
        return out

    def transpose_workspace(self, n_rows: int, n_cols: int, band_width: int = DEFAULT_BAND_WIDTH) -> torch.Tensor:
        """Zeroed workspace of ``transpose_banded`` (its first n_bands * n_cols int32 are bucket counts)."""
        nbk = -(-n_rows // band_width) * n_cols
        ws = self._ws(self.lib.grf_transpose_workspace_bytes(nbk))
        ws.zero_()
        return ws

    def transpose_banded(self, phi: DeviceCSR, band_width: int = DEFAULT_BAND_WIDTH,
                         counted_ws: Optional[torch.Tensor] = None, staged: Optional[bool] = None,
                         nnz_bound: Optional[int] = None, rec_unit: Optional[int] = None,
                         self_count: Optional[bool] = None, split: bool = False, slots: bool = False,
                         triples: bool = False) -> Banded:
        """Banded transpose of Phi.  counted_ws: workspace whose bucket counts ``walk_phi`` filled.
        staged: two-pass binned fill (default when band_width % 64 == 0) or the atomic fill.
        self_count: the staged fill without a plan (grf_transpose_banded_self; default unless
        counted_ws is given or GRF_TRANSPOSE_SELF=0): buckets in per-region slabs.
        nnz_bound: an upper bound of nnz(Phi) (e.g. ``compact(..., sync_free=True)``'s): the record
        buffer is then sized from bounds and no size is read back (no host synchronisation).
        split: (self-count transpose) lay every bucket out by sub-band and return the offsets
        (``Banded.t_split``) for the symmetric Gram's diagonal-tile skip -- measured no faster (a skip
        saves records inside lines the tile fetches anyway: profiles/r03_split_ab.txt), so off by default.
        slots: (self-count transpose) where the buckets are sparse enough for packed pairs and the bands
        wider than 4096 (8-wave Gram tiles), the GRF_REC_SLOT layout instead: each bucket's header and
        first two pairs in one 32-byte slot, so the Gram reads a small bucket with one line (the column
        blocks over power-law graphs, C5).  Not for the hub-column split (which edits descriptors).
        triples: (self-count transpose, band_width <= 4096, line buckets) 16-byte record triples instead of
        12-byte pairs: three entries per gathered stream position of the Gram (``Banded.rec_kind``); with
        split, slots, a wider band or the planned / atomic fills a ValueError (GRF_EINVAL), nothing launched."""
        n_rows, n_cols = phi.n_rows, phi.n_cols
        nb = -(-n_rows // band_width)
        nbk = nb * n_cols
        t_desc = self._empty(2 * (nbk + 1), torch.int32)
        t_max = self._empty(1, torch.float32)
        t_shift = self._empty(max(n_rows, 1), torch.int32)
        if staged is None:
            staged = band_width % 64 == 0 and os.environ.get("GRF_TRANSPOSE_STAGED", "1") != "0"
        if self_count is None:
            self_count = SELF_COUNT_TRANSPOSE and counted_ws is None and staged
        if triples and not self_count:
            raise ValueError("transpose_banded: record triples come from the self-counting transpose only "
                             "(not the planned or atomic fills)")
        if self_count:
            if counted_ws is not None or not staged:
                raise ValueError("self_count: the staged transpose counts its own buckets (no counted_ws)")
            if triples:  # (line buckets; the library refuses split, slots and bands wider than 4096)
                rec_unit = C.REC_SLOT if slots else C.REC_LINE if rec_unit is None else rec_unit
            elif slots and not split and rec_unit is None and band_width > 4096:
                u0 = _phi_rec_unit(phi, nnz_bound, band_width)
                rec_unit = C.REC_SLOT if u0 == C.REC_PACKED else u0
            return self._transpose_self(phi, band_width, nnz_bound, rec_unit, t_desc, t_max, t_shift, split, triples)
        ws = counted_ws if counted_ws is not None else self._ws(self.lib.grf_transpose_workspace_bytes(nbk))
        if rec_unit is None:
            rec_unit = _phi_rec_unit(phi, nnz_bound, band_width)
        u = int(rec_unit)
        C.check(self.lib.grf_transpose_banded_plan(n_rows, n_cols, band_width, u, _p(phi.ptr), _p(phi.idx),
                                                   _p(t_desc), int(counted_ws is not None), _p(ws), ws.numel(),
                                                   self.stream), "grf_transpose_banded_plan")
        # the Gram kernel addresses a band's records with 32-bit byte offsets.  A bucket of c entries
        # takes ceil(12 ceil(c / 2) / u) units: lines (u = 128) <= 0.047 c + 1.1, pairs (u = 12)
        # <= c, so a band of rows with at most `row_cap` entries each holds < 6 bw row_cap +
        # 141 n_cols bytes (lines) or 12 bw row_cap bytes (pairs).
        row_cap = min(n_cols, max(1, -(-(nnz_bound or 0) // max(n_rows, 1)))) if nnz_bound is not None else None
        band_bytes = (None if row_cap is None else
                      6 * band_width * row_cap + 141 * n_cols if u == C.REC_LINE else 12 * band_width * row_cap)
        if nnz_bound is not None and nb and band_bytes < 2 ** 31:
            # bound: no read-back
            units = int(0.047 * nnz_bound + 1.1 * nbk) + 1 if u == C.REC_LINE else int(nnz_bound) + 1
        else:
            # band starts (first unit of bucket (band, 0)) and the total, read back
            starts = torch.cat([t_desc[0:2 * nbk:2 * n_cols], t_desc[2 * nbk:2 * nbk + 1]]).cpu().numpy()
            starts = starts.view(np.uint32).astype(np.int64)
            tail = t_desc[2 * nbk:].cpu().numpy().view(np.uint32).astype(np.int64)
            units = int(tail[0] + (tail[1] << 32))
            starts[-1] = units
            if nb and int(np.diff(starts).max(initial=0)) * u >= 2 ** 31:
                raise NotImplementedError("a transpose band holds >= 2 GiB of records; use a smaller band_width")
        # (+128 B: a masked Gram lane reads the first pair of an empty last band)
        t_rec = self._empty(max(units, 1) * u + 128, torch.uint8)  # torch allocations are 256-B aligned
        if staged:
            nnz = nnz_bound if nnz_bound is not None else phi.nnz
            sg = self._ws(self.lib.grf_transpose_staging_bytes(n_rows, n_cols, band_width, nnz))
            C.check(self.lib.grf_transpose_banded_fill_staged(
                n_rows, n_cols, band_width, u, _p(phi.ptr), _p(phi.idx), _p(phi.val32), _p(t_desc), _p(t_rec),
                t_rec.numel(), _p(t_max), _p(t_shift), _p(ws), ws.numel(), nnz, _p(sg), sg.numel(), self.stream),
                "grf_transpose_banded_fill_staged")
        else:
            C.check(self.lib.grf_transpose_banded_fill(n_rows, n_cols, band_width, u, _p(phi.ptr), _p(phi.idx),
                                                       _p(phi.val32), _p(t_desc), _p(t_rec), t_rec.numel(),
                                                       _p(t_max), _p(t_shift), _p(ws), ws.numel(), self.stream),
                    "grf_transpose_banded_fill")
        return Banded(t_desc, t_rec, t_max, t_shift, band_width, n_rows, n_cols, u)

    def _transpose_self(self, phi: DeviceCSR, band_width: int, nnz_bound: Optional[int], rec_unit: Optional[int],
                        t_desc, t_max, t_shift, split: bool = False, triples: bool = False) -> Banded:
        """The plan-free staged transpose (grf_transpose_banded_self): buckets counted by the placing
        workgroups themselves, no counts from the walk and no scan over every bucket."""
        n_rows, n_cols = phi.n_rows, phi.n_cols
        nnz = int(nnz_bound) if nnz_bound is not None else phi.nnz
        if rec_unit is None:
            rec_unit = _phi_rec_unit(phi, nnz_bound, band_width)
        u = int(rec_unit)
        # the Gram addresses a band's records with 32-bit byte offsets: bound one band's slabs
        row_cap = min(n_cols, max(1, -(-nnz // max(n_rows, 1))))
        kind = C.REC_TRIPLES if triples else C.REC_PAIRS

        def units_bound(rows: int, entries: int) -> int:
            if triples:
                return self.lib.grf_transpose_self_triples_lines_bound(rows, n_cols, band_width, entries)
            return self.lib.grf_transpose_self_units_bound(rows, n_cols, band_width, u, entries)

        band_units = units_bound(min(band_width, n_rows), min(nnz, band_width * row_cap))
        if n_rows and band_units * u >= 2 ** 31:
            raise NotImplementedError("a transpose band holds >= 2 GiB of records; use a smaller band_width")
        units = units_bound(n_rows, nnz)
        if u == C.REC_SLOT and units * u >= 2 ** 30:
            # (slot offsets are counted from the first slot of all bands: fall back to packed pairs)
            return self._transpose_self(phi, band_width, nnz_bound, C.REC_PACKED, t_desc, t_max, t_shift, split)
        t_rec = self._empty(max(units, 1) * u + 128, torch.uint8)
        ws = self._ws(self.lib.grf_transpose_self_workspace_bytes(n_rows, n_cols, band_width))
        sg = self._ws(self.lib.grf_transpose_staging_bytes(n_rows, n_cols, band_width, nnz))
        nbk = -(-n_rows // band_width) * n_cols
        t_split = self._empty(8 * nbk, torch.int16) if split and band_width <= 8192 else None
        C.check(self.lib.grf_transpose_banded_self_rec(kind, n_rows, n_cols, band_width, u, _p(phi.ptr), _p(phi.idx),
                                                       _p(phi.val32), _p(t_desc), _p(t_split), _p(t_rec),
                                                       t_rec.numel(), _p(t_max), _p(t_shift), _p(ws), ws.numel(), nnz,
                                                       _p(sg), sg.numel(), self.stream),
                "grf_transpose_banded_self_rec")
        return Banded(t_desc, t_rec, t_max, t_shift, band_width, n_rows, n_cols, u, t_split, kind)

    # ----------------------------------------------------------------- Gram
    @staticmethod
    def leading_dim(n: int) -> int:
        return max(64, -(-n // 64) * 64)

    def gram_sparse(self, phi: DeviceCSR, tr: Banded, row_begin: int = 0, row_end: Optional[int] = None,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """K[row_begin:row_end, :] (float32) with leading dimension padded to 64."""
        n = tr.n_rows
        row_end = n if row_end is None else row_end
        ldk = self.leading_dim(n)
        if out is None:
            out = torch.empty((row_end - row_begin, ldk), dtype=torch.float32, device=self.device)
        C.check(self.lib.grf_gram_sparse_rec(tr.rec_kind, n, row_begin, row_end, _p(phi.ptr), _p(phi.idx),
                                             _p(phi.val32), tr.band_width, tr.rec_unit, _p(tr.t_desc), _p(tr.t_rec),
                                             _p(tr.t_rowshift), _p(out), out.stride(0), self.stream),
                "grf_gram_sparse_rec")
        return out[:, :n]

    def phi_row_shifts(self, phi: DeviceCSR) -> torch.Tensor:
        """The Gram fixed-point shifts of every row of Phi (int32 [n_rows]; grf_phi_row_shifts): the
        same values as ``transpose_banded(phi).t_rowshift``, for rows that are not in the transpose."""
        n = phi.n_rows
        shift = self._empty(max(n, 1), torch.int32)
        mx = self._empty(1, torch.float32)
        if isinstance(phi, PaddedRows):  # (the walk's rows, not compacted: grf_phi_row_shifts_padded)
            if phi.val32 is None:
                raise ValueError("phi_row_shifts: padded rows need their float32 values")
            ws = self._ws(self.lib.grf_phi_row_shifts_workspace_bytes(n))
            C.check(self.lib.grf_phi_row_shifts_padded(n, phi.cap, _p(phi.cnt), _p(phi.val32), _p(mx), _p(shift),
                                                       _p(ws), ws.numel(), self.stream), "grf_phi_row_shifts_padded")
            return shift
        st = getattr(phi, "row_stats", None)
        if st is not None:  # (left by compact(..., stats=True): same bits, no pass over the values)
            C.check(self.lib.grf_phi_row_shifts_stats(n, _p(st), _p(mx), _p(shift), self.stream),
                    "grf_phi_row_shifts_stats")
            return shift
        ws = self._ws(self.lib.grf_phi_row_shifts_workspace_bytes(n))
        C.check(self.lib.grf_phi_row_shifts(n, _p(phi.ptr), _p(phi.val32), _p(mx), _p(shift), _p(ws), ws.numel(),
                                            self.stream), "grf_phi_row_shifts")
        return shift

    def gram_sparse_cols(self, phi: DeviceCSR, row_shift: torch.Tensor, tr_b: Banded, row_begin: int = 0,
                         row_end: Optional[int] = None, out: Optional[torch.Tensor] = None,
                         sym_row0: Optional[int] = None) -> torch.Tensor:
        """Column block K[row_begin:row_end, B] = Phi[rows] Phi_B^T (float32) from the banded transpose
        ``tr_b`` of another row set Phi_B (grf_gram_sparse_cols); row_shift = ``phi_row_shifts(phi)``.
        With Phi_B = Phi[b:e] this is K[:, b:e], bit-identical to ``gram_sparse(...)[:, b:e]``;
        sym_row0 = b says so, and the square K[b:e, b:e] is then computed on and above its diagonal
        and mirrored (the symmetric mode's bits there)."""
        n = phi.n_rows
        row_end = n if row_end is None else row_end
        t_rows = tr_b.n_rows
        self._pairs_only(tr_b, "gram_sparse_cols")
        if out is None:
            out = torch.empty((row_end - row_begin, self.leading_dim(max(t_rows, 1))), dtype=torch.float32,
                              device=self.device)
        if isinstance(phi, PaddedRows):
            # Phi as the walk's padded rows (rows 0 .. n of Phi, not compacted): the pipelined kernel reads them
            if sym_row0 is not None or tr_b.rec_unit != C.REC_SLOT:
                raise ValueError("gram_sparse_cols: padded rows take a GRF_REC_SLOT transpose and no symmetric square")
            C.check(self.lib.grf_gram_sparse_cols_padded(phi.n_cols, row_begin, row_end, phi.cap, _p(phi.cnt),
                                                         _p(phi.idx), _p(phi.val32), _p(row_shift), t_rows,
                                                         tr_b.band_width, _p(tr_b.t_desc), _p(tr_b.t_rec), _p(out),
                                                         out.stride(0), self.stream), "grf_gram_sparse_cols_padded")
            return out[:, :t_rows]
        C.check(self.lib.grf_gram_sparse_cols(phi.n_cols, row_begin, row_end, _p(phi.ptr), _p(phi.idx),
                                              _p(phi.val32), _p(row_shift), t_rows,
                                              -1 if sym_row0 is None else int(sym_row0), tr_b.band_width, tr_b.rec_unit,
                                              _p(tr_b.t_desc), _p(tr_b.t_rec), _p(tr_b.t_split), _p(out), out.stride(0),
                                              _p(self._gram_ws), self._gram_ws.numel(), self.stream),
                "grf_gram_sparse_cols")
        return out[:, :t_rows]

    @staticmethod
    def _pairs_only(tr: Banded, who: str) -> None:
        if tr.rec_kind != C.REC_PAIRS:
            raise ValueError(f"{who}: record triples are read by the whole-K and row Gram only")

    def gram_sparse_kslice(self, phi: DeviceCSR, tr: Banded, k_begin: int, k_end: int, row_begin: int = 0,
                           row_end: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Partial K[row_begin:row_end, :] over the inner-dimension slice [k_begin, k_end) (float32)."""
        n = tr.n_rows
        row_end = n if row_end is None else row_end
        ldk = self.leading_dim(n)
        self._pairs_only(tr, "gram_sparse_kslice")
        if out is None:
            out = torch.empty((row_end - row_begin, ldk), dtype=torch.float32, device=self.device)
        C.check(self.lib.grf_gram_sparse_kslice(n, row_begin, row_end, k_begin, k_end, _p(phi.ptr), _p(phi.idx),
                                                _p(phi.val32), tr.band_width, tr.rec_unit, _p(tr.t_desc),
                                                _p(tr.t_rec),
                                                _p(tr.t_rowshift), _p(out), out.stride(0), _p(self._gram_ws),
                                                self._gram_ws.numel(), self.stream), "grf_gram_sparse_kslice")
        return out[:, :n]

    def gram_sparse_sym(self, phi: DeviceCSR, tr: Banded, out: Optional[torch.Tensor] = None,
                        skewed: bool = False) -> torch.Tensor:
        """Whole K (float32) on this device from the upper band tiles plus a mirror pass (skewed: see
        ``row_cuts``)."""
        n = tr.n_rows
        ldk = self.leading_dim(n)
        if out is None:
            out = torch.empty((n, ldk), dtype=torch.float32, device=self.device)
        cuts = self.row_cuts(phi, tr, skewed)
        if cuts is not None or tr.rec_kind != C.REC_PAIRS:  # (the waves' pair-balanced shares: same bits)
            self._gram_upper_cuts(phi, tr, out, cuts, (0, 1, 1), False)
            self.gram_mirror(out, n)
            return out[:, :n]
        C.check(self.lib.grf_gram_sparse_sym(n, _p(phi.ptr), _p(phi.idx), _p(phi.val32), tr.band_width,
                                             tr.rec_unit, _p(tr.t_desc), _p(tr.t_rec), _p(tr.t_split), _p(tr.t_rowshift),
                                             _p(out), out.stride(0),
                                             _p(self._gram_ws), self._gram_ws.numel(), self.stream),
                "grf_gram_sparse_sym")
        return out[:, :n]

    def row_cuts(self, phi: DeviceCSR, tr: Banded, skewed: bool = False) -> Optional[torch.Tensor]:
        """8 cuts per row of Phi splitting its nonzeros into shares of about equal record pairs (weights:
        every column's pairs -- or triples: the descriptors' counts -- over all bands of ``tr``), for the whole-K
        Gram's waves; None when the
        policy says no (GRF_GRAM_CUTS: auto = when ``skewed``, ``column_stats``) or the buckets are slots.
        Measured: Facebook 2.86-2.91 -> 2.75-2.79 ms per K; C4 (not skewed) would pay 0.5 ms for the
        cuts and gain nothing (profiles/r03_gram_balance_ab.txt)."""
        on = ROW_CUTS == "1" or (ROW_CUTS == "auto" and skewed)
        if not on or tr.rec_unit == C.REC_SLOT or phi.n_rows == 0:
            return None
        nb = -(-tr.n_rows // tr.band_width)
        col_w = torch.empty(max(1, tr.n_cols), dtype=torch.int32, device=self.device)
        cuts = torch.empty(8 * phi.n_rows, dtype=torch.int32, device=self.device)
        C.check(self.lib.grf_gram_row_cuts(phi.n_rows, _p(phi.ptr), _p(phi.idx), nb, tr.n_cols, _p(tr.t_desc),
                                           _p(col_w), _p(cuts), self.stream), "grf_gram_row_cuts")
        return cuts

    def _gram_upper_cuts(self, phi: DeviceCSR, tr: Banded, out: torch.Tensor, cuts: Optional[torch.Tensor], parts,
                         add_k: bool) -> None:
        """The upper tiles of either record kind, with row cuts or (None) without."""
        C.check(self.lib.grf_gram_sparse_upper_rec(tr.rec_kind, tr.n_rows, _p(phi.ptr), _p(phi.idx), _p(phi.val32),
                                                   tr.band_width, tr.rec_unit, _p(tr.t_desc), _p(tr.t_rec),
                                                   _p(tr.t_split), _p(tr.t_rowshift), _p(cuts), _p(out), out.stride(0),
                                                   int(parts[0]), int(parts[1]), int(parts[2]), int(add_k),
                                                   self.stream),
                "grf_gram_sparse_upper_rec")

    def gram_sparse_upper(self, phi: DeviceCSR, tr: Banded, out: torch.Tensor, parts=(0, 1, 1),
                          cuts: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The Gram half of ``gram_sparse_sym`` (tiles K[i, band >= band(i)]); ``gram_mirror`` completes K.
        parts = (begin, end, n): only those parts of the band-major tile sequence cut into n.
        cuts: ``row_cuts(phi, tr)`` (the waves' pair-balanced shares; same bits)."""
        n = tr.n_rows
        if cuts is not None or tr.rec_kind != C.REC_PAIRS:
            self._gram_upper_cuts(phi, tr, out, cuts, parts, False)
            return out[:, :n]
        C.check(self.lib.grf_gram_sparse_upper(n, _p(phi.ptr), _p(phi.idx), _p(phi.val32), tr.band_width,
                                               tr.rec_unit, _p(tr.t_desc), _p(tr.t_rec), _p(tr.t_split),
                                               _p(tr.t_rowshift), _p(out),
                                               out.stride(0), int(parts[0]), int(parts[1]), int(parts[2]),
                                               _p(self._gram_ws), self._gram_ws.numel(), self.stream),
                "grf_gram_sparse_upper")
        return out[:, :n]

    def hub_split(self, phi: DeviceCSR, tr: Banded, hubs: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """Split Phi's ``hubs`` densest columns off the banded transpose ``tr`` of Phi (modified in place:
        their buckets emptied in every band) into a dense fp32 panel P (n_rows x ldp, ldp a multiple of 32).
        The columns are ranked by their record pairs over all bands (the descriptors the transpose left:
        no host read), ties by column id; the panel holds them in ascending column order.
        Returns (P, cols).  Hub-heavy graphs: a column in a large share of the rows costs the sparse
        Gram one gathered record per multiply-add, the MFMA Gram of the panel ~60x less."""
        if tr.rec_unit == C.REC_SLOT:
            raise ValueError("hub_split: the GRF_REC_SLOT layout keeps no descriptor table to edit")
        n_rows, n = phi.n_rows, tr.n_cols
        h = max(0, min(int(hubs), n))
        nb = -(-tr.n_rows // tr.band_width)
        pairs = tr.t_desc[:2 * nb * n].view(nb, n, 2)[:, :, 1].sum(0, dtype=torch.int64)
        top = torch.sort(pairs, descending=True, stable=True).indices[:h]
        cols = torch.sort(top).values.to(torch.int32).contiguous()
        pos = torch.full((n,), -1, dtype=torch.int32, device=self.device)
        pos[cols.long()] = torch.arange(h, dtype=torch.int32, device=self.device)
        ldp = max(32, -(-h // 32) * 32)
        P = torch.zeros((n_rows, ldp), dtype=torch.float32, device=self.device)
        C.check(self.lib.grf_hub_panel(n_rows, _p(phi.ptr), _p(phi.idx), _p(phi.val32), _p(pos), _p(P), ldp,
                                       self.stream), "grf_hub_panel")
        C.check(self.lib.grf_transpose_drop_columns(nb, n, _p(tr.t_desc), _p(cols), h, self.stream),
                "grf_transpose_drop_columns")
        return P, cols

    def gram_sparse_sym_hubs(self, phi: DeviceCSR, tr: Banded, hubs: int, out: Optional[torch.Tensor] = None,
                             mirror_workgroups: int = 0, after_tiles=None, skewed: bool = False,
                             early_front: bool = False) -> torch.Tensor:
        """Whole K with the hub-column split: the panel of Phi's ``hubs`` densest columns through the
        MFMA Gram (tiles on and above the diagonal), the rest through the sparse Gram tiles adding to
        it, then the mirror.  ``tr`` is consumed (its hub buckets emptied).  Within the fp32 K
        tolerance of ``gram_sparse_sym`` (the hub part is an fp32 MFMA sum), exactly symmetric.
        ``after_tiles(event)``: called between the tiles and the mirror (the pipelined bench)."""
        n = tr.n_rows
        if out is None:
            out = torch.empty((n, self.leading_dim(n)), dtype=torch.float32, device=self.device)
        if int(hubs) <= 0:  # (no split: the plain symmetric Gram)
            self.gram_sparse_upper(phi, tr, out, cuts=self.row_cuts(phi, tr, skewed))
            ev = None
            if after_tiles is not None:
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(self.device))
            self.gram_mirror(out, n, mirror_workgroups)
            if after_tiles is not None:
                after_tiles(ev)
            return out[:, :n]
        P, cols = self.hub_split(phi, tr, hubs)
        h = int(cols.numel())
        if early_front and after_tiles is not None:
            # (the pipelined bench's next front beside the compute-bound MFMA panel, the tiles and the mirror)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.device))
            after_tiles(ev)
            after_tiles = None
        upper = self.lib.grf_gram_dense_split_upper if self.dense_precision == "split" else self.lib.grf_gram_dense_upper
        C.check(upper(n, h, _p(P), P.stride(0), _p(out), out.stride(0), self.stream), "grf_gram_dense_upper")
        cuts = self.row_cuts(phi, tr, skewed)  # (after the hub drop: the weights of the columns left)
        if cuts is not None or tr.rec_kind != C.REC_PAIRS:
            self._gram_upper_cuts(phi, tr, out, cuts, (0, 1, 1), True)
        else:
            C.check(self.lib.grf_gram_sparse_upper_add(n, _p(phi.ptr), _p(phi.idx), _p(phi.val32), tr.band_width,
                                                       tr.rec_unit, _p(tr.t_desc), _p(tr.t_rec), _p(tr.t_split),
                                                       _p(tr.t_rowshift), _p(out), out.stride(0), 0, 1, 1,
                                                       _p(self._gram_ws), self._gram_ws.numel(), self.stream),
                    "grf_gram_sparse_upper_add")
        ev = None
        if after_tiles is not None:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.device))
        self.gram_mirror(out, n, mirror_workgroups)
        if after_tiles is not None:
            after_tiles(ev)
        return out[:, :n]

    def gram_mirror(self, K: torch.Tensor, n: int, max_workgroups: int = 0) -> torch.Tensor:
        """K[j, i] = K[i, j] for every j > i (the second half of ``gram_sparse_sym``).
        max_workgroups > 0 bounds the grid (leaves CU slots to work on another stream)."""
        C.check(self.lib.grf_gram_mirror(n, _p(K), K.stride(0), int(max_workgroups), self.stream), "grf_gram_mirror")
        return K[:, :n]

    def densify(self, phi: DeviceCSR) -> torch.Tensor:
        lda = max(64, -(-phi.n_cols // 64) * 64)  # (zero-padded k: every k-tile width of the MFMA Gram divides it)
        out = torch.empty((phi.n_rows, lda), dtype=torch.float32, device=self.device)
        C.check(self.lib.grf_densify(phi.n_rows, _p(phi.ptr), _p(phi.idx), _p(phi.val32), _p(out), lda, self.stream),
                "grf_densify")
        return out

    def densify_padded(self, rows: PaddedRows, planes: bool = False):
        """The dense fp32 Phi (zero-padded lda, as ``densify``) straight from the walk's padded rows, no
        compaction (grf_densify_padded); rows too wide for one CU's LDS take compact + densify.
        planes: the split Gram's three bf16 planes instead (``DensePlanes``, grf_densify_padded_planes), for
        ``gram_dense``'s planes path."""
        n = rows.n_rows
        lda = max(64, -(-rows.n_cols // 64) * 64)
        if planes and rows.val32 is not None and -(-rows.n_cols // 16) * 64 <= 160 * 1024:
            ldp = int(self.lib.grf_planes_row_bytes(rows.n_cols))
            P = torch.empty((n, ldp), dtype=torch.uint8, device=self.device)
            C.check(self.lib.grf_densify_padded_planes(n, rows.cap, rows.n_cols, _p(rows.cnt), _p(rows.idx),
                                                       _p(rows.val32), _p(P), ldp, self.stream),
                    "grf_densify_padded_planes")
            return DensePlanes(P, n, rows.n_cols)
        if rows.val32 is None or lda * 4 > 160 * 1024:
            out = self.densify(self.compact(rows, want64=False, sync_free=True))
            return self.split_planes(out, rows.n_cols) if planes else out
        out = torch.empty((n, lda), dtype=torch.float32, device=self.device)
        C.check(self.lib.grf_densify_padded(n, rows.cap, rows.n_cols, _p(rows.cnt), _p(rows.idx), _p(rows.val32),
                                            _p(out), lda, self.stream), "grf_densify_padded")
        return self.split_planes(out, rows.n_cols) if planes else out

    @staticmethod
    def use_planes(n: int) -> bool:
        """The split Gram on pre-split bf16 planes (grf_gram_dense_planes) where the wide kernels run (from 64 tile
        rows on, n > 8064; GRF_DENSE_WIDE=0 turns it off with them): with the wide kernels' XCD-ordered whole-item
        rounds the staged k-tiles are L2 / Infinity-Cache hits, so staging the planes' 1.5x bytes costs less than
        the split's VALU -- C2 Gram 4.40 -> 4.01 ms (profiles/r06_dense_xcd_ab.txt; before those rounds the planes
        were staging-bound and slower, r06_dense_planes_ab.txt).  Below, the 128-tile kernel splits in registers:
        its planes twin (gram_planes_tile_kernel) measured equal at C3 (0.133 ms both: that Gram is bound by neither
        the split nor the staged bytes).  GRF_DENSE_PLANES (read per call): 1 always, 0 never.  Same K bits."""
        env = os.environ.get("GRF_DENSE_PLANES")
        if env in ("0", "1"):
            return env == "1"
        return -(-int(n) // 128) >= 64 and os.environ.get("GRF_DENSE_WIDE") != "0"

    def split_planes(self, dense_phi: torch.Tensor, k_dim: int) -> "DensePlanes":
        """The dense fp32 Phi's three bf16 planes, split once (grf_split_planes)."""
        n = dense_phi.shape[0]
        ldp = int(self.lib.grf_planes_row_bytes(k_dim))
        P = torch.empty((n, ldp), dtype=torch.uint8, device=self.device)
        C.check(self.lib.grf_split_planes(n, k_dim, _p(dense_phi), dense_phi.stride(0), _p(P), ldp, self.stream),
                "grf_split_planes")
        return DensePlanes(P, n, k_dim)

    def gram_dense(self, dense_phi: torch.Tensor, k_dim: int, precision: Optional[str] = None) -> torch.Tensor:
        """K = A A^T of the dense fp32 Phi on the MFMA.  precision 'fp32': the fp32 matrix instruction
        (grf_gram_dense_ws); 'split': the same product on the bf16 matrix cores from an exact three-plane
        split of A (grf_gram_dense_split, error bound the fp32 path's + (2^-23 + 2^-32) sum |a b|); None: the engine's
        ``dense_precision`` (GRF_GRAM_DENSE_PRECISION, default 'split')."""
        precision = precision or self.dense_precision
        if precision not in ("fp32", "split"):
            raise ValueError(f"unknown dense Gram precision {precision!r}")
        split = precision == "split"
        planes = isinstance(dense_phi, DensePlanes)
        if planes and not split:
            raise ValueError("gram_dense: the bf16 planes take precision 'split'")
        if split and not planes and self.use_planes(dense_phi.shape[0]):
            dense_phi = self.split_planes(dense_phi, k_dim)  # (the split once, then the planes' k-loop)
            planes = True
        n = dense_phi.shape[0]
        ldk = self.leading_dim(n)
        out = torch.empty((n, ldk), dtype=torch.float32, device=self.device)
        # split-K partial tiles (small n, or the last tiles of a large n) and their tickets: a cached
        # workspace per stream, ZEROED when allocated (the kernel leaves the tickets zero after every
        # launch; an uninitialised block gave round 4's NaN, profiles/AB_LOG.md "dense-Gram NaN"), dropped
        # after a failed call so that no ticket a broken launch may have left is read again.  The split
        # path sizes it for its own (wide-workgroup) slabs as well.
        need = int(self.lib.grf_gram_dense_split_workspace_bytes(n, k_dim) if split
                   else self.lib.grf_gram_dense_workspace_bytes(n, k_dim))
        stream = self.stream
        cache = self.__dict__.setdefault("_dense_ws", {})
        ws = cache.get(stream.value)
        if ws is None or ws.numel() < need:
            ws = cache[stream.value] = torch.zeros(max(need, 16), dtype=torch.uint8, device=self.device)
        fn = self.lib.grf_gram_dense_split if split else self.lib.grf_gram_dense_ws
        try:
            if planes:
                C.check(self.lib.grf_gram_dense_planes(n, k_dim, _p(dense_phi.P), dense_phi.P.stride(0), _p(out), ldk,
                                                       _p(ws), ws.numel(), stream), "grf_gram_dense_planes")
            else:
                C.check(fn(n, k_dim, _p(dense_phi), dense_phi.stride(0), _p(out), ldk, _p(ws), ws.numel(), stream),
                        "grf_gram_dense_split" if split else "grf_gram_dense_ws")
        except Exception:
            cache.pop(stream.value, None)
            raise
        return out[:, :n]

    @staticmethod
    def column_stats(phi: DeviceCSR, share: float = HUB_SHARE,
                     extend: Optional[float] = None) -> Tuple[int, bool]:
        """(hub_count, skewed) from one column count of Phi: skewed when the densest column holds at
        least SKEW_RATIO times the mean column's entries (the policy of ``row_cuts``).  extend: when at least
        one panel width of columns reaches ``share``, the hub count is taken at this (lower) share instead
        (``HUB_EXTEND_SHARE``, the split panel's).  One host read."""
        n = phi.n_cols
        if phi.nnz == 0 or n == 0:
            return 0, False
        c = torch.bincount(phi.idx[:phi.nnz].long(), minlength=n)
        low = share if extend is None else min(share, extend)
        hubs, wide, cmax = (int(x) for x in torch.stack([(c >= share * phi.n_rows).sum(),
                                                          (c >= low * phi.n_rows).sum(), c.max()]).tolist())
        hubs = hubs // 32 * 32
        if hubs and extend is not None:
            hubs = wide // 32 * 32
        return hubs, cmax >= SKEW_RATIO * phi.nnz / n

    def hub_extend_share(self) -> Optional[float]:
        """The panel's extension share for this engine's dense precision (None: the fp32 panel)."""
        return HUB_EXTEND_SHARE if self.dense_precision == "split" else None

    def hub_count(self, phi: DeviceCSR, share: float = HUB_SHARE) -> int:
        """Hub columns worth the dense MFMA panel of the hub-column split (the policy of ``gram_sparse_auto``
        and the bench's --hubs auto): the columns of Phi present in at least ``share`` of its rows, in
        multiples of 32 (the panel's width) -- with the split panel, once there are any, those down to
        ``HUB_EXTEND_SHARE``.  A column in c of the n rows saves ~c^2 / 2 gathered records and costs n^2 / 2
        MFMA multiply-adds, ~60x cheaper each on the fp32 panel, so it pays from c / n ~ 1 / sqrt(60) = 0.13
        (profiles/r02_hubs_sweep.txt); the split panel's 3/8 of that cost moved Enron's best count from 96 to
        192 columns (profiles/r05_hub_sweep_split.txt).  One host read."""
        return self.column_stats(phi, share, extend=self.hub_extend_share())[0]

    def gram_sparse_auto(self, phi: DeviceCSR, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Whole K on the sparse path exactly as the bench assembles it: the symmetric tiles + mirror,
        with the hub-column split when Phi has hub columns (``hub_count``)."""
        tr = self.transpose_banded(phi)
        hubs, skewed = self.column_stats(phi, extend=self.hub_extend_share())
        if hubs:
            return self.gram_sparse_sym_hubs(phi, tr, hubs, out=out, skewed=skewed)
        return self.gram_sparse_sym(phi, tr, out=out, skewed=skewed)

    def gram(self, phi: DeviceCSR, method: str = "auto") -> torch.Tensor:
        """K = Phi Phi^T (float32).  'dense' = MFMA on densified Phi, 'sparse' = LDS Gustavson (+ the
        hub-column split when Phi has hub columns); 'auto' picks by the measured crossover."""
        if method == "auto":
            method = "dense" if phi.n_rows <= DENSE_GRAM_MAX_N else "sparse"
        if method == "dense":
            return self.gram_dense(self.densify(phi), phi.n_cols)
        if method == "sparse":
            return self.gram_sparse_auto(phi)
        if method == "sparse-rows":
            return self.gram_sparse(phi, self.transpose_banded(phi, ROWS_BAND_WIDTH))
        raise ValueError(f"unknown gram method {method!r}")

    # ------------------------------------- K.v and CG (models/sparse_grf_model.py:21-45)
    def _row_map(self, rows) -> Optional[torch.Tensor]:
        if rows is None:
            return None
        return torch.as_tensor(rows, device=self.device).to(torch.int32).flatten().contiguous()

    def csr_transpose(self, phi: DeviceCSR, rows=None) -> DeviceCSR:
        """(Phi[rows])^T as CSR (n_cols x len(rows), float32); column lists in ascending row order."""
        rmap = self._row_map(rows)
        n_sel = phi.n_rows if rmap is None else rmap.numel()
        # the entries to transpose, or an upper bound of them (no host read; the C side ignores the tail)
        exact = True
        if rmap is None:
            nnz = phi.nnz_or_bound()
            exact = phi._nnz is not None
        elif phi.rows_entry_bound(n_sel) is not None:
            nnz, exact = phi.rows_entry_bound(n_sel), False
        else:
            rl = rmap.long()
            nnz = int((phi.ptr[rl + 1] - phi.ptr[rl]).sum().item()) if n_sel else 0
        t_ptr = self._empty(phi.n_cols + 1, torch.int64)
        t_idx = self._empty(nnz, torch.int32)
        t_val = self._empty(nnz, torch.float32)
        ws = self._ws(self.lib.grf_csr_transpose_workspace_bytes(n_sel, phi.n_cols, nnz))
        C.check(self.lib.grf_csr_transpose(n_sel, _p(phi.ptr), _p(phi.idx), _p(phi.val32), _p(rmap), phi.n_cols, nnz,
                                           _p(t_ptr), _p(t_idx), _p(t_val), _p(ws), ws.numel(), self.stream),
                "grf_csr_transpose")
        return DeviceCSR(phi.n_cols, n_sel, t_ptr, t_idx, None, t_val, nnz if exact else None, nnz_bound=nnz)

    def spmm(self, A: DeviceCSR, X: torch.Tensor, rows=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Y = A[rows] X (X float32 or float64, n_cols x S with unit column stride; Y the same type)."""
        if X.dtype not in (torch.float32, torch.float64) or X.dim() != 2 or X.stride(1) != 1 \
                or X.shape[0] != A.n_cols:
            raise ValueError("spmm: X must be a float32/float64 (n_cols x S) row-major matrix")
        rmap = self._row_map(rows)
        n_out = A.n_rows if rmap is None else rmap.numel()
        S = X.shape[1]
        if out is None:
            out = torch.empty((n_out, S), dtype=X.dtype, device=self.device)
        fn = self.lib.grf_spmm_csr if X.dtype == torch.float32 else self.lib.grf_spmm_csr_f64
        C.check(fn(n_out, _p(A.ptr), _p(A.idx), _p(A.val32), _p(rmap), _p(X), X.stride(0), S, _p(out),
                   out.stride(0), self.stream), "grf_spmm_csr")
        return out

    # ------------------------------------------------- sparse x sparse: the exact step matrices
    SPGEMM_ENTRY_BYTES = 16  # an output entry: int32 column, float64 and float32 value

    def _spgemm(self, A: DeviceCSR, B: DeviceCSR, max_nnz: Optional[int], what: str) -> DeviceCSR:
        if A.n_cols != B.n_rows:
            raise ValueError(f"spgemm: A is {A.n_rows} x {A.n_cols} but B has {B.n_rows} rows")
        a_val = A.val if A.val is not None else A.val32.double()
        b_val = B.val if B.val is not None else B.val32.double()
        n, n_mid, n_cols = A.n_rows, A.n_cols, B.n_cols
        ws = self._ws(self.lib.grf_spgemm_workspace_bytes(n, n_mid, n_cols))
        cnt = self._empty(n, torch.int32)
        C.check(self.lib.grf_spgemm_csr_count(n, n_mid, n_cols, _p(A.ptr), _p(A.idx), _p(B.ptr), _p(B.idx), _p(cnt),
                                              _p(ws), ws.numel(), self.stream), "grf_spgemm_csr_count")
        ptr = self._empty(n + 1, torch.int64)
        sws = self._ws(self.lib.grf_scan_workspace_bytes(n))
        C.check(self.lib.grf_scan_counts(n, _p(cnt), _p(ptr), _p(sws), sws.numel(), self.stream), "grf_scan_counts")
        nnz = int(ptr[-1].item())  # (set-up, as preprocessing is: the one host read per product)
        if max_nnz is None:
            max_nnz = torch.cuda.mem_get_info(self.device)[0] // self.SPGEMM_ENTRY_BYTES
        if nnz > max_nnz:
            raise ValueError(f"{what} has nnz = {nnz}, more than max_nnz = {int(max_nnz)}")
        idx = self._empty(max(nnz, 1), torch.int32)
        val = self._empty(max(nnz, 1), torch.float64)
        val32 = self._empty(max(nnz, 1), torch.float32)
        C.check(self.lib.grf_spgemm_csr_fill(n, n_mid, n_cols, _p(A.ptr), _p(A.idx), _p(a_val), _p(B.ptr), _p(B.idx),
                                             _p(b_val), _p(ptr), _p(idx), _p(val), _p(val32), _p(ws), ws.numel(),
                                             self.stream), "grf_spgemm_csr_fill")
        return DeviceCSR(n, n_cols, ptr, idx, val, val32, nnz)

    def spgemm(self, A: DeviceCSR, B: DeviceCSR, max_nnz: Optional[int] = None) -> DeviceCSR:
        """C = A B (CSR x CSR -> compact CSR, fp64 and fp32 values, ``nnz`` known) by the fixed rule of
        include/grf.h grf_spgemm_csr_*: structural pattern (exact-zero sums kept), columns ascending, every
        entry summed from +0.0 in the order of A's row entries without FMA -- scipy's ``A @ B`` to the bit."""
        return self._spgemm(A, B, max_nnz, "spgemm: the product")

    def exact_steps(self, G: DeviceCSR, max_walk_length: int, max_nnz: Optional[int] = None) -> list[DeviceCSR]:
        """The exact step matrices [I, G, G^2, ...] (``max_walk_length`` of them, M_l = M_{l-1} G: the
        reference's compute_pstep_walk_matrix, general_kernel_pofm.py:7-42) as device CSR -- what the walk
        estimator's M_l are the expectation of.  A power with more than ``max_nnz`` entries (default: what
        fits in free device memory) raises ValueError before it is allocated."""
        if G.n_rows != G.n_cols:
            raise ValueError("exact_steps: the walk matrix must be square")
        if max_walk_length < 1:
            raise ValueError("exact_steps: max_walk_length must be at least 1")
        n = G.n_rows
        ar = torch.arange(n + 1, dtype=torch.int64, device=self.device)
        M = DeviceCSR(n, n, ar, ar[:n].to(torch.int32), torch.ones(n, dtype=torch.float64, device=self.device),
                      torch.ones(n, dtype=torch.float32, device=self.device), n)
        steps = [M]
        for l in range(1, int(max_walk_length)):
            M = self._spgemm(M, G, max_nnz, f"exact_steps: step {l}")
            steps.append(M)
        return steps

    def gram_matvec(self, phi: DeviceCSR, V: torch.Tensor, rows=None, cols=None, phi_t: Optional[DeviceCSR] = None,
                    noise: float = 0.0) -> torch.Tensor:
        """K[rows, cols] V = Phi[rows] (Phi[cols]^T V) (+ noise V when rows == cols), K never formed."""
        phi_t = self.csr_transpose(phi, cols) if phi_t is None else phi_t
        Y = self.spmm(phi, self.spmm(phi_t, V), rows)
        if noise:
            Y.add_(V, alpha=float(noise))
        return Y

    def _precond(self, precond, n_sys: int, B: torch.Tensor, what: str) -> Optional[torch.Tensor]:
        """The checked inverse diagonal of a preconditioned solve (None: the plain solve)."""
        if precond is None:
            return None
        if B.dtype != torch.float64:
            raise ValueError(f"{what}: a preconditioned solve needs a float64 B")
        if not isinstance(precond, torch.Tensor) or precond.dtype != torch.float64 or precond.numel() != n_sys:
            raise ValueError(f"{what}: precond must be a float64 tensor of {n_sys} inverse diagonal entries")
        return precond.to(self.device).flatten().contiguous()

    def gram_jacobi(self, phi: DeviceCSR, rows=None, noise: float = 0.0) -> torch.Tensor:
        """dinv[r] = 1 / (sum_e Phi[rows[r], e]^2 + noise) = 1 / diag(Phi_T Phi_T^T + noise I)[r], fp64 on the
        device (grf_gram_jacobi_f64): the Jacobi preconditioner of ``cg_solve(precond=...)``.  The squares are
        summed in the row's stored order; a row whose sum plus noise is not positive gets 1."""
        if phi.val32 is None:
            raise ValueError("gram_jacobi: Phi needs its float32 values (val32)")
        rmap = self._row_map(rows)
        n_sel = phi.n_rows if rmap is None else rmap.numel()
        dinv = self._empty(n_sel, torch.float64)
        C.check(self.lib.grf_gram_jacobi_f64(n_sel, _p(phi.ptr), _p(phi.idx), _p(phi.val32), _p(rmap), float(noise),
                                             _p(dinv), self.stream), "grf_gram_jacobi_f64")
        return dinv

    def poly_jacobi(self, op: WalkPolynomial, f, rows, noise: float) -> torch.Tensor:
        """The same inverse diagonal for the exact kernel: 1 / (poly_kernel_diag(op, f, x=rows) + noise).  Correct
        but dear -- the diagonal costs len(rows) / 256 operator chains, about as much as that many CG
        iterations -- and the exact kernel is well conditioned, so this mostly serves as the default behind
        ``preconditioner="jacobi"``; pass an explicit ``precond`` vector where a cheaper diagonal is at hand."""
        d = self.poly_kernel_diag(op, f, x=rows) + float(noise)
        return torch.where(d > 0, 1.0 / d, torch.ones_like(d))

    def cg_solve(self, phi: DeviceCSR, B: torch.Tensor, noise: float, rows=None, phi_t: Optional[DeviceCSR] = None,
                 tolerance: float = 1.0, max_iter: int = 1000, return_residuals: bool = False,
                 return_lanczos: bool = False, precond: Optional[torch.Tensor] = None):
        """linear_cg on (Phi[rows] Phi[rows]^T + noise I) X = B for the columns of B (n x S, S <= 256).

        B float64 runs the recurrence in fp64, float32 in the reference's fp32.  Returns
        (X, iterations) [+ the final residual norms of the normalised columns].  tolerance / max_iter default to gpytorch's settings.cg_tolerance (1)
        and settings.max_cg_iterations (1000).  return_lanczos (fp64 only) appends the CG coefficients, a
        (2 max_iter x S) fp64 device tensor: row k holds alpha_k of every column, row max_iter + k its
        beta_k, zero for the iterations that did not run (the Lanczos tridiagonals come from these).
        precond (fp64 only): the inverse diagonal ``dinv`` (n,) of a diagonal preconditioner, e.g.
        ``gram_jacobi(phi, rows, noise)``: linear_cg with the closure z = dinv . r (grf_pcg_gram_solve_f64); the
        residual norms and the stopping rule stay those of the unpreconditioned residual, and the coefficients
        are then the Lanczos coefficients of D^-1/2 K^ D^-1/2.  Ones reproduce the plain solve bit for bit."""
        rmap = self._row_map(rows)
        n_sys = phi.n_rows if rmap is None else rmap.numel()
        if B.dtype not in (torch.float32, torch.float64) or B.dim() != 2 or B.stride(1) != 1 \
                or B.shape[0] != n_sys:
            raise ValueError("cg_solve: B must be a float32/float64 (n_rows x S) row-major matrix")
        if return_lanczos and B.dtype != torch.float64:
            raise ValueError("cg_solve: return_lanczos needs a float64 B")
        dinv = self._precond(precond, n_sys, B, "cg_solve")
        phi_t = self.csr_transpose(phi, rmap) if phi_t is None else phi_t
        operator = (n_sys, _p(phi.ptr), _p(phi.idx), _p(phi.val32), _p(rmap), phi.n_cols, _p(phi_t.ptr),
                    _p(phi_t.idx), _p(phi_t.val32))
        return self._cg_call("gram", operator, phi.n_cols, B, noise, tolerance, max_iter, dinv, return_residuals,
                             return_lanczos)

    def _cg_call(self, family: str, operator: tuple, n_inner: int, B: torch.Tensor, noise: float, tolerance: float,
                 max_iter: int, dinv: Optional[torch.Tensor], return_residuals: bool, return_lanczos: bool):
        """What cg_solve and cg_solve_poly share: one solve's buffers, its C entry from CG_ENTRIES called with the
        operator's own arguments (n_sys first), the recurrence's and the entry's trailing ones, the return tuple."""
        n_sys, S = operator[0], B.shape[1]
        X = torch.empty((n_sys, S), dtype=B.dtype, device=self.device)
        ws = self._ws(getattr(self.lib, CG_WORKSPACES[family, dinv is not None])(n_sys, n_inner, S))
        iters = ctypes.c_int32(0)
        resid = np.zeros(S, np.float64)
        args = operator + (float(noise), _p(B), B.stride(0), S, float(tolerance), int(max_iter), _p(X), X.stride(0),
                           _p(ws), ws.numel(), ctypes.byref(iters), resid.ctypes.data_as(ctypes.c_void_p))
        coef = None
        if return_lanczos:
            coef = torch.empty((2 * max(int(max_iter), 0), S), dtype=torch.float64, device=self.device)
            args += (_p(coef), S)
        if dinv is not None:
            args += (_p(dinv),)
        name = CG_ENTRIES[family, B.dtype == torch.float64, bool(return_lanczos), dinv is not None]
        C.check(getattr(self.lib, name)(*args, self.stream), name)
        return (X, int(iters.value)) + ((resid,) if return_residuals else ()) + ((coef,) if return_lanczos else ())

    # ------------------------------------- matrix-free marginal likelihood (CG + stochastic Lanczos quadrature)
    def steps_frob(self, steps, rows, A: torch.Tensor, WA: torch.Tensor, B: torch.Tensor, WB: torch.Tensor,
                   wt: torch.Tensor, n_steps: Optional[int] = None) -> torch.Tensor:
        """out[l] = sum_c wt[c] sum_r (A[r,c] (M_l[rows[r]] WB)[c] + B[r,c] (M_l[rows[r]] WA)[c]) for the first
        n_steps (default: all) step matrices of ``steps`` (a features.StepMatrices): (L,) fp64 on the device.
        A, B: (len(rows) x S), WA, WB: (n_cols x S), fp64 row-major, S <= 256 (grf_steps_frob_f64)."""
        rmap = self._row_map(rows)
        n_sel = steps.shape[0] if rmap is None else rmap.numel()
        L = steps.L if n_steps is None else int(n_steps)
        if not 1 <= L <= steps.L:
            raise ValueError("steps_frob: n_steps must be in [1, L]")
        if A.dim() != 2 or A.shape[0] != n_sel or B.shape != A.shape or WA.dim() != 2 or WB.shape != WA.shape \
                or WA.shape != (steps.shape[1], A.shape[1]):
            raise ValueError("steps_frob: A, B must be (rows x S) and WA, WB (n_cols x S)")
        if wt.numel() != A.shape[1]:
            raise ValueError("steps_frob: wt must hold one weight per column")
        A, B, WA, WB, wt = (t.to(self.device, torch.float64).contiguous() for t in (A, B, WA, WB, wt.flatten()))
        S = A.shape[1]
        out = self._empty(L, torch.float64)
        ws = self._ws(self.lib.grf_steps_frob_workspace_bytes(n_sel, L))
        sp = steps._ptrs
        C.check(self.lib.grf_steps_frob_f64(n_sel, L, sp[0], sp[1], sp[2], _p(rmap), _p(A), _p(B), max(S, 1), _p(WA),
                                            _p(WB), max(S, 1), _p(wt), S, _p(out), _p(ws), ws.numel(), self.stream),
                "grf_steps_frob_f64")
        return out

    # ------------------------------------- the exact kernel as a matrix-free operator (WalkPolynomial)
    def _poly_f(self, op: WalkPolynomial, f) -> Tuple[torch.Tensor, int]:
        ft = torch.as_tensor(f).detach().to(self.device, torch.float64).flatten().contiguous()
        if ft.numel() < 1:
            raise ValueError("the modulator needs at least one entry")
        return ft, op.n_terms(ft)

    def _inv_map(self, rmap: torch.Tensor, n: int) -> torch.Tensor:
        """node -> its position in rmap, or -1 (int32 [n]); rmap must not repeat a node."""
        inv = torch.full((n,), -1, dtype=torch.int32, device=self.device)
        inv[rmap.long()] = torch.arange(rmap.numel(), dtype=torch.int32, device=self.device)
        if int((inv >= 0).sum().item()) != rmap.numel():
            raise ValueError("a row selection of the walk operator must not repeat a node")
        return inv

    @staticmethod
    def _check_block(X: torch.Tensor, n_rows: int, what: str) -> None:
        if X.dtype != torch.float64 or X.dim() != 2 or X.stride(1) != 1 or X.shape[0] != n_rows:
            raise ValueError(f"{what} must be a float64 ({n_rows} x S) row-major matrix")

    def poly_apply(self, op: WalkPolynomial, f, X: torch.Tensor, in_rows=None, out_rows=None,
                   transpose: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Y = (p(G) S_in^T X)[out_rows] (``transpose``: p(G^T)) by Horner chains with the walk matrix
        (grf_poly_apply_f64; fp64, S <= 256).  in_rows: the nodes X's rows belong to (None: X has a row per
        node); out_rows: the rows wanted (None: all)."""
        ft, n_f = self._poly_f(op, f)
        A = op.Gt if transpose else op.G
        n = A.n_rows
        imap = self._row_map(in_rows)
        self._check_block(X, n if imap is None else imap.numel(), "poly_apply: X")
        inv = None if imap is None else self._inv_map(imap, n)
        rmap = self._row_map(out_rows)
        n_out = n if rmap is None else rmap.numel()
        S = X.shape[1]
        if out is None:
            out = torch.empty((n_out, S), dtype=torch.float64, device=self.device)
        ws = self._ws(self.lib.grf_poly_workspace_bytes(n, n_f, S))
        C.check(self.lib.grf_poly_apply_f64(n, _p(A.ptr), _p(A.idx), _p(A.val), _p(ft), n_f, _p(inv), _p(rmap), n_out,
                                            _p(X), X.stride(0), S, _p(out), out.stride(0), _p(ws), ws.numel(),
                                            self.stream), "grf_poly_apply_f64")
        return out

    def poly_gram_matvec(self, op: WalkPolynomial, f, V: torch.Tensor, rows=None, cols=None,
                         noise: float = 0.0) -> torch.Tensor:
        """K[rows, cols] V = S_rows p(G) p(G)^T S_cols^T V (+ noise V when rows == cols), K never formed."""
        W = self.poly_apply(op, f, V, in_rows=cols, transpose=True)
        Y = self.poly_apply(op, f, W, out_rows=rows)
        if noise:
            Y.add_(V, alpha=float(noise))
        return Y

    def cg_solve_poly(self, op: WalkPolynomial, f, B: torch.Tensor, noise: float, rows, tolerance: float = 1.0,
                      max_iter: int = 1000, return_residuals: bool = False, return_lanczos: bool = False,
                      precond: Optional[torch.Tensor] = None):
        """``cg_solve`` on (S_T p(G) p(G)^T S_T^T + noise I) X = B for the training nodes ``rows`` (fp64): the
        same recurrence and return shape, every matvec two Horner chains with the walk matrix.  ``precond``: the
        inverse diagonal of a diagonal preconditioner, as in ``cg_solve`` (grf_pcg_poly_solve_f64)."""
        ft, n_f = self._poly_f(op, f)
        rmap = self._row_map(rows)
        if rmap is None:
            rmap = torch.arange(op.shape[0], dtype=torch.int32, device=self.device)
        n_sys, n = rmap.numel(), op.shape[0]
        self._check_block(B, n_sys, "cg_solve_poly: B")
        dinv = self._precond(precond, n_sys, B, "cg_solve_poly")
        inv = self._inv_map(rmap, n)
        G, Gt = op.G, op.Gt
        operator = (n_sys, n, _p(G.ptr), _p(G.idx), _p(G.val), _p(Gt.ptr), _p(Gt.idx), _p(Gt.val), _p(ft), n_f,
                    _p(rmap), _p(inv))
        return self._cg_call("poly", operator, n, B, noise, tolerance, max_iter, dinv, return_residuals,
                             return_lanczos)

    def poly_grad(self, op: WalkPolynomial, f, rows, A: torch.Tensor, B: torch.Tensor,
                  wt: torch.Tensor) -> torch.Tensor:
        """out[l] = sum_c wt[c] a_c^T (dK/df_l) b_c for K = S_T p(G) p(G)^T S_T^T, T = ``rows``, and the
        columns a_c, b_c of A, B (len(rows) x S, fp64): (n_f,) fp64 on the device (grf_poly_grad_f64)."""
        ft, n_f = self._poly_f(op, f)
        rmap = self._row_map(rows)
        n_sel, n = rmap.numel(), op.shape[0]
        A, B = (t.to(self.device, torch.float64).contiguous() for t in (A, B))
        self._check_block(A, n_sel, "poly_grad: A")
        self._check_block(B, n_sel, "poly_grad: B")
        wt = wt.to(self.device, torch.float64).flatten().contiguous()
        S = A.shape[1]
        if B.shape != A.shape or wt.numel() != S:
            raise ValueError("poly_grad: A, B must be (rows x S) with one weight per column")
        inv = self._inv_map(rmap, n)
        out = self._empty(n_f, torch.float64)
        ws = self._ws(self.lib.grf_poly_grad_workspace_bytes(n, S))
        Gt = op.Gt
        C.check(self.lib.grf_poly_grad_f64(n, _p(Gt.ptr), _p(Gt.idx), _p(Gt.val), _p(ft), n_f, n_sel, _p(inv), _p(A),
                                           _p(B), A.stride(0), _p(wt), S, _p(out), _p(ws), ws.numel(), self.stream),
                "grf_poly_grad_f64")
        return out

    # ------------------------------------- K blocks, diagonals and their gradients from the operator
    def _nodes(self, x, n: int) -> torch.Tensor:
        """The node indices of a kernel argument as int32 on the device (None: all n nodes)."""
        if x is None:
            return torch.arange(n, dtype=torch.int32, device=self.device)
        return self._row_map(x)

    def _poly_memory_guard(self, what: str, n1: int, n2: int, nbytes: int) -> None:
        """ValueError before allocating when ``nbytes`` does not fit in free device memory (a driver query:
        no device data is read and the stream is not waited for)."""
        free = torch.cuda.mem_get_info(self.device)[0]
        if nbytes > free:
            raise ValueError(f"{what}: the {n1} x {n2} block and its workspace need {int(nbytes)} bytes, more than "
                             f"the {int(free)} bytes of free device memory")

    def poly_kernel_block(self, op: WalkPolynomial, f, x1=None, x2=None) -> torch.Tensor:
        """K[x1, x2] = S_1 p(G) p(G)^T S_2^T (fp64, len(x1) x len(x2); None: all nodes; indices may repeat) in
        column blocks of 256 unit columns (grf_poly_kernel_block_f64).  Every column is bit-identical to
        ``poly_gram_matvec`` on its unit vector."""
        ft, n_f = self._poly_f(op, f)
        n = op.shape[0]
        r1, r2 = self._nodes(x1, n), self._nodes(x2, n)
        n1, n2 = r1.numel(), r2.numel()
        need = self.lib.grf_poly_kernel_block_workspace_bytes(n, n_f, n2)
        self._poly_memory_guard("poly_kernel_block", n1, n2, n1 * n2 * 8 + need)
        K = torch.empty((n1, n2), dtype=torch.float64, device=self.device)
        ws = self._ws(need)
        G, Gt = op.G, op.Gt
        C.check(self.lib.grf_poly_kernel_block_f64(n, _p(G.ptr), _p(G.idx), _p(G.val), _p(Gt.ptr), _p(Gt.idx),
                                                   _p(Gt.val), _p(ft), n_f, _p(r1), n1, _p(r2), n2, _p(K),
                                                   max(n2, 1), _p(ws), ws.numel(), self.stream),
                "grf_poly_kernel_block_f64")
        return K

    def poly_kernel_diag(self, op: WalkPolynomial, f, x=None) -> torch.Tensor:
        """diag K[x] (fp64, len(x); None: all nodes) from the first chain alone (grf_poly_kernel_diag_f64)."""
        ft, n_f = self._poly_f(op, f)
        n = op.shape[0]
        r = self._nodes(x, n)
        n_x = r.numel()
        need = self.lib.grf_poly_kernel_diag_workspace_bytes(n, n_f, n_x)
        self._poly_memory_guard("poly_kernel_diag", n_x, 1, n_x * 8 + need)
        out = self._empty(n_x, torch.float64)
        ws = self._ws(need)
        Gt = op.Gt
        C.check(self.lib.grf_poly_kernel_diag_f64(n, _p(Gt.ptr), _p(Gt.idx), _p(Gt.val), _p(ft), n_f, _p(r), n_x,
                                                  _p(out), _p(ws), ws.numel(), self.stream),
                "grf_poly_kernel_diag_f64")
        return out

    def _merged_axis(self, r: torch.Tensor, n: int, g: torch.Tensor, dim: int):
        """(inv, g'): inv[node] = one position of the node in r (or -1), and g with the slices of a node's repeated
        positions along ``dim`` added into that one and the others zero.  No host read."""
        pos = torch.arange(r.numel(), dtype=torch.int32, device=self.device)
        inv = torch.full((n,), -1, dtype=torch.int32, device=self.device)
        inv[r.long()] = pos
        return inv, torch.zeros_like(g).index_add_(dim, inv[r.long()].long(), g)

    def poly_kernel_grad(self, op: WalkPolynomial, f, g: torch.Tensor, x1=None, x2=None,
                         diag: bool = False) -> torch.Tensor:
        """d<g, K[x1, x2]>/df_l (g: len(x1) x len(x2)) or, ``diag``, d<g, diag K[x1]>/df_l (g: len(x1)):
        (n_f,) fp64 on the device (grf_poly_kernel_grad_f64).  Repeated indices are allowed."""
        ft, n_f = self._poly_f(op, f)
        n = op.shape[0]
        r1 = self._nodes(x1, n)
        n1 = r1.numel()
        g = g.detach().to(self.device, torch.float64)
        Gt = op.Gt
        out = self._empty(n_f, torch.float64)
        if diag:
            g = g.flatten().contiguous()
            if g.numel() != n1:
                raise ValueError(f"poly_kernel_grad: g must hold one entry per node of x ({n1})")
            need = self.lib.grf_poly_kernel_grad_workspace_bytes(n, n1, n1, 1)
            self._poly_memory_guard("poly_kernel_grad", n1, 1, need)
            ws = self._ws(need)
            C.check(self.lib.grf_poly_kernel_grad_f64(n, _p(Gt.ptr), _p(Gt.idx), _p(Gt.val), _p(ft), n_f, _p(r1), n1,
                                                      None, None, n1, None, _p(g), 1, 1, _p(out), _p(ws), ws.numel(),
                                                      self.stream), "grf_poly_kernel_grad_f64")
            return out
        r2 = self._nodes(x2, n)
        n2 = r2.numel()
        if g.dim() != 2 or tuple(g.shape) != (n1, n2):
            raise ValueError(f"poly_kernel_grad: g must be ({n1} x {n2})")
        need = self.lib.grf_poly_kernel_grad_workspace_bytes(n, n1, n2, 0)
        self._poly_memory_guard("poly_kernel_grad", n1, n2, 2 * n1 * n2 * 8 + need)
        inv1, g = self._merged_axis(r1, n, g, 0)
        inv2, g = self._merged_axis(r2, n, g, 1)
        g = g.contiguous()
        ws = self._ws(need)
        C.check(self.lib.grf_poly_kernel_grad_f64(n, _p(Gt.ptr), _p(Gt.idx), _p(Gt.val), _p(ft), n_f, _p(r1), n1,
                                                  _p(inv1), _p(r2), n2, _p(inv2), _p(g), max(n2, 1), 0, _p(out),
                                                  _p(ws), ws.numel(), self.stream), "grf_poly_kernel_grad_f64")
        return out

    # ------------------------------------- the exact diffusion kernel exp(-beta L) on the fp64 matrix cores
    def _dense_f64(self, M: torch.Tensor, what: str) -> torch.Tensor:
        """A 2-D fp64 device matrix whose rows are contiguous (any row pitch), copied only if it is not one."""
        if not torch.is_tensor(M) or M.dim() != 2:
            raise ValueError(f"{what} must be a 2-D tensor")
        if M.dtype != torch.float64 or M.device != self.device:
            M = M.to(self.device, torch.float64)
        if M.shape[1] > 1 and M.stride(1) != 1 or (M.shape[0] > 1 and M.stride(0) < M.shape[1]):
            M = M.contiguous()
        return M

    @staticmethod
    def _pitch(M: torch.Tensor) -> int:
        return int(M.stride(0)) if M.shape[0] > 1 else max(int(M.shape[1]), 1)

    def _checked_rows(self, r, n_rows: int, what: str) -> Optional[torch.Tensor]:
        """An int32 row map on the device, its entries checked against the operand's rows (one host read)."""
        if r is None:
            return None
        r = self._row_map(r)
        if r.numel() and not bool(((r >= 0) & (r < n_rows)).all()):
            raise ValueError(f"{what}: row indices must lie in [0, {n_rows})")
        return r

    def _dense_memory_guard(self, what: str, n: int, nbytes: int) -> None:
        free = torch.cuda.mem_get_info(self.device)[0]
        if nbytes > free:
            raise ValueError(f"{what}: n = {n} needs {int(nbytes)} bytes for its result and workspace, more than the "
                             f"{int(free)} bytes of free device memory")

    def gemm_nt_f64(self, A: Optional[torch.Tensor], B: Optional[torch.Tensor], *, alpha: float = 1.0, ra=None,
                    rb=None, gamma: float = 1.0, Z: Optional[torch.Tensor] = None, delta: float = 0.0,
                    out: Optional[torch.Tensor] = None, symmetric: bool = False,
                    W: Optional[torch.Tensor] = None) -> torch.Tensor:
        """C = alpha A[ra] B[rb]^T + gamma Z + delta I in fp64 on the matrix cores (grf_gemm_nt_f64): A (rows x nk)
        and B (rows x nk) are read by rows through the optional row maps; ``out`` (n1 x n2, may be ``Z``) receives
        C and is returned.  ``symmetric``: the caller promises a symmetric result; the upper tiles are computed
        and mirrored, so C is bitwise symmetric.  ``W`` (n1 x n2): nothing is written and sum_ij W_ij C_ij comes
        back as a one-element fp64 device tensor.  A = B = None: C = gamma Z + delta I."""
        if (A is None) != (B is None):
            raise ValueError("gemm_nt_f64: A and B go together")
        if A is not None:
            A, B = self._dense_f64(A, "gemm_nt_f64: A"), self._dense_f64(B, "gemm_nt_f64: B")
            if A.shape[1] != B.shape[1]:
                raise ValueError(f"gemm_nt_f64: A has {A.shape[1]} columns, B {B.shape[1]}")
            nk = int(A.shape[1])
            ra = self._checked_rows(ra, A.shape[0], "gemm_nt_f64: ra")
            rb = self._checked_rows(rb, B.shape[0], "gemm_nt_f64: rb")
            n1 = int(A.shape[0]) if ra is None else ra.numel()
            n2 = int(B.shape[0]) if rb is None else rb.numel()
        else:
            ref = Z if Z is not None else (out if out is not None else W)
            if ref is None or ra is not None or rb is not None:
                raise ValueError("gemm_nt_f64: without operands the shape comes from Z, out or W (and no row maps)")
            nk, (n1, n2) = 0, (int(ref.shape[0]), int(ref.shape[1]))
        for name, M in (("Z", Z), ("out", out), ("W", W)):
            if M is not None and (M.dim() != 2 or tuple(M.shape) != (n1, n2)):
                raise ValueError(f"gemm_nt_f64: {name} must be ({n1} x {n2})")
        if Z is not None:
            Z = Z if Z is out else self._dense_f64(Z, "gemm_nt_f64: Z")
        contract = W is not None
        need = self.lib.grf_gemm_nt_f64_workspace_bytes(n1, n2) if contract else 0
        if contract:
            W = self._dense_f64(W, "gemm_nt_f64: W")
            self._dense_memory_guard("gemm_nt_f64", max(n1, n2), need)
            res = torch.zeros(1, dtype=torch.float64, device=self.device)
        else:
            if out is None:
                self._dense_memory_guard("gemm_nt_f64", max(n1, n2), n1 * n2 * 8)
                out = torch.empty((n1, n2), dtype=torch.float64, device=self.device)
            elif out.dtype != torch.float64 or out.device != self.device or (n2 > 1 and out.stride(1) != 1):
                raise ValueError("gemm_nt_f64: out must be an fp64 tensor on this device with contiguous rows")
            res = out
        ws = self._ws(need) if contract else None
        C.check(self.lib.grf_gemm_nt_f64(
            n1, n2, nk, float(alpha), _p(A), self._pitch(A) if nk else 0, int(A.shape[0]) if nk else 0, _p(ra),
            _p(B), self._pitch(B) if nk else 0, int(B.shape[0]) if nk else 0, _p(rb), float(gamma), _p(Z),
            self._pitch(Z) if Z is not None else 0, float(delta), None if contract else _p(out),
            0 if contract else self._pitch(out), int(bool(symmetric)), _p(W), self._pitch(W) if contract else 0,
            _p(res) if contract else None, _p(ws), ws.numel() if contract else 0, self.stream), "grf_gemm_nt_f64")
        return res

    def expm_squarings(self, rho: float) -> int:
        """s = max(0, ceil(log2 rho)) of grf_expm_sym_f64 (its product count is 17 + s)."""
        return int(self.lib.grf_expm_squarings(float(rho)))

    def diffusion_expm(self, L_dev: torch.Tensor, beta: float, rho: float) -> torch.Tensor:
        """E = exp(-beta L) (fp64, n x n, bitwise symmetric) of a dense symmetric ``L_dev`` on the device by scaling
        and squaring (grf_expm_sym_f64); ``rho`` bounds the spectral radius of beta L.  No host read."""
        L_dev = self._dense_f64(L_dev, "diffusion_expm: L")
        n = int(L_dev.shape[0])
        if L_dev.shape[1] != n or n < 1:
            raise ValueError("diffusion_expm: L must be square and non-empty")
        need = self.lib.grf_expm_sym_f64_workspace_bytes(n)
        self._dense_memory_guard("diffusion_expm", n, n * n * 8 + need)
        E = torch.empty((n, n), dtype=torch.float64, device=self.device)
        ws = self._ws(need)
        C.check(self.lib.grf_expm_sym_f64(n, _p(L_dev), self._pitch(L_dev), float(beta), float(rho), _p(E), n, _p(ws),
                                          ws.numel(), self.stream), "grf_expm_sym_f64")
        return E

    # ------------------------------------- dense exact GPR: the fp64 Cholesky factorisation and triangular solves
    def _cached_ws(self, name: str, need: int) -> torch.Tensor:
        """The call family's workspace, kept between calls and grown on demand (calls on this engine's stream are
        ordered, and every call rewrites what it reads)."""
        cache = self.__dict__.setdefault("_dense_solve_ws", {})
        ws = cache.get(name)
        if ws is None or ws.numel() < need:
            ws = cache[name] = self._ws(need)
        return ws

    def cholesky(self, A: torch.Tensor):
        """(F, logdet, info) of grf_potrf_f64 for a symmetric positive-definite ``A`` (n x n; only its lower triangle
        and diagonal are read): F (n x n fp64) holds L below and L^T mirrored above, ``logdet`` (one fp64) is
        2 sum log L_ii, ``info`` (one int32) is 0 or the 1-based index of the first pivot that is not positive and
        finite (then logdet is NaN).  All three stay on the device: no host read."""
        A = self._dense_f64(A, "cholesky: A")
        n = int(A.shape[0])
        if A.shape[1] != n or n < 1:
            raise ValueError("cholesky: A must be square and non-empty")
        need = int(self.lib.grf_potrf_f64_workspace_bytes(n))
        ws = self._cached_ws("potrf", need)
        self._dense_memory_guard("cholesky", n, n * n * 8)
        F = torch.empty((n, n), dtype=torch.float64, device=self.device)
        logdet = torch.empty(1, dtype=torch.float64, device=self.device)
        info = torch.empty(1, dtype=torch.int32, device=self.device)
        C.check(self.lib.grf_potrf_f64(n, _p(A), self._pitch(A), _p(F), n, _p(logdet), _p(info), _p(ws), ws.numel(),
                                       self.stream), "grf_potrf_f64")
        return F, logdet, info

    def cholesky_solve(self, F: torch.Tensor, B: torch.Tensor, transposed: Optional[bool] = None,
                       inplace: bool = False) -> torch.Tensor:
        """Triangular solves with the factor of ``cholesky`` (grf_trsm_f64).  ``B`` is nrhs x n, ONE RIGHT-HAND SIDE
        PER ROW.  ``transposed=False``: L x = b; ``True``: L^T x = b; ``None`` (default): both, x = (L L^T)^-1 b.
        Returns the solutions in B's layout (a new tensor unless ``inplace`` and B is already an fp64 matrix on the
        device with contiguous rows)."""
        F = self._dense_f64(F, "cholesky_solve: F")
        n = int(F.shape[0])
        if F.shape[1] != n:
            raise ValueError("cholesky_solve: F must be square")
        Bd = self._dense_f64(B, "cholesky_solve: B")
        if Bd.shape[1] != n:
            raise ValueError(f"cholesky_solve: B must be (nrhs x {n}), one right-hand side per row")
        if Bd is B and not inplace:
            Bd = B.clone(memory_format=torch.contiguous_format)
        nrhs = int(Bd.shape[0])
        if n == 0 or nrhs == 0:
            return Bd
        need = int(self.lib.grf_trsm_f64_workspace_bytes(n, nrhs))
        ws = self._cached_ws("trsm", need)
        for t in ((0, 1) if transposed is None else (int(bool(transposed)),)):
            C.check(self.lib.grf_trsm_f64(n, nrhs, _p(F), self._pitch(F), t, _p(Bd), self._pitch(Bd), _p(ws),
                                          ws.numel(), self.stream), "grf_trsm_f64")
        return Bd

    # ------------------------------------- SVGP classification (include/grf_svgp.h): the RobustMax quadrature
    GH_POINTS = 20  # gpflow.likelihoods.MultiClass's num_gauss_hermite_points

    def _gauss_hermite(self):
        """numpy's hermgauss(20) nodes and weights on the device (what GPflow calls), uploaded once per engine."""
        gh = self.__dict__.get("_gh")
        if gh is None:
            x, w = np.polynomial.hermite.hermgauss(self.GH_POINTS)
            gh = self.__dict__["_gh"] = (torch.from_numpy(x).to(self.device), torch.from_numpy(w).to(self.device))
        return gh

    def _latents(self, mu: torch.Tensor, var: torch.Tensor, what: str):
        mu, var = self._dense_f64(mu, f"{what}: mu"), self._dense_f64(var, f"{what}: var")
        if mu.shape != var.shape:
            raise ValueError(f"{what}: mu and var must have one shape (n x P)")
        return mu, var, int(mu.shape[0]), int(mu.shape[1])

    def robustmax_ve(self, mu: torch.Tensor, var: torch.Tensor, y: torch.Tensor, with_grad: bool = True,
                     epsilon: float = 1e-3):
        """MultiClass(RobustMax)'s variational expectations (grf_robustmax_ve_f64): ``mu`` and ``var`` n x P fp64,
        ``y`` n int32 labels on the device.  Returns (ve (n,), d ve/d mu, d ve/d var) -- the gradients (n x P) are
        None without ``with_grad``.  A label outside [0, P) gives a NaN row.  No host read."""
        mu, var, n, P = self._latents(mu, var, "robustmax_ve")
        if y.dtype != torch.int32 or y.device != self.device or y.dim() != 1 or y.numel() != n or not y.is_contiguous():
            raise ValueError("robustmax_ve: y must be a contiguous int32 vector of n labels on this device")
        gx, gw = self._gauss_hermite()
        ve = torch.empty(n, dtype=torch.float64, device=self.device)
        dmu = torch.empty((n, P), dtype=torch.float64, device=self.device) if with_grad else None
        dvar = torch.empty((n, P), dtype=torch.float64, device=self.device) if with_grad else None
        C.check(self.lib.grf_robustmax_ve_f64(n, P, _p(mu), self._pitch(mu), _p(var), self._pitch(var), _p(y), _p(gx),
                                              _p(gw), gx.numel(), float(epsilon), _p(ve), _p(dmu), P, _p(dvar), P,
                                              self.stream), "grf_robustmax_ve_f64")
        return ve, dmu, dvar

    def robustmax_predict(self, mu: torch.Tensor, var: torch.Tensor, epsilon: float = 1e-3) -> torch.Tensor:
        """The predictive class probabilities ps (n x P) of MultiClass._predict_mean_and_var
        (grf_robustmax_predict_f64)."""
        mu, var, n, P = self._latents(mu, var, "robustmax_predict")
        gx, gw = self._gauss_hermite()
        ps = torch.empty((n, P), dtype=torch.float64, device=self.device)
        C.check(self.lib.grf_robustmax_predict_f64(n, P, _p(mu), self._pitch(mu), _p(var), self._pitch(var), _p(gx),
                                                   _p(gw), gx.numel(), float(epsilon), _p(ps), P, self.stream),
                "grf_robustmax_predict_f64")
        return ps

    def rows_sqsum(self, T: torch.Tensor, groups: int, base: Optional[torch.Tensor] = None) -> torch.Tensor:
        """out[r, g] = base[r] + sum_j T[r, g len + j]^2 for the ``groups`` equal column groups of T (n x groups len)
        in a fixed order (grf_rows_sqsum_f64); ``base``: n fp64 values or None."""
        T = self._dense_f64(T, "rows_sqsum: T")
        n, width, groups = int(T.shape[0]), int(T.shape[1]), int(groups)
        if groups < 1 or width % groups:
            raise ValueError(f"rows_sqsum: T's {width} columns do not split into {groups} equal groups")
        if base is not None:
            base = base.to(self.device, torch.float64).contiguous()
            if base.dim() != 1 or base.numel() != n:
                raise ValueError("rows_sqsum: base must hold one value per row of T")
        out = torch.empty((n, groups), dtype=torch.float64, device=self.device)
        C.check(self.lib.grf_rows_sqsum_f64(n, groups, width // groups, _p(T), self._pitch(T), _p(base), _p(out),
                                            groups, self.stream), "grf_rows_sqsum_f64")
        return out

    def laplacian_dense_matrix(self, W, mode: int) -> torch.Tensor:
        """The Laplacian of grf_laplacian_dense as a dense fp64 n x n device matrix."""
        G = self.walk_matrix_dense(W, mode)
        n, nnz = G.n_rows, G.nnz
        L = torch.zeros((n, n), dtype=torch.float64, device=self.device)
        r = torch.repeat_interleave(torch.arange(n, device=self.device), G.ptr[1:] - G.ptr[:-1], output_size=nnz)
        L[r, G.idx[:nnz].long()] = G.val[:nnz]
        return L

    @staticmethod
    def slq_logdet(coef: np.ndarray, iters: int, sq_norms: np.ndarray) -> float:
        """Stochastic Lanczos quadrature from CG coefficients: coef (2 max_iter x t) holds the probe columns'
        alpha rows then beta rows (cg_solve(return_lanczos=True)), sq_norms their ||z_i||^2.  Column c's
        tridiagonal covers its first m_c iterations (up to its first zero alpha, or all that ran):
        T[k,k] = 1/alpha_k + beta_{k-1}/alpha_{k-1}, T[k,k+1] = sqrt(beta_k)/alpha_k, and
        log det ~ (1/t) sum_i ||z_i||^2 sum_j V_i[0,j]^2 log lambda_ij.  Host fp64: t small eigenproblems."""
        max_iter, t = coef.shape[0] // 2, coef.shape[1]
        total = 0.0
        for c in range(t):
            a, b = coef[:iters, c], coef[max_iter:max_iter + iters, c]
            zero = np.flatnonzero(a == 0.0)
            m = int(zero[0]) if zero.size else int(iters)
            if m == 0:
                continue
            T = np.zeros((m, m))
            d = 1.0 / a[:m]
            d[1:] += b[:m - 1] / a[:m - 1]
            T[np.arange(m), np.arange(m)] = d
            off = np.sqrt(b[:m - 1]) / a[:m - 1]
            T[np.arange(m - 1), np.arange(1, m)] = off
            T[np.arange(1, m), np.arange(m - 1)] = off
            lam, V = np.linalg.eigh(T)
            total += float(sq_norms[c]) * float(np.sum(V[0] ** 2 * np.log(lam)))
        return total / t

    def marginal_log_likelihood(self, steps, f: torch.Tensor, train_idx, y: torch.Tensor, noise: float,
                                probes: torch.Tensor, tolerance: float = 1.0, max_iter: int = 1000,
                                preconditioner=None):
        """MLL(f, s2) = -1/2 y^T K^-1 y - 1/2 log det K^ - n/2 log 2 pi with K^ = Phi_T Phi_T^T + s2 I,
        Phi = sum_l f_l M_l, and its gradient, K never formed (fp64): one CG solve of [y | Z] for the
        probes Z (n_train x t, t <= 255), log det by stochastic Lanczos quadrature from the solve's own
        coefficients, the gradients by gpytorch's estimators
            1/2 a^T dK a - 1/(2t) sum_i u_i^T dK z_i,   a = K^-1 y, u_i = K^-1 z_i.
        ``steps``: a features.StepMatrices, or a WalkPolynomial (Phi = p(G), the exact kernel: the same
        estimator on cg_solve_poly and poly_grad, neither Phi nor a power of G formed).
        ``preconditioner="jacobi"``: the solve is preconditioned by D = diag(K^) (gram_jacobi; for a
        WalkPolynomial poly_jacobi, which costs n_train / 256 operator chains).  ``probes`` stay the caller's
        standard-normal g_i: the solve's columns are [y | D^1/2 g_i], whose preconditioned coefficients are the
        Lanczos coefficients of D^-1/2 K^ D^-1/2 started at g_i / ||g_i||, so
            log det K^ ~ sum_r log d_r + slq_logdet(coef, iters, ||g_i||^2),
        and with z_i = D^1/2 g_i (covariance D), u_i = K^-1 z_i, tr(K^-1 dK) ~ (1/t) sum_i u_i^T dK (D^-1 z_i):
        the gradient's probe columns become D^-1/2 g_i.  D is held constant (unbiased for any fixed D > 0).
        The noise gradient's a.a comes from one more one-column solve (see _mll_jacobi); the iteration count
        returned is the main solve's.
        Returns (value (float), d/df ((min(len(f), L),) fp64 device tensor), d/ds2 (float), CG iterations)."""
        tr = self._row_map(train_idx)
        n = tr.numel()
        yv = y.detach().to(self.device, torch.float64).flatten()
        if probes.dim() != 2 or probes.shape[0] != n or yv.numel() != n:
            raise ValueError("marginal_log_likelihood: probes must be (n_train x t) and y (n_train,)")
        t = probes.shape[1]
        if not 1 <= t <= 255:
            raise ValueError("marginal_log_likelihood: between 1 and 255 probes per call")
        jacobi = preconditioner_name(preconditioner, "marginal_log_likelihood")
        G = probes.detach().to(self.device, torch.float64)
        op = kernel_operator(self, steps, f, tr, noise, "marginal_log_likelihood")
        if jacobi:
            return self._mll_jacobi(op, yv, G, tolerance, max_iter)
        rhs = torch.cat([yv[:, None], G], dim=1).contiguous()
        X, iters, coef = op.solve(rhs, tolerance, max_iter, return_lanczos=True)
        # the weighted column sums both scalars need, one host read with the coefficients' probe columns
        wt = torch.full((1 + t,), -0.5 / t, dtype=torch.float64, device=self.device)
        wt[0] = 0.5
        cols = torch.stack([(rhs * X).sum(0), (X * X).sum(0), (rhs * rhs).sum(0)]).cpu().numpy()
        lanczos = coef[:, 1:].cpu().numpy()
        # d/df_l: dK = M_l[T] Phi_T^T + Phi_T M_l[T]^T; the y column pairs a with itself
        Bm = rhs
        Bm[:, 0] = X[:, 0]
        # d/ds2: dK = I -> 1/2 a.a - 1/(2t) sum_i u_i.z_i (row 0 of cols)
        return self._mll_tail(op, X, Bm, wt, cols, lanczos, iters, 0.0, 0)

    def _mll_tail(self, op, X, Bm, wt, cols, lanczos, iters, logdet_d, trace_row):
        """The end of both routes of marginal_log_likelihood.  cols (3 x (1 + t), host): [0, 0] y.a, [1, 0] a.a,
        [trace_row, 1:] the probes' terms of tr(K^-1), [2, 1:] their squared norms; logdet_d: the route's log det D."""
        n, t = X.shape[0], X.shape[1] - 1
        logdet = logdet_d + self.slq_logdet(lanczos, iters, cols[2, 1:])
        value = -0.5 * cols[0, 0] - 0.5 * logdet - 0.5 * n * float(np.log(2.0 * np.pi))
        g_noise = 0.5 * cols[1, 0] - 0.5 / t * float(cols[trace_row, 1:].sum())
        return float(value), op.modulator_grad(X, Bm, wt), float(g_noise), iters

    def _mll_jacobi(self, op, yv, G, tolerance, max_iter):
        """marginal_log_likelihood's Jacobi route (see there) on the kernel operator ``op``."""
        t = G.shape[1]
        dinv = op.jacobi()
        sq = torch.sqrt(dinv)[:, None]                                         # D^-1/2
        rhs = torch.cat([yv[:, None], G / sq], dim=1).contiguous()             # [y | D^1/2 g_i]
        X, iters, coef = op.solve(rhs, tolerance, max_iter, precond=dinv, return_lanczos=True)
        Bm = torch.cat([X[:, :1], G * sq], dim=1).contiguous()                 # [a | D^-1 z_i = D^-1/2 g_i]
        wt = torch.full((1 + t,), -0.5 / t, dtype=torch.float64, device=self.device)
        wt[0] = 0.5
        # a.a for the noise gradient: a_k.a_k is of second order in the iterate's error under plain CG (K^-1 a_k
        # stays in the Krylov space up to a multiple of a) but of first order under a preconditioner, so it is taken
        # as a_k.a_k + 2 w.r_k with r_k = y - K^ a_k and w ~ K^-1 a_k from one more one-column solve:
        # y^T K^-1 a_k = a_k.a_k + w.r_k and a_k.(a - a_k) = w.r_k, each up to a product of two solve errors
        a = X[:, :1].contiguous()
        r = yv[:, None] - op.matvec(a)
        w, _ = op.solve(a, tolerance, max_iter, precond=dinv)
        quad = (Bm * X).sum(0)
        quad[0] = quad[0] + 2.0 * (w * r).sum()
        cols = torch.stack([(rhs * X).sum(0), quad, torch.cat([dinv.log().sum()[None], (G * G).sum(0)])])
        cols = cols.cpu().numpy()
        # log det K^ = -sum log dinv + the quadrature of D^-1/2 K^ D^-1/2; the trace terms are quad's (row 1)
        return self._mll_tail(op, X, Bm, wt, cols, coef[:, 1:].cpu().numpy(), iters, -cols[2, 0], 1)

    def pathwise_predict(self, phi: DeviceCSR, train_idx, test_idx, y_train: torch.Tensor, noise: float,
                         eps1: torch.Tensor, eps2: torch.Tensor, tolerance: float = 1.0, max_iter: int = 1000,
                         dtype: torch.dtype = torch.float64, f=None, preconditioner=None):
        """SparseGraphGP.predict (models/sparse_grf_model.py:21-45) given its random draws.

        phi: Phi as a DeviceCSR, or a WalkPolynomial with its modulator ``f`` (fp64 only): f_train and
        f_test then come from one chain p(G) E, the solve from cg_solve_poly, and K_test,train V from
        S_test p(G) p(G)^T S_train^T V.

        eps1: (S x n_nodes) prior weights, eps2: (S x n_train) noise draws (already scaled by
        the noise std).  dtype: float64 (default) or the reference's float32 for every dense
        block and the CG recurrence.  ``preconditioner="jacobi"`` (float64 only) preconditions the solve
        by diag(K^).  Returns (S x n_test) posterior samples (dtype) and the CG iteration count."""
        tr = self._row_map(train_idx)
        te = self._row_map(test_idx)
        jacobi = preconditioner_name(preconditioner, "pathwise_predict")
        if jacobi and dtype != torch.float64:
            raise ValueError("pathwise_predict: a preconditioned solve runs in float64 only")
        op = kernel_operator(self, phi, f, tr, noise, "pathwise_predict", dtype)
        E = eps1.to(self.device, dtype).t().contiguous()                      # n_nodes x S
        f_train = op.prior_draw(E, tr)                                         # (eps1 @ phi_train.T)^T
        f_test = op.prior_draw(E, te)
        y = y_train.to(self.device, dtype).flatten()
        B = y[:, None] - (f_train + eps2.to(self.device, dtype).t())          # b_batch^T
        V, iters = op.solve(B.contiguous(), tolerance, max_iter, precond=op.jacobi() if jacobi else None)
        out = f_test + op.cross(te, V)                                         # + K_test_train v
        return out.t(), iters

    # ------------------------------------- the exact posterior mean and variance (predict_f)
    POSTERIOR_CHUNK = 256  # test nodes per batched solve: the solvers' column limit

    def posterior_rhs(self, phi: DeviceCSR, nodes, E: Optional[torch.Tensor] = None,
                      prior: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(E, prior) of <= 256 node indices (repeats allowed): E = Phi[nodes]^T as a dense (n_cols x S) fp64
        block -- ``E`` may be a column window of a wider buffer, whose other columns stay untouched -- and
        prior[c] = sum_k Phi[nodes[c], k]^2 = K[x_c, x_c] (grf_posterior_rhs_f64)."""
        r = self._row_map(nodes)
        S = r.numel()
        if E is None:
            E = torch.empty((phi.n_cols, S), dtype=torch.float64, device=self.device)
        if prior is None:
            prior = self._empty(S, torch.float64)
        if E.dtype != torch.float64 or E.dim() != 2 or tuple(E.shape) != (phi.n_cols, S) or \
                (S > 1 and E.stride(1) != 1) or prior.dtype != torch.float64 or prior.numel() != S \
                or not prior.is_contiguous():
            raise ValueError("posterior_rhs: E must be a float64 (n_cols x S) row-major block and prior hold S values")
        C.check(self.lib.grf_posterior_rhs_f64(phi.n_rows, _p(phi.ptr), _p(phi.idx), _p(phi.val32), phi.n_cols, _p(r),
                                               S, _p(E), self._pitch(E), _p(prior), self.stream),
                "grf_posterior_rhs_f64")
        return E, prior

    def posterior_reduce(self, B: torch.Tensor, X: torch.Tensor, prior: torch.Tensor,
                         alpha: Optional[torch.Tensor] = None, add_noise: float = 0.0,
                         var: Optional[torch.Tensor] = None, mean: Optional[torch.Tensor] = None):
        """var[c] = prior[c] - sum_r B[r,c] X[r,c] (+ add_noise) and, with ``alpha`` (n,), mean[c] =
        sum_r B[r,c] alpha[r], in one deterministic pass over the (n x S) fp64 blocks B and X, S <= 256
        (grf_posterior_reduce_f64).  Returns (var, mean); mean is None without alpha."""
        if B.dim() != 2 or X.shape != B.shape:
            raise ValueError("posterior_reduce: B and X must be (n x S) blocks of one shape")
        n, S = int(B.shape[0]), int(B.shape[1])
        self._check_block(B, n, "posterior_reduce: B")
        self._check_block(X, n, "posterior_reduce: X")
        if prior.dtype != torch.float64 or prior.numel() != S or not prior.is_contiguous():
            raise ValueError("posterior_reduce: prior must hold one float64 per column")
        if alpha is not None:
            alpha = alpha.to(self.device, torch.float64).flatten().contiguous()
            if alpha.numel() != n:
                raise ValueError("posterior_reduce: alpha must hold one value per row")
            if mean is None:
                mean = self._empty(S, torch.float64)
        if var is None:
            var = self._empty(S, torch.float64)
        ws = self._ws(self.lib.grf_posterior_reduce_workspace_bytes(n, S))
        C.check(self.lib.grf_posterior_reduce_f64(n, S, _p(B), self._pitch(B), _p(X), self._pitch(X), _p(alpha),
                                                  _p(prior), float(add_noise), _p(var),
                                                  _p(mean) if alpha is not None else None, _p(ws), ws.numel(),
                                                  self.stream), "grf_posterior_reduce_f64")
        return var, (mean if alpha is not None else None)

    def posterior_moments(self, phi, train_idx, test_idx, y_train: torch.Tensor, noise: float, *, f=None,
                          full_cov: bool = False, tolerance: float = 1e-2, max_iter: int = 1000,
                          info: Optional[dict] = None, add_noise: bool = False, preconditioner=None):
        """The exact posterior mean and variance of the GP at ``test_idx`` (what the reference's dense baseline
        calls predict_f, run_scaling_experiment.py:729), K never formed: with K^ = K[T,T] + noise I,
        alpha = K^-1 y and b_c = K[T, x_c],
            mean_c = b_c^T alpha,   var_c = K[x_c, x_c] - b_c^T K^-1 b_c,   cov = K[x,x] - B^T K^-1 B.
        Returns (mean, var), fp64 device tensors of shape (n*,), or with ``full_cov`` (mean, cov), cov
        (n* x n*) and exactly symmetric.  ``add_noise`` adds ``noise`` to the variances / the covariance's
        diagonal (predict_y).  The test nodes (repeats and training nodes allowed) go in chunks of 256 columns,
        one batched CG solve each; ``tolerance`` defaults to gpytorch's eval_cg_tolerance.  Variances are
        returned as computed: from its zero start CG's b^T x_k rises monotonically to b^T K^-1 b, so a solve
        stopped early over-estimates a variance and never under-estimates it, up to rounding.  So that this
        also holds once CG has lost orthogonality, the quadratic form is taken as x^T (2 b - K^ x) =
        b^T K^-1 b - ||x - x_k||^2_K (one more operator product per chunk); the mean is B^T alpha, and with
        ``full_cov`` the off-diagonal entries are K[x,x] - B^T X symmetrised, the diagonal the variances.

        phi: Phi as a DeviceCSR (rhs -> spmm -> cg_solve -> reduce per chunk), or a WalkPolynomial with its
        modulator ``f`` (poly_kernel_block / poly_kernel_diag / cg_solve_poly, then the same reduce kernel).
        ``info`` receives ``cg_iterations`` (a list, one count per chunk) and ``alpha_iterations``.
        ``preconditioner="jacobi"``: 1 / diag(K^) is built once and preconditions every solve (alpha and each
        chunk); the energy form bounds b^T K^-1 b from below for any x, so the statement on the variances holds
        for the preconditioned iterates unchanged."""
        jacobi = preconditioner_name(preconditioner, "posterior_moments")
        tr, te = self._row_map(train_idx), self._row_map(test_idx)
        op = kernel_operator(self, phi, f, tr, noise, "posterior_moments")
        n, ns = tr.numel(), te.numel()
        y = y_train.detach().to(self.device, torch.float64).flatten()
        if y.numel() != n:
            raise ValueError("posterior_moments: y_train must hold one value per training node")
        chunk = self.POSTERIOR_CHUNK
        if full_cov:  # B for every test node, its transpose for the product, the result and its symmetrisation
            self._dense_memory_guard("posterior_moments (full_cov)", max(n, ns),
                                     2 * n * ns * 8 + 2 * ns * ns * 8 + op.scratch_rows * min(chunk, ns) * 8)
        mean = torch.zeros(ns, dtype=torch.float64, device=self.device)
        var = torch.empty(ns, dtype=torch.float64, device=self.device)
        iters, alpha_iters = [], 0
        if info is not None:
            info["cg_iterations"], info["alpha_iterations"] = iters, 0
        if ns == 0:
            return mean, (torch.empty((0, 0), dtype=torch.float64, device=self.device) if full_cov else var)
        alpha, dinv = None, None
        if n:
            dinv = op.jacobi() if jacobi else None
            alpha, alpha_iters = op.solve(y[:, None].contiguous(), tolerance, max_iter, precond=dinv)
            alpha = alpha.flatten()
        if info is not None:
            info["alpha_iterations"] = alpha_iters
        width = min(chunk, ns)
        prior = torch.empty(ns, dtype=torch.float64, device=self.device)
        E_buf = torch.empty((op.scratch_rows, width), dtype=torch.float64, device=self.device)
        B_all = torch.empty((n, ns if full_cov else width), dtype=torch.float64, device=self.device)
        cov = torch.empty((ns, ns), dtype=torch.float64, device=self.device) if full_cov else None
        extra = float(noise) if add_noise else 0.0
        scratch = torch.empty(width, dtype=torch.float64, device=self.device)

        def rhs(c0, c1):
            """B[:, c0:c1] = K[T, chunk] (a window of B_all), prior[c0:c1], and cov[:, c0:c1] = K[x, chunk]."""
            Bv = B_all[:, c0:c1] if full_cov else B_all[:, :c1 - c0]
            op.columns(te[c0:c1], Bv, prior[c0:c1], E_buf, te, cov[:, c0:c1] if full_cov else None)
            return Bv

        def solve(Bv, c0, c1):
            if not n:
                iters.append(0)
                self.posterior_reduce(Bv, Bv, prior[c0:c1], None, extra, var[c0:c1])
                return Bv
            X, it = op.solve(Bv, tolerance, max_iter, precond=dinv)
            iters.append(it)
            # b^T x alone is below b^T K^-1 b only while CG keeps r_k orthogonal to its Krylov space; the
            # energy form 2 b^T x - x^T K^ x = x^T (2 b - K^ x) is below it for any x, so the variance uses that
            KX = op.matvec(X)
            KX.mul_(-1.0).add_(Bv, alpha=2.0)
            self.posterior_reduce(KX, X, prior[c0:c1], None, extra, var[c0:c1])
            self.posterior_reduce(Bv, X, prior[c0:c1], alpha, 0.0, scratch[:c1 - c0], mean[c0:c1])
            return X

        bounds = [(c0, min(c0 + chunk, ns)) for c0 in range(0, ns, chunk)]
        if not full_cov:
            for c0, c1 in bounds:
                solve(rhs(c0, c1), c0, c1)
            return mean, var
        for c0, c1 in bounds:
            rhs(c0, c1)
        if n:
            B_t = B_all.t().contiguous()                                       # (n* x n): read by rows in the product
            for c0, c1 in bounds:
                X = solve(B_all[:, c0:c1], c0, c1)
                Cv = cov[:, c0:c1]
                self.gemm_nt_f64(B_t, X.t().contiguous(), alpha=-1.0, Z=Cv, out=Cv)   # K[x, chunk] - B_all^T X
        else:
            for c0, c1 in bounds:
                solve(B_all[:, c0:c1], c0, c1)
        cov = (cov + cov.t()).mul_(0.5)
        cov.diagonal().copy_(var)                                              # (the energy form, noise included)
        return mean, cov

    # ------------------------------------------------------------- pipelines
    def kernel_matrix(self, A, modulator_vector: Sequence[float], walks_per_node: int, p_halt: float,
                      max_walk_length: int, *, rng: int = C.RNG_PHILOX, seed: int = 42, n_chunks: int = 1,
                      laplacian: bool = True, method: str = "auto", norm: int = C.NORM_MUL_RECIP) -> torch.Tensor:
        """Sparse-path K = Phi Phi^T (fast_grf_kernel_general.py:42-55), float32 on the device."""
        G = self.laplacian(A) if laplacian else self.to_device(A)
        slots = self.walk(G, walks_per_node, p_halt, max_walk_length, rng=rng, seed=seed, n_chunks=n_chunks)
        phi = self.compact(self.features(slots, modulator_vector, norm))
        return self.gram(phi, method)


class PhiOperator:
    """K^ = Phi_T Phi_T^T + noise I, T = ``tr``, for Phi as a DeviceCSR (or the step matrices it is made of, with
    ``f``), as marginal_log_likelihood, pathwise_predict and posterior_moments use it; made once per call.  Phi_T^T
    is transposed once: with the step matrices at once, otherwise before the first Jacobi diagonal or solve."""

    def __init__(self, eng: "GRFEngine", phi, f, tr: torch.Tensor, noise: float):
        self.eng, self.f, self.tr, self.noise, self.steps, self._phi_t = eng, f, tr, noise, None, None
        if isinstance(phi, DeviceCSR):
            self.phi = phi
        else:
            self.steps, self.phi = phi, phi.phi(f)
            self.phi_t()
        self.scratch_rows = self.phi.n_cols   # rows of columns()' scratch block, Phi[nodes]^T

    def phi_t(self) -> DeviceCSR:
        if self._phi_t is None:
            self._phi_t = self.eng.csr_transpose(self.phi, self.tr)
        return self._phi_t

    def jacobi(self) -> torch.Tensor:
        self.phi_t()
        return self.eng.gram_jacobi(self.phi, self.tr, self.noise)

    def solve(self, B, tolerance, max_iter, precond=None, return_lanczos=False):
        return self.eng.cg_solve(self.phi, B, self.noise, self.tr, self.phi_t(), tolerance, max_iter,
                                 return_lanczos=return_lanczos, precond=precond)

    def cross(self, rows, V, noise=0.0):
        """K[rows, T] V (+ noise V)."""
        return self.eng.gram_matvec(self.phi, V, rows=rows, cols=self.tr, phi_t=self.phi_t(), noise=noise)

    def matvec(self, V):
        return self.cross(self.tr, V, self.noise)   # K^ V, the noise term included

    def prior_draw(self, E, rows):
        """(Phi E)[rows]: the rows of the prior sample with the weights E (n_nodes x S)."""
        return self.eng.spmm(self.phi, E, rows)

    def columns(self, nodes, Bv, prior, scratch, test_rows, cov=None):
        """Bv = K[T, nodes], prior = diag K[nodes] and, when given, cov = K[test_rows, nodes], into the caller's
        windows; scratch: its (scratch_rows x >= len(nodes)) block."""
        E = scratch[:, :nodes.numel()]
        self.eng.posterior_rhs(self.phi, nodes, E, prior)
        if self.tr.numel():
            self.eng.spmm(self.phi, E, self.tr, out=Bv)
        if cov is not None:
            self.eng.spmm(self.phi, E, test_rows, out=cov)

    def modulator_grad(self, X, Bm, wt):
        """out[l] = sum_c wt[c] x_c^T (dK/df_l) b_c, dK/df_l = M_l[T] Phi_T^T + Phi_T M_l[T]^T (needs the steps)."""
        WX = self.eng.spmm(self.phi_t(), X)
        WB = self.eng.spmm(self.phi_t(), Bm)
        n_f = min(int(self.f.numel()), self.steps.L)
        return self.eng.steps_frob(self.steps, self.tr, X, WX, Bm, WB, wt, n_steps=n_f)


class WalkOperator:
    """The same methods for the exact kernel K = S p(G) p(G)^T S^T of a WalkPolynomial with its modulator ``f``
    (fp64 only): Horner chains with the walk matrix, neither Phi nor a power of G formed."""
    scratch_rows = 0

    def __init__(self, eng: "GRFEngine", op: WalkPolynomial, f, tr: torch.Tensor, noise: float):
        self.eng, self.op, self.f, self.tr, self.noise, self._draw = eng, op, f, tr, noise, None

    def jacobi(self) -> torch.Tensor:
        return self.eng.poly_jacobi(self.op, self.f, self.tr, self.noise)

    def solve(self, B, tolerance, max_iter, precond=None, return_lanczos=False):
        return self.eng.cg_solve_poly(self.op, self.f, B, self.noise, self.tr, tolerance, max_iter,
                                      return_lanczos=return_lanczos, precond=precond)

    def cross(self, rows, V, noise=0.0):
        return self.eng.poly_gram_matvec(self.op, self.f, V, rows=rows, cols=self.tr, noise=noise)

    def matvec(self, V):
        return self.cross(self.tr, V, self.noise)

    def prior_draw(self, E, rows):
        """(p(G) E)[rows]; one chain per E gives every node's draw, kept for the next rows."""
        if self._draw is None or self._draw[0] is not E:
            self._draw = (E, self.eng.poly_apply(self.op, self.f, E))
        return self._draw[1][rows.long()]

    def columns(self, nodes, Bv, prior, scratch, test_rows, cov=None):
        if self.tr.numel():
            Bv.copy_(self.eng.poly_kernel_block(self.op, self.f, x1=self.tr, x2=nodes))
        prior.copy_(self.eng.poly_kernel_diag(self.op, self.f, x=nodes))
        if cov is not None:
            cov.copy_(self.eng.poly_kernel_block(self.op, self.f, x1=test_rows, x2=nodes))

    def modulator_grad(self, X, Bm, wt):
        return self.eng.poly_grad(self.op, self.f, self.tr, X, Bm, wt)


def kernel_operator(eng: GRFEngine, phi, f, tr: torch.Tensor, noise: float, what: str, dtype=None):
    """The one place that asks "Phi as a CSR, or the walk operator?": a PhiOperator (a DeviceCSR or StepMatrices) or
    a WalkOperator (a WalkPolynomial: needs ``f`` and, where the caller ``what`` has a ``dtype`` to choose, float64)."""
    if not isinstance(phi, WalkPolynomial):
        return PhiOperator(eng, phi, f, tr, noise)
    if f is None or dtype not in (None, torch.float64):
        raise ValueError(f"{what}: a WalkPolynomial needs its modulator f" +
                         (" and dtype float64" if dtype is not None else ""))
    return WalkOperator(eng, phi, f, tr, noise)


_engines: dict = {}


def get_engine(device=None) -> GRFEngine:
    """Process-wide engine per device (GRF_AMD_DEVICE overrides the default)."""
    if device is None:
        device = os.environ.get("GRF_AMD_DEVICE")
    key = str(device)
    if key not in _engines:
        _engines[key] = GRFEngine(device)
    return _engines[key]
