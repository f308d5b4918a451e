"""Device-resident GRF features and a differentiable K[x1, x2] for the GPyTorch surface.

Replaces the tensor algebra of the reference's GPyTorch kernels
(``efficient_graph_gp_sparse/gptorch_kernels_sparse/sparse_grf_kernel.py:24-61``,
``sparse_diffusion_kernel.py:74-96``)::

    phi = sum(f_l * M_l)                      # grf_phi_steps_csr_count / _fill
    phi[x1], phi[x2]                          # grf_csr_row_lengths + grf_scan_counts + grf_csr_gather_rows
    K = phi[x1] @ phi[x2].T                   # banded transpose + grf_gram_sparse_cols (exact fixed point)
    diag = (phi[x1] * phi[x2]).sum(-1)        # grf_csr_rowdot

with the modulator gradient of ``K`` in ``backward`` (``GRFKernelFunction``):

    dL/df_l = sum_{r,s} G[r,s] (M_l[x1_r] . Phi[x2_s] + Phi[x1_r] . M_l[x2_s])
            = sum_r (M_l[x1] Z1)[r, r] + sum_s (M_l[x2] Z2)[s, s],
    Z1 = Phi[x2]^T G^T,  Z2 = Phi[x1]^T G       # grf_csr_transpose + grf_spmm_csr, then grf_csr_rows_dot_cols

Nothing here densifies Phi, and the step matrices never leave the device.

On a ``WalkPolynomial`` (the exact Phi = sum_l f_l G^l, never formed) ``grf_kernel`` runs forward and backward on the
operator's K-block entry points instead (``WalkOperatorKernelFunction``).
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib as C
from .engine import (DeviceCSR, GRFEngine, WalkPolynomial, _p, cols_band_width, get_engine,  # noqa: F401
                     preconditioner_name)


def _torch_csr(mat) -> torch.Tensor:
    t = getattr(mat, "sparse_csr_tensor", mat)
    if not (torch.is_tensor(t) and t.is_sparse_csr):
        raise ValueError("step matrices must be torch sparse CSR tensors (or SparseLinearOperator over them)")
    return t


def _rows_sorted_unique(t: torch.Tensor) -> bool:
    """Every row's column indices strictly increasing (one device pass, one host read)."""
    col = t.col_indices()
    nnz = col.numel()
    if nnz < 2:
        return True
    crow = t.crow_indices().long()
    starts = torch.zeros(nnz, dtype=torch.bool, device=col.device)
    first = crow[:-1]
    starts[first[first < nnz]] = True  # entry e opens a row: no order constraint against e - 1
    bad = (col[1:] <= col[:-1]) & ~starts[1:]
    return not bool(bad.any().item())


class StepMatrices:
    """The L step matrices of one graph on one device: int64 row pointers, int32 columns and the
    preprocessor's float32 values (views of the torch CSR tensors where the dtypes already match)."""

    def __init__(self, mats: Sequence, engine: Optional[GRFEngine] = None):
        ts = [_torch_csr(m) for m in mats]
        if not ts:
            raise ValueError("no step matrices")
        self.engine = engine or get_engine(ts[0].device if ts[0].is_cuda else None)
        dev = self.engine.device
        self.shape = tuple(ts[0].shape)
        self.steps: List[DeviceCSR] = []
        for t in ts:
            if tuple(t.shape) != self.shape:
                raise ValueError("step matrices differ in shape")
            if not _rows_sorted_unique(t):
                # grf_phi_steps_csr's L-way merge needs sorted, duplicate-free columns in every row;
                # torch's own sparse ops accept any order and sum duplicates, so coalesce to that meaning
                t = t.to_sparse_coo().coalesce().to_sparse_csr()
            ptr = t.crow_indices().to(dev, torch.int64).contiguous()
            idx = t.col_indices().to(dev, torch.int32).contiguous()
            val = t.values().to(dev, torch.float32).contiguous()
            self.steps.append(DeviceCSR(self.shape[0], self.shape[1], ptr, idx, None, val, int(idx.numel())))
        # bounds of Phi = sum_l f_l M_l, from one host read here (the forward / backward read nothing back):
        # its entries <= sum_l nnz(M_l), a row's entries <= sum_l (the longest row of M_l)
        self.nnz_sum = sum(s.nnz for s in self.steps)
        lens = torch.stack([(s.ptr[1:] - s.ptr[:-1]).max() if self.shape[0] else s.ptr[:1] * 0 for s in self.steps])
        self.row_bound = int(min(self.shape[1], int(lens.sum().item())))
        # host arrays of the L device pointers (the C ABI's step_ptr / step_idx / step_val)
        self._arrays = [(ctypes.c_void_p * len(self.steps))(*[getattr(s, a).data_ptr() for s in self.steps])
                        for a in ("ptr", "idx", "val32")]
        self._ptrs = [ctypes.cast(a, ctypes.c_void_p) for a in self._arrays]

    @property
    def L(self) -> int:
        return len(self.steps)

    def phi(self, f: torch.Tensor, want64: bool = False) -> DeviceCSR:
        """Phi = sum_l f_l M_l (compact CSR, fp32 values [+ fp64]) for the modulator f (len >= 1).
        No host synchronisation: the entry buffers are sized by ``nnz_sum`` (``DeviceCSR.nnz_bound``)."""
        eng = self.engine
        n = self.shape[0]
        ft = f.detach().to(eng.device, torch.float64).contiguous().flatten()
        nf = min(int(ft.numel()), self.L)
        cnt = eng._empty(n, torch.int32)
        C.check(eng.lib.grf_phi_steps_csr_count(n, self.L, self._ptrs[0], self._ptrs[1], self._ptrs[2], _p(ft), nf,
                                                _p(cnt), eng.stream), "grf_phi_steps_csr_count")
        ptr = eng._empty(n + 1, torch.int64)
        ws = eng._ws(eng.lib.grf_scan_workspace_bytes(n))
        C.check(eng.lib.grf_scan_counts(n, _p(cnt), _p(ptr), _p(ws), ws.numel(), eng.stream), "grf_scan_counts")
        cap = max(self.nnz_sum, 1)
        idx = eng._empty(cap, torch.int32)
        v32 = eng._empty(cap, torch.float32)
        v64 = eng._empty(cap, torch.float64) if want64 else None
        C.check(eng.lib.grf_phi_steps_csr_fill(n, self.L, self._ptrs[0], self._ptrs[1], self._ptrs[2], _p(ft), nf,
                                               _p(ptr), _p(idx), _p(v64), _p(v32), eng.stream),
                "grf_phi_steps_csr_fill")
        return DeviceCSR(n, self.shape[1], ptr, idx, v64, v32, None, nnz_bound=self.nnz_sum, row_bound=self.row_bound)


def gather_rows(eng: GRFEngine, A: DeviceCSR, rows: torch.Tensor) -> DeviceCSR:
    """A[rows] as a compact CSR (rows may repeat).  With ``A.row_bound`` known the entry buffers are
    sized by rows x that bound and nothing is read back to the host."""
    rmap = rows.to(eng.device, torch.int32).contiguous()
    n_sel = rmap.numel()
    cnt = eng._empty(n_sel, torch.int32)
    C.check(eng.lib.grf_csr_row_lengths(n_sel, _p(A.ptr), _p(rmap), _p(cnt), eng.stream), "grf_csr_row_lengths")
    ptr = eng._empty(n_sel + 1, torch.int64)
    ws = eng._ws(eng.lib.grf_scan_workspace_bytes(n_sel))
    C.check(eng.lib.grf_scan_counts(n_sel, _p(cnt), _p(ptr), _p(ws), ws.numel(), eng.stream), "grf_scan_counts")
    bound = A.rows_entry_bound(n_sel)
    if bound is not None:
        nnz = None
    else:
        nnz = int(ptr[-1].item()) if n_sel else 0
        bound = nnz
    idx = eng._empty(max(bound, 1), torch.int32)
    val = eng._empty(max(bound, 1), torch.float32)
    C.check(eng.lib.grf_csr_gather_rows(n_sel, _p(A.ptr), _p(A.idx), _p(A.val32), _p(rmap), _p(ptr), _p(idx),
                                        _p(val), eng.stream), "grf_csr_gather_rows")
    return DeviceCSR(n_sel, A.n_cols, ptr, idx, None, val, nnz, nnz_bound=bound, row_bound=A.row_bound)


def _square_symmetrised(K: torch.Tensor, i1: Optional[torch.Tensor], i2: Optional[torch.Tensor]) -> torch.Tensor:
    """K(x1, x2) for equal-length index tensors that are different objects: where x1 and x2 hold the
    same values (decided on the device, no host read), the block is K(x, x) and is returned exactly
    symmetric as (K + K^T) / 2 -- what the symmetric path's mirrored tiles give up to the K tolerance;
    otherwise K unchanged.  K (a fresh block) is updated in place with one temporary: lerp with a 0 / 1
    weight returns its start or its end exactly (torch evaluates weight >= 0.5 as end - (end - start)(1 - w))."""
    if i1 is None or i2 is None or K.dim() != 2 or K.shape[0] != K.shape[1] or i1.shape != i2.shape:
        return K
    same = torch.eq(i1, i2).all().to(K.dtype)
    T = K + K.t()
    return K.lerp_(T.mul_(0.5), same)


def rowdot(eng: GRFEngine, A: DeviceCSR, rows_a: Optional[torch.Tensor], B: DeviceCSR,
           rows_b: Optional[torch.Tensor], n_pairs: int) -> torch.Tensor:
    """out[r] = A[rows_a[r]] . B[rows_b[r]] (fp64)."""
    ra = None if rows_a is None else rows_a.to(eng.device, torch.int32).contiguous()
    rb = None if rows_b is None else rows_b.to(eng.device, torch.int32).contiguous()
    out = eng._empty(n_pairs, torch.float64)
    C.check(eng.lib.grf_csr_rowdot(n_pairs, _p(A.ptr), _p(A.idx), _p(A.val32), _p(ra), _p(B.ptr), _p(B.idx),
                                   _p(B.val32), _p(rb), _p(out), eng.stream), "grf_csr_rowdot")
    return out


def rows_dot_cols(eng: GRFEngine, M: DeviceCSR, rows: Optional[torch.Tensor], Z: torch.Tensor) -> torch.Tensor:
    """out[r] = sum_e M[rows[r], e] Z[col_e, r] (fp64), Z float32 (n_cols x >= n_sel) row-major."""
    rmap = None if rows is None else rows.to(eng.device, torch.int32).contiguous()
    n_sel = M.n_rows if rmap is None else rmap.numel()
    if Z.dtype != torch.float32 or Z.stride(1) != 1 or Z.shape[0] != M.n_cols:
        raise ValueError("rows_dot_cols: Z must be a float32 (n_cols x S) row-major matrix")
    out = eng._empty(n_sel, torch.float64)
    C.check(eng.lib.grf_csr_rows_dot_cols(n_sel, _p(M.ptr), _p(M.idx), _p(M.val32), _p(rmap), _p(Z), Z.stride(0),
                                          _p(out), eng.stream), "grf_csr_rows_dot_cols")
    return out


def kernel_block(eng: GRFEngine, phi: DeviceCSR, x1: Optional[torch.Tensor], x2: Optional[torch.Tensor],
                 same: bool) -> torch.Tensor:
    """K[x1, x2] = Phi[x1] Phi[x2]^T (float32, |x1| x |x2|) on the sparse Gram kernels: the
    column-block Gram of Phi[x1]'s rows against the banded transpose of Phi[x2] (exact fixed-point
    sums; with x1 == x2 the symmetric enumeration + mirror, so K comes out exactly symmetric)."""
    P1 = phi if x1 is None else gather_rows(eng, phi, x1)
    P2 = P1 if same else (phi if x2 is None else gather_rows(eng, phi, x2))
    n1, n2 = P1.n_rows, P2.n_rows
    if n1 == 0 or n2 == 0:
        return torch.zeros((n1, n2), dtype=torch.float32, device=eng.device)
    tr = eng.transpose_banded(P2, cols_band_width(n2), nnz_bound=P2.nnz_or_bound())
    # the fixed-point shift of row r bounds |Phi[r, k] Phi[j, k]| with max|Phi| over the OTHER operand's
    # rows j too: take it over all of Phi (a superset of Phi[x1] and Phi[x2]) and pick the x1 rows
    shifts = eng.phi_row_shifts(phi)
    if x1 is not None:
        shifts = shifts[x1.to(eng.device).long()].contiguous()
    return eng.gram_sparse_cols(P1, shifts, tr, 0, n1, sym_row0=0 if same else None)


def _index(x: Optional[torch.Tensor], dev) -> Optional[torch.Tensor]:
    return None if x is None else x.long().flatten().to(dev)


def _same_rows(x1, x2, i1: Optional[torch.Tensor], i2: Optional[torch.Tensor]) -> bool:
    """x1 and x2 are the same rows, decided without reading them back: both None, the same tensor, or views of
    the same memory."""
    return (x1 is None and x2 is None) or (x1 is x2) or (
        i1 is not None and i2 is not None and i1.shape == i2.shape and i1.data_ptr() == i2.data_ptr()
        and i1.stride() == i2.stride())


class GRFKernelFunction(torch.autograd.Function):
    """K[x1, x2] (or its diagonal) = Phi(f)[x1] Phi(f)[x2]^T, differentiable w.r.t. the modulator f."""

    @staticmethod
    def forward(ctx, f: torch.Tensor, steps: StepMatrices, x1, x2, diag: bool):
        eng = steps.engine
        dev = eng.device
        n = steps.shape[0]
        i1, i2 = _index(x1, dev), _index(x2, dev)
        # x1 and x2 the same rows (the symmetric block): decided without reading the indices back -- the
        # same tensor, or views of the same memory (a K(x, x) call); equal values in two different tensors
        # take the general column-block path (the same numbers within the K tolerance)
        same = _same_rows(x1, x2, i1, i2)
        phi = steps.phi(f)
        if diag:
            n1 = n if i1 is None else i1.numel()
            n2 = n if i2 is None else i2.numel()
            if n1 != n2:
                raise ValueError("diag=True needs x1 and x2 of the same length")
            out = rowdot(eng, phi, i1, phi, i2, n1).to(f.dtype)
        else:
            out = kernel_block(eng, phi, i1, i2, same)
            if not same:
                out = _square_symmetrised(out, i1, i2)
            out = out.to(f.dtype) if out.dtype != f.dtype else out
        ctx.steps, ctx.phi, ctx.i1, ctx.i2, ctx.diag, ctx.n_f = steps, phi, i1, i2, diag, f.numel()
        ctx.f_dtype, ctx.f_device = f.dtype, f.device
        return out

    @staticmethod
    def backward(ctx, g: torch.Tensor):
        steps, phi, i1, i2 = ctx.steps, ctx.phi, ctx.i1, ctx.i2
        eng = steps.engine
        L = min(steps.L, ctx.n_f)
        grad = torch.zeros(ctx.n_f, dtype=torch.float64, device=eng.device)
        n = steps.shape[0]
        if ctx.diag:
            gd = g.to(eng.device, torch.float64)
            m = gd.numel()
            for l in range(L):
                M = steps.steps[l]
                d = rowdot(eng, M, i1, phi, i2, m) + rowdot(eng, phi, i1, M, i2, m)
                grad[l] = (gd * d).sum()
        else:
            G = g.to(eng.device, torch.float32).contiguous()
            n1 = n if i1 is None else i1.numel()
            n2 = n if i2 is None else i2.numel()
            if n1 and n2:
                Z1 = eng.spmm(eng.csr_transpose(phi, i2), G.t().contiguous())  # N x n1: Phi[x2]^T G^T
                Z2 = eng.spmm(eng.csr_transpose(phi, i1), G)                   # N x n2: Phi[x1]^T G
                for l in range(L):
                    M = steps.steps[l]
                    grad[l] = rows_dot_cols(eng, M, i1, Z1).sum() + rows_dot_cols(eng, M, i2, Z2).sum()
        # (on f's own device: a modulator parameter left on the CPU still gets its gradient)
        return grad.to(device=ctx.f_device, dtype=ctx.f_dtype), None, None, None, None


class WalkOperatorKernelFunction(torch.autograd.Function):
    """K[x1, x2] (or diag K[x]) of the exact kernel Phi = p(G) on a WalkPolynomial, differentiable w.r.t. the
    modulator f: forward and backward run on the operator's K-block entry points in fp64 (GRFEngine.
    poly_kernel_block / poly_kernel_diag / poly_kernel_grad), Phi never formed, nothing read back to the host."""

    @staticmethod
    def forward(ctx, f: torch.Tensor, op: WalkPolynomial, x1, x2, diag: bool):
        eng = op.engine
        i1, i2 = _index(x1, eng.device), _index(x2, eng.device)
        if diag:
            if not _same_rows(x1, x2, i1, i2):
                raise ValueError("diag=True on a WalkPolynomial needs x1 and x2 to be the same tensor (diag K[x])")
            out = eng.poly_kernel_diag(op, f, i1)
        else:
            out = eng.poly_kernel_block(op, f, i1, i2)
            # (the two chains of K(x, x) round differently above and below the diagonal)
            if i1 is None and i2 is None:
                out = (out + out.t()).mul_(0.5)
            else:
                out = _square_symmetrised(out, i1, i2)
        ctx.save_for_backward(f)
        ctx.op, ctx.i1, ctx.i2, ctx.diag = op, i1, i2, diag
        return out.to(f.dtype)

    @staticmethod
    def backward(ctx, g: torch.Tensor):
        eng = ctx.op.engine
        f, = ctx.saved_tensors
        grad = torch.zeros(f.numel(), dtype=torch.float64, device=eng.device)
        out = eng.poly_kernel_grad(ctx.op, f, g, ctx.i1, ctx.i2, ctx.diag)
        grad[:out.numel()] = out  # (entries of f past the walk length do not enter)
        # (on f's own device: a modulator parameter left on the CPU still gets its gradient)
        return grad.to(device=f.device, dtype=f.dtype), None, None, None, None


def grf_kernel(f: torch.Tensor, steps, x1=None, x2=None, diag: bool = False) -> torch.Tensor:
    """K[x1, x2] = Phi[x1] Phi[x2]^T, differentiable in f, with Phi = sum_l f_l M_l on a StepMatrices or the
    exact Phi = sum_l f_l G^l on a WalkPolynomial (matrix-free, fp64 arithmetic, the result in f's dtype)."""
    if isinstance(steps, WalkPolynomial):
        return WalkOperatorKernelFunction.apply(f, steps, x1, x2, diag)
    return GRFKernelFunction.apply(f, steps, x1, x2, diag)


class GRFMarginalLikelihoodFunction(torch.autograd.Function):
    """The matrix-free marginal log-likelihood of y under K^ = Phi(f)[T] Phi(f)[T]^T + noise I
    (``GRFEngine.marginal_log_likelihood``: CG + stochastic Lanczos quadrature, fp64, K never formed),
    differentiable w.r.t. the modulator f and the noise.  ``steps`` is a StepMatrices or a WalkPolynomial (the
    exact kernel Phi = p(G) as a matrix-free operator: the same estimator, no step matrix).  The forward computes the value and both
    gradients (they share the one CG solve); the backward scales them by the incoming scalar."""

    @staticmethod
    def forward(ctx, f: torch.Tensor, noise: torch.Tensor, steps, train_idx, y, probes,
                tolerance: float, max_iter: int, info: Optional[dict], preconditioner=None):
        eng = steps.engine
        value, g_f, g_noise, iters = eng.marginal_log_likelihood(
            steps, f, train_idx, y, float(noise.detach().reshape(-1)[0].item()), probes, tolerance, max_iter,
            preconditioner=preconditioner)
        grad_f = torch.zeros(f.numel(), dtype=torch.float64, device=eng.device)
        grad_f[:g_f.numel()] = g_f  # (modulator entries past the last step matrix do not enter Phi)
        ctx.grad_f = grad_f.reshape(f.shape).to(device=f.device, dtype=f.dtype)
        ctx.grad_noise = torch.full(noise.shape, g_noise, dtype=noise.dtype, device=noise.device)
        if info is not None:
            info["cg_iterations"] = iters
        return torch.tensor(value, dtype=torch.float64, device=f.device)

    @staticmethod
    def backward(ctx, g: torch.Tensor):
        gf = ctx.grad_f * g.to(device=ctx.grad_f.device, dtype=ctx.grad_f.dtype)
        gn = ctx.grad_noise * g.to(device=ctx.grad_noise.device, dtype=ctx.grad_noise.dtype)
        return gf, gn, None, None, None, None, None, None, None, None


def resolve_cg_tolerance(tolerance: Optional[float]) -> float:
    """None -> gpytorch.settings.cg_tolerance when gpytorch is installed, else its default 1.0 (the one rule of
    SparseGraphGP.predict and the marginal likelihood)."""
    if tolerance is not None:
        return float(tolerance)
    try:
        import gpytorch
    except ImportError:
        return 1.0
    return float(gpytorch.settings.cg_tolerance.value())


def grf_marginal_log_likelihood(f: torch.Tensor, noise, steps, train_idx, y, probes=None,
                                n_probes: int = 64, generator=None, tolerance: Optional[float] = None,
                                max_iter: int = 1000, per_datum: bool = True,
                                info: Optional[dict] = None, preconditioner=None) -> torch.Tensor:
    """MLL(f, noise) of y at the training nodes, a differentiable fp64 scalar (on f's device).  steps: a
    StepMatrices (Phi = sum_l f_l M_l) or a WalkPolynomial (Phi = sum_l f_l G^l, matrix-free).

    f, noise: torch tensors (noise with one element; a float is a constant) -- the gradient flows to
    whatever they were computed from.  probes: (n_train x t) Hutchinson probes, t <= 255; by default
    ``torch.randn(n_train, n_probes, generator=generator)`` drawn on the generator's device, or on the
    engine's when there is none (no host draw and upload per training step).  per_datum divides by n_train,
    as gpytorch's ExactMarginalLogLikelihood does.  info: a dict that receives ``cg_iterations``.
    preconditioner: None, or "jacobi" -- the solve preconditioned by diag(K^), the probes rescaled so that the
    value and the gradients estimate the same quantities (``GRFEngine.marginal_log_likelihood``); typically
    several times fewer CG iterations on the walk estimator's Phi."""
    eng = steps.engine
    preconditioner_name(preconditioner, "grf_marginal_log_likelihood")
    idx = torch.as_tensor(train_idx).flatten()
    n = idx.numel()
    yt = torch.as_tensor(y).flatten()
    if n == 0 or yt.numel() != n:
        raise ValueError("grf_marginal_log_likelihood: y must hold one value per training node")
    if probes is None:
        if not 1 <= int(n_probes) <= 255:
            raise ValueError("grf_marginal_log_likelihood: between 1 and 255 probes per call")
        probes = torch.randn(n, int(n_probes), generator=generator,
                             device=generator.device if generator is not None else eng.device)
    elif probes.dim() != 2 or probes.shape[0] != n:
        raise ValueError(f"grf_marginal_log_likelihood: probes must be ({n} x t), got {tuple(probes.shape)}")
    elif not 1 <= probes.shape[1] <= 255:
        raise ValueError("grf_marginal_log_likelihood: between 1 and 255 probes per call")
    if not torch.is_tensor(noise):
        noise = torch.tensor(float(noise), dtype=torch.float64)
    if noise.numel() != 1:
        raise ValueError("grf_marginal_log_likelihood: noise must have one element")
    out = GRFMarginalLikelihoodFunction.apply(f, noise, steps, idx, yt, probes, resolve_cg_tolerance(tolerance),
                                              int(max_iter), info, preconditioner)
    return out / n if per_datum else out


def feature_matrix(f: torch.Tensor, steps: StepMatrices) -> torch.Tensor:
    """Phi as a torch sparse CSR tensor (float32 values, int64 indices) on the device (not differentiable)."""
    phi = steps.phi(f)
    return torch.sparse_csr_tensor(phi.ptr, phi.idx[:phi.nnz].long(), phi.val32[:phi.nnz], steps.shape,
                                   dtype=torch.float32)


# ----------------------------------------------------------------- dense step tensors (GPflow surface)
class DenseSteps:
    """A dense (N, N, L) step tensor F resident on the device once (the GPflow wrappers'
    ``feature_matrices_tf``, gpflow_kernels/general_kernel_fast_grf.py:44-59).  Per modulator value:
    Phi = F f on ``grf_dense_steps_phi`` (fp64, plus the fp32 image of the Gram), K = Phi Phi^T on the
    MFMA Gram (``GRFEngine.gram_dense``: the engine's dense precision, by default the exact bf16 split
    ``grf_gram_dense_split``), cached; the modulator gradient on ``grf_dense_steps_grad``."""

    def __init__(self, F, engine: Optional[GRFEngine] = None):
        self.engine = engine or get_engine()
        Ft = F if torch.is_tensor(F) else torch.from_numpy(np.ascontiguousarray(F, dtype=np.float64))
        self.F = Ft.to(self.engine.device, torch.float64).contiguous()
        if self.F.dim() != 3 or self.F.shape[0] != self.F.shape[1]:
            raise ValueError("step tensor must be (N, N, L)")
        self.n, self.L = self.F.shape[0], self.F.shape[2]
        self.lda = max(64, -(-self.n // 64) * 64)  # (zero-padded k range of the MFMA Gram)
        self._key = None  # the cached K's key (gram)
        self._K = None
        self._phi64 = None

    def _modulator(self, f: torch.Tensor) -> torch.Tensor:
        ft = f.detach().to(self.engine.device, torch.float64).reshape(-1).contiguous()
        if ft.numel() != self.L:
            raise ValueError(f"modulator length {ft.numel()} != the step tensor's L = {self.L}")
        return ft

    def _phi_both(self, f: torch.Tensor):
        eng, n = self.engine, self.n
        ft = self._modulator(f)
        phi64 = torch.empty((n, n), dtype=torch.float64, device=eng.device)
        phi32 = torch.empty((n, self.lda), dtype=torch.float32, device=eng.device)
        C.check(eng.lib.grf_dense_steps_phi(n, self.L, _p(self.F), _p(ft), _p(phi64), _p(phi32), self.lda,
                                            eng.stream), "grf_dense_steps_phi")
        return phi64, phi32

    def phi(self, f: torch.Tensor) -> torch.Tensor:
        """Phi = F f (N x N, fp64 on the device): ``tf.linalg.matmul(F, f[:, None])`` (:76)."""
        return self._phi_both(f)[0]

    def gram(self, f: torch.Tensor, key=None) -> torch.Tensor:
        """K = Phi Phi^T (fp32, N x N) on the MFMA Gram, cached.  The cache key:
        * ``key`` when the caller has a host-side one (the modulator's own parameters, e.g. ("beta", b));
        * a modulator on the HOST (a CPU tensor, numpy-backed or not): its values (exact bytes), so a write
          through numpy or ``.data`` is seen;
        * a device modulator: the same memory at the same version counter (an in-place update such as an
          optimiser step bumps it; a tensor autograd saved for the backward shares both) -- no host read
          of f.  A write that bypasses the counter (``p.data.copy_(...)``: ``.data`` has a counter of its
          own) is not seen: call ``invalidate()`` after one.
        The cached K and Phi are dropped by ``invalidate()``."""
        k = self._key
        if key is not None:
            new_key = ("host", key)
            hit = k == new_key
        elif f.device.type == "cpu":
            new_key = ("value", tuple(f.shape), f.detach().to(torch.float64).contiguous().numpy().tobytes())
            hit = k == new_key
        else:
            new_key = ("tensor", f, f._version)
            hit = k is not None and k[0] == "tensor" and f.data_ptr() == k[1].data_ptr() and \
                f._version == k[2] and f.shape == k[1].shape and f.dtype == k[1].dtype and f.stride() == k[1].stride()
        if not hit:
            self._phi64, phi32 = self._phi_both(f)
            self._K = self.engine.gram_dense(phi32, self.n)
            self._key = new_key
        return self._K

    def invalidate(self) -> None:
        """Drop the cached K (and Phi): the next ``gram`` recomputes whatever the modulator's key says."""
        self._key, self._K, self._phi64 = None, None, None

    def grad(self, f: torch.Tensor, G: torch.Tensor) -> torch.Tensor:
        """dL/df_l = <F_l, (G + G^T) Phi> for the upstream gradient G of K (fp64, length L)."""
        eng, n = self.engine, self.n
        self.gram(f)  # (Phi of this modulator value)
        Gd = G.to(eng.device, torch.float64).contiguous()
        out = torch.empty(self.L, dtype=torch.float64, device=eng.device)
        need = int(eng.lib.grf_dense_steps_grad_workspace_bytes(n, self.L))
        ws = getattr(self, "_grad_ws", None)
        if ws is None or ws.numel() < need:
            ws = self._grad_ws = eng._ws(need)
        C.check(eng.lib.grf_dense_steps_grad(n, self.L, _p(self.F), _p(self._phi64), _p(Gd), Gd.stride(0), _p(out),
                                             _p(ws), ws.numel(), eng.stream), "grf_dense_steps_grad")
        return out


class DenseGramFunction(torch.autograd.Function):
    """K = (F f)(F f)^T with dK/df_l = F_l Phi^T + Phi F_l^T: the backward contracts the upstream
    G with it, dL/df_l = <F_l, (G + G^T) Phi> (grf_dense_steps_grad: fp64 MFMA GEMM + fused reduction)."""

    @staticmethod
    def forward(ctx, f: torch.Tensor, steps: DenseSteps):
        ctx.steps = steps
        ctx.save_for_backward(f)
        return steps.gram(f).to(f.dtype)

    @staticmethod
    def backward(ctx, g: torch.Tensor):
        (f,) = ctx.saved_tensors
        grad = ctx.steps.grad(f, g)
        return grad.to(device=f.device, dtype=f.dtype), None


# ------------------------------------------------------------------ the dense exact GPR (gpflow.models.GPR)
_LOG_2PI = float(np.log(2.0 * np.pi))


def gpr_factor(K: torch.Tensor, noise: torch.Tensor, engine: Optional[GRFEngine] = None):
    """(F, logdet, info) of ``GRFEngine.cholesky`` for K^ = K + noise I (K widened to fp64; no host read)."""
    eng = engine or get_engine()
    Kh = K.detach().to(eng.device, torch.float64, copy=True)
    Kh.diagonal().add_(noise.detach().to(eng.device, torch.float64).reshape(()))
    return eng.cholesky(Kh)


class GPRLogMarginalLikelihoodFunction(torch.autograd.Function):
    """log N(Y | 0, K + noise I) summed over Y's p columns (gpflow.models.GPR.log_marginal_likelihood), on the
    fp64 Cholesky of grf_potrf_f64 and the solves of grf_trsm_f64, with K^ = K + noise I and alpha = K^^-1 Y:

        lml = -1/2 sum_c y_c^T alpha_c - (p / 2) logdet K^ - (n p / 2) log 2 pi
        dL/dK = 1/2 (alpha alpha^T - p K^^-1),   dL/dnoise = trace(dL/dK),   dL/dY = -alpha.

    K^^-1 is two grf_trsm_f64 passes on the identity, alpha alpha^T - p K^^-1 one grf_gemm_nt_f64 call with Z.
    No host synchronisation in either direction.  Returns (lml, info): with info != 0 (K^ not positive definite)
    the value is NaN."""

    @staticmethod
    def forward(ctx, K: torch.Tensor, noise: torch.Tensor, Y: torch.Tensor, eng: GRFEngine, factor):
        n, p = int(Y.shape[0]), int(Y.shape[1])
        F, logdet, info = factor if factor is not None else gpr_factor(K, noise, eng)
        Yt = Y.detach().to(eng.device, torch.float64).t().contiguous()           # p x n: one right-hand side per row
        alpha_t = eng.cholesky_solve(F, Yt)                                       # (K^^-1 Y)^T
        quad = (Yt * alpha_t).sum()
        lml = -0.5 * quad - 0.5 * p * logdet[0] - 0.5 * n * p * _LOG_2PI
        ctx.eng, ctx.F, ctx.alpha_t = eng, F, alpha_t
        ctx.meta = (K.dtype, K.device, noise.dtype, noise.device, noise.shape, Y.dtype, Y.device)
        ctx.mark_non_differentiable(info)
        return lml, info

    @staticmethod
    def backward(ctx, g: torch.Tensor, _g_info):
        eng, F, alpha_t = ctx.eng, ctx.F, ctx.alpha_t
        k_dtype, k_dev, n_dtype, n_dev, n_shape, y_dtype, y_dev = ctx.meta
        p, n = int(alpha_t.shape[0]), int(alpha_t.shape[1])
        g = g.to(eng.device, torch.float64)
        gK = gn = gY = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            Kinv = eng.cholesky_solve(F, torch.eye(n, dtype=torch.float64, device=eng.device), inplace=True)
            alpha = alpha_t.t().contiguous()                                      # n x p
            G = eng.gemm_nt_f64(alpha, alpha, alpha=0.5, gamma=-0.5 * p, Z=Kinv, out=Kinv, symmetric=True)
            if ctx.needs_input_grad[1]:
                gn = (g * G.diagonal().sum()).reshape(n_shape).to(device=n_dev, dtype=n_dtype)
            if ctx.needs_input_grad[0]:
                gK = (g * G).to(device=k_dev, dtype=k_dtype)
        if ctx.needs_input_grad[2]:
            gY = (-g * alpha_t.t()).to(device=y_dev, dtype=y_dtype)
        return gK, gn, gY, None, None


def gpr_log_marginal_likelihood(K: torch.Tensor, noise, Y: torch.Tensor, factor=None,
                                engine: Optional[GRFEngine] = None):
    """(lml, info) of the dense exact GP regression: K (n x n, fp32 as ``K_torch`` returns it or fp64; widened to
    fp64), noise (a one-element tensor; a float is a constant), Y (n x p), zero mean, summed over the p columns as
    GPflow does.  ``lml`` is a differentiable fp64 scalar on the engine's device (gradients to K, noise and Y);
    ``info`` is the device int32 of the factorisation (non-zero: K + noise I is not positive definite and lml is
    NaN).  ``factor``: a (F, logdet, info) of ``gpr_factor`` for the same K and noise, to share one factorisation
    with other uses."""
    if K.dim() != 2 or K.shape[0] != K.shape[1] or K.shape[0] < 1:
        raise ValueError("gpr_log_marginal_likelihood: K must be square and non-empty")
    if Y.dim() != 2 or Y.shape[0] != K.shape[0] or Y.shape[1] < 1:
        raise ValueError(f"gpr_log_marginal_likelihood: Y must be ({K.shape[0]} x p)")
    eng = engine or get_engine()
    if not torch.is_tensor(noise):
        noise = torch.tensor(float(noise), dtype=torch.float64, device=eng.device)
    if noise.numel() != 1:
        raise ValueError("gpr_log_marginal_likelihood: noise must have one element")
    return GPRLogMarginalLikelihoodFunction.apply(K, noise, Y, eng, factor)


# ------------------------------------------------------------------ the sparse variational GP (gpflow.models.SVGP)
def svgp_factor(Kmm: torch.Tensor, jitter: float, engine: Optional[GRFEngine] = None):
    """(F, logdet, info) of ``GRFEngine.cholesky`` for Kmm + jitter I (Kmm widened to fp64; no host read)."""
    eng = engine or get_engine()
    Kh = Kmm.detach().to(eng.device, torch.float64, copy=True)
    Kh.diagonal().add_(float(jitter))
    return eng.cholesky(Kh)


def svgp_conditional(eng: GRFEngine, F: torch.Tensor, Knm: torch.Tensor, Knn_diag: torch.Tensor, q_mu: torch.Tensor,
                     Lq: torch.Tensor):
    """GPflow's whitened base_conditional with a full q_sqrt: (AT, T, fmean, fvar) for the factor F of Kmm.
    AT (N x M): row n is Lm^-1 k_n (one forward solve, the data points as right-hand-side rows; ``Knm`` is solved
    in place and must be the caller's own copy); fmean = AT q_mu (N x P); T = AT [Lq_1 ... Lq_P] (N x P M: one
    product against the stacked transposes); fvar[n, p] = Knn[n] - sum_m AT[n, m]^2 + sum_j T_p[n, j]^2."""
    P, M = int(Lq.shape[0]), int(Lq.shape[1])
    AT = eng.cholesky_solve(F, Knm, transposed=False, inplace=True)
    fmean = eng.gemm_nt_f64(AT, q_mu.t().contiguous())
    T = eng.gemm_nt_f64(AT, Lq.transpose(1, 2).reshape(P * M, M))
    base = Knn_diag - eng.rows_sqsum(AT, 1)[:, 0]
    fvar = eng.rows_sqsum(T, P, base)
    return AT, T, fmean, fvar


class SVGPElboFunction(torch.autograd.Function):
    """The whitened SVGP evidence lower bound, elbo = scale sum_n ve_n - KL (gpflow.models.SVGP.elbo with
    whiten=True, full q_sqrt), on grf_potrf_f64, grf_trsm_f64, grf_gemm_nt_f64, grf_rows_sqsum_f64 and the
    likelihood's expectations (grf_robustmax_ve_f64 for MultiClass):

        Lm = chol(Kmm + jitter I),  AT = (Lm^-1 Kmn)^T,  fmean = AT q_mu,  T_p = AT Lq_p,  Lq_p = tril(q_sqrt_p),
        fvar[n, p] = Knn[n] - sum_m AT[n, m]^2 + sum_j T_p[n, j]^2,
        KL = 1/2 (sum q_mu^2 - P M - sum_p sum_m log Lq_p[m, m]^2 + sum Lq^2).

    Backward, with Gm = d/dfmean, Gv = d/dfvar (N x P, from the likelihood's own launch), W_p = 2 Gv_p o T_p:
        d/dq_mu = AT^T Gm - q_mu,    d/dLq_p = tril(AT^T W_p - Lq_p + diag(1 / Lq_p[m, m])),    d/dKnn = sum_p Gv_p,
        ATbar   = Gm q_mu^T + sum_p W_p Lq_p^T - 2 (sum_p Gv_p) o AT,
        Knm_bar = ATbar Lm^-1 (rows Lm^-T abar_n),    L_bar = -tril(Kmn_bar A),
        Kmm_bar = sym(Lm^-T Phi(Lm^T L_bar) Lm^-1),   Phi: the lower triangle with the diagonal halved,
    by grf_gemm_nt_f64, cholesky_solve, transposes and tril only.  No host synchronisation in either direction.
    Returns (elbo, info): with info != 0 (Kmm + jitter I not positive definite) the value is NaN."""

    @staticmethod
    def forward(ctx, Kmm, Knm, Knn_diag, q_mu, q_sqrt, lik_param, Y, likelihood, scale, jitter, eng, factor):
        dev, f64 = eng.device, torch.float64
        F, _logdet, info = factor if factor is not None else svgp_factor(Kmm, jitter, eng)
        qm = q_mu.detach().to(dev, f64)
        Lq = torch.tril(q_sqrt.detach().to(dev, f64))
        P, M = int(Lq.shape[0]), int(Lq.shape[1])
        Knn = Knn_diag.detach().to(dev, f64)
        AT, T, fmean, fvar = svgp_conditional(eng, F, Knm.detach().to(dev, f64, copy=True), Knn, qm, Lq)
        par = lik_param.detach().to(dev, f64) if lik_param is not None else None
        ve, gmu, gvar, gpar = likelihood.variational_expectations(eng, fmean, fvar, Y, par, with_grad=True)
        kl = 0.5 * ((qm * qm).sum() - float(P * M) - torch.log(Lq.diagonal(dim1=1, dim2=2) ** 2).sum()
                    + (Lq * Lq).sum())
        elbo = float(scale) * ve.sum() - kl
        elbo = torch.where(info[0] != 0, torch.full_like(elbo, float("nan")), elbo)
        ctx.eng, ctx.scale = eng, float(scale)
        ctx.saved = (F, AT, T, qm, Lq, gmu, gvar, gpar)
        ctx.meta = [(t.dtype, t.device) if t is not None else None for t in (Kmm, Knm, Knn_diag, q_mu, q_sqrt,
                                                                             lik_param)]
        ctx.mark_non_differentiable(info)
        return elbo, info

    @staticmethod
    def backward(ctx, g, _g_info):
        eng = ctx.eng
        F, AT, T, qm, Lq, gmu, gvar, gpar = ctx.saved
        N, M, P = int(AT.shape[0]), int(AT.shape[1]), int(Lq.shape[0])
        g = g.to(eng.device, torch.float64)
        gs = g * ctx.scale
        Gm, Gv = gs * gmu, gs * gvar
        A = AT.t().contiguous()                                                      # M x N
        g_qmu = eng.gemm_nt_f64(A, Gm.t().contiguous()) - g * qm                     # AT^T Gm - q_mu
        W = ((2.0 * Gv)[:, :, None] * T.view(N, P, M)).reshape(N, P * M)
        g_LqT = eng.gemm_nt_f64(W.t().contiguous(), A)                               # rows (p, j): (AT^T W_p)[:, j]
        diag = Lq.diagonal(dim1=1, dim2=2)
        g_qsqrt = torch.tril(g_LqT.view(P, M, M).transpose(1, 2) - g * (Lq - torch.diag_embed(1.0 / diag)))
        Gs = Gv.sum(dim=1)
        ATbar = eng.gemm_nt_f64(Gm, qm)                                              # Gm q_mu^T
        ATbar = eng.gemm_nt_f64(W, Lq.permute(1, 0, 2).reshape(M, P * M), gamma=1.0, Z=ATbar, out=ATbar)
        ATbar.sub_((2.0 * Gs)[:, None] * AT)
        del W
        g_Kmm = g_Knm = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            Knm_bar = eng.cholesky_solve(F, ATbar, transposed=True, inplace=True)    # N x M: rows Lm^-T abar_n
            g_Knm = Knm_bar
            if ctx.needs_input_grad[0]:
                L_bar = -torch.tril(eng.gemm_nt_f64(Knm_bar.t().contiguous(), A))
                S = eng.gemm_nt_f64(torch.triu(F), L_bar.t().contiguous())          # Lm^T L_bar
                Phi = torch.tril(S)
                Phi.diagonal().mul_(0.5)
                X = eng.cholesky_solve(F, Phi, transposed=True, inplace=True)        # Phi Lm^-1
                X = eng.cholesky_solve(F, X.t().contiguous(), transposed=True, inplace=True)
                g_Kmm = 0.5 * (X + X.t())
        grads = [g_Kmm, g_Knm, Gs, g_qmu, g_qsqrt, gs * gpar if gpar is not None else None]
        out = []
        for need, meta, t in zip(ctx.needs_input_grad[:6], ctx.meta, grads):
            out.append(t.to(device=meta[1], dtype=meta[0]) if need and t is not None else None)
        return (*out, None, None, None, None, None, None)


def svgp_elbo(Kmm: torch.Tensor, Knm: torch.Tensor, Knn_diag: torch.Tensor, q_mu: torch.Tensor, q_sqrt: torch.Tensor,
              Y: torch.Tensor, likelihood, scale: float = 1.0, jitter: float = 1e-6, factor=None,
              engine: Optional[GRFEngine] = None):
    """(elbo, info) of the whitened sparse variational GP: Kmm (M x M), Knm (N x M), Knn_diag (N), fp32 as ``K_torch``
    returns them or fp64 (widened); q_mu (M x P), q_sqrt (P x M x M, its lower triangles are read); Y as the
    likelihood wants it (``efficient_graph_gp.likelihoods``: int32 labels on the device for MultiClass, N x P
    values for Gaussian).  ``elbo`` is a differentiable fp64 scalar on the engine's device (gradients to Kmm, Knm,
    Knn_diag, q_mu, q_sqrt's lower triangle and a Gaussian likelihood's variance); ``info`` is the device int32 of
    the factorisation (non-zero: Kmm + jitter I is not positive definite and elbo is NaN).  ``factor``: a
    (F, logdet, info) of ``svgp_factor`` for the same Kmm and jitter."""
    if Kmm.dim() != 2 or Kmm.shape[0] != Kmm.shape[1] or Kmm.shape[0] < 1:
        raise ValueError("svgp_elbo: Kmm must be square and non-empty")
    M = int(Kmm.shape[0])
    if Knm.dim() != 2 or Knm.shape[1] != M or Knm.shape[0] < 1:
        raise ValueError(f"svgp_elbo: Knm must be (N x {M})")
    N = int(Knm.shape[0])
    if Knn_diag.dim() != 1 or Knn_diag.numel() != N:
        raise ValueError(f"svgp_elbo: Knn_diag must hold {N} values")
    if q_mu.dim() != 2 or q_mu.shape[0] != M or q_sqrt.dim() != 3 or \
            tuple(q_sqrt.shape) != (q_mu.shape[1], M, M):
        raise ValueError(f"svgp_elbo: q_mu must be ({M} x P) and q_sqrt (P x {M} x {M})")
    eng = engine or get_engine()
    par = likelihood.parameter()
    return SVGPElboFunction.apply(Kmm, Knm, Knn_diag, q_mu, q_sqrt, par, Y, likelihood, scale, jitter, eng, factor)
