"""CPU: the argument and capacity contracts of the C entry points that had no contract module -- the Laplacians,
walks, steps and Phi, scan / compact / concat, the banded transposes, the sparse and dense Grams with their helpers,
the dense step tensor, the CSR transpose and SpMM, and the feature algebra.

Every case calls one entry with made-up pointers (abi_contract.P, never dereferenced) through
abi_contract.device_less_lib(), i.e. only in a process that sees no device.  There a call that passes every check
reaches a HIP call and returns GRF_EHIP; a refused one returns GRF_EINVAL, GRF_EUNSUPPORTED or GRF_ECAPACITY with
its own message.  Each table therefore starts from a baseline call that must come back GRF_EHIP (all its arguments
are acceptable) and changes one argument at a time: the refusal is due to that argument alone.

Sizes "just past the launch limit" come from the launch's own grid (blocks * threads >= 2^32), one per
variable-size launch; data-dependent arrays (idx, val, out_idx, t_rec contents ...) may be NULL when empty, which
the engine relies on for empty torch tensors, so no NEW guard refuses those: the cases that expect GRF_EINVAL for a
NULL idx / val / t_rec (the transposes, the column-block Gram) pin guards those entries always had.
"""
import os
import re

import pytest

import abi_contract as C
from abi_contract import ECAPACITY, EHIP, EINVAL, EUNSUPPORTED, OK, P, Case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "grf.h")
NAN = float("nan")
BIG = 1 << 62                                   # a byte count no size function reaches for an accepted size
I31 = (1 << 31) + 5                             # a size past the int32 node / column ids


def prototypes():
    """{function: [parameter names]} of include/grf.h."""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(grf_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        params = params.strip()
        out[name] = [] if params in ("", "void") else [re.findall(r"[A-Za-z_0-9]+", p)[-1] for p in params.split(",")]
    return out


PROTO = prototypes()

# entries with nothing to check: no arguments, no failure
NOTHING_TO_CHECK = ["grf_version", "grf_last_error", "grf_device_count"]

# entries whose contract tables are the older modules' (each is called there with made-up pointers or sizes)
ELSEWHERE = {
    "test_mll_abi": ["grf_steps_frob_f64", "grf_steps_frob_workspace_bytes"],
    "test_pcg_abi": ["grf_cg_workspace_bytes", "grf_gram_jacobi_f64", "grf_pcg_workspace_bytes",
                     "grf_pcg_gram_solve_f64", "grf_pcg_gram_solve_lanczos_f64", "grf_pcg_poly_workspace_bytes",
                     "grf_pcg_poly_solve_f64", "grf_pcg_poly_solve_lanczos_f64"],
    "test_poly_abi": ["grf_poly_workspace_bytes", "grf_poly_apply_f64", "grf_cg_poly_workspace_bytes",
                      "grf_cg_poly_solve_f64", "grf_cg_poly_solve_lanczos_f64", "grf_poly_grad_workspace_bytes",
                      "grf_poly_grad_f64"],
    "test_poly_block_abi": ["grf_poly_kernel_block_workspace_bytes", "grf_poly_kernel_block_f64",
                            "grf_poly_kernel_diag_workspace_bytes", "grf_poly_kernel_diag_f64",
                            "grf_poly_kernel_grad_workspace_bytes", "grf_poly_kernel_grad_f64"],
    "test_spgemm_abi": ["grf_spgemm_workspace_bytes", "grf_spgemm_csr_count", "grf_spgemm_csr_fill"],
    "test_expm_abi": ["grf_gemm_nt_f64_workspace_bytes", "grf_gemm_nt_f64", "grf_expm_squarings",
                      "grf_expm_sym_f64_workspace_bytes", "grf_expm_sym_f64"],
    "test_posterior_abi": ["grf_posterior_rhs_f64", "grf_posterior_reduce_workspace_bytes",
                           "grf_posterior_reduce_f64"],
}

# size and bound functions, checked by test_size_functions_* below (not by status codes)
SIZE_FUNCTIONS = ["grf_laplacian_csr_workspace_bytes", "grf_laplacian_dense_workspace_bytes", "grf_walk_aug_bytes",
                  "grf_scan_workspace_bytes", "grf_transpose_workspace_bytes", "grf_transpose_staging_bytes",
                  "grf_transpose_self_workspace_bytes", "grf_transpose_self_units_bound",
                  "grf_transpose_self_triples_lines_bound", "grf_gram_workspace_bytes",
                  "grf_phi_row_shifts_workspace_bytes", "grf_gram_dense_workspace_bytes",
                  "grf_gram_dense_split_workspace_bytes", "grf_planes_row_bytes",
                  "grf_dense_steps_grad_workspace_bytes", "grf_csr_transpose_workspace_bytes"]
HOST_HELPERS = ["grf_chunk_bounds"]             # test_chunk_bounds_is_array_split below

BASE = {}                                       # entry -> {parameter: acceptable value}
TABLES = {}                                     # family -> [(entry, {changed parameters}, status, substring)]


def sizes():
    from grf_amd import _lib
    return _lib.load()                          # (size functions take no pointers: called in this process)


def base(entry, **kw):
    assert list(kw) == [a for a in PROTO[entry] if a != "stream"], (entry, list(kw), PROTO[entry])
    BASE[entry] = kw


def rows(family, entry, *cases):
    """cases: (status, substring of grf_last_error(), {changed parameters}), after the entry's baseline call."""
    TABLES.setdefault(family, []).append((entry, {}, EHIP, ""))               # the baseline reaches the device
    for status, sub, change in cases:
        TABLES[family].append((entry, change, status, sub))


def nulls(sub, *names):
    return [(EINVAL, sub, {n: None}) for n in names]


def negs(sub, *names):
    return [(EINVAL, sub, {n: -1}) for n in names]


def grid(**change):
    return (EUNSUPPORTED, "work-items exceed one launch", change)


def build_tables():
    if TABLES:
        return
    S = sizes()
    p = iter(range(1, 1000))
    ptr = lambda: P(next(p))  # noqa: E731
    WP = C.walk_params

    # ------------------------------------------------------------------ device selection
    base("grf_set_device", device=0)
    TABLES["device"] = [("grf_set_device", {"device": -1}, EINVAL, "device")]

    # ------------------------------------------------------------------ Laplacians
    e = "grf_laplacian_csr"
    need = S.grf_laplacian_csr_workspace_bytes(100)
    base(e, n=100, a_ptr=ptr(), a_idx=ptr(), a_val=ptr(), mode=0, l_ptr=ptr(), l_idx=ptr(), l_val=ptr(), l_cap=1000,
         deg=ptr(), dinv=ptr(), workspace=ptr(), workspace_bytes=need)
    rows("laplacian", e, *negs("bad arguments", "n", "l_cap"), *nulls("bad arguments", "a_ptr", "l_ptr", "deg", "dinv"),
         (EUNSUPPORTED, "GRF_LAP_SCIPY", {"mode": 1}), (EUNSUPPORTED, "GRF_LAP_SCIPY", {"mode": 5}),
         (EUNSUPPORTED, "GRF_LAP_SCIPY", {"mode": -1}),
         (EINVAL, "workspace", {"workspace": None, "workspace_bytes": BIG}),
         (EINVAL, "workspace too small", {"workspace_bytes": need - 1}),
         (EUNSUPPORTED, "int32", {"n": I31, "workspace_bytes": BIG}),
         (EUNSUPPORTED, "int32", {"n": (1 << 39) + 32, "workspace_bytes": BIG}),
         grid(n=(1 << 29) + 1, workspace_bytes=BIG))               # lap_deg_group_kernel: cdiv(n, 32) x 256
    e = "grf_laplacian_dense"
    need = S.grf_laplacian_dense_workspace_bytes(100)
    base(e, n=100, W=ptr(), mode=1, l_ptr=ptr(), l_idx=ptr(), l_val=ptr(), l_cap=1000, deg=ptr(), workspace=ptr(),
         workspace_bytes=need)
    rows("laplacian", e, *negs("bad arguments", "n", "l_cap"), *nulls("bad arguments", "W", "l_ptr", "deg"),
         (EINVAL, "bad mode", {"mode": 0}), (EINVAL, "bad mode", {"mode": 5}), (EINVAL, "bad mode", {"mode": -1}),
         (EINVAL, "8-byte aligned", {"W": BASE[e]["W"] + 4}),
         (EINVAL, "workspace", {"workspace": None, "workspace_bytes": BIG}),
         (EINVAL, "256-byte aligned", {"workspace": BASE[e]["workspace"] + 128, "workspace_bytes": BIG}),
         (EINVAL, "workspace too small", {"workspace_bytes": need - 1}),
         (EUNSUPPORTED, "int32", {"n": I31, "workspace_bytes": BIG}),
         (EUNSUPPORTED, "int32", {"n": (1 << 31) - 1, "workspace_bytes": BIG}),   # (column ids < 2^31 - 1)
         grid(n=(1 << 26) + 1, workspace_bytes=BIG))               # lapd_stage_kernel: cdiv(n, 4) x 256

    # ------------------------------------------------------------------ walks
    for e in ("grf_walk", "grf_walk_ex"):
        aug = {"g_aug": ptr()} if e == "grf_walk_ex" else {}
        base(e, n=100, g_ptr=ptr(), g_idx=ptr(), g_val=ptr(), **aug, params=WP(), src_begin=0, src_end=100,
             slot_node=ptr(), slot_load=ptr())
        rows("walk", e, (EINVAL, "params is NULL", {"params": None}), *negs("bad arguments", "n"),
             *nulls("bad arguments", "g_ptr", "slot_node", "slot_load"),
             (EINVAL, "walks_per_node", {"params": WP(m=0)}), (EINVAL, "walks_per_node", {"params": WP(m=1 << 31)}),
             (EINVAL, "max_walk_length", {"params": WP(L=0)}),
             (EINVAL, "p_halt", {"params": WP(p=1.0)}), (EINVAL, "p_halt", {"params": WP(p=-0.125)}),
             (EINVAL, "p_halt", {"params": WP(p=NAN)}),
             (EINVAL, "load_rule", {"params": WP(load_rule=3)}), (EINVAL, "load_rule", {"params": WP(load_rule=-1)}),
             (EINVAL, "bad rng", {"params": WP(rng=2)}), (EINVAL, "bad rng", {"params": WP(rng=-1)}),
             (EINVAL, "source range", {"src_begin": -1}), (EINVAL, "source range", {"src_end": 101}),
             (EINVAL, "source range", {"src_begin": 60, "src_end": 50}),
             (EUNSUPPORTED, "int32 node ids", {"n": I31}),
             (EINVAL, "n_chunks", {"params": WP(rng=0, n_chunks=0)}),
             (EINVAL, "whole chunks", {"params": WP(rng=0, n_chunks=3), "src_end": 50}),   # chunks end at 34, 67, 100
             (EHIP, "", {"params": WP(rng=0, n_chunks=3), "src_end": 67}),
             grid(n=1 << 20, src_end=1 << 20, params=WP(m=(1 << 12) + 1)),      # walk_philox_kernel: cdiv(ns m, 256) x 256
             *([(EINVAL, "32-byte aligned", {"g_aug": aug["g_aug"] + 16})] if aug else []))
    e = "grf_walk_phi"
    base(e, n=100, g_ptr=ptr(), g_idx=ptr(), g_val=ptr(), g_aug=None, params=WP(), src_begin=0, src_end=100, norm=0,
         f=ptr(), n_f=4, phi_cap=32, phi_cnt=ptr(), phi_idx=ptr(), phi_val=ptr(), phi_val32=None, t_count=None,
         band_width=64, count_row0=0)
    tc = ptr()
    rows("walk", e, (EINVAL, "params is NULL", {"params": None}), *negs("bad arguments", "n"),
         *nulls("bad arguments", "g_ptr", "phi_cnt", "phi_idx", "phi_val"),       # (phi_val32 is NULL in the baseline)
         (EUNSUPPORTED, "Philox", {"params": WP(rng=0)}), (EUNSUPPORTED, "Philox", {"params": WP(rng=2)}),
         (EINVAL, "walks_per_node", {"params": WP(m=0)}), (EINVAL, "max_walk_length", {"params": WP(L=0)}),
         (EINVAL, "p_halt", {"params": WP(p=1.0)}), (EINVAL, "p_halt", {"params": WP(p=NAN)}),
         (EINVAL, "load_rule", {"params": WP(load_rule=3)}),
         (EINVAL, "source range", {"src_end": 101}), (EINVAL, "source range", {"src_begin": -1}),
         (EUNSUPPORTED, "int32 node ids", {"n": I31}),
         (EINVAL, "counting needs", {"t_count": tc, "band_width": 0}),
         (EINVAL, "counting needs", {"t_count": tc, "phi_cap": 31}),              # min(m L, n) = 32
         (EINVAL, "count_row0", {"t_count": tc, "count_row0": 1}),
         (EINVAL, "32-byte aligned", {"g_aug": P(900, 16)}),
         (EINVAL, "bad norm", {"norm": 2}), (EINVAL, "bad modulator", {"n_f": -1}),
         (EINVAL, "bad modulator", {"f": None}), (EUNSUPPORTED, "4096", {"params": WP(m=1025)}),
         (EINVAL, "phi_cap", {"phi_cap": 0}),
         grid(n=1 << 26, src_end=1 << 26))                                        # phi_fused_kernel: n_src x 64
    e = "grf_walk_aug"
    base(e, n=100, g_ptr=ptr(), g_idx=ptr(), g_val=ptr(), g_aug=ptr())
    rows("walk", e, *negs("bad arguments", "n"), *nulls("bad arguments", "g_ptr", "g_idx", "g_val", "g_aug"),
         (EINVAL, "32-byte aligned", {"g_aug": BASE[e]["g_aug"] + 16}), (EUNSUPPORTED, "int32", {"n": I31}))

    # ------------------------------------------------------------------ steps and Phi
    e = "grf_steps"
    base(e, n_src=10, m=8, L=4, norm=0, slot_node=ptr(), slot_load=ptr(), step_cnt=ptr(), step_idx=ptr(),
         step_val=ptr())
    rows("steps", e, *negs("bad arguments", "n_src"), (EINVAL, "bad arguments", {"m": 0}),
         (EINVAL, "bad arguments", {"L": 0}),
         *nulls("bad arguments", "slot_node", "slot_load", "step_cnt", "step_idx", "step_val"),
         (EINVAL, "bad norm", {"norm": 2}), (EINVAL, "bad norm", {"norm": -1}),
         (EUNSUPPORTED, "16384", {"m": 16385}), grid(n_src=1 << 24))             # steps_kernel: n_src L x 64
    e = "grf_steps_densify"
    base(e, n_src=10, m=8, L=4, n_cols=50, step_cnt=ptr(), step_idx=ptr(), step_val=ptr(), out=ptr())
    rows("steps", e, *negs("bad arguments", "n_src", "n_cols"), (EINVAL, "bad arguments", {"m": 0}),
         (EINVAL, "bad arguments", {"L": 0}), *nulls("bad arguments", "step_cnt", "step_idx", "step_val", "out"),
         (EUNSUPPORTED, "int32", {"n_cols": I31}), grid(n_src=1 << 24))           # cdiv(n_src L, 4) x 256
    e = "grf_phi"
    base(e, n_src=10, m=8, L=4, step_cnt=ptr(), step_idx=ptr(), step_val=ptr(), f=ptr(), n_f=4, phi_cap=32,
         phi_cnt=ptr(), phi_idx=ptr(), phi_val=ptr(), phi_val32=None)
    rows("steps", e, *negs("bad arguments", "n_src"), (EINVAL, "bad arguments", {"m": 0}),
         (EINVAL, "bad arguments", {"L": 0}),
         *nulls("bad arguments", "step_cnt", "step_idx", "step_val", "phi_cnt", "phi_idx", "phi_val"),
         (EINVAL, "bad modulator", {"n_f": -1}), (EINVAL, "bad modulator", {"f": None}),
         (EUNSUPPORTED, "64", {"L": 65}), (EINVAL, "phi_cap", {"phi_cap": 0}), (EINVAL, "phi_cap", {"phi_cap": -1}),
         grid(n_src=1 << 26))                                                     # phi_merge_kernel: cdiv(n_src, 4) x 256
    e = "grf_phi_fused"
    base(e, n_src=10, m=8, L=4, norm=0, slot_node=ptr(), slot_load=ptr(), f=ptr(), n_f=4, phi_cap=32, phi_cnt=ptr(),
         phi_idx=ptr(), phi_val=ptr(), phi_val32=None)
    rows("steps", e, *negs("bad arguments", "n_src"), (EINVAL, "bad arguments", {"m": 0}),
         (EINVAL, "bad arguments", {"L": 0}),
         *nulls("bad arguments", "slot_node", "slot_load", "phi_cnt", "phi_idx", "phi_val"),
         (EINVAL, "bad norm", {"norm": 2}), (EINVAL, "bad modulator", {"n_f": -1}),
         (EINVAL, "bad modulator", {"f": None}), (EUNSUPPORTED, "4096", {"m": 1025}),
         (EINVAL, "phi_cap", {"phi_cap": 0}), grid(n_src=1 << 26))                # phi_fused_kernel: n_src x 64

    # ------------------------------------------------------------------ scan, compact, concat
    e = "grf_scan_counts"
    n_scan = 10_000_000                                                           # (a scan that needs a workspace)
    need = S.grf_scan_workspace_bytes(n_scan)
    base(e, n=n_scan, cnt=ptr(), out_ptr=ptr(), workspace=ptr(), workspace_bytes=need)
    rows("sparse", e, *negs("bad arguments", "n"), *nulls("bad arguments", "cnt", "out_ptr"),
         (EINVAL, "workspace", {"workspace": None}), (EINVAL, "workspace too small", {"workspace_bytes": need - 1}),
         (EHIP, "", {"n": 100, "workspace": None, "workspace_bytes": 0}),         # (one tile: no workspace)
         grid(n=1 << 36, workspace_bytes=BIG))                                    # scan_reduce_kernel: cdiv(n, 4096) x 256
    for e in ("grf_compact_rows", "grf_compact_rows_stats"):
        st = e.endswith("stats")
        need = S.grf_phi_row_shifts_workspace_bytes(100)
        extra = {"stats": ptr(), "stats_bytes": need} if st else {}
        base(e, n_rows=100, cap=16, cnt=ptr(), out_ptr=ptr(), in_idx=ptr(), in_val=ptr(), in_val32=ptr(),
             out_idx=ptr(), out_val=ptr(), out_val32=ptr(), **extra)
        rows("sparse", e, *negs("bad arguments", "n_rows", "cap"),
             *nulls("bad arguments", "cnt", "out_ptr", "in_idx", "out_idx"),
             (EINVAL, "out_val needs in_val", {"in_val": None}),
             *([(EINVAL, "bad arguments", {"in_val32": None}), (EINVAL, "bad arguments", {"out_val32": None}),
                (EINVAL, "bad arguments", {"stats": None}),
                (EINVAL, "stats buffer too small", {"stats_bytes": need - 1}),
                (EUNSUPPORTED, "int32", {"n_rows": I31, "stats_bytes": BIG}),
                grid(n_rows=1 << 28, stats_bytes=BIG)] if st else
               [(EINVAL, "out_val32 needs in_val32", {"in_val32": None}),
                (EHIP, "", {"in_val": None, "out_val": None}), (EUNSUPPORTED, "int32", {"n_rows": I31}),
                grid(n_rows=1 << 28)]))                                            # cdiv(n_rows, 16) x 256
    e = "grf_concat_segments"
    base(e, n_seg=4, stride=1000, src=ptr(), seg_len=ptr(), dst_off=ptr(), dst=ptr())
    rows("sparse", e, *negs("bad arguments", "n_seg", "stride"), (EINVAL, "bad arguments", {"n_seg": 65536}),
         *nulls("bad arguments", "src", "seg_len", "dst_off", "dst"),
         (EHIP, "", {"stride": 1 << 40}))                                         # (a bounded grid-stride launch)

    # ------------------------------------------------------------------ banded transposes
    nr, nc, bw = 200, 300, 64
    nbk = -(-nr // bw) * nc
    common = dict(n_rows=nr, n_cols=nc, band_width=bw, rec_unit=128)

    def tr_common(e, ws_need, slot_ok=False, ws_sub="workspace"):
        return [*negs("bad arguments", "n_rows"), (EINVAL, "bad arguments", {"n_cols": 0}),
                (EINVAL, "bad arguments", {"n_cols": -1}), (EINVAL, "bad arguments", {"band_width": 0}),
                (EINVAL, "bad arguments", {"band_width": 8192 + 64}), (EINVAL, "rec_unit", {"rec_unit": 7}),
                (EINVAL, "rec_unit", {"rec_unit": 0}), *([] if slot_ok else [(EINVAL, "rec_unit", {"rec_unit": 32})]),
                (EINVAL, ws_sub, {"workspace": None}),
                (EINVAL, "workspace too small", {"workspace_bytes": ws_need - 1}),
                (EUNSUPPORTED, "int32", {"n_cols": I31, "workspace_bytes": BIG}),
                (EUNSUPPORTED, "int32", {"n_rows": I31, "workspace_bytes": BIG})]

    e = "grf_transpose_banded_plan"
    need = S.grf_transpose_workspace_bytes(nbk)
    base(e, **common, ptr=ptr(), idx=ptr(), t_desc=ptr(), counted=0, workspace=ptr(), workspace_bytes=need)
    rows("transpose", e, *tr_common(e, need), *nulls("bad arguments", "ptr", "idx", "t_desc"),
         grid(n_rows=1 << 26, n_cols=1, band_width=8192, workspace_bytes=BIG))    # tr_count_kernel: cdiv(n_rows, 4) x 256
    e = "grf_transpose_banded_fill"
    base(e, **common, ptr=ptr(), idx=ptr(), val=ptr(), t_desc=ptr(), t_rec=ptr(), t_rec_bytes=1 << 20,
         t_maxabs=ptr(), t_rowshift=ptr(), workspace=ptr(), workspace_bytes=need)
    rows("transpose", e, *tr_common(e, need),
         *nulls("bad arguments", "ptr", "idx", "val", "t_desc", "t_rec", "t_maxabs", "t_rowshift"),
         *negs("bad arguments", "t_rec_bytes"), (EINVAL, "128-byte aligned", {"t_rec": BASE[e]["t_rec"] + 64}),
         grid(n_rows=1 << 26, n_cols=1, band_width=8192, workspace_bytes=BIG))    # tr_fill_kernel: cdiv(n_rows, 4) x 256
    nnz = 1000
    stg = S.grf_transpose_staging_bytes(nr, nc, bw, nnz)
    e = "grf_transpose_banded_fill_staged"
    base(e, **common, ptr=ptr(), idx=ptr(), val=ptr(), t_desc=ptr(), t_rec=ptr(), t_rec_bytes=1 << 20,
         t_maxabs=ptr(), t_rowshift=ptr(), workspace=ptr(), workspace_bytes=need, nnz=nnz, staging=ptr(),
         staging_bytes=stg)
    rows("transpose", e, *tr_common(e, need),
         *nulls("bad arguments", "ptr", "idx", "val", "t_desc", "t_rec", "t_maxabs", "t_rowshift", "staging"),
         *negs("bad arguments", "t_rec_bytes"), (EINVAL, "128-byte aligned", {"t_rec": BASE[e]["t_rec"] + 64}),
         (EUNSUPPORTED, "multiple of 64", {"band_width": 100}),
         (EINVAL, "staging too small", {"staging_bytes": stg - 1}), (EINVAL, "staging too small", {"nnz": -1}),
         grid(n_rows=1 << 28, n_cols=1, band_width=8192, workspace_bytes=BIG, staging_bytes=BIG))  # tr_bin: n_rows / 16 x 256
    for e in ("grf_transpose_banded_self", "grf_transpose_banded_self_rec"):
        rec = e.endswith("_rec")
        kind = {"rec_kind": 0} if rec else {}
        need = S.grf_transpose_self_workspace_bytes(nr, nc, bw)
        units = S.grf_transpose_self_units_bound(nr, nc, bw, 128, nnz)
        base(e, **kind, **common, ptr=ptr(), idx=ptr(), val=ptr(), t_desc=ptr(), t_split=None, t_rec=ptr(),
             t_rec_bytes=units * 128, t_maxabs=ptr(), t_rowshift=ptr(), workspace=ptr(), workspace_bytes=need,
             nnz=nnz, staging=ptr(), staging_bytes=stg)
        lines = S.grf_transpose_self_triples_lines_bound(nr, nc, bw, nnz)
        split = ptr()
        rows("transpose", e, *tr_common(e, need, slot_ok=True, ws_sub="bad arguments"),
             *nulls("bad arguments", "ptr", "idx", "val", "t_desc", "t_rec", "t_maxabs", "t_rowshift", "staging"),
             *negs("bad arguments", "t_rec_bytes"), (EINVAL, "128-byte aligned", {"t_rec": BASE[e]["t_rec"] + 64}),
             (EUNSUPPORTED, "multiple of 64", {"band_width": 100}),
             (EUNSUPPORTED, "sub-band split", {"rec_unit": 32, "t_split": split}),
             (EINVAL, "staging too small", {"staging_bytes": stg - 1}), (EINVAL, "staging too small", {"nnz": -1}),
             (ECAPACITY, "t_rec too small", {"t_rec_bytes": units * 128 - 128}),
             (ECAPACITY, "t_rec too small", {"t_rec_bytes": units * 128 - 1}),
             (ECAPACITY, "t_rec too small", {"rec_unit": 12, "t_rec_bytes":
                                             S.grf_transpose_self_units_bound(nr, nc, bw, 12, nnz) * 12 - 12}),
             (EINVAL, "16-byte aligned", {"t_split": split + 8}), (EHIP, "", {"t_split": split}),
             grid(n_rows=1 << 28, n_cols=1, band_width=8192, workspace_bytes=BIG, staging_bytes=BIG, t_rec_bytes=BIG),
             *([(EINVAL, "rec_kind", {"rec_kind": 2}), (EINVAL, "rec_kind", {"rec_kind": -1}),
                (EHIP, "", {"rec_kind": 1, "t_rec_bytes": lines * 128}),
                (ECAPACITY, "t_rec too small", {"rec_kind": 1, "t_rec_bytes": lines * 128 - 128}),
                (EINVAL, "GRF_REC_TRIPLES needs", {"rec_kind": 1, "band_width": 8192}),
                (EINVAL, "GRF_REC_TRIPLES needs", {"rec_kind": 1, "rec_unit": 12}),
                (EINVAL, "GRF_REC_TRIPLES needs", {"rec_kind": 1, "t_split": split})] if rec else []))

    # ------------------------------------------------------------------ sparse Gram
    nt = 300
    g = dict(ptr=ptr(), idx=ptr(), val=ptr(), band_width=64, rec_unit=128, t_desc=ptr(), t_rec=ptr())
    K, shift, cuts, split = ptr(), ptr(), ptr(), ptr()

    def gram_common(e, total="n_total", ld=nt, nul=("ptr", "t_desc", "t_rec", "K")):
        return [*negs("bad arguments", total), *nulls("bad arguments", *nul),
                (EINVAL, "rec_unit", {"rec_unit": 7}), (EINVAL, "rec_unit", {"rec_unit": 0}),
                (EINVAL, "128-byte aligned", {"t_rec": g["t_rec"] + 64}), (EINVAL, "ldk <", {"ldk": ld - 1}),
                *[(EUNSUPPORTED, "multiple of 64", {"band_width": b}) for b in (0, 32, 100, 8192 + 64)]]

    def past_int32(total="n_total"):
        return (EUNSUPPORTED, "int32", {total: I31, "ldk": I31})

    ws = dict(workspace=None, workspace_bytes=0)
    e = "grf_gram_sparse"
    base(e, n_total=nt, row_begin=0, row_end=100, **g, t_rowshift=shift, K=K, ldk=nt, **ws)
    rng_rows = [(EINVAL, "bad arguments", {"row_begin": -1}), (EINVAL, "bad arguments", {"row_end": nt + 1}),
                (EINVAL, "bad arguments", {"row_begin": 60, "row_end": 50})]
    rows("gram", e, *gram_common(e), *nulls("bad arguments", "t_rowshift"), *rng_rows, past_int32())
    e = "grf_gram_sparse_rec"
    base(e, rec_kind=0, n_total=nt, row_begin=0, row_end=100, **g, t_rowshift=shift, K=K, ldk=nt)
    tri = [(EINVAL, "GRF_REC_TRIPLES needs", {"rec_kind": 2}), (EINVAL, "GRF_REC_TRIPLES needs", {"rec_kind": -1}),
           (EHIP, "", {"rec_kind": 1}), (EINVAL, "GRF_REC_TRIPLES needs", {"rec_kind": 1, "rec_unit": 12}),
           (EINVAL, "GRF_REC_TRIPLES needs", {"rec_kind": 1, "band_width": 8192})]
    rows("gram", e, *gram_common(e), *nulls("bad arguments", "t_rowshift"), *rng_rows, past_int32(), *tri)
    e = "grf_gram_sparse_kslice"
    base(e, n_total=nt, row_begin=0, row_end=100, k_begin=0, k_end=nt, **g, t_rowshift=shift, K=K, ldk=nt, **ws)
    rows("gram", e, *gram_common(e), *nulls("bad arguments", "t_rowshift"), *rng_rows, past_int32(),
         (EINVAL, "column slice", {"k_begin": -1}), (EINVAL, "column slice", {"k_end": nt + 1}),
         (EINVAL, "column slice", {"k_begin": 60, "k_end": 50}))
    parts = [(EINVAL, "tile parts", {"n_parts": 0}), (EINVAL, "tile parts", {"part_begin": -1}),
             (EINVAL, "tile parts", {"part_end": 2}), (EINVAL, "tile parts", {"part_begin": 1, "part_end": 0})]
    e = "grf_gram_sparse_sym"
    base(e, n_total=nt, **g, t_split=None, t_rowshift=shift, K=K, ldk=nt, **ws)
    rows("gram", e, *gram_common(e), *nulls("bad arguments", "t_rowshift"), past_int32(),
         (EUNSUPPORTED, "split", {"rec_unit": 32, "t_split": split}))
    for e in ("grf_gram_sparse_upper", "grf_gram_sparse_upper_add"):
        base(e, n_total=nt, **g, t_split=None, t_rowshift=shift, K=K, ldk=nt, part_begin=0, part_end=1, n_parts=1, **ws)
        rows("gram", e, *gram_common(e), *nulls("bad arguments", "t_rowshift"), past_int32(), *parts,
             (EUNSUPPORTED, "split", {"rec_unit": 32, "t_split": split}))
    e = "grf_gram_sparse_upper_ex"
    base(e, n_total=nt, **g, t_split=None, t_rowshift=shift, row_cuts=cuts, K=K, ldk=nt, part_begin=0, part_end=1,
         n_parts=1, add_k=0)
    rows("gram", e, *gram_common(e), *nulls("bad arguments", "t_rowshift"), past_int32(), *parts,
         (EUNSUPPORTED, "row cuts", {"rec_unit": 32}), (EHIP, "", {"row_cuts": None, "add_k": 1}))
    e = "grf_gram_sparse_upper_rec"
    base(e, rec_kind=0, n_total=nt, **g, t_split=None, t_rowshift=shift, row_cuts=None, K=K, ldk=nt, part_begin=0,
         part_end=1, n_parts=1, add_k=0)
    rows("gram", e, *gram_common(e), *nulls("bad arguments", "t_rowshift"), past_int32(), *parts, *tri,
         (EINVAL, "GRF_REC_TRIPLES needs", {"rec_kind": 1, "t_split": split}))
    e = "grf_gram_sparse_cols"
    base(e, n_cols=nt, row_begin=0, row_end=100, ptr=g["ptr"], idx=g["idx"], val=g["val"], row_shift=shift, t_rows=80,
         sym_row0=-1, band_width=64, rec_unit=128, t_desc=g["t_desc"], t_rec=g["t_rec"], t_split=None, K=K, ldk=80,
         **ws)
    rows("gram", e, *gram_common(e, total="t_rows", ld=80, nul=("ptr", "idx", "val", "row_shift", "t_desc", "t_rec", "K")),
         (EINVAL, "bad arguments", {"n_cols": 0}), (EINVAL, "bad arguments", {"n_cols": -1}),
         (EINVAL, "bad arguments", {"row_begin": -1}), (EINVAL, "bad arguments", {"row_begin": 60, "row_end": 50}),
         (EUNSUPPORTED, "int32", {"n_cols": I31}), (EUNSUPPORTED, "int32", {"t_rows": I31, "ldk": I31}),
         (EINVAL, "symmetric square", {"sym_row0": 30}), (EHIP, "", {"sym_row0": 20}),
         (EINVAL, "symmetric square", {"row_begin": 10, "sym_row0": 5}))
    e = "grf_gram_sparse_cols_padded"
    base(e, n_cols=nt, row_begin=0, row_end=100, cap=16, cnt=ptr(), idx=g["idx"], val=g["val"], row_shift=shift,
         t_rows=80, band_width=64, t_desc=g["t_desc"], t_rec=g["t_rec"], K=K, ldk=80)
    rows("gram", e, (EINVAL, "padded rows", {"cap": 0}), (EINVAL, "padded rows", {"cap": -1}),
         (EINVAL, "padded rows", {"cnt": None}), *negs("bad arguments", "t_rows", "row_begin"),
         *nulls("bad arguments", "idx", "val", "row_shift", "t_desc", "t_rec", "K"),
         (EINVAL, "bad arguments", {"n_cols": 0}), (EINVAL, "128-byte aligned", {"t_rec": g["t_rec"] + 64}),
         (EINVAL, "ldk <", {"ldk": 79}), (EUNSUPPORTED, "multiple of 64", {"band_width": 100}),
         (EUNSUPPORTED, "int32", {"n_cols": I31}),
         (EUNSUPPORTED, "32-bit record offsets", {"n_cols": 1 << 25, "t_rows": 64, "ldk": 64}))
    e = "grf_gram_row_cuts"
    base(e, n_rows=100, ptr=g["ptr"], idx=g["idx"], n_bands=2, n_cols=nt, t_desc=g["t_desc"], col_w=ptr(),
         row_cuts=cuts)
    rows("gram", e, *negs("bad arguments", "n_rows", "n_bands", "n_cols"),
         *nulls("bad arguments", "ptr", "idx", "t_desc", "col_w", "row_cuts"),
         (EUNSUPPORTED, "int32", {"n_cols": I31}), grid(n_rows=1 << 26))          # row_cuts_kernel: cdiv(n_rows, 4) x 256
    e = "grf_hub_panel"
    base(e, n_rows=100, ptr=g["ptr"], idx=g["idx"], val=g["val"], hub_pos=ptr(), P=ptr(), ldp=16)
    rows("gram", e, *negs("bad arguments", "n_rows", "ldp"), *nulls("bad arguments", "ptr", "idx", "val", "hub_pos", "P"),
         grid(n_rows=1 << 26))                                                    # hub_panel_kernel: cdiv(n_rows, 4) x 256
    e = "grf_transpose_drop_columns"
    base(e, n_bands=4, n_cols=nt, t_desc=g["t_desc"], cols=ptr(), n_drop=5)
    rows("gram", e, *negs("bad arguments", "n_bands", "n_cols", "n_drop"), *nulls("bad arguments", "t_desc", "cols"),
         (EUNSUPPORTED, "int32", {"n_cols": I31}), grid(n_drop=1 << 30))          # cdiv(n_bands n_drop, 256) x 256
    e = "grf_gram_mirror"
    base(e, n=nt, K=K, ldk=nt, max_workgroups=0)
    big_n = 5793 * 64                                                             # 5793 * 5794 / 2 blocks x 256 >= 2^32
    rows("gram", e, *negs("bad arguments", "n"), *nulls("bad arguments", "K"), (EINVAL, "bad arguments", {"ldk": nt - 1}),
         grid(n=big_n, ldk=big_n), (EHIP, "", {"n": big_n, "ldk": big_n, "max_workgroups": 1024}))

    # ------------------------------------------------------------------ row shifts
    need = S.grf_phi_row_shifts_workspace_bytes(100)
    e = "grf_phi_row_shifts"
    base(e, n_rows=100, ptr=ptr(), val=ptr(), maxabs=ptr(), row_shift=ptr(), workspace=ptr(), workspace_bytes=need)
    rows("shifts", e, *negs("bad arguments", "n_rows"),
         *nulls("bad arguments", "ptr", "val", "maxabs", "row_shift", "workspace"),
         (EINVAL, "workspace too small", {"workspace_bytes": need - 1}),
         (EUNSUPPORTED, "int32", {"n_rows": I31, "workspace_bytes": BIG}),
         grid(n_rows=1 << 26, workspace_bytes=BIG))                               # phi_row_stats_kernel: cdiv(n_rows, 4) x 256
    e = "grf_phi_row_shifts_padded"
    base(e, n_rows=100, cap=16, cnt=ptr(), val=ptr(), maxabs=ptr(), row_shift=ptr(), workspace=ptr(),
         workspace_bytes=need)
    rows("shifts", e, *negs("bad arguments", "n_rows", "cap"), (EINVAL, "bad arguments", {"cap": 0}),
         *nulls("bad arguments", "cnt", "val", "maxabs", "row_shift", "workspace"),
         (EINVAL, "workspace too small", {"workspace_bytes": need - 1}),
         (EUNSUPPORTED, "int32", {"n_rows": I31, "workspace_bytes": BIG}), grid(n_rows=1 << 26, workspace_bytes=BIG))
    e = "grf_phi_row_shifts_stats"
    base(e, n_rows=100, stats=ptr(), maxabs=ptr(), row_shift=ptr())
    rows("shifts", e, *negs("bad arguments", "n_rows"), *nulls("bad arguments", "stats", "maxabs", "row_shift"),
         (EUNSUPPORTED, "int32", {"n_rows": I31}),
         (EHIP, "", {"n_rows": (1 << 31) - 1}))   # (tr_rowshift_kernel: cdiv(n_rows, 256) x 256 fits for every int32 count)

    # ------------------------------------------------------------------ dense Gram and its producers
    A, Pl = ptr(), ptr()
    d = dict(n=nt, k_dim=64, A=A, lda=64, K=K, ldk=nt)

    def dense_common(e, upper=False, planes=False):
        return [*negs("bad arguments", "n", "k_dim"), *nulls("bad arguments", "K", *([] if planes else ["A"])),
                (EINVAL, "bad arguments", {"ldk": nt - 4}), (EUNSUPPORTED, "int32", {"n": I31, "ldk": I31 + 3}),
                *([] if planes else [(EINVAL, "bad arguments", {"lda": 48}), (EINVAL, "multiple of 16", {"lda": 72}),
                                     (EINVAL, "16-byte aligned", {"A": A + 4})]),
                *([(EHIP, "", {"ldk": nt + 2}), (EHIP, "", {"K": K + 4})] if upper else
                  [(EINVAL, "multiple of 4", {"ldk": nt + 2}), (EINVAL, "16-byte aligned", {"K": K + 4})])]

    def dense_ws(e, need, sub="256-byte aligned"):
        w = BASE[e]["workspace"]
        return [(EINVAL, "workspace", {"workspace": None}), (EINVAL, sub, {"workspace": w + 128}),
                (EINVAL, "workspace too small", {"workspace_bytes": need - 1})]

    for e in ("grf_gram_dense", "grf_gram_dense_upper", "grf_gram_dense_split_upper"):
        base(e, **d)
        rows("dense", e, *dense_common(e, upper=e.endswith("upper")))
    e = "grf_gram_dense_ws"
    need = S.grf_gram_dense_workspace_bytes(nt, 64)
    base(e, **d, workspace=ptr(), workspace_bytes=need)
    rows("dense", e, *dense_common(e), (EHIP, "", {"workspace": None, "workspace_bytes": 0}),   # (runs unsplit)
         (EHIP, "", {"workspace_bytes": need - 1}))
    e = "grf_gram_dense_split"
    need = S.grf_gram_dense_split_workspace_bytes(nt, 64)
    base(e, **d, workspace=ptr(), workspace_bytes=need)
    rows("dense", e, *dense_common(e), *dense_ws(e, need))
    e = "grf_gram_dense_planes"
    base(e, n=nt, k_dim=64, P=Pl, ldp=384, K=K, ldk=nt, workspace=ptr(), workspace_bytes=need)
    rows("dense", e, *dense_common(e, planes=True), *dense_ws(e, need), *nulls("bad arguments", "P"),
         (EINVAL, "ldp must cover", {"ldp": 368}), (EINVAL, "multiple of 16", {"ldp": 392}),
         (EINVAL, "16-byte aligned", {"P": Pl + 8}))
    e = "grf_split_planes"
    base(e, n=nt, k_dim=60, A=A, lda=64, P=Pl, ldp=384)
    rows("dense", e, *negs("bad arguments", "n", "k_dim"), *nulls("bad arguments", "A", "P"),
         (EINVAL, "lda must cover", {"lda": 60}), (EINVAL, "lda must cover", {"lda": 66}),
         (EINVAL, "A 16-byte aligned", {"A": A + 4}), (EINVAL, "ldp must cover", {"ldp": 368}),
         (EINVAL, "multiple of 16", {"ldp": 392}), (EINVAL, "P 16-byte aligned", {"P": Pl + 8}),
         grid(n=1 << 29))                                                         # cdiv(2 n kt, 256) x 256, kt = 4
    e = "grf_densify_padded_planes"
    base(e, n_rows=100, cap=16, n_cols=60, cnt=ptr(), idx=ptr(), val=ptr(), P=Pl, ldp=384)
    rows("dense", e, *negs("bad arguments", "n_rows", "cap", "n_cols"), (EINVAL, "bad arguments", {"cap": 0}),
         *nulls("bad arguments", "cnt", "idx", "val", "P"), (EINVAL, "ldp must cover", {"ldp": 368}),
         (EINVAL, "multiple of 16", {"ldp": 392}), (EINVAL, "P 16-byte aligned", {"P": Pl + 8}),
         (EUNSUPPORTED, "LDS", {"n_cols": 40961, "ldp": 96 * 2561}), grid(n_rows=1 << 24))   # n_rows x 256
    e = "grf_densify"
    base(e, n_rows=100, ptr=ptr(), idx=ptr(), val=ptr(), out=ptr(), lda=nt)
    rows("dense", e, *negs("bad arguments", "n_rows", "lda"), *nulls("bad arguments", "ptr", "out"),
         grid(n_rows=1 << 26, lda=1))                                             # densify_kernel: cdiv(n_rows, 4) x 256
    e = "grf_densify_padded"
    base(e, n_rows=100, cap=16, n_cols=nt, cnt=ptr(), idx=ptr(), val=ptr(), out=ptr(), lda=nt)
    rows("dense", e, *negs("bad arguments", "n_rows", "cap", "n_cols"), (EINVAL, "bad arguments", {"cap": 0}),
         *nulls("bad arguments", "cnt", "idx", "val", "out"), (EINVAL, "bad arguments", {"lda": nt - 4}),
         (EINVAL, "multiple of 4", {"lda": nt + 2}), (EINVAL, "16-byte aligned", {"out": BASE[e]["out"] + 4}),
         (EUNSUPPORTED, "LDS", {"lda": 40964}), grid(n_rows=1 << 24))             # densify_padded_kernel: n_rows x 256

    # ------------------------------------------------------------------ the dense step tensor
    e = "grf_dense_steps_phi"
    base(e, n=100, L=4, F=ptr(), f=ptr(), phi64=None, phi32=ptr(), lda32=112)
    rows("dense_steps", e, *negs("bad arguments", "n"), (EINVAL, "bad arguments", {"L": 0}),
         (EINVAL, "bad arguments", {"lda32": 99}), *nulls("bad arguments", "F", "f", "phi32"),
         (EUNSUPPORTED, "int32", {"n": I31, "lda32": I31}),
         grid(n=1 << 16, lda32=1 << 16))                                          # cdiv(n lda32, 256) x 256
    e = "grf_dense_steps_grad"
    need = S.grf_dense_steps_grad_workspace_bytes(100, 4)
    base(e, n=100, L=4, F=ptr(), phi64=ptr(), G=ptr(), ldg=100, grad=ptr(), workspace=ptr(), workspace_bytes=need)
    rows("dense_steps", e, *negs("bad arguments", "n"), (EINVAL, "bad arguments", {"L": 0}),
         (EINVAL, "bad arguments", {"ldg": 99}), *nulls("bad arguments", "F", "phi64", "G", "grad", "workspace"),
         (EINVAL, "workspace needs", {"workspace_bytes": need - 1}),
         (EUNSUPPORTED, "int32", {"n": I31, "ldg": I31, "workspace_bytes": BIG}),
         grid(n=1 << 18, ldg=1 << 18, workspace_bytes=BIG))                       # (n / 64)^2 x 256

    # ------------------------------------------------------------------ CSR transpose and SpMM
    e = "grf_csr_transpose"
    need = S.grf_csr_transpose_workspace_bytes(100, nt, nnz)
    base(e, n_sel=100, ptr=ptr(), idx=ptr(), val=ptr(), row_map=None, n_cols=nt, nnz=nnz, t_ptr=ptr(), t_idx=ptr(),
         t_val=ptr(), workspace=ptr(), workspace_bytes=need)
    rows("cg", e, *negs("bad arguments", "n_sel", "nnz"), (EINVAL, "bad arguments", {"n_cols": 0}),
         *nulls("bad arguments", "ptr", "t_ptr"), (EINVAL, "workspace too small", {"workspace": None}),
         (EINVAL, "workspace too small", {"workspace_bytes": need - 1}),
         (EUNSUPPORTED, "2^31", {"n_sel": 1 << 31, "workspace_bytes": BIG}),
         (EUNSUPPORTED, "2^31", {"n_cols": 1 << 31, "workspace_bytes": BIG}),
         grid(n_sel=1 << 26, workspace_bytes=BIG),                                # csr_tr_gather_kernel: cdiv(n_sel, 4) x 256
         grid(nnz=1 << 32, workspace_bytes=BIG))                                  # csr_tr_unpack_kernel: cdiv(nnz + 1, 256) x 256
    for e in ("grf_spmm_csr", "grf_spmm_csr_f64"):
        base(e, n_out=100, ptr=ptr(), idx=ptr(), val=ptr(), row_map=None, X=ptr(), ldx=8, n_rhs=8, Y=ptr(), ldy=8)
        rows("cg", e, *negs("bad arguments", "n_out", "n_rhs"), *nulls("bad arguments", "ptr", "X", "Y"),
             (EINVAL, "bad arguments", {"ldx": 7}), (EINVAL, "bad arguments", {"ldy": 7}),
             (EHIP, "", {"n_out": 1 << 40}))                                      # (a bounded grid-stride launch)

    # (the unpreconditioned Gram solves: the older modules call only one of the three, for its message)
    need = S.grf_cg_workspace_bytes(4, 8, 4)
    for e in ("grf_cg_gram_solve", "grf_cg_gram_solve_f64", "grf_cg_gram_solve_lanczos_f64"):
        lz = e.endswith("lanczos_f64")
        coef = {"coef": ptr(), "ld_coef": 4} if lz else {}
        base(e, n_sys=4, ptr=ptr(), idx=ptr(), val=ptr(), row_map=None, n_cols=8, t_ptr=ptr(), t_idx=ptr(), t_val=ptr(),
             noise=0.1, rhs=ptr(), ld_rhs=4, n_rhs=4, tolerance=1.0, max_iter=5, x=ptr(), ldx=4, workspace=ptr(),
             workspace_bytes=need, iters_out=None, resid_out=None, **coef)
        rows("cg", e, *negs("bad arguments", "n_sys"), (EINVAL, "bad arguments", {"n_sys": 0}),
             (EINVAL, "bad arguments", {"n_cols": 0}), *nulls("bad arguments", "ptr", "t_ptr", "rhs", "x"),
             (EUNSUPPORTED, "n_rhs must be in", {"n_rhs": 0}),
             (EUNSUPPORTED, "n_rhs must be in", {"n_rhs": 257, "ld_rhs": 257, "ldx": 257, "workspace_bytes": BIG,
                                                 **({"ld_coef": 257} if lz else {})}),
             (EINVAL, "noise is NaN", {"noise": NAN}),
             (EINVAL, "bad strides", {"ld_rhs": 3}), (EINVAL, "bad strides", {"ldx": 3}),
             (EINVAL, "bad strides", {"max_iter": -1}), (EINVAL, "workspace", {"workspace": None}),
             (EINVAL, "workspace", {"workspace_bytes": need - 1}),
             *([(EINVAL, "coefficient", {"coef": None}), (EINVAL, "coefficient", {"ld_coef": 3})] if lz else []))

    # ------------------------------------------------------------------ the feature algebra
    steps = [C.host_ptrs(ptr(), ptr(), ptr()) for _ in range(3)]
    holed = C.host_ptrs(ptr(), 0, ptr())
    many = [C.host_ptrs(*[ptr() for _ in range(65)]) for _ in range(3)]
    fs = dict(n_rows=100, L=3, step_ptr=steps[0], step_idx=steps[1], step_val=steps[2], f=ptr(), n_f=3)
    fcommon = [*negs("bad arguments", "n_rows"), (EINVAL, "bad arguments", {"L": 0}),
               *nulls("bad arguments", "step_ptr", "step_idx", "step_val"),
               (EUNSUPPORTED, "step matrices", {"L": 65, "step_ptr": many[0], "step_idx": many[1], "step_val": many[2]}),
               (EINVAL, "bad modulator", {"n_f": -1}), (EINVAL, "bad modulator", {"f": None}),
               (EINVAL, "step 1 has no row pointers", {"step_ptr": holed}),
               grid(n_rows=1 << 26)]                                              # phi_steps_csr_kernel: cdiv(n_rows, 4) x 256
    e = "grf_phi_steps_csr_count"
    base(e, **fs, phi_cnt=ptr())
    rows("features", e, *fcommon, (EINVAL, "phi_cnt is NULL", {"phi_cnt": None}))
    e = "grf_phi_steps_csr_fill"
    base(e, **fs, phi_ptr=ptr(), phi_idx=ptr(), phi_val=ptr(), phi_val32=None)
    rows("features", e, *fcommon, *nulls("bad outputs", "phi_ptr", "phi_idx", "phi_val"))
    e = "grf_csr_row_lengths"
    base(e, n_sel=100, ptr=ptr(), row_map=None, len=ptr())
    rows("features", e, *negs("bad arguments", "n_sel"), *nulls("bad arguments", "ptr", "len"),
         grid(n_sel=1 << 32), grid(n_sel=1 << 40))                                # csr_row_lengths_kernel: cdiv(n_sel, 256) x 256
    e = "grf_csr_gather_rows"
    base(e, n_sel=100, ptr=ptr(), idx=ptr(), val=ptr(), row_map=ptr(), out_ptr=ptr(), out_idx=ptr(), out_val=ptr())
    rows("features", e, *negs("bad arguments", "n_sel"), *nulls("bad arguments", "ptr", "row_map", "out_ptr"),
         grid(n_sel=1 << 26))                                                     # cdiv(n_sel, 4) x 256
    e = "grf_csr_rowdot"
    base(e, n_pairs=100, a_ptr=ptr(), a_idx=ptr(), a_val=ptr(), rows_a=None, b_ptr=ptr(), b_idx=ptr(), b_val=ptr(),
         rows_b=None, out=ptr())
    rows("features", e, *negs("bad arguments", "n_pairs"), *nulls("bad arguments", "a_ptr", "b_ptr", "out"),
         grid(n_pairs=1 << 26))                                                   # cdiv(n_pairs, 4) x 256
    e = "grf_csr_rows_dot_cols"
    base(e, n_sel=100, ptr=ptr(), idx=ptr(), val=ptr(), row_map=None, Z=ptr(), ldz=100, out=ptr())
    rows("features", e, *negs("bad arguments", "n_sel"), *nulls("bad arguments", "ptr", "Z", "out"),
         (EINVAL, "bad arguments", {"ldz": 99}), grid(n_sel=1 << 26, ldz=1 << 26))   # cdiv(n_sel, 4) x 256
    e = "grf_dense_to_csr_count"
    base(e, n_rows=100, n_cols=nt, K=K, ldk=nt, cnt=ptr())
    rows("features", e, *negs("bad arguments", "n_rows", "n_cols"), *nulls("bad arguments", "K", "cnt"),
         (EINVAL, "bad arguments", {"ldk": nt - 1}), (EUNSUPPORTED, "int32", {"n_cols": 1 << 31, "ldk": 1 << 31}),
         grid(n_rows=1 << 26))                                                    # dense_to_csr_kernel: cdiv(n_rows, 4) x 256
    e = "grf_dense_to_csr_fill"
    base(e, n_rows=100, n_cols=nt, K=K, ldk=nt, out_ptr=ptr(), out_idx=ptr(), out_val=ptr())
    rows("features", e, *negs("bad arguments", "n_rows", "n_cols"),
         *nulls("bad arguments", "K", "out_ptr", "out_idx", "out_val"), (EINVAL, "bad arguments", {"ldk": nt - 1}),
         (EUNSUPPORTED, "int32", {"n_cols": 1 << 31, "ldk": 1 << 31}), grid(n_rows=1 << 26))


def cases_of(family):
    build_tables()
    out = []
    for entry, change, status, sub in TABLES[family]:
        args = dict(BASE[entry])
        assert set(change) <= set(args), (entry, change)
        args.update(change)
        stream = [None] if PROTO[entry][-1:] == ["stream"] else []                # (the default stream)
        out.append(Case(entry, list(args.values()) + stream, status, sub))
    return out


FAMILIES = ["device", "laplacian", "walk", "steps", "sparse", "transpose", "gram", "shifts", "dense", "dense_steps",
            "cg", "features"]


@pytest.mark.parametrize("family", FAMILIES)
def test_argument_contracts(family):
    bad = C.failures(cases_of(family))
    assert not bad, "\n" + "\n".join(bad)


def test_every_family_is_run():
    build_tables()
    assert sorted(TABLES) == sorted(FAMILIES)


def test_every_declared_function_has_a_contract():
    """A function of include/grf.h is in a table of this module, in an older contract module (which must really
    call it), a size function or host helper checked below, or in the short list with nothing to check."""
    build_tables()
    tabled = {entry for fam in TABLES.values() for entry, _, _, _ in fam}
    assert tabled == set(BASE), sorted(tabled ^ set(BASE))
    elsewhere = set()
    for module, names in ELSEWHERE.items():
        text = open(os.path.join(ROOT, "tests", module + ".py")).read()
        for name in names:
            assert re.search(r"\blib\." + name + r"\(", text), (module, name)
            elsewhere.add(name)
    groups = [tabled, elsewhere, set(SIZE_FUNCTIONS), set(HOST_HELPERS), set(NOTHING_TO_CHECK)]
    seen = set()
    for grp in groups:
        assert not (seen & grp), sorted(seen & grp)
        seen |= grp
    declared = set(PROTO)
    assert declared - seen == set(), sorted(declared - seen)
    assert seen - declared == set(), sorted(seen - declared)
    for name in SIZE_FUNCTIONS:
        assert re.search(r"_(workspace_bytes|bytes|bound)$", name), name
    sized = {n for n in declared if re.search(r"_(workspace_bytes|bytes|bound)$", n)}
    assert sized <= set(SIZE_FUNCTIONS) | elsewhere, sorted(sized - set(SIZE_FUNCTIONS) - elsewhere)


def test_the_child_process_gives_the_same_answers():
    """The route a GPU host takes: the same calls served by the child that was started without visible devices."""
    build_tables()
    child = C._ChildLib()
    try:
        assert child.grf_device_count() == 0 and child.grf_version() == 9
        for c in cases_of("laplacian")[:6] + cases_of("walk")[:8] + cases_of("features")[:10]:
            rc = getattr(child, c.entry)(*c.args)
            want = c.status if isinstance(c.status, tuple) else (c.status,)
            assert rc in want, (c.entry, rc)
            assert rc == EHIP or c.substr.encode() in child.grf_last_error()
    finally:
        child.close()
    assert child._proc is None


def test_chunk_bounds_is_array_split():
    import numpy as np
    S = sizes()
    for n, k in [(0, 1), (1, 1), (10, 3), (100, 7), (5, 8), ((1 << 31) - 1, 1000)]:
        got = [S.grf_chunk_bounds(n, k, c) for c in range(k + 1)]
        assert got[0] == 0 and got[-1] == n and got == sorted(got)
        if n <= 100:
            want = np.cumsum([0] + [len(x) for x in np.array_split(np.arange(n), k)]).tolist()
            assert got == want
    assert S.grf_chunk_bounds(10, 0, 0) == 0 and S.grf_chunk_bounds(10, -3, 1) == 0


# ---------------------------------------------------------------------- size and bound functions
SAT = (1 << 64) - 1                             # size_t functions saturate beyond their entry's domain
NS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 4095, 4096, 4097, 65535, 65536, 65537, (1 << 20) - 1,
      1 << 20, (1 << 24) + 1, (1 << 26) - 1, 1 << 26, (1 << 30) - 1, 1 << 30, (1 << 31) - 1]
BEYOND = [1 << 31, (1 << 32) + 1, 1 << 40, 1 << 61, 1 << 62, (1 << 63) - 1]      # past the int32 ids
BEYOND_ENTRIES = [(1 << 40) + 1, 1 << 61, 1 << 62, (1 << 63) - 1]                 # past the entry counts (nnz, buckets)


def al256(x):
    return (x + 255) & ~255


def scan_bytes(n):
    """The scan's scratch: two partials per 4096-element tile (+ 1), recursively."""
    nb = -(-n // 4096)
    return 0 if nb <= 1 else 8 * (2 * nb + 1) + scan_bytes(nb)


def monotone(values, what):
    assert values == sorted(values), what


def test_size_functions_of_one_size():
    S = sizes()
    lower = {
        "grf_laplacian_csr_workspace_bytes": lambda n: al256(4 * max(n, 1)) + scan_bytes(n),
        "grf_laplacian_dense_workspace_bytes": lambda n: max(n, 1) * (8 + 4 + 127 * 12 + 8) + 256,
        "grf_walk_aug_bytes": lambda n: 32 + 32 * n,
        "grf_scan_workspace_bytes": scan_bytes,
        "grf_transpose_workspace_bytes": lambda n: 2 * al256(4 * n) + al256(8 * (n + 1)) + scan_bytes(n),
        "grf_phi_row_shifts_workspace_bytes": lambda n: 12 * max(n, 1) + max(n, 1),
    }
    for name, low in lower.items():
        fn = getattr(S, name)
        vals = [fn(n) for n in NS]
        monotone(vals, name)
        for n, v in zip(NS, vals):
            assert low(n) <= v < 1 << 48, (name, n, v)
        assert all(v > 0 for v in vals) or name == "grf_scan_workspace_bytes", name
        assert fn(-1) == fn(0) and fn(-(1 << 62)) == fn(0), name                 # (a negative size is refused by the entry)
        counts_entries = name in ("grf_walk_aug_bytes", "grf_scan_workspace_bytes", "grf_transpose_workspace_bytes")
        for n in BEYOND_ENTRIES if counts_entries else BEYOND:                    # never a small wrapped value
            assert fn(n) == SAT, (name, n, fn(n))
        if counts_entries:
            big = [fn(n) for n in (1 << 31, 1 << 36, 1 << 40)]
            assert big == sorted(big) and vals[-1] <= big[0] and low(1 << 40) <= big[-1] < 1 << 62, name
    assert S.grf_scan_workspace_bytes(4096) == 0 and S.grf_scan_workspace_bytes(4097) == scan_bytes(4097) > 0
    assert S.grf_gram_workspace_bytes() == 256
    # grf_planes_row_bytes (int64): 96 bytes per k-tile of 16
    vals = [S.grf_planes_row_bytes(k) for k in NS]
    assert vals == [96 * -(-k // 16) for k in NS]
    assert S.grf_planes_row_bytes(-1) == 0 and S.grf_planes_row_bytes(-(1 << 40)) == 0
    for k in BEYOND:
        assert S.grf_planes_row_bytes(k) == (1 << 63) - 1, k


def dense_gram_slabs(n, k, wide):
    """The 64 KiB slabs (128 x 128 floats) the dense Grams' workspace holds after its 4 KiB ticket block, as
    include/grf.h's size functions bound them from the tile and k-tile counts alone: every tile in <= min(4, k-tiles)
    pieces and at most one piece per slot below 512 tiles (2 slots per CU, 256 CUs), a tail of <= 1023 tiles in
    <= 3 pieces from there on; two slabs per stream-K slot; two double slabs per CU for the wide items."""
    nt = -(-n // 128)
    tiles, kt = nt * (nt + 1) // 2, -(-k // 16)
    units = max(tiles * kt, 1)
    per_tile = min(tiles * min(4, kt), 512) if tiles < 512 else 1023 * min(3, kt)
    return max(per_tile, 2 * min(512, units), 4 * min(256, units) if wide else 0)


def test_size_functions_of_the_dense_gram_and_the_step_tensor():
    S = sizes()
    # every tile count from 1 to past the 512-tile change of plan, the wide plan's threshold (8064 / 8065), and up
    ns = sorted(set(range(0, 4300, 61)) | {1, 127, 128, 129, 255, 256, 257, 3968, 3969, 4096, 4097, 5000, 6000, 7000,
                                             8064, 8065, 8192, 10000, 65536, (1 << 20) + 1, (1 << 31) - 1})
    ks = [0, 1, 15, 16, 17, 31, 32, 33, 48, 49, 64, 65, 200, 500, 1000, 4096, 65536, (1 << 31) - 1]
    for name, wide in (("grf_gram_dense_workspace_bytes", False), ("grf_gram_dense_split_workspace_bytes", True)):
        fn = getattr(S, name)
        table = {(n, k): fn(n, k) for n in ns for k in ks}
        for k in ks:
            monotone([table[n, k] for n in ns], (name, "n", k))
        for n in ns:
            monotone([table[n, k] for k in ks], (name, "k_dim", n))
        for (n, k), v in table.items():
            low = 16 if n == 0 else 4096 + 65536 * dense_gram_slabs(n, k, wide)
            assert low <= v <= max(low, 4096 + 65536 * 3069), (name, n, k, v, low)
        for n in BEYOND:
            assert fn(n, 64) == SAT and fn(64, n) == SAT, (name, n)
        assert fn(-1, 64) == fn(0, 64) == 16, name
    for n in ns:                                      # (the split entries' workspace also serves the fp32 ones)
        assert S.grf_gram_dense_split_workspace_bytes(n, 64) >= S.grf_gram_dense_workspace_bytes(n, 64), n
    fn = S.grf_dense_steps_grad_workspace_bytes
    ns = [0, 1, 63, 64, 65, 127, 128, 129, 1000, 4096, 65536, (1 << 18) - 1, 1 << 18, (1 << 20) + 1, 1 << 30, (1 << 31) - 1]
    Ls = [1, 2, 3, 4, 64, 2048, 1 << 20, 1 << 30, (1 << 31) - 1]
    low = lambda n, L: 8 * L * (-(-max(n, 1) // 64)) ** 2  # noqa: E731  (one double per 64 x 64 block and step)
    for L in Ls:
        vals = [fn(n, L) for n in ns]
        monotone(vals, L)
        for n, v in zip(ns, vals):                    # the product itself, or saturated where it does not fit size_t
            assert v == (low(n, L) if low(n, L) < 1 << 64 else SAT) and v > 0, (n, L, v)
    for n in ns:
        monotone([fn(n, L) for L in Ls], n)
    assert fn((1 << 31) - 1, 2048) == SAT and fn(1 << 30, 1 << 30) == SAT       # (2^50 blocks x L x 8 wraps)
    assert fn(-1, 4) == fn(0, 4) and fn(100, 0) == fn(100, 1) == fn(100, -7)
    for n in BEYOND:
        assert fn(n, 4) == SAT, n


def test_size_functions_of_the_transposes():
    S = sizes()
    rows_ = [0, 1, 63, 64, 65, 8191, 8192, 8193, 70001, 1 << 20, (1 << 26) - 1]
    cols_ = [1, 127, 128, 129, 4097, 70001, 1 << 20, (1 << 31) - 1]
    bands = [64, 128, 1024, 4096, 8192]
    nnzs = [0, 1, 1000, 1 << 20, (1 << 31) - 1, 1 << 36]
    for bw in bands:
        for nc in cols_:
            ws = [S.grf_transpose_self_workspace_bytes(nr, nc, bw) for nr in rows_]
            monotone(ws, ("self_ws rows", nc, bw))
            for nr, v in zip(rows_, ws):
                nb = -(-max(nr, 1) // bw)
                assert 4 * max(nr, 1) + 4 * nb * nc <= v < 1 << 56, (nr, nc, bw, v)
        for nr in rows_:
            for nnz in (0, 1000, 1 << 36):
                st = [S.grf_transpose_staging_bytes(nr, nc, bw, nnz) for nc in cols_]
                assert all(v >= 8 * nnz + 8 * max(nr, 1) + 4 * max(-(-nr // 16), 1) for v in st), (nr, bw, nnz)
            st = [S.grf_transpose_staging_bytes(nr, 70001, bw, nnz) for nnz in nnzs]
            monotone(st, ("staging nnz", nr, bw))
    for unit, per in ((128, 128), (12, 12), (32, 32)):
        for bw in bands:
            for nr, nc in [(0, 1), (1, 1), (200, 300), (8193, 4097), (70001, 70001), (1 << 20, 1 << 20)]:
                nbk = -(-max(nr, 1) // bw) * nc
                ub = [S.grf_transpose_self_units_bound(nr, nc, bw, unit, nnz) for nnz in nnzs]
                monotone(ub, ("units nnz", unit, bw, nr, nc))
                for nnz, v in zip(nnzs, ub):
                    # every entry is 6 bytes of a pair; a line bucket rounds up to whole lines, a slot bucket has its slot
                    low = {128: max(-(-6 * nnz // 128), 1), 12: max(nnz // 2, 1), 32: nbk + 6 * nnz // 32}[unit]
                    assert low <= v < 1 << 62, (unit, bw, nr, nc, nnz, v)
                if unit == 128:
                    tl = [S.grf_transpose_self_triples_lines_bound(nr, nc, bw, nnz) for nnz in nnzs]
                    monotone(tl, ("triples nnz", bw, nr, nc))
                    for nnz, v in zip(nnzs, tl):
                        assert max(-(-nnz // 24), 1) <= v < 1 << 62, (bw, nr, nc, nnz, v)   # 3 entries per 16 bytes
    # the degenerate sizes the entries refuse, and sizes beyond them: never a small wrapped value
    assert S.grf_transpose_staging_bytes(100, 0, 64, 10) == 0 and S.grf_transpose_staging_bytes(100, 10, 0, 10) == 0
    assert S.grf_transpose_self_workspace_bytes(100, 0, 64) == 16
    for n in BEYOND:
        assert S.grf_transpose_self_workspace_bytes(n, 300, 64) == SAT and S.grf_transpose_self_workspace_bytes(200, n, 64) == SAT
        assert S.grf_transpose_staging_bytes(n, 300, 64, 1000) == SAT and S.grf_transpose_staging_bytes(200, n, 64, 1000) == SAT
        assert S.grf_transpose_self_units_bound(n, 300, 64, 128, 1000) == (1 << 63) - 1
        assert S.grf_transpose_self_units_bound(200, n, 64, 128, 1000) == (1 << 63) - 1
        assert S.grf_transpose_self_triples_lines_bound(n, 300, 64, 1000) == (1 << 63) - 1
        assert S.grf_transpose_self_triples_lines_bound(200, n, 64, 1000) == (1 << 63) - 1
    for nnz in (1 << 61, 1 << 62, (1 << 63) - 1):
        assert S.grf_transpose_staging_bytes(200, 300, 64, nnz) == SAT
        assert S.grf_transpose_self_units_bound(200, 300, 64, 128, nnz) == (1 << 63) - 1
        assert S.grf_transpose_self_triples_lines_bound(200, 300, 64, nnz) == (1 << 63) - 1


def test_size_function_of_the_csr_transpose():
    S = sizes()
    fn = S.grf_csr_transpose_workspace_bytes
    ns = [0, 1, 255, 256, 4096, 4097, 70001, 1 << 20, (1 << 31) - 1]
    zs = [0, 1, 1000, 1 << 20, (1 << 31) - 1, 1 << 32, 1 << 36]
    for nc in (1, 255, 256, 257, 70001, (1 << 31) - 1):
        for z in zs:
            vals = [fn(n, nc, z) for n in ns]
            monotone(vals, ("n_sel", nc, z))
            for n, v in zip(ns, vals):
                assert 12 * (n + 1) + scan_bytes(n + 1) + 24 * max(z, 1) <= v < 1 << 48, (n, nc, z, v)
        for n in ns:
            monotone([fn(n, nc, z) for z in zs], ("nnz", n, nc))
    for n in BEYOND:
        assert fn(n, 300, 1000) == SAT and fn(100, n, 1000) == SAT, n
    for z in (1 << 60, 1 << 62, (1 << 63) - 1):
        assert fn(100, 300, z) == SAT, z
    assert fn(-1, 300, 10) == fn(0, 300, 10) and fn(100, 300, -5) == fn(100, 300, 0)


def test_size_functions_of_the_older_modules_are_positive_and_monotone():
    """(Their argument checks live in their own modules; here only the common shape on the common grid.)"""
    S = sizes()
    ns = [1, 2, 63, 64, 65, 257, 4097, 70001, 1 << 20]
    for name, call in [
        ("grf_cg_workspace_bytes", lambda n: S.grf_cg_workspace_bytes(n, n, 8)),
        ("grf_pcg_workspace_bytes", lambda n: S.grf_pcg_workspace_bytes(n, n, 8)),
        ("grf_cg_poly_workspace_bytes", lambda n: S.grf_cg_poly_workspace_bytes(n, n, 8)),
        ("grf_pcg_poly_workspace_bytes", lambda n: S.grf_pcg_poly_workspace_bytes(n, n, 8)),
        ("grf_poly_workspace_bytes", lambda n: S.grf_poly_workspace_bytes(n, 4, 8)),
        ("grf_poly_grad_workspace_bytes", lambda n: S.grf_poly_grad_workspace_bytes(n, 8)),
        ("grf_poly_kernel_block_workspace_bytes", lambda n: S.grf_poly_kernel_block_workspace_bytes(n, 4, 8)),
        ("grf_poly_kernel_diag_workspace_bytes", lambda n: S.grf_poly_kernel_diag_workspace_bytes(n, 4, 8)),
        ("grf_poly_kernel_grad_workspace_bytes", lambda n: S.grf_poly_kernel_grad_workspace_bytes(n, 8, 8, 0)),
        ("grf_steps_frob_workspace_bytes", lambda n: S.grf_steps_frob_workspace_bytes(n, 4)),
        ("grf_spgemm_workspace_bytes", lambda n: S.grf_spgemm_workspace_bytes(n, n, n)),
        ("grf_gemm_nt_f64_workspace_bytes", lambda n: S.grf_gemm_nt_f64_workspace_bytes(n, n)),
        ("grf_posterior_reduce_workspace_bytes", lambda n: S.grf_posterior_reduce_workspace_bytes(n, 8)),
    ]:
        vals = [call(n) for n in ns]
        assert all(v > 0 for v in vals), name
        monotone(vals, name)
    vals = [S.grf_expm_sym_f64_workspace_bytes(n) for n in (1, 2, 63, 64, 65, 257, 4097)]
    assert all(v >= 3 * 8 * n * n for v, n in zip(vals, (1, 2, 63, 64, 65, 257, 4097))) and vals == sorted(vals)
