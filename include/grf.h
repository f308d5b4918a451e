/*
 * grf.h -- C ABI of the MI355X (gfx950) Graph Random Features engine.
 *
 * Every compute entry point is asynchronous on the HIP stream it is given,
 * takes DEVICE pointers (allocated by the caller, e.g. torch tensors on
 * cuda:N), plain integer sizes and no C++ / torch types.  Return value:
 * GRF_OK (0) or a negative grf_status; the message of the last failure on
 * the calling thread is in grf_last_error().  No exception crosses the ABI.
 * Buffers whose size depends on the data are bounded by documented caps
 * (`*_cap` arguments) so that no entry point needs a host round trip.
 *
 * Argument checks.  Every entry checks its arguments on the host before anything touches a device; a refused
 * call launches nothing, writes nothing and leaves its reason in grf_last_error():
 *   GRF_EINVAL        a negative size or capacity; a NULL pointer to an array of fixed size (row pointers of
 *                     n + 1, per-row inputs and outputs, parameter structs, a workspace that is needed); a leading
 *                     dimension below the width; a broken alignment rule (stated per entry: 8, 16, 32, 128 or 256
 *                     bytes); a workspace that is NULL or shorter than its *_workspace_bytes; an enum or scalar
 *                     out of range (p_halt outside [0, 1), walks_per_node < 1, NaN, a PCG64 source range that is
 *                     not whole chunks, ...).
 *   GRF_EUNSUPPORTED  a node, row or column count past the int32 ids the CSR arrays hold (> 2^31 - 1); a launch
 *                     of 2^32 or more work-items (split the input); a band_width that is not a multiple of 64 in
 *                     [64, 8192] where the entry bins by bands; a variant this build does not have.
 *   GRF_ECAPACITY     a capacity the host can check is short (t_rec_bytes below the units bound).
 * NULL when empty.  Arrays whose length depends on the data -- a CSR's idx / val, out_idx / out_val, t_idx /
 * t_val, the records t_rec point at -- hold no element when there are no entries, and callers (the Python engine:
 * the data pointer of an empty tensor) pass NULL for them then.  Entries that do not already insist on them must
 * therefore not be given new NULL checks for these arrays; they are never read or written when empty.
 * Size functions are pure host functions.  Those of the Laplacians, grf_walk_aug, the scan, the banded transposes
 * (workspace, staging, units and lines bounds), grf_phi_row_shifts, the dense Grams (grf_gram_dense_workspace_bytes,
 * grf_gram_dense_split_workspace_bytes, grf_planes_row_bytes), grf_dense_steps_grad and grf_csr_transpose are
 * monotone in every argument over the sizes their entry accepts (a workspace sized for the largest problem serves
 * every smaller one), count a negative size as 0, and saturate: an argument beyond the entry's domain -- a node /
 * row / column count > 2^31 - 1, an entry or bucket count (nnz, n_buckets) > 2^40 -- or a product that would wrap
 * gives SIZE_MAX (INT64_MAX for the int64 bounds), never a small wrapped value.  (The size functions of the CG,
 * polynomial, SpGEMM, expm, posterior and steps_frob entries are specified with those entries and make no such
 * promise beyond their entries' domains.)
 *
 * The reference has no FFI: its boundary is a set of Python functions
 * (SURVEY.md §8b).  Each entry point below replaces the reference routine
 * cited next to it (paths relative to the reference checkout).
 */
#ifndef GRF_H
#define GRF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *grf_stream_t; /* hipStream_t; NULL = default stream */

enum grf_status {
    GRF_OK = 0,
    GRF_EINVAL = -1,      /* bad argument (reference: ValueError / AssertionError) */
    GRF_EHIP = -2,        /* HIP runtime / launch failure                           */
    GRF_ECAPACITY = -3,   /* an output cap was too small                            */
    GRF_EUNSUPPORTED = -4 /* size outside what this build handles                   */
};

/* Record unit of the banded transpose (bytes per descriptor unit) */
enum grf_rec_unit {
    GRF_REC_LINE = 128,  /* every bucket starts on a 128-byte line: dense buckets (C4)      */
    GRF_REC_PACKED = 12, /* buckets packed pair after pair: sparse buckets (C5, N = 1M)     */
    GRF_REC_SLOT = 32    /* one 32-byte slot per bucket: {u32 pairs, u32 first overflow pair,
                            the first two pairs inline}, the rest packed after all the slots:
                            the Gram reads a small bucket with its header in ONE line
                            (grf_transpose_banded_self and the 8-wave Gram tiles only)           */
};

/* Laplacian semantics */
enum grf_laplacian_mode {
    GRF_LAP_SCIPY = 0,         /* utils_sparse/graph_utils.py:5-30  (D^-1/2 (D-A) D^-1/2, scipy order) */
    GRF_LAP_NUMPY = 1,         /* graph_kernels/utils.py:21-26      (I - D^-1/2 W D^-1/2, dinv=0 at deg<=0) */
    GRF_LAP_NUMPY_SAFE = 2,    /* preprocessing/laplacian_np.py:13-20 (safe degrees)                   */
    GRF_LAP_COMBINATORIAL = 3, /* preprocessing/laplacian_np.py:32-34 (D - W)                          */
    GRF_LAP_NONE = 4           /* walk the matrix as given (RandomWalk(Graph(adj)))                    */
};

enum grf_rng {
    GRF_RNG_PCG64 = 0, /* numpy PCG64 stream replay, one sequential stream per chunk (reference-exact) */
    GRF_RNG_PHILOX = 1 /* Philox4x32-10 keyed (seed), counter (step pair, walk, source, block)     */
};

enum grf_load_rule {
    GRF_LOAD_CUMULATIVE = 0,    /* load *= deg*w/(1-p)   sparse_sampler.py:54, sampler.py:58 */
    GRF_LOAD_NONCUMULATIVE = 1, /* load  = deg*w/(1-p)   sampler.py:183                      */
    GRF_LOAD_ABLATION = 2       /* load  = w             sampler.py:180-181                  */
};

enum grf_norm {
    GRF_NORM_DIV = 0,      /* value / m       (sampler.py:201)                          */
    GRF_NORM_MUL_RECIP = 1 /* value * (1/m)   (sparse_sampler.py:130 via scipy _mul_scalar) */
};

/* The ABI revision of this header: grf_version() returns it, and a binding must refuse a library whose
 * revision differs (argument lists, or -- ABI 7 -- the GRF_RNG_PHILOX stream, change between revisions;
 * ABI 8 added grf_phi_row_shifts_padded and grf_gram_sparse_cols_padded; ABI 9 the marginal likelihood's
 * grf_cg_gram_solve_lanczos_f64 and grf_steps_frob_f64; grf_spgemm_* and the record kinds' *_rec entries came
 * later, as did the diagonally preconditioned grf_pcg_* solves and grf_gram_jacobi_f64, purely additive: no
 * argument list of revision 9 changed, so the revision stays). */
#define GRF_ABI_VERSION 9

const char *grf_last_error(void);
int32_t grf_version(void);
/* number of HIP devices visible (0 if none); never fails */
int32_t grf_device_count(void);
/* select the device for subsequent calls on this host thread */
int32_t grf_set_device(int32_t device); /* device < 0: GRF_EINVAL */

/* ------------------------------------------------------------------ Laplacian
 * Replaces efficient_graph_gp_sparse/utils_sparse/graph_utils.py:5-30
 * (get_normalized_laplacian, sparse) for mode GRF_LAP_SCIPY.
 * In : A (n x n CSR, canonical: sorted, no duplicates): a_ptr[n+1] (int64),
 *      a_idx[nnz] (int32), a_val[nnz] (float64).
 * Out: l_ptr[n+1], l_idx[l_cap], l_val[l_cap] with l_cap >= nnz(A) + n;
 *      deg[n], dinv[n] (float64, scratch + diagnostics).  Columns ascending.
 * n <= 2^31 - 1 (GRF_EUNSUPPORTED beyond); mode must be GRF_LAP_SCIPY (GRF_EUNSUPPORTED otherwise); workspace:
 * grf_laplacian_csr_workspace_bytes(n) bytes, not NULL.  n == 0 writes l_ptr[0] = 0 and nothing else.
 * Truncation rule (both Laplacians): l_cap is a data-dependent cap, so a short one is not an error the host can
 * see.  l_ptr is always the FULL row pointer (l_ptr[n] = the entries the result has); an entry whose position is
 * >= l_cap is not written (every store to l_idx / l_val is behind `position < l_cap`), so the words at and past
 * l_cap are untouched and the entries below l_cap are the exact prefix of the full result.  The caller compares
 * l_ptr[n] with l_cap. */
int32_t grf_laplacian_csr(int64_t n, const int64_t *a_ptr, const int32_t *a_idx, const double *a_val, int32_t mode,
                          int64_t *l_ptr, int32_t *l_idx, double *l_val, int64_t l_cap, double *deg, double *dinv,
                          void *workspace, size_t workspace_bytes, grf_stream_t stream);

size_t grf_laplacian_csr_workspace_bytes(int64_t n);

/* Replaces efficient_graph_gp/graph_kernels/utils.py:6-28 and
 * efficient_graph_gp/preprocessing/laplacian_np.py:3-35 followed by the
 * neighbour scan np.flatnonzero(L[row]) of random_walk_samplers/sampler.py:22-28.
 * In : W dense row-major n x n float64.  mode: NUMPY / NUMPY_SAFE / COMBINATORIAL / NONE.
 * Out: the walk matrix as CSR of its nonzeros (ascending columns), l_cap >= nnz (truncation rule above).
 * n < 2^31 - 1 (GRF_EUNSUPPORTED beyond); a mode other than the four is GRF_EINVAL; W 8-byte aligned; workspace:
 * grf_laplacian_dense_workspace_bytes(n) bytes, 256-byte aligned, not NULL.  n == 0 writes l_ptr[0] = 0 only. */
int32_t grf_laplacian_dense(int64_t n, const double *W, int32_t mode, int64_t *l_ptr, int32_t *l_idx, double *l_val,
                            int64_t l_cap, double *deg, void *workspace, size_t workspace_bytes, grf_stream_t stream);

size_t grf_laplacian_dense_workspace_bytes(int64_t n);

/* --------------------------------------------------------------------- walks
 * Replaces the walk loops of
 *   efficient_graph_gp_sparse/random_walk_samplers_sparse/sparse_sampler.py:26-56 and
 *   efficient_graph_gp/random_walk_samplers/sampler.py:30-61,148-186.
 * Walks on the CSR (g_ptr, g_idx, g_val).  Records visit slots
 *   slot_node[(s - src_begin) * L * m + l * m + w] (int32, -1 = no visit),
 *   slot_load[same]                                   (float64)
 * for sources s in [src_begin, src_end).
 * RNG GRF_RNG_PHILOX: key = seed (64 bit).  Any [src_begin, src_end).  Block (l / 2, w, s, 0) of
 *   Philox4x32-10 serves steps l = 2j, 2j + 1 of walk (s, w): the even step halts iff x0 < ceil(p 2^32)
 *   and takes neighbour Lemire(x1, deg), the odd step uses x2 and x3; a Lemire rejection of step l
 *   continues on blocks (l, w, s, 1), (l, w, s, 2), ...; the L-th recorded visit draws nothing.
 * RNG GRF_RNG_PCG64 : chunks = np.array_split(arange(n), n_chunks); chunk c is one
 *   numpy default_rng(seed + c) stream; [src_begin, src_end) must be a union of
 *   whole chunks (use grf_chunk_bounds), n_chunks >= 1.
 * Checked (GRF_EINVAL): params not NULL, walks_per_node in [1, 2^31), max_walk_length >= 1, p_halt in [0, 1) (a NaN
 * is refused), load_rule and rng in their enums, 0 <= src_begin <= src_end <= n, g_aug 32-byte aligned; n <=
 * 2^31 - 1 and (src_end - src_begin) * walks_per_node < 2^32 else GRF_EUNSUPPORTED.  No sources: nothing written. */
typedef struct grf_walk_params {
    int64_t walks_per_node; /* m                     */
    double p_halt;          /* p                     */
    int32_t max_walk_length;/* L                     */
    int32_t load_rule;      /* enum grf_load_rule    */
    int32_t rng;            /* enum grf_rng          */
    int32_t reserved;
    int64_t n_chunks;       /* PCG64 only            */
    uint64_t seed;          /* PCG64: chunk c seeded with seed + c; Philox: key */
} grf_walk_params;

int32_t grf_walk(int64_t n, const int64_t *g_ptr, const int32_t *g_idx, const double *g_val,
                 const grf_walk_params *params, int64_t src_begin, int64_t src_end, int32_t *slot_node,
                 double *slot_load, grf_stream_t stream);
/* grf_walk with the augmented walk matrix (grf_walk_aug of the same walk matrix; NULL: grf_walk):
 * each step is one dependent memory round trip instead of two; the same draws, bit-identical slots in
 * both RNG modes (the PCG64 replay's one lane per chunk is latency-bound on exactly that chain). */
int32_t grf_walk_ex(int64_t n, const int64_t *g_ptr, const int32_t *g_idx, const double *g_val, const void *g_aug,
                    const grf_walk_params *params, int64_t src_begin, int64_t src_end, int32_t *slot_node,
                    double *slot_load, grf_stream_t stream);

/* host helper: first source of chunk c (np.array_split boundaries) */
int64_t grf_chunk_bounds(int64_t n, int64_t n_chunks, int64_t c);

/* ------------------------------------------------------- per-step occupancy
 * Replaces the accumulate/normalise part of sparse_sampler.py:36-47,107-130 and
 * sampler.py:137-146,188-203: for every (source, step) the distinct visited nodes
 * (ascending) with value = (sum of loads in walk order) normalised by `norm`.
 * Out (padded rows, row capacity m): step_cnt[ns*L], step_idx[ns*L*m],
 * step_val[ns*L*m] at row (s_local * L + l).  Explicit zeros are kept.
 * m in [1, 16384] (GRF_EUNSUPPORTED above), L >= 1, norm in its enum; n_src == 0 writes nothing. */
int32_t grf_steps(int64_t n_src, int64_t m, int32_t L, int32_t norm, const int32_t *slot_node,
                  const double *slot_load, int32_t *step_cnt, int32_t *step_idx, double *step_val,
                  grf_stream_t stream);

/* Dense (N, N, L) feature tensor of RandomWalk.get_random_walk_matrices
 * (sampler.py:188-203): out[(s * n_cols + j) * L + l] = step value; out must be
 * zero-filled by the caller.  n_cols <= 2^31 - 1. */
int32_t grf_steps_densify(int64_t n_src, int64_t m, int32_t L, int64_t n_cols, const int32_t *step_cnt,
                          const int32_t *step_idx, const double *step_val, double *out, grf_stream_t stream);

/* ------------------------------------------------------------------------ Phi
 * Replaces efficient_graph_gp_sparse/graph_kernels_sparse/fast_grf_kernel_general.py:47-52
 * (Phi = sum_l f_l M_l, exact zeros dropped; steps l < min(n_f, L)).
 * From padded step rows (grf_steps output).  Out: padded Phi rows with capacity
 * phi_cap >= min(m * L, n): phi_cnt[ns], phi_idx[ns*phi_cap], phi_val[ns*phi_cap]
 * (float64), and optionally phi_val32 (float32 copy, may be NULL).
 * L <= 64 (GRF_EUNSUPPORTED above); phi_cap >= 1; n_f >= 0 with f not NULL unless n_f == 0 (grf_phi_fused and
 * grf_walk_phi alike).  A row longer than phi_cap is cut at phi_cap entries (phi_cnt holds what was written). */
int32_t grf_phi(int64_t n_src, int64_t m, int32_t L, const int32_t *step_cnt, const int32_t *step_idx,
                const double *step_val, const double *f, int32_t n_f, int64_t phi_cap, int32_t *phi_cnt,
                int32_t *phi_idx, double *phi_val, float *phi_val32, grf_stream_t stream);

/* Fused slots -> Phi (no step rows), same result bit-for-bit as grf_steps + grf_phi.
 * Requires m * L <= 4096.  norm as in grf_steps. */
/* Philox walks of the sources [src_begin, src_end) straight to Phi rows in one kernel (the
 * visit slots never touch HBM): bit-identical to grf_walk (params->rng = GRF_RNG_PHILOX)
 * followed by grf_phi_fused.  Requires m * L <= 4096.
 * Optional (t_count != NULL): also count the banded transpose's buckets of the rows written,
 * t_count[((row - count_row0) / band_width) * n + col] += 1 -- pass the transpose workspace (zeroed)
 * and then grf_transpose_banded_plan(..., counted = 1, ...); phi_cap must not truncate rows.
 * count_row0 (<= src_begin) is the first row of the transposed matrix: 0 for all of Phi, src_begin
 * for a transpose of these rows alone (the column-block multi-GPU Gram). 
 * phi_val (float64) may be NULL when phi_val32 is given: only the float32 copy is written. 
 * Optional (g_aug != NULL, from grf_walk_aug on the same walk matrix, nnz < 2^32): each step of a
 * walk is one dependent memory round trip instead of two -- same draws, same Phi bits. */
int32_t grf_walk_phi(int64_t n, const int64_t *g_ptr, const int32_t *g_idx, const double *g_val, const void *g_aug,
                     const grf_walk_params *params, int64_t src_begin, int64_t src_end, int32_t norm, const double *f,
                     int32_t n_f, int64_t phi_cap, int32_t *phi_cnt, int32_t *phi_idx, double *phi_val,
                     float *phi_val32, int32_t *t_count, int64_t band_width, int64_t count_row0,
                     grf_stream_t stream);
/* The augmented walk matrix of grf_walk_phi (opaque to the caller): a 32-byte header, then one
 * record per entry e of the CSR walk matrix (g_ptr, g_idx, g_val) holding the target v, the row
 * start and row length of v and the weight g_val[e] -- 16 bytes ({v, row start, length} packed
 * into 64 bits, float64 weight) when the node ids, row starts and lengths fit 64 bits together,
 * else 32 bytes; one record per walk step either way.  grf_walk_aug_bytes(nnz) bytes (enough for
 * both), 32-byte aligned. */
int32_t grf_walk_aug(int64_t n, const int64_t *g_ptr, const int32_t *g_idx, const double *g_val, void *g_aug,
                     grf_stream_t stream);
size_t grf_walk_aug_bytes(int64_t nnz);
int32_t grf_phi_fused(int64_t n_src, int64_t m, int32_t L, int32_t norm, const int32_t *slot_node,
                      const double *slot_load, const double *f, int32_t n_f, int64_t phi_cap, int32_t *phi_cnt,
                      int32_t *phi_idx, double *phi_val, float *phi_val32, grf_stream_t stream);

/* --------------------------------------------------------- sparse utilities */
/* exclusive scan of int32 counts -> int64 row pointers out[n+1] (n == 0: out[0] = 0).  workspace:
 * grf_scan_workspace_bytes(n) bytes -- 0 up to one tile of 4096 counts, where NULL is accepted. */
int32_t grf_scan_counts(int64_t n, const int32_t *cnt, int64_t *out_ptr, void *workspace, size_t workspace_bytes,
                        grf_stream_t stream);
size_t grf_scan_workspace_bytes(int64_t n);
/* padded rows (row r at r*cap, cnt[r] entries) -> compact CSR using out_ptr from grf_scan_counts.
 * Any of the value arrays may be NULL. */
int32_t grf_compact_rows(int64_t n_rows, int64_t cap, const int32_t *cnt, const int64_t *out_ptr,
                         const int32_t *in_idx, const double *in_val, const float *in_val32, int32_t *out_idx,
                         double *out_val, float *out_val32, grf_stream_t stream);
/* (n_rows, cap >= 0; cnt, out_ptr, in_idx, out_idx not NULL; an output array needs its input array.)
 * grf_compact_rows (float values required) that also writes the rows' Gram shift statistics into
 * `stats` (grf_phi_row_shifts_workspace_bytes(n_rows) bytes) for grf_phi_row_shifts_stats. */
int32_t grf_compact_rows_stats(int64_t n_rows, int64_t cap, const int32_t *cnt, const int64_t *out_ptr,
                               const int32_t *in_idx, const double *in_val, const float *in_val32, int32_t *out_idx,
                               double *out_val, float *out_val32, void *stats, size_t stats_bytes,
                               grf_stream_t stream);

/* dst[dst_off[r] + i] = src[r * stride + i] for i < seg_len[r], r < n_seg (4-byte elements; lengths
 * and offsets are device arrays): the compaction of a fixed-stride all-gather of n_seg ranks'
 * CSR segments (the multi-GPU Phi gather, grf_amd/dist.py) without reading any size back.
 * n_seg in [0, 65535], stride >= 0; n_seg == 0 or stride == 0 touches nothing. */
int32_t grf_concat_segments(int32_t n_seg, int64_t stride, const void *src, const int64_t *seg_len,
                            const int64_t *dst_off, void *dst, grf_stream_t stream);

/* Banded transpose for the Gram kernel: entries (j, k, v) of Phi (CSR rows j)
 * bucketed by (band = j / band_width, k):  bucket id b = band * n_cols + k.
 * A bucket is a run of 12-byte record PAIRS {u16 8 (j0 - band start), u16 8 (j1 - band start)
 * (low / high half of one word), f32 v0, f32 v1}, starting on a unit boundary (rec_unit =
 * GRF_REC_LINE: a 128-byte line; GRF_REC_PACKED: right after the previous bucket); an odd
 * bucket ends with the pad record (0, +0.0).  Two calls (and the Gram) take the same rec_unit:
 *   plan: t_desc[2 * (n_bands * n_cols + 1)] = per bucket {first unit, pairs}; the last
 *         entry holds the total unit count (lo, hi words).  counted = 1: the bucket counts
 *         are already in the workspace (from grf_walk_phi over all rows), skip counting.
 *   fill: t_rec (>= total units * rec_unit bytes, 128-byte aligned), t_maxabs[1] = max |Phi| and
 *         t_rowshift[n_rows]: the Gram kernel's per-row fixed-point scale 2^shift (every term
 *         < 2^51, the row's sum of |terms| < 2^62).
 * workspace >= grf_transpose_workspace_bytes(n_bands * n_cols), shared by both calls (not NULL).
 * band_width <= 8192; n_rows, n_cols <= 2^31 - 1, n_cols >= 1.  The launch sizes of a call's own kernels and of its
 * first-level scan are checked before its first launch or memset, in all the transpose entries: a refused call has
 * touched nothing. */
int32_t grf_transpose_banded_plan(int64_t n_rows, int64_t n_cols, int64_t band_width, int32_t rec_unit,
                                  const int64_t *ptr, const int32_t *idx, uint32_t *t_desc, int32_t counted,
                                  void *workspace, size_t workspace_bytes, grf_stream_t stream);
int32_t grf_transpose_banded_fill(int64_t n_rows, int64_t n_cols, int64_t band_width, int32_t rec_unit,
                                  const int64_t *ptr, const int32_t *idx, const float *val, const uint32_t *t_desc,
                                  void *t_rec, int64_t t_rec_bytes, float *t_maxabs, int32_t *t_rowshift,
                                  void *workspace, size_t workspace_bytes, grf_stream_t stream);
size_t grf_transpose_workspace_bytes(int64_t n_buckets);
/* The same fill in two coalesced passes (entries binned by (band, 128-column region) into
 * `staging`, then each region's records built in LDS and written whole); band_width must be
 * a multiple of 64, nnz = ptr[n_rows].  Record order inside a bucket is unspecified in both
 * fills (the Gram's fixed-point sum does not depend on it). */
int32_t grf_transpose_banded_fill_staged(int64_t n_rows, int64_t n_cols, int64_t band_width, int32_t rec_unit,
                                         const int64_t *ptr, const int32_t *idx, const float *val,
                                         const uint32_t *t_desc, void *t_rec, int64_t t_rec_bytes, float *t_maxabs,
                                         int32_t *t_rowshift, void *workspace, size_t workspace_bytes, int64_t nnz,
                                         void *staging, size_t staging_bytes, grf_stream_t stream);
size_t grf_transpose_staging_bytes(int64_t n_rows, int64_t n_cols, int64_t band_width, int64_t nnz);

/* The staged transpose without a plan: no bucket counts from the walk (grf_walk_phi's t_count may
 * then be NULL) and no scan over every bucket.  Each (band, region) of the binning gets a slab of
 * record units bounded by its entry and bucket counts (one scan over the regions); its placing
 * workgroup counts its buckets in LDS, lays them out in the slab and writes their descriptors
 * t_desc (same meaning as the plan's: {first unit, pairs}; t_desc[nbk] = the slabs' total, an
 * upper bound of the units written).  Buckets stay in (band, column) order; unused slab tails are
 * never read.  t_rec >= grf_transpose_self_units_bound(...) * rec_unit bytes; workspace >=
 * grf_transpose_self_workspace_bytes; staging as for grf_transpose_banded_fill_staged.
 * t_split (NULL: none; else 16 bytes per bucket, 16-byte aligned, band_width <= 8192): every
 * bucket's entries are laid out by sub-band (the 8 row ranges of band_width / 8 rows, in order)
 * and t_split[b] holds 8 uint16 entry offsets, the entries of bucket b before each sub-band
 * (all 0 for a region too large for the LDS image: order unspecified there).  The symmetric
 * Gram entry points take it to start a diagonal tile's buckets at its row's sub-band. */
int32_t grf_transpose_banded_self(int64_t n_rows, int64_t n_cols, int64_t band_width, int32_t rec_unit,
                                  const int64_t *ptr, const int32_t *idx, const float *val, uint32_t *t_desc,
                                  void *t_split, void *t_rec, int64_t t_rec_bytes, float *t_maxabs, int32_t *t_rowshift,
                                  void *workspace, size_t workspace_bytes, int64_t nnz, void *staging,
                                  size_t staging_bytes, grf_stream_t stream);
size_t grf_transpose_self_workspace_bytes(int64_t n_rows, int64_t n_cols, int64_t band_width);
int64_t grf_transpose_self_units_bound(int64_t n_rows, int64_t n_cols, int64_t band_width, int32_t rec_unit,
                                       int64_t nnz);

/* Record kinds (additive to ABI 9).  GRF_REC_PAIRS: the 12-byte pairs {u16 8 * row0 | u16 8 * row1 << 16, f32 v0, f32 v1} of
 * every entry point above.  GRF_REC_TRIPLES: 16-byte triples {u32 cols, f32 v0, f32 v1, f32 v2}, 8 per 128-byte
 * line, cols = c0 | o1 << 12 | o2 << 22 with c0 the first entry's row in the band and o1 / o2 the other entries'
 * rows as offsets from c0 & ~511 (the start of c0's aligned 512-row block of the band).  A bucket's entries are
 * laid out by block and cut greedily: a triple whose first entry is in block e takes the following entries while
 * they lie in block e or e + 1; unused places are padding (row c0, +0.0).  Triples exist as line buckets only:
 * rec_unit = GRF_REC_LINE, band_width <= 4096, no t_split (NULL) -- anything else is GRF_EINVAL, nothing launched
 * -- and only from grf_transpose_banded_self_rec, which is grf_transpose_banded_self for the given kind;
 * t_desc holds {first line, triples} per bucket and t_rec >= grf_transpose_self_triples_lines_bound(...) * 128
 * bytes.  The Gram entries below read either kind; K's bits do not depend on it (integer sums, padding adds 0). */
enum grf_rec_kind { GRF_REC_PAIRS = 0, GRF_REC_TRIPLES = 1 };
int32_t grf_transpose_banded_self_rec(int32_t rec_kind, int64_t n_rows, int64_t n_cols, int64_t band_width,
                                      int32_t rec_unit, const int64_t *ptr, const int32_t *idx, const float *val,
                                      uint32_t *t_desc, void *t_split, void *t_rec, int64_t t_rec_bytes,
                                      float *t_maxabs, int32_t *t_rowshift, void *workspace, size_t workspace_bytes,
                                      int64_t nnz, void *staging, size_t staging_bytes, grf_stream_t stream);
int64_t grf_transpose_self_triples_lines_bound(int64_t n_rows, int64_t n_cols, int64_t band_width, int64_t nnz);

/* ---------------------------------------------------------------------- Gram
 * Replaces `Phi @ Phi.T` of fast_grf_kernel_general.py:55 (sparse) and :39 (dense).
 * Sparse path: K[r, :] for rows r in [row_begin, row_end) of Phi (compact CSR,
 * float32 values) against the banded transpose of the FULL Phi (band_width equal
 * to the transpose's, multiple of 64, <= 8192; t_desc / t_rec / t_rowshift from the transpose).
 * K is float32, row-major with leading dimension ldk (>= n_total); K row
 * (r - row_begin) is written.  Each K entry is the fp32 rounding of the exact
 * int64 fixed-point sum of the exact products Phi[r,k]*Phi[j,k] (per-row
 * power-of-two scale), so K does not depend on summation order: it is
 * bit-reproducible run to run, across row splits and GPU counts. */
int32_t grf_gram_sparse(int64_t n_total, int64_t row_begin, int64_t row_end, const int64_t *ptr, const int32_t *idx,
                        const float *val, int64_t band_width, int32_t rec_unit, const uint32_t *t_desc,
                        const void *t_rec, const int32_t *t_rowshift, float *K, int64_t ldk, void *workspace,
                        size_t workspace_bytes, grf_stream_t stream);
/* device workspace of one grf_gram_sparse / grf_gram_sparse_sym call (reserved for a tile
 * work counter; this build does not touch it and accepts NULL) */
size_t grf_gram_workspace_bytes(void);

/* Whole K = Phi Phi^T on one device using its symmetry: the Gram kernel computes the tiles
 * K[i, band >= band(i)] (about half the work) and a mirror pass copies K[j, i] = K[i, j]
 * for band(j) > band(i).  Same arguments and per-entry values as grf_gram_sparse with
 * row_begin = 0, row_end = n_total, except that the mirrored entries carry the
 * fixed-point rounding of row i (K is exactly symmetric).  band_width multiple of 64.
 * t_split: the transpose's sub-band split (grf_transpose_banded_self) or NULL; with it a tile on
 * its row's own band fetches only the buckets' sub-bands from the row's on (the entries below the
 * diagonal it skips are the mirror's to write). */
int32_t grf_gram_sparse_sym(int64_t n_total, const int64_t *ptr, const int32_t *idx, const float *val,
                            int64_t band_width, int32_t rec_unit, const uint32_t *t_desc, const void *t_rec,
                            const void *t_split, const int32_t *t_rowshift, float *K, int64_t ldk, void *workspace, size_t workspace_bytes,
                            grf_stream_t stream);

/* The Gram half of grf_gram_sparse_sym alone: the tiles K[i, band >= band(i)] (the lower parts
 * of the diagonal band tiles are written too and are overwritten by the mirror), restricted to
 * the parts [part_begin, part_end) of the band-major tile sequence cut into n_parts equal parts
 * (0, 1, 1 = all).  All parts followed by grf_gram_mirror on one stream is grf_gram_sparse_sym;
 * split so that other work can be scheduled against the Gram's tail and the HBM-bound mirror. */
int32_t grf_gram_sparse_upper(int64_t n_total, const int64_t *ptr, const int32_t *idx, const float *val,
                              int64_t band_width, int32_t rec_unit, const uint32_t *t_desc, const void *t_rec,
                              const void *t_split, const int32_t *t_rowshift, float *K, int64_t ldk, int32_t part_begin,
                              int32_t part_end, int32_t n_parts, void *workspace, size_t workspace_bytes,
                              grf_stream_t stream);

/* grf_gram_sparse_upper whose tile write-out ADDS the rounded fixed-point sums to K instead of
 * storing them: K's entries on and above the diagonal must hold the dense part first (the hub
 * columns' MFMA Gram, grf_gram_dense_upper).  With the hub columns' buckets emptied from the
 * transpose (grf_transpose_drop_columns) and their entries in the dense panel (grf_hub_panel),
 * dense upper + this + grf_gram_mirror is K = Phi Phi^T within the fp32 K tolerance (the hub part is
 * an fp32 MFMA sum instead of the exact fixed-point one).  Same arguments as grf_gram_sparse_upper. */
int32_t grf_gram_sparse_upper_add(int64_t n_total, const int64_t *ptr, const int32_t *idx, const float *val,
                                  int64_t band_width, int32_t rec_unit, const uint32_t *t_desc, const void *t_rec,
                                  const void *t_split, const int32_t *t_rowshift, float *K, int64_t ldk, int32_t part_begin,
                                  int32_t part_end, int32_t n_parts, void *workspace, size_t workspace_bytes,
                                  grf_stream_t stream);

/* Wave shares by record pairs (skewed graphs, where a row's long buckets cluster in its column
 * order).  grf_gram_row_cuts: col_w[k] = the record pairs of column k over all n_bands bands of
 * the transpose (t_desc, after any hub drop), then for every row of Phi (ptr, idx) 8 cuts
 * row_cuts[8 row + s] = the first nonzero (offset in the row) whose prefix of column weights
 * reaches s / 8 of the row's total (s = 0: 0).  col_w: n_cols int32 scratch; row_cuts: 8 n_rows int32.
 * grf_gram_sparse_upper_ex: grf_gram_sparse_upper (add_k = 0) or _add (add_k = 1) whose tiles give
 * each wave the nonzeros between its cuts instead of equal counts; row_cuts NULL = the plain call.
 * K is bit-identical either way (integer sums).  Line / packed buckets only (not GRF_REC_SLOT).
 * Replaces nothing in the reference: scheduling only (the reference's Phi @ Phi.T,
 * efficient_graph_gp_sparse/graph_kernels_sparse/fast_grf_kernel_general.py:55). */
int32_t grf_gram_row_cuts(int64_t n_rows, const int64_t *ptr, const int32_t *idx, int64_t n_bands, int64_t n_cols,
                          const uint32_t *t_desc, int32_t *col_w, int32_t *row_cuts, grf_stream_t stream);
int32_t grf_gram_sparse_upper_ex(int64_t n_total, const int64_t *ptr, const int32_t *idx, const float *val,
                                 int64_t band_width, int32_t rec_unit, const uint32_t *t_desc, const void *t_rec,
                                 const void *t_split, const int32_t *t_rowshift, const int32_t *row_cuts, float *K,
                                 int64_t ldk, int32_t part_begin, int32_t part_end, int32_t n_parts, int32_t add_k,
                                 grf_stream_t stream);

/* grf_gram_sparse and grf_gram_sparse_upper_ex for a transpose of the given record kind (additive to ABI 9; GRF_REC_PAIRS:
 * exactly those calls).  GRF_REC_TRIPLES: line buckets of grf_transpose_banded_self_rec, band_width <= 4096,
 * t_split NULL, else GRF_EINVAL.  grf_gram_row_cuts and grf_transpose_drop_columns read and edit the
 * descriptors' counts alone and serve both kinds. */
int32_t grf_gram_sparse_rec(int32_t rec_kind, int64_t n_total, int64_t row_begin, int64_t row_end, const int64_t *ptr,
                            const int32_t *idx, const float *val, int64_t band_width, int32_t rec_unit,
                            const uint32_t *t_desc, const void *t_rec, const int32_t *t_rowshift, float *K, int64_t ldk,
                            grf_stream_t stream);
int32_t grf_gram_sparse_upper_rec(int32_t rec_kind, int64_t n_total, const int64_t *ptr, const int32_t *idx,
                                  const float *val, int64_t band_width, int32_t rec_unit, const uint32_t *t_desc,
                                  const void *t_rec, const void *t_split, const int32_t *t_rowshift,
                                  const int32_t *row_cuts, float *K, int64_t ldk, int32_t part_begin, int32_t part_end,
                                  int32_t n_parts, int32_t add_k, grf_stream_t stream);

/* Hub-column split (hub-heavy graphs: Enron, Facebook, power-law).  grf_hub_panel writes the entries
 * Phi[r, k] of the columns with hub_pos[k] >= 0 into the dense fp32 panel P[r, hub_pos[k]] (row-major,
 * n_rows x ldp, zeroed by the caller; int32 hub_pos[n_cols], -1 elsewhere).  grf_transpose_drop_columns
 * empties the buckets of the n_drop columns cols[] in all n_bands bands of a banded transpose
 * (t_desc as returned by grf_transpose_banded_*, n_cols = the transposed matrix's columns). */
int32_t grf_hub_panel(int64_t n_rows, const int64_t *ptr, const int32_t *idx, const float *val,
                      const int32_t *hub_pos, float *P, int64_t ldp, grf_stream_t stream);
int32_t grf_transpose_drop_columns(int64_t n_bands, int64_t n_cols, uint32_t *t_desc, const int32_t *cols,
                                   int32_t n_drop, grf_stream_t stream);

/* Column block of K against another row set: K[r - row_begin, 0 : t_rows] = sum_k Phi[r, k] Phi_B[:, k]
 * for the rows r in [row_begin, row_end) of Phi (CSR ptr/idx/val, n_cols columns), where Phi_B
 * (t_rows rows, the same n_cols columns) is given by its banded transpose (grf_transpose_banded_*
 * of Phi_B) and row_shift holds the fixed-point shifts of Phi's rows (grf_phi_row_shifts over all
 * of Phi).  With Phi_B = Phi[b:e] the block is K[:, b:e], entry for entry the row mode's K[r, b + j]
 * (bit-identical to grf_gram_sparse): the multi-GPU path in which each rank transposes only its
 * own rows.  band_width: a multiple of 64 in [64, 8192]; ldk >= t_rows.
 * sym_row0 >= 0 declares Phi_B = Phi[sym_row0, sym_row0 + t_rows) (inside [row_begin, row_end)):
 * the square K[B, B] is then computed on and above its diagonal only and mirrored (its entries
 * below the diagonal carry the upper entry's bits, as in grf_gram_sparse_sym); sym_row0 < 0: none. */
int32_t grf_gram_sparse_cols(int64_t n_cols, int64_t row_begin, int64_t row_end, const int64_t *ptr,
                             const int32_t *idx, const float *val, const int32_t *row_shift, int64_t t_rows,
                             int64_t sym_row0, int64_t band_width, int32_t rec_unit, const uint32_t *t_desc,
                             const void *t_rec, const void *t_split, float *K, int64_t ldk, void *workspace,
                             size_t workspace_bytes, grf_stream_t stream);
/* The Gram fixed-point row shifts of a CSR (n_rows rows; float values) and its max |value|
 * (*maxabs, device): the same rule and the same per-row summation order as the banded transpose's
 * t_rowshift / t_maxabs, so grf_gram_sparse_cols reproduces grf_gram_sparse's bits. */
size_t grf_phi_row_shifts_workspace_bytes(int64_t n_rows);
int32_t grf_phi_row_shifts(int64_t n_rows, const int64_t *ptr, const float *val, float *maxabs, int32_t *row_shift,
                           void *workspace, size_t workspace_bytes, grf_stream_t stream);
/* The same shifts from statistics grf_compact_rows_stats left in `stats` while compacting the rows
 * (one pass over the values fewer; identical bits). */
int32_t grf_phi_row_shifts_stats(int64_t n_rows, const void *stats, float *maxabs, int32_t *row_shift,
                                 grf_stream_t stream);
/* The same shifts of padded rows (ABI 8): row r's cnt[r] entries at val[r * cap ...) (grf_walk_phi's output, not
 * compacted); workspace as grf_phi_row_shifts'. */
int32_t grf_phi_row_shifts_padded(int64_t n_rows, int64_t cap, const int32_t *cnt, const float *val, float *maxabs,
                                  int32_t *row_shift, void *workspace, size_t workspace_bytes, grf_stream_t stream);
/* grf_gram_sparse_cols from Phi as padded rows (ABI 8): row r's cnt[r] entries at idx / val [r * cap, ...) for
 * every row r < row_end (grf_walk_phi's output over sources [0, row_end), not compacted), Phi_B's transpose in
 * GRF_REC_SLOT buckets, no symmetric square; the pipelined column-block kernel (bit-identical to the CSR path
 * on the compacted rows). */
int32_t grf_gram_sparse_cols_padded(int64_t n_cols, int64_t row_begin, int64_t row_end, int64_t cap,
                                    const int32_t *cnt, const int32_t *idx, const float *val, const int32_t *row_shift,
                                    int64_t t_rows, int64_t band_width, const uint32_t *t_desc, const void *t_rec,
                                    float *K, int64_t ldk, grf_stream_t stream);

/* Partial Gram over a slice of the inner dimension: K[r, :] = sum over k in [k_begin, k_end)
 * of Phi[r, k] Phi[:, k] (same fixed-point rule as grf_gram_sparse).  The partial Grams of
 * disjoint slices sum to K -- the "partial K + all-reduce" multi-GPU option. */
int32_t grf_gram_sparse_kslice(int64_t n_total, int64_t row_begin, int64_t row_end, int64_t k_begin, int64_t k_end,
                               const int64_t *ptr, const int32_t *idx, const float *val, int64_t band_width,
                               int32_t rec_unit, const uint32_t *t_desc, const void *t_rec,
                               const int32_t *t_rowshift, float *K, int64_t ldk, void *workspace,
                               size_t workspace_bytes, grf_stream_t stream);

/* The mirror pass of grf_gram_sparse_sym alone: K[j, i] = K[i, j] for every j > i.
 * max_workgroups <= 0: one workgroup per 64 x 64 block (fastest alone); > 0: at most that many
 * workgroups striding over the blocks, which leaves CU slots to work on another stream (1024 =
 * 4 per CU was best beside the next step's walks: tools/gpu_mirror_ab.sh). */
int32_t grf_gram_mirror(int64_t n, float *K, int64_t ldk, int64_t max_workgroups, grf_stream_t stream);

/* Dense path: K = A A^T for A float32 row-major [n x lda] (columns >= k_dim are zero padding;
 * lda % 16 == 0, A 16-byte aligned).  K float32 [n x ldk] (ldk % 4 == 0, K 16-byte aligned), exactly
 * symmetric: the 128 x 128 tiles on and above the diagonal on the fp32 MFMA
 * (v_mfma_f32_16x16x4f32 / 32x32x2f32), each written to both triangles.
 * Replaces efficient_graph_gp/graph_kernels/fast_grf_kernel_general.py:39 (Phi @ Phi.T). */
int32_t grf_gram_dense(int64_t n, int64_t k_dim, const float *A, int64_t lda, float *K, int64_t ldk,
                       grf_stream_t stream);
/* grf_gram_dense's tiles on and above the diagonal only, nothing mirrored: every K[i, j >= i] is
 * written, entries below the diagonal only where a diagonal tile covers them.  The hub part of the
 * hub-column split (grf_gram_sparse_upper_add adds the sparse part on top). */
int32_t grf_gram_dense_upper(int64_t n, int64_t k_dim, const float *A, int64_t lda, float *K, int64_t ldk,
                             grf_stream_t stream);
/* As grf_gram_dense, with a device workspace for split-K: when the tiles alone would leave CUs idle
 * (every tile for small n, the last tiles of a large n), a tile is cut into k-slices whose partial
 * tiles are summed in slice order (deterministic) by the last of them to finish.  workspace:
 * grf_gram_dense_workspace_bytes(n, k_dim) bytes, 256-byte aligned, ZERO on first use (its first
 * 4 KiB hold the tiles' tickets, which every call leaves zero; the layout does not depend on n or
 * k_dim, so one workspace serves calls of any size in stream order); NULL or a smaller workspace
 * runs unsplit. */
size_t grf_gram_dense_workspace_bytes(int64_t n, int64_t k_dim);
int32_t grf_gram_dense_ws(int64_t n, int64_t k_dim, const float *A, int64_t lda, float *K, int64_t ldk,
                          void *workspace, size_t workspace_bytes, grf_stream_t stream);
/* The same K on the bf16 matrix cores (ABI 6): A is split exactly into three bf16 planes (a = a0 + a1 +
 * a2), K = sum over the six plane products a_p b_q with p + q <= 2 on v_mfma_f32_32x32x16_bf16 (16x the
 * fp32 MFMA's rate), a0 b0 and the five corrections accumulated apart in fp32.  The dropped products
 * |a1 b2| + |a2 b1| + |a2 b2| are at most (2u^3 + u^4) |a b| = (2^-23 + 2^-32) |a b| per term (bf16 unit
 * roundoff u = 2^-8), so the error bound is the fp32 path's plus (2^-23 + 2^-32) sum_k |A_ik A_jk| for
 * normal planes (an entry within 2^16 of the bf16 subnormal range can also lose its plane 2)
 * (measured against fp64: tests/test_gpu_parity.py test_gram_dense_split_*).  Symmetry and determinism as
 * grf_gram_dense_ws; from 64 tile rows on (n > 8064) 256 x 128 items of 8 waves on stream-K (bits then differ
 * from the 128-tile decomposition's within the bound above; GRF_DENSE_WIDE=0 / 1 forces it off / on).  Finite inputs below 2^128 (1 - 2^-9)
 * in magnitude only: an entry whose sum involves an infinite or NaN value of A (or one that rounds to an
 * infinite bf16) is NaN, where grf_gram_dense_ws follows IEEE (+-inf where no 0 * inf occurs).  workspace (required):
 * grf_gram_dense_split_workspace_bytes(n, k_dim) bytes, 256-byte aligned, ZERO on first use (the ticket
 * block of grf_gram_dense_ws at the same place, then the partial tiles of either decomposition). */
size_t grf_gram_dense_split_workspace_bytes(int64_t n, int64_t k_dim);
int32_t grf_gram_dense_split(int64_t n, int64_t k_dim, const float *A, int64_t lda, float *K, int64_t ldk,
                             void *workspace, size_t workspace_bytes, grf_stream_t stream);
/* grf_gram_dense_upper on the split products (ABI 6): the hub-column split's panel. */
int32_t grf_gram_dense_split_upper(int64_t n, int64_t k_dim, const float *A, int64_t lda, float *K, int64_t ldk,
                                   grf_stream_t stream);
/* The split's three bf16 planes written once (ABI 7): P row r holds, per k-tile t of 16, 96 bytes at
 * r ldp + 96 t -- plane 0 of k = 16 t .. 16 t + 15 (bf16, k order), plane 1, plane 2 -- the planes
 * grf_gram_dense_split forms in registers for every staged k-tile.  ldp >= grf_planes_row_bytes(k_dim)
 * (= 96 ceil(k_dim / 16)), a multiple of 16.  grf_split_planes reads A (zero-padded to 16 ceil(k_dim / 16)
 * columns, as grf_gram_dense_split requires); grf_densify_padded_planes writes them straight from the walk's
 * padded rows (grf_densify_padded's arguments, n_cols = k_dim).  grf_gram_dense_planes: K = A A^T from them with
 * nothing but fragment reads and MFMAs in the k-loop, on grf_gram_dense_split's decomposition for the size (the
 * 256 x 128 wide workgroups from 64 tile rows on, GRF_DENSE_WIDE as there; else the 128-tiles with their k-slices)
 * and bit-identical to it wherever both take the same work items (the same planes, the same products in the same
 * order); workspace as grf_gram_dense_split's (grf_gram_dense_split_workspace_bytes, ZERO on first use). */
int64_t grf_planes_row_bytes(int64_t k_dim);
int32_t grf_split_planes(int64_t n, int64_t k_dim, const float *A, int64_t lda, void *P, int64_t ldp,
                         grf_stream_t stream);
int32_t grf_densify_padded_planes(int64_t n_rows, int64_t cap, int64_t n_cols, const int32_t *cnt, const int32_t *idx,
                                  const float *val, void *P, int64_t ldp, grf_stream_t stream);
int32_t grf_gram_dense_planes(int64_t n, int64_t k_dim, const void *P, int64_t ldp, float *K, int64_t ldk,
                              void *workspace, size_t workspace_bytes, grf_stream_t stream);

/* CSR (float32) -> dense float32 [n_rows x lda], zero filled. */
int32_t grf_densify(int64_t n_rows, const int64_t *ptr, const int32_t *idx, const float *val, float *out,
                    int64_t lda, grf_stream_t stream);
/* The same from padded rows (grf_walk_phi's output: row r's cnt[r] entries at idx / val [r * cap, ...),
 * columns < n_cols), with no compaction: every row written whole once (zeros included) through LDS.
 * lda % 4 == 0, lda >= n_cols, lda * 4 <= 160 KiB (one CU's LDS), out 16-byte aligned.  ABI v5.
 * Replaces the dense path's Phi = F f (efficient_graph_gp/graph_kernels/fast_grf_kernel_general.py:38)
 * handed to the Gram as a dense matrix. */
int32_t grf_densify_padded(int64_t n_rows, int64_t cap, int64_t n_cols, const int32_t *cnt, const int32_t *idx,
                           const float *val, float *out, int64_t lda, grf_stream_t stream);

/* -------------------------------------- GPflow surface: a dense (N, N, L) step tensor F
 * Replaces efficient_graph_gp/gpflow_kernels/general_kernel_fast_grf.py:74-77 and
 * diffusion_kernel_fast_grf.py:52-60 (Phi = F f by tf.linalg.matmul, K = Phi Phi^T) and the
 * modulator gradient TensorFlow takes through them.  F float64 [n][n][L] contiguous (the
 * RandomWalk.get_random_walk_matrices tensor, random_walk_samplers/sampler.py:188-203).
 * grf_dense_steps_phi: Phi[i, j] = sum_l F[i, j, l] f[l] (fp64, l ascending) -> phi64 [n x n]
 * (optional, NULL to skip) and the zero-padded fp32 image phi32 [n x lda32] (lda32 >= n) that
 * grf_gram_dense / grf_gram_dense_ws read as A.
 * grf_dense_steps_grad: grad[l] = sum_ij F[i, j, l] ((G + G^T) Phi)[i, j] for the upstream gradient
 * G [n x ldg] of L w.r.t. K = Phi Phi^T (fp64 MFMA GEMM with the reduction fused into its
 * epilogue; partials summed in a fixed order: deterministic).  workspace:
 * grf_dense_steps_grad_workspace_bytes(n, L) bytes. */
int32_t grf_dense_steps_phi(int64_t n, int32_t L, const double *F, const double *f, double *phi64, float *phi32,
                            int64_t lda32, grf_stream_t stream);
size_t grf_dense_steps_grad_workspace_bytes(int64_t n, int32_t L);
int32_t grf_dense_steps_grad(int64_t n, int32_t L, const double *F, const double *phi64, const double *G,
                             int64_t ldg, double *grad, void *workspace, size_t workspace_bytes,
                             grf_stream_t stream);

/* ------------------------------------------- K.v and the pathwise-conditioning CG
 * The step after the path: SparseGraphGP.predict
 * (efficient_graph_gp_sparse/models/sparse_grf_model.py:21-45) and the linear_cg it
 * calls (line 43; linear_operator 0.5 via gpytorch==1.11).  K = Phi Phi^T is never
 * formed: K_rows,cols V = Phi[rows] (Phi[cols]^T V).  Dense blocks are float32
 * row-major [rows x ld] with the S right-hand sides / samples as columns.
 * `row_map` (int32, optional) selects rows of Phi; NULL = rows 0..n-1. */

/* (Phi[row_map])^T as CSR: t_ptr[n_cols + 1] (int64), t_idx / t_val [nnz]; t_idx are positions in
 * row_map; every column lists them in ascending order (a stable radix sort by column of the entries
 * laid out in row order).  nnz: the entries of the selected rows, or any upper bound of them (then
 * t_ptr[n_cols] holds the real count and the tail of t_idx / t_val is unused): a caller sizing from
 * bounds reads nothing back to the host. */
int32_t grf_csr_transpose(int64_t n_sel, const int64_t *ptr, const int32_t *idx, const float *val,
                          const int32_t *row_map, int64_t n_cols, int64_t nnz, int64_t *t_ptr, int32_t *t_idx,
                          float *t_val, void *workspace, size_t workspace_bytes, grf_stream_t stream);
size_t grf_csr_transpose_workspace_bytes(int64_t n_sel, int64_t n_cols, int64_t nnz);

/* Y[r, :] = sum_e val[e] X[idx[e], :] over row row_map[r] (fp32, fixed summation order):
 * phi_test @ v, eps1 @ phi_train.T (sparse_grf_model.py:39-40, 45). */
int32_t grf_spmm_csr(int64_t n_out, const int64_t *ptr, const int32_t *idx, const float *val, const int32_t *row_map,
                     const float *X, int64_t ldx, int32_t n_rhs, float *Y, int64_t ldy, grf_stream_t stream);
/* the same with fp64 dense blocks and accumulation (A's fp32 values widened) */
int32_t grf_spmm_csr_f64(int64_t n_out, const int64_t *ptr, const int32_t *idx, const float *val,
                         const int32_t *row_map, const double *X, int64_t ldx, int32_t n_rhs, double *Y, int64_t ldy,
                         grf_stream_t stream);

/* linear_cg(A._matmul, rhs, tolerance) with A = Phi_t Phi_t^T + noise I, Phi_t = Phi[row_map]
 * (n_sys rows; t_* its transpose from grf_csr_transpose): sparse_grf_model.py:34, 43.
 * rhs / x: [n_sys x ld] fp32, n_rhs in [1, 256] columns solved together (GRF_EUNSUPPORTED outside); n_sys and
 * n_cols >= 1, ld_rhs and ldx >= n_rhs, max_iter >= 0, a NaN noise is GRF_EINVAL (all the Gram solves).  Same rule as
 * linear_cg: per-column normalisation, eps = stop_updating_after = 1e-10, stop after
 * iteration k >= min(10, max_iter - 1) once the mean residual norm < tolerance.
 * *iters_out (host pointer, may be NULL) receives the iterations run and resid_out (host,
 * n_rhs doubles, may be NULL) the final residual norms of the normalised systems (the
 * quantities the stopping rule averages); the call returns when they are (it polls a
 * device flag, so it synchronises the stream).
 * grf_cg_gram_solve keeps the reference's fp32 vectors and scalars; the _f64 variant
 * runs the same recurrence in fp64 (Phi's fp32 values widened).  linear_cg's
 * trajectory is sensitive to rounding once CG loses orthogonality (K + s2 I with
 * condition ~1e4 reaches the cg_tolerance after 24 iterations in fp64, 36 in fp32; in
 * fp64 a 1e-15 relative change of the rhs already moves the 11-iteration result by ~1e-3),
 * so the fp64 solve is the one that tracks the algorithm itself. */
int32_t grf_cg_gram_solve(int64_t n_sys, const int64_t *ptr, const int32_t *idx, const float *val,
                          const int32_t *row_map, int64_t n_cols, const int64_t *t_ptr, const int32_t *t_idx,
                          const float *t_val, double noise, const float *rhs, int64_t ld_rhs, int32_t n_rhs,
                          double tolerance, int32_t max_iter, float *x, int64_t ldx, void *workspace,
                          size_t workspace_bytes, int32_t *iters_out, double *resid_out, grf_stream_t stream);
int32_t grf_cg_gram_solve_f64(int64_t n_sys, const int64_t *ptr, const int32_t *idx, const float *val,
                              const int32_t *row_map, int64_t n_cols, const int64_t *t_ptr, const int32_t *t_idx,
                              const float *t_val, double noise, const double *rhs, int64_t ld_rhs, int32_t n_rhs,
                              double tolerance, int32_t max_iter, double *x, int64_t ldx, void *workspace,
                              size_t workspace_bytes, int32_t *iters_out, double *resid_out, grf_stream_t stream);
/* (covers both precisions) */
size_t grf_cg_workspace_bytes(int64_t n_sys, int64_t n_cols, int32_t n_rhs);

/* ------------------------------------------- matrix-free marginal likelihood (training)
 * MLL(f, s2) = -1/2 y^T K^-1 y - 1/2 log det K^ - n/2 log 2 pi with K^ = Phi_T Phi_T^T + s2 I, estimated
 * the way the reference trains (gpytorch under max_cholesky_size = 0: CG + stochastic Lanczos
 * quadrature): one CG solve of [y | Z] whose per-column coefficients give the Lanczos tridiagonals,
 * and the modulator gradient by the contraction below.  K is never formed. */

/* grf_cg_gram_solve_f64 (same solve: x, *iters_out and resid_out are bit-identical) that also
 * records the CG coefficients of every iteration k that ran: coef[k * ld_coef + c] = alpha_k and
 * coef[(max_iter + k) * ld_coef + c] = beta_k of column c, as the recurrence used them (alpha = 0
 * where p.Ap < eps or the column had converged; beta = 0 where the old r.r < eps).  coef: device,
 * 2 * max_iter rows of ld_coef >= n_rhs doubles, zeroed first.  Same workspace as the plain solve. */
int32_t grf_cg_gram_solve_lanczos_f64(int64_t n_sys, const int64_t *ptr, const int32_t *idx, const float *val,
                                      const int32_t *row_map, int64_t n_cols, const int64_t *t_ptr,
                                      const int32_t *t_idx, const float *t_val, double noise, const double *rhs,
                                      int64_t ld_rhs, int32_t n_rhs, double tolerance, int32_t max_iter, double *x,
                                      int64_t ldx, void *workspace, size_t workspace_bytes, int32_t *iters_out,
                                      double *resid_out, double *coef, int64_t ld_coef, grf_stream_t stream);

/* out[l] = sum_c wt[c] sum_r ( A[r,c] (M_l[row_map[r]] WB)[c] + B[r,c] (M_l[row_map[r]] WA)[c] ), l < L:
 * the step matrices' rows (step_* are HOST arrays of L <= 64 device pointers, as in
 * grf_phi_steps_csr_*) times the dense WA / WB (n_cols x ldw, fp64), contracted with A / B
 * (n_sel x ld, fp64) and the column weights wt[n_rhs]; n_rhs in [1, 256]; row_map int32 or NULL.
 * With A = K^-1 [y | Z], WA = Phi_T^T A and the same for B = [K^-1 y | Z] this is
 * sum_c wt[c] a_c^T (dK^/df_l) b_c.  One launch for all steps, the n_sel x n_rhs products never
 * stored; fp64 sums in a fixed order (two calls give the same bits).  out: L doubles (device). */
int32_t grf_steps_frob_f64(int64_t n_sel, int32_t L, const int64_t *const *step_ptr, const int32_t *const *step_idx,
                           const float *const *step_val, const int32_t *row_map, const double *A, const double *B,
                           int64_t ld, const double *WA, const double *WB, int64_t ldw, const double *wt,
                           int32_t n_rhs, double *out, void *workspace, size_t workspace_bytes,
                           grf_stream_t stream);
size_t grf_steps_frob_workspace_bytes(int64_t n_sel, int32_t L);

/* ------------------------------------------- the GPyTorch surface's feature algebra
 * Device-resident step matrices (one CSR per step: int64 row pointers, sorted int32 columns,
 * float32 values -- the preprocessor's torch CSR values) for
 * efficient_graph_gp_sparse/gptorch_kernels_sparse/sparse_grf_kernel.py:24-61 and
 * sparse_diffusion_kernel.py:74-96; K[x1, x2] = Phi[x1] Phi[x2]^T runs on the Gram kernels above
 * (grf_gram_sparse_cols), the modulator gradient on grf_csr_transpose + grf_spmm_csr + these. */

/* Phi = sum_l f_l M_l over L <= 64 step matrices (step_* are HOST arrays of L device pointers):
 * `phi = sum(mod_vec * mat for ...)` (sparse_grf_kernel.py:54-60).  Per entry the terms of the
 * steps holding it are summed in step order in fp64 (0.0 + first term, left to right), exact
 * zeros dropped.  Two passes: _count writes the row lengths (int32 [n_rows]; scan them with
 * grf_scan_counts), _fill writes the rows at phi_ptr (phi_val and/or phi_val32 may be NULL). */
int32_t grf_phi_steps_csr_count(int64_t n_rows, int32_t L, const int64_t *const *step_ptr,
                                const int32_t *const *step_idx, const float *const *step_val, const double *f,
                                int32_t n_f, int32_t *phi_cnt, grf_stream_t stream);
int32_t grf_phi_steps_csr_fill(int64_t n_rows, int32_t L, const int64_t *const *step_ptr,
                               const int32_t *const *step_idx, const float *const *step_val, const double *f,
                               int32_t n_f, const int64_t *phi_ptr, int32_t *phi_idx, double *phi_val,
                               float *phi_val32, grf_stream_t stream);

/* phi[x_idx] (sparse_grf_kernel.py:33-41): len[r] = nnz of row row_map[r] (NULL map: row r);
 * then, with out_ptr = grf_scan_counts(len), the rows copied contiguously. */
int32_t grf_csr_row_lengths(int64_t n_sel, const int64_t *ptr, const int32_t *row_map, int32_t *len,
                            grf_stream_t stream);
int32_t grf_csr_gather_rows(int64_t n_sel, const int64_t *ptr, const int32_t *idx, const float *val,
                            const int32_t *row_map, const int64_t *out_ptr, int32_t *out_idx, float *out_val,
                            grf_stream_t stream);

/* out[r] = A[rows_a[r]] . B[rows_b[r]] (sorted CSR rows, fp64 sum of the exact products,
 * deterministic order; NULL row maps = identity): `(phi_x1 * phi_x2).sum(dim=-1)` (:43-45), and
 * with A = M_l the diagonal's modulator gradient. */
int32_t grf_csr_rowdot(int64_t n_pairs, const int64_t *a_ptr, const int32_t *a_idx, const float *a_val,
                       const int32_t *rows_a, const int64_t *b_ptr, const int32_t *b_idx, const float *b_val,
                       const int32_t *rows_b, double *out, grf_stream_t stream);

/* out[r] = sum_e val[e] Z[idx[e] * ldz + r] over the entries e of row row_map[r]: one step matrix's
 * rows contracted with the columns of a dense Z (n_cols x ldz, fp32, ldz >= n_sel).  With
 * Z = Phi[x2]^T G^T this is the modulator gradient of K[x1, x2] = Phi[x1] Phi[x2]^T:
 * dL/df_l = sum_r (M_l[x1] Z)[r, r] + (the same with x1, x2 and G^T swapped). */
int32_t grf_csr_rows_dot_cols(int64_t n_sel, const int64_t *ptr, const int32_t *idx, const float *val,
                              const int32_t *row_map, const float *Z, int64_t ldz, double *out, grf_stream_t stream);

/* K (dense fp32 on the device, n_rows x n_cols, row pitch ldk) -> the scipy CSR the reference's sparse
 * entry point returns (graph_kernels_sparse/fast_grf_kernel_general.py:55: `Phi @ Phi.T`, float64
 * values, sorted columns, exact zeros absent).  _count: cnt[r] = nonzeros of row r; with
 * out_ptr = grf_scan_counts(cnt), _fill writes the int32 columns and the float64-widened values. */
int32_t grf_dense_to_csr_count(int64_t n_rows, int64_t n_cols, const float *K, int64_t ldk, int32_t *cnt,
                               grf_stream_t stream);
int32_t grf_dense_to_csr_fill(int64_t n_rows, int64_t n_cols, const float *K, int64_t ldk, const int64_t *out_ptr,
                              int32_t *out_idx, double *out_val, grf_stream_t stream);

/* ------------------------------------------- sparse x sparse: the exact step matrices' producer
 * C = A B, CSR x CSR -> CSR in fp64 (A: n_rows x n_mid, B: n_mid x n_cols; the project's CSR: int64 row
 * pointers, int32 columns ascending and unique per row, float64 values; rows may be empty; every dimension
 * up to 2^31 - 1).  Chained as M_l = M_{l-1} L from M_0 = I it gives the exact walk-power tensor
 * [I, L, L^2, ...] of the reference's compute_pstep_walk_matrix (general_kernel_pofm.py:7-42), which its
 * GraphGeneralPoFMKernel / GraphDiffusionPoFMKernel are built on.
 *
 * The result is fixed to the bit: row i's pattern is the union of the patterns of B's rows k over the stored
 * entries (i, k) of A, columns ascending, exact-zero sums KEPT (structural pattern); c_ij starts from +0.0
 * and adds RN(a_ik b_kj) one product at a time in the order of A's row entries (ascending k), multiply and
 * add rounded separately (no FMA).  This is Gustavson's order and scipy's: the bits of scipy's `A @ B` after
 * sort_indices, apart from exact-zero sums, which scipy may drop.  No floating-point atomics: two calls give
 * the same bits.
 *
 * Same convention as grf_phi_steps_csr_count / _fill: _count writes the row lengths (int32 [n_rows]; scan
 * them with grf_scan_counts), _fill writes the rows at c_ptr (c_val32, the values rounded once to float32,
 * may be NULL).  Both need grf_spgemm_workspace_bytes(n_rows, n_mid, n_cols) bytes of workspace, run
 * asynchronously on `stream` and read nothing back.  Per output row the kernels choose, on the device, by
 * the row's product count P = sum over A's entries (i, k) of len(B[k]): up to GRF_SPGEMM_SORT_PRODUCTS the
 * products are sorted by (column, sequence) in LDS and summed in order; larger rows go to a fixed set of
 * waves (between GRF_SPGEMM_BIG_MIN_WAVES and GRF_SPGEMM_BIG_MAX_WAVES, by n_cols) that mark the columns in
 * a bitmap of n_cols bits each and accumulate GRF_SPGEMM_ACC_SLOTS output entries at a time in LDS. */
#define GRF_SPGEMM_SORT_PRODUCTS 1024
#define GRF_SPGEMM_ACC_SLOTS 4096
#define GRF_SPGEMM_BIG_MIN_WAVES 8
#define GRF_SPGEMM_BIG_MAX_WAVES 256
size_t grf_spgemm_workspace_bytes(int64_t n_rows, int64_t n_mid, int64_t n_cols);
/* general_kernel_pofm.py:7-42 (the pattern of current_power @ adj_matrix) */
int32_t grf_spgemm_csr_count(int64_t n_rows, int64_t n_mid, int64_t n_cols, const int64_t *a_ptr, const int32_t *a_idx,
                             const int64_t *b_ptr, const int32_t *b_idx, int32_t *row_cnt, void *workspace,
                             size_t workspace_bytes, grf_stream_t stream);
/* general_kernel_pofm.py:7-42 (current_power @ adj_matrix itself) */
int32_t grf_spgemm_csr_fill(int64_t n_rows, int64_t n_mid, int64_t n_cols, const int64_t *a_ptr, const int32_t *a_idx,
                            const double *a_val, const int64_t *b_ptr, const int32_t *b_idx, const double *b_val,
                            const int64_t *c_ptr, int32_t *c_idx, double *c_val, float *c_val32, void *workspace,
                            size_t workspace_bytes, grf_stream_t stream);

/* ------------------------------------------- the exact walk-power kernel as a matrix-free operator
 * Phi = p(G) = sum_{l < n_f} f_l G^l (the exact kernel of general_kernel_pofm.py:7-42, :45-96) without its
 * powers, which fill in (G^4 of a mean-degree-20 graph is dense): every product is a Horner chain with the
 * walk matrix itself,
 *     H_{n_f-1} = f_{n_f-1} X,   H_l = A H_{l+1} + f_l X  (l = n_f - 2 .. 0),   p(A) X = H_0,
 * and K_TT V = S_T p(G) p(G)^T S_T^T V is two chains, one with G^T and one with G.  A: n x n CSR as
 * grf_laplacian_csr writes it (int64 row pointers, sorted int32 columns, float64 values); it is NOT assumed
 * symmetric, the caller passes G^T where the transpose is meant.  f: n_f >= 1 coefficients on the DEVICE.
 * Dense blocks are float64 row-major with the n_rhs in [1, 256] right-hand sides as columns.
 *
 * Order rule.  One output element of a step is computed as follows (fp64 throughout):
 *   1. start from +0.0;
 *   2. add the row's products val[e] * x[idx[e], c] one at a time in the order of the row's entries
 *      (ascending column), each by one fused multiply-add; in the chain's first step the gathered value is
 *      x = RN(f_{n_f-1} * X[., c]) (the scale of H_{n_f-1} folded into the read);
 *   3. add the f_l X addend by one fused multiply-add, fma(f_l, X[row, c], sum);
 *   4. add the noise addend, if present, by one fused multiply-add, fma(noise, P[r, c], sum).
 * n_f = 1 is the single step 0.0 + f_0 X without a matrix (K_TT = f_0^2 I).  Rows that a map sends to -1
 * add nothing in steps 2 and 3.  No floating-point atomics: two calls give the same bits. */

/* Y = p(A) X~ on the rows `row_map` (general_kernel_pofm.py:45-96: the kernel's products without K).
 * inv_map (int32 [n], optional): node -> its row of X, or -1 for a node whose row of X~ is zero (X~ = S^T X
 * for a node subset, never stored); NULL: X has n rows.  row_map (int32 [n_out], optional): the rows of p(A) X~
 * written to Y (n_out x ldy); NULL: all of them, and n_out must be n.  ldx, ldy >= n_rhs; nothing outside
 * [rows x n_rhs] of Y is written.  Y and the workspace must not overlap X.  Workspace:
 * grf_poly_workspace_bytes(n, n_f, n_rhs) bytes (two n x n_rhs blocks; none for n_f <= 2). */
size_t grf_poly_workspace_bytes(int64_t n, int32_t n_f, int32_t n_rhs);
int32_t grf_poly_apply_f64(int64_t n, const int64_t *ptr, const int32_t *idx, const double *val, const double *f,
                           int32_t n_f, const int32_t *inv_map, const int32_t *row_map, int64_t n_out,
                           const double *X, int64_t ldx, int32_t n_rhs, double *Y, int64_t ldy, void *workspace,
                           size_t workspace_bytes, grf_stream_t stream);

/* grf_cg_gram_solve_f64 / grf_cg_gram_solve_lanczos_f64 (same contract, same recurrence, reductions, stopping
 * rule, polling and coefficient records) on A = S_T p(G) p(G)^T S_T^T + noise I: models/sparse_grf_model.py:21-45
 * on the exact kernel.  (g_*, gt_*): G and G^T (n x n); row_map (int32 [n_sys]): the training nodes T;
 * inv_map (int32 [n]): a node's position in row_map, or -1.  Every matvec is the chain with G^T read from the
 * direction block through inv_map, then the chain with G whose last step runs on row_map only and adds
 * noise * P.  Workspace: grf_cg_poly_workspace_bytes(n_sys, n, n_rhs). */
size_t grf_cg_poly_workspace_bytes(int64_t n_sys, int64_t n, int32_t n_rhs);
int32_t grf_cg_poly_solve_f64(int64_t n_sys, int64_t n, const int64_t *g_ptr, const int32_t *g_idx,
                              const double *g_val, const int64_t *gt_ptr, const int32_t *gt_idx, const double *gt_val,
                              const double *f, int32_t n_f, const int32_t *row_map, const int32_t *inv_map,
                              double noise, const double *rhs, int64_t ld_rhs, int32_t n_rhs, double tolerance,
                              int32_t max_iter, double *x, int64_t ldx, void *workspace, size_t workspace_bytes,
                              int32_t *iters_out, double *resid_out, grf_stream_t stream);
int32_t grf_cg_poly_solve_lanczos_f64(int64_t n_sys, int64_t n, const int64_t *g_ptr, const int32_t *g_idx,
                                      const double *g_val, const int64_t *gt_ptr, const int32_t *gt_idx,
                                      const double *gt_val, const double *f, int32_t n_f, const int32_t *row_map,
                                      const int32_t *inv_map, double noise, const double *rhs, int64_t ld_rhs,
                                      int32_t n_rhs, double tolerance, int32_t max_iter, double *x, int64_t ldx,
                                      void *workspace, size_t workspace_bytes, int32_t *iters_out, double *resid_out,
                                      double *coef, int64_t ld_coef, grf_stream_t stream);

/* ------------------------------------------- diagonally preconditioned solves (fp64; purely additive to ABI 9)
 * linear_cg with a `preconditioner` closure z = dinv . r, dinv (device, n_sys doubles, all positive) the inverse
 * of a diagonal D -- for D = diag(K^) the Jacobi preconditioner, which suits the walk estimator: its rows differ
 * by orders of magnitude in norm and are nearly orthogonal once scaled, so D^-1/2 K^ D^-1/2 is close to I.
 *     init:  r = b / ||b||, p = z = dinv . r, x = 0, rz = sum r.z
 *     step:  alpha = rz / p.Ap (0 where p.Ap < eps or the column has converged); r -= alpha Ap; x += alpha p;
 *            z = dinv . r; beta = rz_new / rz_old (0 where rz_old < eps); p = z + beta p.
 * The residual norm behind has_converged, resid_out and the stopping rule stays the unpreconditioned ||r||; eps,
 * stop_updating_after, the zero-rhs mask, the polling and the result * ||b|| write-out are those of
 * grf_cg_gram_solve_f64.  z is never stored (formed where it is used); the init and update reductions carry two
 * sums per column (r.z and r.r) in the plain solve's fixed order, so two calls give the same bits, and dinv = 1
 * reproduces grf_cg_gram_solve_f64 / grf_cg_poly_solve_f64 bit for bit (x, iterations, residuals, coefficients).
 * The _lanczos variants record alpha_k and beta_k as the plain ones do: they are the Lanczos coefficients of
 * D^-1/2 K^ D^-1/2 started at D^1/2 b / ||.||.  Arguments: those of the unpreconditioned function, then dinv
 * before the stream.  Workspaces: grf_pcg_workspace_bytes / grf_pcg_poly_workspace_bytes (larger than the plain
 * ones by the second partial sums).
 *
 * grf_gram_jacobi_f64: dinv[r] = 1 / (sum_e Phi[row_map[r], e]^2 + noise), r < n_sel (row_map int32 or NULL; idx
 * is not read).  Order rule: the squares (fp32 widened: exact in fp64) are added to +0.0 one by one in the row's
 * stored order, then the noise, then one IEEE division.  Where the sum plus noise is not positive (an empty row
 * with zero noise) dinv[r] = 1: the row is not preconditioned.  noise >= 0; n_sel == 0 touches nothing. */
int32_t grf_gram_jacobi_f64(int64_t n_sel, const int64_t *ptr, const int32_t *idx, const float *val,
                            const int32_t *row_map, double noise, double *dinv, grf_stream_t stream);
size_t grf_pcg_workspace_bytes(int64_t n_sys, int64_t n_cols, int32_t n_rhs);
int32_t grf_pcg_gram_solve_f64(int64_t n_sys, const int64_t *ptr, const int32_t *idx, const float *val,
                               const int32_t *row_map, int64_t n_cols, const int64_t *t_ptr, const int32_t *t_idx,
                               const float *t_val, double noise, const double *rhs, int64_t ld_rhs, int32_t n_rhs,
                               double tolerance, int32_t max_iter, double *x, int64_t ldx, void *workspace,
                               size_t workspace_bytes, int32_t *iters_out, double *resid_out, const double *dinv,
                               grf_stream_t stream);
int32_t grf_pcg_gram_solve_lanczos_f64(int64_t n_sys, const int64_t *ptr, const int32_t *idx, const float *val,
                                       const int32_t *row_map, int64_t n_cols, const int64_t *t_ptr,
                                       const int32_t *t_idx, const float *t_val, double noise, const double *rhs,
                                       int64_t ld_rhs, int32_t n_rhs, double tolerance, int32_t max_iter, double *x,
                                       int64_t ldx, void *workspace, size_t workspace_bytes, int32_t *iters_out,
                                       double *resid_out, double *coef, int64_t ld_coef, const double *dinv,
                                       grf_stream_t stream);
size_t grf_pcg_poly_workspace_bytes(int64_t n_sys, int64_t n, int32_t n_rhs);
int32_t grf_pcg_poly_solve_f64(int64_t n_sys, int64_t n, const int64_t *g_ptr, const int32_t *g_idx,
                               const double *g_val, const int64_t *gt_ptr, const int32_t *gt_idx,
                               const double *gt_val, const double *f, int32_t n_f, const int32_t *row_map,
                               const int32_t *inv_map, double noise, const double *rhs, int64_t ld_rhs, int32_t n_rhs,
                               double tolerance, int32_t max_iter, double *x, int64_t ldx, void *workspace,
                               size_t workspace_bytes, int32_t *iters_out, double *resid_out, const double *dinv,
                               grf_stream_t stream);
int32_t grf_pcg_poly_solve_lanczos_f64(int64_t n_sys, int64_t n, const int64_t *g_ptr, const int32_t *g_idx,
                                       const double *g_val, const int64_t *gt_ptr, const int32_t *gt_idx,
                                       const double *gt_val, const double *f, int32_t n_f, const int32_t *row_map,
                                       const int32_t *inv_map, double noise, const double *rhs, int64_t ld_rhs,
                                       int32_t n_rhs, double tolerance, int32_t max_iter, double *x, int64_t ldx,
                                       void *workspace, size_t workspace_bytes, int32_t *iters_out, double *resid_out,
                                       double *coef, int64_t ld_coef, const double *dinv, grf_stream_t stream);

/* The modulator gradient's contraction on the operator (the training step of models/sparse_grf_model.py:21-45's
 * model; A, B, wt as in grf_steps_frob_f64): with a~ = S_T^T A, b~ = S_T^T B, W_A = p(G^T) a~, W_B = p(G^T) b~,
 * U_l = (G^T)^l a~, V_l = (G^T)^l b~,
 *     out[l] = sum_c wt[c] ( <U_l[:, c], W_B[:, c]> + <V_l[:, c], W_A[:, c]> ),  l < n_f,
 * which is sum_c wt[c] a_c^T (dK^/df_l) b_c.  A, B: n_sel x ld (ld >= n_rhs); inv_map (int32 [n]): a node's row
 * of A / B, or -1.  Each step U_l = G^T U_{l-1} is fused with its inner products; per element of U_l the
 * order rule's steps 1-2, then per node fma(wt[c], fma(U, W_B, RN(V W_A)), sum) over the node's columns
 * c = lane, lane + 64, ...; a wave's nodes ascending, the 64 lanes by an xor tree, the 4 waves in order, one
 * fp64 partial per block, the last block (by a ticket at the workspace's start, zero again afterwards) adds
 * the partials in block order.  out: n_f doubles on the device.  Workspace:
 * grf_poly_grad_workspace_bytes(n, n_rhs) (six n x n_rhs blocks). */
size_t grf_poly_grad_workspace_bytes(int64_t n, int32_t n_rhs);
int32_t grf_poly_grad_f64(int64_t n, const int64_t *gt_ptr, const int32_t *gt_idx, const double *gt_val,
                          const double *f, int32_t n_f, int64_t n_sel, const int32_t *inv_map, const double *A,
                          const double *B, int64_t ld, const double *wt, int32_t n_rhs, double *out, void *workspace,
                          size_t workspace_bytes, grf_stream_t stream);

/* K blocks, diagonals and their modulator gradients from the operator (the K = Phi[x1] Phi[x2]^T of
 * general_kernel_pofm.py:45-96 where Phi cannot be formed).  With Psi_i = p(G^T) S_i^T (n x n_i, S_i selecting
 * the nodes x_i, which may repeat and need not be sorted: an entry of x_i is just a column),
 *     K[x1, x2] = Psi_1^T Psi_2 = S_1 p(G) p(G)^T S_2^T,     diag K[x]_c = sum_r Psi[r, c]^2.
 * x1, x2, x: int32 node indices on the device.  Columns are processed in blocks of at most 256; every step
 * follows the order rule above, unchanged.
 *
 * Unit columns.  Chain 1 runs on the unit columns e_{x2[c]} without reading a block: the value gathered at
 * node j, column c, is RN(f_{n_f-1} * 1) if j == x2[c], else +0.0, and the f_l X addend is fma(f_l, [row == x2[c]],
 * sum).  Column c of the block is therefore bit-identical to grf_poly_apply_f64 (G^T, then G on the rows x1)
 * applied to e_{x2[c]}.
 *
 * grf_poly_kernel_block_f64: K (n1 x n2 into a row-major block, ldk >= n2; nothing outside it is written).  Per
 * column block chain 1 with G^T from the unit columns, then chain 2 with G whose last step runs on the rows x1
 * only and writes into K at the block's column offset.  n_f = 1: f_0^2 [x1[r] == x2[c]], no matrix read.
 * n1 = 0 or n2 = 0: nothing is touched.  Workspace: grf_poly_kernel_block_workspace_bytes(n, n_f, n2) (one
 * n x min(n2, 256) block, three for n_f > 2). */
size_t grf_poly_kernel_block_workspace_bytes(int64_t n, int32_t n_f, int64_t n2);
int32_t grf_poly_kernel_block_f64(int64_t n, const int64_t *g_ptr, const int32_t *g_idx, const double *g_val,
                                  const int64_t *gt_ptr, const int32_t *gt_idx, const double *gt_val, const double *f,
                                  int32_t n_f, const int32_t *x1, int64_t n1, const int32_t *x2, int64_t n2, double *K,
                                  int64_t ldk, void *workspace, size_t workspace_bytes, grf_stream_t stream);

/* diag K[x] (n_x doubles): chain 1 only; its last step computes Psi[r, :] by the order rule and adds
 * fma(Psi[r, c], Psi[r, c], sum) per column without writing Psi: a wave's rows ascending, the 4 waves in order,
 * one fp64 partial per (block, column), the last block (by the ticket at the workspace's start, zero again
 * afterwards) adds a column's partials in block order.  n_f = 1: RN(f_0^2).  Workspace:
 * grf_poly_kernel_diag_workspace_bytes(n, n_f, n_x). */
size_t grf_poly_kernel_diag_workspace_bytes(int64_t n, int32_t n_f, int64_t n_x);
int32_t grf_poly_kernel_diag_f64(int64_t n, const int64_t *gt_ptr, const int32_t *gt_idx, const double *gt_val,
                                 const double *f, int32_t n_f, const int32_t *x, int64_t n_x, double *out,
                                 void *workspace, size_t workspace_bytes, grf_stream_t stream);

/* The modulator gradient of <g, K[x1, x2]> (diag = 0; g: n1 x n2, ldg >= n2) or of <g, diag K[x1]> (diag != 0;
 * g: n1 doubles; x2, inv1, inv2, ldg unused):
 *     out[l] = sum_c <((G^T)^l S_1^T g)[:, c], Psi_2[:, c]> + sum_r <((G^T)^l S_2^T g^T)[:, r], Psi_1[:, r]>,
 *     out[l] = 2 sum_c g_c <(G^T)^l e_{x_c}, Psi[:, c]>                                     (diagonal),  l < n_f.
 * inv1 / inv2 (int32 [n]): a node's row / column of g, or -1; S_i^T g is read through them and never stored.  A
 * node that x_i repeats has one row (column) there: the caller adds its repeats' cotangents into it and zeroes
 * the others, which leaves the sum unchanged.  Per column block Psi comes from chain 1 on the unit columns;
 * each Krylov step U_l = G^T U_{l-1} (order rule steps 1-2) is fused with fma(U, Psi, sum) over a node's
 * columns c = lane, lane + 64, ..., reduced as in grf_poly_grad_f64; the column blocks' contributions are added
 * in block order, the first half before the mirrored one (which reads g^T from a transposed copy in the
 * workspace).  The diagonal form starts from U_0 = [g_c e_{x_c}]_c, read from no block, and scales each block's
 * sum by 2.  An empty block gives zeros.  out: n_f doubles on the device.  Workspace:
 * grf_poly_kernel_grad_workspace_bytes(n, n1, n2, diag) (three n x min(max(n1, n2), 256) blocks and n1 x n2). */
size_t grf_poly_kernel_grad_workspace_bytes(int64_t n, int64_t n1, int64_t n2, int32_t diag);
int32_t grf_poly_kernel_grad_f64(int64_t n, const int64_t *gt_ptr, const int32_t *gt_idx, const double *gt_val,
                                 const double *f, int32_t n_f, const int32_t *x1, int64_t n1, const int32_t *inv1,
                                 const int32_t *x2, int64_t n2, const int32_t *inv2, const double *g, int64_t ldg,
                                 int32_t diag, double *out, void *workspace, size_t workspace_bytes,
                                 grf_stream_t stream);

/* ------------------------------------------- the exact diffusion kernel exp(-beta L) on the fp64 matrix cores
 * Replaces efficient_graph_gp/graph_kernels/diffusion_kernel.py:6-12 (scipy.linalg.expm of -beta L) and the
 * kernel matrix of efficient_graph_gp/gpflow_kernels/diffusion_kernel_exact.py:6-46 (tf.linalg.expm).  Purely
 * additive to ABI 9.
 *
 * grf_gemm_nt_f64: a dense fp64 product on v_mfma_f64_16x16x4_f64,
 *     C[i, j] = alpha * sum_k A[ra(i), k] B[rb(j), k] + gamma * Z[i, j] + delta * [i == j],  i < n1, j < n2, k < nk.
 * Both operands are read by rows; lda, ldb >= nk, ldc, ldz, ldw >= n2.  ra / rb: optional int32 row maps (NULL:
 * identity; repeated and unsorted indices are just rows); a_rows / b_rows: the rows A / B hold (n1 / n2 without
 * a map), used for the overlap check only -- a map's entries must lie in [0, rows).  Z optional (NULL: no addend,
 * gamma unused); Z may alias C exactly (same pointer and pitch).  C must overlap neither A nor B.
 *
 * Order rule of an entry (fp64 throughout, no split-k, no floating-point atomics: two calls give the same bits):
 *   1. acc starts from +0.0; the k-tiles of 16 are added in ascending order, within a k-tile its four groups
 *      of 4 consecutive k in ascending order, each group by one v_mfma_f64_16x16x4_f64 onto acc (k >= nk reads
 *      +0.0); one accumulator chain per entry, the same in every mode;
 *   2. c = RN(alpha * acc);  3. with Z: c = RN(c + RN(gamma * Z[i, j]));  4. if i == j: c = RN(c + delta).
 * Modes:
 *   general      (symmetric = 0, W = NULL) every 128 x 128 tile is computed and written.
 *   symmetric    (symmetric != 0) needs n1 == n2, no row maps, W = NULL, and the caller's promise that the product
 *                and Z are symmetric.  Only tiles with bj >= bi are computed; an entry j >= i is written to C[i, j]
 *                and C[j, i] from the same accumulator (Z is read at [i, j], j >= i, only), so C is bitwise
 *                symmetric even when A != B, and its upper triangle equals the general mode's bit for bit.
 *   contraction  (W != NULL) out[0] = sum_ij W[i, j] c_ij on the device; C is not read or written (may be NULL).
 *                A lane adds its 64 entries of the tile by fma(W, c, sum) in a fixed order, the 64 lanes by an
 *                xor tree, the 4 waves in order, one fp64 partial per tile; the last tile (by a ticket at the
 *                workspace's start, zero again afterwards) adds the partials in tile order.  Summation depth
 *                beyond the product's nk: 64 + 6 + 3 + tiles.  Workspace: grf_gemm_nt_f64_workspace_bytes(n1, n2)
 *                (other modes need none).
 * Columns [n2, ldc) of C and everything past the buffer are never written; GRF_EINVAL writes nothing; n1 == 0 or
 * n2 == 0 touches nothing; nk == 0 gives gamma Z + delta I (A, B unused). */
size_t grf_gemm_nt_f64_workspace_bytes(int64_t n1, int64_t n2);
int32_t grf_gemm_nt_f64(int64_t n1, int64_t n2, int64_t nk, double alpha, const double *A, int64_t lda,
                        int64_t a_rows, const int32_t *ra, const double *B, int64_t ldb, int64_t b_rows,
                        const int32_t *rb, double gamma, const double *Z, int64_t ldz, double delta, double *C,
                        int64_t ldc, int32_t symmetric, const double *W, int64_t ldw, double *out, void *workspace,
                        size_t workspace_bytes, grf_stream_t stream);

/* grf_expm_sym_f64: E = exp(-beta L) for a dense symmetric L (n x n, ldl >= n) on the device, by scaling and
 * squaring; a host-side chain of grf_gemm_nt_f64 calls, no host read of device data.  rho: the caller's bound on
 * the spectral radius of beta L (2 beta for a normalised Laplacian of non-negative weights, beta ||L||_inf
 * otherwise).
 * Order rule (17 + s products):
 *   1. s = grf_expm_squarings(rho) = max(0, ceil(log2 rho)) (theta = 1: ||X||_2 <= 1, Taylor remainder <= 1 / 19!);
 *   2. X = RN(-beta 2^-s * L) entry by entry (the factor itself is exact);
 *   3. Horner on the degree-18 Taylor polynomial: H_18 = RN(RN(RN(1/18) X) + I), then for k = 17 .. 1
 *      H_k = I + RN(1/k) (X H_{k+1}) by one symmetric-mode product (alpha = RN(1/k), delta = 1): 17 products;
 *   4. s squarings P <- P P (symmetric mode, alpha = 1) between two ping-pong buffers; the last product of all
 *      is written to E.  Every intermediate has its spectrum in (0, 1]: nothing overflows for any beta > 0.
 * E (lde >= n) is bitwise symmetric; n = 1 works.  beta <= 0, a non-finite beta or rho, or a rho that needs more
 * than 64 squarings: GRF_EINVAL.  E, L and the workspace must not overlap.  Workspace:
 * grf_expm_sym_f64_workspace_bytes(n) (three n x n blocks, rows padded to an even length). */
int32_t grf_expm_squarings(double rho);
size_t grf_expm_sym_f64_workspace_bytes(int64_t n);
int32_t grf_expm_sym_f64(int64_t n, const double *L, int64_t ldl, double beta, double rho, double *E, int64_t lde,
                         void *workspace, size_t workspace_bytes, grf_stream_t stream);

/* ------------------------------------------- the exact posterior mean and variance (predict_f)
 * For training nodes T (n of them), K^ = K[T,T] + s2 I, alpha = K^-1 y and test nodes x_c with b_c = K[T, x_c]:
 *     mean_c = b_c^T alpha,    var_c = K[x_c, x_c] - b_c^T K^-1 b_c,    cov = K[x,x] - B^T K^-1 B,
 * K never formed, the test nodes in chunks of <= 256 columns with one batched CG solve (grf_cg_gram_solve_f64 or
 * grf_cg_poly_solve_f64) per chunk.  Replaces the reference's only route on the sparse model, the moments of 64
 * pathwise samples (experiments/graph_bo/scripts/wind_experiment.py:396-398,
 * experiments/sparse/scaling_exp/run_scaling_experiment.py:621: samples.mean(0) / samples.std(0), a standard
 * deviation with ~9 % Monte-Carlo error), by what its dense baseline has (model.predict_f,
 * run_scaling_experiment.py:729); the NLPD of wind_experiment.py:319-324 is evaluated on these moments.  Purely
 * additive to ABI 9.
 *
 * grf_posterior_rhs_f64: the chunk's right-hand sides from Phi (the device CSR of grf_cg_gram_solve*: int64 row
 * pointers, int32 columns, fp32 values; n_rows x n_cols) and n_nodes <= 256 node indices (device int32; repeats
 * allowed; an index outside [0, n_rows) counts as an empty row):
 *     E[k, c] = Phi[nodes[c], k]  (fp32 widened: exact), every other E[k, c], c < n_nodes, zero;
 *     prior[c] = sum_k Phi[nodes[c], k]^2 = K[x_c, x_c].
 * E: n_cols x n_nodes fp64 row-major, lde >= n_nodes; the columns [n_nodes, lde) of a row are never written.
 * B = Phi[T] E is then one grf_spmm_csr_f64.  Order rule: the squares (exact in fp64) are added to +0.0 one by one
 * in the row's stored order, without FMA.  n_nodes == 0 touches nothing.
 *
 * grf_posterior_reduce_f64: one pass over B and X = K^-1 B (n x n_rhs fp64 row-major, pitches ldb, ldx >= n_rhs):
 *     q[c] = sum_r B[r,c] X[r,c],   var[c] = (prior[c] - q[c]) + add_noise  (never clamped),
 *     mean[c] = sum_r B[r,c] alpha[r]   (alpha[n] and mean both NULL: no mean).
 * (The engine calls it twice per chunk: with 2 B - K^ X in B's place for the variances -- x^T (2 b - K^ x) is below
 * b^T K^-1 b for any x, b^T x only while CG keeps its orthogonality -- and with B and alpha for the mean.)
 * Order rule (fp64, no floating-point atomics: two calls give the same bits, and a permutation of the columns
 * permutes the results bit for bit): with P the power of two >= min(n_rhs, 64) a wave covers 64 / P rows at a
 * time; the rows are cut into consecutive blocks whose length depends on (n, n_rhs) alone; within a block a lane
 * adds its rows ascending by fma from +0.0, lanes of one column by an xor tree, the eight waves in order; one
 * partial per (block, column); the last block (a ticket at the workspace's start, zero again afterwards) adds
 * them in block order within G = 512 / (64 ceil(n_rhs / 64)) groups of consecutive blocks, then the groups in
 * order.  Summation depth <= rows per lane + 6 + 7 + 256 blocks.
 * n_rhs in [0, 256] (0 touches nothing); n == 0 writes var = prior + add_noise and mean = 0.  var and mean must
 * overlap neither an input, the workspace nor each other.  Workspace: grf_posterior_reduce_workspace_bytes. */
int32_t grf_posterior_rhs_f64(int64_t n_rows, const int64_t *ptr, const int32_t *idx, const float *val,
                              int64_t n_cols, const int32_t *nodes, int32_t n_nodes, double *E, int64_t lde,
                              double *prior, grf_stream_t stream);
size_t grf_posterior_reduce_workspace_bytes(int64_t n, int32_t n_rhs);
int32_t grf_posterior_reduce_f64(int64_t n, int32_t n_rhs, const double *B, int64_t ldb, const double *X,
                                 int64_t ldx, const double *alpha, const double *prior, double add_noise,
                                 double *var, double *mean, void *workspace, size_t workspace_bytes,
                                 grf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GRF_H */
