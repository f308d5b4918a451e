// grf_potrf.hip -- dense exact GP regression: a blocked fp64 Cholesky factorisation and triangular solves.
//
// grf_potrf_f64  F = chol(A), blocked right-looking with block edge 128: per block step potf2_kernel (the diagonal
//                block), trsm_block_kernel (the panel below it: each panel row is a right-hand side of L11 x = a)
//                and one symmetric-mode grf_gemm_nt_f64 (the trailing update on a workspace copy W of A).
// grf_trsm_f64   L x = b or L^T x = b for the rows b of B: per block step trsm_block_kernel, then one
//                grf_gemm_nt_f64 update of the remaining columns.
//
// potf2_kernel.  One workgroup of 128 threads, thread i owns row i of the block.  The block's lower triangle sits
// in LDS at a row pitch of 129 doubles: the column reads (lane -> row, fixed k) are 258 dwords apart, bank
// 2 lane mod 64, so the 32 lanes of a ds_read_b64 group touch every bank once.  Column j: every thread i >= j adds
// its own chain s = sum_{k<j} S[i][k] S[j][k] and, redundantly, the pivot's chain p = sum_{k<j} S[j][k]^2 (the
// row-j reads are broadcasts), so the pivot sqrt(S[j][j] - p) needs no second barrier; then S[i][j] =
// (S[i][j] - s) / pivot and one barrier per column.  The pivots live in their own array, S[j][j] keeps A's entry.
//
// trsm_block_kernel.  One wave per workgroup, lane r owns right-hand side r0 + r.  The diagonal block is in LDS as
// a packed lower triangle (every read of it is a broadcast: one address per instruction); the 64 right-hand
// sides' block entries are in LDS as xs[k][lane] at pitch 65, staged through coalesced global reads (lane -> k)
// whose transposed LDS writes are 130 dwords apart (every bank once).  Substitution in order, in place in xs.
//
// Nothing here depends on the data: a failed factorisation propagates NaN, sets info and ends like any other.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "grf_common.h"
#include "grf_dense_solve.h"

namespace grf {
namespace {

constexpr int kNB = GRF_DENSE_SOLVE_NB;      // block edge
constexpr int kP = kNB + 1;                  // potf2's LDS row pitch in doubles
constexpr int kXP = 65;                      // trsm_block's pitch of xs[k][lane]
constexpr int kTri = kNB * (kNB + 1) / 2;    // packed lower triangle
constexpr int kCopyTile = 32;

// W = the symmetric matrix whose lower triangle is A's (A's strict upper triangle is never read); block 0 also
// starts logdet and info
__global__ __launch_bounds__(256) void sym_copy_kernel(int64_t n, const double *A, int64_t lda, double *W, int64_t ldw,
                                                       int64_t tiles, double *logdet, int32_t *info) {
    __shared__ double t[kCopyTile][kCopyTile + 1];
    // the lower-triangular tiles only, row by row: block b is tile (bi, bj), b = bi (bi + 1) / 2 + bj, bj <= bi
    const int64_t b = blockIdx.x;
    int64_t bi = (int64_t)((sqrt(8.0 * (double)b + 1.0) - 1.0) * 0.5);
    while (bi * (bi + 1) / 2 > b) --bi;
    while ((bi + 1) * (bi + 2) / 2 <= b) ++bi;
    const int64_t bj = b - bi * (bi + 1) / 2;
    if (bi >= tiles) return;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *logdet = 0.0;
        *info = 0;
    }
    for (int e = threadIdx.x; e < kCopyTile * kCopyTile; e += 256) {
        const int r = e / kCopyTile, c = e % kCopyTile;
        const int64_t i = bi * kCopyTile + r, j = bj * kCopyTile + c;
        t[r][c] = (i < n && j <= i) ? A[i * lda + j] : 0.0;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < kCopyTile * kCopyTile; e += 256) {
        const int r = e / kCopyTile, c = e % kCopyTile;
        if (bi == bj) {
            const int64_t i = bi * kCopyTile + r, j = bj * kCopyTile + c;
            if (i < n && j < n) W[i * ldw + j] = c <= r ? t[r][c] : t[c][r];
        } else {
            const int64_t i = bi * kCopyTile + r, j = bj * kCopyTile + c;
            if (i < n && j < n) W[i * ldw + j] = t[r][c];
            const int64_t it = bj * kCopyTile + r, jt = bi * kCopyTile + c;
            if (it < n && jt < n) W[it * ldw + jt] = t[c][r];
        }
    }
}

// the b x b diagonal block at W (lower triangle read) -> F (both triangles); logdet and info are carried on
__global__ __launch_bounds__(kNB) void potf2_kernel(const double *W, int64_t ldw, int b, int64_t j0, double *F,
                                                    int64_t ldf, double *logdet, int32_t *info) {
    __shared__ double S[kNB * kP];
    __shared__ double dg[kNB];
    __shared__ double lg[kNB];
    const int i = threadIdx.x;
    for (int r = 0; r < b; ++r)
        if (i <= r) S[r * kP + i] = W[(int64_t)r * ldw + i];
    __syncthreads();
    for (int j = 0; j < b; ++j) {
        if (i >= j && i < b) {
            const double *ri = &S[i * kP], *rj = &S[j * kP];
            double s = 0.0, p = 0.0;
            for (int k = 0; k < j; ++k) {
                const double a = rj[k];
                s += ri[k] * a;
                p += a * a;
            }
            const double piv = sqrt(rj[j] - p);
            if (i == j)
                dg[j] = piv;
            else
                S[i * kP + j] = (ri[j] - s) / piv;
        }
        __syncthreads();
    }
    if (i < b) {
        for (int r = 0; r < b; ++r)
            F[(int64_t)r * ldf + i] = i < r ? S[r * kP + i] : (i == r ? dg[r] : S[i * kP + r]);
        lg[i] = 2.0 * log(dg[i]);
    }
    __syncthreads();
    if (i == 0) {
        int32_t bad = *info;
        double ld = *logdet;
        for (int r = 0; r < b; ++r) {
            const double piv = dg[r];
            if (bad == 0 && !(piv > 0.0 && piv < INFINITY)) bad = (int32_t)(j0 + r + 1);
            ld += lg[r];
        }
        *info = bad;
        *logdet = bad ? (double)NAN : ld;
    }
}

struct TrsmArgs {
    const double *T;   // the b x b diagonal block inside F (its lower triangle is read)
    int64_t ldt;
    int32_t b;
    int64_t nrhs;
    const double *src;  // nrhs x b block of right-hand sides
    int64_t lds;
    double *dst;        // nrhs x b solutions (may be src)
    int64_t ldd;
    double *copy;       // optional second copy of the solutions
    int64_t ldc;
    double *mirror;     // optional transposed copy: mirror[k * ldm + r]
    int64_t ldm;
};

template <bool TRANS>
__global__ __launch_bounds__(64) void trsm_block_kernel(TrsmArgs a) {
    __shared__ double Lp[kTri];
    __shared__ double xs[kNB * kXP];
    const int lane = threadIdx.x, b = a.b;
    const int64_t r0 = (int64_t)blockIdx.x * 64;
    const int rows = (int)min((int64_t)64, a.nrhs - r0);
    for (int r = 0; r < b; ++r)
        for (int c = lane; c <= r; c += 64) Lp[r * (r + 1) / 2 + c] = a.T[(int64_t)r * a.ldt + c];
    for (int rr = 0; rr < 64; ++rr)
        for (int k = lane; k < b; k += 64)
            xs[k * kXP + rr] = rr < rows ? a.src[(r0 + rr) * a.lds + k] : 0.0;
    __syncthreads();
    if (!TRANS) {
        for (int i = 0; i < b; ++i) {
            const double *li = &Lp[i * (i + 1) / 2];
            double s = 0.0;
            for (int k = 0; k < i; ++k) s += li[k] * xs[k * kXP + lane];
            xs[i * kXP + lane] = (xs[i * kXP + lane] - s) / li[i];
        }
    } else {
        for (int i = b - 1; i >= 0; --i) {
            double s = 0.0;
            for (int k = i + 1; k < b; ++k) s += Lp[k * (k + 1) / 2 + i] * xs[k * kXP + lane];
            xs[i * kXP + lane] = (xs[i * kXP + lane] - s) / Lp[i * (i + 1) / 2 + i];
        }
    }
    __syncthreads();
    for (int rr = 0; rr < rows; ++rr)
        for (int k = lane; k < b; k += 64) {
            const double x = xs[k * kXP + rr];
            a.dst[(r0 + rr) * a.ldd + k] = x;
            if (a.copy) a.copy[(r0 + rr) * a.ldc + k] = x;
        }
    if (a.mirror && lane < rows)
        for (int k = 0; k < b; ++k) a.mirror[(int64_t)k * a.ldm + r0 + lane] = xs[k * kXP + lane];
}

bool overlaps(const void *p, size_t pn, const void *q, size_t qn) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return pn && qn && a < b + qn && b < a + pn;
}

// bytes spanned by `rows` rows of `cols` doubles at pitch ld; saturates (kSizeSaturated) instead of wrapping
size_t span(int64_t rows, int64_t cols, int64_t ld) {
    if (rows <= 0 || cols <= 0) return 0;
    const size_t limit = (kSizeSaturated / sizeof(double) - (size_t)cols);
    if (rows > 1 && (size_t)ld > limit / (size_t)(rows - 1)) return kSizeSaturated;
    return ((size_t)(rows - 1) * (size_t)ld + (size_t)cols) * sizeof(double);
}

// a buffer whose span saturated, or whose end would wrap the address space, cannot be checked for overlap
bool addressable(const void *p, size_t bytes) {
    return bytes != kSizeSaturated && (uintptr_t)p <= ~(uintptr_t)0 - bytes;
}

int64_t even(int64_t n) { return (n + 1) & ~(int64_t)1; }

int32_t launch_trsm_block(bool transposed, const TrsmArgs &a, hipStream_t st) {
    const int64_t blocks = cdiv<int64_t>(a.nrhs, 64);
    GRF_REQUIRE_GRID(blocks, 64, "trsm_block_kernel");
    if (transposed)
        trsm_block_kernel<true><<<(unsigned)blocks, 64, 0, st>>>(a);
    else
        trsm_block_kernel<false><<<(unsigned)blocks, 64, 0, st>>>(a);
    GRF_CHECK_LAUNCH("trsm_block_kernel");
    return GRF_OK;
}

// C <- C - A B^T (C aliasing Z) through the public product
int32_t gemm_update(int64_t n1, int64_t n2, int64_t nk, const double *A, int64_t lda, const double *B, int64_t ldb,
                    double *C, int64_t ldc, int32_t symmetric, grf_stream_t stream) {
    return grf_gemm_nt_f64(n1, n2, nk, -1.0, A, lda, n1, nullptr, B, ldb, n2, nullptr, 1.0, C, ldc, 0.0, C, ldc,
                           symmetric, nullptr, 0, nullptr, nullptr, 0, stream);
}

}  // namespace
}  // namespace grf

using namespace grf;

extern "C" {
#pragma GCC visibility push(default)

size_t grf_potrf_f64_workspace_bytes(int64_t n) {
    if (n > kMaxIds) return kSizeSaturated;
    const int64_t m = std::max<int64_t>(n, 1);
    return al256((size_t)m * (size_t)even(m) * sizeof(double));
}

int32_t grf_potrf_f64(int64_t n, const double *A, int64_t lda, double *F, int64_t ldf, double *logdet,
                      int32_t *info, void *workspace, size_t workspace_bytes, grf_stream_t stream) {
    GRF_REQUIRE(n >= 0, GRF_EINVAL, "grf_potrf_f64: negative size");
    GRF_REQUIRE(n < (1ll << 31), GRF_EUNSUPPORTED, "grf_potrf_f64: more than 2^31 rows");
    GRF_REQUIRE(n >= 1, GRF_EINVAL, "grf_potrf_f64: n must be at least 1 (logdet and info are written)");
    GRF_REQUIRE(A && F && logdet && info, GRF_EINVAL, "grf_potrf_f64: A, F, logdet or info missing");
    GRF_REQUIRE(lda >= n && ldf >= n, GRF_EINVAL, "grf_potrf_f64: lda / ldf below n");
    const size_t need = grf_potrf_f64_workspace_bytes(n);
    GRF_REQUIRE(workspace && workspace_bytes >= need, GRF_EINVAL, "grf_potrf_f64: workspace too small (%zu < %zu)",
                workspace_bytes, need);
    GRF_REQUIRE(addressable(A, span(n, n, lda)) && addressable(F, span(n, n, ldf)), GRF_EINVAL,
                "grf_potrf_f64: lda / ldf too large: the matrix does not fit the address space");
    {
        const void *p[5] = {A, F, workspace, logdet, info};
        const size_t s[5] = {span(n, n, lda), span(n, n, ldf), need, sizeof(double), sizeof(int32_t)};
        for (int x = 0; x < 5; ++x)
            for (int y = x + 1; y < 5; ++y)
                GRF_REQUIRE(!overlaps(p[x], s[x], p[y], s[y]), GRF_EINVAL,
                            "grf_potrf_f64: A, F, the workspace, logdet and info must not overlap");
    }
    hipStream_t st = S(stream);
    double *W = (double *)workspace;
    const int64_t ldw = even(n);
    const int64_t tiles = cdiv<int64_t>(n, kCopyTile);
    const int64_t copy_blocks = tiles * (tiles + 1) / 2;
    GRF_REQUIRE_GRID(copy_blocks, 256, "sym_copy_kernel");
    sym_copy_kernel<<<(unsigned)copy_blocks, 256, 0, st>>>(n, A, lda, W, ldw, tiles, logdet, info);
    GRF_CHECK_LAUNCH("sym_copy_kernel");
    for (int64_t j0 = 0; j0 < n; j0 += kNB) {
        const int b = (int)std::min<int64_t>(kNB, n - j0);
        const int64_t j1 = j0 + b, rest = n - j1;
        potf2_kernel<<<1, kNB, 0, st>>>(W + j0 * ldw + j0, ldw, b, j0, F + j0 * ldf + j0, ldf, logdet, info);
        GRF_CHECK_LAUNCH("potf2_kernel");
        if (rest == 0) break;
        TrsmArgs t{};
        t.T = F + j0 * ldf + j0; t.ldt = ldf; t.b = b; t.nrhs = rest;
        t.src = W + j1 * ldw + j0; t.lds = ldw;
        t.dst = F + j1 * ldf + j0; t.ldd = ldf;
        t.mirror = F + j0 * ldf + j1; t.ldm = ldf;
        int32_t rc = launch_trsm_block(false, t, st);
        if (rc != GRF_OK) return rc;
        rc = gemm_update(rest, rest, b, F + j1 * ldf + j0, ldf, F + j1 * ldf + j0, ldf, W + j1 * ldw + j1, ldw, 1,
                         stream);
        if (rc != GRF_OK) return rc;
    }
    return GRF_OK;
}

size_t grf_trsm_f64_workspace_bytes(int64_t n, int64_t nrhs) {
    (void)n;
    if (nrhs > kMaxIds) return kSizeSaturated;
    return al256((size_t)std::max<int64_t>(nrhs, 1) * kNB * sizeof(double));
}

int32_t grf_trsm_f64(int64_t n, int64_t nrhs, const double *F, int64_t ldf, int32_t transposed, double *B,
                     int64_t ldb, void *workspace, size_t workspace_bytes, grf_stream_t stream) {
    GRF_REQUIRE(n >= 0 && nrhs >= 0, GRF_EINVAL, "grf_trsm_f64: negative size");
    GRF_REQUIRE(n < (1ll << 31) && nrhs < (1ll << 31), GRF_EUNSUPPORTED,
                "grf_trsm_f64: more than 2^31 rows or right-hand sides");
    if (n == 0 || nrhs == 0) return GRF_OK;
    GRF_REQUIRE(F && B, GRF_EINVAL, "grf_trsm_f64: F or B missing");
    GRF_REQUIRE(ldf >= n && ldb >= n, GRF_EINVAL, "grf_trsm_f64: ldf / ldb below n");
    const size_t need = grf_trsm_f64_workspace_bytes(n, nrhs);
    GRF_REQUIRE(workspace && workspace_bytes >= need, GRF_EINVAL, "grf_trsm_f64: workspace too small (%zu < %zu)",
                workspace_bytes, need);
    const size_t fs = span(n, n, ldf), bs = span(nrhs, n, ldb);
    GRF_REQUIRE(addressable(F, fs) && addressable(B, bs), GRF_EINVAL,
                "grf_trsm_f64: ldf / ldb too large: the matrix does not fit the address space");
    GRF_REQUIRE(!overlaps(F, fs, B, bs) && !overlaps(F, fs, workspace, need) && !overlaps(B, bs, workspace, need),
                GRF_EINVAL, "grf_trsm_f64: F, B and the workspace must not overlap");
    hipStream_t st = S(stream);
    double *X = (double *)workspace;  // nrhs x kNB: the current block's solutions
    const int64_t n_blocks = cdiv<int64_t>(n, kNB);
    for (int64_t q = 0; q < n_blocks; ++q) {
        const int64_t j0 = (transposed ? n_blocks - 1 - q : q) * kNB;
        const int b = (int)std::min<int64_t>(kNB, n - j0);
        const int64_t j1 = j0 + b;
        const int64_t rest = transposed ? j0 : n - j1;  // the columns still to be updated
        TrsmArgs t{};
        t.T = F + j0 * ldf + j0; t.ldt = ldf; t.b = b; t.nrhs = nrhs;
        t.src = B + j0; t.lds = ldb;
        t.dst = B + j0; t.ldd = ldb;
        if (rest > 0) {
            t.copy = X;
            t.ldc = kNB;
        }
        int32_t rc = launch_trsm_block(transposed != 0, t, st);
        if (rc != GRF_OK) return rc;
        if (rest == 0) continue;
        // L: B[:, j1:] -= X L[j1:, J]^T;  L^T: B[:, :j0] -= X (L[J, :j0])^T, read from F's mirrored upper triangle
        const int64_t c0 = transposed ? 0 : j1;
        rc = gemm_update(nrhs, rest, b, X, kNB, F + c0 * ldf + j0, ldf, B + c0, ldb, 0, stream);
        if (rc != GRF_OK) return rc;
    }
    return GRF_OK;
}

#pragma GCC visibility pop
}  // extern "C"
