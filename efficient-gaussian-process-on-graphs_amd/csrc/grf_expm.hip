// grf_expm.hip -- the exact diffusion kernel exp(-beta L) on the fp64 matrix cores of gfx950.
//
// grf_gemm_nt_f64   C = alpha A~ B~^T + gamma Z + delta I on v_mfma_f64_16x16x4_f64.  Both operands are read by
//                   rows (A~ = A through the row map ra, B~ = B through rb), so every fetch is contiguous.
// grf_expm_sym_f64  E = exp(-beta L) of a dense symmetric L by scaling and squaring: a host-side chain of
//                   grf_gemm_nt_f64 calls (degree-18 Taylor polynomial by Horner, then s squarings), no host read.
//
// The kernel.  One 128 x 128 tile of C per 256-thread workgroup; the four waves are 2 x 2, each owning 64 x 64 =
// 4 x 4 MFMA blocks of 16 x 16 (64 fp64 accumulators per lane).  The k dimension is cut into tiles of 16, staged
// through LDS as As[i][k] / Bs[j][k] with a row pitch of 18 doubles: a fragment read (lane -> row lane & 15,
// k = lane >> 4) then touches every bank pair once per 32-lane half, and the 16-byte staging writes stay aligned.
// The LDS ring is two k-tiles deep: while the MFMAs of k-tile t run from one slot, the global loads of k-tile
// t + 1 (issued before them) are in flight to registers and are written to the other slot afterwards -- one
// barrier per k-tile.  k past nk is staged as +0.0 and a row past n1 / n2 from the last valid row (it feeds only
// entries that are never written), so nothing outside the operands is read and padding (NaN or not) never
// enters a sum.
//
// Every entry of the product is ONE accumulator chain: k-tiles ascending, the four k-steps of a k-tile ascending,
// the four k of an MFMA in the instruction's own order.  No split-k, no floating-point atomics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "grf_common.h"

namespace grf {
namespace {

constexpr int kTile = 128;          // output tile (rows and columns)
constexpr int kKT = 16;             // k-tile depth
constexpr int kPitch = kKT + 2;     // LDS row pitch in doubles
constexpr int kRing = 2;            // LDS ring depth (k-tiles)
constexpr int kExpmDegree = 18;     // Taylor degree of grf_expm_sym_f64
constexpr int kExpmMaxSquarings = 64;

typedef double f64x4 __attribute__((ext_vector_type(4)));

enum GemmMode { kGeneral = 0, kSymmetric = 1, kContract = 2 };

struct GemmArgs {
    int64_t n1, n2, nk;
    const double *A;
    int64_t lda;
    const int32_t *ra;
    const double *B;
    int64_t ldb;
    const int32_t *rb;
    double alpha, gamma, delta;
    const double *Z;
    int64_t ldz;
    double *C;
    int64_t ldc;
    const double *W;
    int64_t ldw;
    double *part;
    uint32_t *ticket;
    double *out;
    int64_t tiles_j;
    int32_t vec_a, vec_b;  // rows are 16-byte aligned: stage with 16-byte loads
};

// two consecutive k of one operand row of a whole k-tile (no bounds to check)
__device__ __forceinline__ void load_pair(const double *row, int64_t k, bool vec, double &x, double &y) {
    if (vec) {
        const double2 v = *reinterpret_cast<const double2 *>(row + k);
        x = v.x;
        y = v.y;
    } else {
        x = row[k];
        y = row[k + 1];
    }
}

// the same in the last, partial k-tile: +0.0 past nk
__device__ __forceinline__ void load_pair_tail(const double *row, int64_t k, int64_t nk, double &x, double &y) {
    x = k < nk ? row[k] : 0.0;
    y = k + 1 < nk ? row[k + 1] : 0.0;
}

template <int MODE>
__global__ __launch_bounds__(256, 2) void gemm_nt_f64_kernel(GemmArgs a) {
    __shared__ __attribute__((aligned(16))) double As[kRing][kTile * kPitch];
    __shared__ __attribute__((aligned(16))) double Bs[kRing][kTile * kPitch];
    __shared__ double red[4];
    __shared__ uint32_t last;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    int64_t bi, bj;
    if constexpr (MODE == kSymmetric) {  // the tiles with bj >= bi, row by row
        int64_t t = blockIdx.x, len = a.tiles_j;
        bi = 0;
        while (t >= len) {
            t -= len;
            --len;
            ++bi;
        }
        bj = bi + t;
    } else {
        bi = blockIdx.x / a.tiles_j;
        bj = blockIdx.x - bi * a.tiles_j;
    }
    const int64_t i0 = bi * kTile, j0 = bj * kTile;
    // a diagonal tile's lower-left quarter is not kept: its wave stages and waits, but issues no MFMA
    const bool idle = MODE == kSymmetric && bi == bj && wm > wn;

    // staging: thread -> rows (tid >> 3) + 32 q, q < 4, and the k pair 2 (tid & 7) of the k-tile.  A row past
    // n1 / n2 is staged from the last valid row instead of zeros (no branch in the loop): it only feeds
    // accumulators of entries that are never written or contracted.
    const int srow = tid >> 3, sk = (tid & 7) * 2;
    const double *pa[4], *pb[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t i = min(i0 + srow + 32 * q, a.n1 - 1), j = min(j0 + srow + 32 * q, a.n2 - 1);
        pa[q] = a.A + (a.ra ? (int64_t)a.ra[i] : i) * a.lda;
        pb[q] = a.B + (a.rb ? (int64_t)a.rb[j] : j) * a.ldb;
    }
    double sa[4][2], sb[4][2];
    auto stage_load = [&](int64_t k0) {
        const int64_t k = k0 + sk;
        if (k0 + kKT <= a.nk) {  // (uniform) a whole k-tile
#pragma unroll
            for (int q = 0; q < 4; ++q) load_pair(pa[q], k, a.vec_a != 0, sa[q][0], sa[q][1]);
#pragma unroll
            for (int q = 0; q < 4; ++q) load_pair(pb[q], k, a.vec_b != 0, sb[q][0], sb[q][1]);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                load_pair_tail(pa[q], k, a.nk, sa[q][0], sa[q][1]);
                load_pair_tail(pb[q], k, a.nk, sb[q][0], sb[q][1]);
            }
        }
    };
    auto stage_write = [&](int slot) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int o = (srow + 32 * q) * kPitch + sk;
            *reinterpret_cast<double2 *>(&As[slot][o]) = double2{sa[q][0], sa[q][1]};
            *reinterpret_cast<double2 *>(&Bs[slot][o]) = double2{sb[q][0], sb[q][1]};
        }
    };

    f64x4 acc[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] = f64x4{0.0, 0.0, 0.0, 0.0};

    const int64_t n_kt = cdiv<int64_t>(a.nk, kKT);
    if (n_kt > 0) {
        stage_load(0);
        stage_write(0);
    }
    __syncthreads();
    for (int64_t t = 0; t < n_kt; ++t) {
        const int cur = (int)(t & 1);
        const bool more = t + 1 < n_kt;
        if (more) stage_load((t + 1) * kKT);
        if (!idle) {
            const double *as = &As[cur][(wm * 64 + (lane & 15)) * kPitch + (lane >> 4)];
            const double *bs = &Bs[cur][(wn * 64 + (lane & 15)) * kPitch + (lane >> 4)];
#pragma unroll
            for (int ks = 0; ks < kKT; ks += 4) {
                double fa[4], fb[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    fa[u] = as[u * 16 * kPitch + ks];
                    fb[u] = bs[u * 16 * kPitch + ks];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int v = 0; v < 4; ++v)
                        acc[u][v] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[u], fb[v], acc[u][v], 0, 0, 0);
            }
        }
        if (more) stage_write(cur ^ 1);
        __syncthreads();
    }

    // epilogue: C/D map of v_mfma_f64_16x16x4_f64 -- col = lane & 15, row = (lane >> 4) + 4 r.
    // value = RN(RN(RN(alpha acc) + RN(gamma Z[i, j])) + delta [i == j]), the addends only where present
    double csum = 0.0;
    if (!idle) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int v = 0; v < 4; ++v)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int64_t i = i0 + wm * 64 + u * 16 + (lane >> 4) + 4 * r;
                    const int64_t j = j0 + wn * 64 + v * 16 + (lane & 15);
                    if (i >= a.n1 || j >= a.n2) continue;
                    if (MODE == kSymmetric && j < i) continue;
                    double c = a.alpha * acc[u][v][r];
                    if (a.Z) c = c + a.gamma * a.Z[i * a.ldz + j];
                    if (i == j) c = c + a.delta;
                    if constexpr (MODE == kContract) {
                        csum = fma(a.W[i * a.ldw + j], c, csum);
                    } else {
                        a.C[i * a.ldc + j] = c;
                        if (MODE == kSymmetric && j > i) a.C[j * a.ldc + i] = c;
                    }
                }
    }
    if constexpr (MODE == kContract) {
        // a lane's entries in the loop's order, the lanes by an xor tree, the four waves in order, one partial
        // per tile; the last tile (by ticket, zero again afterwards) adds the partials in tile order
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) csum += __shfl_xor(csum, off);
        if (lane == 0) red[wave] = csum;
        __syncthreads();
        if (tid == 0) a.part[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
        __threadfence();
        __syncthreads();
        if (tid == 0) last = atomicAdd(a.ticket, 1u) == gridDim.x - 1;
        __syncthreads();
        if (!last) return;
        __threadfence();
        if (tid == 0) {
            double sum = 0.0;
            for (unsigned b = 0; b < gridDim.x; ++b) sum += __builtin_nontemporal_load(&a.part[b]);
            a.out[0] = sum;
            *a.ticket = 0u;
        }
    }
}

bool overlaps(const void *p, size_t pn, const void *q, size_t qn) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return pn && qn && a < b + qn && b < a + pn;
}

// bytes spanned by `rows` rows of `cols` doubles at pitch ld
size_t span(int64_t rows, int64_t cols, int64_t ld) {
    if (rows <= 0 || cols <= 0) return 0;
    return ((size_t)(rows - 1) * (size_t)ld + (size_t)cols) * sizeof(double);
}

int64_t tiles_of(int64_t n) { return cdiv<int64_t>(n, kTile); }

}  // namespace
}  // namespace grf

using namespace grf;

extern "C" {
#pragma GCC visibility push(default)

size_t grf_gemm_nt_f64_workspace_bytes(int64_t n1, int64_t n2) {
    const int64_t tiles = tiles_of(std::max<int64_t>(n1, 1)) * tiles_of(std::max<int64_t>(n2, 1));
    return 256 + al256((size_t)tiles * sizeof(double));  // the ticket, one partial per tile
}

int32_t grf_gemm_nt_f64(int64_t n1, int64_t n2, int64_t nk, double alpha, const double *A, int64_t lda,
                        int64_t a_rows, const int32_t *ra, const double *B, int64_t ldb, int64_t b_rows,
                        const int32_t *rb, double gamma, const double *Z, int64_t ldz, double delta, double *C,
                        int64_t ldc, int32_t symmetric, const double *W, int64_t ldw, double *out, void *workspace,
                        size_t workspace_bytes, grf_stream_t stream) {
    GRF_REQUIRE(n1 >= 0 && n2 >= 0 && nk >= 0, GRF_EINVAL, "grf_gemm_nt_f64: negative size");
    GRF_REQUIRE(n1 < (1ll << 31) && n2 < (1ll << 31), GRF_EUNSUPPORTED, "grf_gemm_nt_f64: more than 2^31 rows");
    if (n1 == 0 || n2 == 0) return GRF_OK;
    const bool contract = W != nullptr;
    GRF_REQUIRE(nk == 0 || (A && B && lda >= nk && ldb >= nk), GRF_EINVAL,
                "grf_gemm_nt_f64: operands missing or lda / ldb below nk");
    GRF_REQUIRE(nk == 0 || ((ra ? a_rows >= 1 : a_rows == n1) && (rb ? b_rows >= 1 : b_rows == n2)), GRF_EINVAL,
                "grf_gemm_nt_f64: a_rows / b_rows must be n1 / n2 without a row map (and >= 1 with one)");
    GRF_REQUIRE(!Z || ldz >= n2, GRF_EINVAL, "grf_gemm_nt_f64: ldz below n2");
    GRF_REQUIRE(!symmetric || (n1 == n2 && !ra && !rb && !contract), GRF_EINVAL,
                "grf_gemm_nt_f64: the symmetric mode needs n1 == n2, no row maps and no contraction");
    if (contract) {
        GRF_REQUIRE(ldw >= n2 && out, GRF_EINVAL, "grf_gemm_nt_f64: contraction needs ldw >= n2 and out");
        const size_t need = grf_gemm_nt_f64_workspace_bytes(n1, n2);
        GRF_REQUIRE(workspace && workspace_bytes >= need, GRF_EINVAL,
                    "grf_gemm_nt_f64: workspace too small (%zu < %zu)", workspace_bytes, need);
    } else {
        GRF_REQUIRE(C && ldc >= n2, GRF_EINVAL, "grf_gemm_nt_f64: C missing or ldc below n2");
        const size_t cn = span(n1, n2, ldc);
        if (nk > 0)
            GRF_REQUIRE(!overlaps(C, cn, A, span(a_rows, nk, lda)) && !overlaps(C, cn, B, span(b_rows, nk, ldb)),
                        GRF_EINVAL, "grf_gemm_nt_f64: C overlaps an operand");
        GRF_REQUIRE(!Z || (Z == C && ldz == ldc) || !overlaps(C, cn, Z, span(n1, n2, ldz)), GRF_EINVAL,
                    "grf_gemm_nt_f64: Z may alias C exactly (same pitch) or not overlap it");
    }
    hipStream_t st = S(stream);
    GemmArgs a{};
    a.n1 = n1; a.n2 = n2; a.nk = nk;
    a.A = A; a.lda = lda; a.ra = ra; a.B = B; a.ldb = ldb; a.rb = rb;
    a.alpha = alpha; a.gamma = gamma; a.delta = delta;
    a.Z = Z; a.ldz = ldz; a.C = C; a.ldc = ldc; a.W = W; a.ldw = ldw; a.out = out;
    a.tiles_j = tiles_of(n2);
    a.vec_a = nk > 0 && (lda % 2 == 0) && ((uintptr_t)A % 16 == 0);
    a.vec_b = nk > 0 && (ldb % 2 == 0) && ((uintptr_t)B % 16 == 0);
    const int64_t ti = tiles_of(n1), tj = tiles_of(n2);
    const int64_t blocks = symmetric ? ti * (ti + 1) / 2 : ti * tj;
    GRF_REQUIRE_GRID(blocks, 256, "gemm_nt_f64_kernel");
    if (contract) {
        a.ticket = (uint32_t *)workspace;
        a.part = (double *)((char *)workspace + 256);
        GRF_CHECK_HIP(hipMemsetAsync(workspace, 0, 256, st));
        gemm_nt_f64_kernel<kContract><<<(unsigned)blocks, 256, 0, st>>>(a);
    } else if (symmetric) {
        gemm_nt_f64_kernel<kSymmetric><<<(unsigned)blocks, 256, 0, st>>>(a);
    } else {
        gemm_nt_f64_kernel<kGeneral><<<(unsigned)blocks, 256, 0, st>>>(a);
    }
    GRF_CHECK_LAUNCH("gemm_nt_f64_kernel");
    return GRF_OK;
}

int32_t grf_expm_squarings(double rho) {
    if (!std::isfinite(rho)) return -1;
    if (!(rho > 1.0)) return 0;
    int e = 0;
    const double m = std::frexp(rho, &e);  // rho = m 2^e, m in [0.5, 1)
    return m == 0.5 ? e - 1 : e;           // ceil(log2 rho), exactly
}

size_t grf_expm_sym_f64_workspace_bytes(int64_t n) {
    const size_t ld = ((size_t)std::max<int64_t>(n, 1) + 1) & ~(size_t)1;
    return 3 * al256((size_t)std::max<int64_t>(n, 1) * ld * sizeof(double));  // X and the two ping-pong buffers
}

int32_t grf_expm_sym_f64(int64_t n, const double *L, int64_t ldl, double beta, double rho, double *E, int64_t lde,
                         void *workspace, size_t workspace_bytes, grf_stream_t stream) {
    GRF_REQUIRE(n >= 1 && L && E && ldl >= n && lde >= n, GRF_EINVAL, "grf_expm_sym_f64: bad arguments");
    GRF_REQUIRE(n < (1ll << 31), GRF_EUNSUPPORTED, "grf_expm_sym_f64: more than 2^31 rows");
    GRF_REQUIRE(std::isfinite(beta) && beta > 0.0 && std::isfinite(rho), GRF_EINVAL,
                "grf_expm_sym_f64: beta must be positive and finite, rho finite");
    const int32_t s = grf_expm_squarings(rho);
    GRF_REQUIRE(s >= 0 && s <= kExpmMaxSquarings, GRF_EINVAL, "grf_expm_sym_f64: rho needs %d squarings (at most %d)",
                s, kExpmMaxSquarings);
    const size_t need = grf_expm_sym_f64_workspace_bytes(n);
    GRF_REQUIRE(workspace && workspace_bytes >= need, GRF_EINVAL, "grf_expm_sym_f64: workspace too small (%zu < %zu)",
                workspace_bytes, need);
    GRF_REQUIRE(!overlaps(E, span(n, n, lde), L, span(n, n, ldl)) && !overlaps(E, span(n, n, lde), workspace, need) &&
                    !overlaps(L, span(n, n, ldl), workspace, need),
                GRF_EINVAL, "grf_expm_sym_f64: E, L and the workspace must not overlap");
    const int64_t ld = (n + 1) & ~(int64_t)1;
    char *w = (char *)workspace;
    double *X = (double *)w;
    double *P[2] = {(double *)(w + need / 3), (double *)(w + 2 * (need / 3))};
    auto gemm = [&](int64_t nk, double alpha, const double *A, int64_t lda, const double *B, int64_t ldb, double gamma,
                    const double *Z, int64_t ldz, double delta, double *C, int64_t ldc, int32_t sym) {
        return grf_gemm_nt_f64(n, n, nk, alpha, A, lda, n, nullptr, B, ldb, n, nullptr, gamma, Z, ldz, delta, C, ldc,
                               sym, nullptr, 0, nullptr, nullptr, 0, stream);
    };
    // X = -beta 2^-s L;  H_18 = I + X / 18
    int32_t rc = gemm(0, 0.0, nullptr, 0, nullptr, 0, std::ldexp(-beta, -s), L, ldl, 0.0, X, ld, 0);
    if (rc != GRF_OK) return rc;
    rc = gemm(0, 0.0, nullptr, 0, nullptr, 0, 1.0 / kExpmDegree, X, ld, 1.0, P[0], ld, 0);
    if (rc != GRF_OK) return rc;
    // H_k = I + (X H_{k+1}) / k, k = 17 .. 1, then s squarings; the last product of all goes to E
    const int32_t products = (kExpmDegree - 1) + s;
    int cur = 0;
    for (int32_t q = 0; q < products; ++q) {
        const bool final_product = q + 1 == products;
        double *dst = final_product ? E : P[cur ^ 1];
        const int64_t ldd = final_product ? lde : ld;
        if (q < kExpmDegree - 1) {
            const int k = kExpmDegree - 1 - q;
            rc = gemm(n, 1.0 / k, X, ld, P[cur], ld, 0.0, nullptr, 0, 1.0, dst, ldd, 1);
        } else {
            rc = gemm(n, 1.0, P[cur], ld, P[cur], ld, 0.0, nullptr, 0, 0.0, dst, ldd, 1);
        }
        if (rc != GRF_OK) return rc;
        cur ^= 1;
    }
    return GRF_OK;
}

#pragma GCC visibility pop
}  // extern "C"
