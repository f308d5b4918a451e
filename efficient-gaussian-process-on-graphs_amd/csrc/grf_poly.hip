// grf_poly.hip -- the exact walk-power kernel as a matrix-free operator on gfx950.
//
// Phi = p(G) = sum_l f_l G^l is never formed (its powers fill in: G^4 of a mean-degree-20 graph is dense).
// Every product with it is a Horner chain of n_f - 1 SpMMs with the walk matrix itself,
//     H_{n_f-1} = f_{n_f-1} X,   H_l = G H_{l+1} + f_l X,   p(G) X = H_0,
// and K_TT V = S_T p(G) p(G)^T S_T^T V is two such chains (G^T, then G).
//
// Kernels
//   poly_step_kernel<NC>          one Horner step Y[r] = sum_e val[e] xs X[x(idx[e])] + a V[v(row(r))] + b P[r]:
//                                 fp64 matrix values, optional output row map, optional node -> row maps on
//                                 the gathered block and on the addend (rows without one contribute 0, so
//                                 S_T^T P is never stored as a zero-filled n x S block), the CG's done flag.
//   poly_krylov_frob_kernel<NC>   the gradient's step U_l = G^T U_{l-1}, V_l = G^T V_{l-1} fused with the weighted
//                                 column inner products <U_l, W_B> + <V_l, W_A>.
// One wave per output row; lane c owns the columns c + 64 i, i < NC = ceil(S / 64).  A row's indices and values
// are loaded once (64 at a time) and broadcast lane by lane for all NC chunks, so every gathered row is one
// contiguous S x 8-byte read.  Every sum has a fixed order (include/grf.h, "order rule"); no atomics on
// floating-point data.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "grf_poly.h"

namespace grf {
namespace {

constexpr int kKrylovBlocks = 512;  // row blocks of poly_krylov_frob_kernel (one fp64 partial each)

size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

__device__ inline double readlane_f64(double v, int j) {
    const uint64_t u = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int32_t)(uint32_t)u, j);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int32_t)(uint32_t)(u >> 32), j);
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

struct PolyStep {
    const int64_t *ptr;  // A (NULL: no matrix -- the sum over the row is empty)
    const int32_t *idx;
    const double *val;
    const int32_t *row_map;  // output row r is row row_map[r] of A (NULL: r)
    const double *X;         // the gathered block: row x_map[k] (NULL map: k) of X, times *xs (NULL: 1)
    int64_t ldx;
    const int32_t *x_map;
    const double *xs;
    const double *V;  // addend (*a) V[v_map[row]] (V NULL: none)
    int64_t ldv;
    const int32_t *v_map;
    const double *a;
    const double *P;  // addend b P[r] (NULL: none)
    int64_t ldp;
    double b;
    double *Y;
    int64_t ldy;
};

template <int NC>
__global__ __launch_bounds__(256) void poly_step_kernel(int64_t n_out, PolyStep p, int32_t S, const int32_t *done) {
    if (done && __builtin_nontemporal_load(done)) return;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    bool ok[NC];
    int col[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        ok[i] = lane + 64 * i < S;
        col[i] = ok[i] ? lane + 64 * i : 0;
    }
    const double xs = p.xs ? *p.xs : 1.0;  // (1.0 * x is x: the scale is exact when absent)
    const double a = p.V ? *p.a : 0.0;
    const int64_t n_waves = (int64_t)gridDim.x * 4;
    for (int64_t r = (int64_t)blockIdx.x * 4 + w; r < n_out; r += n_waves) {
        const int64_t row = uniform(p.row_map ? (int64_t)p.row_map[r] : r);
        double acc[NC];
#pragma unroll
        for (int i = 0; i < NC; ++i) acc[i] = 0.0;
        if (p.ptr) {
            const int64_t e0 = uniform(p.ptr[row]), e1 = uniform(p.ptr[row + 1]);
            for (int64_t eb = e0; eb < e1; eb += 64) {
                const int64_t e = eb + lane;
                int32_t k_l = e < e1 ? p.idx[e] : 0;
                const double v_l = e < e1 ? p.val[e] : 0.0;
                if (p.x_map) k_l = e < e1 ? p.x_map[k_l] : -1;
                const int cnt = (int)min<int64_t>(64, e1 - eb);
                int j = 0;
                for (; j + 4 <= cnt; j += 4) {  // four entries' rows of X in flight
                    double x[4][NC], v[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int64_t k = __builtin_amdgcn_readlane(k_l, j + u);
                        v[u] = readlane_f64(v_l, j + u);
#pragma unroll
                        for (int i = 0; i < NC; ++i) x[u][i] = (ok[i] && k >= 0) ? xs * p.X[k * p.ldx + col[i]] : 0.0;
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u)
#pragma unroll
                        for (int i = 0; i < NC; ++i) acc[i] = fma(v[u], x[u][i], acc[i]);
                }
                for (; j < cnt; ++j) {
                    const int64_t k = __builtin_amdgcn_readlane(k_l, j);
                    const double v = readlane_f64(v_l, j);
#pragma unroll
                    for (int i = 0; i < NC; ++i)
                        acc[i] = fma(v, (ok[i] && k >= 0) ? xs * p.X[k * p.ldx + col[i]] : 0.0, acc[i]);
                }
            }
        }
        if (p.V) {
            const int64_t q = uniform(p.v_map ? (int64_t)p.v_map[row] : row);
            if (q >= 0) {
#pragma unroll
                for (int i = 0; i < NC; ++i) acc[i] = fma(a, ok[i] ? p.V[q * p.ldv + col[i]] : 0.0, acc[i]);
            }
        }
        if (p.P) {
#pragma unroll
            for (int i = 0; i < NC; ++i) acc[i] = fma(p.b, ok[i] ? p.P[r * p.ldp + col[i]] : 0.0, acc[i]);
        }
#pragma unroll
        for (int i = 0; i < NC; ++i)
            if (ok[i]) p.Y[r * p.ldy + col[i]] = acc[i];
    }
}

int32_t poly_step_launch(int64_t n_out, const PolyStep &p, int32_t S, const int32_t *done, hipStream_t st) {
    if (n_out == 0) return GRF_OK;
    const unsigned blocks = (unsigned)std::min<int64_t>(cdiv<int64_t>(n_out, 4), 1 << 16);
#define GRF_POLY(NCV) poly_step_kernel<NCV><<<blocks, 256, 0, st>>>(n_out, p, S, done)
    if (S <= 64) GRF_POLY(1);
    else if (S <= 128) GRF_POLY(2);
    else if (S <= 192) GRF_POLY(3);
    else GRF_POLY(4);
#undef GRF_POLY
    GRF_CHECK_LAUNCH("poly_step_kernel");
    return GRF_OK;
}

// One step of both Krylov sequences and its contraction.  With ptr: UA = A XA~, UB = A XB~ (row r of A; X~ the
// block X through x_map); without: UA = XA~[r], UB = XB~[r] (step 0).  UA / UB are stored to YA / YB (pitch S)
// unless those are NULL, and
//     out[0] = sum_r sum_c wt[c] (UA[r,c] WB[r,c] + UB[r,c] WA[r,c])
// summed in a fixed order: a wave's rows ascending (columns c = lane, lane + 64, ... in turn), the lanes by an
// xor tree, the four waves in order, one fp64 partial per block, and the last block (by ticket, reset
// afterwards) adds the partials in block order.
template <int NC>
__global__ __launch_bounds__(256) void poly_krylov_frob_kernel(int64_t n, const int64_t *ptr, const int32_t *idx,
                                                               const double *val, const double *XA,
                                                               const double *XB, int64_t ldx, const int32_t *x_map,
                                                               double *YA, double *YB, const double *WA,
                                                               const double *WB, const double *wt, int32_t S,
                                                               double *part, uint32_t *ticket, double *out) {
    __shared__ double red[4];
    __shared__ uint32_t last;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    bool ok[NC];
    int col[NC];
    double wgt[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        ok[i] = lane + 64 * i < S;
        col[i] = ok[i] ? lane + 64 * i : 0;
        wgt[i] = ok[i] ? wt[col[i]] : 0.0;
    }
    double acc = 0.0;
    const int64_t n_waves = (int64_t)gridDim.x * 4;
    for (int64_t r = (int64_t)blockIdx.x * 4 + w; r < n; r += n_waves) {
        double ua[NC], ub[NC];
#pragma unroll
        for (int i = 0; i < NC; ++i) ua[i] = ub[i] = 0.0;
        if (ptr) {
            const int64_t e0 = uniform(ptr[r]), e1 = uniform(ptr[r + 1]);
            for (int64_t eb = e0; eb < e1; eb += 64) {
                const int64_t e = eb + lane;
                int32_t k_l = e < e1 ? idx[e] : 0;
                const double v_l = e < e1 ? val[e] : 0.0;
                if (x_map) k_l = e < e1 ? x_map[k_l] : -1;
                const int cnt = (int)min<int64_t>(64, e1 - eb);
                int j = 0;
                for (; j + 2 <= cnt; j += 2) {  // two entries' rows of XA / XB in flight
                    double xa[2][NC], xb[2][NC], v[2];
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        const int64_t k = __builtin_amdgcn_readlane(k_l, j + u);
                        v[u] = readlane_f64(v_l, j + u);
#pragma unroll
                        for (int i = 0; i < NC; ++i) {
                            xa[u][i] = (ok[i] && k >= 0) ? XA[k * ldx + col[i]] : 0.0;
                            xb[u][i] = (ok[i] && k >= 0) ? XB[k * ldx + col[i]] : 0.0;
                        }
                    }
#pragma unroll
                    for (int u = 0; u < 2; ++u)
#pragma unroll
                        for (int i = 0; i < NC; ++i) {
                            ua[i] = fma(v[u], xa[u][i], ua[i]);
                            ub[i] = fma(v[u], xb[u][i], ub[i]);
                        }
                }
                for (; j < cnt; ++j) {
                    const int64_t k = __builtin_amdgcn_readlane(k_l, j);
                    const double v = readlane_f64(v_l, j);
#pragma unroll
                    for (int i = 0; i < NC; ++i) {
                        ua[i] = fma(v, (ok[i] && k >= 0) ? XA[k * ldx + col[i]] : 0.0, ua[i]);
                        ub[i] = fma(v, (ok[i] && k >= 0) ? XB[k * ldx + col[i]] : 0.0, ub[i]);
                    }
                }
            }
        } else {
            const int64_t q = uniform(x_map ? (int64_t)x_map[r] : r);
            if (q >= 0) {
#pragma unroll
                for (int i = 0; i < NC; ++i) {
                    ua[i] = ok[i] ? XA[q * ldx + col[i]] : 0.0;
                    ub[i] = ok[i] ? XB[q * ldx + col[i]] : 0.0;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            if (YA && ok[i]) {
                YA[r * S + col[i]] = ua[i];
                YB[r * S + col[i]] = ub[i];
            }
            const double wa = ok[i] ? WA[r * S + col[i]] : 0.0, wb = ok[i] ? WB[r * S + col[i]] : 0.0;
            acc = fma(wgt[i], fma(ua[i], wb, ub[i] * wa), acc);
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
    if (lane == 0) red[w] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) last = atomicAdd(ticket, 1u) == gridDim.x - 1;
    __syncthreads();
    if (!last) return;
    __threadfence();
    if (threadIdx.x == 0) {
        double sum = 0.0;
        for (unsigned bq = 0; bq < gridDim.x; ++bq) sum += __builtin_nontemporal_load(&part[bq]);
        out[0] = sum;
        *ticket = 0u;
    }
}

unsigned krylov_blocks(int64_t n) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv<int64_t>(n, 4), kKrylovBlocks));
}

struct GradLayout {
    size_t part, blk[6], total;
};

GradLayout grad_layout(int64_t n, int32_t S) {
    GradLayout l{};
    size_t o = 256;  // the ticket
    l.part = o; o += al256((size_t)krylov_blocks(n) * sizeof(double));
    for (int i = 0; i < 6; ++i) {
        l.blk[i] = o; o += al256((size_t)std::max<int64_t>(n, 1) * S * sizeof(double));
    }
    l.total = o;
    return l;
}

}  // namespace

int32_t poly_chain(const PolyOp &op, const int32_t *x_map, const double *X, int64_t ldx, int32_t S,
                   const int32_t *row_map, int64_t n_out, double *Y, int64_t ldy, const double *P, int64_t ldp,
                   double b, double *H0, double *H1, const int32_t *done, hipStream_t st) {
    PolyStep p{};
    p.V = X; p.ldv = ldx; p.v_map = x_map;
    double *H[2] = {H0, H1};
    const double *in = nullptr;  // the block the step gathers (the first step: X itself, scaled by f[n_f - 1])
    // l = n_f - 2 .. 0: H_l = A H_{l+1} + f_l X; n_f = 1 is the one step Y = f_0 X without a matrix
    for (int32_t l = std::max(op.n_f - 2, 0), q = 0;; --l, ++q) {
        if (op.n_f > 1) {
            p.ptr = op.ptr; p.idx = op.idx; p.val = op.val;
            if (!in) {
                p.X = X; p.ldx = ldx; p.x_map = x_map; p.xs = op.f + (op.n_f - 1);
            } else {
                p.X = in; p.ldx = S; p.x_map = nullptr; p.xs = nullptr;
            }
        }
        p.a = op.f + l;
        const bool final_step = l == 0;
        if (final_step) {
            p.row_map = row_map; p.Y = Y; p.ldy = ldy; p.P = P; p.ldp = ldp; p.b = b;
        } else {
            p.row_map = nullptr; p.Y = H[q & 1]; p.ldy = S;
        }
        const int32_t rc = poly_step_launch(final_step ? n_out : op.n, p, S, done, st);
        if (rc != GRF_OK || final_step) return rc;
        in = H[q & 1];
    }
}

}  // namespace grf

using namespace grf;

extern "C" {
#pragma GCC visibility push(default)

size_t grf_poly_workspace_bytes(int64_t n, int32_t n_f, int32_t n_rhs) {
    if (n_f <= 2) return 0;  // (no intermediate block)
    return 2 * al256((size_t)std::max<int64_t>(n, 1) * std::max<int32_t>(n_rhs, 1) * sizeof(double));
}

int32_t grf_poly_apply_f64(int64_t n, const int64_t *ptr, const int32_t *idx, const double *val, const double *f,
                           int32_t n_f, const int32_t *inv_map, const int32_t *row_map, int64_t n_out,
                           const double *X, int64_t ldx, int32_t n_rhs, double *Y, int64_t ldy, void *workspace,
                           size_t workspace_bytes, grf_stream_t stream) {
    GRF_REQUIRE(n >= 1 && n_out >= 0 && ptr && f && n_f >= 1 && X && Y, GRF_EINVAL, "grf_poly_apply_f64: bad arguments");
    GRF_REQUIRE(n < (1ll << 31) && n_out < (1ll << 31), GRF_EUNSUPPORTED, "grf_poly_apply_f64: more than 2^31 rows");
    GRF_REQUIRE(row_map || n_out == n, GRF_EINVAL, "grf_poly_apply_f64: n_out must be n without a row map");
    GRF_REQUIRE(n_rhs >= 1 && n_rhs <= kPolyMaxRhs, GRF_EUNSUPPORTED, "grf_poly_apply_f64: n_rhs must be in [1, %d]",
                kPolyMaxRhs);
    GRF_REQUIRE(ldx >= n_rhs && ldy >= n_rhs, GRF_EINVAL, "grf_poly_apply_f64: bad strides");
    const size_t need = grf_poly_workspace_bytes(n, n_f, n_rhs);
    GRF_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), GRF_EINVAL,
                "grf_poly_apply_f64: workspace too small (%zu < %zu)", workspace_bytes, need);
    const PolyOp op{n, ptr, idx, val, f, n_f};
    double *H0 = (double *)workspace, *H1 = need ? (double *)((char *)workspace + need / 2) : nullptr;
    return poly_chain(op, inv_map, X, ldx, n_rhs, row_map, n_out, Y, ldy, nullptr, 0, 0.0, H0, H1, nullptr,
                      S(stream));
}

size_t grf_poly_grad_workspace_bytes(int64_t n, int32_t n_rhs) {
    return grad_layout(n, std::max<int32_t>(n_rhs, 1)).total;
}

int32_t grf_poly_grad_f64(int64_t n, const int64_t *gt_ptr, const int32_t *gt_idx, const double *gt_val,
                          const double *f, int32_t n_f, int64_t n_sel, const int32_t *inv_map, const double *A,
                          const double *B, int64_t ld, const double *wt, int32_t n_rhs, double *out, void *workspace,
                          size_t workspace_bytes, grf_stream_t stream) {
    GRF_REQUIRE(n >= 1 && n_sel >= 1 && gt_ptr && f && n_f >= 1 && inv_map && A && B && wt && out, GRF_EINVAL,
                "grf_poly_grad_f64: bad arguments");
    GRF_REQUIRE(n < (1ll << 31) && n_sel < (1ll << 31), GRF_EUNSUPPORTED, "grf_poly_grad_f64: more than 2^31 rows");
    GRF_REQUIRE(n_rhs >= 1 && n_rhs <= kPolyMaxRhs, GRF_EUNSUPPORTED, "grf_poly_grad_f64: n_rhs must be in [1, %d]",
                kPolyMaxRhs);
    GRF_REQUIRE(ld >= n_rhs, GRF_EINVAL, "grf_poly_grad_f64: bad strides");
    const GradLayout l = grad_layout(n, n_rhs);
    GRF_REQUIRE(workspace && workspace_bytes >= l.total, GRF_EINVAL,
                "grf_poly_grad_f64: workspace too small (%zu < %zu)", workspace_bytes, l.total);
    hipStream_t st = S(stream);
    char *w = (char *)workspace;
    uint32_t *ticket = (uint32_t *)w;
    double *part = (double *)(w + l.part);
    double *WA = (double *)(w + l.blk[0]), *WB = (double *)(w + l.blk[1]);
    double *U[2] = {(double *)(w + l.blk[2]), (double *)(w + l.blk[3])};
    double *V[2] = {(double *)(w + l.blk[4]), (double *)(w + l.blk[5])};
    GRF_CHECK_HIP(hipMemsetAsync(ticket, 0, 256, st));
    // W_A = p(G^T) S_T^T A, W_B = p(G^T) S_T^T B (the U / V blocks serve as the chains' intermediates)
    const PolyOp op{n, gt_ptr, gt_idx, gt_val, f, n_f};
    int32_t rc = poly_chain(op, inv_map, A, ld, n_rhs, nullptr, n, WA, n_rhs, nullptr, 0, 0.0, U[0], U[1], nullptr, st);
    if (rc != GRF_OK) return rc;
    rc = poly_chain(op, inv_map, B, ld, n_rhs, nullptr, n, WB, n_rhs, nullptr, 0, 0.0, V[0], V[1], nullptr, st);
    if (rc != GRF_OK) return rc;
    const unsigned blocks = krylov_blocks(n);
    for (int32_t s = 0; s < n_f; ++s) {
        // step 0 contracts S_T^T A / S_T^T B themselves; step 1 gathers them through inv_map; later steps the
        // stored U_{s-1} / V_{s-1}.  The last step's U / V are not stored.
        const bool first = s <= 1, store = s >= 1 && s + 1 < n_f;
        const double *xa = first ? A : U[(s - 1) & 1], *xb = first ? B : V[(s - 1) & 1];
        const int64_t ldx = first ? ld : n_rhs;
        double *ya = store ? U[s & 1] : nullptr, *yb = store ? V[s & 1] : nullptr;
#define GRF_KRYLOV(NCV)                                                                                          \
    poly_krylov_frob_kernel<NCV><<<blocks, 256, 0, st>>>(n, s ? gt_ptr : nullptr, gt_idx, gt_val, xa, xb, ldx,    \
                                                         first ? inv_map : nullptr, ya, yb, WA, WB, wt, n_rhs, \
                                                         part, ticket, out + s)
        if (n_rhs <= 64) GRF_KRYLOV(1);
        else if (n_rhs <= 128) GRF_KRYLOV(2);
        else if (n_rhs <= 192) GRF_KRYLOV(3);
        else GRF_KRYLOV(4);
#undef GRF_KRYLOV
        GRF_CHECK_LAUNCH("poly_krylov_frob_kernel");
    }
    return GRF_OK;
}

#pragma GCC visibility pop
}  // extern "C"
