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
//                                 UNIT: the block X~ is the unit columns e_{unit[c]}, read from no memory.
//   poly_step_colsq_kernel<NC>    the same step (UNIT) fused with the per-column sums of squares of its result,
//                                 which is not written: diag K = sum_r Psi[r, c]^2.
//   poly_krylov_frob_kernel<NC>   the gradient's step U_l = G^T U_{l-1}, V_l = G^T V_{l-1} fused with the weighted
//                                 column inner products <U_l, W_B> + <V_l, W_A>; one-sided (TWO = false): U_l and
//                                 <U_l, W> alone, U_0 a row-mapped block or (UNIT) the scaled unit columns.
// One wave per output row; lane c owns the columns c + 64 i, i < NC = ceil(S / 64).  A row's indices and values
// are loaded once (64 at a time) and broadcast lane by lane for all NC chunks, so every gathered row is one
// contiguous S x 8-byte read.  Every sum has a fixed order (include/grf.h, "order rule"); no atomics on
// floating-point data.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "grf_block.h"
#include "grf_poly.h"

namespace grf {
namespace {

constexpr int kKrylovBlocks = 512;  // row blocks of poly_krylov_frob_kernel (one fp64 partial each)

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
    const int32_t *unit;  // UNIT kernels: X~ = V~ = the unit columns e_{unit[c]} (X NULL: the gathered block too)
    const double *P;  // addend b P[r] (NULL: none)
    int64_t ldp;
    double b;
    double *Y;
    int64_t ldy;
};

// Lane state of the step kernels: the NC columns a lane owns (and, UNIT, the node of each one's unit column).
template <int NC>
struct PolyCols {
    bool ok[NC];
    int col[NC];
    int32_t ux[NC];
};

template <int NC, bool UNIT>
__device__ __forceinline__ PolyCols<NC> poly_cols(int lane, int32_t S, const int32_t *unit) {
    PolyCols<NC> c;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        c.ok[i] = lane + 64 * i < S;
        c.col[i] = c.ok[i] ? lane + 64 * i : 0;
        c.ux[i] = -1;
        if constexpr (UNIT) c.ux[i] = c.ok[i] ? unit[c.col[i]] : -1;
    }
    return c;
}

// One output row of a Horner step by the order rule: acc = sum_e val[e] x~[idx[e]] (+ a V~[row]) (+ b P[r]).
template <int NC, bool UNIT>
__device__ __forceinline__ void poly_step_row(const PolyStep &p, const PolyCols<NC> &c, int lane, int64_t r,
                                              int64_t row, double xs, double a, double (&acc)[NC]) {
    // the value gathered at node k, column chunk i
    auto gathered = [&](int64_t k, int i) -> double {
        if constexpr (UNIT) {
            if (!p.X) return k == c.ux[i] ? xs : 0.0;  // RN(f * 1) at the column's node, +0.0 elsewhere
        }
        return (c.ok[i] && k >= 0) ? xs * p.X[k * p.ldx + c.col[i]] : 0.0;
    };
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
                    for (int i = 0; i < NC; ++i) x[u][i] = gathered(k, i);
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
                for (int i = 0; i < NC; ++i) acc[i] = fma(v, gathered(k, i), acc[i]);
            }
        }
    }
    if constexpr (UNIT) {
#pragma unroll
        for (int i = 0; i < NC; ++i) acc[i] = fma(a, row == c.ux[i] ? 1.0 : 0.0, acc[i]);
    } else if (p.V) {
        const int64_t q = uniform(p.v_map ? (int64_t)p.v_map[row] : row);
        if (q >= 0) {
#pragma unroll
            for (int i = 0; i < NC; ++i) acc[i] = fma(a, c.ok[i] ? p.V[q * p.ldv + c.col[i]] : 0.0, acc[i]);
        }
    }
    if (p.P) {
#pragma unroll
        for (int i = 0; i < NC; ++i) acc[i] = fma(p.b, c.ok[i] ? p.P[r * p.ldp + c.col[i]] : 0.0, acc[i]);
    }
}

template <int NC, bool UNIT>
__global__ __launch_bounds__(256) void poly_step_kernel(int64_t n_out, PolyStep p, int32_t S, const int32_t *done) {
    if (done && __builtin_nontemporal_load(done)) return;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const PolyCols<NC> c = poly_cols<NC, UNIT>(lane, S, p.unit);
    const double xs = p.xs ? *p.xs : 1.0;  // (1.0 * x is x: the scale is exact when absent)
    const double a = (UNIT || p.V) ? *p.a : 0.0;
    const int64_t n_waves = (int64_t)gridDim.x * 4;
    for (int64_t r = (int64_t)blockIdx.x * 4 + w; r < n_out; r += n_waves) {
        const int64_t row = uniform(p.row_map ? (int64_t)p.row_map[r] : r);
        double acc[NC];
        poly_step_row<NC, UNIT>(p, c, lane, r, row, xs, a, acc);
#pragma unroll
        for (int i = 0; i < NC; ++i)
            if (c.ok[i]) p.Y[r * p.ldy + c.col[i]] = acc[i];
    }
}

unsigned krylov_blocks(int64_t n) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv<int64_t>(n, 4), kKrylovBlocks));
}

// The last Horner step of Psi = p(A) [e_{unit[c]}]_c fused with out[c] = sum_r Psi[r, c]^2; Psi is not written.
// A lane squares its own columns: fma(h, h, sum) over a wave's rows ascending, the four waves in order through
// LDS, one fp64 partial per (block, column), and the last block (by ticket, reset afterwards) adds a column's
// partials in block order.
template <int NC>
__global__ __launch_bounds__(256) void poly_step_colsq_kernel(int64_t n, PolyStep p, int32_t S, double *part,
                                                              uint32_t *ticket, double *out) {
    __shared__ double red[4][64 * NC];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const PolyCols<NC> c = poly_cols<NC, true>(lane, S, p.unit);
    const double xs = p.xs ? *p.xs : 1.0;
    const double a = *p.a;
    double sq[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) sq[i] = 0.0;
    const int64_t n_waves = (int64_t)gridDim.x * 4;
    for (int64_t r = (int64_t)blockIdx.x * 4 + w; r < n; r += n_waves) {
        double acc[NC];
        poly_step_row<NC, true>(p, c, lane, r, r, xs, a, acc);
#pragma unroll
        for (int i = 0; i < NC; ++i) sq[i] = fma(acc[i], acc[i], sq[i]);
    }
#pragma unroll
    for (int i = 0; i < NC; ++i) red[w][lane + 64 * i] = sq[i];
    __syncthreads();
    for (int q = threadIdx.x; q < S; q += 256)
        part[(int64_t)blockIdx.x * S + q] = ((red[0][q] + red[1][q]) + red[2][q]) + red[3][q];
    if (!block_is_last(ticket, gridDim.x)) return;
    for (int q = threadIdx.x; q < S; q += 256) {
        double sum = 0.0;
        for (unsigned bq = 0; bq < gridDim.x; ++bq) sum += __builtin_nontemporal_load(&part[(int64_t)bq * S + q]);
        out[q] = sum;
    }
    if (threadIdx.x == 0) *ticket = 0u;
}

int32_t poly_step_launch(int64_t n_out, const PolyStep &p, int32_t S, const int32_t *done, hipStream_t st) {
    if (n_out == 0) return GRF_OK;
    const unsigned blocks = (unsigned)std::min<int64_t>(cdiv<int64_t>(n_out, 4), 1 << 16);
#define GRF_POLY(NCV)                                                              \
    do {                                                                           \
        if (p.unit) poly_step_kernel<NCV, true><<<blocks, 256, 0, st>>>(n_out, p, S, done); \
        else poly_step_kernel<NCV, false><<<blocks, 256, 0, st>>>(n_out, p, S, done);       \
    } while (0)
    if (S <= 64) GRF_POLY(1);
    else if (S <= 128) GRF_POLY(2);
    else if (S <= 192) GRF_POLY(3);
    else GRF_POLY(4);
#undef GRF_POLY
    GRF_CHECK_LAUNCH("poly_step_kernel");
    return GRF_OK;
}

// the sums of squares of the step's n rows into out[S]; part: krylov_blocks(n) x S doubles
int32_t poly_step_colsq_launch(int64_t n, const PolyStep &p, int32_t S, double *part, uint32_t *ticket, double *out,
                               hipStream_t st) {
    const unsigned blocks = krylov_blocks(n);
#define GRF_POLY(NCV) poly_step_colsq_kernel<NCV><<<blocks, 256, 0, st>>>(n, p, S, part, ticket, out)
    if (S <= 64) GRF_POLY(1);
    else if (S <= 128) GRF_POLY(2);
    else if (S <= 192) GRF_POLY(3);
    else GRF_POLY(4);
#undef GRF_POLY
    GRF_CHECK_LAUNCH("poly_step_colsq_kernel");
    return GRF_OK;
}

// One step of both Krylov sequences and its contraction.  With ptr: UA = A XA~, UB = A XB~ (row r of A; X~ the
// block X through x_map); without: UA = XA~[r], UB = XB~[r] (step 0).  UA / UB are stored to YA / YB (pitch S)
// unless those are NULL, and
//     out[0] = sum_r sum_c wt[c] (UA[r,c] WB[r,c] + UB[r,c] WA[r,c])
// summed in a fixed order: a wave's rows ascending (columns c = lane, lane + 64, ... in turn), the lanes by an
// xor tree, the four waves in order, one fp64 partial per block, and the last block (by ticket, reset
// afterwards) adds the partials in block order.
// One-sided (TWO = false; XB, YB, WA, wt unused): UA alone and sum_r sum_c UA[r,c] WB[r,c], one fma per element,
// and out[0] = (add ? out[0] : 0) + scale * sum -- the K block's gradient adds its column blocks in order.  UNIT
// (one-sided only): XA~ = [XA[c] e_{unit[c]}]_c while x_unit is set (steps 0 and 1), read from no block.
struct KrylovStep {
    const int64_t *ptr;
    const int32_t *idx;
    const double *val;
    const double *XA, *XB;
    int64_t ldx;
    const int32_t *x_map;
    const int32_t *x_unit;
    double *YA, *YB;
    const double *WA, *WB, *wt;
    double *part;
    uint32_t *ticket;
    double *out;
    double scale;
    int32_t add;
};

template <int NC, bool TWO, bool UNIT>
__global__ __launch_bounds__(256) void poly_krylov_frob_kernel(int64_t n, KrylovStep p, int32_t S) {
    static_assert(!(TWO && UNIT), "the unit columns are one-sided");
    __shared__ double red[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const bool from_unit = UNIT && p.x_unit;
    bool ok[NC];
    int col[NC];
    double wgt[NC];   // TWO: the column's weight; UNIT: its scale XA[c]
    int32_t ux[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        ok[i] = lane + 64 * i < S;
        col[i] = ok[i] ? lane + 64 * i : 0;
        wgt[i] = 0.0;
        ux[i] = -1;
        if constexpr (TWO) wgt[i] = ok[i] ? p.wt[col[i]] : 0.0;
        if constexpr (UNIT) {
            if (from_unit) {
                wgt[i] = ok[i] ? p.XA[col[i]] : 0.0;
                ux[i] = ok[i] ? p.x_unit[col[i]] : -1;
            }
        }
    }
    auto gathered = [&](const double *X, int64_t k, int i) -> double {
        if constexpr (UNIT) {
            if (from_unit) return k == ux[i] ? wgt[i] : 0.0;
        }
        return (ok[i] && k >= 0) ? X[k * p.ldx + col[i]] : 0.0;
    };
    double acc = 0.0;
    const int64_t n_waves = (int64_t)gridDim.x * 4;
    for (int64_t r = (int64_t)blockIdx.x * 4 + w; r < n; r += n_waves) {
        double ua[NC], ub[NC];
#pragma unroll
        for (int i = 0; i < NC; ++i) ua[i] = ub[i] = 0.0;
        if (p.ptr) {
            const int64_t e0 = uniform(p.ptr[r]), e1 = uniform(p.ptr[r + 1]);
            for (int64_t eb = e0; eb < e1; eb += 64) {
                const int64_t e = eb + lane;
                int32_t k_l = e < e1 ? p.idx[e] : 0;
                const double v_l = e < e1 ? p.val[e] : 0.0;
                if (p.x_map) k_l = e < e1 ? p.x_map[k_l] : -1;
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
                            xa[u][i] = gathered(p.XA, k, i);
                            if constexpr (TWO) xb[u][i] = gathered(p.XB, k, i);
                        }
                    }
#pragma unroll
                    for (int u = 0; u < 2; ++u)
#pragma unroll
                        for (int i = 0; i < NC; ++i) {
                            ua[i] = fma(v[u], xa[u][i], ua[i]);
                            if constexpr (TWO) ub[i] = fma(v[u], xb[u][i], ub[i]);
                        }
                }
                for (; j < cnt; ++j) {
                    const int64_t k = __builtin_amdgcn_readlane(k_l, j);
                    const double v = readlane_f64(v_l, j);
#pragma unroll
                    for (int i = 0; i < NC; ++i) {
                        ua[i] = fma(v, gathered(p.XA, k, i), ua[i]);
                        if constexpr (TWO) ub[i] = fma(v, gathered(p.XB, k, i), ub[i]);
                    }
                }
            }
        } else if (from_unit) {
#pragma unroll
            for (int i = 0; i < NC; ++i) ua[i] = r == ux[i] ? wgt[i] : 0.0;
        } else {
            const int64_t q = uniform(p.x_map ? (int64_t)p.x_map[r] : r);
            if (q >= 0) {
#pragma unroll
                for (int i = 0; i < NC; ++i) {
                    ua[i] = ok[i] ? p.XA[q * p.ldx + col[i]] : 0.0;
                    if constexpr (TWO) ub[i] = ok[i] ? p.XB[q * p.ldx + col[i]] : 0.0;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            if (p.YA && ok[i]) {
                p.YA[r * S + col[i]] = ua[i];
                if constexpr (TWO) p.YB[r * S + col[i]] = ub[i];
            }
            const double wb = ok[i] ? p.WB[r * S + col[i]] : 0.0;
            if constexpr (TWO) {
                const double wa = ok[i] ? p.WA[r * S + col[i]] : 0.0;
                acc = fma(wgt[i], fma(ua[i], wb, ub[i] * wa), acc);
            } else {
                acc = fma(ua[i], wb, acc);
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
    if (lane == 0) red[w] = acc;
    __syncthreads();
    if (threadIdx.x == 0) p.part[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
    if (!block_is_last(p.ticket, gridDim.x)) return;
    if (threadIdx.x == 0) {
        double sum = 0.0;
        for (unsigned bq = 0; bq < gridDim.x; ++bq) sum += __builtin_nontemporal_load(&p.part[bq]);
        if constexpr (TWO) p.out[0] = sum;
        else p.out[0] = p.add ? p.out[0] + p.scale * sum : p.scale * sum;
        *p.ticket = 0u;
    }
}

template <bool TWO, bool UNIT>
int32_t krylov_launch(int64_t n, const KrylovStep &p, int32_t S, hipStream_t st) {
    const unsigned blocks = krylov_blocks(n);
#define GRF_KRYLOV(NCV) poly_krylov_frob_kernel<NCV, TWO, UNIT><<<blocks, 256, 0, st>>>(n, p, S)
    if (S <= 64) GRF_KRYLOV(1);
    else if (S <= 128) GRF_KRYLOV(2);
    else if (S <= 192) GRF_KRYLOV(3);
    else GRF_KRYLOV(4);
#undef GRF_KRYLOV
    GRF_CHECK_LAUNCH("poly_krylov_frob_kernel");
    return GRF_OK;
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

namespace {

// where a chain's last step goes: rows `row_map` of H_0 (+ b P) into Y, or (sq_out set) H_0's per-column sums
// of squares into sq_out[S] without writing H_0
struct ChainOut {
    const int32_t *row_map;
    int64_t n_out;
    double *Y;
    int64_t ldy;
    const double *P;
    int64_t ldp;
    double b;
    double *sq_part;
    uint32_t *sq_ticket;
    double *sq_out;
};

// The Horner chain on X~ = X through x_map, or (unit set) on the unit columns e_{unit[c]}.
int32_t chain_run(const PolyOp &op, const int32_t *x_map, const double *X, int64_t ldx, const int32_t *unit, int32_t S,
                  const ChainOut &o, double *H0, double *H1, const int32_t *done, hipStream_t st) {
    PolyStep p{};
    p.V = X; p.ldv = ldx; p.v_map = x_map; p.unit = unit;
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
            if (o.sq_out) return poly_step_colsq_launch(op.n, p, S, o.sq_part, o.sq_ticket, o.sq_out, st);
            p.row_map = o.row_map; p.Y = o.Y; p.ldy = o.ldy; p.P = o.P; p.ldp = o.ldp; p.b = o.b;
        } else {
            p.row_map = nullptr; p.Y = H[q & 1]; p.ldy = S;
        }
        const int32_t rc = poly_step_launch(final_step ? o.n_out : op.n, p, S, done, st);
        if (rc != GRF_OK || final_step) return rc;
        in = H[q & 1];
    }
}

// Psi = p(A) [e_{unit[c]}]_c, all n rows (pitch S)
int32_t chain_unit(const PolyOp &op, const int32_t *unit, int32_t S, double *Psi, double *H0, double *H1,
                   hipStream_t st) {
    ChainOut o{};
    o.n_out = op.n; o.Y = Psi; o.ldy = S;
    return chain_run(op, nullptr, nullptr, 0, unit, S, o, H0, H1, nullptr, st);
}

}  // namespace

int32_t poly_chain(const PolyOp &op, const int32_t *x_map, const double *X, int64_t ldx, int32_t S,
                   const int32_t *row_map, int64_t n_out, double *Y, int64_t ldy, const double *P, int64_t ldp,
                   double b, double *H0, double *H1, const int32_t *done, hipStream_t st) {
    ChainOut o{};
    o.row_map = row_map; o.n_out = n_out; o.Y = Y; o.ldy = ldy; o.P = P; o.ldp = ldp; o.b = b;
    return chain_run(op, x_map, X, ldx, nullptr, S, o, H0, H1, done, st);
}

namespace {

// T[c, r] = g[r, c] (g: n1 x n2, pitch ldg; T: n2 x n1, pitch n1)
__global__ __launch_bounds__(256) void poly_transpose_kernel(int64_t n1, int64_t n2, const double *g, int64_t ldg,
                                                             double *T) {
    __shared__ double tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    for (int64_t t = blockIdx.x;; t += gridDim.x) {
        const int64_t tiles_c = cdiv<int64_t>(n2, 32), tiles_r = cdiv<int64_t>(n1, 32);
        if (t >= tiles_c * tiles_r) return;
        const int64_t r0 = (t / tiles_c) * 32, c0 = (t % tiles_c) * 32;
        for (int i = ty; i < 32; i += 8)
            if (r0 + i < n1 && c0 + tx < n2) tile[i][tx] = g[(r0 + i) * ldg + c0 + tx];
        __syncthreads();
        for (int i = ty; i < 32; i += 8)
            if (c0 + i < n2 && r0 + tx < n1) T[(c0 + i) * n1 + r0 + tx] = tile[tx][i];
        __syncthreads();
    }
}

int32_t block_cols(int64_t n_cols) { return (int32_t)std::min<int64_t>(std::max<int64_t>(n_cols, 1), kPolyMaxRhs); }

struct KernelGradLayout {
    size_t part, psi, u[2], gt, total;
};

KernelGradLayout kernel_grad_layout(int64_t n, int64_t n1, int64_t n2, bool diag) {
    KernelGradLayout l{};
    const size_t blk = al256((size_t)std::max<int64_t>(n, 1) * block_cols(std::max(n1, n2)) * sizeof(double));
    size_t o = 256;  // the ticket
    l.part = o; o += al256((size_t)krylov_blocks(n) * sizeof(double));
    l.psi = o; o += blk;
    l.u[0] = o; o += blk;
    l.u[1] = o; o += blk;
    l.gt = o; o += diag ? 0 : al256((size_t)std::max<int64_t>(n1, 1) * std::max<int64_t>(n2, 1) * sizeof(double));
    l.total = o;
    return l;
}

// One half of the K block's gradient: out[l] (+)= sum over the column blocks of xb, in order, of
// sum_c <((G^T)^l S_a^T g[:, c]), Psi_b[:, c]>, Psi_b = p(G^T) [e_{xb[c]}]_c.  g: rows through inv_a (node -> row
// or -1), one column per entry of xb, pitch ldg.  Diagonal (g_diag set): U_0 = [g_diag[c] e_{xb[c]}]_c, scale 2.
int32_t kernel_grad_half(const PolyOp &op, const int32_t *inv_a, const int32_t *xb, int64_t nb, const double *g,
                         int64_t ldg, const double *g_diag, bool first, double *out, char *w,
                         const KernelGradLayout &l, hipStream_t st) {
    double *Psi = (double *)(w + l.psi), *U[2] = {(double *)(w + l.u[0]), (double *)(w + l.u[1])};
    KrylovStep k{};
    k.idx = op.idx; k.val = op.val; k.WB = Psi; k.part = (double *)(w + l.part); k.ticket = (uint32_t *)w;
    k.scale = g_diag ? 2.0 : 1.0;
    for (int64_t c0 = 0; c0 < nb; c0 += kPolyMaxRhs) {
        const int32_t S = (int32_t)std::min<int64_t>(kPolyMaxRhs, nb - c0);
        int32_t rc = chain_unit(op, xb + c0, S, Psi, U[0], U[1], st);
        if (rc != GRF_OK) return rc;
        for (int32_t s = 0; s < op.n_f; ++s) {
            // steps 0 and 1 read U_0 through its map (or its unit columns), later steps the stored U_{s-1}
            const bool head = s <= 1, store = s >= 1 && s + 1 < op.n_f;
            k.ptr = s ? op.ptr : nullptr;
            k.XA = head ? (g_diag ? g_diag + c0 : g + c0) : U[(s - 1) & 1];
            k.ldx = head ? ldg : S;
            k.x_map = head && !g_diag ? inv_a : nullptr;
            k.x_unit = head && g_diag ? xb + c0 : nullptr;
            k.YA = store ? U[s & 1] : nullptr;
            k.out = out + s;
            k.add = !(first && c0 == 0);
            rc = g_diag ? krylov_launch<false, true>(op.n, k, S, st) : krylov_launch<false, false>(op.n, k, S, st);
            if (rc != GRF_OK) return rc;
        }
    }
    return GRF_OK;
}

}  // namespace

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
    KrylovStep k{};
    k.idx = gt_idx; k.val = gt_val; k.WA = WA; k.WB = WB; k.wt = wt; k.part = part; k.ticket = ticket;
    for (int32_t s = 0; s < n_f; ++s) {
        // step 0 contracts S_T^T A / S_T^T B themselves; step 1 gathers them through inv_map; later steps the
        // stored U_{s-1} / V_{s-1}.  The last step's U / V are not stored.
        const bool first = s <= 1, store = s >= 1 && s + 1 < n_f;
        k.ptr = s ? gt_ptr : nullptr;
        k.XA = first ? A : U[(s - 1) & 1]; k.XB = first ? B : V[(s - 1) & 1];
        k.ldx = first ? ld : n_rhs;
        k.x_map = first ? inv_map : nullptr;
        k.YA = store ? U[s & 1] : nullptr; k.YB = store ? V[s & 1] : nullptr;
        k.out = out + s;
        rc = krylov_launch<true, false>(n, k, n_rhs, st);
        if (rc != GRF_OK) return rc;
    }
    return GRF_OK;
}

size_t grf_poly_kernel_block_workspace_bytes(int64_t n, int32_t n_f, int64_t n2) {
    // Psi and (n_f > 2) the chains' two intermediate blocks
    return (size_t)(n_f > 2 ? 3 : 1) * al256((size_t)std::max<int64_t>(n, 1) * block_cols(n2) * sizeof(double));
}

int32_t grf_poly_kernel_block_f64(int64_t n, const int64_t *g_ptr, const int32_t *g_idx, const double *g_val,
                                  const int64_t *gt_ptr, const int32_t *gt_idx, const double *gt_val, const double *f,
                                  int32_t n_f, const int32_t *x1, int64_t n1, const int32_t *x2, int64_t n2, double *K,
                                  int64_t ldk, void *workspace, size_t workspace_bytes, grf_stream_t stream) {
    GRF_REQUIRE(n >= 1 && n1 >= 0 && n2 >= 0 && g_ptr && gt_ptr && f && n_f >= 1, GRF_EINVAL,
                "grf_poly_kernel_block_f64: bad arguments");
    GRF_REQUIRE(n < (1ll << 31) && n1 < (1ll << 31) && n2 < (1ll << 31), GRF_EUNSUPPORTED,
                "grf_poly_kernel_block_f64: more than 2^31 rows");
    if (n1 == 0 || n2 == 0) return GRF_OK;
    GRF_REQUIRE(x1 && x2 && K && ldk >= n2, GRF_EINVAL, "grf_poly_kernel_block_f64: bad arguments");
    const size_t need = grf_poly_kernel_block_workspace_bytes(n, n_f, n2);
    GRF_REQUIRE(workspace && workspace_bytes >= need, GRF_EINVAL,
                "grf_poly_kernel_block_f64: workspace too small (%zu < %zu)", workspace_bytes, need);
    hipStream_t st = S(stream);
    const size_t blk = al256((size_t)n * block_cols(n2) * sizeof(double));
    double *Psi = (double *)workspace;
    double *H0 = n_f > 2 ? (double *)((char *)workspace + blk) : nullptr;
    double *H1 = n_f > 2 ? (double *)((char *)workspace + 2 * blk) : nullptr;
    const PolyOp opt{n, gt_ptr, gt_idx, gt_val, f, n_f}, op{n, g_ptr, g_idx, g_val, f, n_f};
    for (int64_t c0 = 0; c0 < n2; c0 += kPolyMaxRhs) {
        const int32_t Sb = (int32_t)std::min<int64_t>(kPolyMaxRhs, n2 - c0);
        int32_t rc = chain_unit(opt, x2 + c0, Sb, Psi, H0, H1, st);  // Psi = p(G^T) S_2^T, this block's columns
        if (rc != GRF_OK) return rc;
        rc = poly_chain(op, nullptr, Psi, Sb, Sb, x1, n1, K + c0, ldk, nullptr, 0, 0.0, H0, H1, nullptr, st);
        if (rc != GRF_OK) return rc;
    }
    return GRF_OK;
}

size_t grf_poly_kernel_diag_workspace_bytes(int64_t n, int32_t n_f, int64_t n_x) {
    const int32_t Sb = block_cols(n_x);
    return 256 + al256((size_t)krylov_blocks(n) * Sb * sizeof(double)) +
           (size_t)(n_f > 2 ? 2 : 0) * al256((size_t)std::max<int64_t>(n, 1) * Sb * sizeof(double));
}

int32_t grf_poly_kernel_diag_f64(int64_t n, const int64_t *gt_ptr, const int32_t *gt_idx, const double *gt_val,
                                 const double *f, int32_t n_f, const int32_t *x, int64_t n_x, double *out,
                                 void *workspace, size_t workspace_bytes, grf_stream_t stream) {
    GRF_REQUIRE(n >= 1 && n_x >= 0 && gt_ptr && f && n_f >= 1, GRF_EINVAL, "grf_poly_kernel_diag_f64: bad arguments");
    GRF_REQUIRE(n < (1ll << 31) && n_x < (1ll << 31), GRF_EUNSUPPORTED,
                "grf_poly_kernel_diag_f64: more than 2^31 rows");
    if (n_x == 0) return GRF_OK;
    GRF_REQUIRE(x && out, GRF_EINVAL, "grf_poly_kernel_diag_f64: bad arguments");
    const size_t need = grf_poly_kernel_diag_workspace_bytes(n, n_f, n_x);
    GRF_REQUIRE(workspace && workspace_bytes >= need, GRF_EINVAL,
                "grf_poly_kernel_diag_f64: workspace too small (%zu < %zu)", workspace_bytes, need);
    hipStream_t st = S(stream);
    char *w = (char *)workspace;
    const int32_t Smax = block_cols(n_x);
    const size_t part_bytes = al256((size_t)krylov_blocks(n) * Smax * sizeof(double));
    const size_t blk = al256((size_t)n * Smax * sizeof(double));
    ChainOut o{};
    o.sq_ticket = (uint32_t *)w;
    o.sq_part = (double *)(w + 256);
    double *H0 = n_f > 2 ? (double *)(w + 256 + part_bytes) : nullptr;
    double *H1 = n_f > 2 ? (double *)(w + 256 + part_bytes + blk) : nullptr;
    GRF_CHECK_HIP(hipMemsetAsync(w, 0, 256, st));
    const PolyOp opt{n, gt_ptr, gt_idx, gt_val, f, n_f};
    for (int64_t c0 = 0; c0 < n_x; c0 += kPolyMaxRhs) {
        const int32_t Sb = (int32_t)std::min<int64_t>(kPolyMaxRhs, n_x - c0);
        o.sq_out = out + c0;
        const int32_t rc = chain_run(opt, nullptr, nullptr, 0, x + c0, Sb, o, H0, H1, nullptr, st);
        if (rc != GRF_OK) return rc;
    }
    return GRF_OK;
}

size_t grf_poly_kernel_grad_workspace_bytes(int64_t n, int64_t n1, int64_t n2, int32_t diag) {
    return kernel_grad_layout(n, n1, diag ? n1 : n2, diag != 0).total;
}

int32_t grf_poly_kernel_grad_f64(int64_t n, const int64_t *gt_ptr, const int32_t *gt_idx, const double *gt_val,
                                 const double *f, int32_t n_f, const int32_t *x1, int64_t n1, const int32_t *inv1,
                                 const int32_t *x2, int64_t n2, const int32_t *inv2, const double *g, int64_t ldg,
                                 int32_t diag, double *out, void *workspace, size_t workspace_bytes,
                                 grf_stream_t stream) {
    GRF_REQUIRE(n >= 1 && n1 >= 0 && n2 >= 0 && gt_ptr && f && n_f >= 1 && out, GRF_EINVAL,
                "grf_poly_kernel_grad_f64: bad arguments");
    GRF_REQUIRE(n < (1ll << 31) && n1 < (1ll << 31) && n2 < (1ll << 31), GRF_EUNSUPPORTED,
                "grf_poly_kernel_grad_f64: more than 2^31 rows");
    hipStream_t st = S(stream);
    if (n1 == 0 || (!diag && n2 == 0)) {  // an empty block: the gradient is zero
        GRF_CHECK_HIP(hipMemsetAsync(out, 0, (size_t)n_f * sizeof(double), st));
        return GRF_OK;
    }
    GRF_REQUIRE(x1 && g && (diag || (inv1 && x2 && inv2 && ldg >= n2)), GRF_EINVAL,
                "grf_poly_kernel_grad_f64: bad arguments");
    if (diag) n2 = n1;
    const KernelGradLayout l = kernel_grad_layout(n, n1, n2, diag != 0);
    GRF_REQUIRE(workspace && workspace_bytes >= l.total, GRF_EINVAL,
                "grf_poly_kernel_grad_f64: workspace too small (%zu < %zu)", workspace_bytes, l.total);
    char *w = (char *)workspace;
    GRF_CHECK_HIP(hipMemsetAsync(w, 0, 256, st));
    const PolyOp opt{n, gt_ptr, gt_idx, gt_val, f, n_f};
    if (diag) return kernel_grad_half(opt, nullptr, x1, n1, nullptr, 0, g, true, out, w, l, st);
    // sum_c <(G^T)^l S_1^T g[:, c], Psi_2[:, c]>, then the mirrored half on g^T
    int32_t rc = kernel_grad_half(opt, inv1, x2, n2, g, ldg, nullptr, true, out, w, l, st);
    if (rc != GRF_OK) return rc;
    double *gT = (double *)(w + l.gt);
    const int64_t tiles = cdiv<int64_t>(n1, 32) * cdiv<int64_t>(n2, 32);
    poly_transpose_kernel<<<(unsigned)std::min<int64_t>(tiles, 1 << 16), 256, 0, st>>>(n1, n2, g, ldg, gT);
    GRF_CHECK_LAUNCH("poly_transpose_kernel");
    return kernel_grad_half(opt, inv2, x1, n1, gT, n1, nullptr, false, out, w, l, st);
}

#pragma GCC visibility pop
}  // extern "C"
