// grf_poly.h -- the walk polynomial p(A) = sum_l f_l A^l as a matrix-free operator (grf_poly.hip), shared with
// the CG of grf_cg.hip.
#pragma once
#include "grf_common.h"

namespace grf {

constexpr int kPolyMaxRhs = 256;  // 4 columns per lane

// A: n x n CSR with fp64 values; f[n_f]: the coefficients, on the device
struct PolyOp {
    int64_t n;
    const int64_t *ptr;
    const int32_t *idx;
    const double *val;
    const double *f;
    int32_t n_f;
};

// Y[r, :] = (p(A) X~)[row(r), :] + b P[r, :] by Horner (the order rule of include/grf.h).  X~ = X, or with x_map
// (int32 [n]: a node's row of X, or -1) the n-row block whose rows without one are zero.  row(r) = row_map[r]
// (n_out rows) or r (row_map NULL, n_out = n).  P NULL: no such addend.  H0, H1: n x S doubles each (pitch S),
// the chain's intermediate blocks (unused when n_f <= 2); neither Y nor H0 / H1 may alias X or P.  `done`: the
// CG's flag (NULL: none).
int32_t poly_chain(const PolyOp &op, const int32_t *x_map, const double *X, int64_t ldx, int32_t S,
                   const int32_t *row_map, int64_t n_out, double *Y, int64_t ldy, const double *P, int64_t ldp,
                   double b, double *H0, double *H1, const int32_t *done, hipStream_t st);

}  // namespace grf
