// grf_posterior.hip -- the exact posterior mean and variance's two own kernels.
//
// With K^ = K[T,T] + s2 I, alpha = K^-1 y and the right-hand sides b_c = K[T, x_c] of a chunk of <= 256 test
// nodes, X = K^-1 B from one batched CG solve:
//     mean_c = b_c^T alpha,     var_c = K[x_c, x_c] - b_c^T x_c.
// posterior_rhs_*: E = Phi[x]^T as a dense n_cols x S fp64 block (B = Phi[T] E then comes from grf_spmm_csr_f64)
// and prior[c] = sum_k Phi[x_c, k]^2 = K[x_c, x_c].  One wave per test node: its row's entries are loaded 64 at
// a time, every lane stores its own entry's fp32 value widened (exactly) into column c, and the squares -- exact
// in fp64, 24 x 24 bits -- are added one by one in the row's stored order.
//
// posterior_reduce_kernel: q[c] = sum_r B[r,c] X[r,c] and mean[c] = sum_r B[r,c] alpha[r] in one pass over the two
// n x S blocks (16 n S bytes, read once).  A wave covers R = 64 / P rows of P columns at a time, P the power of
// two >= min(S, 64): for S >= 64 a lane owns the columns lane + 64 i of one row, for small S the wave packs R
// rows so that it still reads whole contiguous stretches.  Every sum has a fixed order that depends on (n, S)
// alone and is the same for every column: a lane's rows ascending by fma, the R row groups by an xor tree, the
// eight waves in order, one fp64 partial per (row block, column), and the last block (by ticket) adds the
// partials in block order within a few groups of consecutive blocks and then the groups in order -- two calls
// give the same bits, and permuting the columns permutes the results.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "grf_block.h"

namespace grf {
namespace {

constexpr int kPostMaxRhs = 256;    // 4 columns per lane
constexpr int kPostWaves = 8;       // waves per block
constexpr int kPostThreads = 64 * kPostWaves;
constexpr int kPostBlocks = 256;    // row blocks at the most
constexpr int kPostBlockIters = 4;  // a block has at least this many rows per lane before there is a second one
constexpr int kPostBatch = 8;       // partials in flight per thread of the last block

// log2 of the columns a wave's row group spans: the power of two >= min(S, 64)
int post_lg_cols(int32_t S) { return ceil_log2((uint64_t)std::max(1, std::min(S, 64))); }

// the row partition, a function of (n, S) only: blocks of rows_per_block consecutive rows
struct PostPlan {
    unsigned blocks_bound, blocks;
    int64_t rows_per_block;
};
PostPlan post_plan(int64_t n, int32_t S) {
    const int64_t wave_rows = 64 >> post_lg_cols(S);
    PostPlan p;
    p.blocks_bound =
        (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv<int64_t>(n, kPostWaves * wave_rows * kPostBlockIters), kPostBlocks));
    p.rows_per_block = cdiv<int64_t>(n, p.blocks_bound);
    p.blocks = (unsigned)std::max<int64_t>(1, p.rows_per_block ? cdiv<int64_t>(n, p.rows_per_block) : 1);
    return p;
}

bool overlaps(const void *p, size_t pn, const void *q, size_t qn) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return p && q && pn && qn && a < b + qn && b < a + pn;
}
size_t span(int64_t rows, int64_t cols, int64_t ld) {
    return rows > 0 && cols > 0 ? ((size_t)(rows - 1) * (size_t)ld + (size_t)cols) * sizeof(double) : 0;
}

// E[r, 0..S) = 0 for r < n_cols; the columns [S, lde) are not touched
__global__ __launch_bounds__(256) void posterior_rhs_zero_kernel(int64_t n_cols, int32_t S, int32_t lg_cols, double *E,
                                                                 int64_t lde) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int wave_rows = 64 >> lg_cols;
    const int rsub = lane >> lg_cols, cl = lane & ((1 << lg_cols) - 1);
    const int64_t stride = (int64_t)gridDim.x * 4 * wave_rows;
    for (int64_t r = ((int64_t)blockIdx.x * 4 + w) * wave_rows + rsub; r < n_cols; r += stride)
        for (int c = cl; c < S; c += 64) E[r * lde + c] = 0.0;
}

// one wave per test node c: E[idx, c] = val (widened), prior[c] = sum val^2 in stored order
__global__ __launch_bounds__(256) void posterior_rhs_kernel(int64_t n_rows, const int64_t *__restrict__ ptr,
                                                            const int32_t *__restrict__ idx,
                                                            const float *__restrict__ val, int64_t n_cols,
                                                            const int32_t *__restrict__ nodes, int32_t S, double *E,
                                                            int64_t lde, double *prior) {
    const int lane = threadIdx.x & 63;
    const int c = uniform32((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (c >= S) return;
    const int64_t row = uniform32(nodes[c]);
    double sum = 0.0;
    if (row >= 0 && row < n_rows) {  // (an index outside Phi is an empty row: nothing is read or written for it)
        const int64_t e0 = uniform(ptr[row]), e1 = uniform(ptr[row + 1]);
        for (int64_t eb = e0; eb < e1; eb += 64) {
            const int64_t e = eb + lane;
            const int32_t k = e < e1 ? idx[e] : -1;
            const float v = e < e1 ? val[e] : 0.f;
            if (k >= 0 && k < n_cols) E[(int64_t)k * lde + c] = (double)v;
            const int cnt = (int)min<int64_t>(64, e1 - eb);
            for (int j = 0; j < cnt; ++j) {
                const double vj =
                    (double)__builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int32_t, v), j));
                sum += vj * vj;
            }
        }
    }
    if (lane == 0) prior[c] = sum;
}

// NC = ceil(S / 64) column chunks per lane (NC > 1: one row per wave step)
template <int NC>
__global__ __launch_bounds__(kPostThreads) void posterior_reduce_kernel(int64_t n, int32_t S, int32_t lg_cols,
                                                               int64_t rows_per_block, const double *__restrict__ B,
                                                               int64_t ldb, const double *__restrict__ X, int64_t ldx,
                                                               const double *__restrict__ alpha,
                                                               const double *__restrict__ prior, double add_noise,
                                                               double *part, uint32_t *ticket, double *var,
                                                               double *mean) {
    constexpr int CP = 64 * NC;  // column slots
    __shared__ double red[2][kPostWaves][CP];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int wave_rows = 64 >> lg_cols;
    const int rsub = lane >> lg_cols, cl = lane & ((1 << lg_cols) - 1);
    const bool with_mean = alpha != nullptr;
    bool ok[NC];
    int col[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        const int c = cl + 64 * i;
        ok[i] = c < S;
        col[i] = ok[i] ? c : 0;
    }
    double q[NC], m[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) q[i] = m[i] = 0.0;
    const int64_t r_begin = (int64_t)blockIdx.x * rows_per_block;
    const int64_t r_end = min<int64_t>(n, r_begin + rows_per_block);
    const int64_t step = kPostWaves * wave_rows;
#pragma unroll 4
    for (int64_t r = r_begin + (int64_t)w * wave_rows + rsub; r < r_end; r += step) {
        const double a = with_mean ? alpha[r] : 0.0;
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            const double b = ok[i] ? B[r * ldb + col[i]] : 0.0;
            const double x = ok[i] ? X[r * ldx + col[i]] : 0.0;
            q[i] = fma(b, x, q[i]);
            m[i] = fma(b, a, m[i]);
        }
    }
    // the wave's row groups (lanes with the same column), by an xor tree
    for (int off = 1 << lg_cols; off < 64; off <<= 1) {
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            q[i] += __shfl_xor(q[i], off);
            m[i] += __shfl_xor(m[i], off);
        }
    }
    if (rsub == 0) {
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            red[0][w][cl + 64 * i] = q[i];
            red[1][w][cl + 64 * i] = m[i];
        }
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t < S) {  // (S <= 64 NC: column t's slot was written by every wave)
        double *pb = part + (int64_t)blockIdx.x * 2 * S;
        double qs = red[0][0][t], ms = red[1][0][t];
#pragma unroll
        for (int v = 1; v < kPostWaves; ++v) {
            qs += red[0][v][t];
            ms += red[1][v][t];
        }
        pb[t] = qs;
        pb[S + t] = ms;
    }
    if (!block_is_last(ticket, gridDim.x)) return;
    // the last block: G = threads / CP groups of consecutive blocks; a thread adds its column's partials of its
    // group in block order (kPostBatch loads in flight), then the groups are added in order
    constexpr int G = kPostThreads / CP;
    const int nb = gridDim.x;
    const int per_group = (nb + G - 1) / G;
    const int g = t / CP, c = t % CP;
    if (g < G && c < S) {
        const int b_begin = g * per_group, b_end = min(nb, b_begin + per_group);
        double qs = 0.0, ms = 0.0;
        for (int bq = b_begin; bq < b_end; bq += kPostBatch) {
            double pq[kPostBatch], pm[kPostBatch];
#pragma unroll
            for (int u = 0; u < kPostBatch; ++u) {
                const bool in = bq + u < b_end;
                const double *src = part + (int64_t)(in ? bq + u : bq) * 2 * S;
                pq[u] = __builtin_nontemporal_load(&src[c]);
                pm[u] = __builtin_nontemporal_load(&src[S + c]);
                if (!in) pq[u] = pm[u] = 0.0;
            }
#pragma unroll
            for (int u = 0; u < kPostBatch; ++u) {
                qs += pq[u];
                ms += pm[u];
            }
        }
        red[0][g][c] = qs;
        red[1][g][c] = ms;
    }
    __syncthreads();
    if (t < S) {
        double qs = red[0][0][t], ms = red[1][0][t];
#pragma unroll
        for (int v = 1; v < G; ++v) {
            qs += red[0][v][t];
            ms += red[1][v][t];
        }
        var[t] = (prior[t] - qs) + add_noise;
        if (with_mean) mean[t] = ms;
    }
    if (threadIdx.x == 0) *ticket = 0u;
}

}  // namespace
}  // namespace grf

using namespace grf;

extern "C" {
#pragma GCC visibility push(default)

int32_t grf_posterior_rhs_f64(int64_t n_rows, const int64_t *ptr, const int32_t *idx, const float *val,
                              int64_t n_cols, const int32_t *nodes, int32_t n_nodes, double *E, int64_t lde,
                              double *prior, grf_stream_t stream) {
    GRF_REQUIRE(n_rows >= 0 && n_cols >= 0 && n_nodes >= 0, GRF_EINVAL, "grf_posterior_rhs_f64: negative size");
    GRF_REQUIRE(n_nodes <= kPostMaxRhs, GRF_EUNSUPPORTED, "grf_posterior_rhs_f64: n_nodes must be in [0, %d]",
                kPostMaxRhs);
    GRF_REQUIRE(n_rows < (1ll << 31) && n_cols < (1ll << 31), GRF_EUNSUPPORTED,
                "grf_posterior_rhs_f64: more than 2^31 rows or columns");
    if (n_nodes == 0) return GRF_OK;
    GRF_REQUIRE(ptr && nodes && prior, GRF_EINVAL, "grf_posterior_rhs_f64: a pointer is NULL");
    GRF_REQUIRE(lde >= n_nodes, GRF_EINVAL, "grf_posterior_rhs_f64: lde is below n_nodes");
    GRF_REQUIRE(n_cols == 0 || E, GRF_EINVAL, "grf_posterior_rhs_f64: E is NULL");
    const size_t en = span(n_cols, n_nodes, lde), pn = (size_t)n_nodes * sizeof(double);
    GRF_REQUIRE(!overlaps(E, en, prior, pn) && !overlaps(E, en, nodes, (size_t)n_nodes * sizeof(int32_t)) &&
                    !overlaps(prior, pn, nodes, (size_t)n_nodes * sizeof(int32_t)) &&
                    !overlaps(E, en, ptr, (size_t)(n_rows + 1) * sizeof(int64_t)) &&
                    !overlaps(prior, pn, ptr, (size_t)(n_rows + 1) * sizeof(int64_t)),
                GRF_EINVAL, "grf_posterior_rhs_f64: an output overlaps an input or the other output");
    hipStream_t st = S(stream);
    if (n_cols > 0) {
        const int lg = post_lg_cols(n_nodes);
        const int64_t wave_rows = 64 >> lg;
        const unsigned zb = (unsigned)std::min<int64_t>(cdiv<int64_t>(n_cols, 4 * wave_rows), 4096);
        posterior_rhs_zero_kernel<<<zb, 256, 0, st>>>(n_cols, n_nodes, lg, E, lde);
        GRF_CHECK_LAUNCH("posterior_rhs_zero_kernel");
    }
    posterior_rhs_kernel<<<(unsigned)cdiv<int32_t>(n_nodes, 4), 256, 0, st>>>(n_rows, ptr, idx, val, n_cols, nodes,
                                                                               n_nodes, E, lde, prior);
    GRF_CHECK_LAUNCH("posterior_rhs_kernel");
    return GRF_OK;
}

size_t grf_posterior_reduce_workspace_bytes(int64_t n, int32_t n_rhs) {
    const int32_t S = std::max<int32_t>(1, std::min<int32_t>(n_rhs, kPostMaxRhs));
    const int64_t rows = std::max<int64_t>(0, std::min<int64_t>(n, (1ll << 31) - 1));
    return 256 + al256((size_t)post_plan(rows, S).blocks_bound * 2 * S * sizeof(double));  // ticket, partials
}

int32_t grf_posterior_reduce_f64(int64_t n, int32_t n_rhs, const double *B, int64_t ldb, const double *X,
                                 int64_t ldx, const double *alpha, const double *prior, double add_noise,
                                 double *var, double *mean, void *workspace, size_t workspace_bytes,
                                 grf_stream_t stream) {
    GRF_REQUIRE(n >= 0 && n_rhs >= 0, GRF_EINVAL, "grf_posterior_reduce_f64: negative size");
    GRF_REQUIRE(n_rhs <= kPostMaxRhs, GRF_EUNSUPPORTED, "grf_posterior_reduce_f64: n_rhs must be in [0, %d]",
                kPostMaxRhs);
    GRF_REQUIRE(n < (1ll << 31), GRF_EUNSUPPORTED, "grf_posterior_reduce_f64: more than 2^31 rows");
    if (n_rhs == 0) return GRF_OK;
    GRF_REQUIRE(prior && var, GRF_EINVAL, "grf_posterior_reduce_f64: prior or var is NULL");
    GRF_REQUIRE((alpha == nullptr) == (mean == nullptr), GRF_EINVAL,
                "grf_posterior_reduce_f64: alpha and mean go together");
    GRF_REQUIRE(n == 0 || (B && X), GRF_EINVAL, "grf_posterior_reduce_f64: a dense operand is NULL");
    GRF_REQUIRE(n == 0 || (ldb >= n_rhs && ldx >= n_rhs), GRF_EINVAL, "grf_posterior_reduce_f64: a pitch is below n_rhs");
    const size_t need = grf_posterior_reduce_workspace_bytes(n, n_rhs);
    GRF_REQUIRE(workspace && workspace_bytes >= need, GRF_EINVAL,
                "grf_posterior_reduce_f64: workspace too small (%zu < %zu)", workspace_bytes, need);
    const size_t cn = (size_t)n_rhs * sizeof(double);
    const struct {
        const void *p;
        size_t bytes;
    } ins[] = {{B, span(n, n_rhs, ldb)}, {X, span(n, n_rhs, ldx)}, {alpha, (size_t)n * sizeof(double)},
               {prior, cn},              {workspace, need}};
    for (const auto &in : ins)
        GRF_REQUIRE(!overlaps(var, cn, in.p, in.bytes) && !overlaps(mean, cn, in.p, in.bytes), GRF_EINVAL,
                    "grf_posterior_reduce_f64: an output overlaps an input or the workspace");
    GRF_REQUIRE(!overlaps(var, cn, mean, cn), GRF_EINVAL, "grf_posterior_reduce_f64: var overlaps mean");
    hipStream_t st = S(stream);
    uint32_t *ticket = (uint32_t *)workspace;
    double *part = (double *)((char *)workspace + 256);
    GRF_CHECK_HIP(hipMemsetAsync(ticket, 0, 256, st));
    const PostPlan p = post_plan(n, n_rhs);
    const int lg = post_lg_cols(n_rhs);
#define GRF_POST(NCV)                                                                                              \
    posterior_reduce_kernel<NCV><<<p.blocks, kPostThreads, 0, st>>>(n, n_rhs, lg, p.rows_per_block, B, ldb, X, ldx, \
                                                                    alpha, prior, add_noise, part, ticket, var, mean)
    if (n_rhs <= 64) GRF_POST(1);
    else if (n_rhs <= 128) GRF_POST(2);
    else if (n_rhs <= 192) GRF_POST(3);
    else GRF_POST(4);
#undef GRF_POST
    GRF_CHECK_LAUNCH("posterior_reduce_kernel");
    return GRF_OK;
}

#pragma GCC visibility pop
}  // extern "C"
