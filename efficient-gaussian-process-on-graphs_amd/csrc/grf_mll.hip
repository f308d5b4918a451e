// grf_mll.hip -- the modulator gradient's contraction of the matrix-free marginal likelihood.
//
// With K^ = Phi_T Phi_T^T + s2 I and Phi = sum_l f_l M_l, dK^/df_l = M_l[T] Phi_T^T + Phi_T M_l[T]^T, so
// for a pair of vectors (a, b) with W_a = Phi_T^T a, W_b = Phi_T^T b
//     a^T dK^/df_l b = sum_r a_r (M_l[T] W_b)_r + b_r (M_l[T] W_a)_r.
// The gradient needs this for S = 1 + t pairs at once (the data column and t probes) and only its weighted
// sum over the pairs:
//     out[l] = sum_c wt[c] sum_r ( A[r,c] (M_l[row_map[r]] WB)[c] + B[r,c] (M_l[row_map[r]] WA)[c] ).
// steps_frob_kernel is that SpMM fused with the weighted Frobenius inner product: the n_sel x S products
// M_l[T] W are never written, and all L steps go in one launch (blockIdx.y = step).
//
// One wave per (row, step) item; lanes own the columns lane + 64 i.  The row's entry indices and values are
// loaded 64 at a time and broadcast lane by lane, so every gathered row of WA / WB is one contiguous
// S x 8-byte read.  A[r, :] and B[r, :] are read once per item.  Every sum has a fixed order: the wave's
// rows ascending, the lanes by an xor tree, the four waves in order, one fp64 partial per block, and the
// last block (by ticket) adds the partials in block order -- two calls give the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "grf_block.h"

namespace grf {
namespace {

constexpr int kFrobMaxSteps = 64;
constexpr int kFrobMaxRhs = 256;   // 4 columns per lane
constexpr int kFrobBlocks = 512;   // row blocks per step (grid.x)

struct FrobSteps {  // L <= 64 step matrices (device pointers), passed by value
    const int64_t *ptr[kFrobMaxSteps];
    const int32_t *idx[kFrobMaxSteps];
    const float *val[kFrobMaxSteps];
};

unsigned frob_row_blocks(int64_t n_sel) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv<int64_t>(n_sel, 4), kFrobBlocks));
}

// NC = ceil(S / 64) column chunks per lane
template <int NC>
__global__ __launch_bounds__(256) void steps_frob_kernel(int64_t n_sel, int32_t L, FrobSteps sp,
                                                         const int32_t *row_map, const double *A, const double *B,
                                                         int64_t ld, const double *WA, const double *WB, int64_t ldw,
                                                         const double *wt, int32_t S, double *part, uint32_t *ticket,
                                                         double *out) {
    __shared__ double red[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int l = blockIdx.y;
    const int64_t *ptr = sp.ptr[l];
    const int32_t *idx = sp.idx[l];
    const float *val = sp.val[l];
    bool ok[NC];
    int col[NC];
    double wgt[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        const int c = lane + 64 * i;
        ok[i] = c < S;
        col[i] = ok[i] ? c : 0;
        wgt[i] = ok[i] ? wt[c] : 0.0;
    }
    double acc = 0.0;
    const int64_t n_waves = (int64_t)gridDim.x * 4;
    for (int64_t r = (int64_t)blockIdx.x * 4 + w; r < n_sel; r += n_waves) {
        const int64_t row = uniform(row_map ? (int64_t)row_map[r] : r);
        const int64_t e0 = uniform(ptr[row]), e1 = uniform(ptr[row + 1]);
        if (e0 >= e1) continue;
        double a[NC], b[NC], s[NC];
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            a[i] = ok[i] ? A[r * ld + col[i]] : 0.0;
            b[i] = ok[i] ? B[r * ld + col[i]] : 0.0;
            s[i] = 0.0;
        }
        for (int64_t eb = e0; eb < e1; eb += 64) {
            const int64_t e = eb + lane;
            const int32_t k_l = e < e1 ? idx[e] : 0;
            const float v_l = e < e1 ? val[e] : 0.f;
            const int cnt = (int)min<int64_t>(64, e1 - eb);
            int j = 0;
            for (; j + 2 <= cnt; j += 2) {  // two entries' rows of WA / WB in flight
                double xa[2][NC], xb[2][NC], v[2];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int64_t k = __builtin_amdgcn_readlane(k_l, j + u);
                    v[u] = (double)__builtin_bit_cast(
                        float, __builtin_amdgcn_readlane(__builtin_bit_cast(int32_t, v_l), j + u));
#pragma unroll
                    for (int i = 0; i < NC; ++i) {
                        xa[u][i] = ok[i] ? WA[k * ldw + col[i]] : 0.0;
                        xb[u][i] = ok[i] ? WB[k * ldw + col[i]] : 0.0;
                    }
                }
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int i = 0; i < NC; ++i) s[i] = fma(v[u], fma(a[i], xb[u][i], b[i] * xa[u][i]), s[i]);
            }
            for (; j < cnt; ++j) {
                const int64_t k = __builtin_amdgcn_readlane(k_l, j);
                const double v =
                    (double)__builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int32_t, v_l), j));
#pragma unroll
                for (int i = 0; i < NC; ++i) {
                    const double xa = ok[i] ? WA[k * ldw + col[i]] : 0.0;
                    const double xb = ok[i] ? WB[k * ldw + col[i]] : 0.0;
                    s[i] = fma(v, fma(a[i], xb, b[i] * xa), s[i]);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < NC; ++i) acc = fma(wgt[i], s[i], acc);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
    if (lane == 0) red[w] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[(int64_t)l * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
    if (!block_is_last(ticket, gridDim.x * gridDim.y)) return;
    // the last block: step ll's partials summed in block order
    const int nb = gridDim.x;
    for (int ll = threadIdx.x; ll < L; ll += 256) {
        double sum = 0.0;
        for (int bq = 0; bq < nb; ++bq) sum += __builtin_nontemporal_load(&part[(int64_t)ll * nb + bq]);
        out[ll] = sum;
    }
    if (threadIdx.x == 0) *ticket = 0u;
}

}  // namespace
}  // namespace grf

using namespace grf;

extern "C" {
#pragma GCC visibility push(default)

size_t grf_steps_frob_workspace_bytes(int64_t n_sel, int32_t L) {
    const int64_t steps = std::max<int32_t>(1, std::min<int32_t>(L, kFrobMaxSteps));
    return 256 + al256((size_t)steps * frob_row_blocks(n_sel) * sizeof(double));  // ticket, partials
}

int32_t grf_steps_frob_f64(int64_t n_sel, int32_t L, const int64_t *const *step_ptr, const int32_t *const *step_idx,
                           const float *const *step_val, const int32_t *row_map, const double *A, const double *B,
                           int64_t ld, const double *WA, const double *WB, int64_t ldw, const double *wt,
                           int32_t n_rhs, double *out, void *workspace, size_t workspace_bytes,
                           grf_stream_t stream) {
    GRF_REQUIRE(n_sel >= 0 && L >= 1 && step_ptr && step_idx && step_val && out, GRF_EINVAL,
                "grf_steps_frob_f64: bad arguments");
    GRF_REQUIRE(L <= kFrobMaxSteps, GRF_EUNSUPPORTED, "grf_steps_frob_f64: more than %d step matrices",
                kFrobMaxSteps);
    GRF_REQUIRE(n_rhs >= 1, GRF_EINVAL, "grf_steps_frob_f64: n_rhs must be at least 1");
    GRF_REQUIRE(n_rhs <= kFrobMaxRhs, GRF_EUNSUPPORTED, "grf_steps_frob_f64: n_rhs must be in [1, %d]", kFrobMaxRhs);
    GRF_REQUIRE(ld >= n_rhs && ldw >= n_rhs && wt, GRF_EINVAL, "grf_steps_frob_f64: bad strides or weights");
    GRF_REQUIRE(n_sel == 0 || (A && B && WA && WB), GRF_EINVAL, "grf_steps_frob_f64: a dense operand is NULL");
    GRF_REQUIRE(n_sel < (1ll << 31), GRF_EUNSUPPORTED, "grf_steps_frob_f64: more than 2^31 rows");
    for (int l = 0; l < L; ++l)
        GRF_REQUIRE(step_ptr[l], GRF_EINVAL, "grf_steps_frob_f64: step %d has no row pointers", l);
    const size_t need = grf_steps_frob_workspace_bytes(n_sel, L);
    GRF_REQUIRE(workspace && workspace_bytes >= need, GRF_EINVAL,
                "grf_steps_frob_f64: workspace too small (%zu < %zu)", workspace_bytes, need);
    hipStream_t st = S(stream);
    if (n_sel == 0) {
        GRF_CHECK_HIP(hipMemsetAsync(out, 0, (size_t)L * sizeof(double), st));
        return GRF_OK;
    }
    uint32_t *ticket = (uint32_t *)workspace;
    double *part = (double *)((char *)workspace + 256);
    GRF_CHECK_HIP(hipMemsetAsync(ticket, 0, 256, st));
    FrobSteps sp{};
    for (int l = 0; l < L; ++l) {
        sp.ptr[l] = step_ptr[l];
        sp.idx[l] = step_idx[l];
        sp.val[l] = step_val[l];
    }
    const dim3 grid(frob_row_blocks(n_sel), (unsigned)L);
#define GRF_FROB(NCV)                                                                                               \
    steps_frob_kernel<NCV><<<grid, 256, 0, st>>>(n_sel, L, sp, row_map, A, B, ld, WA, WB, ldw, wt, n_rhs, part, \
                                                  ticket, out)
    if (n_rhs <= 64) GRF_FROB(1);
    else if (n_rhs <= 128) GRF_FROB(2);
    else if (n_rhs <= 192) GRF_FROB(3);
    else GRF_FROB(4);
#undef GRF_FROB
    GRF_CHECK_LAUNCH("steps_frob_kernel");
    return GRF_OK;
}

#pragma GCC visibility pop
}  // extern "C"
