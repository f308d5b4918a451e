// grf_spgemm.hip -- C = A B, CSR x CSR -> CSR in fp64: the producer of the exact step matrices
// M_0 = I, M_l = M_{l-1} L (the reference's compute_pstep_walk_matrix, general_kernel_pofm.py:7-42).
//
// The result is fixed to the bit.  Row i's pattern is the union of the patterns of B's rows k over the
// stored entries (i, k) of A, columns ascending, exact-zero sums kept; c_ij starts from +0.0 and adds
// RN(a_ik b_kj) one product at a time in the order of A's row entries (ascending k), multiply and add
// rounded separately (__dmul_rn / __dadd_rn).  That is Gustavson's order, and scipy's.  No floating-point
// atomics anywhere: every c_ij is summed by one lane (sort path) or in one LDS slot by one wave (big path).
//
// Two passes, as grf_phi_steps_csr_count / _fill: count writes the row lengths, the caller scans them
// (grf_scan_counts), fill writes the rows.  In each pass a wave owns an output row and picks the row's
// path on the device from its product count P = sum over A's entries (i, k) of len(B[k]):
//   * P <= GRF_SPGEMM_SORT_PRODUCTS -- the sort path (spgemm_rows_kernel).  The products are expanded into
//     the wave's LDS as keys (column << 32 | sequence number) with the rounded product beside them, the keys
//     are sorted by a bitonic network, and the lane that finds the head of a run of equal columns adds the
//     run's products in sequence order (= k order, since one k gives a column at most once).
//   * larger rows are queued for spgemm_big_kernel (a fixed number of waves, each with a bitmap of n_cols
//     bits and a per-word rank array in the workspace).  The wave marks the row's columns in its bitmap
//     (atomicOr on bits: order-free), scans the touched word range once for the row length, the ascending
//     column list and the per-word ranks, then accumulates GRF_SPGEMM_ACC_SLOTS output slots at a time in an
//     LDS accumulator: it walks A's entries in order while the lanes cover B's row k, so the slots of one k
//     are distinct (plain read-add-write, no conflicts) and each slot receives its terms in k order.  Rows
//     with more distinct columns than one accumulator walk the products once per accumulator-full.
// Launch geometry is fixed by the shapes alone; nothing is read back to the host.
//
// Compiler resource report (hipcc -O3, gfx950; -Rpass-analysis=kernel-resource-usage), no private segment:
//   spgemm_rows_kernel<false>: 42 VGPR, 59 SGPR, 32768 B LDS (keys only), scratch 0
//   spgemm_rows_kernel<true>:  52 VGPR, 73 SGPR, 65536 B LDS, scratch 0
//   spgemm_big_kernel<false>:  36 VGPR, 52 SGPR,     0 B LDS, scratch 0
//   spgemm_big_kernel<true>:   48 VGPR, 88 SGPR, 32768 B LDS, scratch 0
#include <hip/hip_runtime.h>

#include <algorithm>

#include "grf_common.h"

namespace grf {
namespace {

constexpr int kSortCap = GRF_SPGEMM_SORT_PRODUCTS;  // products per wave in LDS (8-byte key + 8-byte product)
constexpr int kAccSlots = GRF_SPGEMM_ACC_SLOTS;     // output slots per LDS accumulator of the big path
constexpr int kRowsWaves = 4;                       // waves (rows in flight) per block of spgemm_rows_kernel
constexpr int64_t kRowsMaxBlocks = 1 << 16;
constexpr size_t kBigBudget = (size_t)256 << 20;    // bytes of bitmaps + ranks the big path aims to stay within
constexpr int kBigMinWaves = GRF_SPGEMM_BIG_MIN_WAVES, kBigMaxWaves = GRF_SPGEMM_BIG_MAX_WAVES;

struct BigPlan {  // the workspace: [counters 256 B][row queue int32 n_rows][waves x (bitmap, ranks)]
    size_t queue_off, wave_off, bitmap_bytes, wave_bytes, total;
    int64_t words;
    int waves;
};

BigPlan big_plan(int64_t n_rows, int64_t n_cols) {
    BigPlan p;
    p.words = std::max<int64_t>(1, cdiv<int64_t>(n_cols, 64));
    p.bitmap_bytes = al256((size_t)p.words * 8);
    p.wave_bytes = p.bitmap_bytes + al256((size_t)p.words * 4);
    int64_t w = (int64_t)(kBigBudget / p.wave_bytes);
    w = std::max<int64_t>(kBigMinWaves, std::min<int64_t>(kBigMaxWaves, w));
    p.waves = (int)std::max<int64_t>(1, std::min<int64_t>(w, n_rows));
    p.queue_off = 256;
    p.wave_off = p.queue_off + al256((size_t)std::max<int64_t>(n_rows, 1) * 4);
    p.total = p.wave_off + (size_t)p.waves * p.wave_bytes;
    return p;
}

__device__ inline int64_t wave_sum(int64_t v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ inline int wave_incl_scan(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int u = __shfl_up(v, d);
        if (lane >= d) v += u;
    }
    return v;
}

// P of row [a0, a1): the products of the row
__device__ inline int64_t row_products(int64_t a0, int64_t a1, const int32_t *a_idx, const int64_t *b_ptr, int lane) {
    int64_t p = 0;
    for (int64_t eb = a0; eb < a1; eb += 64) {
        const int64_t e = eb + lane;
        if (e < a1) {
            const int64_t k = a_idx[e];
            p += b_ptr[k + 1] - b_ptr[k];
        }
    }
    return uniform(wave_sum(p));
}

// Every product of the row in sequence order: A's entries ascending, 64 of them loaded at a time (their
// B rows' bounds with them) and broadcast one by one while the lanes cover B's row k.
// fn(av, b entry, sequence number) runs on one lane per product; after_k() once per A entry (wave-uniform).
template <bool VALUES, typename Fn, typename After>
__device__ inline void for_each_product(int64_t a0, int64_t a1, const int32_t *a_idx, const double *a_val,
                                        const int64_t *b_ptr, int lane, Fn fn, After after_k) {
    int64_t off = 0;
    for (int64_t eb = a0; eb < a1; eb += 64) {
        const int64_t e = eb + lane;
        int64_t b0_l = 0;
        int len_l = 0;
        double av_l = 0.0;
        if (e < a1) {
            const int64_t k = a_idx[e];
            b0_l = b_ptr[k];
            len_l = (int)(b_ptr[k + 1] - b0_l);
            if (VALUES) av_l = a_val[e];
        }
        const int incl = wave_incl_scan(len_l, lane);
        const int cnt = (int)min((int64_t)64, a1 - eb);
        for (int j = 0; j < cnt; ++j) {
            const int64_t b0 = uniform(__shfl(b0_l, j));
            const int len = uniform32(__shfl(len_l, j));
            const int64_t o = off + uniform32(__shfl(incl - len_l, j));
            const double av = VALUES ? __shfl(av_l, j) : 0.0;
            for (int t = lane; t < len; t += 64) fn(av, b0 + t, o + t);
            after_k();
        }
        off += uniform32(__shfl(incl, 63));
    }
}

// ---------------------------------------------------------------- the sort path (and the rows' triage)
template <bool FILL>
__global__ __launch_bounds__(64 * kRowsWaves) void spgemm_rows_kernel(
    int64_t n_rows, const int64_t *a_ptr, const int32_t *a_idx, const double *a_val, const int64_t *b_ptr,
    const int32_t *b_idx, const double *b_val, int32_t *row_cnt, const int64_t *c_ptr, int32_t *c_idx, double *c_val,
    float *c_val32, int32_t *queue, uint32_t *q_tail) {
    __shared__ uint64_t s_key[kRowsWaves][kSortCap];
    __shared__ double s_val[kRowsWaves][kSortCap];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint64_t *key = s_key[w];
    double *val = s_val[w];
    const int64_t stride = (int64_t)gridDim.x * kRowsWaves;
    for (int64_t row = (int64_t)blockIdx.x * kRowsWaves + w; row < n_rows; row += stride) {
        const int64_t a0 = uniform(a_ptr[row]), a1 = uniform(a_ptr[row + 1]);
        const int64_t P64 = row_products(a0, a1, a_idx, b_ptr, lane);
        if (P64 > kSortCap) {
            if (lane == 0) queue[atomicAdd(q_tail, 1u)] = (int32_t)row;
            continue;
        }
        const int P = (int)P64;
        if (P == 0) {
            if (!FILL && lane == 0) row_cnt[row] = 0;
            continue;
        }
        for_each_product<FILL>(
            a0, a1, a_idx, a_val, b_ptr, lane,
            [&](double av, int64_t be, int64_t seq) {
                key[seq] = ((uint64_t)(uint32_t)b_idx[be] << 32) | (uint32_t)seq;
                if (FILL) val[seq] = __dmul_rn(av, b_val[be]);
            },
            [] {});
        const int n_pad = max(64, (int)next_pow2_u32((uint32_t)P));
        for (int t = P + lane; t < n_pad; t += 64) key[t] = ~0ull;
        __builtin_amdgcn_wave_barrier();
        for (int k = 2; k <= n_pad; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = lane; t < (n_pad >> 1); t += 64) {
                    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                    const int l = i | j;
                    const uint64_t x = key[i], y = key[l];
                    if ((x > y) == ((i & k) == 0)) {
                        key[i] = y;
                        key[l] = x;
                    }
                }
                __builtin_amdgcn_wave_barrier();
            }
        }
        // runs of equal columns: the head's lane owns the output entry
        const int64_t cbase = FILL ? uniform(c_ptr[row]) : 0;
        int n_out = 0;
        for (int t0 = 0; t0 < P; t0 += 64) {
            const int t = t0 + lane;
            const bool valid = t < P;
            const uint32_t col = valid ? (uint32_t)(key[t] >> 32) : 0u;
            const bool head = valid && (t == 0 || (uint32_t)(key[t - 1] >> 32) != col);
            const uint64_t m = __ballot(head);
            if (FILL && head) {
                const int64_t pos = cbase + n_out + __popcll(m & ((1ull << lane) - 1ull));
                double sum = 0.0;
                for (int u = t; u < P; ++u) {
                    const uint64_t ku = key[u];
                    if ((uint32_t)(ku >> 32) != col) break;
                    sum = __dadd_rn(sum, val[(uint32_t)ku]);
                }
                c_idx[pos] = (int32_t)col;
                c_val[pos] = sum;
                if (c_val32) c_val32[pos] = (float)sum;
            }
            n_out += __popcll(m);
        }
        if (!FILL && lane == 0) row_cnt[row] = n_out;
        __builtin_amdgcn_wave_barrier();  // (the next row's keys overwrite these)
    }
}

// ---------------------------------------------------------------- the big path: one wave per block
template <bool FILL>
__global__ __launch_bounds__(64) void spgemm_big_kernel(
    const int64_t *a_ptr, const int32_t *a_idx, const double *a_val, const int64_t *b_ptr, const int32_t *b_idx,
    const double *b_val, int32_t *row_cnt, const int64_t *c_ptr, int32_t *c_idx, double *c_val, float *c_val32,
    const int32_t *queue, const uint32_t *q_tail, uint32_t *q_head, char *wave_ws, size_t wave_bytes,
    size_t bitmap_bytes) {
    __shared__ double acc[FILL ? kAccSlots : 1];
    const int lane = threadIdx.x;
    unsigned long long *bm = (unsigned long long *)(wave_ws + (size_t)blockIdx.x * wave_bytes);
    int32_t *rank = (int32_t *)((char *)bm + bitmap_bytes);
    const uint32_t n_q = *q_tail;
    for (;;) {
        uint32_t q = 0;
        if (lane == 0) q = atomicAdd(q_head, 1u);
        q = (uint32_t)uniform32((int32_t)__shfl((int)q, 0));
        if (q >= n_q) break;
        const int64_t row = queue[q];
        const int64_t a0 = uniform(a_ptr[row]), a1 = uniform(a_ptr[row + 1]);
        // 1. the row's columns into the wave's bitmap (all zero on entry)
        int32_t cmin = 0x7FFFFFFF, cmax = 0;
        for_each_product<false>(
            a0, a1, a_idx, a_val, b_ptr, lane,
            [&](double, int64_t be, int64_t) {
                const int32_t c = b_idx[be];
                atomicOr(&bm[c >> 6], 1ull << (c & 63));
                cmin = min(cmin, c);
                cmax = max(cmax, c);
            },
            [] {});
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            cmin = min(cmin, __shfl_xor(cmin, off));
            cmax = max(cmax, __shfl_xor(cmax, off));
        }
        const int64_t w_lo = uniform32(cmin) >> 6, w_hi = uniform32(cmax) >> 6;
        __threadfence();  // the bits are in memory before the scan reads them
        // 2. one ordered scan of the touched words: the row length, the columns, every word's rank
        const int64_t cbase = FILL ? uniform(c_ptr[row]) : 0;
        int n_out = 0;
        for (int64_t w0 = w_lo; w0 <= w_hi; w0 += 64) {
            const int64_t wd = w0 + lane;
            unsigned long long word = 0;
            if (wd <= w_hi) word = __hip_atomic_load(&bm[wd], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int c = __popcll(word);
            const int incl = wave_incl_scan(c, lane);
            if (FILL && wd <= w_hi) {
                int r = n_out + incl - c;
                rank[wd] = r;
                while (word) {
                    const int b = __ffsll((long long)word) - 1;
                    c_idx[cbase + r++] = (int32_t)(wd * 64 + b);
                    word &= word - 1;
                }
            }
            n_out += uniform32(__shfl(incl, 63));
        }
        if (!FILL && lane == 0) row_cnt[row] = n_out;
        if (FILL) {
            __threadfence();  // the ranks are in memory before other lanes read them
            // 3. the values, kAccSlots output slots at a time
            for (int c0 = 0; c0 < n_out; c0 += kAccSlots) {
                const int n_acc = min(kAccSlots, n_out - c0);
                for (int s = lane; s < n_acc; s += 64) acc[s] = 0.0;
                __builtin_amdgcn_wave_barrier();
                for_each_product<true>(
                    a0, a1, a_idx, a_val, b_ptr, lane,
                    [&](double av, int64_t be, int64_t) {
                        const int32_t c = b_idx[be];
                        const int64_t wd = c >> 6;
                        const int s = rank[wd] + __popcll(bm[wd] & ((1ull << (c & 63)) - 1ull)) - c0;
                        if (s >= 0 && s < n_acc) acc[s] = __dadd_rn(acc[s], __dmul_rn(av, b_val[be]));
                    },
                    [] { __builtin_amdgcn_wave_barrier(); });
                for (int s = lane; s < n_acc; s += 64) {
                    const double v = acc[s];
                    c_val[cbase + c0 + s] = v;
                    if (c_val32) c_val32[cbase + c0 + s] = (float)v;
                }
                __builtin_amdgcn_wave_barrier();
            }
        }
        // 4. the bitmap back to zero for the wave's next row
        for (int64_t wd = w_lo + lane; wd <= w_hi; wd += 64) bm[wd] = 0ull;
        __threadfence();
    }
}

int32_t check_shapes(const char *who, int64_t n_rows, int64_t n_mid, int64_t n_cols) {
    GRF_REQUIRE(n_rows >= 0 && n_mid >= 0 && n_cols >= 0, GRF_EINVAL, "%s: negative shape", who);
    GRF_REQUIRE(n_rows <= 0x7FFFFFFFll && n_mid <= 0x7FFFFFFFll && n_cols <= 0x7FFFFFFFll, GRF_EUNSUPPORTED,
                "%s: a dimension exceeds 2^31 - 1", who);
    return GRF_OK;
}

template <bool FILL>
int32_t run(const char *who, int64_t n_rows, int64_t n_cols, const int64_t *a_ptr, const int32_t *a_idx,
            const double *a_val, const int64_t *b_ptr, const int32_t *b_idx, const double *b_val, int32_t *row_cnt,
            const int64_t *c_ptr, int32_t *c_idx, double *c_val, float *c_val32, void *ws, size_t ws_bytes,
            hipStream_t st) {
    const BigPlan p = big_plan(n_rows, n_cols);
    GRF_REQUIRE(ws && ws_bytes >= p.total, GRF_EINVAL, "%s: workspace too small (%zu < %zu)", who, ws_bytes, p.total);
    if (n_rows == 0) return GRF_OK;
    char *base = (char *)ws;
    uint32_t *q_tail = (uint32_t *)base, *q_head = (uint32_t *)(base + 64);
    int32_t *queue = (int32_t *)(base + p.queue_off);
    char *wave_ws = base + p.wave_off;
    GRF_CHECK_HIP(hipMemsetAsync(base, 0, 256, st));
    GRF_CHECK_HIP(hipMemsetAsync(wave_ws, 0, (size_t)p.waves * p.wave_bytes, st));
    const unsigned blocks = (unsigned)std::min<int64_t>(cdiv<int64_t>(n_rows, kRowsWaves), kRowsMaxBlocks);
    spgemm_rows_kernel<FILL><<<blocks, 64 * kRowsWaves, 0, st>>>(n_rows, a_ptr, a_idx, a_val, b_ptr, b_idx, b_val,
                                                                  row_cnt, c_ptr, c_idx, c_val, c_val32, queue, q_tail);
    GRF_CHECK_LAUNCH("spgemm_rows_kernel");
    spgemm_big_kernel<FILL><<<(unsigned)p.waves, 64, 0, st>>>(a_ptr, a_idx, a_val, b_ptr, b_idx, b_val, row_cnt, c_ptr,
                                                              c_idx, c_val, c_val32, queue, q_tail, q_head, wave_ws,
                                                              p.wave_bytes, p.bitmap_bytes);
    GRF_CHECK_LAUNCH("spgemm_big_kernel");
    return GRF_OK;
}

}  // namespace
}  // namespace grf

using namespace grf;

extern "C" {
#pragma GCC visibility push(default)

size_t grf_spgemm_workspace_bytes(int64_t n_rows, int64_t n_mid, int64_t n_cols) {
    (void)n_mid;
    return big_plan(std::max<int64_t>(n_rows, 0), std::max<int64_t>(n_cols, 0)).total;
}

int32_t grf_spgemm_csr_count(int64_t n_rows, int64_t n_mid, int64_t n_cols, const int64_t *a_ptr, const int32_t *a_idx,
                             const int64_t *b_ptr, const int32_t *b_idx, int32_t *row_cnt, void *workspace,
                             size_t workspace_bytes, grf_stream_t stream) {
    const int32_t rc = check_shapes("grf_spgemm_csr_count", n_rows, n_mid, n_cols);
    if (rc != GRF_OK) return rc;
    GRF_REQUIRE(a_ptr && b_ptr && (n_rows == 0 || row_cnt), GRF_EINVAL, "grf_spgemm_csr_count: a NULL array");
    return run<false>("grf_spgemm_csr_count", n_rows, n_cols, a_ptr, a_idx, nullptr, b_ptr, b_idx, nullptr, row_cnt,
                      nullptr, nullptr, nullptr, nullptr, workspace, workspace_bytes, S(stream));
}

int32_t grf_spgemm_csr_fill(int64_t n_rows, int64_t n_mid, int64_t n_cols, const int64_t *a_ptr, const int32_t *a_idx,
                            const double *a_val, const int64_t *b_ptr, const int32_t *b_idx, const double *b_val,
                            const int64_t *c_ptr, int32_t *c_idx, double *c_val, float *c_val32, void *workspace,
                            size_t workspace_bytes, grf_stream_t stream) {
    const int32_t rc = check_shapes("grf_spgemm_csr_fill", n_rows, n_mid, n_cols);
    if (rc != GRF_OK) return rc;
    GRF_REQUIRE(a_ptr && b_ptr && c_ptr, GRF_EINVAL, "grf_spgemm_csr_fill: a NULL row-pointer array");
    GRF_REQUIRE(n_rows == 0 || (c_idx && c_val), GRF_EINVAL, "grf_spgemm_csr_fill: c_idx / c_val is NULL");
    return run<true>("grf_spgemm_csr_fill", n_rows, n_cols, a_ptr, a_idx, a_val, b_ptr, b_idx, b_val, nullptr, c_ptr,
                     c_idx, c_val, c_val32, workspace, workspace_bytes, S(stream));
}

#pragma GCC visibility pop
}  // extern "C"
