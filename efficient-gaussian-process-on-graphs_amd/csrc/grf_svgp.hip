// grf_svgp.hip -- sparse variational GP classification: the RobustMax likelihood's Gauss-Hermite quadrature with
// its gradient, the predictive class probabilities, and row sums of squares (include/grf_svgp.h).
//
// robustmax_ve_kernel / robustmax_predict_kernel.  The quadrature is short and latency-bound (n P n_gh erf and exp
// evaluations), so a data point's nodes are spread over G = next_pow2(n_gh) neighbouring lanes, 64 / G points per
// wave, four waves per workgroup; lane i of a group holds node i in registers (x_i, w_i, the running product, one
// running sum): no lane keeps an array, so there is no private segment.  mu[n, c] and var[n, c] are read by every
// lane of a group at one address (a broadcast).  The sums over the nodes are xor butterflies over the group's lanes
// (ds_bpermute): lane a adds v_a + v_b where lane b adds v_b + v_a, so every lane ends with the same bits, those of
// the pairwise tree of the header's order rule.  The gradient pass evaluates C_ic again instead of keeping P
// values per lane: the leave-one-out product is the full product divided by C_ic.
//
// rows_sqsum_kernel.  One wave per (row, group): lane l chains RN(t * t) over j = l, l + 64, ... (coalesced), then
// the same butterfly over the 64 lanes.
//
// No control flow depends on the data: an out-of-range label reads class 0 and its row is overwritten with NaN.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>

#include "grf_common.h"
#include "grf_svgp.h"

namespace grf {
namespace {

constexpr double kClip = 1e-10;                    // GPflow's clip of the variances
constexpr double kSqrt2 = 1.4142135623730951;      // RN(sqrt 2) = np.sqrt(2.0)
constexpr double kSqrtPi = 1.7724538509055159;     // RN(sqrt pi) = np.sqrt(np.pi)
constexpr double kSqrt2Pi = 2.5066282746310002;    // RN(sqrt(2 pi))
constexpr double kCdfScale = 1.0 - 2e-4;
constexpr double kCdfShift = 1e-4;
constexpr int kThreads = 256;

__device__ inline double clip(double v) { return v < kClip ? kClip : v; }  // (a NaN stays a NaN)

__device__ inline double cdf(double d) { return (0.5 * (1.0 + erf(d / kSqrt2))) * kCdfScale + kCdfShift; }

// the pairwise tree over the G lanes of a group (G a power of two <= 64); every lane gets the sum
__device__ inline double group_sum(double v, int G) {
    for (int off = 1; off < G; off <<= 1) v = v + __shfl_xor(v, off, kWave);
    return v;
}

// prod_{c != y} C_ic in ascending c for the node at x
__device__ inline double product(int P, const double *m, const double *v, int y, double x) {
    double prod = 1.0;
    for (int c = 0; c < P; ++c) {
        const double C = cdf((x - m[c]) / sqrt(clip(v[c])));
        prod = prod * (c == y ? 1.0 : C);
    }
    return prod;
}

struct Lane {
    int64_t pt, r;   // the group's data point, and the row it reads (the last row where pt >= n)
    int i;           // the lane's node
    bool row, live;  // pt < n; i < n_gh
    double gx, w;    // gh_x[i], gh_w[i] / sqrt(pi) (0 on the lanes beyond n_gh)
};

__device__ inline Lane lane_of(int64_t n, int G, const double *gh_x, const double *gh_w, int n_gh) {
    Lane l;
    l.pt = (int64_t)blockIdx.x * (kThreads / G) + threadIdx.x / G;
    l.i = threadIdx.x % G;
    l.row = l.pt < n;
    l.r = l.row ? l.pt : n - 1;
    l.live = l.i < n_gh;
    const int k = l.live ? l.i : 0;
    l.gx = l.live ? gh_x[k] : 0.0;
    l.w = l.live ? gh_w[k] / kSqrtPi : 0.0;
    return l;
}

__global__ __launch_bounds__(kThreads) void robustmax_ve_kernel(
    int64_t n, int P, const double *mu, int64_t ldmu, const double *var, int64_t ldvar, const int32_t *y,
    const double *gh_x, const double *gh_w, int n_gh, int G, double log_hit, double log_miss, double *ve, double *dmu,
    int64_t lddmu, double *dvar, int64_t lddvar) {
    const Lane l = lane_of(n, G, gh_x, gh_w, n_gh);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const int32_t label = y[l.r];
    const bool ok = label >= 0 && label < P;
    const int yc = ok ? label : 0;
    const double *m = mu + l.r * ldmu, *v = var + l.r * ldvar;
    const double vy2 = 2.0 * v[yc];
    const double sx = sqrt(clip(vy2));
    const double x = m[yc] + l.gx * sx;
    const double prod = product(P, m, v, yc, x);
    const double p = group_sum(l.live ? prod * l.w : 0.0, G);
    const bool writer = l.row && l.i == 0;
    if (writer) ve[l.pt] = ok ? p * log_hit + (1.0 - p) * log_miss : nan;
    if (!dmu) return;
    const double dve = log_hit - log_miss;
    double *gm = dmu + l.r * lddmu, *gv = dvar + l.r * lddvar;
    double own = 0.0;   // this node's sum_{c != y} t_ic / s_c
    double sum_mu = 0.0;  // sum_{c != y} dp/dmu_c
    for (int c = 0; c < P; ++c) {
        const double vc = v[c];
        const double s = sqrt(clip(vc));
        const double d = (x - m[c]) / s;
        const double t = l.w * (prod / cdf(d)) * kCdfScale * (exp(-0.5 * (d * d)) / kSqrt2Pi);
        const bool other = c != yc;
        const bool on = l.live && other;
        const double ts = t / s;
        const double g_mu = -group_sum(on ? ts : 0.0, G);
        const double td = group_sum(on ? t * d : 0.0, G);
        const double g_var = vc < kClip ? 0.0 : -td / (2.0 * vc);
        own = own + (other ? ts : 0.0);
        sum_mu = sum_mu + (other ? g_mu : 0.0);
        if (writer && other) {
            gm[c] = ok ? dve * g_mu : nan;
            gv[c] = ok ? dve * g_var : nan;
        }
    }
    const double up = group_sum(l.live ? own * l.gx / sx : 0.0, G);
    if (writer) {
        gm[yc] = ok ? dve * (-sum_mu) : nan;
        gv[yc] = ok ? dve * (vy2 < kClip ? 0.0 : up) : nan;
    }
}

__global__ __launch_bounds__(kThreads) void robustmax_predict_kernel(
    int64_t n, int P, const double *mu, int64_t ldmu, const double *var, int64_t ldvar, const double *gh_x,
    const double *gh_w, int n_gh, int G, double hit, double miss, double *ps, int64_t ldps) {
    const Lane l = lane_of(n, G, gh_x, gh_w, n_gh);
    const double *m = mu + l.r * ldmu, *v = var + l.r * ldvar;
    for (int yy = 0; yy < P; ++yy) {
        const double x = m[yy] + l.gx * sqrt(clip(2.0 * v[yy]));
        const double prod = product(P, m, v, yy, x);
        const double p = group_sum(l.live ? prod * l.w : 0.0, G);
        if (l.row && l.i == 0) ps[l.pt * ldps + yy] = p * hit + (1.0 - p) * miss;
    }
}

__global__ __launch_bounds__(kThreads) void rows_sqsum_kernel(int64_t n, int64_t groups, int64_t len, const double *T,
                                                              int64_t ldt, const double *base, double *out,
                                                              int64_t ldout) {
    const int64_t total = n * groups;
    const int64_t wv = (int64_t)blockIdx.x * (kThreads / kWave) + threadIdx.x / kWave;
    const int lane = threadIdx.x % kWave;
    const bool live = wv < total;
    const int64_t q = live ? wv : total - 1;
    const int64_t r = q / groups, g = q % groups;
    const double *t = T + r * ldt + g * len;
    double s = 0.0;
    for (int64_t j = lane; j < len; j += kWave) {
        const double x = t[j];
        s = s + x * x;
    }
    s = group_sum(s, kWave);
    if (live && lane == 0) out[r * ldout + g] = base ? base[r] + s : s;
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

bool addressable(const void *p, size_t bytes) {
    return bytes != kSizeSaturated && (uintptr_t)p <= ~(uintptr_t)0 - bytes;
}

// the checks the two quadrature entries share (what: the entry's name)
int32_t check_quadrature(const char *what, int64_t n, int32_t P, const void *mu, int64_t ldmu, const void *var,
                         int64_t ldvar, const void *gh_x, const void *gh_w, int32_t n_gh, double epsilon) {
    GRF_REQUIRE(P >= 2 && P <= GRF_SVGP_MAX_CLASSES, GRF_EINVAL, "%s: P = %d outside [2, %d]", what, (int)P,
                GRF_SVGP_MAX_CLASSES);
    GRF_REQUIRE(n_gh >= 1 && n_gh <= GRF_SVGP_MAX_GH, GRF_EINVAL, "%s: n_gh = %d outside [1, %d]", what, (int)n_gh,
                GRF_SVGP_MAX_GH);
    GRF_REQUIRE(epsilon > 0.0 && epsilon < 1.0, GRF_EINVAL, "%s: epsilon must lie in (0, 1)", what);
    GRF_REQUIRE(mu && var && gh_x && gh_w, GRF_EINVAL, "%s: mu, var, gh_x or gh_w missing", what);
    GRF_REQUIRE(ldmu >= P && ldvar >= P, GRF_EINVAL, "%s: ldmu / ldvar below P", what);
    GRF_REQUIRE(addressable(mu, span(n, P, ldmu)) && addressable(var, span(n, P, ldvar)), GRF_EINVAL,
                "%s: ldmu / ldvar too large: the matrix does not fit the address space", what);
    return GRF_OK;
}

int group_width(int32_t n_gh) { return (int)next_pow2_u32((uint32_t)n_gh); }

}  // namespace
}  // namespace grf

using namespace grf;

extern "C" {
#pragma GCC visibility push(default)

int32_t grf_robustmax_ve_f64(int64_t n, int32_t P, const double *mu, int64_t ldmu, const double *var, int64_t ldvar,
                             const int32_t *y, const double *gh_x, const double *gh_w, int32_t n_gh, double epsilon,
                             double *ve, double *dmu, int64_t lddmu, double *dvar, int64_t lddvar,
                             grf_stream_t stream) {
    const char *who = "grf_robustmax_ve_f64";
    GRF_REQUIRE(n >= 0, GRF_EINVAL, "%s: negative size", who);
    GRF_REQUIRE(n < (1ll << 31), GRF_EUNSUPPORTED, "%s: more than 2^31 rows", who);
    if (n == 0) return GRF_OK;
    const int32_t rc = check_quadrature(who, n, P, mu, ldmu, var, ldvar, gh_x, gh_w, n_gh, epsilon);
    if (rc != GRF_OK) return rc;
    GRF_REQUIRE(y && ve, GRF_EINVAL, "%s: y or ve missing", who);
    GRF_REQUIRE((dmu == nullptr) == (dvar == nullptr), GRF_EINVAL, "%s: dmu and dvar go together", who);
    const size_t in_mu = span(n, P, ldmu), in_var = span(n, P, ldvar);
    size_t out_mu = 0, out_var = 0;
    if (dmu) {
        GRF_REQUIRE(lddmu >= P && lddvar >= P, GRF_EINVAL, "%s: lddmu / lddvar below P", who);
        out_mu = span(n, P, lddmu);
        out_var = span(n, P, lddvar);
        GRF_REQUIRE(addressable(dmu, out_mu) && addressable(dvar, out_var), GRF_EINVAL,
                    "%s: lddmu / lddvar too large: the matrix does not fit the address space", who);
    }
    {
        const void *in[5] = {mu, var, y, gh_x, gh_w};
        const size_t ins[5] = {in_mu, in_var, (size_t)n * sizeof(int32_t), (size_t)n_gh * sizeof(double),
                               (size_t)n_gh * sizeof(double)};
        const void *out[3] = {ve, dmu, dvar};
        const size_t outs[3] = {(size_t)n * sizeof(double), out_mu, out_var};
        for (int a = 0; a < 3; ++a) {
            for (int b = 0; b < 5; ++b)
                GRF_REQUIRE(!overlaps(out[a], outs[a], in[b], ins[b]), GRF_EINVAL,
                            "%s: ve, dmu and dvar must not overlap the inputs", who);
            for (int b = a + 1; b < 3; ++b)
                GRF_REQUIRE(!overlaps(out[a], outs[a], out[b], outs[b]), GRF_EINVAL,
                            "%s: ve, dmu and dvar must not overlap one another", who);
        }
    }
    const int G = group_width(n_gh);
    const int64_t blocks = cdiv<int64_t>(n, kThreads / G);
    GRF_REQUIRE_GRID(blocks, kThreads, "robustmax_ve_kernel");
    robustmax_ve_kernel<<<(unsigned)blocks, kThreads, 0, S(stream)>>>(
        n, P, mu, ldmu, var, ldvar, y, gh_x, gh_w, n_gh, G, std::log(1.0 - epsilon),
        std::log(epsilon / (double)(P - 1)), ve, dmu, lddmu, dvar, lddvar);
    GRF_CHECK_LAUNCH("robustmax_ve_kernel");
    return GRF_OK;
}

int32_t grf_robustmax_predict_f64(int64_t n, int32_t P, const double *mu, int64_t ldmu, const double *var,
                                  int64_t ldvar, const double *gh_x, const double *gh_w, int32_t n_gh,
                                  double epsilon, double *ps, int64_t ldps, grf_stream_t stream) {
    const char *who = "grf_robustmax_predict_f64";
    GRF_REQUIRE(n >= 0, GRF_EINVAL, "%s: negative size", who);
    GRF_REQUIRE(n < (1ll << 31), GRF_EUNSUPPORTED, "%s: more than 2^31 rows", who);
    if (n == 0) return GRF_OK;
    const int32_t rc = check_quadrature(who, n, P, mu, ldmu, var, ldvar, gh_x, gh_w, n_gh, epsilon);
    if (rc != GRF_OK) return rc;
    GRF_REQUIRE(ps, GRF_EINVAL, "%s: ps missing", who);
    GRF_REQUIRE(ldps >= P, GRF_EINVAL, "%s: ldps below P", who);
    const size_t out = span(n, P, ldps);
    GRF_REQUIRE(addressable(ps, out), GRF_EINVAL, "%s: ldps too large: the matrix does not fit the address space",
                who);
    GRF_REQUIRE(!overlaps(ps, out, mu, span(n, P, ldmu)) && !overlaps(ps, out, var, span(n, P, ldvar)) &&
                    !overlaps(ps, out, gh_x, (size_t)n_gh * sizeof(double)) &&
                    !overlaps(ps, out, gh_w, (size_t)n_gh * sizeof(double)),
                GRF_EINVAL, "%s: ps must not overlap the inputs", who);
    const int G = group_width(n_gh);
    const int64_t blocks = cdiv<int64_t>(n, kThreads / G);
    GRF_REQUIRE_GRID(blocks, kThreads, "robustmax_predict_kernel");
    robustmax_predict_kernel<<<(unsigned)blocks, kThreads, 0, S(stream)>>>(
        n, P, mu, ldmu, var, ldvar, gh_x, gh_w, n_gh, G, 1.0 - epsilon, epsilon / (double)(P - 1), ps, ldps);
    GRF_CHECK_LAUNCH("robustmax_predict_kernel");
    return GRF_OK;
}

int32_t grf_rows_sqsum_f64(int64_t n, int64_t groups, int64_t len, const double *T, int64_t ldt, const double *base,
                           double *out, int64_t ldout, grf_stream_t stream) {
    const char *who = "grf_rows_sqsum_f64";
    GRF_REQUIRE(n >= 0 && groups >= 0 && len >= 0, GRF_EINVAL, "%s: negative size", who);
    GRF_REQUIRE(n < (1ll << 31) && groups < (1ll << 31) && len < (1ll << 31) && groups * len < (1ll << 31),
                GRF_EUNSUPPORTED, "%s: more than 2^31 rows or columns", who);
    if (n == 0 || groups == 0) return GRF_OK;
    const int64_t width = groups * len;
    GRF_REQUIRE(out && (T || width == 0), GRF_EINVAL, "%s: T or out missing", who);
    GRF_REQUIRE(ldt >= width && ldout >= groups, GRF_EINVAL, "%s: ldt below groups * len or ldout below groups", who);
    const size_t ts = span(n, width, ldt), os = span(n, groups, ldout);
    GRF_REQUIRE(addressable(T, ts) && addressable(out, os), GRF_EINVAL,
                "%s: ldt / ldout too large: the matrix does not fit the address space", who);
    GRF_REQUIRE(!overlaps(out, os, T, ts) && !(base && overlaps(out, os, base, (size_t)n * sizeof(double))),
                GRF_EINVAL, "%s: out must not overlap T or base", who);
    const int64_t blocks = cdiv<int64_t>(n * groups, kThreads / kWave);
    GRF_REQUIRE_GRID(blocks, kThreads, "rows_sqsum_kernel");
    rows_sqsum_kernel<<<(unsigned)blocks, kThreads, 0, S(stream)>>>(n, groups, len, T, ldt, base, out, ldout);
    GRF_CHECK_LAUNCH("rows_sqsum_kernel");
    return GRF_OK;
}

#pragma GCC visibility pop
}  // extern "C"
