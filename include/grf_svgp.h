/* grf_svgp.h -- sparse variational GP classification: the RobustMax / MultiClass likelihood's Gauss-Hermite
 * quadrature with its gradient, the predictive class probabilities, and the row sums of squares of the whitened
 * conditional's variance.  An additive companion of grf.h (same library, same status codes, GRF_ABI_VERSION
 * unchanged): grf.h and grf_dense_solve.h keep naming exactly what they named before.
 *
 * Serves the reference's headline dense experiment, node classification on Cora: the notebooks
 * experiments/dense/cora/classification_multiple_{GRF,GRF_small,diff,diff_small}.ipynb build
 *     likelihood = gpflow.likelihoods.MultiClass(num_classes=7)
 *     model = gpflow.models.SVGP(kernel=graph_kernel, likelihood=likelihood, inducing_variable=Z,
 *                                num_latent_gps=7, whiten=True)
 * run Adam on model.training_loss((X, Y)) and report argmax(model.predict_y(x_test)[0]).  The formulas are those of
 * GPflow's likelihoods/multiclass.py: RobustMax.prob_is_largest, MultiClass._variational_expectations,
 * MultiClass._predict_non_logged_density and MultiClass._predict_mean_and_var.
 *
 * Layout.  Every matrix is row-major fp64 with a leading dimension; mu and var are n x P (one data point per row,
 * one latent function per column), labels are device int32.  gh_x and gh_w are the n_gh Gauss-Hermite nodes and
 * weights of numpy.polynomial.hermite.hermgauss(n_gh) as device fp64 arrays (what GPflow calls, so their bits are
 * GPflow's).  Columns [P, ld) of every matrix are never read or written.
 *
 * The probability (RobustMax.prob_is_largest) of row n with label y, node i, class c:
 *     x_i  = mu_y + gh_x[i] sqrt(max(2 var_y, 1e-10))
 *     d_ic = (x_i - mu_c) / sqrt(max(var_c, 1e-10))
 *     C_ic = (1 - 2e-4) (1/2) (1 + erf(d_ic / sqrt 2)) + 1e-4
 *     p    = sum_i (gh_w[i] / sqrt pi) prod_{c != y} C_ic
 *
 * Order rule (all three entries; fp64 throughout, no contraction, no floating-point atomics, two calls give the
 * same bits).  A data point's quadrature nodes sit on G = the next power of two >= n_gh neighbouring lanes (lanes
 * i >= n_gh hold 0).  Every product over c is one chain in ascending c, starting from 1, the factor of c = y
 * being 1.  Every sum over i is the pairwise tree over the G lanes: level k adds the partial sums of the index
 * blocks [2^(k+1) j, 2^(k+1) j + 2^k) and [2^(k+1) j + 2^k, 2^(k+1) (j + 1)), k = 0, 1, ...; the term of node i is
 * RN(w_i * prod), w_i = RN(gh_w[i] / sqrt pi).  Every sum over c (the label's own gradient) is one chain in
 * ascending c.  The leave-one-out product prod_{c' != y, c} C_ic' is the full product divided by C_ic: C >= 1e-4
 * and P <= 64, so the product cannot underflow.  grf_rows_sqsum_f64: lane l of one wave adds RN(t * t) for
 * j = l, l + 64, ... in ascending j, then the pairwise tree over the 64 lanes, then base[r] + that sum.
 */
#ifndef GRF_SVGP_H
#define GRF_SVGP_H

#include "grf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GRF_SVGP_MAX_CLASSES 64
#define GRF_SVGP_MAX_GH 64

/* grf_robustmax_ve_f64: MultiClass._variational_expectations with the RobustMax inverse link,
 *     ve[n] = p log(1 - epsilon) + (1 - p) log(epsilon / (P - 1)),
 * and in the same launch d ve[n] / d mu[n, :] and d ve[n] / d var[n, :] (dmu, dvar: n x P).  dmu and dvar are both
 * NULL for the forward-only call, whose ve has the fused call's bits.  With
 *     t_ic = w_i (prod_{c' != y, c} C_ic') (1 - 2e-4) phi(d_ic),   s_c = sqrt(max(var_c, 1e-10)),
 *     dp/dmu_c  = -sum_i t_ic / s_c,                 dp/dvar_c = -(sum_i t_ic d_ic) / (2 var_c)      (c != y),
 *     dp/dmu_y  = -sum_{c != y} dp/dmu_c,            dp/dvar_y = sum_i (sum_{c != y} t_ic / s_c) gh_x[i] / sqrt(2 var_y),
 * and d ve = (log(1 - epsilon) - log(epsilon / (P - 1))) dp.  A clipped variance (var_c < 1e-10, 2 var_y < 1e-10)
 * gets gradient 0, as tf.clip_by_value gives.  A label outside [0, P) gives NaN in that row's ve, dmu and dvar:
 * nothing is read out of bounds and no control flow depends on it.
 * n == 0 touches nothing and returns GRF_OK; n >= 2^31 is GRF_EUNSUPPORTED, and so is an n beyond one launch (2^32
 * work-items at 256 / G data points per 256-thread workgroup, G = the next power of two >= n_gh: n > 2^32 / G, which
 * is 2^26 for n_gh > 32).  P < 2, P > 64, n_gh < 1, n_gh > 64, a leading dimension below P, exactly one of dmu / dvar, an epsilon outside (0, 1) and a leading dimension whose
 * byte span does not fit the address space are GRF_EINVAL, checked before any device call.  Outputs must not
 * overlap inputs or one another. */
int32_t grf_robustmax_ve_f64(int64_t n, int32_t P, const double *mu, int64_t ldmu, const double *var, int64_t ldvar,
                             const int32_t *y, const double *gh_x, const double *gh_w, int32_t n_gh, double epsilon,
                             double *ve, double *dmu, int64_t lddmu, double *dvar, int64_t lddvar,
                             grf_stream_t stream);

/* grf_robustmax_predict_f64: MultiClass._predict_mean_and_var's mean (_predict_non_logged_density for every
 * possible label),  ps[n, c] = p_c (1 - epsilon) + (1 - p_c) epsilon / (P - 1),  p_c the probability above with the
 * label set to c.  (The variance is ps - ps^2.)  Arguments are checked as in grf_robustmax_ve_f64. */
int32_t grf_robustmax_predict_f64(int64_t n, int32_t P, const double *mu, int64_t ldmu, const double *var,
                                  int64_t ldvar, const double *gh_x, const double *gh_w, int32_t n_gh,
                                  double epsilon, double *ps, int64_t ldps, grf_stream_t stream);

/* grf_rows_sqsum_f64: out[r, g] = base[r] + sum_{j < len} T[r, g len + j]^2 (base == NULL: the sum alone), T n x
 * (groups len) at pitch ldt, out n x groups at pitch ldout.  The variational term of the whitened conditional's
 * variance (groups = P latents, len = M inducing points) without an n x P M temporary of squares.  n == 0 or
 * groups == 0 touches nothing and returns GRF_OK; len == 0 writes base (or 0).  Negative sizes, ldt < groups len,
 * ldout < groups and a byte span that does not fit the address space are GRF_EINVAL; n, groups len >= 2^31 or more
 * than 2^32 work-items (n groups > 2^26) are GRF_EUNSUPPORTED.  out must not overlap T or base. */
int32_t grf_rows_sqsum_f64(int64_t n, int64_t groups, int64_t len, const double *T, int64_t ldt, const double *base,
                           double *out, int64_t ldout, grf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GRF_SVGP_H */
