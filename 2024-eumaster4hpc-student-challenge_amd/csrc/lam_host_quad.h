// lam_host_quad.h -- Gauss quadrature from a Lanczos tridiagonal on the HOST: e_1^T f(T + sigma I) e_1 for the functions of
// lam_hip_trace_quadrature, the body of lam_hip_tridiag_quadrature.  No HIP, no context, no allocation beyond a few
// std::vector<double>: tests/host_quad builds this file (and lam_host_tridiag.h, which it stands on) alone with
// g++ -fsanitize=address,undefined.
//
// T = S diag(theta) S^T gives e_1^T f(T + sigma I) e_1 = sum_i S_{1i}^2 f(theta_i + sigma): the nodes are T's eigenvalues and the
// weights the squared FIRST components of its eigenvectors.  tridiag_eigen's one-row sweep carries the LAST components, so it is run
// on the reversed tridiagonal J T J (J the exchange matrix: diagonal and off-diagonal read back to front), whose eigenvectors are
// J s_i: their last components are the first components of T's.  O(k^2), and S is never formed.  A shift moves the nodes and leaves
// the weights alone, so every shift of a sweep is one more pass over the k nodes.
#pragma once

#include <cmath>
#include <vector>

#include "lam_host_tridiag.h"

namespace lam {

constexpr int kQuadLog = 0;           // == LAM_HIP_QUAD_LOG: f(t) = log t
constexpr int kQuadInv = 1;           // == LAM_HIP_QUAD_INV: f(t) = 1 / t
constexpr int kQuadPow = 2;           // == LAM_HIP_QUAD_POW: f(t) = t^p, p = (int)param >= 0

// where tridiag_quadrature found a node it cannot take: the first one in (shift, node) order
struct QuadBad {
    int shift = -1, node = -1;
    double value = 0.0;               // theta_node + sigma_shift
};

// nodes theta[0..k) ascending and weights w[0..k) = S_{1i}^2 of the tridiagonal (alpha[0..k), beta[0..k-1)).
// Returns 0, -1 for k outside 1..kMaxLanczos or a null array, -2 for a non-finite coefficient.
inline int tridiag_gauss_rule(int k, const double *alpha, const double *beta, double *theta, double *w)
{
    if (k < 1 || k > kMaxLanczos || !alpha || !theta || !w || (k > 1 && !beta)) return -1;
    std::vector<double> ra((size_t)k), rb((size_t)k, 0.0);
    for (int i = 0; i < k; i++) ra[(size_t)i] = alpha[k - 1 - i];
    for (int i = 0; i + 1 < k; i++) rb[(size_t)i] = beta[k - 2 - i];
    const int rc = tridiag_eigen(k, ra.data(), rb.data(), theta, w, nullptr);
    if (rc != 0) return rc;
    for (int i = 0; i < k; i++) w[i] *= w[i];
    return 0;
}

// out[s] = sum_i w_i f(theta_i + sigma_s), i ascending; sigma null: the one shift 0 (nshifts must be 1 then).
// Returns 0; -1 k outside 1..kMaxLanczos, nshifts < 1, a null array or an unknown fn; -2 a non-finite coefficient or shift;
// -3 kQuadPow with a param that is not an integer >= 0; -4 a node the function cannot take (kQuadLog: theta_i + sigma_s <= 0 or not
// finite; kQuadInv: == 0 or not finite), *bad (may be null) says which.
inline int tridiag_quadrature(int k, const double *alpha, const double *beta, int fn, double param, int nshifts, const double *sigma,
                              double *out, QuadBad *bad)
{
    if (nshifts < 1 || !out || (fn != kQuadLog && fn != kQuadInv && fn != kQuadPow) || (!sigma && nshifts != 1)) return -1;
    if (k < 1 || k > kMaxLanczos) return -1;
    if (fn == kQuadPow && !(param >= 0.0 && param <= 1e9 && param == std::floor(param))) return -3;
    std::vector<double> theta((size_t)k), w((size_t)k);
    const int rc = tridiag_gauss_rule(k, alpha, beta, theta.data(), w.data());
    if (rc != 0) return rc;
    for (int s = 0; s < nshifts; s++)
        if (sigma && !std::isfinite(sigma[s])) return -2;
    for (int s = 0; s < nshifts; s++) {
        const double sg = sigma ? sigma[s] : 0.0;
        double acc = 0.0;
        for (int i = 0; i < k; i++) {
            const double t = theta[(size_t)i] + sg;
            const bool refuse = !std::isfinite(t) || (fn == kQuadLog && !(t > 0.0)) || (fn == kQuadInv && t == 0.0);
            if (refuse) {
                if (bad) { bad->shift = s; bad->node = i; bad->value = t; }
                return -4;
            }
            const double f = fn == kQuadLog ? std::log(t) : (fn == kQuadInv ? 1.0 / t : std::pow(t, param));
            acc += w[(size_t)i] * f;
        }
        out[s] = acc;
    }
    return 0;
}

// mean of v[0..n) summed in ascending order, and its standard error: the sample standard deviation (ddof 1) / sqrt(n), NaN for
// n == 1.  Every operation is one IEEE operation in the order written -- no contraction into fused multiply-adds, whatever the
// compiler's default -- so that a caller who repeats the loop gets the same bits.
inline void quad_mean_error(int n, const double *v, double *mean_out, double *error_out)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double sum = 0.0;
    for (int j = 0; j < n; j++) sum += v[j];
    const double mean = sum / n;
    double ss = 0.0;
    for (int j = 0; j < n; j++) {
        const double d = v[j] - mean;
        ss += d * d;
    }
    *mean_out = mean;
    *error_out = n > 1 ? std::sqrt(ss / (n - 1)) / std::sqrt((double)n) : std::nan("");
}

}  // namespace lam
