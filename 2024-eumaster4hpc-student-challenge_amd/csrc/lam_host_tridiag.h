// lam_host_tridiag.h -- eigenvalues and eigenvectors of a symmetric tridiagonal matrix on the HOST: the small eigenproblem of the
// Lanczos eigensolver (lam_hip_eigs, lam_eigs.h) and the body of lam_hip_tridiag_eigen.  No HIP, no context, no allocation beyond two
// std::vector<double>: tests/host_tridiag builds this file alone with g++ -fsanitize=address,undefined.
//
// Implicit QL with Wilkinson's shift (the classical tql2 sweep).  Every rotation of the sweep acts on two COLUMNS of the eigenvector
// matrix and on each of its rows independently, so the sweep carries whichever rows it is given: the one bottom row for a
// convergence check (O(k^2) per check), all k rows for the Ritz vectors at the end (O(k^3), once).
#pragma once

#include <cmath>
#include <cstdint>
#include <utility>
#include <vector>

namespace lam {

constexpr int kMaxLanczos = 256;      // == LAM_HIP_MAX_LANCZOS

// d[0..k), e[0..k) (e[i] couples i and i + 1; e[k - 1] is ignored and taken as 0) -> d = eigenvalues, ascending.
// Z: nr rows of the eigenvector matrix, column i contiguous at Z + i * ld, on entry the same rows of the identity.
// Returns 0, or -1 if some eigenvalue did not converge in 60 sweeps (non-finite input).
inline int tridiag_ql(int k, double *d, double *e, double *Z, int nr, int ld)
{
    if (k < 1) return -1;
    e[k - 1] = 0.0;
    double f = 0.0, tst1 = 0.0;
    for (int l = 0; l < k; l++) {
        int sweeps = 0;
        const double h0 = std::fabs(d[l]) + std::fabs(e[l]);
        if (tst1 < h0) tst1 = h0;
        int m = l;                                  // the first negligible coupling at or behind l: e[k - 1] == 0 ends the search
        while (m < k - 1 && tst1 + std::fabs(e[m]) != tst1) m++;
        if (m > l) {
            double tst2;
            do {
                if (++sweeps > 60) return -1;
                const int l1 = l + 1;
                double g = d[l];
                double p = (d[l1] - g) / (2.0 * e[l]);
                double r = std::hypot(p, 1.0);
                const double pr = p + std::copysign(r, p);
                d[l] = e[l] / pr;
                d[l1] = e[l] * pr;
                const double dl1 = d[l1];
                double h = g - d[l];
                for (int i = l1 + 1; i < k; i++) d[i] -= h;
                f += h;
                p = d[m];
                double c = 1.0, c2 = 1.0, c3 = 1.0, s = 0.0, s2 = 0.0;
                const double el1 = e[l1];
                for (int i = m - 1; i >= l; i--) {
                    c3 = c2; c2 = c; s2 = s;
                    g = c * e[i];
                    h = c * p;
                    r = std::hypot(p, e[i]);
                    e[i + 1] = s * r;
                    s = e[i] / r;
                    c = p / r;
                    p = c * d[i] - s * g;
                    d[i + 1] = h + s * (c * g + s * d[i]);
                    double *zi = Z + (size_t)i * ld, *zi1 = Z + (size_t)(i + 1) * ld;
                    for (int q = 0; q < nr; q++) {
                        const double t = zi1[q];
                        zi1[q] = s * zi[q] + c * t;
                        zi[q] = c * zi[q] - s * t;
                    }
                }
                p = -s * s2 * c3 * el1 * e[l] / dl1;
                e[l] = s * p;
                d[l] = c * p;
                tst2 = tst1 + std::fabs(e[l]);
            } while (tst2 > tst1);
        }
        d[l] += f;
    }
    // ascending order (selection sort: k <= 256, and the columns move with their values)
    for (int i = 0; i + 1 < k; i++) {
        int best = i;
        for (int j = i + 1; j < k; j++)
            if (d[j] < d[best]) best = j;
        if (best != i) {
            std::swap(d[i], d[best]);
            for (int q = 0; q < nr; q++) std::swap(Z[(size_t)i * ld + q], Z[(size_t)best * ld + q]);
        }
    }
    return 0;
}

// The symmetric tridiagonal T with diagonal alpha[0..k) and off-diagonal beta[0..k-1): theta[0..k) ascending; last_row[i] = bottom
// component of eigenvector i (may be null); S != null: the whole k x k eigenvector matrix, column i contiguous at S + i * k.
// Returns 0, -1 for k outside 1..kMaxLanczos or a null alpha / theta (or beta with k > 1), -2 for non-finite input.
inline int tridiag_eigen(int k, const double *alpha, const double *beta, double *theta, double *last_row, double *S)
{
    if (k < 1 || k > kMaxLanczos || !alpha || !theta || (k > 1 && !beta)) return -1;
    std::vector<double> e((size_t)k, 0.0);
    for (int i = 0; i < k; i++) {
        if (!std::isfinite(alpha[i])) return -2;
        theta[i] = alpha[i];
    }
    for (int i = 0; i + 1 < k; i++) {
        if (!std::isfinite(beta[i])) return -2;
        e[i] = beta[i];
    }
    if (S) {
        for (size_t i = 0; i < (size_t)k * k; i++) S[i] = 0.0;
        for (int i = 0; i < k; i++) S[(size_t)i * k + i] = 1.0;
        if (tridiag_ql(k, theta, e.data(), S, k, k) != 0) return -2;
        if (last_row)
            for (int i = 0; i < k; i++) last_row[i] = S[(size_t)i * k + (k - 1)];
        return 0;
    }
    std::vector<double> row((size_t)k, 0.0);
    row[k - 1] = 1.0;
    if (tridiag_ql(k, theta, e.data(), row.data(), 1, 1) != 0) return -2;
    if (last_row)
        for (int i = 0; i < k; i++) last_row[i] = row[i];
    return 0;
}

}  // namespace lam
