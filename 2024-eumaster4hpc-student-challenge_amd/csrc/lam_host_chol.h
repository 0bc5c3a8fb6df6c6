// lam_host_chol.h -- the inverse of a small symmetric positive definite matrix on the HOST: the m x m system of the deflated batch
// (lam_hip_set_deflation*, lam_deflate.h) and the body of lam_hip_chol_inverse.  No HIP, no context, no allocation beyond four
// std::vector<double>: tests/test_deflation_cpu.py builds this file alone with g++ -fsanitize=address,undefined.
//
// Square-root-free Cholesky G = L D L^T in fp64 (L unit lower triangular, row by row, sums in ascending index), L^-1 by forward
// substitution, G^-1 = L^-T D^-1 L^-1 formed as its lower triangle and mirrored, so the result is symmetric bit for bit; no square
// root, so a G whose factors are powers of two is inverted exactly.  Only the lower triangle of G is read.
#pragma once

#include <cmath>
#include <vector>

namespace lam {

constexpr int kMaxDeflation = 32;     // == LAM_HIP_MAX_DEFLATION

// G, Ginv: m x m, row-major (Ginv may not alias G).  A pivot d_j = G_jj - sum_k L_jk^2 d_k must be finite and
// > max(floor, m * 2^-52 * max_i G_ii) -- the second term is the rounding error of the factorisation's own sums, so a matrix
// that is singular in exact arithmetic (a duplicated column) is refused whatever its rounding made of the pivot.
// Returns 0; -1: m outside 1..kMaxDeflation (*bad_col = -1); -2: the pivot of column *bad_col was refused.  Nothing is written to
// Ginv by a refused call.
inline int chol_inverse(int m, const double *G, double *Ginv, double floor, int *bad_col)
{
    if (bad_col) *bad_col = -1;
    if (m < 1 || m > kMaxDeflation) return -1;
    double dmax = 0.0;
    for (int i = 0; i < m; i++) dmax = std::fmax(dmax, G[(size_t)i * m + i]);      // fmax: a NaN on the diagonal is met by its pivot
    const double lim = std::fmax(floor, (double)m * 0x1p-52 * dmax);
    std::vector<double> L((size_t)m * m, 0.0), Li((size_t)m * m, 0.0), D(m, 0.0), T(m, 0.0);
    for (int j = 0; j < m; j++) {
        // T_i = L_ji d_i, then L_ji
        for (int i = 0; i < j; i++) {
            double s = G[(size_t)j * m + i];
            for (int k = 0; k < i; k++) s -= T[k] * L[(size_t)i * m + k];
            T[i] = s;
            L[(size_t)j * m + i] = s / D[i];
        }
        double d = G[(size_t)j * m + j];
        for (int k = 0; k < j; k++) d -= L[(size_t)j * m + k] * T[k];
        if (!(d > lim) || !std::isfinite(d)) {
            if (bad_col) *bad_col = j;
            return -2;
        }
        D[j] = d;
        L[(size_t)j * m + j] = 1.0;
    }
    // Li = L^-1, unit lower triangular: column c by forward substitution
    for (int c = 0; c < m; c++) {
        Li[(size_t)c * m + c] = 1.0;
        for (int i = c + 1; i < m; i++) {
            double s = 0.0;
            for (int k = c; k < i; k++) s -= L[(size_t)i * m + k] * Li[(size_t)k * m + c];
            Li[(size_t)i * m + c] = s;
        }
    }
    // Ginv_ij = sum_{k >= i} Li_ki Li_kj / d_k, i >= j, mirrored
    for (int i = 0; i < m; i++)
        for (int j = 0; j <= i; j++) {
            double s = 0.0;
            for (int k = i; k < m; k++) s += Li[(size_t)k * m + i] * Li[(size_t)k * m + j] / D[k];
            Ginv[(size_t)i * m + j] = Ginv[(size_t)j * m + i] = s;
        }
    return 0;
}

}  // namespace lam
