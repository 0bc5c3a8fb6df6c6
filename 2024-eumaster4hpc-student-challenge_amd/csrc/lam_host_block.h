// lam_host_block.h -- the s x s matrices of block CG (lam_hip_solve_block, lam_block.h), s <= 8, fp64, written once for the host and
// the device: the LDL^T factorisation with the pivot rule and the inverse it gives, and the upper Cholesky factor S (G = S^T S) with
// its inverse.  The kernels of lam_kernels.h ("Block CG") call them on matrices held in LDS, lam_hip_solve_block on the initial
// B^T B, lam_hip_block_factor hands them to a caller.  No HIP, no context, no allocation, no array of their own: every matrix is the
// caller's, so on the device nothing is indexed dynamically in registers.  tests/test_block_cg_cpu.py builds this file alone with
// g++ -fsanitize=address,undefined (tests/host_block/block_asan_main.cpp).
//
// Every matrix is s x s, row-major with leading dimension s, fp64; sums run in ascending index.  Only the upper triangle of G
// (i <= j) is read.  The pivot rule (both factorisations): a pivot fails when it is not finite or <= floor, where the caller's
// floor is block_pivot_floor: s * u_TV * max_i G_ii, u_TV the unit roundoff of the VECTOR dtype (2^-53 fp64, 2^-24 fp32) -- the
// rounding level of G's own entries, as in lam_hip_eigs' breakdown rule.  Neither routine takes a square root or a quotient that a
// diagonal G of powers of four does not give exactly.
#pragma once

#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LAM_HD __host__ __device__
#else
#define LAM_HD
#endif

namespace lam {

constexpr int kBlockMaxS = 8;         // == LAM_HIP_MAX_RHS

LAM_HD inline bool block_finite(double v) { return v - v == 0.0; }

// s * u * max_i G_ii; a NaN on the diagonal is skipped here and met by its own pivot
LAM_HD inline double block_pivot_floor(int s, bool f32, const double *G)
{
    double dmax = 0.0;
    for (int i = 0; i < s; i++) {
        const double g = G[i * s + i];
        if (g > dmax) dmax = g;
    }
    return (double)s * (f32 ? 0x1p-24 : 0x1p-53) * dmax;
}

// G = L D L^T (L unit lower triangular, kept as its TRANSPOSE in the upper triangle of L: L_ji at L[i * s + j], i < j), then
// L := L^-1 in place (same storage), then Ginv = L^-T D^-1 L^-1, upper triangle computed and mirrored: symmetric bit for bit.
// L (s * s) and D (s) are scratch; Ginv may not alias G.  Returns 0, or -2 with *bad = the column whose pivot failed (Ginv is then
// not written).
LAM_HD inline int block_ldlt_inverse(int s, const double *G, double floor, double *L, double *D, double *Ginv, int *bad)
{
    *bad = -1;
    for (int j = 0; j < s; j++) {
        // t_i = L_ji d_i (parked in the lower triangle, L[j * s + i]), then L_ji
        for (int i = 0; i < j; i++) {
            double t = G[i * s + j];
            for (int k = 0; k < i; k++) t -= L[j * s + k] * L[k * s + i];
            L[j * s + i] = t;
            L[i * s + j] = t / D[i];
        }
        double d = G[j * s + j];
        for (int k = 0; k < j; k++) d -= L[k * s + j] * L[j * s + k];
        if (!block_finite(d) || !(d > floor)) { *bad = j; return -2; }
        D[j] = d;
    }
    // M = L^-1 (unit lower triangular), M_ic kept at L[i * s + c], i > c: the lower triangle, whose t values are spent.  Column c by
    // forward substitution: M_ic = -(L_ic + sum_{c < k < i} L_ik M_kc)
    for (int c = 0; c < s; c++)
        for (int i = c + 1; i < s; i++) {
            double t = L[c * s + i];
            for (int k = c + 1; k < i; k++) t += L[k * s + i] * L[k * s + c];
            L[i * s + c] = -t;
        }
    // Ginv_ij = sum_{k >= j} M_ki M_kj / d_k, i <= j (M_jj = 1)
    for (int i = 0; i < s; i++)
        for (int j = i; j < s; j++) {
            double t = 0.0;
            for (int k = j; k < s; k++) {
                const double mki = k == i ? 1.0 : L[k * s + i], mkj = k == j ? 1.0 : L[k * s + j];
                t += mki * mkj / D[k];
            }
            Ginv[i * s + j] = Ginv[j * s + i] = t;
        }
    return 0;
}

// G = S^T S, S upper triangular with a positive diagonal (row by row), and Sinv = S^-1 (upper triangular, column by column); both
// are written in full, zeros below the diagonal.  The pivot of column j is G_jj - sum_{k < j} S_kj^2.  Returns 0, or -2 with
// *bad = the column whose pivot failed (S and Sinv then hold the columns in front of it and are of no use).
LAM_HD inline int block_upper(int s, const double *G, double floor, double *S, double *Sinv, int *bad)
{
    *bad = -1;
    for (int i = 0; i < s; i++) {
        double d = G[i * s + i];
        for (int k = 0; k < i; k++) d -= S[k * s + i] * S[k * s + i];
        if (!block_finite(d) || !(d > floor)) { *bad = i; return -2; }
        const double r = std::sqrt(d);
        S[i * s + i] = r;
        for (int j = 0; j < i; j++) S[i * s + j] = 0.0;
        for (int j = i + 1; j < s; j++) {
            double t = G[i * s + j];
            for (int k = 0; k < i; k++) t -= S[k * s + i] * S[k * s + j];
            S[i * s + j] = t / r;
        }
    }
    // S Sinv = I: column j from its diagonal upwards
    for (int j = 0; j < s; j++) {
        for (int i = j + 1; i < s; i++) Sinv[i * s + j] = 0.0;
        Sinv[j * s + j] = 1.0 / S[j * s + j];
        for (int i = j - 1; i >= 0; i--) {
            double t = 0.0;
            for (int k = i + 1; k <= j; k++) t -= S[i * s + k] * Sinv[k * s + j];
            Sinv[i * s + j] = t / S[i * s + i];
        }
    }
    return 0;
}

}  // namespace lam
