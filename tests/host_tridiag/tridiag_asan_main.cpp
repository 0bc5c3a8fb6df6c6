// csrc/lam_host_tridiag.h -- the very header the product build includes -- as a stand-alone program for
// g++ -fsanitize=address,undefined (tests/test_lanczos_cpu.py builds and runs it; it is never loaded into another process).
// Every output array is allocated at exactly its stated size, so a write past k, k - 1 or k * k elements is a heap overflow the
// sanitizer reports.  Checks the eigen-residual ||T s - theta s|| and the order of theta itself; prints "ok tridiag" at the end.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lam_host_tridiag.h"

static unsigned long long g_state = 0x9E3779B97F4A7C15ull;
static double uniform()
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_state >> 11) * (1.0 / 9007199254740992.0) * 2.0 - 1.0;
}

static int run(int k, int flavour)
{
    std::vector<double> alpha((size_t)k), beta((size_t)(k > 1 ? k - 1 : 0)), theta((size_t)k), row((size_t)k), S((size_t)k * k);
    for (double &a : alpha) a = flavour == 2 ? 1.0 : uniform();
    for (double &b : beta) b = flavour == 2 ? 1e-9 * uniform() : uniform();
    if (flavour == 1 && k > 2) beta[(size_t)k / 2] = 0.0;                     // a zero coupling in the middle decouples T
    const double *bp = beta.empty() ? nullptr : beta.data();
    if (lam::tridiag_eigen(k, alpha.data(), bp, theta.data(), row.data(), nullptr) != 0) return 1;
    std::vector<double> theta2((size_t)k), row2((size_t)k);
    if (lam::tridiag_eigen(k, alpha.data(), bp, theta2.data(), row2.data(), S.data()) != 0) return 2;
    double norm = 0.0;
    for (int i = 0; i < k; i++) {
        const double r = std::fabs(alpha[i]) + (i > 0 ? std::fabs(beta[i - 1]) : 0.0) + (i + 1 < k ? std::fabs(beta[i]) : 0.0);
        if (r > norm) norm = r;
    }
    const double gate = 8.0 * k * 0x1p-53 * norm;
    for (int i = 0; i < k; i++) {
        if (i > 0 && theta[i] < theta[i - 1]) return 3;
        if (theta[i] != theta2[i] || std::fabs(row[i]) != std::fabs(row2[i])) return 4;   // the same sweep with one row or all of them
        const double *s = &S[(size_t)i * k];
        double rr = 0.0;
        for (int q = 0; q < k; q++) {
            double t = (alpha[q] - theta[i]) * s[q];
            if (q > 0) t += beta[q - 1] * s[q - 1];
            if (q + 1 < k) t += beta[q] * s[q + 1];
            rr += t * t;
        }
        if (!(std::sqrt(rr) <= gate)) return 5;
    }
    return 0;
}

int main()
{
    const int sizes[] = {1, 2, 3, 17, 64, 255, 256};
    for (int k : sizes)
        for (int flavour = 0; flavour < 3; flavour++) {
            const int rc = run(k, flavour);
            if (rc != 0) { std::printf("k = %d flavour %d: check %d failed\n", k, flavour, rc); return 1; }
        }
    // the refusals touch nothing
    double one = 1.0, nan = std::nan(""), out = 0.0;
    if (lam::tridiag_eigen(0, &one, nullptr, &out, nullptr, nullptr) == 0) return 1;
    if (lam::tridiag_eigen(lam::kMaxLanczos + 1, &one, &one, &out, nullptr, nullptr) == 0) return 1;
    if (lam::tridiag_eigen(1, &nan, nullptr, &out, nullptr, nullptr) == 0) return 1;
    if (lam::tridiag_eigen(1, nullptr, nullptr, &out, nullptr, nullptr) == 0) return 1;
    std::printf("ok tridiag\n");
    return 0;
}
