// csrc/lam_host_chol.h -- the very header the product build includes -- as a stand-alone program for
// g++ -fsanitize=address,undefined (tests/test_deflation_cpu.py builds and runs it; it is never loaded into another process).
// G and Ginv are allocated at exactly m * m doubles, so a read or write past them is a heap overflow the sanitizer reports.  Checks
// ||G Ginv - I||, the symmetry of Ginv bit for bit and the refusals; prints "ok chol" at the end.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lam_host_chol.h"

static unsigned long long g_state = 0x9E3779B97F4A7C15ull;
static double uniform()
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_state >> 11) * (1.0 / 9007199254740992.0) * 2.0 - 1.0;
}

// G = X X^T + m I: symmetric positive definite, condition below 4
static int run(int m)
{
    std::vector<double> X((size_t)m * m), G((size_t)m * m), Ginv((size_t)m * m);
    for (double &x : X) x = uniform();
    for (int i = 0; i < m; i++)
        for (int j = 0; j < m; j++) {
            double s = i == j ? (double)m : 0.0;
            for (int k = 0; k < m; k++) s += X[(size_t)i * m + k] * X[(size_t)j * m + k];
            G[(size_t)i * m + j] = s;
        }
    int bad = 99;
    if (lam::chol_inverse(m, G.data(), Ginv.data(), 0.0, &bad) != 0 || bad != -1) return 1;
    for (int i = 0; i < m; i++)
        for (int j = 0; j < m; j++) {
            if (Ginv[(size_t)i * m + j] != Ginv[(size_t)j * m + i]) return 2;
            double s = i == j ? -1.0 : 0.0;
            for (int k = 0; k < m; k++) s += G[(size_t)i * m + k] * Ginv[(size_t)k * m + j];
            if (!(std::fabs(s) <= 64.0 * m * 0x1p-53)) return 3;
        }
    // a floor above every pivot refuses column 0 and leaves Ginv alone
    std::vector<double> keep(Ginv);
    if (lam::chol_inverse(m, G.data(), Ginv.data(), 1e300, &bad) != -2 || bad != 0 || keep != Ginv) return 4;
    // a duplicated column: the last one's pivot
    if (m >= 2) {
        for (int i = 0; i < m; i++) G[(size_t)i * m + m - 1] = G[(size_t)(m - 1) * m + i] = G[(size_t)i * m + 0];
        G[(size_t)(m - 1) * m + m - 1] = G[0];
        if (lam::chol_inverse(m, G.data(), Ginv.data(), 0.0, &bad) != -2 || bad != m - 1 || keep != Ginv) return 5;
    }
    return 0;
}

int main()
{
    const int sizes[] = {1, 2, 3, 7, 31, 32};
    for (int m : sizes) {
        const int rc = run(m);
        if (rc != 0) { std::printf("m = %d: check %d failed\n", m, rc); return 1; }
    }
    double one = 1.0, zero = 0.0, nan = std::nan(""), out = 7.0;
    int bad = 0;
    if (lam::chol_inverse(0, &one, &out, 0.0, &bad) != -1 || bad != -1) return 1;
    if (lam::chol_inverse(lam::kMaxDeflation + 1, &one, &out, 0.0, &bad) != -1 || bad != -1) return 1;
    if (lam::chol_inverse(1, &zero, &out, 0.0, &bad) != -2 || bad != 0) return 1;
    if (lam::chol_inverse(1, &nan, &out, 0.0, nullptr) != -2) return 1;
    if (out != 7.0) return 1;
    std::printf("ok chol\n");
    return 0;
}
