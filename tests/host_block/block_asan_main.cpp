// csrc/lam_host_block.h -- the very header the product build includes -- as a stand-alone program for
// g++ -fsanitize=address,undefined (tests/test_block_cg_cpu.py builds and runs it; it is never loaded into another process).
// Every matrix is allocated at exactly s * s doubles (D at s), so a read or write past one is a heap overflow the sanitizer reports.
// Checks ||G Ginv - I||, the symmetry of Ginv bit for bit, S^T S = G, S Sinv = I and the refusals; prints "ok block" at the end.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lam_host_block.h"

static unsigned long long g_state = 0x9E3779B97F4A7C15ull;
static double uniform()
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_state >> 11) * (1.0 / 9007199254740992.0) * 2.0 - 1.0;
}

// G = X X^T + s I: symmetric positive definite, condition below 4
static int run(int s, bool f32)
{
    const size_t ss = (size_t)s * s;
    std::vector<double> X(ss), G(ss), L(ss), D(s), Ginv(ss), S(ss), Sinv(ss);
    for (double &x : X) x = uniform();
    for (int i = 0; i < s; i++)
        for (int j = 0; j < s; j++) {
            double t = i == j ? (double)s : 0.0;
            for (int k = 0; k < s; k++) t += X[(size_t)i * s + k] * X[(size_t)j * s + k];
            G[(size_t)i * s + j] = t;
        }
    const double floor = lam::block_pivot_floor(s, f32, G.data());
    if (!(floor > 0.0)) return 1;
    int bad = 99;
    if (lam::block_ldlt_inverse(s, G.data(), floor, L.data(), D.data(), Ginv.data(), &bad) != 0 || bad != -1) return 2;
    if (lam::block_upper(s, G.data(), floor, S.data(), Sinv.data(), &bad) != 0 || bad != -1) return 3;
    const double tol = 64.0 * s * 0x1p-53 * s;
    for (int i = 0; i < s; i++)
        for (int j = 0; j < s; j++) {
            if (Ginv[(size_t)i * s + j] != Ginv[(size_t)j * s + i]) return 4;
            double a = i == j ? -1.0 : 0.0, b = -G[(size_t)i * s + j], c = i == j ? -1.0 : 0.0;
            for (int k = 0; k < s; k++) {
                a += G[(size_t)i * s + k] * Ginv[(size_t)k * s + j];
                b += S[(size_t)k * s + i] * S[(size_t)k * s + j];
                c += S[(size_t)i * s + k] * Sinv[(size_t)k * s + j];
            }
            if (!(std::fabs(a) <= tol) || !(std::fabs(b) <= tol * 2 * s) || !(std::fabs(c) <= tol)) return 5;
            if (i > j && (S[(size_t)i * s + j] != 0.0 || Sinv[(size_t)i * s + j] != 0.0)) return 6;
        }
    // a floor above every pivot refuses column 0
    if (lam::block_ldlt_inverse(s, G.data(), 1e300, L.data(), D.data(), Ginv.data(), &bad) != -2 || bad != 0) return 7;
    if (lam::block_upper(s, G.data(), 1e300, S.data(), Sinv.data(), &bad) != -2 || bad != 0) return 8;
    // a duplicated column: the last one's pivot
    if (s >= 2) {
        for (int i = 0; i < s; i++) G[(size_t)i * s + s - 1] = G[(size_t)(s - 1) * s + i] = G[(size_t)i * s + 0];
        G[(size_t)(s - 1) * s + s - 1] = G[0];
        if (lam::block_ldlt_inverse(s, G.data(), floor, L.data(), D.data(), Ginv.data(), &bad) != -2 || bad != s - 1) return 9;
        if (lam::block_upper(s, G.data(), floor, S.data(), Sinv.data(), &bad) != -2 || bad != s - 1) return 10;
    }
    return 0;
}

int main()
{
    for (int s = 1; s <= lam::kBlockMaxS; s++)
        for (int f32 = 0; f32 < 2; f32++) {
            const int rc = run(s, f32 != 0);
            if (rc != 0) { std::printf("s = %d, f32 = %d: check %d failed\n", s, f32, rc); return 1; }
        }
    double zero = 0.0, nan = std::nan(""), l = 0.0, d = 0.0, out = 7.0, s1 = 7.0, s2 = 7.0;
    int bad = 0;
    if (lam::block_ldlt_inverse(1, &zero, 0.0, &l, &d, &out, &bad) != -2 || bad != 0 || out != 7.0) return 1;
    if (lam::block_ldlt_inverse(1, &nan, 0.0, &l, &d, &out, &bad) != -2 || bad != 0 || out != 7.0) return 1;
    if (lam::block_upper(1, &zero, 0.0, &s1, &s2, &bad) != -2 || bad != 0) return 1;
    if (lam::block_upper(1, &nan, 0.0, &s1, &s2, &bad) != -2 || bad != 0) return 1;
    std::printf("ok block\n");
    return 0;
}
