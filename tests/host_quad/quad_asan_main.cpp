// csrc/lam_host_quad.h -- the very header the product build includes -- as a stand-alone program for
// g++ -fsanitize=address,undefined (tests/test_quadrature_cpu.py builds and runs it; it is never loaded into another process).
// Every array is allocated at exactly its stated size, so a read or write past k, k - 1 or nshifts elements is a heap overflow the
// sanitizer reports.  Checks the rule against the moments it must integrate exactly (sum of the weights = 1, first moment =
// alpha_1, second = alpha_1^2 + beta_1^2), the shift identity and every refusal; prints "ok quadrature" at the end.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "lam_host_quad.h"

static unsigned long long g_state = 0x9E3779B97F4A7C15ull;
static double uniform()
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_state >> 11) * (1.0 / 9007199254740992.0);
}

static int run(int k)
{
    std::vector<double> alpha((size_t)k), beta((size_t)(k > 1 ? k - 1 : 0));
    for (double &a : alpha) a = 1.0 + 2.0 * uniform();
    for (double &b : beta) b = 0.05 + 0.4 * uniform();
    const double *bp = beta.empty() ? nullptr : beta.data();
    const double gate = 32.0 * k * 0x1p-53;
    std::vector<double> theta((size_t)k), w((size_t)k);
    if (lam::tridiag_gauss_rule(k, alpha.data(), bp, theta.data(), w.data()) != 0) return 1;
    double sw = 0.0;
    for (int i = 0; i < k; i++) {
        if (i > 0 && theta[(size_t)i] < theta[(size_t)i - 1]) return 2;
        if (!(w[(size_t)i] >= 0.0)) return 3;
        sw += w[(size_t)i];
    }
    if (std::fabs(sw - 1.0) > gate) return 4;
    std::vector<double> sigma = {0.0, 0.5, 2.0}, out(sigma.size());
    lam::QuadBad bad;
    // p = 0, 1, 2: exact whatever k
    if (lam::tridiag_quadrature(k, alpha.data(), bp, lam::kQuadPow, 0.0, 3, sigma.data(), out.data(), &bad) != 0) return 5;
    for (double v : out)
        if (std::fabs(v - 1.0) > gate) return 6;
    if (lam::tridiag_quadrature(k, alpha.data(), bp, lam::kQuadPow, 1.0, 3, sigma.data(), out.data(), &bad) != 0) return 7;
    for (size_t s = 0; s < sigma.size(); s++)
        if (std::fabs(out[s] - (alpha[0] + sigma[s])) > gate * 8.0) return 8;
    if (lam::tridiag_quadrature(k, alpha.data(), bp, lam::kQuadPow, 2.0, 3, sigma.data(), out.data(), &bad) != 0) return 9;
    for (size_t s = 0; s < sigma.size(); s++) {
        const double a = alpha[0] + sigma[s], want = a * a + (k > 1 ? beta[0] * beta[0] : 0.0);
        if (std::fabs(out[s] - want) > gate * 64.0) return 10;
    }
    // log and inverse: finite, ordered in the shift as the functions are; one shift through the NULL form
    std::vector<double> lg(sigma.size()), iv(sigma.size()), one(1);
    if (lam::tridiag_quadrature(k, alpha.data(), bp, lam::kQuadLog, 0.0, 3, sigma.data(), lg.data(), &bad) != 0) return 11;
    if (lam::tridiag_quadrature(k, alpha.data(), bp, lam::kQuadInv, 0.0, 3, sigma.data(), iv.data(), &bad) != 0) return 12;
    if (!(lg[0] < lg[1] && lg[1] < lg[2] && iv[0] > iv[1] && iv[1] > iv[2] && iv[2] > 0.0)) return 13;
    if (lam::tridiag_quadrature(k, alpha.data(), bp, lam::kQuadInv, 0.0, 1, nullptr, one.data(), nullptr) != 0 || one[0] != iv[0]) return 14;
    // a node the function cannot take: the first (shift, node)
    std::vector<double> neg = {0.0, -theta[0], -1e3};
    if (lam::tridiag_quadrature(k, alpha.data(), bp, lam::kQuadLog, 0.0, 3, neg.data(), out.data(), &bad) != -4) return 15;
    if (bad.shift != 1 || bad.node != 0 || bad.value != 0.0) return 16;
    if (lam::tridiag_quadrature(k, alpha.data(), bp, lam::kQuadInv, 0.0, 3, neg.data(), out.data(), &bad) != -4 || bad.shift != 1) return 17;
    return 0;
}

int main()
{
    const int sizes[] = {1, 2, 3, 7, 40, 255, 256};
    for (int k : sizes) {
        const int rc = run(k);
        if (rc != 0) { printf("k = %d: check %d failed\n", k, rc); return 1; }
    }
    // refusals
    std::vector<double> a = {2.0, 3.0}, b = {0.5}, out(1), s1 = {0.0};
    lam::QuadBad bad;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    int fails = 0;
    fails += lam::tridiag_quadrature(0, a.data(), b.data(), lam::kQuadInv, 0.0, 1, s1.data(), out.data(), &bad) != -1;
    fails += lam::tridiag_quadrature(lam::kMaxLanczos + 1, a.data(), b.data(), lam::kQuadInv, 0.0, 1, s1.data(), out.data(), &bad) != -1;
    fails += lam::tridiag_quadrature(2, nullptr, b.data(), lam::kQuadInv, 0.0, 1, s1.data(), out.data(), &bad) != -1;
    fails += lam::tridiag_quadrature(2, a.data(), nullptr, lam::kQuadInv, 0.0, 1, s1.data(), out.data(), &bad) != -1;
    fails += lam::tridiag_quadrature(2, a.data(), b.data(), lam::kQuadInv, 0.0, 1, s1.data(), nullptr, &bad) != -1;
    fails += lam::tridiag_quadrature(2, a.data(), b.data(), lam::kQuadInv, 0.0, 0, s1.data(), out.data(), &bad) != -1;
    fails += lam::tridiag_quadrature(2, a.data(), b.data(), lam::kQuadInv, 0.0, 2, nullptr, out.data(), &bad) != -1;
    fails += lam::tridiag_quadrature(2, a.data(), b.data(), 3, 0.0, 1, s1.data(), out.data(), &bad) != -1;
    fails += lam::tridiag_quadrature(2, a.data(), b.data(), lam::kQuadPow, 2.5, 1, s1.data(), out.data(), &bad) != -3;
    fails += lam::tridiag_quadrature(2, a.data(), b.data(), lam::kQuadPow, -1.0, 1, s1.data(), out.data(), &bad) != -3;
    fails += lam::tridiag_quadrature(2, a.data(), b.data(), lam::kQuadPow, nan, 1, s1.data(), out.data(), &bad) != -3;
    for (double v : {nan, inf}) {
        std::vector<double> a2 = {2.0, v}, b2 = {v}, s2 = {v};
        fails += lam::tridiag_quadrature(2, a2.data(), b.data(), lam::kQuadInv, 0.0, 1, s1.data(), out.data(), &bad) != -2;
        fails += lam::tridiag_quadrature(2, a.data(), b2.data(), lam::kQuadInv, 0.0, 1, s1.data(), out.data(), &bad) != -2;
        fails += lam::tridiag_quadrature(2, a.data(), b.data(), lam::kQuadInv, 0.0, 1, s2.data(), out.data(), &bad) != -2;
    }
    if (fails != 0) { printf("%d refusals missed\n", fails); return 1; }
    printf("ok quadrature\n");
    return 0;
}
