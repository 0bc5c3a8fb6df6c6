// Generate-mode driver of the multi-right-hand-side solve (lam_hip_solve_many): dense tridiag(1,2,1) of -s N rows, -k nrhs
// right-hand sides, column j constant 2^j, solved together with one pass over the matrix per iteration.
//     test_CG_multi_rhs.out -s N -k nrhs -i max_iters [-e rel_error] [-t f64|f32] [-J] [-w W] [-T] [-S s0,s1,...] [-M] [-m] [-Y 0|1|2] [-P 0|1]
//     test_CG_multi_rhs.out -s N -E nev [-W s|l|b] [-i max_steps] [-e tol] [-t f64|f32] [-Y 0|1|2]
//     test_CG_multi_rhs.out -s N -k nrhs -i max_iters -D m [-W s|l|b] [-e rel_error] [-t f64|f32] [-T] [-Y 0|1|2]
//     test_CG_multi_rhs.out -s N -k nrhs -i max_iters -B [-e rel_error] [-t f64|f32] [-T] [-Y 0|1|2]
//     test_CG_multi_rhs.out -s N -Q nprobes [-i steps] [-S s0,s1,...] [-t f64|f32] [-Y 0|1|2]
// -J: Jacobi-preconditioned recurrences (lam_hip_solve_many_pc; off by default).  tridiag(1,2,1) has a constant diagonal, so the
// iteration and residual columns are the plain ones digit for digit: the flag exercises the path, it does not save iterations here.
// -w W: two stages (lam_hip_solve_many_x0): W iterations from x = 0, then a continuation from that solution (a fresh r = b - A x)
// for the remaining max_iters - W; num_iters is the two stages' sum, rel_err the second stage's.
// -T: each column's true residual ||b - A x|| / ||b|| (lam_hip_true_residual_many) as one more CSV column behind t_cg.
// -S s0,s1,...: 1 to 8 shifts >= 0 (lam_hip_set_shifts_many); they set nrhs, column j is (A + s_j I) x_j = b_j with the SAME
// right-hand side in every column (constant 1), and the shift is one more CSV column at the end of the line.  With -J the
// preconditioner is diag(A) + s_j I; with -w the second stage continues under the same shifts; -T measures against them.
// -M (with -S, which may then list up to 64 shifts): multi-shift CG (lam_hip_solve_mshift) -- ONE right-hand side, column 0's
// constant 1, and every shift solved behind the single-column product of the smallest shift's system; one CSV line per shift in the
// same columns, -T prints lam_hip_true_residual_mshift's values.  -M without -S, with -J or with -w is refused.
// -m: batched MINRES (lam_hip_solve_many_minres) in place of CG, from x = 0 and without a preconditioner; with it -S takes finite
// shifts of EITHER sign (without it a negative shift is refused as ever).  Same CSV columns; -T measures under the shifts.  -m with
// -J, -w or -M is refused.
// -Y 0|1|2: option "symmetric_many" of the solver's context (the batched product reads every pair of the matrix once; tridiag(1,2,1)
// is symmetric).  After the solve one line on STDERR says which product the last batched launch ran ("symmetric_many_effective"), so
// the CSV stays as it is; with more than 4 columns the option is not effective and the run proceeds on the general product.
// -P 0|1: option "packed_many" of the solver's context, with every mode of this driver (the general batched product of up to 4 fp64
// columns reads the 7-byte image of the matrix; without -P the option keeps its default, automatic).  After the solve one line on
// STDERR says whether the last batched launch read the image ("packed_many_effective"); the CSV stays as it is.  tridiag(1,2,1) is
// not packable (its rows are zeros but for three elements), so on this driver's matrix the line reports the plain product.
// -E nev: the Lanczos eigensolver (lam_hip_eigs) in place of a solve: nev extreme eigenpairs of the matrix, -W s (smallest, the
// default), l (largest) or b (both ends); -i is max_steps (default min(N, 256)), -e is tol; the start vector is
// lam_hip_generate_random_rhs(0)'s, convergence is checked every 8 steps.  One CSV line per pair found:
//     index,theta,bound,residual,converged,steps,t_load,t_comm_init,t_gemv,t_iter,t_cg
// with residual = ||A y - theta y|| / ||y|| formed on the device (lam_hip_eig_residuals; -T is implied).  -E with -J, -w, -S, -M, -m
// or -k is a usage error.
// -D m: deflated CG (lam_hip_solve_many_deflated) in place of the plain batch: lam_hip_eigs finds m (1..32) Ritz pairs of the matrix,
// -W s (smallest, the default), l or b, with its own defaults (min(N, 256) steps, tol 1e-10 / 1e-5 for f64 / f32, the start vector of
// lam_hip_generate_random_rhs(0)); they become the deflation space (lam_hip_set_deflation_eigs) and the generated right-hand sides are
// solved on it.  The usual CSV line per column; t_cg is the solve's alone.  -D with -J, -S, -M, -m, -w or -E is a usage error.
// -B: block CG (lam_hip_solve_block) in place of the plain batch: ONE block Krylov space for the nrhs columns.  The constant columns
// of the plain driver are multiples of one another, which a block refuses (and periodic columns span
// a block Krylov space of a few dimensions on this matrix), so column j is b_j[i] = 1 + (((i * 8 + j) * 2654435761) mod 2^32 >> 28).  The usual
// CSV line per column (num_iters: the first iteration at which the column met the test); one line on STDERR gives the iterations
// run and the breakdown pair.  -B with -J, -S, -M, -m, -D, -w or -E is a usage error.
// -Q nprobes: Lanczos quadrature (lam_hip_lanczos_many + lam_hip_trace_quadrature) in place of a solve: nprobes (1..64) Rademacher
// probes built on the device from seed 0, -i steps of plain Lanczos each (default min(N, 64)), and -S s0,s1,... (up to 64 finite
// shifts; none: the one shift 0) as the shifts of the quadrature -- all of them from the ONE run.  One CSV line per shift:
//     shift,logdet_estimate,logdet_std_error,trinv_estimate,trinv_std_error,steps,seconds
// the estimates of log det(A + s I) and tr (A + s I)^-1 with their standard errors over the probes, the largest number of steps a
// probe ran, and the seconds of the run and its quadratures.  -Q with -J, -w, -M, -m, -T, -k, -e, -E, -D or -B is a usage error.
// Without these flags the calls and the output are those of the driver before them.
// One CSV line per column in the format of the getopt drivers (test_CG_MultiGPUS_HIP_RCCL.cpp; the reference's
// challenge/main/test/test_CG_CPU_MPI_OMP.cpp:196-206 plus the comm-init column, 0 here):
//     rows,procs,threads,t_load,t_comm_init,t_gemv,t_iter,num_iters,rel_err,t_cg
// t_gemv / t_iter / t_cg are the batch's (the columns share every launch); num_iters and rel_err are the column's own.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <vector>

#include <unistd.h>

#include "LAM.hpp"

static int g_packed_many = -2;          // -P: option "packed_many" (-2: no -P, nothing is touched)

// -Y: set the option in front of the solve (sym < 0: no -Y, nothing is touched) ...  (-P travels with it: the same two places)
static bool set_symmetric_many(lam_hip_ctx *ctx, int sym)
{
    if (g_packed_many != -2 && (ctx == nullptr || lam_hip_set_option(ctx, "packed_many", g_packed_many) != 0)) {
        fprintf(stderr, "Failed to set option packed_many = %d\n", g_packed_many);
        return false;
    }
    if (sym < 0) return true;
    if (ctx != nullptr && lam_hip_set_option(ctx, "symmetric_many", sym) == 0) return true;
    fprintf(stderr, "Failed to set option symmetric_many = %d\n", sym);
    return false;
}
// ... and say behind it which product ran
static void report_symmetric_many(lam_hip_ctx *ctx, int sym)
{
    if (g_packed_many != -2 && ctx != nullptr) {
        int64_t eff = 0, k = 0;
        lam_hip_get_option(ctx, "packed_many_effective", &eff);
        lam_hip_get_option(ctx, "multi_rhs_k", &k);
        fprintf(stderr, "packed_many = %d, packed_many_effective = %lld: K = %lld read %s\n", g_packed_many, (long long)eff, (long long)k,
                eff ? "the packed image" : "the matrix");
    }
    if (sym < 0 || ctx == nullptr) return;
    int64_t eff = 0, k = 0;
    lam_hip_get_option(ctx, "symmetric_many_effective", &eff);
    lam_hip_get_option(ctx, "multi_rhs_k", &k);
    fprintf(stderr, "symmetric_many = %d, symmetric_many_effective = %lld: K = %lld ran on the %s batched product%s\n", sym, (long long)eff,
            (long long)k, eff ? "symmetric" : "general", !eff && sym != 0 && k > 4 ? " (the option is not effective for more than 4 columns)" : "");
}

template <typename T>
static int run(size_t rows, int nrhs, int max_iters, double rel_error, bool jacobi, int warm, bool true_res, const std::vector<double> &shifts,
               bool minres, int sym)
{
    using clk = std::chrono::high_resolution_clock;
    LAM::ConjugateGradient_HIP<T> cg(0);
    cg.set_text_output(false);
    const auto t0 = clk::now();
    if (!cg.generate_matrix(rows, rows)) {
        fprintf(stderr, "Failed to generate matrix\n");
        return 1;
    }
    const double t_load = std::chrono::duration<double>(clk::now() - t0).count();
    if (!set_symmetric_many(cg.context(), sym)) return 3;
    std::vector<T> B((size_t)nrhs * rows);
    for (int j = 0; j < nrhs; j++)
        for (size_t i = 0; i < rows; i++) B[(size_t)j * rows + i] = shifts.empty() ? (T)(double)(1u << j) : (T)1;
    if (!shifts.empty() && !minres) cg.set_shifts_many(nrhs, shifts.data());
    std::vector<int32_t> iters(nrhs), conv(nrhs);
    std::vector<double> rel(nrhs);
    const auto t1 = clk::now();
    const int pc = jacobi ? LAM_HIP_PC_JACOBI : LAM_HIP_PC_NONE;
    if (minres) {
        cg.solve_many_minres(nrhs, B.data(), shifts.empty() ? nullptr : shifts.data(), nullptr, max_iters, (T)rel_error, iters.data(),
                             conv.data(), rel.data());
        if (cg.batch_failed()) return 3;
    } else if (warm >= 0) {
        // stage 1 from a zero guess (the plain solve, bit for bit), stage 2 from its solution; 0 iterations is an answer here,
        // so failure is the call's own report
        const std::vector<T> zero((size_t)nrhs * rows, (T)0);
        std::vector<int32_t> first(nrhs);
        cg.solve_many_x0(pc, nrhs, B.data(), zero.data(), nullptr, warm, (T)rel_error, first.data(), conv.data(), rel.data());
        if (cg.batch_failed()) return 3;
        // a column that stopped in stage 1 is born stopped in stage 2 (0 more iterations); one that hit the cap reports W + 1
        for (int j = 0; j < nrhs; j++) first[j] = conv[j] ? first[j] : warm;
        cg.solve_many_x0(pc, nrhs, nullptr, nullptr, nullptr, max_iters - warm, (T)rel_error, iters.data(), conv.data(), rel.data());
        if (cg.batch_failed()) return 3;
        for (int j = 0; j < nrhs; j++) iters[j] += first[j];
    } else {
        if (jacobi) cg.solve_many_pc(pc, nrhs, B.data(), nullptr, max_iters, (T)rel_error, iters.data(), conv.data(), rel.data());
        else cg.solve_many(nrhs, B.data(), nullptr, max_iters, (T)rel_error, iters.data(), conv.data(), rel.data());
        if (cg.batch_failed()) return 3;               // the solve itself failed (reported on stderr)
    }
    const double t_cg = std::chrono::duration<double>(clk::now() - t1).count();
    report_symmetric_many(cg.context(), sym);
    std::vector<double> tres(nrhs);
    if (true_res && !cg.true_residual_many(nrhs, tres.data())) return 3;
    const lam_hip_stats &st = cg.stats();
    for (int j = 0; j < nrhs; j++) {
        std::cout << rows << "," << 1 << "," << 1 << "," << t_load << "," << st.t_comm_init << "," << st.t_gemv << "," << st.t_iter << ","
                  << iters[j] << "," << rel[j] << "," << t_cg;
        if (true_res) std::cout << "," << tres[j];
        if (!shifts.empty()) std::cout << "," << shifts[j];
        std::cout << std::endl;
    }
    return 0;
}

// -M: every shift of -S against the one right-hand side b = 1 by multi-shift CG
template <typename T>
static int run_mshift(size_t rows, int max_iters, double rel_error, bool true_res, const std::vector<double> &shifts, int sym)
{
    using clk = std::chrono::high_resolution_clock;
    const int ns = (int)shifts.size();
    LAM::ConjugateGradient_HIP<T> cg(0);
    cg.set_text_output(false);
    const auto t0 = clk::now();
    if (!cg.generate_matrix(rows, rows)) {
        fprintf(stderr, "Failed to generate matrix\n");
        return 1;
    }
    const double t_load = std::chrono::duration<double>(clk::now() - t0).count();
    if (!set_symmetric_many(cg.context(), sym)) return 3;
    const std::vector<T> b(rows, (T)1);
    std::vector<int32_t> iters(ns), conv(ns);
    std::vector<double> rel(ns), tres(ns);
    const auto t1 = clk::now();
    cg.solve_mshift(ns, shifts.data(), b.data(), nullptr, max_iters, (T)rel_error, iters.data(), conv.data(), rel.data());
    if (cg.batch_failed()) return 3;
    const double t_cg = std::chrono::duration<double>(clk::now() - t1).count();
    report_symmetric_many(cg.context(), sym);
    if (true_res && !cg.true_residual_mshift(ns, tres.data())) return 3;
    const lam_hip_stats &st = cg.stats();
    for (int j = 0; j < ns; j++) {
        std::cout << rows << "," << 1 << "," << 1 << "," << t_load << "," << st.t_comm_init << "," << st.t_gemv << "," << st.t_iter << ","
                  << iters[j] << "," << rel[j] << "," << t_cg;
        if (true_res) std::cout << "," << tres[j];
        std::cout << "," << shifts[j] << std::endl;
    }
    return 0;
}

// -E: nev extreme eigenpairs of the generated matrix by lam_hip_eigs
template <typename T>
static int run_eigs(size_t rows, int nev, int which, int max_steps, double tol, int sym)
{
    using clk = std::chrono::high_resolution_clock;
    LAM::ConjugateGradient_HIP<T> cg(0);
    cg.set_text_output(false);
    const auto t0 = clk::now();
    if (!cg.generate_matrix(rows, rows)) {
        fprintf(stderr, "Failed to generate matrix\n");
        return 1;
    }
    const double t_load = std::chrono::duration<double>(clk::now() - t0).count();
    if (!set_symmetric_many(cg.context(), sym)) return 3;
    std::vector<double> theta(nev), bound(nev), res(nev);
    std::vector<int32_t> conv(nev);
    int32_t found = 0;
    const auto t1 = clk::now();
    cg.eigs(which, nev, max_steps, tol, 8, nullptr, 0, &found, theta.data(), bound.data(), conv.data());
    if (cg.batch_failed()) return 3;
    const double t_cg = std::chrono::duration<double>(clk::now() - t1).count();
    const lam_hip_stats st = cg.stats();
    report_symmetric_many(cg.context(), sym);
    if (found > 0 && !cg.eig_residuals(found, res.data())) return 3;
    std::cout.precision(17);
    for (int i = 0; i < found; i++)
        std::cout << i << "," << theta[i] << "," << bound[i] << "," << res[i] << "," << conv[i] << "," << st.num_iters << "," << t_load << ","
                  << st.t_comm_init << "," << st.t_gemv << "," << st.t_iter << "," << t_cg << std::endl;
    return 0;
}

// -D m: the generated right-hand sides by deflated CG on the m Ritz pairs -W asks lam_hip_eigs for
template <typename T>
static int run_deflated(size_t rows, int nrhs, int m, int which, int max_iters, double rel_error, bool true_res, int sym)
{
    using clk = std::chrono::high_resolution_clock;
    LAM::ConjugateGradient_HIP<T> cg(0);
    cg.set_text_output(false);
    const auto t0 = clk::now();
    if (!cg.generate_matrix(rows, rows)) {
        fprintf(stderr, "Failed to generate matrix\n");
        return 1;
    }
    const double t_load = std::chrono::duration<double>(clk::now() - t0).count();
    if (!set_symmetric_many(cg.context(), sym)) return 3;
    // the space: lam_hip_eigs' own defaults (min(N, 256) steps, the binding's tolerances); pairs that did not converge still span a
    // legal space, so only a run that found fewer than m pairs is a failure
    const int max_steps = (int)(rows < (size_t)LAM_HIP_MAX_LANCZOS ? rows : (size_t)LAM_HIP_MAX_LANCZOS);
    std::vector<double> theta(m);
    int32_t found = 0;
    const bool all = cg.eigs(which, m, max_steps, sizeof(T) == 8 ? 1e-10 : 1e-5, 8, nullptr, 0, &found, theta.data());
    if (cg.batch_failed()) return 3;
    if (found < m) {
        fprintf(stderr, "lam_hip_eigs found %d of the %d pairs -D asks for\n", (int)found, m);
        return 3;
    }
    if (!all) fprintf(stderr, "lam_hip_eigs: not every one of the %d pairs converged in %d steps; deflating with the Ritz vectors as they are\n", m, max_steps);
    if (!cg.set_deflation_from_eigs(m)) return 3;
    std::vector<T> B((size_t)nrhs * rows);
    for (int j = 0; j < nrhs; j++)
        for (size_t i = 0; i < rows; i++) B[(size_t)j * rows + i] = (T)(double)(1u << j);
    std::vector<int32_t> iters(nrhs), conv(nrhs);
    std::vector<double> rel(nrhs), tres(nrhs);
    const auto t1 = clk::now();
    cg.solve_many_deflated(nrhs, B.data(), nullptr, max_iters, (T)rel_error, iters.data(), conv.data(), rel.data());
    if (cg.batch_failed()) return 3;
    const double t_cg = std::chrono::duration<double>(clk::now() - t1).count();
    report_symmetric_many(cg.context(), sym);
    if (true_res && !cg.true_residual_many(nrhs, tres.data())) return 3;
    const lam_hip_stats &st = cg.stats();
    for (int j = 0; j < nrhs; j++) {
        std::cout << rows << "," << 1 << "," << 1 << "," << t_load << "," << st.t_comm_init << "," << st.t_gemv << "," << st.t_iter << ","
                  << iters[j] << "," << rel[j] << "," << t_cg;
        if (true_res) std::cout << "," << tres[j];
        std::cout << std::endl;
    }
    return 0;
}

// -B: the nrhs columns by block CG
template <typename T>
static int run_block(size_t rows, int nrhs, int max_iters, double rel_error, bool true_res, int sym)
{
    using clk = std::chrono::high_resolution_clock;
    LAM::ConjugateGradient_HIP<T> cg(0);
    cg.set_text_output(false);
    const auto t0 = clk::now();
    if (!cg.generate_matrix(rows, rows)) {
        fprintf(stderr, "Failed to generate matrix\n");
        return 1;
    }
    const double t_load = std::chrono::duration<double>(clk::now() - t0).count();
    if (!set_symmetric_many(cg.context(), sym)) return 3;
    std::vector<T> B((size_t)nrhs * rows);
    for (int j = 0; j < nrhs; j++)
        for (size_t i = 0; i < rows; i++) B[(size_t)j * rows + i] = (T)(double)(1u + ((uint32_t)((i * 8 + (size_t)j) * 2654435761ull) >> 28));
    std::vector<int32_t> iters(nrhs), conv(nrhs);
    std::vector<double> rel(nrhs), tres(nrhs);
    int32_t bd[2] = {0, 0};
    const auto t1 = clk::now();
    cg.solve_block(nrhs, B.data(), nullptr, max_iters, (T)rel_error, iters.data(), conv.data(), rel.data(), bd);
    if (cg.batch_failed()) return 3;
    const double t_cg = std::chrono::duration<double>(clk::now() - t1).count();
    report_symmetric_many(cg.context(), sym);
    if (true_res && !cg.true_residual_many(nrhs, tres.data())) return 3;
    const lam_hip_stats &st = cg.stats();
    fprintf(stderr, "block CG: %d iterations, breakdown = (%d, %d)\n", (int)st.num_iters, (int)bd[0], (int)bd[1]);
    for (int j = 0; j < nrhs; j++) {
        std::cout << rows << "," << 1 << "," << 1 << "," << t_load << "," << st.t_comm_init << "," << st.t_gemv << "," << st.t_iter << ","
                  << iters[j] << "," << rel[j] << "," << t_cg;
        if (true_res) std::cout << "," << tres[j];
        std::cout << std::endl;
    }
    return 0;
}

// -Q: log det(A + s I) and tr (A + s I)^-1 of the generated matrix for every shift, from one run of nprobes Rademacher probes
template <typename T>
static int run_quadrature(size_t rows, int nprobes, int steps, const std::vector<double> &shifts, int sym)
{
    using clk = std::chrono::high_resolution_clock;
    LAM::ConjugateGradient_HIP<T> cg(0);
    cg.set_text_output(false);
    if (!cg.generate_matrix(rows, rows)) {
        fprintf(stderr, "Failed to generate matrix\n");
        return 1;
    }
    if (!set_symmetric_many(cg.context(), sym)) return 3;
    const int ns = shifts.empty() ? 1 : (int)shifts.size();
    const double *sigma = shifts.empty() ? nullptr : shifts.data();
    std::vector<double> ld(ns), ld_se(ns), ti(ns), ti_se(ns);
    const auto t1 = clk::now();
    cg.lanczos_many(nprobes, nullptr, 0, steps);
    if (cg.batch_failed()) return 3;
    const lam_hip_stats st = cg.stats();
    report_symmetric_many(cg.context(), sym);
    if (!cg.trace_quadrature(LAM_HIP_QUAD_LOG, 0.0, ns, sigma, ld.data(), ld_se.data())) return 3;
    if (!cg.trace_quadrature(LAM_HIP_QUAD_INV, 0.0, ns, sigma, ti.data(), ti_se.data())) return 3;
    const double t_q = std::chrono::duration<double>(clk::now() - t1).count();
    std::cout.precision(17);
    for (int j = 0; j < ns; j++)
        std::cout << (sigma ? sigma[j] : 0.0) << "," << ld[j] << "," << ld_se[j] << "," << ti[j] << "," << ti_se[j] << "," << st.num_iters << ","
                  << t_q << std::endl;
    return 0;
}

// "s0,s1,...": 1..LAM_HIP_MAX_SHIFTS numbers (main holds a list without -M to LAM_HIP_MAX_RHS), each finite, nothing else; *negative:
// one of them is < 0, which main accepts under -m only (it decides once every option is parsed)
static bool parse_shifts(const char *arg, std::vector<double> *out, bool *negative)
{
    out->clear();
    *negative = false;
    const char *p = arg;
    for (;;) {
        char *end = nullptr;
        const double v = strtod(p, &end);
        if (end == p || !std::isfinite(v) || out->size() == (size_t)LAM_HIP_MAX_SHIFTS) return false;
        if (v < 0.0) *negative = true;
        out->push_back(v);
        if (*end == '\0') return true;
        if (*end != ',') return false;
        p = end + 1;
    }
}

int main(int argc, char **argv)
{
    size_t rows = 0;
    int nrhs = 1, max_iters = 1000, opt;
    int nev = 0, which = LAM_HIP_EIG_SMALLEST;      // nev == 0: no -E
    int defl = 0;                                    // 0: no -D
    bool d_given = false;
    bool block = false;                              // -B
    int nprobes = 0;                                 // -Q
    bool q_given = false, e_given = false;
    bool bad_eigs = false, i_given = false, s_given = false;
    double rel_error = 1e-9;
    const char *precision = "f64";
    bool jacobi = false, true_res = false, mshift = false, minres = false, negative = false;
    int warm = -1;                  // -1: no -w
    int sym = -1;                   // -1: no -Y
    bool bad_sym = false, bad_packed = false;
    bool bad_warm = false, bad_shifts = false, k_given = false;
    std::vector<double> shifts;
    while ((opt = getopt(argc, argv, "s:k:i:e:t:Jw:TS:MmY:P:E:W:D:BQ:h")) != -1) {
        switch (opt) {
        case 's': rows = (size_t)atoll(optarg); break;
        case 'k': nrhs = atoi(optarg); k_given = true; break;
        case 'i': max_iters = atoi(optarg); i_given = true; break;
        case 'e': rel_error = atof(optarg); e_given = true; break;
        case 't': precision = optarg; break;
        case 'J': jacobi = true; break;
        case 'w': warm = atoi(optarg); bad_warm = warm < 0; break;
        case 'T': true_res = true; break;
        case 'S': bad_shifts = !parse_shifts(optarg, &shifts, &negative); s_given = true; break;
        case 'M': mshift = true; break;
        case 'm': minres = true; break;
        case 'E': nev = atoi(optarg); bad_eigs = bad_eigs || nev < 1; break;
        case 'D': defl = atoi(optarg); d_given = true; break;
        case 'B': block = true; break;
        case 'Q': nprobes = atoi(optarg); q_given = true; break;
        case 'W':
            if (!strcmp(optarg, "s")) which = LAM_HIP_EIG_SMALLEST;
            else if (!strcmp(optarg, "l")) which = LAM_HIP_EIG_LARGEST;
            else if (!strcmp(optarg, "b")) which = LAM_HIP_EIG_BOTH;
            else bad_eigs = true;
            break;
        case 'Y': bad_sym = strlen(optarg) != 1 || optarg[0] < '0' || optarg[0] > '2'; sym = optarg[0] - '0'; break;
        case 'P': bad_packed = strlen(optarg) != 1 || optarg[0] < '0' || optarg[0] > '1'; g_packed_many = optarg[0] - '0'; break;
        default:
            fprintf(stderr, "Usage: %s -s N -k nrhs -i max_iters [-e rel_error] [-t f64|f32] [-J (Jacobi preconditioner)] [-w W (two stages)] "
                    "[-T (true residuals)] [-S s0,s1,... (1..%d shifts >= 0: column j solves (A + s_j I) x = b; sets nrhs)] "
                    "[-M (with -S, up to %d shifts: multi-shift CG on one right-hand side; not with -J, -w)] "
                    "[-m (MINRES in place of CG: -S then takes finite shifts of either sign; not with -J, -w, -M)] "
                    "[-Y 0|1|2 (option symmetric_many: the batched product of up to 4 columns reads every pair of the matrix once)] "
                    "[-P 0|1 (option packed_many: the general batched product of up to 4 fp64 columns reads the 7-byte image of the matrix)] "
                    "[-E nev (Lanczos eigensolver lam_hip_eigs in place of a solve: nev extreme eigenpairs; -W s|l|b smallest / largest / both, "
                    "-i max_steps up to %d, -e tol; not with -J, -w, -S, -M, -m, -k)] "
                    "[-D m (deflated CG on m = 1..%d Ritz pairs of lam_hip_eigs, -W s|l|b; not with -J, -w, -S, -M, -m, -E)] "
                    "[-B (block CG lam_hip_solve_block: one block Krylov space for the nrhs columns; not with -J, -w, -S, -M, -m, -D, -E)] "
                    "[-Q nprobes (Lanczos quadrature lam_hip_lanczos_many in place of a solve: log det(A + s I) and tr (A + s I)^-1 for the "
                    "shifts of -S from 1..%d Rademacher probes, -i steps each; not with -J, -w, -M, -m, -T, -k, -e, -E, -D, -B)]\n", argv[0],
                    LAM_HIP_MAX_RHS, LAM_HIP_MAX_SHIFTS, LAM_HIP_MAX_LANCZOS, LAM_HIP_MAX_DEFLATION, LAM_HIP_MAX_PROBES);
            return opt == 'h' ? 0 : 1;
        }
    }
    if (bad_sym) {
        fprintf(stderr, "Usage: -Y takes 0 (the general batched product), 1 (the symmetric one where it pays) or 2 (always, up to 4 columns)\n");
        return 1;
    }
    if (bad_packed) {
        fprintf(stderr, "Usage: -P takes 0 (the batched product reads the matrix) or 1 (the packed image, up to 4 fp64 columns)\n");
        return 1;
    }
    if (q_given) {
        if (jacobi || warm >= 0 || bad_warm || mshift || minres || true_res || k_given || e_given || nev != 0 || bad_eigs || d_given || block) {
            fprintf(stderr, "Usage: -Q takes neither -J, -w, -M, -m, -T, -k, -e, -E, -D nor -B: the quadrature runs on the matrix alone, -i are "
                    "its steps and -S its shifts\n");
            return 1;
        }
        if (!i_given) max_iters = (int)(rows < 64 ? rows : 64);
        if (rows == 0 || nprobes < 1 || nprobes > LAM_HIP_MAX_PROBES || max_iters < 1 || bad_shifts) {
            fprintf(stderr, "Usage: %s -s N -Q nprobes (1..%d) [-i steps (1..min(N, %d))] [-S s0,s1,... (up to %d finite shifts)] [-t f64|f32] "
                    "[-Y 0|1|2]\n", argv[0], LAM_HIP_MAX_PROBES, LAM_HIP_MAX_LANCZOS, LAM_HIP_MAX_SHIFTS);
            return 1;
        }
        if (!strcmp(precision, "f64")) return run_quadrature<double>(rows, nprobes, max_iters, shifts, sym);
        if (!strcmp(precision, "f32")) return run_quadrature<float>(rows, nprobes, max_iters, shifts, sym);
        fprintf(stderr, "Unknown precision '%s' (f64, f32)\n", precision);
        return 1;
    }
    if (block) {
        if (jacobi || warm >= 0 || bad_warm || s_given || mshift || minres || d_given || nev != 0 || bad_eigs) {
            fprintf(stderr, "Usage: -B takes neither -J, -S, -M, -m, -D, -w nor -E: block CG has no preconditioner, no shifts, no deflation "
                    "space and no guess\n");
            return 1;
        }
        if (rows == 0 || nrhs < 1 || nrhs > LAM_HIP_MAX_RHS || max_iters < 0) {
            fprintf(stderr, "Usage: %s -s N -k nrhs (1..%d) -i max_iters -B [-e rel_error] [-t f64|f32] [-T] [-Y 0|1|2]\n", argv[0], LAM_HIP_MAX_RHS);
            return 1;
        }
        if (!strcmp(precision, "f64")) return run_block<double>(rows, nrhs, max_iters, rel_error, true_res, sym);
        if (!strcmp(precision, "f32")) return run_block<float>(rows, nrhs, max_iters, rel_error, true_res, sym);
        fprintf(stderr, "Unknown precision '%s' (f64, f32)\n", precision);
        return 1;
    }
    if (d_given) {
        if (defl < 1 || defl > LAM_HIP_MAX_DEFLATION || bad_eigs || nev != 0 || jacobi || warm >= 0 || bad_warm || s_given || mshift || minres) {
            fprintf(stderr, "Usage: -D m (1..%d) [-W s|l|b] takes neither -J, -w, -S, -M, -m nor -E: deflated CG has no preconditioner, no "
                    "guess and no shifts\n", LAM_HIP_MAX_DEFLATION);
            return 1;
        }
        if (rows == 0 || nrhs < 1 || nrhs > LAM_HIP_MAX_RHS || max_iters < 0) {
            fprintf(stderr, "Usage: %s -s N -k nrhs (1..%d) -i max_iters -D m [-W s|l|b] [-e rel_error] [-t f64|f32] [-T] [-Y 0|1|2]\n", argv[0],
                    LAM_HIP_MAX_RHS);
            return 1;
        }
        if (!strcmp(precision, "f64")) return run_deflated<double>(rows, nrhs, defl, which, max_iters, rel_error, true_res, sym);
        if (!strcmp(precision, "f32")) return run_deflated<float>(rows, nrhs, defl, which, max_iters, rel_error, true_res, sym);
        fprintf(stderr, "Unknown precision '%s' (f64, f32)\n", precision);
        return 1;
    }
    if (nev != 0 || bad_eigs) {
        if (bad_eigs || jacobi || warm >= 0 || bad_warm || s_given || mshift || minres || k_given) {
            fprintf(stderr, "Usage: -E nev (>= 1) [-W s|l|b] takes neither -J, -w, -S, -M, -m nor -k: the eigensolver runs on the matrix alone\n");
            return 1;
        }
        if (!i_given) max_iters = (int)(rows < (size_t)LAM_HIP_MAX_LANCZOS ? rows : (size_t)LAM_HIP_MAX_LANCZOS);
        if (rows == 0) {
            fprintf(stderr, "Usage: %s -s N -E nev [-W s|l|b] [-i max_steps] [-e tol] [-t f64|f32] [-Y 0|1|2]\n", argv[0]);
            return 1;
        }
        if (!strcmp(precision, "f64")) return run_eigs<double>(rows, nev, which, max_iters, rel_error, sym);
        if (!strcmp(precision, "f32")) return run_eigs<float>(rows, nev, which, max_iters, rel_error, sym);
        fprintf(stderr, "Unknown precision '%s' (f64, f32)\n", precision);
        return 1;
    }
    if (minres && (jacobi || warm >= 0 || bad_warm || mshift)) {
        fprintf(stderr, "Usage: -m takes neither -J, -w nor -M: MINRES has no preconditioner, starts from x = 0 and is not multi-shift\n");
        return 1;
    }
    if (negative && !minres) bad_shifts = true;      // a negative shift is MINRES' alone
    if (mshift && (shifts.empty() || bad_shifts || jacobi || warm >= 0 || bad_warm || k_given)) {
        fprintf(stderr, "Usage: -M needs -S s0,s1,... (1..%d finite shifts >= 0) and takes neither -J, -w nor -k: multi-shift CG has one "
                "right-hand side, no preconditioner and no guess\n", LAM_HIP_MAX_SHIFTS);
        return 1;
    }
    if (!mshift && shifts.size() > (size_t)LAM_HIP_MAX_RHS) bad_shifts = true;
    if (minres && (bad_shifts || (!shifts.empty() && k_given && nrhs != (int)shifts.size()))) {
        fprintf(stderr, "-S takes 1..%d comma-separated finite shifts (of either sign under -m), and -k, if given, their number\n", LAM_HIP_MAX_RHS);
        return 1;
    }
    if (bad_shifts || (!shifts.empty() && k_given && nrhs != (int)shifts.size())) {
        fprintf(stderr, "-S takes 1..%d comma-separated finite shifts >= 0, and -k, if given, their number\n", LAM_HIP_MAX_RHS);
        return 1;
    }
    if (mshift) {
        if (rows == 0 || max_iters < 0) {
            fprintf(stderr, "Usage: %s -s N -i max_iters [-e rel_error] [-t f64|f32] [-T] -S s0,s1,... -M\n", argv[0]);
            return 1;
        }
        if (!strcmp(precision, "f64")) return run_mshift<double>(rows, max_iters, rel_error, true_res, shifts, sym);
        if (!strcmp(precision, "f32")) return run_mshift<float>(rows, max_iters, rel_error, true_res, shifts, sym);
        fprintf(stderr, "Unknown precision '%s' (f64, f32)\n", precision);
        return 1;
    }
    if (!shifts.empty()) nrhs = (int)shifts.size();
    if (rows == 0 || nrhs < 1 || nrhs > LAM_HIP_MAX_RHS || max_iters < 0 || bad_warm || warm > max_iters) {
        fprintf(stderr, "Usage: %s -s N -k nrhs (1..%d) -i max_iters [-e rel_error] [-t f64|f32] [-J (Jacobi preconditioner)] [-w W (0..max_iters)] [-T] [-S s0,s1,...]\n",
                argv[0], LAM_HIP_MAX_RHS);
        return 1;
    }
    if (!strcmp(precision, "f64")) return run<double>(rows, nrhs, max_iters, rel_error, jacobi, warm, true_res, shifts, minres, sym);
    if (!strcmp(precision, "f32")) return run<float>(rows, nrhs, max_iters, rel_error, jacobi, warm, true_res, shifts, minres, sym);
    fprintf(stderr, "Unknown precision '%s' (f64, f32)\n", precision);
    return 1;
}
