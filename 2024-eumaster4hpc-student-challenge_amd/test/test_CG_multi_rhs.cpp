// Generate-mode driver of the multi-right-hand-side solve (lam_hip_solve_many): dense tridiag(1,2,1) of -s N rows, -k nrhs
// right-hand sides, column j constant 2^j, solved together with one pass over the matrix per iteration.
//     test_CG_multi_rhs.out -s N -k nrhs -i max_iters [-e rel_error] [-t f64|f32] [-J]
// -J: Jacobi-preconditioned recurrences (lam_hip_solve_many_pc; off by default).  tridiag(1,2,1) has a constant diagonal, so the
// iteration and residual columns are the plain ones digit for digit: the flag exercises the path, it does not save iterations here.
// One CSV line per column in the format of the getopt drivers (test_CG_MultiGPUS_HIP_RCCL.cpp; the reference's
// challenge/main/test/test_CG_CPU_MPI_OMP.cpp:196-206 plus the comm-init column, 0 here):
//     rows,procs,threads,t_load,t_comm_init,t_gemv,t_iter,num_iters,rel_err,t_cg
// t_gemv / t_iter / t_cg are the batch's (the columns share every launch); num_iters and rel_err are the column's own.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <vector>

#include <unistd.h>

#include "LAM.hpp"

template <typename T>
static int run(size_t rows, int nrhs, int max_iters, double rel_error, bool jacobi)
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
    std::vector<T> B((size_t)nrhs * rows);
    for (int j = 0; j < nrhs; j++)
        for (size_t i = 0; i < rows; i++) B[(size_t)j * rows + i] = (T)(double)(1u << j);
    std::vector<int32_t> iters(nrhs), conv(nrhs);
    std::vector<double> rel(nrhs);
    const auto t1 = clk::now();
    if (jacobi) cg.solve_many_pc(LAM_HIP_PC_JACOBI, nrhs, B.data(), nullptr, max_iters, (T)rel_error, iters.data(), conv.data(), rel.data());
    else cg.solve_many(nrhs, B.data(), nullptr, max_iters, (T)rel_error, iters.data(), conv.data(), rel.data());
    const double t_cg = std::chrono::duration<double>(clk::now() - t1).count();
    if (cg.stats().num_iters == 0) return 3;       // the solve itself failed (reported on stderr)
    const lam_hip_stats &st = cg.stats();
    for (int j = 0; j < nrhs; j++)
        std::cout << rows << "," << 1 << "," << 1 << "," << t_load << "," << st.t_comm_init << "," << st.t_gemv << "," << st.t_iter << ","
                  << iters[j] << "," << rel[j] << "," << t_cg << std::endl;
    return 0;
}

int main(int argc, char **argv)
{
    size_t rows = 0;
    int nrhs = 1, max_iters = 1000, opt;
    double rel_error = 1e-9;
    const char *precision = "f64";
    bool jacobi = false;
    while ((opt = getopt(argc, argv, "s:k:i:e:t:Jh")) != -1) {
        switch (opt) {
        case 's': rows = (size_t)atoll(optarg); break;
        case 'k': nrhs = atoi(optarg); break;
        case 'i': max_iters = atoi(optarg); break;
        case 'e': rel_error = atof(optarg); break;
        case 't': precision = optarg; break;
        case 'J': jacobi = true; break;
        default:
            fprintf(stderr, "Usage: %s -s N -k nrhs -i max_iters [-e rel_error] [-t f64|f32] [-J (Jacobi preconditioner)]\n", argv[0]);
            return opt == 'h' ? 0 : 1;
        }
    }
    if (rows == 0 || nrhs < 1 || nrhs > LAM_HIP_MAX_RHS || max_iters < 0) {
        fprintf(stderr, "Usage: %s -s N -k nrhs (1..%d) -i max_iters [-e rel_error] [-t f64|f32] [-J (Jacobi preconditioner)]\n", argv[0],
                LAM_HIP_MAX_RHS);
        return 1;
    }
    if (!strcmp(precision, "f64")) return run<double>(rows, nrhs, max_iters, rel_error, jacobi);
    if (!strcmp(precision, "f32")) return run<float>(rows, nrhs, max_iters, rel_error, jacobi);
    fprintf(stderr, "Unknown precision '%s' (f64, f32)\n", precision);
    return 1;
}
