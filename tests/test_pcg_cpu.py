"""CPU-side checks of the Jacobi-preconditioned batched solve (include/lam_hip.h, lam_hip_solve_many_pc / lam_hip_get_diagonal): the
numpy restatement of the recurrence (tests/pcg_reference.py) against the CPU oracle and on the badly scaled systems it is for,
the header as C99, the exports, the ABI history, and the driver's argument handling."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import pcg_reference as R
from conftest import GOLDEN, ROOT, PKG_NAME

NEW = ("lam_hip_solve_many_pc", "lam_hip_get_diagonal")
HEADER = os.path.join(ROOT, "include", "lam_hip.h")


def test_reference_without_preconditioner_is_the_oracle_recurrence(oracle):
    """dinv = 1: the suite's gates against the oracle on a golden system (iterations max(3, 2 %), x to 1e-9)."""
    A = oracle.read_bin(os.path.join(GOLDEN, "spd_n256_s3.matrix.bin"), np.float64)
    n = A.shape[0]
    for seed in (1, 2):
        b = np.random.default_rng(seed).uniform(-1, 1, n)
        x_or, st_or = oracle.cg_solve(A, b, 10000, 1e-9)
        x, st = R.pcg(A, b, 10000, 1e-9, None)
        x1, st1 = R.pcg(A, b, 10000, 1e-9, np.ones(n))
        assert st_or["converged"] and st["converged"]
        assert abs(st["num_iters"] - st_or["num_iters"]) <= max(3, 0.02 * st_or["num_iters"]), (st, st_or)
        assert np.linalg.norm(x - x_or) / np.linalg.norm(x_or) <= 1e-9
        assert st1 == st and np.array_equal(x, x1)
    # the cap and the degenerate column, as lam_hip_solve counts them
    _, st = R.pcg(A, b, 3, 1e-30, R.jacobi_dinv(A))
    assert st["num_iters"] == 4 and not st["converged"]
    x, st = R.pcg(A, np.zeros(n), 5, 1e-9, R.jacobi_dinv(A))
    assert st["num_iters"] == 6 and not st["converged"] and np.isnan(st["rel_err"]) and np.isnan(x).all()


def test_plain_cg_stalls_on_scaled_systems_where_jacobi_converges():
    """A = S M S, n = 512, fp64, tolerance 1e-10, cap 4 n: plain CG does not get there, the preconditioned recurrence does."""
    n = 512
    A, rng = R.sms_system(n)
    assert np.array_equal(A, A.T)
    X = rng.uniform(-1, 1, (2, n))
    B = X @ A.T
    dinv = R.jacobi_dinv(A)
    for j in range(2):
        x0, st0 = R.pcg(A, B[j], 4 * n, 1e-10, None)
        x1, st1 = R.pcg(A, B[j], 4 * n, 1e-10, dinv)
        print(f"column {j}: plain {st0}, true residual {R.true_residual(A, x0, B[j]):.3e}; jacobi {st1}, "
              f"true residual {R.true_residual(A, x1, B[j]):.3e}")
        assert not st0["converged"] and st0["num_iters"] == 4 * n + 1 and R.true_residual(A, x0, B[j]) > 1e-8
        assert st1["converged"] and st1["num_iters"] < n // 4 and R.true_residual(A, x1, B[j]) <= 2e-10


def test_header_compiles_as_c99_with_the_new_names(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "lam_hip.h"\n'
                   "#if LAM_HIP_PC_NONE != 0 || LAM_HIP_PC_JACOBI != 1\n#error LAM_HIP_PC\n#endif\n"
                   "int use(lam_hip_ctx *c, double *d)\n{\n"
                   "    int32_t it[LAM_HIP_MAX_RHS], cv[LAM_HIP_MAX_RHS];\n    double re[LAM_HIP_MAX_RHS];\n    lam_hip_stats st;\n"
                   "    return lam_hip_solve_many_pc(c, LAM_HIP_PC_JACOBI, 10, 1e-9, &st, it, cv, re) + lam_hip_get_diagonal(c, d);\n}\n")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                        "-o", str(tmp_path / "use.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_library_exports_the_new_entry_points(lam):
    lam.build()
    L = C.CDLL(lam.lib_path())
    for name in NEW:
        assert hasattr(L, name), name
    assert set(NEW) <= set(lam.lib()._lam_symbols)
    assert (lam.PC_NONE, lam.PC_JACOBI) == (0, 1)


def test_abi_version_stays_4_and_the_history_names_the_additions(lam):
    txt = open(HEADER).read()
    assert re.search(r"#define LAM_HIP_ABI_VERSION 4\b", txt) and lam.lib().lam_hip_abi_version() == 4
    history = txt[txt.index("ABI history"):txt.index("#define LAM_HIP_ABI_VERSION")]
    for name in NEW + ("LAM_HIP_PC_NONE", "LAM_HIP_PC_JACOBI"):
        assert name in history, name
    assert re.search(r"#define LAM_HIP_PC_NONE +0\b", txt) and re.search(r"#define LAM_HIP_PC_JACOBI +1\b", txt)


def test_driver_lists_the_flag_and_refuses_bad_arguments_before_touching_a_gpu(lam):
    lam.build()
    exe = os.path.join(ROOT, PKG_NAME, "test", "test_CG_multi_rhs.out")
    r = subprocess.run([exe, "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "-J" in r.stderr
    for args in (["-J", "-s", "16", "-k", "9", "-i", "3"], ["-J", "-k", "2", "-i", "3"], ["-J", "-s", "16", "-k", "2", "-i", "-1"],
                 ["-J", "-s", "16", "-k", "2", "-i", "3", "-t", "f16"], ["-s", "16", "-k", "2", "-i", "3", "-Q"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and ("Usage" in r.stderr or "Unknown precision" in r.stderr), (args, r.stderr)


def test_host_asan_still_builds_against_its_fake_of_the_abi():
    """solve_many_pc is a sibling member of solve_many in a class template: instantiated only where called, so the sanitized host
    build, whose fake ABI has neither entry point, links as before."""
    here = os.path.join(ROOT, "tests", "host_asan")
    r = subprocess.run(["make", "-C", here, "all"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "lam_hip_solve_many_pc" not in open(os.path.join(here, "fake_lam_hip.cpp")).read()
