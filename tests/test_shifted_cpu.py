"""CPU-side checks of lam_hip_set_shifts_many (include/lam_hip.h, "shifted systems"): the header, the library and the binding carry
it, the ABI version did not move, the driver lists -S and refuses bad lists before anything touches a GPU, and the host side of
tests/test_gpu_shifted.py (tests/shifted_data.py): the references run on A + s I formed on the host state the problem the device
solves, and the oracle is a tenth of the gate sure of every tracked column."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import exact_data as E
import pcg_reference as R
import shifted_data as S
from conftest import ROOT, PKG_NAME
from tracking_data import FP32_TRACKING_GATE, ITERATION_TRACKING_GATES, TRACKED_K

HEADER = os.path.join(ROOT, "include", "lam_hip.h")
EXE = os.path.join(ROOT, PKG_NAME, "test", "test_CG_multi_rhs.out")


def test_header_compiles_as_c99_with_the_new_entry_point(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "lam_hip.h"\n'
                   "int use(lam_hip_ctx *c, const double *sigma)\n{\n"
                   "    return lam_hip_set_shifts_many(c, 3, sigma) + lam_hip_set_shifts_many(c, 3, 0);\n}\n")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                        "-o", str(tmp_path / "use.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_library_and_binding_carry_the_entry_point_and_the_abi_version_stays_4(lam):
    lam.build()
    assert hasattr(C.CDLL(lam.lib_path()), "lam_hip_set_shifts_many")
    assert "lam_hip_set_shifts_many" in lam.lib()._lam_symbols
    assert callable(lam.Solver.set_shifts) and callable(lam.Solver.solve_shifted)
    txt = open(HEADER).read()
    assert re.search(r"#define LAM_HIP_ABI_VERSION 4\b", txt) and lam.lib().lam_hip_abi_version() == 4
    assert "lam_hip_set_shifts_many" in txt[txt.index("ABI history"):txt.index("#define LAM_HIP_ABI_VERSION")]


def test_driver_lists_the_flag_and_refuses_bad_lists_before_touching_a_gpu(lam):
    lam.build()
    r = subprocess.run([EXE, "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "-S s0,s1,..." in r.stderr, r.stderr
    for bad in ("-1", "1,,2", "1,2,", ",1", "abc", "nan", "inf", "1e999", "1,2,3,4,5,6,7,8,9", "", "1;2", "0.5,-0.5"):
        r = subprocess.run([EXE, "-s", "16", "-i", "3", "-S", bad], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "-S takes" in r.stderr and not r.stdout, (bad, r.returncode, r.stdout, r.stderr)
    r = subprocess.run([EXE, "-s", "16", "-i", "3", "-k", "2", "-S", "1,2,3"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "-S takes" in r.stderr and not r.stdout, (r.returncode, r.stdout, r.stderr)


def test_host_asan_still_builds_with_set_shifts_many_in_the_class():
    here = os.path.join(ROOT, "tests", "host_asan")
    r = subprocess.run(["make", "-C", here, "all"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "lam_hip_set_shifts_many" not in open(os.path.join(here, "fake_lam_hip.cpp")).read()
    hpp = open(os.path.join(ROOT, PKG_NAME, "LAM", "src", "HIP", "ConjugateGradient_HIP_base.hpp")).read()
    assert "void set_shifts_many(int nrhs, const double *sigma)" in hpp


def test_the_restatement_with_the_shift_apart_reproduces_the_reference_on_the_formed_matrix():
    """pcg_shifted (A p + s p, dinv from A_ii + s) against pcg_reference.pcg on A + s I formed on the host, every tracked column and
    k, plain and Jacobi: the two differ by the rounding of A_ii + s and of the one more addition per row only, and stay inside a TENTH
    of the gates the GPU test applies (fp64: ITERATION_TRACKING_GATES; fp32: FP32_TRACKING_GATE up to k = 20, where that reference
    still agrees with itself).  The gates are the plain recurrence's on this system; Jacobi is held to them up to k = 20 only: at
    k = 40 the column with the largest shift has converged to 1e-11 of b, and rel_err there is itself only known to 1e-5 or so
    relative to its size (fp64 roundoff over that residual)."""
    A, B, sh = S.shifted_tracking_columns()
    for dt in (np.float64, np.float32):
        for k in TRACKED_K:
            if dt is np.float32 and k > 20:
                continue
            if dt is np.float64:
                g_re, g_x = [(g1, g2) for kk, g1, g2 in ITERATION_TRACKING_GATES if kk == k][0]
            else:
                g_re = g_x = FP32_TRACKING_GATE[k]
            for jac in (False, True):
                if jac and k > 20:
                    continue
                for j in range(8):
                    M = S.formed(A, sh[j], dt)
                    x1, s1 = R.pcg(M, B[j], k, 1e-30, R.jacobi_dinv(M, dt) if jac else None, dt)
                    x2, s2 = S.pcg_shifted(A, sh[j], B[j], k, 1e-30, jac, dt)
                    d_re = abs(s2["rel_err"] / s1["rel_err"] - 1)
                    d_x = np.linalg.norm(x2.astype(np.float64) - x1) / np.linalg.norm(x1.astype(np.float64))
                    assert s1["num_iters"] == s2["num_iters"] == k + 1
                    assert d_re <= 0.1 * g_re and d_x <= 0.1 * g_x, (dt, k, jac, j, d_re, d_x, g_re, g_x)
    # and the shifted dinv is the formed matrix's Jacobi dinv wherever A_ii + s is exact in the vector dtype
    assert np.array_equal(S.shifted_dinv(np.diag([1.0, 3.0, 7.0, 0.0]), 1.0, np.float32), np.float32([1 / 2, 1 / 4, 1 / 8, 1.0]))


def test_the_oracle_is_a_tenth_of_the_gate_sure_of_every_shifted_column(oracle):
    """tests/test_multi_rhs_cpu.py's check on the shifted systems: the oracle at 1 thread against 4 / 8 threads and 3 emulated ranks
    on (A + s_j I, b_j), every tracked k.  The columns were assigned (tests/shifted_data.py) to stay at or below 0.3 of this limit."""
    A, B, sh = S.shifted_tracking_columns()
    assert len(set(sh)) == 8 and sh[0] == 0 and all(np.float32(v) == v for v in sh)
    for k, gate_res, gate_x in ITERATION_TRACKING_GATES:
        if k not in TRACKED_K:
            continue
        for j in range(8):
            M = S.formed(A, sh[j])
            x1, s1 = oracle.cg_solve(M, B[j], k, 1e-30, threads=1)
            for kw in (dict(threads=4), dict(threads=8), dict(threads=1, P=3)):
                x2, s2 = oracle.cg_solve(M, B[j], k, 1e-30, **kw)
                assert abs(s2["rel_err"] / s1["rel_err"] - 1) <= 0.1 * gate_res, (k, j, kw)
                assert np.linalg.norm(x2 - x1) / np.linalg.norm(x1) <= 0.1 * gate_x, (k, j, kw)


def test_integer_shifts_keep_the_exact_tests_inside_exact_data_s_bounds():
    """The inputs of tests/test_gpu_shifted.py's exact tests, on the host: p.Ap of the first steps is not zero, every quantity is an
    integer inside fp32's 2^24, and the patched diagonal d - 1 has zeros."""
    INT_SHIFTS = S.INT_SHIFTS
    assert len(set(INT_SHIFTS)) == 8 and {0, 1, 2, 4, 8} <= set(INT_SHIFTS) and max(INT_SHIFTS) <= 8
    for n in (1, 5, 64, 513, 1030, 4097):
        B = [E.int_vec(n, 51 * n + j) for j in range(8)]
        for v in B:
            v[v == 0] = 1.0
        AB = E.generate(n, [], B)
        for j in range(8):
            Ab = AB[j] + INT_SHIFTS[j] * B[j]
            assert np.abs(Ab).max() <= 64 * (n + 1) < 2 ** 24
            E.first_cg_step(B[j], Ab, np.float32)                                  # asserts p.Ap != 0
    for n in (64, 513, 1030):
        assert (E.pow2_diagonal(n, 61 * n) == 1).any()
