"""CPU-side checks of the batched solve from an initial guess (include/lam_hip.h, lam_hip_solve_many_x0 / lam_hip_true_residual_many):
the numpy restatement's own properties (tests/warm_start_reference.py), the header, the exports, the binding and the driver's
argument handling."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import exact_data as E
import pcg_reference as R
import warm_start_reference as W
from conftest import ROOT, PKG_NAME

NEW = ("lam_hip_solve_many_x0", "lam_hip_true_residual_many")
HEADER = os.path.join(ROOT, "include", "lam_hip.h")
KEYS = ("num_iters", "converged", "rel_err")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def test_zero_guess_is_pcg_bit_for_bit():
    """Plain and Jacobi, fp64 and fp32, BLAS and the three fixed orders, with a tolerance that stops and at the cap."""
    A, rng = R.sms_system(96)
    b = rng.uniform(-1, 1, 96)
    for dt in (np.float64, np.float32):
        for dinv in (None, R.jacobi_dinv(A, dt)):
            for k, tol in ((1, 0.0), (5, 0.0), (40, 0.0), (200, 1e-3), (3, 1.0)):
                x, st = R.pcg(A, b, k, tol, dinv, dt)
                xw, stw = W.pcg_x0(A, b, np.zeros(96), k, tol, dinv, dt)
                assert np.array_equal(_bits(x), _bits(xw)) and all(st[q] == stw[q] for q in KEYS), (dt, k, tol, st, stw)
                assert len(stw["rel_err_history"]) == min(st["num_iters"], k) + 1 and stw["rel_err_history"][0] == 1.0
                for order in R.ORDERS:
                    x, st = R.pcg_ordered(A, b, k, tol, dinv, dt, order)
                    xw, stw = W.pcg_x0(A, b, np.zeros(96), k, tol, dinv, dt, order)
                    assert np.array_equal(_bits(x), _bits(xw)) and all(st[q] == stw[q] for q in KEYS), (dt, k, tol, order, st, stw)
    # a zero guess meets a tolerance above 1 at k = 0: where the identity ends
    _, st = W.pcg_x0(A, b, np.zeros(96), 5, 1.5)
    assert st["num_iters"] == 0 and st["converged"] and st["rel_err"] == 1.0


def test_exact_guess_takes_no_iteration_and_max_iters_0_returns_the_start():
    n = 257
    A = W.tridiag(n)
    xs = E.int_vec(n, 3)
    b = E.tridiag_product(xs)
    for dt in (np.float64, np.float32):
        for dinv in (None, R.jacobi_dinv(A, dt)):
            x, st = W.pcg_x0(A, b, xs, 50, 1e-30, dinv, dt)
            assert st["num_iters"] == 0 and st["converged"] and st["rel_err"] == 0.0 and np.array_equal(x, xs.astype(dt))
            # rel_error <= 0 never stops, k = 0 included: 0/0 to the cap, like a b = 0 column
            x, st = W.pcg_x0(A, b, xs, 3, 0.0, dinv, dt)
            assert st["num_iters"] == 4 and not st["converged"] and np.isnan(x).all()
            x0 = xs + 1.0
            x, st = W.pcg_x0(A, b, x0, 0, 1e-30, dinv, dt)
            assert st["num_iters"] == 1 and not st["converged"] and np.array_equal(x, x0.astype(dt))
            assert st["rel_err"] == np.sqrt(np.sum(E.tridiag_product(np.ones(n)) ** 2) / np.dot(b, b))


def test_shift_identity_on_integer_data():
    """c = b - A x0 exact: the warm run on (b, x0) and the cold run on c share r, p, alpha, beta bit for bit, so rr_k is the same
    number and only the stop test's denominator differs; x_warm - (x0 + x_cold) stays within one rounding per update and run."""
    n, k = 257, 40
    A = W.tridiag(n)
    for dt in (np.float64, np.float32):
        x0 = E.int_vec(n, 5)
        c = E.int_vec(n, 6)
        b = c + E.tridiag_product(x0)
        xw, sw = W.pcg_x0(A, b, x0, k, 0.0, None, dt)
        xc, sc = W.pcg_x0(A, c, np.zeros(n), k, 0.0, None, dt)
        nb, nc = np.sqrt(np.dot(b, b)), np.sqrt(np.dot(c, c))
        for hw, hc in zip(sw["rel_err_history"], sc["rel_err_history"]):
            assert abs(hw * nb - hc * nc) <= 4 * np.spacing(hc * nc), (dt, hw, hc)
        bound = 2 * k * np.finfo(dt).eps * np.maximum(sw["x_absmax"], np.abs(x0) + sc["x_absmax"]).astype(np.float64)
        assert (np.abs(xw.astype(np.float64) - (x0 + xc.astype(np.float64))) <= bound).all()


def test_header_declares_both_entry_points_and_compiles_as_c99(tmp_path):
    txt = open(HEADER).read()
    assert re.search(r"int lam_hip_solve_many_x0\(lam_hip_ctx \*ctx, int precond, const void \*x0_host, int max_iters, double rel_error,\s*"
                     r"lam_hip_stats \*stats, int32_t \*num_iters, int32_t \*converged, double \*rel_err\);", txt)
    assert re.search(r"int lam_hip_true_residual_many\(lam_hip_ctx \*ctx, int nrhs, double \*rel_res\);", txt)
    history = txt[txt.index("ABI history"):txt.index("#define LAM_HIP_ABI_VERSION")]
    assert all(name in history for name in NEW) and re.search(r"#define LAM_HIP_ABI_VERSION 4\b", txt)
    src = tmp_path / "use.c"
    src.write_text('#include "lam_hip.h"\n'
                   "int use(lam_hip_ctx *c, const double *x0, double *res)\n{\n"
                   "    int32_t it[LAM_HIP_MAX_RHS], cv[LAM_HIP_MAX_RHS];\n    double re[LAM_HIP_MAX_RHS];\n    lam_hip_stats st;\n"
                   "    return lam_hip_solve_many_x0(c, LAM_HIP_PC_JACOBI, x0, 10, 1e-9, &st, it, cv, re)\n"
                   "           + lam_hip_solve_many_x0(c, LAM_HIP_PC_NONE, 0, 10, 1e-9, &st, it, cv, re) + lam_hip_true_residual_many(c, 2, res);\n}\n")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                        "-o", str(tmp_path / "use.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_library_exports_and_binding_binds_both_entry_points(lam):
    lam.build()
    L = C.CDLL(lam.lib_path())
    for name in NEW:
        assert hasattr(L, name), name
    assert set(NEW) <= set(lam.lib()._lam_symbols)
    assert len(lam.lib().lam_hip_solve_many_x0.argtypes) == 9 and len(lam.lib().lam_hip_true_residual_many.argtypes) == 3
    assert callable(lam.Solver.true_residuals) and "x0" in lam.Solver.solve_many.__code__.co_varnames


def test_driver_lists_the_flags_and_refuses_bad_arguments_before_touching_a_gpu(lam):
    lam.build()
    exe = os.path.join(ROOT, PKG_NAME, "test", "test_CG_multi_rhs.out")
    r = subprocess.run([exe, "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "-w" in r.stderr and "-T" in r.stderr
    for args in (["-s", "16", "-k", "2", "-i", "3", "-w", "4"], ["-s", "16", "-k", "2", "-i", "3", "-w"], ["-T", "-k", "2", "-i", "3"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "Usage" in r.stderr, (args, r.stderr)
