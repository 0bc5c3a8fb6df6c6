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


# ------------------------------------------------------------------------------------------------
# host helpers of tests/test_gpu_batch_recurrence.py
# ------------------------------------------------------------------------------------------------
def test_unit_diagonal_and_scaled_systems_are_what_they_claim():
    for dt in (np.float64, np.float32):
        for n in (1, 2, 3, 5, 257):
            Cm, rng = R.unit_diagonal_system(n, dt)
            e = R.varying_exponents(n, rng)
            A, s = R.scale_system(Cm, e)
            assert np.array_equal(Cm, Cm.T) and np.array_equal(np.diag(Cm), np.ones(n)) and np.linalg.eigvalsh(Cm)[0] > 0
            assert np.array_equal(Cm.astype(dt).astype(np.float64), Cm) and np.array_equal(A.astype(dt).astype(np.float64), A)
            assert e.min() >= -6 and e.max() <= 6 and (np.diff(e) != 0).all() and (n < 64 or len(set(e)) == 13)
            assert np.array_equal(A, A.T) and np.array_equal(np.diag(A), 4.0 ** e) and np.array_equal(A / s[:, None] / s[None, :], Cm)
            assert np.array_equal(R.jacobi_dinv(A, dt), (0.25 ** e).astype(dt))


def test_jacobi_on_the_scaled_system_is_the_plain_recurrence_scaled_bit_for_bit():
    """The identity tests/test_gpu_batch_recurrence.py demands of the kernels, on the numpy restatement: with A = S C S, diag(C) = 1,
    S = diag(2^e), pcg(A, S b, jacobi) is 2^-e o pcg(C, b, plain) bit for bit, in fp64 and fp32, at every k."""
    for dt in (np.float64, np.float32):
        for n in (5, 257, 1025):
            Cm, rng = R.unit_diagonal_system(n, dt)
            e = R.varying_exponents(n, rng)
            A, s = R.scale_system(Cm, e)
            dinv = R.jacobi_dinv(A, dt)
            B = rng.uniform(-1, 1, (3, n)).astype(dt)
            for k in sorted({min(k, n) for k in (1, 2, 5, 40)}):
                for j in range(3):
                    x0, st0 = R.pcg(Cm, B[j], k, 0.0, None, dt)
                    x1, st1 = R.pcg(A, (s * B[j]).astype(dt), k, 0.0, dinv, dt)
                    assert st0["num_iters"] == st1["num_iters"] == k + 1 and st0["rel_err"] > 1e-30, (dt, n, k, j, st0)
                    bad = np.flatnonzero(x1 != (x0 / s).astype(dt))
                    assert x1.dtype == dt and bad.size == 0, (dt, n, k, j, bad[:6])


def test_an_eigenvector_column_stops_at_once_where_random_columns_run_on():
    """What the frozen-column variant of the scaled-system test relies on, on the reference: tolerance 1e-3, cap 12."""
    for dt in (np.float64, np.float32):
        for n in (257, 1025):
            Cm, rng = R.unit_diagonal_system(n, dt)
            A, s = R.scale_system(Cm, R.varying_exponents(n, rng))
            B = rng.uniform(-1, 1, (8, n))
            B[1] = np.linalg.eigh(Cm)[1][:, n // 2]
            dinv = R.jacobi_dinv(A, dt)
            for j in range(8):
                _, st = R.pcg(A, (s * B[j].astype(dt)).astype(dt), 12, 1e-3, dinv, dt)
                assert (st["converged"] and st["num_iters"] <= 2) if j == 1 else (st["rel_err"] > 1e-2 and not st["converged"]), (dt, n, j, st)


def _spread(results):
    """Largest relative difference in x and in rel_err between any two (x, stats) of `results`."""
    wx = wr = 0.0
    for a in range(len(results)):
        for c in range(a + 1, len(results)):
            xa, xc = results[a][0].astype(np.float64), results[c][0].astype(np.float64)
            wx = max(wx, np.linalg.norm(xa - xc) / np.linalg.norm(xc))
            wr = max(wr, abs(results[a][1]["rel_err"] / results[c][1]["rel_err"] - 1))
    return wx, wr


def _all_orders(A, b, k, dinv, dt):
    """pcg (BLAS: the reference the GPU tests compare with) and pcg_ordered in its three orders."""
    return [R.pcg(A, b, k, 1e-30, dinv, dt)] + [R.pcg_ordered(A, b, k, 1e-30, dinv, dt, o) for o in R.ORDERS]


def test_fp64_references_are_a_tenth_of_the_gates_sure_of_themselves():
    """pcg and pcg_ordered's three summation orders against one another in fp64, every tracked k, all 8 columns: x and rel_err of the
    plain run on the n = 384 system, rel_err of the Jacobi run on scaled_tracking_system -- the reference of
    test_jacobi_rel_err_tracks_the_reference_iteration_by_iteration[F64] -- within a tenth of the single solve's gates."""
    from tracking_data import ITERATION_TRACKING_GATES, TRACKED_K, scaled_tracking_system, tracking_columns
    A, B = tracking_columns()
    As, Bs, dinv = scaled_tracking_system(np.float64)
    for k, gate_res, gate_x in ITERATION_TRACKING_GATES:
        if k not in TRACKED_K:
            continue
        for j in range(8):
            wx, wr = _spread(_all_orders(A, B[j], k, None, np.float64))
            _, jr = _spread(_all_orders(As, Bs[j], k, dinv, np.float64))
            assert wx <= 0.1 * gate_x and wr <= 0.1 * gate_res and jr <= 0.1 * gate_res, (k, j, wx, wr, jr)


def test_fp32_reference_spread_is_a_tenth_of_the_fp32_gates():
    """What FP32_TRACKING_GATE is derived from, re-measured in fp32 on the two systems of test_gpu_batch_recurrence.py's tracking
    tests: the spread between pcg_ordered's three summation orders ("rows" is the GPU tests' reference; no BLAS, the same bits on
    every machine) is at most a tenth of the gate at every k, and so is the spread with pcg (BLAS) among them up to k = 30.  At
    k = 40 the recurrence is chaotic and BLAS's own order can change from run to run, so there pcg is printed, not asserted."""
    from tracking_data import FP32_TRACKING_GATE, scaled_tracking_system, tracking_columns
    A, B = tracking_columns()
    As, Bs, dinv = scaled_tracking_system(np.float32)
    for k, gate in FP32_TRACKING_GATE.items():
        worst = with_blas = 0.0
        for j in range(8):
            plain, jac = _all_orders(A, B[j], k, None, np.float32), _all_orders(As, Bs[j], k, dinv, np.float32)
            with_blas = max(with_blas, *_spread(plain), _spread(jac)[1])
            worst = max(worst, *_spread(plain[1:]), _spread(jac[1:])[1])
        print(f"fp32 k={k}: spread between summation orders {worst:.3e}, with BLAS among them {with_blas:.3e}, gate {gate:.3e}")
        assert 10 * worst <= gate and (k > 30 or 10 * with_blas <= gate), (k, worst, with_blas, gate)
