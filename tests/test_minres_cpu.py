"""CPU-side checks of batched MINRES (include/lam_hip.h, lam_hip_solve_many_minres): the numpy model of the recurrence
(tests/minres_reference.py) against scipy.sparse.linalg.minres and against its own true residual, the gates of
tests/minres_data.py re-measured, the inputs' condition of tests/test_gpu_minres.py's indefinite case, and that the header, the
library, the binding, the class and the driver carry the entry point."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import minres_data as D
import minres_reference as M
import pcg_reference as R
from conftest import ROOT, PKG_NAME
from tracking_data import tracking_columns

NEW = "lam_hip_solve_many_minres"
HEADER = os.path.join(ROOT, "include", "lam_hip.h")
EXE = os.path.join(ROOT, PKG_NAME, "test", "test_CG_multi_rhs.out")


def _shifted_cases(n):
    """The smoke system of size n under: no shift, 0.5, -1.003 x the median eigenvalue (half the spectrum negative), -2 lambda_max
    (negative definite)."""
    A, rng = R.smoke_system(n, seed=n)
    ev = np.linalg.eigvalsh(A)
    b = rng.uniform(-1, 1, n)
    return A, b, ev, (0.0, 0.5, -1.003 * float(np.median(ev)), -2.0 * float(ev[-1]))


@pytest.mark.parametrize("n", [7, 64, 384])
def test_the_model_is_scipy_minres(n):
    """Per shift: the model converges to 1e-10 within 6 n iterations; its rel_err agrees with its own true residual to three digits;
    and run for exactly as many iterations as the model took, SciPy's iterate is the model's to the level of SciPy's own residual:
    ||x - x_scipy|| <= 4 (res_model + res_scipy) ||b|| / min |lambda(A + s I)| (two points whose residuals are that small are that
    close), plus rounding."""
    sp = pytest.importorskip("scipy.sparse.linalg")
    A, b, ev, shifts = _shifted_cases(n)
    for s in shifts:
        lam_s = ev + s
        assert (s > -1 or (lam_s < 0).any()) and (s > -10 or (lam_s < 0).all())
        h = []
        x, st = M.minres(A, s, b, 6 * n, 1e-10, history=h)
        res = M.true_residual(A, s, x, b)
        what = f"n={n} shift {s:.4g}: {st['num_iters']} iterations, rel_err {st['rel_err']:.3e}, true residual {res:.3e}"
        assert st["converged"] and st["rel_err"] < 1e-10, what
        # three digits, over the floor at which a residual can be formed at all: 8 n u ||A + s I|| ||x|| / ||b|| (n = 7 terminates
        # at k = n with a residual of rounding size)
        floor = 8 * n * 2.0 ** -53 * np.abs(lam_s).max() * np.linalg.norm(x) / np.linalg.norm(b)
        assert abs(res - st["rel_err"]) < 5e-3 * st["rel_err"] + floor, what
        assert all(h[i + 1][2] <= h[i][2] for i in range(len(h) - 1)), what + ": rel_err is not monotone"
        xs, _ = sp.minres(A, b, shift=-s, rtol=1e-300, maxiter=st["num_iters"])
        res_s = M.true_residual(A, s, xs, b)
        dist = np.linalg.norm(x - xs)
        bound = 4 * (res + res_s) * np.linalg.norm(b) / np.abs(lam_s).min() + 1e-12 * np.linalg.norm(x)
        print(what + f"; SciPy's residual after as many {res_s:.3e}, iterates apart {dist:.3e} (bound {bound:.3e})")
        assert res_s < 1e-9 and dist <= bound, what


def test_rel_err_is_the_true_residual_along_the_way():
    """fp64, the tracking system under minres_data's shifts, every iteration up to 30: phibar / beta1 against ||b - (A + s I) x|| /
    ||b|| of the iterate.  Equal in exact arithmetic; 1e-9 relative leaves five orders over k u cond and pins every sign and index of
    the rotation, which move it by percents -- over the floor at which a residual can be formed at all, 8 n u ||A + s I|| ||x|| / ||b||,
    which the negative definite column (cond 2.8) reaches by k = 10."""
    A, B = tracking_columns()
    ev = np.linalg.eigvalsh(A)
    for j, s in enumerate(D.TRACKING_SHIFTS):
        for k, x, re in D.tracking_histories(np.float64, "rows")[j]:
            res = M.true_residual(A, s, x, B[j])
            floor = 8 * ev.size * 2.0 ** -53 * np.abs(ev + s).max() * np.linalg.norm(x) / np.linalg.norm(B[j])
            assert abs(res - re) < 1e-9 * re + floor, (j, s, k, re, res, floor)


def test_the_tracking_shifts_are_what_minres_data_says():
    A, _ = tracking_columns()
    ev = np.linalg.eigvalsh(A)
    sh = np.array(D.TRACKING_SHIFTS)
    assert len(sh) == 8 and (sh > 0).any() and (sh < 0).any() and (sh == 0).any()
    assert np.array_equal(sh.astype(np.float32).astype(np.float64), sh)                   # exact in both vector dtypes
    assert abs(-sh[D.NEAR_MEDIAN] / np.median(ev) - 1) < 0.01
    assert sh.min() < -2 * ev[-1]                                                         # a negative definite column
    assert sum(((ev + s) < 0).any() and ((ev + s) > 0).any() for s in sh) >= 4            # indefinite columns


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["fp64", "fp32"])
def test_the_gates_are_ten_times_the_models_own_spread(dt):
    """minres_data.GATE re-measured: per tracked k the largest relative spread of x and of rel_err between the model's three sum
    orders, the 8 columns.  The gate is 10 x what was measured when the table was written; here the spread must lie between a
    hundredth and three tenths of the gate (another BLAS draws the system's Q a few ulp differently: the spread is a maximum over
    few values and moves by small factors, not by orders)."""
    sp = D.measure_spreads(dt)
    assert tuple(sorted(D.GATE[dt])) == D.TRACKED_K
    for k in D.TRACKED_K:
        worst = max(sp[k])
        print(f"{dt.__name__} k={k}: spread of x {sp[k][0]:.2e}, of rel_err {sp[k][1]:.2e}; gate {D.GATE[dt][k]:.1e}")
        assert 0.01 * D.GATE[dt][k] <= worst <= 0.3 * D.GATE[dt][k], (k, sp[k], D.GATE[dt][k])


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("n", D.INDEFINITE_SIZES)
def test_the_indefinite_inputs_meet_their_condition(n, dt):
    """The condition tests/test_gpu_minres.py's "solves what CG cannot" relies on: on its inputs the MODEL converges within the cap
    and its own true residual is <= 1.1 x rel_error, so that 2 x rel_error on the device is a gate on the kernels and not on the
    recurrence.  And the system is indefinite: about half the spectrum on either side, none within a third of the half gap of zero."""
    A, B, s, cap, tol = D.indefinite_case(n, dt)
    ev = np.linalg.eigvalsh(A) + s
    _, half = D.central_gap_shift(A)
    assert n // 4 <= (ev < 0).sum() <= 3 * n // 4 and np.abs(ev).min() > half / 3, (s, half, np.abs(ev).min())
    for j in range(8):
        x, st = M.minres(A, s, B[j], cap, tol, dt)
        res = M.true_residual(A, s, x, B[j])
        print(f"n={n} {dt.__name__} column {j}: {st['num_iters']} iterations, rel_err {st['rel_err']:.3e}, true residual {res:.3e}")
        assert st["converged"] and st["num_iters"] <= cap // 2 and res <= 1.1 * tol, (j, st, res)


def test_special_cases_of_the_model():
    """beta' = 0 at k = 1 (b an eigenvector; here a unit vector of a diagonal matrix with a negative pivot): stops with rel_err 0 and
    x = b / pivot bit for bit.  b = 0: NaN to the cap.  max_iters = 0: x = 0, rel_err 1, num_iters 1."""
    Adiag = np.diag([4.0, 2.0, 8.0])
    b = np.array([0.0, 0.5, 0.0])
    x, st = M.minres(Adiag, -4.0, b, 5, 1e-30)
    assert st == dict(num_iters=1, converged=True, rel_err=0.0) and np.array_equal(x, [0.0, -0.25, 0.0])
    x, st = M.minres(Adiag, -4.0, np.zeros(3), 5, 1e-3)
    assert np.isnan(x).all() and np.isnan(st["rel_err"]) and st["num_iters"] == 6 and not st["converged"]
    x, st = M.minres(Adiag, -3.0, np.ones(3), 0, 1e-3)
    assert not x.any() and st == dict(num_iters=1, converged=False, rel_err=1.0)


def test_the_banded_model_is_the_dense_model_on_the_tridiagonal_matrix():
    n = 200
    T = np.diag(np.full(n, 2.0)) + np.diag(np.ones(n - 1), 1) + np.diag(np.ones(n - 1), -1)
    b = np.random.default_rng(n).uniform(-1, 1, n)
    for dt in (np.float64, np.float32):
        xb, sb = M.minres(None, -2.0, b, 5, 0.0, dt, "rows", band=M.tridiag_band(n, dt))
        xd, sd = M.minres(T, -2.0, b, 5, 0.0, dt, "rows")
        u = 2.0 ** -53 if dt is np.float64 else 2.0 ** -24
        assert D.rel_diff_x(xb, xd) < 200 * u and abs(sb["rel_err"] / sd["rel_err"] - 1) < 200 * u
        assert abs(M.band_true_residual(M.tridiag_band(n), -2.0, xb, b) / M.true_residual(T, -2.0, xb, b) - 1) < 1e-12


def test_header_compiles_as_c99_with_the_new_entry_point(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "lam_hip.h"\n'
                   "int use(lam_hip_ctx *c, const double *sigma, lam_hip_stats *st, int32_t *it, int32_t *cv, double *re)\n{\n"
                   "    return lam_hip_solve_many_minres(c, sigma, 10, 1e-9, st, it, cv, re) + lam_hip_solve_many_minres(c, 0, 10, 1e-9, 0, 0, 0, 0);\n}\n")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                        "-o", str(tmp_path / "use.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_library_binding_and_class_carry_the_entry_point_and_the_abi_version_stays_4(lam):
    lam.build()
    L = C.CDLL(lam.lib_path())
    txt = open(HEADER).read()
    history = txt[txt.index("ABI history"):txt.index("#define LAM_HIP_ABI_VERSION")]
    assert hasattr(L, NEW) and NEW in lam.lib()._lam_symbols and NEW in history
    assert re.search(r"#define LAM_HIP_ABI_VERSION 4\b", txt) and lam.lib().lam_hip_abi_version() == 4
    for member in ("solve_minres", "solve_shifted_minres"):
        assert callable(getattr(lam.Solver, member)), member
    hpp = open(os.path.join(ROOT, PKG_NAME, "LAM", "src", "HIP", "ConjugateGradient_HIP_base.hpp")).read()
    assert "bool solve_many_minres(int nrhs, const FloatingType *B, const double *sigma" in hpp
    # the header says what is out of scope and which alpha the recurrence takes
    body = txt[txt.index("Batched MINRES"):txt.index("int lam_hip_solve_many_minres")]
    for word in ("preconditioner", "initial guess", "multi-shift", "several shards", "bf16", "NOT v.(A v - beta v_old)"):
        assert word in body, word


def test_driver_lists_the_flag_and_refuses_its_misuse_before_touching_a_gpu(lam):
    lam.build()
    r = subprocess.run([EXE, "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "[-m " in r.stderr, r.stderr
    for args in (["-m", "-J"], ["-m", "-w", "2"], ["-m", "-S", "0,-1", "-M"], ["-m", "-S", "-1,1", "-J"]):
        r = subprocess.run([EXE, "-s", "16", "-i", "3"] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "Usage" in r.stderr and "-m" in r.stderr and not r.stdout, (args, r.returncode, r.stdout, r.stderr)
    for args in (["-m", "-S", "-1,nan"], ["-m", "-S", "-1,inf"], ["-m", "-S", "-1,,2"], ["-m", "-S", "x"], ["-m", "-S", ",".join(["-1"] * 9)],
                 ["-m", "-S", "-1,1", "-k", "3"]):
        r = subprocess.run([EXE, "-s", "16", "-i", "3"] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "-S takes" in r.stderr and "either sign" in r.stderr and not r.stdout, (args, r.returncode, r.stdout, r.stderr)
    # without -m a negative shift is refused with the words of before, wherever -S stands on the line
    for args in (["-S", "0,-1"], ["-S", "-0.5"], ["-T", "-S", "1,-2", "-J"]):
        r = subprocess.run([EXE, "-s", "16", "-i", "3"] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "-S takes 1..8 comma-separated finite shifts >= 0" in r.stderr and not r.stdout, (args, r.stderr)


def test_host_asan_still_builds_without_the_new_symbol():
    here = os.path.join(ROOT, "tests", "host_asan")
    r = subprocess.run(["make", "-C", here, "all"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "minres" not in open(os.path.join(here, "fake_lam_hip.cpp")).read()
