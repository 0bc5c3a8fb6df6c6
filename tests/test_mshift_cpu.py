"""CPU-side checks of multi-shift CG (include/lam_hip.h, lam_hip_solve_mshift): the numpy model of the recurrence
(tests/mshift_reference.py) against direct solves, against the definition of zeta and against per-shift plain CG -- the figures
tests/test_gpu_mshift.py gates with -- the underflow freeze, and that the header, the library, the binding, the class and the driver
carry the entry points."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mshift_reference as M
import pcg_reference as R
import shifted_data as SD
from conftest import GOLDEN, ROOT, PKG_NAME

NEW = ("lam_hip_solve_mshift", "lam_hip_get_solution_mshift", "lam_hip_true_residual_mshift")
HEADER = os.path.join(ROOT, "include", "lam_hip.h")
EXE = os.path.join(ROOT, PKG_NAME, "test", "test_CG_multi_rhs.out")
U_TV = {np.float64: 2.0 ** -53, np.float32: 2.0 ** -24}
# unsorted, a duplicate (0.5), a zero (the seed) and 1e6
SHIFTS = (3.0, 0.5, 1e6, 0.0, 40.0, 0.5, 0.0625, 11.0, 1.0, 200.0, 0.25)


def _systems(oracle):
    A, rng = R.smoke_system(513, seed=513)
    yield "smoke513", A, rng.uniform(-1, 1, 513)
    G = oracle.read_bin(os.path.join(GOLDEN, "spd_n256_s3.matrix.bin"), np.float64)
    yield "spd_n256_s3", G, np.random.default_rng(256).uniform(-1, 1, G.shape[0])


@pytest.mark.parametrize("dt,tol", [(np.float64, 1e-10), (np.float32, 1e-5)], ids=["fp64", "fp32"])
def test_the_model_solves_every_shift(oracle, dt, tol):
    """Against np.linalg.solve on A_TV + s_j I and against plain CG (pcg_reference.pcg) on that matrix, per shift: every shift meets
    its stop test; the error against the direct solve is at most twice plain CG's (two recurrences that stop a few iterations apart;
    floor: 16 u of the vector dtype, where both have converged to rounding); the host true residual at most twice
    max(plain CG's, rel_error); the slots of the seed's shift ARE the seed, bit for bit, and duplicates agree bit for bit."""
    for name, A, b in _systems(oracle):
        A = A.astype(dt).astype(np.float64)
        b = b.astype(dt)
        n = b.size
        X, st, _ = M.mshift_cg(M.dense_operator(A, dt), b, SHIFTS, 4000, tol, dt)
        assert st["converged"].all() and (st["rel_err"] < tol).all() and not st["frozen"].any(), (name, st)
        assert np.array_equal(X[1], X[5]) and st["num_iters"][1] == st["num_iters"][5]
        b64 = b.astype(np.float64)
        for j, sj in enumerate(SHIFTS):
            Mj = SD.formed(A, dt(sj), dt)
            xc, stc = R.pcg(Mj, b, 4000, tol, None, dt)
            direct = np.linalg.solve(Mj, b64)
            e_ms, e_cg = (np.linalg.norm(v.astype(np.float64) - direct) / np.linalg.norm(direct) for v in (X[j], xc))
            t_ms, t_cg = (np.linalg.norm(b64 - Mj @ v.astype(np.float64)) / np.linalg.norm(b64) for v in (X[j], xc))
            what = f"{name} {dt.__name__} shift {sj}: x error {e_ms:.2e} (CG {e_cg:.2e}), true residual {t_ms:.2e} (CG {t_cg:.2e}), " \
                   f"iterations {st['num_iters'][j]} (CG {stc['num_iters']})"
            print(what)
            assert e_ms <= 2 * max(e_cg, 16 * U_TV[dt]) and t_ms <= 2 * max(t_cg, tol), what
            assert abs(int(st["num_iters"][j]) - stc["num_iters"]) <= 2 * M.MODEL_ITERS_DEVIATION["F64" if dt is np.float64 else "F32"], what
            if sj == 0:
                assert np.array_equal(X[j], xc) and st["num_iters"][j] == stc["num_iters"] and st["rel_err"][j] == stc["rel_err"], what


def test_zeta_is_the_ratio_of_the_residual_norms(oracle):
    """zeta_k = ||r_j|| / ||r|| by definition: the model's zeta after k = 1 .. 20 iterations against rel_err of plain CG on
    A + s_j I over rel_err of plain CG on the seed's matrix, fp64.  Two recursive residuals drift apart like k u cond (20 * 1.1e-16 *
    55 = 1.2e-13 here) times a modest constant: 1e-9 leaves four orders and still pins an index or a sign in the recurrence, which
    moves zeta by percents."""
    A, rng = R.smoke_system(513, seed=513)
    b = rng.uniform(-1, 1, 513)
    sh = np.array([s for s in SHIFTS if s <= 40])
    _, _, hist = M.mshift_cg(M.dense_operator(A, np.float64), b, sh, 20, 0.0)
    for k in range(1, 21):
        rel = [R.pcg(SD.formed(A, s), b, k, 0.0)[1]["rel_err"] for s in sh]
        seed = R.pcg(A, b, k, 0.0)[1]["rel_err"]
        want = np.array(rel) / seed
        got = hist[k - 1]["zeta"]
        live = sh != 0
        assert np.allclose(got[live], want[live], rtol=1e-9, atol=0), (k, got, want)
        assert hist[k - 1]["rel"] == seed and np.allclose(hist[k - 1]["rel_err"][live], np.array(rel)[live], rtol=1e-9, atol=0)


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["fp64", "fp32"])
def test_an_underflowing_zeta_freezes_the_shift(dt):
    """rel_error = 0, cap 70, s = 1e6: zeta leaves fp64's normal range, the shift is frozen before that step: everything finite, not
    converged, num_iters the last completed step, x within 32 u of the direct solve (cond(A + 1e6 I) = 1 + 1e-5)."""
    A, rng = R.smoke_system(513, seed=513)
    A = A.astype(dt).astype(np.float64)
    b = rng.uniform(-1, 1, 513).astype(dt)
    X, st, hist = M.mshift_cg(M.dense_operator(A, dt), b, [0.5, 1e6, 0.0], 70, 0.0, dt)
    assert np.isfinite(X).all() and np.isfinite(st["rel_err"]).all() and not st["converged"].any()
    assert st["frozen"].tolist() == [False, True, False] and st["num_iters"][0] == 71 and st["num_iters"][2] == 71
    k = int(st["num_iters"][1])
    assert 5 < k < 70 and hist[k - 1]["live"][1] and not hist[k]["live"][1] and hist[k - 1]["zeta"][1] >= M.TINY
    direct = np.linalg.solve(A + np.float64(dt(1e6)) * np.eye(513), b.astype(np.float64))
    err = np.linalg.norm(X[1].astype(np.float64) - direct) / np.linalg.norm(direct)
    print(f"{dt.__name__}: frozen after {k} steps at rel_err {st['rel_err'][1]:.3e}, x off the direct solve by {err:.3e}")
    assert err <= 32 * U_TV[dt]
    # b = 0: 0/0 in the seed, NaN everywhere, nothing frozen, the cap's count
    X, st, _ = M.mshift_cg(M.dense_operator(A, dt), np.zeros(513, dt), [0.5, 1e6, 0.0], 5, 1e-3, dt)
    assert np.isnan(X).all() and np.isnan(st["rel_err"]).all() and (st["num_iters"] == 6).all() and not st["frozen"].any()


def test_the_recorded_deviations_hold_for_the_blas_pair():
    """mshift_reference.MODEL_ITERS_DEVIATION / MODEL_TRUE_RATIO were measured in four summation orders, model and CG in the same
    one, at n = 513 and 1030 (minutes); here the BLAS pair on the n = 513 system, 9 and 64 shifts, must stay inside them."""
    for dt, name, tol in ((np.float64, "F64", 1e-10), (np.float32, "F32", 1e-5)):
        A, b = M.converged_system(513, dt)
        b64 = b.astype(np.float64)
        for S in (9, 64):
            sh = M.converged_shifts(S)
            assert sh.min() == 0 and sh.max() == 100 and (np.diff(sh) < 0).any() and (np.diff(sh) > 0).any()
            X, st, _ = M.mshift_cg(M.dense_operator(A, dt), b, sh, 4000, tol, dt)
            assert st["converged"].all()
            for j, sj in enumerate(sh):
                Mj = SD.formed(A, dt(sj), dt)
                xc, stc = R.pcg(Mj, b, 4000, tol, None, dt)
                t_ms, t_cg = (np.linalg.norm(b64 - Mj @ v.astype(np.float64)) / np.linalg.norm(b64) for v in (X[j], xc))
                assert abs(int(st["num_iters"][j]) - stc["num_iters"]) <= M.MODEL_ITERS_DEVIATION[name], (name, S, j)
                assert t_ms / max(t_cg, tol) <= M.MODEL_TRUE_RATIO[name] * 1.0001, (name, S, j, t_ms, t_cg)


def test_header_compiles_as_c99_with_the_new_entry_points(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "lam_hip.h"\n'
                   "int use(lam_hip_ctx *c, const double *b, const double *sigma, double *x, double *res, int32_t *it)\n{\n"
                   "    double s[LAM_HIP_MAX_SHIFTS];\n    (void)s;\n"
                   "    return lam_hip_solve_mshift(c, b, 3, sigma, 10, 1e-9, 0, it, 0, 0) + lam_hip_get_solution_mshift(c, 3, x)\n"
                   "           + lam_hip_true_residual_mshift(c, 3, res);\n}\n")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                        "-o", str(tmp_path / "use.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_library_binding_and_class_carry_the_entry_points_and_the_abi_version_stays_4(lam):
    lam.build()
    L = C.CDLL(lam.lib_path())
    txt = open(HEADER).read()
    history = txt[txt.index("ABI history"):txt.index("#define LAM_HIP_ABI_VERSION")]
    for name in NEW:
        assert hasattr(L, name) and name in lam.lib()._lam_symbols and name in history, name
    assert "LAM_HIP_MAX_SHIFTS" in history and re.search(r"#define LAM_HIP_MAX_SHIFTS 64\b", txt) and lam.MAX_SHIFTS == 64
    assert re.search(r"#define LAM_HIP_ABI_VERSION 4\b", txt) and lam.lib().lam_hip_abi_version() == 4
    for member in ("solve_multishift", "multishift_solutions", "multishift_true_residuals", "solve_shifted"):
        assert callable(getattr(lam.Solver, member)), member
    hpp = open(os.path.join(ROOT, PKG_NAME, "LAM", "src", "HIP", "ConjugateGradient_HIP_base.hpp")).read()
    assert "bool solve_mshift(int nshifts, const double *sigma" in hpp and "bool true_residual_mshift(int nshifts, double *rel_res)" in hpp


def test_driver_lists_the_flag_and_refuses_its_misuse_before_touching_a_gpu(lam):
    lam.build()
    r = subprocess.run([EXE, "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "[-M " in r.stderr, r.stderr
    many = ",".join(["1"] * 65)
    for args in (["-M"], ["-M", "-S", "0,1", "-J"], ["-M", "-S", "0,1", "-w", "2"], ["-M", "-S", "0,-1"], ["-M", "-S", many],
                 ["-M", "-S", "0,1", "-k", "2"]):
        r = subprocess.run([EXE, "-s", "16", "-i", "3"] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "Usage" in r.stderr and "-M" in r.stderr and not r.stdout, (args, r.returncode, r.stdout, r.stderr)
    # without -M a list of nine stays refused as before
    r = subprocess.run([EXE, "-s", "16", "-i", "3", "-S", ",".join(["1"] * 9)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "-S takes" in r.stderr and not r.stdout


def test_host_asan_still_builds_without_the_new_symbols():
    here = os.path.join(ROOT, "tests", "host_asan")
    r = subprocess.run(["make", "-C", here, "all"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "mshift" not in open(os.path.join(here, "fake_lam_hip.cpp")).read()
