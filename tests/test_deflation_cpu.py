"""Deflated CG for the batch without a GPU: the host's small inverse through the C ABI and under sanitizers, the numpy model
tests/deflation_reference.py against the mathematics it claims, the gates and margins tests/test_gpu_deflation.py holds the device to
(tests/deflation_data.py), and the presence of the new names in every layer."""
import os
import subprocess

import numpy as np
import pytest

import deflation_data as D
import deflation_reference as R
import lanczos_data as LD
import lanczos_reference as L
import pcg_reference as P
from conftest import ROOT, PKG_NAME


# ------------------------------------------------------------------------------------------------
# lam_hip_chol_inverse
# ------------------------------------------------------------------------------------------------
def test_chol_inverse_is_exact_on_power_of_two_factors(lam):
    """G = L D L^T with integer L and D a power of two: every quotient and product of the factorisation is exact, so is the inverse."""
    Lf = np.array([[1.0, 0, 0, 0], [2, 1, 0, 0], [-1, 3, 1, 0], [4, -2, 1, 1]])
    for Dd in (np.array([4.0, 2.0, 0.5, 8.0]), np.ones(4)):
        G = Lf @ np.diag(Dd) @ Lf.T
        Li = np.round(np.linalg.inv(Lf))
        assert np.array_equal(Li @ Lf, np.eye(4))
        want = Li.T @ np.diag(1.0 / Dd) @ Li
        got = lam.chol_inverse(G)
        assert np.array_equal(got, want) and np.array_equal(got, got.T)
        assert np.array_equal(R.chol_inverse(G), want)              # the model's restatement is the same routine
    assert np.array_equal(lam.chol_inverse([[0.25]]), [[4.0]])
    # only the lower triangle is read
    G2 = G.copy()
    G2[0, 3] = 1e9
    assert np.array_equal(lam.chol_inverse(G2), got)


@pytest.mark.parametrize("m", D.CHOL_SIZES)
def test_chol_inverse_against_numpy(lam, m):
    """Against numpy.linalg.inv within 10 x numpy's own error against the longdouble inverse (deflation_data.CHOL_GATE), which is
    re-measured here: it must lie between a hundredth and three tenths of the gate."""
    G = D.chol_case(m)
    own = D.measure_chol_margin(m)
    ref = np.linalg.inv(G)
    got = lam.chol_inverse(G)
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"m={m}: |Ginv - inv(G)| / |inv(G)| {err:.2e}; numpy against longdouble {own:.2e}; gate {D.CHOL_GATE[m]:.1e}")
    assert 0.01 * D.CHOL_GATE[m] <= own <= 0.3 * D.CHOL_GATE[m]
    assert err <= D.CHOL_GATE[m]
    assert np.array_equal(got, got.T)
    assert np.array_equal(got, R.chol_inverse(G))


def test_chol_inverse_refusals_name_the_column(lam):
    def refused(G):
        with pytest.raises(lam.LamHipError) as e:
            lam.chol_inverse(G)
        assert e.value.code == -1
        return e.value.bad_col, str(e.value)

    G = D.chol_case(7)
    zero = G.copy()
    zero[3, :] = zero[:, 3] = 0.0
    assert refused(zero)[0] == 3                                     # a zero pivot
    assert "column 3" in refused(zero)[1]
    X = np.random.default_rng(1).uniform(-1, 1, (9, 5))
    X[:, 4] = X[:, 1]
    assert refused(X.T @ X)[0] == 4                                  # a duplicated column: the later one's pivot
    nan = G.copy()
    nan[5, 5] = np.nan
    assert refused(nan)[0] == 5
    off = G.copy()
    off[4, 2] = np.nan
    assert refused(off)[0] == 4                                      # an off-diagonal NaN reaches the pivot of its row
    neg = G.copy()
    neg[6, 6] = -1.0
    assert refused(neg)[0] == 6
    assert refused(np.eye(lam.MAX_DEFLATION + 1))[0] == -1           # m out of range
    assert "outside 1..32" in refused(np.zeros((0, 0)))[1]


def test_chol_header_under_sanitizers(tmp_path):
    """csrc/lam_host_chol.h -- the header the product build includes, no HIP in it -- as a stand-alone program with its own main under
    g++ -fsanitize=address,undefined: built and run as an executable, with G and Ginv at exactly their stated size."""
    csrc = os.path.join(ROOT, PKG_NAME, "csrc")
    header = open(os.path.join(csrc, "lam_host_chol.h")).read()
    assert "hip_runtime" not in header and "#include <hip" not in header
    assert '#include "lam_host_chol.h"' in open(os.path.join(csrc, "lam_kernels.h")).read()
    assert "lam::chol_inverse(" in open(os.path.join(csrc, "lam_deflate.h")).read()
    exe = str(tmp_path / "chol_asan.out")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", csrc,
                        os.path.join(ROOT, "tests", "host_chol", "chol_asan_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0 and r.stdout.strip().endswith("ok chol"), r.stdout[-2000:] + r.stderr[-2000:]


# ------------------------------------------------------------------------------------------------
# the model is a deflated CG
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", ["F64", "F32"])
def test_exact_eigenvectors_take_the_outliers_out_and_a_random_space_does_not(dtype_name):
    """On the known-spectrum system: with the 8 outliers' eigenvectors the model needs fewer iterations than plain CG (14 against 35
    in fp64, 7 against 33 in fp32, the figures of DESIGN §16), with the four low ones alone still fewer; a random W of the same size
    keeps the plain count to within the two iterations the fp32 model's own orders differ by; W^T r stays at rounding level --
    N u_TV ||A|| ||x|| relative to ||b||, the size of r's own rounding error -- and the true residual stays at the plain solve's."""
    dtype, tol = D.DTYPES[dtype_name], D.KNOWN_REL_ERROR[dtype_name]
    u = L.UNIT_ROUNDOFF[dtype]
    A = LD.known_matrix(dtype_name)
    ev, Q = np.linalg.eigh(A)
    b = D.known_rhs()[0]
    _, plain = P.pcg_ordered(A, b, D.KNOWN_MAX_ITERS, tol, None, dtype, "rows")
    counts = {}
    for name, W in (("eight", np.concatenate([Q[:, :4], Q[:, -4:]], axis=1).T), ("low", Q[:, :4].T),
                    ("random", np.random.default_rng(8).uniform(-1, 1, (8, D.KNOWN_N)))):
        sp = R.space(A, W, dtype)
        x, st = R.deflated_cg(A, sp, b, D.KNOWN_MAX_ITERS, tol, dtype)
        r = b - A @ x.astype(np.float64)
        Wn = sp["W"].astype(np.float64)
        wr = np.abs(Wn @ r).max() / (np.linalg.norm(Wn, axis=1).max() * np.linalg.norm(b))
        floor = D.KNOWN_N * u * np.abs(ev).max() * np.linalg.norm(x.astype(np.float64)) / np.linalg.norm(b)
        counts[name] = st["num_iters"]
        print(f"{dtype_name} {name}: {st['num_iters']} iterations (plain {plain['num_iters']}), |W^T r| / (|W| |b|) {wr:.2e} (floor {floor:.2e}), "
              f"true residual {P.true_residual(A, x, b):.2e}")
        assert st["converged"] and wr <= floor
        assert P.true_residual(A, x, b) <= 2 * tol
    assert counts["eight"] < counts["low"] < plain["num_iters"]
    assert counts["eight"] == {"F64": 14, "F32": 7}[dtype_name]
    assert abs(counts["random"] - plain["num_iters"]) <= 2


def test_a_right_hand_side_inside_the_space_is_solved_by_the_start_vector():
    n = 65
    A = np.diag(2.0 ** (np.arange(n) % 5))
    W = np.zeros((2, n))
    W[0, 3] = W[1, 40] = 1.0
    b = np.zeros(n)
    b[3], b[40] = 3.0, -2.0
    for dtype in (np.float64, np.float32):
        sp = R.space(A, W, dtype)
        x, st = R.deflated_cg(A, sp, b, 10, 1e-12, dtype)
        assert st == dict(num_iters=0, converged=True, rel_err=0.0) and np.array_equal(x, b / np.diag(A))
        b2 = np.zeros(n)
        b2[3] = b2[7] = 1.0
        x, st = R.deflated_cg(A, sp, b2, 10, 1e-12, dtype)
        assert st["num_iters"] == 1 and st["rel_err"] == 0.0 and np.array_equal(x, b2 / np.diag(A))


def test_the_operator_model_is_the_integer_answer():
    rng = np.random.default_rng(4)
    n, m = 300, 5
    Wd, Wa, M, u = rng.integers(-1, 2, (m, n)), rng.integers(-1, 2, (m, n)), rng.integers(-2, 3, (m, m)), rng.integers(-3, 4, n)
    for dtype in (np.float64, np.float32):
        for order in D.ORDERS:
            coeff, out = R.operator(Wd.astype(dtype), Wa.astype(dtype), M, u, dtype, order)
            assert np.array_equal(coeff, Wd @ u) and np.array_equal(out, u - Wa.T @ (M @ (Wd @ u)))


# ------------------------------------------------------------------------------------------------
# gates and margins
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,dtype_name,m", sorted(D.PARITY_GATE))
def test_the_parity_gates_are_ten_times_the_models_own_spread(n, dtype_name, m):
    """deflation_data.PARITY_GATE re-measured: per capped run the largest relative spread of rel_err and of x between the model's three
    sum orders, over the 8 columns.  The gate is 10 x what was measured when the table was written; here the spread must lie between
    a hundredth and three tenths of the gate (tests/test_lanczos_cpu.py's rule)."""
    assert (n, m) == D.PARITY_M_LARGE or (n in D.PARITY_SIZES and m == D.PARITY_M)
    sp = D.measure_parity_spreads(n, dtype_name, m)
    gate = D.PARITY_GATE[(n, dtype_name, m)]
    assert tuple(sorted(gate)) == D.PARITY_K
    for k in D.PARITY_K:
        print(f"n={n} {dtype_name} m={m} k={k}: spread of rel_err {sp[k][0]:.2e}, of x {sp[k][1]:.2e}, gate {gate[k]:.1e}")
        assert 0.01 * gate[k] <= max(sp[k]) <= 0.3 * gate[k], (k, sp[k], gate[k])


@pytest.mark.parametrize("dtype_name", ["F64", "F32"])
def test_the_end_to_end_margins_are_the_models(dtype_name):
    """deflation_data.KNOWN_ITER_MARGIN and KNOWN_TRUE_MARGIN re-measured over the three sum orders and over numpy's eigenvectors in
    place of the model's Ritz vectors: the deflated count does not move at all, stays strictly below every plain count, and the
    largest ratio of the true residuals is a tenth of the recorded margin."""
    runs = [D.known_model(dtype_name, o) for o in D.ORDERS] + [D.known_model(dtype_name, "rows", True)]
    base = runs[0]["deflated"]
    spread = max(int(np.abs(r["deflated"] - base).max()) for r in runs)
    ratio = max(float((r["true_deflated"] / r["true_plain"]).max()) for r in runs)
    print(f"{dtype_name}: deflated {[list(r['deflated']) for r in runs]}, plain {[list(r['plain']) for r in runs]}, true residual ratio {ratio:.2f}")
    assert spread + 1 == D.KNOWN_ITER_MARGIN[dtype_name]
    assert all((r["deflated"] + D.KNOWN_ITER_MARGIN[dtype_name] < r["plain"]).all() for r in runs)
    assert 0.01 * D.KNOWN_TRUE_MARGIN[dtype_name] <= ratio <= 0.3 * D.KNOWN_TRUE_MARGIN[dtype_name]


# ------------------------------------------------------------------------------------------------
# presence
# ------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("lam_hip_set_deflation", "lam_hip_set_deflation_eigs", "lam_hip_solve_many_deflated", "lam_hip_deflate_many",
               "lam_hip_chol_inverse")


def test_every_layer_carries_the_new_names(lam):
    import ctypes as C
    header = open(os.path.join(ROOT, "include", "lam_hip.h")).read()
    history = header[header.index("ABI history"):header.index("#define LAM_HIP_ABI_VERSION")]
    for name in NEW_SYMBOLS + ("LAM_HIP_MAX_DEFLATION", '"deflation_m"'):
        assert name in history, name
    assert "#define LAM_HIP_MAX_DEFLATION 32" in header
    lib = C.CDLL(lam.lib_path())
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in lam.lib()._lam_symbols, name
    for member in ("set_deflation", "set_deflation_from_eigs", "solve_deflated", "deflate_many"):
        assert callable(getattr(lam.Solver, member)), member
    assert callable(lam.chol_inverse) and lam.MAX_DEFLATION == 32
    cls = open(os.path.join(ROOT, PKG_NAME, "LAM", "src", "HIP", "ConjugateGradient_HIP_base.hpp")).read()
    for member in ("bool set_deflation(", "bool set_deflation_from_eigs(", "bool solve_many_deflated("):
        assert member in cls, member
    driver = open(os.path.join(ROOT, PKG_NAME, "test", "test_CG_multi_rhs.cpp")).read()
    assert "-D m" in driver and "W:D:" in driver
    tu = open(os.path.join(ROOT, PKG_NAME, "csrc", "lam_hip.hip")).read()
    assert '#include "lam_deflate.h"' in tu
