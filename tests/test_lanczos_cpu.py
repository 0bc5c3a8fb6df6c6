"""The Lanczos eigensolver (lam_hip_eigs) without a GPU: the host's tridiagonal eigensolver through the C ABI and under sanitizers,
the numpy model tests/lanczos_reference.py against the mathematics it claims, the gates and step caps tests/test_gpu_eigs.py holds
the device to (tests/lanczos_data.py), and the presence of the new names in every layer."""
import os
import subprocess

import numpy as np
import pytest

import lanczos_data as D
import lanczos_reference as L
from conftest import ROOT, PKG_NAME

U64 = 2.0 ** -53


# ------------------------------------------------------------------------------------------------
# lam_hip_tridiag_eigen
# ------------------------------------------------------------------------------------------------
def _tridiag_case(k, flavour):
    rng = np.random.default_rng(1000 * k + len(flavour))
    a, b = rng.standard_normal(k), rng.standard_normal(max(k - 1, 0))
    if flavour == "decoupled" and k > 2:
        b[k // 2] = 0.0                      # a zero beta in the middle: T is two independent blocks
    if flavour == "close" and k >= 2:
        a[:] = 1.0                           # eigenvalues in pairs 1e-9 apart
        b[:] = 0.0
        b[::2] = 1e-9 * rng.uniform(0.5, 1.0, b[::2].size)
    return a, b


@pytest.mark.parametrize("flavour", ["random", "decoupled", "close"])
@pytest.mark.parametrize("k", [1, 2, 3, 17, 256])
def test_tridiag_eigen_against_numpy(lam, k, flavour):
    """Eigenvalues to 4 k u ||T|| against numpy.linalg.eigh of the dense T; the eigenvectors -- and with them last_row, up to sign --
    through the eigen-residual ||T s - theta s|| <= 8 k u ||T||; the one-row sweep and the full one give the same theta and the same
    bottom row."""
    a, b = _tridiag_case(k, flavour)
    T = L.tridiag(a, np.append(b, 0.0))
    norm = np.linalg.norm(T, 2)
    want = np.linalg.eigvalsh(T)
    theta, row, S = lam.tridiag_eigen(a, b, vectors=True)
    theta1, row1 = lam.tridiag_eigen(a, b)
    err, res = np.abs(theta - want).max(), np.linalg.norm(T @ S - S * theta, axis=0).max()
    print(f"k={k} {flavour}: |theta - eigvalsh| {err:.2e} (gate {4 * k * U64 * norm:.2e}), residual {res:.2e} (gate {8 * k * U64 * norm:.2e})")
    assert (np.diff(theta) >= 0).all()
    assert err <= 4 * k * U64 * norm
    assert res <= 8 * k * U64 * norm
    assert np.abs(np.linalg.norm(S, axis=0) - 1).max() <= 8 * k * U64
    assert np.array_equal(row, S[k - 1])
    assert np.array_equal(theta1, theta) and np.array_equal(np.abs(row1), np.abs(row))


def test_tridiag_eigen_refuses_bad_input(lam):
    for bad in (np.zeros(0), np.zeros(lam.MAX_LANCZOS + 1)):
        with pytest.raises(lam.LamHipError) as e:
            lam.tridiag_eigen(bad, np.zeros(max(bad.size - 1, 0)))
        assert e.value.code == -1
    with pytest.raises(lam.LamHipError):
        lam.tridiag_eigen([1.0, np.nan], [0.5])
    with pytest.raises(lam.LamHipError):
        lam.tridiag_eigen([1.0, 2.0], [np.inf])


def test_tridiag_header_under_sanitizers(tmp_path):
    """csrc/lam_host_tridiag.h -- the header the product build includes, no HIP in it -- as a stand-alone program with its own main
    under g++ -fsanitize=address,undefined: built and run as an executable, with every output array at exactly its stated size."""
    csrc = os.path.join(ROOT, PKG_NAME, "csrc")
    header = open(os.path.join(csrc, "lam_host_tridiag.h")).read()
    assert "hip_runtime" not in header and "#include <hip" not in header
    assert '#include "lam_host_tridiag.h"' in open(os.path.join(csrc, "lam_kernels.h")).read()
    assert "lam::tridiag_eigen(" in open(os.path.join(csrc, "lam_eigs.h")).read()
    exe = str(tmp_path / "tridiag_asan.out")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", csrc,
                        os.path.join(ROOT, "tests", "host_tridiag", "tridiag_asan_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0 and r.stdout.strip().endswith("ok tridiag"), r.stdout[-2000:] + r.stderr[-2000:]


# ------------------------------------------------------------------------------------------------
# the model is a Lanczos
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", ["F64", "F32"])
def test_the_model_is_a_lanczos(dtype_name):
    """V orthonormal to 16 k u_TV; A V_k = V_k T_k + beta_k v_{k+1} e_k^T to rounding (k u_TV ||A|| per column: every column carries
    the roundings of one product and of 2 (k + 1) Gram-Schmidt updates that T does not fold in); every Ritz pair has an eigenvalue
    within its residual plus an fp64 floor."""
    dtype = D.DTYPES[dtype_name]
    u = L.UNIT_ROUNDOFF[dtype]
    n, k = 384, 40
    A = D.parity_matrix(n, dtype_name)
    _, _, v0 = D.parity_inputs(n)
    run = L.lanczos(A, v0, k, dtype, "rows", nev=4, which=L.BOTH, tol=0.0, check_every=k)
    assert run["steps"] == k and not run["broke"]
    V = run["V"].astype(np.float64)
    orth = np.abs(V @ V.T - np.eye(k + 1)).max()
    T = L.tridiag(run["alpha"], run["beta"])
    R = A @ V[:k].T - V[:k].T @ T
    R[:, k - 1] -= run["beta"][k - 1] * V[k]
    norm = np.linalg.norm(A, 2)
    rel = np.linalg.norm(R, axis=0).max() / norm
    print(f"{dtype_name}: |V V^T - I| {orth:.2e} (gate {16 * k * u:.2e}); |A V - V T - beta v e^T| / |A| {rel:.2e} (gate {4 * k * u:.2e})")
    assert orth <= 16 * k * u
    assert rel <= 4 * k * u
    ev = np.linalg.eigvalsh(A)
    Y = L.ritz_vectors(run)
    for theta, y in zip(run["theta"], Y):
        rho = np.linalg.norm(A @ y - theta * y) / np.linalg.norm(y)
        assert np.abs(ev - theta).min() <= rho + n * U64 * norm, (theta, rho)


@pytest.mark.parametrize("which", [L.SMALLEST, L.LARGEST, L.BOTH], ids=["smallest", "largest", "both"])
@pytest.mark.parametrize("dtype_name", ["F64", "F32"])
def test_the_model_converges_inside_the_gpu_tests_step_cap(dtype_name, which):
    """On the known-spectrum system the model alone converges the wanted pairs well inside max_steps, finds the extreme
    eigenvalues, and its own residuals meet rho <= bound + 8 N u_TV ||A|| -- so the constant 8 stands for the GPU test."""
    run = D.known_run(dtype_name, which)
    A = D.known_matrix(dtype_name)
    ev = np.linalg.eigvalsh(A)
    norm = np.abs(ev).max()
    assert run["all_converged"] and not run["broke"] and run["steps"] <= D.KNOWN_MAX_STEPS // 2, (run["steps"], run["converged"])
    idx = L.wanted(which, D.KNOWN_NEV, D.KNOWN_N, D.KNOWN_NEV)
    floor = D.residual_floor(D.KNOWN_N, dtype_name, norm)
    Y = L.ritz_vectors(run)
    for i, (theta, bound, y) in enumerate(zip(run["theta"], run["bound"], Y)):
        rho = np.linalg.norm(A @ y - theta * y) / np.linalg.norm(y)
        print(f"{dtype_name} which={which} pair {i}: theta {theta:.12g} bound {bound:.2e} rho {rho:.2e} floor {floor:.2e} steps {run['steps']}")
        assert abs(ev[idx[i]] - theta) <= rho + D.KNOWN_N * U64 * norm
        assert rho <= bound + floor


def test_the_model_breaks_down_on_an_invariant_subspace():
    """diag(1..65), v0 = e_1 + e_2 + e_3: three steps, theta = {1, 2, 3}, no fourth basis vector."""
    n = 65
    v0 = np.zeros(n)
    v0[:3] = 1.0
    for dtype in (np.float64, np.float32):
        run = L.lanczos(np.diag(np.arange(1.0, n + 1)), v0, 32, dtype, "rows", nev=4, tol=1e-10, check_every=8)
        assert run["broke"] and run["steps"] == 3 and run["nfound"] == 3 and len(run["V"]) == 3
        assert np.abs(run["theta"] - [1, 2, 3]).max() <= 64 * L.UNIT_ROUNDOFF[dtype] * 3


# ------------------------------------------------------------------------------------------------
# gates
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", ["F64", "F32"])
@pytest.mark.parametrize("n", D.PARITY_SIZES)
def test_the_coefficient_gates_are_ten_times_the_models_own_spread(n, dtype_name):
    """lanczos_data.COEFF_GATE re-measured: per checked step the largest relative spread of alpha and beta between the model's three
    sum orders.  The gate is 10 x what was measured when the table was written; here the spread must lie between a hundredth and three
    tenths of the gate (tests/test_minres_cpu.py's rule), and no checked step is beyond the 1e-2 where gating stops."""
    sp = D.measure_coefficient_spreads(n, dtype_name)
    gate = D.COEFF_GATE[(n, dtype_name)]
    assert tuple(sorted(gate)) == D.PARITY_K
    for k in D.PARITY_K:
        print(f"n={n} {dtype_name} k={k}: spread {sp[k]:.2e}, gate {gate[k]:.1e}")
        assert sp[k] <= D.UNGATED_ABOVE
        assert 0.01 * gate[k] <= sp[k] <= 0.3 * gate[k], (k, sp[k], gate[k])


# ------------------------------------------------------------------------------------------------
# presence
# ------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("lam_hip_eigs", "lam_hip_get_lanczos", "lam_hip_get_eigenvectors", "lam_hip_eig_residuals", "lam_hip_project_out",
               "lam_hip_tridiag_eigen")


def test_every_layer_carries_the_new_names(lam):
    import ctypes as C
    header = open(os.path.join(ROOT, "include", "lam_hip.h")).read()
    for name in NEW_SYMBOLS + ("LAM_HIP_MAX_LANCZOS 256", "LAM_HIP_EIG_SMALLEST 0", "LAM_HIP_EIG_LARGEST  1", "LAM_HIP_EIG_BOTH     2"):
        assert name in header, name
    lib = C.CDLL(lam.lib_path())
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in lam.lib()._lam_symbols, name
    for member in ("eigs", "eigenvectors", "eig_residuals", "lanczos_coefficients", "project_out"):
        assert callable(getattr(lam.Solver, member)), member
    assert callable(lam.tridiag_eigen) and lam.MAX_LANCZOS == 256
    cls = open(os.path.join(ROOT, PKG_NAME, "LAM", "src", "HIP", "ConjugateGradient_HIP_base.hpp")).read()
    for member in ("bool eigs(", "bool get_eigenvectors(", "bool eig_residuals(", "bool get_lanczos("):
        assert member in cls, member
    driver = open(os.path.join(ROOT, PKG_NAME, "test", "test_CG_multi_rhs.cpp")).read()
    assert "-E nev" in driver and "-W s|l|b" in driver and "E:W:" in driver
