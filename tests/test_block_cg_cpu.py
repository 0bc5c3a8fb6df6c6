"""Block CG for the batch without a GPU: the s x s routines through the C ABI (lam_hip_block_factor) and under sanitizers, the numpy
model tests/block_cg_reference.py against what it claims, the gates and margins tests/test_gpu_block_cg.py holds the device to
(tests/block_cg_data.py), and the presence of the new names in every layer."""
import os
import subprocess

import numpy as np
import pytest

import block_cg_data as D
import block_cg_reference as R
from conftest import ROOT, PKG_NAME

F = {"F64": 0, "F32": 1}        # include/lam_hip.h LAM_HIP_F64 / LAM_HIP_F32
U = {"F64": 2.0 ** -53, "F32": 2.0 ** -24}


def _refused(lam, G, dtype=0):
    with pytest.raises(lam.LamHipError) as e:
        lam.block_factor(G, dtype)
    assert e.value.code == -1
    return e.value.bad_col, str(e.value)


# ------------------------------------------------------------------------------------------------
# lam_hip_block_factor
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", ["F64", "F32"])
def test_block_factor_is_exact_on_powers_of_two(lam, dtype_name):
    """s = 1 and s = 8.  A diagonal of powers of four: every square root and quotient is exact.  G = S^T S with S upper triangular,
    small integers off and powers of two on the diagonal: the upper factor and S^-1 come back exactly, and so does G^-1 = S^-1 S^-T."""
    assert all(np.array_equal(m, [[w]]) for m, w in zip(lam.block_factor([[0.25]], F[dtype_name]), (4.0, 0.5, 2.0)))
    d = 4.0 ** np.array([0, 1, -1, 2, -2, 3, 0, 1])
    Gi, S, Si = lam.block_factor(np.diag(d), F[dtype_name])
    assert np.array_equal(Gi, np.diag(1 / d)) and np.array_equal(S, np.diag(np.sqrt(d))) and np.array_equal(Si, np.diag(1 / np.sqrt(d)))
    rng = np.random.default_rng(4)
    S0 = np.triu(rng.integers(-2, 3, (8, 8)).astype(np.float64), 1) + np.diag(2.0 ** rng.integers(0, 3, 8))
    G = S0.T @ S0
    Si0 = np.linalg.inv(S0)
    assert np.array_equal(Si0 * 2 ** 40, np.round(Si0 * 2 ** 40))            # S^-1 is a matrix of dyadic fractions
    Gi, S, Si = lam.block_factor(G, F[dtype_name])
    assert np.array_equal(S, S0) and np.array_equal(Si, Si0)
    assert np.array_equal(Gi, Gi.T) and np.allclose(Gi, Si0 @ Si0.T, rtol=0, atol=1e-12 * np.abs(Si0 @ Si0.T).max())
    # only the upper triangle is read
    G2 = G.copy()
    G2[5, 1] = 1e9
    assert all(np.array_equal(a, b) for a, b in zip(lam.block_factor(G2, F[dtype_name]), (Gi, S, Si)))


@pytest.mark.parametrize("s", D.FACTOR_SIZES)
def test_block_factor_against_numpy_and_the_model(lam, s):
    G = D.factor_case(s)
    gate = D.factor_gate(G)
    Gi, S, Si = lam.block_factor(G)
    want = (np.linalg.inv(G), np.linalg.cholesky(G).T, np.linalg.inv(np.linalg.cholesky(G).T))
    for name, got, ref in zip(("Ginv", "S", "Sinv"), (Gi, S, Si), want):
        err = np.abs(got - ref).max() / np.abs(ref).max()
        print(f"s={s} {name}: {err:.2e}, gate {gate:.2e}")
        assert err <= gate
    assert np.array_equal(Gi, Gi.T) and np.array_equal(S, np.triu(S)) and np.array_equal(Si, np.triu(Si))
    # the model restates the routines statement by statement
    floor = R.pivot_floor(G, np.float64)
    assert np.array_equal(R.ldlt_inverse(G, floor)[0], Gi)
    assert np.array_equal(R.upper(G, floor)[0], S) and np.array_equal(R.upper(G, floor)[1], Si)


@pytest.mark.parametrize("s", D.FACTOR_SIZES)
@pytest.mark.parametrize("dtype_name", ["F64", "F32"])
def test_block_factor_pivot_rule_at_the_threshold(lam, dtype_name, s):
    """The last pivot of diag(1, ..., 1, x) is x itself (s = 1: of diag(x) next to nothing, so the floor is s u x < x and only a
    zero fails): it fails at x = s u exactly (<=) and passes one ulp above, for the unit roundoff of `dtype`."""
    u = U[dtype_name]
    if s == 1:
        assert _refused(lam, [[0.0]], F[dtype_name])[0] == 0
        assert lam.block_factor([[2.0 ** -900]], F[dtype_name])[0][0, 0] == 2.0 ** 900
        return
    d = np.ones(s)
    d[-1] = s * u
    assert _refused(lam, np.diag(d), F[dtype_name])[0] == s - 1
    d[-1] = np.nextafter(s * u, 1.0)
    Gi, S, Si = lam.block_factor(np.diag(d), F[dtype_name])
    assert Gi[-1, -1] == 1.0 / d[-1] and S[-1, -1] == np.sqrt(d[-1])
    if dtype_name == "F64":          # the fp32 rule refuses what the fp64 rule takes
        d[-1] = s * U["F32"]
        lam.block_factor(np.diag(d), F["F64"])
        assert _refused(lam, np.diag(d), F["F32"])[0] == s - 1


def test_block_factor_refusals_name_the_column(lam):
    X = np.random.default_rng(1).uniform(-1, 1, (9, 8))
    X[:, 6] = X[:, 2]
    bad, msg = _refused(lam, X.T @ X)
    assert bad == 6 and "column 6" in msg                             # a duplicated column: the later one's pivot
    G = D.factor_case(8)
    nan = G.copy()
    nan[5, 5] = np.nan
    assert _refused(lam, nan)[0] == 5
    off = G.copy()
    off[2, 4] = np.nan
    assert _refused(lam, off)[0] == 4                                 # an off-diagonal NaN reaches the pivot of its column
    assert _refused(lam, [[np.nan]])[0] == 0 and _refused(lam, [[np.inf]])[0] == 0 and _refused(lam, [[-1.0]])[0] == 0
    assert _refused(lam, np.eye(lam.MAX_RHS + 1))[0] == -1            # s out of range
    assert _refused(lam, np.eye(2), 2)[0] == -1                       # BF16 has no rule
    assert "outside 1..8" in _refused(lam, np.zeros((0, 0)))[1]


def test_block_header_under_sanitizers(tmp_path):
    """csrc/lam_host_block.h -- the header the product build includes and its kernels call, no HIP in it -- as a stand-alone program
    with its own main under g++ -fsanitize=address,undefined: built and run as an executable, every matrix at exactly its size."""
    csrc = os.path.join(ROOT, PKG_NAME, "csrc")
    header = open(os.path.join(csrc, "lam_host_block.h")).read()
    assert "hip_runtime" not in header and "#include <hip" not in header
    kernels = open(os.path.join(csrc, "lam_kernels.h")).read()
    assert '#include "lam_host_block.h"' in kernels and "block_ldlt_inverse(s, s_h" in kernels and "block_upper(s, s_g" in kernels
    assert "lam::block_upper(" in open(os.path.join(csrc, "lam_block.h")).read()
    exe = str(tmp_path / "block_asan.out")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", csrc,
                        os.path.join(ROOT, "tests", "host_block", "block_asan_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0 and r.stdout.strip().endswith("ok block"), r.stdout[-2000:] + r.stderr[-2000:]


# ------------------------------------------------------------------------------------------------
# the model is a block CG, and the gates are what it shows
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", ["F64", "F32"])
@pytest.mark.parametrize("nrhs", [2, 4, 8])
def test_model_needs_fewer_iterations_than_independent_cg(dtype_name, nrhs):
    """On the data module's system the block converges in fewer iterations than the fastest of the same columns alone, to a true
    residual under the gate the device is held to."""
    m = D.model(D.POINT_N, nrhs, dtype_name)
    plain = D.plain_counts(D.POINT_N, nrhs, dtype_name)
    print(f"N={D.POINT_N} {dtype_name} nrhs={nrhs}: block {m['info']['iters']}, independent {plain}")
    assert m["info"]["converged"].all() and m["info"]["breakdown"] == (0, 0)
    assert (plain <= D.MAX_ITERS).all() and m["info"]["iters"] < plain.min()
    assert m["true"].max() < D.REL_ERROR[dtype_name]
    assert (m["info"]["num_iters"] <= m["info"]["iters"]).all() and m["info"]["num_iters"].max() == m["info"]["iters"]


def test_model_with_one_column_is_cg():
    """s = 1: block CG is CG; the model's two statements of it agree to within the iteration gate."""
    for dtype_name in ("F64", "F32"):
        for n in (65, 2049):
            assert abs(D.model(n, 1, dtype_name)["info"]["iters"] - D.plain_counts(n, 1, dtype_name)[0]) <= D.iter_gate(n, 1, dtype_name)


@pytest.mark.parametrize("n", D.SIZES)
def test_recorded_figures_are_what_the_model_shows(n):
    """Every (nrhs, dtype) at this size over the model's sum orders against block_cg_data.RECORDED: the rows-order run's iterations
    and breakdown, the spread of the iteration count, the largest true residual (recorded rounded up in its third digit); the kind
    of ending is the same in every order, and a run ends converged, or in breakdown kind 2 (the block Krylov space is full), or
    refused (nrhs > N)."""
    for dtype_name in ("F64", "F32"):
        for nrhs in D.NRHS:
            if nrhs > n:
                assert D.model(n, nrhs, dtype_name)["info"]["refused"] == n and (n, dtype_name, nrhs) not in D.RECORDED
                continue
            m = D.measure(n, nrhs, dtype_name)
            iters, bd, spread, true = D.RECORDED[(n, dtype_name, nrhs)]
            print(f"N={n} {dtype_name} nrhs={nrhs}: {m}")
            assert (m["iters"], m["breakdown"], m["spread"]) == (iters, bd, spread)
            assert len(m["kinds"]) == 1 and m["kinds"] <= {0, 2}
            assert 0.98 * true <= m["true"] <= true
            assert D.iter_gate(n, nrhs, dtype_name) == spread + 1


@pytest.mark.parametrize("n", sorted(D.PRECISION_GAP))
def test_true_residual_margin_is_the_models_precision_gap(n):
    gap = D.measure_precision_gap(n)
    print(f"N={n}: fp32 against fp64 arithmetic, true residual formed in fp32: largest ratio {gap:.3f}; recorded {D.PRECISION_GAP[n]}")
    assert 0.9 * D.PRECISION_GAP[n] <= gap <= D.PRECISION_GAP[n]
    assert D.true_gate(n, 1, "F32") == D.PRECISION_GAP[n] * D.RECORDED[(n, "F32", 1)][3]
    assert D.true_gate(65537, 8, "F64") == D.PRECISION_GAP[2049] * D.RECORDED[(65537, "F64", 8)][3]


def test_model_reports_exact_convergence_and_the_rank_deficient_block():
    """A = diag of powers of four, B = scaled unit vectors: converged at k = 1 with rel_err 0; the same with rel_error = 0: breakdown
    (1, 2) and the same X.  A duplicated column is refused naming it."""
    n = 33
    d = 4.0 ** (np.arange(n) % 4 - 1)
    B = np.zeros((3, n))
    B[0, 5], B[1, 17], B[2, 30] = 2.0, 0.5, 8.0
    ap = lambda P: d[:, None] * P
    for dtype in (np.float64, np.float32):
        X, info = R.block_cg(ap, B, 10, 1e-6, dtype)
        assert info["iters"] == 1 and info["breakdown"] == (0, 0) and (info["rel_err"] == 0).all() and info["converged"].all()
        assert np.array_equal(X, B / d)
        X0, info0 = R.block_cg(ap, B, 10, 0.0, dtype)
        assert info0["breakdown"] == (1, 2) and np.array_equal(X0, X) and not info0["converged"].any()
        dup = B.copy()
        dup[2] = B[0]
        assert R.block_cg(ap, dup, 10, 1e-6, dtype)[1]["refused"] == 2


# ------------------------------------------------------------------------------------------------
# every layer names the feature
# ------------------------------------------------------------------------------------------------
def test_every_layer_names_block_cg(lam):
    assert {"lam_hip_solve_block", "lam_hip_block_factor"} <= set(lam.lib()._lam_symbols)
    assert hasattr(lam.Solver, "solve_block") and callable(lam.block_factor)
    pkg = os.path.join(ROOT, PKG_NAME)
    header = open(os.path.join(ROOT, "include", "lam_hip.h")).read()
    assert "int lam_hip_solve_block(" in header and "int lam_hip_block_factor(" in header
    assert "lam_hip_solve_block and lam_hip_block_factor" in header       # the ABI history
    assert "solve_block" in open(os.path.join(pkg, "LAM", "src", "HIP", "ConjugateGradient_HIP_base.hpp")).read()
    assert "'B'" in open(os.path.join(pkg, "test", "test_CG_multi_rhs.cpp")).read()
    assert os.path.exists(os.path.join(ROOT, "tools", "block_probe.py"))
    assert "§17" in open(os.path.join(ROOT, "DESIGN.md")).read() and "lam_hip_solve_block" in open(os.path.join(ROOT, "README.md")).read()
