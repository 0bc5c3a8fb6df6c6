"""Block CG for the batch on the device (lam_hip_solve_block), held to exact known answers, to the numpy model
tests/block_cg_reference.py and to the plain batch of the same build.  Systems, gates and margins: tests/block_cg_data.py,
established without a GPU by tests/test_block_cg_cpu.py."""
import os
import subprocess

import numpy as np
import pytest

import block_cg_data as D
from conftest import ROOT, PKG_NAME

pytestmark = pytest.mark.gpu

NP = D.DTYPES
EINVAL, ESTATE = -1, -6


def _refused(lam, code, call, *args, **kw):
    with pytest.raises(lam.LamHipError) as e:
        call(*args, **kw)
    assert e.value.code == code, e.value
    return str(e.value)


def _solver(lam, n, dtype_name, symmetric_many=0):
    eig, V, _ = D.system(n)
    s = lam.Solver(getattr(lam, dtype_name))
    s.generate_spectrum_spd(eig, V)
    s.set_option("symmetric_many", symmetric_many)
    return s


# ------------------------------------------------------------------------------------------------
# 1. exact known answers: A = diag of powers of four, B = scaled distinct unit vectors
# ------------------------------------------------------------------------------------------------
EXACT_N = 2049
EXACT_ROWS = (6, 77, 1028, 2048, 0, 513, 1500, 255)          # rows of different workgroups, the first and the last row
EXACT_SCALES = (2.0, 0.5, 8.0, 1.0, 4.0, 0.25, 16.0, 2.0)


@pytest.mark.parametrize("nrhs", [1, 3, 8])
@pytest.mark.parametrize("dtype_name", ["F64", "F32"])
def test_exact_known_answers(lam, dtype_name, nrhs):
    """Every square root and quotient is exact: C = diag(scales), Q = P = the unit vectors, H = diag(a), X = B / a, Q~ = 0.
    Converged at k = 1 with X exact bit for bit, rel_err = 0 and no breakdown; with rel_error = 0 the same X and breakdown (1, 2)."""
    n = EXACT_N
    a = 4.0 ** (np.arange(n) % 4 - 1)
    B = np.zeros((nrhs, n))
    for j in range(nrhs):
        B[j, EXACT_ROWS[j]] = EXACT_SCALES[j]
    want = (B / a).astype(NP[dtype_name])
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.set_matrix(np.diag(a))
        s.set_rhs_many(B)
        ni, cv, re, bd = s.solve_block(50, 1e-6)
        assert bd == (0, 0) and cv.all() and (ni == 1).all() and (re == 0).all() and s.stats["num_iters"] == 1 and s.stats["converged"]
        X = s.solutions()
        assert X.tobytes() == want.tobytes()
        assert (s.true_residuals() == 0).all()
        ni, cv, re, bd = s.solve_block(50, 0.0)
        assert bd == (1, 2) and not cv.any() and (ni == 51).all() and (re == 0).all() and s.stats["num_iters"] == 1
        assert s.solutions().tobytes() == want.tobytes()
        ni, cv, re, bd = s.solve_block(0, 1e-6)
        assert bd == (0, 0) and (ni == 1).all() and (re == 1).all() and not cv.any() and not s.solutions().any()
        _refused(lam, EINVAL, s.solve_block, -1, 1e-6)


@pytest.mark.parametrize("bad", [0, 2])
@pytest.mark.parametrize("dtype_name", ["F64", "F32"])
def test_breakdown_kind_one_leaves_x_alone(lam, dtype_name, bad):
    """A singular A met exactly: A = diag of powers of four with one zero, and column `bad` of B is that unit vector, so
    P^T A P = diag(.., 0, ..) exactly and the pivot of column `bad` fails in iteration 1: breakdown (1, 1), no iteration completed,
    X stays iterate 0, rel_err the start's.  The same matrix without that column converges at k = 1 as ever."""
    n = EXACT_N
    a = 4.0 ** (np.arange(n) % 4 - 1)
    a[EXACT_ROWS[bad]] = 0.0
    B = np.zeros((3, n))
    for j in range(3):
        B[j, EXACT_ROWS[j]] = EXACT_SCALES[j]
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.set_matrix(np.diag(a))
        s.set_rhs_many(B)
        ni, cv, re, bd = s.solve_block(50, 1e-6)
        assert bd == (1, 1) and not cv.any() and (ni == 51).all() and (re == 1).all()
        assert s.stats["num_iters"] == 0 and not s.stats["converged"]
        assert not s.solutions().any()
        keep = [j for j in range(3) if j != bad]
        s.set_rhs_many(B[keep])
        ni, cv, re, bd = s.solve_block(50, 1e-6)
        assert bd == (0, 0) and cv.all() and (ni == 1).all()
        with np.errstate(divide="ignore", invalid="ignore"):
            want = np.where(B[keep] != 0, B[keep] / a, 0.0).astype(NP[dtype_name])
        assert s.solutions().tobytes() == want.tobytes()


# ------------------------------------------------------------------------------------------------
# 2. against the model
# ------------------------------------------------------------------------------------------------
def _check_against_model(s, n, nrhs, dtype_name):
    """One case against what the model recorded for it (block_cg_data.RECORDED); None where the model's block is refused."""
    tol = D.REL_ERROR[dtype_name]
    s.set_rhs_many(D.system(n)[2][:nrhs])
    if nrhs > n:
        return None
    m_iters, m_bd, _, m_true = D.RECORDED[(n, dtype_name, nrhs)]
    ni, cv, re, bd = s.solve_block(D.MAX_ITERS, tol)
    iters = s.stats["num_iters"]
    true = s.true_residuals()
    gate, gate_k = D.true_gate(n, nrhs, dtype_name), D.iter_gate(n, nrhs, dtype_name)
    print(f"N={n} {dtype_name} nrhs={nrhs}: device {iters} iterations, breakdown {bd}; model {m_iters}, {m_bd}, gate +-{gate_k}; "
          f"true residual {true.max():.3e}, model {m_true:.3e}, gate {gate:.3e}")
    assert abs(iters - m_iters) <= gate_k
    assert bd[1] == m_bd[1] and abs(bd[0] - m_bd[0]) <= gate_k
    assert (true <= gate).all()
    # num_iters, converged and rel_err are consistent with each other
    assert (cv == (re < tol)).all() and bool(s.stats["converged"]) == bool(cv.all()) == (bd == (0, 0))
    assert ((ni <= iters) | (ni == D.MAX_ITERS + 1)).all() and (ni[cv] <= iters).all()
    if cv.all():
        assert ni.max() == iters and s.stats["rel_err"] == re.max()
    assert s.get_option("multi_rhs_k") == (1 if nrhs == 1 else 2 if nrhs == 2 else 4 if nrhs <= 4 else 8)
    return iters


@pytest.mark.parametrize("dtype_name", ["F64", "F32"])
@pytest.mark.parametrize("n", D.SIZES)
def test_block_follows_the_model(lam, n, dtype_name):
    """Every nrhs of the data module on one matrix: iteration counts within the iteration gate, true residuals under the true-residual
    gate, the same kind of ending as the model (converged; breakdown kind 2 where the block Krylov space fills the whole space;
    refused where nrhs > N)."""
    with _solver(lam, n, dtype_name) as s:
        for nrhs in D.NRHS:
            if _check_against_model(s, n, nrhs, dtype_name) is None:
                assert f"column {n}" in _refused(lam, EINVAL, s.solve_block, D.MAX_ITERS, D.REL_ERROR[dtype_name])


def _launches_per_iteration(s):
    """Capped runs that cannot stop early (rel_error = 0, far from a full block Krylov space): the launches of 7 against 3 iterations."""
    counts = {}
    for iters in (3, 7):
        l0 = s.get_option("hip_calls_launch")
        s.solve_block(iters, 0.0)
        assert s.breakdown == (0, 0) and s.stats["num_iters"] == iters
        counts[iters] = s.get_option("hip_calls_launch") - l0
    assert (counts[7] - counts[3]) % 4 == 0
    return (counts[7] - counts[3]) // 4


@pytest.mark.parametrize("dtype_name", ["F64", "F32"])
@pytest.mark.parametrize("n", [65, 2049])
def test_block_under_the_symmetric_product(lam, n, dtype_name):
    """Option symmetric_many = 2 at K <= 4: the same gates, five launches per iteration, and the option reads effective."""
    with _solver(lam, n, dtype_name, symmetric_many=2) as s:
        for nrhs in (1, 2, 3):
            _check_against_model(s, n, nrhs, dtype_name)
            assert s.get_option("symmetric_many_effective") == 1
            assert _launches_per_iteration(s) == 5


@pytest.mark.parametrize("dtype_name", ["F64", "F32"])
def test_one_column_is_cg(lam, dtype_name):
    n = D.POINT_N
    with _solver(lam, n, dtype_name) as s:
        s.set_rhs_many(D.system(n)[2][:1])
        s.solve_block(D.MAX_ITERS, D.REL_ERROR[dtype_name])
        block = s.stats["num_iters"]
        s.solve_many(D.MAX_ITERS, D.REL_ERROR[dtype_name])
        assert abs(block - int(s.num_iters_many[0])) <= D.iter_gate(n, 1, dtype_name)


@pytest.mark.parametrize("nrhs", [2, 4, 8])
@pytest.mark.parametrize("dtype_name", ["F64", "F32"])
def test_block_needs_fewer_iterations_than_the_batch(lam, dtype_name, nrhs):
    """The point of the feature: fewer iterations than the fastest column of lam_hip_solve_many in the same build, every one of
    them one pass over the matrix; four launches per iteration; the single-vector state is untouched."""
    n, tol = D.POINT_N, D.REL_ERROR[dtype_name]
    with _solver(lam, n, dtype_name) as s:
        b1 = np.ones(n)
        s.set_rhs(b1)
        s.solve(3, 0.0)
        x1 = s.solution().copy()
        s.set_rhs_many(D.system(n)[2][:nrhs])
        s.solve_many(D.MAX_ITERS, tol)
        plain = s.num_iters_many.copy()
        assert s.converged_many.all()
        ni, cv, re, bd = s.solve_block(D.MAX_ITERS, tol)
        block = s.stats["num_iters"]
        print(f"N={n} {dtype_name} nrhs={nrhs}: block {block}, independent {plain}")
        assert cv.all() and bd == (0, 0) and block < plain.min()
        assert s.stats["gemv_bytes"] > 0 and s.stats["t_total"] > 0
        X = s.solutions()
        assert X.shape == (nrhs, n) and np.isfinite(X).all()
        assert np.array_equal(s.solution(), x1)
        assert _launches_per_iteration(s) == 4 and s.get_option("symmetric_many_effective") == 0


@pytest.mark.parametrize("dtype_name", ["F64", "F32"])
def test_two_identical_calls_give_identical_bits(lam, dtype_name):
    n = 65537
    with _solver(lam, n, dtype_name) as s:
        s.set_rhs_many(D.system(n)[2][:5])
        first = s.solve_block(D.MAX_ITERS, D.REL_ERROR[dtype_name])
        X = s.solutions()
        second = s.solve_block(D.MAX_ITERS, D.REL_ERROR[dtype_name])
        assert X.tobytes() == s.solutions().tobytes()
        assert all(np.array_equal(a, b) for a, b in zip(first, second))


# ------------------------------------------------------------------------------------------------
# 3. recovery
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", ["F64", "F32"])
def test_recovery_after_the_cap(lam, dtype_name):
    n, nrhs, tol, cap = D.POINT_N, 5, D.REL_ERROR[dtype_name], 6
    with _solver(lam, n, dtype_name) as s:
        s.set_rhs_many(D.system(n)[2][:nrhs])
        ni, cv, re, bd = s.solve_block(cap, tol)
        assert bd == (0, 0) and not cv.all() and s.stats["num_iters"] == cap and (ni[~cv] == cap + 1).all() and (re[~cv] >= tol).all()
        mid = s.true_residuals()
        s.solve_many(D.MAX_ITERS, tol, x0="continue")
        assert s.converged_many.all()
        assert (s.true_residuals() <= D.PRECISION_GAP[n] * tol).all() and (s.true_residuals() < mid).all()
        # the same through fallback=True
        ni, cv, re, bd = s.solve_block(cap, tol, fallback=True, fallback_max_iters=D.MAX_ITERS)
        assert cv.all() and (re < tol).all() and s.fallback_iters is not None and (s.fallback_iters <= D.MAX_ITERS).all()
        assert (s.true_residuals() <= D.PRECISION_GAP[n] * tol).all()
        s.solve_block(D.MAX_ITERS, tol, fallback=True)
        assert s.fallback_iters is None                              # converged: nothing to fall back from


def test_recovery_after_a_breakdown(lam):
    """N = 65 with 8 columns: the block Krylov space is full after 8 iterations (breakdown kind 2, X valid); the continuation
    converges."""
    n, tol = 65, D.REL_ERROR["F64"]
    with _solver(lam, n, "F64") as s:
        s.set_rhs_many(D.system(n)[2][:8])
        ni, cv, re, bd = s.solve_block(D.MAX_ITERS, tol, fallback=True)
        assert s.breakdown[1] == 2 and cv.all() and s.fallback_iters is not None
        assert (s.true_residuals() <= D.PRECISION_GAP[n] * tol).all()


# ------------------------------------------------------------------------------------------------
# 4. refusals
# ------------------------------------------------------------------------------------------------
def test_refusals(lam, monkeypatch):
    n = 130
    rng = np.random.default_rng(3)
    B = rng.uniform(-1, 1, (4, n))
    A = np.diag(np.linspace(1.0, 2.0, n))
    with lam.Solver(lam.F64) as s:
        s.set_problem(n)
        assert "matrix" in _refused(lam, ESTATE, s.solve_block, 10, 1e-6)           # no matrix
        s.set_matrix(A)
        assert "right-hand sides" in _refused(lam, ESTATE, s.solve_block, 10, 1e-6)  # no right-hand sides
        dup = B.copy()
        dup[3] = dup[1]
        s.set_rhs_many(dup)
        assert "column 3" in _refused(lam, EINVAL, s.solve_block, 10, 1e-6)          # a duplicated column
        zero = B.copy()
        zero[2] = 0.0
        s.set_rhs_many(zero)
        assert "column 2" in _refused(lam, EINVAL, s.solve_block, 10, 1e-6)          # a zero column
        _refused(lam, ESTATE, s.solutions)                                          # nothing was iterated
        s.set_rhs_many(B)
        s.set_shifts([0.0, 0.5, 0.0, 0.0])
        assert "shift 1 in force is 0.5" in _refused(lam, EINVAL, s.solve_block, 10, 1e-6)
        s.set_shifts(None)
        s.solve_block(50, 1e-6)
        assert s.converged_many.all() and s.solutions().shape == (4, n)
    with lam.Solver(lam.BF16) as s:
        s.set_matrix(A)
        assert "LAM_HIP_BF16" in _refused(lam, EINVAL, s.solve_block, 10, 1e-6)
    with lam.Solver(lam.F64, device_ids=[0, 0]) as s:
        s.set_matrix(A)
        assert "one shard only" in _refused(lam, EINVAL, s.solve_block, 10, 1e-6)


# ------------------------------------------------------------------------------------------------
# 5. driver
# ------------------------------------------------------------------------------------------------
EXE = os.path.join(ROOT, PKG_NAME, "test", "test_CG_multi_rhs.out")


def _run(*args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, timeout=300)


def test_driver_solves_with_block_cg():
    """tridiag(1, 2, 1), N = 240, 4 columns: independent CG needs N / 2 = 120 iterations, the block at most N / 4 = 60, where its
    Krylov space is the whole space."""
    r = _run("-s", 240, "-k", 4, "-i", 2000, "-e", 1e-9, "-B", "-T")
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [ln.split(",") for ln in r.stdout.strip().splitlines()]
    assert len(rows) == 4 and all(len(f) == 11 for f in rows)
    assert "breakdown = (0, 0)" in r.stderr
    for f in rows:
        assert int(f[0]) == 240 and 0 < int(f[7]) <= 60 and float(f[8]) < 1e-9 and float(f[10]) < 1e-6, f


@pytest.mark.parametrize("extra", [["-J"], ["-w", "3"], ["-S", "0.5"], ["-M"], ["-m"], ["-D", "2"], ["-E", "2"]])
def test_driver_refuses_conflicting_flags(extra):
    r = _run("-s", 64, "-B", *extra)
    assert r.returncode == 1 and "Usage" in r.stderr and r.stdout == "", (extra, r.stderr)
