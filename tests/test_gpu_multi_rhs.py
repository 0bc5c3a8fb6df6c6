"""Several right-hand sides on one matrix: lam_hip_set_rhs_many / solve_many / get_solution_many / gemv_many / gemv_many_only.

nrhs independent CG recurrences share ONE product launch per iteration (the matrix is read once for all of them).  The batched
kernels exist for K = 1, 2, 4, 8 columns (nrhs runs on the smallest K >= nrhs with zero padding columns), 4 rows per 4-wave
workgroup, and stage a 32-KiB tile of the interleaved p vectors: TILE[dtype][K] columns below.

The product is pinned bit for bit on the integer systems of tests/exact_data.py (any summation order is exact there), the first CG
step too; the recurrences against the CPU oracle with the suite's existing gates; independence of the columns, freezing of early
columns and the confinement of NaN columns bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import exact_data as E
from conftest import GOLDEN, ROOT, PKG_NAME

pytestmark = pytest.mark.gpu

DTYPES = ("F64", "F32")
VEC = {"F64": 2, "F32": 4}                          # matrix elements per 16-byte vector
U_TV = {"F64": 2.0 ** -53, "F32": 2.0 ** -24}
GATE = {"F64": 1e-13, "F32": 32 * 2.0 ** -24}       # the suite's GEMV gates, relative to |A| |x|
TOL = {"F64": 1e-9, "F32": 1e-5}
ITER_GATE = {"F64": lambda ref: max(3, 0.02 * ref), "F32": lambda ref: max(3, 0.05 * ref)}
# column-tile sizes of multi_gemv_kernel (csrc/lam_kernels.h, multi_tile): 32 KiB of LDS whatever K
TILE = {"F64": {1: 4096, 2: 2048, 4: 1024, 8: 512}, "F32": {1: 4096, 2: 4096, 4: 2048, 8: 1024}}
K_FOR = {1: 1, 2: 2, 3: 4, 4: 4, 5: 8, 6: 8, 7: 8, 8: 8}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _smoke_system(n=512, seed=0, spread=2.0):
    """The 512 x 512 system of __graft_entry__.smoke (cond ~ 55) with its eigenvectors."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.uniform(-1, 1, (n, n)))
    A = (q * np.exp(spread * rng.uniform(-1, 1, n))) @ q.T
    return 0.5 * (A + A.T), q, rng


def _edge_sizes(dtype_name):
    V = VEC[dtype_name]
    sizes = set(range(1, 2 * V + 2))
    for base in (64 * V, 64 * V * 4, 64 * V * 8):                      # a wave step, a 4- and an 8-wave super-step
        sizes |= {base + d for d in (-V, -1, 0, 1, V)}
    for T in set(TILE[dtype_name].values()):                           # every column tile of the batched kernels
        sizes |= {T - 1, T, T + 1, T + V, 2 * T + 1}
    sizes |= {4095, 4096, 4097, 10001}
    return sorted(sizes)


# ------------------------------------------------------------------------------------------------
# 1. product, exact
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_gemv_many_exact_at_edges(lam, dtype_name):
    """Y = A X bit for bit, every nrhs in 1..8, at the structural edges of every instantiation."""
    with lam.Solver(getattr(lam, dtype_name)) as s:
        assert s.get_option("multi_rhs_k") == 0
        for n in _edge_sizes(dtype_name):
            X = [E.int_vec(n, 100 * n + j) for j in range(8)]
            s.set_problem(n)
            Y = E.generate(n, [s.upload_rows], X)
            for nrhs in range(1, 9):
                got = s.gemv_many(np.stack(X[:nrhs]))
                want = np.stack(Y[:nrhs]).astype(s.vec_dtype)
                assert s.get_option("multi_rhs_k") == K_FOR[nrhs]
                bad = np.argwhere(got != want)
                assert bad.size == 0, f"{dtype_name} n={n} nrhs={nrhs}: {len(bad)} entries wrong, first (column, row) {bad[:6].tolist()}"


@pytest.mark.parametrize("n", [1001, 6150])
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_gemv_many_nonfinite_entries_propagate(lam, dtype_name, n):
    """+Inf in the last VEC columns of some rows (what the lanes past a ragged tile's end would meet), -Inf and NaN elsewhere:
    every column's rows have the IEEE class of a plain fp64 product and sum; finite rows keep the gate."""
    V = VEC[dtype_name]
    rng = np.random.default_rng(n + 17)
    A = rng.uniform(-1, 1, (n, n))
    for i in (5, n // 2, n - V - 3):
        A[i, n - V:] = np.inf
    A[7, 0] = -np.inf
    A[11, n // 3] = np.nan

    def row_class(y):
        return np.where(np.isnan(y), 3, np.where(np.isposinf(y), 1, np.where(np.isneginf(y), 2, 0)))

    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.set_matrix(A)
        A_dev = A.astype(s.mat_host_dtype).astype(np.float64)
        for nrhs in (1, 2, 3, 8):
            X = rng.uniform(0.5, 1.0, (nrhs, n)).astype(s.vec_dtype)
            Y = s.gemv_many(X).astype(np.float64)
            for j in range(nrhs):
                x64 = X[j].astype(np.float64)
                with np.errstate(invalid="ignore"):
                    want = (A_dev * x64).sum(axis=1)
                cls = row_class(want)
                fin = cls == 0
                assert set(cls) == {0, 1, 2, 3}
                got = row_class(Y[j])
                bad = np.flatnonzero(got != cls)
                assert bad.size == 0, (dtype_name, n, nrhs, j, bad[:8], got[bad[:8]], cls[bad[:8]])
                scale = np.abs(A_dev[fin]) @ np.abs(x64)
                assert np.max(np.abs(Y[j][fin] - want[fin]) / scale) <= GATE[dtype_name], (dtype_name, n, nrhs, j)


# ------------------------------------------------------------------------------------------------
# 2. product, precision
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_gemv_many_dense_random(lam, dtype_name):
    n = 8193
    rng = np.random.default_rng(n)
    A = rng.uniform(-1, 1, (n, n))
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.set_matrix(A)
        A_dev = A.astype(s.mat_host_dtype).astype(np.float64)
        for nrhs in (1, 2, 4, 7, 8):
            X = rng.uniform(-1, 1, (nrhs, n)).astype(s.vec_dtype)
            Y = s.gemv_many(X).astype(np.float64)
            X64 = X.astype(np.float64)
            err = np.max(np.abs(Y - X64 @ A_dev.T) / (np.abs(X64) @ np.abs(A_dev).T))
            assert err <= GATE[dtype_name], (dtype_name, nrhs, err)


# ------------------------------------------------------------------------------------------------
# 3. first step, exact
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1025, 10001])
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_first_step_exact(lam, dtype_name, n):
    """solve_many(1, 1e-30) from x = 0: every column's x is fl(alpha_TV b) bit for bit, alpha = fl64(b.b / b.Ab): K sets of b.b,
    K sets of thousands of p.Ap partials and the x update; rel_err within exact_data.rel_err_bound."""
    with lam.Solver(getattr(lam, dtype_name)) as s:
        vdt = s.vec_dtype
        B = [E.int_vec(n, 7 * n + j) for j in range(8)]
        s.set_problem(n)
        AB = E.generate(n, [s.upload_rows], B)
        for nrhs in (1, 3, 8):
            s.set_rhs_many(np.stack(B[:nrhs]))
            conv = s.solve_many(1, 1e-30)
            X = s.solutions()
            assert not conv.any() and list(s.num_iters_many) == [2] * nrhs and s.stats["num_iters"] == 2
            for j in range(nrhs):
                alpha, x1, bb, pAp, r1 = E.first_cg_step(B[j], AB[j], vdt)
                x1 = x1 + vdt(0)
                bad = np.flatnonzero(_bits(X[j]) != _bits(x1))
                assert bad.size == 0, f"{dtype_name} n={n} nrhs={nrhs} column {j}: x1 differs in {bad.size} entries (alpha {alpha!r}, b.b {bb}, p.Ap {pAp})"
                re_host, bound = E.rel_err_bound(B[j], AB[j], alpha, r1, bb, U_TV[dtype_name])
                assert abs(s.rel_err_many[j] - re_host) <= bound, (dtype_name, n, nrhs, j, s.rel_err_many[j], re_host, bound)


# ------------------------------------------------------------------------------------------------
# 4. columns are independent of slot and neighbours
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_columns_independent_of_slot_and_neighbours(lam, dtype_name):
    A, _, rng = _smoke_system()
    n = A.shape[0]
    b = rng.uniform(-1, 1, n)
    tol = TOL[dtype_name]
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.set_matrix(A)
        s.set_rhs_many(np.tile(b, (8, 1)))
        assert s.solve_many(2000, tol).all()
        X, it, re = s.solutions(), s.num_iters_many, s.rel_err_many
        for j in range(1, 8):
            assert np.array_equal(_bits(X[j]), _bits(X[0])) and it[j] == it[0] and re[j] == re[0], (dtype_name, j)
        res = []
        for slot, seed in ((2, 5), (6, 9)):
            B = np.random.default_rng(seed).uniform(-1, 1, (8, n)) * np.array([1, 3, 1, 0.01, 100, 1, 1, 7])[:, None]
            B[slot] = b
            s.set_rhs_many(B)
            s.solve_many(2000, tol)
            res.append((s.solutions()[slot], s.num_iters_many[slot], s.rel_err_many[slot], s.converged_many[slot]))
        (xa, ia, ra, ca), (xb, ib, rb, cb) = res
        assert ca and cb and ia == ib and ra == rb and np.array_equal(_bits(xa), _bits(xb)), (dtype_name, ia, ib, ra, rb)
        assert ia == it[0] and ra == re[0] and np.array_equal(_bits(xa), _bits(X[0]))


# ------------------------------------------------------------------------------------------------
# 5. scaling, exact
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_power_of_two_scaling_is_exact(lam, dtype_name):
    """Every quantity of the recurrence scales by an exact power of two with b, alpha and beta not at all: the columns b,
    2^-10 b, 2^10 b, 2^-20 b give exactly scaled solutions, the same iteration count and the same rel_err."""
    A, _, rng = _smoke_system()
    b = rng.uniform(-1, 1, A.shape[0])
    scales = [1.0, 2.0 ** -10, 2.0 ** 10, 2.0 ** -20]
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.set_matrix(A)
        bv = b.astype(s.vec_dtype)
        s.set_rhs_many(np.stack([bv * s.vec_dtype(c) for c in scales]))
        assert s.solve_many(2000, TOL[dtype_name]).all()
        X, it, re = s.solutions(), s.num_iters_many, s.rel_err_many
        assert it[0] > 20
        for j, c in enumerate(scales):
            assert it[j] == it[0] and re[j] == re[0], (dtype_name, j, it, re)
            assert np.array_equal(_bits(X[j]), _bits(X[0] * s.vec_dtype(c))), (dtype_name, j)


# ------------------------------------------------------------------------------------------------
# 6. parity per column
# ------------------------------------------------------------------------------------------------
def _parity_systems(oracle, dtype_name):
    """(name, matrix, tolerance).  The tolerance has to lie above what the number format can attain on the system, or the gate
    `true residual <= 2 tol` tests the format and not the code: the recursive residual drifts from b - A x by about u * cond.
    fp64: 1e-9 everywhere (u * cond ~ 1e-13).  fp32, u = 2^-24: the 512 x 512 system has cond ~ 55, u * cond = 3e-6, tol 1e-5; the
    golden fp32 system spd_n128_s42 has cond 863, u * cond = 5e-5 -- at tol 1e-5 the reference's own fp32 loop (the oracle) leaves
    true residuals of 1.9e-5 ... 2.4e-5 on these very columns, above 2 tol -- so it runs at tol 1e-4, where the reference's loop
    leaves 7.4e-5 ... 1.0e-4 (measured on the CPU with the oracle, not with the code under test)."""
    A, _, _ = _smoke_system()
    yield "smoke 512", A, TOL[dtype_name]
    if dtype_name == "F64":
        yield "spd_n256_s3", oracle.read_bin(os.path.join(GOLDEN, "spd_n256_s3.matrix.bin"), np.float64), 1e-9
    else:
        yield "spd_n128_s42.f32", oracle.read_bin(os.path.join(GOLDEN, "spd_n128_s42.f32.matrix.bin"), np.float32), 1e-4


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_parity_per_column(lam, oracle, dtype_name):
    for name, A, tol in _parity_systems(oracle, dtype_name):
        n = A.shape[0]
        with lam.Solver(getattr(lam, dtype_name)) as s:
            A_dev = np.ascontiguousarray(A, dtype=s.mat_host_dtype)
            A64 = A_dev.astype(np.float64)
            s.set_matrix(A_dev)
            B = np.random.default_rng(77).uniform(-1, 1, (5, n)).astype(s.vec_dtype)
            s.set_rhs_many(B)
            conv = s.solve_many(10000, tol)
            X, it = s.solutions(), s.num_iters_many.copy()
            assert conv.all() and s.stats["converged"] == 1 and s.stats["num_iters"] == it.max(), (name, conv, it)
            for j in range(5):
                x_or, st_or = oracle.cg_solve(A_dev, B[j], 10000, tol)
                what = (dtype_name, name, j, int(it[j]), st_or["num_iters"])
                assert st_or["converged"] and abs(int(it[j]) - st_or["num_iters"]) <= ITER_GATE[dtype_name](st_or["num_iters"]), what
                b64, x64 = B[j].astype(np.float64), X[j].astype(np.float64)
                assert np.linalg.norm(b64 - A64 @ x64) / np.linalg.norm(b64) <= 2 * tol + 1e-13, what
                s.set_rhs(B[j])
                assert s.solve(10000, tol)
                x_single = s.solution().astype(np.float64)
                if dtype_name == "F64":
                    assert np.linalg.norm(x64 - x_or) / np.linalg.norm(x_or) <= 10 * tol, what
                    assert np.linalg.norm(x64 - x_single) / np.linalg.norm(x_single) <= 10 * tol, what
                else:       # fp32: test_cg_low_precision's gate against the fp64 solve of the rounded system
                    x_true = np.linalg.solve(A64, b64)
                    assert np.linalg.norm(x64 - x_true) / np.linalg.norm(x_true) < 1e-3, what
                    assert np.linalg.norm(x_single - x_true) / np.linalg.norm(x_true) < 1e-3, what


# ------------------------------------------------------------------------------------------------
# 7. early columns freeze
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_early_columns_freeze(lam, oracle, dtype_name):
    A, q, rng = _smoke_system()
    n = A.shape[0]
    tol = TOL[dtype_name]
    e0 = np.zeros(n)
    e0[0] = 1.0
    with lam.Solver(getattr(lam, dtype_name)) as s:
        A_dev = np.ascontiguousarray(A, dtype=s.mat_host_dtype)
        B = np.stack([rng.uniform(-1, 1, n), q[:, 0] + 2 * q[:, 1] - q[:, 2], e0]).astype(s.vec_dtype)
        s.set_matrix(A_dev)
        s.set_rhs_many(B)
        assert s.solve_many(2000, tol).all()
        X, it, re = s.solutions(), s.num_iters_many.copy(), s.rel_err_many.copy()
        for j in range(3):
            _, st_or = oracle.cg_solve(A_dev, B[j], 2000, tol)
            assert abs(int(it[j]) - st_or["num_iters"]) <= ITER_GATE[dtype_name](st_or["num_iters"]), (dtype_name, j, it, st_or)
        assert 2 * it[1] < min(it[0], it[2]), it
        assert s.stats["num_iters"] == it.max()
        # nothing touched the early column while the others ran on: the same batch capped at ITS iteration count
        s.solve_many(int(it[1]), tol)
        assert s.converged_many[1] and not s.converged_many[0]
        assert s.num_iters_many[1] == it[1] and s.rel_err_many[1] == re[1]
        assert np.array_equal(_bits(s.solutions()[1]), _bits(X[1]))


# ------------------------------------------------------------------------------------------------
# 8. degenerate columns stay in their column
# ------------------------------------------------------------------------------------------------
def _like_reference(x, st, x_or, st_or, what):
    """What test_degenerate_inputs_behave_like_the_reference_loop demands of a single solve."""
    assert st["num_iters"] == st_or["num_iters"] and bool(st["converged"]) == bool(st_or["converged"]), what
    assert np.array_equal(np.isnan(x), np.isnan(x_or)), what
    assert np.allclose(np.nan_to_num(x), np.nan_to_num(x_or), rtol=1e-12, atol=1e-300), what
    e, e_or = st["rel_err"], st_or["rel_err"]
    assert (np.isnan(e) and np.isnan(e_or)) or max(abs(e), abs(e_or)) < 1e-14 or abs(e - e_or) <= 1e-9 * abs(e_or), what


def test_degenerate_columns_stay_in_their_column(lam, oracle):
    rng = np.random.default_rng(3)
    n = 96
    q, _ = np.linalg.qr(rng.uniform(-1, 1, (n, n)))
    A = (q * np.exp(rng.uniform(-1, 1, n))) @ q.T
    A = 0.5 * (A + A.T)
    b = rng.uniform(-1, 1, n)
    with lam.Solver(lam.F64) as s:
        s.set_matrix(A)
        s.set_rhs_many(np.stack([b, np.zeros(n), b]))
        conv = s.solve_many(20, 1e-9)
        X = s.solutions()
        x_or, st_or = oracle.cg_solve(A, b, 20, 1e-9)
        assert np.isnan(X[1]).all() and s.num_iters_many[1] == 21 and not conv[1] and np.isnan(s.rel_err_many[1])
        assert np.isnan(s.stats["rel_err"]) and s.stats["num_iters"] == 21 and s.stats["converged"] == 0
        assert np.array_equal(_bits(X[0]), _bits(X[2])) and np.isfinite(X[0]).all()
        assert s.num_iters_many[0] == s.num_iters_many[2] and s.rel_err_many[0] == s.rel_err_many[2]
        for j in (0, 1, 2):
            x_ref, st_ref = (x_or, st_or) if j != 1 else oracle.cg_solve(A, np.zeros(n), 20, 1e-9)
            st = {"num_iters": int(s.num_iters_many[j]), "converged": bool(conv[j]), "rel_err": float(s.rel_err_many[j])}
            _like_reference(X[j], st, x_ref, st_ref, ("B = [b, 0, b]", j, st, st_ref))
    cases = [("A = I", np.eye(n), b, 20, 1e-9), ("tolerance 10", A, b, 20, 10.0), ("max_iters 0", A, b, 0, 1e-9),
             ("max_iters 1", A, b, 1, 1e-9), ("1 x 1", np.array([[4.0]]), np.array([2.0]), 5, 1e-9),
             ("2 x 2", np.array([[2.0, 1.0], [1.0, 3.0]]), np.array([1.0, -1.0]), 10, 1e-12)]
    for name, A_, b_, iters, tol in cases:
        B = np.stack([b_, -0.5 * b_, 3.0 * b_])
        with lam.Solver(lam.F64) as s:
            s.set_matrix(A_)
            s.set_rhs_many(B)
            conv = s.solve_many(iters, tol)
            X = s.solutions()
            for j in range(3):
                x_ref, st_ref = oracle.cg_solve(A_, B[j], iters, tol)
                st = {"num_iters": int(s.num_iters_many[j]), "converged": bool(conv[j]), "rel_err": float(s.rel_err_many[j])}
                _like_reference(X[j], st, x_ref, st_ref, (name, j, st, st_ref))


# ------------------------------------------------------------------------------------------------
# 9. reproducible; the single-vector state is undisturbed
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_reproducible_and_single_state_undisturbed(lam, dtype_name):
    A, _, rng = _smoke_system()
    n = A.shape[0]
    tol = TOL[dtype_name]
    b = rng.uniform(-1, 1, n)
    B = rng.uniform(-1, 1, (6, n))
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.set_matrix(A)
        s.set_rhs(b)
        s.solve(2000, tol)
        x_fresh, st_fresh = s.solution(), s.stats
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.set_matrix(A)
        s.set_rhs(b)
        s.solve(2000, tol)
        x0 = s.solution()
        s.set_rhs_many(B)
        s.solve_many(2000, tol)
        X1, it1, re1 = s.solutions(), s.num_iters_many.copy(), s.rel_err_many.copy()
        # the single solution is still there, and a new single solve gives the bits of a fresh context
        assert np.array_equal(_bits(s.solution()), _bits(x0)) and np.array_equal(_bits(x0), _bits(x_fresh))
        s.solve(2000, tol)
        assert np.array_equal(_bits(s.solution()), _bits(x_fresh)) and s.stats["num_iters"] == st_fresh["num_iters"]
        assert s.stats["rel_err"] == st_fresh["rel_err"]
        # the batch is still there too, and solving it again gives the same bits
        assert np.array_equal(_bits(s.solutions()), _bits(X1))
        s.solve_many(2000, tol)
        assert np.array_equal(_bits(s.solutions()), _bits(X1)) and (s.num_iters_many == it1).all() and (s.rel_err_many == re1).all()
        # the benchmark's loop after a batched call
        s.cg_init()
        st = s.cg_iterate(10, 0.0)
        assert st["num_iters"] == 11 and np.isfinite(st["rel_err"]) and st["rel_err"] < 1.0


# ------------------------------------------------------------------------------------------------
# 10. refusals
# ------------------------------------------------------------------------------------------------
def test_refusals(lam, monkeypatch):
    import ctypes as C
    n = 64
    A = np.eye(n)
    B = np.ones((2, n))
    EINVAL, ESTATE = -1, -6

    def refused(s, code, fn, *args):
        launches = s.get_option("hip_calls_launch")
        with pytest.raises(lam.LamHipError) as e:
            fn(*args)
        assert e.value.code == code, (fn, e.value)
        msg = (s._L.lam_hip_last_error(s._h) or b"").decode()
        assert msg, fn
        assert s.get_option("hip_calls_launch") == launches
        return msg

    def every_entry_point(s, code):
        refused(s, code, s.set_rhs_many, B)
        s.nrhs = 2
        refused(s, code, s.solve_many, 5, 1e-9)
        refused(s, code, s.solutions)
        refused(s, code, s.gemv_many, B)
        refused(s, code, s.gemv_many_only, 2, 3)

    with lam.Solver(lam.F64, device_ids=[0, 0]) as s:
        s.set_matrix(A)
        assert "shard" in refused(s, EINVAL, s.set_rhs_many, B)
        every_entry_point(s, EINVAL)
    with lam.Solver(lam.BF16) as s:
        s.set_matrix(A)
        assert "BF16" in refused(s, EINVAL, s.set_rhs_many, B.astype(np.float32))
        every_entry_point(s, EINVAL)
    monkeypatch.setenv("LAM_HIP_FORCE_RCCL", "1")      # a one-rank communicator: the rank mode on one GPU
    with lam.Solver(lam.F64, rank=0, nranks=1, device_id=0, unique_id=None) as s:
        monkeypatch.delenv("LAM_HIP_FORCE_RCCL")
        s.set_problem(n)
        s.upload_rows(0, A)
        assert "rank mode" in refused(s, EINVAL, s.set_rhs_many, B)
        every_entry_point(s, EINVAL)
    with lam.Solver(lam.F64) as s:
        vp = C.c_void_p
        buf = np.zeros((9, n))
        # before a problem / a matrix / the right-hand sides: ESTATE, as the single-vector calls
        s.n = n
        refused(s, ESTATE, s.set_rhs_many, B)
        refused(s, ESTATE, s.gemv_many, B)
        refused(s, ESTATE, s.gemv_many_only, 2, 3)
        s.set_problem(n)
        refused(s, ESTATE, s.gemv_many, B)
        s.upload_rows(0, A)
        s.nrhs = 2
        refused(s, ESTATE, s.solve_many, 5, 1e-9)
        refused(s, ESTATE, s.solutions)
        for nrhs in (0, -1, lam.MAX_RHS + 1):
            for call in (lambda: s._L.lam_hip_set_rhs_many(s._h, nrhs, buf.ctypes.data_as(vp)),
                         lambda: s._L.lam_hip_get_solution_many(s._h, nrhs, buf.ctypes.data_as(vp)),
                         lambda: s._L.lam_hip_gemv_many(s._h, nrhs, buf.ctypes.data_as(vp), buf.ctypes.data_as(vp)),
                         lambda: s._L.lam_hip_gemv_many_only(s._h, nrhs, 3, C.byref(C.c_double()))):
                assert "nrhs" in refused(s, EINVAL, lambda: s._chk(call()))
        # and the path works on this context afterwards
        s.set_rhs_many(B)
        assert s.solve_many(5, 1e-9).all() and np.allclose(s.solutions(), B)
        # a set_problem invalidates the right-hand sides, as for the single solve
        s.set_problem(n)
        s.upload_rows(0, A)
        refused(s, ESTATE, s.solve_many, 5, 1e-9)


# ------------------------------------------------------------------------------------------------
# 11. it pays
# ------------------------------------------------------------------------------------------------
def test_batched_product_is_cheaper_than_single_ones(lam):
    """A condition, not a benchmark: one batched product for 4 vectors takes less than 4 single products (by the byte model the
    ratio is 1).  Minimum over three alternated measurements each."""
    n, reps = 16384, 20
    with lam.Solver(lam.F64) as s:
        s.generate_random_spd(n, 5, 100.0)
        s.gemv_only(3), s.gemv_many_only(4, 3)
        single, batch = [], []
        for _ in range(3):
            single.append(s.gemv_only(reps))
            batch.append(s.gemv_many_only(4, reps))
        print(f"\nN={n} fp64: gemv_only {min(single) * 1e6:.1f} us, gemv_many_only(4) {min(batch) * 1e6:.1f} us, "
              f"ratio {min(batch) / min(single):.3f} (4 = break even)")
        assert min(batch) < 4 * min(single), (single, batch)


# ------------------------------------------------------------------------------------------------
# 12. driver
# ------------------------------------------------------------------------------------------------
def test_multi_rhs_driver_known_answer():
    exe = os.path.join(ROOT, PKG_NAME, "test", "test_CG_multi_rhs.out")
    r = subprocess.run([exe, "-s", "4096", "-k", "3", "-i", "15"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln.split(",") for ln in r.stdout.strip().splitlines()]
    assert len(lines) == 3 and all(len(ln) == 10 and ln[0] == "4096" for ln in lines), r.stdout
    assert lines[0][7] == "16" and abs(float(lines[0][8]) / 0.000368282 - 1) < 1e-5, lines[0]
    # the columns are 1, 2 and 4 times the same vector: the same iteration count and the same rel_err digits
    assert lines[1][7:9] == lines[0][7:9] and lines[2][7:9] == lines[0][7:9], r.stdout


# ------------------------------------------------------------------------------------------------
# 13. full size
# ------------------------------------------------------------------------------------------------
@pytest.mark.slow
def test_gemv_many_exact_full_size(lam):
    n = 65536
    X = [E.int_vec(n, 900 + j) for j in range(8)]
    with lam.Solver(lam.F64) as s:
        s.set_problem(n)
        Y = E.generate(n, [s.upload_rows], X)
        got = s.gemv_many(np.stack(X))
        assert np.array_equal(got, np.stack(Y))
