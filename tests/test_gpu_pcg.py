"""Jacobi-preconditioned batched CG on the GPU: lam_hip_solve_many_pc / lam_hip_get_diagonal (include/lam_hip.h).

Pinned bit for bit where arithmetic allows it -- on tridiag(1,2,1) the diagonal is the constant 2, dinv = 0.5, and every quantity of
the preconditioned recurrence is the plain one's times an exact power of two, so x, the iteration counts and rel_err must be the
plain batch's bits -- and against the numpy restatement of the recurrence (tests/pcg_reference.py) on the badly scaled systems
A = S M S the preconditioner is for."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pcg_reference as R
from conftest import ROOT, PKG_NAME
from test_gpu_multi_rhs import ITER_GATE, _edge_sizes

pytestmark = pytest.mark.gpu

DTYPES = ("F64", "F32")
NP = {"F64": np.float64, "F32": np.float32}
TOL = {"F64": 1e-10, "F32": 1e-5}
EINVAL, ESTATE = -1, -6


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _solve_pc(s, precond, max_iters, rel_error):
    """lam_hip_solve_many_pc itself, whatever `precond` (Solver.solve_many sends PC_NONE to lam_hip_solve_many)."""
    k = s.nrhs
    ni, cv, re = np.zeros(k, np.int32), np.zeros(k, np.int32), np.zeros(k, np.float64)
    st = s._L.lam_hip_solve_many_pc.argtypes[4]._type_()       # the binding's Stats
    s._chk(s._L.lam_hip_solve_many_pc(s._h, precond, max_iters, rel_error, C.byref(st), ni.ctypes.data_as(C.POINTER(C.c_int32)),
                                      cv.ctypes.data_as(C.POINTER(C.c_int32)), re.ctypes.data_as(C.POINTER(C.c_double))))
    return ni, cv.astype(bool), re, st.asdict()


def _result(s):
    return s.solutions(), s.num_iters_many.copy(), s.converged_many.copy(), s.rel_err_many.copy()


# ------------------------------------------------------------------------------------------------
# 1. exact
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1025, 4097])
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_jacobi_on_tridiag_is_the_plain_batch_bit_for_bit(lam, dtype_name, n):
    """diag = 2, dinv = 0.5: p, Ap are the plain ones halved, rz = rr / 2, p.Ap a quarter, alpha doubled, beta the same -- all exact."""
    rng = np.random.default_rng(n)
    i = np.arange(1, n + 1)
    cols = [np.ones(n), np.sin(3 * np.pi * i / (n + 1))] + [rng.uniform(-1, 1, n) for _ in range(6)]   # smooth, an eigenvector, rough
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.generate_matrix(n)
        assert _same(s.diagonal(), np.full(n, 2.0, s.vec_dtype))
        for nrhs in (1, 3, 8):
            B = np.stack(cols[:nrhs]).astype(s.vec_dtype)
            s.set_rhs_many(B)
            for tol in (0.0, 1e-3):
                s.solve_many(40, tol)
                X0, it0, cv0, re0 = _result(s)
                st0 = s.stats
                s.solve_many(40, tol, lam.PC_JACOBI)
                X1, it1, cv1, re1 = _result(s)
                what = (dtype_name, n, nrhs, tol, it0, it1, re0, re1)
                assert np.isfinite(X0).all() and (it0 == it1).all() and (cv0 == cv1).all() and _same(re0, re1), what
                assert _same(X0, X1), what
                assert s.stats["num_iters"] == st0["num_iters"] and s.stats["converged"] == st0["converged"], what
                assert s.stats["rel_err"] == st0["rel_err"] and s.stats["gemv_bytes"] == st0["gemv_bytes"], what
                if tol == 0.0:
                    assert (it0 == 41).all() and not cv0.any(), what
                else:       # some columns stop early and stay frozen while the others run on
                    assert cv0[0] and it0[0] < 40, what
                    if nrhs >= 3:
                        assert cv0[1] and it0[1] < it0[0] and not cv0[2:].any() and (it0[2:] == 41).all(), what


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_pc_none_is_solve_many_bit_for_bit(lam, dtype_name):
    A, rng = R.smoke_system()
    B = rng.uniform(-1, 1, (5, A.shape[0]))
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.set_matrix(A)
        s.set_rhs_many(B)
        s.solve_many(2000, 1e-5)
        X0, it0, cv0, re0 = _result(s)
        st0 = s.stats
        it1, cv1, re1, st1 = _solve_pc(s, lam.PC_NONE, 2000, 1e-5)
        assert cv0.all() and (it0 == it1).all() and (cv0 == cv1).all() and _same(re0, re1) and _same(X0, s.solutions())
        assert st1["num_iters"] == st0["num_iters"] and st1["rel_err"] == st0["rel_err"] and st1["gemv_bytes"] == st0["gemv_bytes"]
        assert s.get_option("multi_rhs_k") == 8


# ------------------------------------------------------------------------------------------------
# 2. parity with the reference recurrence on badly scaled systems
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [512, 2049])
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_parity_with_the_reference_recurrence_on_scaled_systems(lam, dtype_name, n):
    tol, dt = TOL[dtype_name], NP[dtype_name]
    A, rng = R.sms_system(n)
    Xstar = rng.uniform(-1, 1, (8, n))
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.set_matrix(A)
        A_dev = s.download_rows(0, n)
        assert A_dev.dtype == dt and np.array_equal(A_dev, A_dev.T)
        B = (Xstar @ A_dev.astype(np.float64).T).astype(dt)
        dinv = R.jacobi_dinv(A_dev, dt)
        ref = [R.pcg(A_dev, B[j], 4 * n, tol, dinv, dt)[1] for j in range(8)]
        assert all(r["converged"] for r in ref), ref
        for nrhs in (1, 4, 8):
            s.set_rhs_many(B[:nrhs])
            conv = s.solve_many(4 * n, tol, lam.PC_JACOBI)
            X, it, _, re = _result(s)
            print(f"\n{dtype_name} n={n} nrhs={nrhs}: jacobi iterations {it.tolist()}, reference {[r['num_iters'] for r in ref[:nrhs]]}")
            assert conv.all() and s.stats["converged"] == 1 and s.stats["num_iters"] == it.max(), (dtype_name, n, nrhs, it, re)
            for j in range(nrhs):
                res = R.true_residual(A_dev, X[j], B[j])
                what = (dtype_name, n, nrhs, j, int(it[j]), ref[j], res)
                assert abs(int(it[j]) - ref[j]["num_iters"]) <= ITER_GATE[dtype_name](ref[j]["num_iters"]), what
                assert res <= 2 * tol, what
            plain = s.solve_many(4 * n, tol)
            print(f"   plain iterations {s.num_iters_many.tolist()}, rel_err {s.rel_err_many.tolist()}")
            if dtype_name == "F64":
                assert not plain.any() and (s.num_iters_many == 4 * n + 1).all(), (n, nrhs, s.num_iters_many, s.rel_err_many)


# ------------------------------------------------------------------------------------------------
# 3. where it pays
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_a_tenth_of_the_iterations_on_the_generated_spd_matrix(lam, dtype_name):
    n, tol, dt = 2049, TOL[dtype_name], NP[dtype_name]
    B = np.random.default_rng(11).uniform(-1, 1, (4, n)).astype(dt)
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.generate_random_spd(n, 5, 1e4)
        A_dev = s.download_rows(0, n)
        assert _same(s.diagonal(), np.diag(A_dev).copy())
        s.set_rhs_many(B)
        assert s.solve_many(4 * n, tol).all()
        it_plain = s.num_iters_many.copy()
        assert s.solve_many(4 * n, tol, lam.PC_JACOBI).all()
        X, it, _, _ = _result(s)
        print(f"\n{dtype_name} n={n}: plain {it_plain.tolist()}, jacobi {it.tolist()}")
        for j in range(4):
            assert 10 * int(it[j]) <= int(it_plain[j]), (dtype_name, j, it, it_plain)
            assert R.true_residual(A_dev, X[j], B[j]) <= 2 * tol, (dtype_name, j)


# ------------------------------------------------------------------------------------------------
# 4. column semantics
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_columns_are_independent_and_degenerate_ones_stay_in_their_column(lam, dtype_name):
    tol, dt, cap = TOL[dtype_name], NP[dtype_name], 150
    A, rng = R.sms_system(512)
    n = A.shape[0]
    b = (A @ rng.uniform(-1, 1, n)).astype(dt)
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.set_matrix(A)
        s.set_rhs_many(np.tile(b, (8, 1)))
        assert s.solve_many(cap, tol, lam.PC_JACOBI).all()
        X, it, _, re = _result(s)
        for j in range(1, 8):
            assert _same(X[j], X[0]) and it[j] == it[0] and re[j] == re[0], (dtype_name, j)
        for nrhs, slot in ((8, 2), (8, 6), (3, 1)):
            B = (np.random.default_rng(slot).uniform(-1, 1, (nrhs, n)) * np.array([1, 3, 1, 0.01, 100, 1, 1, 7])[:nrhs, None]).astype(dt)
            B[slot] = b
            B[(slot + 1) % nrhs] = np.nan
            B[(slot + 2) % nrhs] = 0.0
            s.set_rhs_many(B)
            conv = s.solve_many(cap, tol, lam.PC_JACOBI)
            Xs, its, _, res = _result(s)
            what = (dtype_name, nrhs, slot, its, res)
            assert conv[slot] and its[slot] == it[0] and res[slot] == re[0] and _same(Xs[slot], X[0]), what
            for bad in ((slot + 1) % nrhs, (slot + 2) % nrhs):      # NaN and 0/0: to the cap, and only there
                assert not conv[bad] and its[bad] == cap + 1 and np.isnan(res[bad]) and np.isnan(Xs[bad]).all(), what
            others = [j for j in range(nrhs) if j not in (slot, (slot + 1) % nrhs, (slot + 2) % nrhs)]
            assert np.isfinite(Xs[others]).all() and conv[others].all(), what
            assert np.isnan(s.stats["rel_err"]) and s.stats["num_iters"] == cap + 1 and s.stats["converged"] == 0, what
        # one column alone (K = 1) is a column of the batch
        s.set_rhs_many(b[None, :])
        assert s.solve_many(cap, tol, lam.PC_JACOBI).all() and s.get_option("multi_rhs_k") == 1
        assert _same(s.solutions()[0], X[0]) and s.num_iters_many[0] == it[0] and s.rel_err_many[0] == re[0]


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_early_columns_freeze(lam, dtype_name):
    tol, dt = TOL[dtype_name], NP[dtype_name]
    A, rng = R.sms_system(512)
    n = A.shape[0]
    d = np.sqrt(np.diag(A))
    _, V = np.linalg.eigh(A / d[:, None] / d[None, :])
    fast = d * V[:, n // 2]                 # an eigenvector of the preconditioned operator: a step or two
    B = np.stack([A @ rng.uniform(-1, 1, n), fast, A @ rng.uniform(-1, 1, n)]).astype(dt)
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.set_matrix(A)
        s.set_rhs_many(B)
        assert s.solve_many(4 * n, tol, lam.PC_JACOBI).all()
        X, it, _, re = _result(s)
        assert 2 * it[1] < min(it[0], it[2]) and s.stats["num_iters"] == it.max(), it
        # nothing touched the early column while the others ran on: the same batch capped at ITS iteration count
        s.solve_many(int(it[1]), tol, lam.PC_JACOBI)
        assert s.converged_many[1] and not s.converged_many[0] and not s.converged_many[2]
        assert s.num_iters_many[1] == it[1] and s.rel_err_many[1] == re[1] and _same(s.solutions()[1], X[1])
        assert s.num_iters_many[0] == it[1] + 1


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_interleaving_with_the_plain_solves_disturbs_nothing(lam, dtype_name):
    tol = TOL[dtype_name]
    A, rng = R.smoke_system()
    n = A.shape[0]
    b = rng.uniform(-1, 1, n)
    B = rng.uniform(-1, 1, (6, n))
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.set_matrix(A)
        s.set_rhs(b)
        assert s.solve(2000, tol)
        x0, st0 = s.solution(), s.stats
        s.set_rhs_many(B)
        assert s.solve_many(2000, tol).all()
        P0 = _result(s)
        assert s.solve_many(2000, tol, lam.PC_JACOBI).all()
        J0 = _result(s)
        assert _same(s.solution(), x0)                       # the single solution is still there
        assert s.solve(2000, tol) and _same(s.solution(), x0) and s.stats["num_iters"] == st0["num_iters"]
        assert s.stats["rel_err"] == st0["rel_err"]
        assert _same(s.solutions(), J0[0])                   # and so is the preconditioned batch
        s.solve_many(2000, tol)
        P1 = _result(s)
        s.solve_many(2000, tol, lam.PC_JACOBI)
        J1 = _result(s)
        for a, c in ((P0, P1), (J0, J1)):
            assert _same(a[0], c[0]) and (a[1] == c[1]).all() and (a[2] == c[2]).all() and _same(a[3], c[3])
        s.cg_init()                                          # the benchmark's loop after a preconditioned batch
        st = s.cg_iterate(10, 0.0)
        assert st["num_iters"] == 11 and np.isfinite(st["rel_err"]) and st["rel_err"] < 1.0


# ------------------------------------------------------------------------------------------------
# 5. the diagonal
# ------------------------------------------------------------------------------------------------
def _bf16_rne(a):
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)).view(np.float32)


@pytest.mark.parametrize("shards", [1, 3])
@pytest.mark.parametrize("dtype_name", ["F64", "F32", "BF16"])
def test_diagonal_is_the_uploaded_diagonal_bit_for_bit(lam, dtype_name, shards):
    sizes = [n for n in _edge_sizes("F32" if dtype_name == "BF16" else dtype_name) if n >= shards]     # set_problem refuses n < shards
    with lam.Solver(getattr(lam, dtype_name), device_ids=[0] * shards) as s:
        for n in sizes:
            rng = np.random.default_rng(n)
            diag = rng.uniform(-2, 2, n).astype(s.mat_host_dtype)
            s.set_problem(n)
            step = max(1, (32 << 20) // (8 * n))
            buf = np.full((min(step, n), n), -7.0, s.mat_host_dtype)      # off the diagonal: a value no diagonal element has
            for r0 in range(0, n, step):
                rows = buf[:min(step, n - r0)]
                i = np.arange(rows.shape[0])
                rows[i, r0 + i] = diag[r0:r0 + rows.shape[0]]
                s.upload_rows(r0, rows)
                rows[i, r0 + i] = -7.0
            want = _bf16_rne(diag) if dtype_name == "BF16" else diag.astype(s.vec_dtype)
            got = s.diagonal()
            bad = np.flatnonzero(_bits(got) != _bits(want))
            assert got.dtype == s.vec_dtype and bad.size == 0, (dtype_name, shards, n, bad[:6], got[bad[:6]], want[bad[:6]])


def _spd(n):
    return 2.0 * np.eye(n) + 0.001


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_a_diagonal_that_cannot_be_inverted_is_refused_with_its_row(lam, dtype_name):
    n, dt = 1000, NP[dtype_name]
    A = _spd(n).astype(dt)
    B = np.ones((2, n), dt)
    values = [0.0, -1.0, -0.0, np.nan, np.inf, 1e-40 if dtype_name == "F32" else 5e-324]     # the last: 1 / subnormal overflows
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.set_matrix(A)
        s.set_rhs_many(B)
        assert s.solve_many(50, TOL[dtype_name], lam.PC_JACOBI).all()
        X_good = s.solutions()
        for v in values:
            for row in (0, n // 2, n - 1):
                r = A[row:row + 1].copy()
                r[0, row] = v
                s.upload_rows(row, r)
                assert _same(s.diagonal()[row:row + 1], np.array([v], dt))
                with pytest.raises(lam.LamHipError) as e:
                    s.solve_many(50, TOL[dtype_name], lam.PC_JACOBI)
                assert e.value.code == EINVAL and f"row {row} " in str(e.value), (v, row, e.value)
                with pytest.raises(lam.LamHipError) as e:     # and again: the verdict is the matrix's, not the first call's
                    s.solve_many(50, TOL[dtype_name], lam.PC_JACOBI)
                assert e.value.code == EINVAL and f"row {row} " in str(e.value), (v, row, e.value)
                with pytest.raises(lam.LamHipError) as e:
                    s.solutions()
                assert e.value.code == ESTATE, (v, row, e.value)
                # the corrected row is seen by the next solve: the diagonal is cached per matrix CONTENT
                s.upload_rows(row, A[row:row + 1])
                assert s.solve_many(50, TOL[dtype_name], lam.PC_JACOBI).all() and _same(s.solutions(), X_good), (v, row)
        # several bad rows: the first one is named
        for row in (700, 41, 999):
            r = A[row:row + 1].copy()
            r[0, row] = -3.0
            s.upload_rows(row, r)
        with pytest.raises(lam.LamHipError) as e:
            s.solve_many(50, TOL[dtype_name], lam.PC_JACOBI)
        assert e.value.code == EINVAL and "row 41 " in str(e.value) and "-3" in str(e.value) and "3 such rows" in str(e.value), e.value
        # the plain batch does not care, and a generator call is seen too
        s.solve_many(5, TOL[dtype_name])
        s.generate_matrix(n)
        s.set_rhs_many(B)
        s.solve_many(5, 0.0, lam.PC_JACOBI)
        assert (s.num_iters_many == 6).all() and np.isfinite(s.solutions()).all()


# ------------------------------------------------------------------------------------------------
# 6. refusals
# ------------------------------------------------------------------------------------------------
def test_refusals(lam, monkeypatch):
    n = 64
    A = np.eye(n)
    B = np.ones((2, n))

    def refused(s, code, fn, *args):
        launches = s.get_option("hip_calls_launch")
        with pytest.raises(lam.LamHipError) as e:
            fn(*args)
        assert e.value.code == code, (fn, e.value)
        assert s.get_option("hip_calls_launch") == launches
        return str(e.value)

    with lam.Solver(lam.F64, device_ids=[0, 0]) as s:
        s.set_matrix(A)
        s.nrhs = 2
        assert "shard" in refused(s, EINVAL, s.solve_many, 5, 1e-9, lam.PC_JACOBI)
        assert "shard" in refused(s, EINVAL, _solve_pc, s, lam.PC_NONE, 5, 1e-9)
        assert np.array_equal(s.diagonal(), np.ones(n))
    with lam.Solver(lam.BF16) as s:
        s.set_matrix(A)
        s.nrhs = 2
        assert "BF16" in refused(s, EINVAL, s.solve_many, 5, 1e-9, lam.PC_JACOBI)
        assert np.array_equal(s.diagonal(), np.ones(n, np.float32))
    monkeypatch.setenv("LAM_HIP_FORCE_RCCL", "1")      # a one-rank communicator: the rank mode on one GPU
    with lam.Solver(lam.F64, rank=0, nranks=1, device_id=0, unique_id=None) as s:
        monkeypatch.delenv("LAM_HIP_FORCE_RCCL")
        s.set_problem(n)
        s.upload_rows(0, A)
        s.nrhs = 2
        assert "rank mode" in refused(s, EINVAL, s.solve_many, 5, 1e-9, lam.PC_JACOBI)
        assert "rank mode" in refused(s, EINVAL, s.diagonal)
    with lam.Solver(lam.F64) as s:
        s.n, s.nrhs = n, 2
        refused(s, ESTATE, s.solve_many, 5, 1e-9, lam.PC_JACOBI)
        refused(s, ESTATE, s.diagonal)
        s.set_problem(n)
        refused(s, ESTATE, s.solve_many, 5, 1e-9, lam.PC_JACOBI)
        refused(s, ESTATE, s.diagonal)
        s.upload_rows(0, A)
        refused(s, ESTATE, s.solve_many, 5, 1e-9, lam.PC_JACOBI)      # no right-hand sides yet
        s.set_rhs_many(B)
        for precond in (2, -1, 7):
            assert "preconditioner" in refused(s, EINVAL, s.solve_many, 5, 1e-9, precond)
        refused(s, EINVAL, s.solve_many, -1, 1e-9, lam.PC_JACOBI)
        assert s._L.lam_hip_solve_many_pc(None, lam.PC_JACOBI, 5, 1e-9, None, None, None, None) == EINVAL
        assert s._L.lam_hip_get_diagonal(None, None) == EINVAL and s._L.lam_hip_get_diagonal(s._h, None) == EINVAL
        # and the path works on this context afterwards, every output optional
        assert s._L.lam_hip_solve_many_pc(s._h, lam.PC_JACOBI, 5, 1e-9, None, None, None, None) == 0
        assert s.solve_many(5, 1e-9, lam.PC_JACOBI).all() and np.allclose(s.solutions(), B)
        X, ni, cv, re = s.solve_all(np.ones((11, n)), 5, 1e-9, precond=lam.PC_JACOBI)
        assert cv.all() and np.allclose(X, 1.0) and (ni == 1).all()
        # a set_problem invalidates the right-hand sides, as for the plain batch
        s.set_problem(n)
        s.upload_rows(0, A)
        refused(s, ESTATE, s.solve_many, 5, 1e-9, lam.PC_JACOBI)


# ------------------------------------------------------------------------------------------------
# 7. driver
# ------------------------------------------------------------------------------------------------
def test_driver_flag_J_prints_the_plain_columns_on_tridiag():
    exe = os.path.join(ROOT, PKG_NAME, "test", "test_CG_multi_rhs.out")
    out = []
    for extra in ([], ["-J"]):
        r = subprocess.run([exe, "-s", "4096", "-k", "3", "-i", "25"] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = [ln.split(",") for ln in r.stdout.strip().splitlines()]
        assert len(lines) == 3 and all(len(ln) == 10 and ln[0] == "4096" for ln in lines), r.stdout
        out.append([ln[7:9] for ln in lines])
    assert out[0] == out[1] and out[0][0][0] == "26", out
