"""Batched CG on shifted systems, (A + s_j I) x_j = b_j in one pass over A: lam_hip_set_shifts_many (include/lam_hip.h), i.e. the
SHIFT = true instantiations of multi_gemv_kernel, the K-wide-dinv (DK) instantiations of multi_init / xr / p_kernel and
shifted_dinv_kernel (csrc/lam_kernels.h).

Sizes: the fp64 K = 8 p tile is 512 columns, the K = 4 tile 1024, the K = 1 tile 4096, and the vector kernels (the new dinv launch
among them) wrap at N = 65537; so N in {1, 5 / 7, 64, 513, 1030, 4097} and 65537 on the device-filled tridiag(1,2,1).

 1. zero shifts, and cleared ones, are the unshifted batch bit for bit (plain, Jacobi, from a guess);
 2. the exact product and the exact first step on tests/exact_data.py's integer matrix with integer shifts; true residuals;
 3. the exact first Jacobi step with M_j = diag(A) + s_j I over zeros on A's own diagonal; the refusal where the sum is zero;
 4. a column of a shifted batch of 8 is the column alone at K = 1 with its own shift, bit for bit, past the wrap too;
 5. every column iteration by iteration against the references of tests/test_gpu_batch_recurrence.py (C) on A + s_j I formed on
    the host;
 6. guess, continuation, path-following, true residuals under new shifts;
 7. refusals and lifetime; 8. the driver's -S."""
import os
import subprocess

import numpy as np
import pytest

import exact_data as E
import pcg_reference as R
import shifted_data as S
from conftest import ROOT, PKG_NAME
from tracking_data import ITERATION_TRACKING_GATES, TRACKED_K

pytestmark = pytest.mark.gpu

DTYPES = ("F64", "F32")
NP = {"F64": np.float64, "F32": np.float32}
U_TV = {"F64": 2.0 ** -53, "F32": 2.0 ** -24}
K_FOR = {1: 1, 2: 2, 3: 4, 4: 4, 5: 8, 6: 8, 7: 8, 8: 8}
EINVAL, ESTATE = -1, -6
INT_SHIFTS = S.INT_SHIFTS
# eight different shifts over six octaves, a zero among them (column 0)
REAL_SHIFTS = (0.0, 0.5, 0.03125, 4.0, 0.25, 1.0, 2.0, 0.125)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _assert_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = np.argwhere(_bits(got) != _bits(want))
    if bad.size:
        j, i = bad[0]
        raise AssertionError(f"{what}: {len(bad)} entries differ in columns {sorted(set(bad[:, 0].tolist()))}, first (column, row) = ({j}, {i}): "
                             f"got {got[j, i]!r}, want {want[j, i]!r}; next {bad[1:6].tolist()}")


def _result(s):
    return s.solutions(), s.num_iters_many.copy(), s.converged_many.copy(), s.rel_err_many.copy()


def _assert_same_run(got, want, what):
    _assert_bits(got[0], want[0], what + ": x")
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (what, got[1], want[1], got[2], want[2])
    assert np.array_equal(_bits(got[3]), _bits(want[3])), (what, got[3], want[3])


# ------------------------------------------------------------------------------------------------
# 1. zero shifts are the unshifted batch
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[(d, n) for n in (1, 7, 513, 1030) for d in DTYPES], ids=lambda p: f"{p[0]}-{p[1]}")
def spd(lam, request):
    """The smoke system of size n, 8 right-hand sides and 8 guesses; one context per (dtype, n)."""
    dtype_name, n = request.param
    dt = NP[dtype_name]
    A, rng = R.smoke_system(n, seed=n)
    A = A.astype(dt).astype(np.float64)
    B = rng.uniform(-1, 1, (8, n)).astype(dt)
    X0 = rng.uniform(-1, 1, (8, n)).astype(dt)
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.set_matrix(A)
        yield dtype_name, n, dt, A, B, X0, s


def test_zero_shifts_are_the_unshifted_batch_bit_for_bit(lam, spd):
    """set_shifts([0] * nrhs) and set_shifts(None) against no call at all: x, num_iters, converged, rel_err, multi_rhs_k; cap 6 with
    a tolerance some columns meet.  -0.0 is a zero shift too."""
    dtype_name, n, dt, A, B, X0, s = spd
    cap, tol = min(6, n), 3e-2
    for nrhs in range(1, 9):
        for precond in (lam.PC_NONE, lam.PC_JACOBI):
            for x0 in (None, X0[:nrhs]):
                what = f"{dtype_name} n={n} nrhs={nrhs} precond={precond} guess={x0 is not None}"
                s.set_rhs_many(B[:nrhs])
                s.solve_many(cap, tol, precond, x0)
                want, k_want = _result(s), s.get_option("multi_rhs_k")
                for zero in ([0.0] * nrhs, [-0.0] * nrhs, None):
                    s.set_rhs_many(B[:nrhs])
                    if zero is None:
                        s.set_shifts([1.0] * nrhs)       # cleared again: nothing of it stays
                    s.set_shifts(zero)
                    s.solve_many(cap, tol, precond, x0)
                    assert s.get_option("multi_rhs_k") == k_want == K_FOR[nrhs]
                    _assert_same_run(_result(s), want, what + f" shifts {zero}")


# ------------------------------------------------------------------------------------------------
# 2. exact product and first step on the integer matrix
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=(1, 5, 64, 513, 1030, 4097), ids=lambda n: f"n{n}")
def integer_system(lam, request):
    """exact_data's integer matrix of size n on an fp64 and an fp32 context (one generation), the dense matrix on the host, integer
    right-hand sides B, integer vectors V, C and the exact products A B, A V."""
    n = request.param
    assert n + 1 <= E.MAX_EXACT_N_FP32
    dense = np.empty((n, n))

    def keep(r0, blk):
        dense[r0:r0 + blk.shape[0]] = blk

    B = [E.int_vec(n, 51 * n + j) for j in range(8)]
    V = [E.int_vec(n, 53 * n + j) for j in range(8)]
    for v in B + V:
        v[v == 0] = 1.0           # no zero vector at n = 1
    Cc = np.stack([E.int_vec(n, 59 * n + j) for j in range(8)])
    Cc[Cc == 0] = 1.0
    with lam.Solver(lam.F64) as s64, lam.Solver(lam.F32) as s32:
        s64.set_problem(n)
        s32.set_problem(n)
        prod = E.generate(n, [s64.upload_rows, s32.upload_rows, keep], B + V)
        yield n, dense, np.stack(B), np.stack(V), Cc, np.stack(prod[:8]), np.stack(prod[8:]), {"F64": s64, "F32": s32}


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_shifted_product_is_exact(lam, integer_system, dtype_name):
    """b_j = A v_j + s_j v_j + c_j, all integers.  From the guess v_j with max_iters = 0 the start's rel_err is
    ||b - (A + s_j I) v_j|| / ||b|| = sqrt(c.c / b.b) with both sums exact integers in any order: 2 ulp (a division, a square root).
    The guess's product and lam_hip_true_residual_many's product are two launches: both are checked.  A shift taken from the
    neighbouring column, or left out, moves c by a multiple of v."""
    n, dense, _, V, Cc, _, AV, ctx = integer_system
    s, dt = ctx[dtype_name], NP[dtype_name]
    sh = np.array(INT_SHIFTS, np.float64)
    Bs = AV + sh[:, None] * V + Cc
    assert np.abs(Bs).max() < 2 ** 24
    want = np.sqrt(np.sum(Cc * Cc, axis=1) / np.sum(Bs * Bs, axis=1))
    for nrhs in (1, 3, 8):
        s.set_rhs_many(Bs[:nrhs])
        s.set_shifts(sh[:nrhs])
        s.solve_many(0, 1e-30, x0=V[:nrhs])
        X, it, cv, re = _result(s)
        what = f"{dtype_name} n={n} nrhs={nrhs}"
        assert (it == 1).all() and not cv.any() and s.get_option("multi_rhs_k") == K_FOR[nrhs], (what, it)
        _assert_bits(X, V[:nrhs].astype(dt), what)
        res = s.true_residuals()
        for got in (re, res):
            print(f"{what}: off by {(np.abs(got - want[:nrhs]) / np.spacing(want[:nrhs])).tolist()} ulp")
            assert (np.abs(got - want[:nrhs]) <= 2 * np.spacing(want[:nrhs])).all(), (what, got, want[:nrhs])
        # gemv_many stays the plain product of A, shifts set or not
        _assert_bits(s.gemv_many(V[:nrhs]), AV[:nrhs].astype(dt), f"{dtype_name} n={n} nrhs={nrhs}: gemv_many under shifts")


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_first_shifted_step_is_exact(lam, integer_system, dtype_name):
    """solve_many(1, 1e-30) under integer shifts: x1 = fl(alpha_TV b) bit for bit with alpha = fl64(b.b / b.(A b + s_j b)), both
    sums exact integers (exact_data.first_cg_step on A b + s_j b); rel_err within exact_data.rel_err_bound.  The true residual of
    x1 against the exact r1 = b - alpha (A + s_j I) b: tests/shifted_data.py's bound for the product and the subtraction, plus the
    rounding of x1 itself, u (|A| + s I)|x1|."""
    n, dense, B, _, _, AB, _, ctx = integer_system
    s, vdt, u = ctx[dtype_name], NP[dtype_name], U_TV[dtype_name]
    sh = np.array(INT_SHIFTS, np.float64)
    absA = np.abs(dense)
    for nrhs in (1, 3, 8):
        s.set_rhs_many(B[:nrhs])
        s.set_shifts(sh[:nrhs])
        s.solve_many(1, 1e-30)
        X, it, cv, re = _result(s)
        # the cap convention: 2 for a column that has not stopped.  n = 1: the first step IS the solution, and a column whose r1 rounds to
        # exactly 0 stops in it (1 iteration, converged)
        assert n == 1 or not cv.any()
        assert list(it) == [1 if c else 2 for c in cv] and s.stats["num_iters"] == it.max() and s.get_option("multi_rhs_k") == K_FOR[nrhs]
        res = s.true_residuals()
        for j in range(nrhs):
            Ab = AB[j] + sh[j] * B[j]
            alpha, x1, bb, _, r1 = E.first_cg_step(B[j], Ab, vdt)
            what = f"{dtype_name} n={n} nrhs={nrhs} column {j} shift {sh[j]} (alpha {alpha!r})"
            _assert_bits(X[j:j + 1], (x1 + vdt(0))[None], what)
            if np.any(r1):
                re_host, bound = E.rel_err_bound(B[j], Ab, alpha, r1, bb, u)
                assert abs(re[j] - re_host) <= bound and not cv[j], (what, re[j], re_host, bound)
            else:
                # n = 1 and fl64(alpha (a + s) b) = b, so the host's r1 is 0; the device's fma rounds b - alpha (a + s) b once, and the
                # exact product is within u |b| of b: |r| <= 2 u |b|
                assert n == 1 and re[j] <= 2 * u, (what, re[j])
            x64 = x1.astype(np.float64)
            w = absA @ np.abs(x64)
            ref = np.linalg.norm(r1) / np.sqrt(bb)
            tb = (S.true_residual_bound(w, B[j], sh[j], x64, n, u) + u * np.linalg.norm(w + sh[j] * np.abs(x64)) / np.sqrt(bb)
                  + 2 * (n + 8) * 2.0 ** -53 * ref)
            print(f"{what}: true residual {res[j]:.6e}, exact r1 gives {ref:.6e}, difference {abs(res[j] - ref):.3e}, bound {tb:.3e}")
            assert abs(res[j] - ref) <= tb, (what, res[j], ref, tb)


# ------------------------------------------------------------------------------------------------
# 3. the first Jacobi step with M_j = diag(A) + s_j I
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 513, 1030])
def test_first_shifted_jacobi_step_is_exact_and_a_zero_sum_is_refused(lam, n):
    """A's diagonal is d - 1 with d_i in {1, 2, 4, 8}: zeros among it, where today's Jacobi refuses.  Shift 1 in every column lifts
    it to d: dinv = 1 / d exactly, z0 = b / d, and the step is exact_data.first_pcg_step(b, d, (A + I) z0).  With shift 0 in column 1
    of 3 the sum is zero in that column at the first row with d_i = 1: refused, naming that row and column, nothing iterated and
    no batched solution left."""
    assert n <= E.MAX_EXACT_N_FP32_JACOBI
    d = E.pow2_diagonal(n, 61 * n)
    assert (d == 1).any()
    first_zero = int(np.argmax(d == 1))
    B = [E.int_vec(n, 67 * n + j) for j in range(8)]
    with lam.Solver(lam.F64) as s64, lam.Solver(lam.F32) as s32:
        s64.set_problem(n)
        s32.set_problem(n)
        AZ = E.generate(n, [s64.upload_rows, s32.upload_rows], [b / d for b in B], diag=d - 1)
        AZ = [az + b / d for az, b in zip(AZ, B)]                                  # (A + I) z0
        for dtype_name, s in (("F64", s64), ("F32", s32)):
            vdt = s.vec_dtype
            _assert_bits(s.diagonal()[None], (d - 1).astype(vdt)[None], f"{dtype_name} n={n} diagonal")
            for nrhs in (1, 3, 8):
                what = f"{dtype_name} n={n} nrhs={nrhs}"
                s.set_rhs_many(np.stack(B[:nrhs]))
                with pytest.raises(lam.LamHipError) as e:                          # unshifted: the zero diagonal is refused as ever
                    s.solve_many(1, 1e-30, lam.PC_JACOBI)
                assert e.value.code == EINVAL and f"row {first_zero} " in str(e.value), e.value
                s.set_shifts([1.0] * nrhs)
                for rep in range(2):                                               # the second run meets the cached dinv
                    conv = s.solve_many(1, 1e-30, lam.PC_JACOBI)
                    X = s.solutions()
                    assert not conv.any() and list(s.num_iters_many) == [2] * nrhs and s.get_option("multi_rhs_k") == K_FOR[nrhs]
                    steps = [E.first_pcg_step(B[j], d, AZ[j], vdt) for j in range(nrhs)]
                    _assert_bits(X, np.stack([x1 + vdt(0) for _, x1, _, _ in steps]), what)
                    for j, (alpha, _, bb, r1) in enumerate(steps):
                        re_host, bound = E.rel_err_bound(B[j], AZ[j], alpha, r1, bb, U_TV[dtype_name])
                        assert abs(s.rel_err_many[j] - re_host) <= bound, (what, j, s.rel_err_many[j], re_host, bound)
                if nrhs >= 3:
                    sh = [1.0] * nrhs
                    sh[1] = 0.0
                    s.set_shifts(sh)
                    for x0 in (None, np.stack(B[:nrhs])):
                        with pytest.raises(lam.LamHipError) as e:
                            s.solve_many(1, 1e-30, lam.PC_JACOBI, x0)
                        assert e.value.code == EINVAL and f"row {first_zero}, column 1 " in str(e.value), e.value
                        with pytest.raises(lam.LamHipError) as e:
                            s.solutions()
                        assert e.value.code == ESTATE
                    s.solve_many(1, 1e-30)                                         # the plain shifted batch does not need the diagonal
                    assert list(s.num_iters_many) == [2] * nrhs


# ------------------------------------------------------------------------------------------------
# 4. a column does not depend on its neighbours
# ------------------------------------------------------------------------------------------------
def _columns_alone(lam, s, B, sh, cap, tol, what, early=None):
    """early: precond -> the right-hand side of column 1 that stops after one step under that preconditioner (default: B[1])"""
    B = B.copy()
    for precond in (lam.PC_NONE, lam.PC_JACOBI):
        if early is not None:
            B[1] = early[precond]
        s.set_rhs_many(B)
        s.set_shifts(sh)
        s.solve_many(cap, tol, precond)
        X, it, cv, re = _result(s)
        assert s.get_option("multi_rhs_k") == 8
        assert cv[1] and it[1] <= 2 and (it == cap + 1).any(), (what, precond, it, cv, re)
        # the same columns in the reverse order: column j with its shift in slot 7 - j, between other neighbours
        s.set_rhs_many(B[::-1])
        s.set_shifts(sh[::-1])
        s.solve_many(cap, tol, precond)
        Xr, itr, cvr, rer = _result(s)
        _assert_same_run((Xr[::-1].copy(), itr[::-1], cvr[::-1], rer[::-1].copy()), (X, it, cv, re), f"{what} precond={precond}: columns reversed")
        for j in range(8):
            s.set_rhs_many(B[j:j + 1])
            s.set_shifts(sh[j:j + 1])
            s.solve_many(cap, tol, precond)
            assert s.get_option("multi_rhs_k") == 1
            w = (f"{what} precond={precond} column {j} shift {sh[j]} (shown as column 0): alone {int(s.num_iters_many[0])} iterations, "
                 f"rel_err {s.rel_err_many[0]!r}; in the batch {int(it[j])}, {re[j]!r}")
            if sh[j] == 0:
                # alone, the zero shift runs the unshifted kernels; in the batch the column passes through fma(0, p, s): the same value,
                # but -0 + 0 = +0, so the sign of a zero may differ: == on finite data, not the bits
                assert np.isfinite(X[j]).all() and np.array_equal(s.solutions()[0], X[j]), w
            else:
                _assert_bits(s.solutions(), X[j:j + 1], w)
            assert s.num_iters_many[0] == it[j] and s.converged_many[0] == cv[j] and s.rel_err_many[0] == re[j], w


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_a_column_of_the_shifted_batch_is_the_column_alone(lam, dtype_name):
    """n = 1030 (past the K = 8 and the K = 4 tile), cap 12, tolerance 1e-5, eight different shifts, plain and Jacobi: column j of the
    batch of 8 against the same right-hand side alone at K = 1 under its own shift, and against itself in another slot.  Column 1
    is an eigenvector of A, so of every A + s I, and stops early; under Jacobi it is M v for an eigenvector v of the pencil
    (A + s_1 I, M), M = diag(A) + s_1 I, which is what stops the preconditioned recurrence after one step.
    The matrix is tridiagonal with a NON-constant diagonal, A = tridiag(1, 2 + i mod 3, 1), uploaded from the host.  K = 8 and K = 1
    stage p in tiles of different width and so add up a DENSE row's products in different orders: across K, a dense system agrees
    to rounding only, shifted or not (the unshifted batch's tests compare columns across slots of one K, never across K).  A
    tridiagonal row has three products, which every lane meets in one order whatever the tile, so the comparison across K is bit
    for bit here as it is on tridiag(1,2,1) past the wrap; the diagonal varies so that M_j = diag(A) + s_j I has a different dinv
    in every row AND column."""
    n, dt = 1030, NP[dtype_name]
    i = np.arange(n)
    A = np.diag(2.0 + i % 3) + np.diag(np.ones(n - 1), 1) + np.diag(np.ones(n - 1), -1)
    B = np.random.default_rng(n).uniform(-1, 1, (8, n)).astype(dt)
    sh = np.array(REAL_SHIFTS)
    m = np.diag(A) + sh[1]
    w = np.linalg.eigh((A + sh[1] * np.eye(n)) / np.sqrt(m)[:, None] / np.sqrt(m)[None, :])[1][:, n // 2]
    early = {lam.PC_NONE: np.linalg.eigh(A)[1][:, n // 2].astype(dt), lam.PC_JACOBI: (np.sqrt(m) * w).astype(dt)}
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.set_matrix(A)
        _columns_alone(lam, s, B, sh, 12, 1e-5, f"{dtype_name} n={n}", early)      # cond(A) = 6.6: 1e-5 takes 15 steps


def test_a_dense_shifted_column_does_not_depend_on_its_slot_or_neighbours(lam, spd):
    """The dense smoke system (n = 513 and 1030: past the K = 8 tile, and past the K = 4 tile), eight shifts, plain and Jacobi, cap 12
    with a tolerance the strongly shifted columns meet: the batch against the same columns in the reverse order (column j with its
    shift in slot 7 - j), and, at K = 4, columns 2..5 as a batch of their own slots 0..3 of a batch of 4 against slots 0..3 of
    another batch of 4 with other neighbours -- within ONE K, where a dense row is added up in one order."""
    dtype_name, n, dt, A, B, X0, s = spd
    if n < 513:
        return
    sh = np.array(REAL_SHIFTS)
    for precond in (lam.PC_NONE, lam.PC_JACOBI):
        what = f"{dtype_name} n={n} precond={precond}"
        s.set_rhs_many(B)
        s.set_shifts(sh)
        s.solve_many(12, 1e-3, precond)
        X, it, cv, re = _result(s)
        assert cv.any() and not cv.all() and np.isfinite(X).all(), (what, it, cv)
        s.set_rhs_many(B[::-1])
        s.set_shifts(sh[::-1])
        s.solve_many(12, 1e-3, precond)
        Xr, itr, cvr, rer = _result(s)
        _assert_same_run((Xr[::-1].copy(), itr[::-1], cvr[::-1], rer[::-1].copy()), (X, it, cv, re), what + ": columns reversed")
        for cols in ((1, 3, 5, 7), (7, 5, 3, 1), (3, 0, 7, 2)):                      # K = 4: columns 3 and 7 among changing neighbours
            c = list(cols)
            s.set_rhs_many(B[c])
            s.set_shifts(sh[c])
            s.solve_many(12, 1e-3, precond)
            got = _result(s)
            assert s.get_option("multi_rhs_k") == 4
            if cols == (1, 3, 5, 7):
                first = {j: tuple(a[q:q + 1].copy() for a in got) for q, j in enumerate(c)}
            else:
                for q, j in enumerate(c):
                    if j in first:
                        _assert_same_run(tuple(a[q:q + 1].copy() for a in got), first[j], f"{what}: column {j} in slot {q} of {cols}")


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_first_shifted_jacobi_step_is_exact_past_the_wrap(lam, dtype_name):
    """n = 65537 on the device-filled tridiag(1,2,1), shifts 0 / 2 / 6 so that M_j = (2 + s_j) I is 2 I / 4 I / 8 I: the first Jacobi
    step is exact_data.first_pcg_step on (A + s_j I) z0 with z0 = b / (2 + s_j), in EVERY row -- x1 = alpha z0 bit for bit pins
    dinv[i K + j] of shifted_dinv_kernel for the rows a thread takes in its second trip (65536 on), against the host and not
    against another launch of the device.  fp32: |8 (A + s I) z0| <= 8 * 10 * 8 stays far inside 2^24."""
    n = 65537
    shifts = (2.0, 6.0, 0.0, 6.0, 2.0, 0.0, 2.0, 6.0)
    B = np.stack([E.int_vec(n, 71 * n + j) for j in range(8)])
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.generate_matrix(n)
        vdt = s.vec_dtype
        for nrhs in (1, 3, 8):
            s.set_rhs_many(B[:nrhs])
            s.set_shifts(shifts[:nrhs])
            s.solve_many(1, 1e-30, lam.PC_JACOBI)
            X, it, cv, re = _result(s)
            assert list(it) == [2] * nrhs and s.get_option("multi_rhs_k") == K_FOR[nrhs]
            for j in range(nrhs):
                d = np.full(n, 2.0 + shifts[j])
                z0 = B[j] / d
                Az = E.tridiag_product(z0) + shifts[j] * z0
                alpha, x1, bb, r1 = E.first_pcg_step(B[j], d, Az, vdt)
                what = f"{dtype_name} n={n} nrhs={nrhs} column {j} shift {shifts[j]} (alpha {alpha!r})"
                _assert_bits(X[j:j + 1], (x1 + vdt(0))[None], what)
                re_host, bound = E.rel_err_bound(B[j], Az, alpha, r1, bb, U_TV[dtype_name])
                assert abs(re[j] - re_host) <= bound, (what, re[j], re_host, bound)


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_a_column_of_the_shifted_batch_is_the_column_alone_past_the_wrap(lam, dtype_name):
    """n = 65537 > 256 workgroups x 256 threads on the device-filled tridiag(1,2,1): a thread of every vector kernel, and of the
    launch that builds the K-wide dinv, handles a second element."""
    n = 65537
    rng = np.random.default_rng(n)
    i = np.arange(1, n + 1)
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.generate_matrix(n)
        B = np.stack([np.ones(n), np.sin(3 * np.pi * i / (n + 1))] + [rng.uniform(-1, 1, n) for _ in range(6)]).astype(s.vec_dtype)
        _columns_alone(lam, s, B, np.array(REAL_SHIFTS), 12, 1e-3, f"{dtype_name} n={n}")


# ------------------------------------------------------------------------------------------------
# 5. past the first step: every column, iteration by iteration
# ------------------------------------------------------------------------------------------------
def test_every_shifted_column_tracks_the_oracle_iteration_by_iteration_fp64(lam, oracle):
    """solve_many(k, 1e-30), k = 1, 2, 5, 20, 40, under tests/shifted_data.py's eight shifts: column j against oracle.cg_solve on
    A + s_j I formed on the host, with the single solve's gates (tests/tracking_data.py)."""
    A, B, sh = S.shifted_tracking_columns()
    gates = {k: (g_res, g_x) for k, g_res, g_x in ITERATION_TRACKING_GATES if k in TRACKED_K}
    with lam.Solver(lam.F64) as s:
        s.set_matrix(A)
        s.set_rhs_many(B)
        s.set_shifts(sh)
        for k in sorted(gates):
            s.solve_many(k, 1e-30)
            X, it, _, re = _result(s)
            assert (it == k + 1).all(), (k, it)
            for j in range(8):
                x_ref, st_ref = oracle.cg_solve(S.formed(A, sh[j]), B[j], k, 1e-30)
                d_re = abs(re[j] / st_ref["rel_err"] - 1)
                d_x = np.linalg.norm(X[j] - x_ref) / np.linalg.norm(x_ref)
                print(f"F64 k={k} column {j} shift {sh[j]}: rel_err off by {d_re:.3e} (gate {gates[k][0]:.1e}), x by {d_x:.3e} (gate {gates[k][1]:.1e})")
                assert st_ref["num_iters"] == k + 1 and d_re < gates[k][0] and d_x < gates[k][1], (k, j, d_re, d_x, gates[k])


def test_every_shifted_jacobi_column_tracks_the_reference_iteration_by_iteration_fp64(lam):
    """The fp64 K-wide-dinv instantiations past the first step: solve_many(k, 1e-30, PC_JACOBI) under the eight shifts against
    pcg_reference.pcg on A + s_j I formed on the host with that matrix's jacobi_dinv -- the reference and the gates of
    tests/test_gpu_batch_recurrence.py::test_jacobi_rel_err_tracks_the_reference_iteration_by_iteration -- x and rel_err, at
    k = 1, 2, 5, 20.  k = 40 is left to the fp32 case: there the column with the largest shift has converged to 1e-11 of b and two
    HOST statements of this recurrence already differ by 6e-11 in rel_err (tests/test_shifted_cpu.py), six times that k's gate."""
    A, B, sh = S.shifted_tracking_columns()
    gates = {k: (g_res, g_x) for k, g_res, g_x in ITERATION_TRACKING_GATES if k in TRACKED_K and k <= 20}
    with lam.Solver(lam.F64) as s:
        s.set_matrix(A)
        s.set_rhs_many(B)
        s.set_shifts(sh)
        for k in sorted(gates):
            s.solve_many(k, 1e-30, lam.PC_JACOBI)
            X, it, _, re = _result(s)
            assert (it == k + 1).all(), (k, it)
            for j in range(8):
                M = S.formed(A, sh[j])
                x_ref, st_ref = R.pcg(M, B[j], k, 1e-30, R.jacobi_dinv(M), np.float64)
                d_re = abs(re[j] / st_ref["rel_err"] - 1)
                d_x = np.linalg.norm(X[j] - x_ref) / np.linalg.norm(x_ref)
                print(f"F64 jacobi k={k} column {j} shift {sh[j]}: rel_err off by {d_re:.3e} (gate {gates[k][0]:.1e}), x by {d_x:.3e} (gate {gates[k][1]:.1e})")
                assert d_re < gates[k][0] and d_x < gates[k][1], (k, j, d_re, d_x, gates[k])


@pytest.mark.parametrize("precond_name", ["plain", "jacobi"])
def test_every_shifted_column_tracks_the_restatement_iteration_by_iteration_fp32(lam, precond_name):
    """fp32, same k: column j against pcg_reference.pcg_ordered(order="rows") on A + s_j I formed on the host (Jacobi: with
    jacobi_dinv of that matrix).  Gate per k: 10 x the largest spread, over the columns, that this reference shows against ITSELF
    between its three summation orders on these very systems, x or rel_err, whichever is larger -- tracking_data's rule for
    FP32_TRACKING_GATE, computed here as tests/test_gpu_warm_start.py computes it."""
    dt = np.float32
    A, B, sh = S.shifted_tracking_columns()
    B = B.astype(dt)
    jac = precond_name == "jacobi"
    Ms = [S.formed(A, sh[j], dt) for j in range(8)]
    dinvs = [R.jacobi_dinv(M, dt) if jac else None for M in Ms]
    with lam.Solver(lam.F32) as s:
        s.set_matrix(A)
        s.set_rhs_many(B)
        s.set_shifts(sh)
        for k in TRACKED_K:
            ref = {o: [R.pcg_ordered(Ms[j], B[j], k, 1e-30, dinvs[j], dt, o) for j in range(8)] for o in R.ORDERS}
            sp_re = max(abs(ref[a][j][1]["rel_err"] / ref[b][j][1]["rel_err"] - 1) for a in R.ORDERS for b in R.ORDERS if a != b for j in range(8))
            sp_x = max(np.linalg.norm(ref[a][j][0].astype(np.float64) - ref[b][j][0]) / np.linalg.norm(ref[b][j][0].astype(np.float64))
                       for a in R.ORDERS for b in R.ORDERS if a != b for j in range(8))
            gate = 10 * max(sp_re, sp_x)          # tracking_data's rule: one gate per k for x and rel_err alike, from the larger spread
            s.solve_many(k, 1e-30, lam.PC_JACOBI if jac else lam.PC_NONE)
            X, it, _, re = _result(s)
            assert (it == k + 1).all(), (k, it)
            for j in range(8):
                x_ref, st_ref = ref["rows"][j]
                d_re = abs(re[j] / st_ref["rel_err"] - 1)
                d_x = np.linalg.norm(X[j].astype(np.float64) - x_ref) / np.linalg.norm(x_ref.astype(np.float64))
                print(f"F32 {precond_name} k={k} column {j} shift {sh[j]}: rel_err off by {d_re:.3e}, x by {d_x:.3e} (gate {gate:.1e}; reference "
                      f"spread rel_err {sp_re:.1e}, x {sp_x:.1e})")
                assert d_re < gate and d_x < gate, (precond_name, k, j, d_re, d_x, sp_re, sp_x)


# ------------------------------------------------------------------------------------------------
# 6. guess, continuation, path-following
# ------------------------------------------------------------------------------------------------
def test_zero_guess_under_shifts_is_the_shifted_solve_from_zero(lam, spd):
    dtype_name, n, dt, A, B, X0, s = spd
    sh = np.array(REAL_SHIFTS)
    for nrhs in (1, 3, 8):
        for precond in (lam.PC_NONE, lam.PC_JACOBI):
            s.set_rhs_many(B[:nrhs])
            s.set_shifts(sh[:nrhs] + 0.5)
            s.solve_many(min(6, n), 3e-2, precond)
            want = _result(s)
            s.solve_many(min(6, n), 3e-2, precond, x0=np.zeros((nrhs, n), dt))
            _assert_same_run(_result(s), want, f"{dtype_name} n={n} nrhs={nrhs} precond={precond}")


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_exact_guess_of_the_shifted_system_is_born_stopped(lam, integer_system, dtype_name):
    n, dense, _, V, _, _, AV, ctx = integer_system
    s, dt = ctx[dtype_name], NP[dtype_name]
    sh = np.array(INT_SHIFTS, np.float64)
    Bs = AV + sh[:, None] * V
    keep = [j for j in range(8) if Bs[j].any()]                                    # n = 1: (a + s) v may be 0
    Bs, XS, sh = Bs[keep], V[keep].astype(dt), sh[keep]
    for nrhs in sorted({1, min(3, len(keep)), len(keep)}):
        s.set_rhs_many(Bs[:nrhs])
        s.set_shifts(sh[:nrhs])
        for cap in (0, 7):
            conv = s.solve_many(cap, 1e-30, x0=XS[:nrhs])
            X, it, cv, re = _result(s)
            what = f"{dtype_name} n={n} nrhs={nrhs} cap={cap}"
            assert conv.all() and (it == 0).all() and (re == 0.0).all() and s.stats["num_iters"] == 0, (what, it, re)
            _assert_bits(X, XS[:nrhs], what)
            assert (s.true_residuals() == 0.0).all(), (what, s.true_residuals())
        if sh[:nrhs].any():
            s.set_shifts(None)                                                     # against A alone the guess is off by s x
            s.solve_many(0, 1e-30, x0=XS[:nrhs])
            assert (s.rel_err_many[sh[:nrhs] != 0] > 0).all()


def test_path_following_continues_from_the_previous_shifts_solution(lam, spd):
    """Solve at shifts s, set_shifts(s'), continue with x0 = NULL == downloading X and passing it as x0_host under s', bit for bit;
    and true_residuals() after set_shifts measures against the new shifts: numpy's fp64 ||b - (A + s' I) x|| / ||b|| within
    tests/shifted_data.py's bound (the product's and the subtraction's roundings, tests/test_gpu_warm_start.py's gate with the
    epilogue's one more operation)."""
    dtype_name, n, dt, A, B, X0, s = spd
    u = U_TV[dtype_name]
    sh0, sh1 = np.array(REAL_SHIFTS) + 1.0, np.array(REAL_SHIFTS)[::-1].copy()
    k1, k2 = min(3, n), 4
    absA = np.abs(A)
    for nrhs in (1, 3, 8):
        for precond in (lam.PC_NONE, lam.PC_JACOBI):
            what = f"{dtype_name} n={n} nrhs={nrhs} precond={precond}"
            s.set_rhs_many(B[:nrhs])
            s.set_shifts(sh0[:nrhs])
            s.solve_many(k1, 1e-30, precond)
            X1 = s.solutions()
            res0 = s.true_residuals()
            s.set_shifts(sh1[:nrhs])
            _assert_bits(s.solutions(), X1, what + ": the solution after set_shifts")
            res1 = s.true_residuals()
            for j in range(nrhs):
                b, x = B[j].astype(np.float64), X1[j].astype(np.float64)
                for got, sj in ((res0[j], sh0[j]), (res1[j], sh1[j])):
                    ref = np.linalg.norm(b - A @ x - sj * x) / np.linalg.norm(b)
                    bound = S.true_residual_bound(absA @ np.abs(x), b, sj, x, n, u) + 2 * (n + 8) * 2.0 ** -53 * ref
                    print(f"{what} column {j} shift {sj}: device {got:.6e}, numpy {ref:.6e}, difference {abs(got - ref):.3e}, bound {bound:.3e}")
                    assert abs(got - ref) <= bound, (what, j, sj, got, ref, bound)
            s.solve_many(k2, 1e-30, precond, x0="continue")
            got = _result(s)
            s.set_rhs_many(B[:nrhs])
            s.set_shifts(sh1[:nrhs])
            s.solve_many(k2, 1e-30, precond, x0=X1)
            _assert_same_run(got, _result(s), what)
            if n > 1:
                s.set_shifts(sh0[:nrhs])
                s.solve_many(k2, 1e-30, precond, x0=X1)
                assert not np.array_equal(s.solutions(), got[0]), what + ": the continuation ran under the old shifts"


# ------------------------------------------------------------------------------------------------
# 7. refusals and lifetime
# ------------------------------------------------------------------------------------------------
def test_refusals(lam, monkeypatch):
    n = 64
    A = R.smoke_system(n)[0]
    B = np.ones((2, n))

    def refused(s, code, fn, *args, **kw):
        launches = s.get_option("hip_calls_launch")
        with pytest.raises(lam.LamHipError) as e:
            fn(*args, **kw)
        assert e.value.code == code, (fn, e.value)
        msg = (s._L.lam_hip_last_error(s._h) or b"").decode()
        assert msg, fn
        assert s.get_option("hip_calls_launch") == launches
        return msg

    with lam.Solver(lam.F64, device_ids=[0, 0]) as s:
        s.set_matrix(A)
        s.nrhs = 2
        assert "shard" in refused(s, EINVAL, s.set_shifts, [1.0, 2.0])
        assert "shard" in refused(s, EINVAL, s.set_shifts, None)
    with lam.Solver(lam.BF16) as s:
        s.set_matrix(A)
        s.nrhs = 2
        assert "BF16" in refused(s, EINVAL, s.set_shifts, [1.0, 2.0])
    monkeypatch.setenv("LAM_HIP_FORCE_RCCL", "1")      # a one-rank communicator: the rank mode on one GPU
    with lam.Solver(lam.F64, rank=0, nranks=1, device_id=0, unique_id=None) as s:
        monkeypatch.delenv("LAM_HIP_FORCE_RCCL")
        s.set_problem(n)
        s.upload_rows(0, A)
        s.nrhs = 2
        assert "rank mode" in refused(s, EINVAL, s.set_shifts, [1.0, 2.0])
    with lam.Solver(lam.F64) as s:
        s.n, s.nrhs = n, 2
        refused(s, ESTATE, s.set_shifts, [1.0, 2.0])                               # no problem yet
        s.set_matrix(A)
        assert "lam_hip_set_rhs_many" in refused(s, ESTATE, s.set_shifts, [1.0, 2.0])      # before the right-hand sides
        s.set_rhs_many(B)
        s.solve_many(5, 1e-9)
        want = _result(s)
        s.set_shifts([0.5, 2.0])
        s.solve_many(5, 1e-9)
        shifted = _result(s)
        assert not np.array_equal(shifted[0], want[0])
        for bad, word in (([-1.0, 1.0], "-1"), ([1.0, -1e-300], "-1e-300"), ([np.nan, 1.0], "nan"), ([1.0, np.inf], "inf"),
                          ([-np.inf, 1.0], "-inf")):
            msg = refused(s, EINVAL, s.set_shifts, bad)
            assert word in msg and f"shift {int(np.argmax([not (v >= 0 and np.isfinite(v)) for v in bad]))} " in msg, msg
        for wrong in ([1.0], [1.0, 2.0, 3.0], [1.0] * 9, []):
            refused(s, EINVAL, s.set_shifts, wrong)
        assert s._L.lam_hip_set_shifts_many(None, 2, None) == EINVAL
        # a refused call leaves the shifts in force
        s.solve_many(5, 1e-9)
        _assert_same_run(_result(s), shifted, "after refused set_shifts calls")
        # gemv_many ignores the shifts; set_rhs_many clears them
        Y = s.gemv_many(B)
        s.set_shifts(None)
        _assert_bits(s.gemv_many(B), Y, "gemv_many with and without shifts")
        s.set_shifts([0.5, 2.0])
        s.set_rhs_many(B)
        s.solve_many(5, 1e-9)
        _assert_same_run(_result(s), want, "set_rhs_many clears the shifts")
        s.set_shifts([0.5, 2.0])
        s.set_problem(n)                                                           # and so does set_problem
        s.upload_rows(0, A)
        refused(s, ESTATE, s.set_shifts, [0.5, 2.0])
        s.set_rhs_many(B)
        s.solve_many(5, 1e-9)
        _assert_same_run(_result(s), want, "set_problem clears the shifts")
        # the convenience: b replicated
        conv = s.solve_shifted(B[0], [0.5, 2.0], 5, 1e-9)
        assert conv.shape == (2,)
        _assert_same_run(_result(s), shifted, "solve_shifted")
    with lam.Solver(lam.F32) as s:
        s.set_matrix(A)
        s.set_rhs_many(B)
        msg = refused(s, EINVAL, s.set_shifts, [1.0, 1e39])                        # finite in fp64, Inf in the vector dtype
        assert "shift 1 " in msg and "1e+39" in msg, msg
        s.set_shifts([1.0, 3e38])


# ------------------------------------------------------------------------------------------------
# 8. driver
# ------------------------------------------------------------------------------------------------
def test_driver_shifts():
    """tridiag(1,2,1), n = 1024, b = 1 in every column, -S 0,0.5,4 -J -T: converges, echoes the shifts as the last CSV field, and
    the iteration counts do not increase with the shift (the condition number only falls).  With -w the second stage continues
    under the same shifts."""
    exe = os.path.join(ROOT, PKG_NAME, "test", "test_CG_multi_rhs.out")
    n, tol = 1024, 1e-9
    for extra, fields in ((["-J", "-T"], 12), (["-T"], 12), (["-w", "10", "-T"], 12), ([], 11)):
        r = subprocess.run([exe, "-s", str(n), "-i", "3000", "-e", str(tol), "-S", "0,0.5,4"] + extra, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = [ln.split(",") for ln in r.stdout.strip().splitlines()]
        assert len(lines) == 3 and all(ln[0] == str(n) and len(ln) == fields for ln in lines), r.stdout
        assert [float(ln[-1]) for ln in lines] == [0.0, 0.5, 4.0], r.stdout
        iters = [int(ln[7]) for ln in lines]
        print(extra, iters, [ln[8] for ln in lines])
        assert all(float(ln[8]) < tol for ln in lines) and iters[0] >= iters[1] >= iters[2] >= 1 and iters[0] > iters[2], (extra, r.stdout)
        if "-T" in extra:
            assert all(float(ln[10]) < 1e-7 for ln in lines), r.stdout
