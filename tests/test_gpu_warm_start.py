"""The batched solve from an initial guess and the batch's true residuals: lam_hip_solve_many_x0 / lam_hip_true_residual_many
(include/lam_hip.h), i.e. the GUESS = true instantiations of multi_init_kernel / multi_init_scalars_kernel, multi_residual_kernel
and multi_residual_scalars_kernel (csrc/lam_kernels.h).

Sizes: N in {1, 5, 255, 256, 257, 513, 4097} -- workgroup edges of the vector kernels, the K = 8 fp64 product tile of 512 columns,
one past the 4096 tile -- and N = 65537 on the device-filled tridiag(1,2,1) for the vector kernels' grid-stride wrap.

 1. a zero guess is lam_hip_solve_many_pc, bit for bit (catches another order of the r.r / r.z partial sums);
 2. an exact guess is born stopped: 0 iterations, x = x0 bit for bit, true residual exactly 0; a partly exact batch;
 3. the exact shift identity on integer data: warm on (b, x0) == cold on c = b - A x0;
 4. the known first step from a non-zero integer guess, plain and Jacobi on the {1, 2, 4, 8} diagonal (tests/exact_data.py);
 5. the Jacobi scaling identity of tests/test_gpu_batch_recurrence.py (A) with a guess (catches a wrong dinv index in the init pass);
 6. continuation from the batch's own solution == the downloaded solution passed explicitly; LAM_HIP_ESTATE where there is none;
 7. rel_err iteration by iteration against tests/warm_start_reference.py, gate = 10 x that reference's own spread between orders;
 8. true residuals against numpy's fp64 ones within the product's rounding bound, exact on integer data, 0/0 for b_j = 0;
 9. NaN confinement, and a guess run at K = 4 / 2 / 1 over what a K = 8 batch with a NaN column left behind (inside 4);
10. refusals; 11. past the grid-stride wrap; 12. the driver's -w and -T."""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import exact_data as E
import pcg_reference as R
import warm_start_reference as W
from conftest import ROOT, PKG_NAME
from tracking_data import scaled_case

pytestmark = pytest.mark.gpu

DTYPES = ("F64", "F32")
NP = {"F64": np.float64, "F32": np.float32}
U_TV = {"F64": 2.0 ** -53, "F32": 2.0 ** -24}
K_FOR = {1: 1, 2: 2, 3: 4, 4: 4, 5: 8, 6: 8, 7: 8, 8: 8}
KS = (1, 2, 5, 40)
SIZES = (1, 5, 255, 256, 257, 513, 4097)
EINVAL, ESTATE = -1, -6


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


def _nrhs_set(n):
    return range(1, 9) if n <= 513 else (1, 3, 8)


# ------------------------------------------------------------------------------------------------
# 1, 5: the scaled systems of tests/test_gpu_batch_recurrence.py (A): C with a unit diagonal, A = S C S
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[(d, n) for n in SIZES for d in DTYPES], ids=lambda p: f"{p[0]}-{p[1]}")
def scaled(lam, request):
    """One pair of contexts per (dtype, n), C and A = S C S uploaded once, shared by the tests of cases 1 and 5."""
    dtype_name, n = request.param
    dt = NP[dtype_name]
    Cm, e, s, A, Bh = scaled_case(n, dt)
    with lam.Solver(getattr(lam, dtype_name)) as sc, lam.Solver(getattr(lam, dtype_name)) as sa:
        sc.set_matrix(Cm)
        sa.set_matrix(A)
        yield dtype_name, n, dt, Cm, s, Bh, sc, sa


def test_zero_guess_is_the_plain_solve_bit_for_bit(lam, scaled):
    """solve_many(x0 = 0) against solve_many on the same context at rel_error = 0, k = 1, 2, 5, 40: plain on C, Jacobi on A = S C S
    (a non-constant power-of-two diagonal) and plain on A."""
    dtype_name, n, dt, Cm, s, Bh, sc, sa = scaled
    Bs = (s * Bh).astype(dt)
    for nrhs in _nrhs_set(n):
        Z = np.zeros((nrhs, n), dt)
        sc.set_rhs_many(Bh[:nrhs])
        sa.set_rhs_many(Bs[:nrhs])
        for ctx, precond in ((sc, lam.PC_NONE), (sa, lam.PC_JACOBI), (sa, lam.PC_NONE)):
            for k in sorted({min(k, n) for k in KS}):
                ctx.solve_many(k, 0.0, precond)
                want = _result(ctx)
                ctx.solve_many(k, 0.0, precond, x0=Z)
                assert ctx.get_option("multi_rhs_k") == K_FOR[nrhs]
                _assert_same_run(_result(ctx), want, f"{dtype_name} n={n} nrhs={nrhs} precond={precond} k={k}")


@pytest.mark.parametrize("n", [257, 513])
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_zero_guess_is_the_plain_solve_when_a_column_freezes_early(lam, dtype_name, n):
    """Tolerance 1e-3, cap 12: column 1 is an eigenvector of C and stops after a step or two, the others run to the cap."""
    dt, cap, tol = NP[dtype_name], 12, 1e-3
    Cm, e, s, A, Bh = scaled_case(n, dt)
    Bh = Bh.copy()
    Bh[1] = np.linalg.eigh(Cm)[1][:, n // 2].astype(dt)
    Bs = (s * Bh).astype(dt)
    with lam.Solver(getattr(lam, dtype_name)) as sc, lam.Solver(getattr(lam, dtype_name)) as sa:
        sc.set_matrix(Cm)
        sa.set_matrix(A)
        for ctx, B, precond in ((sc, Bh, lam.PC_NONE), (sa, Bs, lam.PC_JACOBI)):
            for nrhs in (3, 8):
                ctx.set_rhs_many(B[:nrhs])
                ctx.solve_many(cap, tol, precond)
                want = _result(ctx)
                assert want[2][1] and want[1][1] <= 2 and not want[2][2:].any() and (want[1][2:] == cap + 1).all(), (want[1], want[2])
                ctx.solve_many(cap, tol, precond, x0=np.zeros((nrhs, n), dt))
                _assert_same_run(_result(ctx), want, f"{dtype_name} n={n} nrhs={nrhs} precond={precond}")


def test_jacobi_from_a_scaled_guess_is_the_plain_run_scaled_bit_for_bit(lam, scaled):
    """A = S C S, b -> S b, x0 -> S^-1 x0: x_jacobi[i] == 2^-e_i x_plain[i] bit for bit (A S^-1 x0 = S (C x0) term by term, so
    r0 scales by S exactly and the argument of tests/test_gpu_batch_recurrence.py (A) runs from there)."""
    dtype_name, n, dt, Cm, s, Bh, sc, sa = scaled
    X0 = np.random.default_rng(1000 + n).uniform(-1, 1, (8, n)).astype(dt)
    Bs, X0s = (s * Bh).astype(dt), (X0 / s).astype(dt)
    assert np.array_equal(X0s.astype(np.float64) * s, X0.astype(np.float64))          # exact
    for nrhs in (1, 3, 8):
        sc.set_rhs_many(Bh[:nrhs])
        sa.set_rhs_many(Bs[:nrhs])
        for k in sorted({min(k, n) for k in KS}):
            sc.solve_many(k, 0.0, x0=X0[:nrhs])
            Xp, itp, _, rep = _result(sc)
            sa.solve_many(k, 0.0, lam.PC_JACOBI, x0=X0s[:nrhs])
            Xj, itj, _, rej = _result(sa)
            what = f"{dtype_name} n={n} nrhs={nrhs} k={k}"
            assert (itp == k + 1).all() and (itj == k + 1).all() and np.isfinite(Xp).all() and np.isfinite(rej).all(), (what, itp, itj)
            _assert_bits(Xj, (Xp / s).astype(dt), what)


# ------------------------------------------------------------------------------------------------
# 2, 3, 6, 8 (integer part): tridiag(1,2,1) filled on the device, integer vectors
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[(d, n) for n in SIZES for d in DTYPES], ids=lambda p: f"{p[0]}-{p[1]}")
def tri(lam, request):
    dtype_name, n = request.param
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.generate_matrix(n)
        yield dtype_name, n, s


def _ints(n, seed, count=8):
    X = np.stack([E.int_vec(n, seed * 100003 + 31 * n + j) for j in range(count)])
    X[X == 0] = 1.0           # no zero vector at n = 1
    return X


def _shifted(X0, Cc):
    """c and b = c + A x0, no b the zero vector: where c = -A x0 (it happens at n = 1) c changes its sign, and b = 2 A x0 != 0."""
    AX0 = E.tridiag_product(X0.astype(np.float64))
    Cc = np.where((Cc + AX0).any(axis=1, keepdims=True), Cc, -Cc)
    assert (Cc + AX0).any(axis=1).all() and Cc.any(axis=1).all()
    return Cc, Cc + AX0


def test_exact_guess_is_born_stopped(lam, tri):
    dtype_name, n, s = tri
    dt = s.vec_dtype
    XS = _ints(n, 1).astype(dt)
    B = E.tridiag_product(XS).astype(dt)
    for precond in (lam.PC_NONE, lam.PC_JACOBI):
        for nrhs in _nrhs_set(n):
            what = f"{dtype_name} n={n} nrhs={nrhs} precond={precond}"
            s.set_rhs_many(B[:nrhs])
            for cap in (0, 7):
                conv = s.solve_many(cap, 1e-30, precond, x0=XS[:nrhs])
                X, it, cv, re = _result(s)
                assert conv.all() and (it == 0).all() and (re == 0.0).all() and s.stats["num_iters"] == 0 and s.stats["converged"] == 1, (what, it, re)
                assert s.get_option("multi_rhs_k") == K_FOR[nrhs]
                _assert_bits(X, XS[:nrhs], what)
                assert (s.true_residuals() == 0.0).all(), (what, s.true_residuals())
        # only columns 0 and 2 of 3 / 0, 2, 5, 6 of 8 get the exact guess: born stopped and untouched, the others run and are their own
        # single-column run
        for nrhs, exact in ((3, (0, 2)), (8, (0, 2, 5, 6))):
            G = XS[:nrhs] + dt(1)
            G[list(exact)] = XS[list(exact)]
            cap = min(5, n)
            s.set_rhs_many(B[:nrhs])
            s.solve_many(cap, 1e-30, precond, x0=G)
            X, it, cv, re = _result(s)
            what = f"{dtype_name} n={n} nrhs={nrhs} precond={precond} exact columns {exact}: iterations {it.tolist()}"
            assert all(it[j] == 0 and cv[j] and re[j] == 0.0 for j in exact), what
            _assert_bits(X[list(exact)], XS[list(exact)], what)
            for j in set(range(nrhs)) - set(exact):
                assert it[j] >= 1, what
                s.set_rhs_many(B[j:j + 1])
                s.solve_many(cap, 1e-30, precond, x0=G[j:j + 1])
                assert s.get_option("multi_rhs_k") == 1
                _assert_same_run(_result(s), (X[j:j + 1], it[j:j + 1], cv[j:j + 1], re[j:j + 1]), what + f" column {j} alone")


def test_max_iters_0_returns_the_start_and_integer_true_residuals_are_exact(lam, tri):
    """The k = 0 state: x = x0, rel_err = sqrt(rr0/bb), num_iters = max_iters + 1 = 1; and ||b - A x0|| / ||b|| of integer data, whose
    sums are exact integers in any order: 2 ulp (one division, one square root)."""
    dtype_name, n, s = tri
    dt = s.vec_dtype
    X0 = _ints(n, 3).astype(dt)
    Cc, B = _shifted(X0, _ints(n, 4))
    B = B.astype(dt)                                                               # b - A x0 = c exactly
    want = np.sqrt(np.sum(Cc * Cc, axis=1) / np.sum(B.astype(np.float64) ** 2, axis=1))
    for nrhs in (1, 3, 8):
        s.set_rhs_many(B[:nrhs])
        for precond in (lam.PC_NONE, lam.PC_JACOBI):
            conv = s.solve_many(0, 1e-30, precond, x0=X0[:nrhs])
            X, it, cv, re = _result(s)
            what = f"{dtype_name} n={n} nrhs={nrhs} precond={precond}"
            assert not conv.any() and (it == 1).all(), (what, it)
            _assert_bits(X, X0[:nrhs], what)
            res = s.true_residuals()
            for got in (re, res):
                assert (np.abs(got - want[:nrhs]) <= 2 * np.spacing(want[:nrhs])).all(), (what, got, want[:nrhs])
        assert (np.abs(s.true_residuals(1) - want[:1]) <= 2 * np.spacing(want[:1])).all()


def test_exact_shift_identity(lam, tri):
    """Integer b, x0 with c = b - A x0 exact.  The warm run on (b, x0) and the cold run on c at rel_error = 0 and equal caps share
    r, p, alpha and beta bit for bit, so rr_k is one number: rel_err_warm ||b|| == rel_err_cold ||c|| to 4 ulp (a division, a square
    root and a product round on each side).  x_warm and x0 + x_cold then differ by the roundings of the x updates alone: one per
    update and run, each at most eps/2 of the iterate it produces, plus the final x0 + x_cold: (2 k + 1) eps/2 max|x| <= 2 k eps
    max|x| elementwise, with max|x| the running maximum of both runs from a numpy replay (warm_start_reference, stencil product)."""
    dtype_name, n, s = tri
    dt = s.vec_dtype
    eps = float(np.finfo(dt).eps)
    X0 = _ints(n, 5)
    Cc, B = _shifted(X0, _ints(n, 6))
    nb, nc = np.sqrt(np.sum(B * B, axis=1)), np.sqrt(np.sum(Cc * Cc, axis=1))
    for nrhs in (1, 3, 8):
        for k in sorted({k for k in KS if k <= n}):
            s.set_rhs_many(B[:nrhs])
            s.solve_many(k, 0.0, x0=X0[:nrhs])
            Xw, itw, _, rew = _result(s)
            s.set_rhs_many(Cc[:nrhs])
            s.solve_many(k, 0.0)
            Xc, itc, _, rec = _result(s)
            what = f"{dtype_name} n={n} nrhs={nrhs} k={k}"
            assert (itw == k + 1).all() and (itc == k + 1).all(), (what, itw, itc)
            lhs, rhs = rew * nb[:nrhs], rec * nc[:nrhs]
            print(f"{what}: rel_err_warm ||b|| - rel_err_cold ||c|| = {((lhs - rhs) / np.spacing(rhs)).tolist()} ulp")
            # k = n included: there the last step annihilates the residual and rr is rounding noise, but the same noise in both runs
            assert (np.abs(lhs - rhs) <= 4 * np.spacing(rhs)).all(), (what, lhs, rhs)
            if nrhs == 3 or n <= 513:
                for j in range(nrhs):
                    _, sw = W.pcg_x0(E.tridiag_product, B[j], X0[j], k, 0.0, None, dt)
                    _, sc = W.pcg_x0(E.tridiag_product, Cc[j], np.zeros(n), k, 0.0, None, dt)
                    bound = 2 * k * eps * np.maximum(sw["x_absmax"], np.abs(X0[j]) + sc["x_absmax"]).astype(np.float64)
                    diff = np.abs(Xw[j].astype(np.float64) - (X0[j] + Xc[j].astype(np.float64)))
                    assert np.isfinite(diff).all() and (diff <= bound).all(), (what, j, float((diff / bound).max()))


def test_continuation_is_the_downloaded_solution_passed_explicitly(lam, tri):
    dtype_name, n, s = tri
    dt = s.vec_dtype
    B = np.random.default_rng(n).uniform(-1, 1, (8, n)).astype(dt)
    k1, k2 = min(3, n), 4
    for precond in (lam.PC_NONE, lam.PC_JACOBI):
        for nrhs in (1, 3, 8):
            what = f"{dtype_name} n={n} nrhs={nrhs} precond={precond}"
            s.set_rhs_many(B[:nrhs])
            s.solve_many(k1, 1e-30, precond)
            X1 = s.solutions()
            s.solve_many(k2, 1e-30, precond, x0=X1)
            want = _result(s)
            s.solve_many(k1, 1e-30, precond)
            res = s.true_residuals()
            _assert_bits(s.solutions(), X1, what + ": the solution after true_residuals")
            assert np.array_equal(_bits(s.true_residuals()), _bits(res))
            s.solve_many(k2, 1e-30, precond, x0="continue")
            _assert_same_run(_result(s), want, what)
            # and once more from there: a continuation of a continuation
            X2 = want[0]
            s.solve_many(k2, 1e-30, precond, x0="continue")
            got = _result(s)
            s.solve_many(k2, 1e-30, precond, x0=X2)
            _assert_same_run(got, _result(s), what + " (second continuation)")


def test_no_solution_to_continue_from_is_estate(lam):
    n = 64
    A = R.smoke_system(n)[0]
    B = np.ones((2, n))

    def refused(s, code, fn, *args, **kw):
        with pytest.raises(lam.LamHipError) as e:
            fn(*args, **kw)
        assert e.value.code == code, (fn, e.value)

    with lam.Solver(lam.F64) as s:
        s.set_matrix(A)
        s.set_rhs_many(B)
        refused(s, ESTATE, s.solve_many, 5, 1e-9, x0="continue")                  # before the first solve
        refused(s, ESTATE, s.true_residuals)
        s.solve_many(5, 1e-9)
        s.solve_many(5, 1e-9, x0="continue")
        bad = A[3:4].copy()
        bad[0, 3] = -1.0
        s.upload_rows(3, bad)
        refused(s, ESTATE, s.solve_many, 5, 1e-9, x0="continue")                  # a new matrix content
        s.solve_many(5, 1e-9)
        refused(s, EINVAL, s.solve_many, 5, 1e-9, lam.PC_JACOBI, x0="continue")   # the diagonal is refused ...
        refused(s, ESTATE, s.solve_many, 5, 1e-9, x0="continue")                  # ... and nothing is left to continue from
        refused(s, ESTATE, s.true_residuals)
        s.upload_rows(3, A[3:4])
        s.solve_many(5, 1e-9)
        s.gemv_many(B)
        refused(s, ESTATE, s.solve_many, 5, 1e-9, x0="continue")                  # after gemv_many
        s.solve_many(5, 1e-9)
        s.gemv_many_only(2, 1)
        refused(s, ESTATE, s.solve_many, 5, 1e-9, x0="continue")                  # after gemv_many_only
        s.solve_many(5, 1e-9)
        s.set_problem(n)
        s.upload_rows(0, A)
        refused(s, ESTATE, s.solve_many, 5, 1e-9, x0="continue")                  # after set_problem (no right-hand sides either)
        refused(s, ESTATE, s.solve_many, 5, 1e-9, x0=B)
        s.set_rhs_many(B)
        refused(s, ESTATE, s.solve_many, 5, 1e-9, x0="continue")
        s.solve_many(5, 1e-9, x0=B)
        s.solve_many(5, 1e-9, x0="continue")


# ------------------------------------------------------------------------------------------------
# 4, 9: the known first step from a non-zero integer guess, over dirty pad rows
# ------------------------------------------------------------------------------------------------
def _fma(alpha_tv, p, x, vdt):
    """fl(alpha p + x) with ONE rounding to vdt, elementwise (the x update contracts to an fma).  Exact rational arithmetic; for
    fp32 the exact value must fit fp64 so that the one rounding to fp32 is the only one."""
    a = Fraction(float(alpha_tv))
    out = np.empty(p.size, np.float64)
    for i in range(p.size):
        v = a * Fraction(float(p[i])) + Fraction(float(x[i]))
        out[i] = float(v)
        assert vdt is np.float64 or Fraction(out[i]) == v
    return out.astype(vdt)


@pytest.mark.parametrize("n", [257, 4097])
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_first_step_from_an_integer_guess_exact_over_dirty_pad_rows(lam, dtype_name, n):
    """Integer matrix with diagonal d_i in {1, 2, 4, 8}, integer c and x0 in [-8, 8], b = c + A x0 (|b_i| <= 64 n + 8: exact in
    fp32).  The device's A x0 and r0 = b - A x0 = c are exact, so the first step is exact_data's closed form on c:
    x1 = fl(alpha p0 + x0) with p0 = c (Jacobi: c / d), one rounding.  rel_err = sqrt(r1.r1 / b.b): exact_data.rel_err_bound's
    value for c, rescaled by sqrt(c.c / b.b).
    Before EVERY check a K = 8 batch runs with a NaN column and a 1e30 column (test_gpu_batch_recurrence.py, D): the guess is staged
    in P, whose rows behind row n then hold NaN in the layouts of K = 4, 2, 1.  A NaN column in x0 stays in its column."""
    assert n <= E.MAX_EXACT_N_FP32_JACOBI
    with lam.Solver(getattr(lam, dtype_name)) as s:
        vdt = s.vec_dtype
        d = E.pow2_diagonal(n, 29 * n)
        Cc = [E.int_vec(n, 31 * n + j) for j in range(4)]
        X0 = [E.int_vec(n, 37 * n + j) for j in range(4)]
        s.set_problem(n)
        prod = E.generate(n, [s.upload_rows], Cc + X0 + [c / d for c in Cc], diag=d)
        AC, AX0, AZ = prod[:4], prod[4:8], prod[8:]
        B = np.stack([c + ax for c, ax in zip(Cc, AX0)])
        assert np.abs(B).max() < 2 ** 24 and np.abs(np.stack(X0)).max() > 0
        X0 = np.stack(X0)
        dirty = np.stack([E.int_vec(n, 41 * n + j) for j in range(8)])
        dirty[3] = np.nan
        dirty[5] *= 1e30

        def soil():
            s.set_rhs_many(dirty)
            s.solve_many(20, 0.0)
            assert s.get_option("multi_rhs_k") == 8 and np.isnan(s.solutions()[3]).all()

        def want(j, precond):
            if precond == lam.PC_NONE:
                alpha, _, cc, _, r1 = E.first_cg_step(Cc[j], AC[j], vdt)
                p0, Ap = Cc[j], AC[j]
            else:
                alpha, _, cc, r1 = E.first_pcg_step(Cc[j], d, AZ[j], vdt)
                p0, Ap = Cc[j] / d, AZ[j]
            re_host, bound = E.rel_err_bound(Cc[j], Ap, alpha, r1, cc, U_TV[dtype_name])
            scale = np.sqrt(cc / float(np.dot(B[j], B[j])))
            return _fma(alpha, p0, X0[j], vdt), re_host * scale, bound * scale + 4 * np.spacing(re_host * scale)

        expected = {(j, pc): want(j, pc) for j in range(4) for pc in (lam.PC_NONE, lam.PC_JACOBI)}
        for step, nrhs in enumerate((4, 2, 1, 3, 2)):
            for precond in (lam.PC_NONE, lam.PC_JACOBI):
                what = f"{dtype_name} n={n} step {step} nrhs={nrhs} precond={precond} after a K = 8 batch with a NaN column"
                soil()
                s.set_rhs_many(B[:nrhs])
                s.solve_many(1, 1e-30, precond, x0=X0[:nrhs])
                X, it, cv, re = _result(s)
                assert s.get_option("multi_rhs_k") == K_FOR[nrhs] and (it == 2).all() and not cv.any(), (what, it)
                _assert_bits(X, np.stack([expected[j, precond][0] for j in range(nrhs)]), what)
                for j in range(nrhs):
                    assert abs(re[j] - expected[j, precond][1]) <= expected[j, precond][2], (what, j, re[j], expected[j, precond][1:])
                assert np.isfinite(s.true_residuals()).all()
                if nrhs >= 2:        # a NaN in column 1 of the guess stays there
                    G = X0[:nrhs].copy()
                    G[1, n // 2] = np.nan
                    s.solve_many(1, 1e-30, precond, x0=G)
                    Xn, itn, _, ren = _result(s)
                    keep = [j for j in range(nrhs) if j != 1]
                    assert np.isnan(Xn[1]).any() and np.isnan(ren[1]) and (itn == 2).all(), (what, itn, ren)
                    _assert_bits(Xn[keep], X[keep], what + ": next to a NaN column")
                    assert np.array_equal(_bits(ren[keep]), _bits(re[keep]))
                    res = s.true_residuals()
                    assert np.isnan(res[1]) and np.isfinite(res[keep]).all(), (what, res)


# ------------------------------------------------------------------------------------------------
# 7. tracking the restatement
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_rel_err_from_a_random_guess_tracks_the_restatement(lam, dtype_name):
    """The smoke system (n = 512), 8 right-hand sides, a random guess, plain and Jacobi: rel_err per column at k = 1, 2, 5, 20
    against warm_start_reference.pcg_x0 in the fixed order "rows".  Gate per k: 10 x the largest spread, over the columns, that the
    restatement shows against ITSELF between its three summation orders -- the rule of tests/tracking_data.py, computed here."""
    dt = NP[dtype_name]
    n, ks = 512, (1, 2, 5, 20)
    A, rng = R.smoke_system(n)
    A = A.astype(dt).astype(np.float64)
    B = rng.uniform(-1, 1, (8, n)).astype(dt)
    X0 = rng.uniform(-1, 1, (8, n)).astype(dt)
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.set_matrix(A)
        s.set_rhs_many(B)
        for precond in (lam.PC_NONE, lam.PC_JACOBI):
            dinv = None if precond == lam.PC_NONE else R.jacobi_dinv(A, dt)
            hist = {o: np.array([W.pcg_x0(A, B[j], X0[j], max(ks), 1e-30, dinv, dt, o)[1]["rel_err_history"] for j in range(8)])
                    for o in R.ORDERS}
            for k in ks:
                cols = np.stack([hist[o][:, k] for o in R.ORDERS])
                spread = max(np.abs(cols[a] / cols[b] - 1).max() for a in range(3) for b in range(3) if a != b)
                gate = 10 * spread
                s.solve_many(k, 1e-30, precond, x0=X0)
                assert (s.num_iters_many == k + 1).all()
                off = np.abs(s.rel_err_many / hist["rows"][:, k] - 1)
                print(f"{dtype_name} precond={precond} k={k}: rel_err off by {off.max():.3e}, reference spread {spread:.3e}, gate {gate:.3e}")
                assert (off < gate).all(), (dtype_name, precond, k, off.tolist(), gate)


# ------------------------------------------------------------------------------------------------
# 8. true residuals
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [257, 513])
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_true_residuals_against_numpy_within_the_product_bound(lam, dtype_name, n):
    """res_dev = ||fl(b - fl(A x))|| / ||b|| with the product accumulated in the vector dtype (unit roundoff u): per row
    |fl(A x) - A x| <= gamma_(n+2) (|A||x|), gamma_m = m u / (1 - m u), and the subtraction adds u (|b| + |A||x|) (1 + gamma), so
    | ||r_dev|| - ||r|| | <= ||r_dev - r||_2 <= gamma ||(|A||x|)||_2 + u (1 + gamma) || |b| + |A||x| ||_2; numpy's fp64 side obeys
    the same law with 2^-53; the fp64 sums, the division and the square root add (n + 8) 2^-53 relative on each side."""
    dt, u, u64 = NP[dtype_name], U_TV[dtype_name], 2.0 ** -53
    A, rng = R.smoke_system(n)
    A = A.astype(dt).astype(np.float64)
    B = rng.uniform(-1, 1, (8, n)).astype(dt)
    B[2] = 0.0
    live = [j for j in range(8) if j != 2]
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.set_matrix(A)
        for nrhs in (1, 3, 8):
            s.set_rhs_many(B[:nrhs])
            for precond, k in ((lam.PC_NONE, 3), (lam.PC_JACOBI, 25)):
                s.solve_many(k, 1e-30, precond)
                X = s.solutions().astype(np.float64)
                res = s.true_residuals()
                for j in range(nrhs):
                    if j == 2:
                        assert np.isnan(res[j]), res                              # 0/0
                        continue
                    b = B[j].astype(np.float64)
                    absAx = np.abs(A) @ np.abs(X[j])
                    nb = np.linalg.norm(b)
                    ref = np.linalg.norm(b - A @ X[j]) / nb

                    def gamma(m, v):
                        return m * v / (1 - m * v)
                    bound = sum(gamma(n + 2, v) * np.linalg.norm(absAx) + v * (1 + gamma(n + 2, v)) * np.linalg.norm(np.abs(b) + absAx)
                                for v in (u, u64)) / nb + 2 * (n + 8) * u64 * ref
                    print(f"{dtype_name} n={n} nrhs={nrhs} precond={precond} column {j}: device {res[j]:.6e}, numpy {ref:.6e}, "
                          f"difference {abs(res[j] - ref):.3e}, bound {bound:.3e}, recursive {s.rel_err_many[j]:.6e}")
                    assert abs(res[j] - ref) <= bound, (dtype_name, n, nrhs, precond, j, res[j], ref, bound)
            if nrhs == 8:
                with pytest.raises(lam.LamHipError) as e:
                    s.true_residuals(9)
                assert e.value.code == EINVAL
            else:
                with pytest.raises(lam.LamHipError) as e:
                    s.true_residuals(nrhs + 1)                                    # more than were solved
                assert e.value.code == EINVAL and "were solved" in str(e.value)
        assert live


# ------------------------------------------------------------------------------------------------
# 10. refusals
# ------------------------------------------------------------------------------------------------
def test_refusals(lam, monkeypatch):
    n = 64
    A = np.eye(n)
    B = np.ones((2, n))

    def refused(s, code, fn, *args, **kw):
        launches = s.get_option("hip_calls_launch")
        with pytest.raises(lam.LamHipError) as e:
            fn(*args, **kw)
        assert e.value.code == code, (fn, e.value)
        assert s.get_option("hip_calls_launch") == launches
        return str(e.value)

    def both(s, code, word):
        s.nrhs = 2
        for precond in (lam.PC_NONE, lam.PC_JACOBI):
            assert word in refused(s, code, s.solve_many, 5, 1e-9, precond, x0=B)
            assert word in refused(s, code, s.solve_many, 5, 1e-9, precond, x0="continue")
        assert word in refused(s, code, s.true_residuals)

    with lam.Solver(lam.F64, device_ids=[0, 0]) as s:
        s.set_matrix(A)
        both(s, EINVAL, "shard")
    with lam.Solver(lam.BF16) as s:
        s.set_matrix(A)
        both(s, EINVAL, "BF16")
    monkeypatch.setenv("LAM_HIP_FORCE_RCCL", "1")      # a one-rank communicator: the rank mode on one GPU
    with lam.Solver(lam.F64, rank=0, nranks=1, device_id=0, unique_id=None) as s:
        monkeypatch.delenv("LAM_HIP_FORCE_RCCL")
        s.set_problem(n)
        s.upload_rows(0, A)
        both(s, EINVAL, "rank mode")
    with lam.Solver(lam.F64) as s:
        s.n, s.nrhs = n, 2
        refused(s, ESTATE, s.solve_many, 5, 1e-9, x0=B)
        s.set_problem(n)
        s.upload_rows(0, A)
        refused(s, ESTATE, s.solve_many, 5, 1e-9, x0=B)                            # no right-hand sides yet
        s.set_rhs_many(B)
        for precond in (2, -1, 7):
            assert "preconditioner" in refused(s, EINVAL, s.solve_many, 5, 1e-9, precond, x0=B)
        refused(s, EINVAL, s.solve_many, -1, 1e-9, x0=B)
        assert s._L.lam_hip_solve_many_x0(None, 0, None, 5, 1e-9, None, None, None, None) == EINVAL
        assert s._L.lam_hip_true_residual_many(None, 1, None) == EINVAL and s._L.lam_hip_true_residual_many(s._h, 1, None) == EINVAL
        # and the path works on this context afterwards, every output optional; A = I: the exact guess is b itself
        assert s._L.lam_hip_solve_many_x0(s._h, lam.PC_JACOBI, B.ctypes.data, 5, 1e-9, None, None, None, None) == 0
        assert s.solve_many(5, 1e-9, x0=B).all() and (s.num_iters_many == 0).all() and np.array_equal(s.solutions(), B)
        refused(s, EINVAL, s.true_residuals, 3)                                    # more than were solved
        refused(s, EINVAL, s.true_residuals, 0)
        assert (s.true_residuals() == 0.0).all()


# ------------------------------------------------------------------------------------------------
# 11. past the grid-stride wrap
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_past_the_grid_stride_wrap(lam, dtype_name):
    """n = 65537 > 256 workgroups x 256 threads: a thread of the init pass and of the residual pass handles a second element.
    tridiag(1,2,1) filled on the device: the zero-guess identity, and the exact integer guess born stopped."""
    n = 65537
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.generate_matrix(n)
        dt = s.vec_dtype
        rng = np.random.default_rng(n)
        B = rng.uniform(-1, 1, (8, n)).astype(dt)
        XS = np.stack([E.int_vec(n, 43 * n + j) for j in range(8)]).astype(dt)
        BX = E.tridiag_product(XS).astype(dt)
        for nrhs in (3, 8):
            for precond in (lam.PC_NONE, lam.PC_JACOBI):
                what = f"{dtype_name} n={n} nrhs={nrhs} precond={precond}"
                s.set_rhs_many(B[:nrhs])
                s.solve_many(12, 0.0, precond)
                want = _result(s)
                s.solve_many(12, 0.0, precond, x0=np.zeros((nrhs, n), dt))
                _assert_same_run(_result(s), want, what)
                G = XS[:nrhs].copy()
                G[1, n - 1] += 1                                                   # column 1 is off in the LAST element only
                s.set_rhs_many(BX[:nrhs])
                s.solve_many(3, 1e-30, precond, x0=G)
                X, it, cv, re = _result(s)
                keep = [j for j in range(nrhs) if j != 1]
                assert (it[keep] == 0).all() and cv[keep].all() and (re[keep] == 0.0).all() and it[1] == 4 and re[1] > 0, (what, it, re)
                _assert_bits(X[keep], XS[keep], what)
                res = s.true_residuals()
                assert (res[keep] == 0.0).all() and res[1] > 0, (what, res)


# ------------------------------------------------------------------------------------------------
# 12. driver
# ------------------------------------------------------------------------------------------------
def test_driver_two_stages_and_true_residuals():
    """tridiag(1,2,1), n = 1024, b_j = 2^j: x_i = 2^j i (n + 1 - i) / 2 in closed form, which gives case 8's bound without the
    solution.  -w 0 is a zero-iteration stage and a continuation from x = 0: the plain run's digits."""
    exe = os.path.join(ROOT, PKG_NAME, "test", "test_CG_multi_rhs.out")
    n, tol = 1024, 1e-9

    def run(extra):
        r = subprocess.run([exe, "-s", str(n), "-k", "3", "-i", "3000", "-e", str(tol)] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = [ln.split(",") for ln in r.stdout.strip().splitlines()]
        assert len(lines) == 3 and all(ln[0] == str(n) for ln in lines), r.stdout
        return lines

    plain = run([])
    assert all(len(ln) == 10 for ln in plain)
    for w in ("-1", "3001"):                                                       # a usage error, not "no flag"
        r = subprocess.run([exe, "-s", str(n), "-k", "3", "-i", "3000", "-w", w], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "Usage" in r.stderr and not r.stdout, (w, r.returncode, r.stdout, r.stderr)
    for extra in (["-J"], ["-w", "0"]):
        assert [ln[7:9] for ln in run(extra)] == [ln[7:9] for ln in plain], extra
    i = np.arange(1, n + 1, dtype=np.float64)
    x = i * (n + 1 - i) / 2                                                        # for b = 1; every column scales both norms alike
    absAx = E.tridiag_product(x)
    u = 2.0 ** -53
    gamma = (n + 2) * u / (1 - (n + 2) * u)
    bound = (gamma * np.linalg.norm(absAx) + u * (1 + gamma) * np.linalg.norm(1.0 + absAx)) / np.sqrt(n)
    for extra in (["-w", "100", "-T"], ["-w", "100", "-T", "-J"], ["-T"]):
        lines = run(extra)
        assert all(len(ln) == 11 for ln in lines), lines
        for ln in lines:
            iters, rel, true = int(ln[7]), float(ln[8]), float(ln[10])
            print(f"{extra}: {iters} iterations, recursive {rel:.3e}, true {true:.3e}, bound on their difference {bound:.3e}")
            assert 100 < iters <= 3000 and rel < tol and abs(true - rel) <= bound, (extra, ln, bound)
        if "-w" not in extra:
            assert [ln[7:9] for ln in lines] == [ln[7:9] for ln in plain]
