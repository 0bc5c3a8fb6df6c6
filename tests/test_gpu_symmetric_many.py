"""Option "symmetric_many": the batched product of K = 1, 2, 4 interleaved columns reads every pair {A_ij, A_ji} once
(csrc/lam_kernels.h "Symmetric batched product", csrc/lam_multi.h multi_sym_launch).

What is pinned, without a tolerance wherever the product itself is compared:
  1  the exact product of the integer matrix (tests/exact_data.py: every sum exact in any order) for nrhs = 1 ... 4, K = 8 untouched;
  2  only the upper triangle is read: NaN everywhere below the diagonal changes nothing;
  3  column j is bit for bit lam_hip_gemv under "symmetric" = 2 on that vector, at K = 1, 2 and 4, tall tasks included;
  4  the fused p.Ap partials and the shift epilogue: the exact first CG step;
  5  columns never mix;
  6  every caller of the batch's product converges under the option, judged by the general product;
  7  launch counts: one more launch per product;
  8  lifecycle of the option and of the batch's own plan and partials on one context.
Sizes: a strip of the symmetric plan is SS = 256 * VEC columns (512 fp64, 1024 fp32), VEC = elements per 16-byte vector."""
import contextlib

import numpy as np
import pytest

import exact_data as E
import minres_data as MD
import mshift_reference as MS
import pcg_reference as R

pytestmark = pytest.mark.gpu

DTYPES = ("F64", "F32")
NP = {"F64": np.float64, "F32": np.float32}
VEC = {"F64": 2, "F32": 4}
SS = {"F64": 512, "F32": 1024}
K_FOR = {1: 1, 2: 2, 3: 4, 4: 4, 8: 8}
EINVAL = -1


def _three_strips(d):
    """Two full strips plus a ragged one of one vector and one more column."""
    return 2 * SS[d] + VEC[d] + 1


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _assert_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = np.argwhere(_bits(got) != _bits(want))
    assert bad.size == 0, f"{what}: {len(bad)} entries differ, first {bad[:4].tolist()}: {got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}"


def _row_class(y):
    return np.where(np.isnan(y), 3, np.where(np.isposinf(y), 1, np.where(np.isneginf(y), 2, 0)))


@contextlib.contextmanager
def _integer_context(lam, dtype_name, n, vecs, nan_below_diagonal=False):
    """A context holding exact_data's integer matrix, and [A v for v in vecs] exactly."""
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.set_problem(n)
        if nan_below_diagonal:
            A = np.empty((n, n))
            refs = E.generate(n, [lambda r0, blk: A.__setitem__(slice(r0, r0 + blk.shape[0]), blk)], vecs)
            A[np.tril_indices(n, -1)] = np.nan
            s.set_matrix(A)
        else:
            refs = E.generate(n, [s.upload_rows], vecs)
        yield s, refs


def _single_symmetric(s, X):
    """lam_hip_gemv under "symmetric" = 2, row by row of X; the option is put back."""
    s.set_option("symmetric", 2)
    Y = np.stack([s.gemv(x) for x in X])
    assert s.get_option("symmetric_effective") == 1
    s.set_option("symmetric", 0)
    return Y


# ------------------------------------------------------------------------------------------------
# 1. exact product
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name,n", [(d, n) for d in DTYPES for n in (1001, _three_strips(d), 6150)])
def test_exact_product_for_one_to_four_columns_and_k8_is_untouched(lam, dtype_name, n):
    dt = NP[dtype_name]
    X = np.stack([E.int_vec(n, 100 + j) for j in range(8)])
    with _integer_context(lam, dtype_name, n, list(X)) as (s, refs):
        want = np.stack(refs).astype(dt)
        assert s.get_option("symmetric_many") == 0 and s.get_option("symmetric_many_effective") == 0
        general8 = s.gemv_many(X.astype(dt))
        assert s.get_option("symmetric_many_effective") == 0
        s.set_option("symmetric_many", 2)
        assert s.get_option("symmetric_many") == 2
        for nrhs in (1, 2, 3, 4):
            Y = s.gemv_many(X[:nrhs].astype(dt))
            what = f"{dtype_name} n={n} nrhs={nrhs}"
            assert s.get_option("symmetric_many_effective") == 1 and s.get_option("multi_rhs_k") == K_FOR[nrhs], what
            assert np.array_equal(Y, want[:nrhs]), (what, np.argwhere(Y != want[:nrhs])[:6].tolist())
        Y = s.gemv_many(X.astype(dt))
        assert s.get_option("symmetric_many_effective") == 0 and s.get_option("multi_rhs_k") == 8
        assert np.array_equal(Y, want)
        _assert_bits(Y, general8, f"{dtype_name} n={n}: K = 8 under the option against option 0")


# ------------------------------------------------------------------------------------------------
# 2. only the upper triangle is used
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_only_the_upper_triangle_is_read(lam, dtype_name):
    """NaN in every element strictly below the diagonal: the task kernel skips what it does not use by select, so the exact answer of
    the symmetric matrix comes out, in the batch as in the single symmetric product."""
    n, dt = _three_strips(dtype_name), NP[dtype_name]
    X = np.stack([E.int_vec(n, 200 + j) for j in range(4)])
    with _integer_context(lam, dtype_name, n, list(X), nan_below_diagonal=True) as (s, refs):
        want = np.stack(refs).astype(dt)
        s.set_option("symmetric_many", 2)
        Y = s.gemv_many(X.astype(dt))
        assert s.get_option("symmetric_many_effective") == 1
        single = _single_symmetric(s, X.astype(dt))
        _assert_bits(Y, single, f"{dtype_name} n={n}: against lam_hip_gemv under symmetric = 2")
        assert np.array_equal(Y, want), np.argwhere(Y != want)[:6].tolist()


# ------------------------------------------------------------------------------------------------
# 3. bit for bit against the single symmetric path, and across K
# ------------------------------------------------------------------------------------------------
def _bitwise_against_single_and_across_k(s, X, what):
    single = _single_symmetric(s, X)
    s.set_option("symmetric_many", 2)
    Y4 = s.gemv_many(X)
    assert s.get_option("symmetric_many_effective") == 1 and s.get_option("multi_rhs_k") == 4
    _assert_bits(Y4, single, what + ": K = 4 against the single symmetric product")
    for j in range(4):
        Y1 = s.gemv_many(X[j:j + 1])
        assert s.get_option("symmetric_many_effective") == 1 and s.get_option("multi_rhs_k") == 1
        _assert_bits(Y1[0], single[j], what + f": column {j} alone at K = 1")
    for pair in ((0, 1), (3, 2)):
        Y2 = s.gemv_many(X[list(pair)])
        assert s.get_option("symmetric_many_effective") == 1 and s.get_option("multi_rhs_k") == 2
        _assert_bits(Y2, single[list(pair)], what + f": columns {pair} at K = 2")


@pytest.mark.parametrize("dtype_name,n", [(d, n) for d in DTYPES for n in (1001, 4097 + VEC[d])])
def test_bit_for_bit_against_the_single_symmetric_product_and_across_k(lam, dtype_name, n):
    dt = NP[dtype_name]
    rng = np.random.default_rng(n)
    Rm = rng.uniform(-1, 1, (n, n))
    A = 0.5 * (Rm + Rm.T)
    del Rm
    X = rng.uniform(-1, 1, (4, n)).astype(dt)
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.set_matrix(A)
        _bitwise_against_single_and_across_k(s, X, f"{dtype_name} n={n}")


@pytest.mark.parametrize("dtype_name,n", [("F64", 32768), ("F32", 40000)])
def test_bit_for_bit_at_tall_tasks(lam, dtype_name, n):
    """The smallest sizes at which the plan gives tasks of 512 rows (2 * 256 * 3000 <= n * nstrips): the 256-row LDS buffer of row
    partials is flushed twice per task.  The generated SPD matrix is symmetric bit for bit; integer columns."""
    dt = NP[dtype_name]
    X = np.stack([E.int_vec(n, 300 + j) for j in range(4)]).astype(dt)
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.generate_random_spd(n, 5, 100.0)
        _bitwise_against_single_and_across_k(s, X, f"{dtype_name} n={n}")


# ------------------------------------------------------------------------------------------------
# 4. fused p.Ap and the shift epilogue, exact
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shifts", [None, (0.0, 1.0, 2.0, 4.0)], ids=["unshifted", "shifted"])
@pytest.mark.parametrize("dtype_name,n", [(d, n) for d in DTYPES for n in (1001, _three_strips(d))])
def test_first_cg_step_is_exact_under_the_option(lam, dtype_name, n, shifts):
    """solve_many(1, 1e-30) from x = 0 on the integer system: x_1 = fl(alpha_TV b) bit for bit with alpha = fl64(b.b / b.(A + s I) b),
    which pins every workgroup's p.Ap partial of the second pass and the epilogue's shift; rel_err within exact_data.rel_err_bound.
    (A + s_j I) b_j = A b_j + s_j b_j stays an exact integer vector."""
    dt = NP[dtype_name]
    u = {"F64": 2.0 ** -53, "F32": 2.0 ** -24}[dtype_name]
    B = np.stack([E.int_vec(n, 400 + j) for j in range(4)])
    with _integer_context(lam, dtype_name, n, list(B)) as (s, AB):
        s.set_option("symmetric_many", 2)
        s.set_rhs_many(B.astype(dt))
        if shifts is not None:
            s.set_shifts(shifts)
        conv = s.solve_many(1, 1e-30)
        assert s.get_option("symmetric_many_effective") == 1 and s.get_option("multi_rhs_k") == 4
        X = s.solutions()
        assert not conv.any() and (s.num_iters_many == 2).all(), s.num_iters_many
        for j in range(4):
            Ab = AB[j] + (shifts[j] if shifts is not None else 0.0) * B[j]
            alpha, x1, bb, pAp, r1 = E.first_cg_step(B[j], Ab, dt)
            x1 = x1 + dt(0)
            _assert_bits(X[j], x1, f"{dtype_name} n={n} column {j}: x1 (alpha {alpha!r}, b.b {bb}, p.Ap {pAp})")
            re_host, bound = E.rel_err_bound(B[j], Ab, alpha, r1, bb, u)
            assert abs(s.rel_err_many[j] - re_host) <= bound, (j, s.rel_err_many[j], re_host, bound)


# ------------------------------------------------------------------------------------------------
# 5. columns never mix
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_a_poisoned_column_stays_in_its_column(lam, dtype_name):
    n, dt = _three_strips(dtype_name), NP[dtype_name]
    X = np.stack([E.int_vec(n, 500 + j) for j in range(4)]).astype(dt)
    Xp = X.copy()
    Xp[2, n // 3] = np.nan
    Xp[2, n - 2] = np.inf
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.set_problem(n)
        A = np.empty((n, n))
        E.generate(n, [lambda r0, blk: A.__setitem__(slice(r0, r0 + blk.shape[0]), blk), s.upload_rows], [])
        s.set_option("symmetric_many", 2)
        clean = s.gemv_many(X)
        Y = s.gemv_many(Xp)
        assert s.get_option("symmetric_many_effective") == 1
        for j in (0, 1, 3):
            _assert_bits(Y[j], clean[j], f"{dtype_name}: column {j} next to the poisoned one")
        with np.errstate(invalid="ignore"):
            want = (A * Xp[2].astype(np.float64)).sum(axis=1)
        got, cls = _row_class(Y[2].astype(np.float64)), _row_class(want)
        assert np.array_equal(got, cls), np.flatnonzero(got != cls)[:8]


# ------------------------------------------------------------------------------------------------
# 6. every caller
# ------------------------------------------------------------------------------------------------
CG_TOL = {"F64": 1e-9, "F32": 1e-5}             # tests/test_gpu_multi_rhs.py, test_gpu_warm_start.py, test_gpu_shifted.py
PCG_TOL = {"F64": 1e-10, "F32": 1e-5}           # tests/test_gpu_pcg.py, tests/test_gpu_mshift.py


@pytest.fixture(scope="module", params=DTYPES)
def spd(request, lam):
    """One SPD system per dtype: pcg_reference.smoke_system (the matrix family of the batched tests), in the storage type's values."""
    d = request.param
    n, dt = _three_strips(d), NP[d]
    A, rng = R.smoke_system(n, seed=n)
    A = A.astype(dt).astype(np.float64)
    B = rng.uniform(-1, 1, (4, n)).astype(dt)
    with lam.Solver(getattr(lam, d)) as s:
        s.set_matrix(A)
        yield s, d, n, A, B


def _judged_by_the_general_product(s):
    """True residuals of the batch's solution, measured with the option back at 0; the option is restored."""
    s.set_option("symmetric_many", 0)
    res = s.true_residuals()
    assert s.get_option("symmetric_many_effective") == 0
    s.set_option("symmetric_many", 2)
    return res


def test_cg_jacobi_and_warm_start_converge_under_the_option(lam, spd):
    s, d, n, A, B = spd
    s.set_option("symmetric_many", 2)
    s.set_rhs_many(B)
    for what, tol, call in (("plain", CG_TOL[d], lambda t: s.solve_many(4 * n, t)),
                            ("jacobi", PCG_TOL[d], lambda t: s.solve_many(4 * n, t, lam.PC_JACOBI)),
                            ("from a guess", CG_TOL[d], lambda t: s.solve_many(4 * n, t, lam.PC_NONE, 0.5 * B)),
                            ("continued", CG_TOL[d], lambda t: (s.solve_many(3, t), s.solve_many(4 * n, t, lam.PC_NONE, "continue"))[1])):
        conv = call(tol)
        assert s.get_option("symmetric_many_effective") == 1, what
        res = _judged_by_the_general_product(s)
        print(f"{d} n={n} {what}: iterations {s.num_iters_many.tolist()}, true residuals {res.tolist()}")
        assert conv.all() and (s.rel_err_many < tol).all(), (what, s.num_iters_many, s.rel_err_many)
        assert (res <= 2 * tol + 1e-13).all(), (what, res, tol)
        X = s.solutions()
        for j in range(4):
            assert R.true_residual(A, X[j], B[j]) <= 2 * tol + 1e-13, (what, j)
    s.set_option("symmetric_many", 0)


def test_the_shifted_batch_converges_under_the_option(lam, spd):
    s, d, n, A, B = spd
    tol, sh = CG_TOL[d], np.array([0.0, 0.5, 2.0, 8.0])
    s.set_option("symmetric_many", 2)
    for precond in (lam.PC_NONE, lam.PC_JACOBI):
        s.set_rhs_many(B)
        s.set_shifts(sh)
        conv = s.solve_many(4 * n, tol, precond)
        assert s.get_option("symmetric_many_effective") == 1
        res = _judged_by_the_general_product(s)
        print(f"{d} n={n} shifted precond={precond}: iterations {s.num_iters_many.tolist()}, true residuals {res.tolist()}")
        assert conv.all() and (res <= 2 * tol + 1e-13).all(), (s.num_iters_many, res)
        X = s.solutions()
        for j in range(4):
            assert R.true_residual(A + sh[j] * np.eye(n), X[j], B[j]) <= 2 * tol + 1e-13, j
    s.set_option("symmetric_many", 0)


def test_minres_converges_under_a_negative_shift_under_the_option(lam, spd):
    s, d, n, A, B = spd
    tol = MD.INDEFINITE_TOL[NP[d]]
    shift, _ = MD.central_gap_shift(A)
    assert shift < 0
    s.set_option("symmetric_many", 2)
    s.set_rhs_many(B)
    conv = s.solve_minres(4 * n, tol, [shift] * 4)
    assert s.get_option("symmetric_many_effective") == 1
    res = _judged_by_the_general_product(s)
    print(f"{d} n={n} MINRES shift {shift}: iterations {s.num_iters_many.tolist()}, true residuals {res.tolist()}")
    assert conv.all() and (s.rel_err_many < tol).all() and (res <= 2 * tol).all(), (s.num_iters_many, s.rel_err_many, res)
    s.set_rhs_many(B)                   # clears the negative shift for the tests that follow
    s.set_option("symmetric_many", 0)


def test_multishift_converges_under_the_option_and_its_true_residuals_stay_general(lam, spd):
    """The seed is the K = 1 batch: symmetric under the option.  Gate of tests/test_gpu_mshift.py: per shift the host's true residual
    <= 2 max(the shifted batch's, rel_error), the shifted batch run with the option at 0."""
    s, d, n, A, B = spd
    tol, sh, b = PCG_TOL[d], MS.converged_shifts(9), B[0]
    s.set_option("symmetric_many", 2)
    conv = s.solve_multishift(b, sh, 4000, tol)
    assert s.get_option("symmetric_many_effective") == 1
    X = s.multishift_solutions()
    res = s.multishift_true_residuals()
    assert s.get_option("symmetric_many_effective") == 0            # the K = 8 product
    assert conv.all() and (s.rel_err_shift < tol).all(), (s.num_iters_shift, s.rel_err_shift)
    s.set_option("symmetric_many", 0)
    Xb = np.empty_like(X)
    for first in range(0, 9, 8):
        assert s.solve_shifted(b, sh[first:first + 8], 4000, tol).all()
        Xb[first:first + 8] = s.solutions()
    b64 = b.astype(np.float64)
    host = lambda Xs: np.array([np.linalg.norm(b64 - (A @ x + sj * x)) / np.linalg.norm(b64) for sj, x in zip(sh, Xs.astype(np.float64))])
    t_ms, t_b = host(X), host(Xb)
    print(f"{d} n={n} multi-shift: true {t_ms.tolist()}, shifted batch {t_b.tolist()}, device {res.tolist()}")
    assert (t_ms <= 2 * np.maximum(t_b, tol)).all(), (t_ms, t_b)
    assert (res <= 2 * np.maximum(t_b, tol) + 1e-13).all(), (res, t_b)


# ------------------------------------------------------------------------------------------------
# 7. launch counts (as tests/test_gpu_batch_launch_counts.py counts them)
# ------------------------------------------------------------------------------------------------
COUNT_N, ITERS = 130, 11
NINE_SHIFTS = (0.0, 0.25, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 8.0)


def _launches(s, call):
    l0 = s.get_option("hip_calls_launch")
    call()
    return s.get_option("hip_calls_launch") - l0


@pytest.mark.parametrize("nrhs", [1, 3])
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_one_more_launch_per_product(lam, dtype_name, nrhs):
    """rel_error = 0 on a random SPD system of condition 1e4: exactly 11 iterations are enqueued.  Option 0: 3 launches per iteration
    (4 multi-shift), 1 per product; option 2: one more per product."""
    dt = NP[dtype_name]
    rng = np.random.default_rng(11)
    B, X0 = rng.uniform(-1, 1, (nrhs, COUNT_N)).astype(dt), rng.uniform(-1, 1, (nrhs, COUNT_N)).astype(dt)
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.generate_random_spd(COUNT_N, 5, 1e4)
        s.set_rhs_many(B)
        for value, extra in ((0, 0), (2, 1), (0, 0)):
            s.set_option("symmetric_many", value)
            what = f"{dtype_name} nrhs={nrhs} symmetric_many={value}"
            assert _launches(s, lambda: s.solve_many(ITERS, 0.0)) == (3 + extra) * ITERS, what
            assert (s.num_iters_many == ITERS + 1).all(), what
            assert s.get_option("symmetric_many_effective") == extra
            assert _launches(s, lambda: s.solve_many(ITERS, 0.0, lam.PC_JACOBI)) == (3 + extra) * ITERS, what
            assert _launches(s, lambda: s.solve_many(ITERS, 0.0, lam.PC_NONE, X0)) == (3 + extra) * ITERS + 1 + extra, what
            assert _launches(s, s.true_residuals) == 1 + extra, what
            assert _launches(s, lambda: s.gemv_many(X0)) == 1 + extra, what
            assert _launches(s, lambda: s.solve_minres(ITERS, 0.0)) == (3 + extra) * ITERS, what
            assert (s.num_iters_many == ITERS + 1).all(), what
            assert _launches(s, lambda: s.solve_multishift(B[0], NINE_SHIFTS, ITERS, 0.0)) == (4 + extra) * ITERS, what
            assert (s.num_iters_shift == ITERS + 1).all(), what
            assert _launches(s, s.multishift_true_residuals) == 2, what           # two groups of 8: K = 8, always general
            s.set_rhs_many(B)


# ------------------------------------------------------------------------------------------------
# 8. lifecycle on one context
# ------------------------------------------------------------------------------------------------
def _solve(s, B, iters=6):
    s.set_rhs_many(B)
    s.solve_many(iters, 1e-30)
    return s.solutions(), s.num_iters_many.copy(), s.rel_err_many.copy()


def _assert_same_solve(got, want, what):
    _assert_bits(got[0], want[0], what + ": x")
    assert np.array_equal(got[1], want[1]) and np.array_equal(_bits(got[2]), _bits(want[2])), what


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_lifecycle_of_the_option_and_the_partials(lam, dtype_name):
    n, dt = _three_strips(dtype_name), NP[dtype_name]
    n2 = 1001
    A, rng = R.smoke_system(n, seed=3)
    A2, _ = R.smoke_system(n2, seed=4)
    B = rng.uniform(-1, 1, (4, n)).astype(dt)
    B2 = rng.uniform(-1, 1, (4, n2)).astype(dt)
    b = B[0]
    with lam.Solver(getattr(lam, dtype_name)) as f:                 # fresh contexts: what each solve gives alone
        f.set_matrix(A)
        general = {k: _solve(f, B[:k]) for k in (1, 2, 4)}
        f.set_rhs(b)
        f.set_option("symmetric", 2)
        f.solve(6, 1e-30)
        single_alone = f.solution()
    with lam.Solver(getattr(lam, dtype_name)) as f:
        f.set_matrix(A)
        f.set_option("symmetric_many", 2)
        sym = {k: _solve(f, B[:k]) for k in (1, 2, 4)}
    with lam.Solver(getattr(lam, dtype_name)) as f:
        f.set_matrix(A2)
        f.set_option("symmetric_many", 2)
        sym_small = _solve(f, B2)

    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.set_matrix(A)
        s.set_option("symmetric_many", 2)
        for k in (4, 1, 2):                                         # the partials grow once and are re-used
            _assert_same_solve(_solve(s, B[:k]), sym[k], f"{dtype_name} K {k} in the order 4, 1, 2")
            assert s.get_option("symmetric_many_effective") == 1 and s.get_option("multi_rhs_k") == k
        s.set_option("symmetric_many", 0)                           # toggled between two solves
        _assert_same_solve(_solve(s, B), general[4], "option 0 after option 2 against a fresh context")
        assert s.get_option("symmetric_many_effective") == 0
        s.set_option("symmetric_many", 2)
        _assert_same_solve(_solve(s, B), sym[4], "option 2 again")
        # a single solve under "symmetric" = 2 interleaved with the batch under "symmetric_many" = 2
        s.set_option("symmetric", 2)
        s.set_rhs(b)
        s.solve(6, 1e-30)
        _assert_bits(s.solution(), single_alone, "the single symmetric solve next to the batch")
        _assert_same_solve(_solve(s, B[:2]), sym[2], "the batch next to the single symmetric solve")
        s.set_rhs(b)
        s.solve(6, 1e-30)
        _assert_bits(s.solution(), single_alone, "the single symmetric solve after the batch")
        s.set_option("symmetric", 0)
        # value 1 at this small N: below the threshold
        s.set_option("symmetric_many", 1)
        assert s.get_option("symmetric_many") == 1
        _assert_same_solve(_solve(s, B), general[4], "value 1 below the threshold")
        assert s.get_option("symmetric_many_effective") == 0
        # refused values leave the value in force
        for bad in (3, -1):
            with pytest.raises(lam.LamHipError) as e:
                s.set_option("symmetric_many", bad)
            assert e.value.code == EINVAL and s.get_option("symmetric_many") == 1
        # another N and back
        s.set_option("symmetric_many", 2)
        s.set_matrix(A2)
        _assert_same_solve(_solve(s, B2), sym_small, "another N")
        s.set_matrix(A)
        _assert_same_solve(_solve(s, B), sym[4], "back at the first N")
        assert s.get_option("symmetric_many_effective") == 1


@pytest.mark.parametrize("dtype_name,n", [("F64", 5017), ("F32", 7095)])
def test_value_1_takes_effect_from_192_mib_of_matrix_on(lam, dtype_name, n):
    """The threshold of option "symmetric": n^2 esz >= 192 MiB first holds at N = 5017 (fp64) / 7095 (fp32); one row less stays on
    the general product.  Every measured (dtype, K <= 4) is admitted (profiles/symv_many_probe.txt); K = 8 never is."""
    dt = NP[dtype_name]
    X = np.stack([E.int_vec(n, 600 + j) for j in range(8)]).astype(dt)
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.generate_random_spd(n, 5, 100.0)
        s.set_option("symmetric_many", 2)
        always = {k: s.gemv_many(X[:k]) for k in (1, 2, 4)}
        s.set_option("symmetric_many", 1)
        for k in (1, 2, 4):
            _assert_bits(s.gemv_many(X[:k]), always[k], f"{dtype_name} n={n} K={k}: value 1 against value 2")
            assert s.get_option("symmetric_many_effective") == 1
        s.gemv_many(X)
        assert s.get_option("symmetric_many_effective") == 0 and s.get_option("multi_rhs_k") == 8
        s.generate_random_spd(n - 1, 5, 100.0)
        s.gemv_many(X[:4, :n - 1])
        assert s.get_option("symmetric_many_effective") == 0 and s.get_option("multi_rhs_k") == 4
