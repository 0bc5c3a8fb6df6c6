"""Batched MINRES, (A + s_j I) x_j = b_j for shifts of either sign: lam_hip_solve_many_minres (include/lam_hip.h), i.e.
minres_init / init_scalars / start / lanczos / update_kernel (csrc/lam_kernels.h) around the batch's product.

Sizes: the fp64 K = 8 p tile is 512 columns, the K = 4 tile 1024, the K = 1 tile 4096, and the vector kernels wrap at N = 65537; so N
in {1, 7, 513, 1030, 4097} and 65537 on the device-filled tridiag(1,2,1).

 1. exact answers on a diagonal matrix of powers of two: the sign of a negative pivot, the beta' = 0 stop;
 2. every column iteration by iteration against tests/minres_reference.py within tests/minres_data.py's measured gates;
 3. a column of a batch is the column alone at K = 1 under its own shift, bit for bit, past the wrap too;
 4. frozen columns; a zero and a NaN right-hand side stay in their column;
 5. an indefinite system converges, its true residuals, and CG's refusal under the negative shift;
 6. agreement with CG on SPD systems;
 7. refusals and lifetime; 8. the driver's -m."""
import os
import subprocess

import numpy as np
import pytest

import minres_data as D
import minres_reference as M
import pcg_reference as R
from conftest import ROOT, PKG_NAME
from tracking_data import tracking_columns

pytestmark = pytest.mark.gpu

DTYPES = ("F64", "F32")
NP = {"F64": np.float64, "F32": np.float32}
K_FOR = {1: 1, 2: 2, 3: 4, 4: 4, 5: 8, 6: 8, 7: 8, 8: 8}
EINVAL, ESTATE = -1, -6
# eight different nonzero shifts of both signs, each exact in fp32 (a zero shift alone runs the unshifted product, in a batch
# fma(0, v, u): the same value, but the sign of a zero may differ -- section 7 covers zero shifts)
MIXED_SHIFTS = (0.5, -0.5, -1.125, 2.0, -3.0, -0.125, 4.0, -6.0)


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


def _column(run, j):
    return tuple(a[j:j + 1].copy() for a in run)


# ------------------------------------------------------------------------------------------------
# 1. exact answers
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 513, 1030, 4097])
def test_unit_vectors_on_a_diagonal_of_powers_of_two_are_solved_exactly_in_one_step(lam, n):
    """A = diag(2^e_i), b_j = 2^m_j e_(i_j), s_j = +-2^q_j - a_ii: every operation of the first iteration is exact, beta' = 0, the
    column stops at k = 1 with rel_err == 0 and x_j = b_j / (a_ii + s_j) bit for bit -- negative for the negative pivots."""
    i = np.arange(n)
    e = (i * 7) % 5 - 2
    A = np.diag(2.0 ** e)
    rows = [(37 * j + 5) % n for j in range(8)]
    m = [3, -2, 0, 5, -4, 1, 2, -1]
    q = [1, 3, -2, 0, 2, -3, 4, -1]
    sign = [1, -1, -1, 1, -1, 1, -1, -1]
    B = np.zeros((8, n))
    want = np.zeros((8, n))
    sh = np.zeros(8)
    for j in range(8):
        a = 2.0 ** e[rows[j]]
        sh[j] = sign[j] * 2.0 ** q[j] - a
        assert a + sh[j] == sign[j] * 2.0 ** q[j] and np.float32(sh[j]) == sh[j]
        B[j, rows[j]] = 2.0 ** m[j]
        want[j, rows[j]] = sign[j] * 2.0 ** (m[j] - q[j])
    for dtype_name in DTYPES:
        dt = NP[dtype_name]
        with lam.Solver(getattr(lam, dtype_name)) as s:
            s.set_matrix(A)
            for nrhs in (1, 3, 8):
                what = f"{dtype_name} n={n} nrhs={nrhs}"
                s.set_rhs_many(B[:nrhs])
                conv = s.solve_minres(5, 1e-30, sh[:nrhs])
                X, it, cv, re = _result(s)
                assert conv.all() and (it == 1).all() and (re == 0.0).all() and s.get_option("multi_rhs_k") == K_FOR[nrhs], (what, it, cv, re)
                assert s.stats["num_iters"] == 1 and s.stats["converged"] and s.stats["rel_err"] == 0.0
                assert np.array_equal(X, want[:nrhs].astype(dt)), (what, X[:, rows[:nrhs]], want[:nrhs, rows[:nrhs]])
                assert (s.true_residuals() == 0.0).all(), (what, s.true_residuals())


# ------------------------------------------------------------------------------------------------
# 2. iteration by iteration against the model
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_every_column_tracks_the_model_iteration_by_iteration(lam, dtype_name):
    """solve_minres(k, 0), k = 1, 2, 5, 10, 20, 30, on the n = 384 tracking system under minres_data.TRACKING_SHIFTS (both signs, one
    within 1 % of the median eigenvalue, one negative definite): x and rel_err of column j against the model with its sums in
    "rows" order, within minres_data.GATE (10 x the model's own spread between its sum orders, tests/test_minres_cpu.py)."""
    dt = NP[dtype_name]
    A, B = tracking_columns()
    ref = D.tracking_histories(dt, "rows")
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.set_matrix(A)
        s.set_rhs_many(B)
        worst = {}
        for k in D.TRACKED_K:
            s.solve_minres(k, 0.0, D.TRACKING_SHIFTS)
            X, it, cv, re = _result(s)
            assert (it == k + 1).all() and not cv.any(), (k, it, cv)
            for j in range(8):
                _, x_ref, re_ref = ref[j][k - 1]
                d_x, d_re = D.rel_diff_x(X[j], x_ref), abs(re[j] / re_ref - 1)
                print(f"{dtype_name} k={k} column {j} shift {D.TRACKING_SHIFTS[j]}: x off by {d_x:.3e}, rel_err by {d_re:.3e} (gate {D.GATE[dt][k]:.1e})")
                worst[k] = max(worst.get(k, 0.0), d_x, d_re)
        for k in D.TRACKED_K:
            assert worst[k] < D.GATE[dt][k], (dtype_name, k, worst[k], D.GATE[dt][k], worst)


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_the_indefinite_tridiagonal_system_tracks_the_banded_model_past_the_wrap(lam, dtype_name):
    """n = 65537 > 256 workgroups x 256 threads on the device-filled tridiag(1,2,1) under shift -2 (tridiag(1,0,1): eigenvalues
    symmetric about zero), k = 1, 2, 5: every thread of the vector kernels takes a second element.  Reference: the banded model in
    "rows" order; gate per k: 10 x its own largest spread between its three orders over the 8 columns, x or rel_err, computed here by
    minres_data's rule."""
    n, dt = 65537, NP[dtype_name]
    B = np.random.default_rng(n).uniform(-1, 1, (8, n)).astype(dt)
    band = M.tridiag_band(n, dt)
    ks = (1, 2, 5)
    hist = {}
    for o in R.ORDERS:
        for j in range(8):
            h = []
            M.minres(None, -2.0, B[j], max(ks), 0.0, dt, o, band=band, history=h)
            hist[o, j] = h
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.generate_matrix(n)
        s.set_rhs_many(B)
        for k in ks:
            sp = max(max(D.rel_diff_x(hist[a, j][k - 1][1], hist[b, j][k - 1][1]), abs(hist[a, j][k - 1][2] / hist[b, j][k - 1][2] - 1))
                     for a in R.ORDERS for b in R.ORDERS if a != b for j in range(8))
            gate = 10 * sp
            s.solve_minres(k, 0.0, [-2.0] * 8)
            X, it, cv, re = _result(s)
            assert (it == k + 1).all() and not cv.any(), (k, it)
            for j in range(8):
                _, x_ref, re_ref = hist["rows", j][k - 1]
                d_x, d_re = D.rel_diff_x(X[j], x_ref), abs(re[j] / re_ref - 1)
                print(f"{dtype_name} n={n} k={k} column {j}: x off by {d_x:.3e}, rel_err by {d_re:.3e} (gate {gate:.1e})")
                assert d_x < gate and d_re < gate, (dtype_name, k, j, d_x, d_re, gate)


# ------------------------------------------------------------------------------------------------
# 3. columns never mix
# ------------------------------------------------------------------------------------------------
def _columns_alone(s, B, sh, cap, tol, what):
    """Every nrhs = 1..8 on its K: column j of the batch of the first nrhs columns against the column alone at K = 1.  A tridiagonal
    row has three products, which every lane meets in one order whatever the tile, so the comparison ACROSS K is bit for bit (a
    dense row is added up in another order at another K: tests/test_gpu_shifted.py)."""
    alone = []
    for j in range(8):
        s.set_rhs_many(B[j:j + 1])
        s.solve_minres(cap, tol, sh[j:j + 1])
        assert s.get_option("multi_rhs_k") == 1
        alone.append(_result(s))
    stops = [bool(a[2][0]) for a in alone]
    assert any(stops) and not all(stops), (what, [int(a[1][0]) for a in alone])       # some columns stop early, some hit the cap
    for nrhs in range(1, 9):
        s.set_rhs_many(B[:nrhs])
        s.solve_minres(cap, tol, sh[:nrhs])
        got = _result(s)
        assert s.get_option("multi_rhs_k") == K_FOR[nrhs]
        for j in range(nrhs):
            _assert_same_run(_column(got, j), alone[j], f"{what} nrhs={nrhs} column {j} shift {sh[j]}")
    # the same columns in the reverse order: column j with its shift in slot 7 - j
    s.set_rhs_many(B[::-1])
    s.solve_minres(cap, tol, sh[::-1])
    got = _result(s)
    for j in range(8):
        _assert_same_run(_column(got, 7 - j), alone[j], f"{what} reversed, column {j}")


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_a_column_of_the_batch_is_the_column_alone(lam, dtype_name):
    """n = 1030 (past the K = 8 and the K = 4 tile), A = tridiag(1, 2 + i mod 3, 1) uploaded from the host, eight shifts of both signs,
    cap 12, tolerance 1e-2: the strongly shifted columns stop, the indefinite ones run to the cap."""
    n, dt = 1030, NP[dtype_name]
    i = np.arange(n)
    A = np.diag(2.0 + i % 3) + np.diag(np.ones(n - 1), 1) + np.diag(np.ones(n - 1), -1)
    B = np.random.default_rng(n).uniform(-1, 1, (8, n)).astype(dt)
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.set_matrix(A)
        _columns_alone(s, B, np.array(MIXED_SHIFTS), 12, 1e-2, f"{dtype_name} n={n}")


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_a_column_of_the_batch_is_the_column_alone_past_the_wrap(lam, dtype_name):
    n, dt = 65537, NP[dtype_name]
    B = np.random.default_rng(n + 1).uniform(-1, 1, (8, n)).astype(dt)
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.generate_matrix(n)
        _columns_alone(s, B, np.array(MIXED_SHIFTS), 12, 1e-2, f"{dtype_name} n={n}")


# ------------------------------------------------------------------------------------------------
# 4. freezing and confinement
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[(d, n) for n in (7, 513, 1030) for d in DTYPES], ids=lambda p: f"{p[0]}-{p[1]}")
def smoke(lam, request):
    """The smoke system of size n and 8 right-hand sides; one context per (dtype, n)."""
    dtype_name, n = request.param
    dt = NP[dtype_name]
    A, rng = R.smoke_system(n, seed=n)
    A = A.astype(dt).astype(np.float64)
    B = rng.uniform(-1, 1, (8, n)).astype(dt)
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.set_matrix(A)
        yield dtype_name, n, dt, A, B, s


def test_a_stopped_column_is_frozen_and_nan_stays_in_its_column(lam, smoke):
    """Cap 10, tolerance 0.05, MIXED_SHIFTS: the strongly shifted columns stop within a few iterations.  A stopped column's x and
    rel_err are those of a run capped at its own stopping iteration that never stops (rel_error = 0), bit for bit.  With column 2's
    right-hand side zero, or one NaN in it, that column ends NaN at the cap and every other column is bit for bit what it was."""
    dtype_name, n, dt, A, B, s = smoke
    sh = np.array(MIXED_SHIFTS)
    cap, tol = 10, 0.05
    s.set_rhs_many(B)
    s.solve_minres(cap, tol, sh)
    base = _result(s)
    X, it, cv, re = base
    what = f"{dtype_name} n={n}"
    assert cv.any() and (re[cv] < tol).all() and (it[~cv] == cap + 1).all(), (what, it, cv, re)
    assert n <= cap or not cv.all(), (what, it)
    for k in sorted(set(it[cv].tolist())):
        s.solve_minres(k, 0.0, sh)
        Xk, itk, cvk, rek = _result(s)
        assert (itk == k + 1).all() and not cvk.any()
        for j in np.flatnonzero(cv & (it == k)):
            _assert_bits(X[j:j + 1], Xk[j:j + 1], f"{what}: column {j}, stopped at {k}")
            assert re[j] == rek[j], (what, j, re[j], rek[j])
    for poison in ("zero", "nan"):
        Bp = B.copy()
        if poison == "zero":
            Bp[2] = 0
        else:
            Bp[2, n // 2] = np.nan
        s.set_rhs_many(Bp)
        s.solve_minres(cap, tol, sh)
        got = _result(s)
        assert np.isnan(got[0][2]).all() and np.isnan(got[3][2]) and got[1][2] == cap + 1 and not got[2][2], (what, poison, got[1], got[3])
        assert np.isnan(s.stats["rel_err"]) and not s.stats["converged"]
        keep = [j for j in range(8) if j != 2]
        _assert_same_run(tuple(a[keep].copy() for a in got), tuple(a[keep].copy() for a in base), f"{what}: next to a {poison} column")


# ------------------------------------------------------------------------------------------------
# 5. it solves what CG cannot
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("n", D.INDEFINITE_SIZES)
def test_an_indefinite_system_converges_and_cg_is_refused_under_its_shift(lam, n, dtype_name):
    """The smoke system shifted into the middle of its widest central spectral gap (about half the eigenvalues negative): all 8
    columns converge within the cap, true_residuals() <= 2 x rel_error (the model's own is <= 1.1 x on these inputs,
    tests/test_minres_cpu.py), and solve_many on that state is refused naming the column and the value, the solution untouched."""
    dt = NP[dtype_name]
    A, B, shift, cap, tol = D.indefinite_case(n, dt)
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.set_matrix(A)
        s.set_rhs_many(B)
        conv = s.solve_minres(cap, tol, [shift] * 8)
        X, it, cv, re = _result(s)
        res = s.true_residuals()
        print(f"{dtype_name} n={n} shift {shift}: iterations {it.tolist()}, rel_err {re.tolist()}, true residuals {res.tolist()}")
        assert conv.all() and (it <= cap).all() and (re < tol).all() and s.stats["converged"], (it, cv, re)
        assert (res <= 2 * tol).all(), (res, tol)
        for j in range(8):
            host = M.true_residual(A, shift, X[j], B[j])
            assert host <= 2 * tol, (j, host, tol)
        launches = s.get_option("hip_calls_launch")
        for call in (lambda: s.solve_many(5, 1e-3), lambda: s.solve_many(5, 1e-3, lam.PC_JACOBI), lambda: s.solve_many(5, 1e-3, x0="continue"),
                     lambda: s.solve_many(5, 1e-3, x0=X)):
            with pytest.raises(lam.LamHipError) as e:
                call()
            assert e.value.code == EINVAL and f"shift 0 in force is {shift:g}" in str(e.value), e.value
        assert s.get_option("hip_calls_launch") == launches
        _assert_bits(s.solutions(), X, "the solution after the refused CG calls")
        assert np.array_equal(s.true_residuals(), res)


# ------------------------------------------------------------------------------------------------
# 6. SPD agreement
# ------------------------------------------------------------------------------------------------
def test_minres_and_cg_agree_on_spd_systems(lam, smoke):
    """Shifts >= 0 set with set_shifts, solve_minres(shifts=None) against solve_many, both converged to rel_error with true residuals
    <= 2 x rel_error each (asserted): ||x_m - x_c|| = ||(A + s I)^-1 (r_c - r_m)|| <= 4 rel_error ||b|| / lambda_min(A + s I), from the
    host matrix's eigenvalues."""
    dtype_name, n, dt, A, B, s = smoke
    tol = 1e-9 if dt is np.float64 else 1e-4
    sh = np.array([0.0, 0.5, 0.03125, 4.0, 0.25, 1.0, 2.0, 0.125])
    ev = np.linalg.eigvalsh(A)
    assert ev[0] > 0
    s.set_rhs_many(B)
    s.set_shifts(sh)
    assert s.solve_minres(20 * n + 50, tol).all()
    Xm, res_m = s.solutions(), s.true_residuals()
    assert s.solve_many(20 * n + 50, tol).all()
    Xc, res_c = s.solutions(), s.true_residuals()
    assert (res_m <= 2 * tol).all() and (res_c <= 2 * tol).all(), (res_m, res_c)
    for j in range(8):
        dist = np.linalg.norm(Xm[j].astype(np.float64) - Xc[j])
        bound = 4 * tol * np.linalg.norm(B[j].astype(np.float64)) / (ev[0] + sh[j])
        print(f"{dtype_name} n={n} column {j} shift {sh[j]}: MINRES and CG apart {dist:.3e}, bound {bound:.3e}")
        assert dist <= bound, (j, dist, bound)


# ------------------------------------------------------------------------------------------------
# 7. refusals and lifetime
# ------------------------------------------------------------------------------------------------
def test_refusals_and_lifetime(lam, monkeypatch):
    n = 64
    A = R.smoke_system(n)[0]
    B = np.random.default_rng(n).uniform(-1, 1, (2, n))

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
        assert "shard" in refused(s, EINVAL, s.solve_minres, 5, 1e-9, [1.0, -2.0])
    with lam.Solver(lam.BF16) as s:
        s.set_matrix(A)
        s.nrhs = 2
        assert "BF16" in refused(s, EINVAL, s.solve_minres, 5, 1e-9)
    monkeypatch.setenv("LAM_HIP_FORCE_RCCL", "1")      # a one-rank communicator: the rank mode on one GPU
    with lam.Solver(lam.F64, rank=0, nranks=1, device_id=0, unique_id=None) as s:
        monkeypatch.delenv("LAM_HIP_FORCE_RCCL")
        s.set_problem(n)
        s.upload_rows(0, A)
        s.nrhs = 2
        assert "rank mode" in refused(s, EINVAL, s.solve_minres, 5, 1e-9)
    with lam.Solver(lam.F64) as s:
        s.n, s.nrhs = n, 2
        refused(s, ESTATE, s.solve_minres, 5, 1e-9)                                # no problem yet
        s.set_matrix(A)
        assert "lam_hip_set_rhs_many" in refused(s, ESTATE, s.solve_minres, 5, 1e-9, [1.0, -2.0])      # before the right-hand sides
        assert s._L.lam_hip_solve_many_minres(None, None, 5, 1e-9, None, None, None, None) == EINVAL
        # a single solve on the same context, before and after
        b1 = np.random.default_rng(1).uniform(-1, 1, n)
        s.set_rhs(b1)
        s.solve(200, 1e-10)
        x1, t1 = s.solution(), s.true_residual()
        s.set_rhs_many(B)
        assert "max_iters" in refused(s, EINVAL, s.solve_minres, -1, 1e-9)
        s.solve_many(5, 1e-9)
        cg = _result(s)
        # max_iters = 0
        conv = s.solve_minres(0, 1e-9, [0.5, -2.0])
        X, it, cv, re = _result(s)
        assert not conv.any() and not X.any() and list(it) == [1, 1] and list(re) == [1.0, 1.0] and s.stats["num_iters"] == 1
        assert s.get_option("multi_rhs_k") == 2
        s.solve_minres(5, 0.0, [0.5, -2.0])
        want = _result(s)
        assert list(want[1]) == [6, 6] and not want[2].any()                       # rel_error <= 0 never stops
        for bad, word in (([np.nan, 1.0], "nan"), ([1.0, np.inf], "inf"), ([-np.inf, 1.0], "-inf")):
            msg = refused(s, EINVAL, s.solve_minres, 5, 0.0, bad)
            assert word in msg and f"shift {int(np.argmax(~np.isfinite(bad)))} " in msg, msg
        # a refused call leaves the shifts in force and the solution readable; sigma = NULL runs under them
        _assert_bits(s.solutions(), want[0], "after refused calls")
        s.solve_minres(5, 0.0)
        _assert_same_run(_result(s), want, "sigma = NULL after refused calls")
        # a negative shift in force: CG is refused, set_shifts keeps refusing one, a valid set_shifts or set_rhs_many lets CG run again
        assert "shift 1 in force is -2" in refused(s, EINVAL, s.solve_many, 5, 1e-9)
        assert ">= 0" in refused(s, EINVAL, s.set_shifts, [0.5, -2.0])
        s.set_shifts([0.5, 2.0])
        s.solve_many(5, 0.0, x0="continue")                                        # continues from MINRES' solution
        assert list(s.num_iters_many) == [6, 6]
        s.solve_minres(5, 0.0, [0.5, -2.0])
        s.set_rhs_many(B)                                                          # clears the negative shifts
        s.solve_many(5, 1e-9)
        _assert_same_run(_result(s), cg, "set_rhs_many clears the shifts")
        # all shifts zero: the unshifted product, and what no shifts at all give
        s.solve_minres(5, 0.0)
        plain = _result(s)
        s.solve_minres(5, 0.0, [0.0, -0.0])
        _assert_same_run(_result(s), plain, "zero shifts")
        # set_shifts' shifts are the ones in force for sigma = NULL
        s.set_shifts([0.5, 2.0])
        s.solve_minres(5, 0.0)
        a = _result(s)
        s.set_rhs_many(B)
        s.solve_minres(5, 0.0, [0.5, 2.0])
        _assert_same_run(_result(s), a, "set_shifts then sigma = NULL")
        assert not np.array_equal(a[0], plain[0])
        # the convenience: b replicated
        conv = s.solve_shifted_minres(B[0], [0.5, -2.0], 5, 0.0)
        assert conv.shape == (2,) and s.nrhs == 2
        s.set_rhs_many(np.stack([B[0], B[0]]))
        s.solve_minres(5, 0.0, [0.5, -2.0])
        rep = _result(s)
        s.solve_shifted_minres(B[0], [0.5, -2.0], 5, 0.0)
        _assert_same_run(_result(s), rep, "solve_shifted_minres")
        # the single solve was not disturbed
        assert np.array_equal(s.solution(), x1) and s.true_residual() == t1
    with lam.Solver(lam.F32) as s:
        s.set_matrix(A)
        s.set_rhs_many(B)
        msg = refused(s, EINVAL, s.solve_minres, 5, 1e-3, [1.0, -1e39])            # finite in fp64, -Inf in the vector dtype
        assert "shift 1 " in msg and "-1e+39" in msg, msg
        s.solve_minres(5, 1e-3, [1.0, -3e38])


# ------------------------------------------------------------------------------------------------
# 8. driver
# ------------------------------------------------------------------------------------------------
def test_driver_minres():
    """tridiag(1,2,1), n = 1024, b = 1 in both columns, -m -S -0.5,0.5 -T: one CSV line per column, the shift last, rel_err and the
    true residual below the tolerance.  (On the host the model takes 512 iterations under -0.5 -- b excites 512 eigenvectors -- and
    lands at 8e-13, and 24 under 0.5, at 7.6e-10 with the true residual equal to nine digits.)"""
    exe = os.path.join(ROOT, PKG_NAME, "test", "test_CG_multi_rhs.out")
    n, tol = 1024, 1e-9
    r = subprocess.run([exe, "-s", str(n), "-i", "5000", "-e", str(tol), "-m", "-S", "-0.5,0.5", "-T"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln.split(",") for ln in r.stdout.strip().splitlines()]
    assert len(lines) == 2 and all(ln[0] == str(n) and len(ln) == 12 for ln in lines), r.stdout
    assert [float(ln[-1]) for ln in lines] == [-0.5, 0.5], r.stdout
    print([ln[7] for ln in lines], [ln[8] for ln in lines], [ln[10] for ln in lines])
    assert all(1 <= int(ln[7]) <= 5000 and float(ln[8]) < tol and float(ln[10]) < tol for ln in lines), r.stdout
