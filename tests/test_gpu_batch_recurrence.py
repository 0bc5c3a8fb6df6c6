"""The batched CG recurrences past their first step, Jacobi included: multi_init/xr/p_kernel, pcg_init/xr/p_kernel, the interleave /
de-interleave pair (csrc/lam_kernels.h) through lam_hip_solve_many / _solve_many_pc / _gemv_many.

A. Jacobi with a NON-constant diagonal, bit for bit.  C is symmetric positive definite with a unit diagonal (the smoke system
   divided by sqrt(d_i d_j), tests/pcg_reference.py), S = diag(2^e_i) with integer e_i in [-6, 6] that differ between neighbouring
   rows, A = S C S.  Every product, partial sum and scalar of the Jacobi run on (A, S b) is the plain run's on (C, b) times an exact
   power of two (multi_p_kernel's comment makes the contraction argument), so x_jacobi[i] = 2^-e_i x_plain[i] BIT FOR BIT for every
   column and every iteration count; a wrong index into dinv anywhere breaks it in the rows it touches.  tests/test_pcg_cpu.py
   holds the same identity on the numpy restatement.  rel_err of the plain run stays above 1e-30 (nothing underflows, no 0/0);
   where the cap is k = n the last step annihilates the residual (exactly, for n = 1: C = [1], alpha = 1, r = b - b), so there the
   floor is asserted on the residual that ENTERED the last step (the run capped at k - 1).
   The independent known answer is the exact first Jacobi step on the integer system of tests/exact_data.py with a power-of-two
   diagonal d_i in {1, 2, 4, 8}: fp32 is exact while 8 * 64 n < 2^24, n <= 32767 (that file's docstring).
B. The grid-stride wrap: vec_grid() caps the vector kernels at 256 workgroups of 256 threads, so from n = 65537 on a thread
   handles a second element.  tridiag(1,2,1) filled on the device (no host matrix; the reference is the stencil on integer
   vectors) at n = 65537 and 65536 + 257.  A non-constant diagonal cannot be reached cheaply at this size (an upload of 17 GB in
   fp32): beyond element 65536 dinv is pinned as the constant 0.5 only, in position through A's sizes only.
C. Every column iteration by iteration: fp64 against the oracle with the gates of
   test_gpu_parity.py::test_cg_matches_oracle_iteration_by_iteration (imported), fp32 against tests/pcg_reference.py with gates
   from that reference's own spread between summation orders (tests/tracking_data.py, FP32_TRACKING_GATE; fp32 is followed at
   k = 10 and 30 too, and its k = 40 is informational: the fp32 reference no longer agrees with itself there).
D. A change of K over dirty pad rows: after a K = 8 batch with a NaN column and a 1e30 column, the rows behind P's end in every
   other K's layout hold NaN; the exact product and the exact first steps must not notice."""
import functools

import numpy as np
import pytest

import exact_data as E
import pcg_reference as R
from tracking_data import (FP32_TRACKING_GATE, ITERATION_TRACKING_GATES, TRACKED_K, TRACKED_K_FP32, scaled_case, scaled_tracking_system,
                           tracking_columns)

pytestmark = pytest.mark.gpu

DTYPES = ("F64", "F32")
NP = {"F64": np.float64, "F32": np.float32}
U_TV = {"F64": 2.0 ** -53, "F32": 2.0 ** -24}
K_FOR = {1: 1, 2: 2, 3: 4, 4: 4, 5: 8, 6: 8, 7: 8, 8: 8}
KS = (1, 2, 5, 40)

def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _assert_bits(got, want, what):
    """got, want: (columns, n).  The message names the first bad (column, row), what is there and what belongs there."""
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = np.argwhere(_bits(got) != _bits(want))
    if bad.size:
        j, i = bad[0]
        raise AssertionError(f"{what}: {len(bad)} entries differ in columns {sorted(set(bad[:, 0].tolist()))}, first (column, row) = ({j}, {i}): "
                             f"got {got[j, i]!r}, want {want[j, i]!r}; next {bad[1:6].tolist()}")


def _result(s):
    return s.solutions(), s.num_iters_many.copy(), s.converged_many.copy(), s.rel_err_many.copy()


# ------------------------------------------------------------------------------------------------
# A. Jacobi with a non-constant diagonal
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 5, 255, 256, 257, 1025, 2049, 4097])
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_jacobi_on_a_scaled_system_is_the_plain_batch_scaled_bit_for_bit(lam, dtype_name, n):
    dt = NP[dtype_name]
    Cm, e, s, A, Bh = scaled_case(n, dt)
    Bs = (s * Bh).astype(dt)                                                       # exact
    with lam.Solver(getattr(lam, dtype_name)) as sc, lam.Solver(getattr(lam, dtype_name)) as sa:
        sc.set_matrix(Cm)
        sa.set_matrix(A)
        assert _same(sc.diagonal(), np.ones(n, dt))
        _assert_bits(sa.diagonal()[None], (4.0 ** e).astype(dt)[None], f"{dtype_name} n={n} diagonal")
        for nrhs in range(1, 9):
            sc.set_rhs_many(Bh[:nrhs])
            sa.set_rhs_many(Bs[:nrhs])
            for k in sorted({min(k, n) for k in KS}):
                sc.solve_many(k, 0.0)
                X0, it0, cv0, re0 = _result(sc)
                sa.solve_many(k, 0.0, lam.PC_JACOBI)
                X1, it1, cv1, re1 = _result(sa)
                what = f"{dtype_name} n={n} nrhs={nrhs} k={k}"
                print(f"{what}: plain rel_err {re0.min():.3e} ... {re0.max():.3e}")
                assert sa.get_option("multi_rhs_k") == K_FOR[nrhs] and (it0 == k + 1).all() and (it1 == k + 1).all(), (what, it0, it1)
                assert not cv0.any() and not cv1.any() and np.isfinite(X0).all() and np.isfinite(re1).all(), what
                if k < n:
                    assert (re0 > 1e-30).all(), (what, re0)
                elif k > 1:      # k = n: the residual that entered the last step (module docstring)
                    sc.solve_many(k - 1, 0.0)
                    assert (sc.rel_err_many > 1e-30).all(), (what, sc.rel_err_many)
                _assert_bits(X1, (X0 / s).astype(dt), what)


@pytest.mark.parametrize("n", [257, 1025])
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_a_column_frozen_in_the_jacobi_run_keeps_its_bits_and_disturbs_nobody(lam, dtype_name, n):
    """Tolerance 1e-3, cap 12: column 1 is an eigenvector of C (one step: tests/test_pcg_cpu.py shows the pattern on the reference)
    and stops, the random columns run to the cap.  The frozen x is the x of its stop iteration -- the same batch capped there, and
    2^-e times the plain run capped there -- and the running columns hold the bits of the run without a tolerance."""
    dt, cap, tol = NP[dtype_name], 12, 1e-3
    Cm, e, s, A, Bh = scaled_case(n, dt)
    Bh = Bh.copy()
    Bh[1] = np.linalg.eigh(Cm)[1][:, n // 2].astype(dt)
    Bs = (s * Bh).astype(dt)
    with lam.Solver(getattr(lam, dtype_name)) as sc, lam.Solver(getattr(lam, dtype_name)) as sa:
        sc.set_matrix(Cm)
        sa.set_matrix(A)
        sc.set_rhs_many(Bh)
        sa.set_rhs_many(Bs)
        sa.solve_many(cap, 0.0, lam.PC_JACOBI)
        Xfree = sa.solutions()
        sa.solve_many(cap, tol, lam.PC_JACOBI)
        X, it, cv, re = _result(sa)
        what = f"{dtype_name} n={n}: iterations {it.tolist()}, rel_err {re.tolist()}"
        running = [j for j in range(8) if j != 1]
        assert cv[1] and it[1] <= 2 and re[1] < tol and not cv[running].any() and (it[running] == cap + 1).all(), what
        assert sa.stats["num_iters"] == cap + 1 and sa.stats["converged"] == 0, what
        _assert_bits(X[running], Xfree[running], what + " (running columns)")
        stop = int(it[1])
        sa.solve_many(stop, tol, lam.PC_JACOBI)
        X2, it2, cv2, re2 = _result(sa)
        assert cv2[1] and it2[1] == stop and re2[1] == re[1] and (it2[running] == stop + 1).all(), (what, it2, re2)
        _assert_bits(X[1:2], X2[1:2], what + " (frozen column against the batch capped at its stop)")
        sc.solve_many(stop, 0.0)
        _assert_bits(X2, (sc.solutions() / s).astype(dt), what + f" (every column against the plain run capped at {stop})")


@pytest.mark.parametrize("n", [1025, 10001])
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_first_jacobi_step_exact(lam, dtype_name, n):
    """solve_many(1, 1e-30, PC_JACOBI) on the integer matrix with diagonal d_i in {1, 2, 4, 8}: x1 = fl(alpha_TV z0) bit for bit with
    z0 = b / d and alpha = fl64(r.z / p.Ap), both sums exact; rel_err within exact_data.rel_err_bound with A z0 in place of A b."""
    assert n <= E.MAX_EXACT_N_FP32_JACOBI
    with lam.Solver(getattr(lam, dtype_name)) as s:
        vdt = s.vec_dtype
        d = E.pow2_diagonal(n, 11 * n)
        B = [E.int_vec(n, 13 * n + j) for j in range(8)]
        s.set_problem(n)
        AZ = E.generate(n, [s.upload_rows], [b / d for b in B], diag=d)
        _assert_bits(s.diagonal()[None], d.astype(vdt)[None], f"{dtype_name} n={n} diagonal")
        for nrhs in (1, 3, 8):
            s.set_rhs_many(np.stack(B[:nrhs]))
            conv = s.solve_many(1, 1e-30, lam.PC_JACOBI)
            X = s.solutions()
            assert not conv.any() and list(s.num_iters_many) == [2] * nrhs and s.stats["num_iters"] == 2
            steps = [E.first_pcg_step(B[j], d, AZ[j], vdt) for j in range(nrhs)]
            _assert_bits(X, np.stack([x1 + vdt(0) for _, x1, _, _ in steps]), f"{dtype_name} n={n} nrhs={nrhs} (alphas {[a for a, _, _, _ in steps]})")
            for j, (alpha, _, bb, r1) in enumerate(steps):
                re_host, bound = E.rel_err_bound(B[j], AZ[j], alpha, r1, bb, U_TV[dtype_name])
                assert abs(s.rel_err_many[j] - re_host) <= bound, (dtype_name, n, nrhs, j, s.rel_err_many[j], re_host, bound)


# ------------------------------------------------------------------------------------------------
# B. the grid-stride wrap
# ------------------------------------------------------------------------------------------------
WRAP = [("F32", 65537), ("F32", 65536 + 257), ("F64", 65537), ("F64", 65536 + 257)]


@pytest.fixture(scope="module", params=WRAP, ids=lambda p: f"{p[0]}-{p[1]}")
def wrap(lam, request):
    """One context per (dtype, n) with tridiag(1,2,1) filled on the device, shared by the tests of this section."""
    dtype_name, n = request.param
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.generate_matrix(n)
        assert s.n == n > 256 * 256          # past vec_grid()'s cap: a thread of every vector kernel handles a second element
        yield dtype_name, n, s


def _wrap_columns(n):
    rng = np.random.default_rng(n)
    i = np.arange(1, n + 1)
    return [np.ones(n), np.sin(3 * np.pi * i / (n + 1))] + [rng.uniform(-1, 1, n) for _ in range(6)]     # smooth, an eigenvector, rough


def test_wrap_gemv_many_exact(wrap):
    dtype_name, n, s = wrap
    X = np.stack([E.int_vec(n, 100 * n + j) for j in range(8)])
    Y = E.tridiag_product(X)
    for nrhs in (1, 2, 3, 8):
        _assert_bits(s.gemv_many(X[:nrhs]), Y[:nrhs].astype(s.vec_dtype), f"{dtype_name} n={n} nrhs={nrhs}")


def test_wrap_first_steps_exact(lam, wrap):
    """Plain and Jacobi (dinv = 0.5), integer b, every column."""
    dtype_name, n, s = wrap
    vdt = s.vec_dtype
    B = np.stack([E.int_vec(n, 7 * n + j) for j in range(8)])
    AB = E.tridiag_product(B)
    two = np.full(n, 2.0)
    assert _same(s.diagonal(), two.astype(vdt))
    for nrhs in (1, 3, 8):
        s.set_rhs_many(B[:nrhs])
        for precond in (lam.PC_NONE, lam.PC_JACOBI):
            s.solve_many(1, 1e-30, precond)
            X = s.solutions()
            assert list(s.num_iters_many) == [2] * nrhs
            for j in range(nrhs):
                if precond == lam.PC_NONE:
                    alpha, x1, bb, _, r1 = E.first_cg_step(B[j], AB[j], vdt)
                    Ap = AB[j]
                else:
                    Ap = AB[j] / 2                        # A z0, z0 = b / 2: exact
                    alpha, x1, bb, r1 = E.first_pcg_step(B[j], two, Ap, vdt)
                _assert_bits(X[j:j + 1], (x1 + vdt(0))[None], f"{dtype_name} n={n} nrhs={nrhs} precond={precond} column {j} of the batch (alpha {alpha!r})")
                re_host, bound = E.rel_err_bound(B[j], Ap, alpha, r1, bb, U_TV[dtype_name])
                assert abs(s.rel_err_many[j] - re_host) <= bound, (dtype_name, n, nrhs, precond, j, s.rel_err_many[j], re_host, bound)


def test_wrap_jacobi_is_the_plain_batch_after_40_iterations(lam, wrap):
    dtype_name, n, s = wrap
    cols = _wrap_columns(n)
    for nrhs in (3, 8):
        s.set_rhs_many(np.stack(cols[:nrhs]))
        s.solve_many(40, 0.0)
        X0, it0, cv0, re0 = _result(s)
        s.solve_many(40, 0.0, lam.PC_JACOBI)
        X1, it1, cv1, re1 = _result(s)
        what = f"{dtype_name} n={n} nrhs={nrhs}"
        assert np.isfinite(X0).all() and (it0 == 41).all() and (it1 == 41).all() and not cv0.any() and not cv1.any(), (what, it0, it1)
        assert _same(re0, re1) and (re0 < 1.0).all(), (what, re0, re1)
        _assert_bits(X1, X0, what)


def test_wrap_a_column_of_the_batch_is_the_column_alone(lam, wrap):
    """Cap 12, tolerance 1e-3, plain and Jacobi: K = 8 against K = 1, column by column: x, iteration count, converged, rel_err.
    Column 1 is an eigenvector of tridiag(1,2,1) and stops after one step while the others run to the cap, so the per-column
    stop state of both sets of kernels is compared past the wrap, not only 13 == 13."""
    dtype_name, n, s = wrap
    B = np.stack(_wrap_columns(n)).astype(s.vec_dtype)
    for precond in (lam.PC_NONE, lam.PC_JACOBI):
        s.set_rhs_many(B)
        s.solve_many(12, 1e-3, precond)
        X, it, cv, re = _result(s)
        assert cv[1] and it[1] <= 2 and not cv[2:].any() and (it[2:] == 13).all(), (dtype_name, n, precond, it, cv, re)
        for j in range(8):
            s.set_rhs_many(B[j:j + 1])
            s.solve_many(12, 1e-3, precond)
            assert s.get_option("multi_rhs_k") == 1
            what = (f"{dtype_name} n={n} precond={precond} column {j} (shown as column 0): alone {int(s.num_iters_many[0])} iterations, rel_err "
                    f"{s.rel_err_many[0]!r}; in the batch {int(it[j])}, {re[j]!r}")
            _assert_bits(s.solutions(), X[j:j + 1], what)
            assert s.num_iters_many[0] == it[j] and s.converged_many[0] == cv[j] and s.rel_err_many[0] == re[j], what


# ------------------------------------------------------------------------------------------------
# C. every column, iteration by iteration
# ------------------------------------------------------------------------------------------------
def _gates(dtype_name):
    """k -> (gate on rel_err / ref - 1, gate on ||x - x_ref|| / ||x_ref||)"""
    if dtype_name == "F64":
        return {k: (g_res, g_x) for k, g_res, g_x in ITERATION_TRACKING_GATES if k in TRACKED_K}
    assert sorted(FP32_TRACKING_GATE) == list(TRACKED_K_FP32) and set(TRACKED_K) <= set(TRACKED_K_FP32)
    return {k: (g, g) for k, g in FP32_TRACKING_GATE.items()}


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_every_column_tracks_the_reference_iteration_by_iteration(lam, oracle, dtype_name):
    """solve_many(k, 1e-30), k = 1, 2, 5, 20, 40 (fp32: 10 and 30 too), 8 different right-hand sides: every column's x and rel_err.
    fp64: against oracle.cg_solve with the single solve's gates.  fp32: against pcg_reference.pcg_ordered(dtype=float32, order="rows")
    -- pcg statement for statement with its sums in a fixed order, so the reference has the same bits on every machine -- with
    FP32_TRACKING_GATE, 10 x that reference's spread between summation orders (the table in tests/tracking_data.py, which
    tests/test_pcg_cpu.py re-measures); its k = 40 is informational (gate 0.76), k = 30 is the last that pins fp32."""
    dt = NP[dtype_name]
    A, B = tracking_columns()
    gates = _gates(dtype_name)
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.set_matrix(A)
        s.set_rhs_many(B)
        for k in sorted(gates):
            s.solve_many(k, 1e-30)
            X, it, _, re = _result(s)
            assert (it == k + 1).all(), (dtype_name, k, it)
            for j in range(8):
                if dtype_name == "F64":
                    x_ref, st_ref = oracle.cg_solve(A, B[j], k, 1e-30)
                else:
                    x_ref, st_ref = R.pcg_ordered(A, B[j], k, 1e-30, None, dt, "rows")
                    x_ref = x_ref.astype(np.float64)
                d_re = abs(re[j] / st_ref["rel_err"] - 1)
                d_x = np.linalg.norm(X[j].astype(np.float64) - x_ref) / np.linalg.norm(x_ref)
                print(f"{dtype_name} k={k} column {j}: rel_err off by {d_re:.3e} (gate {gates[k][0]:.1e}), x by {d_x:.3e} (gate {gates[k][1]:.1e})")
                assert st_ref["num_iters"] == k + 1 and d_re < gates[k][0] and d_x < gates[k][1], (dtype_name, k, j, d_re, d_x, gates[k])


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_jacobi_rel_err_tracks_the_reference_iteration_by_iteration(lam, dtype_name):
    """x of the Jacobi run is pinned by section A together with the plain tracking; this pins its rel_err -- sqrt(r.r / b.b), NOT
    the r.z the recurrence runs on -- against pcg_reference.pcg with dinv (fp32: pcg_ordered "rows"), same k, same gates.
    tests/test_pcg_cpu.py holds that reference's own spread between summation orders on this system below a tenth of them."""
    dt = NP[dtype_name]
    A, Bs, dinv = scaled_tracking_system(dt)
    gates = _gates(dtype_name)
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.set_matrix(A)
        s.set_rhs_many(Bs)
        for k in sorted(gates):
            s.solve_many(k, 1e-30, lam.PC_JACOBI)
            assert (s.num_iters_many == k + 1).all(), (dtype_name, k, s.num_iters_many)
            for j in range(8):
                _, st_ref = (R.pcg if dtype_name == "F64" else functools.partial(R.pcg_ordered, order="rows"))(A, Bs[j], k, 1e-30, dinv, dt)
                d_re = abs(s.rel_err_many[j] / st_ref["rel_err"] - 1)
                print(f"{dtype_name} jacobi k={k} column {j}: rel_err {s.rel_err_many[j]:.6e}, off by {d_re:.3e} (gate {gates[k][0]:.1e})")
                assert d_re < gates[k][0], (dtype_name, k, j, s.rel_err_many[j], st_ref["rel_err"], d_re, gates[k][0])


# ------------------------------------------------------------------------------------------------
# D. K changes over dirty pad rows
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1025, 4097 + 1])
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_a_change_of_K_does_not_see_what_another_K_left_behind_P(lam, dtype_name, n):
    """Before EVERY check a K = 8 batch runs 20 iterations with a NaN column and a 1e30 column: in the layout of K = 4, 2, 1 the
    rows behind P's end then hold NaN (K = 8's rows n/2, n/4, n/8 ...), which the last ragged 16-byte vector of every matrix row
    multiplies with the zeros of the row padding.  Sequence of nrhs 4, 2, 1, 1, 2: K = 8 -> 4 -> 8 -> 2 -> 8 -> 1 and 1 -> 8 -> 2.
    gemv_many_only (which clears P its own way) runs in between too."""
    with lam.Solver(getattr(lam, dtype_name)) as s:
        vdt = s.vec_dtype
        d = E.pow2_diagonal(n, 17 * n)
        B = [E.int_vec(n, 19 * n + j) for j in range(4)]
        s.set_problem(n)
        prod = E.generate(n, [s.upload_rows], B + [b / d for b in B], diag=d)
        AB, AZ = np.stack(prod[:4]), np.stack(prod[4:])
        B = np.stack(B)
        dirty = np.stack([E.int_vec(n, 23 * n + j) for j in range(8)])
        dirty[3] = np.nan
        dirty[5] *= 1e30

        def soil():
            s.set_rhs_many(dirty)
            s.solve_many(20, 0.0)
            assert s.get_option("multi_rhs_k") == 8 and np.isnan(s.solutions()[3]).all() and (s.num_iters_many == 21).all()

        def first_step(nrhs, precond, what):
            s.set_rhs_many(B[:nrhs])
            s.solve_many(1, 1e-30, precond)
            assert s.get_option("multi_rhs_k") == K_FOR[nrhs]
            if precond == lam.PC_NONE:
                want = [E.first_cg_step(B[j], AB[j], vdt)[1] for j in range(nrhs)]
            else:
                want = [E.first_pcg_step(B[j], d, AZ[j], vdt)[1] for j in range(nrhs)]
            _assert_bits(s.solutions(), np.stack(want) + vdt(0), what)

        for step, nrhs in enumerate((4, 2, 1, 1, 2)):
            what = f"{dtype_name} n={n} step {step} nrhs={nrhs} after a K = 8 batch with a NaN column"
            soil()
            _assert_bits(s.gemv_many(B[:nrhs]), AB[:nrhs].astype(vdt), what + ": gemv_many")
            soil()
            first_step(nrhs, lam.PC_NONE, what + ": first plain step")
            soil()
            first_step(nrhs, lam.PC_JACOBI, what + ": first Jacobi step")
            soil()
            s.gemv_many_only(8 if step % 2 else nrhs, 1)
            first_step(nrhs, lam.PC_NONE, what + ": first plain step after gemv_many_only")
            s.gemv_many_only(nrhs, 1)
            _assert_bits(s.gemv_many(B[:nrhs]), AB[:nrhs].astype(vdt), what + ": gemv_many after gemv_many_only")
