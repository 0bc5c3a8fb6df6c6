"""Deflated CG for the batch on the device (lam_hip_set_deflation*, lam_hip_solve_many_deflated, lam_hip_deflate_many), held to exact
integer arithmetic, to exact known answers, to the numpy model tests/deflation_reference.py and to the plain batch of the same build.
Systems, gates and margins: tests/deflation_data.py, established without a GPU by tests/test_deflation_cpu.py."""
import os
import subprocess

import numpy as np
import pytest

import deflation_data as D
import generator_model as G
import lanczos_data as LD
from conftest import ROOT, PKG_NAME

pytestmark = pytest.mark.gpu

NP = D.DTYPES
EINVAL, ESTATE = -1, -6


def _refused(lam, code, call, *args, **kw):
    with pytest.raises(lam.LamHipError) as e:
        call(*args, **kw)
    assert e.value.code == code, e.value
    return str(e.value)


# ------------------------------------------------------------------------------------------------
# 1. the operator alone, exact
# ------------------------------------------------------------------------------------------------
def _integer_case(n, m, nrhs, seed):
    """Wd, Wa in {-1, 0, 1}, M in -2..2, U in -3..3, all int64, and the exact answer.  Every dot product is an fp64 sum of integers
    below 2^53; (TV)mu and every intermediate value of the fma chain must be integers below 2^24 for fp32 to hold them: asserted
    here on the exact values, prefix sum by prefix sum."""
    rng = np.random.default_rng(seed)
    Wd, Wa = rng.integers(-1, 2, (m, n)), rng.integers(-1, 2, (m, n))
    M, U = rng.integers(-2, 3, (m, m)), rng.integers(-3, 4, (nrhs, n))
    coeff = Wd @ U.T                                  # (m, nrhs)
    mu = M @ coeff
    out = U.copy()
    worst = int(np.abs(mu).max())
    for i in range(m):
        out -= mu[i][:, None] * Wa[i][None, :]
        worst = max(worst, int(np.abs(out).max()))
    assert worst < 2 ** 24 and int(np.abs(coeff).max()) < 2 ** 53, worst
    return Wd, Wa, M, U, coeff, out


# The sizes at which tests/test_gpu_eigs.py runs lam_hip_project_out, for its reasons: below one 16-byte vector, ragged for it,
# wrapping the grid of slabs, workgroups without rows (m below the 16 of the dots kernel's y) or without elements, several rounds per
# slab -- a slab is longer than one round of 2048 / K fp64 (4096 / K fp32, K <= 4) rows from 65537 (dots, K = 8) to 1048576 + 4099
# (apply, K = 1).  nrhs 3 and 5 leave padding columns.
@pytest.mark.parametrize("dtype_name", ["F64", "F32"])
@pytest.mark.parametrize("n,m,nrhs", [(1, 1, 1), (7, 3, 2), (65, 3, 3), (2049, 32, 5), (2049, 3, 8), (2049, 1, 4), (65537, 32, 8), (65536 + 257, 3, 2),
                                      (262144 + 4099, 32, 4), (262144 + 4099, 3, 8), (1048576 + 4099, 3, 1), (1048576 + 4099, 1, 3)])
def test_deflate_many_is_exact_on_integers(lam, dtype_name, n, m, nrhs):
    Wd, Wa, M, U, want_c, want_u = _integer_case(n, m, nrhs, 1000 * m + 10 * nrhs + n % 7)
    with lam.Solver(getattr(lam, dtype_name)) as s:
        coeff, got = s.deflate_many(Wd, Wa, M, U)
    assert got.dtype == NP[dtype_name] and coeff.shape == (m, nrhs) and got.shape == (nrhs, n)
    assert np.array_equal(coeff, want_c.astype(np.float64)), np.argwhere(coeff != want_c)[:5]
    assert np.array_equal(got.astype(np.float64), want_u.astype(np.float64)), np.argwhere(got != want_u)[:5]


@pytest.mark.parametrize("dtype_name", ["F64", "F32"])
@pytest.mark.parametrize("nrhs,bad", [(3, 1), (8, 6)])
def test_deflate_many_confines_a_nan_to_its_column(lam, dtype_name, nrhs, bad):
    n, m = 2049, 3
    Wd, Wa, M, U, want_c, want_u = _integer_case(n, m, nrhs, 5)
    Un = U.astype(np.float64)
    Un[bad, 1030] = np.nan
    with lam.Solver(getattr(lam, dtype_name)) as s:
        coeff, got = s.deflate_many(Wd, Wa, M, Un)
    others = np.arange(nrhs) != bad
    assert np.isnan(coeff[:, bad]).all() and np.isnan(got[bad]).any()
    assert np.array_equal(coeff[:, others], want_c[:, others].astype(np.float64))
    assert np.array_equal(got[others].astype(np.float64), want_u[others].astype(np.float64))


# ------------------------------------------------------------------------------------------------
# 2. exact known answers: A = diag of powers of two, W = two unit vectors
# ------------------------------------------------------------------------------------------------
EXACT_N = 2049
EXACT_A, EXACT_A2, EXACT_C = 6, 1028, 77          # e_a and e_a2 span W; e_c is outside it; d_a = 4, d_a2 = 1/4, d_c = 1


def _exact_diagonal():
    return 2.0 ** ((np.arange(EXACT_N) % 4) * 2 - 2)          # 1/4, 1, 4, 16


@pytest.mark.parametrize("symmetric_many", [0, 2])
@pytest.mark.parametrize("dtype_name", ["F64", "F32"])
def test_exact_known_answers(lam, dtype_name, symmetric_many):
    """Column 0, b in span(W): x0 = A^-1 b exactly and r = 0, born stopped.  Column 1, b = e_a + e_c: x0 takes e_a / d_a, p = r = e_c
    is an eigenvector, iteration 1 ends in r = 0 -- the plain batch needs 2 (two distinct eigenvalues).  Column 2 runs on behind
    them (four distinct eigenvalues outside W), and the two stopped columns keep their exact x bit for bit."""
    n, d = EXACT_N, _exact_diagonal()
    W = np.zeros((2, n))
    W[0, EXACT_A] = W[1, EXACT_A2] = 1.0
    B = np.zeros((3, n))
    B[0, EXACT_A], B[0, EXACT_A2] = 3.0, -2.0
    B[1, EXACT_A] = B[1, EXACT_C] = 1.0
    B[2] = np.random.default_rng(3).integers(-4, 5, n)
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.set_matrix(np.diag(d))
        s.set_option("symmetric_many", symmetric_many)
        s.set_rhs_many(B)
        tol = {"F64": 1e-12, "F32": 1e-5}[dtype_name]        # the plain run's second step ends at rounding level, not at 0
        s.solve_many(50, tol)
        plain = s.num_iters_many.copy()
        s.set_deflation(W)
        assert s.get_option("deflation_m") == 2
        s.solve_deflated(50, tol)
        X = s.solutions().astype(np.float64)
        print(f"{dtype_name} symmetric_many={symmetric_many}: plain {plain}, deflated {s.num_iters_many}, rel_err {s.rel_err_many}")
        assert s.get_option("symmetric_many_effective") == (1 if symmetric_many else 0)
        assert list(s.num_iters_many[:2]) == [0, 1] and s.converged_many.all()
        assert list(s.rel_err_many[:2]) == [0.0, 0.0]
        assert plain[1] == 2 and 1 < s.num_iters_many[2] <= plain[2]
        assert np.array_equal(X[0], B[0] / d) and np.array_equal(X[1], B[1] / d)
        # max_iters = 0 returns the k = 0 state: x0, column 0 born stopped, the others at the cap's count
        s.solve_deflated(0, tol)
        X0 = s.solutions().astype(np.float64)
        want = np.zeros(n)
        want[EXACT_A] = 0.25
        assert list(s.num_iters_many) == [0, 1, 1] and list(s.converged_many) == [True, False, False]
        assert np.array_equal(X0[0], B[0] / d) and np.array_equal(X0[1], want)


# ------------------------------------------------------------------------------------------------
# 3. recurrence parity
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[(n, d) for n in D.PARITY_SIZES for d in ("F64", "F32")], ids=lambda p: f"n{p[0]}-{p[1]}")
def parity(request, lam):
    n, dtype_name = request.param
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.set_matrix(LD.parity_matrix(n, dtype_name))
        yield lam, s, n, dtype_name


def _follow(s, n, dtype_name, m, ks):
    """Runs capped at every k of PARITY_K on the first K columns, for every K of ks; returns {(K, k): (X, rel_err)} and asserts the
    gates against the model."""
    B, W = D.parity_inputs(n, m)
    model = D.parity_model(n, dtype_name, m)
    gate = D.PARITY_GATE[(n, dtype_name, m)]
    s.set_deflation(W)
    got, worst = {}, {}
    for K in ks:
        s.set_rhs_many(B[:K])
        for k in D.PARITY_K:
            s.solve_deflated(k, 0.0)
            assert s.get_option("multi_rhs_k") == K and list(s.num_iters_many) == [k + 1] * K and not s.converged_many.any()
            X = s.solutions().astype(np.float64)
            got[(K, k)] = (X, s.rel_err_many.copy())
            Xm, rem = model[k]
            d_re = np.abs(s.rel_err_many / rem[:K] - 1).max()
            d_x = (np.linalg.norm(X - Xm[:K].astype(np.float64), axis=1) / np.linalg.norm(Xm[:K].astype(np.float64), axis=1)).max()
            worst[(K, k)] = (d_re, d_x)
            print(f"n={n} {dtype_name} m={m} K={K} k={k}: rel_err off by {d_re:.2e}, x by {d_x:.2e}; gate {gate[k]:.1e}")
    for (K, k), w in worst.items():
        assert max(w) <= gate[k], (K, k, w, gate[k])
    return got, gate


def test_every_column_follows_the_model(parity):
    lam, s, n, dtype_name = parity
    got, gate = _follow(s, n, dtype_name, D.PARITY_M, (1, 2, 4, 8))
    # a column of a batch is the same column solved alone, within the same gates
    for K in (2, 4, 8):
        for k in D.PARITY_K:
            (X1, re1), (XK, reK) = got[(1, k)], got[(K, k)]
            d_re, d_x = abs(reK[0] / re1[0] - 1), np.linalg.norm(XK[0] - X1[0]) / np.linalg.norm(X1[0])
            assert max(d_re, d_x) <= gate[k], (K, k, d_re, d_x, gate[k])


def test_the_largest_space_follows_the_model(parity):
    lam, s, n, dtype_name = parity
    if n != D.PARITY_M_LARGE[0]:
        return                                       # the one run with m = LAM_HIP_MAX_DEFLATION is at one size
    _follow(s, n, dtype_name, D.PARITY_M_LARGE[1], (8,))
    assert s.get_option("deflation_m") == lam.MAX_DEFLATION


# ------------------------------------------------------------------------------------------------
# 4. Ritz vectors end to end
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("symmetric_many", [0, 2])
@pytest.mark.parametrize("dtype_name", ["F64", "F32"])
def test_ritz_vectors_take_the_outliers_out_of_every_solve(lam, dtype_name, symmetric_many):
    n, tol = D.KNOWN_N, D.KNOWN_REL_ERROR[dtype_name]
    _, _, v0 = LD.known_inputs()
    B = D.known_rhs()
    model = D.known_model(dtype_name)
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.set_matrix(LD.known_matrix(dtype_name))
        s.set_option("symmetric_many", symmetric_many)
        s.set_rhs_many(B)
        s.solve_many(D.KNOWN_MAX_ITERS, tol)
        plain, true_plain = s.num_iters_many.copy(), s.true_residuals()
        assert s.converged_many.all()
        out = s.eigs(D.KNOWN_NEV, "both", max_steps=LD.KNOWN_MAX_STEPS, tol=LD.KNOWN_TOL[dtype_name], check_every=LD.KNOWN_CHECK_EVERY,
                     v0=v0.astype(NP[dtype_name]))
        assert out["nfound"] == D.KNOWN_NEV and out["converged"].all()
        s.set_deflation_from_eigs(D.KNOWN_NEV)
        assert s.get_option("deflation_m") == D.KNOWN_NEV
        s.solve_deflated(D.KNOWN_MAX_ITERS, tol)
        deflated, true_deflated = s.num_iters_many.copy(), s.true_residuals()
        assert s.get_option("symmetric_many_effective") == (1 if symmetric_many else 0)
        print(f"{dtype_name} symmetric_many={symmetric_many}: plain {plain} (model {model['plain']}), deflated {deflated} (model "
              f"{model['deflated']}); true residual plain {true_plain}, deflated {true_deflated} (model {model['true_deflated']})")
        assert s.converged_many.all()
        assert (deflated < plain).all()
        assert (np.abs(deflated - model["deflated"]) <= D.KNOWN_ITER_MARGIN[dtype_name]).all()
        assert (true_deflated <= D.KNOWN_TRUE_MARGIN[dtype_name] * true_plain).all()
        # afterwards the batch holds a batched solution: plain CG continues it
        s.solve_many(D.KNOWN_MAX_ITERS, tol, x0="continue")
        assert s.converged_many.all() and (s.num_iters_many < plain).all()


# ------------------------------------------------------------------------------------------------
# 5. non-interference, determinism
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", ["F64", "F32"])
def test_a_space_changes_no_other_solve_and_two_deflated_calls_agree(lam, dtype_name):
    n = 130
    rng = np.random.default_rng(11)
    B = rng.uniform(-1, 1, (3, n)).astype(NP[dtype_name])
    W = rng.uniform(-1, 1, (4, n))

    def everything(s):
        out = []
        s.set_rhs_many(B)
        s.solve_many(25, 1e-6)
        out += [s.solutions(), s.num_iters_many.copy(), s.rel_err_many.copy()]
        s.solve_many(25, 1e-6, lam.PC_JACOBI)
        out += [s.solutions(), s.num_iters_many.copy(), s.rel_err_many.copy()]
        s.solve_many(5, 0.0)
        s.solve_many(25, 1e-6, x0="continue")
        out += [s.solutions(), s.num_iters_many.copy(), s.rel_err_many.copy()]
        s.solve_many(25, 1e-6, x0=0.5 * B)
        out += [s.solutions(), s.num_iters_many.copy(), s.rel_err_many.copy()]
        s.solve_minres(25, 1e-6, shifts=[0.0, 0.5, -0.25])
        out += [s.solutions(), s.num_iters_many.copy(), s.rel_err_many.copy()]
        s.solve_multishift(B[0], [0.0, 0.5, 2.0], 25, 1e-6)
        out += [s.multishift_solutions(), s.num_iters_shift.copy(), s.rel_err_shift.copy()]
        s.generate_random_rhs(4)
        s.solve(60, 1e-6)
        out += [s.solution(), np.array([s.stats["num_iters"]]), np.array([s.stats["rel_err"]])]
        return out

    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.generate_random_spd(n, 5, 100.0)
        without = everything(s)
        s.set_deflation(W)
        with_space = everything(s)
        assert s.get_option("deflation_m") == 4               # no solve, no new right-hand sides touched the space
        for a, b in zip(without, with_space):
            assert np.array_equal(G.bits(a), G.bits(b))
        runs = []
        for _ in range(2):
            s.set_rhs_many(B)
            s.solve_deflated(25, 1e-6)
            runs.append((s.solutions(), s.num_iters_many.copy(), s.rel_err_many.copy(), s.true_residuals()))
        for a, b in zip(*runs):
            assert np.array_equal(G.bits(a), G.bits(b))
        # setting the same space again gives the same bits too
        s.set_deflation(W)
        s.solve_deflated(25, 1e-6)
        assert np.array_equal(G.bits(s.solutions()), G.bits(runs[0][0]))


# ------------------------------------------------------------------------------------------------
# 6. launch accounting
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("symmetric_many", [0, 2])
@pytest.mark.parametrize("nrhs", [1, 3, 8])
def test_an_iteration_is_a_fixed_number_of_launches(lam, nrhs, symmetric_many):
    """include/lam_hip.h: 5 launches per iteration -- the plain batch's three and two more -- and 6 under symmetric_many at K <= 4.
    Counted as the difference between two capped runs, so the launches in front of the loop cancel."""
    per = 6 if symmetric_many and nrhs <= 4 else 5
    n = 130
    rng = np.random.default_rng(1)
    with lam.Solver(lam.F64) as s:
        s.generate_random_spd(n, 5, 1e4)
        s.set_option("symmetric_many", symmetric_many)
        s.set_deflation(rng.uniform(-1, 1, (5, n)))
        s.set_rhs_many(rng.uniform(-1, 1, (nrhs, n)))
        counts = {}
        for iters in (3, 11):
            l0 = s.get_option("hip_calls_launch")
            s.solve_deflated(iters, 0.0)
            counts[iters] = s.get_option("hip_calls_launch") - l0
        assert counts[11] - counts[3] == per * 8, counts
        assert s.stats["gemv_bytes"] > 0 and s.get_option("multi_rhs_k") == (1 if nrhs == 1 else 4 if nrhs == 3 else 8)


# ------------------------------------------------------------------------------------------------
# 7. refusals and lifetime
# ------------------------------------------------------------------------------------------------
def test_refusals(lam, monkeypatch):
    n = 48
    A = G.random_spd(n, 1, 10.0)
    rng = np.random.default_rng(2)
    W = rng.uniform(-1, 1, (3, n))
    B = rng.uniform(-1, 1, (2, n))
    with lam.Solver(lam.F64, device_ids=[0, 0]) as s:
        s.set_matrix(A)
        assert "shards: the multi-right-hand-side path supports one shard only" in _refused(lam, EINVAL, s.set_deflation, W)
        assert "one shard only" in _refused(lam, EINVAL, s.set_deflation_from_eigs, 1)
        s.nrhs = 1
        assert "one shard only" in _refused(lam, EINVAL, s.solve_deflated, 5, 1e-6)
    with lam.Solver(lam.BF16) as s:
        s.set_matrix(A)
        assert "LAM_HIP_BF16 storage is not supported" in _refused(lam, EINVAL, s.set_deflation, W)
    monkeypatch.setenv("LAM_HIP_FORCE_RCCL", "1")      # a one-rank communicator: the rank mode on one GPU
    with lam.Solver(lam.F64, rank=0, nranks=1, device_id=0, unique_id=None) as s:
        monkeypatch.delenv("LAM_HIP_FORCE_RCCL")
        s.set_problem(n)
        s.upload_rows(0, A)
        assert "rank mode" in _refused(lam, EINVAL, s.set_deflation, W)
    with lam.Solver(lam.F64) as s:
        s.set_problem(n)
        assert "matrix" in _refused(lam, ESTATE, s.set_deflation, W)               # no matrix
        assert "matrix" in _refused(lam, ESTATE, s.set_deflation_from_eigs, 1)
        s.upload_rows(0, A)
        assert s.get_option("deflation_m") == 0
        assert "m = 33" in _refused(lam, EINVAL, s.set_deflation, np.ones((33, n)))
        assert "m = -1" in _refused(lam, EINVAL, s.set_deflation_from_eigs, -1)
        _refused(lam, ESTATE, s.set_deflation_from_eigs, 2)                         # no eigen-solution
        s.eigs(2, max_steps=8, tol=0.0)
        assert "2 pairs were found" in _refused(lam, EINVAL, s.set_deflation_from_eigs, 3)
        s.set_rhs_many(B)
        assert "no deflation space" in _refused(lam, ESTATE, s.solve_deflated, 5, 1e-6)
        bad = W.copy()
        bad[1, 7] = np.nan
        assert "vector 1, element 7" in _refused(lam, EINVAL, s.set_deflation, bad)
        bad[1, 7] = np.inf
        assert "vector 1, element 7" in _refused(lam, EINVAL, s.set_deflation, bad)
        dup = W.copy()
        dup[2] = dup[0]
        assert "column 2" in _refused(lam, EINVAL, s.set_deflation, dup)             # rank-deficient: the duplicate's pivot
        zero = W.copy()
        zero[1] = 0.0
        assert "column 1" in _refused(lam, EINVAL, s.set_deflation, zero)
        assert s.get_option("deflation_m") == 0                                     # nothing was set by a refused call
        s.set_deflation(W)
        assert s.get_option("deflation_m") == 3
        s.solve_deflated(40, 1e-8)
        X = s.solutions()
        assert "column 2" in _refused(lam, EINVAL, s.set_deflation, dup)
        assert s.get_option("deflation_m") == 3                                     # the previous space stays
        _refused(lam, ESTATE, s.solutions)                                          # ... but the staging vectors were used
        s.solve_deflated(40, 1e-8)
        assert np.array_equal(G.bits(s.solutions()), G.bits(X))
        # shifts: a non-zero one in force is refused by name, zeros are not
        s.set_shifts([0.0, 0.5])
        assert "shift 1 in force is 0.5" in _refused(lam, EINVAL, s.solve_deflated, 40, 1e-8)
        s.set_shifts([0.0, 0.0])
        s.solve_deflated(40, 1e-8)
        assert "max_iters" in _refused(lam, EINVAL, s.solve_deflated, -1, 1e-8)
        # m = 0 clears; N below the limit bounds m
        s.set_deflation(None)
        assert s.get_option("deflation_m") == 0
        assert "no deflation space" in _refused(lam, ESTATE, s.solve_deflated, 5, 1e-6)
        # the operator's own argument checks
        assert "LAM_HIP_MAX_DEFLATION" in _refused(lam, EINVAL, s.deflate_many, np.ones((33, 4)), np.ones((33, 4)), np.eye(33), np.ones(4))
        assert "LAM_HIP_MAX_RHS" in _refused(lam, EINVAL, s.deflate_many, np.ones((2, 4)), np.ones((2, 4)), np.eye(2), np.ones((9, 4)))
    with lam.Solver(lam.F64) as s:                                                  # min(N, LAM_HIP_MAX_DEFLATION)
        s.set_matrix(np.diag([1.0, 2.0, 3.0]))
        assert "must be 0..3" in _refused(lam, EINVAL, s.set_deflation, np.ones((4, 3)))


@pytest.mark.parametrize("dtype_name", ["F64", "F32"])
def test_a_new_matrix_invalidates_the_space(lam, dtype_name):
    n = 130
    rng = np.random.default_rng(9)
    B = rng.uniform(-1, 1, (3, n)).astype(NP[dtype_name])
    W = rng.uniform(-1, 1, (2, n))
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.generate_random_spd(n, 5, 100.0)
        s.set_rhs_many(B)
        s.set_deflation(W)
        s.solve_deflated(40, 1e-6)
        X = s.solutions()
        # lam_hip_eigs and new right-hand sides leave it alone
        s.eigs(2, "both", max_steps=16, tol=0.0)
        s.set_rhs_many(B)
        assert s.get_option("deflation_m") == 2
        s.solve_deflated(40, 1e-6)
        assert np.array_equal(G.bits(s.solutions()), G.bits(X))
        # a generator call, an upload and lam_hip_set_problem invalidate it
        s.generate_random_spd(n, 6, 100.0, keep_problem=True)
        assert s.get_option("deflation_m") == 0
        assert "no deflation space" in _refused(lam, ESTATE, s.solve_deflated, 40, 1e-6)
        s.set_deflation(W)
        A = s.download_rows(0, n)
        s.upload_rows(0, A[:1])
        assert s.get_option("deflation_m") == 0
        _refused(lam, ESTATE, s.solve_deflated, 40, 1e-6)
        s.set_deflation(W)
        s.set_problem(n)
        assert s.get_option("deflation_m") == 0
        s.upload_rows(0, A)
        s.set_rhs_many(B)
        _refused(lam, ESTATE, s.solve_deflated, 40, 1e-6)
        s.set_deflation(W)
        s.solve_deflated(40, 1e-6)


# ------------------------------------------------------------------------------------------------
# 8. driver
# ------------------------------------------------------------------------------------------------
EXE = os.path.join(ROOT, PKG_NAME, "test", "test_CG_multi_rhs.out")


def _run(*args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, timeout=300)


def test_driver_solves_deflated():
    """N = 200: lam_hip_eigs' cap of min(N, 256) steps spans the whole space, so the four Ritz vectors are eigenvectors to rounding
    and the model gives 97 iterations against the plain run's 100 (the constant right-hand side meets the 100 symmetric eigenvectors
    only).  At N = 384 the cap leaves the four pairs unconverged (bounds of 1e-3), such a W breaks that symmetry, and model and
    device alike need 287 iterations against 192: a space is only as good as its vectors."""
    base = ("-s", 200, "-k", 3, "-i", 2000, "-e", 1e-9)
    plain, deflated = _run(*base), _run(*base, "-D", 4)
    assert plain.returncode == 0 and deflated.returncode == 0, plain.stderr[-1000:] + deflated.stderr[-2000:]
    rows_p = [ln.split(",") for ln in plain.stdout.strip().splitlines()]
    rows_d = [ln.split(",") for ln in deflated.stdout.strip().splitlines()]
    assert len(rows_p) == len(rows_d) == 3 and all(len(f) == len(rows_p[0]) for f in rows_p + rows_d)
    for p, d in zip(rows_p, rows_d):
        assert int(d[0]) == int(p[0]) == 200 and 0 < int(d[7]) <= int(p[7]) <= 2000 and float(d[8]) < 1e-9, (p, d)


@pytest.mark.parametrize("extra", [["-J"], ["-w", "3"], ["-S", "0.5"], ["-M"], ["-m"], ["-D", "0"], ["-D", "33"], ["-E", "2"]])
def test_driver_refuses_conflicting_flags(extra):
    args = ["-s", 64] + ([] if extra[0] == "-D" else ["-D", 2]) + extra
    r = _run(*args)
    assert r.returncode == 1 and "Usage" in r.stderr and r.stdout == "", (extra, r.stderr)
