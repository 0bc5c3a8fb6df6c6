"""Multi-shift CG, (A + s_j I) x_j = b for every shift behind the single-column product of the seed system: lam_hip_solve_mshift,
lam_hip_get_solution_mshift, lam_hip_true_residual_mshift (include/lam_hip.h), i.e. mshift_init / step / copy_seed / residual_kernel
(csrc/lam_kernels.h) and the hook of multi_solve (csrc/lam_multi.h).

Sizes: N in {1, 7, 513, 1030} (the K = 1 p tile is 4096 columns; 1030 is ragged) and 65537 on the device-filled tridiag(1,2,1), where
a thread of every vector launch takes a second element; S in {1, 8, 9, 64}: one group, a full group, a second group that is mostly
padding, the maximum.

 1. exact: A = I, shifts 2^m - 1, every slot of every group bit for bit; 2. the seed's slots are the K = 1 batch bit for bit;
 3. every shift iteration by iteration against tests/mshift_reference.py; 4. converged runs against solve_shifted in groups of 8;
 5. past the wrap; 6. freeze, cap, underflow, NaN; 7. refusals and lifetime; 8. the driver's -M."""
import os
import subprocess

import numpy as np
import pytest

import mshift_reference as M
import pcg_reference as R
import shifted_data as SD
from conftest import ROOT, PKG_NAME
from tracking_data import ITERATION_TRACKING_GATES

pytestmark = pytest.mark.gpu

DTYPES = ("F64", "F32")
NP = {"F64": np.float64, "F32": np.float32}
U_TV = {"F64": 2.0 ** -53, "F32": 2.0 ** -24}
EINVAL, ESTATE = -1, -6
GROUP_SIZES = (1, 8, 9, 64)
# nine shifts in no order: the seed (0) twice, first group full, the ninth alone in a second group; each exact in fp32
TRACK_SHIFTS = (0.5, 0.0, 2.0, 0.125, 8.0, 0.03125, 32.0, 1.0, 0.0)
WRAP_SHIFTS = (0.0, 2.0, 6.0, 0.5, 14.0, 0.0, 1.0, 30.0, 3.0)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _assert_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = np.argwhere(_bits(got) != _bits(want))
    if bad.size:
        j, i = bad[0]
        raise AssertionError(f"{what}: {len(bad)} entries differ in shifts {sorted(set(bad[:, 0].tolist()))}, first (shift, row) = ({j}, {i}): "
                             f"got {got[j, i]!r}, want {want[j, i]!r}; next {bad[1:6].tolist()}")


def _rel(X, Xref):
    X, Xref = X.astype(np.float64), Xref.astype(np.float64)
    return np.linalg.norm(X - Xref, axis=-1) / np.linalg.norm(Xref, axis=-1)


def _host_true(A, sh, X, b):
    b = b.astype(np.float64)
    return np.array([np.linalg.norm(b - A @ x - s * x) for s, x in zip(sh, X.astype(np.float64))]) / np.linalg.norm(b)


@pytest.fixture(scope="module", params=[(d, n) for n in (513, 1030) for d in DTYPES], ids=lambda p: f"{p[0]}-{p[1]}")
def dense(lam, request):
    """The smoke system of size n in the storage type's values and one right-hand side; one context per (dtype, n)."""
    dtype_name, n = request.param
    dt = NP[dtype_name]
    A, rng = R.smoke_system(n, seed=n)
    A = A.astype(dt).astype(np.float64)
    b = rng.uniform(-1, 1, n).astype(dt)
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.set_matrix(A)
        yield dtype_name, n, dt, A, b, s


@pytest.fixture(scope="module", params=DTYPES)
def tridiag(lam, request):
    """tridiag(1,2,1) at n = 65537, filled on the device, and one right-hand side."""
    n, dt = 65537, NP[request.param]
    b = np.random.default_rng(n).uniform(-1, 1, n).astype(dt)
    with lam.Solver(getattr(lam, request.param)) as s:
        s.generate_matrix(n)
        yield request.param, n, dt, b, s


# ------------------------------------------------------------------------------------------------
# 1. exact
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 513, 1030])
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_identity_with_power_of_two_shifts_is_exact_in_every_slot(lam, dtype_name, n):
    """A = I, b small integers, s_j = 2^m_j - 1 with the m_j scrambled over the 64 slots (0..22, so exact in fp32; repeats are 23
    apart).  Every sum is exact: the seed (the smallest m of the S slots in use) stops at k = 1 with r = 0, zeta_1 = 2^(m_min - m_j),
    x_j = b 2^-m_j bit for bit, num_iters 1, converged, rel_err 0, and the device's true residuals are exactly 0.  A coefficient taken
    from another slot or group is another power of two."""
    dt = NP[dtype_name]
    m = np.random.default_rng(64).permutation(64) % 23
    b = (np.arange(n) % 7 - 3.0).astype(dt)
    b[b == 0] = 5
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.set_matrix(np.eye(n))
        for S in GROUP_SIZES:
            sh = 2.0 ** m[:S] - 1
            conv = s.solve_multishift(b, sh, 5, 1e-30)
            what = f"{dtype_name} n={n} S={S}"
            assert conv.all() and (s.num_iters_shift == 1).all() and (s.rel_err_shift == 0).all(), (what, s.num_iters_shift, s.rel_err_shift)
            assert s.stats["num_iters"] == 1 and s.stats["converged"] == 1 and s.stats["rel_err"] == 0
            _assert_bits(s.multishift_solutions(), (b[None, :].astype(np.float64) * 2.0 ** -m[:S, None]).astype(dt), what)
            res = s.multishift_true_residuals()
            assert (res == 0).all(), (what, res)


# ------------------------------------------------------------------------------------------------
# 2. the seed is the batch
# ------------------------------------------------------------------------------------------------
def _seed_is_the_batch(lam, s, dtype_name, n, b, make_matrix, cap, tol, what):
    for smin in (0.25, 0.0):
        for S in (1, 9, 64):
            sh = smin + np.abs(np.random.default_rng(S).uniform(0.5, 8, S)).round(3)
            slots = sorted({0, S - 1, S // 2, min(8, S - 1)})       # first, last, duplicated, and the second group's first
            sh[slots] = smin
            s.solve_multishift(b, sh, cap, tol)
            X = s.multishift_solutions()
            got = (s.num_iters_shift.copy(), s.converged_shift.copy(), s.rel_err_shift.copy())
            seed_x, seed_res = s.solutions(), s.true_residuals(1)   # the batch state afterwards is the seed's
            with lam.Solver(getattr(lam, dtype_name)) as f:
                make_matrix(f)
                f.solve_shifted(b, [smin], cap, tol)
                want_x, want_res = f.solutions(), f.true_residuals()
                w = f"{what} s_min={smin} S={S}"
                for j in slots:
                    _assert_bits(X[j:j + 1], want_x, f"{w} slot {j}")
                    assert got[0][j] == f.num_iters_many[0] and got[1][j] == f.converged_many[0], (w, j, got[0][j], f.num_iters_many)
                    assert _bits(got[2][j:j + 1]) == _bits(f.rel_err_many), (w, j, got[2][j], f.rel_err_many)
                _assert_bits(seed_x, want_x, w + ": the batch's X")
                assert _bits(seed_res) == _bits(want_res), (w, seed_res, want_res)
            assert s.get_option("multi_rhs_k") == 1
            if S > 1:
                assert not np.array_equal(X[1], X[0]), w


def test_the_seed_slots_are_the_k1_batch_bit_for_bit(lam, dense):
    dtype_name, n, dt, A, b, s = dense
    _seed_is_the_batch(lam, s, dtype_name, n, b, lambda f: f.set_matrix(A), 12, 1e-3, f"{dtype_name} n={n}")


def test_the_seed_slots_are_the_k1_batch_bit_for_bit_past_the_wrap(lam, tridiag):
    dtype_name, n, dt, b, s = tridiag
    _seed_is_the_batch(lam, s, dtype_name, n, b, lambda f: f.generate_matrix(n), 12, 1e-3, f"{dtype_name} n={n}")


# ------------------------------------------------------------------------------------------------
# 3. every shift, iteration by iteration
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_every_shift_tracks_the_model_iteration_by_iteration(lam, dtype_name):
    """n = 513, cap k = 1 .. 20 with rel_error = 0, one call per cap: x and rel_err of every shift after k iterations against the
    model's.  fp64: tracking_data.ITERATION_TRACKING_GATES, the residual gate for rel_err and the x gate for x, of the next listed
    k (the model's own spread between summation orders on this system is 6e-16 ... 1.3e-15 in x, a hundredth of the gates, so they
    fit).  fp32: 10 x the spread, per k, between the model's three summation orders (pcg_reference.ORDERS) on this very system,
    over the shifts, x or rel_err, whichever is larger -- tracking_data's rule, one gate for both."""
    n, dt = 513, NP[dtype_name]
    A, rng = R.smoke_system(n, seed=n)
    A = A.astype(dt).astype(np.float64)
    b = rng.uniform(-1, 1, n).astype(dt)
    sh = np.array(TRACK_SHIFTS)
    seed = sh == 0

    def rel_errs(h):
        return np.where(seed, h["rel"], h["rel_err"])

    ref = M.mshift_cg(M.dense_operator(A, dt), b, sh, 20, 0.0, dt, snapshots=True)[2]
    if dtype_name == "F32":
        H = [M.mshift_cg(M.ordered_operator(A, dt, o), b, sh, 20, 0.0, dt, dot=M.ordered_dot(o), snapshots=True)[2] for o in R.ORDERS]
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.set_matrix(A)
        for k in range(1, 21):
            if dtype_name == "F64":
                gate_re, gate_x = [(g_res, g_x) for kk, g_res, g_x in ITERATION_TRACKING_GATES if kk >= k][0]
            else:
                pairs = [(a, c) for a in range(3) for c in range(3) if a != c]
                sp_x = max(_rel(H[a][k - 1]["X"], H[c][k - 1]["X"]).max() for a, c in pairs)
                sp_re = max(np.abs(rel_errs(H[a][k - 1]) / rel_errs(H[c][k - 1]) - 1).max() for a, c in pairs)
                gate_re = gate_x = 10 * max(sp_x, sp_re)
            s.solve_multishift(b, sh, k, 0.0)
            X = s.multishift_solutions()
            assert (s.num_iters_shift == k + 1).all() and not s.converged_shift.any(), (k, s.num_iters_shift)
            d = _rel(X, ref[k - 1]["X"])
            d_re = np.abs(s.rel_err_shift / rel_errs(ref[k - 1]) - 1)
            print(f"{dtype_name} k={k}: x off by {d.max():.3e} (gate {gate_x:.1e}), rel_err by {d_re.max():.3e} (gate {gate_re:.1e})")
            assert (d < gate_x).all() and (d_re < gate_re).all(), (dtype_name, k, d.tolist(), d_re.tolist(), gate_x, gate_re)


# ------------------------------------------------------------------------------------------------
# 4. converged runs against solve_shifted in groups of 8
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [9, 64])
@pytest.mark.parametrize("n", [513, 1030])
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_converged_shifts_against_the_shifted_batch(lam, dtype_name, n, S):
    """mshift_reference.converged_system / converged_shifts (cond ~ e^7, shifts 0 ... 100), rel_error 1e-10 (fp64) / 1e-5 (fp32).  Per
    shift, fp64 on the host: true = ||b - (A_TV + s I) x|| / ||b|| of the multi-shift x and of solve_shifted's in groups of 8.
      a: true_ms <= 2 max(true_batch, rel_error): two recurrences that stop a few iterations apart;
      b: |num_iters_ms - num_iters_batch| <= 2 x mshift_reference.MODEL_ITERS_DEVIATION, the largest deviation the CPU model shows
         against per-shift model CG on these systems (tests/test_mshift_cpu.py);
    every shift converges; multishift_true_residuals() agrees with the host value under tests/shifted_data.py's bound."""
    dt, tol = NP[dtype_name], {"F64": 1e-10, "F32": 1e-5}[dtype_name]
    A, b = M.converged_system(n, dt)
    sh = M.converged_shifts(S)
    absA = np.abs(A)
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.set_matrix(A)
        conv = s.solve_multishift(b, sh, 4000, tol)
        X, it = s.multishift_solutions(), s.num_iters_shift.copy()
        res = s.multishift_true_residuals()
        assert conv.all() and s.stats["converged"] == 1 and s.stats["num_iters"] == it.max(), (it, conv)
        assert (s.rel_err_shift < tol).all()
        Xb, itb = np.empty_like(X), np.zeros(S, int)
        for first in range(0, S, 8):
            cb = s.solve_shifted(b, sh[first:first + 8], 4000, tol)
            assert cb.all()
            Xb[first:first + 8], itb[first:first + 8] = s.solutions(), s.num_iters_many
    t_ms, t_b = _host_true(A, sh, X, b), _host_true(A, sh, Xb, b)
    ratio = t_ms / np.maximum(t_b, tol)
    dev = np.abs(it - itb)
    gate_b = 2 * M.MODEL_ITERS_DEVIATION[dtype_name]
    print(f"{dtype_name} n={n} S={S}: true_ms / max(true_batch, tol) up to {ratio.max():.3f}; iterations {it.min()}..{it.max()}, "
          f"|ms - batch| up to {dev.max()} (gate {gate_b})")
    assert (ratio <= 2).all(), (ratio.tolist(), t_ms.tolist(), t_b.tolist())
    assert (dev <= gate_b).all(), (it.tolist(), itb.tolist())
    u = U_TV[dtype_name]
    for j in range(S):
        x = X[j].astype(np.float64)
        bound = SD.true_residual_bound(absA @ np.abs(x), b.astype(np.float64), sh[j], x, n, u) + 2 * (n + 8) * 2.0 ** -53 * t_ms[j]
        assert abs(res[j] - t_ms[j]) <= bound, (j, sh[j], res[j], t_ms[j], bound)


# ------------------------------------------------------------------------------------------------
# 5. past the wrap
# ------------------------------------------------------------------------------------------------
def test_every_shift_tracks_the_model_past_the_wrap(lam, tridiag):
    """n = 65537, S = 9, cap 12, rel_error = 0: x of every shift against the O(N) model, over all rows and over the rows a thread takes
    in its second trip (65536 on) explicitly.  Gates as in 3: fp64 ITERATION_TRACKING_GATES' x gate at k = 20; fp32 10 x the model's
    own spread between its three dot-product orders and two orders of the three-term row sum."""
    dtype_name, n, dt, b, s = tridiag
    sh = np.array(WRAP_SHIFTS)
    ref = M.mshift_cg(M.tridiag_operator(dt), b, sh, 12, 0.0, dt)[0]
    if dtype_name == "F64":
        gate = [g for kk, _, g in ITERATION_TRACKING_GATES if kk >= 12][0]
    else:
        def other(p):
            y = p.copy()
            y[1:] += p[:-1]
            y = y + p
            y[:-1] += p[1:]
            return y
        V = [M.mshift_cg(M.tridiag_operator(dt), b, sh, 12, 0.0, dt, dot=M.ordered_dot(o))[0] for o in R.ORDERS]
        V.append(M.mshift_cg(other, b, sh, 12, 0.0, dt)[0])
        gate = 10 * max(_rel(a, c).max() for i, a in enumerate(V) for c in V[i + 1:])
    s.solve_multishift(b, sh, 12, 0.0)
    X = s.multishift_solutions()
    assert (s.num_iters_shift == 13).all() and not s.converged_shift.any()
    d = _rel(X, ref)
    rms = np.linalg.norm(ref.astype(np.float64), axis=1) / np.sqrt(n)
    tail = np.abs(X[:, 65536].astype(np.float64) - ref[:, 65536]) / rms
    print(f"{dtype_name} n={n}: x off by {d.max():.3e} (gate {gate:.1e}); row 65536 off by {tail.max():.3e} of a typical element")
    assert (d < gate).all(), (d.tolist(), gate)
    # one element against the typical one: a vector within `gate` in norm has elements off by `gate` of the typical one on
    # average; 8 x that for a single element -- a row the second trip never reaches is off by 1
    assert (tail < 8 * gate).all() and np.all(X[:, 65536] != 0), (tail.tolist(), gate)


# ------------------------------------------------------------------------------------------------
# 6. freeze, cap, underflow, NaN
# ------------------------------------------------------------------------------------------------
def test_a_stopped_shift_is_frozen_and_the_cap_counts_as_the_batch_counts(lam, dense):
    dtype_name, n, dt, A, b, s = dense
    sh = np.array(TRACK_SHIFTS)
    s.solve_multishift(b, sh, 200, 1e-3)
    X, it, cv = s.multishift_solutions(), s.num_iters_shift.copy(), s.converged_shift.copy()
    assert cv.all() and it.max() == it[sh == 0][0] and len(set(it.tolist())) >= 4, it
    for k in sorted(set(it.tolist()))[:-1]:
        s.solve_multishift(b, sh, int(k), 1e-3)
        at = it == k
        _assert_bits(s.multishift_solutions()[at], X[at], f"{dtype_name} n={n}: shifts that stop at {k}, run on to {it.max()}")
        assert (s.num_iters_shift[at] == k).all() and s.converged_shift[at].all()
        later = it > k
        assert (s.num_iters_shift[later] == k + 1).all() and not s.converged_shift[later].any(), (k, s.num_iters_shift)
        assert s.stats["num_iters"] == k + 1 and s.stats["converged"] == 0
    s.solve_multishift(b, sh, 0, 1e-3)
    assert (s.num_iters_shift == 1).all() and not s.converged_shift.any() and (s.rel_err_shift == 1).all()
    assert not s.multishift_solutions().any()


def test_an_underflowing_zeta_freezes_the_shift_with_a_finite_answer(lam, dense):
    """cap 70, rel_error = 0, s = 1e6 next to the seed and a moderate shift: zeta of 1e6 falls by ~1e-6 per iteration and leaves
    fp64's normal range; the shift is frozen before that step with x finite and within rounding of the direct solve -- cond(A + 1e6 I)
    is 1 + 1e-5, the product's error is relative to a diagonal that carries all of it: 32 u of the vector dtype."""
    dtype_name, n, dt, A, b, s = dense
    sh = np.array([0.5, 1e6, 0.0])
    s.solve_multishift(b, sh, 70, 0.0)
    X, it, cv, re = s.multishift_solutions(), s.num_iters_shift, s.converged_shift, s.rel_err_shift
    assert np.isfinite(X).all() and np.isfinite(re).all() and not cv.any(), (it, re)
    assert it[0] == 71 and it[2] == 71 and 5 < it[1] < 70, it
    direct = np.linalg.solve(A + np.float64(dt(1e6)) * np.eye(n), b.astype(np.float64))
    err = _rel(X[1], direct)
    print(f"{dtype_name} n={n}: frozen after {it[1]} steps at rel_err {re[1]:.3e}, x off the direct solve by {err:.3e}")
    assert err <= 32 * U_TV[dtype_name], err


def test_a_zero_right_hand_side_runs_to_the_cap_as_nan_and_the_context_stays_usable(lam, dense):
    dtype_name, n, dt, A, b, s = dense
    sh = np.array(TRACK_SHIFTS)
    s.solve_multishift(b, sh, 6, 1e-3)
    want = s.multishift_solutions()
    s.solve_multishift(np.zeros(n, dt), sh, 6, 1e-3)
    assert (s.num_iters_shift == 7).all() and not s.converged_shift.any() and np.isnan(s.rel_err_shift).all(), (s.num_iters_shift, s.rel_err_shift)
    assert np.isnan(s.multishift_solutions()).all() and np.isnan(s.stats["rel_err"])
    s.solve_multishift(b, sh, 6, 1e-3)
    _assert_bits(s.multishift_solutions(), want, f"{dtype_name} n={n}: after the NaN run")


# ------------------------------------------------------------------------------------------------
# 7. refusals and lifetime
# ------------------------------------------------------------------------------------------------
def test_refusals_and_lifetime(lam, monkeypatch):
    n = 64
    A = R.smoke_system(n)[0]
    b = np.ones(n)

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
        assert "shard" in refused(s, EINVAL, s.solve_multishift, b, [0.0, 1.0], 5, 1e-9)
    with lam.Solver(lam.BF16) as s:
        s.set_matrix(A)
        assert "BF16" in refused(s, EINVAL, s.solve_multishift, b, [0.0, 1.0], 5, 1e-9)
    monkeypatch.setenv("LAM_HIP_FORCE_RCCL", "1")      # a one-rank communicator: the rank mode on one GPU
    with lam.Solver(lam.F64, rank=0, nranks=1, device_id=0, unique_id=None) as s:
        monkeypatch.delenv("LAM_HIP_FORCE_RCCL")
        s.set_problem(n)
        s.upload_rows(0, A)
        assert "rank mode" in refused(s, EINVAL, s.solve_multishift, b, [0.0, 1.0], 5, 1e-9)
    with lam.Solver(lam.F64) as s:
        s.set_problem(n)
        refused(s, ESTATE, s.solve_multishift, b, [0.0, 1.0], 5, 1e-9)             # no matrix set
        s.nshifts = 2
        refused(s, ESTATE, s.multishift_solutions)                                 # before a solve
        refused(s, ESTATE, s.multishift_true_residuals)
        s.upload_rows(0, A)
        assert "LAM_HIP_MAX_SHIFTS" in refused(s, EINVAL, s.solve_multishift, b, [], 5, 1e-9)
        assert "LAM_HIP_MAX_SHIFTS" in refused(s, EINVAL, s.solve_multishift, b, [1.0] * 65, 5, 1e-9)
        for bad, word in (([0.0, -1.0], "-1"), ([np.nan, 1.0], "nan"), ([1.0, 2.0, np.inf], "inf")):
            msg = refused(s, EINVAL, s.solve_multishift, b, bad, 5, 1e-9)
            assert word in msg and f"shift {int(np.argmax([not (v >= 0 and np.isfinite(v)) for v in bad]))} " in msg, msg
        assert s._L.lam_hip_solve_mshift(None, None, 1, None, 1, 0.0, None, None, None, None) == EINVAL
        # interleaved with the single solve: neither disturbs the other
        s.set_rhs(2 * b)
        s.solve(50, 1e-9)
        x_single = s.solution()
        s.solve_multishift(b, [0.5, 0.0, 2.0], 50, 1e-9)
        want = s.multishift_solutions()
        assert np.array_equal(s.solution(), x_single)
        s.solve(50, 1e-9)
        assert np.array_equal(s.solution(), x_single)
        _assert_bits(s.multishift_solutions(), want, "after lam_hip_solve")
        res = s.multishift_true_residuals()
        _assert_bits(s.multishift_solutions(), want, "after the true residuals")
        assert (res < 1e-8).all() and _bits(s.solutions()).tolist() == _bits(want[1:2]).tolist()
        s.nshifts = 3
        refused(s, EINVAL, lambda: s._chk(s._L.lam_hip_get_solution_mshift(s._h, 4, want.ctypes.data)))      # more than were solved
        # the batch calls end its readability
        s.set_rhs_many(np.stack([b, b]))
        refused(s, ESTATE, s.multishift_solutions)
        s.solve_multishift(b, [0.5, 0.0, 2.0], 50, 1e-9)
        s.solve_many(3, 1e-9, x0="continue")                                       # the seed's batch continues ...
        refused(s, ESTATE, s.multishift_solutions)                                 # ... and is no longer the multi-shift run's seed
        s.solve_multishift(b, [0.5, 0.0, 2.0], 50, 1e-9)
        s.gemv_many(b[None, :])
        refused(s, ESTATE, s.multishift_true_residuals)
        s.solve_multishift(b, [0.5, 0.0, 2.0], 50, 1e-9)
        s.upload_rows(0, A)                                                        # a new matrix
        refused(s, ESTATE, s.multishift_solutions)
        s.solve_multishift(b, [0.5, 0.0, 2.0], 50, 1e-9)
        _assert_bits(s.multishift_solutions(), want, "solved again")
        s.set_problem(n)
        s.nshifts = 3
        refused(s, ESTATE, s.multishift_solutions)
    with lam.Solver(lam.F32) as s:
        s.set_matrix(A)
        msg = refused(s, EINVAL, s.solve_multishift, b, [1.0, 1e39], 5, 1e-5)      # finite in fp64, Inf in the vector dtype
        assert "shift 1 " in msg and "1e+39" in msg, msg
        assert s.solve_multishift(b, [1.0, 3e38], 5, 1e-5).shape == (2,)


# ------------------------------------------------------------------------------------------------
# 8. driver
# ------------------------------------------------------------------------------------------------
def test_driver_multishift(lam):
    """tridiag(1,2,1), n = 513, b = 1: -M -S ... -T against the binding's results on the same system, line by line; -M without -S,
    with -J, with -w is refused with a usage message and no output."""
    exe = os.path.join(ROOT, PKG_NAME, "test", "test_CG_multi_rhs.out")
    n, tol = 513, 1e-9
    sh = [4.0, 0.0, 0.5, 16.0, 0.0, 1.0, 2.0, 8.0, 0.25, 32.0]
    for prec, dtype_name in (("f64", "F64"), ("f32", "F32")):
        with lam.Solver(getattr(lam, dtype_name)) as s:
            s.generate_matrix(n)
            s.solve_multishift(np.ones(n), sh, 3000, tol)
            it, re, res = s.num_iters_shift, s.rel_err_shift, s.multishift_true_residuals()
        r = subprocess.run([exe, "-s", str(n), "-i", "3000", "-e", str(tol), "-t", prec, "-S", ",".join(map(str, sh)), "-M", "-T"],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = [ln.split(",") for ln in r.stdout.strip().splitlines()]
        assert len(lines) == len(sh) and all(ln[0] == str(n) and len(ln) == 12 for ln in lines), r.stdout
        assert [float(ln[-1]) for ln in lines] == sh and [int(ln[7]) for ln in lines] == it.tolist(), (r.stdout, it)
        assert np.allclose([float(ln[8]) for ln in lines], re, rtol=1e-5, atol=0) and np.allclose([float(ln[10]) for ln in lines], res, rtol=1e-5, atol=0)
    for args in (["-M"], ["-M", "-S", "0,1", "-J"], ["-M", "-S", "0,1", "-w", "2"]):
        r = subprocess.run([exe, "-s", "16", "-i", "3"] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "Usage" in r.stderr and "-M" in r.stderr and not r.stdout, (args, r.returncode, r.stdout, r.stderr)
