"""Lanczos quadrature for the batch: lam_hip_lanczos_many, lam_hip_get_lanczos_many and lam_hip_trace_quadrature (include/lam_hip.h),
i.e. quad_probe / start_scalars / start / three_term / next_kernel (csrc/lam_kernels.h) around the batch's product.

Sizes: the fp64 K = 8 p tile is 512 columns, the K = 4 tile 1024, the K = 1 tile 4096, and the vector kernels wrap at N = 65537; so N
in {1, 7, 513, 1030, 4097} and 65537 on the device-filled tridiag(1,2,1).

 1. exact answers on a diagonal matrix of powers of two;            2. coefficients against tests/quadrature_reference.py;
 3. the law of the generated probes;                                 4. a column is the column alone, past the wrap too;
 5. Gauss exactness on the device;                                   6. convergence of log and inverse under shifts, from ONE run;
 7. the trace itself, deterministically;                             8. option "symmetric_many";
 9. launch counts, refusals, lifetime, determinism;                 10. the driver's -Q."""
import os
import subprocess

import numpy as np
import pytest

import quadrature_data as D
import quadrature_reference as Q
from conftest import ROOT, PKG_NAME

pytestmark = pytest.mark.gpu

DTYPES = ("F64", "F32")
NP = {"F64": np.float64, "F32": np.float32}
EINVAL, ESTATE = -1, -6


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _assert_same_coefficients(got, want, what, rows=None):
    """alpha, beta, znorm2 and steps_run bit for bit (NaN entries past steps_run: the same canonical NaN on both sides)."""
    rows = slice(None) if rows is None else rows
    assert np.array_equal(got["steps_run"][rows], want["steps_run"][rows]), (what, got["steps_run"], want["steps_run"])
    for key in ("znorm2", "alpha", "beta"):
        g, w = _bits(got[key][rows]), _bits(want[key][rows])
        assert g.shape == w.shape and np.array_equal(g, w), (what, key, np.argwhere(g != w)[:6].tolist(), got[key][rows], want[key][rows])


# ------------------------------------------------------------------------------------------------
# 1. exact answers
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("n", [1, 7, 513, 1030, 4097])
def test_exact_answers_on_a_diagonal_matrix_of_powers_of_two(lam, dtype_name, n):
    """A = diag(2^e_i), probe j = 2^m_j e_(i_j): u = a_ii v, alpha_1 = a_ii, u - alpha_1 v = 0, so beta_1 = 0 and every probe stops at
    step 1 by the breakdown rule, every figure exact.  The quadrature is then znorm2 f(a_ii + s): its INV and POW values under
    power-of-two shifts are single correctly rounded operations on both sides.  nprobes = 11: two groups, the second at K = 4."""
    dt = NP[dtype_name]
    i = np.arange(n)
    a = 2.0 ** ((i % 7) - 3)
    steps = min(n, 3)
    shifts = np.array([0.0, 0.25, 2.0, 16.0])
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.set_matrix(np.diag(a))
        for nprobes in (1, 3, 8, 11):
            idx = (np.arange(nprobes) * 37 + 5) % n
            m = (np.arange(nprobes) % 5) - 2
            Z = np.zeros((nprobes, n), dt)
            Z[np.arange(nprobes), idx] = 2.0 ** m
            run = s.lanczos_many(Z, steps)
            what = (dtype_name, n, nprobes)
            assert (run["steps_run"] == 1).all(), (what, run["steps_run"])
            assert np.array_equal(run["alpha"][:, 0], a[idx]) and np.array_equal(run["znorm2"], 4.0 ** m), (what, run["alpha"][:, 0], run["znorm2"])
            assert not run["beta"][:, 0].any() and np.isnan(run["alpha"][:, 1:]).all() and np.isnan(run["beta"][:, 1:]).all(), what
            assert s.stats["num_iters"] == 1 and s.stats["converged"] == 1 and s.stats["rel_err"] == 0.0, s.stats
            assert s.get_option("multi_rhs_k") == {1: 1, 3: 4, 8: 8, 11: 4}[nprobes]
            _, _, inv = s.trace_quadrature("inv", shifts, per_probe=True)
            assert np.array_equal(inv, (4.0 ** m)[None, :] * (1.0 / (a[idx][None, :] + shifts[:, None]))), what
            for p in (0, 1, 2, 5):
                est, _, pw = s.trace_quadrature("pow", shifts, p, per_probe=True)
                want = (4.0 ** m)[None, :] * (a[idx][None, :] + shifts[:, None]) ** p
                assert np.array_equal(pw, want) and np.array_equal(est, D.mean_and_error(want)[0]), (what, p)
            _, _, lg = s.trace_quadrature("log", None, per_probe=True)
            # log is the one function here that is not a single correctly rounded operation: two libraries' logarithms, 2 ulp
            assert (np.abs(lg[0] - (4.0 ** m) * np.log(a[idx])) <= 2 * 2.0 ** -52 * np.abs((4.0 ** m) * np.log(a[idx]))).all(), what


# ------------------------------------------------------------------------------------------------
# 2. coefficients against the model
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("name", sorted(D.COEFF_SYSTEMS))
def test_coefficients_track_the_model(lam, name, dtype_name):
    """alpha_k and beta_k at k in {1, 2, 5, 20} of every device-generated Rademacher probe against the model in "rows" order, within
    10 x the model's own spread between its sum orders (tests/quadrature_data.py; tests/test_quadrature_cpu.py asserts that every
    one of these steps stays under lanczos_data.UNGATED_ABOVE, so all are gated)."""
    n, nprobes, seed = D.COEFF_SYSTEMS[name]
    ref = D.model_run(name, dtype_name, "rows")
    gate = D.COEFF_GATE[(name, dtype_name)]
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.set_matrix(D.system_matrix(name, dtype_name))
        run = s.lanczos_many(nprobes, D.COEFF_STEPS, seed)
    assert (run["steps_run"] == D.COEFF_STEPS).all() and np.array_equal(run["znorm2"], ref["znorm2"])
    worst = {}
    for k in D.COEFF_K:
        da = np.abs(run["alpha"][:, k - 1] / ref["alpha"][:, k - 1] - 1).max()
        db = np.abs(run["beta"][:, k - 1] / ref["beta"][:, k - 1] - 1).max()
        print(f"{name} {dtype_name} k={k}: alpha off by {da:.3e}, beta by {db:.3e} (gate {gate[k]:.1e})")
        worst[k] = max(da, db)
    for k in D.COEFF_K:
        assert worst[k] < gate[k], (name, dtype_name, k, worst)


# ------------------------------------------------------------------------------------------------
# 3. the law of the generated probes
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_generated_probes_follow_the_law(lam, dtype_name):
    """z_host = NULL with a seed against the same 11 probes built by the numpy law and passed from the host: identical bits in alpha,
    beta and znorm2 -- across the group boundary, where only the GLOBAL probe index gives probes 8..10 their law -- and
    znorm2 == N exactly."""
    n, nprobes, steps, seed = 1030, 11, 5, 0x5EED0000FFFFFFFF
    A = D.stored(np.diag(2.0 + np.arange(n) % 3) + np.diag(np.ones(n - 1), 1) + np.diag(np.ones(n - 1), -1), dtype_name)
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.set_matrix(A)
        dev = s.lanczos_many(nprobes, steps, seed)
        host = s.lanczos_many(Q.rademacher_probes(seed, nprobes, n, NP[dtype_name]), steps)
        other = s.lanczos_many(nprobes, steps, seed + 1)
    assert (dev["znorm2"] == float(n)).all() and (dev["steps_run"] == steps).all()
    _assert_same_coefficients(dev, host, dtype_name)
    assert len({dev["alpha"][j].tobytes() for j in range(nprobes)}) == nprobes
    assert not np.array_equal(dev["alpha"], other["alpha"])


# ------------------------------------------------------------------------------------------------
# 4. a column is the column alone
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_a_probe_of_a_group_is_the_probe_alone(lam, dtype_name):
    """n = 1030.  Rows 0 and 1 hold a block near the top of the dtype's range and are otherwise zero, rows 2 and 3 are diagonal, the
    rest is a tridiagonal SPD matrix.  Probe 1 = e_0 + e_1 overflows in its first product (alpha_1 = Inf, beta_1 = NaN: it stops at
    step 1, and the run reports not converged); probe 2 = e_2 breaks down at step 1 with exact figures; the other six live on rows
    >= 4.  Every probe run alone at K = 1 from the host gives the bits it gave in the group."""
    n, dt, steps = 1030, NP[dtype_name], 6
    big = 1.7e308 if dtype_name == "F64" else 3.3e38
    A = np.diag(2.0 + np.arange(n) % 3) + np.diag(np.ones(n - 1), 1) + np.diag(np.ones(n - 1), -1)
    A[:4, :] = 0.0
    A[:, :4] = 0.0
    A[0:2, 0:2] = big
    A[2, 2], A[3, 3] = 4.0, 8.0
    Z = np.random.default_rng(n).uniform(-1, 1, (8, n)).astype(dt)
    Z[:, :4] = 0
    Z[1] = 0
    Z[1, :2] = 1
    Z[2] = 0
    Z[2, 2] = 0.5
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.set_matrix(A)
        group = s.lanczos_many(Z, steps)
        assert s.stats["converged"] == 0 and s.stats["num_iters"] == steps
        assert list(group["steps_run"]) == [steps, 1, 1] + [steps] * 5, group["steps_run"]
        assert group["alpha"][1, 0] == np.inf and np.isnan(group["beta"][1, 0])
        assert group["alpha"][2, 0] == 4.0 and group["beta"][2, 0] == 0.0 and group["znorm2"][2] == 0.25
        assert np.isfinite(group["alpha"][[0, 3, 4, 5, 6, 7]]).all() and np.isfinite(group["beta"][[0, 3, 4, 5, 6, 7]]).all()
        for j in range(8):
            alone = s.lanczos_many(Z[j], steps)
            assert s.get_option("multi_rhs_k") == 1
            if j == 1:
                assert alone["steps_run"][0] == 1 and alone["alpha"][0, 0] == np.inf and np.isnan(alone["beta"][0, 0])
                continue
            _assert_same_coefficients({k: v[j:j + 1] for k, v in group.items() if k != "stats"}, alone, (dtype_name, j))
        # the quadrature refuses the run because of probe 1, and says so
        with pytest.raises(lam.LamHipError) as e:
            s.lanczos_many(Z, steps)
            s.trace_quadrature("inv")
        assert e.value.code == EINVAL and "probe 1 " in str(e.value), e.value


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_a_probe_of_a_group_is_the_probe_alone_past_the_wrap(lam, dtype_name):
    """n = 65537 > 256 workgroups x 256 threads on the device-filled tridiag(1,2,1), 3 steps: every thread of the vector kernels takes a
    second element.  Probes 0, 3 and 7 of a group of 8 alone at K = 1 give the group's bits.  alpha_1 = z^T A z / z^T z of the +-1
    probes is a ratio of two integers.  On the device every |v_i| is the ONE value c = fl(1 / sqrt(N)) = (1 + d) / sqrt(N), |d| <= u_TV:
    that is a factor (1 + d)^2 on alpha_1, 3 u_TV.  A row of A v adds c, 2c and c with signs: every partial sum is a small multiple
    of c, and only 3c can be inexact, so an element is off by at most 3 c u_TV from that and 4 c u_TV from the rounding of what
    follows: 7 c u_TV against v_i = c in N terms is 7 u_TV absolute, 8 u_TV / alpha_1 relative with room.  The fp64 sum of the N
    products, each at most 4 / N, against a total of alpha_1: (N + 2) 2^-53 (4 / alpha_1)."""
    n, dt, steps = 65537, NP[dtype_name], 3
    Z = Q.rademacher_probes(n, 8, n, dt)
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.generate_matrix(n)
        group = s.lanczos_many(Z, steps)
        assert (group["steps_run"] == steps).all() and (group["znorm2"] == float(n)).all()
        z64 = Z.astype(np.float64)
        exact = (2.0 * n + 2.0 * (z64[:, 1:] * z64[:, :-1]).sum(axis=1)) / n
        u = 2.0 ** -53 if dtype_name == "F64" else 2.0 ** -24
        bound = 3 * u + 8 * u / exact + (n + 2) * 2.0 ** -53 * 4.0 / exact
        assert (np.abs(group["alpha"][:, 0] / exact - 1) <= bound).all(), (group["alpha"][:, 0], exact, bound)
        for j in (0, 3, 7):
            alone = s.lanczos_many(Z[j], steps)
            _assert_same_coefficients({k: v[j:j + 1] for k, v in group.items() if k != "stats"}, alone, (dtype_name, j))


# ------------------------------------------------------------------------------------------------
# 5. moments on the device
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_six_device_steps_integrate_eleven_powers(lam, dtype_name):
    """m = 6 on the tracking system, POW p = 0 .. 11 against z^T A^p z from eigh of the stored matrix, within 10 x the model's own worst
    error; p = 12 misses, as it must."""
    A, Z = D.system_matrix("tracking", dtype_name), D.system_probes("tracking", dtype_name)
    n, nprobes, seed = D.COEFF_SYSTEMS["tracking"]
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.set_matrix(A)
        s.lanczos_many(nprobes, D.MOMENT_STEPS, seed)
        err = {}
        for p in D.MOMENT_EXACT_P + (D.MOMENT_MISS_P,):
            _, _, per = s.trace_quadrature("pow", None, p, per_probe=True)
            err[p] = float(np.abs(per[0] / Q.exact_forms(A, Z, Q.POW, (0.0,), p)[0] - 1).max())
    print(dtype_name, {p: f"{v:.2e}" for p, v in err.items()})
    assert all(err[p] < D.MOMENT_GATE[dtype_name] for p in D.MOMENT_EXACT_P), err
    assert err[D.MOMENT_MISS_P] >= D.MOMENT_MISS_AT_LEAST, err


# ------------------------------------------------------------------------------------------------
# 6. convergence, every shift from one run
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_log_and_inverse_converge_under_shifts_from_one_run(lam, dtype_name):
    """Per-probe LOG and INV quadratures on the tracking system under the shifts (0, 0.5, 2.0) against z^T f(A + s I) z from eigh, 100
    steps fp64 / 60 fp32, within 10 x the model's own worst error.  All three shifts come from ONE run: shifts in force on the batch
    are ignored, so a run made after set_shifts gives the same coefficient bits."""
    A, Z = D.system_matrix("tracking", dtype_name), D.system_probes("tracking", dtype_name)
    n, nprobes, seed = D.COEFF_SYSTEMS["tracking"]
    steps = D.CONV_STEPS[dtype_name]
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.set_matrix(A)
        run = s.lanczos_many(nprobes, steps, seed)
        for fn, name in ((Q.LOG, "log"), (Q.INV, "inv")):
            est, se, per = s.trace_quadrature(name, D.CONV_SHIFTS, per_probe=True)
            exact = Q.exact_forms(A, Z, fn, D.CONV_SHIFTS)
            err = float(np.abs(per / exact - 1).max())
            print(f"{dtype_name} {name}: worst per-probe error {err:.3e} (gate {D.CONV_GATE[dtype_name][fn]:.1e}); estimate {est}, std_error {se}")
            assert err < D.CONV_GATE[dtype_name][fn], (dtype_name, name, err)
            # the estimate is the trace's to within a few standard errors (8 probes: a sanity check of the estimator, 6 sigma)
            lam_A = np.linalg.eigvalsh(A)
            tr = np.array([Q.apply_fn(fn, lam_A + sh).sum() for sh in D.CONV_SHIFTS])
            assert (np.abs(est - tr) < 6 * se).all(), (est, tr, se)
        s.set_rhs_many(Z[:2])
        s.set_shifts([0.5, 2.0])
        again = s.lanczos_many(nprobes, steps, seed)
        _assert_same_coefficients(again, run, "under shifts in force")
        assert s.get_option("multi_rhs_k") == 8


# ------------------------------------------------------------------------------------------------
# 7. the trace itself, deterministically
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_the_trace_from_the_unit_vectors(lam, dtype_name):
    """N = 64, the 64 host probes 8 e_i (8 groups), 64 steps: the mean of z^T f(A + s I) z over them IS tr f(A + s I), so `estimate`
    equals log det(A + s I) and tr (A + s I)^-1 from eigh within 10 x the model's own error.  std_error and estimate agree exactly
    with numpy on the per-probe values, summed in the same order; one probe gives a NaN std_error."""
    A, Z = D.trace_matrix(dtype_name), D.trace_probes(dtype_name)
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.set_matrix(A)
        run = s.lanczos_many(Z, D.TRACE_N)
        assert (run["znorm2"] == 64.0).all() and s.stats["converged"] == 1
        for fn, name in ((Q.LOG, "log"), (Q.INV, "inv")):
            est, se, per = s.trace_quadrature(name, D.TRACE_SHIFTS, per_probe=True)
            exact = D.trace_exact(dtype_name, fn)
            err = float((np.abs(est - exact) / D.trace_scale(fn, exact)).max())
            print(f"{dtype_name} {name}: estimate {est}, exact {exact}, error {err:.3e} (gate {D.TRACE_GATE[dtype_name][fn]:.1e})")
            assert err < D.TRACE_GATE[dtype_name][fn], (dtype_name, name, err)
            want_est, want_se = D.mean_and_error(per)
            assert np.array_equal(_bits(est), _bits(want_est)) and np.array_equal(_bits(se), _bits(want_se)), (est, want_est, se, want_se)
            est2, se2 = s.trace_quadrature(name, D.TRACE_SHIFTS)
            assert np.array_equal(est2, est) and np.array_equal(se2, se)
        s.lanczos_many(Z[5], D.TRACE_N)
        est, se, per = s.trace_quadrature("log", D.TRACE_SHIFTS, per_probe=True)
        assert per.shape == (3, 1) and np.array_equal(est, per[:, 0]) and np.isnan(se).all()


# ------------------------------------------------------------------------------------------------
# 8. option "symmetric_many"
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_symmetric_many_runs_groups_of_four(lam, dtype_name):
    """symmetric_many = 2: the 8 probes of the tracking system run as two groups of 4 on the symmetric batched product
    ("symmetric_many_effective" == 1, "multi_rhs_k" == 4), and alpha_k, beta_k agree with the general product's within the gates of
    section 2 -- the two products differ in the order of their sums, which is what those gates measure."""
    n, nprobes, seed = D.COEFF_SYSTEMS["tracking"]
    gate = D.COEFF_GATE[("tracking", dtype_name)]
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.set_matrix(D.system_matrix("tracking", dtype_name))
        gen = s.lanczos_many(nprobes, D.COEFF_STEPS, seed)
        assert s.get_option("symmetric_many_effective") == 0 and s.get_option("multi_rhs_k") == 8
        s.set_option("symmetric_many", 2)
        l0 = s.get_option("hip_calls_launch")
        sym = s.lanczos_many(nprobes, D.COEFF_STEPS, seed)
        assert s.get_option("hip_calls_launch") - l0 == 2 * D.COEFF_STEPS * 4
        assert s.get_option("symmetric_many_effective") == 1 and s.get_option("multi_rhs_k") == 4
    assert (sym["steps_run"] == D.COEFF_STEPS).all() and np.array_equal(sym["znorm2"], gen["znorm2"])
    for k in D.COEFF_K:
        d = max(np.abs(sym["alpha"][:, k - 1] / gen["alpha"][:, k - 1] - 1).max(), np.abs(sym["beta"][:, k - 1] / gen["beta"][:, k - 1] - 1).max())
        print(f"{dtype_name} k={k}: symmetric against general {d:.3e} (gate {gate[k]:.1e})")
        assert d < gate[k], (dtype_name, k, d)


# ------------------------------------------------------------------------------------------------
# 9. launch counts, refusals, lifetime, determinism
# ------------------------------------------------------------------------------------------------
def test_launch_counts_and_determinism(lam):
    """3 launches per step and group -- 11 probes are the groups 8 + 3, 5 steps: 30 --, 4 under the symmetric product, whose groups are
    4 + 4 + 3: 60.  No probe of this system breaks down, so no launch past the last step is enqueued.  Two identical calls give
    identical bits."""
    A = D.system_matrix("tracking", "F64")
    with lam.Solver(lam.F64) as s:
        s.set_matrix(A)
        l0 = s.get_option("hip_calls_launch")
        a = s.lanczos_many(11, 5, 3)
        assert s.get_option("hip_calls_launch") - l0 == 2 * 5 * 3
        assert s.get_option("multi_rhs_k") == 4
        l0 = s.get_option("hip_calls_launch")
        b = s.lanczos_many(11, 5, 3)
        assert s.get_option("hip_calls_launch") - l0 == 30
        _assert_same_coefficients(a, b, "two identical calls")
        _assert_same_coefficients(s.lanczos_many_coefficients(), a, "lam_hip_get_lanczos_many")
        part = s.lanczos_many_coefficients(4)
        assert part["alpha"].shape == (4, 5) and np.array_equal(part["alpha"], a["alpha"][:4])
        s.set_option("symmetric_many", 2)
        l0 = s.get_option("hip_calls_launch")
        s.lanczos_many(11, 5, 3)
        assert s.get_option("hip_calls_launch") - l0 == 3 * 5 * 4
        # the host arithmetic launches nothing
        l0 = s.get_option("hip_calls_launch")
        s.trace_quadrature("log", [0.0, 1.0])
        assert s.get_option("hip_calls_launch") == l0


def test_refusals_and_lifetime(lam, monkeypatch):
    n = 384
    A = D.system_matrix("tracking", "F64")
    B = np.random.default_rng(9).uniform(-1, 1, (2, n))

    def refused(s, code, fn, *args, **kw):
        launches = s.get_option("hip_calls_launch")
        with pytest.raises(lam.LamHipError) as e:
            fn(*args, **kw)
        assert e.value.code == code, (fn, e.value)
        assert s.get_option("hip_calls_launch") == launches
        return str(e.value)

    with lam.Solver(lam.F64, device_ids=[0, 0]) as s:
        s.set_matrix(A)
        assert "shard" in refused(s, EINVAL, s.lanczos_many, 2, 5)
        assert "shard" in refused(s, EINVAL, s.trace_quadrature, "log")
    with lam.Solver(lam.BF16) as s:
        s.set_matrix(A)
        assert "BF16" in refused(s, EINVAL, s.lanczos_many, 2, 5)
    monkeypatch.setenv("LAM_HIP_FORCE_RCCL", "1")      # a one-rank communicator: the rank mode on one GPU
    with lam.Solver(lam.F64, rank=0, nranks=1, device_id=0, unique_id=None) as s:
        monkeypatch.delenv("LAM_HIP_FORCE_RCCL")
        s.set_problem(n)
        s.upload_rows(0, A)
        assert "rank mode" in refused(s, EINVAL, s.lanczos_many, 2, 5)
    with lam.Solver(lam.F64) as s:
        s.n = n
        refused(s, ESTATE, s.lanczos_many, 2, 5)                                   # no problem yet
        refused(s, ESTATE, s.trace_quadrature, "log")
        s.set_problem(n)
        assert "matrix" in refused(s, ESTATE, s.lanczos_many, 2, 5)                # no matrix yet
        s.set_matrix(A)
        refused(s, ESTATE, s.trace_quadrature, "log")                              # no coefficients yet
        refused(s, ESTATE, s.lanczos_many_coefficients, 1)
        for bad in (0, -1, 65):
            assert f"nprobes = {bad}," in refused(s, EINVAL, s.lanczos_many, bad, 5)
        for bad in (0, -3, 257):
            assert f"steps = {bad}," in refused(s, EINVAL, s.lanczos_many, 2, bad)
        Z = np.random.default_rng(1).uniform(-1, 1, (3, n))
        Z[1] = 0
        assert "probe 1 " in refused(s, EINVAL, s.lanczos_many, Z, 5)
        Z[1] = 1
        Z[2, 7] = np.nan
        assert "probe 2 " in refused(s, EINVAL, s.lanczos_many, Z, 5)
        Z[2, 7] = np.inf
        assert "probe 2 " in refused(s, EINVAL, s.lanczos_many, Z, 5)
        assert s._L.lam_hip_lanczos_many(None, 1, None, 0, 1, None, None, None, None, None) == EINVAL
    with lam.Solver(lam.F64) as s:                                                 # steps is capped by N as well
        s.set_matrix(np.diag([1.0, 2.0, 4.0]))
        assert "steps = 4," in refused(s, EINVAL, s.lanczos_many, 1, 4)
        s.lanczos_many(1, 3)

    with lam.Solver(lam.F64) as s:
        s.set_matrix(A)
        # what must be left alone: B and its shifts, the deflation space, the eigen-solution, the single-vector state
        b1 = np.random.default_rng(1).uniform(-1, 1, n)
        s.set_rhs(b1)
        s.solve(200, 1e-10)
        x1 = s.solution()
        eig = s.eigs(2, "largest", max_steps=40)
        Y = s.eigenvectors()
        s.set_deflation_from_eigs(2)
        s.set_rhs_many(B)
        s.set_shifts([0.5, 2.0])
        s.solve_many(30, 1e-9)
        X = s.solutions()
        it = s.num_iters_many.copy()
        run = s.lanczos_many(3, 10, 1)
        # a batched solution is no longer readable, exactly as after gemv_many
        refused(s, ESTATE, s.solutions)
        assert s.get_option("multi_rhs_k") == 4 and s.get_option("deflation_m") == 2
        assert np.array_equal(s.eigenvectors(), Y) and np.array_equal(s.solution(), x1)
        s.solve_many(30, 1e-9)                                                     # B and the shifts are what they were
        assert np.array_equal(s.solutions(), X) and np.array_equal(s.num_iters_many, it)
        s.set_shifts(None)
        s.solve_deflated(30, 1e-9)                                                 # the deflation space is still the matrix's
        # the coefficients are host data: they survive every batch call
        _assert_same_coefficients(s.lanczos_many_coefficients(), run, "after solve_many")
        est = s.trace_quadrature("log", [0.0, 0.5])
        # refusals of the quadrature leave them readable
        msg = refused(s, EINVAL, s.trace_quadrature, "log", [0.0, -100.0])
        assert "probe 0," in msg and "shift 1 (-100)" in msg and "node 0 " in msg, msg
        assert "fn = 3," in refused(s, EINVAL, s.trace_quadrature, 3)
        assert "param = 2.5," in refused(s, EINVAL, s.trace_quadrature, "pow", None, 2.5)
        assert "param = -1," in refused(s, EINVAL, s.trace_quadrature, "pow", None, -1)
        assert "nshifts = 65," in refused(s, EINVAL, s.trace_quadrature, "log", np.zeros(65))
        assert "nprobes = 4," in refused(s, EINVAL, s.lanczos_many_coefficients, 4)
        again = s.trace_quadrature("log", [0.0, 0.5])
        assert np.array_equal(again[0], est[0]) and np.array_equal(again[1], est[1])
        # logdet is lanczos_many + trace_quadrature
        ld = s.logdet([0.0, 0.5], nprobes=3, steps=10, seed=1)
        assert np.array_equal(ld[0], est[0]) and np.array_equal(ld[1], est[1])
        # they die with a new matrix content and with set_problem
        s.upload_rows(0, A[:1])
        refused(s, ESTATE, s.trace_quadrature, "log")
        s.lanczos_many(3, 10, 1)
        s.trace_quadrature("log")
        s.set_problem(n)
        refused(s, ESTATE, s.trace_quadrature, "log")
        refused(s, ESTATE, s.lanczos_many_coefficients, 1)


# ------------------------------------------------------------------------------------------------
# 10. driver
# ------------------------------------------------------------------------------------------------
def test_driver_quadrature(lam):
    """tridiag(1,2,1), n = 1024, -Q 8 -i 40 -S 0.5,2: one CSV line per shift -- shift, log det estimate, standard error, tr inverse
    estimate, standard error, steps, seconds -- whose figures are the Python call's for the same seed (the driver's is 0), to
    the 17 digits the driver prints."""
    exe = os.path.join(ROOT, PKG_NAME, "test", "test_CG_multi_rhs.out")
    n, steps, seed = 1024, 40, 0
    r = subprocess.run([exe, "-s", str(n), "-Q", "8", "-i", str(steps), "-S", "0.5,2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln.split(",") for ln in r.stdout.strip().splitlines()]
    assert len(lines) == 2 and all(len(ln) == 7 for ln in lines), r.stdout
    with lam.Solver(lam.F64) as s:
        s.generate_matrix(n)
        s.lanczos_many(8, steps, seed)
        ld, inv = s.trace_quadrature("log", [0.5, 2.0]), s.trace_quadrature("inv", [0.5, 2.0])
    for q, ln in enumerate(lines):
        got = [float(x) for x in ln]
        assert got[0] == (0.5, 2.0)[q] and int(ln[5]) == steps and got[6] > 0, ln
        for g, w in zip(got[1:5], (ld[0][q], ld[1][q], inv[0][q], inv[1][q])):
            assert abs(g / w - 1) < 1e-14, (ln, w)
    # combinations with the solve flags are refused with a message
    for extra in (["-m"], ["-J"], ["-T"], ["-k", "2"], ["-M"], ["-B"], ["-E", "2"], ["-D", "2"], ["-w", "3"], ["-e", "1e-6"]):
        r = subprocess.run([exe, "-s", "64", "-Q", "2", "-i", "5"] + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "-Q" in r.stderr, (extra, r.stdout, r.stderr)
