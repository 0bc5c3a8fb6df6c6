"""lam_hip_eigs on the device: Lanczos with full reorthogonalisation around the batch's K = 1 product launch, held to the numpy model
tests/lanczos_reference.py and to fp64 numpy on the downloaded matrix.  Systems, gates and step caps: tests/lanczos_data.py, established
without a GPU by tests/test_lanczos_cpu.py."""
import functools
import os
import subprocess

import numpy as np
import pytest

import generator_model as G
import lanczos_data as D
import lanczos_reference as L
from conftest import ROOT, PKG_NAME

pytestmark = pytest.mark.gpu

NP = D.DTYPES
U64 = 2.0 ** -53
EINVAL, ESTATE = -1, -6
WHICH = {"smallest": L.SMALLEST, "largest": L.LARGEST, "both": L.BOTH}


def u_tv(dtype_name):
    return L.UNIT_ROUNDOFF[NP[dtype_name]]


# ------------------------------------------------------------------------------------------------
# 1. project_out, exact
# ------------------------------------------------------------------------------------------------
def _integer_case(n, m, seed):
    """V[j] = +-1 where i % (j + 2) == 0 (overlapping strided supports), u in -3..3: every dot product, every coefficient and every
    partial sum of the update is an integer below 3 n (1/2 + ... + 1/(m + 1)) + 3 < 2^24."""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    V = np.array([np.where(i % (j + 2) == 0, rng.integers(0, 2, n) * 2 - 1, 0) for j in range(m)], dtype=np.int64)
    u = rng.integers(-3, 4, n).astype(np.int64)
    assert 3 * n * sum(1.0 / (j + 2) for j in range(m)) + 3 < 2 ** 24
    return V, u


@pytest.mark.parametrize("dtype_name", ["F64", "F32"])
@pytest.mark.parametrize("n,m", [(1, 1), (7, 3), (65, 8), (2049, 9), (2049, 65), (65537, 9), (65536 + 257, 9), (262144 + 4099, 3), (1048576 + 4099, 2)])
def test_project_out_is_exact_on_integers(lam, dtype_name, n, m):
    """The last two sizes are those at which a workgroup's slab no longer fits the registers of one round (2048 fp64 / 4096 fp32
    elements), ragged: 64 slabs of 4161 elements in the dots kernel, then 256 slabs of 4113 in the apply kernel as well.  m = 65 and 9
    deal the rows over the 16 workgroups of a slab unevenly, m = 2 and 3 leave most of them without a row."""
    V, u = _integer_case(n, m, 100 * n + m)
    want_c = V @ u
    want_u = u - V.T @ want_c
    with lam.Solver(getattr(lam, dtype_name)) as s:
        coeff, got = s.project_out(V, u)
    assert got.dtype == NP[dtype_name]
    assert np.array_equal(coeff, want_c.astype(np.float64)), np.flatnonzero(coeff != want_c)[:5]
    assert np.array_equal(got.astype(np.float64), want_u.astype(np.float64)), np.flatnonzero(got != want_u)[:5]


@pytest.mark.parametrize("dtype_name", ["F64", "F32"])
def test_project_out_confines_a_nan_to_its_column(lam, dtype_name):
    n, m, bad = 2049, 9, 4
    V, u = _integer_case(n, m, 5)
    Vn = V.astype(np.float64)
    Vn[bad, 2 * (bad + 2)] = np.nan
    with lam.Solver(getattr(lam, dtype_name)) as s:
        coeff, got = s.project_out(Vn, u)
    want_c = V @ u
    others = np.arange(m) != bad
    assert np.isnan(coeff[bad]) and np.isnan(got).any()
    assert np.array_equal(coeff[others], want_c[others].astype(np.float64))


def test_project_out_refuses_bad_arguments(lam):
    with lam.Solver(lam.F64) as s:
        with pytest.raises(lam.LamHipError) as e:
            s.project_out(np.zeros((lam.MAX_LANCZOS + 1, 4)), np.zeros(4))
        assert e.value.code == EINVAL and "LAM_HIP_MAX_LANCZOS" in str(e.value)


# ------------------------------------------------------------------------------------------------
# 2. coefficient parity
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[(n, d) for n in D.PARITY_SIZES for d in ("F64", "F32")], ids=lambda p: f"n{p[0]}-{p[1]}")
def parity(request, lam):
    """The device's parity system, its matrix downloaded, and the model's coefficients on that very matrix -- computed once."""
    n, dtype_name = request.param
    eig, V, v0 = D.parity_inputs(n)
    v0 = v0.astype(NP[dtype_name])
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.generate_spectrum_spd(eig, V)
        A = s.download_rows(0, n).astype(np.float64)
        model = D.coefficients(A, v0, NP[dtype_name], "rows")
        yield lam, s, n, dtype_name, v0, model


def test_coefficients_follow_the_model(parity):
    lam, s, n, dtype_name, v0, (alpha_m, beta_m) = parity
    out = s.eigs(1, "smallest", max_steps=D.PARITY_STEPS, tol=0.0, check_every=8, v0=v0)
    alpha, beta = s.lanczos_coefficients()
    assert out["steps"] == D.PARITY_STEPS and alpha.size == beta.size == D.PARITY_STEPS
    gate = D.COEFF_GATE[(n, dtype_name)]
    worst = {}
    for k in D.PARITY_K:
        da, db = abs(alpha[k - 1] / alpha_m[k - 1] - 1), abs(beta[k - 1] / beta_m[k - 1] - 1)
        worst[k] = (da, db)
        print(f"n={n} {dtype_name} k={k}: alpha off by {da:.2e}, beta by {db:.2e}; gate {gate[k]:.1e}")
    for k in D.PARITY_K:
        assert max(worst[k]) <= gate[k], (k, worst[k], gate[k])


def test_two_identical_calls_agree_bit_for_bit(parity):
    lam, s, n, dtype_name, v0, _ = parity
    runs = []
    for _ in range(2):
        out = s.eigs(3, "both", max_steps=24, tol=0.0, check_every=5, v0=v0)
        runs.append((out["theta"], out["bound"], *s.lanczos_coefficients(), s.eigenvectors(), s.eig_residuals()))
    for a, b in zip(*runs):
        assert np.array_equal(G.bits(a), G.bits(b))


def test_the_seeded_start_is_the_generator_models_vector(parity):
    lam, s, n, dtype_name, _, _ = parity
    seed = 77
    s.eigs(2, "largest", max_steps=12, tol=0.0, seed=seed)
    seeded = s.lanczos_coefficients()
    s.eigs(2, "largest", max_steps=12, tol=0.0, v0=G.stored_vector(G.random_rhs(n, seed), dtype_name))
    given = s.lanczos_coefficients()
    assert np.array_equal(seeded[0], given[0]) and np.array_equal(seeded[1], given[1])


# ------------------------------------------------------------------------------------------------
# 3. known spectrum
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["F64", "F32"])
def known(request, lam):
    dtype_name = request.param
    eig, V, v0 = D.known_inputs()
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.generate_spectrum_spd(eig, V)
        A = s.download_rows(0, D.KNOWN_N).astype(np.float64)
        yield lam, s, dtype_name, A, np.linalg.eigvalsh(A), v0.astype(NP[dtype_name])
        s.set_option("symmetric_many", 0)


@pytest.mark.parametrize("symmetric_many", [0, 2])
@pytest.mark.parametrize("which", ["smallest", "largest", "both"])
def test_known_spectrum(known, which, symmetric_many):
    lam, s, dtype_name, A, ev, v0 = known
    n, nev, u = D.KNOWN_N, D.KNOWN_NEV, u_tv(dtype_name)
    s.set_option("symmetric_many", symmetric_many)
    out = s.eigs(nev, which, max_steps=D.KNOWN_MAX_STEPS, tol=D.KNOWN_TOL[dtype_name], check_every=D.KNOWN_CHECK_EVERY, v0=v0)
    assert s.get_option("symmetric_many_effective") == (1 if symmetric_many else 0)
    assert s.get_option("multi_rhs_k") == 1
    model = D.known_run(dtype_name, WHICH[which])
    Y = s.eigenvectors().astype(np.float64)
    res = s.eig_residuals()
    norm = np.abs(ev).max()
    floor = D.residual_floor(n, dtype_name, norm)
    idx = L.wanted(WHICH[which], nev, n, nev)
    print(f"{dtype_name} {which} symmetric_many={symmetric_many}: steps {out['steps']} (model {model['steps']}), stats {out['stats']}")
    assert out["nfound"] == nev and out["converged"].all() and out["stats"]["converged"] == 1
    assert abs(out["steps"] - model["steps"]) <= D.KNOWN_CHECK_EVERY
    assert out["stats"]["rel_err"] <= D.KNOWN_TOL[dtype_name]
    for i in range(nev):
        theta, y = out["theta"][i], Y[i]
        rho = np.linalg.norm(A @ y - theta * y) / np.linalg.norm(y)
        print(f"  pair {i}: theta {theta:.15g} (true {ev[idx[i]]:.15g}) bound {out['bound'][i]:.2e} rho {rho:.2e} device residual {res[i]:.2e} "
              f"floor {floor:.2e}")
        assert np.abs(ev - theta).min() <= rho + n * U64 * norm
        assert abs(ev[idx[i]] - theta) <= rho + n * U64 * norm               # the i-th extreme eigenvalue, not just an eigenvalue
        if rho > floor:
            assert abs(res[i] - rho) <= 1e-3 * rho
        else:
            assert res[i] <= floor
        assert rho <= out["bound"][i] + floor
    k = out["steps"]
    gram = Y @ Y.T
    print(f"  |Y Y^T - I| {np.abs(gram - np.eye(nev)).max():.2e} (gate {64 * k * u:.2e})")
    assert np.abs(gram - np.eye(nev)).max() <= 64 * k * u


# ------------------------------------------------------------------------------------------------
# 4. analytic spectrum: the whole of tridiag(1, 2, 1), which no Lanczos without reorthogonalisation recovers
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", ["F64", "F32"])
def test_the_whole_spectrum_of_the_tridiagonal_matrix(lam, dtype_name):
    n = 255
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.generate_matrix(n)
        out = s.eigs(1, "smallest", max_steps=n, tol=0.0, check_every=64, seed=3)
        alpha, beta = s.lanczos_coefficients()
    assert out["steps"] == n, out
    theta, _ = lam.tridiag_eigen(alpha, beta)
    want = np.sort(2.0 + 2.0 * np.cos(np.arange(1, n + 1) * np.pi / (n + 1)))
    err = np.abs(theta - want).max()
    print(f"{dtype_name}: the {n} eigenvalues off by at most {err:.2e} (gate {16 * n * u_tv(dtype_name) * 4.0:.2e})")
    assert err <= 16 * n * u_tv(dtype_name) * 4.0


# ------------------------------------------------------------------------------------------------
# 5. breakdown
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", ["F64", "F32"])
def test_an_invariant_subspace_stops_the_run(lam, dtype_name):
    n = 65
    v0 = np.zeros(n)
    v0[:3] = 1.0
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.set_matrix(np.diag(np.arange(1.0, n + 1)))
        out = s.eigs(4, "smallest", max_steps=32, tol=1e-10, check_every=8, v0=v0)
        Y = s.eigenvectors()
        alpha, beta = s.lanczos_coefficients()
        res = s.eig_residuals()
    print(f"{dtype_name}: {out}, beta {beta}")
    assert out["steps"] == 3 and out["nfound"] == 3 and alpha.size == 3
    assert np.abs(out["theta"][:3] - [1, 2, 3]).max() <= 64 * u_tv(dtype_name) * 3
    assert np.isnan(out["theta"][3]) and np.isnan(out["bound"][3]) and not out["converged"][3]
    assert out["converged"][:3].all() and out["stats"]["converged"] == 0
    assert Y.shape == (3, n) and np.isfinite(Y).all() and np.isfinite(alpha).all() and np.isfinite(beta).all() and np.isfinite(res).all()
    assert np.abs(Y[:, 3:]).max() <= 64 * u_tv(dtype_name)             # the Ritz vectors live in span(e_1, e_2, e_3)


# ------------------------------------------------------------------------------------------------
# 6. refusals and lifetime
# ------------------------------------------------------------------------------------------------
def _refused(lam, code, call, *args, **kw):
    with pytest.raises(lam.LamHipError) as e:
        call(*args, **kw)
    assert e.value.code == code, e.value
    return str(e.value)


def test_refusals(lam, monkeypatch):
    n = 48
    A = G.random_spd(n, 1, 10.0)
    with lam.Solver(lam.F64, device_ids=[0, 0]) as s:
        s.set_matrix(A)
        assert "shards: the multi-right-hand-side path supports one shard only" in _refused(lam, EINVAL, s.eigs, 2, max_steps=8)
    with lam.Solver(lam.BF16) as s:
        s.set_matrix(A)
        assert "LAM_HIP_BF16 storage is not supported" in _refused(lam, EINVAL, s.eigs, 2, max_steps=8, tol=1e-3)
    monkeypatch.setenv("LAM_HIP_FORCE_RCCL", "1")      # a one-rank communicator: the rank mode on one GPU
    with lam.Solver(lam.F64, rank=0, nranks=1, device_id=0, unique_id=None) as s:
        monkeypatch.delenv("LAM_HIP_FORCE_RCCL")
        s.set_problem(n)
        s.upload_rows(0, A)
        assert "rank mode" in _refused(lam, EINVAL, s.eigs, 2, max_steps=8)
    with lam.Solver(lam.F64) as s:
        s.n = n
        _refused(lam, ESTATE, s.eigs, 2, max_steps=8)                      # no problem
        s.set_problem(n)
        assert "matrix" in _refused(lam, ESTATE, s.eigs, 2, max_steps=8)    # no matrix
        _refused(lam, ESTATE, s.lanczos_coefficients)
        s.upload_rows(0, A)
        assert "nev = 0" in _refused(lam, EINVAL, s.eigs, 0, max_steps=8)
        assert "nev = 9" in _refused(lam, EINVAL, s.eigs, 9, max_steps=8)
        assert "max_steps = 0" in _refused(lam, EINVAL, s.eigs, 1, max_steps=0)
        assert f"max_steps = {n + 1}" in _refused(lam, EINVAL, s.eigs, 1, max_steps=n + 1)
        assert "which = 3" in _refused(lam, EINVAL, s.eigs, 1, which=3, max_steps=8)
        assert "check_every = 0" in _refused(lam, EINVAL, s.eigs, 1, max_steps=8, check_every=0)
        assert "start vector" in _refused(lam, EINVAL, s.eigs, 1, max_steps=8, v0=np.zeros(n))
        v = np.ones(n)
        v[5] = np.inf
        assert "start vector" in _refused(lam, EINVAL, s.eigs, 1, max_steps=8, v0=v)
        s.nfound = 1
        _refused(lam, ESTATE, s.eigenvectors)                              # none of the refused calls left an eigen-solution
    with lam.Solver(lam.F64) as s:                                          # N beyond the limit: min(N, LAM_HIP_MAX_LANCZOS)
        s.generate_matrix(300)
        assert "max_steps = 257" in _refused(lam, EINVAL, s.eigs, 1, max_steps=257)


@pytest.mark.parametrize("dtype_name", ["F64", "F32"])
def test_lifetime_next_to_the_batch_and_the_single_solve(lam, dtype_name):
    n = 130
    rng = np.random.default_rng(9)
    B = rng.uniform(-1, 1, (3, n)).astype(NP[dtype_name])
    shifts = [0.0, 0.5, 2.0]
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.generate_random_spd(n, 5, 100.0)
        s.set_rhs_many(B)
        s.set_shifts(shifts)
        s.solve_many(40, 1e-6)
        X = s.solutions()
        iters = s.num_iters_many.copy()
        s.generate_random_rhs(4)
        s.solve(200, 1e-6)
        x1 = s.solution()
        # the eigen-solve: the batched solution is gone, B and the shifts are not, the single-vector state is untouched
        out = s.eigs(2, "both", max_steps=16, tol=0.0)
        y16 = s.eigenvectors()
        assert out["steps"] == 16
        _refused(lam, ESTATE, s.solutions)
        _refused(lam, ESTATE, s.true_residuals)
        assert np.array_equal(s.solution(), x1)
        s.solve_many(40, 1e-6)
        assert np.array_equal(G.bits(s.solutions()), G.bits(X)) and np.array_equal(s.num_iters_many, iters)
        # the batch and the single solve leave the eigen-solution readable ...
        s.solve(200, 1e-6)
        assert np.array_equal(s.solution(), x1)
        assert np.array_equal(G.bits(s.eigenvectors()), G.bits(y16))
        s.eig_residuals()
        assert np.array_equal(G.bits(s.solutions()), G.bits(X))             # ... and the residuals leave the batched solution
        # growing max_steps between calls re-allocates and agrees with a fresh context's run on the steps they share
        out = s.eigs(2, "both", max_steps=40, tol=0.0)
        a40, b40 = s.lanczos_coefficients()
        assert out["steps"] == 40
        s.eigs(2, "both", max_steps=16, tol=0.0)
        a16, b16 = s.lanczos_coefficients()
        assert np.array_equal(a16, a40[:16]) and np.array_equal(b16, b40[:16])
        assert np.array_equal(G.bits(s.eigenvectors()), G.bits(y16))
        # set_problem and a new matrix invalidate it
        s.generate_random_spd(n, 6, 100.0, keep_problem=True)
        _refused(lam, ESTATE, s.eigenvectors)
        s.eigs(1, max_steps=8, tol=0.0)
        s.set_problem(n)
        _refused(lam, ESTATE, s.eig_residuals)
        _refused(lam, ESTATE, s.lanczos_coefficients)


# ------------------------------------------------------------------------------------------------
# 7. launch accounting
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("symmetric_many", [0, 2])
@pytest.mark.parametrize("dtype_name", ["F64", "F32"])
def test_a_step_is_a_fixed_number_of_launches(lam, dtype_name, symmetric_many):
    """include/lam_hip.h: 7 launches per step -- the product and six vector launches -- whatever k; 8 under symmetric_many."""
    per_step = 8 if symmetric_many else 7
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.generate_random_spd(130, 5, 1e4)
        s.set_option("symmetric_many", symmetric_many)
        for steps in (3, 11, 30):
            l0 = s.get_option("hip_calls_launch")
            out = s.eigs(1, max_steps=steps, tol=0.0, check_every=4)
            assert out["steps"] == steps
            assert s.get_option("hip_calls_launch") - l0 == per_step * steps


# ------------------------------------------------------------------------------------------------
# 8. driver
# ------------------------------------------------------------------------------------------------
EXE = os.path.join(ROOT, PKG_NAME, "test", "test_CG_multi_rhs.out")


def _run(*args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, timeout=300)


def test_driver_prints_the_bindings_eigenvalues(lam):
    n = 384
    r = _run("-s", n, "-E", 4, "-W", "b", "-i", 200, "-e", 1e-9)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [ln.split(",") for ln in r.stdout.strip().splitlines()]
    assert len(rows) == 4 and all(len(f) == 11 for f in rows)
    with lam.Solver(lam.F64) as s:
        s.generate_matrix(n)
        out = s.eigs(4, "both", max_steps=200, tol=1e-9, check_every=8, seed=0)
        res = s.eig_residuals()
    for i, f in enumerate(rows):
        assert int(f[0]) == i and float(f[1]) == out["theta"][i] and float(f[2]) == out["bound"][i] and float(f[3]) == res[i]
        assert int(f[4]) == int(out["converged"][i]) and int(f[5]) == out["steps"]


@pytest.mark.parametrize("extra", [["-J"], ["-w", "3"], ["-S", "0.5"], ["-S", "0.5", "-M"], ["-m"], ["-k", "2"], ["-W", "x"], ["-E", "0"]])
def test_driver_refuses_conflicting_flags(extra):
    r = _run("-s", 64, "-E", 2, *extra)
    assert r.returncode == 1 and "Usage" in r.stderr and r.stdout == "", (extra, r.stderr)
