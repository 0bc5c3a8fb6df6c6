"""The guard of the symmetric product: the asymmetry measurement (lam_hip_check_symmetry / asymmetry_kernel), the policy a context
applies when the product was asked for through LAM_HIP_SYMMETRIC (env_symmetric_check), and what bf16 storage holds.

The symmetric product reads the upper triangle only, so on a matrix with A != A^T it solves another system without any sign of it.
With the environment variable nobody calls lam_hip_check_symmetry: the library vouches for A = A^T itself.  A measurement that
comes out too small -- a tile skipped, a row read from the wrong shard, a NaN that drops out of a maximum -- or a tolerance that is
too wide lets an asymmetric matrix through; so the measurement is compared BIT FOR BIT with numpy on the matrix the device holds
(both compute fl64(u - l) of the same two numbers and take a maximum: no rounding freedom), and every outcome of the policy is
asserted for every storage type and every entry point that can run the product.  References are plain numpy in fp64."""
import numpy as np
import pytest

import symmetry_data as S
from conftest import slow
from test_gpu_exact import GATE

pytestmark = pytest.mark.gpu

DTYPES = ("F64", "F32", "BF16")
ENV = "LAM_HIP_SYMMETRIC"


def _dev64(s, row0=0, nrows=None):
    """Rows of the matrix the device holds, as fp64 (bf16 storage travels as fp32: every step is exact)."""
    return s.download_rows(row0, s.n if nrows is None else nrows).astype(np.float64)


def _host_asymmetry(A_dev):
    with np.errstate(invalid="ignore"):
        return np.max(np.abs(A_dev - A_dev.T))


# ------------------------------------------------------------------------------------------------
# A1. dense non-symmetric random data: the measurement equals numpy's, bit for bit
# ------------------------------------------------------------------------------------------------
# below one tile, the tile edges, a ragged last tile, a padded pitch; 1, 3, 7 and 33 shards (33 at n = 1000: 30 rows a shard, shorter
# than a tile; at n = 33 ... 65: one or two rows a shard); n = 1001 on 3 and n = 4099 on 5: the last shard holds remainder rows
DENSE_CASES = [(n, (1, 3, 7, 33)) for n in (1, 2, 31, 32, 33, 63, 64, 65, 1000, 1025, 4097)] + [(1001, (3,)), (4099, (5,))]


@pytest.mark.parametrize("dtype_name,n,shard_counts", [pytest.param(d, n, P, id=f"{d}-{n}-shards{'_'.join(map(str, P))}")
                                                      for d in DTYPES for n, P in DENSE_CASES])
def test_asymmetry_of_dense_random_matrix_is_exact(lam, dtype_name, n, shard_counts):
    A = np.random.default_rng(1000 + n).uniform(-1, 1, (n, n))
    counts = [P for P in shard_counts if P <= n]
    assert counts
    for P in counts:
        with lam.Solver(getattr(lam, dtype_name), device_ids=[0] * P) as s:
            s.set_matrix(A)
            want = _host_asymmetry(_dev64(s))
            # the maximum is far from zero, so agreement cannot be an accident
            assert want > 0.5 if n >= 31 else (want > 0 if n >= 2 else want == 0), (n, want)
            got = s.check_symmetry()
            print(f"{dtype_name} n={n} shards={P}: check_symmetry {got!r}, numpy {want!r}")
            assert got == want, f"{dtype_name} n={n} shards={P}: check_symmetry() = {got!r}, max|A_dev - A_dev^T| = {want!r}"


# ------------------------------------------------------------------------------------------------
# A2. a single planted entry on a bit-symmetric matrix: no other pair can hide a wrong answer
# ------------------------------------------------------------------------------------------------
# n = 65537: 2049 tile rows, about 2.1 million tiles -- the far end of the tile numbering (a float sqrt plus correction loops)
PLANTED_CASES = ([(d, n, P) for d in DTYPES for n in (1001, 4099) for P in (1, 5)]
                 + [(d, 65537, P) for d in ("F32", "BF16") for P in (1, 3)] + [slow("F64", 65537, P) for P in (1, 3)])


@pytest.mark.parametrize("dtype_name,n,P", PLANTED_CASES)
def test_asymmetry_of_single_planted_entry_is_exact(lam, dtype_name, n, P):
    """One entry moved by a power of two (0.25; for bf16 a step that keeps the entry a bf16 number, checked on the downloaded
    row), at (i, j) and at (j, i) for each position of symmetry_data.planted_positions: exactly |A_ij - A_ji| of the downloaded
    rows comes back, and exactly 0 after the row is restored."""
    with lam.Solver(getattr(lam, dtype_name), device_ids=[0] * P) as s:
        s.generate_random_spd(n, 5, 10.0)
        assert s.check_symmetry() == 0.0
        hdt = s.mat_host_dtype
        for i, j in S.planted_positions(n, P):
            row, other = s.download_rows(i, 1), s.download_rows(j, 1)
            assert row[0, j] == other[0, i]
            if dtype_name == "BF16":
                delta = S.bf16_exact_delta(row[0, j])
            else:
                delta = 0.25
            new = row.copy()
            new[0, j] = hdt(np.float64(row[0, j]) + delta)
            s.upload_rows(i, new)
            held = s.download_rows(i, 1)
            if dtype_name == "BF16":                     # the step is exact in bf16 at this entry's magnitude
                assert np.float64(held[0, j]) == np.float64(row[0, j]) + delta, (i, j, row[0, j], delta, held[0, j])
            assert np.array_equal(held, new)
            want = abs(np.float64(held[0, j]) - np.float64(other[0, i]))
            assert want > 0
            got = s.check_symmetry()
            assert got == want, f"{dtype_name} n={n} shards={P}: entry ({i}, {j}) moved by {delta}: check_symmetry() = {got!r}, expected {want!r}"
            s.upload_rows(i, row)
            got = s.check_symmetry()
            assert got == 0.0, f"{dtype_name} n={n} shards={P}: entry ({i}, {j}) restored: check_symmetry() = {got!r}"


# ------------------------------------------------------------------------------------------------
# B. the environment path: every storage type, every entry point
# ------------------------------------------------------------------------------------------------
def _sym_uniform(n, seed):
    R = np.random.default_rng(seed).uniform(-1, 1, (n, n))
    return 0.5 * (R + R.T)


def _bf16_neighbour(v):
    """The bf16 value next to the bf16 value v (as fp32), away from zero: one unit in bf16's last place."""
    u = np.array([v], dtype=np.float32).view(np.uint32)
    assert u[0] & 0xFFFF == 0 and 0 < (u[0] & 0x7FFFFFFF) < 0x7F000000
    return (u + np.uint32(0x10000)).view(np.float32)[0]


def _general(name):
    return "symv" not in name


def test_bf16_outcomes_of_the_environment_check(lam, monkeypatch, capfd):
    """bf16 storage rounds each side of a pair separately from an fp32 file, so two entries that agree to fp32 rounding hold the
    same bf16 value or neighbours: bit-symmetric -> silent; one entry one bf16 ulp away -> a warning, the product runs; an
    off-diagonal entry changed by 0.1 max|A| -> refused, and the solve gives bit for bit what a context without the variable gives
    on the same uploaded matrix (the rule used to accept anything up to 0.5 max|A| for bf16)."""
    n = 1500
    monkeypatch.setenv(ENV, "2")
    with lam.Solver(lam.BF16) as s:
        assert s.get_option("symmetric") == 2
        s.generate_random_spd(n, 5, 100.0)
        s.generate_random_rhs(6)
        amax = np.max(np.abs(_dev64(s)))
        rows_ok = s.download_rows(7, 1)
        s.solve(30, 0.0)
        assert s.get_option("symmetric_effective") == 1
        assert ENV not in capfd.readouterr().err
        # one bf16 ulp
        rows = rows_ok.copy()
        rows[0, 100] = _bf16_neighbour(rows[0, 100])
        s.upload_rows(7, rows)
        assert np.array_equal(s.download_rows(7, 1), rows) and rows[0, 100] != rows_ok[0, 100]
        s.generate_random_rhs(6)
        s.solve(30, 0.0)
        err = capfd.readouterr().err
        assert s.get_option("symmetric_effective") == 1 and "equal to rounding only" in err, err
        # a tenth of the largest element
        rows = rows_ok.copy()
        rows[0, 100] += np.float32(0.1 * amax)
        s.upload_rows(7, rows)
        asym = s.check_symmetry()
        assert 0.09 * amax < asym < 0.11 * amax
        s.generate_random_rhs(6)
        s.solve(30, 0.0)
        err = capfd.readouterr().err
        assert s.get_option("symmetric_effective") == 0 and "refused" in err and "general GEMV" in err, err
        x_refused = s.solution()
    monkeypatch.delenv(ENV)
    with lam.Solver(lam.BF16) as s:
        s.generate_random_spd(n, 5, 100.0)
        s.upload_rows(7, rows)
        s.generate_random_rhs(6)
        s.solve(30, 0.0)
        assert np.array_equal(s.solution(), x_refused)


@pytest.mark.parametrize("shards", [1, 3])
def test_bf16_small_entry_is_judged_by_its_own_size(lam, monkeypatch, capfd, shards):
    """Uniform data (entries of every size below max|A|): an entry of 2^-12 ... 2^-6 of max|A| replaced by four times its value
    differs from its mirror image by 3 |A_ij| -- 96 times the pair's own term 2^-7 * 4 |A_ij|, and at least 192 times the absolute term
    64 * 2^-24 max|A| -- but by less than 0.05 max|A|: refused."""
    n = 1000
    A = _sym_uniform(n, 21)
    monkeypatch.setenv(ENV, "2")
    with lam.Solver(lam.BF16, device_ids=[0] * shards) as s:
        s.set_matrix(A)
        s.set_rhs(np.ones(n))
        A_dev = _dev64(s)
        assert np.array_equal(A_dev, A_dev.T)
        s.cg_init()
        assert s.get_option("symmetric_effective") == 1 and ENV not in capfd.readouterr().err
        amax = np.max(np.abs(A_dev))
        cand = np.argwhere((np.abs(A_dev) >= 2.0 ** -12 * amax) & (np.abs(A_dev) <= 2.0 ** -6 * amax) & ~np.eye(n, dtype=bool))
        assert len(cand) > 100
        i, j = (int(v) for v in cand[len(cand) // 2])
        row = s.download_rows(i, 1)
        row[0, j] *= 4                                          # exact in bf16
        s.upload_rows(i, row)
        assert s.check_symmetry() == 3 * abs(A_dev[i, j]) > 0
        s.cg_init()
        err = capfd.readouterr().err
        assert s.get_option("symmetric_effective") == 0 and "refused" in err, (i, j, A_dev[i, j], amax, err)


def _asymmetric_order_one(n, seed):
    """Symmetric uniform data with one pair set to (0.5, 0.75): exact in every storage type, asymmetry 0.25 on entries of order 1."""
    A = _sym_uniform(n, seed)
    i, j = n // 3, 2 * n // 3 + 1
    A[i, j], A[j, i] = 0.5, 0.75
    return A, i, j


def _products(A_dev, x64):
    """The fp64 product of the full matrix, the product the upper triangle defines, and the scale |A| |x| of the gate."""
    up = np.triu(A_dev) + np.triu(A_dev, 1).T
    return A_dev @ x64, up @ x64, np.abs(A_dev) @ np.abs(x64)


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_gemv_before_any_cg_init_is_guarded(lam, monkeypatch, capfd, dtype_name):
    """lam_hip_gemv and lam_hip_gemv_only branch on the symmetric product themselves: as the first operation after an upload they
    must apply the environment's check as lam_hip_cg_init does.  Asymmetric matrix: the full matrix's product, 'refused', a general
    kernel.  Symmetric matrix: silent, the symmetric kernel.  Several shards keep the general GEMV for lam_hip_gemv."""
    n = 1003
    dt = getattr(lam, dtype_name)
    A, i, j = _asymmetric_order_one(n, 33)
    x = np.random.default_rng(34).uniform(0.5, 1.0, n)
    monkeypatch.setenv(ENV, "2")
    with lam.Solver(dt) as s:
        s.set_matrix(A)
        xv = x.astype(s.vec_dtype)
        y = s.gemv(xv).astype(np.float64)                        # the first operation on this context
        err = capfd.readouterr().err
        A_dev = _dev64(s)
        assert A_dev[i, j] == 0.5 and A_dev[j, i] == 0.75
        full, upper, scale = _products(A_dev, xv.astype(np.float64))
        assert np.max(np.abs(y - full) / scale) <= GATE[dtype_name], (np.argmax(np.abs(y - full) / scale), y[j], full[j], upper[j])
        assert abs(full[j] - upper[j]) > 0.12 and abs(y[j] - upper[j]) > 0.1          # row j of the upper-triangle product reads 0.5
        assert "refused" in err and "general GEMV" in err, err
        assert _general(s.gemv_kernel_name()) and s.get_option("symmetric_effective") == 0
    with lam.Solver(dt) as s:
        s.set_matrix(A)
        s.gemv_only(1)
        err = capfd.readouterr().err
        assert s.get_option("symmetric_effective") == 0 and _general(s.gemv_kernel_name()) and "refused" in err, err
    A[j, i] = 0.5
    with lam.Solver(dt) as s:
        s.set_matrix(A)
        y = s.gemv(xv).astype(np.float64)
        full, upper, scale = _products(_dev64(s), xv.astype(np.float64))
        assert np.array_equal(full, upper) and np.max(np.abs(y - full) / scale) <= GATE[dtype_name]
        assert not _general(s.gemv_kernel_name()) and s.get_option("symmetric_effective") == 1
        s.gemv_only(1)
        assert not _general(s.gemv_kernel_name()) and s.get_option("symmetric_effective") == 1
        assert ENV not in capfd.readouterr().err
    A[j, i] = 0.75
    with lam.Solver(dt, device_ids=[0, 0, 0]) as s:
        s.set_matrix(A)
        y = s.gemv(xv).astype(np.float64)
        full, upper, scale = _products(_dev64(s), xv.astype(np.float64))
        assert np.max(np.abs(y - full) / scale) <= GATE[dtype_name] and abs(y[j] - upper[j]) > 0.1
        assert _general(s.gemv_kernel_name())


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_explicit_option_after_a_refusal_takes_over(lam, monkeypatch, capfd, dtype_name):
    """lam_hip_set_option("symmetric") is the caller vouching for A = A^T: after the environment's check refused a matrix it makes
    the product effective again, without a check or a message, the answer is the upper triangle's, and a later upload does not
    bring the environment's check back for this context."""
    n = 1003
    A, i, j = _asymmetric_order_one(n, 35)
    x = np.random.default_rng(36).uniform(0.5, 1.0, n)
    monkeypatch.setenv(ENV, "2")
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.set_matrix(A)
        s.set_rhs(np.ones(n))
        s.cg_init()
        assert s.get_option("symmetric_effective") == 0 and "refused" in capfd.readouterr().err
        s.set_option("symmetric", 2)
        assert s.get_option("symmetric_effective") == 1
        xv = x.astype(s.vec_dtype)
        full, upper, scale = _products(_dev64(s), xv.astype(np.float64))
        for again in (False, True):
            if again:
                s.upload_rows(0, A)
                assert s.get_option("symmetric_effective") == 1
            y = s.gemv(xv).astype(np.float64)
            assert np.max(np.abs(y - upper) / scale) <= GATE[dtype_name] and abs(y[j] - full[j]) > 0.1
            s.cg_init()
            assert s.get_option("symmetric_effective") == 1 and not _general(s.gemv_kernel_name())
        assert ENV not in capfd.readouterr().err


# (A_ij, A_ji, the environment's check refuses, check_symmetry's answer): a pair the two triangles disagree on is a violation whatever
# max|A| is; a pair they agree on -- equal infinities, two NaNs, zeros of either sign -- contributes nothing
NONFINITE_PAIRS = [
    ("one-sided NaN", np.nan, 0.5, True, np.inf),
    ("one-sided +Inf", np.inf, 0.5, True, np.inf),
    ("+Inf against -Inf", np.inf, -np.inf, True, np.inf),
    ("NaN against +Inf", np.nan, np.inf, True, np.inf),
    ("+Inf on both sides", np.inf, np.inf, False, 0.0),
    ("NaN on both sides", np.nan, np.nan, False, 0.0),
    ("+0 against -0", 0.0, -0.0, False, 0.0),
]


@pytest.mark.parametrize("shards", [1, 3])
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_nonfinite_entries_and_the_guard(lam, monkeypatch, capfd, dtype_name, shards):
    """Ordinary data that a maximum kept with `d > m ? d : m` gets wrong: a one-sided NaN drops out of it, a one-sided Inf is
    'within 64 ulp of max|A| = Inf'.  With the variable set each is refused and lam_hip_check_symmetry returns inf; equal
    non-finite pairs and signed zeros are accepted in silence.  Last: equal infinities elsewhere in the matrix must not widen the
    tolerance for a finite asymmetry (max|A| is taken over the finite entries)."""
    n = 300
    base = _sym_uniform(n, 41)
    monkeypatch.setenv(ENV, "2")
    cases = [(label, [(11, 250, u, l)], refused, want) for label, u, l, refused, want in NONFINITE_PAIRS]
    cases += [(label + ", mirrored", [(250, 11, u, l)], refused, want) for label, u, l, refused, want in NONFINITE_PAIRS[:2]]
    cases.append(("equal +Inf pair and a finite asymmetry of 0.25", [(3, 200, np.inf, np.inf), (20, 270, 0.5, 0.75)], True, 0.25))
    problems = []
    with lam.Solver(getattr(lam, dtype_name), device_ids=[0] * shards) as s:
        s.set_problem(n)
        for label, pairs, refused, want in cases:
            A = base.copy()
            for i, j, u, l in pairs:
                A[i, j], A[j, i] = u, l
            s.upload_rows(0, A)
            s.set_rhs(np.ones(n))
            got = s.check_symmetry()
            if got != want:
                problems.append(f"{label}: check_symmetry() = {got!r}, expected {want!r}")
            capfd.readouterr()
            s.cg_init()
            err = capfd.readouterr().err
            eff = s.get_option("symmetric_effective")
            if (eff != 0 or "refused" not in err) if refused else (eff != 1 or ENV in err):
                problems.append(f"{label}: expected {'a refusal' if refused else 'silence'}, got symmetric_effective = {eff}, stderr {err!r}")
    assert not problems, f"{dtype_name} shards={shards}: " + "; ".join(problems)


# ------------------------------------------------------------------------------------------------
# D. what bf16 storage holds: round to nearest even of the fp32 value, compared as bit patterns
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_by_row", [False, True])
@pytest.mark.parametrize("shards", [1, 3])
def test_bf16_storage_rounds_to_nearest_even(lam, shards, row_by_row):
    """n = 1003: pitch 1008, a row ends inside a 16-byte vector.  Four rows around the boundary between shards 0 and 1 (rows 334
    of 3 shards) carry the probe values of symmetry_data.BF16_PROBES, shifted from row to row so that each meets several
    alignments and the row's end; uploaded as one block or row by row.  Then finite rows go the same way and a GEMV of ones must give
    the row sums: the padding behind the rows is still zero."""
    n, r0, nr = 1003, 332, 4
    probes = S.BF16_PROBES
    u = np.stack([np.roll(np.resize(probes, n + 7 * k), 7 * k)[:n] for k in range(nr)])
    want, nan = S.bf16_rne_bits(u), S.is_nan_bits(u)
    assert nan.any() and all(set(probes.tolist()) <= set(r.tolist()) for r in u)

    def upload(s, block):
        if row_by_row:
            for k in range(nr):
                s.upload_rows(r0 + k, block[k:k + 1])
        else:
            s.upload_rows(r0, block)

    with lam.Solver(lam.BF16, device_ids=[0] * shards) as s:
        s.generate_random_spd(n, 9, 10.0)
        if shards > 1:
            assert r0 < s.partition(1)[0] < r0 + nr
        upload(s, u.view(np.float32))
        got = s.download_rows(r0, nr).view(np.uint32)
        assert np.all(S.is_nan_bits(got[nan])), "a NaN did not stay a NaN"
        bad = np.argwhere((got != want) & ~nan)
        assert len(bad) == 0, [(tuple(b), hex(u[tuple(b)]), hex(got[tuple(b)]), hex(want[tuple(b)])) for b in bad[:8]]
        # the rows around the block are untouched, and finite again afterwards: the padding is still zero
        finite = np.random.default_rng(12).uniform(-1, 1, (nr, n)).astype(np.float32)
        upload(s, finite)
        A_dev = _dev64(s)
        assert np.all(np.isfinite(A_dev))
        y = s.gemv(np.ones(n)).astype(np.float64)
        assert np.max(np.abs(y - A_dev.sum(axis=1)) / np.abs(A_dev).sum(axis=1)) <= GATE["BF16"]
