"""Option "packed_many": the batched product of K = 1, 2, 4 columns on the 7-byte image of the matrix (multi_gemv_packed_kernel,
csrc/lam_host_pack.h pack_many_pos) gives multi_gemv_kernel's result BIT FOR BIT, for every consumer of the batch's one launch site,
or does not run at all.

`packed_many` = 1 is checked against `packed_many` = 0 in the same context, raw bits compared.  Shapes: n = 384 (one ragged batch
tile), 1547 (odd; two batch tiles of one unit at K = 4), 4097 (a whole unit and a two-column one), 9001 (three units, the last
ragged: nine batch tiles at K = 4, five at K = 2, and the rotation of most workgroups starts inside a unit), 12288 (three whole
units).  ADMITTED is lam_multi.h's pack_many_admitted: the K automatic mode serves (tools/packed_many_probe.py decides).

Every assertion is equality of bits or integers (one np.allclose is a sanity check of the tridiagonal product's values, as in
test_gpu_packed.py, and one compares the single product with the batched one, which are different kernels)."""
import numpy as np
import pytest

import packed_model as M
from test_gpu_packed import CAP, COND, SEED, bits, special_matrix, vec
from test_gpu_packed_edges import probe_columns, where

pytestmark = pytest.mark.gpu

ADMITTED = (1,)         # lam_multi.h pack_many_admitted: the K of automatic mode
N = 1547
PLAIN_SINGLE = "gemv_coop_kernel<double,double,R=2"


def vecs(nrhs, n, seed, scale=1.0):
    return np.random.default_rng(seed).standard_normal((nrhs, n)) * scale


def eff(s):
    return s.get_option("packed_many_effective")


def many_both_ways(s, X):
    """(plain, on the image, packed_many_effective after each) of the context's current matrix."""
    s.set_option("packed_many", 0)
    y0 = s.gemv_many(X)
    e0 = eff(s)
    s.set_option("packed_many", 1)
    y1 = s.gemv_many(X)
    return y0, y1, e0, eff(s)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------
# a. both ways
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt", (1, 0))
@pytest.mark.parametrize("n", (384, 1547, 4097, 9001))
def test_the_ladder_both_ways(lam, n, nt):
    with lam.Solver(lam.F64) as s:
        s.set_matrix(M.ladder(n))
        s.set_option("nt_loads", nt)
        for nrhs in (1, 2, 3, 4):
            for X in (vecs(nrhs, n, 30 + nrhs), vecs(nrhs, n, 40 + nrhs, 2.0 ** -20)):
                y0, y1, e0, e1 = many_both_ways(s, X)
                assert e0 == 0 and e1 == 1, nrhs
                bad = np.argwhere(bits(y0) != bits(y1))
                assert bad.size == 0, (nrhs, bad[:8], bad[:8, 1] % M.NCLASS)
            assert np.all(np.isfinite(y0)) and np.count_nonzero(y0) >= nrhs * (n - 1)


def test_ladder_rows_in_a_three_unit_matrix_both_ways(lam):
    n, k = 12288, 16
    rows = M.ladder_rows(k, n, seed=3)
    with lam.Solver(lam.F64) as s:
        s.generate_random_spd(n, SEED, COND)
        for r0 in (0, 4097, n - k):
            s.upload_rows(r0, rows)
        for nt in (1, 0):
            s.set_option("nt_loads", nt)
            for nrhs in (1, 2, 3, 4):
                for X in (vecs(nrhs, n, 50 + nrhs), vecs(nrhs, n, 60 + nrhs, 2.0 ** -20)):
                    y0, y1, e0, e1 = many_both_ways(s, X)
                    assert e0 == 0 and e1 == 1, nrhs
                    bad = np.argwhere(bits(y0) != bits(y1))
                    assert bad.size == 0, (nrhs, bad[:8])


# ------------------------------------------------------------------------------------------------
# b. independent of the plain kernel: unit vectors read the matrix's columns back
# ------------------------------------------------------------------------------------------------
def edge_columns(n):
    """probe_columns plus the first and last column of every batch tile (1024 columns at K = 4: those of K = 2, 1 and of the units
    are among them)."""
    cols = set(probe_columns(n))
    for c0 in range(0, n, 1024):
        cols |= {c0, min(n, c0 + 1024) - 1}
    return sorted(cols)


@pytest.mark.parametrize("nrhs", (1, 2, 4))
@pytest.mark.parametrize("n", (384, 1547, 4097))
def test_unit_vectors_read_the_matrix_columns_back_bit_for_bit(lam, n, nrhs):
    """Y = A [e_j ...]: the other terms of a row are a_k * 0 = +-0, so whatever the order of the sum, column c of Y has the bits of
    A[:, j_c] where that is not zero, and is zero where it is."""
    A = M.ladder(n)
    Ab = M.bits(A)
    cols = edge_columns(n)
    cols += cols[:(-len(cols)) % nrhs]
    with lam.Solver(lam.F64) as s:
        s.set_matrix(A)
        s.set_option("packed_many", 1)
        X = np.zeros((nrhs, n))
        for g in range(0, len(cols), nrhs):
            js = cols[g:g + nrhs]
            for c, j in enumerate(js):
                X[c, j] = 1.0
            Y = s.gemv_many(X)
            assert eff(s) == 1
            for c, j in enumerate(js):
                X[c, j] = 0.0
                nz = A[:, j] != 0.0
                bad = np.flatnonzero((bits(Y[c]) != Ab[:, j]) & nz)
                assert bad.size == 0, (f"{where(j)}, column {c} of {nrhs}: {bad.size} rows wrong, first {bad[:6]} "
                                       f"(classes {bad[:6] % M.NCLASS})")
                bad = np.flatnonzero((Y[c] != 0.0) & ~nz)
                assert bad.size == 0, f"{where(j)}, column {c} of {nrhs}: rows {bad[:6]} hold a zero or a pad and give {Y[c][bad[:6]]}"


# ------------------------------------------------------------------------------------------------
# c. columns do not mix
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nrhs", (2, 3, 4))
def test_a_nan_in_one_column_stays_in_that_column(lam, nrhs):
    n = N
    with lam.Solver(lam.F64) as s:
        s.generate_random_spd(n, SEED, COND)
        s.set_option("packed_many", 1)
        X = vecs(nrhs, n, 70)
        clean = s.gemv_many(X)
        assert eff(s) == 1 and np.all(np.isfinite(clean))
        for c in range(nrhs):
            Xn = X.copy()
            Xn[c, 777] = np.nan
            Y = s.gemv_many(Xn)
            assert np.all(np.isnan(Y[c]))
            others = [j for j in range(nrhs) if j != c]
            assert same(Y[others], clean[others]), c


# ------------------------------------------------------------------------------------------------
# d. the SHIFT epilogue
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ("cg", "minres"))
def test_shifted_solves_both_ways(lam, solver):
    n = N
    shifts = {"cg": (0.0, 1e-3, 0.5, 40.0), "minres": (-0.75, 1e-3, 0.5, -40.0)}[solver]
    with lam.Solver(lam.F64) as s:
        s.generate_random_spd(n, SEED, COND)
        b = vec(n, 80)
        got = {}
        for pm in (0, 1):
            s.set_option("packed_many", pm)
            for k in (1, 2, 5, 20):
                for count in (1, 2, 4):
                    if solver == "cg":
                        s.solve_shifted(b, shifts[:count], k, 1e-30)
                    else:
                        s.solve_shifted_minres(b, shifts[:count], k, 1e-30)
                    assert eff(s) == pm
                    got[pm, k, count] = (s.solutions(), s.rel_err_many.copy(), s.num_iters_many.copy())
        for k in (1, 2, 5, 20):
            for count in (1, 2, 4):
                (x0, e0, i0), (x1, e1, i1) = got[0, k, count], got[1, k, count]
                assert same(x0, x1) and same(e0, e1) and np.array_equal(i0, i1), (k, count)
        assert not np.array_equal(got[0, 5, 4][0], got[0, 20, 4][0])
        assert not np.array_equal(got[0, 20, 4][0][0], got[0, 20, 4][0][2])      # the shifts say something


# ------------------------------------------------------------------------------------------------
# e. every consumer once
# ------------------------------------------------------------------------------------------------
def consumers(lam, s, n):
    """name -> (arrays to compare, launches) of every consumer of the batch's launch site, under the option in force."""
    out = {}
    B = vecs(3, n, 90)

    def launches(f):
        l0 = s.get_option("hip_calls_launch")
        r = f()
        return r, s.get_option("hip_calls_launch") - l0

    def solved():
        return [s.solutions(), s.rel_err_many.copy(), s.num_iters_many.astype(np.float64)]

    s.set_rhs_many(B)
    _, ln = launches(lambda: s.solve_many(12, 1e-30))
    out["solve_many"] = (solved(), ln, eff(s))
    res = s.true_residuals()
    out["true_residuals"] = ([res], 0, eff(s))
    _, ln = launches(lambda: s.solve_many(12, 1e-30, precond=lam.PC_JACOBI))
    out["jacobi"] = (solved(), ln, eff(s))
    _, ln = launches(lambda: s.solve_many(6, 1e-30, x0=vecs(3, n, 91)))
    out["guess"] = (solved(), ln, eff(s))
    _, ln = launches(lambda: s.solve_multishift(B[0], np.linspace(0.0, 4.0, 9), 12, 1e-30))
    out["multishift"] = ([s.multishift_solutions(), s.rel_err_shift.copy()], ln, eff(s))
    r, ln = launches(lambda: s.eigs(3, "smallest", max_steps=24, tol=0.0, seed=5))
    a, b = s.lanczos_coefficients()
    out["eigs"] = ([r["theta"], a, b], ln, eff(s))
    out["eig_residuals"] = ([s.eig_residuals()], 0, eff(s))
    s.set_deflation_from_eigs(2)
    e_defl = eff(s)
    s.set_rhs_many(B)
    _, ln = launches(lambda: s.solve_deflated(10, 1e-30))
    out["deflated"] = (solved(), ln, min(eff(s), e_defl))
    s.set_deflation(None)
    r, ln = launches(lambda: s.lanczos_many(5, 10, seed=7))
    out["lanczos_many"] = ([r["alpha"], r["beta"], r["znorm2"]], ln, None)      # 5 probes are one K = 8 group: plain either way
    r, ln = launches(lambda: s.lanczos_many(3, 10, seed=8))
    out["lanczos_many_3"] = ([r["alpha"], r["beta"], r["znorm2"]], ln, eff(s))
    s.set_rhs_many(B)
    _, ln = launches(lambda: s.solve_block(8, 1e-30))
    out["block"] = (solved(), ln, eff(s))
    return out


def test_every_consumer_of_the_launch_site_both_ways(lam):
    n = N
    with lam.Solver(lam.F64) as s:
        s.generate_random_spd(n, SEED, COND)
        s.set_option("packed_many", 0)
        plain = consumers(lam, s, n)
        s.set_option("packed_many", 1)
        image = consumers(lam, s, n)
    assert plain.keys() == image.keys() and len(plain) == 11
    for name in plain:
        (a0, l0, e0), (a1, l1, e1) = plain[name], image[name]
        assert e0 in (0, None) and e1 in (1, None), name
        assert l0 == l1, (name, l0, l1)
        for u, v in zip(a0, a1):
            assert same(u, v), name
            assert np.any(np.asarray(u) != 0.0), name


# ------------------------------------------------------------------------------------------------
# f. the option and the refusals
# ------------------------------------------------------------------------------------------------
def test_the_option_its_values_and_where_it_does_not_engage(lam):
    n = 384
    with lam.Solver(lam.F64) as s:
        assert s.get_option("packed_many") == -1
        for bad in (2, -2):
            with pytest.raises(lam.LamHipError):
                s.set_option("packed_many", bad)
            assert s.get_option("packed_many") == -1
        s.set_option("packed_many", 1)
        with pytest.raises(lam.LamHipError):
            s.set_option("packed_many", 2)
        assert s.get_option("packed_many") == 1
        s.generate_random_spd(n, SEED, COND)
        assert eff(s) == 0                                   # before any product
        for nrhs in (5, 8):
            X = vecs(nrhs, n, 100)
            y1 = s.gemv_many(X)
            assert eff(s) == 0, nrhs
            s.set_option("packed_many", 0)
            assert same(s.gemv_many(X), y1)
            s.set_option("packed_many", 1)
        X = vecs(4, n, 101)
        y1 = s.gemv_many(X)
        assert eff(s) == 1
        # the symmetric batched product reads half the bytes and wins
        s.set_option("symmetric_many", 2)
        for nrhs in (1, 2, 4):
            s.gemv_many(X[:nrhs])
            assert eff(s) == 0 and s.get_option("symmetric_many_effective") == 1, nrhs
        s.set_option("symmetric_many", 0)
        assert same(s.gemv_many(X), y1) and eff(s) == 1
    with lam.Solver(lam.F32) as s:
        s.set_option("packed_many", 1)
        assert s.get_option("packed_many") == 1
        s.generate_random_spd(n, SEED, COND)
        X = vecs(2, n, 102).astype(np.float32)
        y1 = s.gemv_many(X)
        assert eff(s) == 0
        s.set_option("packed_many", 0)
        assert np.array_equal(s.gemv_many(X), y1)


def test_unpackable_contents_stay_plain(lam):
    n = 384
    X = vecs(3, n, 110)
    with lam.Solver(lam.F64) as s:
        s.set_matrix(special_matrix(n, np.random.default_rng(7), CAP + 1))
        y0, y1, e0, e1 = many_both_ways(s, X)
        assert e0 == 0 and e1 == 0 and same(y0, y1)
        s.generate_matrix(N)
        X = vecs(3, N, 111)
        y0, y1, e0, e1 = many_both_ways(s, X)
        assert e0 == 0 and e1 == 0 and same(y0, y1)
        want = 2.0 * X
        want[:, 1:] += X[:, :-1]
        want[:, :-1] += X[:, 1:]
        assert np.allclose(y1, want, rtol=1e-13, atol=1e-13)
        # special values and exactly CAP exceptions in a tile: packable
        s.set_matrix(special_matrix(n, np.random.default_rng(8), CAP))
        X = vecs(3, n, 112)
        y0, y1, e0, e1 = many_both_ways(s, X)
        assert e0 == 0 and e1 == 1 and same(y0, y1)
        assert np.all(np.isnan(y0[:, 0])) and np.all(np.isfinite(y0[:, 5]))


def test_a_new_upload_voids_the_image(lam):
    n = N
    X = vecs(2, n, 120)
    with lam.Solver(lam.F64) as s:
        s.generate_random_spd(n, SEED, COND)
        s.set_option("packed_many", 1)
        y_old = s.gemv_many(X)
        assert eff(s) == 1
        rows = np.random.default_rng(121).standard_normal((3, n))
        s.upload_rows(700, rows)
        y_new = s.gemv_many(X)
        assert eff(s) == 1                                   # packed again in front of that product
        s.set_option("packed_many", 0)
        assert same(s.gemv_many(X), y_new) and eff(s) == 0
        assert same(y_new[:, :700], y_old[:, :700]) and same(y_new[:, 703:], y_old[:, 703:])
        assert not np.any(y_new[:, 700:703] == y_old[:, 700:703])
        # a content that is not packable after one that was
        s.set_option("packed_many", 1)
        s.upload_rows(0, np.zeros((1, n)))
        y_zero = s.gemv_many(X)
        assert eff(s) == 0 and np.all(y_zero[:, 0] == 0.0) and same(y_zero[:, 1:], y_new[:, 1:])


def test_packed_zero_keeps_the_single_product_plain_and_the_batch_on_the_image(lam):
    n = N
    with lam.Solver(lam.F64) as s:
        s.generate_random_spd(n, SEED, COND)
        s.set_option("packed", 0)
        s.set_option("packed_many", 1)
        X = vecs(2, n, 130)
        Y = s.gemv_many(X)
        assert eff(s) == 1
        y = s.gemv(X[0])
        assert s.get_option("packed_effective") == 0 and PLAIN_SINGLE in s.gemv_kernel_name()
        s.gemv_many(X)
        assert eff(s) == 1
        # the single product of the same vector: another kernel, another order of the sum -- close, and here only as a sanity check
        assert np.allclose(y, Y[0], rtol=1e-9, atol=1e-9 * np.abs(Y[0]).max())


# ------------------------------------------------------------------------------------------------
# g. automatic mode
# ------------------------------------------------------------------------------------------------
def automatic(s, after):
    s.set_option("packed_many", -1)
    s.set_option("packed_min_bytes", 0)
    s.set_option("packed_after", after)


def test_automatic_mode(lam):
    n = N
    with lam.Solver(lam.F64) as s:
        s.generate_random_spd(n, SEED, COND)
        s.set_option("packed", 0)                            # the single product neither packs nor counts: the batch alone
        for nrhs in (1, 2, 4):
            s.upload_rows(0, s.download_rows(0, 1))          # new content: no image, the counter starts again
            automatic(s, 3)
            X = vecs(nrhs, n, 140 + nrhs)
            seen = []
            ys = []
            for _ in range(5):
                ys.append(s.gemv_many(X))
                seen.append(eff(s))
            assert seen == ([0, 0, 0, 1, 1] if nrhs in ADMITTED else [0] * 5), (nrhs, seen)
            assert all(same(y, ys[0]) for y in ys)
        if not ADMITTED:
            # no K was admitted by measurement: automatic mode never engages, whatever has been served
            s.set_option("packed", -1)
            for _ in range(5):
                s.gemv(vec(n, 150))
            s.gemv_many(vecs(1, n, 151))
            assert s.get_option("packed_effective") == 1 and eff(s) == 0       # the single product's image is there; the batch does not read it
            return
        k = ADMITTED[0]
        # single and batched products count on the same counter
        s.set_option("packed", -1)
        s.upload_rows(0, s.download_rows(0, 1))
        automatic(s, 3)
        X = vecs(k, n, 152)
        s.gemv(X[0]); s.gemv_many(X); s.gemv(X[0])
        assert eff(s) == 0 and s.get_option("packed_effective") == 0
        y = s.gemv_many(X)
        assert eff(s) == 1
        # the counter resets on new content
        s.upload_rows(0, s.download_rows(0, 1))
        for i in range(4):
            assert same(s.gemv_many(X), y)
            assert eff(s) == (1 if i == 3 else 0), i
        # an unpackable content is refused once
        s.upload_rows(0, np.zeros((1, n)))
        for i in range(6):
            s.gemv_many(X)
            assert eff(s) == 0
        # the switch in the middle of a batched solve is invisible
        s.upload_rows(0, s.download_rows(1, 1))
        B = vecs(k, n, 153)
        s.set_rhs_many(B)
        s.set_option("packed_many", 0)
        s.solve_many(20, 1e-30)
        want = (s.solutions(), s.rel_err_many.copy())
        assert eff(s) == 0
        s.upload_rows(0, s.download_rows(0, 1))
        automatic(s, 5)
        s.solve_many(20, 1e-30)
        assert eff(s) == 1
        assert same(s.solutions(), want[0]) and same(s.rel_err_many, want[1])


# ------------------------------------------------------------------------------------------------
# h. the byte count
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1547, 4097))
def test_gemv_bytes_of_a_batched_solve_is_the_models_integer(lam, n):
    with lam.Solver(lam.F64) as s:
        s.generate_random_spd(n, SEED, COND)
        content = s.download_rows(0, n)
        hdrs = M.headers(bits(content), M.ncols_vec(n))
        image = M.packed_bytes(hdrs, n, n) - 16 * n
        for nrhs in (1, 2, 4):
            s.set_rhs_many(vecs(nrhs, n, 160))
            s.set_option("packed_many", 1)
            s.solve_many(2, 1e-30)
            assert eff(s) == 1
            want = image + 16 * nrhs * n
            assert s.stats["gemv_bytes"] == float(want) and int(s.stats["gemv_bytes"]) == want, (nrhs, s.stats["gemv_bytes"] - want)
            s.set_option("packed_many", 0)
            s.solve_many(2, 1e-30)
            assert s.stats["gemv_bytes"] == float(8 * (n * n + 2 * nrhs * n)), nrhs
