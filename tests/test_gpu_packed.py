"""Option "packed": the fp64 general product on the 7-byte image of the matrix (csrc/lam_host_pack.h, pack_rows_kernel,
gemv_packed_kernel) gives the plain kernel's result BIT FOR BIT -- the decode is exact and the lane mapping and accumulation order are
those of gemv_coop_kernel<double,double,R=2,NT,WAVES=8> -- or does not run at all.

`packed` = 1 is checked against `packed` = 0 in the same context, raw bits compared (NaNs included).  Shapes: n = 384 (one ragged
tile), 1547 (odd, ragged, a row pitch off the tile), 4097 (a whole tile and a one-column tile), 12288 = 8192 + 4096 (three whole
tiles, rotated start).  CAP is lam_host_pack.h's kPackCap: exceptions a (row, tile) may hold."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CAP = 256
SIZES = (384, 1547, 4097, 12288)
SEED, COND = 5, 100.0


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def vec(n, seed):
    return np.random.default_rng(seed).standard_normal(n)


def product_both_ways(s, x):
    """(plain, packed, packed_effective after the packed product) of the context's current matrix."""
    s.set_option("packed", 0)
    y0 = s.gemv(x)
    assert s.get_option("packed_effective") == 0 and "gemv_coop_kernel<double,double,R=2" in s.gemv_kernel_name()
    s.set_option("packed", 1)
    y1 = s.gemv(x)
    return y0, y1, s.get_option("packed_effective")


@pytest.mark.parametrize("n", SIZES)
def test_product_of_the_random_spd_matrix_is_the_plain_one_bit_for_bit(lam, n):
    with lam.Solver(lam.F64) as s:
        s.generate_random_spd(n, SEED, COND)
        y0, y1, eff = product_both_ways(s, vec(n, 1))
        assert eff == 1 and s.gemv_kernel_name().startswith("gemv_packed_kernel<double,double,R=2,TILE=4096,NT=true,WAVES=8>")
        assert np.array_equal(bits(y0), bits(y1))
        assert np.all(np.isfinite(y0)) and np.any(y0 != 0.0)
        # a second vector on the image that is already there, and the byte model
        x2 = vec(n, 2)
        y1b = s.gemv(x2)
        s.set_option("packed", 0)
        assert s.get_option("packed_bytes") == 0
        assert np.array_equal(bits(s.gemv(x2)), bits(y1b))
        s.set_option("packed", 1)
        pb = s.get_option("packed_bytes")
        ntiles = (n + 1) // 2 * 2
        ntiles = (ntiles + 4095) // 4096
        assert pb >= n * ntiles * (8 * 3584 + 4) + 16 * n
        if n % 4096 == 0:
            # 7 of 8 bytes an element, plus a header and a few dozen exact values per row and tile
            assert 0.875 < pb / (8.0 * n * n) < 0.90


def special_matrix(n, rng, cap_row_exceptions):
    """One binade of ordinary values; +-0, denormals, +-Inf, a NaN with a payload and one huge element in every row; row 5 has
    exactly `cap_row_exceptions` elements outside any window in its first tile."""
    A = (1.0 + rng.random((n, n))) * rng.choice([-1.0, 1.0], (n, n))
    special = np.array([0x0, 0x8000000000000000, 0x1, 0x800fffffffffffff, 0x7ff0000000000000, 0xfff0000000000000, 0x7ff4000000abcdef],
                       dtype=np.uint64).view(np.float64)
    w = min(n, 4096)
    for i in range(n):
        if i == 5:
            continue
        cols = rng.choice(w, special.size + 1, replace=False)
        if i % 7 == 0:
            A[i, cols[:-1]] = special                                 # non-finite values in every 7th row only
        else:
            A[i, cols[:4]] = special[:4]
        A[i, cols[-1]] = 1e200 * (1.0 + i)                            # one huge element per row
    cols = rng.choice(w, cap_row_exceptions, replace=False)
    # zeros, and small values 7 binades apart from each other: no window of 7 holds more than one of them, so the window that holds
    # the most elements is the ordinary values' and exactly these elements lie outside it
    k = np.arange(cap_row_exceptions)
    A[5, cols] = np.where(k % 2 == 0, 0.0, 1.5 * 2.0 ** (-100.0 - 7.0 * (k // 2)))
    return A


@pytest.mark.parametrize("n", (384, 4097))
def test_special_values_and_a_tile_with_exactly_cap_exceptions(lam, n):
    rng = np.random.default_rng(n)
    A = special_matrix(n, rng, CAP)
    with lam.Solver(lam.F64) as s:
        s.set_matrix(A)
        y0, y1, eff = product_both_ways(s, vec(n, 3))
        assert eff == 1
        assert np.array_equal(bits(y0), bits(y1))
        assert np.isnan(y0[0]) and np.isfinite(y0[1]) and np.isfinite(y0[5])
        # a vector with zeros and a negative zero against the non-finite elements
        x = vec(n, 4)
        x[::3] = 0.0
        x[1::5] = -0.0
        y1 = s.gemv(x)
        s.set_option("packed", 0)
        assert np.array_equal(bits(s.gemv(x)), bits(y1))


def test_solve_is_the_plain_one_bit_for_bit(lam):
    n = 1547
    with lam.Solver(lam.F64) as s:
        s.generate_random_spd(n, SEED, COND)
        s.generate_random_rhs(SEED + 1)
        got = {}
        for packed in (0, 1):
            s.set_option("packed", packed)
            for k in (1, 2, 5, 20):
                s.solve(k, 1e-30)
                assert s.get_option("packed_effective") == packed
                got[packed, k] = (s.solution(), s.stats["rel_err"], s.stats["num_iters"])
        for k in (1, 2, 5, 20):
            (x0, e0, i0), (x1, e1, i1) = got[0, k], got[1, k]
            assert np.array_equal(bits(x0), bits(x1)) and bits(np.array([e0]))[0] == bits(np.array([e1]))[0] and i0 == i1, k
        assert not np.array_equal(got[0, 5][0], got[0, 20][0])


def test_a_tile_with_one_exception_too_many_and_the_tridiagonal_matrix_stay_plain(lam):
    n = 384
    A = special_matrix(n, np.random.default_rng(7), CAP + 1)
    x = vec(n, 5)
    with lam.Solver(lam.F64) as s:
        s.set_matrix(A)
        y0, y1, eff = product_both_ways(s, x)
        assert eff == 0 and "gemv_coop_kernel" in s.gemv_kernel_name() and s.get_option("packed_bytes") == 0
        assert np.array_equal(bits(y0), bits(y1))
        s.generate_matrix(1547)
        x = vec(1547, 6)
        y0, y1, eff = product_both_ways(s, x)
        assert eff == 0 and "gemv_coop_kernel" in s.gemv_kernel_name()
        assert np.array_equal(bits(y0), bits(y1))
        want = 2.0 * x
        want[1:] += x[:-1]
        want[:-1] += x[1:]
        assert np.allclose(y1, want, rtol=1e-13, atol=1e-13)


def test_out_of_scope_configurations_are_not_packed(lam):
    n = 384
    for kind in ("F32", "BF16", "two shards", "symmetric"):
        kw = {"device_ids": [0, 0]} if kind == "two shards" else {}
        with lam.Solver(getattr(lam, kind) if kind in ("F32", "BF16") else lam.F64, **kw) as s:
            s.generate_random_spd(n, SEED, COND)
            if kind == "symmetric":
                s.set_option("symmetric", 1)
            s.set_option("packed", 1)
            x = vec(n, 8).astype(s.vec_dtype)
            y1 = s.gemv(x)
            assert s.get_option("packed_effective") == 0 and s.get_option("packed_bytes") == 0, kind
            assert "packed" not in s.gemv_kernel_name(), kind
            s.set_option("packed", 0)
            assert np.array_equal(s.gemv(x), y1), kind
    with lam.Solver(lam.F64) as s:
        with pytest.raises(lam.LamHipError):
            s.set_option("packed", 2)
        # the other shapes of the product read A
        s.generate_random_spd(n, SEED, COND)
        s.set_option("packed", 1)
        for name, value in (("gemv_variant", 17), ("force_generic", 1)):
            s.set_option(name, value)
            s.gemv(vec(n, 9))
            assert s.get_option("packed_effective") == 0, name
            s.set_option(name, -1 if name == "gemv_variant" else 0)


def test_new_rows_after_packing_are_what_the_next_product_reads(lam):
    n = 1547
    x = vec(n, 10)
    with lam.Solver(lam.F64) as s:
        s.generate_random_spd(n, SEED, COND)
        s.set_option("packed", 1)
        y_old = s.gemv(x)
        assert s.get_option("packed_effective") == 1
        rows = np.random.default_rng(11).standard_normal((3, n))
        s.upload_rows(700, rows)
        assert s.get_option("packed_effective") == 0          # the image holds the old content
        y_new = s.gemv(x)
        assert s.get_option("packed_effective") == 1          # packed again in front of that product
        s.set_option("packed", 0)
        y_plain = s.gemv(x)
        assert np.array_equal(bits(y_new), bits(y_plain))
        assert np.array_equal(bits(y_new[:700]), bits(y_old[:700])) and np.array_equal(bits(y_new[703:]), bits(y_old[703:]))
        assert not np.any(y_new[700:703] == y_old[700:703])
        # a content that is not packable after one that was, and back
        s.set_option("packed", 1)
        s.upload_rows(0, np.zeros((1, n)))
        y_zero = s.gemv(x)
        assert s.get_option("packed_effective") == 0
        assert y_zero[0] == 0.0 and np.array_equal(bits(y_zero[1:]), bits(y_plain[1:]))
        s.upload_rows(0, rows[:1])
        s.gemv(x)
        assert s.get_option("packed_effective") == 1


def test_automatic_mode_stays_plain_at_small_sizes(lam):
    n = 1547
    with lam.Solver(lam.F64) as s:
        assert s.get_option("packed") == -1
        s.generate_random_spd(n, SEED, COND)
        s.generate_random_rhs(SEED + 1)
        x = vec(n, 12)
        ys = [s.gemv(x) for _ in range(12)]
        s.solve(30, 1e-30)
        s.gemv_only(20)
        assert s.get_option("packed_effective") == 0 and s.get_option("packed_bytes") == 0
        assert "gemv_coop_kernel<double,double,R=2" in s.gemv_kernel_name()
        assert all(np.array_equal(bits(y), bits(ys[0])) for y in ys)
        assert s.stats["gemv_bytes"] == 8.0 * n * n + 8.0 * 2 * n
