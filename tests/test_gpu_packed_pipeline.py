"""Option "packed": what a tile-ahead pipeline in gemv_packed_kernel can get wrong.

A kernel that loads a tile's headers one tile ahead, stages the exception lists of consecutive tiles into alternating LDS buffers
or refills its p tile for the next tile while the current one is still being multiplied (three such variants
were built and measured; the kernel that ships stages p between its two barriers in one round trip) has state that crosses the
tile boundary.  test_gpu_packed.py and test_gpu_packed_edges.py cover n = 384, 1547, 4097 and one 12288 case; here are
  a. two-tile matrices whose last tile ends around every super-step (1024 columns) and half-tile (2048 columns) edge, odd sizes
     and one size with a two-column last tile behind three whole ones, with ladder rows (tests/packed_model.py) planted so that
     consecutive tiles and the two rows of a workgroup differ in window and carry lists of 0 to 256 values.  With two tiles the
     rotated start wraps inside the loop for odd workgroups;
  b. three products in a row at ntiles = 1 (n = 384, 4096), a different vector each: a stale next-tile header or a wrong buffer
     parity shows in the second or third product, not in the first;
  c. one solve in pieces that runs past convergence, so that launches behind the stop flag are in it.
Everything is equality of raw bits, packed = 1 against packed = 0 in one context."""
import functools

import numpy as np
import pytest

import packed_model as M
from test_gpu_packed import COND, SEED, bits, product_both_ways, vec
from test_gpu_packed_edges import on_image, small, u64

pytestmark = pytest.mark.gpu

K = 16                  # planted ladder rows a block
ODD_ROW = 1001          # the second row of workgroup 500: a ladder row beside a generated one, and so on through the block

# last tile of two: 2, 1024, 1026, 2046, 2048, 2050, 3072, 3074, 4094 and 4096 columns; odd n (the last workgroup's second row is
# clamped, the last vector is ragged); 12290 = 3 * 4096 + 2: three whole tiles and a two-column one
SIZES = (4098, 5120, 5122, 6142, 6144, 6146, 7168, 7170, 8190, 8192, 4099, 6147, 12290)


@functools.lru_cache(maxsize=None)
def planted(n):
    """The K ladder rows planted into an n-column matrix, after the precondition on the numpy model of their headers: a list
    longer than the 64 values that are always read in a tile that is not the last, followed by a tile with another window; and
    a full list somewhere."""
    rows = M.ladder_rows(K, n, seed=3)
    base, count = M.headers(M.bits(rows), M.ncols_vec(n))
    assert base.shape == (K, -(-M.ncols_vec(n) // M.TILE))
    assert np.any((count[:, :-1] > M.FIRST) & (base[:, :-1] != base[:, 1:]))
    assert count.max() == M.CAP
    return rows


@pytest.mark.parametrize("n", SIZES)
def test_ladder_rows_around_every_tile_edge_both_ways(lam, n):
    rows = planted(n)
    offsets = (0, ODD_ROW, n - K)
    with lam.Solver(lam.F64) as s:
        s.generate_random_spd(n, SEED, COND)
        for r0 in offsets:
            s.upload_rows(r0, rows)
        for r0 in offsets:
            assert np.array_equal(bits(s.download_rows(r0, K)), M.bits(rows))
        for nt in (1, 0):
            s.set_option("nt_loads", nt)
            for x in (vec(n, 51), small(n, 52)):
                y0, y1, eff = product_both_ways(s, x)
                assert eff == 1 and on_image(s, "true" if nt else "false")
                bad = np.flatnonzero(bits(y0) != bits(y1))
                assert bad.size == 0, (n, nt, bad[:8])
        assert np.all(np.isfinite(y0)) and np.count_nonzero(y0) >= n - 1


@pytest.mark.parametrize("n", (384, 4096))
def test_three_products_in_a_row_on_a_one_tile_image(lam, n):
    """ntiles = 1: the tile is the first and the last one, there is no next header and no next p tile."""
    xs = [small(n, 61), small(n, 62) * 3.0, small(n, 63) - 2.0 ** -22]
    with lam.Solver(lam.F64) as s:
        s.set_matrix(M.ladder(n))
        s.set_option("packed", 0)
        want = [s.gemv(x) for x in xs]
        assert s.get_option("packed_effective") == 0
        s.set_option("packed", 1)
        got = [s.gemv(x) for x in xs]
        assert on_image(s)
        for i, (y0, y1) in enumerate(zip(want, got)):
            bad = np.flatnonzero(bits(y0) != bits(y1))
            assert bad.size == 0, (n, i, bad[:8], bad[:8] % M.NCLASS)
        assert not np.array_equal(want[0], want[1]) and not np.array_equal(want[1], want[2])
        assert np.all(np.isfinite(want[2])) and np.count_nonzero(want[2]) >= n - 1


def test_a_solve_in_pieces_past_convergence_is_the_plain_one(lam):
    """n = 5122 (two tiles, the last 1026 columns wide), cond = 100.  The tolerance is the residual the plain solve reports after 4
    iterations, so the stop comes inside the third piece (iterations 4 .. 8) and the launches behind it -- in that piece and in
    the fourth -- return at the stop flag."""
    n = 5122
    with lam.Solver(lam.F64) as s:
        s.generate_random_spd(n, SEED, COND)
        s.generate_random_rhs(SEED + 1)
        s.set_option("packed", 0)
        s.solve(4, 1e-30)
        tol = s.stats["rel_err"] * (1.0 + 2.0 ** -40)
        assert 0.0 < tol < 1.0
        got = {}
        for packed in (0, 1):
            s.set_option("packed", packed)
            s.cg_init()
            for piece in (1, 2, 5, 5):
                st = s.cg_iterate(piece, tol)
                assert s.get_option("packed_effective") == packed
                got.setdefault(packed, []).append((s.solution(), st["rel_err"], st["num_iters"]))
            assert on_image(s) if packed else s.get_option("packed_bytes") == 0
        assert got[0][-1][2] <= 5 and got[0][-1][2] == got[0][-2][2]      # converged inside the third piece; the fourth adds nothing
        for (x0, e0, i0), (x1, e1, i1) in zip(got[0], got[1]):
            assert np.array_equal(bits(x0), bits(x1)) and u64(e0) == u64(e1) and i0 == i1
        assert not np.array_equal(got[0][0][0], got[0][2][0])
