"""Option "packed" where test_gpu_packed.py cannot see: decode, window choice, list staging and the automatic switch.

test_gpu_packed.py compares the packed product with the plain one on matrices that have ONE window throughout and a few dozen
exceptions a tile.  Here the inputs are tests/packed_model.py's ladders -- every row of a workgroup's pair and every tile of a row
has a window of its own, the ends of the exponent range included, and the lists hold 0, 1, 63, 64, 65, 128, 255 and 256 values in
every tile -- and the references are not the plain kernel alone:
  a. the product with a unit vector must be the matrix's own column, bit for bit;
  b. the ladder both ways (packed = 0 against packed = 1 in one context, raw bits), also with nt_loads = 0 and patched into a
     three-tile random matrix;
  c. packed_bytes must be the integer the numpy model of the header gives for the device's content (tied to lam_host_pack.h by
     test_packed_model_cpu.py): pack_rows_kernel's window choice and counts, which no product can see;
  d. exact_data's known answers (GEMV, first CG step) on the image;
  e. the other readers of the image: true_residual, cg_iterate in pieces, gemv_only under probe_rows, a reused image buffer;
  f. the automatic mode, moved to test sizes by the testing options packed_after / packed_min_bytes: the counter, its reset on
     new content, the refusal of an unpackable content, the switch between two iterations of a running solve.
Everything is equality of bits or integers."""
import functools

import numpy as np
import pytest

import exact_data as E
import packed_model as M
from test_gpu_exact import _check_first_step, _integer_contexts
from test_gpu_packed import COND, SEED, bits, product_both_ways, vec

pytestmark = pytest.mark.gpu

PACKED = "gemv_packed_kernel<double,double,R=2,TILE=4096,NT={},WAVES=8>"
PLAIN = "gemv_coop_kernel<double,double,R=2"


def on_image(s, nt="true"):
    return s.get_option("packed_effective") == 1 and s.gemv_kernel_name().startswith(PACKED.format(nt))


def plain_bytes(n):
    return 8 * n * n + 8 * 2 * n


@functools.lru_cache(maxsize=None)
def ladder_headers(n):
    return M.headers(M.bits(M.ladder(n)), M.ncols_vec(n))


def where(j):
    """Tile column j % 4096 in the image's terms (lam_host_pack.h, pack_pos)."""
    t, c = divmod(j, M.TILE)
    return f"column {j}: tile {t}, wave group {(c >> 7) & 7}, lane {(c & 127) >> 1}, element {2 * (c >> 10) + (c & 1)}"


def small(n, seed):
    """A dense vector small enough that no row of a ladder overflows: n terms below 2^1024 * 2^-20 * 5."""
    return vec(n, seed) * 2.0 ** -20


# ------------------------------------------------------------------------------------------------
# a. decode through the kernel against the matrix itself
# ------------------------------------------------------------------------------------------------
def probe_columns(n):
    if n < M.TILE:
        return range(n)
    cols = {j for j in range(n) if j % 128 in (0, 1, 126, 127)} | {n - 3, n - 2, n - 1}
    return sorted(cols | set(np.random.default_rng(n).choice(n, 256, replace=False).tolist()))


@pytest.mark.parametrize("n", (384, 1547, 4097))
def test_a_unit_vector_reads_the_matrix_column_back_bit_for_bit(lam, n):
    """y = A e_j: the other terms of a row are a_k * 0 = +-0, so whatever the order of the sum, y_i has the bits of A[i, j] where
    that is not zero, and is zero where it is."""
    A = M.ladder(n)
    Ab = M.bits(A)
    with lam.Solver(lam.F64) as s:
        s.set_matrix(A)
        s.set_option("packed", 1)
        x = np.zeros(n)
        for j in probe_columns(n):
            x[j] = 1.0
            y = s.gemv(x)
            x[j] = 0.0
            assert on_image(s)
            nz = A[:, j] != 0.0
            bad = np.flatnonzero((bits(y) != Ab[:, j]) & nz)
            assert bad.size == 0, (f"{where(j)}: {bad.size} rows wrong, first {bad[:6]} (classes {bad[:6] % M.NCLASS}): "
                                   f"{[hex(v) for v in bits(y)[bad[:6]]]} != {[hex(v) for v in Ab[bad[:6], j]]}")
            bad = np.flatnonzero((y != 0.0) & ~nz)
            assert bad.size == 0, f"{where(j)}: rows {bad[:6]} hold a zero or a pad and give {y[bad[:6]]}"


# ------------------------------------------------------------------------------------------------
# b. the ladder both ways
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt", (1, 0))
@pytest.mark.parametrize("n", (384, 1547, 4097))
def test_the_ladder_both_ways(lam, n, nt):
    with lam.Solver(lam.F64) as s:
        s.set_matrix(M.ladder(n))
        s.set_option("nt_loads", nt)
        for x in (vec(n, 21), small(n, 22)):
            y0, y1, eff = product_both_ways(s, x)
            assert eff == 1 and on_image(s, "true" if nt else "false")
            bad = np.flatnonzero(bits(y0) != bits(y1))
            assert bad.size == 0, (bad[:8], bad[:8] % M.NCLASS)
        assert np.all(np.isfinite(y0)) and np.count_nonzero(y0) >= n - 1      # the small vector: every class of row says something


def test_ladder_rows_in_a_three_tile_matrix_both_ways(lam):
    n, k = 12288, 16
    rows = M.ladder_rows(k, n, seed=3)
    with lam.Solver(lam.F64) as s:
        s.generate_random_spd(n, SEED, COND)
        for r0 in (0, 4097, n - k):
            s.upload_rows(r0, rows)
        for r0 in (0, 4097, n - k):
            got = s.download_rows(r0, k)
            assert np.array_equal(bits(got), M.bits(rows))
            base, count = M.headers(bits(got), M.ncols_vec(n))
            assert base.shape == (k, 3) and np.all(base[:, :-1] != base[:, 1:]) and np.all(base[:-1] != base[1:]) and count.max() == M.CAP
        for nt in (1, 0):
            s.set_option("nt_loads", nt)
            for x in (vec(n, 23), small(n, 24)):
                y0, y1, eff = product_both_ways(s, x)
                assert eff == 1 and on_image(s, "true" if nt else "false")
                bad = np.flatnonzero(bits(y0) != bits(y1))
                assert bad.size == 0, bad[:8]


# ------------------------------------------------------------------------------------------------
# c. packed_bytes exactly
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("ladder", "random_spd"))
@pytest.mark.parametrize("n", (384, 1547, 4097))
def test_packed_bytes_is_the_models_integer(lam, n, kind):
    with lam.Solver(lam.F64) as s:
        if kind == "ladder":
            s.set_matrix(M.ladder(n))
            s.set_rhs(small(n, 25))
        else:
            s.generate_random_spd(n, SEED, COND)
            s.generate_random_rhs(SEED + 1)
        content = s.download_rows(0, n)
        hdrs = M.headers(bits(content), M.ncols_vec(n))
        want = M.packed_bytes(hdrs, n, n)
        assert hdrs[1].max() <= M.CAP
        s.set_option("packed", 1)
        s.gemv(vec(n, 26))
        assert on_image(s)
        assert s.get_option("packed_bytes") == want, (s.get_option("packed_bytes") - want, hdrs[1].sum())
        s.solve(2, 1e-30)
        assert on_image(s)
        assert s.stats["gemv_bytes"] == float(want) and int(s.stats["gemv_bytes"]) == want
        s.set_option("packed", 0)
        s.solve(2, 1e-30)
        assert s.get_option("packed_bytes") == 0 and s.stats["gemv_bytes"] == float(plain_bytes(n))


# ------------------------------------------------------------------------------------------------
# d. known answers on the image
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (384, 1547, 3000))
def test_exact_known_answers_on_the_image(lam, n):
    """exact_data's integer matrix (every zero an exception; packable at these sizes: test_packed_model_cpu.py): the GEMV is the
    exact integer product and the first CG step is first_cg_step / rel_err_bound, as test_gpu_exact.py holds the plain kernel to."""
    x, b = E.int_vec(n, 11), E.int_vec(n, 12)
    with _integer_contexts(lam, "F64", n, (1,), [x, b]) as ((s,), (y, Ab)):
        s.set_rhs(b)
        s.set_option("packed", 1)
        got = s.gemv(x)
        assert on_image(s)
        bad = np.flatnonzero(got != y)
        assert bad.size == 0, f"n={n}: {bad.size} rows wrong, first {bad[:6]}: {got[bad[:6]]} != {y[bad[:6]]}"
        _check_first_step(s, "F64", b, Ab, f"F64 n={n} packed")
        # the helper ends on its base options: the step it checked first, and this one, ran on the image
        s.solve(1, 1e-30)
        want_bytes = M.packed_bytes(M.headers(M.bits(E.int_block(0, n, n)), M.ncols_vec(n)), n, n)
        assert on_image(s) and s.stats["gemv_bytes"] == float(want_bytes) and s.get_option("packed_bytes") == want_bytes
        _, x1, _, _, _ = E.first_cg_step(b, Ab, np.float64)
        assert np.array_equal(bits(s.solution()), bits(x1 + 0.0))


# ------------------------------------------------------------------------------------------------
# e. the other readers of the image
# ------------------------------------------------------------------------------------------------
def u64(v):
    return bits(np.array([v]))[0]


def test_true_residual_pieces_and_probe_rows_read_the_image(lam):
    n = 1547
    with lam.Solver(lam.F64) as s:
        s.generate_random_spd(n, SEED, COND)
        s.generate_random_rhs(SEED + 1)
        got = {}
        for packed in (0, 1):
            s.set_option("packed", packed)
            s.solve(20, 1e-30)
            assert s.get_option("packed_effective") == packed
            whole = (s.solution(), s.stats["rel_err"], s.stats["num_iters"])
            tr = s.true_residual()
            assert s.get_option("packed_effective") == packed and (on_image(s) if packed else PLAIN in s.gemv_kernel_name())
            s.cg_init()
            for piece in (1, 2, 5, 12):
                st = s.cg_iterate(piece, 1e-30)
                assert s.get_option("packed_effective") == packed
                assert st["gemv_bytes"] == float(s.get_option("packed_bytes") if packed else plain_bytes(n))
            pieces = (s.solution(), st["rel_err"], st["num_iters"])
            got[packed] = (whole, tr, pieces)
        (w0, t0, p0), (w1, t1, p1) = got[0], got[1]
        assert 0.0 < t0 < 1.0 and u64(t0) == u64(t1)
        for (xa, ea, ia), (xb, eb, ib) in ((w0, w1), (p0, p1), (w0, p0)):
            assert np.array_equal(bits(xa), bits(xb)) and u64(ea) == u64(eb) and ia == ib == 21
        # gemv_only on the first 7 rows of the image (s.nrows < pk.nrows; the fourth workgroup's second row is clamped).  The C
        # interface has no accessor for Ap, so what the call leaves in it cannot be read back: it runs on the image, times a
        # product, and the image serves the next product unchanged.
        y_before = s.gemv(vec(n, 27))
        s.set_option("probe_rows", 7)
        assert s.gemv_only(3) > 0.0 and on_image(s)
        s.set_option("probe_rows", 0)
        assert s.gemv_only(2) > 0.0 and on_image(s)
        y0, y1, eff = product_both_ways(s, vec(n, 27))
        assert eff == 1 and np.array_equal(bits(y0), bits(y1)) and np.array_equal(bits(y1), bits(y_before))


def test_the_image_buffer_is_reused_across_problems_of_different_sizes(lam):
    """One context, n = 4097, 384, 1547, 4097: the allocation only grows, so the smaller images lie in a buffer that holds the
    larger one's lists (256 values long in the ladder) behind and between their own."""
    with lam.Solver(lam.F64) as s:
        s.set_option("packed", 1)
        for visit, n in enumerate((4097, 384, 1547, 4097)):
            if visit == 3:
                s.generate_random_spd(n, SEED, COND)          # the same size again, another content
                want = None
            else:
                s.set_matrix(M.ladder(n))
                want = M.packed_bytes(ladder_headers(n), n, n)
            for x in (vec(n, 28 + visit), small(n, 32 + visit)):
                y0, y1, eff = product_both_ways(s, x)
                assert eff == 1 and on_image(s)
                bad = np.flatnonzero(bits(y0) != bits(y1))
                assert bad.size == 0, (n, bad[:8])
            if want is not None:
                assert s.get_option("packed_bytes") == want, n
                x = np.zeros(n)
                x[n - 1] = 1.0                                # the last column: its list slot is the last one written
                assert np.array_equal(bits(s.gemv(x)), M.bits(M.ladder(n))[:, n - 1])


# ------------------------------------------------------------------------------------------------
# f. the automatic switch
# ------------------------------------------------------------------------------------------------
def automatic(s, after=None):
    assert s.get_option("packed") == -1
    s.set_option("packed_min_bytes", 0)
    if after is not None:
        s.set_option("packed_after", after)


def test_the_testing_options_have_the_constants_as_defaults_and_refuse_negative_values(lam):
    with lam.Solver(lam.F64) as s:
        assert s.get_option("packed_after") == 65 and s.get_option("packed_min_bytes") == 8 << 30
        for name in ("packed_after", "packed_min_bytes"):
            with pytest.raises(lam.LamHipError):
                s.set_option(name, -1)
        assert s.get_option("packed_after") == 65 and s.get_option("packed_min_bytes") == 8 << 30
        s.set_option("packed_min_bytes", 9 << 30)
        assert s.get_option("packed_min_bytes") == 9 << 30


def test_automatic_packs_in_front_of_the_66th_product(lam):
    n = 384
    x = vec(n, 40)
    with lam.Solver(lam.F64) as s:
        s.generate_random_spd(n, SEED, COND)
        automatic(s)
        ys = []
        for i in range(66):
            ys.append(s.gemv(x))
            assert s.get_option("packed_effective") == (1 if i == 65 else 0), i
        assert on_image(s) and PLAIN not in s.gemv_kernel_name()
        assert all(np.array_equal(bits(y), bits(ys[0])) for y in ys)
        assert s.get_option("packed_bytes") == M.packed_bytes(M.headers(bits(s.download_rows(0, n)), M.ncols_vec(n)), n, n)


def test_automatic_counts_plain_products_of_the_current_content(lam):
    n = 384
    x = vec(n, 41)
    with lam.Solver(lam.F64) as s:
        s.generate_random_spd(n, SEED, COND)
        automatic(s, after=3)

        def products(count):
            out = []
            for _ in range(count):
                y = s.gemv(x)
                out.append((s.get_option("packed_effective"), y))
            return [e for e, _ in out], [y for _, y in out]

        eff, ys = products(5)
        assert eff == [0, 0, 0, 1, 1]                      # three plain products, the image in front of the fourth
        assert all(np.array_equal(bits(y), bits(ys[0])) for y in ys)
        # new content: plain again, and the count starts anew
        s.upload_rows(100, np.random.default_rng(42).standard_normal((2, n)))
        assert s.get_option("packed_effective") == 0
        eff, ys = products(5)
        assert eff == [0, 0, 0, 1, 1]
        assert all(np.array_equal(bits(y), bits(ys[0])) for y in ys)
        # a larger threshold while the image is there changes nothing; the option counts for the next content
        s.set_option("packed_after", 5)
        s.upload_rows(100, np.random.default_rng(43).standard_normal((2, n)))
        eff, _ = products(7)
        assert eff == [0, 0, 0, 0, 0, 1, 1]
        # a content that is not packable is refused once and stays plain, however many products follow
        s.set_option("packed_after", 3)
        s.generate_matrix(n)
        eff, ys = products(10)
        assert eff == [0] * 10 and s.get_option("packed_bytes") == 0 and PLAIN in s.gemv_kernel_name()
        assert np.allclose(ys[-1], E.tridiag_product(x), rtol=1e-13, atol=1e-13)
        assert all(np.array_equal(bits(y), bits(ys[0])) for y in ys)
        # below packed_min_bytes nothing happens
        s.generate_random_spd(n, SEED, COND)
        s.set_option("packed_min_bytes", 8 * n * s.get_option("row_pitch") + 1)
        assert products(6)[0] == [0] * 6
        s.set_option("packed_min_bytes", 8 * n * s.get_option("row_pitch"))
        assert products(1)[0] == [1]


def test_the_switch_in_the_middle_of_a_solve_is_invisible(lam):
    """packed_after = 7 at n = 1547: pack_maybe packs between the 7th and the 8th iteration of lam_hip_cg_iterate's enqueue loop --
    a stream synchronise, an allocation and the pack pass with the stop flag and the timing ring live.  x, rel_err and num_iters
    are those of packed = 0, bit for bit; packed_effective afterwards is 1 exactly when more than 7 products were run."""
    n, after = 1547, 7
    with lam.Solver(lam.F64) as s:
        s.generate_random_spd(n, SEED, COND)
        s.generate_random_rhs(SEED + 1)
        want_bytes = M.packed_bytes(M.headers(bits(s.download_rows(0, n)), M.ncols_vec(n)), n, n)
        s.set_option("packed", 0)
        plain = {}
        for k in (3, 5, 7, 8, 18, 20):
            s.solve(k, 1e-30)
            plain[k] = (s.solution(), s.stats["rel_err"], s.stats["num_iters"])
        s.set_option("packed", -1)
        automatic(s, after)

        def fresh():
            """The same content as new content: the count starts at zero."""
            s.generate_random_spd(n, SEED, COND, keep_problem=True)
            assert s.get_option("packed_effective") == 0

        def same(k, what):
            x0, e0, i0 = plain[k]
            assert np.array_equal(bits(s.solution()), bits(x0)) and u64(s.stats["rel_err"]) == u64(e0) and s.stats["num_iters"] == i0, what

        for k, timing in ((5, 8), (7, 8), (8, 8), (20, 8), (20, 1)):
            fresh()
            s.set_option("gemv_timing", timing)
            s.solve(k, 1e-30)
            same(k, (k, timing))
            assert s.get_option("packed_effective") == (1 if k > after else 0), (k, timing)
            assert s.stats["gemv_bytes"] == float(want_bytes if k > after else plain_bytes(n)), (k, timing)
            if timing == 1:
                assert s.stats["t_gemv"] > 0.0
        s.set_option("gemv_timing", 8)
        # in pieces: the third call of three iterations holds the switch
        fresh()
        s.cg_init()
        eff = []
        for _ in range(6):
            st = s.cg_iterate(3, 1e-30)
            eff.append(s.get_option("packed_effective"))
            assert st["gemv_bytes"] == float(want_bytes if eff[-1] else plain_bytes(n))
        assert eff == [0, 0, 1, 1, 1, 1]
        same(18, "six calls of three iterations")
        # a solve that has converged before the switch stays plain.  The tolerance is the residual the plain solve reports after 3
        # iterations, so the stop comes at iteration 3 at the latest; the host runs kLag - 1 = 3 products ahead of the stop flag:
        # at most 6 products are counted, fewer than packed_after
        fresh()
        tol = plain[3][1] * (1.0 + 2.0 ** -40)
        assert s.solve(20, tol) and s.stats["num_iters"] <= 3
        assert s.get_option("packed_effective") == 0 and s.stats["gemv_bytes"] == float(plain_bytes(n))
        x_auto, st_auto = s.solution(), s.stats
        s.set_option("packed", 0)
        assert s.solve(20, tol)
        assert np.array_equal(bits(s.solution()), bits(x_auto)) and s.stats["num_iters"] == st_auto["num_iters"]


def test_out_of_scope_contexts_ignore_the_testing_options(lam):
    n = 384
    for kind in ("F32", "two shards"):
        kw = {"device_ids": [0, 0]} if kind == "two shards" else {}
        with lam.Solver(lam.F32 if kind == "F32" else lam.F64, **kw) as s:
            s.generate_random_spd(n, SEED, COND)
            s.generate_random_rhs(SEED + 1)
            automatic(s, after=1)
            x = vec(n, 44).astype(s.vec_dtype)
            ys = [s.gemv(x) for _ in range(4)]
            s.solve(6, 1e-30)
            assert s.get_option("packed_effective") == 0 and s.get_option("packed_bytes") == 0, kind
            assert "packed" not in s.gemv_kernel_name(), kind
            assert all(np.array_equal(y, ys[0]) for y in ys), kind
