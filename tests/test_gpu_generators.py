"""The device-side system generators against the host model of their laws (tests/generator_model.py), element for element.

bench.py's system, the rank-mode doubles and most of the suite's solves start from lam_hip_generate_random_spd /
lam_hip_generate_random_rhs / lam_hip_generate_tridiag / lam_hip_generate_spectrum_spd.  Here every element of what they write is
compared -- as BIT PATTERNS unless a gate is named -- with the law, at the sizes where the kernels can go wrong:

  * the matrix generators launch 4096 x 256 = 2^20 threads: n = 1024 is one element per thread, n = 1025 the first trip round the
    grid-stride loop, n = 1777 on 3 shards (592 / 592 / 593 rows) wraps on every shard with the remainder on the last one;
  * a row pitch equal to n (n = 1024, 2048: no padding) and larger than n, in all three storage types;
  * seeds 0 and 2^64 - 1 (`seed + hash` wraps; the binding passes a full uint64);
  * the right-hand side past the vector launches' 65 536 threads (n = 65537);
  * the matrix allocation re-used by a SMALLER problem whose row padding lands on what the previous problem left there.

Every context lives on GPU 0."""
import numpy as np
import pytest

import exact_data as E
import generator_model as M

pytestmark = pytest.mark.gpu

DTYPES = ("F64", "F32", "BF16")
SEED_MAX = (1 << 64) - 1


def _ctx(lam, dtype_name, shards):
    return lam.Solver(getattr(lam, dtype_name), device_ids=[0] * shards)


def _assert_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    msg = M.first_mismatches(got, want)
    assert not msg, f"{what}: {msg}"


def _assert_pitch(s, n, dtype_name, padded=None):
    pitch = s.get_option("row_pitch")
    assert pitch == M.row_pitch(n, M.ESZ[dtype_name]), (dtype_name, n, pitch)
    if padded is not None:
        assert (pitch > n) == padded, f"{dtype_name} n={n}: pitch {pitch}, the case is meant to be {'padded' if padded else 'unpadded'}"


# ------------------------------------------------------------------------------------------------
# a + c. random SPD matrix and tridiag(1, 2, 1)
# ------------------------------------------------------------------------------------------------
# n, shard counts (the first is the one-shard download every other sharding must equal)
MATRIX_CASES = [(1, (1,)), (2, (1,)), (3, (1, 3)), (7, (1,)), (300, (1, 4)), (1024, (1,)), (1025, (1,)), (1777, (1, 3)), (2048, (1, 3))]
EXACT_CONDS = (1.0, 3.0, 1025.0)          # (cond - 1) u is exact: one model value
CANDIDATE_CONDS = (1e6, 50.0, 10.0)       # 1 + (cond - 1) u may or may not be contracted: two candidates (1234, 1e6: bench.py's system)


def _intended_padding(n, dtype_name):
    """Whether the case is MEANT to have row padding (the pitch itself is asserted against the model's rule as well)."""
    if n in (1024, 2048):
        return False                       # whole 4-KiB pages (or, bf16 at 1024, whole 16-byte vectors) in every storage type
    if n == 300:
        return dtype_name == "BF16"        # 300 elements are whole 16-byte vectors of fp64 and fp32, not of bf16 (304)
    if n == 2:
        return dtype_name != "F64"
    return True                            # 1, 3, 7, 1025, 1777


def _spd_seeds_and_conds(n):
    if n <= 300:
        return [(seed, cond) for seed in (0, 1234, SEED_MAX) for cond in EXACT_CONDS + CANDIDATE_CONDS]
    return [(1234, 1e6), (1234, 10.0)]


def _random_spd_model(n, seed, cond, dtype_name):
    """[(label, the stored matrix with the unfused diagonal, [the stored unfused diagonal, the stored fused diagonal])]: one entry,
    or for bf16 storage one per rounding the compiler may give `__float2bfloat16((float)v)` (tests/generator_model.py, Storage)."""
    A, diags = M.random_spd(n, seed, cond), M.random_spd_diagonals(n, seed, cond)
    if dtype_name != "BF16":
        return [("", M.stored(A, dtype_name), [M.stored(d, dtype_name) for d in diags])]
    return [(f", bf16 rounded {r}", M.stored(A, dtype_name, r), [M.stored(d, dtype_name, r) for d in diags]) for r in M.BF16_ROUNDINGS]


def _check_random_spd(A, model, cond, what):
    """Off-diagonals bit for bit; the diagonal equals ONE of the two candidates at every row; in bf16 the WHOLE matrix follows one
    of the two roundings.  Returns the fitting [(diagonal: 'exact' / 'unfused' / 'fused' / 'both', bf16 rounding label)]."""
    idx = np.arange(A.shape[0])
    got_d = A[idx, idx].copy()
    verdicts, complaints = [], []
    for label, want, cand in model:
        off = A.copy()
        off[idx, idx] = want[idx, idx]
        msg = M.first_mismatches(off, want)
        if msg:
            complaints.append(f"off-diagonal elements{label}: {msg}")
            continue
        eq = [np.array_equal(M.bits(got_d), M.bits(c)) for c in cand]
        if cond in EXACT_CONDS:
            assert np.array_equal(M.bits(cand[0]), M.bits(cand[1]))
            if eq[0]:
                verdicts.append(("exact", label))
            else:
                complaints.append(f"diagonal{label} (row: got, want): {M.first_mismatches(got_d, cand[0])}")
            continue
        which = "both" if all(eq) else "unfused" if eq[0] else "fused" if eq[1] else None
        if which is not None:
            verdicts.append((which, label))
        else:
            complaints.append(f"the diagonal{label} is neither candidate at every row -- against unfused fl(1 + fl((cond-1) u)): "
                              f"{M.first_mismatches(got_d, cand[0])}; against fused fl(1 + (cond-1) u): {M.first_mismatches(got_d, cand[1])}")
    assert verdicts, f"{what}: " + "; ".join(complaints)
    return verdicts


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("n,shard_counts", MATRIX_CASES)
def test_matrix_generators_match_the_model(lam, n, shard_counts, dtype_name):
    """lam_hip_generate_tridiag and lam_hip_generate_random_spd, every element, every sharding; the random matrix equals its own
    transpose and the one-shard download bit for bit."""
    ctxs = [_ctx(lam, dtype_name, P) for P in shard_counts]
    try:
        tri = M.stored(M.tridiag(n), dtype_name)
        for P, s in zip(shard_counts, ctxs):
            s.generate_matrix(n)
            _assert_pitch(s, n, dtype_name, _intended_padding(n, dtype_name))
            _assert_bits(s.download_rows(0, n), tri, f"tridiag {dtype_name} n={n} shards={P}")
        seen, alone_diag, alone_rounding = {}, set(), set()
        for seed, cond in _spd_seeds_and_conds(n):
            first, model = None, _random_spd_model(n, seed, cond, dtype_name)
            for P, s in zip(shard_counts, ctxs):
                what = f"random_spd {dtype_name} n={n} shards={P} seed={seed} cond={cond}"
                s.generate_random_spd(n, seed, cond, keep_problem=True)
                A = s.download_rows(0, n)
                fits = _check_random_spd(A, model, cond, what)
                seen.setdefault(cond, set()).add(" or ".join(d + label for d, label in fits))
                if len({d for d, _ in fits}) == 1:
                    alone_diag |= {fits[0][0]} & {"unfused", "fused"}
                if len(fits) == 1:
                    alone_rounding.add(fits[0][1])
                _assert_bits(np.ascontiguousarray(A.T), A, f"{what}: transpose (the row index is the column here)")
                if first is None:
                    first = A
                else:
                    _assert_bits(A, first, f"{what}: against the one-shard matrix")
        print(f"diagonal candidates {dtype_name} n={n}: " + ", ".join(f"cond={c:g}: {'/'.join(sorted(w))}" for c, w in seen.items()))
        # one compiled kernel: a call that fits one candidate alone must not be contradicted by another call
        assert len(alone_diag) <= 1 and len(alone_rounding) <= 1, f"{dtype_name} n={n}: different candidates from call to call: {seen}"
    finally:
        for s in ctxs:
            s.close()


# ------------------------------------------------------------------------------------------------
# b. right-hand sides
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name,n,shards", [(d, 1777, P) for d in DTYPES for P in (1, 3)] + [("F64", 65537, 1), ("BF16", 65537, 1)])
def test_rhs_generators_match_the_model(lam, dtype_name, n, shards):
    """b[i] = TV(2 u01(sm(seed ^ sm(0xB5 + i))) - 1) by GLOBAL row; 65537 rows are one more than the vector launches have threads.
    The constant right-hand side is TV(value) everywhere."""
    with _ctx(lam, dtype_name, shards) as s:
        s.set_problem(n)
        for seed in (1235, 0, SEED_MAX):
            s.generate_random_rhs(seed)
            _assert_bits(s.rhs(), M.stored_vector(M.random_rhs(n, seed), dtype_name), f"random_rhs {dtype_name} n={n} shards={shards} seed={seed}")
        s.generate_rhs(0.1)
        _assert_bits(s.rhs(), M.stored_vector(np.full(n, 0.1), dtype_name), f"rhs(0.1) {dtype_name} n={n} shards={shards}")
        s.generate_rhs()
        _assert_bits(s.rhs(), np.ones(n, dtype=M.VEC_DTYPE[dtype_name]), f"rhs() {dtype_name} n={n} shards={shards}")


# ------------------------------------------------------------------------------------------------
# d. spectrum matrix
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", ["F64", "F32"])
@pytest.mark.parametrize("n,k,shard_counts", [(64, 1, (1, 3)), (257, 6, (1, 3)), (513, 3, (1, 3)), (1025, 2, (1, 3)), (1777, 1, (3,))])
def test_spectrum_generator_matches_the_model_elementwise(lam, n, k, shard_counts, dtype_name):
    """max |A_device - A_model| <= gate * max(eig), the model in longdouble (tests/generator_model.py): an orthogonal similarity
    with the wrong reflector, order or tau has the right eigenvalues and the wrong elements.  The gates are the ones the
    eigenvalue test uses (1e-12 fp64, 2e-5 fp32); the device's algorithm emulated on the CPU stays below 1 / 100 of them
    (tests/test_generator_model_cpu.py).  (1025, 2) and (1777, 1) take gen_diag_kernel and rank2_update_kernel round their
    grid-stride loops; k >= 2 is where the order of the reflectors shows.  Symmetric bit for bit."""
    eig, V = M.spectrum_inputs(n, k)
    model = M.spectrum_spd(M.spectrum_eig_as_uploaded(eig, dtype_name), V)
    mats = []
    for P in shard_counts:
        with _ctx(lam, dtype_name, P) as s:
            s.generate_spectrum_spd(eig, V)
            A = s.download_rows(0, n)
        mats.append(A)
        what = f"spectrum {dtype_name} n={n} k={k} shards={P}"
        diff = np.abs(A.astype(np.longdouble) - model)
        worst = np.unravel_index(np.argmax(diff), diff.shape)
        err = float(diff[worst]) / eig.max()
        print(f"{what}: max |A_dev - A_model| / max(eig) = {err:.3g}")
        over = np.argwhere(~(diff <= M.SPECTRUM_GATE[dtype_name] * eig.max()))
        assert over.size == 0, (f"{what}: {len(over)} elements beyond {M.SPECTRUM_GATE[dtype_name]:g} max(eig), worst {err:.3g}; first "
                                + " ".join(f"({i}, {j}: got {A[i, j]!r} want {float(model[i, j])!r})" for i, j in over[:4]))
        _assert_bits(np.ascontiguousarray(A.T), A, f"{what}: transpose")
    if len(mats) == 2:
        # every row starts on a 16-byte boundary at its padded pitch whatever the shard, so w = A v is summed in the same order on
        # every sharding and the matrices agree bit for bit (odd n included)
        _assert_bits(mats[1], mats[0], f"spectrum {dtype_name} n={n} k={k}: shards={shard_counts[1]} against shards={shard_counts[0]}")


@pytest.mark.parametrize("dtype_name", ["F64", "F32"])
@pytest.mark.parametrize("n", [128, 1025])
def test_spectrum_generator_without_reflectors_is_the_diagonal(lam, n, dtype_name):
    """k = 0: the diagonal is TV(eig) bit for bit and every off-diagonal element is +0."""
    eig, _ = M.spectrum_inputs(n, 0)
    want = np.zeros((n, n), dtype=M.VEC_DTYPE[dtype_name])
    want[np.arange(n), np.arange(n)] = M.stored_vector(eig, dtype_name)
    for P in (1, 3):
        with _ctx(lam, dtype_name, P) as s:
            s.generate_spectrum_spd(eig, np.zeros((0, n)))
            _assert_bits(s.download_rows(0, n), want, f"spectrum k=0 {dtype_name} n={n} shards={P}")


# ------------------------------------------------------------------------------------------------
# e. the matrix allocation re-used at another size and pitch (option reuse_matrix, the default)
# ------------------------------------------------------------------------------------------------
# sizes in units of the dtype's 4-KiB row (512 fp64, 1024 fp32, 2048 bf16 elements): n = q * unit + r, and the pitch in units
REUSE_WALK = [((3, 1), 4),      # 1537 in fp64: padded to 2048
              ((2, 6), 3),      # 1030: SHRINKS, padded to 1536 -- its padding lies where the first problem's rows were
              ((2, 0), 2),      # 1024: unpadded
              ((1, 3), 2),      # 515: the same pitch, half of every row is padding now
              ((4, 1), 5)]      # 2049: grows past the first allocation


def _walk_sizes(dtype_name):
    unit = 4096 // M.ESZ[dtype_name]
    return [(q * unit + r, p * unit) for (q, r), p in REUSE_WALK]


def _poison(s, n):
    """NaN in every element of the matrix: what the next layout's padding lands on unless lam_hip_set_problem clears it."""
    step = E.block_rows(n)
    blk = np.full((min(step, n), n), np.nan, dtype=s.mat_host_dtype)
    for r0 in range(0, n, step):
        s.upload_rows(r0, blk[:min(step, n - r0)])


def _product_walk(s, dtype_name, shards, tag):
    for n, pitch in _walk_sizes(dtype_name):
        what = f"{tag} {dtype_name} shards={shards} n={n}"
        s.set_problem(n)
        _assert_pitch(s, n, dtype_name)
        assert s.get_option("row_pitch") == pitch, (what, pitch)
        X = [E.int_vec(n, 100 * n + j) for j in range(8)]
        Y = E.generate(n, [s.upload_rows], X)
        for generic in (0, 1):
            s.set_option("force_generic", generic)
            _assert_bits(s.gemv(X[0]), Y[0].astype(s.vec_dtype), f"{what}: gemv force_generic={generic}")
        s.set_option("force_generic", 0)
        if shards == 1 and dtype_name != "BF16":          # the batched product: one shard, fp64 / fp32
            _assert_bits(s.gemv_many(np.stack(X)), np.stack(Y).astype(s.vec_dtype), f"{what}: gemv_many (column, row)")
        _poison(s, n)


@pytest.mark.parametrize("mode", ["reuse", "fresh", "generate"])
@pytest.mark.parametrize("shards", [1, 3])
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_matrix_allocation_reuse_leaves_no_stale_padding(lam, dtype_name, shards, mode):
    """One context walks 1537 -> 1030 -> 1024 -> 515 -> 2049 (fp64; scaled by the row unit of the other dtypes) and fills the whole
    matrix with NaN before it moves on, so that every shrink puts the new layout's row padding on NaNs.  The vector kernels read
    that padding against the zeros behind p: an exact integer product (tests/exact_data.py) comes out bit for bit only if the
    padding reads as zero.
      reuse     option reuse_matrix at its default (1): the allocation is kept and re-sliced at the new pitch;
      fresh     reuse_matrix = 0: free + allocate per problem, the same walk;
      generate  reuse_matrix = 1, and at the two shrinking steps the matrix comes from lam_hip_generate_random_spd instead of an
                upload: it equals a fresh context's bit for bit and its product is finite."""
    with _ctx(lam, dtype_name, shards) as s:
        assert s.get_option("reuse_matrix") == 1           # the default
        if mode in ("reuse", "fresh"):
            if mode == "fresh":
                s.set_option("reuse_matrix", 0)
            _product_walk(s, dtype_name, shards, mode)
            return
        for step, (n, pitch) in enumerate(_walk_sizes(dtype_name)):
            what = f"generate {dtype_name} shards={shards} n={n}"
            s.set_problem(n)
            assert s.get_option("row_pitch") == pitch, (what, pitch)
            if step in (1, 3):
                s.generate_random_spd(n, 1234, 50.0, keep_problem=True)
                A = s.download_rows(0, n)
                with _ctx(lam, dtype_name, shards) as f:
                    f.generate_random_spd(n, 1234, 50.0)
                    _assert_bits(A, f.download_rows(0, n), f"{what}: against a fresh context")
                y = s.gemv(np.ones(n))
                assert np.isfinite(y).all(), f"{what}: rows {np.flatnonzero(~np.isfinite(y))[:6].tolist()} of A 1 are not finite"
            _poison(s, n)
