"""tests/generator_model.py checked on the CPU: the host model that tests/test_gpu_generators.py holds the generator kernels to is
itself held to published constants, to a plain Python-int restatement, to exact rational arithmetic and to explicit Householder
matrices."""
from fractions import Fraction

import numpy as np
import pytest

import generator_model as M


# ------------------------------------------------------------------------------------------------
# hash, uniform
# ------------------------------------------------------------------------------------------------
def test_splitmix64_published_outputs():
    """The first two outputs of the published SplitMix64 generator seeded with 0: its state advances by the golden-ratio constant,
    so they are the output function at 0 and at 0x9E3779B97F4A7C15."""
    assert int(M.splitmix64(np.uint64(0))) == 0xE220A8397B1DCDAF
    assert int(M.splitmix64(np.uint64(0x9E3779B97F4A7C15))) == 0x6E789E6AA1B965F4
    assert M.splitmix64_int(0) == 0xE220A8397B1DCDAF
    assert M.splitmix64_int(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4


def test_splitmix64_array_equals_python_ints():
    rng = np.random.default_rng(1)
    z = np.concatenate([rng.integers(0, 1 << 64, 2000, dtype=np.uint64, endpoint=False),
                        np.array([0, 1, (1 << 63) - 1, 1 << 63, (1 << 63) + 1, (1 << 64) - 1, 0x61C8864680B583EB], dtype=np.uint64)])
    assert np.count_nonzero(z >= np.uint64(1 << 63)) > 500
    got = M.splitmix64(z)
    want = np.array([M.splitmix64_int(int(v)) for v in z], dtype=np.uint64)
    assert got.dtype == np.uint64 and np.array_equal(got, want)


def test_u01_is_the_top_53_bits():
    h = np.array([0, (1 << 11) - 1, 1 << 11, (1 << 64) - 1, 1 << 63], dtype=np.uint64)
    want = [0.0, 0.0, 2.0 ** -53, 1.0 - 2.0 ** -53, 0.5]
    assert M.u01(h).tolist() == want


# ------------------------------------------------------------------------------------------------
# random SPD matrix and right-hand side
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,seed", [(1, 0), (2, 1234), (7, 0), (97, 1234), (300, (1 << 64) - 1)])
def test_random_spd_model_is_symmetric_and_in_range(n, seed):
    cond = 50.0
    A = M.random_spd(n, seed, cond)
    assert A.shape == (n, n) and A.dtype == np.float64
    assert np.array_equal(M.bits(A), M.bits(A.T.copy()))
    off = A[~np.eye(n, dtype=bool)]
    inv_n = 1.0 / n
    assert np.all(off >= -inv_n) and np.all(off < inv_n)
    d = np.diag(A)
    assert np.all(d >= 1.0) and np.all(d < cond)
    if n >= 97:
        assert len(np.unique(off)) == n * (n - 1) // 2 and len(np.unique(d)) == n        # nothing is shared but the mirror image
    # a row block is the same block of the whole matrix (what a shard generates)
    rows = np.arange(n // 3, n)
    assert np.array_equal(M.random_spd_signed_uniform(n, seed, rows), M.random_spd_signed_uniform(n, seed)[n // 3:])


def test_random_spd_model_elements_from_python_ints():
    """A handful of elements restated with Python ints and fractions: `+` off the diagonal, `^` on it, lo * n + hi."""
    n, cond = 300, 3.0
    for seed in (0, 1234, (1 << 64) - 1):
        A = M.random_spd(n, seed, cond)
        for i, j in [(0, 1), (1, 0), (5, 299), (299, 5), (150, 151), (298, 299)]:
            lo, hi = min(i, j), max(i, j)
            h = M.splitmix64_int((seed + M.splitmix64_int(lo * n + hi)) & M.MASK64)
            t = Fraction(2 * (h >> 11), 1 << 53) - 1
            assert A[i, j] == float(t) * (1.0 / n)                   # float(t) is exact: a multiple of 2^-52 below 1
            assert Fraction(float(t)) == t
        for i in (0, 1, 299):
            h = M.splitmix64_int(seed ^ M.splitmix64_int(2 * i + 1))
            assert A[i, i] == float(1 + 2 * Fraction(h >> 11, 1 << 53))       # cond - 1 = 2: exact product, one rounding


def test_signed_uniform_is_exact():
    """2 u - 1 in fp64 equals the exact rational on a sample (so contraction into an fma cannot change it)."""
    t = M.random_spd_signed_uniform(64, 1234)
    u = (t + 1.0) / 2.0
    for x, y in zip(u.ravel()[::37], t.ravel()[::37]):
        assert Fraction(float(y)) == 2 * Fraction(float(x)) - 1
    b = M.random_rhs(500, 1235)
    assert np.all(b >= -1.0) and np.all(b < 1.0)
    for i in (0, 1, 499):
        h = M.splitmix64_int(1235 ^ M.splitmix64_int(0xB5 + i))
        assert Fraction(float(b[i])) == Fraction(2 * (h >> 11), 1 << 53) - 1


@pytest.mark.parametrize("cond", [1.0, 3.0, 1025.0])
def test_diagonal_candidates_agree_where_the_product_is_exact(cond):
    unfused, fused = M.random_spd_diagonals(4000, 1234, cond)
    assert np.array_equal(M.bits(unfused), M.bits(fused))
    if cond == 1.0:
        assert np.all(unfused == 1.0)


def test_diagonal_candidates_differ_at_cond_10():
    unfused, fused = M.random_spd_diagonals(4000, 1234, 10.0)
    ndiff = np.count_nonzero(unfused != fused)
    assert 0 < ndiff < 400, ndiff                         # a few per cent of the elements, each by one unit in the last place
    assert np.max(np.abs(unfused - fused)) <= 2.0 ** -49  # ulp of [8, 16)
    # fused is the correctly rounded exact value: never further from it than the unfused one
    u = M.random_spd_diagonal_uniform(4000, 1234)
    for i in np.flatnonzero(unfused != fused)[:20]:
        exact = 1 + 9 * Fraction(float(u[i]))
        assert abs(Fraction(float(fused[i])) - exact) <= abs(Fraction(float(unfused[i])) - exact)


def test_fp64_cond_10_tells_the_candidates_apart_at_the_gpu_sizes():
    """The GPU test's candidate rule is not vacuous: in fp64 at cond = 10, seed 1234, the two candidates are different vectors at
    the sizes it uses, so `both` cannot be its verdict there."""
    for n in (300, 1025, 1777, 2048):
        unfused, fused = M.random_spd_diagonals(n, 1234, 10.0)
        assert np.count_nonzero(unfused != fused) > 0, n


def test_storage_rounding():
    v = np.array([1.0, 1.0 + 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -50, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 0.1, -0.1])
    assert M.stored(v, "F64") is not None and np.array_equal(M.stored(v, "F64"), v)
    f32 = M.stored(v, "F32")
    assert f32.dtype == np.float32 and f32.tolist() == [1.0, 1.0, 1.0 + 2.0 ** -23, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8,
                                                        float(np.float32(0.1)), float(np.float32(-0.1))]
    bf = M.stored(v, "BF16")
    # ties to even: 1 + 2^-8 -> 1, 1 + 3 * 2^-8 -> 1 + 2^-6; 0.1 -> 0x3DCD0000
    assert bf.dtype == np.float32 and bf.tolist() == [1.0, 1.0, 1.0, 1.0, 1.0 + 2.0 ** -6, 0.10009765625, -0.10009765625]
    assert M.stored_vector([0.1], "BF16").dtype == np.float32 and M.stored_vector([0.1], "F64").dtype == np.float64


def _nearest_bf16_exact(v):
    """The bf16 number nearest to the Python float v (ties to even), as a float, by rational arithmetic; v in bf16's normal range."""
    import math
    x = Fraction(v)
    e = math.floor(math.log2(abs(v)))
    if Fraction(2) ** e > abs(x):
        e -= 1
    ulp = Fraction(2) ** (e - 7)                          # 8 significant bits
    q, r = divmod(abs(x), ulp)
    if r > ulp / 2 or (r == ulp / 2 and q % 2 == 1):
        q += 1
    return float((-1 if v < 0 else 1) * q * ulp)


def test_bf16_rounded_once_is_the_nearest_bf16_of_the_fp64_value():
    """stored(..., "once") against exact arithmetic: on random values, on fp64 values a hair either side of a bf16 tie (where fp32
    lands ON the tie and the two roundings part), on exact ties and exact bf16 / fp32 values, both signs."""
    rng = np.random.default_rng(7)
    # fp32 numbers exactly half way between two bf16 numbers: even below, odd below, small, and one that carries into 2.0
    ties = np.array([0x3F808000, 0x3F818000, 0x3B368000, 0x3FFF8000], dtype=np.uint32).view(np.float32).astype(np.float64)
    near = np.concatenate([ties * (1 + s * 2.0 ** -40) for s in (-1, 0, 1)])
    v = np.concatenate([rng.uniform(-1, 1, 3000) / 300, 1 + 49 * rng.uniform(0, 1, 1000), near, -near, [0.0, 1.0, 0.1, 1.0 + 2.0 ** -23]])
    once, twice = M.stored(v, "BF16", "once"), M.stored(v, "BF16", "twice")
    want = np.array([_nearest_bf16_exact(float(x)) if x != 0 else 0.0 for x in v], dtype=np.float32)
    assert np.array_equal(M.bits(once), M.bits(want))
    # the two roundings are different laws: of the 16 probes a hair off a tie (4 ties, 2 sides, 2 signs) fp32 puts every one ON the
    # tie, and the 8 on the side away from the even neighbour come out differently; on the ties themselves and elsewhere they agree
    assert np.count_nonzero(once[4000:] != twice[4000:]) == 8
    assert np.count_nonzero(once[:4000] != twice[:4000]) < 4


def test_row_pitch_and_partition():
    assert [M.row_pitch(n, 8) for n in (1, 2, 3, 7, 300, 511, 512, 513, 1024, 1025, 1777, 2048)] == \
        [2, 2, 4, 8, 300, 512, 512, 1024, 1024, 1536, 2048, 2048]
    assert [M.row_pitch(n, 4) for n in (1, 3, 300, 1023, 1024, 1025, 2048)] == [4, 4, 300, 1024, 1024, 2048, 2048]
    assert [M.row_pitch(n, 2) for n in (1, 7, 300, 1024, 1025, 1777, 2047, 2048, 2049)] == [8, 8, 304, 1024, 1032, 1784, 2048, 2048, 4096]
    assert M.partition(1777, 3) == [(0, 592), (592, 592), (1184, 593)]
    assert M.partition(3, 3) == [(0, 1), (1, 1), (2, 1)]


def test_tridiag_model():
    assert M.tridiag(1).tolist() == [[2.0]]
    assert M.tridiag(3).tolist() == [[2.0, 1.0, 0.0], [1.0, 2.0, 1.0], [0.0, 1.0, 2.0]]
    assert not np.signbit(M.tridiag(5)).any()


# ------------------------------------------------------------------------------------------------
# spectrum matrix
# ------------------------------------------------------------------------------------------------
def test_spectrum_model_equals_explicit_reflectors():
    """n = 64: the O(k n^2) longdouble recurrence equals Q diag(eig) Q^T with Q = H_k ... H_1 from explicit H matrices, has the
    prescribed eigenvalues, and a reversed reflector order is a DIFFERENT matrix by far more than the elementwise gates."""
    n, k = 64, 3
    eig, V = M.spectrum_inputs(n, k)
    A = M.spectrum_spd(eig, V)
    Q = M.householder_q(V)
    eps = float(np.finfo(np.longdouble).eps)
    assert np.max(np.abs(Q @ Q.T - np.eye(n))) <= 64 * n * eps
    want = (Q * eig.astype(np.longdouble)) @ Q.T
    assert float(np.max(np.abs(A - want))) <= 64 * n * eps * eig.max()
    assert np.max(np.abs(A - A.T)) <= 16 * eps * eig.max()
    w = np.linalg.eigvalsh(A.astype(np.float64))
    assert np.max(np.abs(w - np.sort(eig))) <= 1e-13 * eig.max()
    moved = float(np.max(np.abs(M.spectrum_spd(eig, V[::-1]) - A))) / eig.max()
    assert moved > 1e-4, moved
    assert np.array_equal(np.diag(M.spectrum_spd(eig, V[:0]).astype(np.float64)), eig)


@pytest.mark.parametrize("dtype_name", ["F64", "F32"])
@pytest.mark.parametrize("n,k", [(64, 1), (300, 4), (513, 3), (257, 6)])
def test_device_algorithm_stays_far_inside_the_gate(dtype_name, n, k):
    """The device's algorithm emulated in numpy in its working precision stays within 1 / 100 of the gate the GPU test sets on
    max |A_device - A_model| / max(eig) (measured: <= 2.1e-16 in fp64, <= 1.1e-7 in fp32): the gate leaves room for the product's
    summation order and for nothing else."""
    eig, V = M.spectrum_inputs(n, k)
    eig_up = M.spectrum_eig_as_uploaded(eig, dtype_name)
    model = M.spectrum_spd(eig_up, V)
    emu = M.spectrum_spd_emulated(eig_up, V, M.VEC_DTYPE[dtype_name])
    assert emu.dtype == M.VEC_DTYPE[dtype_name]
    assert np.array_equal(emu, emu.T)                     # separately rounded products: symmetric bit for bit
    err = float(np.max(np.abs(emu.astype(np.longdouble) - model))) / eig_up.max()
    print(f"emulated {dtype_name} n={n} k={k}: max |A_emu - A_model| / max(eig) = {err:.3g}")
    assert err <= M.SPECTRUM_GATE[dtype_name] / 100, err
