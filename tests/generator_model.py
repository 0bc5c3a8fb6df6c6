"""The laws of the device-side system generators, stated in numpy: what tests/test_gpu_generators.py holds the kernels to element
for element, itself checked without a GPU by tests/test_generator_model_cpu.py.  Written from the kernels (csrc/lam_kernels.h,
"generators"; lam_hip_generate_spectrum_spd in csrc/lam_hip.hip) and named by include/lam_hip.h as the statement of the law.

Hash and uniform (all index and hash arithmetic is 64-bit and WRAPS):
    sm(z)  = SplitMix64's output function of z (splitmix64 below)
    u01(h) = (h >> 11) * 2^-53                      53 random bits: exact in fp64, in [0, 1)

Random SPD matrix, by GLOBAL indices i, j with lo = min(i, j), hi = max(i, j):
    A[i][j] = (2 u01(sm(seed + sm(lo n + hi))) - 1) * fl(1 / n)       i != j    (`+`)
    A[i][i] = 1 + (cond - 1) u01(sm(seed ^ sm(2 i + 1)))                        (`^`)
  2 u - 1 is exact in fp64 (a multiple of 2^-52 of magnitude <= 1), so an off-diagonal element has ONE rounding, the product with
  fl(1 / n), whether or not the compiler contracts 2 u - 1 into an fma.  The diagonal has two candidates, because the compiler may
  or may not contract 1 + (cond - 1) u: unfused fl(1 + fl((cond - 1) u)) and fused fl(1 + (cond - 1) u); random_spd_diagonals
  returns both (the fused one exactly, in rational arithmetic).  They are the same number wherever (cond - 1) u is exact in fp64
  (cond = 1, 3, 1025: cond - 1 a power of two) and differ in some elements otherwise (cond = 10: about 3 % of them).

Right-hand sides:   b[i] = TV(2 u01(sm(seed ^ sm(0xB5 + i))) - 1), i the global row;  the constant one is TV(value).

Storage (`stored`): fp64 as computed; fp32 = that value rounded once; bf16, written `__float2bfloat16((float)v)` in the kernel,
has two candidates like the diagonal, returned as the fp32 number download_rows hands back:
    twice   the fp32 value rounded to nearest even (symmetry_data.bf16_rne_bits): fp64 -> fp32 -> bf16, two roundings;
    once    the fp64 value rounded to nearest even bf16 directly.  Both conversions carry the `contract` flag and the gfx950 backend
            merges them into this one correctly rounded step (fp64 -> fp32 round-to-odd -> bf16): what the MI355X build does.
  They differ where the fp32 value falls exactly on a bf16 tie and the fp64 value does not: about 2^-17 of the elements (8 per
  million).  The matrix an UPLOAD stores is rounded from the caller's fp32 either way.
TV, the vector type, is fp64 for fp64 storage and fp32 otherwise.

tridiag(1, 2, 1): 2 on the diagonal, 1 next to it, +0 elsewhere.

Spectrum matrix A = H_k ... H_1 diag(eig) H_1 ... H_k, H_j = I - tau_j v_j v_j^T, tau_j = 2 / v_j.v_j, in the O(k n^2) form the
device uses, per reflector   w = A v,  u = w - (tau v.w / 2) v,  A <- A - (tau v) u^T - u (tau v)^T   (spectrum_spd: np.longdouble,
the reference of the elementwise test; spectrum_spd_emulated: the same steps in one working precision with separately rounded
products, the device's arithmetic up to the summation order of w)."""
import functools
from fractions import Fraction

import numpy as np

from symmetry_data import bf16_rne_bits

MASK64 = (1 << 64) - 1
RHS_SALT = 0xB5
ESZ = {"F64": 8, "F32": 4, "BF16": 2}                       # bytes per stored matrix element
VEC_DTYPE = {"F64": np.float64, "F32": np.float32, "BF16": np.float32}
# max |A_device - A_model| <= gate * max(eig) for the spectrum matrix: the gates test_spectrum_generator_has_the_prescribed_spectrum
# (tests/test_gpu_parity.py) holds the eigenvalues to
SPECTRUM_GATE = {"F64": 1e-12, "F32": 2e-5}


# ------------------------------------------------------------------------------------------------
# hash, uniform
# ------------------------------------------------------------------------------------------------
def splitmix64(z):
    """SplitMix64's output function on np.uint64 arrays (or anything np.asarray turns into one), wrapping."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def splitmix64_int(z):
    """The same function on one Python int (arbitrary precision, masked): the array version's check."""
    z = (z + 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def u01(h):
    return (np.asarray(h, dtype=np.uint64) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def _seed(seed):
    return np.uint64(int(seed) & MASK64)


# ------------------------------------------------------------------------------------------------
# layout
# ------------------------------------------------------------------------------------------------
def row_pitch(n, esz):
    """Row pitch of the device matrix in elements of `esz` bytes: whole 4-KiB pages per row, whole 16-byte vectors when a row is
    shorter than a page."""
    align = 4096 // esz if n * esz >= 4096 else 16 // esz
    return -(-n // align) * align


def partition(n, shards):
    """[(row0, nrows)]: n // shards rows each, the remainder on the last shard."""
    base = n // shards
    return [(q * base, base + (n % shards if q == shards - 1 else 0)) for q in range(shards)]


# ------------------------------------------------------------------------------------------------
# random SPD matrix, right-hand sides, tridiag
# ------------------------------------------------------------------------------------------------
def random_spd_signed_uniform(n, seed, rows=None):
    """2 u - 1 of the off-diagonal law for rows `rows` (default all) x all columns, fp64, exact.  The diagonal positions hold the
    value the off-diagonal law would give there; random_spd overwrites them."""
    i = (np.arange(n, dtype=np.uint64) if rows is None else np.asarray(rows, dtype=np.uint64))[:, None]
    j = np.arange(n, dtype=np.uint64)[None, :]
    lo, hi = np.minimum(i, j), np.maximum(i, j)
    with np.errstate(over="ignore"):
        h = splitmix64(_seed(seed) + splitmix64(lo * np.uint64(n) + hi))
    return 2.0 * u01(h) - 1.0


def random_spd_diagonal_uniform(n, seed):
    i = np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return u01(splitmix64(_seed(seed) ^ splitmix64(i * np.uint64(2) + np.uint64(1))))


def random_spd_diagonals(n, seed, cond):
    """(unfused, fused): fl(1 + fl((cond - 1) u_i)) and fl(1 + (cond - 1) u_i) with cond - 1 rounded to fp64 first, as the kernel
    forms it.  float(Fraction) is correctly rounded (round to nearest even)."""
    u = random_spd_diagonal_uniform(n, seed)
    cm1 = np.float64(cond) - np.float64(1.0)
    unfused = 1.0 + cm1 * u
    c = Fraction(float(cm1))
    fused = np.array([float(1 + c * Fraction(float(x))) for x in u], dtype=np.float64)
    return unfused, fused


@functools.lru_cache(maxsize=3)
def _offdiag_cached(n, seed):
    a = random_spd_signed_uniform(n, seed) * (1.0 / np.float64(n))
    a.setflags(write=False)
    return a


def random_spd(n, seed, cond, fused=False):
    """The n x n matrix in fp64 with the unfused (default) or the fused diagonal."""
    a = _offdiag_cached(n, int(seed) & MASK64).copy()
    d = random_spd_diagonals(n, seed, cond)[1 if fused else 0]
    a[np.arange(n), np.arange(n)] = d
    return a


def random_rhs(n, seed):
    """fp64, exact (a multiple of 2^-52 in [-1, 1)); `stored_vector` takes it to the vector type."""
    i = np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return 2.0 * u01(splitmix64(_seed(seed) ^ splitmix64(np.uint64(RHS_SALT) + i))) - 1.0


def tridiag(n):
    a = np.zeros((n, n))
    i = np.arange(n)
    a[i, i] = 2.0
    a[i[:-1], i[:-1] + 1] = 1.0
    a[i[:-1] + 1, i[:-1]] = 1.0
    return a


# ------------------------------------------------------------------------------------------------
# storage
# ------------------------------------------------------------------------------------------------
BF16_ROUNDINGS = ("once", "twice")


def f32_round_to_odd_bits(a64):
    """fp32 bit patterns of fp64 values rounded TO ODD: the exact value where fp32 holds it, else the fp32 neighbour towards zero
    with its last bit set.  Rounding that to bf16 (to nearest even) is the single correct rounding of the fp64 value, because the
    sticky bit keeps apart what lies below, on and above a bf16 tie.  For zero and values in fp32's normal range (every value a
    generator produces)."""
    a64 = np.asarray(a64, dtype=np.float64)
    f = np.ascontiguousarray(a64.astype(np.float32))
    u = f.view(np.uint32).copy()
    f64 = f.astype(np.float64)
    inexact = f64 != a64
    assert np.all((u[inexact] & np.uint32(0x7F800000)) != 0) and np.all(np.isfinite(f)), "outside fp32's normal range"
    u[inexact & (np.abs(f64) > np.abs(a64))] -= np.uint32(1)        # sign-magnitude: one step towards zero
    u[inexact] |= np.uint32(1)
    return u


def stored(a64, dtype_name, bf16_rounding="twice"):
    """What download_rows returns for the fp64 value: float64 for F64, float32 for F32, the bf16 value as float32 for BF16
    (bf16_rounding: "twice" = fp64 -> fp32 -> bf16, "once" = fp64 -> bf16)."""
    a64 = np.asarray(a64, dtype=np.float64)
    if dtype_name == "F64":
        return a64
    a32 = np.ascontiguousarray(a64.astype(np.float32))
    if dtype_name == "F32":
        return a32
    assert dtype_name == "BF16" and bf16_rounding in BF16_ROUNDINGS
    u = a32.view(np.uint32) if bf16_rounding == "twice" else f32_round_to_odd_bits(a64)
    return bf16_rne_bits(u).view(np.float32).reshape(a32.shape)


def stored_vector(v64, dtype_name):
    """TV(v): the vector type is fp64 for fp64 storage, fp32 for fp32 and bf16 storage."""
    return np.asarray(v64, dtype=np.float64).astype(VEC_DTYPE[dtype_name])


def bits(a):
    """The bit patterns of a float64 / float32 array as unsigned integers."""
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


# ------------------------------------------------------------------------------------------------
# spectrum matrix
# ------------------------------------------------------------------------------------------------
def spectrum_inputs(n, k, seed=None):
    """eig = exp(3.5 U[-1, 1]) (n values), V = U[-1, 1] (k x n), seeded (default seed n + k)."""
    rng = np.random.default_rng(n + k if seed is None else seed)
    eig = np.exp(3.5 * rng.uniform(-1, 1, n))
    return eig, rng.uniform(-1, 1, (k, n))


def spectrum_eig_as_uploaded(eig, dtype_name):
    """fp32 contexts upload eig rounded to fp32."""
    return np.asarray(eig, np.float64).astype(VEC_DTYPE[dtype_name]).astype(np.float64)


def spectrum_spd(eig, V, work=np.longdouble):
    """O(k n^2), no H is formed.  Reflectors are applied in the order of V's rows."""
    eig = np.asarray(eig, dtype=work)
    n = eig.size
    A = np.zeros((n, n), dtype=work)
    A[np.arange(n), np.arange(n)] = eig
    for v in np.asarray(V, dtype=work).reshape(-1, n):
        w = A @ v
        tau = work(2) / (v @ v)
        tv = tau * v
        u = w - (tau * (v @ w) / work(2)) * v
        A -= np.outer(tv, u) + np.outer(u, tv)
    return A


def spectrum_spd_emulated(eig, V, dtype):
    """The device's algorithm in ONE working precision `dtype` (np.float64 / np.float32): tv_i u_j and u_i tv_j rounded
    separately, then added, then subtracted from the element; w = A v in numpy's summation order."""
    eig = np.asarray(eig, dtype=dtype)
    n = eig.size
    A = np.zeros((n, n), dtype=dtype)
    A[np.arange(n), np.arange(n)] = eig
    for v in np.asarray(V, dtype=dtype).reshape(-1, n):
        w = A @ v
        tau = dtype(2) / (v @ v)
        tv = tau * v
        u = w - (dtype(0.5) * tau * (v @ w)) * v
        p1 = np.outer(tv, u)
        p2 = np.outer(u, tv)
        A = A - (p1 + p2)
    return A


def householder_q(V, work=np.longdouble):
    """Q = H_k ... H_2 H_1 from explicit H matrices, so that H_k ... H_1 D H_1 ... H_k = Q D Q^T.  Small n only."""
    V = np.asarray(V, dtype=work)
    n = V.shape[1]
    Q = np.eye(n, dtype=work)
    for v in V:
        Q = (np.eye(n, dtype=work) - (work(2) / (v @ v)) * np.outer(v, v)) @ Q
    return Q


def first_mismatches(got, want, limit=4):
    """'(row, column, got, want)' of the first few elements whose BIT PATTERNS differ, for assertion messages; '' if none."""
    got, want = np.asarray(got), np.asarray(want)
    bad = np.argwhere(bits(got).reshape(got.shape) != bits(want).reshape(want.shape))
    if bad.size == 0:
        return ""
    items = [f"({', '.join(map(str, ix))}: got {got[tuple(ix)]!r} want {want[tuple(ix)]!r})" for ix in bad[:limit]]
    return f"{len(bad)} of {got.size} elements differ, first " + " ".join(items)
