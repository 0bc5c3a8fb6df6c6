"""Dense integer systems whose GEMV and first CG step have exact answers (tests/test_gpu_exact.py, tests/tuning_cases.py).

A[i, j] = a hash of (min(i, j), max(i, j)) mapped onto [-8, 8]: dense, symmetric, deterministic, integers in [-8, 8]; x and b integers in [-8, 8].
Generated one row block at a time, so no N needs the full matrix in host memory.

Why the answers are exact:
  * every product A[i, j] x[j] is an integer of magnitude <= 64 and a row has n of them, so every partial sum of a row, summed in
    any order, is an integer of magnitude <= 64 n.  fp64 holds it exactly; fp32 (the accumulator of the fp32 and bf16-storage
    paths) holds it exactly while 64 n < 2^24, i.e. n <= 262143;
  * p.Ap with p = b: every term |b_i (A b)_i| <= 8 * 64 n, so p.Ap <= 512 n^2 (< 2^53 up to n ~ 4e6) and b.b <= 64 n are exact
    in the fp64 reductions whatever their order;
  * bf16 has 8 significant bits: every integer of magnitude <= 256 is exact, so bf16 storage holds the matrix as it is.
The host reference (fp64 BLAS on integer blocks) is therefore exact too.

With a power-of-two diagonal (generate(..., diag=d), d_i in {1, 2, 4, 8}: the first JACOBI step, first_pcg_step):
  * dinv_i = 1 / d_i and z0 = dinv o b are exact, z0 a multiple of 1/8 of magnitude <= 8; r.z = sum b_i^2 / d_i is a multiple of 1/8
    below 64 n;
  * every product A[i, j] z0[j] is a multiple of 1/8 of magnitude <= 64 (the diagonal's: d_i z0_i = b_i), so every partial sum of a
    row of A z0 is a multiple of 1/8 of magnitude <= 64 n, i.e. an integer <= 8 * 64 n in units of 1/8: fp64 holds it exactly; fp32
    while 8 * 64 n < 2^24, i.e. n <= 32767;
  * p.Ap with p = z0: multiples of 1/64, |z0_i (A z0)_i| <= 8 * 64 n, the sum <= 512 n^2: exact in fp64 in any order.
An integer vector x against the patched matrix stays under the first set of bounds (|d_i x_i| <= 64)."""
import numpy as np

MAX_EXACT_N_FP32 = (1 << 24) // 64 - 1          # 262143: 64 n < 2^24
MAX_EXACT_N_FP32_JACOBI = (1 << 24) // (8 * 64) - 1     # 32767: 8 * 64 n < 2^24 (A z0 in eighths)


def _keys(n):
    g = np.random.default_rng(0x5EED)
    return g.integers(0, 1 << 32, n, dtype=np.uint32), g.integers(0, 1 << 32, n, dtype=np.uint32)


def int_block(r0, r1, n, keys=None):
    """Rows [r0, r1) of the n x n integer matrix, as float64: entry (i, j) hashes (lo, hi) = (min(i, j), max(i, j)) through
    a[lo] + c[hi] (two random 32-bit key tables) and a 32-bit finaliser, then maps the top bits onto [-8, 8]."""
    a, c = keys if keys is not None else _keys(n)
    i = np.arange(r0, r1)[:, None]
    j = np.arange(n)[None, :]
    h = np.where(j >= i, a[r0:r1, None] + c[None, :], a[None, :] + c[r0:r1, None])     # uint32, wraps
    h *= np.uint32(0x85EBCA6B)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xC2B2AE35)
    h ^= h >> np.uint32(16)
    h >>= np.uint32(16)
    h *= np.uint32(17)
    h >>= np.uint32(16)                                  # floor(17 * top16 / 2^16): 0 ... 16
    return h.astype(np.float64) - 8.0


def int_vec(n, seed):
    return np.random.default_rng(seed).integers(-8, 9, n).astype(np.float64)


def block_rows(n, elems=1 << 24):
    return max(1, elems // max(n, 1))


def pow2_diagonal(n, seed):
    """d_i drawn from {1, 2, 4, 8}, no two neighbouring rows alike (a repeat is moved on to the next power, cyclically)."""
    e = np.random.default_rng(seed).integers(0, 4, n)
    for i in range(1, n):
        if e[i] == e[i - 1]:
            e[i] = (e[i] + 1) % 4
    return 2.0 ** e


def generate(n, sinks, vecs, diag=None):
    """Stream the matrix through every `sink(row0, block)` and return A @ v for each v of `vecs` (exact: integer fp64 BLAS).
    diag (optional, n values): the matrix's diagonal is replaced by it -- each block is patched before it reaches the sinks and the
    returned products are the unpatched ones corrected by (d_i - A_ii) v_i."""
    assert n <= MAX_EXACT_N_FP32
    V = np.stack(vecs, axis=1) if vecs else np.zeros((n, 0))
    out = np.empty((n, V.shape[1]))
    step, keys = block_rows(n), _keys(n)
    for r0 in range(0, n, step):
        r1 = min(n, r0 + step)
        blk = int_block(r0, r1, n, keys)
        out[r0:r1] = blk @ V
        if diag is not None:
            i = np.arange(r1 - r0)
            out[r0:r1] += (diag[r0:r1] - blk[i, r0 + i])[:, None] * V[r0:r1]
            blk[i, r0 + i] = diag[r0:r1]
        for sink in sinks:
            sink(r0, blk)
    return [out[:, k] for k in range(V.shape[1])]


def first_cg_step(b, Ab, vec_dtype):
    """The first CG step from x = 0, r = p = b, as the kernels compute it:  alpha = fl64(b.b / b.Ab) (both exact integers), rounded
    once to the vector type (update_xr_kernel and its fused variants: `(TV)(rr / pAp)`), x1 = fl(alpha_TV * b) (x = alpha p + x
    with x = 0: one rounding).  Returns (alpha_TV, x1, bb, pAp, r1) with r1 = b - alpha_TV A b in fp64."""
    bi, Abi = b.astype(np.int64), Ab.astype(np.int64)
    bb, pAp = int((bi * bi).sum()), int((bi * Abi).sum())
    assert pAp != 0, "p.Ap = 0: the first step is undefined"
    assert abs(pAp) < 2 ** 53 and bb < 2 ** 53
    alpha = np.float64(bb) / np.float64(pAp)
    alpha_tv = vec_dtype(alpha)
    x1 = alpha_tv * b.astype(vec_dtype)                 # numpy: one correctly rounded multiply in vec_dtype
    r1 = b - np.float64(alpha_tv) * Ab
    return alpha_tv, x1, bb, pAp, r1


def first_pcg_step(b, d, Az, vec_dtype):
    """The first Jacobi-preconditioned step from x = 0 as multi_init_kernel / multi_xr_kernel compute it with PC = true, for integer b, a power-of-two
    diagonal d and Az = A z0 with z0 = b / d (exact):  alpha = fl64(r.z / p.Ap) with r.z = sum b_i z0_i and p.Ap = sum z0_i (A z0)_i
    both exact, rounded once to the vector type, x1 = fl(alpha_TV * z0).  Returns (alpha_TV, x1, bb, r1) with bb = b.b and
    r1 = b - alpha_TV A z0 in fp64."""
    assert np.all((d == 1) | (d == 2) | (d == 4) | (d == 8))
    z0 = b / d
    z8, Az8, bi = np.rint(8 * z0).astype(np.int64), np.rint(8 * Az).astype(np.int64), b.astype(np.int64)
    assert np.array_equal(z8 / 8.0, z0) and np.array_equal(Az8 / 8.0, Az), "z0 and A z0 are multiples of 1/8"
    bb, rz8, pAp64 = int((bi * bi).sum()), int((bi * z8).sum()), int((z8 * Az8).sum())
    assert pAp64 != 0, "p.Ap = 0: the first step is undefined"
    assert abs(pAp64) < 2 ** 53 and rz8 < 2 ** 53 and bb < 2 ** 53
    alpha = np.float64(rz8 / 8.0) / np.float64(pAp64 / 64.0)      # both operands exact in fp64: one correctly rounded division
    alpha_tv = vec_dtype(alpha)
    x1 = alpha_tv * z0.astype(vec_dtype)
    r1 = b - np.float64(alpha_tv) * Az
    return alpha_tv, x1, bb, r1


def tridiag_product(x):
    """y = tridiag(1, 2, 1) x for one vector or the rows of a 2-D array (the device-side generator's matrix)."""
    x = np.asarray(x, np.float64)
    y = 2.0 * x
    y[..., 1:] += x[..., :-1]
    y[..., :-1] += x[..., 1:]
    return y


def rel_err_bound(b, Ab, alpha_tv, r1, bb, u_tv):
    """Bound on |rel_err_device - sqrt(r1.r1 / b.b)| for the first step (sqrt(rr / bb) with rr = sum r_i^2 in fp64, any order).

    Per element the device forms r_i = -alpha A b_i + b_i in the vector type: with or without FMA contraction at most two roundings
    of relative size u_tv on terms bounded by |alpha A b_i| and |b_i|, so |r_dev_i - r_i| <= e_i = 2 u_tv (|alpha A b_i| + |b_i|)
    (1 + u_tv); the host's fp64 r1 errs by the same law with u = 2^-53, added to e_i.  Then |r_dev_i^2 - r1_i^2| <= e_i (2|r1_i| +
    e_i); each square is rounded once in fp64 and the n positive terms are summed in some order: relative error <= (n + 1) 2^-53
    on each side (device and host).  sqrt(S) moves by |dS| / (sqrt(S) + sqrt(S')) <= |dS| / sqrt(S) and the final sqrt and
    division add 2 ulp each side."""
    u = 2.0 ** -53
    n = b.size
    e = (2 * u_tv * (1 + u_tv) + 2 * u * (1 + u)) * (np.abs(np.float64(alpha_tv) * Ab) + np.abs(b))
    S = float(np.dot(r1, r1))
    dS = float(np.sum(e * (2 * np.abs(r1) + e))) + 2 * (n + 1) * u * S * (1 + 1e-6)
    re = np.sqrt(S / bb)
    return re, dS / np.sqrt(S) / np.sqrt(bb) + 8 * u * re
