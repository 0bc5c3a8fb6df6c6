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
The host reference (fp64 BLAS on integer blocks) is therefore exact too."""
import numpy as np

MAX_EXACT_N_FP32 = (1 << 24) // 64 - 1          # 262143: 64 n < 2^24


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


def generate(n, sinks, vecs):
    """Stream the matrix through every `sink(row0, block)` and return A @ v for each v of `vecs` (exact: integer fp64 BLAS)."""
    assert n <= MAX_EXACT_N_FP32
    V = np.stack(vecs, axis=1) if vecs else np.zeros((n, 0))
    out = np.empty((n, V.shape[1]))
    step, keys = block_rows(n), _keys(n)
    for r0 in range(0, n, step):
        r1 = min(n, r0 + step)
        blk = int_block(r0, r1, n, keys)
        for sink in sinks:
            sink(r0, blk)
        out[r0:r1] = blk @ V
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
