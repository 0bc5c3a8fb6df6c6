"""numpy restatement of the Jacobi-preconditioned CG recurrence of lam_hip_solve_many_pc (include/lam_hip.h) and the badly scaled
test systems A = S M S.  Scalars are reduced and kept in fp64, vectors live in the vector dtype, alpha and beta are rounded to it,
the stop test is the plain recurrence's on sqrt(rr/bb).  With dinv = 1 this is the recurrence of lam_hip_solve."""
import functools

import numpy as np


def _dot64(x, y):
    return np.float64(np.dot(x.astype(np.float64), y.astype(np.float64)))      # np.float64: 0/0 is NaN, not an exception


def jacobi_dinv(A, dtype=np.float64):
    """1 / A_ii computed in fp64 from the stored value and rounded to the vector dtype."""
    d = np.diag(np.asarray(A)).astype(dtype)
    return (1.0 / d.astype(np.float64)).astype(dtype)


def pcg(A, b, max_iters, rel_error, dinv=None, dtype=np.float64, track=None):
    """Returns (x, stats) with stats = num_iters (max_iters + 1 at the cap), converged, rel_err = sqrt(rr/bb).
    dinv=None: no preconditioner (dinv = 1).  track: a dict whose keys are iteration numbers k; track[k] becomes (x, rel_err) as
    they stand after iteration k -- what the run capped at k returns, bit for bit, as long as the tolerance stops nothing."""
    A = np.ascontiguousarray(A, dtype=dtype)
    b = np.ascontiguousarray(b, dtype=dtype).reshape(-1)
    n = b.size
    dinv = np.ones(n, dtype=dtype) if dinv is None else np.ascontiguousarray(dinv, dtype=dtype)
    x = np.zeros(n, dtype=dtype)
    r = b.copy()
    z = dinv * r
    p = z.copy()
    bb = _dot64(b, b)
    rz = _dot64(r, z)
    rr = bb
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in range(1, max_iters + 1):
            Ap = A @ p
            alpha = dtype(rz / _dot64(p, Ap))
            x = alpha * p + x
            r = -alpha * Ap + r
            rr = _dot64(r, r)
            if track is not None and k in track:
                track[k] = (x.copy(), float(np.sqrt(rr / bb)))
            z = dinv * r
            rz_new = _dot64(r, z)
            if np.sqrt(rr / bb) < rel_error:
                return x, dict(num_iters=k, converged=True, rel_err=float(np.sqrt(rr / bb)))
            beta = dtype(rz_new / rz)
            p = z + beta * p
            rz = rz_new
        return x, dict(num_iters=max_iters + 1, converged=False, rel_err=float(np.sqrt(rr / bb)))


def smoke_system(n=512, seed=0, spread=2.0):
    """tests/test_gpu_multi_rhs.py::_smoke_system: Q exp(spread U[-1,1]) Q^T, symmetrised."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.uniform(-1, 1, (n, n)))
    A = (q * np.exp(spread * rng.uniform(-1, 1, n))) @ q.T
    return 0.5 * (A + A.T), rng


def sms_system(n=512, seed=0):
    """A = S M S: M the smoke system (spread 2.0), S = diag(2^round(log2(10) U[-3,3])) -- exact powers of two, so A is M's entries
    scaled exactly, symmetric bit for bit, in fp32 as in fp64.  cond(A) ~ 1e12 ... 1e13, cond(D^-1/2 A D^-1/2) ~ 50.
    Returns (A, rng) with the generator that drew M and S, for the right-hand sides."""
    M, rng = smoke_system(n, seed)
    s = 2.0 ** np.round(np.log2(10.0) * rng.uniform(-3, 3, n))
    return s[:, None] * M * s[None, :], rng


def true_residual(A, x, b):
    A64, x64, b64 = np.asarray(A, np.float64), np.asarray(x, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(b64 - A64 @ x64) / np.linalg.norm(b64))


# ------------------------------------------------------------------------------------------------
# the scaling identity of tests/test_gpu_batch_recurrence.py (A): C with a unit diagonal, A = S C S with S = diag(2^e)
# ------------------------------------------------------------------------------------------------
def unit_diagonal_system(n, dtype=np.float64, seed=0):
    """C = D^-1/2 M D^-1/2 of the smoke system M, rounded to `dtype`, the upper triangle mirrored onto the lower one and the diagonal
    set to exactly 1: symmetric bit for bit, and Jacobi's dinv on it is exactly 1.  Returns (C as float64 holding dtype's values, rng)."""
    C64, state = _smoke_system_normalised(n, seed)
    rng = np.random.default_rng()
    rng.bit_generator.state = state
    C = C64.astype(dtype).astype(np.float64)
    C = np.triu(C, 1)
    C = C + C.T
    C[np.arange(n), np.arange(n)] = 1.0
    return C, rng


@functools.lru_cache(maxsize=2)
def _smoke_system_normalised(n, seed):
    """M_ij / sqrt(M_ii M_jj) in fp64 and the state of the generator that drew M (shared by the storage types: the QR is the cost)."""
    M, rng = smoke_system(n, seed)
    d = np.sqrt(np.diag(M))
    return M / d[:, None] / d[None, :], rng.bit_generator.state


def varying_exponents(n, rng, lo=-6, hi=6):
    """Integer exponents in [lo, hi], no two neighbouring rows alike (a repeat is moved on by one, cyclically)."""
    span = hi - lo + 1
    e = rng.integers(0, span, n)
    for i in range(1, n):
        if e[i] == e[i - 1]:
            e[i] = (e[i] + 1) % span
    return e + lo


def scale_system(C, e):
    """A = S C S with S = diag(2^e): every entry is C's scaled exactly, A_ii = 4^e_i C_ii.  Returns (A, s = 2^e)."""
    s = 2.0 ** np.asarray(e, np.float64)
    return s[:, None] * C * s[None, :], s


# ------------------------------------------------------------------------------------------------
# the recurrence with its sums taken in another order: the reference's own spread (tests/test_gpu_batch_recurrence.py, C)
# ------------------------------------------------------------------------------------------------
ORDERS = ("rows", "reversed", "lanes")


def _sum_order(T, order):
    """Sum the last axis of T in T's dtype: numpy's pairwise order, the same over the reversed axis, or 64 strided partial sums
    (what 64 lanes would keep) added up at the end."""
    if order == "rows":
        return T.sum(axis=-1, dtype=T.dtype)
    if order == "reversed":
        return np.ascontiguousarray(T[..., ::-1]).sum(axis=-1, dtype=T.dtype)
    assert order == "lanes", order
    n = T.shape[-1]
    pad = (-n) % 64
    if pad:
        T = np.concatenate([T, np.zeros(T.shape[:-1] + (pad,), T.dtype)], axis=-1)
    lanes = T.reshape(T.shape[:-1] + (-1, 64)).sum(axis=-2, dtype=T.dtype)
    return lanes.sum(axis=-1, dtype=T.dtype)


def pcg_ordered(A, b, max_iters, rel_error, dinv=None, dtype=np.float64, order="rows", track=None):
    """pcg() statement for statement, with A @ p formed as rounded products summed in the vector dtype in the order `order` (no
    BLAS: the same bits on every machine) and the fp64 dot products summed in that order too.  track: as in pcg()."""
    A = np.ascontiguousarray(A, dtype=dtype)
    b = np.ascontiguousarray(b, dtype=dtype).reshape(-1)
    n = b.size
    dinv = np.ones(n, dtype=dtype) if dinv is None else np.ascontiguousarray(dinv, dtype=dtype)

    def dot(x, y):
        return np.float64(_sum_order(x.astype(np.float64) * y.astype(np.float64), order))

    x = np.zeros(n, dtype=dtype)
    r = b.copy()
    z = dinv * r
    p = z.copy()
    bb = dot(b, b)
    rz = dot(r, z)
    rr = bb
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in range(1, max_iters + 1):
            Ap = _sum_order(A * p[None, :], order)
            alpha = dtype(rz / dot(p, Ap))
            x = alpha * p + x
            r = -alpha * Ap + r
            rr = dot(r, r)
            if track is not None and k in track:
                track[k] = (x.copy(), float(np.sqrt(rr / bb)))
            z = dinv * r
            rz_new = dot(r, z)
            if np.sqrt(rr / bb) < rel_error:
                return x, dict(num_iters=k, converged=True, rel_err=float(np.sqrt(rr / bb)))
            beta = dtype(rz_new / rz)
            p = z + beta * p
            rz = rz_new
        return x, dict(num_iters=max_iters + 1, converged=False, rel_err=float(np.sqrt(rr / bb)))
