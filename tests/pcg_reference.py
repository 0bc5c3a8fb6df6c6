"""numpy restatement of the Jacobi-preconditioned CG recurrence of lam_hip_solve_many_pc (include/lam_hip.h) and the badly scaled
test systems A = S M S.  Scalars are reduced and kept in fp64, vectors live in the vector dtype, alpha and beta are rounded to it,
the stop test is the plain recurrence's on sqrt(rr/bb).  With dinv = 1 this is the recurrence of lam_hip_solve."""
import numpy as np


def _dot64(x, y):
    return np.float64(np.dot(x.astype(np.float64), y.astype(np.float64)))      # np.float64: 0/0 is NaN, not an exception


def jacobi_dinv(A, dtype=np.float64):
    """1 / A_ii computed in fp64 from the stored value and rounded to the vector dtype."""
    d = np.diag(np.asarray(A)).astype(dtype)
    return (1.0 / d.astype(np.float64)).astype(dtype)


def pcg(A, b, max_iters, rel_error, dinv=None, dtype=np.float64):
    """Returns (x, stats) with stats = num_iters (max_iters + 1 at the cap), converged, rel_err = sqrt(rr/bb).
    dinv=None: no preconditioner (dinv = 1)."""
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
