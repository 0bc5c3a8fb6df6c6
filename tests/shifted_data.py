"""Shifted systems (A + s_j I) x_j = b_j of lam_hip_set_shifts_many (include/lam_hip.h): the shifts, systems, right-hand sides and
host references that tests/test_gpu_shifted.py follows, and that tests/test_shifted_cpu.py establishes on the CPU.

The numpy restatement here, pcg_shifted, is tests/pcg_reference.py's pcg statement for statement with ONE change, the device's: the
product is A p with s p added per element (multi_gemv_kernel's epilogue does it in one fused multiply-add, numpy here in two
roundings), and Jacobi's dinv is 1 / ((double)A_ii + s) rounded to the vector dtype.  The GPU tests do not compare with it: they compare with the references the
unshifted batch is compared with (the oracle, pcg_reference.pcg_ordered) run on the matrix A + s I FORMED on the host.  The
restatement only shows, on the CPU, that the two statements of the problem agree far inside the gates."""
import functools

import numpy as np

import pcg_reference as R
from tracking_data import tracking_columns

# One shift per column of the tracked batch: zero (the unshifted column inside a shifted batch) and seven dyadic values over six
# octaves around the n = 384 system's spectrum (e^-3 ... e^3), each exact in fp32.
TRACKING_SHIFTS = (0.0, 0.03125, 0.0625, 0.125, 0.25, 0.5, 1.0, 2.0)

# Integer shifts of the exact tests, one per column, all different, {0, 1, 2, 4, 8} among them: |s p_i| <= 64 like every product of
# exact_data's rows.  5 is left out: exact_data's 1 x 1 matrix is [-5], and p.Ap of a first step on [0] is zero.
INT_SHIFTS = (1, 2, 0, 4, 8, 3, 7, 6)

# Columns of tracking_data.tracking_columns() that serve as the right-hand sides of columns 0..7, by tracking_data's rule: a
# candidate is kept for column j only if the oracle's own sensitivity to summation order on (A + TRACKING_SHIFTS[j] I, b) -- 1 thread
# against 4 / 8 threads and 3 emulated ranks, the worst of 10 runs -- stays at or below 0.3 of a TENTH of ITERATION_TRACKING_GATES
# at every tracked k.  In their own order (0 .. 7) columns 0 and 3 measured 0.39 and 0.31 and were moved to other shifts; with the
# assignment below the worst fractions of that tenth, columns 0..7, two rounds of 10 runs: 0.15, 0.27, 0.29, 0.22, 0.29, 0.12, 0.20,
# 0.13.  tests/test_shifted_cpu.py re-checks every column against the tenth.
SHIFTED_ROWS = (4, 1, 2, 7, 3, 5, 6, 0)


@functools.lru_cache(maxsize=None)
def shifted_tracking_columns():
    """(A, B, shifts): the n = 384 system, 8 right-hand sides and the 8 shifts; column j is (A + shifts[j] I) x = B[j]."""
    A, B = tracking_columns()
    return A, B[list(SHIFTED_ROWS)], np.array(TRACKING_SHIFTS)


def formed(A, s, dtype=np.float64):
    """A + s I formed on the host from the values the storage type holds: what the references are run on."""
    M = np.asarray(A).astype(dtype).astype(np.float64)
    return M + s * np.eye(M.shape[0])


def shifted_dinv(A, s, dtype=np.float64):
    """1 / ((double)A_ii + s) rounded to the vector dtype: shifted_dinv_kernel's value."""
    d = np.diag(np.asarray(A)).astype(dtype).astype(np.float64)
    with np.errstate(divide="ignore"):
        return (1.0 / (d + np.float64(dtype(s)))).astype(dtype)


def pcg_shifted(A, s, b, max_iters, rel_error, jacobi=False, dtype=np.float64):
    """pcg_reference.pcg with the product written as the device writes it: Ap = A p + s p, A never shifted.  Returns (x, stats)."""
    A = np.ascontiguousarray(A, dtype=dtype)
    b = np.ascontiguousarray(b, dtype=dtype).reshape(-1)
    n = b.size
    s = dtype(s)
    dinv = shifted_dinv(A, s, dtype) if jacobi else np.ones(n, dtype=dtype)
    dot = R._dot64
    x = np.zeros(n, dtype=dtype)
    r = b.copy()
    z = dinv * r
    p = z.copy()
    bb = dot(b, b)
    rz = dot(r, z)
    rr = bb
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in range(1, max_iters + 1):
            Ap = A @ p + s * p
            alpha = dtype(rz / dot(p, Ap))
            x = alpha * p + x
            r = -alpha * Ap + r
            rr = dot(r, r)
            z = dinv * r
            rz_new = dot(r, z)
            if np.sqrt(rr / bb) < rel_error:
                return x, dict(num_iters=k, converged=True, rel_err=float(np.sqrt(rr / bb)))
            beta = dtype(rz_new / rz)
            p = z + beta * p
            rz = rz_new
        return x, dict(num_iters=max_iters + 1, converged=False, rel_err=float(np.sqrt(rr / bb)))


def true_residual_bound(absA_x, b, s, x, n, u_tv):
    """Bound on |res_device - res_numpy| for res = ||b - (A + s I) x|| / ||b||, tests/test_gpu_warm_start.py's bound for the true
    residuals with the product one operation longer (the epilogue's fma): per row |fl((A + s I) x) - (A + s I) x| <= gamma_(n+3)
    ((|A| + s I)|x|), the subtraction adds u (|b| + (|A| + s I)|x|)(1 + gamma); numpy's fp64 side obeys the same law with 2^-53; the
    fp64 sums, the division and the square root add (n + 8) 2^-53 relative on each side.  absA_x = |A||x|.  Returns the bound
    divided by nothing: the caller adds 2 (n + 8) 2^-53 times its reference value."""
    u64 = 2.0 ** -53
    w = absA_x + s * np.abs(x)

    def gamma(m, v):
        return m * v / (1 - m * v)
    nb = np.linalg.norm(b)
    return sum(gamma(n + 3, v) * np.linalg.norm(w) + v * (1 + gamma(n + 3, v)) * np.linalg.norm(np.abs(b) + w) for v in (u_tv, u64)) / nb
