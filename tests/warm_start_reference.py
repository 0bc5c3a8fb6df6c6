"""numpy restatement of lam_hip_solve_many_x0 (include/lam_hip.h): tests/pcg_reference.py's pcg() / pcg_ordered() started from a guess.

    x = x0, r = b - A x0 (the product and the subtraction rounded to the vector dtype), bb = b.b, rr = r.r, p = z = dinv o r, rz = r.z
    k = 0: sqrt(rr/bb) < rel_error -> the column is born stopped: num_iters = 0, converged, x = x0
    k = 1..max_iters: pcg()'s loop, statement for statement

bb = b.b stays the stop test's denominator.  With x0 = 0, A x0 = 0 and r = b - 0 = b exactly, so every later quantity is pcg()'s, bit
for bit, as long as rel_error <= 1 (a zero guess has sqrt(rr/bb) = 1).  max_iters = 0 returns the k = 0 state with pcg()'s "cap"
convention: num_iters = max_iters + 1 = 1 for a column that did not stop."""
import numpy as np

import pcg_reference as R


def pcg_x0(A, b, x0, max_iters, rel_error, dinv=None, dtype=np.float64, order=None):
    """Returns (x, stats): stats = num_iters, converged, rel_err as pcg(); rel_err_history[k] = sqrt(rr_k/bb) for k = 0 .. the last
    iteration run; x_absmax = the elementwise largest |x| over x0 and every iterate (for rounding bounds).
    A: the matrix, or a function v -> A v.  order=None: BLAS products and dots as pcg(); "rows" / "reversed" / "lanes": pcg_ordered()'s fixed summation orders."""
    b = np.ascontiguousarray(b, dtype=dtype).reshape(-1)
    n = b.size
    dinv = np.ones(n, dtype=dtype) if dinv is None else np.ascontiguousarray(dinv, dtype=dtype)
    if callable(A):          # a product given as a function of the vector (a stencil: no dense matrix at large n)
        dot = R._dot64

        def matvec(v):
            return np.asarray(A(v), dtype=dtype)
    elif order is None:
        A = np.ascontiguousarray(A, dtype=dtype)
        dot = R._dot64

        def matvec(v):
            return A @ v
    else:
        A = np.ascontiguousarray(A, dtype=dtype)

        def dot(x, y):
            return np.float64(R._sum_order(x.astype(np.float64) * y.astype(np.float64), order))

        def matvec(v):
            return R._sum_order(A * v[None, :], order)

    x = np.ascontiguousarray(x0, dtype=dtype).reshape(-1).copy()
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        r = b - matvec(x)
        z = dinv * r
        p = z.copy()
        bb = dot(b, b)
        rr = dot(r, r)
        rz = dot(r, z)
        hist = [float(np.sqrt(rr / bb))]
        absmax = np.abs(x)

        def done(k, conv):
            return x, dict(num_iters=k, converged=conv, rel_err=hist[-1], rel_err_history=hist, x_absmax=absmax)

        if np.sqrt(rr / bb) < rel_error:
            return done(0, True)
        for k in range(1, max_iters + 1):
            Ap = matvec(p)
            alpha = dtype(rz / dot(p, Ap))
            x = alpha * p + x
            absmax = np.maximum(absmax, np.abs(x))
            r = -alpha * Ap + r
            rr = dot(r, r)
            z = dinv * r
            rz_new = dot(r, z)
            hist.append(float(np.sqrt(rr / bb)))
            if np.sqrt(rr / bb) < rel_error:
                return done(k, True)
            beta = dtype(rz_new / rz)
            p = z + beta * p
            rz = rz_new
        return done(max_iters + 1, False)


def tridiag(n):
    """Dense tridiag(1, 2, 1): the device-side generator's matrix (lam_hip_generate_tridiag)."""
    return 2.0 * np.eye(n) + np.eye(n, k=1) + np.eye(n, k=-1)
