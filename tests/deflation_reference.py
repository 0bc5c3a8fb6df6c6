"""numpy restatement of the deflated batch (include/lam_hip.h: lam_hip_set_deflation*, lam_hip_solve_many_deflated,
lam_hip_deflate_many), one column at a time.  Vectors live in the vector dtype, every scalar is fp64, the coefficients that multiply
vectors (alpha, beta, every mu_i) are rounded to the vector dtype once.

`order` ("rows" / "reversed" / "lanes", pcg_reference.ORDERS) is the order of every sum -- the product's row sums in the vector dtype,
the fp64 dot products, the m-term sums of mu = Ginv d -- so that the model's own spread between orders can be measured
(tests/deflation_data.py)."""
import numpy as np

from lanczos_reference import _fma
from pcg_reference import _sum_order


def chol_inverse(G):
    """csrc/lam_host_chol.h statement for statement (G = L D L^T in fp64, ascending sums, only the lower triangle read), without its pivot floor:
    returns Ginv, or raises ValueError naming the column whose pivot is not finite and > 0."""
    G = np.asarray(G, np.float64)
    m = G.shape[0]
    L, Li, Ginv, D, T = np.zeros((m, m)), np.zeros((m, m)), np.zeros((m, m)), np.zeros(m), np.zeros(m)
    for j in range(m):
        for i in range(j):
            s = G[j, i]
            for k in range(i):
                s -= T[k] * L[i, k]
            T[i] = s
            L[j, i] = s / D[i]
        d = G[j, j]
        for k in range(j):
            d -= L[j, k] * T[k]
        if not (d > 0 and np.isfinite(d)):
            raise ValueError(f"pivot of column {j} is {d}")
        D[j] = d
        L[j, j] = 1.0
    for c in range(m):
        Li[c, c] = 1.0
        for i in range(c + 1, m):
            s = 0.0
            for k in range(c, i):
                s -= L[i, k] * Li[k, c]
            Li[i, c] = s
    for i in range(m):
        for j in range(i + 1):
            s = 0.0
            for k in range(i, m):
                s += Li[k, i] * Li[k, j] / D[k]
            Ginv[i, j] = Ginv[j, i] = s
    return Ginv


def _dot(x, y, order):
    return np.float64(_sum_order(x.astype(np.float64) * y.astype(np.float64), order))


def _product(A, p, order):
    return _sum_order(A * p[None, :], order).astype(A.dtype)


def space(A, W, dtype=np.float64, order="rows"):
    """What lam_hip_set_deflation builds: W and A W in the vector dtype, G = W^T (A W) from fp64 sums, symmetrised, and its inverse."""
    A = np.ascontiguousarray(A, dtype=dtype)
    W = np.ascontiguousarray(np.atleast_2d(W), dtype=dtype)
    AW = np.array([_product(A, w, order) for w in W])
    G = np.array([[_dot(wi, awj, order) for awj in AW] for wi in W])
    G = 0.5 * (G + G.T)
    return dict(W=W, AW=AW, G=G, Ginv=chol_inverse(G))


def _mu(Ginv, d, order):
    return _sum_order(Ginv * np.asarray(d, np.float64)[None, :], order)


def operator(Wd, Wa, M, u, dtype=np.float64, order="rows"):
    """lam_hip_deflate_many on one column: (coeff = Wd u, u - Wa (M coeff)) with the fma chain in ascending i."""
    u = np.ascontiguousarray(u, dtype=dtype)
    coeff = np.array([_dot(w, u, order) for w in Wd])
    mu = _mu(np.asarray(M, np.float64), coeff, order)
    with np.errstate(invalid="ignore", over="ignore"):
        for i, w in enumerate(Wa):
            u = _fma(-dtype(mu[i]), w, u)
    return coeff, u


def deflated_cg(A, sp, b, max_iters, rel_error, dtype=np.float64, order="rows", track=None):
    """The recurrence of lam_hip_solve_many_deflated on one right-hand side; sp: space().  Returns (x, stats) with stats = num_iters
    (max_iters + 1 at the cap), converged, rel_err = sqrt(rr/bb).  track: a dict whose keys are iteration numbers k (0: the start);
    track[k] becomes (x, rel_err) as they stand after iteration k -- what the run capped at k returns, as long as the tolerance stops
    nothing."""
    A = np.ascontiguousarray(A, dtype=dtype)
    b = np.ascontiguousarray(b, dtype=dtype).reshape(-1)
    W, AW, Ginv = sp["W"], sp["AW"], sp["Ginv"]
    m = W.shape[0]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        mu = _mu(Ginv, [_dot(W[i], b, order) for i in range(m)], order)
        x = np.zeros(b.size, dtype)
        for i in range(m):
            x = _fma(dtype(mu[i]), W[i], x)
        r = b - _product(A, x, order)
        bb, rr = _dot(b, b, order), _dot(r, r, order)
        if track is not None and 0 in track:
            track[0] = (x.copy(), float(np.sqrt(rr / bb)))
        if np.sqrt(rr / bb) < rel_error:
            return x, dict(num_iters=0, converged=True, rel_err=float(np.sqrt(rr / bb)))

        def project(p):
            mu = _mu(Ginv, [_dot(AW[i], r, order) for i in range(m)], order)
            for i in range(m):
                p = _fma(-dtype(mu[i]), W[i], p)
            return p

        p = project(r.copy())
        for k in range(1, max_iters + 1):
            Ap = _product(A, p, order)
            alpha = dtype(rr / _dot(p, Ap, order))
            x = alpha * p + x
            r = -alpha * Ap + r
            rr_new = _dot(r, r, order)
            if track is not None and k in track:
                track[k] = (x.copy(), float(np.sqrt(rr_new / bb)))
            if np.sqrt(rr_new / bb) < rel_error:
                return x, dict(num_iters=k, converged=True, rel_err=float(np.sqrt(rr_new / bb)))
            beta = dtype(rr_new / rr)
            p = project(r + beta * p)
            rr = rr_new
        return x, dict(num_iters=max_iters + 1, converged=False, rel_err=float(np.sqrt(rr / bb)))
