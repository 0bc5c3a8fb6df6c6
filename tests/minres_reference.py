"""numpy restatement of the MINRES recurrence of lam_hip_solve_many_minres (include/lam_hip.h), statement for statement: scalars are
reduced and kept in fp64, vectors live in the vector dtype, the coefficients that multiply vectors (alpha, beta, eps_o, delta, phi
and the reciprocals 1 / beta1, 1 / gamma, 1 / beta') are rounded to it once per iteration, the product is A v with s v added per
element (the device's epilogue; A is never shifted).  The device fuses each multiply-add of the vector statements; numpy rounds
twice, which is inside what a change of summation order does (tests/test_minres_cpu.py measures the latter, and the gates are ten
times it).

order=None: BLAS products and dots.  order in pcg_reference.ORDERS: the loop-written product and the fp64 dot products summed in that
order (pcg_reference.pcg_ordered's: the same bits on every machine).  band=(lower, diag, upper): a tridiagonal matrix given by its
three diagonals, the product written per row; the order then says in which order a row's three products are added."""
import numpy as np

import pcg_reference as R


def tridiag_band(n, dtype=np.float64):
    """tridiag(1, 2, 1) as (lower, diag, upper), each of n entries; lower[0] and upper[n - 1] are zero."""
    lo, up = np.ones(n, dtype), np.ones(n, dtype)
    lo[0] = 0
    up[-1] = 0
    return lo, np.full(n, 2, dtype), up


def _band_product(band, v, order):
    lo, d, up = band
    z = np.zeros(1, v.dtype)
    a = lo * np.concatenate([z, v[:-1]])
    b = d * v
    c = up * np.concatenate([v[1:], z])
    if order == "reversed":
        return (c + b) + a
    if order == "lanes":
        return (a + c) + b
    return (a + b) + c


def minres(A, s, b, max_iters, rel_error, dtype=np.float64, order=None, band=None, history=None):
    """Returns (x, stats) with stats = num_iters (max_iters + 1 at the cap), converged, rel_err = phibar / beta1.
    history: a list that receives (k, x.copy(), rel_err) after every iteration."""
    dt = dtype
    b = np.ascontiguousarray(b, dtype=dt).reshape(-1)
    n = b.size
    s = dt(s)
    if band is None:
        A = np.ascontiguousarray(A, dtype=dt)
    else:
        band = tuple(np.ascontiguousarray(q, dtype=dt) for q in band)

    def dot(x, y):
        if order is None:
            return R._dot64(x, y)
        return np.float64(R._sum_order(x.astype(np.float64) * y.astype(np.float64), order))

    def product(v):
        if band is not None:
            Av = _band_product(band, v, order)
        elif order is None:
            Av = A @ v
        else:
            Av = R._sum_order(A * v[None, :], order)
        return s * v + Av

    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        bb = dot(b, b)
        beta1 = np.sqrt(bb)
        v = b * dt(1.0 / beta1)
        v_old, w, w_old, x = (np.zeros(n, dt) for _ in range(4))
        beta, cs, sn, dbar, eps, phibar = (np.float64(q) for q in (0.0, -1.0, 0.0, 0.0, 0.0, beta1))
        rel_err = phibar / beta1
        for k in range(1, max_iters + 1):
            u = product(v)
            alpha = dot(v, u)
            u = -dt(beta) * v_old + (-dt(alpha) * v + u)
            betan = np.sqrt(dot(u, u))
            eps_o = eps
            delta = cs * dbar + sn * alpha
            gbar = sn * dbar - cs * alpha
            eps = sn * betan
            dbar = -cs * betan
            gamma = np.hypot(gbar, betan)
            cs = gbar / gamma
            sn = betan / gamma
            phi = cs * phibar
            phibar = sn * phibar
            w_new = (-dt(delta) * w + (-dt(eps_o) * w_old + v)) * dt(1.0 / gamma)
            w_old = w
            w = w_new
            x = dt(phi) * w + x
            rel_err = phibar / beta1
            if history is not None:
                history.append((k, x.copy(), float(rel_err)))
            if rel_err < rel_error:
                return x, dict(num_iters=k, converged=True, rel_err=float(rel_err))
            v_old = v
            v = u * dt(1.0 / betan)
            beta = betan
        return x, dict(num_iters=max_iters + 1, converged=False, rel_err=float(rel_err))


def true_residual(A, s, x, b):
    """||b - (A + s I) x|| / ||b|| in fp64."""
    A64, x64, b64 = np.asarray(A, np.float64), np.asarray(x, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(b64 - A64 @ x64 - np.float64(s) * x64) / np.linalg.norm(b64))


def band_true_residual(band, s, x, b):
    x64, b64 = np.asarray(x, np.float64), np.asarray(b, np.float64)
    Ax = _band_product(tuple(np.asarray(q, np.float64) for q in band), x64, "rows")
    return float(np.linalg.norm(b64 - Ax - np.float64(s) * x64) / np.linalg.norm(b64))
