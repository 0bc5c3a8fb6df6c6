"""numpy model of lam_hip_solve_block (block CG for the batch: Dubrulle's BCGrQ with a Cholesky QR), stated in the kernels' operation
order: fp64 Gram sums, s x s matrices in fp64 by the statements of csrc/lam_host_block.h, coefficients rounded to the vector dtype
once, every row's sums as chains in ascending column index.  The reference project has no block solver: this model is the reference.
It does not reproduce the device's bits (the device fuses multiply-adds and sums its partials workgroup by workgroup); `order` permutes
the rows of the Gram sums, which is how tests/block_cg_data.py measures what such a difference can move."""
import math

import numpy as np

UNIT_ROUNDOFF = {np.float64: 2.0 ** -53, np.float32: 2.0 ** -24}
ORDERS = ("rows", "reversed", "shuffled")
MORE_ORDERS = ORDERS + tuple(f"shuffled{i}" for i in range(1, 6))     # eight: where three undersample what the order of a sum can move


# ------------------------------------------------------------------------------------------------
# csrc/lam_host_block.h, statement by statement (python floats are IEEE doubles)
# ------------------------------------------------------------------------------------------------
def pivot_floor(G, dtype):
    s = len(G)
    dmax = 0.0
    for i in range(s):
        if G[i][i] > dmax:
            dmax = float(G[i][i])
    return s * UNIT_ROUNDOFF[dtype] * dmax


def _pivot_fails(d, floor):
    return not math.isfinite(d) or not d > floor


def ldlt_inverse(G, floor):
    """(Ginv, bad): G = L D L^T, Ginv = L^-T D^-1 L^-1, upper triangle computed and mirrored.  bad = the column whose pivot failed
    (Ginv is then None), else -1.  Only the upper triangle of G is read."""
    s = len(G)
    G = [[float(v) for v in row] for row in G]
    L = [[0.0] * s for _ in range(s)]
    D = [0.0] * s
    for j in range(s):
        for i in range(j):
            t = G[i][j]
            for k in range(i):
                t -= L[j][k] * L[k][i]
            L[j][i] = t
            L[i][j] = t / D[i]
        d = G[j][j]
        for k in range(j):
            d -= L[k][j] * L[j][k]
        if _pivot_fails(d, floor):
            return None, j
        D[j] = d
    for c in range(s):
        for i in range(c + 1, s):
            t = L[c][i]
            for k in range(c + 1, i):
                t += L[k][i] * L[k][c]
            L[i][c] = -t
    Ginv = np.zeros((s, s))
    for i in range(s):
        for j in range(i, s):
            t = 0.0
            for k in range(j, s):
                mki = 1.0 if k == i else L[k][i]
                mkj = 1.0 if k == j else L[k][j]
                t += mki * mkj / D[k]
            Ginv[i, j] = Ginv[j, i] = t
    return Ginv, -1


def upper(G, floor):
    """(S, Sinv, bad): G = S^T S with S upper triangular, Sinv = S^-1; bad as in ldlt_inverse."""
    s = len(G)
    G = [[float(v) for v in row] for row in G]
    S = [[0.0] * s for _ in range(s)]
    Si = [[0.0] * s for _ in range(s)]
    for i in range(s):
        d = G[i][i]
        for k in range(i):
            d -= S[k][i] * S[k][i]
        if _pivot_fails(d, floor):
            return None, None, i
        r = math.sqrt(d)
        S[i][i] = r
        for j in range(i + 1, s):
            t = G[i][j]
            for k in range(i):
                t -= S[k][i] * S[k][j]
            S[i][j] = t / r
    for j in range(s):
        Si[j][j] = 1.0 / S[j][j]
        for i in range(j - 1, -1, -1):
            t = 0.0
            for k in range(i + 1, j + 1):
                t -= S[i][k] * Si[k][j]
            Si[i][j] = t / S[i][i]
    return np.array(S), np.array(Si), -1


# ------------------------------------------------------------------------------------------------
# the vector work
# ------------------------------------------------------------------------------------------------
def _row_order(n, order):
    if order == "rows":
        return slice(None)
    if order == "reversed":
        return slice(None, None, -1)
    assert order.startswith("shuffled"), order
    return np.random.default_rng(n + 1000 * int(order[8:] or 0)).permutation(n)


def gram(U, V, rows):
    """U^T V in fp64 with the rows summed in the order `rows`; the upper triangle, mirrored."""
    G = U[rows].astype(np.float64).T @ V[rows].astype(np.float64)
    return np.triu(G) + np.triu(G, 1).T


def _fma(a, b, c, dtype):
    """c + a * b rounded once to dtype where numpy can (fp32: the product is exact in fp64); fp64: two roundings."""
    if dtype is np.float32:
        return (c.astype(np.float64) + a.astype(np.float64) * np.float64(b)).astype(np.float32)
    return c + a * b


def chain(acc, M, C, dtype, lo=None, hi=None):
    """acc[:, j] = fma(M[:, l], C[l, j], acc[:, j]) for l ascending in lo(j) .. hi(j); C already holds values of dtype."""
    s = C.shape[0]
    out = acc.copy()
    for j in range(s):
        a = out[:, j]
        for l in range(lo(j) if lo else 0, hi(j) if hi else s):
            a = _fma(M[:, l], C[l, j], a, dtype)
        out[:, j] = a
    return out


def block_cg(apply_a, B, max_iters, rel_error, dtype=np.float64, order="rows"):
    """B: (s, n), row j = right-hand side j; apply_a(P) -> A P for an (n, s) array, in dtype.  Returns (X (s, n), info) with info:
    iters (completed iterations), num_iters (s: first iteration that met the test, max_iters + 1: never), converged (s), rel_err (s),
    breakdown (iteration, kind), refused (the column of the initial pivot failure, else -1)."""
    s, n = B.shape
    rows = _row_order(n, order)
    Bt = np.ascontiguousarray(B.T).astype(dtype)
    info = dict(iters=0, num_iters=np.full(s, max_iters + 1), converged=np.zeros(s, bool), rel_err=np.ones(s), breakdown=(0, 0),
                refused=-1)
    G = gram(Bt, Bt, rows)
    bb = np.diag(G).copy()
    C, Cinv, bad = upper(G, pivot_floor(G, dtype))
    if bad >= 0:
        info["refused"] = bad
        return None, info
    Q = chain(np.zeros((n, s), dtype), Bt, Cinv.astype(dtype), dtype, hi=lambda j: j + 1)
    P, X, Phi = Q.copy(), np.zeros((n, s), dtype), C
    first = np.zeros(s, int)
    for k in range(1, max_iters + 1):
        Z = apply_a(P).astype(dtype)
        H = gram(P, Z, rows)
        T, bad = ldlt_inverse(H, pivot_floor(H, dtype))
        if bad >= 0:
            info["breakdown"] = (k, 1)
            break
        X = chain(X, P, (T @ Phi).astype(dtype), dtype)
        Q = chain(Q, Z, (-T).astype(dtype), dtype)
        G = gram(Q, Q, rows)
        rr = np.array([Phi[:, j] @ (G @ Phi[:, j]) for j in range(s)])
        rel = np.sqrt(np.where(rr < 0.0, 0.0, rr) / bb)
        info["iters"], info["rel_err"] = k, rel
        hit = rel < rel_error
        first = np.where(hit & (first == 0), k, first)
        if hit.all():
            break
        S, Sinv, bad = upper(G, pivot_floor(G, dtype))
        if bad >= 0:
            info["breakdown"] = (k, 2)
            break
        Qn = chain(np.zeros((n, s), dtype), Q, Sinv.astype(dtype), dtype, hi=lambda j: j + 1)
        P = chain(Qn, P, S.T.astype(dtype), dtype, lo=lambda j: j)
        Q, Phi = Qn, S @ Phi
    info["num_iters"] = np.where(first != 0, first, max_iters + 1)
    info["converged"] = info["rel_err"] < rel_error
    return np.ascontiguousarray(X.T), info


def cg(apply_a, b, max_iters, rel_error, dtype=np.float64):
    """The batch's independent recurrence on one column (lam_hip_solve_many): x = 0, r = p = b, dots in fp64, the stop test
    sqrt(rr / bb) < rel_error in front of the p update.  Returns (x, num_iters) with max_iters + 1 at the cap."""
    b = b.astype(dtype)
    x, r, p = np.zeros_like(b), b.copy(), b.copy()
    dot = lambda u, v: float(u.astype(np.float64) @ v.astype(np.float64))
    bb = rr = dot(b, b)
    for k in range(1, max_iters + 1):
        ap = apply_a(p[:, None])[:, 0].astype(dtype)
        alpha = dtype(rr / dot(p, ap))
        x = x + alpha * p
        r = r - alpha * ap
        rr_new = dot(r, r)
        if math.sqrt(rr_new / bb) < rel_error:
            return x, k
        p = r + dtype(rr_new / rr) * p
        rr = rr_new
    return x, max_iters + 1


def true_residuals(apply_a64, X, B):
    """||b_j - A x_j|| / ||b_j|| per column, formed in fp64."""
    X64, B64 = X.astype(np.float64), B.astype(np.float64)
    R = B64 - apply_a64(np.ascontiguousarray(X64.T)).T
    return np.linalg.norm(R, axis=1) / np.linalg.norm(B64, axis=1)
