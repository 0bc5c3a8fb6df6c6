"""numpy restatement of the recurrence of lam_hip_eigs (include/lam_hip.h): Lanczos with full reorthogonalisation.  Vectors live in
the vector dtype, every scalar is fp64, the coefficients that multiply vectors (alpha, beta, every c_j, 1 / beta, 1 / ||v0||) are
rounded to the vector dtype once; two passes of classical Gram-Schmidt against v_0 .. v_k; T keeps the product's alpha_k = v_k.(A v_k)
and the beta_k behind the reorthogonalisation; the breakdown rule and the host's convergence test as the header states them.

`order` ("rows" / "reversed" / "lanes", pcg_reference.ORDERS) is the order of every sum -- the product's row sums in the vector dtype,
the fp64 dot products -- so that the model's own spread between orders can be measured (tests/lanczos_data.py)."""
import numpy as np

from pcg_reference import _sum_order

SMALLEST, LARGEST, BOTH = 0, 1, 2
UNIT_ROUNDOFF = {np.float64: 2.0 ** -53, np.float32: 2.0 ** -24}


def _fma(a, x, y):
    """a * x + y in the vector dtype.  fp32: through fp64, where the product is exact, so the one rounding of the device's fma but
    for rare double roundings; fp64: numpy has no fma, the product is rounded first."""
    if x.dtype == np.float32:
        return (np.float64(a) * x.astype(np.float64) + y.astype(np.float64)).astype(np.float32)
    return a * x + y


def wanted(which, nev, k, count):
    """Positions in the ascending spectrum of k values of the `count` pairs `which` asks for, in reporting order."""
    ns = count if which == SMALLEST else (0 if which == LARGEST else min((nev + 1) // 2, count))
    return list(range(ns)) + [k - 1 - (i - ns) for i in range(ns, count)]


def tridiag(alpha, beta):
    k = len(alpha)
    return np.diag(np.asarray(alpha, np.float64)) + np.diag(np.asarray(beta[:k - 1], np.float64), 1) + np.diag(np.asarray(beta[:k - 1], np.float64), -1)


def ritz(alpha, beta):
    """(theta ascending, S with S[:, i] eigenvector i) of T_k, k = len(alpha); beta[k - 1] is not part of T_k."""
    return np.linalg.eigh(tridiag(alpha, beta))


def lanczos(A, v0, max_steps, dtype=np.float64, order="rows", nev=1, which=SMALLEST, tol=0.0, check_every=8):
    """Returns a dict: alpha, beta (steps entries each), V (steps + 1 rows; steps rows after a breakdown), steps, broke, and the
    last check's theta / bound / converged for the wanted pairs (nfound entries), all_converged."""
    A = np.ascontiguousarray(A, dtype=dtype)
    n = A.shape[0]
    u_tv = UNIT_ROUNDOFF[dtype]

    def dot(x, y):
        return np.float64(_sum_order(x.astype(np.float64) * y.astype(np.float64), order))

    v0 = np.ascontiguousarray(v0, dtype=dtype).reshape(-1)
    nrm = np.sqrt(dot(v0, v0))
    assert np.isfinite(nrm) and nrm > 0
    V = [v0 * dtype(1.0 / nrm)]
    alpha, beta = [], []
    tmax = 0.0
    broke = False
    out = {}

    def check():
        k = len(alpha)
        theta, S = ritz(alpha, beta)
        norm = max(abs(theta[0]), abs(theta[-1]))
        nf = min(nev, k)
        idx = wanted(which, nev, k, nf)
        bound = np.array([beta[k - 1] * abs(S[k - 1, i]) for i in idx])
        conv = np.array([broke or b <= tol * norm for b in bound], bool)
        out.update(theta=theta[idx], bound=bound, converged=conv, nfound=nf, all_converged=bool(nf == nev and conv.all()), S=S[:, idx],
                   theta_all=theta)
        return broke or k >= max_steps or (tol > 0 and out["all_converged"])

    while True:
        k = len(alpha)
        vk = V[k]
        u = _sum_order(A * vk[None, :], order).astype(dtype)
        a = dot(vk, u)
        u = _fma(-dtype(a), vk, u)
        if k > 0:
            u = _fma(-dtype(beta[k - 1]), V[k - 1], u)
        for _ in range(2):
            c = [dot(V[j], u) for j in range(k + 1)]
            for j in range(k + 1):
                u = _fma(-dtype(c[j]), V[j], u)
        b = np.sqrt(dot(u, u))
        alpha.append(float(a))
        beta.append(float(b))
        tmax = max(tmax, abs(a) + (beta[k - 1] if k > 0 else 0.0) + b)
        broke = (not b > n * u_tv * tmax) or not np.isfinite(b)
        if not broke:
            V.append(u * dtype(1.0 / b))
        if broke or (k + 1) % check_every == 0 or k + 1 >= max_steps:
            if check():
                break
    out.update(alpha=np.array(alpha), beta=np.array(beta), V=np.array(V), steps=len(alpha), broke=broke)
    return out


def ritz_vectors(run):
    """Y (nfound, n) in fp64 from the run's basis and the wanted columns of T's eigenvector matrix."""
    k = run["steps"]
    return run["S"].T @ run["V"][:k].astype(np.float64)
