"""numpy restatement of the plain Lanczos recurrence of lam_hip_lanczos_many (include/lam_hip.h), statement for statement, of the law
of its generated probes and of the quadrature lam_hip_trace_quadrature takes from the coefficients.  Scalars are reduced and kept in
fp64, vectors live in the vector dtype, the coefficients that multiply vectors (alpha, beta and the reciprocals 1 / ||z||, 1 / beta)
are rounded to it once per step.  The device fuses each multiply-add of the vector statements; numpy rounds twice, which is inside
what a change of summation order does (tests/test_quadrature_cpu.py measures the latter, and the gates are ten times it).  No
reorthogonalisation and no basis: three vectors.

order=None: BLAS products and dots.  order in pcg_reference.ORDERS: the loop-written product and the fp64 dot products summed in that
order (the same bits on every machine)."""
import numpy as np

import pcg_reference as R
from generator_model import _seed, splitmix64
from lanczos_reference import UNIT_ROUNDOFF

PROBE_SALT = 0x51AC
LOG, INV, POW = 0, 1, 2              # include/lam_hip.h LAM_HIP_QUAD_*


def rademacher(seed, probe, n, dtype=np.float64):
    """Probe `probe` (the global index) of lam_hip_lanczos_many(z_host = NULL, seed): z[i] = 1 - 2 (h >> 63),
    h = sm(seed ^ sm(0x51AC + probe * n + i)) in wrapping uint64."""
    i = np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        h = splitmix64(_seed(seed) ^ splitmix64(np.uint64(PROBE_SALT) + np.uint64(probe) * np.uint64(n) + i))
    return (1.0 - 2.0 * (h >> np.uint64(63)).astype(np.float64)).astype(dtype)


def rademacher_probes(seed, nprobes, n, dtype=np.float64):
    return np.vstack([rademacher(seed, j, n, dtype) for j in range(nprobes)])


def lanczos_plain(A, z, steps, dtype=np.float64, order=None):
    """One probe.  Returns dict(alpha, beta: `steps` entries each, NaN past steps_run; steps_run; znorm2)."""
    dt = dtype
    A = np.ascontiguousarray(A, dtype=dt)
    z = np.ascontiguousarray(z, dtype=dt).reshape(-1)
    n = z.size
    scale = n * UNIT_ROUNDOFF[dt]

    def dot(x, y):
        if order is None:
            return R._dot64(x, y)
        return np.float64(R._sum_order(x.astype(np.float64) * y.astype(np.float64), order))

    def product(v):
        return A @ v if order is None else R._sum_order(A * v[None, :], order)

    alpha, beta = np.full(steps, np.nan), np.full(steps, np.nan)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        zz = dot(z, z)
        v = z * dt(1.0 / np.sqrt(zz))
        v_old = np.zeros(n, dt)
        b_prev, tmax, ran = np.float64(0.0), np.float64(0.0), 0
        for k in range(1, steps + 1):
            u = product(v)
            a = dot(v, u)
            u = -dt(b_prev) * v_old + (-dt(a) * v + u)
            b = np.sqrt(dot(u, u))
            alpha[k - 1], beta[k - 1], ran = a, b, k
            tmax = np.fmax(tmax, abs(a) + b_prev + b)
            if not (b > scale * tmax) or not np.isfinite(b):
                break
            v_old = v
            v = u * dt(1.0 / b)
            b_prev = b
    return dict(alpha=alpha, beta=beta, steps_run=ran, znorm2=float(zz))


def lanczos_many(A, Z, steps, dtype=np.float64, order=None):
    """Every row of Z on its own (a column is the column alone).  alpha, beta: (nprobes, steps)."""
    runs = [lanczos_plain(A, z, steps, dtype, order) for z in np.atleast_2d(Z)]
    return dict(alpha=np.vstack([r["alpha"] for r in runs]), beta=np.vstack([r["beta"] for r in runs]),
                steps_run=np.array([r["steps_run"] for r in runs], np.int32), znorm2=np.array([r["znorm2"] for r in runs]))


def apply_fn(fn, t, param=0):
    t = np.asarray(t, np.float64)
    if fn == LOG:
        return np.log(t)
    if fn == INV:
        return 1.0 / t
    assert fn == POW and int(param) == param and param >= 0
    return t ** int(param)


def tridiag(alpha, beta):
    k = len(alpha)
    return np.diag(np.asarray(alpha, np.float64)) + np.diag(np.asarray(beta, np.float64)[:k - 1], 1) + np.diag(np.asarray(beta, np.float64)[:k - 1], -1)


def gauss_quadrature(alpha, beta, fn, shifts=(0.0,), param=0):
    """e_1^T f(T + s I) e_1 for every s through numpy.linalg.eigh: nodes theta, weights the squared first components."""
    theta, S = np.linalg.eigh(tridiag(alpha, beta))
    w = S[0, :] ** 2
    return np.array([np.sum(w * apply_fn(fn, theta + np.float64(s), param)) for s in shifts])


def probe_quadrature(run, j, fn, shifts=(0.0,), param=0):
    """znorm2_j times the quadrature of probe j of a lanczos_many result over its steps_run."""
    k = int(run["steps_run"][j])
    return run["znorm2"][j] * gauss_quadrature(run["alpha"][j][:k], run["beta"][j][:k], fn, shifts, param)


def exact_forms(A, Z, fn, shifts=(0.0,), param=0):
    """z^T f(A + s I) z for every row z of Z and every s, from eigh of A in fp64: (nshifts, nprobes)."""
    lam, Q = np.linalg.eigh(np.asarray(A, np.float64))
    C = (np.atleast_2d(np.asarray(Z, np.float64)) @ Q) ** 2
    return np.array([C @ apply_fn(fn, lam + np.float64(s), param) for s in shifts])
