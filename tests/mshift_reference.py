"""numpy model of multi-shift CG as lam_hip_solve_mshift runs it (include/lam_hip.h): (A + s_j I) x_j = b for ONE b, the seed is the
plain recurrence of tests/pcg_reference.py on the smallest shift, and every other shift follows it through the collinearity
r_j = zeta_j r.  The operator is a callback, so tridiag(1,2,1) at N = 65537 costs O(N).  Scalars are fp64, vectors live in the vector
dtype, the seed's alpha and beta and each shift's three coefficients are rounded to it once per iteration, where the kernels do.
The device fuses where numpy rounds twice (x += c p, p = fma(zeta, r, c p), the seed product's s_min p): agreement is to rounding."""
import numpy as np

import pcg_reference as R

TINY = np.finfo(np.float64).tiny


def dense_operator(A, dtype):
    """p -> A p with A rounded to `dtype`, the product formed in it."""
    A = np.ascontiguousarray(A, dtype=dtype)
    return lambda p: A @ p


def tridiag_operator(dtype):
    """p -> tridiag(1,2,1) p (lam_hip_generate_tridiag), O(N)."""
    def apply(p):
        y = dtype(2) * p
        y[1:] += p[:-1]
        y[:-1] += p[1:]
        return y
    return apply


def ordered_operator(A, dtype, order):
    """p -> A p as pcg_reference.pcg_ordered forms it: rounded products summed in the vector dtype in the order `order`."""
    A = np.ascontiguousarray(A, dtype=dtype)
    return lambda p: R._sum_order(A * p[None, :], order)


def ordered_dot(order):
    return lambda x, y: np.float64(R._sum_order(x.astype(np.float64) * y.astype(np.float64), order))


def converged_shifts(S):
    """The 9 and the 64 shifts of the converged runs (tests/test_gpu_mshift.py, 4), spanning 0 ... 100 in no order: a zero (the seed),
    100, a duplicate of the zero among the 64, and the rest 100 * 2^(-j/4) (64) or 100 * 2^-j (9), scrambled by a fixed permutation."""
    assert S in (9, 64)
    v = np.r_[0.0, 100.0 * 2.0 ** (-np.arange(S - 1) / (4.0 if S == 64 else 1.0))]
    if S == 64:
        v[-1] = 0.0
    return v[np.random.default_rng(S).permutation(S)]


def converged_system(n, dtype):
    """(A, b) of the converged runs: Q exp(3.5 U[-1,1]) Q^T (pcg_reference.smoke_system(n, seed=n, spread=3.5); cond ~ e^7) in the
    storage type's values, b uniform in [-1, 1]."""
    A, rng = R.smoke_system(n, seed=n, spread=3.5)
    return A.astype(dtype).astype(np.float64), rng.uniform(-1, 1, n).astype(dtype)


# Largest |num_iters of the model - num_iters of per-shift model CG| on converged_system(513 / 1030) x converged_shifts(9 / 64), at
# rel_error 1e-10 (fp64) / 1e-5 (fp32), the model against the CG in the SAME summation order, for each of four orders (BLAS and
# pcg_reference.ORDERS: rows / reversed / lanes):
#     fp64  n = 513, S = 9: 0 in every order;  S = 64: 4 (BLAS), 2 / 2 / 2;   n = 1030, S = 9: 0;  S = 64: 2 (BLAS), 3 / 3 / 3
#     fp32  n = 513, S = 9: 0;                 S = 64: 3 (BLAS), 2 / 3 / 1;   n = 1030, S = 9: 0;  S = 64: 2 (BLAS), 2 / 2 / 2
# The GPU test gates |multi-shift - shifted batch| at twice the largest, 8 and 6.  (Across DIFFERENT orders of model and CG the
# figures are 6 and 4: that mixes the summation-order spread of plain CG itself into the figure and is not what is gated.)  In the
# same runs the host true residual of the model's x against max(the CG's, rel_error) reached 0.9998 (fp64) and 1.431 (fp32): the
# GPU test's factor 2 has room.  tests/test_mshift_cpu.py re-measures the BLAS pair and holds it to these figures.
MODEL_ITERS_DEVIATION = {"F64": 4, "F32": 3}
MODEL_TRUE_RATIO = {"F64": 0.9998, "F32": 1.431}


def mshift_cg(matvec, b, shifts, max_iters, rel_error, dtype=np.float64, dot=R._dot64, snapshots=False):
    """Returns (X, stats, history).  X: (S, n).  stats: num_iters, converged, rel_err (S entries each, with the library's meaning),
    frozen (the shifts whose zeta underflowed), seed (the slots that ARE the seed, d_j == 0).  history: one dict per iteration k the
    seed ran, with alpha, beta, rel (the seed's sqrt(rr/bb)), zeta (zeta_{k+1}; a frozen shift keeps its last), cx, cr, cp (rounded to
    the vector dtype), rel_err, live (took this step) and, with snapshots, X after the step."""
    b = np.ascontiguousarray(b, dtype=dtype).reshape(-1)
    n = b.size
    sh = np.array([np.float64(dtype(s)) for s in np.atleast_1d(shifts)])
    S = sh.size
    smin = sh.min()
    d = sh - smin
    seed = d == 0
    x = np.zeros(n, dtype=dtype)
    r = b.copy()
    p = b.copy()
    bb = dot(b, b)
    rr = bb
    XS = np.zeros((S, n), dtype=dtype)
    PS = np.tile(b, (S, 1))
    PS[seed] = 0
    z_prev, z_cur = np.ones(S), np.ones(S)
    a_prev, b_prev = np.float64(1.0), np.float64(0.0)
    live = ~seed
    stop, frozen = np.zeros(S, bool), np.zeros(S, bool)
    iters = np.zeros(S, int)
    rel = np.ones(S)
    seed_iters, seed_conv = 0, False
    history = []
    with np.errstate(all="ignore"):
        seed_rel = np.float64(np.sqrt(rr / bb))
        for k in range(1, max_iters + 1):
            Ap = matvec(p)
            if smin != 0:
                Ap = Ap + dtype(smin) * p
            alpha_d = np.float64(rr / dot(p, Ap))
            alpha = dtype(alpha_d)
            x = alpha * p + x
            r = -alpha * Ap + r
            rr_new = dot(r, r)
            beta_d = np.float64(rr_new / rr)
            seed_rel = np.float64(np.sqrt(rr_new / bb))
            seed_stop = bool(seed_rel < rel_error)
            if not seed_stop:
                p = r + dtype(beta_d) * p
            rr = rr_new
            seed_iters = k
            # the shifts, behind the seed's x, r and p
            z1 = z_cur * z_prev * a_prev / (alpha_d * b_prev * (z_prev - z_cur) + z_prev * a_prev * (1.0 + d * alpha_d))
            under = live & (np.abs(z1) < TINY)
            frozen |= under
            live = live & ~under
            ratio = z1 / z_cur
            re = z1 * seed_rel
            stp = re < rel_error
            cx, cr, cp = (alpha_d * ratio).astype(dtype), z1.astype(dtype), (beta_d * ratio * ratio).astype(dtype)
            took = live.copy()
            for j in np.flatnonzero(live):
                XS[j] = cx[j] * PS[j] + XS[j]
                if not stp[j]:
                    PS[j] = cr[j] * r + cp[j] * PS[j]
            rel = np.where(live, re, rel)
            iters = np.where(live, k, iters)
            z_prev, z_cur = np.where(live, z_cur, z_prev), np.where(live, z1, z_cur)
            stop |= live & stp
            live = live & ~stp
            a_prev, b_prev = alpha_d, beta_d
            h = dict(k=k, alpha=alpha_d, beta=beta_d, rel=seed_rel, zeta=z_cur.copy(), cx=cx, cr=cr, cp=cp, rel_err=rel.copy(), live=took)
            if snapshots:
                Xk = XS.copy()
                Xk[seed] = x
                h["X"] = Xk
            history.append(h)
            if seed_stop:
                seed_conv = True
                break
    XS[seed] = x
    seed_ni = seed_iters if seed_conv else max_iters + 1
    num_iters = np.where(seed, seed_ni, np.where(stop | frozen, iters, iters + 1))
    converged = np.where(seed, seed_conv, stop)
    rel_err = np.where(seed | (iters == 0), seed_rel, rel)
    return XS, dict(num_iters=num_iters, converged=converged, rel_err=rel_err, frozen=frozen, seed=seed), history
