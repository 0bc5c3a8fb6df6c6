"""Systems and gates of the deflated batch's tests (tests/test_deflation_cpu.py establishes them on the CPU, tests/test_gpu_deflation.py
follows them on the device): lam_hip_set_deflation*, lam_hip_solve_many_deflated, lam_hip_deflate_many, lam_hip_chol_inverse."""
import functools

import numpy as np

import deflation_reference as R
import lanczos_data as LD
import lanczos_reference as L
import pcg_reference as P
from pcg_reference import ORDERS

DTYPES = LD.DTYPES

# ------------------------------------------------------------------------------------------------
# lam_hip_chol_inverse against numpy.linalg.inv
# ------------------------------------------------------------------------------------------------
CHOL_SIZES = (1, 7, 32)


def chol_case(m):
    """A random SPD G of size m: X X^T + m I with X uniform in [-1, 1) -- cond below 4 for every m here."""
    X = np.random.default_rng(50 + m).uniform(-1, 1, (m, m))
    return X @ X.T + m * np.eye(m)


def measure_chol_margin(m):
    """max |inv(G) - inv_longdouble(G)| / max |inv_longdouble(G)| of numpy.linalg.inv in fp64 against the same inverse formed in
    np.longdouble (Gauss-Jordan without pivoting, which an SPD matrix does not need): numpy's own error, nothing of the library."""
    G = chol_case(m)
    ref = _inv_longdouble(G)
    return float(np.abs(np.linalg.inv(G) - ref).max() / np.abs(ref).max())


def _inv_longdouble(G):
    m = G.shape[0]
    M = np.concatenate([np.asarray(G, np.longdouble), np.eye(m, dtype=np.longdouble)], axis=1)
    for j in range(m):
        M[j] = M[j] / M[j, j]
        for i in range(m):
            if i != j:
                M[i] = M[i] - M[i, j] * M[j]
    return M[:, m:]


# Gate of max |Ginv - numpy.linalg.inv(G)| / max |inv(G)|: 10 x numpy's own error against the longdouble inverse.  Measured:
#     m = 1: 2.80e-17     m = 7: 3.31e-16     m = 32: 5.78e-16
CHOL_GATE = {1: 2.8e-16, 7: 3.4e-15, 32: 5.8e-15}

# ------------------------------------------------------------------------------------------------
# recurrence parity: the parity systems of lanczos_data, a random W, 8 columns
# ------------------------------------------------------------------------------------------------
PARITY_SIZES = LD.PARITY_SIZES
PARITY_K = (1, 2, 5, 20)             # runs capped at max_iters = k
PARITY_M = 3
PARITY_M_LARGE = (384, 32)           # the one run with m = LAM_HIP_MAX_DEFLATION: at this size
PARITY_NRHS = 8


@functools.lru_cache(maxsize=None)
def parity_inputs(n, m):
    """(B (8, n), W (m, n)), uniform in [-1, 1), read-only."""
    rng = np.random.default_rng(31 * n + m)
    B, W = rng.uniform(-1, 1, (PARITY_NRHS, n)), rng.uniform(-1, 1, (m, n))
    B.setflags(write=False)
    W.setflags(write=False)
    return B, W


@functools.lru_cache(maxsize=None)
def parity_model(n, dtype_name, m, order="rows"):
    """{k: (X (8, n), rel_err (8))} of the model on the parity system, every column, every k of PARITY_K."""
    dtype = DTYPES[dtype_name]
    A = LD.parity_matrix(n, dtype_name)
    B, W = parity_inputs(n, m)
    sp = R.space(A, W, dtype, order)
    out = {k: ([], []) for k in PARITY_K}
    for b in B:
        track = {k: None for k in PARITY_K}
        R.deflated_cg(A, sp, b, max(PARITY_K), 0.0, dtype, order, track)
        for k in PARITY_K:
            out[k][0].append(track[k][0])
            out[k][1].append(track[k][1])
    return {k: (np.array(v[0]), np.array(v[1])) for k, v in out.items()}


def measure_parity_spreads(n, dtype_name, m):
    """{k: (largest relative spread of rel_err, of x in the 2-norm)} between the model's three sum orders, over the 8 columns."""
    runs = [parity_model(n, dtype_name, m, o) for o in ORDERS]
    out = {}
    for k in PARITY_K:
        s_re = s_x = 0.0
        for a in runs:
            for b in runs:
                xa, xb = a[k][0].astype(np.float64), b[k][0].astype(np.float64)
                s_re = max(s_re, float(np.abs(a[k][1] / b[k][1] - 1).max()))
                s_x = max(s_x, float((np.linalg.norm(xa - xb, axis=1) / np.linalg.norm(xb, axis=1)).max()))
        out[k] = (s_re, s_x)
    return out


# Relative gates of rel_err and of ||x - x_model|| / ||x_model|| of the run capped at k: 10 x the largest spread the model shows against
# ITSELF when only the order of its sums changes (the rule of tests/pcg_reference.py's tracking gates and of lanczos_data.COEFF_GATE),
# the larger of the two figures for both, measured on the CPU with nothing of the library; tests/test_deflation_cpu.py re-measures all
# of it.  Measured spreads (rel_err, x):
#     n      dtype   m    k = 1                   2                       5                       20
#     384    fp64    3    4.44e-16, 5.31e-16      6.66e-16, 7.53e-16      8.88e-16, 8.39e-16      1.78e-15, 2.58e-15
#     384    fp32    3    7.64e-8,  1.00e-7       1.17e-7,  1.56e-7       1.55e-7,  2.09e-7       6.24e-7,  5.93e-7
#     2049   fp64    3    2.22e-16, 2.40e-16      4.44e-16, 3.85e-16      6.66e-16, 5.93e-16      1.78e-15, 1.42e-15
#     2049   fp32    3    2.39e-8,  5.17e-8       1.17e-7,  1.54e-7       9.19e-8,  2.43e-7       2.55e-7,  3.32e-7
#     384    fp64    32   4.44e-16, 8.08e-16      6.66e-16, 1.04e-15      8.88e-16, 2.22e-15      3.77e-15, 1.10e-14
#     384    fp32    32   1.02e-7,  2.42e-7       1.38e-7,  2.92e-7       3.47e-7,  6.63e-7       1.68e-6,  3.44e-6
PARITY_GATE = {
    (384, "F64", 3): {1: 5.4e-15, 2: 7.6e-15, 5: 8.9e-15, 20: 2.6e-14},
    (384, "F32", 3): {1: 1.1e-6, 2: 1.6e-6, 5: 2.1e-6, 20: 6.3e-6},
    (2049, "F64", 3): {1: 2.4e-15, 2: 4.5e-15, 5: 6.7e-15, 20: 1.8e-14},
    (2049, "F32", 3): {1: 5.2e-7, 2: 1.6e-6, 5: 2.5e-6, 20: 3.4e-6},
    (384, "F64", 32): {1: 8.1e-15, 2: 1.1e-14, 5: 2.3e-14, 20: 1.2e-13},
    (384, "F32", 32): {1: 2.5e-6, 2: 3.0e-6, 5: 6.7e-6, 20: 3.5e-5},
}


# ------------------------------------------------------------------------------------------------
# Ritz vectors end to end: the known-spectrum system of lanczos_data (a bulk on [1, 2], four outliers at either end)
# ------------------------------------------------------------------------------------------------
KNOWN_N = LD.KNOWN_N
KNOWN_NEV = 8                        # which = both: the four low and the four high outliers
KNOWN_NRHS = 3                       # K = 4 with one padding column, so the same batch runs under symmetric_many
KNOWN_MAX_ITERS = 200
KNOWN_REL_ERROR = {"F64": 1e-10, "F32": 1e-5}
# What the model shows on this system (tests/test_deflation_cpu.py re-measures it), the three right-hand sides, the three sum orders:
#     dtype   plain CG      deflated, the model's Ritz vectors   deflated, numpy's eigenvectors   true residual deflated / plain
#     fp64    35 35 35      14 14 14 in every order              14 14 14                         0.45 .. 0.47
#     fp32    31 .. 34      7 7 7 in every order                 7 7 7                            0.55 .. 3.74 (plain: 1.4e-6 .. 1.0e-5)
# KNOWN_ITER_MARGIN: how far the device's deflated count may lie from the model's.  The model's own spread between its sum orders is
# 0; the stop test compares a residual that falls by a factor of about 6 per iteration (a bulk of condition 2) with a fixed
# threshold, so a perturbation far below that factor -- other Ritz vectors of the same accuracy, another sum order -- moves the count
# by at most one: margin = spread + 1.
KNOWN_ITER_MARGIN = {"F64": 1, "F32": 1}
# KNOWN_TRUE_MARGIN: the deflated solve's true residual against the plain solve's of the same run.  The residual-floor yardstick
# (8 N u ||A||) does not fit: both solves stop on their recursive residual well above it in fp64 (2.4e-11 against a floor of 2.2e-11
# only by chance) and far below it in fp32 (5.4e-6 against 1.2e-2).  The model's largest ratio deflated / plain, times 10.
KNOWN_TRUE_MARGIN = {"F64": 4.7, "F32": 38.0}


@functools.lru_cache(maxsize=None)
def known_rhs():
    B = np.random.default_rng(385).uniform(-1, 1, (KNOWN_NRHS, KNOWN_N))
    B.setflags(write=False)
    return B


@functools.lru_cache(maxsize=None)
def known_model(dtype_name, order="rows", exact=False):
    """The model end to end on the known-spectrum system: its own Lanczos run (which = both, nev = 8) and Ritz vectors -- or, exact:
    numpy's eigenvectors of the 8 outliers --, the space, the deflated and the plain solves of every column.  Returns a dict:
    deflated / plain (iteration counts), true_deflated / true_plain (||b - A x|| / ||b|| in fp64), wr (the largest |W^T r| / (|W| |r|)
    of the final recursive residual, formed in fp64)."""
    dtype = DTYPES[dtype_name]
    A = LD.known_matrix(dtype_name)
    if exact:
        ev, Q = np.linalg.eigh(A)
        Y = np.concatenate([Q[:, :4], Q[:, -4:]], axis=1).T
    else:
        _, _, v0 = LD.known_inputs()
        run = L.lanczos(A, v0, LD.KNOWN_MAX_STEPS, dtype, order, nev=KNOWN_NEV, which=L.BOTH, tol=LD.KNOWN_TOL[dtype_name],
                        check_every=LD.KNOWN_CHECK_EVERY)
        assert run["all_converged"]
        Y = L.ritz_vectors(run)
    sp = R.space(A, Y, dtype, order)
    out = dict(deflated=[], plain=[], true_deflated=[], true_plain=[], wr=[])
    for b in known_rhs():
        x, st = R.deflated_cg(A, sp, b, KNOWN_MAX_ITERS, KNOWN_REL_ERROR[dtype_name], dtype, order)
        xp, stp = P.pcg_ordered(A, b, KNOWN_MAX_ITERS, KNOWN_REL_ERROR[dtype_name], None, dtype, order)
        out["deflated"].append(st["num_iters"])
        out["plain"].append(stp["num_iters"])
        out["true_deflated"].append(P.true_residual(A, x, b))
        out["true_plain"].append(P.true_residual(A, xp, b))
        r = b.astype(np.float64) - A @ x.astype(np.float64)
        W = sp["W"].astype(np.float64)
        out["wr"].append(float(np.abs(W @ r).max() / (np.linalg.norm(W, axis=1).max() * np.linalg.norm(r))))
    return {k: np.array(v) for k, v in out.items()}
