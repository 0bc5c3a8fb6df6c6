"""Systems, gates and margins of the block CG tests (tests/test_block_cg_cpu.py establishes them on the CPU with the numpy model
tests/block_cg_reference.py, tests/test_gpu_block_cg.py follows them on the device): lam_hip_solve_block, lam_hip_block_factor."""
import functools

import numpy as np

import block_cg_reference as R

DTYPES = {"F64": np.float64, "F32": np.float32}
REL_ERROR = {"F64": 1e-8, "F32": 1e-4}
MAX_ITERS = 200

# ------------------------------------------------------------------------------------------------
# the outlier system: A = H3 H2 H1 diag(eig) H1 H2 H3, a bulk on [1, 2] over a few eigenvalues in [1e-4, 1e-3]
# ------------------------------------------------------------------------------------------------
SIZES = (7, 65, 2049, 65537)         # below one 16-byte vector of rows, ragged, several workgroups, past the grid-stride wrap (256 x 256)
NRHS = (1, 2, 3, 5, 8)               # 3 and 5 leave padding columns at K = 4 and K = 8
N_OUTLIERS = 6
N_REFLECTORS = 3
POINT_N = 2049                       # "the point of the feature": block against independent CG at this size


@functools.lru_cache(maxsize=None)
def system(n):
    """(eig (n), V (3, n), B (8, n)), read-only: what lam_hip_generate_spectrum_spd and lam_hip_set_rhs_many are given."""
    m = min(N_OUTLIERS, n // 2)
    eig = np.concatenate([np.geomspace(1e-4, 1e-3, m), np.linspace(1.0, 2.0, n - m)])
    rng = np.random.default_rng(7000 + n)
    eig = rng.permutation(eig)
    V = rng.uniform(-1, 1, (N_REFLECTORS, n))
    B = rng.uniform(-1, 1, (max(NRHS), n))
    for a in (eig, V, B):
        a.setflags(write=False)
    return eig, V, B


DENSE_UP_TO = 2049                   # the model holds the device's matrix itself up to this size


@functools.lru_cache(maxsize=None)
def stored_matrix(n, dtype_name):
    """The matrix the device holds, in its dtype: lam_hip_generate_spectrum_spd builds it in the vector dtype
    (tests/generator_model.py, spectrum_spd_emulated), and in fp32 that moves eigenvalues of 1e-4 by parts in a hundred."""
    import generator_model as G
    eig, V, _ = system(n)
    dtype = DTYPES[dtype_name]
    A = G.spectrum_spd_emulated(G.spectrum_eig_as_uploaded(eig, dtype_name), V, dtype).astype(np.float64)
    A = (0.5 * (A + A.T)).astype(dtype)
    A.setflags(write=False)
    return A


def operator(n, dtype_name, order="rows"):
    """P (n, s) -> A P as the model's solver is given it.  Up to DENSE_UP_TO: the stored matrix times P with the sums IN THE VECTOR
    DTYPE, as the device's product has them, its columns taken in `order` -- where u_TV cond(A) comes near rel_error (fp32, N = 7 and
    65) the order of these sums moves the iteration count, and the spread between the orders is how the gates below know.  Above
    (65537, which no host holds): the exact operator in fp64, see exact_operator."""
    if n > DENSE_UP_TO:
        return exact_operator(n)
    A = stored_matrix(n, dtype_name)
    cols = R._row_order(n, order)
    Ap = np.ascontiguousarray(A[:, cols])
    return lambda P: Ap @ np.ascontiguousarray(P[cols].astype(A.dtype))


def operator64(n, dtype_name):
    """The same matrix with every sum in fp64: what true residuals are formed with."""
    if n > DENSE_UP_TO:
        return exact_operator(n)
    A = stored_matrix(n, dtype_name).astype(np.float64)
    return lambda P: A @ P.astype(np.float64)


def exact_operator(n):
    """P (n, s) -> A P in fp64 without forming A: the reflectors H_k .. H_1, the diagonal, H_1 .. H_k."""
    eig, V, _ = system(n)
    vv = (V * V).sum(axis=1)

    def reflect(Y, j):
        return Y - np.outer(V[j], (2.0 / vv[j]) * (V[j] @ Y))

    def apply(P):
        Y = P.astype(np.float64)
        for j in range(N_REFLECTORS - 1, -1, -1):
            Y = reflect(Y, j)
        Y = eig[:, None] * Y
        for j in range(N_REFLECTORS):
            Y = reflect(Y, j)
        return Y
    return apply


def orders(n):
    """The sum orders the model is run in: eight where it holds the device's matrix (in fp32 at N = 65 three orders show 39 .. 40
    iterations for one column and eight show 39 .. 44), three at N = 65537, where a run costs seconds and nothing moves."""
    return R.MORE_ORDERS if n <= DENSE_UP_TO else R.ORDERS


def true_residuals(n, dtype_name, X, B):
    """||b_j - A x_j|| / ||b_j|| as lam_hip_true_residual_many forms it: up to DENSE_UP_TO the stored matrix times x and the
    subtraction IN THE VECTOR DTYPE, the norms in fp64; above, in fp64 on the exact operator."""
    dtype = DTYPES[dtype_name]
    if n > DENSE_UP_TO:
        return R.true_residuals(exact_operator(n), X, B.astype(dtype))
    A = stored_matrix(n, dtype_name)
    Xt, Bt = np.ascontiguousarray(X.T).astype(dtype), np.ascontiguousarray(B.T).astype(dtype)
    Rt = (Bt - A @ Xt).astype(np.float64)
    return np.linalg.norm(Rt, axis=0) / np.linalg.norm(Bt.astype(np.float64), axis=0)


@functools.lru_cache(maxsize=None)
def model(n, nrhs, dtype_name, order="rows"):
    """The model's block run on the first nrhs columns.  Returns a dict: info (block_cg's), X (None if the block was refused), true
    (the solution's true residuals per column, see true_residuals)."""
    B = system(n)[2][:nrhs]
    X, info = R.block_cg(operator(n, dtype_name, order), B, MAX_ITERS, REL_ERROR[dtype_name], DTYPES[dtype_name], order)
    return dict(info=info, X=X, true=None if X is None else true_residuals(n, dtype_name, X, B))


@functools.lru_cache(maxsize=None)
def plain_counts(n, nrhs, dtype_name):
    """Iteration counts of the model's independent CG on the same columns."""
    dtype = DTYPES[dtype_name]
    ap = operator(n, dtype_name)
    return np.array([R.cg(ap, b, MAX_ITERS, REL_ERROR[dtype_name], dtype)[1] for b in system(n)[2][:nrhs]])


def measure(n, nrhs, dtype_name):
    """What the model shows on one case over orders(n): dict(iters, breakdown: of the rows order; spread: largest - smallest number
    of completed iterations; kinds: the set of breakdown kinds; true: the largest true residual of any order and column)."""
    runs = [model(n, nrhs, dtype_name, o) for o in orders(n)]
    iters = [r["info"]["iters"] for r in runs]
    return dict(iters=iters[0], breakdown=runs[0]["info"]["breakdown"], spread=max(iters) - min(iters),
                kinds={r["info"]["breakdown"][1] for r in runs}, true=max(float(r["true"].max()) for r in runs))


# RECORDED[(n, dtype, nrhs)] = (iterations and breakdown of the model's rows-order run, spread of the iteration count over orders(n),
# largest true residual of any order, rounded up in its third digit): what tests/test_gpu_block_cg.py holds the device to, so that
# no GPU test runs the model; tests/test_block_cg_cpu.py re-measures every entry.  A run ends converged, or in breakdown kind 2 where
# the block Krylov space fills the whole space (N = 7; N = 65 with 8 columns in fp64), the same kind in every order; N = 7 with
# 8 columns is refused (B^T B has rank 7: column 7) and has no entry.  fp32 at N = 7 and 65 runs where u_TV cond(A) = 6e-8 * 2e4 is
# ten times rel_error: convergence is delayed by rounding, by an amount that depends on the order of the product's sums.
RECORDED = {
    (7, "F64", 1): (11, (0, 0), 0, 1.03e-12),
    (7, "F64", 2): (3, (3, 2), 1, 3.29e-01),
    (7, "F64", 3): (2, (2, 2), 0, 1.92e+00),
    (7, "F64", 5): (1, (1, 2), 0, 4.14e+00),
    (7, "F32", 1): (13, (0, 0), 1, 9.17e-04),
    (7, "F32", 2): (6, (0, 0), 1, 5.73e-04),
    (7, "F32", 3): (2, (2, 2), 0, 1.92e+00),
    (7, "F32", 5): (1, (1, 2), 0, 4.14e+00),
    (65, "F64", 1): (44, (0, 0), 0, 2.76e-09),
    (65, "F64", 2): (27, (0, 0), 0, 1.01e-09),
    (65, "F64", 3): (21, (0, 0), 0, 5.38e-10),
    (65, "F64", 5): (13, (0, 0), 0, 7.38e-12),
    (65, "F64", 8): (8, (8, 2), 0, 1.79e-03),
    (65, "F32", 1): (39, (0, 0), 5, 4.18e-04),
    (65, "F32", 2): (27, (0, 0), 5, 4.76e-04),
    (65, "F32", 3): (17, (0, 0), 5, 3.88e-04),
    (65, "F32", 5): (14, (0, 0), 1, 4.98e-04),
    (65, "F32", 8): (13, (0, 0), 1, 5.45e-04),
    (2049, "F64", 1): (46, (0, 0), 0, 1.95e-09),
    (2049, "F64", 2): (29, (0, 0), 0, 2.89e-09),
    (2049, "F64", 3): (24, (0, 0), 0, 2.96e-09),
    (2049, "F64", 5): (22, (0, 0), 0, 8.16e-09),
    (2049, "F64", 8): (17, (0, 0), 0, 6.42e-09),
    (2049, "F32", 1): (40, (0, 0), 0, 7.85e-05),
    (2049, "F32", 2): (24, (0, 0), 0, 4.64e-05),
    (2049, "F32", 3): (19, (0, 0), 0, 4.50e-05),
    (2049, "F32", 5): (18, (0, 0), 1, 9.42e-05),
    (2049, "F32", 8): (12, (0, 0), 0, 5.95e-05),
    (65537, "F64", 1): (46, (0, 0), 0, 1.96e-09),
    (65537, "F64", 2): (28, (0, 0), 0, 7.33e-09),
    (65537, "F64", 3): (23, (0, 0), 0, 4.42e-09),
    (65537, "F64", 5): (22, (0, 0), 0, 6.56e-09),
    (65537, "F64", 8): (17, (0, 0), 0, 8.87e-09),
    (65537, "F32", 1): (40, (0, 0), 0, 7.69e-05),
    (65537, "F32", 2): (23, (0, 0), 0, 4.95e-05),
    (65537, "F32", 3): (18, (0, 0), 0, 2.97e-05),
    (65537, "F32", 5): (17, (0, 0), 0, 4.39e-05),
    (65537, "F32", 8): (12, (0, 0), 0, 5.93e-05),
}


def iter_gate(n, nrhs, dtype_name):
    """How far the device's iteration count (and the iteration of a breakdown) may lie from the model's rows-order run: the spread
    the model shows on this very case between its sum orders, plus one."""
    return RECORDED[(n, dtype_name, nrhs)][2] + 1


# PRECISION_GAP[n]: the margin of the true-residual gate.  The device differs from the model by roundings of the vector dtype's size
# (the order of every sum, fused multiply-adds).  How far roundings of that size move the true residual is what the model shows
# between an fp32 run and an fp64-arithmetic run of the SAME stored fp32 system at the SAME tolerance, both residuals formed in
# fp32: the largest ratio, either way, over the nrhs whose two runs end the same way (measure_precision_gap; recorded rounded up,
# measured 2.25 / 3.70 / 1.27).  N = 65537 has no dense model and takes N = 2049's figure: the same spectrum with a smaller
# ||x|| / ||b||.  fp64 takes the fp32 figure of its size: numpy has no wider arithmetic that runs N = 2049 in a test's time, and the
# response to a rounding grows with u_TV / rel_error, 6e-4 in fp32 against 1e-8 in fp64, so the fp32 gap bounds the fp64 one.
PRECISION_GAP = {7: 2.3, 65: 3.8, 2049: 1.3}


def measure_precision_gap(n):
    tol, worst = REL_ERROR["F32"], 1.0
    for nrhs in NRHS:
        if nrhs > n:
            continue
        B = system(n)[2][:nrhs].astype(np.float32)
        X32, i32 = R.block_cg(operator(n, "F32"), B, MAX_ITERS, tol, np.float32)
        X64, i64 = R.block_cg(operator64(n, "F32"), B, MAX_ITERS, tol, np.float64)
        if i32["breakdown"] != i64["breakdown"]:
            continue
        t32, t64 = float(true_residuals(n, "F32", X32, B).max()), float(true_residuals(n, "F32", X64, B).max())
        worst = max(worst, t32 / t64, t64 / t32)
    return worst


def true_gate(n, nrhs, dtype_name):
    """The model's largest true residual of the case, formed as the device forms it, times the precision gap of its size."""
    return PRECISION_GAP[min(n, DENSE_UP_TO)] * RECORDED[(n, dtype_name, nrhs)][3]


# ------------------------------------------------------------------------------------------------
# lam_hip_block_factor
# ------------------------------------------------------------------------------------------------
FACTOR_SIZES = (1, 8)


def factor_case(s):
    """A random SPD G of size s: X X^T + s I with X uniform in [-1, 1)."""
    X = np.random.default_rng(90 + s).uniform(-1, 1, (s, s))
    return X @ X.T + s * np.eye(s)


def factor_gate(G):
    """Relative gate of Ginv, S and Sinv against numpy: the backward error bound of a Cholesky factorisation, s^2 u cond(G), for
    both sides of the comparison (numpy's own routines carry the same bound), times 4."""
    s = G.shape[0]
    return 4 * 2 * s * s * 2.0 ** -53 * np.linalg.cond(G)
