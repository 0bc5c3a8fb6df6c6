"""Systems, shifts and gates of the MINRES tests (tests/test_minres_cpu.py establishes them on the CPU, tests/test_gpu_minres.py follows
them on the device): lam_hip_solve_many_minres, (A + s_j I) x_j = b_j for shifts of either sign."""
import functools

import numpy as np

import minres_reference as M
import pcg_reference as R
from tracking_data import tracking_columns

# One shift per column of tracking_data.tracking_columns() (n = 384, eigenvalues 0.0504 ... 19.83, median 1.1190), each exact in fp32:
# zero; two that keep the matrix positive definite; -1.125, within 0.54 % of the median eigenvalue (182 of 384 eigenvalues negative,
# the one nearest to zero at 3e-3 .. 6e-3); -45, below -2 lambda_max (negative definite); three more inside the spectrum.
TRACKING_SHIFTS = (0.0, 0.5, -0.5, -1.125, -45.0, 2.0, -3.0, -0.125)
NEAR_MEDIAN = 3                      # the column whose shift is within 1 % of the median eigenvalue

TRACKED_K = (1, 2, 5, 10, 20, 30)    # fp64 and fp32; beyond 30 fp32 no longer agrees with itself (informational, not tracked)

# Relative gates per k, for x and rel_err alike: 10 x the largest spread that tests/minres_reference.py shows against ITSELF when only
# the order of its sums changes ("rows" / "reversed" / "lanes", all pairs, the 8 columns under the shifts above) -- the rule of
# tracking_data.FP32_TRACKING_GATE.  Measured on the CPU, nothing with the library; tests/test_minres_cpu.py re-measures all of it:
#     k      fp64 x      fp64 rel_err   gate        fp32 x      fp32 rel_err   gate
#     1      4.66e-16    3.33e-16       4.7e-15     8.88e-8     4.61e-8        8.9e-7
#     2      1.93e-15    6.66e-16       2.0e-14     1.91e-7     5.26e-8        2.0e-6
#     5      1.85e-14    1.55e-15       1.9e-13     2.00e-6     2.81e-7        2.0e-5
#     10     3.82e-15    4.00e-15       4.0e-14     2.40e-6     1.06e-6        2.4e-5
#     20     1.94e-14    7.99e-15       2.0e-13     7.37e-6     2.09e-6        7.4e-5
#     30     2.55e-14    1.15e-14       2.6e-13     1.06e-5     4.66e-6        1.1e-4
# (k = 40, informational: fp64 1.65e-12 / 1.21e-14, fp32 6.3e-3 / 9.7e-2 -- fp32 has lost agreement with itself.)  The fp64 x spread at
# k = 5 is larger than k = 10's; the gates follow the measurement, k by k.
GATE = {
    np.float64: {1: 4.7e-15, 2: 2.0e-14, 5: 1.9e-13, 10: 4.0e-14, 20: 2.0e-13, 30: 2.6e-13},
    np.float32: {1: 8.9e-7, 2: 2.0e-6, 5: 2.0e-5, 10: 2.4e-5, 20: 7.4e-5, 30: 1.1e-4},
}


@functools.lru_cache(maxsize=None)
def tracking_histories(dtype, order):
    """Per column j: [(k, x_k, rel_err_k)] for k = 1..max(TRACKED_K) of the model on the tracking system under TRACKING_SHIFTS."""
    A, B = tracking_columns()
    out = []
    for j in range(8):
        h = []
        M.minres(A, TRACKING_SHIFTS[j], B[j], max(TRACKED_K), 0.0, dtype, order, history=h)
        out.append(h)
    return out


def rel_diff_x(x, x_ref):
    x, x_ref = np.asarray(x, np.float64), np.asarray(x_ref, np.float64)
    return float(np.linalg.norm(x - x_ref) / np.linalg.norm(x_ref))


def measure_spreads(dtype):
    """{k: (largest spread of x, largest spread of rel_err)} between the model's sum orders on the tracking system."""
    out = {}
    for k in TRACKED_K:
        sx = sr = 0.0
        for a in R.ORDERS:
            for b in R.ORDERS:
                if a == b:
                    continue
                for j in range(8):
                    _, xa, ra = tracking_histories(dtype, a)[j][k - 1]
                    _, xb, rb = tracking_histories(dtype, b)[j][k - 1]
                    sx = max(sx, rel_diff_x(xa, xb))
                    sr = max(sr, abs(ra / rb - 1))
        out[k] = (sx, sr)
    return out


# ------------------------------------------------------------------------------------------------
# the indefinite systems of "it solves what CG cannot"
# ------------------------------------------------------------------------------------------------
INDEFINITE_SIZES = (513, 1030)
INDEFINITE_TOL = {np.float64: 1e-8, np.float32: 1e-4}


def central_gap_shift(A):
    """-(midpoint) of the widest gap between neighbouring eigenvalues in the central half of A's spectrum, rounded to fp32 (exact in
    both vector dtypes), and half that gap: A + s I then has about as many negative as positive eigenvalues, the nearest at half a gap."""
    ev = np.linalg.eigvalsh(A)
    n = ev.size
    lo, hi = n // 4, 3 * n // 4
    i = int(np.argmax(np.diff(ev[lo:hi]))) + lo
    return float(np.float32(-0.5 * (ev[i] + ev[i + 1]))), 0.5 * (ev[i + 1] - ev[i])


@functools.lru_cache(maxsize=None)
def indefinite_case(n, dtype):
    """(A in dtype's values as float64, 8 right-hand sides in dtype, shift, cap, rel_error) on pcg_reference.smoke_system(n, seed=n)."""
    A, rng = R.smoke_system(n, seed=n)
    A = A.astype(dtype).astype(np.float64)
    B = rng.uniform(-1, 1, (8, n)).astype(dtype)
    s, _ = central_gap_shift(A)
    return A, B, s, 4 * n, INDEFINITE_TOL[dtype]
