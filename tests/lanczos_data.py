"""Systems and gates of the Lanczos eigensolver's tests (tests/test_lanczos_cpu.py establishes them on the CPU,
tests/test_gpu_eigs.py follows them on the device): lam_hip_eigs."""
import functools

import numpy as np

import generator_model as G
import lanczos_reference as L
from pcg_reference import ORDERS

DTYPES = {"F64": np.float64, "F32": np.float32}

# ------------------------------------------------------------------------------------------------
# coefficient parity: generate_spectrum_spd's law at two sizes, a host-given start vector
# ------------------------------------------------------------------------------------------------
PARITY_SIZES = (384, 2049)           # 2049: ragged for the 4-row workgroups of the product and for the 16-byte vectors
PARITY_K = (1, 2, 5, 20, 40)         # steps (counted from 1) whose alpha and beta are compared
PARITY_STEPS = max(PARITY_K)
UNGATED_ABOVE = 1e-2                 # a step where the model's own spread exceeds this is reported, not gated


def parity_inputs(n):
    """(eig, reflectors, v0) of the parity system of size n: the generator tests' spectrum law, 3 reflectors; v0 uniform in [-1, 1)."""
    eig, V = G.spectrum_inputs(n, 3)
    v0 = np.random.default_rng(7 * n + 1).uniform(-1, 1, n)
    return eig, V, v0


@functools.lru_cache(maxsize=None)
def parity_matrix(n, dtype_name):
    """The parity system as the model builds it (np.longdouble, then the storage's rounding), symmetrised bit for bit."""
    eig, V, _ = parity_inputs(n)
    A = np.asarray(G.spectrum_spd(G.spectrum_eig_as_uploaded(eig, dtype_name), V), np.float64)
    A = G.stored(0.5 * (A + A.T), dtype_name).astype(np.float64)
    A.setflags(write=False)
    return A


def coefficients(A, v0, dtype, order, steps=PARITY_STEPS):
    run = L.lanczos(A, v0, steps, dtype, order, nev=1, tol=0.0, check_every=steps)
    return run["alpha"], run["beta"]


def measure_coefficient_spreads(n, dtype_name):
    """{k: largest relative spread of alpha_{k-1} and beta_{k-1} between the model's three sum orders} on the parity system."""
    dtype = DTYPES[dtype_name]
    _, _, v0 = parity_inputs(n)
    runs = [coefficients(parity_matrix(n, dtype_name), v0, dtype, o) for o in ORDERS]
    out = {}
    for k in PARITY_K:
        s = 0.0
        for a in runs:
            for b in runs:
                s = max(s, abs(a[0][k - 1] / b[0][k - 1] - 1), abs(a[1][k - 1] / b[1][k - 1] - 1))
        out[k] = s
    return out


# Relative gates of alpha_{k-1} and beta_{k-1} at step k: 10 x the largest spread the model shows against ITSELF when only the order of
# its sums changes (the rule of tests/pcg_reference.py's tracking gates), measured on the CPU with nothing of the library;
# tests/test_lanczos_cpu.py re-measures all of it.  Measured spreads:
#     n      dtype   k = 1       2           5           20          40
#     384    fp64    2.22e-16    2.22e-16    4.44e-16    1.33e-15    8.88e-16
#     384    fp32    2.74e-8     1.78e-7     1.46e-7     7.69e-7     3.24e-7
#     2049   fp64    2.22e-16    2.22e-16    2.22e-16    1.55e-15    1.11e-15
#     2049   fp32    1.17e-8     4.10e-8     1.79e-7     5.69e-7     3.29e-7
# None exceeds UNGATED_ABOVE: every checked step is gated.
COEFF_GATE = {
    (384, "F64"): {1: 2.3e-15, 2: 2.3e-15, 5: 4.5e-15, 20: 1.4e-14, 40: 8.9e-15},
    (384, "F32"): {1: 2.8e-7, 2: 1.8e-6, 5: 1.5e-6, 20: 7.7e-6, 40: 3.3e-6},
    (2049, "F64"): {1: 2.3e-15, 2: 2.3e-15, 5: 2.3e-15, 20: 1.6e-14, 40: 1.2e-14},
    (2049, "F32"): {1: 1.2e-7, 2: 4.1e-7, 5: 1.8e-6, 20: 5.7e-6, 40: 3.3e-6},
}


# ------------------------------------------------------------------------------------------------
# known spectrum: 376 values spread evenly on [1, 2] and four outliers at either end
# ------------------------------------------------------------------------------------------------
KNOWN_N = 384
KNOWN_OUTLIERS_LOW = (0.01, 0.05, 0.2, 0.5)
KNOWN_OUTLIERS_HIGH = (8.0, 16.0, 32.0, 64.0)
KNOWN_NEV = 4
KNOWN_MAX_STEPS = 120
KNOWN_CHECK_EVERY = 8
KNOWN_TOL = {"F64": 1e-10, "F32": 1e-5}
RESIDUAL_FLOOR_FACTOR = 8            # floor = 8 N u_TV ||A||: the constant the MINRES tests use for a formable residual


def known_inputs():
    eig = np.concatenate([KNOWN_OUTLIERS_LOW, np.linspace(1.0, 2.0, KNOWN_N - 8), KNOWN_OUTLIERS_HIGH])
    rng = np.random.default_rng(384)
    return eig, rng.uniform(-1, 1, (3, KNOWN_N)), rng.uniform(-1, 1, KNOWN_N)


@functools.lru_cache(maxsize=None)
def known_matrix(dtype_name):
    eig, V, _ = known_inputs()
    A = np.asarray(G.spectrum_spd(G.spectrum_eig_as_uploaded(eig, dtype_name), V), np.float64)
    A = G.stored(0.5 * (A + A.T), dtype_name).astype(np.float64)
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def known_run(dtype_name, which):
    """The model on the known-spectrum system as the GPU test runs the device."""
    _, _, v0 = known_inputs()
    return L.lanczos(known_matrix(dtype_name), v0, KNOWN_MAX_STEPS, DTYPES[dtype_name], "rows", nev=KNOWN_NEV, which=which,
                     tol=KNOWN_TOL[dtype_name], check_every=KNOWN_CHECK_EVERY)


def residual_floor(n, dtype_name, norm_a):
    return RESIDUAL_FLOOR_FACTOR * n * L.UNIT_ROUNDOFF[DTYPES[dtype_name]] * norm_a
