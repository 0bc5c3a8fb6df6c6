"""Systems and gates of the Lanczos quadrature's tests (tests/test_quadrature_cpu.py establishes them on the CPU,
tests/test_gpu_quadrature.py follows them on the device): lam_hip_lanczos_many, lam_hip_trace_quadrature.

Every gate is 10 x what the model (tests/quadrature_reference.py) measures on the CPU with nothing of the library: where the device is
compared with the model, the largest spread the model shows against ITSELF between its three sum orders; where it is compared with
the exact value from numpy.linalg.eigh, the model's own worst error over the probes and the sum orders.  tests/test_quadrature_cpu.py
re-measures all of it."""
import functools

import numpy as np

import lanczos_data
import quadrature_reference as Q
from pcg_reference import ORDERS
from tracking_data import tracking_columns

DTYPES = {"F64": np.float64, "F32": np.float32}
UNGATED_ABOVE = lanczos_data.UNGATED_ABOVE     # a step whose model spread exceeds this is reported, not gated


def stored(A, dtype_name):
    """A as the device holds it under the storage type, in float64."""
    A = np.asarray(A).astype(DTYPES[dtype_name]).astype(np.float64)
    A.setflags(write=False)
    return A


# ------------------------------------------------------------------------------------------------
# coefficients against the model: the n = 384 tracking system and the n = 2049 parity system, Rademacher probes
# ------------------------------------------------------------------------------------------------
COEFF_K = (1, 2, 5, 20)              # steps (counted from 1) whose alpha and beta are compared
COEFF_STEPS = max(COEFF_K)
COEFF_SYSTEMS = {"tracking": (384, 8, 384), "parity": (2049, 3, 2049)}       # name: (n, nprobes, seed)


@functools.lru_cache(maxsize=None)
def system_matrix(name, dtype_name):
    if name == "tracking":
        return stored(tracking_columns()[0], dtype_name)
    assert name == "parity"
    return lanczos_data.parity_matrix(2049, dtype_name)


def system_probes(name, dtype_name):
    n, nprobes, seed = COEFF_SYSTEMS[name]
    return Q.rademacher_probes(seed, nprobes, n, DTYPES[dtype_name])


@functools.lru_cache(maxsize=None)
def model_run(name, dtype_name, order, steps=COEFF_STEPS):
    return Q.lanczos_many(system_matrix(name, dtype_name), system_probes(name, dtype_name), steps, DTYPES[dtype_name], order)


def measure_coefficient_spreads(name, dtype_name):
    """{k: largest relative spread of alpha_k and beta_k between the model's sum orders, over the system's probes}."""
    runs = [model_run(name, dtype_name, o) for o in ORDERS]
    out = {}
    for k in COEFF_K:
        s = 0.0
        for a in runs:
            for b in runs:
                s = max(s, np.abs(a["alpha"][:, k - 1] / b["alpha"][:, k - 1] - 1).max(), np.abs(a["beta"][:, k - 1] / b["beta"][:, k - 1] - 1).max())
        out[k] = float(s)
    return out


# Measured spreads (alpha_k and beta_k, all pairs of orders, all probes):
#     system     dtype   k = 1       2           5           20
#     tracking   fp64    2.22e-16    4.44e-16    1.11e-15    5.55e-15
#     tracking   fp32    1.80e-8     1.49e-7     6.67e-7     1.54e-6
#     parity     fp64    4.44e-16    4.44e-16    8.88e-16    8.88e-16
#     parity     fp32    1.95e-8     1.87e-7     7.79e-7     1.62e-6
# None exceeds UNGATED_ABOVE: every checked step is gated.
COEFF_GATE = {
    ("tracking", "F64"): {1: 2.3e-15, 2: 4.5e-15, 5: 1.2e-14, 20: 5.6e-14},
    ("tracking", "F32"): {1: 1.8e-7, 2: 1.5e-6, 5: 6.7e-6, 20: 1.6e-5},
    ("parity", "F64"): {1: 4.5e-15, 2: 4.5e-15, 5: 8.9e-15, 20: 8.9e-15},
    ("parity", "F32"): {1: 2.0e-7, 2: 1.9e-6, 5: 7.8e-6, 20: 1.7e-5},
}


# ------------------------------------------------------------------------------------------------
# Gauss exactness: m = 6 steps on the tracking system integrate t^p exactly for p = 0 .. 11 and not for p = 12
# ------------------------------------------------------------------------------------------------
MOMENT_STEPS = 6
MOMENT_EXACT_P = tuple(range(2 * MOMENT_STEPS))       # 0 .. 11
MOMENT_MISS_P = 2 * MOMENT_STEPS


def moment_errors(run, A, Z, powers):
    """{p: largest relative error over the probes of znorm2 * e_1^T T^p e_1 against z^T A^p z}."""
    out = {}
    for p in powers:
        exact = Q.exact_forms(A, Z, Q.POW, (0.0,), p)[0]
        got = np.array([Q.probe_quadrature(run, j, Q.POW, (0.0,), p)[0] for j in range(len(exact))])
        out[p] = float(np.abs(got / exact - 1).max())
    return out


def measure_moment_errors(dtype_name):
    """(worst error over p = 0 .. 11, the probes and the sum orders; smallest error at p = 12 over the sum orders of the worst probe)."""
    A, Z = system_matrix("tracking", dtype_name), system_probes("tracking", dtype_name)
    worst, miss = 0.0, np.inf
    for o in ORDERS:
        e = moment_errors(model_run("tracking", dtype_name, o, MOMENT_STEPS), A, Z, MOMENT_EXACT_P + (MOMENT_MISS_P,))
        worst = max(worst, max(e[p] for p in MOMENT_EXACT_P))
        miss = min(miss, e[MOMENT_MISS_P])
    return worst, miss


# Measured over the 8 probes and the three orders: worst error up to p = 11  fp64 6.33e-15, fp32 3.27e-7;  at p = 12 (the first power
# the rule cannot integrate) 7.49e-6 / 7.35e-6: the jump the CPU test asserts (the miss is the rule's, not rounding's, so it is the
# same in both dtypes and more than twice the fp32 gate).
MOMENT_GATE = {"F64": 6.4e-14, "F32": 3.3e-6}
MOMENT_MISS_AT_LEAST = 7e-6


# ------------------------------------------------------------------------------------------------
# convergence: per-probe log and inverse quadratures on the tracking system under shifts, ONE run
# ------------------------------------------------------------------------------------------------
CONV_SHIFTS = (0.0, 0.5, 2.0)
CONV_STEPS = {"F64": 100, "F32": 60}


def convergence_errors(run, A, Z, fn):
    exact = Q.exact_forms(A, Z, fn, CONV_SHIFTS)
    got = np.array([Q.probe_quadrature(run, j, fn, CONV_SHIFTS) for j in range(exact.shape[1])]).T
    return float(np.abs(got / exact - 1).max())


def measure_convergence_errors(dtype_name):
    """{fn: the model's worst relative error against z^T f(A + s I) z over the probes, the shifts and the sum orders}."""
    A, Z = system_matrix("tracking", dtype_name), system_probes("tracking", dtype_name)
    return {fn: max(convergence_errors(model_run("tracking", dtype_name, o, CONV_STEPS[dtype_name]), A, Z, fn) for o in ORDERS)
            for fn in (Q.LOG, Q.INV)}


# Measured: fp64 log 1.96e-10, inverse 5.12e-10 (100 steps); fp32 log 9.76e-6, inverse 6.24e-6 (60 steps).
CONV_GATE = {"F64": {Q.LOG: 2.0e-9, Q.INV: 5.2e-9}, "F32": {Q.LOG: 9.8e-5, Q.INV: 6.3e-5}}


# ------------------------------------------------------------------------------------------------
# the trace itself, deterministically: N = 64, the 64 probes 8 e_i, 64 steps
# ------------------------------------------------------------------------------------------------
TRACE_N = 64
TRACE_SHIFTS = (0.0, 0.25, 1.0)


@functools.lru_cache(maxsize=None)
def trace_matrix(dtype_name):
    """A dense symmetric positive definite matrix of order 64, eigenvalues spread geometrically over [0.5, 8], in the storage's values."""
    rng = np.random.default_rng(64)
    Qm, _ = np.linalg.qr(rng.standard_normal((TRACE_N, TRACE_N)))
    A = (Qm * np.geomspace(0.5, 8.0, TRACE_N)) @ Qm.T
    return stored(0.5 * (A + A.T), dtype_name)


def trace_probes(dtype_name):
    return (8.0 * np.eye(TRACE_N)).astype(DTYPES[dtype_name])


def trace_exact(dtype_name, fn):
    """tr f(A + s I) per shift: what the mean over the 64 probes 8 e_i of z^T f(A + s I) z is."""
    lam = np.linalg.eigvalsh(trace_matrix(dtype_name))
    return np.array([Q.apply_fn(fn, lam + s).sum() for s in TRACE_SHIFTS])


def mean_and_error(per):
    """Per row of `per` (nshifts, nprobes): the mean summed in ascending j and the sample standard deviation (ddof 1) / sqrt(nprobes),
    NaN for one probe -- lam_hip_trace_quadrature's loop, operation for operation in fp64."""
    per = np.asarray(per, np.float64)
    n = per.shape[1]
    est, se = np.zeros(per.shape[0]), np.zeros(per.shape[0])
    for s in range(per.shape[0]):
        tot = np.float64(0.0)
        for j in range(n):
            tot = tot + per[s, j]
        est[s] = tot / np.float64(n)
        ss = np.float64(0.0)
        for j in range(n):
            d = per[s, j] - est[s]
            ss = ss + d * d
        se[s] = np.sqrt(ss / np.float64(n - 1)) / np.sqrt(np.float64(n)) if n > 1 else np.nan
    return est, se


def trace_estimate(run, fn):
    """(estimate, std_error, per_probe) as lam_hip_trace_quadrature forms them: the mean summed in ascending j, ddof 1."""
    n = len(run["steps_run"])
    per = np.array([Q.probe_quadrature(run, j, fn, TRACE_SHIFTS) for j in range(n)]).T
    est, se = mean_and_error(per)
    return est, se, per


@functools.lru_cache(maxsize=None)
def trace_model_run(dtype_name, order):
    return Q.lanczos_many(trace_matrix(dtype_name), trace_probes(dtype_name), TRACE_N, DTYPES[dtype_name], order)


def measure_trace_errors(dtype_name):
    """{fn: the model's worst error of the estimate against tr f(A + s I) over the shifts and the sum orders}; log: relative to
    max(|log det|, N) -- log det may pass through zero --, inverse: relative."""
    out = {}
    for fn in (Q.LOG, Q.INV):
        exact = trace_exact(dtype_name, fn)
        w = 0.0
        for o in ORDERS:
            est, _, _ = trace_estimate(trace_model_run(dtype_name, o), fn)
            w = max(w, float((np.abs(est - exact) / trace_scale(fn, exact)).max()))
        out[fn] = w
    return out


def trace_scale(fn, exact):
    return np.maximum(np.abs(exact), TRACE_N) if fn == Q.LOG else np.abs(exact)


# Measured (no probe breaks down before step 64): fp64 log 3.80e-16, inverse 4.09e-16; fp32 log 3.08e-9, inverse 8.36e-9 -- far below
# the fp32 roundoff of one coefficient: the rounding errors of the 64 probes average out in the trace.
TRACE_GATE = {"F64": {Q.LOG: 3.8e-15, Q.INV: 4.1e-15}, "F32": {Q.LOG: 3.1e-8, Q.INV: 8.4e-8}}
