"""Systems, right-hand sides, iteration counts and gates of the tests that follow CG iteration by iteration
(tests/test_gpu_parity.py::test_cg_matches_oracle_iteration_by_iteration, tests/test_gpu_batch_recurrence.py section C,
tests/test_gpu_single_recurrence.py) and of the CPU tests that establish the references' own sensitivity on them
(tests/test_multi_rhs_cpu.py, tests/test_pcg_cpu.py, tests/test_single_recurrence_cpu.py)."""
import functools

import numpy as np

import pcg_reference as R


@functools.lru_cache(maxsize=None)
def tracking_system(n):
    """(A, b) of the tracking law at size n, read-only: Q from the QR of a uniform matrix, spectrum exp(3 U[-1, 1]) (cond ~ e^6),
    symmetrised bit for bit, b uniform; default_rng(9) at every n."""
    rng = np.random.default_rng(9)
    q, _ = np.linalg.qr(rng.uniform(-1, 1, (n, n)))
    A = (q * np.exp(3.0 * rng.uniform(-1, 1, n))) @ q.T
    A = 0.5 * (A + A.T)
    b = rng.uniform(-1, 1, n)
    A.setflags(write=False)
    b.setflags(write=False)
    return A, b


def iteration_tracking_system():
    """The system of test_cg_matches_oracle_iteration_by_iteration: (A, b), n = 384, cond ~ e^6."""
    A, b = tracking_system(384)
    return A.copy(), b.copy()


# The systems the SINGLE solve is followed on (tests/test_gpu_single_recurrence.py).  384: inside one column tile and one pass of
# the vector step.  1547 = 7 * 13 * 17: n // P is odd for P = 2, 3, 5, 7, 8 (773, 515, 309, 221, 193), so every slice after the
# first starts off a 16-byte boundary in fp64 and in fp32 vectors; the remainder is 1, 2, 2, 3 for P = 2, 3, 5, 8; a slice
# is longer than the 256-thread workgroup of the vector step up to P = 5 and starts inside one at P = 8.  lambda_min 0.04996; cond 400.6 after fp32 rounding, 415.3 after bf16
# rounding (tests/test_single_recurrence_cpu.py re-checks that the matrix stays symmetric positive definite in all three).
SINGLE_TRACKING_N = (384, 1547)
SINGLE_TRACKING_DTYPES = ("F64", "F32", "BF16")


@functools.lru_cache(maxsize=None)
def stored_tracking_system(n, dtype_name):
    """(A, b) of tracking_system(n) as a context of that storage type holds them after an upload, computed on the HOST, read-only:
    F64 as it is; F32 rounded once; BF16 the fp32 value rounded to the nearest even bf16 (generator_model.stored, "twice": the law
    of an upload), returned as the fp32 numbers download_rows hands back.  b in the vector type (fp32 for F32 and BF16)."""
    import generator_model as G
    A, b = tracking_system(n)
    As, bs = np.ascontiguousarray(G.stored(A, dtype_name, "twice")), G.stored_vector(b, dtype_name)
    if As is A:
        return A, b
    As.setflags(write=False)
    bs.setflags(write=False)
    return As, bs


# (k, gate on rel_err / rel_err_ref - 1, gate on ||x - x_ref|| / ||x_ref||): see test_cg_matches_oracle_iteration_by_iteration
ITERATION_TRACKING_GATES = ((1, 1e-13, 1e-13), (2, 1e-13, 1e-13), (5, 1e-13, 1e-13), (20, 1e-12, 1e-12), (40, 1e-11, 1e-10), (60, 5e-2, 5e-5))

TRACKED_K = (1, 2, 5, 20, 40)          # what the batch is followed at (fp64 and fp32)

# fp32: the same k plus 10 and 30, the last k at which the fp32 reference still agrees with itself (below).
TRACKED_K_FP32 = (1, 2, 5, 10, 20, 30, 40)
# fp32 tracking gates, relative, for x and rel_err alike: 10 x the largest spread per k that tests/pcg_reference.py shows against
# ITSELF when only the order of its sums changes: pcg_ordered "rows" (the reference the GPU tests compare with: no BLAS, the same
# bits on every machine) / "reversed" / "lanes" and pcg (BLAS), all pairs, the 8 columns; x and rel_err of the plain run on the n = 384 system and rel_err of the Jacobi run
# on scaled_tracking_system, which share the gates.  Measured on the CPU, nothing with the library; tests/test_pcg_cpu.py
# re-measures all of it:
#     k      plain x     plain rel_err   Jacobi rel_err    largest      gate
#     1      9.70e-8     9.52e-8         9.96e-8           9.96e-8      1.0e-6
#     2      1.27e-7     1.30e-7         1.41e-7           1.41e-7      1.5e-6
#     5      4.17e-7     3.51e-7         3.03e-7           4.17e-7      4.2e-6
#     10     7.38e-7     8.03e-7         6.65e-7           8.03e-7      8.1e-6
#     20     1.31e-6     1.16e-6         1.03e-6           1.31e-6      1.4e-5
#     30     2.51e-6     1.89e-6         1.91e-6           2.51e-6      2.6e-5
#     40     5.23e-4     7.57e-2         5.64e-6           7.57e-2      0.76       (the three fixed orders; 8.06e-2 with BLAS)
# k = 40 in fp32 is INFORMATIONAL: the plain fp32 recurrence has lost orthogonality on cond ~ 400 by then, the reference differs from
# itself by 8 % in rel_err, and a gate of 0.76 catches only a column that has gone astray altogether.  k = 30 is the last tracked
# iteration that pins fp32 to a few 1e-5.
FP32_TRACKING_GATE = {1: 1.0e-6, 2: 1.5e-6, 5: 4.2e-6, 10: 8.1e-6, 20: 1.4e-5, 30: 2.6e-5, 40: 0.76}

# The SINGLE solve (tests/test_gpu_single_recurrence.py) on the systems of SINGLE_TRACKING_N below, per (system, storage type, k):
# the gates above unless the reference's own spread on that system exceeds a tenth of them somewhere; there the gate is 10 x the
# largest spread measured (the same rule), rounded up to two digits.  Measured on the CPU, nothing with the library;
# tests/test_single_recurrence_cpu.py re-measures all of it.
#   fp64 (the oracle at 1 thread against 4 / 8 threads, 40 runs, and against 2, 3, 5, 8 emulated ranks; n = 384: 33 ranks too),
#   largest of x and rel_err:
#     k      n = 384     n = 1547    gate (rel_err, x)
#     1      3.3e-16     4.2e-15     1e-13, 1e-13
#     2      1.1e-15     6.3e-15     1e-13, 1e-13
#     5      2.4e-15     5.7e-15     1e-13, 1e-13
#     20     4.9e-15     9.6e-15     1e-12, 1e-12
#     40     2.6e-12 (x; rel_err 1.6e-14)   1.3e-14   1e-11, 1e-10
#   every one within a tenth: ITERATION_TRACKING_GATES carry over to both systems.
#   fp32 vectors on the fp32-rounded and on the bf16-rounded matrix (pcg_ordered "rows" / "reversed" / "lanes" and pcg with BLAS, all
#   pairs, largest of x and rel_err; BLAS's order depends on its thread count at n = 1547: the largest over 1, 2, 4, 8, 16 threads):
#     k      384 F32     384 BF16    1547 F32               1547 BF16              FP32_TRACKING_GATE
#     1      2.30e-8     6.75e-9     1.19e-8                1.17e-7 -> 1.2e-6      1.0e-6
#     2      1.05e-7     1.34e-7     1.43e-7                2.04e-7 -> 2.1e-6      1.5e-6
#     5      3.24e-7     3.43e-7     4.51e-7 -> 4.6e-6      4.88e-7 -> 4.9e-6      4.2e-6
#     10     6.32e-7     5.66e-7     1.03e-6 -> 1.1e-5      9.88e-7 -> 9.9e-6      8.1e-6
#     20     1.19e-6     1.04e-6     1.97e-6 -> 2.0e-5      1.85e-6 -> 1.9e-5      1.4e-5
#     30     1.48e-6     1.39e-6     2.47e-6                2.31e-6                2.6e-5
#     40     5.89e-2     8.30e-2     2.72e-6                2.54e-6                0.76, informational
#   n = 384 stays within a tenth in both storage types; n = 1547 leaves it where an arrow stands (without BLAS, between the three
#   fixed orders, it stays within a tenth everywhere: at most 1.05e-6 at k = 20, 1.31e-6 at k = 30).  At k = 1 the only rounding x
#   can differ by is alpha's, one fp32 ulp = 1.2e-7: pcg with BLAS lands on the other side of it on the bf16 matrix.
#   k = 40 stays informational on both systems although the n = 1547 reference still agrees with itself there.
SINGLE_FP32_GATE_OVERRIDES = {(1547, "F32"): {5: 4.6e-6, 10: 1.1e-5, 20: 2.0e-5},
                              (1547, "BF16"): {1: 1.2e-6, 2: 2.1e-6, 5: 4.9e-6, 10: 9.9e-6, 20: 1.9e-5}}
INFORMATIONAL_K_FP32 = (40,)


def single_tracking_gates(n, dtype_name):
    """k -> (gate on rel_err / rel_err_ref - 1, gate on ||x - x_ref|| / ||x_ref||, asserted) for the single solve on
    stored_tracking_system(n, dtype_name)."""
    assert n in SINGLE_TRACKING_N and dtype_name in SINGLE_TRACKING_DTYPES
    if dtype_name == "F64":
        return {k: (g_res, g_x, True) for k, g_res, g_x in ITERATION_TRACKING_GATES if k in TRACKED_K}
    gate = {**FP32_TRACKING_GATE, **SINGLE_FP32_GATE_OVERRIDES.get((n, dtype_name), {})}
    assert sorted(gate) == list(TRACKED_K_FP32)
    return {k: (g, g, k not in INFORMATIONAL_K_FP32) for k, g in gate.items()}

# Rows of default_rng(384).uniform(-1, 1, (24, 384)) that serve as columns 1..7.  A candidate is kept only if the oracle's own
# sensitivity to summation order on it (1 thread against 4 / 8 threads and 3 emulated ranks, whose OpenMP reductions combine in an
# order that changes from run to run: the worst of 10 runs) stays at or below 0.3 of a TENTH of the gates above at every tracked k.
# Measured worst fractions of that tenth: b 0.29; rows 0, 1, 4, 6, 8, 9, 10: 0.24, 0.25, 0.23, 0.16, 0.27, 0.27, 0.24.  Replaced:
# rows 2 (1.25 at k = 40), 3 (0.53), 5 (0.56), 7 (0.38).
TRACKED_ROWS = (0, 1, 4, 6, 8, 9, 10)


@functools.lru_cache(maxsize=None)
def tracking_columns():
    """The n = 384 system and 8 right-hand sides, column 0 the single solve's b.  tests/test_multi_rhs_cpu.py re-checks the
    oracle's sensitivity on every one of them against a tenth of the gates."""
    A, b = iteration_tracking_system()
    cands = np.random.default_rng(384).uniform(-1, 1, (24, b.size))
    return A, np.vstack([b[None, :], cands[list(TRACKED_ROWS)]])


def scaled_case(n, dt):
    """(C, e, s = 2^e, A = S C S, 8 right-hand sides for C) of tests/test_gpu_batch_recurrence.py section A in the storage type's
    values, checked on the host: C symmetric positive definite with a unit diagonal, e varying between neighbouring rows."""
    Cm, rng = R.unit_diagonal_system(n, dt)
    e = R.varying_exponents(n, rng)
    A, s = R.scale_system(Cm, e)
    assert np.array_equal(Cm, Cm.T) and np.array_equal(A, A.T) and np.array_equal(np.diag(Cm), np.ones(n))
    assert np.linalg.eigvalsh(Cm)[0] > 0
    assert (np.diff(e) != 0).all() and e.min() >= -6 and e.max() <= 6           # neighbouring rows never share a scale
    assert np.array_equal(A.astype(dt).astype(np.float64), A)                     # the storage type holds A exactly
    Bh = rng.uniform(-1, 1, (8, n)).astype(dt)
    return Cm, e, s, A, Bh


@functools.lru_cache(maxsize=None)
def scaled_tracking_system(dt):
    """A = S C S of scaled_case at n = 384, its 8 scaled right-hand sides and dinv, in dt's values."""
    _, _, s, A, Bh = scaled_case(384, dt)
    return A, (s * Bh).astype(dt), R.jacobi_dinv(A, dt)
