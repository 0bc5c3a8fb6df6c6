"""Systems, right-hand sides, iteration counts and gates of the tests that follow CG iteration by iteration
(tests/test_gpu_parity.py::test_cg_matches_oracle_iteration_by_iteration, tests/test_gpu_batch_recurrence.py section C) and of the CPU
tests that establish the references' own sensitivity on them (tests/test_multi_rhs_cpu.py, tests/test_pcg_cpu.py)."""
import functools

import numpy as np

import pcg_reference as R


def iteration_tracking_system():
    """The system of test_cg_matches_oracle_iteration_by_iteration: (A, b), n = 384, cond ~ e^6."""
    n = 384
    rng = np.random.default_rng(9)
    q, _ = np.linalg.qr(rng.uniform(-1, 1, (n, n)))
    A = (q * np.exp(3.0 * rng.uniform(-1, 1, n))) @ q.T
    A = 0.5 * (A + A.T)
    b = rng.uniform(-1, 1, n)
    return A, b


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
