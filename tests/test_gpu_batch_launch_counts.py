"""The launch sequence of every batched entry point (csrc/lam_multi.h), pinned by the counters behind options "hip_calls_launch"
(LAUNCHED: the product and the per-iteration vector kernels; the init, staging and residual kernels are not counted) and
"hip_calls_record" (RECORD: the event pair around a timed product).

Shape: n = 130 -- not a multiple of the product's 4 rows per workgroup, one block of the vector kernels --, both dtypes, nrhs = 1, 3 and
8 (K = 1, K = 4 with a padding column, K = 8).  rel_error = 0 stops a column only on r.r == 0, which a random SPD system of condition
1e4 does not meet in 11 iterations, so exactly max_iters = 11 iterations are enqueued: past kLag = 4, so the lag path runs; a column
that stops fails the case.  The counts follow from the code of the commit before the batched driver (multi_drive) was factored out:
  3 launches per iteration (product, two vector kernels) for CG -- plain, Jacobi, shifted or not -- and for MINRES;
  one more product in front of the loop for a start from a guess (A x0);
  4 per iteration for the multi-shift solve (its step kernel behind the seed's), whatever the number of shift groups;
  1 product per true residual of the batch, 1 per group of 8 shifts of the multi-shift one, 1 for gemv_many;
  records: 2 per timed iteration; at the default gemv_timing = 8 iterations 1 and 9 of 11 are timed.
RECORDS_PER_SOLVE was read off that commit's library with this file before the refactoring; the test pins it, not the code under test."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 130
ITERS = 11
RECORDS_PER_SOLVE = 4
NP = {"F64": np.float64, "F32": np.float32}
MIXED_SHIFTS = (0.5, -0.5, -1.125, 2.0, -3.0, -0.125, 4.0, -6.0)      # exact in fp32
NINE_SHIFTS = (0.0, 0.25, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 8.0)          # two groups of 8


@pytest.fixture(scope="module", params=[(d, k) for d in ("F64", "F32") for k in (1, 3, 8)], ids=lambda p: f"{p[0]}-nrhs{p[1]}")
def batch(request, lam):
    dtype_name, nrhs = request.param
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.generate_random_spd(N, 5, 1e4)
        assert s.get_option("gemv_timing") == 8
        rng = np.random.default_rng(11)
        B = rng.uniform(-1, 1, (nrhs, N)).astype(NP[dtype_name])
        X0 = rng.uniform(-1, 1, (nrhs, N)).astype(NP[dtype_name])
        yield lam, s, nrhs, B, X0


def _counted(s, call):
    """(launches, records) the call added."""
    l0, r0 = s.get_option("hip_calls_launch"), s.get_option("hip_calls_record")
    call()
    return s.get_option("hip_calls_launch") - l0, s.get_option("hip_calls_record") - r0


def _ran_to_the_cap(s):
    """No column stopped: every one reports max_iters + 1, not converged."""
    assert (s.num_iters_many == ITERS + 1).all() and not s.converged_many.any(), (s.num_iters_many, s.converged_many, s.rel_err_many)
    assert s.stats["num_iters"] == ITERS + 1 and not s.stats["converged"]


@pytest.mark.parametrize("shifted", [False, True], ids=["unshifted", "shifted"])
@pytest.mark.parametrize("precond", ["PC_NONE", "PC_JACOBI"])
def test_cg_solve_is_three_launches_per_iteration(batch, precond, shifted):
    lam, s, nrhs, B, _ = batch
    s.set_rhs_many(B)
    if shifted:
        s.set_shifts(np.abs(MIXED_SHIFTS[:nrhs]))
    counts = _counted(s, lambda: s.solve_many(ITERS, 0.0, getattr(lam, precond)))
    print(f"{precond} shifted={shifted} nrhs={nrhs}: launches, records = {counts}")
    _ran_to_the_cap(s)
    assert s.get_option("multi_rhs_k") == {1: 1, 3: 4, 8: 8}[nrhs]
    assert counts == (3 * ITERS, RECORDS_PER_SOLVE)


@pytest.mark.parametrize("start", ["host guess", "continued"])
def test_a_start_from_a_guess_adds_one_product(batch, start):
    lam, s, nrhs, B, X0 = batch
    s.set_rhs_many(B)
    if start == "continued":
        s.solve_many(2, 0.0)
    counts = _counted(s, lambda: s.solve_many(ITERS, 0.0, lam.PC_NONE, X0 if start == "host guess" else "continue"))
    print(f"x0 {start} nrhs={nrhs}: launches, records = {counts}")
    _ran_to_the_cap(s)
    assert counts == (3 * ITERS + 1, RECORDS_PER_SOLVE)


@pytest.mark.parametrize("shifts", [None, MIXED_SHIFTS], ids=["unshifted", "mixed shifts"])
def test_minres_is_three_launches_per_iteration(batch, shifts):
    lam, s, nrhs, B, _ = batch
    s.set_rhs_many(B)
    counts = _counted(s, lambda: s.solve_minres(ITERS, 0.0, None if shifts is None else shifts[:nrhs]))
    print(f"minres shifts={shifts is not None} nrhs={nrhs}: launches, records = {counts}")
    _ran_to_the_cap(s)
    assert counts == (3 * ITERS, RECORDS_PER_SOLVE)


def test_true_residuals_and_the_batched_product_are_one_launch_each(batch):
    lam, s, nrhs, B, X0 = batch
    s.set_rhs_many(B)
    s.solve_many(ITERS, 0.0)
    counts = _counted(s, s.true_residuals)
    print(f"true_residuals nrhs={nrhs}: launches, records = {counts}")
    assert counts == (1, 0)
    s.set_shifts(np.abs(MIXED_SHIFTS[:nrhs]))
    assert _counted(s, s.true_residuals) == (1, 0)
    counts = _counted(s, lambda: s.gemv_many(X0))
    print(f"gemv_many nrhs={nrhs}: launches, records = {counts}")
    assert counts == (1, 0)


@pytest.mark.parametrize("dtype_name", ["F64", "F32"])
def test_multishift_solve_of_two_groups_is_four_launches_per_iteration(lam, dtype_name):
    with lam.Solver(getattr(lam, dtype_name)) as s:
        s.generate_random_spd(N, 5, 1e4)
        b = np.random.default_rng(12).uniform(-1, 1, N).astype(NP[dtype_name])
        counts = _counted(s, lambda: s.solve_multishift(b, NINE_SHIFTS, ITERS, 0.0))
        print(f"{dtype_name} solve_multishift, 9 shifts: launches, records = {counts}")
        assert (s.num_iters_shift == ITERS + 1).all() and not s.converged_shift.any(), (s.num_iters_shift, s.converged_shift, s.rel_err_shift)
        assert counts == (4 * ITERS, RECORDS_PER_SOLVE)
        counts = _counted(s, s.multishift_true_residuals)
        print(f"{dtype_name} multishift_true_residuals, 9 shifts: launches, records = {counts}")
        assert counts == (2, 0)
