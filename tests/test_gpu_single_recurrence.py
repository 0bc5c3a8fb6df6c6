"""The single solve past its first step -- lam_hip_solve / lam_hip_cg_init / lam_hip_cg_iterate: the r update, r.r, beta, the p update,
the hand-over of the new p between shards, the two alternating gather buffers, the scalars carried from one iteration to the next
(csrc/lam_kernels.h, "the recurrence of the vector step, written ONCE", and its six kernels) -- followed against a reference at
every tracked iteration count, on every storage type and every one-process topology.

What the rest of the suite holds of it: the product and the first step exactly (tests/test_gpu_exact.py), the recurrence past step
1 on fp64, one shard, n = 384 (test_gpu_parity.py::test_cg_matches_oracle_iteration_by_iteration), and everything else past step 1
through convergence-level gates (iteration counts, x to 1e-8 / 1e-3) or bit for bit against another VARIANT.  CG corrects itself:
a beta that is slightly off, a row at the end of a slice that misses its p update, a stale p slice or gather buffer converge an
iteration or two late and pass all of that.  Here solve(k, 1e-30) is compared at k = 1, 2, 5, ... with

  fp64          oracle.cg_solve at one rank, gates ITERATION_TRACKING_GATES (k = 1, 2, 5, 20, 40);
  fp32, bf16    pcg_reference.pcg_ordered(A_stored, b32, order "rows") in fp32, gates FP32_TRACKING_GATE (k = 1, 2, 5, 10, 20, 30;
                k = 40 is printed, not asserted: the fp32 reference no longer agrees with itself there),

on the systems of tests/tracking_data.py (n = 384, and n = 1547 whose slices start off a 16-byte boundary, are ragged and cross the
vector step's workgroup).  The gates rest on the references alone: tests/test_single_recurrence_cpu.py holds every reference's
own spread between summation orders at or below a tenth of them.  The bf16 matrix of the reference is rounded on the HOST
(generator_model.stored); download_rows must return exactly it, and the device's copy never feeds the reference.  Vectors are fp32.

One process, all shards on device 0.  Rank mode and exchange 2 are tied bit for bit to the exchanges tracked here by
test_one_process_gather_ap_is_bit_identical_to_rank_mode_gather_ap, test_symmetric_product_rank_mode_matches_one_process,
test_one_process_direct_exchange_matches_events and test_direct_exchange_is_bit_identical_to_rccl_exchange."""
import numpy as np
import pytest

import pcg_reference as R
from tracking_data import SINGLE_TRACKING_DTYPES, SINGLE_TRACKING_N, single_tracking_gates, stored_tracking_system

pytestmark = pytest.mark.gpu

ONE_SHARD = ({}, {"symmetric": 2}, {"fuse_update": 0})
SEVERAL_SHARDS = ({"exchange": 0}, {"exchange": 1}, {"exchange": 1, "symmetric": 2}, {"exchange": 1, "fuse_update": 0})
MORE_SHARDS_THAN_PARTIALS = ({"exchange": 1}, {"exchange": 1, "symmetric": 2})       # 384 rows on 33 shards: 11 rows each, 32 on the last

CASES = [(d, n, P) for d in SINGLE_TRACKING_DTYPES for n in SINGLE_TRACKING_N for P in (1, 2, 3, 5, 8)] + [("F64", 384, 33)]
CHUNKS = (1, 2, 9, 28)

_references = {}


def _reference(oracle, n, dtype_name):
    """k -> (x_ref in fp64, rel_err_ref), computed once per (system, storage type) and shared by every configuration."""
    key = (n, dtype_name)
    if key not in _references:
        A, b = stored_tracking_system(n, dtype_name)
        ks = sorted(single_tracking_gates(n, dtype_name))
        ref = {}
        if dtype_name == "F64":
            for k in ks:
                x, st = oracle.cg_solve(A, b, k, 1e-30)
                assert st["num_iters"] == k + 1
                ref[k] = (x, st["rel_err"])
        else:
            track = dict.fromkeys(ks)
            _, st = R.pcg_ordered(A, b, ks[-1], 1e-30, None, np.float32, "rows", track=track)
            assert st["num_iters"] == ks[-1] + 1
            ref = {k: (x.astype(np.float64), re) for k, (x, re) in track.items()}
        _references[key] = ref
    return _references[key]


def _configurations(P):
    return ONE_SHARD if P == 1 else (MORE_SHARDS_THAN_PARTIALS if P == 33 else SEVERAL_SHARDS)


def _open(lam, dtype_name, n, P, options):
    """A context of P shards on device 0 holding the system, with `options` set and seen to be in force: nothing passes on a
    fallback.  The matrix it holds is the host's, bit for bit."""
    A, b = stored_tracking_system(n, dtype_name)
    s = lam.Solver(getattr(lam, dtype_name), device_ids=[0] * P)
    try:
        s.set_matrix(A)
        s.set_rhs(b)
        for name, value in options.items():
            s.set_option(name, value)
        dev = s.download_rows(0, n)
        assert dev.dtype == A.dtype and np.array_equal(dev.view(np.uint32 if dev.dtype == np.float32 else np.uint64),
                                                       np.ascontiguousarray(A).view(np.uint32 if A.dtype == np.float32 else np.uint64)), \
            (dtype_name, n, P, "the device's matrix is not the host-rounded one")
        assert s.vec_dtype == b.dtype and [s.partition(q)[1] for q in range(P)] == [n // P] * (P - 1) + [n // P + n % P]
    except BaseException:
        s.close()
        raise
    return s


def _assert_in_force(s, P, options, what):
    """After the first solve / cg_init: the exchange, the product and the launch form the CG state really runs on."""
    want_exchange = options.get("exchange", 0) if P > 1 else 0
    want_fused = 1 if options.get("fuse_update", 1) and (P == 1 or want_exchange == 1) else 0
    got = (s.get_option("exchange_effective"), s.get_option("symmetric_effective"), s.get_option("fuse_effective"))
    assert got == (want_exchange, 1 if options.get("symmetric") else 0, want_fused), (what, got)


def _check(what, k, x, rel_err, num_iters, ref, gates, worst):
    """Prints the observed fractions of the gates, asserts them where k is an asserted one."""
    x_ref, re_ref = ref[k]
    g_res, g_x, asserted = gates[k]
    d_re = abs(rel_err / re_ref - 1)
    d_x = np.linalg.norm(x.astype(np.float64) - x_ref) / np.linalg.norm(x_ref)
    print(f"{what} k={k}: rel_err off by {d_re:.3e} = {d_re / g_res:.3f} of the gate, x by {d_x:.3e} = {d_x / g_x:.3f} of the gate"
          + ("" if asserted else " (informational)"))
    assert num_iters == k + 1, (what, k, num_iters)
    if asserted:
        worst[0] = max(worst[0], d_re / g_res, d_x / g_x)
        assert d_re < g_res and d_x < g_x, (what, k, d_re, g_res, d_x, g_x)


@pytest.mark.parametrize("dtype_name,n,P", CASES, ids=[f"{d}-{n}-P{P}" for d, n, P in CASES])
def test_single_solve_tracks_the_reference_iteration_by_iteration(lam, oracle, dtype_name, n, P):
    """solve(k, 1e-30) for every tracked k in every configuration of this shard count: num_iters = k + 1, rel_err and x within the
    gates of their reference (module docstring).  P = 1: the default, the symmetric product, the two-kernel vector step; P = 2, 3, 5,
    8: the sliced exchange, the gather-Ap exchange, gather-Ap with the symmetric product and with the two-kernel vector step;
    P = 33 (fp64, n = 384): a shard has fewer rows than reduce partials."""
    ref, gates = _reference(oracle, n, dtype_name), single_tracking_gates(n, dtype_name)
    worst = [0.0]
    for options in _configurations(P):
        what = f"{dtype_name} n={n} P={P} {options or 'default'}"
        with _open(lam, dtype_name, n, P, options) as s:
            for k in sorted(gates):
                assert s.solve(k, 1e-30) is False
                if k == min(gates):
                    _assert_in_force(s, P, options, what)
                _check(what, k, s.solution(), s.stats["rel_err"], s.stats["num_iters"], ref, gates, worst)
            _assert_in_force(s, P, options, what)
    print(f"{dtype_name} n={n} P={P}: worst fraction of an asserted gate {worst[0]:.3f}")


@pytest.mark.parametrize("dtype_name", SINGLE_TRACKING_DTYPES)
def test_chunked_iteration_tracks_the_reference_at_its_chunk_ends(lam, oracle, dtype_name):
    """cg_init + cg_iterate(1), (2), (9), (28) on the gather-Ap exchange, n = 1547 on 3 shards: the state that crosses a call -- the
    scalars, the parity of the gather buffers, the explicit p -- at the chunk ends 1, 3, 12, 40.  The ends that are tracked k (1 and
    40) are held to the gates (fp32 / bf16: 40 is informational); at EVERY end x and rel_err are those of solve(end) bit for bit,
    which ties the ends in between to the solves followed above."""
    n, P, options = 1547, 3, {"exchange": 1}
    ref, gates = _reference(oracle, n, dtype_name), single_tracking_gates(n, dtype_name)
    what = f"{dtype_name} n={n} P={P} {options} chunks {CHUNKS}"
    worst = [0.0]
    ends = np.cumsum(CHUNKS).tolist()
    with _open(lam, dtype_name, n, P, options) as s:
        whole = {}
        for k in ends:
            s.solve(k, 1e-30)
            whole[k] = (s.solution(), s.stats["rel_err"])
        s.cg_init()
        _assert_in_force(s, P, options, what)
        for chunk, k in zip(CHUNKS, ends):
            st = s.cg_iterate(chunk, 1e-30)
            x = s.solution()
            assert not st["converged"] and st["num_iters"] == k + 1, (what, k, st)
            assert st["rel_err"] == whole[k][1] and np.array_equal(x, whole[k][0]), (what, k, st["rel_err"], whole[k][1])
            if k in gates:
                _check(what, k, x, st["rel_err"], st["num_iters"], ref, gates, worst)
    assert set(ends) & set(gates) == {1, 40}
    print(f"{what}: worst fraction of an asserted gate {worst[0]:.3f}")
