"""The runtime-call sequence of one CG iteration's enqueue (csrc/lam_iterate.h, csrc/lam_exchange.h), pinned by the counters behind
options "hip_calls_launch" (LAUNCHED), "hip_calls_record" (RECORD), "hip_calls_wait" (WAITEV), "hip_calls_setdevice" (set_dev) and
"collectives_enqueued": what lam_hip_cg_init and then lam_hip_cg_iterate(11, rel_error = 0) add to each of them, on a fresh context.

11 iterations are past kLag = 4, so the lag path and its harvest of the timed slots run; rel_error = 0 stops only on r.r == 0, which
a random SPD system of condition 1e4 does not meet in 11 iterations: the run goes to the cap and reports max_iters + 1 = 12.  Every
case runs with gemv_timing = 1 (every iteration carries the event pair(s) of the timed product) and 8 (iterations 1 and 9 do).
  one shard          n = 1000 fused and two-kernel vector step; the symmetric product; n = 4096 with the own-slice panel 1024..3072
                     (the split product: two launches, two event pairs)
  three shards       all on device 0, n = 1001 = 333 + 333 + 335, the uneven partition with the long last record: the event exchange,
                     and gather-Ap with its join through shard 0 or all-to-all x fused or two-kernel vector step x general or
                     symmetric product
  one rank           a one-rank communicator of the real RCCL (LAM_HIP_FORCE_RCCL=1), n = 1001: the event exchange with the
                     all-gather of p on the comm stream (overlap 1) or not, gather-Ap with the general and the symmetric product
  tuning build       gather-Ap on three shards and on one rank with finalize = 0 (the 1-block reduction launch behind the product):
                     tests/tuning_cases.py `call_counts`, in a child process
The direct exchange and runs with several ranks are pinned by test_one_process_direct_exchange_matches_events and
tests/test_gpu_rank_mock.py.

EXPECTED holds literals.  They were read off the libraries of the commit BEFORE the iteration's product step was written once
(the helpers timed_product / launch_split_gemv / gather_ap_product), with this very file; the test pins them, not the code under
test.  Each value: (launch, record, wait, setdevice, collectives) added by cg_init, then the same five added by cg_iterate."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ITERS = 11
COUNTERS = ("hip_calls_launch", "hip_calls_record", "hip_calls_wait", "hip_calls_setdevice", "collectives_enqueued")

# name -> (n, shards (0 = one rank through RCCL), options in the order they are set)
CASES = {
    "1shard-fused": (1000, 1, {"fuse_update": 1}),
    "1shard-two-kernel": (1000, 1, {"fuse_update": 0}),
    "1shard-symmetric": (1000, 1, {"symmetric": 2}),
    "1shard-split": (4096, 1, {"panel_lo": 1024, "panel_hi": 3072}),
    "3shards-events": (1001, 3, {"exchange": 0}),
    "1rank-events-overlap1": (1001, 0, {"exchange": 0, "overlap": 1}),
    "1rank-events-overlap0": (1001, 0, {"exchange": 0, "overlap": 0}),
    "1rank-gatherAp-general": (1001, 0, {"exchange": 1, "symmetric": 0}),
    "1rank-gatherAp-symmetric": (1001, 0, {"exchange": 1, "symmetric": 2}),
}
for _join in (1, 0):
    for _fuse in (1, 0):
        for _sym in (0, 2):
            CASES[f"3shards-gatherAp-join{_join}-fuse{_fuse}-sym{_sym}"] = (
                1001, 3, {"exchange": 1, "exchange_join": _join, "fuse_update": _fuse, "symmetric": _sym})

# the tuning build's cases: finalize = 0 (no fused vector step without the reducer workgroup, so fuse_update is left alone)
TUNING_CASES = {
    "1rank-gatherAp-general-finalize0": (1001, 0, {"exchange": 1, "symmetric": 0, "finalize": 0}),
    "1rank-gatherAp-symmetric-finalize0": (1001, 0, {"exchange": 1, "symmetric": 2, "finalize": 0}),
}
for _join in (1, 0):
    for _sym in (0, 2):
        TUNING_CASES[f"3shards-gatherAp-join{_join}-sym{_sym}-finalize0"] = (
            1001, 3, {"exchange": 1, "exchange_join": _join, "symmetric": _sym, "finalize": 0})

EXPECTED = {
    "1shard-fused/timing1": ((0, 0, 0, 6, 0), (22, 22, 0, 33, 0)),
    "1shard-fused/timing8": ((0, 0, 0, 6, 0), (22, 4, 0, 33, 0)),
    "1shard-two-kernel/timing1": ((0, 0, 0, 4, 0), (33, 22, 0, 55, 0)),
    "1shard-two-kernel/timing8": ((0, 0, 0, 4, 0), (33, 4, 0, 55, 0)),
    "1shard-symmetric/timing1": ((0, 0, 0, 6, 0), (33, 22, 0, 33, 0)),
    "1shard-symmetric/timing8": ((0, 0, 0, 6, 0), (33, 4, 0, 33, 0)),
    "1shard-split/timing1": ((0, 0, 0, 6, 0), (33, 44, 0, 33, 0)),
    "1shard-split/timing8": ((0, 0, 0, 6, 0), (33, 8, 0, 33, 0)),
    "3shards-events/timing1": ((3, 6, 12, 24, 0), (99, 231, 198, 189, 0)),
    "3shards-events/timing8": ((3, 6, 12, 24, 0), (99, 123, 198, 162, 0)),
    "1rank-events-overlap1/timing1": ((1, 2, 1, 7, 2), (33, 110, 21, 45, 33)),
    "1rank-events-overlap1/timing8": ((1, 2, 1, 7, 2), (33, 38, 21, 45, 33)),
    "1rank-events-overlap0/timing1": ((1, 0, 0, 6, 2), (33, 88, 0, 44, 33)),
    "1rank-events-overlap0/timing8": ((1, 0, 0, 6, 2), (33, 16, 0, 44, 33)),
    "1rank-gatherAp-general/timing1": ((0, 0, 0, 5, 1), (22, 44, 0, 22, 11)),
    "1rank-gatherAp-general/timing8": ((0, 0, 0, 5, 1), (22, 8, 0, 22, 11)),
    "1rank-gatherAp-symmetric/timing1": ((0, 0, 0, 5, 1), (33, 44, 0, 23, 11)),
    "1rank-gatherAp-symmetric/timing8": ((0, 0, 0, 5, 1), (33, 8, 0, 23, 11)),
    "3shards-gatherAp-join1-fuse1-sym0/timing1": ((0, 0, 0, 19, 0), (66, 121, 44, 134, 0)),
    "3shards-gatherAp-join1-fuse1-sym0/timing8": ((0, 0, 0, 19, 0), (66, 49, 44, 107, 0)),
    "3shards-gatherAp-join1-fuse1-sym2/timing1": ((0, 0, 0, 19, 0), (99, 121, 44, 137, 0)),
    "3shards-gatherAp-join1-fuse1-sym2/timing8": ((0, 0, 0, 19, 0), (99, 49, 44, 110, 0)),
    "3shards-gatherAp-join1-fuse0-sym0/timing1": ((0, 0, 0, 15, 0), (99, 121, 44, 134, 0)),
    "3shards-gatherAp-join1-fuse0-sym0/timing8": ((0, 0, 0, 15, 0), (99, 49, 44, 107, 0)),
    "3shards-gatherAp-join1-fuse0-sym2/timing1": ((0, 0, 0, 15, 0), (132, 121, 44, 137, 0)),
    "3shards-gatherAp-join1-fuse0-sym2/timing8": ((0, 0, 0, 15, 0), (132, 49, 44, 110, 0)),
    "3shards-gatherAp-join0-fuse1-sym0/timing1": ((0, 0, 0, 19, 0), (66, 121, 66, 123, 0)),
    "3shards-gatherAp-join0-fuse1-sym0/timing8": ((0, 0, 0, 19, 0), (66, 49, 66, 96, 0)),
    "3shards-gatherAp-join0-fuse1-sym2/timing1": ((0, 0, 0, 19, 0), (99, 121, 66, 126, 0)),
    "3shards-gatherAp-join0-fuse1-sym2/timing8": ((0, 0, 0, 19, 0), (99, 49, 66, 99, 0)),
    "3shards-gatherAp-join0-fuse0-sym0/timing1": ((0, 0, 0, 15, 0), (99, 121, 66, 123, 0)),
    "3shards-gatherAp-join0-fuse0-sym0/timing8": ((0, 0, 0, 15, 0), (99, 49, 66, 96, 0)),
    "3shards-gatherAp-join0-fuse0-sym2/timing1": ((0, 0, 0, 15, 0), (132, 121, 66, 126, 0)),
    "3shards-gatherAp-join0-fuse0-sym2/timing8": ((0, 0, 0, 15, 0), (132, 49, 66, 99, 0)),
    "1rank-gatherAp-general-finalize0/timing1": ((0, 0, 0, 2, 1), (44, 44, 0, 22, 11)),
    "1rank-gatherAp-general-finalize0/timing8": ((0, 0, 0, 2, 1), (44, 8, 0, 22, 11)),
    "1rank-gatherAp-symmetric-finalize0/timing1": ((0, 0, 0, 2, 1), (55, 44, 0, 23, 11)),
    "1rank-gatherAp-symmetric-finalize0/timing8": ((0, 0, 0, 2, 1), (55, 8, 0, 23, 11)),
    "3shards-gatherAp-join1-sym0-finalize0/timing1": ((0, 0, 0, 12, 0), (132, 121, 44, 134, 0)),
    "3shards-gatherAp-join1-sym0-finalize0/timing8": ((0, 0, 0, 12, 0), (132, 49, 44, 107, 0)),
    "3shards-gatherAp-join1-sym2-finalize0/timing1": ((0, 0, 0, 12, 0), (165, 121, 44, 137, 0)),
    "3shards-gatherAp-join1-sym2-finalize0/timing8": ((0, 0, 0, 12, 0), (165, 49, 44, 110, 0)),
    "3shards-gatherAp-join0-sym0-finalize0/timing1": ((0, 0, 0, 12, 0), (132, 121, 66, 123, 0)),
    "3shards-gatherAp-join0-sym0-finalize0/timing8": ((0, 0, 0, 12, 0), (132, 49, 66, 96, 0)),
    "3shards-gatherAp-join0-sym2-finalize0/timing1": ((0, 0, 0, 12, 0), (165, 121, 66, 126, 0)),
    "3shards-gatherAp-join0-sym2-finalize0/timing8": ((0, 0, 0, 12, 0), (165, 49, 66, 99, 0)),
}


def measure(lam, n, shards, options, timing):
    """((the five counters' deltas over cg_init), (over cg_iterate(ITERS, 0))) on a fresh context."""
    if shards == 0:
        os.environ["LAM_HIP_FORCE_RCCL"] = "1"      # a one-rank communicator: the rank mode on one GPU
        try:
            s = lam.Solver(lam.F64, rank=0, nranks=1, device_id=0, unique_id=None)
        finally:
            del os.environ["LAM_HIP_FORCE_RCCL"]
    else:
        s = lam.Solver(lam.F64, device_ids=[0] * shards)
    with s:
        s.generate_random_spd(n, 5, 1e4)
        s.generate_random_rhs(6)
        for name, value in options.items():
            s.set_option(name, value)
        s.set_option("gemv_timing", timing)

        def counters():
            return tuple(s.get_option(k) for k in COUNTERS)

        c0 = counters()
        s.cg_init()
        c1 = counters()
        st = s.cg_iterate(ITERS, 0.0)
        c2 = counters()
        assert st["num_iters"] == ITERS + 1 and not st["converged"], st
        if "exchange" in options:
            assert s.get_option("exchange_effective") == options["exchange"]
        if "symmetric" in options:
            assert s.get_option("symmetric_effective") == (1 if options["symmetric"] else 0)
        if "fuse_update" in options:
            assert s.get_option("fuse_effective") == options["fuse_update"]
    return tuple(b - a for a, b in zip(c0, c1)), tuple(b - a for a, b in zip(c1, c2))


@pytest.mark.parametrize("timing", [1, 8], ids=["timing1", "timing8"])
@pytest.mark.parametrize("case", list(CASES))
def test_iteration_runtime_calls(lam, case, timing):
    n, shards, options = CASES[case]
    got = measure(lam, n, shards, options, timing)
    print(f'    "{case}/timing{timing}": {got},')
    assert got == EXPECTED[f"{case}/timing{timing}"]


def test_iteration_runtime_calls_with_separate_reduction_launches(lam):
    """finalize = 0 is an option of the tuning build: one child process on that library (LAM_HIP_TUNING_LIB names another build of it)."""
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tuning_cases.py")
    env = dict(os.environ, LAM_HIP_LIB=os.environ.get("LAM_HIP_TUNING_LIB") or lam.TUNING_LIB)
    r = subprocess.run([sys.executable, script, "call_counts"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok call_counts"), r.stdout[-2000:] + r.stderr[-3000:]
    got = {k: tuple(map(tuple, v)) for k, v in json.loads(r.stdout.strip().splitlines()[-2]).items()}
    for key, value in got.items():
        print(f'    "{key}": {value},')
    assert sorted(got) == sorted(f"{case}/timing{t}" for case in TUNING_CASES for t in (1, 8))
    assert got == {k: v for k, v in EXPECTED.items() if "finalize0" in k}
