"""Rank mode (one context per GPU rank, RCCL exchange) with P > 1 on a ONE-GPU box.

RCCL refuses two ranks on one device, so the P ranks run as P threads of one process (or P processes)
on GPU 0 with a test double LD_PRELOADed in front of librccl.so:

* tests/mock_rccl/mock_rccl_async.hip -- STREAM-ORDERED: every collective is a kernel enqueued on the
  caller's stream that publishes into a shared slot ring and spins on the peers' generation counters;
  nothing synchronises the hosts or a stream.  These are the semantics real RCCL has, so what is pinned
  down is what will hold on 8 GPUs: every rank enqueues the SAME sequence of collectives whatever the
  relative speed of its host and its GPU (the stop protocol), the in-place all-gather offsets, the
  grouped broadcasts of the uneven split, the own-slice GEMV panel running beside the all-gather on a
  second stream of the same communicator, identical stop decisions, the collective gathers of x.
* tests/mock_rccl/mock_rccl_mp.cpp -- host-synchronous, multi-process: the driver's torchrun command.

(The real RCCL calls are exercised with a 1-rank communicator in test_gpu_drivers.py.)"""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT, slow

pytestmark = pytest.mark.gpu
MOCK_DIR = os.path.join(ROOT, "tests", "mock_rccl")


def ITER_GATE(ref_iters):      # noqa: N802
    """max(3, 2 %): the HIP path lands -3 ... 0 iterations from the reference's own counts over 45 fixture x topology runs
    (profiles/r05_parity_margins.txt: 181 against 184 on the n=128 fixture), so SURVEY 8c's max(2, 1 %) would fail it; the
    reference algorithm moves by as much under a different reduction order alone (oracle with 2-8 threads / 2-5 ranks)."""
    return max(3, 0.02 * ref_iters)


def _env(mock, P, tmp_path, **extra):
    stats = os.path.join(str(tmp_path), "mock_stats.jsonl")
    # a kernel that waits for a peer must never share a hardware queue with the kernel it waits for
    env = dict(os.environ, LD_PRELOAD=mock, GPU_MAX_HW_QUEUES=str(2 * P + 4), MOCK_RCCL_STATS_FILE=stats,
               MOCK_RCCL_TIMEOUT_MS="20000")
    env.update({k: str(v) for k, v in extra.items()})
    return env, stats


def _run(mock, tmp_path, P, n, mode, *opts, env_extra=None, expect_ok=True):
    env, stats = _env(mock, P, tmp_path, **(env_extra or {}))
    r = subprocess.run([sys.executable, os.path.join(MOCK_DIR, "run_ranks.py"), str(P), str(n), mode, *map(str, opts)],
                       env=env, capture_output=True, text=True, timeout=600)
    lines = [json.loads(l) for l in open(stats)] if os.path.exists(stats) else []
    if expect_ok:
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1]) if r.stdout.strip() else {}
    return r, out, lines


def _check_mock_stats(lines, P):
    """One line per communicator: nobody timed out or saw a mismatch, and every rank ENQUEUED the same
    number of collectives."""
    assert len(lines) == P, lines
    assert all(l["abort"] == 0 and l["err"] == 0 and l["host_abort"] == 0 for l in lines), lines
    assert len({l["calls"] for l in lines}) == 1, f"ranks enqueued different numbers of collectives: {lines}"


def _check_solution(out, P, n, mode):
    assert out["ranks_identical"], out          # every rank holds the same x, iteration count and residual
    assert out["converged"]
    assert len(set(out["collectives_enqueued"])) == 1, out
    tol = 1e-9 if mode == "tridiag" else 1e-10
    assert abs(out["iters"] - out["iters_single"]) <= ITER_GATE(out["iters_single"]), out
    assert out["true_residual"] <= 2 * tol + 1e-13
    assert out["x_vs_single"] < (1e-5 if mode == "tridiag" else 1e-8), out   # tridiag(1,2,1): cond ~ N^2/2
    assert out["gemv_vs_single"] < 1e-13
    if n <= 5000:
        # tied to the reference algorithm itself (CPU oracle with the same number of emulated ranks, same system) and to a
        # residual recomputed on the host -- not only to another run of the HIP path; file-mode gates
        assert out["converged_oracle"] and abs(out["iters"] - out["iters_oracle"]) <= ITER_GATE(out["iters_oracle"]), out
        assert out["residual_numpy"] <= 2 * tol + 1e-13, out
        # the device's recomputed residual is the host's (only where it is more than rounding noise)
        assert out["true_residual"] < 1e-12 or abs(out["residual_numpy"] / out["true_residual"] - 1) < 1e-3, out
        assert out["x_vs_oracle"] <= (1e-5 if mode == "tridiag" else 10 * tol), out
    base = n // P
    assert out["partition"] == [[q * base, base + (n % P if q == P - 1 else 0)] for q in range(P)]


@pytest.mark.parametrize("P,n,mode,overlap,exchange", [
    slow(2, 1024, "tridiag", 1, 0),     # even split, aligned panels
    (3, 1001, "tridiag", 1, 0),     # odd N: generic kernel; uneven split: grouped broadcasts
    slow(4, 4096, "spd", 1, 0),
    slow(4, 4096, "spd", 0, 0),         # all-gather on the compute stream
    slow(3, 4098, "spd", 1, 0),         # 1366 rows per rank
    (4, 4102, "spd", 1, 0),         # remainder on the last rank, odd row offsets -> no panel split
    (8, 8192, "spd", 1, 0),         # the node shape
    # exchange = 1: ONE all-gather of [Ap slice | p.Ap partial] per iteration, full-length r and p per rank
    slow(2, 1024, "tridiag", 1, 1),
    slow(4, 4096, "spd", 1, 1),
    (8, 8192, "spd", 1, 1),
    (3, 1001, "tridiag", 1, 1),     # uneven split (the reference's: remainder on the last rank): records of the longest slice
    (3, 4098, "spd", 1, 1),
    (6, 5000, "spd", 1, 1),
    (5, 1001, "spd", 1, 1),
    (4, 5, "spd", 1, 1),            # one row per rank, two on the last (all 36 tiny shapes x exchanges: tests/mock_rccl/tiny_ranks.py)
    (8, 8, "spd", 1, 0),
    (8, 8, "spd", 1, 2),
    (24, 4100, "spd", 1, 1),        # beyond 16 ranks (LAM_HIP_MAX_SHARDS = 64 since round 5), uneven split; exchange 0 passes too
                                    # but takes 97 s: its three collectives per iteration time-slice 24 queues of one GPU
    # exchange = 2: direct stores into peer-mapped mailboxes and p replicas, no collective in the iteration
    slow(2, 1024, "tridiag", 1, 2),
    slow(4, 4096, "spd", 1, 2),
    (8, 8192, "spd", 1, 2),
    (3, 1001, "tridiag", 1, 2),     # odd N (generic kernel), uneven split
    slow(4, 4102, "spd", 1, 2),         # odd row offsets: the GEMV is not split
    slow(4, 4096, "spd", 0, 2),         # overlap 0: flag wait first, then ONE GEMV launch
    slow(8, 8192, "spd", 0, 2),
])
def test_rank_mode_multi_rank_on_async_mock(mock_async, tmp_path, P, n, mode, overlap, exchange):
    r, out, lines = _run(mock_async, tmp_path, P, n, mode, "--overlap", overlap, "--exchange", exchange)
    _check_mock_stats(lines, P)
    _check_solution(out, P, n, mode)
    if exchange == 1:
        assert out["exchange_effective"] == [1] * P, out      # any N >= P: no fallback (round 5)
    # the ranks count who shares their GPU once at creation (here: all P of them), so that the fused vector step --
    # whose workgroups wait for each other -- is used only when the launches of ALL ranks on the device are resident together
    assert out["ranks_on_device"] == [P] * P and len(set(out["fuse_effective"])) == 1, out
    # lam_hip_stats.t_exchange: the collectives of exchanges 0 / 1 are bracketed with HIP events on every rank (sampled with the
    # GEMV timing); the direct exchange waits inside its kernels and reports none
    if not (out["direct_fallbacks"][0] if exchange == 2 else 0):
        assert all((t > 0) == (exchange != 2) for t in out["t_exchange"]) and all(t > 0 for t in out["t_gemv"]), out
    if exchange == 2:
        assert out["exchange_effective"] == [2] * P, out
        # set-up and the collective checks after the solve go through the communicator, the iterations do not
        assert out["collectives_enqueued"][0] < 40 + 4 * P, out


@pytest.mark.parametrize("P,n", [slow(2, 1024), slow(4, 4096), (8, 8192), (3, 1001), (6, 5000)])
def test_one_process_gather_ap_is_bit_identical_to_rank_mode_gather_ap(mock_async, tmp_path, P, n):
    """exchange 1 exists in both multi-GPU topologies: one process per GPU (ONE ncclAllGather of [Ap slice | p.Ap partial]
    per iteration) and one process driving all shards (the GEMV stores the records into the peers' buffers itself, one
    event join).  Same kernels, same arithmetic: iteration count, residual and every bit of x must agree."""
    import hashlib
    import importlib
    r, out, lines = _run(mock_async, tmp_path, P, n, "spd", "--exchange", 1, "--no-single")
    _check_mock_stats(lines, P)
    assert out["exchange_effective"] == [1] * P
    # the rank mode's vector step as two kernels (fuse_update 0) instead of update_full_fused_kernel: same bits
    os.remove(os.path.join(str(tmp_path), "mock_stats.jsonl"))
    r2, out2, lines2 = _run(mock_async, tmp_path, P, n, "spd", "--exchange", 1, "--fuse", 0, "--no-single")
    _check_mock_stats(lines2, P)
    assert (out2["iters"], out2["rel_err"], out2["x_sha"]) == (out["iters"], out["rel_err"], out["x_sha"]), (out, out2)
    lam = importlib.import_module("2024-eumaster4hpc-student-challenge_amd")
    for join in (1, 0):
        with lam.Solver(lam.F64, device_ids=[0] * P) as s:
            s.generate_random_spd(n, 99, 200.0)          # run_ranks.py's system
            s.generate_random_rhs(100)
            s.set_option("exchange", 1)
            s.set_option("exchange_join", join)
            s.solve(2000, 1e-10)
            assert s.get_option("exchange_effective") == 1
            got = (s.stats["num_iters"], s.stats["rel_err"], hashlib.sha256(s.solution().tobytes()).hexdigest())
        assert got == (out["iters"], out["rel_err"], out["x_sha"]), (join, got, out)


@pytest.mark.parametrize("P,n", [slow(2, 1024), slow(4, 4096), (8, 8192), slow(3, 3000), (3, 1001), (6, 5000)])
def test_symmetric_product_rank_mode_matches_one_process(mock_async, tmp_path, P, n):
    """Option "symmetric" in rank mode (one process per GPU; here threads on the stream-ordered RCCL double): the iteration's one
    collective gathers every rank's full-length contribution to A p.  Same kernels and the same summation order as one process
    driving all shards: iteration count, residual and every bit of x agree; against the oracle and a numpy residual like every
    multi-rank case."""
    import hashlib
    import importlib
    r, out, lines = _run(mock_async, tmp_path, P, n, "spd", "--exchange", 1, "--symmetric", 2)
    _check_mock_stats(lines, P)
    _check_solution(out, P, n, "spd")
    assert out["exchange_effective"] == [1] * P and out["symmetric_effective"] == [1] * P
    lam = importlib.import_module("2024-eumaster4hpc-student-challenge_amd")
    with lam.Solver(lam.F64, device_ids=[0] * P) as s:
        s.generate_random_spd(n, 99, 200.0)          # run_ranks.py's system
        s.generate_random_rhs(100)
        s.set_option("exchange", 1)
        s.set_option("symmetric", 2)
        s.solve(2000, 1e-10)
        assert s.get_option("symmetric_effective") == 1
        got = (s.stats["num_iters"], s.stats["rel_err"], hashlib.sha256(s.solution().tobytes()).hexdigest())
    assert got == (out["iters"], out["rel_err"], out["x_sha"]), (got, out)


@pytest.mark.parametrize("P,n,mode", [(2, 1024, "tridiag"), slow(4, 4096, "spd"), slow(8, 8192, "spd"), (3, 4098, "spd")])
def test_direct_exchange_is_bit_identical_to_rccl_exchange(mock_async, tmp_path, P, n, mode):
    """exchange 2 sums the ranks' partial dot products with the same reduction tree as exchange 0, so the
    two must produce the same bits: iteration count, residual and every element of x -- in all four launch shapes
    of the direct exchange (own-slice GEMV panel or not; x/r/p updates fused into one launch, with the waiter
    workgroup, or as two kernels behind wait_p_kernel)."""
    def run(ex, overlap, fuse):
        r, out, lines = _run(mock_async, tmp_path, P, n, mode, "--exchange", ex, "--overlap", overlap, "--fuse", fuse, "--no-single")
        _check_mock_stats(lines, P)
        os.remove(os.path.join(str(tmp_path), "mock_stats.jsonl"))
        return out

    # the own-slice panel changes the order in which a row's products are added, so like is compared with like
    for overlap in (1, 0):
        a = run(0, overlap, 1)
        for fuse in (1, 0):
            b = run(2, overlap, fuse)
            assert b["exchange_effective"] == [2] * P
            assert (a["iters"], a["rel_err"], a["x_sha"]) == (b["iters"], b["rel_err"], b["x_sha"]), (overlap, fuse, a, b)


@pytest.mark.parametrize("P,n,mode,exchange,delay,chunk", [
    # GPU outruns the host (small N: an iteration takes a few microseconds), run to convergence
    slow(2, 1024, "tridiag", 0, "", 0),
    (4, 2048, "tridiag", 0, "", 0),
    slow(8, 4096, "spd", 0, "", 0),
    slow(4, 2048, "tridiag", 1, "", 0),
    (8, 4096, "spd", 1, "", 0),
    # one rank's host lags far behind its GPU (it sleeps before every enqueue) while the others run ahead
    slow(2, 1024, "tridiag", 0, "1:150", 0),
    slow(4, 2048, "spd", 0, "2:200", 0),
    slow(4, 2048, "spd", 1, "0:200", 0),
    (8, 4096, "spd", 0, "3:100,6:250", 0),
    # the host outruns the GPU (four 2 GB shards on one GPU: an iteration takes more than a millisecond)
    slow(4, 32768, "spd", 0, "", 0),
    (4, 32768, "spd", 1, "", 0),
    # the solve split over several lam_hip_cg_iterate calls: the stop must also be agreed on across calls
    (4, 2048, "tridiag", 0, "1:100", 7),
    slow(2, 1024, "tridiag", 1, "", 5),
    # the direct exchange under the same stresses
    slow(4, 2048, "tridiag", 2, "", 0),
    (8, 4096, "spd", 2, "3:100,6:250", 0),
    slow(4, 32768, "spd", 2, "", 0),
    slow(4, 2048, "tridiag", 2, "1:100", 7),
])
def test_stop_protocol_keeps_ranks_in_step(mock_async, tmp_path, P, n, mode, exchange, delay, chunk):
    """Convergence under asynchronous collectives: all ranks must enqueue the same number of collectives
    and the collective calls that follow the solve (solution gather, residual, GEMV) must still pair up."""
    opts = ["--exchange", exchange]
    if chunk:
        opts += ["--chunk", chunk]
    if n >= 32768:
        opts += ["--cond", 50.0, "--no-single"]
    r, out, lines = _run(mock_async, tmp_path, P, n, mode, *opts, env_extra={"MOCK_RCCL_HOST_DELAY_US": delay} if delay else None)
    _check_mock_stats(lines, P)
    assert out["converged"] and out["ranks_identical"], out
    assert len(set(out["collectives_enqueued"])) == 1 and len(set(out["iterate_calls"])) == 1, out
    assert out["true_residual"] <= 2 * (1e-9 if mode == "tridiag" else 1e-10) + 1e-13, out
    if "iters_single" in out:
        _check_solution(out, P, n, mode)


@pytest.mark.parametrize("P,n,mode,dtype,exchange", [
    (4, 4096, "spd", "f32", 0), (4, 4096, "spd", "f32", 1), (4, 4096, "spd", "f32", 2),
    (2, 2048, "tridiag", "bf16", 0), (3, 4104, "spd", "bf16", 2),
])
def test_rank_mode_low_precision(mock_async, tmp_path, P, n, mode, dtype, exchange):
    """float vectors (and bf16 matrix storage) through every exchange: the vector element type changes the
    all-gather datatype, the record layout of exchange 1 and the store width of the direct exchange."""
    opts = ["--exchange", exchange, "--dtype", dtype, "--tol", 2e-5]
    if mode == "tridiag":
        opts += ["--iters", 40]            # fixed count: tridiag(1,2,1) needs N/2 iterations, too many for fp32 rounding
    r, out, lines = _run(mock_async, tmp_path, P, n, mode, *opts)
    _check_mock_stats(lines, P)
    assert out["ranks_identical"] and len(set(out["collectives_enqueued"])) == 1, out
    assert abs(out["iters"] - out["iters_single"]) <= 3, out
    assert out["x_vs_single"] < 1e-3 and out["gemv_vs_single"] < 1e-5, out
    if mode == "spd":
        assert out["converged"] and out["true_residual"] < 1e-4, out
    if exchange == 2:
        assert out["exchange_effective"] == [2] * P


def test_finalize_kernel_variant_matches_in_kernel_reduction(mock_async, tmp_path):
    """option finalize=0 (separate 1-block reduction launches, the round-1 chain) and the default in-kernel
    last-arriver reduction give bit-identical solves."""
    import importlib
    tuning = importlib.import_module("2024-eumaster4hpc-student-challenge_amd").TUNING_LIB     # finalize = 0 lives in the tuning build
    outs = []
    for fin in (1, 0):
        r, out, lines = _run(mock_async, tmp_path, 4, 4096, "spd", "--finalize", fin, env_extra={"LAM_HIP_LIB": tuning})
        _check_mock_stats(lines, 4)
        os.remove(os.path.join(str(tmp_path), "mock_stats.jsonl"))
        outs.append(out)
    a, b = outs
    assert a["iters"] == b["iters"] and a["rel_err"] == b["rel_err"] and a["true_residual"] == b["true_residual"]


def test_async_mock_catches_timing_dependent_stop(mock_async, tmp_path):
    """Negative control: with LAM_HIP_DEBUG_LEVEL_STOP the host acts on ANY stop it has seen (the round-1
    protocol).  A rank whose host lags its GPU then leaves the loop earlier than the others, the ranks'
    collective sequences diverge -- and the stream-ordered mock reports it (a host-synchronous one cannot)."""
    stats = os.path.join(str(tmp_path), "mock_stats.jsonl")
    for delay in ("1:200", "0:300", "1:500"):          # the race is timing-dependent by nature: a few tries
        if os.path.exists(stats):
            os.remove(stats)
        r, out, lines = _run(mock_async, tmp_path, 2, 1024, "tridiag", "--no-single", expect_ok=False,
                             env_extra={"MOCK_RCCL_HOST_DELAY_US": delay, "LAM_HIP_DEBUG_LEVEL_STOP": "1",
                                        "MOCK_RCCL_TIMEOUT_MS": "3000"})
        if r.returncode != 0 or len({l["calls"] for l in lines}) != 1 or any(l["abort"] for l in lines):
            return
    pytest.skip("the timing-dependent stop did not desynchronise the ranks in three tries on this box")


def test_direct_exchange_solve_checks_itself_and_falls_back(mock_async, tmp_path):
    """lam_hip_solve on the direct exchange recomputes the residual afterwards (all ranks get the same number); when it
    does not match the recursion -- here because one rank's p replica is perturbed in iteration 3, what a stale read of
    a peer's slice would amount to -- every rank solves again on the RCCL exchange and the caller gets the right
    answer, with the event counted (exchange 2 is experimental until it has run on real peers)."""
    r, out, lines = _run(mock_async, tmp_path, 4, 4096, "spd", "--exchange", 2, env_extra={"LAM_HIP_DEBUG_DIRECT_STALE": "2"})
    _check_mock_stats(lines, 4)
    _check_solution(out, 4, 4096, "spd")
    assert out["direct_fallbacks"] == [1, 1, 1, 1] and out["exchange_effective"] == [0, 0, 0, 0]
    assert "does not match the recursive residual" in r.stderr
    # without the fault: no fallback, the direct exchange stays in use
    r, out, lines = _run(mock_async, tmp_path, 4, 4096, "spd", "--exchange", 2)
    _check_solution(out, 4, 4096, "spd")
    assert out["direct_fallbacks"] == [0, 0, 0, 0] and out["exchange_effective"] == [2, 2, 2, 2]


@pytest.mark.parametrize("overlap", [1, 0])
def test_direct_exchange_context_can_be_destroyed_right_after_iterating(mock_async, tmp_path, overlap):
    """on the direct exchange a rank's last iteration is complete once it has the peers' r.r, while those peers
    may still be storing p slices into its replica.  lam_hip_cg_iterate therefore ends with one stream-ordered agreement, so a
    caller may destroy the context (or set a new problem) the moment it returns -- here 4 ranks as threads of one process
    (plain pointers into each other's allocations: a late store would hit freed memory), three times over."""
    for _ in range(3):
        r, out, lines = _run(mock_async, tmp_path, 4, 4096, "spd", "--exchange", 2, "--overlap", overlap, "--quick-destroy", 25)
        assert out.get("ok") and out["exchange_effective"] == [2] * 4 and len(set(out["rel_err"])) == 1 and out["iters"] == [26] * 4, out
        _check_mock_stats(lines, 4)
        os.remove(os.path.join(str(tmp_path), "mock_stats.jsonl"))


def test_repeated_solves_on_live_rank_contexts(mock_async, tmp_path):
    """tests/mock_rccl/soak_ranks.py, short form (the long one: profiles/r05_soak.txt, 5100 solves): every rank context solves
    twelve systems to convergence one after the other WITHOUT being recreated -- the three exchanges and both overlap settings
    in rotation, the stop agreed on by all ranks every time --; all ranks hold the same bits, every pass repeats the first
    pass's bits, the direct exchange gives the bits of exchange 0, nothing falls back."""
    for P, n, rounds in ((4, 4096, 36), (3, 1001, 36)):
        env, stats = _env(mock_async, P, tmp_path)
        r = subprocess.run([sys.executable, os.path.join(MOCK_DIR, "soak_ranks.py"), str(P), str(n), str(rounds)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and f"{rounds} solves per rank to convergence" in r.stdout and "0 mismatches" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ---- multi-process: the driver's exact torchrun command ------------------------------------------------
def _bench_torchrun(mock, nproc, tmp_path, extra_env=None):
    # LAM_BENCH_DEVICE_IDS / LAM_HIP_DIRECT_SAME_DEVICE: rank 0's one-process legs put all their shards on GPU 0 too
    env = dict(os.environ, LD_PRELOAD=mock, GPU_MAX_HW_QUEUES=str(2 * nproc + 4), MOCK_RCCL_STATS_FILE=os.path.join(str(tmp_path), "st.jsonl"),
               LAM_BENCH_DEVICE_IDS=",".join(["0"] * nproc), LAM_HIP_DIRECT_SAME_DEVICE="1")
    env.update(extra_env or {})
    env.pop("RANK", None); env.pop("WORLD_SIZE", None)
    port = 29700 + nproc + os.getpid() % 100
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", str(nproc), "--steps", "20",
           "--warmup", "3", "--order", "8192", "--full"]
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)


def _check_bench_line(r, nproc):
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout                          # exactly one JSON line, from rank 0
    out = json.loads(lines[0])
    assert out["n_gpus"] == nproc and out["steps"] == 20 and out["scaling"] == "strong" and out["dtype"] == "f64"
    assert out["metric"] == "cg_iterations_per_sec" and out["value"] > 0
    modes = {k: v for k, v in out["exchange_modes"].items() if k != "default"}
    assert set(modes) == {"allgather_x2+allgather_p", "allgather_x2+allgather_p, no overlap", "allgather_Ap",
                          "allgather_Ap + symmetric product (option, not the headline)", "direct_mailboxes", "direct_mailboxes, no split"}
    for m in modes.values():
        assert m.get("value", 0) > 0 and "error" not in m, out["exchange_modes"]
    # the headline is the product's DEFAULT exchange, whatever the others measured (never a minimum over variants)
    assert out["exchange_modes"]["default"] == "allgather_Ap"           # gather-Ap: the rank mode's default since round 5
    assert out["value"] == modes["allgather_Ap"]["value"]
    assert "ONE RCCL all-gather" in out["config"]["parallelism"] and out["exchange_effective"] == 1
    # ... and it checked itself: true == recursive residual, and the same residual as the one-GPU solve of the system
    sc = out["self_check"]
    assert sc["passed"] and sc["true_vs_recursive"] < 1e-6 and sc["vs_one_gpu"] < 1e-9, sc
    # both exchanges solved the same problem: true residuals agree (different rounding only)
    res = [m["rel_residual_true"] for m in modes.values()]
    assert all(abs(r_ / res[0] - 1) < 1e-6 for r_ in res)
    assert abs(out["rel_residual_true"] / out["rel_residual_recursive"] - 1) < 1e-6
    rf = out["roofline"]
    assert rf["bound"] == "hbm" and rf["peak"] == 8000.0 and 0 < rf["frac"] < 1
    assert abs(rf["algorithmic_bytes_per_launch"] - (8.0 * 8192 * 8192 / nproc + 8.0 * (8192 + 8192 / nproc))) < 1
    assert out["host_plumbing"]["torch_imported"] is False     # the N>1 path is torch-free
    # round 5: RCCL names its ranks, every record times its exchange, and the OTHER topology (one process driving all shards) is
    # on the same line, measured by a child of rank 0 before any rank touched the GPU -- its experimental exchange in a child of its own
    assert out["host_plumbing"]["rccl_ranks"] == nproc and out["host_plumbing"]["rccl_calls_enqueued_rank0"] > 0
    assert out["exchange_us"] > 0 and out["gemv_plus_comm_ms"] > out["gemv_ms"]
    assert 0 < out["exchange_us_min_over_ranks"] <= out["exchange_us"]          # min over ranks = the collective's own latency, max = + skew
    assert all(m["exchange_us"] > 0 for k, m in modes.items() if not k.startswith("direct")), modes
    op = out["one_process_topology"]
    assert "error" not in op and op["value"] > 0 and op["n_gpus"] == nproc and op["exchange_us"] > 0 and op["self_check"]["passed"], op
    op_modes = {k: v for k, v in op["exchange_modes"].items() if k != "default"}
    assert len(op_modes) == 6 and all("error" not in m and m["value"] > 0 for m in op_modes.values()), op_modes
    return out


@pytest.mark.parametrize("nproc", [2, slow(4)])
def test_bench_torchrun_path_end_to_end_on_mock_rccl(mock_mp_lib, tmp_path, nproc):
    """The exact command line the driver uses for N > 1 GPUs -- torch.distributed.run, one process per
    rank, the package's own rendezvous (no torch in the workers), unique-id broadcast, both exchange modes,
    max-over-ranks timing, one JSON line from rank 0 -- with every rank on GPU 0 and the multi-process
    (host-synchronous) mock in front of librccl."""
    _check_bench_line(_bench_torchrun(mock_mp_lib, nproc, tmp_path), nproc)


@pytest.mark.parametrize("nproc", [2, slow(4)])
def test_bench_torchrun_path_on_async_mock_across_processes(mock_async, tmp_path, nproc):
    """Same command on the stream-ordered mock with the ranks in SEPARATE processes (slot ring shared
    through HIP IPC): the process-per-GPU shape of the real deployment under asynchronous collectives."""
    r = _bench_torchrun(mock_async, nproc, tmp_path)
    if "HIP IPC is not available" in r.stderr or "hipIpcOpenMemHandle failed" in r.stderr:
        pytest.skip("HIP IPC between processes is not available on this box")
    _check_bench_line(r, nproc)
    lines = [json.loads(l) for l in open(os.path.join(str(tmp_path), "st.jsonl"))]
    # two communicators in this run: the experimental leg's (fresh processes, exchange 2 only) and the headline's -- each with one
    # line per rank, nobody aborted, every rank of a communicator enqueued the same number of collectives
    assert len(lines) == 2 * nproc and all(l["abort"] == 0 and l["err"] == 0 and l["host_abort"] == 0 for l in lines), lines
    counts = sorted(l["calls"] for l in lines)
    assert counts[:nproc] == [counts[0]] * nproc and counts[nproc:] == [counts[-1]] * nproc and counts[0] < counts[-1], counts


@pytest.mark.parametrize("hook,expect", [
    ({"LAM_HIP_DIRECT_DISABLE": "1"}, "fell back"),               # a rank cannot map its peers: all fall back together
    ({"LAM_HIP_DEBUG_DIRECT_DROP": "1"}, "bounded in-kernel wait"),  # a rank stops posting: every wait downstream expires
])
def test_bench_survives_a_failing_direct_exchange(mock_mp_lib, tmp_path, hook, expect):
    """The direct exchange is tried last in bench.py; when it cannot be set up, or a peer goes silent in the
    middle of it (bounded waits of 5 s expire on every rank, the kernels drain, lam_hip_cg_iterate returns an
    error), the run still ends with ONE JSON line carrying the RCCL variants, exit code 0."""
    r = _bench_torchrun(mock_mp_lib, 2, tmp_path, extra_env=hook)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    d = out["exchange_modes"]["direct_mailboxes"]
    assert "value" not in d and expect in d["error"], d
    for k in ("allgather_x2+allgather_p", "allgather_x2+allgather_p, no overlap", "allgather_Ap"):
        assert out["exchange_modes"][k]["value"] > 0
    assert out["value"] > 0 and "direct" not in out["config"]["parallelism"]


def test_bench_line_fails_loudly_when_the_self_check_fails(mock_mp_lib, tmp_path):
    """A multi-GPU line whose residual does not match the one-GPU solve of the same system must not look like a
    result: "value" is null, the reason is in the line, the exit code is non-zero (hook: the reference solves another system)."""
    r = _bench_torchrun(mock_mp_lib, 2, tmp_path, extra_env={"LAM_BENCH_SELFTEST_FAIL": "1", "LAM_BENCH_DIRECT": "0"})
    assert r.returncode != 0
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["value"] is None and out["self_check"]["passed"] is False and "differs from the one-GPU solve" in out["error"]
    assert out["value_unchecked"] > 0


def test_bench_stdout_is_one_json_line_with_real_rccl(tmp_path):
    """`torch.distributed.run --nproc-per-node 1 bench.py` with LAM_HIP_FORCE_RCCL=1: every exchange runs through the
    REAL librccl on a 1-rank communicator.  RCCL prints a version banner to stdout when the communicator is created;
    the driver expects stdout to be the one JSON line, nothing else."""
    env = dict(os.environ, LAM_HIP_FORCE_RCCL="1")
    env.pop("RANK", None); env.pop("WORLD_SIZE", None); env.pop("LD_PRELOAD", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr", "127.0.0.1",
           "--master-port", str(29800 + os.getpid() % 100), os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "10",
           "--warmup", "2", "--order", "8192", "--full"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout[:2000]
    out = json.loads(lines[0])
    assert out["host_plumbing"]["rccl_version"] > 20000 and out["host_plumbing"]["torch_imported"] is False and out["host_plumbing"]["rccl_ranks"] == 1
    assert set(out["exchange_modes"]) >= {"allgather_x2+allgather_p", "allgather_Ap", "direct_mailboxes"}
    vals = [m["rel_residual_true"] for m in out["exchange_modes"].values() if "rel_residual_true" in m]
    assert all(abs(v / vals[0] - 1) < 1e-6 for v in vals)


@pytest.mark.parametrize("gpus", [2, 4])
def test_bench_one_process_topology_records_every_exchange(mock_async, tmp_path, gpus):
    """`python bench.py --gpus N` WITHOUT a launcher: one process drives N shards (the reference's single-process multi-GPU
    class, GPU/local/ConjugateGradient_MultiGPUS_CUDA.cu:326-409).  The line carries every exchange of that topology under
    exchange_modes -- gather-Ap with both joins, the three-join event exchange, the in-kernel flag exchange with and
    without the own-slice panel -- each with its residual check against the one-GPU solve and the host time per step;
    the headline is the library default (gather-Ap).  All shards on GPU 0 here (LAM_BENCH_DEVICE_IDS), one hardware
    queue per stream so that kernels of one shard can wait for kernels of another."""
    env = _one_process_env(mock_async, gpus)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--steps", "20", "--warmup", "3", "--order", "8192", "--full"],
                       env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout[:2000]
    out = json.loads(lines[0])
    assert out["n_gpus"] == gpus and out["value"] > 0 and out["self_check"]["passed"] and out["self_check"]["vs_one_gpu"] < 1e-9
    assert out["exchange_effective"] == 1
    modes = {k: v for k, v in out["exchange_modes"].items() if k != "default"}
    assert len(modes) == 6, list(modes)      # five exchanges + the symmetric product on the default one
    assert out["exchange_modes"]["default"].startswith("gather_Ap") and out["value"] == modes[out["exchange_modes"]["default"]]["value"]
    for name, m in modes.items():
        assert "error" not in m and m["value"] > 0, (name, m)
        # the symmetric product is another algorithm (other rounding): the one-GPU gate is 1e-6 there, 1e-9 for the exchanges
        assert m["vs_one_gpu"] < (1e-6 if "symmetric" in name else 1e-9) and abs(m["rel_residual_true"] / m["rel_residual_recursive"] - 1) < 1e-6, (name, m)
    hosts = {k: v["host_enqueue_us_per_step"] for k, v in modes.items() if "host_enqueue_us_per_step" in v}
    assert len(hosts) == 6 and all(0 < h < 2000 for h in hosts.values()), hosts
    assert "1 process" in out["config"]["parallelism"]
    # round 5: the SAME command also measured the rank mode -- `gpus` fresh processes on the RCCL exchange (here the stream-ordered
    # double, all on GPU 0), started before the parent touched the GPU -- and every record times its exchange step
    assert out["exchange_us"] > 0 and all(m["exchange_us"] > 0 for k, m in modes.items() if not k.startswith("direct")), modes
    rm = out["rank_mode_rccl"]
    assert "error" not in rm and rm["value"] > 0 and rm["rccl_ranks"] == gpus and rm["n_gpus"] == gpus and rm["rccl_calls_enqueued"] > 0, rm
    assert rm["self_check"]["passed"] and rm["self_check"]["vs_one_gpu"] < 1e-9 and rm["exchange_us"] > 0
    rm_modes = {k: v for k, v in rm["exchange_modes"].items() if k != "default"}
    assert {"allgather_x2+allgather_p", "allgather_Ap", "direct_mailboxes", "direct_mailboxes, no split"} <= set(rm_modes), list(rm_modes)
    assert all("error" not in m and m["value"] > 0 for m in rm_modes.values()), rm_modes
    assert abs(rm["rel_residual_true"] / out["rel_residual_true"] - 1) < 1e-6       # both topologies solved the same system


def _one_process_env(mock, gpus, **extra):
    """`python bench.py --gpus N` on a one-GPU box: all shards of the one-process topology on GPU 0 (LAM_BENCH_DEVICE_IDS), one
    hardware queue per stream; the rank-mode legs (N child processes) get the stream-ordered RCCL double through LD_PRELOAD."""
    env = dict(os.environ, LAM_BENCH_DEVICE_IDS=",".join(["0"] * gpus), GPU_MAX_HW_QUEUES=str(2 * gpus + 4), LAM_HIP_DIRECT_SAME_DEVICE="1",
               LD_PRELOAD=mock, MOCK_RCCL_TIMEOUT_MS="20000")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    env.update(extra)
    return env


@pytest.mark.parametrize("victim", ["one_direct", "rank_direct:init", "rank_mode:main"])
def test_bench_headline_survives_a_dying_leg(mock_async, tmp_path, victim):
    """The EXPERIMENTAL exchange (in-kernel flags over peer-mapped memory) has never run on separate GPUs; a memory fault on a peer
    mapping would abort the process that runs it.  bench.py therefore runs it only in child processes of its own: here the test
    hook makes every process of one leg kill itself with SIGKILL in the middle of its measurement (LAM_BENCH_KILL_LEG) -- the line
    still comes out, with the headline and every other record intact and the dead leg as {"error": ...}.  The same for the
    whole rank-mode leg."""
    gpus = 2
    env = _one_process_env(mock_async, gpus, LAM_BENCH_KILL_LEG=victim)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--steps", "20", "--warmup", "3", "--order", "8192", "--leg-timeout", "90", "--full"],
                       env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout[:2000]
    out = json.loads(lines[0])
    assert out["value"] > 0 and out["self_check"]["passed"] and out["exchange_effective"] == 1
    modes = {k: v for k, v in out["exchange_modes"].items() if k != "default"}
    rm = out["rank_mode_rccl"]
    if victim == "one_direct":
        dead = modes["direct (experimental leg)"]
        assert "signal 9" in dead["error"] and len([m for m in modes.values() if m.get("value", 0) > 0]) == 4, modes
        assert rm["value"] > 0 and "direct_mailboxes" in rm["exchange_modes"]
    elif victim.startswith("rank_direct"):
        assert "signal 9" in rm["exchange_modes"]["direct (experimental leg)"]["error"], rm
        assert rm["value"] > 0 and rm["rccl_ranks"] == gpus and len([m for m in modes.values() if m.get("value", 0) > 0]) == 6
    else:
        assert "error" in rm and "value" not in rm, rm
        assert len([m for m in modes.values() if m.get("value", 0) > 0]) == 6


@pytest.mark.parametrize("how,expect_from", [("raise", "leg"), ("hang", "leg"), ("raise:late", "own"), slow("hang:late", "own")])
def test_bench_line_survives_its_own_topology(mock_async, tmp_path, how, expect_from):
    """`python bench.py --gpus 2`: the process's OWN topology runs in a worker thread under a supervisor.  The test hook
    (LAM_BENCH_FAIL_MAIN) makes it raise or hang before anything is measured -- the line's headline then comes from the OTHER
    topology's leg (the rank mode on the RCCL double, measured by child processes beforehand), named as such -- or behind its
    headline measurement, in the comparison modes -- the headline is its own, complete and checked, with "comparison_error" (exit
    code 0).  Exit code 4 when the headline had to come from the leg: the line says why."""
    gpus = 2
    env = _one_process_env(mock_async, gpus, LAM_BENCH_FAIL_MAIN=how, LAM_BENCH_DIRECT="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--steps", "20", "--warmup", "3", "--order", "8192",
                        "--leg-timeout", "90", "--headline-timeout", "8", "--full"], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == (4 if expect_from == "leg" else 0), r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout[:2000]
    out = json.loads(lines[0])
    assert out["n_gpus"] == gpus and out["value"] > 0 and out["self_check"]["passed"], out
    assert abs(out["value"] * out["ms_per_step"] * 1e-3 - 1) < 1e-9
    rf = out["roofline"]
    assert 0 < rf["frac"] < 1 and abs(rf["algorithmic_bytes_per_launch"] - (8.0 * 8192 * 8192 / gpus + 8.0 * (8192 + 8192 / gpus))) < 1
    if expect_from == "leg":
        assert "rank mode" in out["headline_from"] and "1 process/GPU" in out["config"]["parallelism"], out
        assert ("LAM_BENCH_FAIL_MAIN" if how == "raise" else "--headline-timeout") in out["own_topology_error"]
        assert out["host_plumbing"]["rccl_ranks"] == gpus and out["exchange_modes"]["default"] == "allgather_Ap"
        assert abs(out["value"] / out["exchange_modes"]["allgather_Ap"]["value"] - 1) < 1e-12      # rebuilt from the leg's ms_per_step
        assert out["one_process_topology"] == {"error": out["own_topology_error"]} and "rank_mode_rccl" not in out
    else:
        assert "headline_from" not in out and "1 process" in out["config"]["parallelism"]
        assert ("LAM_BENCH_FAIL_MAIN" if how.startswith("raise") else "--headline-timeout") in out["comparison_error"]
        assert out["exchange_modes"]["default"].startswith("gather_Ap") and out["rank_mode_rccl"]["value"] > 0


@pytest.mark.parametrize("how", ["raise", "raise:late"])
def test_bench_torchrun_line_survives_the_rank_mode(mock_mp_lib, tmp_path, how):
    """The driver's torchrun command with the rank mode (the headline of that launch style) failing on every rank: rank 0 still
    prints ONE line -- from the one-process topology's leg when nothing had been measured, its own headline when only the
    comparison modes failed -- before the launcher tears the job down."""
    r = _bench_torchrun(mock_mp_lib, 2, tmp_path, extra_env={"LAM_BENCH_FAIL_MAIN": how, "LAM_BENCH_DIRECT": "0"})
    assert (r.returncode != 0) == (how == "raise")
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:] + r.stderr[-3000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["value"] > 0 and out["self_check"]["passed"], out
    if how == "raise":
        assert "one-process" in out["headline_from"] and "1 process," in out["config"]["parallelism"] and "LAM_BENCH_FAIL_MAIN" in out["own_topology_error"]
        assert out["rank_mode_rccl"] == {"error": out["own_topology_error"]} and out["exchange_modes"]["default"].startswith("gather_Ap")
    else:
        assert "headline_from" not in out and "LAM_BENCH_FAIL_MAIN" in out["comparison_error"] and out["host_plumbing"]["rccl_ranks"] == 2
        assert out["one_process_topology"]["value"] > 0


def test_bench_torchrun_line_survives_a_tear_down(mock_mp_lib, tmp_path):
    """One rank of the rank mode dies at its start while rank 0 waits for it: the launcher tears the job down with SIGTERM, rank 0's
    supervisor (its main thread, never inside a native call; SIGTERM itself: tests/test_bench_cpu.py) prints the line from the
    one-process topology's leg before it goes."""
    r = _bench_torchrun(mock_mp_lib, 2, tmp_path, extra_env={"LAM_BENCH_FAIL_MAIN": "raise", "LAM_BENCH_FAIL_MAIN_RANK": "1", "LAM_BENCH_DIRECT": "0"})
    assert r.returncode != 0
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:] + r.stderr[-3000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["value"] > 0 and out["self_check"]["passed"], out
    # (what rank 0 notices first: the launcher's SIGTERM, or its rendezvous connection to the dead rank closing)
    assert "one-process" in out["headline_from"] and ("SIGTERM" in out["own_topology_error"] or "rendezvous peer" in out["own_topology_error"]), out
