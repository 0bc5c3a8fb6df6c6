#!/usr/bin/env python3
"""What option "packed_many" buys: the batched product on the 7-byte image (multi_gemv_packed_kernel) against the plain batched product
(multi_gemv_kernel) of the same build, in one process (the method of tools/symv_many_probe.py).

Per size (fp64 N = 65536 and 32768), profiler off, every kernel shape warmed up first, every timed window at least 0.5 s, packed_many
0 and 1 alternated within one process, minimum and median of `--windows` (>= 5) windows, K = 1, 2, 4:
  product(K)     gemv_many_only, seconds per product; share = bytes of the product's model / time / 8 TB/s
  t_batch(K)     seconds per iteration of solve_many with rel_error = 0
  t_minres(K)    seconds per iteration of solve_minres with rel_error = 0
A K is ADMITTED to automatic mode (lam_multi.h pack_many_admitted) when its packed product is faster than the plain one by more than
the spread between the windows of the two figures (median - minimum, the larger of the two) at every size measured.
break-even = pack time / (plain - packed product time): the products after which the image has paid for itself (kPackAfter = 65).
usage: packed_many_probe.py [--out FILE] [--windows 5] [--sizes 65536,32768]"""
import argparse
import importlib
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK = 8.0e12
WINDOW_S = 0.5
KS = (1, 2, 4)


def _iters_for(t_iter):
    return max(10, int(math.ceil(WINDOW_S / max(t_iter, 1e-7))))


def measure(lam, n, windows):
    import numpy as np
    with lam.Solver(lam.F64) as s:
        s.generate_random_spd(n, 5, 1e6)
        B = np.random.default_rng(7).uniform(-1, 1, (4, n))

        def batch(K, iters):
            s.set_rhs_many(B[:K])
            s.solve_many(iters, 0.0)
            return s.stats

        def minres(K, iters):
            s.set_rhs_many(B[:K])
            s.solve_minres(iters, 0.0)
            return s.stats

        it = {}
        for opt in (0, 1):
            s.set_option("packed_many", opt)
            for K in KS:
                it["prod", K, opt] = _iters_for(s.gemv_many_only(K, 10))
                assert s.get_option("packed_many_effective") == opt, "the image was refused"
                it["batch", K, opt] = _iters_for(batch(K, 20)["t_iter"])
                it["minres", K, opt] = _iters_for(minres(K, 20)["t_iter"])
        pack_s = s.get_option("packed_pack_ns") * 1e-9
        res = {k: [] for k in it}
        bytes_model = {}
        for _ in range(windows):
            for K in KS:
                for opt in (0, 1):
                    s.set_option("packed_many", opt)
                    res["prod", K, opt].append(s.gemv_many_only(K, it["prod", K, opt]))
                    st = batch(K, it["batch", K, opt])
                    assert s.get_option("multi_rhs_k") == K and s.get_option("packed_many_effective") == opt
                    res["batch", K, opt].append(st["t_iter"])
                    bytes_model[K, opt] = st["gemv_bytes"]
                    res["minres", K, opt].append(minres(K, it["minres", K, opt])["t_iter"])
        s.set_option("packed_many", 0)
    return res, bytes_model, pack_s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--sizes", default="65536,32768")
    a = ap.parse_args()
    if a.windows < 5:
        ap.error("--windows must be at least 5")
    sys.path.insert(0, ROOT)
    lam = importlib.import_module("2024-eumaster4hpc-student-challenge_amd")
    lines = []

    def emit(text=""):
        print(text, flush=True)
        lines.append(text)

    def flush_out():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    mm = lambda v: (min(v), statistics.median(v))      # noqa: E731
    emit(f"packed_many_probe: fp64, windows >= {WINDOW_S} s, {a.windows} per figure, min / median; ms per product (or per iteration)")
    verdict = {K: True for K in KS}
    for n in (int(v) for v in a.sizes.split(",")):
        res, bytes_model, pack_s = measure(lam, n, a.windows)
        emit()
        emit(f"== fp64 N = {n}   pack time {pack_s * 1e3:.2f} ms")
        emit(f"{'what':>8} {'K':>2} {'plain min':>10} {'median':>9} {'packed min':>11} {'median':>9} {'pck/pln':>8} {'spread':>8} {'faster':>7} "
             f"{'share pln':>9} {'share pck':>9} {'break-even':>10}")
        for what in ("prod", "batch", "minres"):
            for K in KS:
                a0, a0m = mm(res[what, K, 0])
                a1, a1m = mm(res[what, K, 1])
                spread = max(a0m - a0, a1m - a1)
                wins = a0 - a1 > spread
                if what == "prod":
                    verdict[K] = verdict[K] and wins
                    extra = (f"{bytes_model[K, 0] / a0 / PEAK:9.3f} {bytes_model[K, 1] / a1 / PEAK:9.3f} "
                             f"{(pack_s / (a0 - a1) if a0 > a1 else float('inf')):10.1f}")
                else:
                    extra = ""
                emit(f"{what:>8} {K:>2} {a0 * 1e3:10.4f} {a0m * 1e3:9.4f} {a1 * 1e3:11.4f} {a1m * 1e3:9.4f} {a1 / a0:8.4f} {spread * 1e3:8.4f} "
                     f"{'yes' if wins else 'NO':>7} {extra}")
        flush_out()
    emit()
    emit("admitted to automatic mode (the packed product faster by more than the spread at every size): " +
         ", ".join(f"K = {K}: {'yes' if verdict[K] else 'NO'}" for K in KS))
    flush_out()


if __name__ == "__main__":
    main()
