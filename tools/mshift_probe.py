#!/usr/bin/env python3
"""What an iteration of multi-shift CG (lam_hip_solve_mshift) costs next to the K = 1 shifted batch it rides on and next to the shifted
batches of 8 it replaces.

Per shape (default fp64 N = 65536 and fp32 N = 131072) and S = 8, 16, 64 shifts on lam_hip_generate_random_spd, rel_error = 0 (nothing
stops) and a fixed cap: seconds per iteration (lam_hip_stats.t_iter) of
    k1      solve_shifted(b, [s_min]): the K = 1 shifted batch alone
    mshift  solve_multishift(b, shifts)
    batch   solve_shifted(b, 8 shifts at a time) in ceil(S / 8) batches, their t_iter added up: an iteration of the whole sweep
One process, profiler off, warmed up, every window at least 0.5 s, the three ALTERNATED, `--windows` windows each; min / median /
spread ((max - min) / min).  The shifts are small against the spectrum, so that no zeta leaves fp64's range within the cap; the
probe checks that no shift froze.
usage: mshift_probe.py [--out FILE] [--windows 5] [--shapes f64:65536,f32:131072]"""
import argparse
import importlib
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "2024-eumaster4hpc-student-challenge_amd"
WINDOW_S = 0.5
SHAPES = "f64:65536,f32:131072"
NSHIFTS = (8, 16, 64)


def _iters_for(t_iter):
    return max(10, int(math.ceil(WINDOW_S / max(t_iter, 1e-7))))


def probe(lam, dtype, n, windows, emit):
    import numpy as np
    with lam.Solver(lam.F64 if dtype == "f64" else lam.F32) as s:
        s.generate_random_spd(n, 5, 1e4)
        b = np.random.default_rng(7).uniform(-1, 1, n).astype(s.vec_dtype)
        for S in NSHIFTS:
            sh = 1e-3 * (1.0 + np.random.default_rng(S).permutation(S))      # 1e-3 ... S e-3, in no order
            groups = [sh[f:f + 8] for f in range(0, S, 8)]

            def k1(iters):
                s.solve_shifted(b, [sh.min()], iters, 0.0)
                return s.stats["t_iter"]

            def mshift(iters):
                s.solve_multishift(b, sh, iters, 0.0)
                assert (s.num_iters_shift == iters + 1).all(), ("a shift froze or stopped", s.num_iters_shift.tolist())
                return s.stats["t_iter"]

            def batch(iters):
                t = 0.0
                for g in groups:
                    s.solve_shifted(b, g, iters, 0.0)
                    t += s.stats["t_iter"]
                return t

            modes = (("k1", k1), ("mshift", mshift), ("batch", batch))
            iters = max(_iters_for(f(20)) for _, f in modes[:2])      # one cap for all three: the windows of k1 and mshift >= 0.5 s
            t = {name: [] for name, _ in modes}
            for _ in range(windows):
                for name, f in modes:
                    t[name].append(f(iters))
            lo = {name: min(v) for name, v in t.items()}
            for name, _ in modes:
                v = t[name]
                emit(f"{dtype} N={n} S={S:>2} cap={iters:>4} {name:>6}: {min(v) * 1e3:9.4f} {statistics.median(v) * 1e3:9.4f} "
                     f"{(max(v) - min(v)) / min(v) * 100:6.2f}%")
            emit(f"{dtype} N={n} S={S:>2}: mshift / k1 = {lo['mshift'] / lo['k1']:.4f}; mshift / batch = {lo['mshift'] / lo['batch']:.4f} "
                 f"(1 / {lo['batch'] / lo['mshift']:.2f}); step bytes 4 S N esz = {4 * S * n * b.itemsize / 1e6:.1f} MB")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--shapes", default=SHAPES)
    a = ap.parse_args()
    if a.windows < 3:
        ap.error("--windows must be at least 3")
    lines = []

    def emit(text=""):
        print(text, flush=True)
        lines.append(text)

    sys.path.insert(0, ROOT)
    lam = importlib.import_module(PKG)
    emit(f"mshift_probe: windows >= {WINDOW_S} s, {a.windows} per figure, k1 / mshift / batch alternated; ms per iteration: min median spread")
    for shape in a.shapes.split(","):
        dtype, n = shape.split(":")
        probe(lam, dtype, int(n), a.windows, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
