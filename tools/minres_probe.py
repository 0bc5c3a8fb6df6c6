#!/usr/bin/env python3
"""What an iteration of batched MINRES (lam_hip_solve_many_minres) costs against an iteration of batched CG (lam_hip_solve_many) of
the same build and the same K.

Per shape (default fp64 N = 65536 and fp32 N = 131072) and K = 1, 4, 8: seconds per iteration with rel_error = 0 (nothing stops) of
  cg        solve_many, no shifts
  minres    solve_minres, no shifts                     (the same unshifted product launch)
  minres+-  solve_minres under shifts of both signs     (the SHIFT product)
profiler off, warmed up, every window at least 0.5 s, the three ALTERNATED within one process, `--windows` windows each; min / median /
spread ((max - min) / min) and ratio = t(min) / t_cg(min).  Both methods run one product and two vector launches per iteration; the
byte model puts MINRES' vector launches at about 14 K N elements (CG's: about 9 K N) against N^2 for the product.
Every shape runs in a child process of its own.
usage: minres_probe.py [--out FILE] [--windows 5] [--shapes f64:65536,f32:131072]"""
import argparse
import importlib
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "2024-eumaster4hpc-student-challenge_amd"
WINDOW_S = 0.5
SHAPES = "f64:65536,f32:131072"
KS = (1, 4, 8)
MIXED_SHIFTS = (-0.5, 0.5, -1e-3, 2.0, -0.25, 1e-2, -8.0, 1.0)
MODES = ("cg", "minres", "minres+-")


def _iters_for(t_iter):
    return max(10, int(math.ceil(WINDOW_S / max(t_iter, 1e-7))))


def loop(lam, dtype, n, windows):
    """{K: {mode: [seconds per iteration of each window]}}"""
    import numpy as np
    out = {}
    with lam.Solver(lam.F64 if dtype == "f64" else lam.F32) as s:
        s.generate_random_spd(n, 5, 1e4)
        B = np.random.default_rng(7).uniform(-1, 1, (8, n)).astype(s.vec_dtype)

        def run(mode, iters, K):
            s.set_rhs_many(B[:K])                     # clears the shifts: every window starts from the same state
            if mode == "cg":
                s.solve_many(iters, 0.0)
            else:
                s.solve_minres(iters, 0.0, MIXED_SHIFTS[:K] if mode == "minres+-" else None)
            return s.stats["t_iter"]

        for K in KS:
            iters = {m: _iters_for(run(m, 20, K)) for m in MODES}
            t = {m: [] for m in MODES}
            for _ in range(windows):
                for m in MODES:
                    t[m].append(run(m, iters[m], K))
            out[str(K)] = t
    return out


def run_child(dtype, n, windows):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", dtype, str(n), str(windows)], capture_output=True, text=True,
                       timeout=1500)
    if p.returncode != 0 or not p.stdout.strip():
        raise RuntimeError("loop child failed: " + p.stderr[-600:])
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        sys.path.insert(0, ROOT)
        print(json.dumps(loop(importlib.import_module(PKG), sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))))
        return
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

    def fig(v):
        return f"{min(v) * 1e3:9.4f} {statistics.median(v) * 1e3:9.4f} {(max(v) - min(v)) / min(v) * 100:6.2f}%"

    emit(f"minres_probe: windows >= {WINDOW_S} s, {a.windows} per figure, cg / minres / minres+- alternated; ms per iteration: min median spread")
    for shape in a.shapes.split(","):
        dtype, n = shape.split(":")
        n = int(n)
        m = run_child(dtype, n, a.windows)
        emit()
        emit(f"== {dtype} N = {n}   (vector launches by the byte model: 14 K N / N^2 = {14 * 8 / n * 100:.3f} % of the product's elements at K = 8)")
        emit(f"{'K':>2}  {'t_cg: min':>9} {'median':>9} {'spread':>7}   {'t_minres: min':>13} {'median':>9} {'spread':>7} {'ratio':>7}   "
             f"{'t_minres+-: min':>15} {'median':>9} {'spread':>7} {'ratio':>7}")
        for K in KS:
            t = m[str(K)]
            cg = min(t["cg"])
            emit(f"{K:>2}  {fig(t['cg'])}   {fig(t['minres']):>31} {min(t['minres']) / cg:7.4f}   {fig(t['minres+-']):>33} {min(t['minres+-']) / cg:7.4f}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
