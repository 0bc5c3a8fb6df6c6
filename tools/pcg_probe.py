#!/usr/bin/env python3
"""What an iteration of the Jacobi-preconditioned batched solve costs next to a plain batched one (lam_hip_solve_many_pc against
lam_hip_solve_many), and what it saves on the generated SPD matrix.

Per shape (default fp64 N = 65536, fp32 N = 131072) and K = 1, 4, 8: profiler off, both shapes warmed up first, every timed window
at least 0.5 s with rel_error = 0 (nothing stops), plain and preconditioned ALTERNATED within one process, `--windows` windows each:
  t_plain, t_jacobi   ms per iteration, min / median / spread ((max - min) / min) of the windows
  ratio               t_jacobi(min) / t_plain(min); the claim is 1 to within the plain path's own spread (three launches either
                      way, 2 N more vector elements read against N^2 matrix elements)
and, once per shape, the iteration counts of both on lam_hip_generate_random_spd(seed 5, cond 1e4), tolerance 1e-10 / 1e-5.
usage: pcg_probe.py [--out FILE] [--windows 5] [--shapes f64:65536,f32:131072]"""
import argparse
import importlib
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOW_S = 0.5
SHAPES = "f64:65536,f32:131072"
KS = (1, 4, 8)


def _iters_for(t_iter):
    return max(10, int(math.ceil(WINDOW_S / max(t_iter, 1e-7))))


def measure(lam, dtype, n, windows):
    import numpy as np
    out = {}
    with lam.Solver(lam.F64 if dtype == "f64" else lam.F32) as s:
        s.generate_random_spd(n, 5, 1e4)
        B = np.random.default_rng(7).uniform(-1, 1, (8, n)).astype(s.vec_dtype)
        for K in KS:
            s.set_rhs_many(B[:K])
            iters = {}
            for pc in (lam.PC_NONE, lam.PC_JACOBI):
                s.solve_many(20, 0.0, pc)
                iters[pc] = _iters_for(s.stats["t_iter"])
            t = {lam.PC_NONE: [], lam.PC_JACOBI: []}
            for _ in range(windows):
                for pc in (lam.PC_NONE, lam.PC_JACOBI):
                    s.solve_many(iters[pc], 0.0, pc)
                    t[pc].append(s.stats["t_iter"])
            out[K] = (t[lam.PC_NONE], t[lam.PC_JACOBI])
        tol = 1e-10 if dtype == "f64" else 1e-5
        s.set_rhs_many(B[:4])
        s.solve_many(4000, tol)
        plain = (s.num_iters_many.tolist(), s.converged_many.tolist())
        s.solve_many(4000, tol, lam.PC_JACOBI)
        jac = (s.num_iters_many.tolist(), s.converged_many.tolist())
    return out, tol, plain, jac


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--shapes", default=SHAPES)
    a = ap.parse_args()
    if a.windows < 3:
        ap.error("--windows must be at least 3")
    sys.path.insert(0, ROOT)
    lam = importlib.import_module("2024-eumaster4hpc-student-challenge_amd")
    lines = []

    def emit(text=""):
        print(text, flush=True)
        lines.append(text)

    def fig(v):
        return f"{min(v) * 1e3:9.4f} {statistics.median(v) * 1e3:9.4f} {(max(v) - min(v)) / min(v) * 100:6.2f}%"

    emit(f"pcg_probe: windows >= {WINDOW_S} s, {a.windows} per figure, plain and jacobi alternated; ms per iteration: min median spread")
    for shape in a.shapes.split(","):
        dtype, n = shape.split(":")
        n = int(n)
        m, tol, plain, jac = measure(lam, dtype, n, a.windows)
        emit()
        emit(f"== {dtype} N = {n}")
        emit(f"{'K':>2}  {'t_plain: min':>12} {'median':>9} {'spread':>7}   {'t_jacobi: min':>13} {'median':>9} {'spread':>7}   {'ratio':>6}")
        for K in KS:
            p, j = m[K]
            emit(f"{K:>2}  {fig(p):>30}   {fig(j):>31}   {min(j) / min(p):6.4f}")
        emit(f"generate_random_spd(5, 1e4), 4 columns, tolerance {tol:g}: plain iterations {plain[0]} converged {plain[1]}; "
             f"jacobi {jac[0]} converged {jac[1]}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
