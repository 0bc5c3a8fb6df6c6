#!/usr/bin/env python3
"""What a step of the batched Lanczos quadrature (lam_hip_lanczos_many) costs against an iteration of batched MINRES
(lam_hip_solve_many_minres) of the same build and the same K.

Per shape (default fp64 N = 65536 and fp32 N = 131072) and K = 1, 4, 8, plus K = 4 under option "symmetric_many" = 2: seconds per
step / iteration (the calls' own stats t_iter; rel_error = 0, so MINRES never stops, and no probe of this matrix breaks down) of
  minres    solve_minres, no shifts, K right-hand sides
  lanczos   lanczos_many, K Rademacher probes built on the device: one group at this K
profiler off, warmed up, every window at least 0.5 s, the two ALTERNATED within one process, `--windows` windows each; min / median /
spread ((max - min) / min) and ratio = t_lanczos(min) / t_minres(min).  Both run one product launch (two under "symmetric_many") and
two vector launches per step; the byte model puts the quadrature's vector launches at about 7 K N elements (MINRES': about 14 K N)
against N^2 for the product.
Every shape runs in a child process of its own.
usage: quadrature_probe.py [--out FILE] [--windows 5] [--shapes f64:65536,f32:131072]"""
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
CASES = ((1, 0), (4, 0), (8, 0), (4, 2))     # (K, symmetric_many)
MODES = ("minres", "lanczos")
MAX_STEPS = 256                              # LAM_HIP_MAX_LANCZOS: a window of the quadrature is several calls of at most this many steps


def _iters_for(t_iter):
    return max(10, int(math.ceil(WINDOW_S / max(t_iter, 1e-7))))


def loop(lam, dtype, n, windows):
    """{"K/sym": {mode: [seconds per step of each window]}}"""
    import numpy as np
    out = {}
    with lam.Solver(lam.F64 if dtype == "f64" else lam.F32) as s:
        s.generate_random_spd(n, 5, 1e4)
        B = np.random.default_rng(7).uniform(-1, 1, (8, n)).astype(s.vec_dtype)

        def run(mode, iters, K):
            if mode == "minres":
                s.set_rhs_many(B[:K])                 # clears the shifts: every window starts from the same state
                s.solve_minres(iters, 0.0)
                return s.stats["t_iter"]
            t, left = 0.0, iters
            while left > 0:                           # the step count of one call is capped: a window is several calls
                m = min(left, MAX_STEPS)
                r = s.lanczos_many(K, m, 11)
                assert int(r["steps_run"].min()) == m, "a probe broke down: the window would be short"
                t += s.stats["t_iter"] * m
                left -= m
            return t / iters

        for K, sym in CASES:
            s.set_option("symmetric_many", sym)
            iters = {m: _iters_for(run(m, 20, K)) for m in MODES}
            t = {m: [] for m in MODES}
            for _ in range(windows):
                for m in MODES:
                    t[m].append(run(m, iters[m], K))
            assert s.get_option("symmetric_many_effective") == (1 if sym else 0)
            out[f"{K}/{sym}"] = t
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

    emit(f"quadrature_probe: windows >= {WINDOW_S} s, {a.windows} per figure, minres / lanczos alternated; ms per step: min median spread")
    for shape in a.shapes.split(","):
        dtype, n = shape.split(":")
        n = int(n)
        m = run_child(dtype, n, a.windows)
        emit()
        emit(f"== {dtype} N = {n}   (vector launches by the byte model: 7 K N / N^2 = {7 * 8 / n * 100:.3f} % of the product's elements at K = 8)")
        emit(f"{'K':>2} {'sym':>3}  {'t_minres: min':>13} {'median':>9} {'spread':>7}   {'t_lanczos: min':>14} {'median':>9} {'spread':>7} {'ratio':>7}")
        for K, sym in CASES:
            t = m[f"{K}/{sym}"]
            emit(f"{K:>2} {sym:>3}  {fig(t['minres']):>31}   {fig(t['lanczos']):>32} {min(t['lanczos']) / min(t['minres']):7.4f}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
