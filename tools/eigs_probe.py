#!/usr/bin/env python3
"""What a step of the Lanczos eigensolver (lam_hip_eigs) costs against an iteration of the K = 1 batched CG (lam_hip_solve_many) of
the same build.

Per shape (default fp64 N = 65536 and fp32 N = 131072), per option "symmetric_many" = 0 and 2, and per steps = 64, 128, 256: seconds
per step of an eigs run of exactly that many steps (tol = 0: nothing stops; t_iter = the loop's wall time / steps, the host's
convergence checks and their drained stream included) with check_every = 8, the default, and with check_every = steps (one check at
the end), against seconds per iteration of solve_many with rel_error = 0.  Profiler off, warmed up, every CG window at least 0.5 s, the
figures ALTERNATED within one process, `--windows` windows each; min / median / spread ((max - min) / min) and
ratio = t_step(min) / t_cg(min).  A step is the same product launch plus six vector launches; by the byte model the average step of a
run of `steps` steps moves about 2 * steps * N more elements than the product's N^2, so the expectation printed beside each ratio is
1 + 2 * steps / N.  Every shape runs in a child process of its own.
usage: eigs_probe.py [--out FILE] [--windows 5] [--shapes f64:65536,f32:131072]"""
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
STEPS = (64, 128, 256)
SYM = (0, 2)


def loop(lam, dtype, n, windows):
    """{sym: {"cg": [...], "eigs<steps>/<check_every>": [...]}}: seconds per iteration / step of each window"""
    import numpy as np
    out = {}
    with lam.Solver(lam.F64 if dtype == "f64" else lam.F32) as s:
        s.generate_random_spd(n, 5, 1e4)
        b = np.random.default_rng(7).uniform(-1, 1, (1, n)).astype(s.vec_dtype)

        def cg(iters):
            s.set_rhs_many(b)
            s.solve_many(iters, 0.0)
            return s.stats["t_iter"]

        def eigs(steps, check_every):
            return s.eigs(1, "smallest", max_steps=steps, tol=0.0, check_every=check_every, seed=1)["stats"]["t_iter"]

        for sym in SYM:
            s.set_option("symmetric_many", sym)
            iters = max(10, int(math.ceil(WINDOW_S / max(cg(20), 1e-7))))
            modes = [("cg", lambda: cg(iters))]
            for st in STEPS:
                modes.append((f"eigs{st}/8", lambda st=st: eigs(st, 8)))
                modes.append((f"eigs{st}/{st}", lambda st=st: eigs(st, st)))
            eigs(max(STEPS), 8)                     # the basis for the largest run, and every kernel, before the first window
            t = {name: [] for name, _ in modes}
            for _ in range(windows):
                for name, run in modes:
                    t[name].append(run())
            out[str(sym)] = t
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

    emit(f"eigs_probe: CG windows >= {WINDOW_S} s, {a.windows} windows per figure, alternated; ms per iteration / step: min median spread")
    for shape in a.shapes.split(","):
        dtype, n = shape.split(":")
        n = int(n)
        m = run_child(dtype, n, a.windows)
        for sym in SYM:
            t = m[str(sym)]
            cg = min(t["cg"])
            emit()
            emit(f"== {dtype} N = {n}, symmetric_many = {sym}")
            emit(f"{'':>14}  {'min':>9} {'median':>9} {'spread':>7} {'ratio':>8} {'1 + 2 steps / N':>16}")
            emit(f"{'cg K = 1':>14}  {fig(t['cg'])} {1.0:8.4f}")
            for st in STEPS:
                for ce in (8, st):
                    v = t[f"eigs{st}/{ce}"]
                    emit(f"{f'eigs {st} / {ce}':>14}  {fig(v)} {min(v) / cg:8.4f} {1 + 2 * st / n:16.4f}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
