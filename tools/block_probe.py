#!/usr/bin/env python3
"""What an iteration of block CG (lam_hip_solve_block) costs against an iteration of the plain batch (lam_hip_solve_many) of the same
build and K, and what the shared block Krylov space buys end to end.

Per shape (default fp64 N = 65536 and fp32 N = 131072) and per K = 1, 4, 8 (option "symmetric_many" = 0): seconds per iteration with
rel_error = 0, taken as (t_total(I) - t_total(2)) / (I - 2) so that the launches in front of the loop cancel (the block's: one Gram
launch, a copy of 36 partials per workgroup to the host and the init launch).  Profiler off, warmed up, every window at least
`--window-s` seconds of iterations, plain and block ALTERNATED within one process, `--windows` windows each; min / median / spread
((max - min) / min) and ratio = t_block(min) / t_plain(min).  The baseline is the plain batch, never the block code itself.  The
byte model: the block's three vector launches move about 12 K N elements against the plain batch's 9 K N, next to N^2 for the
product; one launch more.

End to end (`--e2e-n`, default 65536, fp64): lam_hip_generate_spectrum_spd with the reference generator's law exp(3.5 U[-1, 1]),
random right-hand sides, rel_error 1e-8, nrhs = 4 and 8: iterations and seconds (stats t_total) of lam_hip_solve_many and of
lam_hip_solve_block, and the worst true residual of each.  Every shape runs in a child process of its own.
usage: block_probe.py [--out FILE] [--windows 5] [--window-s 0.5] [--shapes f64:65536,f32:131072] [--e2e-n 65536]"""
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
SHAPES = "f64:65536,f32:131072"
KS = (1, 4, 8)
E2E_NRHS = (4, 8)
SHORT = 2


def loop(lam, dtype, n, windows, window_s):
    """{K: {"plain": [...], "block": [...]}}: seconds per iteration of each window"""
    import numpy as np
    out = {}
    with lam.Solver(lam.F64 if dtype == "f64" else lam.F32) as s:
        s.generate_random_spd(n, 5, 1e4)
        B = np.random.default_rng(7).uniform(-1, 1, (max(KS), n)).astype(s.vec_dtype)

        def per_iteration(solve, iters):
            solve(SHORT)
            t_short = s.stats["t_total"]
            solve(iters)
            return (s.stats["t_total"] - t_short) / (iters - SHORT)

        def block(iters):
            s.solve_block(iters, 0.0)
            if s.breakdown != (0, 0) or s.stats["num_iters"] != iters:
                raise RuntimeError(f"block CG with rel_error = 0 ended after {s.stats['num_iters']} of {iters} iterations: {s.breakdown}")

        for K in KS:
            s.set_rhs_many(B[:K])
            modes = [("plain", lambda i: s.solve_many(i, 0.0)), ("block", block)]
            iters = max(10, int(math.ceil(window_s / max(per_iteration(modes[0][1], 20), 1e-7))))
            for _, solve in modes:                    # every kernel and every allocation before the first window
                per_iteration(solve, iters)
            t = {name: [] for name, _ in modes}
            for _ in range(windows):
                for name, solve in modes:
                    t[name].append(per_iteration(solve, iters))
            out[str(K)] = t
    return out


def end_to_end(lam, n):
    import numpy as np
    tol = 1e-8
    rng = np.random.default_rng(11)
    eig = np.exp(3.5 * rng.uniform(-1, 1, n))
    out = {"n": n, "tol": tol, "runs": {}}
    with lam.Solver(lam.F64) as s:
        s.generate_spectrum_spd(eig, rng.uniform(-1, 1, (3, n)))
        B = rng.uniform(-1, 1, (max(E2E_NRHS), n))
        for nrhs in E2E_NRHS:
            s.set_rhs_many(B[:nrhs])
            s.solve_many(10, 0.0)                     # warm-up of both
            s.solve_block(10, 0.0)
            s.solve_many(20000, tol)
            plain = dict(iters=int(s.stats["num_iters"]), fastest=int(s.num_iters_many.min()), seconds=s.stats["t_total"],
                         true=float(s.true_residuals().max()))
            s.solve_block(20000, tol)
            block = dict(iters=int(s.stats["num_iters"]), seconds=s.stats["t_total"], true=float(s.true_residuals().max()),
                         breakdown=list(s.breakdown), converged=bool(s.converged_many.all()))
            out["runs"][str(nrhs)] = dict(plain=plain, block=block)
    return out


def run_child(*args):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + [str(a) for a in args], capture_output=True, text=True,
                       timeout=1500)
    if p.returncode != 0 or not p.stdout.strip():
        raise RuntimeError("child failed: " + p.stderr[-600:])
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        sys.path.insert(0, ROOT)
        lam = importlib.import_module(PKG)
        if sys.argv[2] == "e2e":
            print(json.dumps(end_to_end(lam, int(sys.argv[3]))))
        else:
            print(json.dumps(loop(lam, sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), float(sys.argv[5]))))
        return
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.5)
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--e2e-n", type=int, default=65536)
    a = ap.parse_args()
    if a.windows < 3:
        ap.error("--windows must be at least 3")
    lines = []

    def emit(text=""):
        print(text, flush=True)
        lines.append(text)

    def fig(v):
        return f"{min(v) * 1e3:9.4f} {statistics.median(v) * 1e3:9.4f} {(max(v) - min(v)) / min(v) * 100:6.2f}%"

    emit(f"block_probe: windows >= {a.window_s} s, {a.windows} windows per figure, alternated; ms per iteration: min median spread")
    for shape in [x for x in a.shapes.split(",") if x]:
        dtype, n = shape.split(":")
        n = int(n)
        r = run_child(dtype, n, a.windows, a.window_s)
        emit()
        emit(f"== {dtype} N = {n}, symmetric_many = 0")
        emit(f"{'':>16}  {'min':>9} {'median':>9} {'spread':>7} {'ratio':>8} {'added ms':>9}")
        for K in KS:
            t = r[str(K)]
            base = min(t["plain"])
            emit(f"{f'K = {K} plain':>16}  {fig(t['plain'])} {1.0:8.4f}")
            emit(f"{f'K = {K} block':>16}  {fig(t['block'])} {min(t['block']) / base:8.4f} {(min(t['block']) - base) * 1e3:9.4f}")
    if a.e2e_n > 0:
        e = run_child("e2e", a.e2e_n)
        emit()
        emit(f"== end to end: fp64 N = {e['n']}, spectrum exp(3.5 U[-1, 1]), rel_error {e['tol']:g}")
        for nrhs in E2E_NRHS:
            p, b = e["runs"][str(nrhs)]["plain"], e["runs"][str(nrhs)]["block"]
            emit(f"nrhs = {nrhs}  plain  {p['iters']:5d} iterations (fastest column {p['fastest']})  {p['seconds']:.3f} s  "
                 f"{p['seconds'] / p['iters'] * 1e3:.3f} ms / iteration  worst true residual {p['true']:.2e}")
            emit(f"nrhs = {nrhs}  block  {b['iters']:5d} iterations (converged: {b['converged']}, breakdown {tuple(b['breakdown'])})  "
                 f"{b['seconds']:.3f} s  {b['seconds'] / max(b['iters'], 1) * 1e3:.3f} ms / iteration  worst true residual {b['true']:.2e}")
            emit(f"nrhs = {nrhs}  time to solution block / plain = {b['seconds'] / p['seconds']:.3f}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
