#!/usr/bin/env python3
"""What an iteration of the deflated batch (lam_hip_solve_many_deflated) costs against an iteration of the plain batch
(lam_hip_solve_many) of the same build and K, and what deflation buys end to end.

Per shape (default fp64 N = 65536 and fp32 N = 131072), per option "symmetric_many" = 0 and 2, per K = 1, 4, 8 and per m = 4, 16, 32
(a random W: the cost does not depend on its values): seconds per iteration with rel_error = 0, taken as
(t_total(I) - t_total(2)) / (I - 2) so that the launches in front of the loop -- one more product and four vector launches for the
deflated start -- cancel.  Profiler off, warmed up, every window at least `--window-s` seconds of iterations, plain and deflated
ALTERNATED within one process, `--windows` windows each; min / median / spread ((max - min) / min) and
ratio = t_deflated(min) / t_plain(min).  The two launches an iteration adds read A W and r (m N + K N elements), then W and p, and
write p (m N + 2 K N): the expectation printed beside each ratio is 1 + (2 m + 3 K) / N.

End to end (`--e2e-n`, default 65536, fp64): one lam_hip_generate_spectrum_spd system with a cluster of 16 eigenvalues in
[1e-4, 1e-3] below a bulk on [1, 2], 8 random right-hand sides, rel_error 1e-8: iterations and seconds of the plain and of the deflated
solve, the seconds of the lam_hip_eigs run (16 smallest pairs) and of lam_hip_set_deflation_eigs, and after how many batches of 8
right-hand sides the setup has paid for itself.  Every shape runs in a child process of its own.
usage: deflation_probe.py [--out FILE] [--windows 5] [--window-s 0.5] [--shapes f64:65536,f32:131072] [--e2e-n 65536]"""
import argparse
import importlib
import json
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "2024-eumaster4hpc-student-challenge_amd"
SHAPES = "f64:65536,f32:131072"
MS = (4, 16, 32)
KS = (1, 4, 8)
SYM = (0, 2)
SHORT = 2


def loop(lam, dtype, n, windows, window_s):
    """{sym: {K: {"plain": [...], "m<m>": [...]}}}: seconds per iteration of each window"""
    import numpy as np
    out = {}
    with lam.Solver(lam.F64 if dtype == "f64" else lam.F32) as s:
        s.generate_random_spd(n, 5, 1e4)
        rng = np.random.default_rng(7)
        B = rng.uniform(-1, 1, (max(KS), n)).astype(s.vec_dtype)
        W = rng.uniform(-1, 1, (max(MS), n)).astype(s.vec_dtype)

        def per_iteration(solve, iters):
            solve(SHORT)
            t_short = s.stats["t_total"]
            solve(iters)
            return (s.stats["t_total"] - t_short) / (iters - SHORT)

        def plain(iters):
            return per_iteration(lambda i: s.solve_many(i, 0.0), iters)

        def deflated(m, iters):
            s.set_deflation(W[:m])
            return per_iteration(lambda i: s.solve_deflated(i, 0.0), iters)

        for sym in SYM:
            s.set_option("symmetric_many", sym)
            out[str(sym)] = {}
            for K in KS:
                s.set_rhs_many(B[:K])
                iters = max(10, int(math.ceil(window_s / max(plain(20), 1e-7))))
                modes = [("plain", lambda: plain(iters))] + [(f"m{m}", lambda m=m: deflated(m, iters)) for m in MS]
                for _, run in modes:                  # every kernel and every allocation before the first window
                    run()
                t = {name: [] for name, _ in modes}
                for _ in range(windows):
                    for name, run in modes:
                        t[name].append(run())
                out[str(sym)][str(K)] = t
    return out


def end_to_end(lam, n):
    import numpy as np
    nsmall, nrhs, tol = 16, 8, 1e-8
    rng = np.random.default_rng(11)
    eig = np.concatenate([np.geomspace(1e-4, 1e-3, nsmall), np.linspace(1.0, 2.0, n - nsmall)])
    out = {"n": n, "nsmall": nsmall, "nrhs": nrhs, "tol": tol}
    with lam.Solver(lam.F64) as s:
        s.generate_spectrum_spd(eig, rng.uniform(-1, 1, (3, n)))
        B = rng.uniform(-1, 1, (nrhs, n))
        s.set_rhs_many(B)
        s.solve_many(20, 0.0)                         # warm-up
        s.solve_many(20000, tol)
        out["plain"] = dict(iters=[int(i) for i in s.num_iters_many], seconds=s.stats["t_total"], true=float(s.true_residuals().max()))
        res = s.eigs(nsmall, "smallest", tol=1e-8)
        out["eigs"] = dict(steps=int(res["steps"]), converged=bool(res["converged"].all()), seconds=s.stats["t_total"])
        t0 = time.perf_counter()
        s.set_deflation_from_eigs(nsmall)
        out["set_deflation"] = dict(seconds=time.perf_counter() - t0)
        s.solve_deflated(20000, tol)
        out["deflated"] = dict(iters=[int(i) for i in s.num_iters_many], seconds=s.stats["t_total"], true=float(s.true_residuals().max()))
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

    emit(f"deflation_probe: windows >= {a.window_s} s, {a.windows} windows per figure, alternated; ms per iteration: min median spread")
    for shape in [x for x in a.shapes.split(",") if x]:
        dtype, n = shape.split(":")
        n = int(n)
        r = run_child(dtype, n, a.windows, a.window_s)
        for sym in SYM:
            emit()
            emit(f"== {dtype} N = {n}, symmetric_many = {sym}")
            emit(f"{'':>16}  {'min':>9} {'median':>9} {'spread':>7} {'ratio':>8} {'added ms':>9} {'1 + (2m + 3K) / N':>18}")
            for K in KS:
                t = r[str(sym)][str(K)]
                base = min(t["plain"])
                emit(f"{f'K = {K} plain':>16}  {fig(t['plain'])} {1.0:8.4f}")
                for m in MS:
                    v = t[f"m{m}"]
                    emit(f"{f'K = {K} m = {m}':>16}  {fig(v)} {min(v) / base:8.4f} {(min(v) - base) * 1e3:9.4f} {1 + (2 * m + 3 * K) / n:18.4f}")
    if a.e2e_n > 0:
        e = run_child("e2e", a.e2e_n)
        p, d = e["plain"], e["deflated"]
        setup = e["eigs"]["seconds"] + e["set_deflation"]["seconds"]
        saved = p["seconds"] - d["seconds"]
        emit()
        emit(f"== end to end: fp64 N = {e['n']}, {e['nsmall']} eigenvalues in [1e-4, 1e-3] below a bulk on [1, 2], {e['nrhs']} right-hand sides, "
             f"rel_error {e['tol']:g}")
        emit(f"plain     iterations {p['iters']}  {p['seconds']:.3f} s  worst true residual {p['true']:.2e}")
        emit(f"deflated  iterations {d['iters']}  {d['seconds']:.3f} s  worst true residual {d['true']:.2e}")
        emit(f"setup     lam_hip_eigs {e['eigs']['steps']} steps (all converged: {e['eigs']['converged']}) {e['eigs']['seconds']:.3f} s, "
             f"lam_hip_set_deflation_eigs {e['set_deflation']['seconds']:.3f} s")
        emit(f"a batch of {e['nrhs']} saves {saved:.3f} s; the setup of {setup:.3f} s has paid for itself after "
             f"{math.ceil(setup / saved) if saved > 0 else 'no number of'} batches")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
