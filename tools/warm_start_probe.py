#!/usr/bin/env python3
"""What a batched solve from a guess costs (lam_hip_solve_many_x0), and that the loop it shares with lam_hip_solve_many did not move.

  loop      ms per iteration of solve_many (rel_error = 0, windows >= 0.5 s, minimum and spread (max - min) / min of --windows windows)
            at fp64 N = 65536, K = 1, 4, 8, on this tree and -- with --parent DIR, a checkout of the parent commit with its library
            built -- on that tree, alternated parent / this / parent, each in a child process of its own
  start     wall ms of the call with max_iters = 0: the plain init (solve_many) against the start from the batch's own solution
            (x0 = "continue": one product + the fused pass, no upload), minimum of 10 calls each; one iteration for comparison
  restart   the badly scaled S M S system of tests/pcg_reference.py (n = 512, fp64, plain CG, tolerance 1e-10, 4 n iterations in
            all): iterations, recursive and true residual of one run and of runs restarted every R iterations from x (fresh r)
  heat      the steady 2-D heat system (n = 4096) solved again for slightly changed boundary temperatures: iterations from zero
            and from the previous answer
usage: warm_start_probe.py [--parent DIR] [--out FILE] [--windows 5] [--n 65536]"""
import argparse
import importlib
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "2024-eumaster4hpc-student-challenge_amd"
WINDOW_S = 0.5
KS = (1, 4, 8)


def _load(tree):
    sys.path.insert(0, tree)
    return importlib.import_module(PKG)


def loop_child(tree, n, windows):
    import numpy as np
    lam = _load(tree)
    out = {}
    with lam.Solver(lam.F64) as s:
        s.generate_random_spd(n, 5, 1e6)
        B = np.random.default_rng(7).uniform(-1, 1, (8, n))
        for K in KS:
            s.set_rhs_many(B[:K])
            s.solve_many(20, 0.0)
            iters = max(10, int(math.ceil(WINDOW_S / s.stats["t_iter"])))
            ts = []
            for _ in range(windows):
                s.solve_many(iters, 0.0)
                ts.append(s.stats["t_iter"])
            out[K] = ts
    print(json.dumps(out))


def run_loop(tree, n, windows):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--loop-child", tree, str(n), str(windows)], capture_output=True, text=True,
                       timeout=900)
    if p.returncode != 0 or not p.stdout.strip():
        raise RuntimeError("loop child failed: " + p.stderr[-600:])
    return {int(k): v for k, v in json.loads(p.stdout.strip().splitlines()[-1]).items()}


def heat_system(nx, ny):
    """The dense system apps/heat_system.cpp assembles: 4 T - (interior neighbours) = (boundary neighbours), north 0, others 100."""
    import numpy as np
    mx, my = nx - 2, ny - 2
    A, b = np.zeros((mx * my, mx * my)), np.zeros(mx * my)
    for y in range(my):
        for x in range(mx):
            k = y * mx + x
            A[k, k] = 4.0
            for xx, yy in ((x, y + 1), (x, y - 1), (x - 1, y), (x + 1, y)):
                if 0 <= xx < mx and 0 <= yy < my:
                    A[k, yy * mx + xx] = -1.0
                elif yy != my:
                    b[k] += 100.0
    return A, b


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--loop-child":
        return loop_child(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit, library built")
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--n", type=int, default=65536)
    a = ap.parse_args()
    import numpy as np
    lines = []

    def emit(text=""):
        print(text, flush=True)
        lines.append(text)

    emit(f"warm_start_probe: fp64 N = {a.n}")
    emit("== loop: ms per iteration of solve_many, min (spread of the windows)")
    runs = ([("parent", a.parent)] if a.parent else []) + [("this", ROOT)] + ([("parent", a.parent)] if a.parent else [])
    for name, tree in runs:
        r = run_loop(os.path.abspath(tree), a.n, a.windows)
        emit(f"{name:>7}: " + "   ".join(f"K={K} {min(r[K]) * 1e3:8.4f} ({(max(r[K]) - min(r[K])) / min(r[K]) * 100:.2f} %)" for K in KS))

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    lam = _load(ROOT)
    emit("== start: wall ms of a call with max_iters = 0 (min of 10), and one iteration")
    with lam.Solver(lam.F64) as s:
        s.generate_random_spd(a.n, 5, 1e6)
        B = np.random.default_rng(7).uniform(-1, 1, (8, a.n))
        for K in KS:
            s.set_rhs_many(B[:K])
            s.solve_many(30, 0.0)
            t_iter = s.stats["t_iter"]
            cold, warm = [], []
            for _ in range(10):
                s.solve_many(0, 0.0)
                cold.append(s.stats["t_total"])
                s.solve_many(0, 0.0, x0="continue")
                warm.append(s.stats["t_total"])
            emit(f"K={K}: plain init {min(cold) * 1e3:8.4f}   from a guess {min(warm) * 1e3:8.4f}   difference {(min(warm) - min(cold)) * 1e3:8.4f}"
                 f"   one iteration {t_iter * 1e3:8.4f}")

    import pcg_reference as R
    emit("== restart: S M S, n = 512, fp64, plain CG, tolerance 1e-10, 4 n = 2048 iterations in all")
    n = 512
    A, rng = R.sms_system(n)
    Bs = rng.uniform(-1, 1, (2, n)) @ A.T
    with lam.Solver(lam.F64) as s:
        s.set_matrix(A)
        s.set_rhs_many(Bs)
        for every in (0, 64, 256, 512):
            left, total = 4 * n, np.zeros(2, int)
            s.solve_many(min(every or left, left), 1e-10)
            while True:
                ran = np.where(s.converged_many, s.num_iters_many, s.num_iters_many - 1)
                total += ran
                left -= int(ran.max())
                if s.converged_many.all() or left <= 0 or not every:
                    break
                s.solve_many(min(every, left), 1e-10, x0="continue")
            emit(f"restart every {every or 'never':>5}: iterations {total.tolist()}, converged {s.converged_many.tolist()}, recursive "
                 f"{[f'{v:.2e}' for v in s.rel_err_many]}, true {[f'{v:.2e}' for v in s.true_residuals()]}")
    emit("== heat: the steady 2-D heat system of apps/heat_system.cpp (66 x 66 grid, n = 4096, fp64, plain CG, tolerance 1e-9), solved, "
         "then solved again for boundary temperatures changed by 1 %, 0.1 % and 0.01 %: from zero and from the previous answer")
    A, b = heat_system(66, 66)
    with lam.Solver(lam.F64) as s:
        s.set_matrix(A)
        s.set_rhs_many(b[None, :])
        s.solve_many(4 * A.shape[0], 1e-9)
        x_prev, first = s.solutions(), int(s.num_iters_many[0])
        emit(f"first solve from zero: {first} iterations, true residual {s.true_residuals()[0]:.2e}")
        for change in (1e-2, 1e-3, 1e-4):
            s.set_rhs_many((b * (1.0 + change))[None, :] + change * np.random.default_rng(3).uniform(-1, 1, b.size) * (b != 0))
            row = []
            for x0 in (None, x_prev):
                s.solve_many(4 * A.shape[0], 1e-9, x0=x0)
                row.append(f"{int(s.num_iters_many[0])} iterations (true residual {s.true_residuals()[0]:.2e})")
            emit(f"boundary changed by {change:g}: from zero {row[0]}, from the previous answer {row[1]}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
