#!/usr/bin/env python3
"""What the shifts of lam_hip_set_shifts_many cost per iteration, and what a regularisation path gains from one batch.

loop   ms per iteration of solve_many with rel_error = 0 (nothing stops), K = 1, 4, 8, plain and Jacobi, per shape (default fp64
       N = 65536 and fp32 N = 131072): profiler off, warmed up, every window at least 0.5 s, unshifted and shifted ALTERNATED within
       one process, `--windows` windows each; min / median / spread ((max - min) / min) and ratio = t_shifted(min) / t_unshifted(min).
       From the code the difference is R K fused multiply-adds per workgroup outside the stream (and, under Jacobi, K values of
       dinv per row instead of one): the claim is 1 to within the unshifted path's own spread.
       Every loop runs in a child process of its own.  The unshifted loop ALONE (nothing alternated with it) runs on this tree and,
       with --parent DIR (a checkout of the parent commit, library built), on that tree before and after: those runs are measured
       alike, compare this tree with its parent and give the parent's run-to-run spread.
path   generate_random_spd(n, 5, 1e6) (--path-n, default 8192), one right-hand side, eight shifts over four decades, tolerance
       1e-10, plain and Jacobi: iterations per shift; passes over the matrix of the one batch (its longest column) against eight
       single solves (their sum); and path-following -- the shifts taken four at a time from the largest down, each batch continued
       from the previous batch's solutions (set_shifts, then x0 = "continue") against the same batches from zero.
usage: shift_probe.py [--parent DIR] [--out FILE] [--windows 5] [--shapes f64:65536,f32:131072] [--path-n 8192]"""
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
LOOP_SHIFTS = (0.5, 0.0, 1e-3, 2.0, 0.25, 1e-2, 8.0, 1.0)      # a zero among them: it runs the shifted kernels all the same
PATH_SHIFTS = (1e-3, 3e-3, 1e-2, 3e-2, 1e-1, 3e-1, 1.0, 3.0)


def _load(tree):
    sys.path.insert(0, tree)
    return importlib.import_module(PKG)


def _iters_for(t_iter):
    return max(10, int(math.ceil(WINDOW_S / max(t_iter, 1e-7))))


def loop(lam, dtype, n, windows, shifted):
    """{(K, pc): (unshifted windows, shifted windows)}; shifted = False: the unshifted loop alone (a tree that has no shifts)."""
    import numpy as np
    out = {}
    with lam.Solver(lam.F64 if dtype == "f64" else lam.F32) as s:
        s.generate_random_spd(n, 5, 1e4)
        B = np.random.default_rng(7).uniform(-1, 1, (8, n)).astype(s.vec_dtype)
        for K in KS:
            s.set_rhs_many(B[:K])
            for pc in (lam.PC_NONE, lam.PC_JACOBI):
                modes = (None, LOOP_SHIFTS[:K]) if shifted else (None,)
                iters = {}
                for m in modes:
                    if shifted:
                        s.set_shifts(m)
                    s.solve_many(20, 0.0, pc)
                    iters[m] = _iters_for(s.stats["t_iter"])
                t = {m: [] for m in modes}
                for _ in range(windows):
                    for m in modes:
                        if shifted:
                            s.set_shifts(m)
                        s.solve_many(iters[m], 0.0, pc)
                        t[m].append(s.stats["t_iter"])
                out[f"{K},{pc}"] = [t[m] for m in modes]
    return out


def run_child(tree, dtype, n, windows, shifted):
    """One shape's loop in a process of its own: `tree`'s library; shifted = False is the unshifted loop alone."""
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tree, dtype, str(n), str(windows), str(int(shifted))],
                       capture_output=True, text=True, timeout=1500)
    if p.returncode != 0 or not p.stdout.strip():
        raise RuntimeError("loop child failed: " + p.stderr[-600:])
    return json.loads(p.stdout.strip().splitlines()[-1])


def path(lam, n, emit):
    import numpy as np
    tol, cap = 1e-10, 20000
    sh = np.array(PATH_SHIFTS)
    with lam.Solver(lam.F64) as s:
        s.generate_random_spd(n, 5, 1e6)
        b = np.random.default_rng(11).uniform(-1, 1, n)
        for pc, name in ((lam.PC_NONE, "plain"), (lam.PC_JACOBI, "jacobi")):
            s.solve_shifted(b, sh, cap, tol, pc)
            it, conv, res = s.num_iters_many.tolist(), bool(s.converged_many.all()), s.true_residuals()
            singles = []
            for v in sh:
                s.solve_shifted(b, [v], cap, tol, pc)
                singles.append(int(s.num_iters_many[0]))
            emit(f"{name}: shifts {sh.tolist()}")
            emit(f"  iterations per shift, one batch of 8: {it} (all converged: {conv}; true residuals {res.min():.2e} ... {res.max():.2e})")
            emit(f"  the same shifts alone at K = 1:       {singles}")
            emit(f"  passes over the matrix: batch {max(it)}, eight single solves {sum(singles)}: {sum(singles) / max(it):.2f} x fewer")
            # path-following: four shifts at a time from the largest down; each batch starts from the previous batch's solutions
            groups = [sh[4:][::-1], sh[:4][::-1]]
            cold, warm = [], []
            for g in groups:
                s.solve_shifted(b, g, cap, tol, pc)
                cold.append(s.num_iters_many.tolist())
            s.solve_shifted(b, groups[0], cap, tol, pc)
            warm.append(s.num_iters_many.tolist())
            s.set_shifts(groups[1])
            s.solve_many(cap, tol, pc, x0="continue")
            warm.append(s.num_iters_many.tolist())
            emit(f"  path-following, batches of 4 {[g.tolist() for g in groups]}: from zero {cold}, second batch continued from the "
                 f"first's solutions {warm}: passes {sum(max(c) for c in cold)} -> {sum(max(w) for w in warm)}")


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        tree, dtype, n, windows, shifted = sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]), sys.argv[6] == "1"
        print(json.dumps(loop(_load(tree), dtype, n, windows, shifted)))
        return
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit, library built")
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--path-n", type=int, default=8192)
    a = ap.parse_args()
    if a.windows < 3:
        ap.error("--windows must be at least 3")
    lines = []

    def emit(text=""):
        print(text, flush=True)
        lines.append(text)

    def fig(v):
        return f"{min(v) * 1e3:9.4f} {statistics.median(v) * 1e3:9.4f} {(max(v) - min(v)) / min(v) * 100:6.2f}%"

    emit(f"shift_probe: windows >= {WINDOW_S} s, {a.windows} per figure, unshifted and shifted alternated; ms per iteration: min median spread")
    for shape in a.shapes.split(","):
        dtype, n = shape.split(":")
        n = int(n)
        # every loop in a child process of its own: parent alone / this tree alone / this tree alternated / parent alone.  The three
        # "alone" runs are measured alike (unshifted loop, nothing in between) and are what compares this tree with its parent
        before = run_child(os.path.abspath(a.parent), dtype, n, a.windows, False) if a.parent else None
        alone = run_child(ROOT, dtype, n, a.windows, False)
        m = run_child(ROOT, dtype, n, a.windows, True)
        after = run_child(os.path.abspath(a.parent), dtype, n, a.windows, False) if a.parent else None
        emit()
        emit(f"== {dtype} N = {n}")
        emit(f"{'K':>2} {'pc':>6}  {'t_unshifted: min':>16} {'median':>9} {'spread':>7}   {'t_shifted: min':>14} {'median':>9} {'spread':>7}   {'ratio':>6}"
             + "   unshifted alone: this" + (" | parent before / after: min (their difference)" if a.parent else ""))
        for K in KS:
            for pc, name in ((0, "plain"), (1, "jacobi")):
                u, sft = m[f"{K},{pc}"]
                line = f"{K:>2} {name:>6}  {fig(u):>34}   {fig(sft):>32}   {min(sft) / min(u):6.4f}"
                line += f"   {min(alone[f'{K},{pc}'][0]) * 1e3:9.4f}"
                if a.parent:
                    pb, pa = min(before[f"{K},{pc}"][0]), min(after[f"{K},{pc}"][0])
                    line += f" | {pb * 1e3:9.4f} / {pa * 1e3:9.4f} ({abs(pa - pb) / min(pa, pb) * 100:.2f} %)"
                emit(line)
    emit()
    emit(f"== path: generate_random_spd({a.path_n}, 5, 1e6), fp64, tolerance 1e-10")
    path(_load(ROOT), a.path_n, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
