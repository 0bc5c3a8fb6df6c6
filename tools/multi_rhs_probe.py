#!/usr/bin/env python3
"""What several right-hand sides per pass over the matrix cost (lam_hip_solve_many), next to the single solve.

Per shape (fp64 N = 65536, 32768, 10000; fp32 N = 131072), profiler off, every kernel shape warmed up first, every timed window at
least 0.5 s, single and batched alternated within one process, minimum and median of `--windows` (>= 5) windows:
  t_single          seconds per iteration of cg_iterate on THIS build; the same on the PARENT build's library (--parent LIB, loaded
                    in child processes of their own through plain ctypes: it has no batched entry points), twice, before and
                    after -- the spread of those two is the noise floor
  t_batch(K)        seconds per iteration of solve_many with rel_error = 0, K = 1, 2, 4, 8
  product(K)        gemv_many_only; share = esz (N^2 + 2 K N) / product time / 8 TB/s
  r(K)              t_batch(K) / t_single(parent) (this build's t_single without --parent); K / t_batch(K) = solved-system
                    iterations per second
usage: multi_rhs_probe.py [--parent liblam_hip_parent.so] [--out FILE] [--windows 5] [--shapes f64:65536,f32:131072]"""
import argparse
import ctypes as C
import importlib
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK = 8.0e12
WINDOW_S = 0.5
SHAPES = "f64:65536,f64:32768,f64:10000,f32:131072"


def _iters_for(t_iter):
    return max(10, int(math.ceil(WINDOW_S / max(t_iter, 1e-7))))


def parent_child(lib, dtype, n, windows):
    """t_single on another build of the library, through the C ABI alone (entry points both builds have)."""
    class Stats(C.Structure):
        _fields_ = [("num_iters", C.c_int32), ("converged", C.c_int32), ("rel_err", C.c_double), ("t_gemv", C.c_double),
                    ("t_iter", C.c_double), ("t_total", C.c_double), ("t_comm_init", C.c_double), ("gemv_bytes", C.c_double),
                    ("t_exchange", C.c_double)]
    L = C.CDLL(lib)
    L.lam_hip_generate_random_spd.argtypes = [C.c_void_p, C.c_uint64, C.c_double]
    L.lam_hip_generate_random_rhs.argtypes = [C.c_void_p, C.c_uint64]
    L.lam_hip_set_problem.argtypes = [C.c_void_p, C.c_uint64]
    L.lam_hip_cg_iterate.argtypes = [C.c_void_p, C.c_int, C.c_double, C.POINTER(Stats)]
    L.lam_hip_cg_init.argtypes = [C.c_void_p]
    L.lam_hip_destroy.argtypes = [C.c_void_p]
    L.lam_hip_destroy.restype = None
    h = C.c_void_p()

    def chk(rc):
        if rc != 0:
            raise RuntimeError(f"parent library call failed: {rc}")
    chk(L.lam_hip_create(C.byref(h), 0 if dtype == "f64" else 1, 1, None))
    chk(L.lam_hip_set_problem(h, n))
    chk(L.lam_hip_generate_random_spd(h, 5, 1e6))
    chk(L.lam_hip_generate_random_rhs(h, 6))
    st = Stats()
    chk(L.lam_hip_cg_init(h))
    chk(L.lam_hip_cg_iterate(h, 20, 0.0, C.byref(st)))
    iters = _iters_for(st.t_iter)
    ts = []
    for _ in range(windows):
        chk(L.lam_hip_cg_init(h))
        chk(L.lam_hip_cg_iterate(h, iters, 0.0, C.byref(st)))
        ts.append(st.t_iter)
    L.lam_hip_destroy(h)
    print(json.dumps(ts))


def run_parent(lib, dtype, n, windows):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--parent-child", lib, dtype, str(n), str(windows)],
                       capture_output=True, text=True, timeout=900)
    if p.returncode != 0 or not p.stdout.strip():
        raise RuntimeError("parent run failed: " + p.stderr[-600:])
    return json.loads(p.stdout.strip().splitlines()[-1])


def measure(lam, dtype, n, windows):
    import numpy as np
    esz = 8 if dtype == "f64" else 4
    KS = (1, 2, 4, 8)
    with lam.Solver(lam.F64 if dtype == "f64" else lam.F32) as s:
        s.generate_random_spd(n, 5, 1e6)
        s.generate_random_rhs(6)
        B = np.random.default_rng(7).uniform(-1, 1, (8, n)).astype(s.vec_dtype)
        # warm-up of every shape, and the window lengths
        s.cg_init()
        it_single = _iters_for(s.cg_iterate(20, 0.0)["t_iter"])
        it_batch, reps_prod = {}, {}
        for K in KS:
            s.set_rhs_many(B[:K])
            s.solve_many(20, 0.0)
            it_batch[K] = _iters_for(s.stats["t_iter"])
            reps_prod[K] = _iters_for(s.gemv_many_only(K, 10))
        reps_single = _iters_for(s.gemv_only(10))
        single, prod_single = [], []
        batch, prod = {K: [] for K in KS}, {K: [] for K in KS}
        for _ in range(windows):
            s.cg_init()
            single.append(s.cg_iterate(it_single, 0.0)["t_iter"])
            prod_single.append(s.gemv_only(reps_single))
            for K in KS:
                s.set_rhs_many(B[:K])
                s.solve_many(it_batch[K], 0.0)
                assert s.get_option("multi_rhs_k") == K
                batch[K].append(s.stats["t_iter"])
                prod[K].append(s.gemv_many_only(K, reps_prod[K]))
        name = s.gemv_kernel_name()
    return dict(esz=esz, single=single, prod_single=prod_single, batch=batch, prod=prod, kernel=name)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--parent-child":
        return parent_child(sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]))
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="the parent commit's liblam_hip.so (the comparison base)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--shapes", default=SHAPES)
    a = ap.parse_args()
    if a.windows < 5:
        ap.error("--windows must be at least 5")
    sys.path.insert(0, ROOT)
    lam = importlib.import_module("2024-eumaster4hpc-student-challenge_amd")
    lines = []

    def emit(text=""):
        print(text, flush=True)
        lines.append(text)

    mm = lambda v: (min(v), statistics.median(v))
    emit(f"multi_rhs_probe: windows >= {WINDOW_S} s, {a.windows} per figure, min / median; ms per iteration (or per product)")
    for shape in a.shapes.split(","):
        dtype, n = shape.split(":")
        n = int(n)
        par = None
        if a.parent:
            par = [run_parent(os.path.abspath(a.parent), dtype, n, a.windows)]
        m = measure(lam, dtype, n, a.windows)
        if a.parent:
            par.append(run_parent(os.path.abspath(a.parent), dtype, n, a.windows))
        esz = m["esz"]
        emit()
        emit(f"== {dtype} N = {n}   single kernel: {m['kernel']}")
        ts_min, ts_med = mm(m["single"])
        emit(f"t_single  this build      {ts_min * 1e3:9.4f} / {ts_med * 1e3:9.4f}")
        base = ts_min
        if par:
            mins = [min(p) for p in par]
            for i, p in enumerate(par):
                emit(f"t_single  parent run {i + 1}    {min(p) * 1e3:9.4f} / {statistics.median(p) * 1e3:9.4f}")
            base = min(mins)
            emit(f"noise floor (spread of the parent runs' minima) {abs(mins[0] - mins[1]) / base * 100:.2f} %;  this build / parent "
                 f"{ts_min / base:.4f}")
        pm, pmed = mm(m["prod_single"])
        emit(f"product   single          {pm * 1e3:9.4f} / {pmed * 1e3:9.4f}   {esz * (n * n + 2 * n) / pm / PEAK:.3f} of 8 TB/s")
        emit(f"{'K':>2} {'t_batch min':>12} {'median':>9} {'product min':>12} {'median':>9} {'share':>6} {'r(K)':>6} {'K*t_single':>11} "
             f"{'sys-it/s':>9} {'x single':>8}")
        for K in (1, 2, 4, 8):
            b_min, b_med = mm(m["batch"][K])
            p_min, p_med = mm(m["prod"][K])
            share = esz * (n * n + 2 * K * n) / p_min / PEAK
            emit(f"{K:>2} {b_min * 1e3:12.4f} {b_med * 1e3:9.4f} {p_min * 1e3:12.4f} {p_med * 1e3:9.4f} {share:6.3f} {b_min / base:6.3f} "
                 f"{K * base * 1e3:11.4f} {K / b_min:9.1f} {K / b_min * base:8.2f}")
            if K > 1:
                emit(f"   t_batch({K}) < {K} t_single(parent): {'yes' if b_min < K * base else 'NO'}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
