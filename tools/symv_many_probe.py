#!/usr/bin/env python3
"""What option "symmetric_many" buys: the batched iteration on the symmetric two-pass product against the general batched product of
the same build, and the untouched paths against the parent commit's library (the method of tools/multi_rhs_probe.py).

Per shape (fp64 N = 65536, fp32 N = 131072), profiler off, every kernel shape warmed up first, every timed window at least 0.5 s,
general and symmetric alternated within one process, minimum and median of `--windows` (>= 5) windows:
  t_batch(K), K = 1, 2, 4   seconds per iteration of solve_many with rel_error = 0 under symmetric_many = 0 and = 2
  product(K)                gemv_many_only under both; share = bytes of the product's model / time / 8 TB/s
  t_single sym              cg_iterate under "symmetric" = 2: the anchor of K = 1
  multi-shift, 64 shifts    solve_multishift (its seed is the K = 1 batch) under both
  MINRES, K = 4             solve_minres under both
  parent                    t_single (general GEMV) and t_batch(K) at option 0 on the PARENT build's library (--parent LIB), in child
                            processes of their own through plain ctypes, before and after: the spread of the two runs is the noise floor
A (dtype, K) is ADMITTED to symmetric_many = 1 when its symmetric t_batch is faster than the general one by more than the spread
between the windows of the two figures (median - minimum, the larger of the two).
usage: symv_many_probe.py [--parent liblam_hip_parent.so] [--out FILE] [--windows 5] [--shapes f64:65536,f32:131072]"""
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
SHAPES = "f64:65536,f32:131072"
KS = (1, 2, 4)
NSHIFTS = 64


def _iters_for(t_iter):
    return max(10, int(math.ceil(WINDOW_S / max(t_iter, 1e-7))))


def parent_child(lib, dtype, n, windows):
    """The untouched paths on another build of the library, through the C ABI alone: t_single and t_batch(K) at the defaults."""
    class Stats(C.Structure):
        _fields_ = [("num_iters", C.c_int32), ("converged", C.c_int32), ("rel_err", C.c_double), ("t_gemv", C.c_double),
                    ("t_iter", C.c_double), ("t_total", C.c_double), ("t_comm_init", C.c_double), ("gemv_bytes", C.c_double),
                    ("t_exchange", C.c_double)]
    import numpy as np
    L = C.CDLL(lib)
    L.lam_hip_generate_random_spd.argtypes = [C.c_void_p, C.c_uint64, C.c_double]
    L.lam_hip_generate_random_rhs.argtypes = [C.c_void_p, C.c_uint64]
    L.lam_hip_set_problem.argtypes = [C.c_void_p, C.c_uint64]
    L.lam_hip_cg_iterate.argtypes = [C.c_void_p, C.c_int, C.c_double, C.POINTER(Stats)]
    L.lam_hip_cg_init.argtypes = [C.c_void_p]
    L.lam_hip_set_rhs_many.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.lam_hip_solve_many.argtypes = [C.c_void_p, C.c_int, C.c_double, C.POINTER(Stats), C.c_void_p, C.c_void_p, C.c_void_p]
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
    B = np.random.default_rng(7).uniform(-1, 1, (4, n)).astype(np.float64 if dtype == "f64" else np.float32)
    st = Stats()
    chk(L.lam_hip_cg_init(h))
    chk(L.lam_hip_cg_iterate(h, 20, 0.0, C.byref(st)))
    it_single = _iters_for(st.t_iter)
    it_batch = {}
    for K in KS:
        chk(L.lam_hip_set_rhs_many(h, K, B.ctypes.data_as(C.c_void_p)))
        chk(L.lam_hip_solve_many(h, 20, 0.0, C.byref(st), None, None, None))
        it_batch[K] = _iters_for(st.t_iter)
    out = {"single": [], **{str(K): [] for K in KS}}
    for _ in range(windows):
        chk(L.lam_hip_cg_init(h))
        chk(L.lam_hip_cg_iterate(h, it_single, 0.0, C.byref(st)))
        out["single"].append(st.t_iter)
        for K in KS:
            chk(L.lam_hip_set_rhs_many(h, K, B.ctypes.data_as(C.c_void_p)))
            chk(L.lam_hip_solve_many(h, it_batch[K], 0.0, C.byref(st), None, None, None))
            out[str(K)].append(st.t_iter)
    L.lam_hip_destroy(h)
    print(json.dumps(out))


def run_parent(lib, dtype, n, windows):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--parent-child", lib, dtype, str(n), str(windows)],
                       capture_output=True, text=True, timeout=900)
    if p.returncode != 0 or not p.stdout.strip():
        raise RuntimeError("parent run failed: " + p.stderr[-600:])
    return json.loads(p.stdout.strip().splitlines()[-1])


def measure(lam, dtype, n, windows, extras):
    import numpy as np
    with lam.Solver(lam.F64 if dtype == "f64" else lam.F32) as s:
        s.generate_random_spd(n, 5, 1e6)
        s.generate_random_rhs(6)
        B = np.random.default_rng(7).uniform(-1, 1, (4, n)).astype(s.vec_dtype)
        shifts = np.linspace(0.0, 63.0, NSHIFTS)

        def batch(K, iters):
            s.set_rhs_many(B[:K])
            s.solve_many(iters, 0.0)
            return s.stats

        def mshift(iters):
            s.solve_multishift(B[0], shifts, iters, 0.0)
            return s.stats

        def minres(iters):
            s.set_rhs_many(B)
            s.solve_minres(iters, 0.0)
            return s.stats

        def single(iters, sym):
            s.set_option("symmetric", sym)
            s.cg_init()
            t = s.cg_iterate(iters, 0.0)["t_iter"]
            s.set_option("symmetric", 0)
            return t

        # warm-up of every shape under both values, and the window lengths
        it = {}
        for opt in (0, 2):
            s.set_option("symmetric_many", opt)
            for K in KS:
                it["batch", K, opt] = _iters_for(batch(K, 20)["t_iter"])
                assert s.get_option("symmetric_many_effective") == (1 if opt else 0)
                it["prod", K, opt] = _iters_for(s.gemv_many_only(K, 10))
            if extras:
                it["mshift", opt] = _iters_for(mshift(20)["t_iter"])
                it["minres", opt] = _iters_for(minres(20)["t_iter"])
        it["single", 0], it["single", 2] = _iters_for(single(20, 0)), _iters_for(single(20, 2))
        res = {k: [] for k in it}
        bytes_model = {}
        for _ in range(windows):
            for sym in (0, 2):
                res["single", sym].append(single(it["single", sym], sym))
            for K in KS:
                for opt in (0, 2):
                    s.set_option("symmetric_many", opt)
                    st = batch(K, it["batch", K, opt])
                    assert s.get_option("multi_rhs_k") == K and s.get_option("symmetric_many_effective") == (1 if opt else 0)
                    res["batch", K, opt].append(st["t_iter"])
                    bytes_model[K, opt] = st["gemv_bytes"]
                    res["prod", K, opt].append(s.gemv_many_only(K, it["prod", K, opt]))
            if extras:
                for opt in (0, 2):
                    s.set_option("symmetric_many", opt)
                    res["mshift", opt].append(mshift(it["mshift", opt])["t_iter"])
                    res["minres", opt].append(minres(it["minres", opt])["t_iter"])
        s.set_option("symmetric_many", 0)
    return res, bytes_model


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--parent-child":
        return parent_child(sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]))
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="the parent commit's liblam_hip.so (the comparison base of the untouched paths)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--no-extras", action="store_true", help="skip the multi-shift and MINRES cases")
    a = ap.parse_args()
    if a.windows < 5:
        ap.error("--windows must be at least 5")
    sys.path.insert(0, ROOT)
    lam = importlib.import_module("2024-eumaster4hpc-student-challenge_amd")
    lines = []

    def emit(text=""):
        print(text, flush=True)
        lines.append(text)

    def flush_out():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    mm = lambda v: (min(v), statistics.median(v))      # noqa: E731
    emit(f"symv_many_probe: windows >= {WINDOW_S} s, {a.windows} per figure, min / median; ms per iteration (or per product)")
    for shape in a.shapes.split(","):
        dtype, n = shape.split(":")
        n = int(n)
        par = []
        if a.parent:
            par.append(run_parent(os.path.abspath(a.parent), dtype, n, a.windows))
        res, bytes_model = measure(lam, dtype, n, a.windows, not a.no_extras)
        if a.parent:
            par.append(run_parent(os.path.abspath(a.parent), dtype, n, a.windows))
        emit()
        emit(f"== {dtype} N = {n}")
        g0, g0m = mm(res["single", 0])
        s2, s2m = mm(res["single", 2])
        emit(f"t_single  general GEMV, this build       {g0 * 1e3:9.4f} / {g0m * 1e3:9.4f}")
        emit(f"t_single  symmetric = 2 (anchor of K = 1) {s2 * 1e3:9.4f} / {s2m * 1e3:9.4f}")
        emit(f"{'K':>2} {'general min':>12} {'median':>9} {'symmetric min':>14} {'median':>9} {'sym/gen':>8} {'spread':>8} {'admitted':>9}   "
             f"{'product gen':>12} {'product sym':>12} {'share gen':>9} {'share sym':>9}")
        for K in KS:
            a0, a0m = mm(res["batch", K, 0])
            a2, a2m = mm(res["batch", K, 2])
            p0, _ = mm(res["prod", K, 0])
            p2, _ = mm(res["prod", K, 2])
            spread = max(a0m - a0, a2m - a2)
            emit(f"{K:>2} {a0 * 1e3:12.4f} {a0m * 1e3:9.4f} {a2 * 1e3:14.4f} {a2m * 1e3:9.4f} {a2 / a0:8.4f} {spread * 1e3:8.4f} "
                 f"{'yes' if a0 - a2 > spread else 'NO':>9}   {p0 * 1e3:12.4f} {p2 * 1e3:12.4f} {bytes_model[K, 0] / p0 / PEAK:9.3f} "
                 f"{bytes_model[K, 2] / p2 / PEAK:9.3f}")
        if not a.no_extras:
            for key, label in (("mshift", f"multi-shift, {NSHIFTS} shifts"), ("minres", "MINRES, K = 4")):
                a0, a0m = mm(res[key, 0])
                a2, a2m = mm(res[key, 2])
                emit(f"{label:24s} general {a0 * 1e3:9.4f} / {a0m * 1e3:9.4f}   symmetric {a2 * 1e3:9.4f} / {a2m * 1e3:9.4f}   sym/gen {a2 / a0:.4f}")
        if par:
            emit("untouched paths against the parent's library (two parent runs: before / after; this build in between)")
            for key, label, mine in [("single", "t_single general", res["single", 0])] + [(str(K), f"t_batch({K}) option 0", res["batch", K, 0]) for K in KS]:
                mins = [min(p[key]) for p in par]
                base = min(mins)
                emit(f"  {label:22s} parent {mins[0] * 1e3:9.4f} / {mins[1] * 1e3:9.4f}  (spread {abs(mins[0] - mins[1]) / base * 100:.2f} %)   "
                     f"this build {min(mine) * 1e3:9.4f}   this / parent {min(mine) / base:.4f}")
        flush_out()
    flush_out()


if __name__ == "__main__":
    main()
