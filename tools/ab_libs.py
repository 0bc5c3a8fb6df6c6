#!/usr/bin/env python3
"""A/B of two builds of the library on ONE box: alternating child processes, each timing the GEMV alone (lam_hip_gemv_only) and a
short CG run.     usage: ab_libs.py libA.so libB.so [libC.so ...] [rounds]
AB_VECTOR_STEP=1: the child measures instead where the vector step weighs -- ms per iteration (5 windows >= 0.5 s, rel_error = 0) at fp64
N = 65536 and N = 10000 on one shard, fused and with fuse_update 0, and at N = 8192 on 2 shards of device 0 over the gather-Ap exchange."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = r'''
import importlib, json, os, sys
sys.path.insert(0, %r)
lam = importlib.import_module("2024-eumaster4hpc-student-challenge_amd")
out = {}
def ms_per_iteration(n, shards, fuse):
    import time
    with lam.Solver(lam.F64, device_ids=[0] * shards) as s:
        s.generate_random_spd(n, 5, 1e3)
        s.generate_random_rhs(6)
        s.set_option("fuse_update", fuse)
        s.cg_init()
        assert s.get_option("fuse_effective") == fuse and (shards == 1 or s.get_option("exchange_effective") == 1)
        s.cg_iterate(50, 0.0)
        t0 = time.perf_counter(); s.cg_iterate(100, 0.0); per = (time.perf_counter() - t0) / 100
        iters, win = max(100, int(0.5 / per) + 1), []
        for _ in range(5):
            t0 = time.perf_counter(); s.cg_iterate(iters, 0.0); win.append(round(1e3 * (time.perf_counter() - t0) / iters, 5))
        return dict(median=sorted(win)[2], min=min(win), max=max(win))
if os.environ.get("AB_VECTOR_STEP"):
    for n, shards, fuse in ((65536, 1, 1), (65536, 1, 0), (10000, 1, 1), (10000, 1, 0), (8192, 2, 1), (8192, 2, 0)):
        out[f"f64 N={n} shards={shards} fuse_update={fuse}"] = ms_per_iteration(n, shards, fuse)
    print(json.dumps(out))
    sys.exit(0)
for name, dt, n in [x for x in (("f64", lam.F64, 65536), ("f32", lam.F32, 131072), ("bf16", lam.BF16, 131072), ("f64_40000", lam.F64, 40000)) if not os.environ.get("AB_ONLY") or x[0] in os.environ["AB_ONLY"].split(",")]:
    with lam.Solver(dt) as s:
        s.generate_random_spd(n, 5, 1e3)
        s.generate_random_rhs(6)
        s.gemv_only(150)
        ms = [s.gemv_only(100) for _ in range(3)]
        s.set_option("gemv_timing", 1)
        s.solve(100, 1e-30)
        st = s.stats
        out[name] = dict(gemv_only_ms=round(1e3 * min(ms), 4), cg_gemv_ms=round(1e3 * st["t_gemv"], 4))
print(json.dumps(out))
''' % ROOT


def main():
    libs = [a for a in sys.argv[1:] if not a.isdigit()]
    rounds = int(sys.argv[-1]) if sys.argv[-1].isdigit() else 3
    for r in range(rounds):
        for lib in libs:
            env = dict(os.environ, LAM_HIP_LIB=os.path.abspath(lib), LAM_HIP_ALLOW_STALE="1")
            p = subprocess.run([sys.executable, "-c", CHILD], env=env, capture_output=True, text=True, timeout=600)
            line = p.stdout.strip().splitlines()[-1] if p.stdout.strip() else p.stderr[-400:]
            print(r, os.path.basename(lib), line, flush=True)


if __name__ == "__main__":
    main()
