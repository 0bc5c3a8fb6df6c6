#!/usr/bin/env python3
"""Parity cases of the experiments that live in the TUNING build of the library only (liblam_hip_tuning.so, `make tuning`):
the MFMA-fed bf16 GEMV and separate reduction launches (finalize = 0).  The product library refuses these options (tests/test_gpu_parity.py::
test_tuning_build_variants); the GPU tests run this script as a child process with LAM_HIP_LIB pointing at the tuning
build, one case per call:   tuning_cases.py <case> [args ...]   -> exit code 0 and a last line "ok <case>"."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
lam = importlib.import_module("2024-eumaster4hpc-student-challenge_amd")


def mfma(variant, n):
    """Asymmetric random data, so a wrong fragment/diagonal map cannot cancel.  Variant 21 feeds p as three exact bf16 terms
    (fp32-faithful); variant 20 rounds p to bf16 (8 significant bits)."""
    tol = 2.0 ** -8 if variant == 20 else 32 * 2.0 ** -24
    A = np.random.default_rng(n + 3).uniform(-1, 1, (n, n)).astype(np.float32)
    x = np.random.default_rng(n + 4).uniform(-1, 1, n).astype(np.float32)
    with lam.Solver(lam.BF16) as s:
        s.set_matrix(A)
        A_dev = s.download_rows(0, n).astype(np.float64)
        y_valu = s.gemv(x)
        s.set_option("gemv_variant", variant)
        assert "mfma" in s.gemv_kernel_name()
        y = s.gemv(x)
    y64 = A_dev @ x.astype(np.float64)
    scale = np.abs(A_dev) @ np.abs(x.astype(np.float64))
    assert np.max(np.abs(y.astype(np.float64) - y64) / scale) <= tol
    assert np.max(np.abs(y_valu.astype(np.float64) - y64) / scale) <= 32 * 2.0 ** -24


def launch_chain(dtype_name, n, shards):
    """Fused update / two kernels with the reducer workgroup / the round-1 chain with separate reduction launches
    (finalize = 0): the same arithmetic, identical bits -- on both event-ordered exchanges of a multi-shard context."""
    dt = getattr(lam, dtype_name)
    for exchange in ((0, 1) if shards > 1 else (0,)):
        res = []
        for fuse, fin in ((1, 1), (0, 1), (0, 0)):
            with lam.Solver(dt, n_shards=shards, device_ids=[0] * shards) as s:
                s.generate_random_spd(n, 5, 300.0)
                s.generate_random_rhs(6)
                if shards > 1:
                    s.set_option("exchange", exchange)
                s.set_option("fuse_update", fuse)
                s.set_option("finalize", fin)
                s.solve(400, 1e-9 if dtype_name == "F64" else 1e-5)
                res.append((s.stats["num_iters"], s.stats["rel_err"], s.solution().tobytes(), s.true_residual()))
                s.cg_init()
                for _ in range(3):
                    s.cg_iterate(7, 0.0)
                res[-1] += (s.solution().tobytes(),)
        assert res[0] == res[1] == res[2], exchange


def refusals():
    """The experiments that were removed are unknown to the tuning build too, and the MFMA shapes exist for bf16 storage only."""
    import refused_options as R
    with lam.Solver(lam.F64) as s, lam.Solver(lam.BF16) as sb:
        R.check_removed(lam, s)
        R.check_removed(lam, sb)
        for v in R.MFMA_VARIANTS:
            assert R.refused(lam, s.set_option, "gemv_variant", v), v
            sb.set_option("gemv_variant", v)
        for v in R.KEPT_VARIANTS:
            s.set_option("gemv_variant", v)
            sb.set_option("gemv_variant", v)
        s.set_option("finalize", 0)
        s.set_option("finalize", 1)


def call_counts():
    """The runtime calls of cg_init + 11 iterations on the gather-Ap exchange with finalize = 0 (three shards, one rank through RCCL):
    one JSON line, compared with the literals of tests/test_gpu_iteration_call_counts.py by the test that started this process."""
    import json
    import test_gpu_iteration_call_counts as T
    print(json.dumps({f"{case}/timing{timing}": T.measure(lam, n, shards, options, timing)
                      for case, (n, shards, options) in T.TUNING_CASES.items() for timing in (1, 8)}))


CASES = {"mfma": (mfma, (int, int)), "launch_chain": (launch_chain, (str, int, int)), "refusals": (refusals, ()), "call_counts": (call_counts, ())}


def main():
    with lam.Solver(lam.F64) as s:
        assert s.get_option("tuning_variants") == 1, "not the tuning build: set LAM_HIP_LIB to liblam_hip_tuning.so"
    name = sys.argv[1]
    fn, types = CASES[name]
    fn(*(t(a) for t, a in zip(types, sys.argv[2:])))
    print("ok", name)


if __name__ == "__main__":
    main()
