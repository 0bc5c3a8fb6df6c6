"""The symmetric product's bits, pinned against a recorded build (tests/golden/symmetric_product_bits.json).

The second passes of the single product (option "symmetric") and of the batched one (option "symmetric_many") are two entry points of
one body (csrc/lam_kernels.h, symv_reduce_body), so tests/test_gpu_symmetric_many.py, which compares one product with the other, cannot
see a change in the order of that body's sums.  This file can: every case's result is compared, as SHA-256 of its bytes, with what the
build named in the golden file gave.  Inputs come from code the symmetric kernels do not touch: generate_random_spd (symmetric bit for bit, pinned
against its host model by tests/test_gpu_generators.py) and exact_data.int_vec.

Shapes: the smallest at which each path exists.  A strip is SS = 256 * VEC columns (512 fp64, 1024 fp32, 2048 bf16 storage).
  gemv    "symmetric" = 2 on one shard: n = 1001 (one ragged strip), 2 SS + VEC + 1 (interior tasks, the masked rim, a ragged strip),
          6150; F64 n = 32768 is the smallest n whose plan has 512-row tasks (the LDS row buffer is flushed twice per task);
  shards  2 and 3 row shards in one process: cyclic windows, the replicated store, the reducer workgroup; x after 3 iterations;
  many    "symmetric_many" = 2: gemv_many of 1, 2 and 4 columns;
  shift   X after 2 iterations of solve_many with shifts (0, 1, 2, 4): the second pass's SHIFT epilogue and its p.Ap partials.
Regenerate with tests/golden/make_symmetric_bits.py, and only from a build whose symmetric kernels are known to be unchanged."""
import hashlib
import json
import os

import numpy as np
import pytest

import exact_data as E
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

GOLDEN_FILE = os.path.join(GOLDEN, "symmetric_product_bits.json")
VEC = {"F64": 2, "F32": 4, "BF16": 8}
SEED, COND = 5, 100.0


def _three_strips(d):
    return 2 * 256 * VEC[d] + VEC[d] + 1


CASES = ([("gemv", d, n) for d in ("F64", "F32", "BF16") for n in (1001, _three_strips(d), 6150)]
         + [("gemv", "F64", 32768)]
         + [("shards", "F64", 1547, 2), ("shards", "F64", 1547, 3), ("shards", "BF16", 1547, 2)]
         + [("many", d, n, k) for d, n in (("F64", 1027), ("F32", 2053)) for k in (1, 2, 4)]
         + [("shift", "F64", 1027), ("shift", "F32", 2053)])


def case_id(case):
    return "-".join(str(c) for c in case)


def compute(lam, case):
    """The case's result as one contiguous array."""
    kind, d, n = case[:3]
    if kind == "shards":
        with lam.Solver(getattr(lam, d), device_ids=[0] * case[3]) as s:
            s.generate_random_spd(n, SEED, COND)
            s.set_rhs(E.int_vec(n, 700))
            s.set_option("symmetric", 2)
            s.solve(3, 1e-30)
            assert s.get_option("symmetric_effective") == 1 and s.get_option("exchange_effective") == 1
            return s.solution()
    with lam.Solver(getattr(lam, d)) as s:
        s.generate_random_spd(n, SEED, COND)
        dt = s.vec_dtype
        if kind == "gemv":
            s.set_option("symmetric", 2)
            y = s.gemv(E.int_vec(n, 700).astype(dt))
            assert s.get_option("symmetric_effective") == 1
            return y
        X = np.stack([E.int_vec(n, 700 + j) for j in range(4)]).astype(dt)
        s.set_option("symmetric_many", 2)
        if kind == "many":
            Y = s.gemv_many(X[:case[3]])
            assert s.get_option("symmetric_many_effective") == 1 and s.get_option("multi_rhs_k") == case[3]
            return Y
        s.set_rhs_many(X)
        s.set_shifts((0.0, 1.0, 2.0, 4.0))
        s.solve_many(2, 0.0)
        assert s.get_option("symmetric_many_effective") == 1 and s.get_option("multi_rhs_k") == 4
        return s.solutions()


def record(result):
    a = np.ascontiguousarray(result)
    return {"dtype": str(a.dtype), "shape": list(a.shape), "sha256": hashlib.sha256(a.tobytes()).hexdigest(),
            "first": [float(v).hex() for v in a.reshape(-1)[:4]]}


@pytest.fixture(scope="module")
def pinned():
    with open(GOLDEN_FILE) as f:
        return json.load(f)


def test_every_case_is_recorded(pinned):
    assert sorted(pinned["cases"]) == sorted(case_id(c) for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_bits_of_the_symmetric_product_are_those_of_the_recorded_build(lam, pinned, case):
    got, want = record(compute(lam, case)), pinned["cases"][case_id(case)]
    print(case_id(case), got)
    assert got == want, (
        f"{case_id(case)}: got {got}, recorded {want}.  tests/golden/symmetric_product_bits.json pins the summation order of the "
        f"symmetric kernels as built at commit {pinned['commit']} by {pinned['hipcc']!r}; regenerate it "
        "(tests/golden/make_symmetric_bits.py) only from a build whose symmetric kernels are known to be unchanged.")
