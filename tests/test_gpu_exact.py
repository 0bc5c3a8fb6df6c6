"""Exact known answers for the dense GEMV and the first CG step, on dense integer data (tests/exact_data.py says why every sum is
exact), plus the propagation of non-finite matrix entries and dense random data at multi-tile sizes.

Integer data pins what tolerances cannot: a dropped, doubled or shifted column tile, a wrong rotated tile start, a lost or doubled
workgroup partial of p.Ap among thousands, a wrong segment of a panel launch -- each changes an exact integer, so the GEMV is
compared bit for bit and the first CG step's x too.  Dense random data (section 5) catches what integers cannot: a sum carried in
too low a precision."""
import contextlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import exact_data as E
from conftest import MOCK_DIR, slow

pytestmark = pytest.mark.gpu

DTYPES = ("F64", "F32", "BF16")
VEC = {"F64": 2, "F32": 4, "BF16": 8}               # matrix elements per 16-byte vector
U_TV = {"F64": 2.0 ** -53, "F32": 2.0 ** -24, "BF16": 2.0 ** -24}
GATE = {"F64": 1e-13, "F32": 32 * 2.0 ** -24, "BF16": 32 * 2.0 ** -24}     # the suite's GEMV gates, relative to |A| |x|
BASE = {"gemv_variant": -1, "force_generic": 0, "nt_loads": 1, "symmetric": 0}
# every product path of the library: the dtype's default shape, the four product shapes (tile R4; cooperative rows R2 / 4 waves,
# R2 / 8 waves, R4 / 8 waves), the any-alignment kernel, plain loads, the symmetric product (one shard; several shards keep the
# general GEMV for lam_hip_gemv)
PATHS = (("default", {}), ("variant 0", {"gemv_variant": 0}), ("variant 10", {"gemv_variant": 10}),
         ("variant 13", {"gemv_variant": 13}), ("variant 17", {"gemv_variant": 17}), ("generic", {"force_generic": 1}),
         ("nt_loads 0", {"nt_loads": 0}), ("symmetric 2", {"symmetric": 2}))


def _paths(s):
    """Switch the live context through every product path (as test_gemv_generic_path_agrees_with_tiled does)."""
    for name, opts in PATHS:
        for k, v in dict(BASE, **opts).items():
            s.set_option(k, v)
        yield f"{name} [{s.gemv_kernel_name()}]"
    for k, v in BASE.items():
        s.set_option(k, v)


@contextlib.contextmanager
def _integer_contexts(lam, dtype_name, n, shard_counts, vecs):
    """One context per shard count (all on GPU 0), the integer matrix streamed into all of them in row blocks; yields
    (contexts, [A v for v in vecs]) with exact references."""
    with contextlib.ExitStack() as st:
        ctxs = [st.enter_context(lam.Solver(getattr(lam, dtype_name), device_ids=[0] * P)) for P in shard_counts if P <= n]
        for s in ctxs:
            s.set_problem(n)
        refs = E.generate(n, [s.upload_rows for s in ctxs], vecs)
        yield ctxs, refs


def _check_gemv_exact(s, x, y_exact, label):
    want = y_exact.astype(s.vec_dtype)          # integers below 2^24: exact in the vector type
    for path in _paths(s):
        y = s.gemv(x)
        bad = np.flatnonzero(y != want)
        assert bad.size == 0, f"{label}, {path}: {bad.size} of {y.size} rows wrong, first rows {bad[:6]}: {y[bad[:6]]} != {want[bad[:6]]}"


# ------------------------------------------------------------------------------------------------
# 2. known answer for the GEMV at the structural edges, zero tolerance
# ------------------------------------------------------------------------------------------------
def _edge_sizes(V):
    sizes = set(range(1, 2 * V + 2))                                   # one lane's vector, two, the first partial one
    for base in (64 * V, 64 * V * 4, 64 * V * 8):                      # a wave step, a 4- and an 8-wave super-step
        sizes |= {base + d for d in (-V, -1, 0, 1, V)}
    sizes |= {4095, 4096, 4097, 4096 + V, 8191, 8193}                  # one column tile, its edges, two tiles
    # 3 and 8 shards (the reference's split: the remainder on the last shard) with 1 ... R + 1 rows on a shard, R = 2, 4, 16
    sizes |= {P * k for P in (3, 8) for k in (1, 2, 3, 4, 5, 16, 17)} | {8 * 17 + 7}
    return sorted(sizes)


@pytest.mark.parametrize("dtype_name,n", [(d, n) for d in DTYPES for n in _edge_sizes(VEC[d])])
def test_gemv_known_answer_at_edges(lam, dtype_name, n):
    x = E.int_vec(n, n + 1)
    with _integer_contexts(lam, dtype_name, n, (1, 3, 8), [x]) as (ctxs, (y,)):
        for s in ctxs:
            _check_gemv_exact(s, x, y, f"{dtype_name} n={n} shards={s.num_shards()[0]}")


# ------------------------------------------------------------------------------------------------
# 2 + 3 at a multi-tile size: GEMV known answer on every shard count, first CG step on every topology
# ------------------------------------------------------------------------------------------------
def _topologies(P, n):
    """(label, options) of the CG step on a context of P shards: the exchanges x fused / separate updates, the symmetric product,
    a column panel [lo, hi) inside the matrix (panel 2 then runs two segments, accumulated onto y)."""
    lo, hi = n // 3 // 8 * 8, 2 * n // 3 // 8 * 8
    panel = {"panel_lo": lo, "panel_hi": hi}
    if P == 1:
        return [("fused", {}), ("separate updates", {"fuse_update": 0}), ("symmetric 2", {"symmetric": 2}), ("panel", panel)]
    out = [(f"exchange {e} fuse_update {f}", {"exchange": e, "fuse_update": f}) for e in (0, 1, 2) for f in (0, 1)]
    return out + [("symmetric 2", {"exchange": 1, "symmetric": 2}), ("panel", dict(panel, exchange=0))]


CG_BASE = {"fuse_update": 1, "symmetric": 0, "panel_lo": 0, "panel_hi": 0}


def _check_first_step(s, dtype_name, b, Ab, label):
    vdt = s.vec_dtype
    alpha, x1, bb, pAp, r1 = E.first_cg_step(b, Ab, vdt)
    x1 = x1 + vdt(0)                               # the kernels start from x = +0: -0 + +0 = +0
    re_host, bound = E.rel_err_bound(b, Ab, alpha, r1, bb, U_TV[dtype_name])
    P = s.num_shards()[0]
    for name, opts in _topologies(P, s.n):
        for k, v in {**CG_BASE, **({"exchange": 0} if P > 1 else {}), **opts}.items():
            s.set_option(k, v)
        s.solve(1, 1e-30)
        st = s.stats
        x = s.solution()
        where = f"{label} {name}"
        assert st["num_iters"] == 2, where        # max_iters used up: the reference reports max_iters + 1
        bad = np.flatnonzero(x.view(np.uint64 if vdt == np.float64 else np.uint32) != x1.view(np.uint64 if vdt == np.float64 else np.uint32))
        assert bad.size == 0, f"{where}: x1 differs in {bad.size} entries (alpha {alpha!r}, b.b {bb}, p.Ap {pAp}), first {bad[:6]}"
        assert abs(st["rel_err"] - re_host) <= bound, (where, st["rel_err"], re_host, bound)
    for k, v in CG_BASE.items():
        s.set_option(k, v)


MULTI_TILE = [("F64", 20483, (1, 2, 3, 8)), ("F32", 20483, (1, 2, 3, 8)), ("BF16", 20483, (1, 2, 3, 8)),
              slow("F32", 65537, (1, 3)), slow("BF16", 65537, (1, 3))]


@pytest.mark.parametrize("dtype_name,n,shard_counts", MULTI_TILE)
def test_known_answers_at_multi_tile_size(lam, dtype_name, n, shard_counts):
    """GEMV: y = A x bit for bit on every path; CG: solve(1, 1e-30) from x = 0 returns x1 = fl(alpha_TV b) bit for bit, alpha =
    fl64(b.b / b.Ab) -- which pins b.b (cg_init), p.Ap summed from every GEMV workgroup's partial on every shard, the division
    and the x update -- and reports rel_err = sqrt(r1.r1 / b.b) within exact_data.rel_err_bound."""
    x, b = E.int_vec(n, 11), E.int_vec(n, 12)
    with _integer_contexts(lam, dtype_name, n, shard_counts, [x, b]) as (ctxs, (y, Ab)):
        for s in ctxs:
            s.set_rhs(b)
            label = f"{dtype_name} n={n} shards={s.num_shards()[0]}"
            _check_gemv_exact(s, x, y, label)
            _check_first_step(s, dtype_name, b, Ab, label)


@pytest.mark.parametrize("dtype_name,P,exchange", [("F64", 2, 0), ("F64", 3, 1), ("F64", 3, 2), ("F32", 3, 0), ("BF16", 2, 1)])
def test_first_step_rank_mode(lam, mock_async, tmp_path, dtype_name, P, exchange):
    """Rank mode (one context per rank, threads of one process, the stream-ordered RCCL double): the same exact first step on
    rank 0's x.  The integer system goes through a reference-format file (file mode)."""
    from oracle import pyoracle
    n = 3001
    fdt = np.float64 if dtype_name == "F64" else np.float32
    b = E.int_vec(n, 12)
    mat, rhs, xout = tmp_path / "A.bin", tmp_path / "b.bin", tmp_path / "x.npy"
    A = np.empty((n, n), dtype=fdt)
    (Ab,) = E.generate(n, [lambda r0, blk: A.__setitem__(slice(r0, r0 + blk.shape[0]), blk)], [b])
    pyoracle.write_bin(str(mat), A)
    pyoracle.write_bin(str(rhs), b.astype(fdt))
    del A
    env = dict(os.environ, LD_PRELOAD=mock_async, GPU_MAX_HW_QUEUES=str(2 * P + 4), MOCK_RCCL_TIMEOUT_MS="20000",
               MOCK_RCCL_STATS_FILE=str(tmp_path / "mock_stats.jsonl"))
    r = subprocess.run([sys.executable, os.path.join(MOCK_DIR, "run_ranks.py"), str(P), "0", "file", "--matrix", str(mat),
                        "--rhs", str(rhs), "--iters", "1", "--tol", "1e-30", "--save-x", str(xout), "--no-single",
                        "--exchange", str(exchange), "--dtype", dtype_name.lower()], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["ranks_identical"] and out["iters"] == 2, out          # max_iters + 1, as the reference reports it
    vdt = np.float64 if dtype_name == "F64" else np.float32
    alpha, x1, bb, pAp, r1 = E.first_cg_step(b, Ab, vdt)
    x1 = x1 + vdt(0)
    x = np.load(str(xout))
    assert x.dtype == vdt and np.array_equal(x.view(np.uint8), x1.view(np.uint8)), (alpha, bb, pAp)
    re_host, bound = E.rel_err_bound(b, Ab, alpha, r1, bb, U_TV[dtype_name])
    assert abs(out["rel_err"] - re_host) <= bound, (out["rel_err"], re_host, bound)


# ------------------------------------------------------------------------------------------------
# 4. non-finite entries propagate like the reference loop
# ------------------------------------------------------------------------------------------------
def _row_class(y):
    return np.where(np.isnan(y), 3, np.where(np.isposinf(y), 1, np.where(np.isneginf(y), 2, 0)))


@pytest.mark.parametrize("n", [1001, 6150])
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_nonfinite_entries_propagate(lam, dtype_name, n):
    """+Inf in the last VEC columns of some rows (the vector the lanes past a ragged tile's end re-read), -Inf in the first column
    of another, NaN in one more -- each planted at (i, j) and (j, i), so the symmetric product sees the same matrix.  The class of
    every row (finite / +Inf / -Inf / NaN) must be that of a plain fp64 elementwise product and sum (IEEE rules, as the reference's
    loop); finite rows keep the usual gate.  n = 1001 is one ragged tile, n = 6150 a full tile and a ragged one."""
    V = VEC[dtype_name]
    rng = np.random.default_rng(n + 17)
    R = rng.uniform(-1, 1, (n, n))
    A = 0.5 * (R + R.T)
    del R
    for i in (5, n // 2, n - V - 3):
        A[i, n - V:] = np.inf
        A[n - V:, i] = np.inf
    A[7, 0] = A[0, 7] = -np.inf
    A[11, n // 3] = A[n // 3, 11] = np.nan
    x = rng.uniform(0.5, 1.0, n)
    for shards in (1, 3):
        with lam.Solver(getattr(lam, dtype_name), device_ids=[0] * shards) as s:
            s.set_matrix(A)
            A_dev = s.download_rows(0, n).astype(np.float64) if dtype_name == "BF16" else A.astype(s.mat_host_dtype).astype(np.float64)
            xv = x.astype(s.vec_dtype)
            x64 = xv.astype(np.float64)
            with np.errstate(invalid="ignore"):
                want = (A_dev * x64).sum(axis=1)
                cls = _row_class(want)
                fin = cls == 0
                scale = np.abs(A_dev[fin]) @ np.abs(x64)
            assert set(cls) == {0, 1, 2, 3}
            for path in _paths(s):
                y = s.gemv(xv).astype(np.float64)
                got = _row_class(y)
                bad = np.flatnonzero(got != cls)
                assert bad.size == 0, (f"{dtype_name} n={n} shards={shards} {path}: rows {bad[:8]} are class {got[bad[:8]]}, "
                                       f"the fp64 loop gives {cls[bad[:8]]} (0 finite, 1 +Inf, 2 -Inf, 3 NaN)")
                assert np.max(np.abs(y[fin] - want[fin]) / scale) <= GATE[dtype_name], (dtype_name, n, shards, path)


# ------------------------------------------------------------------------------------------------
# 5. dense random data at multi-tile sizes: precision against an fp64 product of the matrix the device holds
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name,n,shard_counts", [(d, n, P) for d in DTYPES for n, P in ((4097 + VEC[d], (1, 3)), (8193, (1, 3)),
                                                                                            (12289, (1,)))]
                         + [slow(d, 12289, (3,)) for d in DTYPES])
def test_dense_random_multi_tile(lam, dtype_name, n, shard_counts):
    rng = np.random.default_rng(n)
    R = rng.uniform(-1, 1, (n, n))
    A = 0.5 * (R + R.T)                 # symmetric: the symmetric product is one of the paths
    del R
    x = rng.uniform(-1, 1, n)
    for shards in shard_counts:
        with lam.Solver(getattr(lam, dtype_name), device_ids=[0] * shards) as s:
            s.set_matrix(A)
            A_dev = s.download_rows(0, n).astype(np.float64) if dtype_name == "BF16" else A.astype(s.mat_host_dtype).astype(np.float64)
            xv = x.astype(s.vec_dtype)
            y64 = A_dev @ xv.astype(np.float64)
            scale = np.abs(A_dev) @ np.abs(xv.astype(np.float64))
            for path in _paths(s):
                y = s.gemv(xv).astype(np.float64)
                err = np.max(np.abs(y - y64) / scale)
                assert err <= GATE[dtype_name], (dtype_name, n, shards, path, err)
