"""What the gates of tests/test_gpu_single_recurrence.py rest on, re-measured without the library: the tracked systems in their three
storage types, and every reference's own spread between summation orders at every tracked k, which must stay at or below a TENTH
of the gate (tests/tracking_data.py has the table and the rule that moves a gate where it does not)."""
import itertools

import numpy as np
import pytest

import generator_model as G
import pcg_reference as R
from tracking_data import (FP32_TRACKING_GATE, ITERATION_TRACKING_GATES, SINGLE_FP32_GATE_OVERRIDES, SINGLE_TRACKING_DTYPES,
                           SINGLE_TRACKING_N, TRACKED_K, TRACKED_K_FP32, iteration_tracking_system, single_tracking_gates,
                           stored_tracking_system, tracking_system)


def _rel(x, x0):
    x, x0 = x.astype(np.float64), x0.astype(np.float64)
    return np.linalg.norm(x - x0) / np.linalg.norm(x0)


def test_tracked_systems_are_what_the_table_says():
    """Symmetric bit for bit and positive definite in every storage type; the bf16 matrix holds bf16 numbers and is the fp32 one
    rounded to nearest even; lambda_min and cond of n = 1547 as recorded; the slices of n = 1547 are odd, ragged and longer than a
    workgroup of the vector step."""
    A0, b0 = iteration_tracking_system()
    assert np.array_equal(A0, tracking_system(384)[0]) and np.array_equal(b0, tracking_system(384)[1]) and A0.flags.writeable
    recorded = {(1547, "F64"): (0.04996, 400.6), (1547, "F32"): (0.04996, 400.6), (1547, "BF16"): (0.04819, 415.3)}
    for n in SINGLE_TRACKING_N:
        A64, b64 = tracking_system(n)
        for name in SINGLE_TRACKING_DTYPES:
            A, b = stored_tracking_system(n, name)
            assert A.shape == (n, n) and b.shape == (n,) and not A.flags.writeable and not b.flags.writeable
            assert A.dtype == (np.float64 if name == "F64" else np.float32) and b.dtype == G.VEC_DTYPE[name]
            assert np.array_equal(A, A.T) and np.array_equal(b, b64.astype(b.dtype))
            w = np.linalg.eigvalsh(A.astype(np.float64))
            assert w[0] > 0.04 and w[-1] / w[0] < 450, (n, name, w[0], w[-1])
            if (n, name) in recorded:
                lmin, cond = recorded[n, name]
                assert abs(w[0] - lmin) < 5e-5 and abs(w[-1] / w[0] - cond) < 0.05, (n, name, w[0], w[-1] / w[0])
            if name == "F32":
                assert np.array_equal(A, A64.astype(np.float32))
            if name == "BF16":
                a32 = A64.astype(np.float32)
                assert not (A.view(np.uint32) & 0xFFFF).any()                                                   # bf16 numbers ...
                up, down = A.view(np.uint32) + np.uint32(0x10000), A.view(np.uint32) - np.uint32(0x10000)       # ... no neighbour nearer
                d = np.abs(A.astype(np.float64) - a32)
                assert (d <= np.abs(up.view(np.float32).astype(np.float64) - a32)).all() and (d <= np.abs(down.view(np.float32).astype(np.float64) - a32)).all()
    n = 1547
    assert [n // P for P in (2, 3, 5, 7, 8)] == [773, 515, 309, 221, 193]        # odd; longer than a workgroup (256) up to P = 5
    assert [n % P for P in (2, 3, 5, 8)] == [1, 2, 2, 3] and 384 // 33 == 11 and 384 % 33 == 21


def test_track_is_the_capped_run_bit_for_bit():
    """pcg / pcg_ordered(track=...) hand out x and rel_err after iteration k as the run capped at k returns them."""
    A, b = stored_tracking_system(384, "BF16")
    for fn in (R.pcg, R.pcg_ordered):
        track = dict.fromkeys((1, 2, 5, 10))
        fn(A, b, 12, 1e-30, None, np.float32, track=track)
        for k in track:
            x, st = fn(A, b, k, 1e-30, None, np.float32)
            assert x.dtype == np.float32 and np.array_equal(x, track[k][0]) and st["rel_err"] == track[k][1], (fn.__name__, k)


def test_gates_are_the_shared_ones_except_where_the_table_moves_them():
    for n in SINGLE_TRACKING_N:
        g = single_tracking_gates(n, "F64")
        assert g == {k: (r, x, True) for k, r, x in ITERATION_TRACKING_GATES if k in TRACKED_K} and sorted(g) == [1, 2, 5, 20, 40]
        for name in ("F32", "BF16"):
            g = single_tracking_gates(n, name)
            assert sorted(g) == list(TRACKED_K_FP32) == [1, 2, 5, 10, 20, 30, 40]
            for k, (g_res, g_x, asserted) in g.items():
                moved = SINGLE_FP32_GATE_OVERRIDES.get((n, name), {}).get(k)
                assert g_res == g_x == (moved or FP32_TRACKING_GATE[k]) and asserted == (k != 40)
                assert moved is None or FP32_TRACKING_GATE[k] < moved < 1.5 * FP32_TRACKING_GATE[k]
    assert set(SINGLE_FP32_GATE_OVERRIDES) == {(1547, "F32"), (1547, "BF16")}


@pytest.mark.parametrize("n", SINGLE_TRACKING_N)
def test_the_oracle_is_a_tenth_of_the_gate_sure_of_the_single_solve(oracle, n):
    """fp64: the oracle at 1 thread (the GPU test's reference) against 4 and 8 threads and against 2, 3, 5 and 8 emulated ranks --
    the shard counts the GPU test runs, whose reductions the ranks restate; n = 384: 33 ranks too."""
    A, b = tracking_system(n)
    gates = single_tracking_gates(n, "F64")
    others = [dict(threads=4), dict(threads=8)] + [dict(threads=1, P=P) for P in (2, 3, 5, 8) + ((33,) if n == 384 else ())]
    for k, (gate_res, gate_x, _) in gates.items():
        x1, s1 = oracle.cg_solve(A, b, k, 1e-30, threads=1)
        for kw in others:
            x2, s2 = oracle.cg_solve(A, b, k, 1e-30, **kw)
            d_re, d_x = abs(s2["rel_err"] / s1["rel_err"] - 1), _rel(x2, x1)
            print(f"fp64 n={n} k={k} {kw}: rel_err {d_re:.2e} (gate {gate_res:.0e}), x {d_x:.2e} (gate {gate_x:.0e})")
            assert s1["num_iters"] == s2["num_iters"] == k + 1 and d_re <= 0.1 * gate_res and d_x <= 0.1 * gate_x, (n, k, kw, d_re, d_x)


@pytest.mark.parametrize("dtype_name", ["F32", "BF16"])
@pytest.mark.parametrize("n", SINGLE_TRACKING_N)
def test_the_fp32_reference_is_a_tenth_of_the_gate_sure_of_the_single_solve(n, dtype_name):
    """fp32 vectors on the fp32- and on the bf16-rounded matrix: pcg_ordered "rows" (the GPU test's reference) against "reversed",
    "lanes" and pcg (BLAS), x and rel_err, all pairs.  k = 40 is informational in the GPU test and is printed here."""
    A, b = stored_tracking_system(n, dtype_name)
    gates = single_tracking_gates(n, dtype_name)
    runs = [lambda t: R.pcg(A, b, 40, 1e-30, None, np.float32, track=t)]
    runs += [lambda t, o=o: R.pcg_ordered(A, b, 40, 1e-30, None, np.float32, o, track=t) for o in R.ORDERS]
    tracks = []
    for run in runs:
        tracks.append(dict.fromkeys(gates))
        _, st = run(tracks[-1])
        assert st["num_iters"] == 41 and not st["converged"]
    for k, (gate, _, asserted) in gates.items():
        worst = max(max(_rel(a[k][0], c[k][0]), abs(a[k][1] / c[k][1] - 1)) for a, c in itertools.combinations(tracks, 2))
        fixed = max(max(_rel(a[k][0], c[k][0]), abs(a[k][1] / c[k][1] - 1)) for a, c in itertools.combinations(tracks[1:], 2))
        print(f"{dtype_name} n={n} k={k}: spread {worst:.3e} (between the fixed orders {fixed:.3e}), gate {gate:.1e}" + ("" if asserted else " (informational)"))
        assert not asserted or 10 * worst <= gate, (n, dtype_name, k, worst, gate)
