"""test_CG_multi_rhs.out -Y 0|1|2: option "symmetric_many" from the generate-mode driver.  The CSV on stdout keeps its columns; which
product ran is one line on stderr."""
import os
import subprocess

import pytest

from conftest import ROOT, PKG_NAME

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, PKG_NAME, "test", "test_CG_multi_rhs.out")
N = 1027            # two full strips of the symmetric plan plus a ragged one (fp64)


def _run(*args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, timeout=300)


def _columns(r):
    """(num_iters, rel_err, true residual) per CSV line."""
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [ln.split(",") for ln in r.stdout.strip().splitlines()]
    return [(int(f[7]), float(f[8]), float(f[10])) for f in rows]


@pytest.mark.parametrize("prec,tol,extra", [("f64", 1e-9, []), ("f32", 1e-5, []), ("f64", 1e-9, ["-J"]), ("f64", 1e-9, ["-m"])],
                         ids=["f64", "f32", "f64 jacobi", "f64 minres"])
def test_driver_runs_the_symmetric_product_and_says_so(prec, tol, extra):
    """tridiag(1,2,1), 4 columns: -Y 2 reports the symmetric product and -Y 0 the general one; both converge, the symmetric run's true
    residual is <= 2 max(the general run's, rel_error) (the gate tests/test_gpu_mshift.py puts on two recurrences that stop a few
    iterations apart), and the per-column iteration counts agree within tests/test_gpu_multi_rhs.py's ITER_GATE: max(3, 2 %)
    iterations in fp64, max(3, 5 %) in fp32."""
    base = ["-s", N, "-k", 4, "-i", 4 * N, "-e", tol, "-t", prec, "-T"] + extra
    general, sym = _run(*base, "-Y", 0), _run(*base, "-Y", 2)
    assert "symmetric_many_effective = 0" in general.stderr and "general batched product" in general.stderr, general.stderr
    assert "symmetric_many_effective = 1" in sym.stderr and "symmetric batched product" in sym.stderr, sym.stderr
    cg, cs = _columns(general), _columns(sym)
    assert len(cg) == len(cs) == 4
    frac = 0.02 if prec == "f64" else 0.05
    for j, ((ig, rg, tg), (isym, rs, ts)) in enumerate(zip(cg, cs)):
        print(f"{prec} {extra} column {j}: iterations {ig} / {isym}, true residuals {tg:.3e} / {ts:.3e}")
        # the general product's own true residual is the yardstick where fp32 cannot reach 2 rel_error on this matrix (cond ~ 4e5)
        assert rg < tol and rs < tol and ts <= 2 * max(tg, tol), (j, rg, rs, tg, ts)
        assert abs(ig - isym) <= max(3, frac * ig), (j, ig, isym)
    plain = _run(*base)                                      # without -Y: nothing on stderr, the CSV of before
    assert plain.returncode == 0 and "symmetric_many" not in plain.stderr
    assert [c[0] for c in _columns(plain)] == [c[0] for c in cg]


def test_more_than_four_columns_proceed_on_the_general_product():
    r = _run("-s", N, "-k", 8, "-i", 4 * N, "-e", 1e-9, "-T", "-Y", 2)
    assert r.returncode == 0 and "symmetric_many_effective = 0" in r.stderr and "not effective for more than 4 columns" in r.stderr, r.stderr
    assert len(_columns(r)) == 8


def test_multishift_seed_runs_the_symmetric_product():
    r = _run("-s", N, "-i", 4 * N, "-e", 1e-9, "-S", "0,0.5,1,2,4,8,16,32,64", "-M", "-Y", 2)
    assert r.returncode == 0 and "symmetric_many_effective = 1" in r.stderr, r.stderr
    assert len(r.stdout.strip().splitlines()) == 9


def test_a_bad_value_is_a_usage_error():
    for bad in ("5", "-1", "22", "x"):
        r = _run("-s", 16, "-k", 2, "-i", 3, "-Y", bad)
        assert r.returncode == 1 and "Usage" in r.stderr and r.stdout == "", (bad, r.stderr)
