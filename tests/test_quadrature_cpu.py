"""The Lanczos quadrature without a GPU: the gates of tests/quadrature_data.py re-measured on the model, the model's own teeth (Gauss
exactness and where it ends), lam_hip_tridiag_quadrature (host only) against numpy.linalg.eigh, csrc/lam_host_quad.h under the
sanitizers as a stand-alone program, and the device entry points' refusals without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import quadrature_data as D
import quadrature_reference as Q
from conftest import PKG_NAME, ROOT
from pcg_reference import ORDERS


# ------------------------------------------------------------------------------------------------
# 1. the gates are what the model measures
# ------------------------------------------------------------------------------------------------
def _in_band(measured, gate, what):
    """The gate is 10 x what was measured when the table was written; re-measured, the figure lies between a hundredth and three tenths
    of it (tests/test_minres_cpu.py's band: another BLAS moves a maximum over few values by small factors, not by orders)."""
    print(f"{what}: measured {measured:.2e}, gate {gate:.1e}")
    assert 0.01 * gate <= measured <= 0.3 * gate, (what, measured, gate)


@pytest.mark.parametrize("dtype_name", ["F64", "F32"])
@pytest.mark.parametrize("name", sorted(D.COEFF_SYSTEMS))
def test_coefficient_gates_are_ten_times_the_models_own_spread(name, dtype_name):
    sp = D.measure_coefficient_spreads(name, dtype_name)
    assert tuple(sorted(D.COEFF_GATE[(name, dtype_name)])) == D.COEFF_K
    for k in D.COEFF_K:
        # every step the GPU test compares is gated: the model stays under lanczos_data's cap
        assert sp[k] <= D.UNGATED_ABOVE, (name, dtype_name, k, sp[k])
        _in_band(sp[k], D.COEFF_GATE[(name, dtype_name)][k], f"{name} {dtype_name} k={k}")
    for o in ORDERS:
        assert (D.model_run(name, dtype_name, o)["steps_run"] == D.COEFF_STEPS).all()      # no probe breaks down on the way


@pytest.mark.parametrize("dtype_name", ["F64", "F32"])
def test_quadrature_gates_are_ten_times_the_models_own_error(dtype_name):
    worst, _ = D.measure_moment_errors(dtype_name)
    _in_band(worst, D.MOMENT_GATE[dtype_name], f"moments {dtype_name}")
    conv = D.measure_convergence_errors(dtype_name)
    tr = D.measure_trace_errors(dtype_name)
    for fn in (Q.LOG, Q.INV):
        _in_band(conv[fn], D.CONV_GATE[dtype_name][fn], f"convergence {dtype_name} fn={fn}")
        _in_band(tr[fn], D.TRACE_GATE[dtype_name][fn], f"trace {dtype_name} fn={fn}")
    for o in ORDERS:
        assert (D.trace_model_run(dtype_name, o)["steps_run"] == D.TRACE_N).all()


# ------------------------------------------------------------------------------------------------
# 2. Gauss exactness gives the model teeth
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", ["F64", "F32"])
def test_six_steps_integrate_eleven_powers_and_not_the_twelfth(dtype_name):
    """m = 6 steps from a Rademacher probe on the n = 384 tracking system: N e_1^T T^p e_1 equals z^T A^p z to rounding for
    p = 0 .. 11 (degree 2m - 1) and misses at p = 12 by a figure that has nothing to do with rounding -- a quadrature that ignored T,
    or that lost a step, would not show this jump."""
    A, Z = D.system_matrix("tracking", dtype_name), D.system_probes("tracking", dtype_name)
    for o in ORDERS:
        run = D.model_run("tracking", dtype_name, o, D.MOMENT_STEPS)
        assert (run["znorm2"] == 384.0).all()
        e = D.moment_errors(run, A, Z, D.MOMENT_EXACT_P + (D.MOMENT_MISS_P,))
        print(dtype_name, o, {p: f"{v:.2e}" for p, v in e.items()})
        assert all(e[p] <= 0.3 * D.MOMENT_GATE[dtype_name] for p in D.MOMENT_EXACT_P), e
        assert e[D.MOMENT_MISS_P] >= D.MOMENT_MISS_AT_LEAST > 2 * D.MOMENT_GATE["F32"], e
        # p = 0 is the weights' sum alone
        assert e[0] <= 8 * 2.0 ** -53


def test_the_probe_law_is_rademacher():
    """+-1 only, both signs, different probes differ, and the global index is what counts: probe 9 of an 11-probe run is probe 9."""
    Z = Q.rademacher_probes(7, 11, 1030)
    assert set(np.unique(Z)) == {-1.0, 1.0} and abs(Z.mean()) < 0.05
    assert len({z.tobytes() for z in Z}) == 11
    assert np.array_equal(Z[9], Q.rademacher(7, 9, 1030))
    assert not np.array_equal(Z[9], Q.rademacher(8, 9, 1030))


# ------------------------------------------------------------------------------------------------
# 3. lam_hip_tridiag_quadrature against eigh
# ------------------------------------------------------------------------------------------------
def _random_tridiag(k, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(1.0, 3.0, k), rng.uniform(0.05, 0.45, max(k - 1, 0))          # diagonally dominant: positive definite


@pytest.mark.parametrize("k", [1, 2, 40, 256])
def test_tridiag_quadrature_agrees_with_eigh(lam, k):
    alpha, beta = _random_tridiag(k, k)
    shifts = np.array([0.0, 0.5, 2.0, -0.25])
    for fn, name, param in ((Q.LOG, "log", 0), (Q.INV, "inv", 0), (Q.POW, "pow", 0), (Q.POW, "pow", 3), (Q.POW, "pow", 11)):
        got = lam.tridiag_quadrature(alpha, beta, name, shifts, param)
        want = Q.gauss_quadrature(alpha, beta, fn, shifts, param)
        # both sum k weights that add up to 1 against values of one sign: 16 k ulp of the result
        assert np.abs(got / want - 1).max() <= 16 * k * 2.0 ** -53, (k, name, param, got, want)
    capi = lam
    # no shift: sigma NULL with nshifts 1
    assert abs(capi.tridiag_quadrature(alpha, beta, "inv")[0] / Q.gauss_quadrature(alpha, beta, Q.INV)[0] - 1) <= 16 * k * 2.0 ** -53
    # k = 1: f(alpha_1 + s) itself
    if k == 1:
        assert np.array_equal(capi.tridiag_quadrature(alpha, beta, "log", shifts), np.log(alpha[0] + shifts))


def test_tridiag_quadrature_refusals(lam):
    capi = lam
    alpha, beta = _random_tridiag(5, 5)
    theta = np.linalg.eigvalsh(Q.tridiag(alpha, beta))

    def refused(*a, **kw):
        with pytest.raises(capi.LamHipError) as e:
            capi.tridiag_quadrature(*a, **kw)
        assert e.value.code == -1, e.value
        return e.value

    # a node <= 0 under LOG: the first bad (shift, node) is reported -- shift 1 pushes the two smallest nodes below zero
    s_bad = -0.5 * (theta[1] + theta[2])
    e = refused(alpha, beta, "log", [0.0, s_bad, -100.0])
    assert e.bad == (1, 0) and "node 0 under shift 1" in str(e)
    # a node == 0 under INV: T = diag(2), shift -2
    e = refused([2.0], [], "inv", [1.0, -2.0])
    assert e.bad == (1, 0)
    # negative nodes are fine for INV and POW
    assert capi.tridiag_quadrature([2.0], [], "inv", [-3.0])[0] == -1.0 and capi.tridiag_quadrature([2.0], [], "pow", [-3.0], 3)[0] == -1.0
    # non-finite input
    for bad_value in (np.nan, np.inf):
        a = alpha.copy()
        a[2] = bad_value
        assert refused(a, beta, "inv").bad == (-1, -1)
        b = beta.copy()
        b[1] = bad_value
        refused(alpha, b, "inv")
        refused(alpha, beta, "inv", [0.0, bad_value])
    # k out of range
    refused([], [], "inv")
    refused(np.ones(257), np.zeros(256), "inv")
    # bad param, unknown function
    refused(alpha, beta, "pow", None, 2.5)
    refused(alpha, beta, "pow", None, -1)
    refused(alpha, beta, 3)
    # nshifts < 1 and NULL arrays at the C level
    L = lam.lib()
    dp = C.POINTER(C.c_double)
    out = np.zeros(1)
    assert L.lam_hip_tridiag_quadrature(5, alpha.ctypes.data_as(dp), beta.ctypes.data_as(dp), 1, 0.0, 0, None, out.ctypes.data_as(dp), None) == -1
    assert L.lam_hip_tridiag_quadrature(5, None, beta.ctypes.data_as(dp), 1, 0.0, 1, None, out.ctypes.data_as(dp), None) == -1
    assert L.lam_hip_tridiag_quadrature(5, alpha.ctypes.data_as(dp), beta.ctypes.data_as(dp), 1, 0.0, 2, None, out.ctypes.data_as(dp), None) == -1
    assert L.lam_hip_tridiag_quadrature(5, alpha.ctypes.data_as(dp), beta.ctypes.data_as(dp), 1, 0.0, 1, None, None, None) == -1


# ------------------------------------------------------------------------------------------------
# 4. the header under the sanitizers, as a stand-alone program
# ------------------------------------------------------------------------------------------------
def test_quadrature_header_under_sanitizers(tmp_path):
    """csrc/lam_host_quad.h -- the header the product build includes, no HIP in it -- as a stand-alone program with its own main under
    g++ -fsanitize=address,undefined: built and run as an executable, with every array at exactly its stated size."""
    csrc = os.path.join(ROOT, PKG_NAME, "csrc")
    header = open(os.path.join(csrc, "lam_host_quad.h")).read()
    assert "hip_runtime" not in header and "#include <hip" not in header
    assert '#include "lam_host_quad.h"' in open(os.path.join(csrc, "lam_kernels.h")).read()
    assert "lam::tridiag_quadrature(" in open(os.path.join(csrc, "lam_quad.h")).read()
    exe = str(tmp_path / "quad_asan.out")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", csrc,
                        os.path.join(ROOT, "tests", "host_quad", "quad_asan_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0 and r.stdout.strip().endswith("ok quadrature"), r.stdout[-2000:] + r.stderr[-2000:]


# ------------------------------------------------------------------------------------------------
# 5. without a device
# ------------------------------------------------------------------------------------------------
def test_device_entry_points_without_a_device(lam):
    """No context can exist without a GPU (lam_hip_create: LAM_HIP_ENODEV, no CPU path), and the three calls that need one refuse a
    NULL context with their argument error before they touch anything."""
    L = lam.lib()
    assert L.lam_hip_lanczos_many(None, 1, None, 0, 1, None, None, None, None, None) == -1
    assert L.lam_hip_get_lanczos_many(None, 1, None, None, None, None, None) == -1
    assert L.lam_hip_trace_quadrature(None, 0, 0.0, 1, None, None, None, None) == -1
    code = ("import importlib, sys; sys.path.insert(0, %r)\n"
            "m = importlib.import_module(%r)\n"
            "try:\n    m.Solver().logdet(); print('RAN')\n"
            "except m.LamHipError as e:\n    print('ERR', e.code)\n" % (ROOT, PKG_NAME))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="")
    import sys
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True).stdout
    assert "ERR -2" in out, out
