"""CPU-side checks of the multi-right-hand-side entry points (include/lam_hip.h, "several right-hand sides on one matrix"): the
header still compiles as C99, the library exports them, the ABI version did not move, the batching of Solver.solve_all, the new
driver builds and the sanitized host build still links against its fake of the ABI without edits."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT, PKG_NAME

NEW = ("lam_hip_set_rhs_many", "lam_hip_solve_many", "lam_hip_get_solution_many", "lam_hip_gemv_many", "lam_hip_gemv_many_only")
HEADER = os.path.join(ROOT, "include", "lam_hip.h")


def test_header_compiles_as_c99_with_the_new_entry_points(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "lam_hip.h"\n'
                   "#if LAM_HIP_MAX_RHS != 8\n#error LAM_HIP_MAX_RHS\n#endif\n"
                   "int use(lam_hip_ctx *c, const double *b, double *x, double *t)\n{\n"
                   "    int32_t it[LAM_HIP_MAX_RHS], cv[LAM_HIP_MAX_RHS];\n    double re[LAM_HIP_MAX_RHS];\n    lam_hip_stats st;\n"
                   "    return lam_hip_set_rhs_many(c, 3, b) + lam_hip_solve_many(c, 10, 1e-9, &st, it, cv, re)\n"
                   "         + lam_hip_get_solution_many(c, 3, x) + lam_hip_gemv_many(c, 3, b, x) + lam_hip_gemv_many_only(c, 3, 5, t);\n}\n")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                        "-o", str(tmp_path / "use.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_library_exports_the_new_entry_points(lam):
    lam.build()
    L = C.CDLL(lam.lib_path())
    for name in NEW:
        assert hasattr(L, name), name
    assert set(NEW) <= set(lam.lib()._lam_symbols)


def test_abi_version_stays_4_and_the_history_names_the_additions(lam):
    txt = open(HEADER).read()
    assert re.search(r"#define LAM_HIP_ABI_VERSION 4\b", txt) and lam.lib().lam_hip_abi_version() == 4
    history = txt[txt.index("ABI history"):txt.index("#define LAM_HIP_ABI_VERSION")]
    for name in NEW + ("LAM_HIP_MAX_RHS", "multi_rhs_k"):
        assert name in history, name
    assert re.search(r"#define LAM_HIP_MAX_RHS 8\b", txt) and lam.MAX_RHS == 8


def test_solve_all_grouping(lam):
    assert lam.rhs_groups(19) == [(0, 8), (8, 8), (16, 3)]
    assert lam.rhs_groups(8) == [(0, 8)]
    assert lam.rhs_groups(1) == [(0, 1)] and lam.rhs_groups(0) == [] and lam.rhs_groups(9) == [(0, 8), (8, 1)]
    assert lam.rhs_groups(7, 3) == [(0, 3), (3, 3), (6, 1)]
    for n in range(0, 40):
        g = lam.rhs_groups(n)
        assert sum(c for _, c in g) == n and all(1 <= c <= lam.MAX_RHS for _, c in g)
        assert [f for f, _ in g] == list(range(0, n, lam.MAX_RHS))


def test_multi_rhs_driver_builds(lam):
    lam.build()
    exe = os.path.join(ROOT, PKG_NAME, "test", "test_CG_multi_rhs.out")
    assert os.path.exists(exe) and os.access(exe, os.X_OK)
    mk = open(os.path.join(ROOT, PKG_NAME, "Makefile")).read()
    assert "test_CG_multi_rhs.out" in mk
    # bad arguments are refused before anything touches a GPU
    r = subprocess.run([exe, "-s", "16", "-k", "9", "-i", "3"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "Usage" in r.stderr


def test_host_asan_still_builds_against_its_fake_of_the_abi():
    """ConjugateGradient_HIP_base::solve_many is a member of a class template: it is instantiated only where it is called, so the
    sanitized host build, whose fake ABI has no batched entry points, links as before."""
    here = os.path.join(ROOT, "tests", "host_asan")
    r = subprocess.run(["make", "-C", here, "all"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    fake = open(os.path.join(here, "fake_lam_hip.cpp")).read()
    assert "lam_hip_solve_many" not in fake
