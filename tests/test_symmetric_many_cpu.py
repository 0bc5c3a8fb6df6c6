"""Option "symmetric_many" without a GPU: the header says what holds, the driver refuses a bad -Y before it touches a device, and the
compiler's resource report of every instantiation of the two K-wide kernels, and of the single symmetric product's kernels, whose
second pass is the same body (cross-compiled for gfx950), shows no scratch and the registers that keep three workgroups per CU."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT, PKG_NAME

HEADER = os.path.join(ROOT, "include", "lam_hip.h")
CSRC = os.path.join(ROOT, PKG_NAME, "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


def test_header_documents_the_option_and_no_longer_says_symmetric_never_applies():
    text = open(HEADER).read()
    assert '"symmetric_many"' in text and '"symmetric_many_effective"' in text
    assert "does NOT apply" not in text
    assert "N (N + 1) / 2 + 2 K N" in text                     # the byte model of stats.gemv_bytes under the option


def test_driver_refuses_a_bad_value_before_touching_a_gpu(lam):
    lam.build()
    exe = os.path.join(ROOT, PKG_NAME, "test", "test_CG_multi_rhs.out")
    r = subprocess.run([exe, "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "-Y" in r.stderr
    for bad in ("5", "3", "-1", "x"):
        r = subprocess.run([exe, "-s", "16", "-k", "2", "-i", "3", "-Y", bad], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "Usage" in r.stderr and r.stdout == "", (bad, r.stderr)


INSTANTIATIONS = [(t, k) for t in ("double", "float") for k in (1, 2, 4)]
# the single product's entry points the library launches: (storage, vectors, columns of a strip), CYC false and true each
SINGLE = [("double", "double", 512), ("float", "float", 1024), ("__hip_bfloat16", "float", 2048)]
ITANIUM = {"double": "d", "float": "f", "__hip_bfloat16": "14__hip_bfloat16"}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs the ROCm compiler")
def test_resource_report_has_no_scratch_and_keeps_three_workgroups_per_cu(tmp_path):
    """-Rpass-analysis=kernel-resource-usage on a translation unit that instantiates exactly the kernels the library launches.
    Scratch must be 0 everywhere; <= 168 VGPRs (AGPRs included) keeps the task kernel's three 4-wave workgroups per CU; its LDS is
    the K-wide row buffer, 4 waves x 256 rows x K elements."""
    lines = ['#include "lam_kernels.h"', "using namespace lam;"]
    for t, k in INSTANTIATIONS:
        ss = 256 * (2 if t == "double" else 4)
        lines.append(f"template __global__ void lam::symv_many_task_kernel<{t}, {t}, {k}>(const {t} *, const {t} *, const SymvTask *, {t} *, "
                     f"{t} *, uint64_t, uint64_t, uint64_t, const MultiScalars *);")
        for shift in ("true", "false"):
            lines.append(f"template __global__ void lam::symv_many_reduce_kernel<{t}, {ss}, {k}, {shift}>(const {t} *, const {t} *, "
                         f"const uint32_t *, SymvIndex, const {t} *, {t} *, double *, uint64_t, ShiftArg<{t}>, const MultiScalars *);")
    for ta, t, ss in SINGLE:
        for cyc in ("false", "true"):
            lines.append(f"template __global__ void lam::symv_task_kernel<{ta}, {t}, {cyc}>(const {ta} *, const {t} *, const SymvTask *, {t} *, "
                         f"{t} *, uint64_t, uint64_t, uint64_t, uint64_t, const CgScalars *);")
        lines.append(f"template __global__ void lam::symv_reduce_kernel<{t}, {ss}>(const {t} *, const {t} *, const uint32_t *, SymvIndex, "
                     f"const {t} *, {t} *, double *, uint64_t, uint64_t, uint64_t, PtrList, Finalize, const CgScalars *);")
    src = tmp_path / "symv_many_resources.hip"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"),
                        "-Rpass-analysis=kernel-resource-usage", "-c", str(src), "-o", str(tmp_path / "out.o")],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    blocks = re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]
    seen = {}
    for b in blocks:
        name = b.split()[0]
        g = lambda key: int(re.search(key + r": (\d+)", b).group(1))       # noqa: E731
        seen[name] = dict(vgpr=g("VGPRs"), agpr=g("AGPRs"), scratch=g(r"ScratchSize \[bytes/lane\]"), lds=g(r"LDS Size \[bytes/block\]"),
                          waves=g(r"Occupancy \[waves/SIMD\]"))
    filt = shutil.which("c++filt")
    names = list(seen)
    dem = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True).stdout.splitlines() if filt else names
    tasks = reduces = single_tasks = single_reduces = 0
    for name, d in zip(names, dem):
        res = seen[name]
        print(f"{d[:110]:110s} {res}")
        assert res["scratch"] == 0, (d, res)
        if "symv_many_task_kernel" in name:
            tasks += 1
            assert res["vgpr"] + res["agpr"] <= 168, (d, res)
        elif "symv_many_reduce_kernel" in name:
            reduces += 1
            assert res["vgpr"] + res["agpr"] <= 128 and res["waves"] >= 4, (d, res)
        elif "symv_task_kernel" in name:
            single_tasks += 1
            assert res["vgpr"] + res["agpr"] <= 168, (d, res)
        elif "symv_reduce_kernel" in name:
            single_reduces += 1
            assert res["vgpr"] + res["agpr"] <= 128 and res["waves"] >= 4, (d, res)
    assert tasks == len(INSTANTIATIONS) and reduces == 2 * len(INSTANTIATIONS), sorted(dem)
    assert single_tasks == 2 * len(SINGLE) and single_reduces == len(SINGLE), sorted(dem)
    for ta, t, ss in SINGLE:                # K = 1: 4 waves x 256 rows x one element of the vector type
        mangled = [n for n in names if "symv_task_kernel" in n and f"I{ITANIUM[ta]}{ITANIUM[t]}Lb" in n]
        assert len(mangled) == 2 and all(seen[m]["lds"] == 4 * 256 * (8 if t == "double" else 4) for m in mangled), (ta, t, mangled)
    for t, k in INSTANTIATIONS:
        mangled = [n for n in names if "symv_many_task_kernel" in n and f"I{'d' if t == 'double' else 'f'}{'d' if t == 'double' else 'f'}Li{k}E" in n]
        assert len(mangled) == 1 and seen[mangled[0]]["lds"] == 4 * 256 * k * (8 if t == "double" else 4), (t, k, mangled)
