"""The packed fp64 matrix format (option "packed") on the host: csrc/lam_host_pack.h -- the header the product build includes, no HIP
in it -- as a stand-alone program with its own main under g++ -fsanitize=address,undefined (tests/host_pack/pack_asan_main.cpp), built
and run as an executable.  The program runs encode -> decode over row-tiles of random bit patterns, the generator model's law,
all-equal exponents, every special value, exactly CAP and CAP + 1 exceptions and ragged tiles, and checks the decoded bits, the
exception count, the overflow condition and that the chosen window is a maximal one."""
import os
import subprocess

import numpy as np

from conftest import ROOT, PKG_NAME
from generator_model import random_spd

CSRC = os.path.join(ROOT, PKG_NAME, "csrc")


def test_the_product_build_includes_the_same_format_header():
    header = open(os.path.join(CSRC, "lam_host_pack.h")).read()
    assert "hip_runtime" not in header and "#include <hip" not in header
    kernels = open(os.path.join(CSRC, "lam_kernels.h")).read()
    assert '#include "lam_host_pack.h"' in kernels
    # the kernels code and decode through the header's element functions, not through copies of them
    for fn in ("pack_encode(", "pack_encode_exception(", "pack_in_window(", "pack_window_count(", "pack_window_key(", "pack_decode(",
               "pack_is_exception(", "pack_header("):
        assert fn in kernels and "LAM_HOST_DEVICE" in header.split(fn)[0].splitlines()[-1], fn


def test_format_under_sanitizers(tmp_path):
    exe = str(tmp_path / "pack_asan.out")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                        os.path.join(ROOT, "tests", "host_pack", "pack_asan_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0 and r.stdout.strip().endswith("ok pack"), r.stdout[-2000:] + r.stderr[-2000:]


def test_the_generator_models_matrix_leaves_a_few_dozen_elements_per_tile_outside_the_best_window():
    """The byte model's premise, on the host model of the benchmark's generator: per row of random_spd(4096, 1234, 1e6) (one 4096-column
    tile) the best window of 7 consecutive binades leaves out a few dozen elements -- far below CAP = 256."""
    A = np.asarray(random_spd(4096, 1234, 1e6), dtype=np.float64)
    e = (A.view(np.uint64) >> np.uint64(52)).astype(np.int64) & 0x7FF
    worst, total = 0, 0
    for row in e[::64]:
        hist = np.bincount(row[(row >= 1) & (row <= 2046)], minlength=2048)
        inside = np.convolve(hist, np.ones(7, dtype=np.int64)).max()
        worst, total = max(worst, 4096 - inside), total + 4096 - inside
    assert worst <= 100 and 20 <= total / len(e[::64]) <= 45, (worst, total / len(e[::64]))
