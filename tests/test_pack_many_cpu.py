"""The batched product's traversal of the packed image (option "packed_many") on the host: csrc/lam_host_pack.h's pack_many_pos -- the
function multi_gemv_packed_kernel calls -- walked by a stand-alone program with its own main under g++ -fsanitize=address,undefined
(tests/host_pack_many/pack_many_main.cpp), built and run as an executable.  For K = 1, 2, 4, ncols in 2, 384, 1548, 4096, 4098, 9002,
12288 and every starting tile of the rotation: every column below ncols exactly once, every lane's sequence of columns the one
multi_gemv_kernel's index arithmetic gives, pack_tile / unpack_tile round-tripped through the mapping, +0.0 behind a ragged end."""
import os
import subprocess

from conftest import ROOT, PKG_NAME

CSRC = os.path.join(ROOT, PKG_NAME, "csrc")


def test_the_kernel_calls_the_header_mapping():
    header = open(os.path.join(CSRC, "lam_host_pack.h")).read()
    assert "LAM_HOST_DEVICE void pack_many_pos(" in header
    kernels = open(os.path.join(CSRC, "lam_kernels.h")).read()
    body = kernels.split("multi_gemv_packed_kernel(MultiGemvArgs<double, double> a, PackedMat pk)")[1].split("\n}\n")[0]
    assert "pack_many_pos(" in body and "pack_decode(" in body and "pack_is_exception(" in body


def test_mapping_under_sanitizers(tmp_path):
    exe = str(tmp_path / "pack_many.out")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                        os.path.join(ROOT, "tests", "host_pack_many", "pack_many_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0 and r.stdout.strip().endswith("ok pack many"), r.stdout[-2000:] + r.stderr[-2000:]
    # 1 + 1 + 1 + 1 + 2 + 3 + 3 batch tiles at K = 1, twice and four times as many (rounded up) at K = 2 and 4: every start was walked
    assert r.stdout.splitlines()[-2] == "%d walks" % (12 + (1 + 1 + 1 + 2 + 3 + 5 + 6) + (1 + 1 + 2 + 4 + 5 + 9 + 12))
