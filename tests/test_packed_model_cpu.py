"""tests/packed_model.py against csrc/lam_host_pack.h, without a GPU.  The GPU tests (test_gpu_packed_edges.py) hold pack_rows_kernel's
headers and the byte model against the numpy model `headers`; here the numpy model is held against the header the product build
includes: tests/host_pack/pack_headers_main.cpp, a stand-alone program under g++ -fsanitize=address,undefined (built exactly as
test_pack_format_cpu.py builds its program), runs pack_tile on every (row, tile) of a matrix and writes the headers, and, after
unpack_tile, whether the bits came back."""
import os
import subprocess

import numpy as np
import pytest

import exact_data as E
import packed_model as M
from conftest import ROOT, PKG_NAME
from generator_model import random_spd

CSRC = os.path.join(ROOT, PKG_NAME, "csrc")


@pytest.fixture(scope="module")
def pack_headers(tmp_path_factory):
    """f(matrix) -> (base, count, flag), three (rows, tiles) arrays from the sanitizer build of pack_tile / unpack_tile."""
    tmp = tmp_path_factory.mktemp("pack_headers")
    exe = str(tmp / "pack_headers.out")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                        os.path.join(ROOT, "tests", "host_pack", "pack_headers_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")

    def run(A):
        rows = M.bits(A)
        src, dst = str(tmp / "in.bin"), str(tmp / "out.bin")
        with open(src, "wb") as f:
            f.write(np.array(rows.shape, dtype=np.uint64).tobytes())
            f.write(rows.tobytes())
        r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=300, env=env)
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-4000:]
        assert r.returncode == 0 and r.stdout.strip().endswith("ok headers"), r.stdout[-2000:] + r.stderr[-2000:]
        rec = np.fromfile(dst, dtype=np.uint32).reshape(rows.shape[0], -1, 2)
        return (rec[..., 0] & 0x7FF).astype(np.int64), (rec[..., 0] >> 16).astype(np.int64), rec[..., 1]
    return run


CASES = {"ladder 384": lambda: M.ladder(384), "ladder 1547": lambda: M.ladder(1547), "ladder 4097": lambda: M.ladder(4097),
         "random_spd 384": lambda: np.asarray(random_spd(384, 5, 100.0), dtype=np.float64)}


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_numpy_model_gives_pack_tiles_headers(pack_headers, case):
    A = CASES[case]()
    n = A.shape[1]
    base, count, flag = pack_headers(A)
    want_base, want_count = M.headers(M.bits(A), M.ncols_vec(n))
    assert base.shape == want_base.shape == (n, -(-M.ncols_vec(n) // M.TILE))
    assert np.array_equal(base, want_base), np.argwhere(base != want_base)[:8]
    assert np.array_equal(count, want_count), np.argwhere(count != want_count)[:8]
    assert np.all(flag == 1), np.argwhere(flag != 1)[:8]             # packable, and unpack_tile gives the bits back
    if case.startswith("ladder"):
        # what the ladder is for: windows at both ends of the exponent range, no two alike side by side, every list length
        assert base.min() == 7 and base.max() == 2046
        assert np.all(base[:-1] != base[1:]) and np.all(base[:, :-1] != base[:, 1:])
        assert {63, 64, 65, 128, 255, 256} <= set(count.ravel().tolist())
    else:
        # the premise of this file's neighbours: the generator's matrix has one window nearly everywhere and short lists
        assert np.unique(base).size <= 3 and count.max() < M.FIRST


def test_packed_bytes_is_the_launchers_formula():
    count = np.array([[0, 1], [63, 64], [65, 300]])
    got = M.packed_bytes((None, count), 4097, 3)
    assert got == 6 * (8 * 3584 + 4) + 8 * (64 * 4 + 65 + 256) + 8 * (4097 + 3)


@pytest.mark.parametrize("n", (384, 1547, 3000))
def test_the_exact_integer_matrix_is_packable(n):
    """test_gpu_packed_edges.py runs exact_data's known answers on the image: every zero of int_block is an exception, and a
    (row, tile) may hold CAP of them."""
    _, count = M.headers(M.bits(E.int_block(0, n, n)), M.ncols_vec(n))
    assert 0 < count.max() <= M.CAP, count.max()
