"""The host-side helpers of tests/test_gpu_symmetry_guard.py (tests/symmetry_data.py), checked without a GPU."""
import subprocess
import sys

import numpy as np
import pytest

import symmetry_data as S


def test_bf16_rne_helper_agrees_with_torch():
    """The bit-pattern formula the GPU test holds the device's float -> bf16 conversion to, against PyTorch's CPU conversion,
    on every probe value; NaN stays NaN (payload not compared)."""
    u = S.BF16_PROBES
    assert len(set(u.tolist())) == u.size
    # torch in a child process: imported into this one, next to the libraries the rest of the CPU suite loads, the interpreter
    # aborted at exit (free(): invalid pointer) after all tests had passed
    child = ("import sys, numpy as np, torch; u = np.array([int(a, 16) for a in sys.argv[1:]], dtype=np.uint32); "
             "print(' '.join('%08x' % b for b in torch.from_numpy(u.view(np.float32)).bfloat16().float().numpy().view(np.uint32)))")
    out = subprocess.run([sys.executable, "-c", child] + ["%08x" % a for a in u], capture_output=True, text=True, check=True).stdout
    got = np.array([int(a, 16) for a in out.split()], dtype=np.uint32)
    assert got.size == u.size
    nan = S.is_nan_bits(u)
    assert nan.sum() == 6 and np.all(S.is_nan_bits(got[nan]))
    want = S.bf16_rne_bits(u)
    assert np.array_equal(got[~nan], want[~nan]), [(hex(a), hex(b), hex(c)) for a, b, c in zip(u[~nan], got[~nan], want[~nan]) if b != c]
    assert np.all((want & 0xFFFF) == 0)
    # the probes do what their comments say
    rne = dict(zip(u.tolist(), want.tolist()))
    assert rne[0x3F808000] == 0x3F800000 and rne[0x3F818000] == 0x3F820000            # ties to even, both directions
    assert rne[0x3F807FFF] == 0x3F800000 and rne[0x3F808001] == 0x3F810000
    assert rne[0x7F7FFFFF] == 0x7F800000 and rne[0x7F7F8000] == 0x7F800000 and rne[0x7F7F7FFF] == 0x7F7F0000
    assert rne[0x00008000] == 0 and rne[0x00008001] == 0x00010000 and rne[0x00018000] == 0x00020000
    assert rne[0x80000000] == 0x80000000 and rne[0xFF800000] == 0xFF800000 and rne[0xFF7FFFFF] == 0xFF800000


def test_bf16_exact_delta_stays_on_the_bf16_grid():
    rng = np.random.default_rng(3)
    vals = rng.uniform(-2, 2, 2000) * 10.0 ** rng.integers(-6, 3, 2000)
    bits = S.bf16_rne_bits(vals.astype(np.float32).view(np.uint32))
    for v in bits.view(np.float32):
        d = S.bf16_exact_delta(v)
        w = np.float32(np.float64(v) + d)
        assert abs(d) == 2.0 ** round(np.log2(abs(d))) and np.float64(w) == np.float64(v) + d and w != v
        assert S.bf16_rne_bits(np.array([w]).view(np.uint32))[0] == np.array([w]).view(np.uint32)[0]


@pytest.mark.parametrize("n,P", [(1001, 1), (1001, 5), (4099, 1), (4099, 5), (65537, 1), (65537, 3), (1024, 4)])
def test_planted_positions_cover_what_they_claim(n, P):
    pos = S.planted_positions(n, P)
    assert len(set(pos)) == len(pos) and all(i != j and 0 <= i < n and 0 <= j < n for i, j in pos)
    assert all((j, i) in pos for i, j in pos)
    base = n // P
    for q in range(P):
        r0 = q * base
        r1 = n - 1 if q == P - 1 else r0 + base - 1
        for r in (r0, r1):
            assert (r == 0 or (r, 0) in pos) and (r == n - 1 or (r, n - 1) in pos)
    assert (31, 32) in pos and any(j == i + 1 and j % 32 == 0 and j + 32 > n - 32 for i, j in pos)
    if n % P:
        assert any(i >= P * base and abs(i - j) > 1 for i, j in pos)                   # a remainder row of the last shard
    if n >= 60000:
        nt = (n + 31) // 32
        tiles = {(min(i, j) // 32, max(i, j) // 32) for i, j in pos}
        assert (0, nt - 1) in tiles and (nt - 2, nt - 1) in tiles and (nt - 2, nt - 2) in tiles
        assert any(nt // 4 < a < 3 * nt // 4 and a < b < nt - 1 for a, b in tiles)
