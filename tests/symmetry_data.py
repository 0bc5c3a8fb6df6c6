"""Inputs and host references of tests/test_gpu_symmetry_guard.py that need no GPU (checked on the CPU by tests/test_symmetry_data_cpu.py).

  * bf16_rne_bits: what bf16 storage must hold for an fp32 value -- round to nearest, ties to even, on the bit patterns;
  * BF16_PROBES: fp32 bit patterns at the places where a float -> bf16 conversion goes wrong (ties, overflow, subnormals, NaN);
  * planted_positions: where a single asymmetric entry is planted (tile edges, shard edges, the last shard's remainder rows,
    both ends of the tile numbering);
  * bf16_exact_delta: a power-of-two step that keeps a bf16 value exactly representable."""
import numpy as np

TILE = 32                      # asymmetry_kernel walks the upper triangle in 32 x 32 tiles


def bf16_rne_bits(u):
    """fp32 bit patterns (uint32 array) -> the fp32 bit patterns of the nearest bf16 value, ties to even.  NaN is not handled here
    (the carry can turn a NaN with a small payload into Inf, or one with a full payload into -0): callers compare NaN as NaN."""
    u = np.asarray(u, dtype=np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000) & 0xFFFFFFFF).astype(np.uint32)


def is_nan_bits(u):
    u = np.asarray(u, dtype=np.uint32)
    return ((u & 0x7F800000) == 0x7F800000) & ((u & 0x007FFFFF) != 0)


_POSITIVE_PROBES = (
    # exact bf16 numbers: 1, 3.140625, 0.099609375, the largest finite bf16, the smallest normal, a bf16 subnormal
    0x3F800000, 0x40490000, 0x3DCC0000, 0x7F7F0000, 0x00800000, 0x00400000,
    # ties: to even downwards, to even upwards; one fp32 ulp either side of each tie
    0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001,
    # a carry that runs through the whole mantissa into the exponent (1.99999988 -> 2)
    0x3FFFFFFF, 0x3FFF8000, 0x3FFF7FFF,
    # overflow: the largest finite fp32 and the tie below it round to +Inf; the largest fp32 that stays finite in bf16
    0x7F7FFFFF, 0x7F7F8000, 0x7F7F7FFF,
    # fp32 subnormals: the smallest, the largest (rounds to the smallest normal), and the neighbours of the smallest bf16
    # subnormal 0x00010000: half of it (a tie, to even = 0), just above half, just below it, just above it, the next tie (to even = 2 units)
    0x00000001, 0x007FFFFF, 0x00008000, 0x00008001, 0x00007FFF, 0x0000FFFF, 0x00010000, 0x00010001, 0x00018000,
    # zero, infinity
    0x00000000, 0x7F800000,
    # NaN: the default quiet NaN; a payload in the low 16 bits only (truncation alone would make it Inf); a full payload (the
    # rounding carry alone would make it -0)
    0x7FC00000, 0x7F800001, 0x7FFFFFFF,
)
BF16_PROBES = np.array(_POSITIVE_PROBES + tuple(u | 0x80000000 for u in _POSITIVE_PROBES), dtype=np.uint32)


def bf16_exact_delta(v):
    """A step d = -+2^k for the bf16 value v != 0 such that v + d is a bf16 value as well: half the power of two below |v|, towards
    zero.  |v| in [2^e, 2^(e+1)) is a multiple of 2^(e-7); v + d has magnitude in [2^(e-1), 1.5 * 2^e), where bf16's spacing is
    2^(e-8) or 2^(e-7): representable, and the sum is exact in fp32 and fp64."""
    v = float(v)
    assert v != 0.0 and np.isfinite(v)
    e = int(np.floor(np.log2(abs(v))))
    return -np.sign(v) * 2.0 ** (e - 1)


def planted_positions(n, P):
    """(i, j), i != j, each followed by (j, i): the matrix corners; (i, i + 1) across the first tile edge and across the edge of
    the last full tile; the first and last row of every shard (the reference's partition: n // P rows each, the remainder on the last
    shard) against the first and the last column; a row among the last shard's remainder rows (the second-to-last row when there is
    none).  At a large tile count also both ends and the middle of the tile numbering: the last tile of the first tile row, the
    diagonal tile of the last tile row that holds an off-diagonal pair, one tile in the middle of the triangle."""
    base = n // P
    pos = [(0, n - 1), (n - 1, n - 2), (TILE - 1, TILE)]
    k = n // TILE
    if TILE * k < n:
        pos.append((TILE * k - 1, TILE * k))
    else:
        pos.append((TILE * (k - 1) - 1, TILE * (k - 1)))
    for q in range(P):
        r0 = q * base
        r1 = n - 1 if q == P - 1 else r0 + base - 1
        for r in (r0, r1):
            for col in (0, n - 1):
                pos.append((r, col))
    pos.append((P * base if n % P else n - 2, n // 2))
    if n >= 60000:
        nt = (n + TILE - 1) // TILE
        last = nt - 1 if n - TILE * (nt - 1) >= 2 else nt - 2        # the last tile row with at least two rows of the matrix
        pos += [(17, n - 3), (TILE * last, TILE * last + 1), (TILE * (nt // 2) + 5, TILE * (3 * nt // 4) + 7)]
    out = []
    for i, j in pos:
        for p in ((i, j), (j, i)):
            if i != j and 0 <= min(i, j) and max(i, j) < n and p not in out:
                out.append(p)
    return out
