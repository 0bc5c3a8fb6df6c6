"""Host model of the packed fp64 matrix (option "packed", csrc/lam_host_pack.h) and the inputs that make its kernels show their
mistakes.  numpy only, no GPU: tests/test_packed_model_cpu.py ties `headers` to lam_host_pack.h's pack_tile (g++, sanitizers);
tests/test_gpu_packed_edges.py then holds pack_rows_kernel and gemv_packed_kernel against it.

headers(rows_bits, ncols)       (base, count) of every (row, 4096-column tile): the window of 7 binades that holds the most normal
                                numbers, ties to the higher base; count = valid columns outside it.  `ncols` is the device's
                                ncols_vec (n rounded up to the 16-byte vector): the zero pad column of an odd n is a valid column
                                and an exception; nothing behind ncols is counted.
packed_bytes(headers, n, nrows) lam_launch.h's gemv_bytes_now on the image, as an exact integer.
ladder(n, seed)                 a finite matrix built from bit patterns whose rows and tiles each have a window of their own (below).
ladder_rows(k, n, seed)         k such rows, to be patched into a larger matrix with upload_rows.

The ladder.  gemv_packed_kernel keeps head[r] / shift[r] for each of its R = 2 rows and for each tile, and stages a (row, tile)'s
exception list in two parts (the first FIRST = 64 values blind, the rest once the header is there).  On a matrix with one window
throughout and a few dozen exceptions a tile, a kernel that took row 0's shift for both rows, tile 0's header for every tile or
started the second part one value late computes the same bits.  So row i is of class i mod 7 -- seven classes, an odd cycle, so that
the rows (2i, 2i + 1) of a workgroup meet in every combination of neighbouring classes -- and every class has its own base; tile t
of a row lies STEP * t binades away from tile 0 (towards the middle of the range):
    0 LOW    biased exponents 1..3 only: the bottom of the range (base 7: ties go up), no exceptions
    1 MID    base 900,  exceptions at random columns
    2 HIGH   biased exponents 2040..2046: the top of the range, no exceptions
    3 FULL   base 960, every one of the seven binades of the window, no exceptions
    4 MID    base 1020, exceptions at random columns
    5 GROUP  base 1080, exceptions concentrated in one wave group of the tile
    6 LANES  base 1140, exceptions in all 8 elements of a few lanes
The exception count of a (row, tile) of classes 1, 4, 5, 6 cycles through TARGETS = 0, 1, 63, 64, 65, 128, 255, 256 (as many as
the tile has room for; the pad column of an odd n is one of them).  The exceptions are +0, -0, denormals of either sign and
normal numbers 8 .. 270 binades above and 14 .. 270 binades below the window, at most a handful in any 7 binades, and one of them
always sits in the tile's last column: the last super-step of a ragged tile.
The premises are asserted here, with headers(), whenever a ladder is built: every count is the planted one and none exceeds CAP,
the rows of every pair differ in base in every tile, adjacent tiles of a row differ in base."""
import functools

import numpy as np

TILE, GROUP_BYTES, CAP, FIRST, WINDOW = 4096, 3584, 256, 64, 7       # lam_host_pack.h: kPackTile, kPackGroupBytes, kPackCap, ...
TARGETS = (0, 1, 63, 64, 65, 128, 255, 256)
NCLASS, STEP = 7, 9
CLASS_BASE = {1: 900, 3: 960, 4: 1020, 5: 1080, 6: 1140}
_U = np.uint64


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def ncols_vec(n):
    return (n + 1) // 2 * 2


def headers(rows_bits, ncols):
    """(base, count): two (rows, tiles) integer arrays."""
    rows_bits = np.asarray(rows_bits, dtype=np.uint64)
    k, n = rows_bits.shape
    assert n <= ncols
    ntiles = -(-ncols // TILE)
    exp = np.zeros((k, ncols), dtype=np.int64)             # the pad columns: +0.0, exponent field 0
    exp[:, :n] = ((rows_bits >> _U(52)) & _U(0x7FF)).astype(np.int64)
    base = np.empty((k, ntiles), dtype=np.int64)
    count = np.empty((k, ntiles), dtype=np.int64)
    for r0 in range(0, k, 512):
        r1 = min(k, r0 + 512)
        for t in range(ntiles):
            e = exp[r0:r1, t * TILE:min(ncols, (t + 1) * TILE)]
            normal = (e >= 1) & (e <= 2046)
            idx = (np.arange(r1 - r0)[:, None] * 2048 + e)[normal]
            hist = np.bincount(idx, minlength=(r1 - r0) * 2048).reshape(r1 - r0, 2048)
            win = np.cumsum(hist, axis=1)                  # win[b] becomes the elements with exponent b - 6 .. b (bin 0 is empty)
            win[:, WINDOW:] -= win[:, :-WINDOW].copy()
            key = win[:, 1:2047] * 2048 + np.arange(1, 2047)           # pack_window_key: more elements first, then the higher base
            b = key.argmax(axis=1) + 1
            base[r0:r1, t] = b
            count[r0:r1, t] = e.shape[1] - win[np.arange(r1 - r0), b]
    return base, count


def packed_bytes(hdrs, n, nrows):
    _, count = hdrs
    assert count.shape[0] == nrows
    units = nrows * count.shape[1]
    return int(units * (8 * GROUP_BYTES + 4) + 8 * int(np.maximum(np.minimum(count, CAP), FIRST).sum()) + 8 * (n + nrows))


def _make(sign, exp, mant):
    return (sign.astype(np.uint64) << _U(63)) | (exp.astype(np.uint64) << _U(52)) | mant.astype(np.uint64)


def _inside(rng, m, lo, hi, every=False):
    """m normal numbers with biased exponents in [lo, hi], random sign and mantissa; every: each binade in turn."""
    exp = lo + np.arange(m) % (hi - lo + 1) if every else rng.integers(lo, hi + 1, m)
    return _make(rng.integers(0, 2, m), exp, rng.integers(0, 1 << 52, m))


def _exceptions(rng, m, base):
    """m values outside the window below `base` (and outside every window near it, a handful in any 7 binades)."""
    k = np.arange(m)
    kind, far = k % 6, 8 * (k // 6 % 32)
    sign = np.where(kind < 4, kind % 2, rng.integers(0, 2, m))
    exp = np.where(kind < 4, 0, np.where(kind == 4, base + 8 + far, base - 14 - far))
    mant = np.where(kind < 2, 0, rng.integers(1, 1 << 52, m))          # kinds 2, 3: denormals, never zero
    return _make(sign, exp, mant)


def _order(rng, cls, row, cols):
    """The tile's columns [0, cols) in the order a row of class `cls` gives them to its exceptions; the last column always first."""
    j = rng.permutation(cols)
    if cls == 5:                                           # one wave group first (lam_host_pack.h pack_pos: w = (j >> 7) & 7)
        j = np.concatenate([j[(j >> 7) & 7 == row % 8], j[(j >> 7) & 7 != row % 8]])
    elif cls == 6:                                         # (wave group, lane) by (wave group, lane): all 8 elements of one, then the next
        j = np.arange(cols)
        owner = ((j >> 7) & 7) * 64 + ((j & 127) >> 1)
        j = j[np.argsort(rng.permutation(512)[owner], kind="stable")]
    return np.concatenate([[cols - 1], j[j != cols - 1]])


def _build(k, n, seed):
    """(bits (k, n), planted counts (k, tiles))."""
    rng = np.random.default_rng(seed)
    ncols = ncols_vec(n)
    ntiles = -(-ncols // TILE)
    out = np.empty((k, n), dtype=np.uint64)
    planted = np.zeros((k, ntiles), dtype=np.int64)
    nth = 0                                                # rows with planted exceptions so far: walks TARGETS
    for i in range(k):
        cls = i % NCLASS
        for t in range(ntiles):
            c0 = t * TILE
            cols = min(n, c0 + TILE) - c0                  # real columns of the tile
            pad = min(ncols, c0 + TILE) - c0 - cols        # 1 in the last tile of an odd n: a zero, an exception
            if cls == 0:
                v = _inside(rng, cols, 1 + 8 * t, 3 + 8 * t)
            elif cls == 2:
                v = _inside(rng, cols, 2040 - 8 * t, 2046 - 8 * t)
            else:
                base = CLASS_BASE[cls] + STEP * t
                v = _inside(rng, cols, base - 6, base, every=True)
                if cls != 3:
                    # at least a third of the tile (and one element) stays inside the window, so that it is the best one
                    m = max(0, min(TARGETS[(nth + t) % len(TARGETS)] - pad, cols - max(cols // 3, 1)))
                    v = v[rng.permutation(cols)]
                    v[_order(rng, cls, i, cols)[:m]] = _exceptions(rng, m, base)
                    planted[i, t] = m
            planted[i, t] += pad
            out[i, c0:c0 + cols] = v
        nth += cls in (1, 4, 5, 6)
    return out, planted


def _check_premises(rows, planted, n, whole):
    base, count = headers(rows, ncols_vec(n))
    assert np.array_equal(count, planted) and count.max() <= CAP, "ladder: a count is not the planted one"
    assert np.all(base[:-1] != base[1:]), "ladder: two neighbouring rows share a base"          # every pair, whichever row it starts on
    assert np.all(base[:, :-1] != base[:, 1:]), "ladder: adjacent tiles of a row share a base"
    assert not np.any((rows >> _U(52)) & _U(0x7FF) == _U(0x7FF)), "ladder: Inf or NaN"
    if whole and rows.shape[0] >= 8 * NCLASS and n >= 384:
        # an odd n of one tile has its pad column in that tile: no empty list there
        want = set(TARGETS) if n % 2 == 0 or count.shape[1] > 1 else {max(v, 1) for v in TARGETS}
        assert want <= set(count[:, 0].tolist()), "ladder: a list length of TARGETS is missing from the first tile"
        assert base.min() == 7 and base.max() == 2046


@functools.lru_cache(maxsize=None)
def _ladder_cached(k, n, seed, whole):
    rows, planted = _build(k, n, seed)
    _check_premises(rows, planted, n, whole)
    a = rows.view(np.float64)
    a.flags.writeable = False
    return a


def ladder(n, seed=1):
    """The n x n ladder as float64 (read-only, shared between callers)."""
    return _ladder_cached(n, n, seed, True)


def ladder_rows(k, n, seed=1):
    """k rows of an n-column ladder as float64 (read-only)."""
    return _ladder_cached(k, n, seed, False)
