"""The single solve's vector step past the grid-stride wrap.

vec_grid() caps the vector kernels at 256 workgroups of 256 threads, so from n = 65537 on a thread of update_xr / update_p /
update_fused (sliced vectors) and update_xr_full / update_p_full / update_full_fused (full-length vectors, gather-Ap exchange)
takes a second trip through its sweeps: the first index and the stride of csrc/lam_kernels.h's sweep_xr / sweep_p are used for the
first time.  n = 65537 wraps one element, n = 65536 + 257 a whole workgroup and one element (test_gpu_batch_recurrence.py part B
does the same for the batch).  tridiag(1,2,1) filled on the device -- no host matrix: 17 GB in fp32, 34 GB in fp64 -- with the
integer right-hand side of tests/exact_data.py; one context per (dtype, n, shard count), the forms switched with option
fuse_update between cg_init calls.

Forms: one shard fused / two kernels (sliced vectors of the whole length), two shards on device 0 over the gather-Ap exchange
fused / two kernels (full-length vectors wrap; the x window [row0, row0 + n_loc) of shard 1 contains the wrapped elements).
The sliced forms on SEVERAL shards (exchange 0 and 2) are not here: a slice wraps only from n > 131072 on two shards, and they run
the same sweep_xr / sweep_p / sweep_p_slice as the one-shard two-kernel form with another row0."""
import numpy as np
import pytest

import exact_data as E

pytestmark = pytest.mark.gpu

U_TV = {"F64": 2.0 ** -53, "F32": 2.0 ** -24}
SIZES = (65537, 65536 + 257)
CASES = [(d, n, P) for d in ("F32", "F64") for n in SIZES for P in (1, 2)]
CHUNKS = (1, 2, 9, 28)


@pytest.fixture(scope="module", params=CASES, ids=lambda p: f"{p[0]}-{p[1]}-{p[2]}shard")
def wrap(lam, request):
    dtype_name, n, P = request.param
    with lam.Solver(getattr(lam, dtype_name), device_ids=[0] * P) as s:
        s.generate_matrix(n)
        assert s.n == n > 256 * 256
        if P > 1:
            s.set_option("exchange", 1)
        b = E.int_vec(n, 12)
        s.set_rhs(b)
        yield dtype_name, n, P, s, b


def _bits(a):
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _form(s, P, fuse):
    s.set_option("fuse_update", fuse)
    s.cg_init()
    assert s.get_option("fuse_effective") == fuse
    if P > 1:
        assert s.get_option("exchange_effective") == 1


def test_wrap_first_step_exact(wrap):
    """solve(1, 1e-30) from x = 0 returns x1 = fl(alpha_TV b) bit for bit at every index, those past 65535 included, and rel_err
    within exact_data.rel_err_bound -- closed forms, independent of the code under test -- in the fused and the two-kernel form."""
    dtype_name, n, P, s, b = wrap
    vdt = s.vec_dtype
    Ab = E.tridiag_product(b)
    alpha, x1, bb, pAp, r1 = E.first_cg_step(b, Ab, vdt)
    x1 = x1 + vdt(0)
    re_host, bound = E.rel_err_bound(b, Ab, alpha, r1, bb, U_TV[dtype_name])
    for fuse in (1, 0):
        _form(s, P, fuse)
        s.solve(1, 1e-30)
        where = f"{dtype_name} n={n} shards={P} fuse_update={fuse}"
        assert s.get_option("fuse_effective") == fuse and s.stats["num_iters"] == 2, where
        x = s.solution()
        bad = np.flatnonzero(_bits(x) != _bits(x1))
        assert bad.size == 0, (f"{where}: x1 differs in {bad.size} entries, {np.count_nonzero(bad >= 65536)} of them past the wrap, first "
                               f"{bad[:6]}: {x[bad[:6]]} != {x1[bad[:6]]} (alpha {alpha!r})")
        assert abs(s.stats["rel_err"] - re_host) <= bound, (where, s.stats["rel_err"], re_host, bound)
    s.set_option("fuse_update", 1)


@pytest.mark.parametrize("wrap", [c for c in CASES if not (c[0] == "F64" and c[2] > 1)], indirect=True,
                         ids=lambda p: f"{p[0]}-{p[1]}-{p[2]}shard")
def test_wrap_fused_and_two_kernel_forms_agree_after_40_iterations(wrap):
    """40 iterations with rel_error = 0, cut into calls of 1, 2, 9 and 28: the fused and the two-kernel form give the same solution
    bits, rel_err and iteration count (fp32: one and two shards; fp64: one shard)."""
    dtype_name, n, P, s, b = wrap
    res = []
    for fuse in (1, 0):
        _form(s, P, fuse)
        for chunk in CHUNKS:
            s.cg_iterate(chunk, 0.0)
        res.append((s.solution(), s.stats["rel_err"], s.stats["num_iters"], s.stats["converged"]))
    s.set_option("fuse_update", 1)
    (x1, re1, it1, cv1), (x0, re0, it0, cv0) = res
    where = f"{dtype_name} n={n} shards={P}"
    assert np.isfinite(x1).all() and np.isfinite(re1) and re1 > 0.0 and it1 == it0 and not cv1 and not cv0, (where, re1, it1, it0, cv1, cv0)
    assert it1 == sum(CHUNKS) + 1, (where, it1)          # cap used up: the reference reports max_iters + 1
    bad = np.flatnonzero(_bits(x1) != _bits(x0))
    assert bad.size == 0, f"{where}: fused and two-kernel x differ in {bad.size} entries, {np.count_nonzero(bad >= 65536)} past the wrap, first {bad[:6]}"
    assert re1 == re0, (where, re1, re0)
