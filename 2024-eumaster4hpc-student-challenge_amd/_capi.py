"""ctypes binding of include/lam_hip.h.  Mirrors the reference's solver interface
(LAM::ConjugateGradient<T>: solve / load_matrix_from_file / load_rhs_from_file /
save_result_to_file, plus generate_matrix / generate_rhs of the distributed classes --
/root/reference/challenge/main/LAM/src/ConjugateGradient.hpp:23-27,
LAM/src/CPU/ConjugateGradient_CPU_MPI_OMP.hpp:31-35) on top of the C ABI."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# LAM_HIP_LIB: load another build of the same ABI instead (the tuning build liblam_hip_tuning.so, tools/gemv_probe.py)
_LIB = os.environ.get("LAM_HIP_LIB") or os.path.join(_HERE, "liblam_hip.so")
TUNING_LIB = os.path.join(_HERE, "liblam_hip_tuning.so")

F64, F32, BF16 = 0, 1, 2
ABI_VERSION = 4     # include/lam_hip.h LAM_HIP_ABI_VERSION
MAX_RHS = 8         # include/lam_hip.h LAM_HIP_MAX_RHS
MAX_SHIFTS = 64     # include/lam_hip.h LAM_HIP_MAX_SHIFTS
MAX_LANCZOS = 256   # include/lam_hip.h LAM_HIP_MAX_LANCZOS
MAX_DEFLATION = 32  # include/lam_hip.h LAM_HIP_MAX_DEFLATION
MAX_PROBES = 64     # include/lam_hip.h LAM_HIP_MAX_PROBES
QUAD_FN = {"log": 0, "inv": 1, "pow": 2}   # include/lam_hip.h LAM_HIP_QUAD_*
EIG_WHICH = {"smallest": 0, "largest": 1, "both": 2}   # include/lam_hip.h LAM_HIP_EIG_*
PC_NONE, PC_JACOBI = 0, 1   # include/lam_hip.h LAM_HIP_PC_*: preconditioner of Solver.solve_many / solve_all
_VEC_DTYPE = {F64: np.float64, F32: np.float32, BF16: np.float32}
_HOST_MAT_DTYPE = {F64: np.float64, F32: np.float32, BF16: np.float32}


class LamHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"lam_hip error {code}: {msg}")
        self.code = code


class Stats(C.Structure):
    _fields_ = [("num_iters", C.c_int32), ("converged", C.c_int32), ("rel_err", C.c_double),
                ("t_gemv", C.c_double), ("t_iter", C.c_double), ("t_total", C.c_double),
                ("t_comm_init", C.c_double), ("gemv_bytes", C.c_double), ("t_exchange", C.c_double)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def rhs_groups(nrows, max_rhs=MAX_RHS):
    """How Solver.solve_all cuts `nrows` right-hand sides into batches of at most `max_rhs`: (first, count) pairs, full batches
    first and the remainder last (19 -> 8 + 8 + 3)."""
    if nrows < 0 or max_rhs < 1:
        raise ValueError("rhs_groups: nrows >= 0 and max_rhs >= 1")
    return [(f, min(max_rhs, nrows - f)) for f in range(0, nrows, max_rhs)]


def lib_path():
    return _LIB


def build(force=False):
    """Compile liblam_hip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    srcs = _source_files()
    stale = (not os.path.exists(_LIB)) or any(os.path.getmtime(s) > os.path.getmtime(_LIB) for s in srcs)
    if force or stale:
        r = subprocess.run(["make", "-C", _HERE, "all"], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("building liblam_hip.so failed:\n" + r.stdout + r.stderr)
    return _LIB


_lib = None


def _source_files():
    """csrc/lam_hip.hip, every csrc/*.h it includes (sorted, as the Makefile's $(sort $(wildcard ...))), include/lam_hip.h."""
    import glob
    return ([os.path.join(_HERE, "csrc", "lam_hip.hip")] + sorted(glob.glob(os.path.join(_HERE, "csrc", "*.h")))
            + [os.path.join(os.path.dirname(_HERE), "include", "lam_hip.h")])


def source_id():
    """sha256 prefix of the sources the library is built from (same recipe as the Makefile's SRC_ID), or None when the
    sources are not next to the package."""
    import hashlib
    h = hashlib.sha256()
    try:
        for f in _source_files():
            with open(f, "rb") as fh:
                h.update(fh.read())
    except OSError:
        return None
    return h.hexdigest()[:16]


def lib():
    """Load the HIP library.  Fails loudly if it is missing: there is no fallback path."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB):
            raise ImportError(f"{_LIB} is not built (run `make -C {_HERE}` or __graft_entry__.build()); "
                              "the product has no CPU fallback")
        L = C.CDLL(_LIB, mode=C.RTLD_GLOBAL)
        vp, u64, i32 = C.c_void_p, C.c_uint64, C.c_int
        sig = {
            "lam_hip_abi_version": ([], i32),
            "lam_hip_build_id": ([], C.c_char_p),
            "lam_hip_device_count": ([C.POINTER(i32)], i32),
            "lam_hip_create": ([C.POINTER(vp), i32, i32, C.POINTER(i32)], i32),
            "lam_hip_get_unique_id": ([vp], i32),
            "lam_hip_create_rank": ([C.POINTER(vp), i32, i32, i32, i32, vp], i32),
            "lam_hip_destroy": ([vp], None),
            "lam_hip_last_error": ([vp], C.c_char_p),
            "lam_hip_set_problem": ([vp, u64], i32),
            "lam_hip_partition": ([u64, i32, i32, C.POINTER(u64), C.POINTER(u64)], i32),
            "lam_hip_n": ([vp, C.POINTER(u64)], i32),
            "lam_hip_num_shards": ([vp, C.POINTER(i32), C.POINTER(i32)], i32),
            "lam_hip_get_partition": ([vp, i32, C.POINTER(u64), C.POINTER(u64)], i32),
            "lam_hip_upload_rows": ([vp, u64, u64, vp], i32),
            "lam_hip_download_rows": ([vp, u64, u64, vp], i32),
            "lam_hip_generate_tridiag": ([vp], i32),
            "lam_hip_generate_random_spd": ([vp, u64, C.c_double], i32),
            "lam_hip_generate_spectrum_spd": ([vp, C.POINTER(C.c_double), C.POINTER(C.c_double), i32], i32),
            "lam_hip_set_rhs": ([vp, vp], i32),
            "lam_hip_get_rhs": ([vp, vp], i32),
            "lam_hip_generate_rhs": ([vp, C.c_double], i32),
            "lam_hip_generate_random_rhs": ([vp, u64], i32),
            "lam_hip_solve": ([vp, i32, C.c_double, C.POINTER(Stats)], i32),
            "lam_hip_cg_init": ([vp], i32),
            "lam_hip_cg_iterate": ([vp, i32, C.c_double, C.POINTER(Stats)], i32),
            "lam_hip_get_solution": ([vp, vp], i32),
            "lam_hip_true_residual": ([vp, C.POINTER(C.c_double)], i32),
            "lam_hip_gemv": ([vp, vp, vp], i32),
            "lam_hip_gemv_only": ([vp, i32, C.POINTER(C.c_double)], i32),
            "lam_hip_set_rhs_many": ([vp, i32, vp], i32),
            "lam_hip_solve_many": ([vp, i32, C.c_double, C.POINTER(Stats), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                    C.POINTER(C.c_double)], i32),
            "lam_hip_solve_many_pc": ([vp, i32, i32, C.c_double, C.POINTER(Stats), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                       C.POINTER(C.c_double)], i32),
            "lam_hip_solve_many_x0": ([vp, i32, vp, i32, C.c_double, C.POINTER(Stats), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                       C.POINTER(C.c_double)], i32),
            "lam_hip_true_residual_many": ([vp, i32, C.POINTER(C.c_double)], i32),
            "lam_hip_set_shifts_many": ([vp, i32, C.POINTER(C.c_double)], i32),
            "lam_hip_solve_many_minres": ([vp, C.POINTER(C.c_double), i32, C.c_double, C.POINTER(Stats), C.POINTER(C.c_int32),
                                           C.POINTER(C.c_int32), C.POINTER(C.c_double)], i32),
            "lam_hip_get_diagonal": ([vp, vp], i32),
            "lam_hip_get_solution_many": ([vp, i32, vp], i32),
            "lam_hip_gemv_many": ([vp, i32, vp, vp], i32),
            "lam_hip_gemv_many_only": ([vp, i32, i32, C.POINTER(C.c_double)], i32),
            "lam_hip_solve_mshift": ([vp, vp, i32, C.POINTER(C.c_double), i32, C.c_double, C.POINTER(Stats), C.POINTER(C.c_int32),
                                      C.POINTER(C.c_int32), C.POINTER(C.c_double)], i32),
            "lam_hip_get_solution_mshift": ([vp, i32, vp], i32),
            "lam_hip_true_residual_mshift": ([vp, i32, C.POINTER(C.c_double)], i32),
            "lam_hip_eigs": ([vp, i32, i32, i32, C.c_double, i32, vp, u64, C.POINTER(Stats), C.POINTER(C.c_int32),
                              C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32)], i32),
            "lam_hip_get_lanczos": ([vp, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_double)], i32),
            "lam_hip_get_eigenvectors": ([vp, i32, vp], i32),
            "lam_hip_eig_residuals": ([vp, i32, C.POINTER(C.c_double)], i32),
            "lam_hip_project_out": ([vp, u64, i32, vp, vp, C.POINTER(C.c_double)], i32),
            "lam_hip_tridiag_eigen": ([i32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                       C.POINTER(C.c_double), C.POINTER(C.c_double)], i32),
            "lam_hip_lanczos_many": ([vp, i32, vp, u64, i32, C.POINTER(Stats), C.POINTER(C.c_int32), C.POINTER(C.c_double),
                                      C.POINTER(C.c_double), C.POINTER(C.c_double)], i32),
            "lam_hip_get_lanczos_many": ([vp, i32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double),
                                          C.POINTER(C.c_double), C.POINTER(C.c_double)], i32),
            "lam_hip_trace_quadrature": ([vp, i32, C.c_double, i32, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                          C.POINTER(C.c_double), C.POINTER(C.c_double)], i32),
            "lam_hip_tridiag_quadrature": ([i32, C.POINTER(C.c_double), C.POINTER(C.c_double), i32, C.c_double, i32,
                                            C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(i32)], i32),
            "lam_hip_set_deflation": ([vp, i32, vp], i32),
            "lam_hip_set_deflation_eigs": ([vp, i32], i32),
            "lam_hip_solve_many_deflated": ([vp, i32, C.c_double, C.POINTER(Stats), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                             C.POINTER(C.c_double)], i32),
            "lam_hip_deflate_many": ([vp, u64, i32, i32, vp, vp, C.POINTER(C.c_double), vp, C.POINTER(C.c_double)], i32),
            "lam_hip_chol_inverse": ([i32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(i32)], i32),
            "lam_hip_solve_block": ([vp, i32, C.c_double, C.POINTER(Stats), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                     C.POINTER(C.c_double), C.POINTER(C.c_int32)], i32),
            "lam_hip_block_factor": ([i32, i32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                      C.POINTER(C.c_double), C.POINTER(i32)], i32),
            "lam_hip_check_symmetry": ([vp, C.POINTER(C.c_double)], i32),
            "lam_hip_debug_symv_plan": ([u64, i32, i32, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)], i32),
            "lam_hip_dot": ([vp, vp, vp, u64, C.POINTER(C.c_double)], i32),
            "lam_hip_axpby": ([vp, C.c_double, vp, C.c_double, vp, u64], i32),
            "lam_hip_all_ok": ([vp, i32, C.POINTER(i32)], i32),
            "lam_hip_rccl_version": ([C.POINTER(i32)], i32),
            "lam_hip_gemv_kernel_name": ([vp, C.c_char_p, C.c_size_t], i32),
            "lam_hip_set_option": ([vp, C.c_char_p, C.c_int64], i32),
            "lam_hip_get_option": ([vp, C.c_char_p, C.POINTER(C.c_int64)], i32),
        }
        for name, (args, res) in sig.items():
            fn = getattr(L, name)      # AttributeError if the library does not export it
            fn.argtypes, fn.restype = args, res
        L._lam_symbols = tuple(sig)
        if L.lam_hip_abi_version() != ABI_VERSION:      # the Stats struct above belongs to one ABI version
            raise ImportError(f"{_LIB} has ABI {L.lam_hip_abi_version()}, this binding was written for ABI {ABI_VERSION}")
        built, want = L.lam_hip_build_id().decode(), source_id()
        if want is not None and built != want and not os.environ.get("LAM_HIP_ALLOW_STALE"):
            raise ImportError(f"{_LIB} was built from other sources (library {built}, sources {want}): rebuild it "
                              f"(`make -C {_HERE} all tuning` or __graft_entry__.build())")
        _lib = L
    return _lib


def device_count():
    n = C.c_int(0)
    rc = lib().lam_hip_device_count(C.byref(n))
    if rc != 0:
        raise LamHipError(rc, (lib().lam_hip_last_error(None) or b"").decode())
    return n.value


def get_unique_id():
    buf = C.create_string_buffer(128)
    rc = lib().lam_hip_get_unique_id(buf)
    if rc != 0:
        raise LamHipError(rc, (lib().lam_hip_last_error(None) or b"").decode())
    return buf.raw


def rccl_version():
    v = C.c_int(0)
    rc = lib().lam_hip_rccl_version(C.byref(v))
    if rc != 0:
        raise LamHipError(rc, (lib().lam_hip_last_error(None) or b"").decode())
    return v.value


def symv_plan_check(n, shards, dtype=0):
    """Host-only check of the symmetric product's task plan (lam_hip_debug_symv_plan): (bad_pairs, bad_interior, tasks)."""
    bp, bi, nt = C.c_uint64(), C.c_uint64(), C.c_uint64()
    rc = lib().lam_hip_debug_symv_plan(n, shards, dtype, C.byref(bp), C.byref(bi), C.byref(nt))
    if rc != 0:
        raise LamHipError(rc, "lam_hip_debug_symv_plan")
    return bp.value, bi.value, nt.value


def tridiag_eigen(alpha, beta, vectors=False):
    """Eigenvalues (ascending) of the symmetric tridiagonal matrix with diagonal alpha[k] and off-diagonal beta[:k-1], and the
    bottom components of its eigenvectors (lam_hip_tridiag_eigen: host only, no GPU, the routine Solver.eigs calls).  Returns
    (theta, last_row), or with vectors=True (theta, last_row, S) with S[:, i] eigenvector i."""
    a = np.ascontiguousarray(alpha, dtype=np.float64).reshape(-1)
    k = a.size
    b = np.zeros(max(k, 1), np.float64)
    bb = np.ascontiguousarray(beta, dtype=np.float64).reshape(-1)
    if bb.size < k - 1:
        raise ValueError("tridiag_eigen: beta needs at least len(alpha) - 1 entries")
    b[:max(k - 1, 0)] = bb[:max(k - 1, 0)]
    theta, row = np.zeros(max(k, 1), np.float64), np.zeros(max(k, 1), np.float64)
    S = np.zeros((max(k, 1), max(k, 1)), np.float64) if vectors else None
    dp = C.POINTER(C.c_double)
    rc = lib().lam_hip_tridiag_eigen(k, a.ctypes.data_as(dp), b.ctypes.data_as(dp), theta.ctypes.data_as(dp), row.ctypes.data_as(dp),
                                     S.ctypes.data_as(dp) if vectors else None)
    if rc != 0:
        raise LamHipError(rc, "lam_hip_tridiag_eigen: k outside 1..MAX_LANCZOS or a non-finite entry")
    return (theta[:k], row[:k], S.T.copy()) if vectors else (theta[:k], row[:k])


def tridiag_quadrature(alpha, beta, fn, shifts=None, param=0):
    """e_1^T f(T + s I) e_1 for every s of `shifts` (None: the one shift 0), T the symmetric tridiagonal matrix with diagonal alpha[k]
    and off-diagonal beta[:k-1] (lam_hip_tridiag_quadrature: host only, no GPU, the routine Solver.trace_quadrature calls).  fn: "log",
    "inv", "pow" (or the LAM_HIP_QUAD_* value); param: the exponent of "pow".  A refusal raises LamHipError; where a node was refused
    its `bad` attribute is (shift, node)."""
    f = QUAD_FN[fn] if isinstance(fn, str) else int(fn)
    a = np.ascontiguousarray(alpha, dtype=np.float64).reshape(-1)
    k = a.size
    b = np.zeros(max(k, 1), np.float64)
    bb = np.ascontiguousarray(beta, dtype=np.float64).reshape(-1)
    if bb.size < k - 1:
        raise ValueError("tridiag_quadrature: beta needs at least len(alpha) - 1 entries")
    b[:max(k - 1, 0)] = bb[:max(k - 1, 0)]
    dp = C.POINTER(C.c_double)
    sg = None if shifts is None else np.ascontiguousarray(shifts, dtype=np.float64).reshape(-1)
    ns = 1 if sg is None else sg.size
    out = np.zeros(max(ns, 1), np.float64)
    bad = (C.c_int * 2)(-1, -1)
    rc = lib().lam_hip_tridiag_quadrature(k, a.ctypes.data_as(dp), b.ctypes.data_as(dp), f, float(param), ns,
                                          None if sg is None else sg.ctypes.data_as(dp), out.ctypes.data_as(dp), bad)
    if rc != 0:
        e = LamHipError(rc, (lib().lam_hip_last_error(None) or b"").decode())
        e.bad = (bad[0], bad[1])
        raise e
    return out[:ns]


def chol_inverse(G):
    """The inverse of the symmetric positive definite matrix G (m x m, m <= MAX_DEFLATION) by the fp64 Cholesky routine the deflation
    setters call (lam_hip_chol_inverse: host only, no GPU).  Only the lower triangle is read.  A refused pivot raises LamHipError
    whose message names the column (also in .bad_col; -1: m out of range)."""
    G = np.ascontiguousarray(G, dtype=np.float64)
    assert G.ndim == 2 and G.shape[0] == G.shape[1], "G is square"
    m = G.shape[0]
    Ginv = np.zeros((max(m, 1), max(m, 1)), np.float64)
    bad = C.c_int(-1)
    dp = C.POINTER(C.c_double)
    rc = lib().lam_hip_chol_inverse(m, G.ctypes.data_as(dp), Ginv.ctypes.data_as(dp), C.byref(bad))
    if rc != 0:
        e = LamHipError(rc, f"lam_hip_chol_inverse: m = {m} outside 1..{MAX_DEFLATION}" if bad.value < 0 else
                        f"lam_hip_chol_inverse: the pivot of column {bad.value} is not finite or not above rounding level")
        e.bad_col = bad.value
        raise e
    return Ginv[:m, :m]


def block_factor(G, dtype=F64):
    """The s x s routines of Solver.solve_block on the symmetric G (s <= MAX_RHS; only the upper triangle is read), under the pivot
    rule of `dtype` (lam_hip_block_factor: host only, no GPU).  Returns (Ginv, S, Sinv): G^-1 by G = L D L^T, the upper factor of
    G = S^T S and its inverse.  A failed pivot raises LamHipError whose message names the column (also in .bad_col; -1: s or dtype
    out of range)."""
    G = np.ascontiguousarray(G, dtype=np.float64)
    assert G.ndim == 2 and G.shape[0] == G.shape[1], "G is square"
    s = G.shape[0]
    out = [np.zeros((max(s, 1), max(s, 1)), np.float64) for _ in range(3)]
    bad = C.c_int(-1)
    dp = C.POINTER(C.c_double)
    rc = lib().lam_hip_block_factor(s, dtype, G.ctypes.data_as(dp), *[o.ctypes.data_as(dp) for o in out], C.byref(bad))
    if rc != 0:
        e = LamHipError(rc, f"lam_hip_block_factor: s = {s} outside 1..{MAX_RHS} or dtype {dtype} not F64 / F32" if bad.value < 0 else
                        f"lam_hip_block_factor: the pivot of column {bad.value} is not finite or not above rounding level")
        e.bad_col = bad.value
        raise e
    return tuple(o[:s, :s] for o in out)


def partition(n, num_shards, shard):
    """Rows (row0, nrows) of shard `shard` of `num_shards` -- the reference's block-row rule."""
    r0, nr = C.c_uint64(), C.c_uint64()
    rc = lib().lam_hip_partition(n, num_shards, shard, C.byref(r0), C.byref(nr))
    if rc != 0:
        raise LamHipError(rc, "bad partition arguments")
    return r0.value, nr.value


def _read_bin(path, dtype):
    """(rows, cols) of a matrix / vector file.  Same rule as LAM::parse_bin_header (the C++ loaders): the
    reference's writers store an `int` with sizeof(size_t) -- cols in ConjugateGradient_CPU_OMP.hpp:206-210,
    both words in ConjugateGradient_MultiGPUS_CUDA_NCCL.cu:754-757 -- leaving garbage in the upper 32 bits, so
    take the words as they are if the file is long enough for them, else their low halves if those fit."""
    size = os.path.getsize(path)
    esz = np.dtype(dtype).itemsize
    with open(path, "rb") as f:
        hdr = np.frombuffer(f.read(16), dtype=np.uint64)
    if hdr.size != 2:
        raise IOError("short header")
    for rows, cols in ((int(hdr[0]), int(hdr[1])), (int(hdr[0]) & 0xFFFFFFFF, int(hdr[1]) & 0xFFFFFFFF)):
        if rows > 0 and cols > 0 and rows * cols * esz <= size - 16:
            return rows, cols
    raise IOError("file is shorter than its header says")


class Solver:
    """Python face of the reference's solver classes.

    Solver(dtype, n_shards=1, device_ids=None)            one process, one or more shards
    Solver(dtype, rank=r, nranks=P, device_id=d, unique_id=..)  one process per GPU (RCCL)
    """

    def __init__(self, dtype=F64, n_shards=1, device_ids=None, rank=None, nranks=None, device_id=0,
                 unique_id=None):
        self._L = lib()
        self._h = C.c_void_p()
        self.dtype = dtype
        self.rank = 0 if rank is None else rank
        if rank is None:
            ids = None
            if device_ids is not None:
                ids = (C.c_int * len(device_ids))(*device_ids)
                n_shards = len(device_ids)
            rc = self._L.lam_hip_create(C.byref(self._h), dtype, n_shards, ids)
        else:
            rc = self._L.lam_hip_create_rank(C.byref(self._h), dtype, device_id, rank, nranks, unique_id)
        if rc != 0:
            raise LamHipError(rc, (self._L.lam_hip_last_error(None) or b"").decode())
        self.vec_dtype = _VEC_DTYPE[dtype]
        self.mat_host_dtype = _HOST_MAT_DTYPE[dtype]

    # -- plumbing -------------------------------------------------------------------------------
    def _chk(self, rc):
        if rc != 0:
            raise LamHipError(rc, (self._L.lam_hip_last_error(self._h) or b"").decode())

    def close(self):
        if self._h:
            self._L.lam_hip_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- problem --------------------------------------------------------------------------------
    def set_problem(self, n):
        self._chk(self._L.lam_hip_set_problem(self._h, n))
        self.n = n

    def num_shards(self):
        t, l = C.c_int(), C.c_int()
        self._chk(self._L.lam_hip_num_shards(self._h, C.byref(t), C.byref(l)))
        return t.value, l.value

    def partition(self, shard):
        r0, nr = C.c_uint64(), C.c_uint64()
        self._chk(self._L.lam_hip_get_partition(self._h, shard, C.byref(r0), C.byref(nr)))
        return r0.value, nr.value

    def upload_rows(self, row0, rows):
        rows = np.ascontiguousarray(rows, dtype=self.mat_host_dtype)
        self._chk(self._L.lam_hip_upload_rows(self._h, row0, rows.shape[0], rows.ctypes.data_as(C.c_void_p)))

    def download_rows(self, row0, nrows):
        out = np.empty((nrows, self.n), dtype=self.mat_host_dtype)
        self._chk(self._L.lam_hip_download_rows(self._h, row0, nrows, out.ctypes.data_as(C.c_void_p)))
        return out

    def set_matrix(self, A):
        """Upload a full host matrix (single-process contexts)."""
        A = np.ascontiguousarray(A, dtype=self.mat_host_dtype)
        assert A.ndim == 2 and A.shape[0] == A.shape[1]
        self.set_problem(A.shape[0])
        self.upload_rows(0, A)

    def generate_matrix(self, rows, cols=None):
        """generate_matrix(rows, cols): dense tridiag(1,2,1) (CPU_MPI_OMP.hpp:167-256)."""
        if cols is not None and cols != rows:
            raise ValueError("Matrix has to be square")
        self.set_problem(rows)
        self._chk(self._L.lam_hip_generate_tridiag(self._h))
        return True

    def generate_random_spd(self, n, seed, cond, keep_problem=False):
        """keep_problem: a context that already holds a problem of this size keeps its allocations (no lam_hip_set_problem: its
        hipFree waits for the whole device, which deadlocks rank contexts that are THREADS of one process -- the test harness's
        shape -- as soon as another rank has a collective in flight that waits for this one)."""
        if not (keep_problem and getattr(self, "n", None) == n):
            self.set_problem(n)
        self._chk(self._L.lam_hip_generate_random_spd(self._h, seed, cond))

    def generate_spectrum_spd(self, eig, reflectors):
        """A = H_k..H_1 diag(eig) H_1..H_k (the reference generator's law, random_spd_system.cpp:66-97, with Householder
        reflectors for Q); `reflectors`: k x N array (k may be 0: the diagonal matrix itself)."""
        eig = np.ascontiguousarray(eig, dtype=np.float64).reshape(-1)
        V = np.ascontiguousarray(reflectors, dtype=np.float64).reshape(-1, eig.size) if np.size(reflectors) else np.zeros((0, eig.size))
        self.set_problem(eig.size)
        dp = C.POINTER(C.c_double)
        self._chk(self._L.lam_hip_generate_spectrum_spd(self._h, eig.ctypes.data_as(dp), V.ctypes.data_as(dp), V.shape[0]))

    def generate_rhs(self, value=1.0):
        self._chk(self._L.lam_hip_generate_rhs(self._h, value))
        return True

    def generate_random_rhs(self, seed):
        self._chk(self._L.lam_hip_generate_random_rhs(self._h, seed))

    def set_rhs(self, b):
        b = np.ascontiguousarray(b, dtype=self.vec_dtype).reshape(-1)
        assert b.size == self.n
        self._chk(self._L.lam_hip_set_rhs(self._h, b.ctypes.data_as(C.c_void_p)))

    def rhs(self):
        b = np.empty(self.n, dtype=self.vec_dtype)
        self._chk(self._L.lam_hip_get_rhs(self._h, b.ctypes.data_as(C.c_void_p)))
        return b

    # -- file mode (format: random_spd_system.cpp:105-121) ------------------------------------------
    def load_matrix_from_file(self, filename, chunk_bytes=256 << 20):
        try:
            rows, cols = _read_bin(filename, np.float64 if self.dtype == F64 else np.float32)
        except OSError:
            return False
        if rows != cols:
            return False            # "Matrix has to be square" (CPU_OMP.hpp:151-155)
        self.set_problem(rows)
        total, local = self.num_shards()
        es = 8 if self.dtype == F64 else 4
        file_dtype = np.float64 if self.dtype == F64 else np.float32
        mm = np.memmap(filename, dtype=file_dtype, mode="r", offset=16, shape=(rows, cols))
        owned = [self.partition(q) for q in range(total)] if local == total else [self.partition(self.rank)]
        step = max(1, chunk_bytes // (cols * es))
        for r0, nr in owned:
            for s in range(r0, r0 + nr, step):
                e = min(s + step, r0 + nr)
                self.upload_rows(s, np.asarray(mm[s:e]))
        return True

    def load_rhs_from_file(self, filename):
        try:
            rows, cols = _read_bin(filename, np.float64 if self.dtype == F64 else np.float32)
        except OSError:
            return False
        if cols != 1 or rows != self.n:
            return False            # CPU_MPI_OMP.hpp:278-287
        file_dtype = np.float64 if self.dtype == F64 else np.float32
        b = np.fromfile(filename, dtype=file_dtype, offset=16, count=rows)
        self.set_rhs(b)
        return True

    def save_result_to_file(self, filename):
        x = self.solution()
        try:
            with open(filename, "wb") as f:
                f.write(np.array([x.size, 1], dtype=np.uint64).tobytes())   # clean cols word
                f.write(x.tobytes())
        except OSError:
            return False
        return True

    # -- hot path -------------------------------------------------------------------------------
    def solve(self, max_iters, rel_error):
        st = Stats()
        self._chk(self._L.lam_hip_solve(self._h, max_iters, rel_error, C.byref(st)))
        self.stats = st.asdict()
        return bool(st.converged)

    def cg_init(self):
        self._chk(self._L.lam_hip_cg_init(self._h))

    def cg_iterate(self, iters, rel_error=0.0):
        st = Stats()
        self._chk(self._L.lam_hip_cg_iterate(self._h, iters, rel_error, C.byref(st)))
        self.stats = st.asdict()
        return self.stats

    def solution(self):
        x = np.empty(self.n, dtype=self.vec_dtype)
        self._chk(self._L.lam_hip_get_solution(self._h, x.ctypes.data_as(C.c_void_p)))
        return x

    def true_residual(self):
        v = C.c_double()
        self._chk(self._L.lam_hip_true_residual(self._h, C.byref(v)))
        return v.value

    # -- several right-hand sides on one matrix (one shard, F64 / F32) ----------------------------
    def _as_columns(self, B):
        B = np.ascontiguousarray(B, dtype=self.vec_dtype)
        if B.ndim == 1:
            B = B.reshape(1, -1)
        assert B.ndim == 2 and B.shape[1] == self.n, "right-hand sides are (nrhs, N)"
        return B

    def set_rhs_many(self, B):
        """B: (nrhs, N), 1 <= nrhs <= MAX_RHS; row j is right-hand side j."""
        B = self._as_columns(B)
        self._chk(self._L.lam_hip_set_rhs_many(self._h, B.shape[0], B.ctypes.data_as(C.c_void_p)))
        self.nrhs = B.shape[0]

    def set_shifts(self, sigma):
        """Column j of the following solve_many / true_residuals is (A + sigma[j] I) x_j = b_j (lam_hip_set_shifts_many): one finite
        shift >= 0 per right-hand side of set_rhs_many, which clears them; None clears them too.  gemv_many stays A's product."""
        k = getattr(self, "nrhs", 0)
        if sigma is None:
            self._chk(self._L.lam_hip_set_shifts_many(self._h, k, None))
            return
        sg = np.ascontiguousarray(np.atleast_1d(sigma), dtype=np.float64)
        assert sg.ndim == 1, "shifts are a list of nrhs numbers"
        self._chk(self._L.lam_hip_set_shifts_many(self._h, sg.size, sg.ctypes.data_as(C.POINTER(C.c_double))))

    def solve_shifted(self, b, shifts, max_iters, rel_error, precond=PC_NONE, x0=None):
        """(A + shifts[j] I) x_j = b for 1..MAX_RHS shifts in one batch: b replicated, set_shifts, solve_many.  Returns what
        solve_many returns; solutions() and true_residuals() follow as usual."""
        sg = np.atleast_1d(np.asarray(shifts, dtype=np.float64))
        b = np.ascontiguousarray(b, dtype=self.vec_dtype).reshape(1, -1)
        self.set_rhs_many(np.repeat(b, sg.size, axis=0))
        self.set_shifts(sg)
        return self.solve_many(max_iters, rel_error, precond, x0)

    def solve_multishift(self, b, shifts, max_iters, rel_error):
        """(A + shifts[j] I) x_j = b for 1..MAX_SHIFTS shifts by multi-shift CG (lam_hip_solve_mshift): the single-column product of
        the smallest shift's system per iteration, whatever the number of shifts.  Returns the per-shift `converged` array;
        self.num_iters_shift / converged_shift / rel_err_shift hold the per-shift results and self.stats the call's.  The batch
        state afterwards is the seed's: one right-hand side b under the smallest shift (solutions(), true_residuals())."""
        sg = np.ascontiguousarray(np.atleast_1d(shifts), dtype=np.float64)
        assert sg.ndim == 1, "shifts are a list of numbers"
        b = np.ascontiguousarray(b, dtype=self.vec_dtype).reshape(-1)
        assert b.size == self.n, "one right-hand side of N elements"
        k = sg.size
        ni, cv, re = np.zeros(max(k, 1), np.int32), np.zeros(max(k, 1), np.int32), np.zeros(max(k, 1), np.float64)
        st = Stats()
        self._chk(self._L.lam_hip_solve_mshift(self._h, b.ctypes.data_as(C.c_void_p), k, sg.ctypes.data_as(C.POINTER(C.c_double)),
                                               max_iters, rel_error, C.byref(st), ni.ctypes.data_as(C.POINTER(C.c_int32)),
                                               cv.ctypes.data_as(C.POINTER(C.c_int32)), re.ctypes.data_as(C.POINTER(C.c_double))))
        self.nrhs = 1
        self.nshifts = k
        self.stats = st.asdict()
        self.num_iters_shift, self.converged_shift, self.rel_err_shift = ni[:k].copy(), cv[:k].astype(bool), re[:k].copy()
        return self.converged_shift

    def multishift_solutions(self):
        """(nshifts, N): row j is the solution under shift j of the last solve_multishift."""
        k = getattr(self, "nshifts", 0)
        X = np.empty((max(k, 1), self.n), dtype=self.vec_dtype)
        self._chk(self._L.lam_hip_get_solution_mshift(self._h, k, X.ctypes.data_as(C.c_void_p)))
        return X[:k]

    def multishift_true_residuals(self):
        """||b - (A + s_j I) x_j|| / ||b|| of every shift of the last solve_multishift, formed on the device with one K = 8 product
        per group of 8 shifts (lam_hip_true_residual_mshift).  The solutions and the seed's batch stay readable."""
        k = getattr(self, "nshifts", 0)
        r = np.zeros(max(k, 1), np.float64)
        self._chk(self._L.lam_hip_true_residual_mshift(self._h, k, r.ctypes.data_as(C.POINTER(C.c_double))))
        return r[:k].copy()

    def solve_many(self, max_iters, rel_error, precond=PC_NONE, x0=None):
        """Independent CG recurrences for the right-hand sides of set_rhs_many, one pass over the matrix per iteration.  Returns
        the per-column `converged` array; self.num_iters_many / converged_many / rel_err_many hold the per-column results and
        self.stats the batch's.  precond: PC_NONE (lam_hip_solve_many) or PC_JACOBI (lam_hip_solve_many_pc, M = diag(A)).
        x0: None = from x = 0; an (nrhs, N) array = from that guess; "continue" = from the batch's current solution, the restart
        or continuation of the last solve_many (both lam_hip_solve_many_x0)."""
        k = getattr(self, "nrhs", 0)
        ni, cv, re = np.zeros(max(k, 1), np.int32), np.zeros(max(k, 1), np.int32), np.zeros(max(k, 1), np.float64)
        st = Stats()
        out = (C.byref(st), ni.ctypes.data_as(C.POINTER(C.c_int32)), cv.ctypes.data_as(C.POINTER(C.c_int32)),
               re.ctypes.data_as(C.POINTER(C.c_double)))
        if x0 is not None:
            if isinstance(x0, str):
                assert x0 == "continue", "x0 is None, an (nrhs, N) array or \"continue\""
                guess = None
            else:
                X0 = self._as_columns(x0)
                assert X0.shape[0] == k, "one guess per right-hand side of set_rhs_many"
                guess = X0.ctypes.data_as(C.c_void_p)
            self._chk(self._L.lam_hip_solve_many_x0(self._h, precond, guess, max_iters, rel_error, *out))
        elif precond == PC_NONE:
            self._chk(self._L.lam_hip_solve_many(self._h, max_iters, rel_error, *out))
        else:
            self._chk(self._L.lam_hip_solve_many_pc(self._h, precond, max_iters, rel_error, *out))
        self.stats = st.asdict()
        self.num_iters_many, self.converged_many, self.rel_err_many = ni[:k].copy(), cv[:k].astype(bool), re[:k].copy()
        return self.converged_many

    def solve_minres(self, max_iters, rel_error, shifts=None):
        """Independent MINRES recurrences on (A + shifts[j] I) x_j = b_j for the right-hand sides of set_rhs_many
        (lam_hip_solve_many_minres): shifts of either sign, always from x = 0, no preconditioner.  shifts=None: the shifts in force;
        else one finite number per right-hand side, which become the shifts in force (true_residuals() measures under them, and
        solve_many refuses to run while one of them is negative).  Returns and fills what solve_many does."""
        k = getattr(self, "nrhs", 0)
        ni, cv, re = np.zeros(max(k, 1), np.int32), np.zeros(max(k, 1), np.int32), np.zeros(max(k, 1), np.float64)
        st = Stats()
        sg = None
        if shifts is not None:
            sg = np.ascontiguousarray(np.atleast_1d(shifts), dtype=np.float64)
            assert sg.ndim == 1 and sg.size == k, "one shift per right-hand side of set_rhs_many"
        self._chk(self._L.lam_hip_solve_many_minres(self._h, None if sg is None else sg.ctypes.data_as(C.POINTER(C.c_double)),
                                                    max_iters, rel_error, C.byref(st), ni.ctypes.data_as(C.POINTER(C.c_int32)),
                                                    cv.ctypes.data_as(C.POINTER(C.c_int32)), re.ctypes.data_as(C.POINTER(C.c_double))))
        self.stats = st.asdict()
        self.num_iters_many, self.converged_many, self.rel_err_many = ni[:k].copy(), cv[:k].astype(bool), re[:k].copy()
        return self.converged_many

    def solve_shifted_minres(self, b, shifts, max_iters, rel_error):
        """(A + shifts[j] I) x_j = b for 1..MAX_RHS shifts of either sign in one MINRES batch: b replicated as solve_shifted does."""
        sg = np.atleast_1d(np.asarray(shifts, dtype=np.float64))
        b = np.ascontiguousarray(b, dtype=self.vec_dtype).reshape(1, -1)
        self.set_rhs_many(np.repeat(b, sg.size, axis=0))
        return self.solve_minres(max_iters, rel_error, sg)

    def solutions(self):
        """(nrhs, N): row j is the solution of right-hand side j of the last solve_many."""
        X = np.empty((self.nrhs, self.n), dtype=self.vec_dtype)
        self._chk(self._L.lam_hip_get_solution_many(self._h, self.nrhs, X.ctypes.data_as(C.c_void_p)))
        return X

    def true_residuals(self, nrhs=None):
        """||b_j - A x_j|| / ||b_j|| of the first nrhs (default: all) columns of the last solve_many, formed on the device with one
        batched product (lam_hip_true_residual_many).  The solution stays readable and solve_many(x0="continue") continues from it."""
        k = self.nrhs if nrhs is None else nrhs
        r = np.zeros(max(k, 1), np.float64)
        self._chk(self._L.lam_hip_true_residual_many(self._h, k, r.ctypes.data_as(C.POINTER(C.c_double))))
        return r[:k].copy()

    def diagonal(self):
        """The stored diagonal of the matrix (N elements of the vector dtype), extracted on the device."""
        d = np.empty(self.n, dtype=self.vec_dtype)
        self._chk(self._L.lam_hip_get_diagonal(self._h, d.ctypes.data_as(C.c_void_p)))
        return d

    def solve_all(self, B, max_iters, rel_error, precond=PC_NONE):
        """Any number of right-hand sides (rows of B), solved in batches of at most MAX_RHS (rhs_groups).  Returns
        (X, num_iters, converged, rel_err), one row / entry per right-hand side."""
        B = self._as_columns(B)
        X = np.empty_like(B)
        ni, cv, re = np.zeros(B.shape[0], np.int32), np.zeros(B.shape[0], bool), np.zeros(B.shape[0], np.float64)
        for first, count in rhs_groups(B.shape[0]):
            self.set_rhs_many(B[first:first + count])
            self.solve_many(max_iters, rel_error, precond)
            X[first:first + count] = self.solutions()
            ni[first:first + count], cv[first:first + count], re[first:first + count] = (self.num_iters_many, self.converged_many,
                                                                                          self.rel_err_many)
        return X, ni, cv, re

    def gemv_many(self, X):
        """Y = A X with the batched product kernel; X: (nrhs, N), row j is vector j."""
        X = self._as_columns(X)
        Y = np.empty_like(X)
        self._chk(self._L.lam_hip_gemv_many(self._h, X.shape[0], X.ctypes.data_as(C.c_void_p), Y.ctypes.data_as(C.c_void_p)))
        return Y

    def gemv_many_only(self, nrhs, reps):
        v = C.c_double()
        self._chk(self._L.lam_hip_gemv_many_only(self._h, nrhs, reps, C.byref(v)))
        return v.value

    # -- Lanczos eigensolver (one shard, F64 / F32) ---------------------------------------------
    def eigs(self, nev, which="smallest", max_steps=None, tol=None, check_every=8, v0=None, seed=0):
        """Extreme eigenpairs of the matrix by Lanczos with full reorthogonalisation (lam_hip_eigs).  which: "smallest", "largest",
        "both" (or the LAM_HIP_EIG_* value); max_steps defaults to min(N, MAX_LANCZOS), tol to 1e-10 (F64) / 1e-5 (F32); v0: a start
        vector of N elements, or None for generate_random_rhs(seed)'s.  Returns a dict: theta, bound, converged (nev entries, NaN /
        NaN / False past the pairs found), steps, nfound, stats."""
        w = EIG_WHICH[which] if isinstance(which, str) else int(which)
        if max_steps is None:
            max_steps = min(self.n, MAX_LANCZOS)
        if tol is None:
            tol = 1e-10 if self.dtype == F64 else 1e-5
        v0p = None
        if v0 is not None:
            v0 = np.ascontiguousarray(v0, dtype=self.vec_dtype).reshape(-1)
            assert v0.size == self.n, "the start vector has N elements"
            v0p = v0.ctypes.data_as(C.c_void_p)
        k = max(int(nev), 1)
        th, bd, cv = np.zeros(k, np.float64), np.zeros(k, np.float64), np.zeros(k, np.int32)
        nf, st = C.c_int32(0), Stats()
        dp = C.POINTER(C.c_double)
        self._chk(self._L.lam_hip_eigs(self._h, w, nev, max_steps, tol, check_every, v0p, seed, C.byref(st), C.byref(nf),
                                       th.ctypes.data_as(dp), bd.ctypes.data_as(dp), cv.ctypes.data_as(C.POINTER(C.c_int32))))
        self.stats = st.asdict()
        self.nfound = nf.value
        return {"theta": th, "bound": bd, "converged": cv.astype(bool), "steps": st.num_iters, "nfound": nf.value, "stats": self.stats}

    def eigenvectors(self):
        """(nfound, N): row i is the Ritz vector of pair i of the last eigs, in theta's order."""
        k = getattr(self, "nfound", 0)
        Y = np.empty((max(k, 1), self.n), dtype=self.vec_dtype)
        self._chk(self._L.lam_hip_get_eigenvectors(self._h, k, Y.ctypes.data_as(C.c_void_p)))
        return Y[:k]

    def eig_residuals(self):
        """||A y_i - theta_i y_i|| / ||y_i|| of every pair found by the last eigs, formed on the device (lam_hip_eig_residuals)."""
        k = getattr(self, "nfound", 0)
        r = np.zeros(max(k, 1), np.float64)
        self._chk(self._L.lam_hip_eig_residuals(self._h, k, r.ctypes.data_as(C.POINTER(C.c_double))))
        return r[:k].copy()

    def lanczos_coefficients(self):
        """(alpha, beta) of the last eigs, `steps` entries each; beta[k] is the norm that made v_{k+1}."""
        a, b = np.zeros(MAX_LANCZOS, np.float64), np.zeros(MAX_LANCZOS, np.float64)
        ns = C.c_int32(0)
        dp = C.POINTER(C.c_double)
        self._chk(self._L.lam_hip_get_lanczos(self._h, C.byref(ns), a.ctypes.data_as(dp), b.ctypes.data_as(dp)))
        return a[:ns.value].copy(), b[:ns.value].copy()

    # -- Lanczos quadrature for the batch (one shard, F64 / F32) ----------------------------------
    def lanczos_many(self, probes, steps, seed=0):
        """`steps` steps of plain Lanczos from every probe, groups of probes sharing each pass over the matrix (lam_hip_lanczos_many).
        probes: an int -- that many Rademacher probes built on the device from `seed` -- or an array of probe vectors of N elements
        each, one per row.  Returns a dict: steps_run (nprobes), znorm2 (nprobes), alpha and beta (nprobes, steps; NaN past
        steps_run), stats."""
        zp = None
        if isinstance(probes, (int, np.integer)):
            nprobes = int(probes)
        else:
            Z = self._as_columns(probes)
            nprobes, zp = Z.shape[0], Z.ctypes.data_as(C.c_void_p)
        k, m = max(nprobes, 1), max(int(steps), 1)
        sr, zz = np.zeros(k, np.int32), np.zeros(k, np.float64)
        a, b = np.zeros((k, m), np.float64), np.zeros((k, m), np.float64)
        st = Stats()
        dp = C.POINTER(C.c_double)
        self._chk(self._L.lam_hip_lanczos_many(self._h, nprobes, zp, seed, steps, C.byref(st), sr.ctypes.data_as(C.POINTER(C.c_int32)),
                                               zz.ctypes.data_as(dp), a.ctypes.data_as(dp), b.ctypes.data_as(dp)))
        self.stats = st.asdict()
        self.nprobes = nprobes
        return {"steps_run": sr, "znorm2": zz, "alpha": a, "beta": b, "stats": self.stats}

    def lanczos_many_coefficients(self, nprobes=None):
        """What the last lanczos_many left in the context (lam_hip_get_lanczos_many): the same dict without the stats."""
        k = int(getattr(self, "nprobes", 1) if nprobes is None else nprobes)
        sr, zz = np.zeros(max(k, 1), np.int32), np.zeros(max(k, 1), np.float64)
        ns = C.c_int32(0)
        dp = C.POINTER(C.c_double)
        # the library lays the rows out at the run's own `steps`: ask for it first, then read into arrays of that shape
        self._chk(self._L.lam_hip_get_lanczos_many(self._h, k, C.byref(ns), None, None, None, None))
        a, b = np.zeros((k, ns.value), np.float64), np.zeros((k, ns.value), np.float64)
        self._chk(self._L.lam_hip_get_lanczos_many(self._h, k, C.byref(ns), sr.ctypes.data_as(C.POINTER(C.c_int32)), zz.ctypes.data_as(dp),
                                                   a.ctypes.data_as(dp), b.ctypes.data_as(dp)))
        return {"steps_run": sr, "znorm2": zz, "alpha": a, "beta": b}

    def trace_quadrature(self, fn, shifts=None, param=0, per_probe=False):
        """The quadrature of the last lanczos_many for every shift (None: the one shift 0) -- host arithmetic
        (lam_hip_trace_quadrature).  fn: "log", "inv", "pow" (or the LAM_HIP_QUAD_* value).  Returns (estimate, std_error), each one
        entry per shift, and with per_probe=True also the (nshifts, nprobes) values the mean is taken over.  For Rademacher probes
        estimate[s] estimates tr f(A + shifts[s] I)."""
        f = QUAD_FN[fn] if isinstance(fn, str) else int(fn)
        dp = C.POINTER(C.c_double)
        sg = None if shifts is None else np.ascontiguousarray(shifts, dtype=np.float64).reshape(-1)
        ns = 1 if sg is None else sg.size
        est, se = np.zeros(max(ns, 1), np.float64), np.zeros(max(ns, 1), np.float64)
        pp = np.zeros((max(ns, 1), max(getattr(self, "nprobes", 1), 1)), np.float64)
        self._chk(self._L.lam_hip_trace_quadrature(self._h, f, float(param), ns, None if sg is None else sg.ctypes.data_as(dp),
                                                   est.ctypes.data_as(dp), se.ctypes.data_as(dp), pp.ctypes.data_as(dp) if per_probe else None))
        return (est[:ns], se[:ns], pp[:ns]) if per_probe else (est[:ns], se[:ns])

    def logdet(self, shifts=None, nprobes=8, steps=64, seed=0):
        """(estimate, std_error) of log det(A + s I) for every s of `shifts` (None: log det A) from ONE run of nprobes Rademacher probes
        and `steps` Lanczos steps (lanczos_many + trace_quadrature); steps is capped at min(N, MAX_LANCZOS)."""
        self.lanczos_many(int(nprobes), min(int(steps), self.n, MAX_LANCZOS), seed)
        return self.trace_quadrature("log", shifts)

    # -- deflated CG for the batch (one shard, F64 / F32) -----------------------------------------
    def set_deflation(self, W):
        """The deflation space of solve_deflated (lam_hip_set_deflation): W (m, N), any full-rank set of m <= MAX_DEFLATION vectors;
        None or an empty W clears it.  A batched solution is no longer readable afterwards."""
        if W is None or np.size(W) == 0:
            self._chk(self._L.lam_hip_set_deflation(self._h, 0, None))
            return
        W = np.ascontiguousarray(W, dtype=self.vec_dtype)
        if W.ndim == 1:
            W = W.reshape(1, -1)
        assert W.ndim == 2 and W.shape[1] == self.n, "W is (m, N)"
        self._chk(self._L.lam_hip_set_deflation(self._h, W.shape[0], W.ctypes.data_as(C.c_void_p)))

    def set_deflation_from_eigs(self, m):
        """The first m Ritz vectors of the last eigs as the deflation space, device to device (lam_hip_set_deflation_eigs)."""
        self._chk(self._L.lam_hip_set_deflation_eigs(self._h, m))

    def solve_deflated(self, max_iters, rel_error):
        """Deflated CG on the right-hand sides of set_rhs_many, from x = 0 (lam_hip_solve_many_deflated).  Returns and fills what
        solve_many does; solutions(), true_residuals() and solve_many(x0="continue") follow as usual."""
        k = getattr(self, "nrhs", 0)
        ni, cv, re = np.zeros(max(k, 1), np.int32), np.zeros(max(k, 1), np.int32), np.zeros(max(k, 1), np.float64)
        st = Stats()
        self._chk(self._L.lam_hip_solve_many_deflated(self._h, max_iters, rel_error, C.byref(st), ni.ctypes.data_as(C.POINTER(C.c_int32)),
                                                      cv.ctypes.data_as(C.POINTER(C.c_int32)), re.ctypes.data_as(C.POINTER(C.c_double))))
        self.stats = st.asdict()
        self.num_iters_many, self.converged_many, self.rel_err_many = ni[:k].copy(), cv[:k].astype(bool), re[:k].copy()
        return self.converged_many

    def deflate_many(self, Wd, Wa, M, U):
        """The deflation operator alone (lam_hip_deflate_many): Wd, Wa (m, n), M (m, m) fp64, U (nrhs, n).  Returns (coeff, U_new)
        with coeff[i, j] = Wd[i].U[j] and U_new[j] = U[j] - sum_i (M coeff[:, j])[i] Wa[i] in the vector dtype."""
        Wd = np.ascontiguousarray(Wd, dtype=self.vec_dtype)
        Wa = np.ascontiguousarray(Wa, dtype=self.vec_dtype)
        U = np.ascontiguousarray(U, dtype=self.vec_dtype)
        if Wd.ndim == 1:
            Wd, Wa = Wd.reshape(1, -1), Wa.reshape(1, -1)
        if U.ndim == 1:
            U = U.reshape(1, -1)
        U = U.copy()
        m, n = Wd.shape
        M = np.ascontiguousarray(M, dtype=np.float64).reshape(m, m)
        assert Wa.shape == (m, n) and U.shape[1] == n, "Wd and Wa are (m, n), U is (nrhs, n)"
        coeff = np.zeros((max(m, 1), max(U.shape[0], 1)), np.float64)
        self._chk(self._L.lam_hip_deflate_many(self._h, n, m, U.shape[0], Wd.ctypes.data_as(C.c_void_p), Wa.ctypes.data_as(C.c_void_p),
                                               M.ctypes.data_as(C.POINTER(C.c_double)), U.ctypes.data_as(C.c_void_p),
                                               coeff.ctypes.data_as(C.POINTER(C.c_double))))
        return coeff[:m, :U.shape[0]], U

    # -- block CG for the batch (one shard, F64 / F32) ---------------------------------------------
    def solve_block(self, max_iters, rel_error, fallback=False, fallback_max_iters=None):
        """Block CG on the right-hand sides of set_rhs_many, from X = 0: one block Krylov space for all of them
        (lam_hip_solve_block).  Returns (num_iters, converged, rel_err, breakdown): per column the first iteration that met the
        test (max_iters + 1: never) and the values at exit, and breakdown = (iteration, kind), (0, 0) for none; self.stats holds the
        batch's, self.num_iters_many / converged_many / rel_err_many the per-column arrays.  solutions() and true_residuals()
        follow as usual.  fallback=True: if some column has not converged (a breakdown, or the cap), solve_many(fallback_max_iters
        (default: max_iters), rel_error, x0="continue") runs behind it -- the independent recurrences from the block's X -- and
        converged and rel_err are that solve's; its iteration counts are in self.fallback_iters (None when it did not run)."""
        k = getattr(self, "nrhs", 0)
        ni, cv, re = np.zeros(max(k, 1), np.int32), np.zeros(max(k, 1), np.int32), np.zeros(max(k, 1), np.float64)
        bd = np.zeros(2, np.int32)
        st = Stats()
        ip = C.POINTER(C.c_int32)
        self._chk(self._L.lam_hip_solve_block(self._h, max_iters, rel_error, C.byref(st), ni.ctypes.data_as(ip), cv.ctypes.data_as(ip),
                                              re.ctypes.data_as(C.POINTER(C.c_double)), bd.ctypes.data_as(ip)))
        self.stats = st.asdict()
        self.num_iters_many, self.converged_many, self.rel_err_many = ni[:k].copy(), cv[:k].astype(bool), re[:k].copy()
        self.breakdown = (int(bd[0]), int(bd[1]))
        self.fallback_iters = None
        block_iters = self.num_iters_many
        if fallback and not self.converged_many.all():
            block_stats = self.stats
            self.solve_many(max_iters if fallback_max_iters is None else fallback_max_iters, rel_error, x0="continue")
            self.fallback_iters = self.num_iters_many
            self.fallback_stats, self.stats = self.stats, block_stats
            self.num_iters_many = block_iters
        return block_iters, self.converged_many, self.rel_err_many, self.breakdown

    # -- single operators -----------------------------------------------------------------------
    def project_out(self, V, u):
        """One pass of the eigensolver's reorthogonalisation (lam_hip_project_out): V (m, n), u (n).  Returns (coeff, u_new) with
        coeff[j] = V[j].u and u_new = u - sum_j coeff[j] V[j] in the vector dtype."""
        V = np.ascontiguousarray(V, dtype=self.vec_dtype)
        if V.ndim == 1:
            V = V.reshape(1, -1)
        u = np.ascontiguousarray(u, dtype=self.vec_dtype).reshape(-1).copy()
        assert V.ndim == 2 and V.shape[1] == u.size, "V is (m, n), u has n elements"
        coeff = np.zeros(max(V.shape[0], 1), np.float64)
        self._chk(self._L.lam_hip_project_out(self._h, u.size, V.shape[0], V.ctypes.data_as(C.c_void_p), u.ctypes.data_as(C.c_void_p),
                                              coeff.ctypes.data_as(C.POINTER(C.c_double))))
        return coeff[:V.shape[0]], u

    def gemv(self, x):
        x = np.ascontiguousarray(x, dtype=self.vec_dtype).reshape(-1)
        assert x.size == self.n
        y = np.empty(self.n, dtype=self.vec_dtype)
        self._chk(self._L.lam_hip_gemv(self._h, x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p)))
        return y

    def gemv_only(self, reps):
        v = C.c_double()
        self._chk(self._L.lam_hip_gemv_only(self._h, reps, C.byref(v)))
        return v.value

    def dot(self, x, y):
        x = np.ascontiguousarray(x, dtype=self.vec_dtype).reshape(-1)
        y = np.ascontiguousarray(y, dtype=self.vec_dtype).reshape(-1)
        v = C.c_double()
        self._chk(self._L.lam_hip_dot(self._h, x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), x.size,
                                      C.byref(v)))
        return v.value

    def axpby(self, alpha, x, beta, y):
        x = np.ascontiguousarray(x, dtype=self.vec_dtype).reshape(-1)
        y = np.ascontiguousarray(y, dtype=self.vec_dtype).reshape(-1).copy()
        self._chk(self._L.lam_hip_axpby(self._h, alpha, x.ctypes.data_as(C.c_void_p), beta,
                                        y.ctypes.data_as(C.c_void_p), x.size))
        return y

    def check_symmetry(self):
        v = C.c_double()
        self._chk(self._L.lam_hip_check_symmetry(self._h, C.byref(v)))
        return v.value

    def all_ok(self, ok):
        g = C.c_int(0)
        self._chk(self._L.lam_hip_all_ok(self._h, 1 if ok else 0, C.byref(g)))
        return bool(g.value)

    def gemv_kernel_name(self):
        buf = C.create_string_buffer(256)
        self._chk(self._L.lam_hip_gemv_kernel_name(self._h, buf, 256))
        return buf.value.decode()

    def get_option(self, name):
        v = C.c_int64()
        self._chk(self._L.lam_hip_get_option(self._h, name.encode(), C.byref(v)))
        return v.value

    def set_option(self, name, value):
        self._chk(self._L.lam_hip_set_option(self._h, name.encode(), value))
