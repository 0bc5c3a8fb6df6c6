// lam_multi.h -- several right-hand sides on one matrix: the host side of every batched entry point.  nrhs independent recurrences
// (NOT block CG: that is lam_block.h, on this file's state and driver) advanced together, one pass over the matrix per iteration.
// Kernels: lam_kernels.h ("Several right-hand sides", "Batched MINRES", "Multi-shift CG").  Part of the one translation unit
// csrc/lam_hip.hip (included from there, in order; not a stand-alone header).
//
// Map of the file:
//   state         multi_release / multi_ensure (MultiState), pcg_ensure (PcgState), minres_ensure, mshift_ensure: allocated lazily for
//                 the batch's n, released together
//   helpers       multi_dispatch, the one dispatch ladder; multi_launch_gemv, the one product launch; multi_upload / _download /
//                 _stage_solution; multi_read_shifts, the one reader of shifts; pcg_scan and read_element, the diagonal scans' host
//                 protocol; multi_residual_tail; multi_report
//   driver        multi_drive, the enqueue loop of every batched solve: the batch's own pinned progress word under the single solve's
//                 lag rule (lag_check; "stopped" means every live column has stopped), the timed product slots, enqueue_ns
//   solves        multi_solve (CG: plain, Jacobi, from a guess, shifted, the multi-shift seed) and minres_solve: checks, lazy
//                 allocation, their launches in front of the loop and behind the product of iteration k, multi_report
//   entry points  extern "C", at the end of the file
//
// Instantiations: K = 1, 2, 4, 8 columns; nrhs runs on the smallest K >= nrhs, the K - nrhs padding columns are zero and born stopped.
// Product shape, every K and both dtypes: 4 rows per 4-wave workgroup, p tile of 32 KiB in LDS whatever K
// (fp64: 4096 / 2048 / 1024 / 512 columns for K = 1 / 2 / 4 / 8; fp32: 4096 / 4096 / 2048 / 1024), non-temporal matrix loads.
// Three launches per iteration (the product and two vector kernels), all on shard 0's stream.
// One CG recurrence in the source: Jacobi runs the PC = true instantiations of the four vector kernels on the same scalars' block, a
// start from a guess the GUESS = true instantiations of the two init kernels behind one more product launch.
// Shifts (column j is the system (A + s_j I) x_j = b_j) travel by value in the product's arguments: its SHIFT = true instantiation, and
// under Jacobi the DK = true vector kernels on a K-wide dinv_k = 1 / (A_ii + s_j).  No shifts, or all of them zero: the plain ones.
// Only MINRES takes a negative shift and can leave one in force; CG refuses to run under it.
// Option "symmetric_many" (K <= 4): the product launch becomes the two passes of the symmetric batched product (multi_sym_launch: every
// pair {A_ij, A_ji} read once, one more launch per product, its own plan and partials in MultiState); K = 8 and option 0 are untouched.
// Option "packed_many" (fp64, K <= 4, where "symmetric_many" does not engage): the product launch reads the packed image of the matrix
// (multi_gemv_packed_kernel: the same grid, partials and bits); pack_many_maybe, in front of a product, is who causes it to be built.
#pragma once

static_assert(lam::kMaxRhs == LAM_HIP_MAX_RHS, "include/lam_hip.h states the limit");
static_assert(lam::kMaxShifts == LAM_HIP_MAX_SHIFTS, "include/lam_hip.h states the limit");
static_assert(lam::kShiftGroup == lam::kMaxRhs, "a group of shifts is handed to the K = 8 product as it is");

namespace {

constexpr int kMultiRows = 4;     // rows per workgroup of multi_gemv_kernel
constexpr int kMultiWaves = 4;    // waves per workgroup

// ---- state -----------------------------------------------------------------------------------------------------------------
void free_dev(std::initializer_list<void *> ptrs)
{
    for (void *q : ptrs) if (q) (void)hipFree(q);
}

void multi_clear_shifts(MultiState &m)
{
    for (double &v : m.shift) v = 0.0;
    m.shifted = false;
}

void multi_release(lam_hip_ctx *c)
{
    MultiState &m = c->multi;
    if (m.n == 0) return;        // the preconditioner's state is allocated behind the batch's only (pcg_ensure)
    if (c->sh.empty() || hipSetDevice(c->sh[0].dev) != hipSuccess) { (void)hipGetLastError(); return; }
    if (c->sh[0].stream) (void)hipStreamSynchronize(c->sh[0].stream);
    free_dev({c->pcg.diag, c->pcg.dinv, c->pcg.dinv_k, c->pcg.part_rz, c->pcg.info});
    c->pcg = PcgState();
    free_dev({m.B, m.X, m.R, m.P, m.AP, m.stage, m.part_gemv, m.part_vec, m.part_rr, m.res, m.sc});
    free_dev({m.ms.XS, m.ms.PS, m.ms.sc});
    free_dev({m.mr.W, m.mr.WOLD, m.mr.sc});
    symv_dev_release(m.sym);
    free_dev({m.lz.V, m.lz.U, m.lz.Y, m.lz.part, m.lz.part_uu, m.lz.S, m.lz.sc});
    free_dev({m.df.W, m.df.AW, m.df.Ginv, m.df.part});
    free_dev({m.bk.part_h, m.bk.part_g, m.bk.sc});
    free_dev({m.qd.sc});
    if (m.sc_host) (void)hipHostFree(m.sc_host);
    if (m.host_flags) (void)hipHostFree(m.host_flags);
    for (int i = 0; i < kLag; i++) {
        if (m.ev0[i]) (void)hipEventDestroy(m.ev0[i]);
        if (m.ev1[i]) (void)hipEventDestroy(m.ev1[i]);
    }
    const int last_K = m.last_K;
    m = MultiState();
    m.last_K = last_K;
}

int multi_ensure(lam_hip_ctx *c)
{
    MultiState &m = c->multi;
    if (m.n == c->n) return 0;
    multi_release(c);
    ShardBase &s = c->sh[0];
    LAMCHK(set_dev(c, s));
    const size_t ev = c->esz_v(), elems = (size_t)(c->n + kMultiPadRows) * kMaxRhs;
    m.n = c->n;                  // from here on multi_release gives back whatever the calls below obtained
    void **vecs[] = {&m.B, &m.X, &m.R, &m.P, &m.AP, &m.stage};
    for (auto v : vecs) HIPCHK(c, hipMalloc(v, elems * ev));
    HIPCHK(c, hipMalloc((void **)&m.part_gemv, sizeof(double) * kMaxRhs * (size_t)c->n));
    HIPCHK(c, hipMalloc((void **)&m.part_vec, sizeof(double) * kMaxRhs * kVecBlocksMax));
    HIPCHK(c, hipMalloc((void **)&m.part_rr, sizeof(double) * kMaxRhs * kVecBlocksMax));
    HIPCHK(c, hipMalloc((void **)&m.res, sizeof(double) * kMaxRhs));
    HIPCHK(c, hipMalloc((void **)&m.sc, sizeof(BatchScalars)));
    HIPCHK(c, hipHostMalloc((void **)&m.sc_host, sizeof(MultiScalars), hipHostMallocDefault));
    HIPCHK(c, hipHostMalloc((void **)&m.host_flags, 64, hipHostMallocDefault));
    m.host_flags[0] = m.host_flags[1] = 0;
    memset(m.sc_host, 0, sizeof(MultiScalars));
    for (int i = 0; i < kLag; i++) {
        HIPCHK(c, hipEventCreate(&m.ev0[i]));
        HIPCHK(c, hipEventCreate(&m.ev1[i]));
    }
    // the product reads whole 16-byte vectors of a row: up to 7 columns behind the end of P are met (by zeros of the row padding),
    // so P is zero behind row n and stays so -- the kernels write rows below n only
    HIPCHK(c, hipMemsetAsync(m.P, 0, elems * ev, s.stream));
    HIPCHK(c, hipMemsetAsync(m.sc, 0, sizeof(BatchScalars), s.stream));
    HIPCHK(c, hipStreamSynchronize(s.stream));
    return 0;
}

// The Jacobi preconditioner of lam_hip_solve_many_pc.  No reference counterpart: the reference is un-preconditioned.
// Sized for the batch's n (multi_solve has checked multi.n == n) and released with the batch, so "allocated" is all there is to know.
int pcg_ensure(lam_hip_ctx *c)
{
    PcgState &g = c->pcg;
    if (g.info) return 0;
    LAMCHK(set_dev(c, c->sh[0]));
    free_dev({g.diag, g.dinv, g.dinv_k, g.part_rz});      // what a failed attempt left: it is retried, never launched on
    g = PcgState();
    HIPCHK(c, hipMalloc(&g.diag, c->n * c->esz_v()));
    HIPCHK(c, hipMalloc(&g.dinv, c->n * c->esz_v()));
    HIPCHK(c, hipMalloc((void **)&g.part_rz, sizeof(double) * kMaxRhs * kVecBlocksMax));
    HIPCHK(c, hipMalloc((void **)&g.info, sizeof(DiagInfo)));
    return 0;
}

// W, W_OLD and the scalars of lam_hip_solve_many_minres for the batch's n (multi.n == n has been checked)
int minres_ensure(lam_hip_ctx *c)
{
    MinresState &r = c->multi.mr;
    if (r.sc) return 0;
    free_dev({r.W, r.WOLD});                 // what a failed attempt left: it is retried, never launched on
    r = MinresState();
    const size_t bytes = (size_t)(c->n + kMultiPadRows) * kMaxRhs * c->esz_v();
    HIPCHK(c, hipMalloc(&r.W, bytes));
    HIPCHK(c, hipMalloc(&r.WOLD, bytes));
    HIPCHK(c, hipMalloc((void **)&r.sc, sizeof(MinresScalars)));
    HIPCHK(c, hipMemsetAsync(r.sc, 0, sizeof(MinresScalars), c->sh[0].stream));
    return 0;
}

// XS / PS for `groups` groups of the batch's n (multi_ensure has run): grow-only; zero once, so that the rows behind row n stay zero
int mshift_ensure(lam_hip_ctx *c, int groups)
{
    MshiftState &ms = c->multi.ms;
    if (!ms.sc) HIPCHK(c, hipMalloc((void **)&ms.sc, sizeof(MshiftScalars)));
    if (groups <= ms.groups_cap) return 0;
    ShardBase &s = c->sh[0];
    HIPCHK(c, hipStreamSynchronize(s.stream));
    free_dev({ms.XS, ms.PS});
    ms.XS = ms.PS = nullptr;
    ms.groups_cap = 0;
    const size_t bytes = (size_t)groups * (c->n + kMultiPadRows) * kShiftGroup * c->esz_v();
    HIPCHK(c, hipMalloc(&ms.XS, bytes));
    HIPCHK(c, hipMalloc(&ms.PS, bytes));
    HIPCHK(c, hipMemsetAsync(ms.XS, 0, bytes, s.stream));
    HIPCHK(c, hipMemsetAsync(ms.PS, 0, bytes, s.stream));
    HIPCHK(c, hipStreamSynchronize(s.stream));
    ms.groups_cap = groups;
    return 0;
}

// ---- helpers ---------------------------------------------------------------------------------------------------------------
// what the batched entry points serve: one process, ONE shard, fp64 / fp32 storage
int multi_supported(lam_hip_ctx *c, const char *fn)
{
    if (c->rank_mode) return fail(c, LAM_HIP_EINVAL, "%s: rank mode (lam_hip_create_rank) is not supported by the multi-right-hand-side path", fn);
    if (c->total_shards != 1)
        return fail(c, LAM_HIP_EINVAL, "%s: %d shards: the multi-right-hand-side path supports one shard only", fn, c->total_shards);
    if (c->dtype == LAM_HIP_BF16) return fail(c, LAM_HIP_EINVAL, "%s: LAM_HIP_BF16 storage is not supported by the multi-right-hand-side path", fn);
    return 0;
}
int multi_check_nrhs(lam_hip_ctx *c, const char *fn, int nrhs)
{
    if (nrhs < 1 || nrhs > LAM_HIP_MAX_RHS) return fail(c, LAM_HIP_EINVAL, "%s: nrhs = %d, must be 1..%d (LAM_HIP_MAX_RHS)", fn, nrhs, LAM_HIP_MAX_RHS);
    return 0;
}
int mshift_check_n(lam_hip_ctx *c, const char *fn, int nshifts)
{
    if (nshifts < 1 || nshifts > LAM_HIP_MAX_SHIFTS)
        return fail(c, LAM_HIP_EINVAL, "%s: nshifts = %d, must be 1..%d (LAM_HIP_MAX_SHIFTS)", fn, nshifts, LAM_HIP_MAX_SHIFTS);
    return 0;
}
int mshift_readable(lam_hip_ctx *c, const char *fn, int nshifts)
{
    MultiState &m = c->multi;
    if (!m.solved || !m.ms.valid || m.n != c->n) return fail(c, LAM_HIP_ESTATE, "no multi-shift solution yet (lam_hip_solve_mshift)");
    if (nshifts > m.ms.nshifts) return fail(c, LAM_HIP_EINVAL, "%s: %d shifts asked, %d were solved", fn, nshifts, m.ms.nshifts);
    return 0;
}
int multi_k_for(int nrhs) { return nrhs <= 1 ? 1 : (nrhs <= 2 ? 2 : (nrhs <= 4 ? 4 : 8)); }
int multi_gemv_grid(const lam_hip_ctx *c) { return (int)((c->n + kMultiRows - 1) / kMultiRows); }
int mshift_groups(int nshifts) { return (nshifts + kShiftGroup - 1) / kShiftGroup; }

// x as the vector dtype holds it (fp64 / fp32 only: multi_supported)
double to_vec_dtype(const lam_hip_ctx *c, double x) { return c->dtype == LAM_HIP_F32 ? (double)(float)x : x; }

// the CG recurrence's form: PC = Jacobi-preconditioned, GUESS = from an initial guess (lam_hip_solve_many_x0), DK = the K-wide dinv of
// the shifted batch
template <bool PC_, bool GUESS_, bool DK_>
struct CgForm { static constexpr bool PC = PC_, GUESS = GUESS_, DK = DK_; };

// The one dispatch ladder of the batched path: f(Impl<TA, TV>(), integral_constant<int, K>()) for the context's dtype (fp64 / fp32
// only: multi_supported) and K; an f that takes a third argument (multi_solve's) is handed the CgForm of (pc, guess, dk) as well.
// Only PC has DK = true instantiations.
template <typename F>
int multi_dispatch(lam_hip_ctx *c, int K, F &&f, bool pc = false, bool guess = false, bool dk = false)
{
    auto with_form = [&](auto impl, auto k) -> int {
        if constexpr (std::is_invocable_v<F &, decltype(impl), decltype(k)>) return f(impl, k);
        else if (!pc) return guess ? f(impl, k, CgForm<false, true, false>()) : f(impl, k, CgForm<false, false, false>());
        else if (dk) return guess ? f(impl, k, CgForm<true, true, true>()) : f(impl, k, CgForm<true, false, true>());
        else return guess ? f(impl, k, CgForm<true, true, false>()) : f(impl, k, CgForm<true, false, false>());
    };
    auto with_k = [&](auto impl) -> int {
        switch (K) {
        case 1: return with_form(impl, std::integral_constant<int, 1>());
        case 2: return with_form(impl, std::integral_constant<int, 2>());
        case 4: return with_form(impl, std::integral_constant<int, 4>());
        case 8: return with_form(impl, std::integral_constant<int, 8>());
        }
        return fail(c, LAM_HIP_EINVAL, "no batched kernels for K = %d", K);
    };
    if (c->dtype == LAM_HIP_F64) return with_k(Impl<double, double>());
    if (c->dtype == LAM_HIP_F32) return with_k(Impl<float, float>());
    return fail(c, LAM_HIP_EINVAL, "the multi-right-hand-side path has no kernels for dtype %d", c->dtype);
}
// f(Impl<TA, TV>()) for the context's dtype: the multi-shift kernels have the one group width
template <typename F>
int mshift_dispatch(lam_hip_ctx *c, F &&f)
{
    if (c->dtype == LAM_HIP_F64) return f(Impl<double, double>());
    if (c->dtype == LAM_HIP_F32) return f(Impl<float, float>());
    return fail(c, LAM_HIP_EINVAL, "the multi-shift path has no kernels for dtype %d", c->dtype);
}

// ---- symmetric batched product (option "symmetric_many"; kernels: lam_kernels.h, "Symmetric batched product") ---------------
// Value 1 ("where it pays") admits the (dtype, K) whose symmetric batched iteration measured faster than the general one of the same
// build at its size, by more than the spread between the windows of the two figures (tools/symv_many_probe.py,
// profiles/symv_many_probe.txt; symmetric / general per iteration): fp64 N = 65536  K = 1: 0.53, 2: 0.50, 4: 0.53;
// fp32 N = 131072  K = 1: 0.52, 2: 0.53, 4: 0.50.  All six are admitted; a (dtype, K) that lost would read false here and stay
// reachable through value 2.
bool multi_sym_admitted(const lam_hip_ctx *c, int K)
{
    static constexpr bool admitted[2][kSymvManyMaxK + 1] = {/* fp64: K = - 1 2 - 4 */ {false, true, true, false, true},
                                                            /* fp32 */ {false, true, true, false, true}};
    if (K < 1 || K > kSymvManyMaxK) return false;
    return c->dtype == LAM_HIP_F64 ? admitted[0][K] : (c->dtype == LAM_HIP_F32 ? admitted[1][K] : false);
}
bool multi_sym_wanted(const lam_hip_ctx *c, int K)
{
    if (K > kSymvManyMaxK || c->n == 0) return false;
    if (c->opt_symmetric_many >= 2) return true;
    return c->opt_symmetric_many == 1 && c->n * c->n * (uint64_t)c->esz_a() >= (192ull << 20) && multi_sym_admitted(c, K);
}
int multi_sym_grid(const lam_hip_ctx *c) { return (int)((c->n + kSymvReduceRows - 1) / kSymvReduceRows); }
// p.Ap partials per column of the product multi_launch_gemv runs for instantiation K: what its consumers are told
int multi_product_blocks(const lam_hip_ctx *c, int K) { return multi_sym_wanted(c, K) ? multi_sym_grid(c) : multi_gemv_grid(c); }

// ---- packed batched product (option "packed_many"; kernel: lam_kernels.h, multi_gemv_packed_kernel) --------------------------
// Automatic mode (-1) admits the K whose packed product measured faster than the plain one of the same build and process by more than
// the spread between the windows of the two figures (multi_sym_admitted's rule; tools/packed_many_probe.py,
// profiles/packed_many_probe.txt; packed / plain per product of lam_hip_gemv_many_only, fp64):
//   N = 65536  K = 1: 0.898 (4.365 / 4.863 ms, spread 0.007)   K = 2: 0.964 (5.062 / 5.252, spread 0.010)   K = 4: 1.105 (5.959 / 5.393)
//   N = 32768  K = 1: 0.897 (1.095 / 1.220 ms, spread 0.001)   K = 2: 1.040 (1.287 / 1.237)                  K = 4: 1.119 (1.553 / 1.387)
// K = 1 wins at both sizes and is admitted: the single packed product's ratio carries over whole.  K = 2 wins at N = 65536 only and
// K = 4 loses at both (a visit of a unit holds 112 element registers a thread: two workgroups a CU, and K pairs of barriers with
// nothing in flight between them); they read false here and stay reachable through value 1.
// Break-even of K = 1, pack time / (plain - packed): 16.3 ms / 0.498 ms = 32.7 products at N = 65536, 31.7 at N = 32768 -- half the
// single product's 64.4, because the batch's plain kernel is the slower one.  The one threshold (kPackAfter = 65) stays: it is
// shared with the single product, and a context that packs after 65 products instead of 33 gives away 16 ms once.
bool pack_many_admitted(int K)
{
    static constexpr bool admitted[kPackManyMaxK + 1] = {/* K = - 1 2 - 4 */ false, true, false, false, false};
    return K >= 1 && K <= (int)kPackManyMaxK && admitted[K];
}
// does the batched product of instantiation K read the image, given one of the current content?
bool pack_many_reads(const lam_hip_ctx *c, int K)
{
    if (!c->pack_many_eligible() || K > (int)kPackManyMaxK || multi_sym_wanted(c, K) || !c->pack_image_ready()) return false;
    return c->opt_packed_many == 1 || pack_many_admitted(K);
}
// The batch's trigger, where pack_maybe is the single product's: in front of a batched product of instantiation K, outside every
// timing event pair.  Value 1: the image is built now; automatic: for an admitted K once "packed"'s thresholds hold (pack_auto_due).
int pack_many_maybe(lam_hip_ctx *c, int K)
{
    if (!c->pack_many_eligible() || !c->have_matrix || K > (int)kPackManyMaxK || multi_sym_wanted(c, K)) return 0;
    const bool automatic = c->opt_packed_many < 0;
    if (automatic && (!pack_many_admitted(K) || !pack_auto_due(c))) return 0;
    return pack_build(c, automatic);
}

void multi_sym_release(MultiState &m)
{
    symv_dev_release(m.sym);
    m.sym_vec = m.sym_cap_K = 0;
}

// Plan (symv_dev_build as the single product has it: one shard, strips of 256 * VEC columns) at first use for the batch's n; partials
// for K columns, grow-only.  All of a step or none of it: a failed allocation leaves what there was, and the batch runs on under option 0.
template <typename TA, typename TV>
int multi_sym_ensure(lam_hip_ctx *c, int K)
{
    MultiState &m = c->multi;
    ShardBase &s = c->sh[0];
    constexpr int VEC = MatVec<TA>::N;
    constexpr uint64_t SS = (uint64_t)kBlock * VEC;
    if (m.sym.tasks != nullptr && m.sym_vec != VEC) {        // the same n under another storage type: another plan
        HIPCHK(c, hipStreamSynchronize(s.stream));
        multi_sym_release(m);
    }
    if (m.sym.tasks == nullptr) {
        LAMCHK(symv_dev_build(c, m.sym, c->n, c->ncols_vec(), SS, 0, c->n, false, sizeof(TV), K, s.stream, "symmetric batched product"));
        m.sym_vec = VEC;
        m.sym_cap_K = K;
    }
    if (K > m.sym_cap_K) {
        LAMCHK(symv_dev_partials(c, m.sym, SS, sizeof(TV), K, s.stream));
        m.sym_cap_K = K;
    }
    return 0;
}

template <typename TA, typename TV, int K>
int multi_sym_launch(lam_hip_ctx *c, const TV *P, TV *Y, double *partial, const MultiScalars *sc, const double *shift)
{
    MultiState &m = c->multi;
    ShardBase &s = c->sh[0];
    c->symv_many_effective = false;
    LAMCHK((multi_sym_ensure<TA, TV>(c, K)));
    constexpr int SS = kBlock * MatVec<TA>::N;
    constexpr unsigned lds_pad = symv_lds_pad<TV, K>();
    hipLaunchKernelGGL((symv_many_task_kernel<TA, TV, K>), dim3(m.sym.ntasks), dim3(kBlock), lds_pad, s.stream,
                       (const TA *)s.A, P, (const SymvTask *)m.sym.tasks, (TV *)m.sym.rowpart, (TV *)m.sym.colpart, c->lda, c->ncols_vec(),
                       c->n, sc);
    LAUNCHED(c);
    ShiftArg<TV> sa;
    for (int j = 0; j < kSymvManyMaxK; j++) sa.s[j] = shift ? (TV)shift[j] : (TV)0;
    hipLaunchKernelGGL((shift ? symv_many_reduce_kernel<TV, SS, K, true> : symv_many_reduce_kernel<TV, SS, K, false>), dim3(multi_sym_grid(c)),
                       dim3(kBlock), 0, s.stream, (const TV *)m.sym.rowpart, (const TV *)m.sym.colpart, (const uint32_t *)m.sym.index, m.sym.ix,
                       P, Y, partial, c->n, sa, sc);
    LAUNCHED(c);
    c->symv_many_effective = true;
    return 0;
}

// shift: null for the plain product of A (lam_hip_gemv_many*, and a batch without shifts: the SHIFT = false instantiation, the only
// one there was), else the K shifts of the batch (MultiState::shift): Y_j = (A + s_j I) P_j
// Under option "symmetric_many" (K <= 4) the launch site runs the two passes of the symmetric batched product instead
// (multi_sym_launch): one more launch, and ceil(n / 32) partials per column instead of multi_gemv_grid(c) -- multi_product_blocks.
// Under option "packed_many" (fp64, K <= 4, the symmetric batched product not wanted: that one reads half the bytes and wins) and an
// image of the current content, multi_gemv_packed_kernel runs in place of multi_gemv_kernel: the same grid, partials and bits.
template <typename TA, typename TV, int K>
int multi_launch_gemv(lam_hip_ctx *c, const TV *P, TV *Y, double *partial, const MultiScalars *sc, const double *shift = nullptr)
{
    ShardBase &s = c->sh[0];
    c->packed_many_effective = false;
    if constexpr (K <= kSymvManyMaxK)
        if (multi_sym_wanted(c, K)) return multi_sym_launch<TA, TV, K>(c, P, Y, partial, sc, shift);
    c->symv_many_effective = false;
    MultiGemvArgs<TA, TV> a;
    a.A = (const TA *)s.A; a.p = P; a.y = Y; a.partial = partial; a.sc = sc;
    a.nrows = c->n; a.ncols = c->ncols_vec(); a.lda = c->lda;
    for (int j = 0; j < kMaxRhs; j++) a.shift[j] = shift ? (TV)shift[j] : (TV)0;
    if constexpr (std::is_same<TA, double>::value && K <= (int)kPackManyMaxK) {
        if (c->pack_many_eligible()) {
            const PackState &pk = c->pack;
            if (pack_many_reads(c, K) && c->n == pk.nrows) {
                const PackLayout L = pack_layout(pk.nrows, pk.ntiles);
                PackedMat m;
                m.data = (const unsigned char *)pk.buf + L.data;
                m.exc = (const double *)((const char *)pk.buf + L.exc);
                m.hdr = (const uint32_t *)((const char *)pk.buf + L.hdr);
                m.ntiles = (uint32_t)pk.ntiles;
                const dim3 grid(multi_gemv_grid(c)), block(kMultiWaves * 64);
                if (shift) {
                    if (c->opt_nt) hipLaunchKernelGGL((multi_gemv_packed_kernel<K, true, true>), grid, block, 0, s.stream, a, m);
                    else hipLaunchKernelGGL((multi_gemv_packed_kernel<K, false, true>), grid, block, 0, s.stream, a, m);
                } else {
                    if (c->opt_nt) hipLaunchKernelGGL((multi_gemv_packed_kernel<K, true, false>), grid, block, 0, s.stream, a, m);
                    else hipLaunchKernelGGL((multi_gemv_packed_kernel<K, false, false>), grid, block, 0, s.stream, a, m);
                }
                LAUNCHED(c);
                c->packed_many_effective = true;
                return 0;
            }
            pack_count_plain(c);
        }
    }
    if (shift)
        hipLaunchKernelGGL((multi_gemv_kernel<TA, TV, K, kMultiRows, kMultiWaves, true, true>), dim3(multi_gemv_grid(c)),
                           dim3(kMultiWaves * 64), 0, s.stream, a);
    else
        hipLaunchKernelGGL((multi_gemv_kernel<TA, TV, K, kMultiRows, kMultiWaves, true>), dim3(multi_gemv_grid(c)), dim3(kMultiWaves * 64), 0,
                           s.stream, a);
    LAUNCHED(c);
    return 0;
}

// host layout (column j contiguous at host + j * n) -> interleaved device vector `dst` of instantiation K, padding columns zero
int multi_upload(lam_hip_ctx *c, int nrhs, int K, const void *host, void *dst)
{
    MultiState &m = c->multi;
    ShardBase &s = c->sh[0];
    HIPCHK(c, hipMemcpyAsync(m.stage, host, (size_t)nrhs * c->n * c->esz_v(), hipMemcpyHostToDevice, s.stream));
    return multi_dispatch(c, K, [&](auto impl, auto kc) -> int {
        using TV = typename ImplTraits<decltype(impl)>::TV;
        constexpr int KK = decltype(kc)::value;
        hipLaunchKernelGGL((multi_interleave_kernel<TV, KK>), dim3(vec_grid(c->n)), dim3(kBlock), 0, s.stream, (const TV *)m.stage, nrhs,
                           (TV *)dst, c->n);
        HIPCHK(c, hipGetLastError());
        return 0;
    });
}
int multi_download(lam_hip_ctx *c, int nrhs, int K, const void *src, void *host)
{
    MultiState &m = c->multi;
    ShardBase &s = c->sh[0];
    LAMCHK(multi_dispatch(c, K, [&](auto impl, auto kc) -> int {
        using TV = typename ImplTraits<decltype(impl)>::TV;
        constexpr int KK = decltype(kc)::value;
        hipLaunchKernelGGL((multi_deinterleave_kernel<TV, KK>), dim3(vec_grid(c->n)), dim3(kBlock), 0, s.stream, (const TV *)src, nrhs,
                           (TV *)m.stage, c->n);
        HIPCHK(c, hipGetLastError());
        return 0;
    }));
    HIPCHK(c, hipMemcpyAsync(host, m.stage, (size_t)nrhs * c->n * c->esz_v(), hipMemcpyDeviceToHost, s.stream));
    HIPCHK(c, hipStreamSynchronize(s.stream));
    return 0;
}

// P = X ([n][K]: the batch's last solution, or a group of the multi-shift one), ready for the product: the rows behind row n zero in
// this K's layout (X's are not kept so)
int multi_stage_solution(lam_hip_ctx *c, const void *X, int K)
{
    MultiState &m = c->multi;
    ShardBase &s = c->sh[0];
    const size_t ev = c->esz_v(), body = (size_t)c->n * K * ev;
    HIPCHK(c, hipMemcpyAsync(m.P, X, body, hipMemcpyDeviceToDevice, s.stream));
    HIPCHK(c, hipMemsetAsync((char *)m.P + body, 0, (size_t)kMultiPadRows * K * ev, s.stream));
    return 0;
}

// The one reader of shifts: out[j] = sigma[j] as the vector dtype holds it, j < count (the caller has zeroed the rest).  Every shift
// must be finite, in the vector dtype too, and unless allow_negative (MINRES alone) >= 0.
struct ShiftsRead {
    bool any = false;        // some shift != 0
    double min = 0.0;        // the smallest one
};
int multi_read_shifts(lam_hip_ctx *c, const char *fn, int count, const double *sigma, bool allow_negative, double *out, ShiftsRead *read)
{
    for (int j = 0; j < count; j++) {
        const double r = to_vec_dtype(c, sigma[j]);
        if ((!allow_negative && !(sigma[j] >= 0.0)) || !std::isfinite(sigma[j]) || !std::isfinite(r))
            return fail(c, LAM_HIP_EINVAL, allow_negative ? "%s: shift %d is %g: every shift must be finite, in the vector dtype too"
                                                          : "%s: shift %d is %g: every shift must be finite and >= 0, in the vector dtype too",
                        fn, j, sigma[j]);
        out[j] = r;
        read->any = read->any || r != 0.0;
        read->min = j == 0 ? r : std::min(read->min, r);
    }
    return 0;
}

// one element of the context's dtype (fp64 / fp32: matrix and vectors alike) on the device, as a double
int read_element(lam_hip_ctx *c, const void *base, uint64_t index, double *value)
{
    double v64 = 0.0;
    float v32 = 0.f;
    const bool f64 = c->dtype == LAM_HIP_F64;
    HIPCHK(c, hipMemcpy(f64 ? (void *)&v64 : (void *)&v32, (const char *)base + index * c->esz_v(), c->esz_v(), hipMemcpyDeviceToHost));
    *value = f64 ? v64 : (double)v32;
    return 0;
}

// The diagonal scans' host protocol: `launch` enqueues the one kernel that builds the reciprocals and scans them for elements that
// cannot be inverted; the host reads a count and the first such element's index -- never the n values.
template <typename L>
int pcg_scan(lam_hip_ctx *c, DiagInfo *found, L &&launch)
{
    ShardBase &s = c->sh[0];
    found->first_bad = ~0ull; found->count = 0;
    HIPCHK(c, hipMemcpyAsync(c->pcg.info, found, sizeof *found, hipMemcpyHostToDevice, s.stream));
    HIPCHK(c, hipStreamSynchronize(s.stream));      // *found is pageable
    LAMCHK(launch());
    HIPCHK(c, hipMemcpyAsync(found, c->pcg.info, sizeof *found, hipMemcpyDeviceToHost, s.stream));
    HIPCHK(c, hipStreamSynchronize(s.stream));
    return 0;
}

// diag / dinv of the matrix held now: one launch over the n diagonal elements of the pitched matrix, once per matrix content
// (matrix_gen); for the message the first bad row's value.
int pcg_extract_diagonal(lam_hip_ctx *c)
{
    PcgState &g = c->pcg;
    if (g.diag_gen == c->matrix_gen) return 0;
    ShardBase &s = c->sh[0];
    DiagInfo h;
    LAMCHK(pcg_scan(c, &h, [&]() -> int {
        return multi_dispatch(c, 1, [&](auto impl, auto) -> int {
            using TA = typename ImplTraits<decltype(impl)>::TA;
            using TV = typename ImplTraits<decltype(impl)>::TV;
            hipLaunchKernelGGL((diag_extract_kernel<TA, TV>), dim3(vec_grid(c->n)), dim3(kBlock), 0, s.stream, (const TA *)s.A, c->lda,
                               (uint64_t)0, c->n, (TV *)g.diag, (TV *)g.dinv, g.info);
            HIPCHK(c, hipGetLastError());
            return 0;
        });
    }));
    g.bad_count = h.count;
    g.bad_row = h.first_bad;
    g.bad_value = 0.0;
    if (h.count != 0 && h.first_bad < c->n) LAMCHK(read_element(c, g.diag, h.first_bad, &g.bad_value));
    g.diag_gen = c->matrix_gen;
    return 0;
}

// dinv_k of the shifted batch, M_j = diag(A) + s_j I: one launch builds and scans it, once per (matrix content, K, nrhs, shifts); for
// the message the first bad (row, column) and that row's one diagonal element plus the column's shift.
int pcg_build_shifted(lam_hip_ctx *c)
{
    PcgState &g = c->pcg;
    MultiState &m = c->multi;
    if (g.dinvk_gen == c->matrix_gen && g.dinvk_K == m.K && g.dinvk_nrhs == m.nrhs && !memcmp(g.dinvk_shift, m.shift, sizeof m.shift))
        return 0;
    ShardBase &s = c->sh[0];
    g.dinvk_gen = ~0ull;
    // K times the shared dinv: allocated by the first shifted Jacobi solve only, released with the rest (multi_release)
    if (!g.dinv_k) HIPCHK(c, hipMalloc(&g.dinv_k, c->n * kMaxRhs * c->esz_v()));
    ShiftList sl;
    for (int j = 0; j < kMaxRhs; j++) sl.s[j] = m.shift[j];
    DiagInfo h;
    LAMCHK(pcg_scan(c, &h, [&]() -> int {
        return multi_dispatch(c, m.K, [&](auto impl, auto kc) -> int {
            using TA = typename ImplTraits<decltype(impl)>::TA;
            using TV = typename ImplTraits<decltype(impl)>::TV;
            hipLaunchKernelGGL((shifted_dinv_kernel<TA, TV, decltype(kc)::value>), dim3(vec_grid(c->n)), dim3(kBlock), 0, s.stream,
                               (const TA *)s.A, c->lda, c->n, m.nrhs, sl, (TV *)g.dinv_k, g.info);
            HIPCHK(c, hipGetLastError());
            return 0;
        });
    }));
    g.badk_count = h.count;
    g.badk_row = 0; g.badk_col = 0; g.badk_value = 0.0;
    if (h.count != 0 && h.first_bad / m.K < c->n) {
        g.badk_row = h.first_bad / m.K;
        g.badk_col = (int)(h.first_bad % m.K);
        double a = 0.0;
        LAMCHK(read_element(c, s.A, g.badk_row * c->lda + g.badk_row, &a));
        g.badk_value = to_vec_dtype(c, a + m.shift[g.badk_col]);
    }
    g.dinvk_gen = c->matrix_gen;
    g.dinvk_K = m.K; g.dinvk_nrhs = m.nrhs;
    memcpy(g.dinvk_shift, m.shift, sizeof m.shift);
    return 0;
}

// The true residual's tail, of the batch and of a multi-shift group alike: X ([n][K]) staged in P, one product under the columns'
// shifts, one K-wide pass over B and the product (`residual`: the caller's kernel -- K right-hand sides, or the one b of the
// multi-shift solve), one workgroup for the K quotients, which reach res[0 .. K).  B and X are left alone; P, AP, the partials and
// MultiState::res are scratch, as they are between any two solves.
template <typename TA, typename TV, int K, typename RK>
int multi_residual_tail(lam_hip_ctx *c, const void *X, const double *shift, RK residual, double *res)
{
    MultiState &m = c->multi;
    ShardBase &s = c->sh[0];
    const int vb = vec_grid(c->n);
    LAMCHK(multi_stage_solution(c, X, K));
    LAMCHK(pack_many_maybe(c, K));
    LAMCHK((multi_launch_gemv<TA, TV, K>(c, (const TV *)m.P, (TV *)m.AP, nullptr, nullptr, shift)));
    hipLaunchKernelGGL(residual, dim3(vb), dim3(kBlock), 0, s.stream, (const TV *)m.B, (const TV *)m.AP, c->n, m.part_rr, m.part_vec);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL((multi_residual_scalars_kernel<K>), dim3(1), dim3(kBlock), 0, s.stream, (const double *)m.part_rr,
                       (const double *)m.part_vec, vb, m.res);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(res, m.res, sizeof(double) * K, hipMemcpyDeviceToHost, s.stream));
    HIPCHK(c, hipStreamSynchronize(s.stream));
    return 0;
}

// the timed products of one solve (option "gemv_timing"), as multi_drive harvested them
struct BatchTiming {
    double gemv_ms = 0.0;
    int samples = 0;
};

void multi_harvest(MultiState &m, int slot, BatchTiming *t)
{
    if (!m.timed_slot[slot]) return;
    m.timed_slot[slot] = false;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, m.ev0[slot], m.ev1[slot]) != hipSuccess) { (void)hipGetLastError(); return; }
    t->gemv_ms += ms;
    t->samples++;
}

// algorithmic bytes of the product launch of instantiation K as it last ran: the product launch alone, with or without the
// preconditioner (the diagonal is read by the two vector launches); under the symmetric batched product the upper triangle once, the
// vectors as before, the K-wide partials written and read
double multi_gemv_bytes(const lam_hip_ctx *c, int K)
{
    const MultiState &m = c->multi;
    if (c->symv_many_effective)
        return (double)c->esz_a() * ((double)c->n * ((double)c->n + 1.0) / 2.0) + (double)c->esz_v() * 2.0 * (double)K * (double)c->n +
               2.0 * (double)c->esz_v() * (double)K *
                   ((double)m.sym.rowpart_elems + (double)m.sym.ntasks * (double)kBlock * (16.0 / (double)c->esz_a()));
    // the image: its elements, headers and max(count, 64) values of every list, each once (what a visit that starts inside a unit
    // re-reads of its list, header and middle / high bytes is overhead, not counted -- as p, which every workgroup re-reads, is counted once)
    if (c->packed_many_effective)
        return (double)c->pack.nrows * (double)c->pack.ntiles * (double)(kPackTileBytes + 4) + 8.0 * (double)c->pack.exc_total +
               8.0 * 2.0 * (double)K * (double)c->n;
    return(double)c->esz_a() * (double)c->n * (double)c->n + (double)c->esz_v() * 2.0 * (double)K * (double)c->n;
}

// what a batched solve reports, CG or MINRES: the per-column arrays and the batch's stats from the scalars' prefix as the host read
// it back; rel_of(j, col) is column j's rel_err (CG: from its r.r ring; MINRES: its own word)
template <typename F>
void multi_report(lam_hip_ctx *c, const MultiScalars &h, F &&rel_of, double t0, double t1, const BatchTiming &timing, lam_hip_stats *st,
                  int32_t *num_iters, int32_t *converged, double *rel_err)
{
    const MultiState &m = c->multi;
    int ran = 0, batch_iters = 0, all_conv = 1;
    double worst = 0.0;
    bool any_nan = false;
    for (int j = 0; j < m.nrhs; j++) {
        const CgScalars &sc = h.col[j];
        const int ni = sc.stop ? sc.iters : sc.iters + 1;
        const double re = rel_of(j, sc);
        if (num_iters) num_iters[j] = ni;
        if (converged) converged[j] = sc.stop != 0;
        if (rel_err) rel_err[j] = re;
        ran = std::max(ran, sc.iters);
        batch_iters = std::max(batch_iters, ni);
        all_conv = all_conv && sc.stop != 0;
        if (re != re) any_nan = true; else worst = std::max(worst, re);
    }
    if (st) {
        memset(st, 0, sizeof *st);
        st->num_iters = batch_iters;
        st->converged = all_conv;
        st->rel_err = any_nan ? std::nan("") : worst;
        st->t_total = t1 - t0;
        st->t_iter = ran > 0 ? (t1 - t0) / ran : 0.0;
        st->t_gemv = timing.samples > 0 ? timing.gemv_ms * 1e-3 / timing.samples : 0.0;
        st->t_comm_init = c->t_comm_init;
        st->gemv_bytes = multi_gemv_bytes(c, m.K);
    }
}

// ---- driver ----------------------------------------------------------------------------------------------------------------
// The enqueue loop of every batched solve, CG and MINRES.  The product of iteration k is the driver's: out = (A + s_j I) in under the
// columns' shifts (null: none), its p.Ap partials and `sc` as in multi_launch_gemv, timed under option "gemv_timing".  The caller's
// are init(), its uncounted launches in front of the loop -- behind the reset of the progress word, into which the init launch posts
// --, and rest(k), the counted vector launches behind the product of iteration k.  Returns with the stream drained.
template <typename TA, typename TV, int K, typename Init, typename Rest>
int multi_drive(lam_hip_ctx *c, int max_iters, const TV *in, TV *out, const MultiScalars *sc, const double *shift, Init &&init, Rest &&rest,
                BatchTiming *timing)
{
    MultiState &m = c->multi;
    ShardBase &s0 = c->sh[0];
    m.host_flags[0] = m.host_flags[1] = 0;
    for (int i = 0; i < kLag; i++) m.timed_slot[i] = false;
    c->prog_t = 0.0;
    m.last_K = m.K;
    // the lag rule reads the batch's own progress word: the single solve's helpers on a view that carries it
    ShardBase view;
    view.dev = s0.dev; view.stream = s0.stream; view.host_flags = m.host_flags;
    LAMCHK(init());
    int enq = 0;
    for (int i = 0; i < max_iters; i++) {
        const int k = i + 1, slot = i % kLag;
        if (i >= kLag) {
            const int d = lag_check(c, view, k);
            if (d < 0) return d;
            if (d != 0) break;
            multi_harvest(m, slot, timing);
        }
        LAMCHK(pack_many_maybe(c, K));          // option "packed_many": in front of the product step, outside its event pair
        const double te = now_s();
        const bool timed = timed_iteration(c, s0, k);
        m.timed_slot[slot] = timed;
        if (timed) RECORD(c, m.ev0[slot], s0.stream);
        LAMCHK((multi_launch_gemv<TA, TV, K>(c, in, out, m.part_gemv, sc, shift)));
        if (timed) RECORD(c, m.ev1[slot], s0.stream);
        LAMCHK(rest(k));
        c->enqueue_ns += (uint64_t)((now_s() - te) * 1e9);
        enq++;
    }
    if (enq > 0) {
        Progress pr;
        LAMCHK(await_progress(c, view, enq, &pr, /*precise=*/true));
    }
    HIPCHK(c, hipStreamSynchronize(s0.stream));
    for (int j = 0; j < kLag; j++) multi_harvest(m, j, timing);
    return 0;
}

// ---- solves ----------------------------------------------------------------------------------------------------------------
// what every batched solve checks first, in this order (MINRES has no preconditioner: LAM_HIP_PC_NONE)
int multi_solve_checks(lam_hip_ctx *c, const char *fn, int precond, int max_iters)
{
    LAMCHK(multi_supported(c, fn));
    if (precond != LAM_HIP_PC_NONE && precond != LAM_HIP_PC_JACOBI)
        return fail(c, LAM_HIP_EINVAL, "%s: unknown preconditioner %d (LAM_HIP_PC_NONE, LAM_HIP_PC_JACOBI)", fn, precond);
    if (max_iters < 0) return fail(c, LAM_HIP_EINVAL, "max_iters must be >= 0");
    if (!c->have_matrix || !c->multi.have_rhs || c->multi.n != c->n)
        return fail(c, LAM_HIP_ESTATE, "matrix and right-hand sides (lam_hip_set_rhs_many) must be set before %s", fn);
    return 0;
}

// where a batched solve starts: x = 0, a guess given on the host, the batch's own last solution, or the deflated start vector
// x0 = W (W^T A W)^-1 W^T b built on the device (lam_hip_solve_many_deflated)
enum MultiGuess { kGuessNone, kGuessHost, kGuessCurrent, kGuessDeflated };

// lam_deflate.h: the two launches of the deflated start vector (into P) and of p -= W Ginv (AW)^T r (counted: inside the iteration)
template <typename TV, int K> int deflate_start(lam_hip_ctx *c);
template <typename TV, int K> int deflate_project(lam_hip_ctx *c, bool counted);

// lam_hip_solve_many (precond = LAM_HIP_PC_NONE), lam_hip_solve_many_pc and lam_hip_solve_many_x0: one body, one sequence of
// launches.  The Jacobi-preconditioned batch runs the PC = true instantiations of the four vector kernels on dinv and a second
// partial array (both null for the plain batch); the scalars' block and the per-column results are shared.  A start from a guess
// stages the guess in P (whose rows behind row n the product needs zero; the upload and multi_stage_solution see to that), forms
// A x0 in AP with one more product launch and runs the GUESS = true instantiations of the two init kernels.
// mshift (lam_hip_solve_mshift only, null for every other entry point): the multi-shift state the K = 1 seed batch drives -- one init
// launch in front of the loop and one step launch behind every multi_p_kernel; nothing else changes, the seed's progress word decides.
// guess == kGuessDeflated (lam_hip_solve_many_deflated only): the guess is built in P by deflate_start, and deflate_project's two
// launches follow the init launches and every multi_p_kernel; the three launches of the plain batch are the ones they were.
int multi_solve(lam_hip_ctx *c, const char *fn, int precond, MultiGuess guess, const void *x0_host, int max_iters, double rel_error,
                lam_hip_stats *st, int32_t *num_iters, int32_t *converged, double *rel_err, MshiftState *mshift = nullptr)
{
    LAMCHK(multi_solve_checks(c, fn, precond, max_iters));
    const bool pc = precond == LAM_HIP_PC_JACOBI;
    MultiState &m = c->multi;
    if (guess == kGuessCurrent && !m.solved)
        return fail(c, LAM_HIP_ESTATE, "%s: x0_host is NULL and there is no batched solution to continue from (lam_hip_solve_many)", fn);
    // only lam_hip_solve_many_minres leaves a negative shift in force; nothing is touched, the batched solution stays readable
    for (int j = 0; j < m.nrhs; j++)
        if (m.shift[j] < 0.0)
            return fail(c, LAM_HIP_EINVAL, "%s: shift %d in force is %g: CG needs every shift >= 0 (a negative one can make the matrix "
                        "indefinite); use lam_hip_solve_many_minres, or replace the shifts (lam_hip_set_shifts_many)", fn, j, m.shift[j]);
    const double t0 = now_s();
    ShardBase &s0 = c->sh[0];
    LAMCHK(set_dev(c, s0));
    HIPCHK(c, hipStreamSynchronize(s0.stream));
    PcgState &g = c->pcg;
    m.solved = false;            // whatever follows, a refusal of the diagonal included, leaves no batched solution behind
    m.ms.valid = false;          // and the batch's vectors are no longer the seed's of a multi-shift solve
    const bool dk = pc && m.shifted;             // M_j = diag(A) + s_j I: the K-wide reciprocal
    const double *const shift = m.shifted ? m.shift : nullptr;
    if (dk) {
        LAMCHK(pcg_ensure(c));
        LAMCHK(pcg_build_shifted(c));
        if (g.badk_count != 0)
            return fail(c, LAM_HIP_EINVAL, "%s: the Jacobi preconditioner needs A[i][i] + shift[j] and its reciprocal finite and > 0: "
                        "row %llu, column %d holds %g (%llu such elements)", fn, (unsigned long long)g.badk_row, g.badk_col, g.badk_value,
                        (unsigned long long)g.badk_count);
    } else if (pc) {
        LAMCHK(pcg_ensure(c));
        LAMCHK(pcg_extract_diagonal(c));
        if (g.bad_count != 0)
            return fail(c, LAM_HIP_EINVAL, "%s: the Jacobi preconditioner needs A[i][i] and 1/A[i][i] finite and > 0: row %llu holds %g "
                        "(%llu such rows)", fn, (unsigned long long)g.bad_row, g.bad_value, (unsigned long long)g.bad_count);
    }
    const int vb = vec_grid(c->n), gb = multi_product_blocks(c, m.K);
    BatchTiming timing;
    LAMCHK(multi_dispatch(c, m.K, [&](auto impl, auto kc, auto form) -> int {
        using I = decltype(impl);
        using TA = typename ImplTraits<I>::TA;
        using TV = typename ImplTraits<I>::TV;
        constexpr int K = decltype(kc)::value;
        constexpr bool PC = decltype(form)::PC, GUESS = decltype(form)::GUESS, DK = decltype(form)::DK;
        const TV *const dinv = PC ? (const TV *)(DK ? g.dinv_k : g.dinv) : nullptr;
        double *const part_rz = PC ? g.part_rz : nullptr;
        double *const part_rr = GUESS ? m.part_rr : nullptr;
        const int sgroups = mshift ? mshift_groups(mshift->nshifts) : 0;
        auto init = [&]() -> int {
            if (guess == kGuessHost) LAMCHK(multi_upload(c, m.nrhs, m.K, x0_host, m.P));
            if (guess == kGuessCurrent) LAMCHK(multi_stage_solution(c, m.X, m.K));
            if (guess == kGuessDeflated) LAMCHK((deflate_start<TV, K>(c)));
            // GUESS: AP = A x0 ((A + s_j I) x0 of a shifted batch) of the guess staged in P, outside the iteration's scalars and partials
            if (GUESS) LAMCHK(pack_many_maybe(c, K));
            if (GUESS) LAMCHK((multi_launch_gemv<TA, TV, K>(c, (const TV *)m.P, (TV *)m.AP, nullptr, nullptr, shift)));
            // x = 0, r = b, p = b, bb_j = b_j.b_j  (PC: p = dinv o b, rz_j = b_j.(dinv o b_j));  GUESS: x = x0, r = b - A x0, p = r,
            // rr_j = r_j.r_j next to bb_j  (PC: p = dinv o r, rz_j = r_j.(dinv o r_j))
            hipLaunchKernelGGL((multi_init_kernel<TV, K, PC, GUESS, DK>), dim3(vb), dim3(kBlock), 0, s0.stream, (const TV *)m.B, (TV *)m.X,
                               (TV *)m.R, (TV *)m.P, c->n, m.part_vec, dinv, part_rz, (const TV *)(GUESS ? m.AP : nullptr), part_rr);
            HIPCHK(c, hipGetLastError());
            hipLaunchKernelGGL((multi_init_scalars_kernel<K, PC, GUESS>), dim3(1), dim3(kBlock), 0, s0.stream, (const double *)m.part_vec, vb,
                               m.nrhs, m.sc, (volatile int *)m.host_flags, (const double *)part_rz, (const double *)part_rr, rel_error);
            HIPCHK(c, hipGetLastError());
            if (mshift) {
                MshiftList dl;
                for (int j = 0; j < kMaxShifts; j++) dl.d[j] = j < mshift->nshifts ? mshift->shift[j] - m.shift[0] : 0.0;
                hipLaunchKernelGGL((mshift_init_kernel<TV, kShiftGroup>), dim3(vb, sgroups), dim3(kBlock), 0, s0.stream, (const TV *)m.B,
                                   (TV *)mshift->XS, (TV *)mshift->PS, c->n, mshift->nshifts, dl, mshift->sc);
                HIPCHK(c, hipGetLastError());
            }
            if (guess == kGuessDeflated) LAMCHK((deflate_project<TV, K>(c, false)));
            return 0;
        };
        auto rest = [&](int k) -> int {
            hipLaunchKernelGGL((multi_xr_kernel<TV, K, PC, DK>), dim3(vb), dim3(kBlock), 0, s0.stream, (const double *)m.part_gemv, gb, m.sc, k,
                               (const TV *)m.P, (const TV *)m.AP, (TV *)m.X, (TV *)m.R, c->n, m.part_vec, dinv, part_rz);
            LAUNCHED(c);
            hipLaunchKernelGGL((multi_p_kernel<TV, K, PC, DK>), dim3(vb), dim3(kBlock), 0, s0.stream, (const double *)m.part_vec, vb, m.sc, k,
                               rel_error, (const TV *)m.R, (TV *)m.P, c->n, (volatile int *)m.host_flags, dinv, (const double *)part_rz);
            LAUNCHED(c);
            if (mshift) {
                hipLaunchKernelGGL((mshift_step_kernel<TV, kShiftGroup>), dim3(vb, sgroups), dim3(kBlock), 0, s0.stream,
                                   (const MultiScalars *)m.sc, mshift->sc, k, rel_error, (const TV *)m.R, (TV *)mshift->XS,
                                   (TV *)mshift->PS, c->n);
                LAUNCHED(c);
            }
            if (guess == kGuessDeflated) LAMCHK((deflate_project<TV, K>(c, true)));
            return 0;
        };
        return multi_drive<TA, TV, K>(c, max_iters, (const TV *)m.P, (TV *)m.AP, m.sc, shift, init, rest, &timing);
    }, pc, guess != kGuessNone, dk));
    HIPCHK(c, hipMemcpyAsync(m.sc_host, m.sc, sizeof(MultiScalars), hipMemcpyDeviceToHost, s0.stream));
    HIPCHK(c, hipStreamSynchronize(s0.stream));
    m.solved = true;
    multi_report(c, *m.sc_host, [](int, const CgScalars &sc) { return std::sqrt(sc.rr[sc.iters & 1] / sc.bb); }, t0, now_s(), timing, st,
                 num_iters, converged, rel_err);
    return 0;
}

// lam_hip_solve_many_minres: K MINRES recurrences around the batch's product launch, with V (the batch's P) as its input, on
// MINRES' own vector launches and scalars' block (MinresState).  Shifts of either sign; sigma null keeps the shifts in force.
int minres_solve(lam_hip_ctx *c, const char *fn, const double *sigma, int max_iters, double rel_error, lam_hip_stats *st,
                 int32_t *num_iters, int32_t *converged, double *rel_err)
{
    LAMCHK(multi_solve_checks(c, fn, LAM_HIP_PC_NONE, max_iters));
    MultiState &m = c->multi;
    double s[kMaxRhs] = {};
    ShiftsRead read;
    if (sigma) LAMCHK(multi_read_shifts(c, fn, m.nrhs, sigma, /*allow_negative=*/true, s, &read));
    const double t0 = now_s();
    ShardBase &s0 = c->sh[0];
    LAMCHK(set_dev(c, s0));
    HIPCHK(c, hipStreamSynchronize(s0.stream));
    // the lazy allocation first: if it fails, the shifts in force and the batched solution are what they were
    LAMCHK(minres_ensure(c));
    if (sigma) {
        memcpy(m.shift, s, sizeof s);
        m.shifted = read.any;
    }
    m.solved = false;
    m.ms.valid = false;
    MinresState &mr = m.mr;
    const int vb = vec_grid(c->n), gb = multi_product_blocks(c, m.K);
    BatchTiming timing;
    LAMCHK(multi_dispatch(c, m.K, [&](auto impl, auto kc) -> int {
        using I = decltype(impl);
        using TA = typename ImplTraits<I>::TA;
        using TV = typename ImplTraits<I>::TV;
        constexpr int K = decltype(kc)::value;
        TV *const V = (TV *)m.P, *const U = (TV *)m.AP, *const VOLD = (TV *)m.R, *const X = (TV *)m.X;
        TV *const W = (TV *)mr.W, *const WOLD = (TV *)mr.WOLD;
        auto init = [&]() -> int {
            hipLaunchKernelGGL((minres_init_kernel<TV, K>), dim3(vb), dim3(kBlock), 0, s0.stream, (const TV *)m.B, X, VOLD, W, WOLD, V, c->n,
                               m.part_vec);
            HIPCHK(c, hipGetLastError());
            hipLaunchKernelGGL((minres_init_scalars_kernel<K>), dim3(1), dim3(kBlock), 0, s0.stream, (const double *)m.part_vec, vb, m.nrhs,
                               mr.sc, (volatile int *)m.host_flags);
            HIPCHK(c, hipGetLastError());
            hipLaunchKernelGGL((minres_start_kernel<TV, K>), dim3(vb), dim3(kBlock), 0, s0.stream, (const TV *)m.B, V, c->n,
                               (const MinresScalars *)mr.sc);
            HIPCHK(c, hipGetLastError());
            return 0;
        };
        auto rest = [&](int k) -> int {
            hipLaunchKernelGGL((minres_lanczos_kernel<TV, K>), dim3(vb), dim3(kBlock), 0, s0.stream, (const double *)m.part_gemv, gb, mr.sc, k,
                               (const TV *)V, (const TV *)VOLD, U, c->n, m.part_vec);
            LAUNCHED(c);
            hipLaunchKernelGGL((minres_update_kernel<TV, K>), dim3(vb), dim3(kBlock), 0, s0.stream, (const double *)m.part_vec, vb, mr.sc, k,
                               rel_error, (const TV *)U, V, VOLD, W, WOLD, X, c->n, (volatile int *)m.host_flags);
            LAUNCHED(c);
            return 0;
        };
        return multi_drive<TA, TV, K>(c, max_iters, (const TV *)V, U, mr.sc, m.shifted ? m.shift : nullptr, init, rest, &timing);
    }));
    const std::unique_ptr<MinresScalars> h(new MinresScalars);
    HIPCHK(c, hipMemcpyAsync(h.get(), mr.sc, sizeof(MinresScalars), hipMemcpyDeviceToHost, s0.stream));
    HIPCHK(c, hipStreamSynchronize(s0.stream));
    m.solved = true;
    multi_report(c, *h, [&](int j, const CgScalars &) { return h->rel_err[j]; }, t0, now_s(), timing, st, num_iters, converged, rel_err);
    return 0;
}

}  // namespace

// ---- entry points ----------------------------------------------------------------------------------------------------------
extern "C" {

int lam_hip_set_rhs_many(lam_hip_ctx *c, int nrhs, const void *b_host)
{
    if (!c) return LAM_HIP_EINVAL;
    LAMCHK(multi_supported(c, "lam_hip_set_rhs_many"));
    LAMCHK(multi_check_nrhs(c, "lam_hip_set_rhs_many", nrhs));
    if (!b_host) return fail(c, LAM_HIP_EINVAL, "lam_hip_set_rhs_many: b_host is NULL");
    if (!c->have_problem) return fail(c, LAM_HIP_ESTATE, "call lam_hip_set_problem first");
    LAMCHK(multi_ensure(c));
    MultiState &m = c->multi;
    m.have_rhs = m.solved = m.ms.valid = false;
    multi_clear_shifts(m);
    const int K = multi_k_for(nrhs);
    LAMCHK(multi_upload(c, nrhs, K, b_host, m.B));
    HIPCHK(c, hipStreamSynchronize(c->sh[0].stream));
    m.nrhs = nrhs; m.K = K;
    m.have_rhs = true;
    return 0;
}

// No launch and no device traffic: the shifts travel by value in the product's arguments.  The batched solution, if there is one,
// stays readable and lam_hip_solve_many_x0(..., NULL, ...) continues from it under the new shifts.
int lam_hip_set_shifts_many(lam_hip_ctx *c, int nrhs, const double *sigma)
{
    if (!c) return LAM_HIP_EINVAL;
    LAMCHK(multi_supported(c, "lam_hip_set_shifts_many"));
    LAMCHK(multi_check_nrhs(c, "lam_hip_set_shifts_many", nrhs));
    MultiState &m = c->multi;
    if (!m.have_rhs || m.n != c->n)
        return fail(c, LAM_HIP_ESTATE, "right-hand sides (lam_hip_set_rhs_many) must be set before lam_hip_set_shifts_many");
    if (nrhs != m.nrhs) return fail(c, LAM_HIP_EINVAL, "lam_hip_set_shifts_many: nrhs = %d, but %d right-hand sides are set", nrhs, m.nrhs);
    if (!sigma) { multi_clear_shifts(m); return 0; }
    double s[kMaxRhs] = {};
    ShiftsRead read;
    LAMCHK(multi_read_shifts(c, "lam_hip_set_shifts_many", nrhs, sigma, /*allow_negative=*/false, s, &read));
    memcpy(m.shift, s, sizeof s);
    m.shifted = read.any;
    return 0;
}

int lam_hip_solve_many(lam_hip_ctx *c, int max_iters, double rel_error, lam_hip_stats *st, int32_t *num_iters, int32_t *converged,
                       double *rel_err)
{
    if (!c) return LAM_HIP_EINVAL;
    return multi_solve(c, "lam_hip_solve_many", LAM_HIP_PC_NONE, kGuessNone, nullptr, max_iters, rel_error, st, num_iters, converged, rel_err);
}

int lam_hip_solve_many_pc(lam_hip_ctx *c, int precond, int max_iters, double rel_error, lam_hip_stats *st, int32_t *num_iters,
                          int32_t *converged, double *rel_err)
{
    if (!c) return LAM_HIP_EINVAL;
    return multi_solve(c, "lam_hip_solve_many_pc", precond, kGuessNone, nullptr, max_iters, rel_error, st, num_iters, converged, rel_err);
}

int lam_hip_solve_many_x0(lam_hip_ctx *c, int precond, const void *x0_host, int max_iters, double rel_error, lam_hip_stats *st,
                          int32_t *num_iters, int32_t *converged, double *rel_err)
{
    if (!c) return LAM_HIP_EINVAL;
    return multi_solve(c, "lam_hip_solve_many_x0", precond, x0_host ? kGuessHost : kGuessCurrent, x0_host, max_iters, rel_error, st,
                       num_iters, converged, rel_err);
}

int lam_hip_solve_many_minres(lam_hip_ctx *c, const double *sigma, int max_iters, double rel_error, lam_hip_stats *st, int32_t *num_iters,
                              int32_t *converged, double *rel_err)
{
    if (!c) return LAM_HIP_EINVAL;
    return minres_solve(c, "lam_hip_solve_many_minres", sigma, max_iters, rel_error, st, num_iters, converged, rel_err);
}

int lam_hip_true_residual_many(lam_hip_ctx *c, int nrhs, double *rel_res)
{
    if (!c) return LAM_HIP_EINVAL;
    LAMCHK(multi_supported(c, "lam_hip_true_residual_many"));
    LAMCHK(multi_check_nrhs(c, "lam_hip_true_residual_many", nrhs));
    if (!rel_res) return fail(c, LAM_HIP_EINVAL, "lam_hip_true_residual_many: rel_res is NULL");
    MultiState &m = c->multi;
    if (!m.solved || !m.have_rhs || m.n != c->n) return fail(c, LAM_HIP_ESTATE, "no batched solution yet (lam_hip_solve_many)");
    if (nrhs > m.nrhs) return fail(c, LAM_HIP_EINVAL, "lam_hip_true_residual_many: %d columns asked, %d were solved", nrhs, m.nrhs);
    LAMCHK(set_dev(c, c->sh[0]));
    double res[kMaxRhs];
    LAMCHK(multi_dispatch(c, m.K, [&](auto impl, auto kc) -> int {
        using I = decltype(impl);
        using TV = typename ImplTraits<I>::TV;
        constexpr int K = decltype(kc)::value;
        return multi_residual_tail<typename ImplTraits<I>::TA, TV, K>(c, m.X, m.shifted ? m.shift : nullptr, multi_residual_kernel<TV, K>, res);
    }));
    for (int j = 0; j < nrhs; j++) rel_res[j] = res[j];
    return 0;
}

// Single-process contexts, any number of shards, every storage type: each shard's device extracts its own rows' diagonal elements.
int lam_hip_get_diagonal(lam_hip_ctx *c, void *d_host)
{
    if (!c) return LAM_HIP_EINVAL;
    if (c->rank_mode) return fail(c, LAM_HIP_EINVAL, "lam_hip_get_diagonal: rank mode (lam_hip_create_rank) is not supported");
    if (!d_host) return fail(c, LAM_HIP_EINVAL, "lam_hip_get_diagonal: d_host is NULL");
    if (!c->have_matrix) return fail(c, LAM_HIP_ESTATE, "matrix not set");
    return dispatch(c, [&](auto impl) -> int {
        using TA = typename ImplTraits<decltype(impl)>::TA;
        using TV = typename ImplTraits<decltype(impl)>::TV;
        for (auto &s : c->sh) {      // no shard is empty: lam_hip_set_problem refuses n < shards
            LAMCHK(set_dev(c, s));
            DevBuf d;
            HIPCHK(c, hipMalloc(&d.p, s.nrows * sizeof(TV)));
            hipLaunchKernelGGL((diag_extract_kernel<TA, TV>), dim3(vec_grid(s.nrows)), dim3(kBlock), 0, s.stream, (const TA *)s.A, c->lda,
                               s.row0, s.nrows, d.as<TV>(), (TV *)nullptr, (DiagInfo *)nullptr);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipMemcpyAsync((TV *)d_host + s.row0, d.p, s.nrows * sizeof(TV), hipMemcpyDeviceToHost, s.stream));
            HIPCHK(c, hipStreamSynchronize(s.stream));
        }
        return 0;
    });
}

int lam_hip_get_solution_many(lam_hip_ctx *c, int nrhs, void *x_host)
{
    if (!c) return LAM_HIP_EINVAL;
    LAMCHK(multi_supported(c, "lam_hip_get_solution_many"));
    LAMCHK(multi_check_nrhs(c, "lam_hip_get_solution_many", nrhs));
    if (!x_host) return fail(c, LAM_HIP_EINVAL, "lam_hip_get_solution_many: x_host is NULL");
    MultiState &m = c->multi;
    if (!m.solved || m.n != c->n) return fail(c, LAM_HIP_ESTATE, "no batched solution yet (lam_hip_solve_many)");
    if (nrhs > m.nrhs) return fail(c, LAM_HIP_EINVAL, "lam_hip_get_solution_many: %d columns asked, %d were solved", nrhs, m.nrhs);
    LAMCHK(set_dev(c, c->sh[0]));
    return multi_download(c, nrhs, m.K, m.X, x_host);
}

int lam_hip_gemv_many(lam_hip_ctx *c, int nrhs, const void *x_host, void *y_host)
{
    if (!c) return LAM_HIP_EINVAL;
    LAMCHK(multi_supported(c, "lam_hip_gemv_many"));
    LAMCHK(multi_check_nrhs(c, "lam_hip_gemv_many", nrhs));
    if (!x_host || !y_host) return fail(c, LAM_HIP_EINVAL, "lam_hip_gemv_many: NULL vector");
    if (!c->have_matrix) return fail(c, LAM_HIP_ESTATE, "matrix not set");
    LAMCHK(multi_ensure(c));
    MultiState &m = c->multi;
    LAMCHK(set_dev(c, c->sh[0]));
    m.solved = m.ms.valid = false;      // P and AP of the batch are overwritten (B is not: a following lam_hip_solve_many starts from it)
    const int K = multi_k_for(nrhs);
    m.last_K = K;
    LAMCHK(multi_upload(c, nrhs, K, x_host, m.P));
    LAMCHK(pack_many_maybe(c, K));
    LAMCHK(multi_dispatch(c, K, [&](auto impl, auto kc) -> int {
        using I = decltype(impl);
        return multi_launch_gemv<typename ImplTraits<I>::TA, typename ImplTraits<I>::TV, decltype(kc)::value>(
            c, (const typename ImplTraits<I>::TV *)m.P, (typename ImplTraits<I>::TV *)m.AP, nullptr, nullptr);
    }));
    return multi_download(c, nrhs, K, m.AP, y_host);
}

int lam_hip_gemv_many_only(lam_hip_ctx *c, int nrhs, int reps, double *sec_per_product)
{
    if (!c) return LAM_HIP_EINVAL;
    LAMCHK(multi_supported(c, "lam_hip_gemv_many_only"));
    LAMCHK(multi_check_nrhs(c, "lam_hip_gemv_many_only", nrhs));
    if (!sec_per_product || reps < 1) return fail(c, LAM_HIP_EINVAL, "lam_hip_gemv_many_only: reps must be >= 1 and the result pointer set");
    if (!c->have_matrix) return fail(c, LAM_HIP_ESTATE, "matrix not set");
    LAMCHK(multi_ensure(c));
    MultiState &m = c->multi;
    ShardBase &s = c->sh[0];
    LAMCHK(set_dev(c, s));
    m.solved = m.ms.valid = false;
    const int K = multi_k_for(nrhs);
    m.last_K = K;
    LAMCHK(pack_many_maybe(c, K));
    LAMCHK(multi_dispatch(c, K, [&](auto impl, auto kc) -> int {
        using I = decltype(impl);
        using TA = typename ImplTraits<I>::TA;
        using TV = typename ImplTraits<I>::TV;
        constexpr int KK = decltype(kc)::value;
        // the product of a zero P: the time of a product does not depend on the vector's values, and the rows behind P's end
        // must be zero in this K's layout
        HIPCHK(c, hipMemsetAsync(m.P, 0, (size_t)(c->n + kMultiPadRows) * kMaxRhs * c->esz_v(), s.stream));
        LAMCHK((multi_launch_gemv<TA, TV, KK>(c, (const TV *)m.P, (TV *)m.AP, m.part_gemv, nullptr)));      // warm-up
        HIPCHK(c, hipEventRecord(m.ev0[0], s.stream));
        for (int i = 0; i < reps; i++) LAMCHK((multi_launch_gemv<TA, TV, KK>(c, (const TV *)m.P, (TV *)m.AP, m.part_gemv, nullptr)));
        HIPCHK(c, hipEventRecord(m.ev1[0], s.stream));
        return 0;
    }));
    HIPCHK(c, hipEventSynchronize(m.ev1[0]));
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, m.ev0[0], m.ev1[0]));
    *sec_per_product = (double)ms * 1e-3 / reps;
    return 0;
}

// The seed is the K = 1 batch on the smallest shift: lam_hip_set_rhs_many(1, b) + lam_hip_set_shifts_many(1, &s_min) +
// lam_hip_solve_many with the multi-shift hook, so the batch state afterwards is the seed's.
int lam_hip_solve_mshift(lam_hip_ctx *c, const void *b_host, int nshifts, const double *sigma, int max_iters, double rel_error,
                         lam_hip_stats *st, int32_t *num_iters, int32_t *converged, double *rel_err)
{
    if (!c) return LAM_HIP_EINVAL;
    const char *const fn = "lam_hip_solve_mshift";
    LAMCHK(multi_supported(c, fn));
    LAMCHK(mshift_check_n(c, fn, nshifts));
    if (!b_host || !sigma) return fail(c, LAM_HIP_EINVAL, "%s: b_host or sigma is NULL", fn);
    double sh[kMaxShifts] = {};
    ShiftsRead read;
    LAMCHK(multi_read_shifts(c, fn, nshifts, sigma, /*allow_negative=*/false, sh, &read));
    const double s_min = read.min;
    if (!c->have_problem) return fail(c, LAM_HIP_ESTATE, "call lam_hip_set_problem first");
    if (!c->have_matrix) return fail(c, LAM_HIP_ESTATE, "matrix not set");
    LAMCHK(set_dev(c, c->sh[0]));
    LAMCHK(multi_ensure(c));
    MultiState &m = c->multi;
    MshiftState &ms = m.ms;
    m.have_rhs = m.solved = ms.valid = false;
    multi_clear_shifts(m);
    const int groups = mshift_groups(nshifts);
    LAMCHK(mshift_ensure(c, groups));
    LAMCHK(multi_upload(c, 1, 1, b_host, m.B));
    HIPCHK(c, hipStreamSynchronize(c->sh[0].stream));
    m.nrhs = 1; m.K = 1;
    m.have_rhs = true;
    m.shift[0] = s_min;
    m.shifted = s_min != 0.0;
    ms.nshifts = nshifts;
    memcpy(ms.shift, sh, sizeof sh);
    lam_hip_stats seed_st;
    int32_t seed_ni = 0, seed_cv = 0;
    double seed_re = 0.0;
    LAMCHK(multi_solve(c, fn, LAM_HIP_PC_NONE, kGuessNone, nullptr, max_iters, rel_error, &seed_st, &seed_ni, &seed_cv, &seed_re, &ms));
    const double t0 = now_s();
    ShardBase &s = c->sh[0];
    unsigned long long seed_slots = 0;
    for (int j = 0; j < nshifts; j++)
        if (sh[j] == s_min) seed_slots |= 1ull << j;
    LAMCHK(mshift_dispatch(c, [&](auto impl) -> int {
        using TV = typename ImplTraits<decltype(impl)>::TV;
        hipLaunchKernelGGL((mshift_copy_seed_kernel<TV, kShiftGroup>), dim3(vec_grid(c->n), groups), dim3(kBlock), 0, s.stream,
                           (const TV *)m.X, (TV *)ms.XS, c->n, seed_slots);
        HIPCHK(c, hipGetLastError());
        return 0;
    }));
    const std::unique_ptr<MshiftScalars> h(new MshiftScalars);
    HIPCHK(c, hipMemcpyAsync(h.get(), ms.sc, sizeof(MshiftScalars), hipMemcpyDeviceToHost, s.stream));
    HIPCHK(c, hipStreamSynchronize(s.stream));
    int most = 0, all_conv = 1;
    double worst = 0.0;
    bool any_nan = false;
    for (int j = 0; j < nshifts; j++) {
        int ni = seed_ni, cv = seed_cv;
        double re = seed_re;
        if (!(seed_slots >> j & 1ull)) {
            // stopped: its iteration; frozen on an underflow of zeta: the last completed step, not converged; still live: the batch's
            // convention for a column that never met its test (max_iters + 1 at the cap)
            cv = h->stop[j] != 0;
            ni = cv || h->frozen_at[j] != 0 ? h->iters[j] : h->iters[j] + 1;
            re = h->iters[j] == 0 ? seed_re : h->rel_err[j];      // no step completed: the start's own sqrt(rr0 / bb), the seed's
        }
        if (num_iters) num_iters[j] = ni;
        if (converged) converged[j] = cv;
        if (rel_err) rel_err[j] = re;
        most = std::max(most, ni);
        all_conv = all_conv && cv;
        if (re != re) any_nan = true; else worst = std::max(worst, re);
    }
    if (st) {
        *st = seed_st;
        st->num_iters = most;
        st->converged = all_conv;
        st->rel_err = any_nan ? std::nan("") : worst;
        st->t_total += now_s() - t0;
    }
    ms.valid = true;
    return 0;
}

int lam_hip_get_solution_mshift(lam_hip_ctx *c, int nshifts, void *x_host)
{
    if (!c) return LAM_HIP_EINVAL;
    const char *const fn = "lam_hip_get_solution_mshift";
    LAMCHK(multi_supported(c, fn));
    LAMCHK(mshift_check_n(c, fn, nshifts));
    if (!x_host) return fail(c, LAM_HIP_EINVAL, "%s: x_host is NULL", fn);
    LAMCHK(mshift_readable(c, fn, nshifts));
    LAMCHK(set_dev(c, c->sh[0]));
    const size_t ev = c->esz_v(), group_elems = (size_t)(c->n + kMultiPadRows) * kShiftGroup;
    for (int first = 0; first < nshifts; first += kShiftGroup)
        LAMCHK(multi_download(c, std::min(kShiftGroup, nshifts - first), kShiftGroup,
                              (const char *)c->multi.ms.XS + (size_t)(first / kShiftGroup) * group_elems * ev,
                              (char *)x_host + (size_t)first * c->n * ev));
    return 0;
}

// Per group of 8 shifts: the group's X is [n][8], the K = 8 layout, so it meets ONE K = 8 SHIFT = true product with the group's
// absolute shifts, then one pass b - Y against the single b.
int lam_hip_true_residual_mshift(lam_hip_ctx *c, int nshifts, double *rel_res)
{
    if (!c) return LAM_HIP_EINVAL;
    const char *const fn = "lam_hip_true_residual_mshift";
    LAMCHK(multi_supported(c, fn));
    LAMCHK(mshift_check_n(c, fn, nshifts));
    if (!rel_res) return fail(c, LAM_HIP_EINVAL, "%s: rel_res is NULL", fn);
    LAMCHK(mshift_readable(c, fn, nshifts));
    const MshiftState &ms = c->multi.ms;
    LAMCHK(set_dev(c, c->sh[0]));
    const size_t group_bytes = (size_t)(c->n + kMultiPadRows) * kShiftGroup * c->esz_v();
    for (int first = 0; first < nshifts; first += kShiftGroup) {
        double gs[kMaxRhs] = {}, res[kMaxRhs];
        for (int j = 0; j < kShiftGroup && first + j < nshifts; j++) gs[j] = ms.shift[first + j];
        LAMCHK(mshift_dispatch(c, [&](auto impl) -> int {
            using I = decltype(impl);
            using TV = typename ImplTraits<I>::TV;
            return multi_residual_tail<typename ImplTraits<I>::TA, TV, kShiftGroup>(
                c, (const char *)ms.XS + (size_t)(first / kShiftGroup) * group_bytes, gs, mshift_residual_kernel<TV, kShiftGroup>, res);
        }));
        for (int j = 0; j < kShiftGroup && first + j < nshifts; j++) rel_res[first + j] = res[j];
    }
    return 0;
}

}  // extern "C"
