// lam_multi.h -- several right-hand sides on one matrix: lam_hip_set_rhs_many / _set_shifts_many / _solve_many / _solve_many_pc /
// _solve_many_x0 / _true_residual_many / _get_solution_many / _gemv_many / _gemv_many_only, and lam_hip_get_diagonal.  nrhs independent CG recurrences (NOT block CG) advanced together, one
// pass over the matrix per iteration.
// Part of the one translation unit csrc/lam_hip.hip (included from there, in order; not a stand-alone header).
//
// Instantiations: K = 1, 2, 4, 8 columns; nrhs runs on the smallest K >= nrhs, the K - nrhs padding columns are zero and born stopped.
// Product shape, every K and both dtypes: 4 rows per 4-wave workgroup, p tile of 32 KiB in LDS whatever K
// (fp64: 4096 / 2048 / 1024 / 512 columns for K = 1 / 2 / 4 / 8; fp32: 4096 / 4096 / 2048 / 1024), non-temporal matrix loads.
// Three launches per iteration (product; x, r; p), all on shard 0's stream; the host follows the batch's own pinned progress word
// with the lag rule of the single solve (lag_check), where "stopped" means every live column has stopped.
// One recurrence in the source: lam_hip_solve_many_pc(JACOBI) runs the PC = true instantiations of the same four vector kernels
// (multi_init_kernel, multi_init_scalars_kernel, multi_xr_kernel, multi_p_kernel) on the same scalars' block, and
// lam_hip_solve_many_x0 the GUESS = true instantiations of the two init kernels behind one more product launch; the loop is shared.
// lam_hip_set_shifts_many makes column j the system (A + s_j I) x_j = b_j: the SHIFT = true instantiation of the product (its epilogue
// adds s_j p_j[row]; the K shifts travel by value in its arguments) in the loop, in the guess's product and in the true residual's, and
// under Jacobi the DK = true instantiations of the vector kernels on a K-wide dinv_k = 1 / (A_ii + s_j) (shifted_dinv_kernel).  No
// shifts, or all of them zero: the instantiations and the launches of before.
// lam_hip_solve_many_minres (minres_solve, next to multi_solve): K MINRES recurrences on the same product launch, shifts of either
// sign; its own three init and two per-iteration vector kernels, W / W_OLD and scalars' block (MinresState), the loop's host side shared
// in shape.  It alone can leave a negative shift in force, under which multi_solve refuses to run.
#pragma once

static_assert(lam::kMaxRhs == LAM_HIP_MAX_RHS, "include/lam_hip.h states the limit");
static_assert(lam::kMaxShifts == LAM_HIP_MAX_SHIFTS, "include/lam_hip.h states the limit");
static_assert(lam::kShiftGroup == lam::kMaxRhs, "a group of shifts is handed to the K = 8 product as it is");

namespace {

constexpr int kMultiRows = 4;     // rows per workgroup of multi_gemv_kernel
constexpr int kMultiWaves = 4;    // waves per workgroup

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
int multi_k_for(int nrhs) { return nrhs <= 1 ? 1 : (nrhs <= 2 ? 2 : (nrhs <= 4 ? 4 : 8)); }

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

template <typename F>
int multi_dispatch_k(lam_hip_ctx *c, int K, F &&f)
{
    switch (K) {
    case 1: return f(std::integral_constant<int, 1>());
    case 2: return f(std::integral_constant<int, 2>());
    case 4: return f(std::integral_constant<int, 4>());
    case 8: return f(std::integral_constant<int, 8>());
    }
    return fail(c, LAM_HIP_EINVAL, "no batched kernels for K = %d", K);
}
// f(Impl<TA, TV>(), integral_constant<int, K>()) for the context's dtype (fp64 / fp32 only: multi_supported)
template <typename F>
int multi_dispatch(lam_hip_ctx *c, int K, F &&f)
{
    if (c->dtype == LAM_HIP_F64) return multi_dispatch_k(c, K, [&](auto k) -> int { return f(Impl<double, double>(), k); });
    if (c->dtype == LAM_HIP_F32) return multi_dispatch_k(c, K, [&](auto k) -> int { return f(Impl<float, float>(), k); });
    return fail(c, LAM_HIP_EINVAL, "the multi-right-hand-side path has no kernels for dtype %d", c->dtype);
}
// the recurrence's: f(Impl<TA, TV>(), integral_constant<int, K>(), bool_constant<PC>()), PC = Jacobi-preconditioned
template <typename F>
int multi_dispatch(lam_hip_ctx *c, int K, bool pc, F &&f)
{
    return multi_dispatch(c, K, [&](auto impl, auto k) -> int { return pc ? f(impl, k, std::true_type()) : f(impl, k, std::false_type()); });
}

// and with the start: f(..., bool_constant<PC>(), bool_constant<GUESS>()), GUESS = from an initial guess (lam_hip_solve_many_x0)
template <typename F>
int multi_dispatch(lam_hip_ctx *c, int K, bool pc, bool guess, F &&f)
{
    return multi_dispatch(c, K, pc, [&](auto impl, auto k, auto pct) -> int {
        return guess ? f(impl, k, pct, std::true_type()) : f(impl, k, pct, std::false_type());
    });
}

int multi_gemv_grid(const lam_hip_ctx *c) { return (int)((c->n + kMultiRows - 1) / kMultiRows); }

// shift: null for the plain product of A (lam_hip_gemv_many*, and a batch without shifts: the SHIFT = false instantiation, the only
// one there was), else the K shifts of the batch (MultiState::shift): Y_j = (A + s_j I) P_j
template <typename TA, typename TV, int K>
int multi_launch_gemv(lam_hip_ctx *c, const TV *P, TV *Y, double *partial, const MultiScalars *sc, const double *shift = nullptr)
{
    ShardBase &s = c->sh[0];
    MultiGemvArgs<TA, TV> a;
    a.A = (const TA *)s.A; a.p = P; a.y = Y; a.partial = partial; a.sc = sc;
    a.nrows = c->n; a.ncols = c->ncols_vec(); a.lda = c->lda;
    for (int j = 0; j < kMaxRhs; j++) a.shift[j] = shift ? (TV)shift[j] : (TV)0;
    if (shift)
        hipLaunchKernelGGL((multi_gemv_kernel<TA, TV, K, kMultiRows, kMultiWaves, true, true>), dim3(multi_gemv_grid(c)),
                           dim3(kMultiWaves * 64), 0, s.stream, a);
    else
        hipLaunchKernelGGL((multi_gemv_kernel<TA, TV, K, kMultiRows, kMultiWaves, true>), dim3(multi_gemv_grid(c)), dim3(kMultiWaves * 64), 0,
                           s.stream, a);
    LAUNCHED(c);
    return 0;
}

// and with the preconditioner's layout: f(..., bool_constant<PC>(), bool_constant<GUESS>(), bool_constant<DK>()), DK = K-wide dinv of
// the shifted batch; only PC has such instantiations
template <typename F>
int multi_dispatch(lam_hip_ctx *c, int K, bool pc, bool guess, bool dk, F &&f)
{
    return multi_dispatch(c, K, pc, guess, [&](auto impl, auto k, auto pct, auto gt) -> int {
        if constexpr (decltype(pct)::value) return dk ? f(impl, k, pct, gt, std::true_type()) : f(impl, k, pct, gt, std::false_type());
        else return f(impl, k, pct, gt, std::false_type());
    });
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

// P = X of the batch's last solve, ready for the product: the rows behind row n zero in this K's layout (X's are not kept so)
int multi_stage_solution(lam_hip_ctx *c, int K)
{
    MultiState &m = c->multi;
    ShardBase &s = c->sh[0];
    const size_t ev = c->esz_v(), body = (size_t)c->n * K * ev;
    HIPCHK(c, hipMemcpyAsync(m.P, m.X, body, hipMemcpyDeviceToDevice, s.stream));
    HIPCHK(c, hipMemsetAsync((char *)m.P + body, 0, (size_t)kMultiPadRows * K * ev, s.stream));
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

// diag / dinv of the matrix held now: one launch over the n diagonal elements of the pitched matrix, once per matrix content
// (matrix_gen).  The scan for rows that cannot be inverted is part of that launch; the host reads a count, the first such row and,
// if there is one, that row's value -- never the n values.
int pcg_extract_diagonal(lam_hip_ctx *c)
{
    PcgState &g = c->pcg;
    if (g.diag_gen == c->matrix_gen) return 0;
    ShardBase &s = c->sh[0];
    DiagInfo h;
    h.first_bad = ~0ull; h.count = 0;
    HIPCHK(c, hipMemcpyAsync(g.info, &h, sizeof h, hipMemcpyHostToDevice, s.stream));
    HIPCHK(c, hipStreamSynchronize(s.stream));      // h is pageable
    LAMCHK(multi_dispatch(c, 1, [&](auto impl, auto) -> int {
        using TA = typename ImplTraits<decltype(impl)>::TA;
        using TV = typename ImplTraits<decltype(impl)>::TV;
        hipLaunchKernelGGL((diag_extract_kernel<TA, TV>), dim3(vec_grid(c->n)), dim3(kBlock), 0, s.stream, (const TA *)s.A, c->lda,
                           (uint64_t)0, c->n, (TV *)g.diag, (TV *)g.dinv, g.info);
        HIPCHK(c, hipGetLastError());
        return 0;
    }));
    HIPCHK(c, hipMemcpyAsync(&h, g.info, sizeof h, hipMemcpyDeviceToHost, s.stream));
    HIPCHK(c, hipStreamSynchronize(s.stream));
    g.bad_count = h.count;
    g.bad_row = h.first_bad;
    g.bad_value = 0.0;
    if (h.count != 0 && h.first_bad < c->n) {
        double v64 = 0.0;
        float v32 = 0.f;
        void *dst = c->dtype == LAM_HIP_F64 ? (void *)&v64 : (void *)&v32;
        HIPCHK(c, hipMemcpy(dst, (const char *)g.diag + h.first_bad * c->esz_v(), c->esz_v(), hipMemcpyDeviceToHost));
        g.bad_value = c->dtype == LAM_HIP_F64 ? v64 : (double)v32;
    }
    g.diag_gen = c->matrix_gen;
    return 0;
}

// dinv_k of the shifted batch, M_j = diag(A) + s_j I: one launch builds and scans it, once per (matrix content, K, nrhs, shifts).
// The host reads the count and the first (row, column) that cannot be inverted, and for the message that row's one diagonal element.
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
    DiagInfo h;
    h.first_bad = ~0ull; h.count = 0;
    HIPCHK(c, hipMemcpyAsync(g.info, &h, sizeof h, hipMemcpyHostToDevice, s.stream));
    HIPCHK(c, hipStreamSynchronize(s.stream));      // h is pageable
    ShiftList sl;
    for (int j = 0; j < kMaxRhs; j++) sl.s[j] = m.shift[j];
    LAMCHK(multi_dispatch(c, m.K, [&](auto impl, auto kc) -> int {
        using TA = typename ImplTraits<decltype(impl)>::TA;
        using TV = typename ImplTraits<decltype(impl)>::TV;
        hipLaunchKernelGGL((shifted_dinv_kernel<TA, TV, decltype(kc)::value>), dim3(vec_grid(c->n)), dim3(kBlock), 0, s.stream,
                           (const TA *)s.A, c->lda, c->n, m.nrhs, sl, (TV *)g.dinv_k, g.info);
        HIPCHK(c, hipGetLastError());
        return 0;
    }));
    HIPCHK(c, hipMemcpyAsync(&h, g.info, sizeof h, hipMemcpyDeviceToHost, s.stream));
    HIPCHK(c, hipStreamSynchronize(s.stream));
    g.badk_count = h.count;
    g.badk_row = 0; g.badk_col = 0; g.badk_value = 0.0;
    if (h.count != 0 && h.first_bad / m.K < c->n) {
        g.badk_row = h.first_bad / m.K;
        g.badk_col = (int)(h.first_bad % m.K);
        double v64 = 0.0;
        float v32 = 0.f;
        void *dst = c->dtype == LAM_HIP_F64 ? (void *)&v64 : (void *)&v32;
        HIPCHK(c, hipMemcpy(dst, (const char *)s.A + (g.badk_row * c->lda + g.badk_row) * c->esz_a(), c->esz_a(), hipMemcpyDeviceToHost));
        const double sum = (c->dtype == LAM_HIP_F64 ? v64 : (double)v32) + m.shift[g.badk_col];
        g.badk_value = c->dtype == LAM_HIP_F64 ? sum : (double)(float)sum;
    }
    g.dinvk_gen = c->matrix_gen;
    g.dinvk_K = m.K; g.dinvk_nrhs = m.nrhs;
    memcpy(g.dinvk_shift, m.shift, sizeof m.shift);
    return 0;
}

void multi_harvest(MultiState &m, int slot, double *ms_sum, int *samples)
{
    if (!m.timed_slot[slot]) return;
    m.timed_slot[slot] = false;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, m.ev0[slot], m.ev1[slot]) != hipSuccess) { (void)hipGetLastError(); return; }
    *ms_sum += ms;
    (*samples)++;
}

}  // namespace

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
    bool any = false;
    for (int j = 0; j < nrhs; j++) {
        const double r = c->dtype == LAM_HIP_F32 ? (double)(float)sigma[j] : sigma[j];
        if (!(sigma[j] >= 0.0) || !std::isfinite(r))
            return fail(c, LAM_HIP_EINVAL, "lam_hip_set_shifts_many: shift %d is %g: every shift must be finite and >= 0, in the vector "
                        "dtype too", j, sigma[j]);
        s[j] = r;
        any = any || r != 0.0;
    }
    memcpy(m.shift, s, sizeof s);
    m.shifted = any;
    return 0;
}

}  // extern "C"

namespace {

// where a batched solve starts: x = 0, a guess given on the host, or the batch's own last solution
enum MultiGuess { kGuessNone, kGuessHost, kGuessCurrent };

// what a batched solve reports, CG or MINRES: the per-column arrays and the batch's stats from the scalars' prefix as the host read
// it back; rel_of(j, col) is column j's rel_err (CG: from its r.r ring; MINRES: its own word)
template <typename F>
void multi_report(lam_hip_ctx *c, const MultiScalars &h, F &&rel_of, double t0, double t1, double gemv_ms, int samples, lam_hip_stats *st,
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
        st->t_gemv = samples > 0 ? gemv_ms * 1e-3 / samples : 0.0;
        st->t_comm_init = c->t_comm_init;
        // the product launch alone, with or without the preconditioner: the diagonal is read by the two vector launches
        st->gemv_bytes = (double)c->esz_a() * (double)c->n * (double)c->n + (double)c->esz_v() * 2.0 * (double)m.K * (double)c->n;
    }
}

// lam_hip_solve_many (precond = LAM_HIP_PC_NONE), lam_hip_solve_many_pc and lam_hip_solve_many_x0: one body, one sequence of
// launches.  The Jacobi-preconditioned batch runs the PC = true instantiations of the four vector kernels on dinv and a second
// partial array (both null for the plain batch); the product launch, the scalars' block, the progress word, the lag rule and the
// per-column results are shared.  A start from a guess stages the guess in P (whose rows behind row n the product needs zero; the
// upload and multi_stage_solution see to that), forms A x0 in AP with one more product launch and runs the GUESS = true
// instantiations of the two init kernels; the loop is the same loop.
// mshift (lam_hip_solve_mshift only, null for every other entry point): the multi-shift state the K = 1 seed batch drives -- one init
// launch in front of the loop and one step launch behind every multi_p_kernel; nothing else changes, the seed's progress word decides.
int multi_solve(lam_hip_ctx *c, const char *fn, int precond, MultiGuess guess, const void *x0_host, int max_iters, double rel_error,
                lam_hip_stats *st, int32_t *num_iters, int32_t *converged, double *rel_err, MshiftState *mshift = nullptr)
{
    LAMCHK(multi_supported(c, fn));
    if (precond != LAM_HIP_PC_NONE && precond != LAM_HIP_PC_JACOBI)
        return fail(c, LAM_HIP_EINVAL, "%s: unknown preconditioner %d (LAM_HIP_PC_NONE, LAM_HIP_PC_JACOBI)", fn, precond);
    const bool pc = precond == LAM_HIP_PC_JACOBI;
    if (max_iters < 0) return fail(c, LAM_HIP_EINVAL, "max_iters must be >= 0");
    MultiState &m = c->multi;
    if (!c->have_matrix || !m.have_rhs || m.n != c->n)
        return fail(c, LAM_HIP_ESTATE, "matrix and right-hand sides (lam_hip_set_rhs_many) must be set before %s", fn);
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
    m.host_flags[0] = m.host_flags[1] = 0;
    for (int i = 0; i < kLag; i++) m.timed_slot[i] = false;
    c->prog_t = 0.0;
    c->multi.last_K = m.K;
    // the lag rule reads the batch's own progress word: the single solve's helpers on a view that carries it
    ShardBase view;
    view.dev = s0.dev; view.stream = s0.stream; view.host_flags = m.host_flags;
    const int vb = vec_grid(c->n), gb = multi_gemv_grid(c);
    double gemv_ms = 0.0;
    int samples = 0, enq = 0;
    if (guess == kGuessHost) LAMCHK(multi_upload(c, m.nrhs, m.K, x0_host, m.P));
    if (guess == kGuessCurrent) LAMCHK(multi_stage_solution(c, m.K));
    LAMCHK(multi_dispatch(c, m.K, pc, guess != kGuessNone, dk, [&](auto impl, auto kc, auto pct, auto gt, auto dkt) -> int {
        using I = decltype(impl);
        using TA = typename ImplTraits<I>::TA;
        using TV = typename ImplTraits<I>::TV;
        constexpr int K = decltype(kc)::value;
        constexpr bool PC = decltype(pct)::value;
        constexpr bool GUESS = decltype(gt)::value;
        constexpr bool DK = decltype(dkt)::value;
        const TV *const dinv = PC ? (const TV *)(DK ? g.dinv_k : g.dinv) : nullptr;
        double *const part_rz = PC ? g.part_rz : nullptr;
        double *const part_rr = GUESS ? m.part_rr : nullptr;
        // GUESS: AP = A x0 ((A + s_j I) x0 of a shifted batch) of the guess staged in P, outside the iteration's scalars and partials
        if (GUESS) LAMCHK((multi_launch_gemv<TA, TV, K>(c, (const TV *)m.P, (TV *)m.AP, nullptr, nullptr, shift)));
        // x = 0, r = b, p = b, bb_j = b_j.b_j  (PC: p = dinv o b, rz_j = b_j.(dinv o b_j));  GUESS: x = x0, r = b - A x0, p = r,
        // rr_j = r_j.r_j next to bb_j  (PC: p = dinv o r, rz_j = r_j.(dinv o r_j))
        hipLaunchKernelGGL((multi_init_kernel<TV, K, PC, GUESS, DK>), dim3(vb), dim3(kBlock), 0, s0.stream, (const TV *)m.B, (TV *)m.X,
                           (TV *)m.R, (TV *)m.P, c->n, m.part_vec, dinv, part_rz, (const TV *)(GUESS ? m.AP : nullptr), part_rr);
        HIPCHK(c, hipGetLastError());
        hipLaunchKernelGGL((multi_init_scalars_kernel<K, PC, GUESS>), dim3(1), dim3(kBlock), 0, s0.stream, (const double *)m.part_vec, vb,
                           m.nrhs, m.sc, (volatile int *)m.host_flags, (const double *)part_rz, (const double *)part_rr, rel_error);
        HIPCHK(c, hipGetLastError());
        const int sgroups = mshift ? (mshift->nshifts + kShiftGroup - 1) / kShiftGroup : 0;
        if (mshift) {
            MshiftList dl;
            for (int j = 0; j < kMaxShifts; j++) dl.d[j] = j < mshift->nshifts ? mshift->shift[j] - m.shift[0] : 0.0;
            hipLaunchKernelGGL((mshift_init_kernel<TV, kShiftGroup>), dim3(vb, sgroups), dim3(kBlock), 0, s0.stream, (const TV *)m.B,
                               (TV *)mshift->XS, (TV *)mshift->PS, c->n, mshift->nshifts, dl, mshift->sc);
            HIPCHK(c, hipGetLastError());
        }
        for (int i = 0; i < max_iters; i++) {
            const int k = i + 1, slot = i % kLag;
            if (i >= kLag) {
                const int d = lag_check(c, view, k);
                if (d < 0) return d;
                if (d != 0) break;
                multi_harvest(m, slot, &gemv_ms, &samples);
            }
            const double te = now_s();
            const bool timed = timed_iteration(c, s0, k);
            m.timed_slot[slot] = timed;
            if (timed) RECORD(c, m.ev0[slot], s0.stream);
            LAMCHK((multi_launch_gemv<TA, TV, K>(c, (const TV *)m.P, (TV *)m.AP, m.part_gemv, m.sc, shift)));
            if (timed) RECORD(c, m.ev1[slot], s0.stream);
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
            c->enqueue_ns += (uint64_t)((now_s() - te) * 1e9);
            enq++;
        }
        return 0;
    }));
    if (enq > 0) {
        Progress pr;
        LAMCHK(await_progress(c, view, enq, &pr, /*precise=*/true));
    }
    HIPCHK(c, hipStreamSynchronize(s0.stream));
    for (int j = 0; j < kLag; j++) multi_harvest(m, j, &gemv_ms, &samples);
    HIPCHK(c, hipMemcpyAsync(m.sc_host, m.sc, sizeof(MultiScalars), hipMemcpyDeviceToHost, s0.stream));
    HIPCHK(c, hipStreamSynchronize(s0.stream));
    m.solved = true;
    multi_report(c, *m.sc_host, [](int, const CgScalars &sc) { return std::sqrt(sc.rr[sc.iters & 1] / sc.bb); }, t0, now_s(), gemv_ms, samples,
                 st, num_iters, converged, rel_err);
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

// lam_hip_solve_many_minres: multi_solve's sibling.  The same enqueue loop -- the batch's progress word under the lag rule, the timed
// product slots, the stats -- around MINRES' own vector launches and scalars' block; the product launch is the batch's, with V (the
// batch's P) as its input.  multi_solve launches what it launched before.
int minres_solve(lam_hip_ctx *c, const char *fn, const double *sigma, int max_iters, double rel_error, lam_hip_stats *st,
                 int32_t *num_iters, int32_t *converged, double *rel_err)
{
    LAMCHK(multi_supported(c, fn));
    if (max_iters < 0) return fail(c, LAM_HIP_EINVAL, "max_iters must be >= 0");
    MultiState &m = c->multi;
    if (!c->have_matrix || !m.have_rhs || m.n != c->n)
        return fail(c, LAM_HIP_ESTATE, "matrix and right-hand sides (lam_hip_set_rhs_many) must be set before %s", fn);
    double s[kMaxRhs] = {};
    bool any = false;
    if (sigma) {
        for (int j = 0; j < m.nrhs; j++) {
            const double r = c->dtype == LAM_HIP_F32 ? (double)(float)sigma[j] : sigma[j];
            if (!std::isfinite(sigma[j]) || !std::isfinite(r))
                return fail(c, LAM_HIP_EINVAL, "%s: shift %d is %g: every shift must be finite, in the vector dtype too", fn, j, sigma[j]);
            s[j] = r;
            any = any || r != 0.0;
        }
    }
    const double t0 = now_s();
    ShardBase &s0 = c->sh[0];
    LAMCHK(set_dev(c, s0));
    HIPCHK(c, hipStreamSynchronize(s0.stream));
    // the lazy allocation first: if it fails, the shifts in force and the batched solution are what they were
    LAMCHK(minres_ensure(c));
    if (sigma) {
        memcpy(m.shift, s, sizeof s);
        m.shifted = any;
    }
    m.solved = false;
    m.ms.valid = false;
    MinresState &mr = m.mr;
    const double *const shift = m.shifted ? m.shift : nullptr;
    m.host_flags[0] = m.host_flags[1] = 0;
    for (int i = 0; i < kLag; i++) m.timed_slot[i] = false;
    c->prog_t = 0.0;
    c->multi.last_K = m.K;
    ShardBase view;
    view.dev = s0.dev; view.stream = s0.stream; view.host_flags = m.host_flags;
    const int vb = vec_grid(c->n), gb = multi_gemv_grid(c);
    double gemv_ms = 0.0;
    int samples = 0, enq = 0;
    LAMCHK(multi_dispatch(c, m.K, [&](auto impl, auto kc) -> int {
        using I = decltype(impl);
        using TA = typename ImplTraits<I>::TA;
        using TV = typename ImplTraits<I>::TV;
        constexpr int K = decltype(kc)::value;
        TV *const V = (TV *)m.P, *const U = (TV *)m.AP, *const VOLD = (TV *)m.R, *const X = (TV *)m.X;
        TV *const W = (TV *)mr.W, *const WOLD = (TV *)mr.WOLD;
        hipLaunchKernelGGL((minres_init_kernel<TV, K>), dim3(vb), dim3(kBlock), 0, s0.stream, (const TV *)m.B, X, VOLD, W, WOLD, V, c->n,
                           m.part_vec);
        HIPCHK(c, hipGetLastError());
        hipLaunchKernelGGL((minres_init_scalars_kernel<K>), dim3(1), dim3(kBlock), 0, s0.stream, (const double *)m.part_vec, vb, m.nrhs,
                           mr.sc, (volatile int *)m.host_flags);
        HIPCHK(c, hipGetLastError());
        hipLaunchKernelGGL((minres_start_kernel<TV, K>), dim3(vb), dim3(kBlock), 0, s0.stream, (const TV *)m.B, V, c->n,
                           (const MinresScalars *)mr.sc);
        HIPCHK(c, hipGetLastError());
        for (int i = 0; i < max_iters; i++) {
            const int k = i + 1, slot = i % kLag;
            if (i >= kLag) {
                const int d = lag_check(c, view, k);
                if (d < 0) return d;
                if (d != 0) break;
                multi_harvest(m, slot, &gemv_ms, &samples);
            }
            const double te = now_s();
            const bool timed = timed_iteration(c, s0, k);
            m.timed_slot[slot] = timed;
            if (timed) RECORD(c, m.ev0[slot], s0.stream);
            LAMCHK((multi_launch_gemv<TA, TV, K>(c, (const TV *)V, U, m.part_gemv, mr.sc, shift)));
            if (timed) RECORD(c, m.ev1[slot], s0.stream);
            hipLaunchKernelGGL((minres_lanczos_kernel<TV, K>), dim3(vb), dim3(kBlock), 0, s0.stream, (const double *)m.part_gemv, gb, mr.sc, k,
                               (const TV *)V, (const TV *)VOLD, U, c->n, m.part_vec);
            LAUNCHED(c);
            hipLaunchKernelGGL((minres_update_kernel<TV, K>), dim3(vb), dim3(kBlock), 0, s0.stream, (const double *)m.part_vec, vb, mr.sc, k,
                               rel_error, (const TV *)U, V, VOLD, W, WOLD, X, c->n, (volatile int *)m.host_flags);
            LAUNCHED(c);
            c->enqueue_ns += (uint64_t)((now_s() - te) * 1e9);
            enq++;
        }
        return 0;
    }));
    if (enq > 0) {
        Progress pr;
        LAMCHK(await_progress(c, view, enq, &pr, /*precise=*/true));
    }
    HIPCHK(c, hipStreamSynchronize(s0.stream));
    for (int j = 0; j < kLag; j++) multi_harvest(m, j, &gemv_ms, &samples);
    const std::unique_ptr<MinresScalars> h(new MinresScalars);
    HIPCHK(c, hipMemcpyAsync(h.get(), mr.sc, sizeof(MinresScalars), hipMemcpyDeviceToHost, s0.stream));
    HIPCHK(c, hipStreamSynchronize(s0.stream));
    m.solved = true;
    multi_report(c, *h, [&](int j, const CgScalars &) { return h->rel_err[j]; }, t0, now_s(), gemv_ms, samples, st, num_iters, converged,
                 rel_err);
    return 0;
}

}  // namespace

extern "C" {

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

// One batched product of X (staged through P, whose rows behind row n the product needs zero), one K-wide pass over B and A X, one
// workgroup for the K quotients.  B, X and the scalars are left alone; P and AP are scratch, as they are between any two solves.
int lam_hip_true_residual_many(lam_hip_ctx *c, int nrhs, double *rel_res)
{
    if (!c) return LAM_HIP_EINVAL;
    LAMCHK(multi_supported(c, "lam_hip_true_residual_many"));
    LAMCHK(multi_check_nrhs(c, "lam_hip_true_residual_many", nrhs));
    if (!rel_res) return fail(c, LAM_HIP_EINVAL, "lam_hip_true_residual_many: rel_res is NULL");
    MultiState &m = c->multi;
    if (!m.solved || !m.have_rhs || m.n != c->n) return fail(c, LAM_HIP_ESTATE, "no batched solution yet (lam_hip_solve_many)");
    if (nrhs > m.nrhs) return fail(c, LAM_HIP_EINVAL, "lam_hip_true_residual_many: %d columns asked, %d were solved", nrhs, m.nrhs);
    ShardBase &s = c->sh[0];
    LAMCHK(set_dev(c, s));
    LAMCHK(multi_stage_solution(c, m.K));
    const int vb = vec_grid(c->n);
    LAMCHK(multi_dispatch(c, m.K, [&](auto impl, auto kc) -> int {
        using I = decltype(impl);
        using TA = typename ImplTraits<I>::TA;
        using TV = typename ImplTraits<I>::TV;
        constexpr int K = decltype(kc)::value;
        LAMCHK((multi_launch_gemv<TA, TV, K>(c, (const TV *)m.P, (TV *)m.AP, nullptr, nullptr, m.shifted ? m.shift : nullptr)));
        hipLaunchKernelGGL((multi_residual_kernel<TV, K>), dim3(vb), dim3(kBlock), 0, s.stream, (const TV *)m.B, (const TV *)m.AP, c->n,
                           m.part_rr, m.part_vec);
        HIPCHK(c, hipGetLastError());
        hipLaunchKernelGGL((multi_residual_scalars_kernel<K>), dim3(1), dim3(kBlock), 0, s.stream, (const double *)m.part_rr,
                           (const double *)m.part_vec, vb, m.res);
        HIPCHK(c, hipGetLastError());
        return 0;
    }));
    double res[kMaxRhs];
    HIPCHK(c, hipMemcpyAsync(res, m.res, sizeof(double) * m.K, hipMemcpyDeviceToHost, s.stream));
    HIPCHK(c, hipStreamSynchronize(s.stream));
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

}  // extern "C"

namespace {

int mshift_check_n(lam_hip_ctx *c, const char *fn, int nshifts)
{
    if (nshifts < 1 || nshifts > LAM_HIP_MAX_SHIFTS)
        return fail(c, LAM_HIP_EINVAL, "%s: nshifts = %d, must be 1..%d (LAM_HIP_MAX_SHIFTS)", fn, nshifts, LAM_HIP_MAX_SHIFTS);
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

// f(Impl<TA, TV>()) for the context's dtype: the multi-shift kernels have the one group width
template <typename F>
int mshift_dispatch(lam_hip_ctx *c, F &&f)
{
    if (c->dtype == LAM_HIP_F64) return f(Impl<double, double>());
    if (c->dtype == LAM_HIP_F32) return f(Impl<float, float>());
    return fail(c, LAM_HIP_EINVAL, "the multi-shift path has no kernels for dtype %d", c->dtype);
}

int mshift_readable(lam_hip_ctx *c, const char *fn, int nshifts)
{
    MultiState &m = c->multi;
    if (!m.solved || !m.ms.valid || m.n != c->n) return fail(c, LAM_HIP_ESTATE, "no multi-shift solution yet (lam_hip_solve_mshift)");
    if (nshifts > m.ms.nshifts) return fail(c, LAM_HIP_EINVAL, "%s: %d shifts asked, %d were solved", fn, nshifts, m.ms.nshifts);
    return 0;
}

}  // namespace

extern "C" {

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
    double s_min = 0.0;
    for (int j = 0; j < nshifts; j++) {
        const double r = c->dtype == LAM_HIP_F32 ? (double)(float)sigma[j] : sigma[j];
        if (!(sigma[j] >= 0.0) || !std::isfinite(r))
            return fail(c, LAM_HIP_EINVAL, "%s: shift %d is %g: every shift must be finite and >= 0, in the vector dtype too", fn, j,
                        sigma[j]);
        sh[j] = r;
        s_min = j == 0 ? r : std::min(s_min, r);
    }
    if (!c->have_problem) return fail(c, LAM_HIP_ESTATE, "call lam_hip_set_problem first");
    if (!c->have_matrix) return fail(c, LAM_HIP_ESTATE, "matrix not set");
    LAMCHK(set_dev(c, c->sh[0]));
    LAMCHK(multi_ensure(c));
    MultiState &m = c->multi;
    MshiftState &ms = m.ms;
    m.have_rhs = m.solved = ms.valid = false;
    multi_clear_shifts(m);
    LAMCHK(mshift_ensure(c, (nshifts + kShiftGroup - 1) / kShiftGroup));
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
    const int groups = (nshifts + kShiftGroup - 1) / kShiftGroup;
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

// Per group of 8 shifts: the group's X is [n][8], the K = 8 layout, so it is staged in P as a batch's X is and meets ONE K = 8
// SHIFT = true product with the group's absolute shifts; then one pass b - Y against the single b.  P, AP, the partials and res are
// scratch, as they are between any two solves; B, X and XS are left alone.
int lam_hip_true_residual_mshift(lam_hip_ctx *c, int nshifts, double *rel_res)
{
    if (!c) return LAM_HIP_EINVAL;
    const char *const fn = "lam_hip_true_residual_mshift";
    LAMCHK(multi_supported(c, fn));
    LAMCHK(mshift_check_n(c, fn, nshifts));
    if (!rel_res) return fail(c, LAM_HIP_EINVAL, "%s: rel_res is NULL", fn);
    LAMCHK(mshift_readable(c, fn, nshifts));
    MultiState &m = c->multi;
    ShardBase &s = c->sh[0];
    LAMCHK(set_dev(c, s));
    const int vb = vec_grid(c->n);
    const size_t ev = c->esz_v(), body = (size_t)c->n * kShiftGroup * ev, group_bytes = (size_t)(c->n + kMultiPadRows) * kShiftGroup * ev;
    for (int first = 0; first < nshifts; first += kShiftGroup) {
        HIPCHK(c, hipMemcpyAsync(m.P, (const char *)m.ms.XS + (size_t)(first / kShiftGroup) * group_bytes, body, hipMemcpyDeviceToDevice,
                                 s.stream));
        HIPCHK(c, hipMemsetAsync((char *)m.P + body, 0, (size_t)kMultiPadRows * kShiftGroup * ev, s.stream));
        double gs[kMaxRhs] = {};
        for (int j = 0; j < kShiftGroup && first + j < nshifts; j++) gs[j] = m.ms.shift[first + j];
        LAMCHK(mshift_dispatch(c, [&](auto impl) -> int {
            using I = decltype(impl);
            using TA = typename ImplTraits<I>::TA;
            using TV = typename ImplTraits<I>::TV;
            constexpr int K = kShiftGroup;
            LAMCHK((multi_launch_gemv<TA, TV, K>(c, (const TV *)m.P, (TV *)m.AP, nullptr, nullptr, gs)));
            hipLaunchKernelGGL((mshift_residual_kernel<TV, K>), dim3(vb), dim3(kBlock), 0, s.stream, (const TV *)m.B, (const TV *)m.AP, c->n,
                               m.part_rr, m.part_vec);
            HIPCHK(c, hipGetLastError());
            hipLaunchKernelGGL((multi_residual_scalars_kernel<K>), dim3(1), dim3(kBlock), 0, s.stream, (const double *)m.part_rr,
                               (const double *)m.part_vec, vb, m.res);
            HIPCHK(c, hipGetLastError());
            return 0;
        }));
        double res[kMaxRhs];
        HIPCHK(c, hipMemcpyAsync(res, m.res, sizeof res, hipMemcpyDeviceToHost, s.stream));
        HIPCHK(c, hipStreamSynchronize(s.stream));
        for (int j = 0; j < kShiftGroup && first + j < nshifts; j++) rel_res[first + j] = res[j];
    }
    return 0;
}

}  // extern "C"
