// lam_deflate.h -- deflated CG for the batch, host side: lam_hip_set_deflation, lam_hip_set_deflation_eigs,
// lam_hip_solve_many_deflated, lam_hip_deflate_many, lam_hip_chol_inverse.  Kernels: lam_kernels.h ("Deflated CG"); the m x m
// inverse: lam_host_chol.h (host only); the recurrence: include/lam_hip.h.  Part of the one translation unit csrc/lam_hip.hip
// (included from there behind lam_eigs.h, whose basis pitch and state it uses; not a stand-alone header).
//
// The solve is multi_solve's GUESS path (lam_multi.h) with the guess built on the device and two launches of this file behind the init
// launches and behind every multi_p_kernel: an iteration is the plain batch's three launches plus deflate_dots_kernel and
// deflate_apply_kernel.
#pragma once

static_assert(lam::kMaxDeflation == LAM_HIP_MAX_DEFLATION, "include/lam_hip.h states the limit");

namespace {

int deflate_dots_blocks(uint64_t n) { return lanczos_dots_blocks(n); }

// the space is set and belongs to the matrix held now
bool deflate_valid(const lam_hip_ctx *c)
{
    const MultiState &m = c->multi;
    return m.df.m > 0 && c->have_matrix && m.n == c->n && m.df.gen == c->matrix_gen;
}

int deflate_part_ensure(lam_hip_ctx *c)
{
    DeflateState &d = c->multi.df;
    if (!d.part) HIPCHK(c, hipMalloc((void **)&d.part, sizeof(double) * (kVecBlocksMax / 4) * (size_t)kMaxDeflation * kMaxRhs));
    return 0;
}

// d = Wd^T u, u -= / = Wa (M d) on the K interleaved columns of u: the two launches, on shard 0's stream
template <typename TV, int K, bool START>
int deflate_launch(lam_hip_ctx *c, const MultiScalars *sc, const void *Wd, const void *Wa, uint64_t pitch, int mm, const double *M,
                   const void *u_dots, void *u_apply, uint64_t n, double *part, double *coeff, int ncoeff, bool counted)
{
    ShardBase &s = c->sh[0];
    const int vb = vec_grid(n), db = deflate_dots_blocks(n);
    hipLaunchKernelGGL((deflate_dots_kernel<TV, K>), dim3(db, kDeflateSplit), dim3(kBlock), 0, s.stream, sc, (const TV *)Wd, pitch, mm,
                       (const TV *)u_dots, n, part);
    if (counted) LAUNCHED(c); else HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL((deflate_apply_kernel<TV, K, START>), dim3(vb), dim3(kBlock), 0, s.stream, sc, (const double *)part, db, M,
                       (const TV *)Wa, pitch, mm, (TV *)u_apply, n, coeff, ncoeff);
    if (counted) LAUNCHED(c); else HIPCHK(c, hipGetLastError());
    return 0;
}

// P = x0 = W Ginv (W^T b), column by column, from 0 (every column: the scalars are not initialised yet)
template <typename TV, int K>
int deflate_start(lam_hip_ctx *c)
{
    MultiState &m = c->multi;
    const DeflateState &d = m.df;
    return deflate_launch<TV, K, true>(c, nullptr, d.W, d.W, d.pitch, d.m, d.Ginv, m.B, m.P, c->n, d.part, nullptr, 0, false);
}

// p -= W Ginv ((AW)^T r) for the columns still running
template <typename TV, int K>
int deflate_project(lam_hip_ctx *c, bool counted)
{
    MultiState &m = c->multi;
    const DeflateState &d = m.df;
    return deflate_launch<TV, K, false>(c, m.sc, d.AW, d.W, d.pitch, d.m, d.Ginv, m.R, m.P, c->n, d.part, nullptr, 0, counted);
}

// What both setters do behind their checks: `src` holds mm vectors of n elements, vector i at src + i * n (host, or the device's Ritz
// vectors).  Builds W, A W and Ginv aside and swaps them in; a refusal leaves the space there was.
int deflate_build(lam_hip_ctx *c, const char *fn, int mm, const void *src, hipMemcpyKind kind)
{
    ShardBase &s = c->sh[0];
    LAMCHK(set_dev(c, s));
    LAMCHK(multi_ensure(c));
    LAMCHK(deflate_part_ensure(c));
    MultiState &m = c->multi;
    DeflateState &d = m.df;
    HIPCHK(c, hipStreamSynchronize(s.stream));
    m.solved = m.ms.valid = false;        // the batch's product scratch is overwritten, as by lam_hip_gemv_many
    const size_t ev = c->esz_v();
    const uint64_t n = c->n, pitch = lanczos_pitch(n, ev);
    const size_t bytes = (size_t)mm * pitch * ev;
    DevBuf W, AW, G, Ginv;
    HIPCHK(c, hipMalloc(&W.p, bytes));
    HIPCHK(c, hipMalloc(&AW.p, bytes));
    HIPCHK(c, hipMalloc(&G.p, sizeof(double) * (size_t)mm * mm));
    HIPCHK(c, hipMalloc(&Ginv.p, sizeof(double) * (size_t)mm * mm));
    // a row is the product's input as it stands: zero behind element n
    HIPCHK(c, hipMemsetAsync(W.p, 0, bytes, s.stream));
    HIPCHK(c, hipMemsetAsync(AW.p, 0, bytes, s.stream));
    HIPCHK(c, hipMemcpy2DAsync(W.p, pitch * ev, src, n * ev, n * ev, (size_t)mm, kind, s.stream));
    const int vb = vec_grid(n), db = deflate_dots_blocks(n);
    // A W by the batch's product launch site, a group of columns at a time; G's columns of the group behind it
    const int group = multi_sym_wanted(c, kSymvManyMaxK) ? kSymvManyMaxK : kMaxRhs;
    for (int first = 0; first < mm; first += group) {
        const int count = std::min(group, mm - first), K = multi_k_for(count);
        m.last_K = K;
        LAMCHK(pack_many_maybe(c, K));
        LAMCHK(multi_dispatch(c, K, [&](auto impl, auto kc) -> int {
            using I = decltype(impl);
            using TA = typename ImplTraits<I>::TA;
            using TV = typename ImplTraits<I>::TV;
            constexpr int KK = decltype(kc)::value;
            hipLaunchKernelGGL((deflate_gather_kernel<TV, KK>), dim3(vb), dim3(kBlock), 0, s.stream, (const TV *)W.p + (uint64_t)first * pitch,
                               pitch, count, (TV *)m.P, n);
            HIPCHK(c, hipGetLastError());
            LAMCHK((multi_launch_gemv<TA, TV, KK>(c, (const TV *)m.P, (TV *)m.AP, nullptr, nullptr)));
            hipLaunchKernelGGL((deflate_scatter_kernel<TV, KK>), dim3(vb), dim3(kBlock), 0, s.stream, (const TV *)m.AP, count,
                               (TV *)AW.p + (uint64_t)first * pitch, pitch, n);
            HIPCHK(c, hipGetLastError());
            hipLaunchKernelGGL((deflate_dots_kernel<TV, KK>), dim3(db, kDeflateSplit), dim3(kBlock), 0, s.stream, (const MultiScalars *)nullptr,
                               (const TV *)W.p, pitch, mm, (const TV *)m.AP, n, d.part);
            HIPCHK(c, hipGetLastError());
            hipLaunchKernelGGL((deflate_gram_kernel<KK>), dim3(1), dim3(kBlock), 0, s.stream, (const double *)d.part, db, mm, count,
                               G.as<double>() + first, mm);
            HIPCHK(c, hipGetLastError());
            return 0;
        }));
    }
    std::vector<double> g((size_t)mm * mm), gs((size_t)mm * mm), gi((size_t)mm * mm);
    HIPCHK(c, hipMemcpyAsync(g.data(), G.p, sizeof(double) * g.size(), hipMemcpyDeviceToHost, s.stream));
    HIPCHK(c, hipStreamSynchronize(s.stream));
    double dmax = 0.0;
    for (int i = 0; i < mm; i++) {
        for (int j = 0; j < mm; j++) gs[(size_t)i * mm + j] = 0.5 * (g[(size_t)i * mm + j] + g[(size_t)j * mm + i]);
        dmax = std::fmax(dmax, gs[(size_t)i * mm + i]);
    }
    // a pivot at the size of the rounding error of G's own entries: W is numerically rank-deficient (lam_hip_eigs' breakdown rule)
    const double floor = (double)n * lanczos_unit_roundoff(c) * dmax;
    int bad = -1;
    if (lam::chol_inverse(mm, gs.data(), gi.data(), floor, &bad) != 0)
        return fail(c, LAM_HIP_EINVAL, "%s: W^T A W is not positive definite to working precision at column %d (its pivot is not finite or "
                    "<= N * u * max_i G_ii = %g): W is rank-deficient there, or holds a non-finite value, or A is not positive definite "
                    "on it", fn, bad, floor);
    HIPCHK(c, hipMemcpyAsync(Ginv.p, gi.data(), sizeof(double) * gi.size(), hipMemcpyHostToDevice, s.stream));
    HIPCHK(c, hipStreamSynchronize(s.stream));      // gi is pageable
    free_dev({d.W, d.AW, d.Ginv});
    d.W = W.p; d.AW = AW.p; d.Ginv = (double *)Ginv.p;
    W.p = AW.p = Ginv.p = nullptr;
    d.m = mm;
    d.pitch = pitch;
    d.gen = c->matrix_gen;
    return 0;
}

void deflate_clear(lam_hip_ctx *c)
{
    DeflateState &d = c->multi.df;
    if (d.W && !c->sh.empty() && hipSetDevice(c->sh[0].dev) == hipSuccess) {
        if (c->sh[0].stream) (void)hipStreamSynchronize(c->sh[0].stream);
        free_dev({d.W, d.AW, d.Ginv});
    }
    d.W = d.AW = nullptr;
    d.Ginv = nullptr;
    d.m = 0;
    d.gen = ~0ull;
}

// what both setters check first, in this order
int deflate_set_checks(lam_hip_ctx *c, const char *fn, int mm)
{
    LAMCHK(multi_supported(c, fn));
    if (!c->have_problem || !c->have_matrix) return fail(c, LAM_HIP_ESTATE, "matrix must be set before %s", fn);
    const int cap = (int)std::min<uint64_t>(c->n, LAM_HIP_MAX_DEFLATION);
    if (mm < 0 || mm > cap) return fail(c, LAM_HIP_EINVAL, "%s: m = %d, must be 0..%d (min(N, LAM_HIP_MAX_DEFLATION))", fn, mm, cap);
    return 0;
}

}  // namespace

extern "C" {

int lam_hip_chol_inverse(int m, const double *G, double *Ginv, int *bad_col)
{
    if (bad_col) *bad_col = -1;
    if (!G || !Ginv) return LAM_HIP_EINVAL;
    try {
        return lam::chol_inverse(m, G, Ginv, 0.0, bad_col) == 0 ? 0 : LAM_HIP_EINVAL;
    } catch (const std::bad_alloc &) {
        return LAM_HIP_ENOMEM;
    }
}

int lam_hip_set_deflation(lam_hip_ctx *c, int mm, const void *W_host)
{
    if (!c) return LAM_HIP_EINVAL;
    const char *const fn = "lam_hip_set_deflation";
    LAMCHK(deflate_set_checks(c, fn, mm));
    if (mm == 0) { deflate_clear(c); return 0; }
    if (!W_host) return fail(c, LAM_HIP_EINVAL, "%s: W_host is NULL", fn);
    const uint64_t total = (uint64_t)mm * c->n;
    for (uint64_t e = 0; e < total; e++) {
        const double v = c->dtype == LAM_HIP_F64 ? ((const double *)W_host)[e] : (double)((const float *)W_host)[e];
        if (!std::isfinite(v))
            return fail(c, LAM_HIP_EINVAL, "%s: vector %llu, element %llu is %g: W must be finite", fn, (unsigned long long)(e / c->n),
                        (unsigned long long)(e % c->n), v);
    }
    return deflate_build(c, fn, mm, W_host, hipMemcpyHostToDevice);
}

int lam_hip_set_deflation_eigs(lam_hip_ctx *c, int mm)
{
    if (!c) return LAM_HIP_EINVAL;
    const char *const fn = "lam_hip_set_deflation_eigs";
    LAMCHK(deflate_set_checks(c, fn, mm));
    if (mm == 0) { deflate_clear(c); return 0; }
    LAMCHK(lanczos_readable(c, fn, mm));
    return deflate_build(c, fn, mm, c->multi.lz.Y, hipMemcpyDeviceToDevice);
}

int lam_hip_solve_many_deflated(lam_hip_ctx *c, int max_iters, double rel_error, lam_hip_stats *st, int32_t *num_iters, int32_t *converged,
                                double *rel_err)
{
    if (!c) return LAM_HIP_EINVAL;
    const char *const fn = "lam_hip_solve_many_deflated";
    LAMCHK(multi_solve_checks(c, fn, LAM_HIP_PC_NONE, max_iters));
    if (!deflate_valid(c))
        return fail(c, LAM_HIP_ESTATE, "%s: no deflation space is set for the matrix held now (lam_hip_set_deflation, "
                    "lam_hip_set_deflation_eigs; a new matrix invalidates the space)", fn);
    const MultiState &m = c->multi;
    for (int j = 0; j < m.nrhs; j++)
        if (m.shift[j] != 0.0)
            return fail(c, LAM_HIP_EINVAL, "%s: shift %d in force is %g: the deflation space belongs to A, not to A + s I; clear the "
                        "shifts (lam_hip_set_shifts_many)", fn, j, m.shift[j]);
    return multi_solve(c, fn, LAM_HIP_PC_NONE, kGuessDeflated, nullptr, max_iters, rel_error, st, num_iters, converged, rel_err);
}

// The operator alone on host vectors: needs no problem and no matrix; runs on shard 0's device like lam_hip_project_out, for every
// storage type (LAM_HIP_BF16: float vectors).
int lam_hip_deflate_many(lam_hip_ctx *c, uint64_t n, int mm, int nrhs, const void *Wd_host, const void *Wa_host, const double *M, void *U_host,
                         double *coeff)
{
    if (!c) return LAM_HIP_EINVAL;
    const char *const fn = "lam_hip_deflate_many";
    if (!Wd_host || !Wa_host || !M || !U_host) return fail(c, LAM_HIP_EINVAL, "%s: NULL argument", fn);
    if (n < 1) return fail(c, LAM_HIP_EINVAL, "%s: n must be >= 1", fn);
    if (mm < 1 || mm > LAM_HIP_MAX_DEFLATION)
        return fail(c, LAM_HIP_EINVAL, "%s: m = %d, must be 1..%d (LAM_HIP_MAX_DEFLATION)", fn, mm, LAM_HIP_MAX_DEFLATION);
    LAMCHK(multi_check_nrhs(c, fn, nrhs));
    ShardBase &s = c->sh[0];
    LAMCHK(set_dev(c, s));
    const size_t ev = c->esz_v();
    const uint64_t pitch = lanczos_pitch(n, ev);
    const int vb = vec_grid(n), db = deflate_dots_blocks(n), K = multi_k_for(nrhs);
    DevBuf wd, wa, mat, cols, inter, part, co;
    HIPCHK(c, hipMalloc(&wd.p, (size_t)mm * pitch * ev));
    HIPCHK(c, hipMalloc(&wa.p, (size_t)mm * pitch * ev));
    HIPCHK(c, hipMalloc(&mat.p, sizeof(double) * (size_t)mm * mm));
    HIPCHK(c, hipMalloc(&cols.p, (size_t)nrhs * n * ev));
    HIPCHK(c, hipMalloc(&inter.p, (size_t)(n + kMultiPadRows) * K * ev));
    HIPCHK(c, hipMalloc(&part.p, sizeof(double) * (size_t)db * mm * K));
    HIPCHK(c, hipMalloc(&co.p, sizeof(double) * (size_t)mm * nrhs));
    HIPCHK(c, hipMemcpy2DAsync(wd.p, pitch * ev, Wd_host, n * ev, n * ev, (size_t)mm, hipMemcpyHostToDevice, s.stream));
    HIPCHK(c, hipMemcpy2DAsync(wa.p, pitch * ev, Wa_host, n * ev, n * ev, (size_t)mm, hipMemcpyHostToDevice, s.stream));
    HIPCHK(c, hipMemcpyAsync(mat.p, M, sizeof(double) * (size_t)mm * mm, hipMemcpyHostToDevice, s.stream));
    HIPCHK(c, hipMemcpyAsync(cols.p, U_host, (size_t)nrhs * n * ev, hipMemcpyHostToDevice, s.stream));
    LAMCHK(dispatch(c, [&](auto impl) -> int {
        using TV = typename ImplTraits<decltype(impl)>::TV;
        auto run = [&](auto kc) -> int {
            constexpr int KK = decltype(kc)::value;
            hipLaunchKernelGGL((multi_interleave_kernel<TV, KK>), dim3(vb), dim3(kBlock), 0, s.stream, (const TV *)cols.p, nrhs, (TV *)inter.p, n);
            HIPCHK(c, hipGetLastError());
            LAMCHK((deflate_launch<TV, KK, false>(c, nullptr, wd.p, wa.p, pitch, mm, mat.as<double>(), inter.p, inter.p, n, part.as<double>(),
                                                  co.as<double>(), nrhs, false)));
            hipLaunchKernelGGL((multi_deinterleave_kernel<TV, KK>), dim3(vb), dim3(kBlock), 0, s.stream, (const TV *)inter.p, nrhs, (TV *)cols.p, n);
            HIPCHK(c, hipGetLastError());
            return 0;
        };
        switch (K) {
        case 1: return run(std::integral_constant<int, 1>());
        case 2: return run(std::integral_constant<int, 2>());
        case 4: return run(std::integral_constant<int, 4>());
        default: return run(std::integral_constant<int, 8>());
        }
    }));
    HIPCHK(c, hipMemcpyAsync(U_host, cols.p, (size_t)nrhs * n * ev, hipMemcpyDeviceToHost, s.stream));
    if (coeff) HIPCHK(c, hipMemcpyAsync(coeff, co.p, sizeof(double) * (size_t)mm * nrhs, hipMemcpyDeviceToHost, s.stream));
    HIPCHK(c, hipStreamSynchronize(s.stream));
    return 0;
}

}  // extern "C"
