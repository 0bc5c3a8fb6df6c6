// lam_quad.h -- stochastic Lanczos quadrature for the batch: lam_hip_lanczos_many, lam_hip_get_lanczos_many,
// lam_hip_trace_quadrature and lam_hip_tridiag_quadrature.  Kernels: lam_kernels.h ("Batched Lanczos quadrature"); the quadrature
// itself: lam_host_quad.h (host only); the recurrence: include/lam_hip.h.  Part of the one translation unit csrc/lam_hip.hip (included
// from there behind lam_multi.h, whose product launch site, state, driver and helpers it uses; not a stand-alone header).
//
// A group of up to 8 probes (4 where option "symmetric_many" engages) is one pass of multi_drive: init = the upload or the probe
// launches, rest(k) = the two vector launches behind the product of step k; behind the group the device block (scalars and the
// coefficient history) comes back with one copy.  What the host keeps is what the getters and the quadrature serve.
#pragma once

static_assert(LAM_HIP_MAX_PROBES == 8 * LAM_HIP_MAX_RHS, "include/lam_hip.h states the limit as 8 groups of LAM_HIP_MAX_RHS");
static_assert(lam::kQuadLog == LAM_HIP_QUAD_LOG && lam::kQuadInv == LAM_HIP_QUAD_INV && lam::kQuadPow == LAM_HIP_QUAD_POW,
              "include/lam_hip.h states the functions");

namespace {

// the device block for the batch's n (multi_ensure has run)
int quad_ensure(lam_hip_ctx *c)
{
    QuadState &q = c->multi.qd;
    if (q.sc) return 0;
    HIPCHK(c, hipMalloc((void **)&q.sc, sizeof(QuadScalars)));
    HIPCHK(c, hipMemsetAsync(q.sc, 0, sizeof(QuadScalars), c->sh[0].stream));
    return 0;
}

int quad_readable(lam_hip_ctx *c)
{
    const QuadState &q = c->multi.qd;
    if (!q.valid || !c->have_matrix) return fail(c, LAM_HIP_ESTATE, "no Lanczos coefficients yet (lam_hip_lanczos_many)");
    return 0;
}

const char *quad_fn_name(int fn) { return fn == LAM_HIP_QUAD_LOG ? "log" : (fn == LAM_HIP_QUAD_INV ? "1/t" : "t^p"); }

}  // namespace

extern "C" {

int lam_hip_tridiag_quadrature(int k, const double *alpha, const double *beta, int fn, double param, int nshifts, const double *sigma,
                               double *out, int *bad)
{
    try {
        lam::QuadBad b;
        const int rc = lam::tridiag_quadrature(k, alpha, beta, fn, param, nshifts, sigma, out, &b);
        if (bad) { bad[0] = b.shift; bad[1] = b.node; }
        if (rc == 0) return 0;
        if (rc == -4)
            return fail(nullptr, LAM_HIP_EINVAL, "lam_hip_tridiag_quadrature: node %d under shift %d is %g: f(t) = %s cannot take it", b.node,
                        b.shift, b.value, quad_fn_name(fn));
        if (rc == -3) return fail(nullptr, LAM_HIP_EINVAL, "lam_hip_tridiag_quadrature: param = %g, LAM_HIP_QUAD_POW needs an integer >= 0", param);
        if (rc == -2) return fail(nullptr, LAM_HIP_EINVAL, "lam_hip_tridiag_quadrature: a coefficient or a shift is not finite");
        return fail(nullptr, LAM_HIP_EINVAL, "lam_hip_tridiag_quadrature: k = %d outside 1..%d (LAM_HIP_MAX_LANCZOS), nshifts = %d < 1, a NULL "
                    "array or an unknown function %d", k, LAM_HIP_MAX_LANCZOS, nshifts, fn);
    } catch (const std::bad_alloc &) {
        return LAM_HIP_ENOMEM;
    }
}

int lam_hip_lanczos_many(lam_hip_ctx *c, int nprobes, const void *z_host, uint64_t seed, int steps, lam_hip_stats *st, int32_t *steps_run,
                         double *znorm2, double *alpha, double *beta)
{
    if (!c) return LAM_HIP_EINVAL;
    const char *const fn = "lam_hip_lanczos_many";
    LAMCHK(multi_supported(c, fn));
    if (nprobes < 1 || nprobes > LAM_HIP_MAX_PROBES)
        return fail(c, LAM_HIP_EINVAL, "%s: nprobes = %d, must be 1..%d (LAM_HIP_MAX_PROBES)", fn, nprobes, LAM_HIP_MAX_PROBES);
    if (!c->have_problem || !c->have_matrix) return fail(c, LAM_HIP_ESTATE, "matrix must be set before %s", fn);
    const int cap = (int)std::min<uint64_t>(c->n, LAM_HIP_MAX_LANCZOS);
    if (steps < 1 || steps > cap) return fail(c, LAM_HIP_EINVAL, "%s: steps = %d, must be 1..%d (min(N, LAM_HIP_MAX_LANCZOS))", fn, steps, cap);
    const size_t ev = c->esz_v();
    if (z_host) {
        // a probe the recurrence cannot start from: its norm in fp64 (the device's own z.z is what znorm2 reports)
        for (int j = 0; j < nprobes; j++) {
            double zz = 0.0;
            for (uint64_t i = 0; i < c->n; i++) {
                const double v = c->dtype == LAM_HIP_F64 ? ((const double *)z_host)[(uint64_t)j * c->n + i]
                                                         : (double)((const float *)z_host)[(uint64_t)j * c->n + i];
                zz += v * v;
            }
            if (!(zz > 0.0) || !std::isfinite(zz))
                return fail(c, LAM_HIP_EINVAL, "%s: probe %d has squared norm %g: it must be finite and > 0", fn, j, zz);
        }
    }

    const double t0 = now_s();
    ShardBase &s0 = c->sh[0];
    LAMCHK(set_dev(c, s0));
    LAMCHK(multi_ensure(c));
    LAMCHK(quad_ensure(c));
    MultiState &m = c->multi;
    QuadState &q = m.qd;
    HIPCHK(c, hipStreamSynchronize(s0.stream));
    m.solved = m.ms.valid = q.valid = false;      // the batch's P, AP and R are overwritten, as by lam_hip_gemv_many
    q.nprobes = nprobes;
    q.steps = steps;
    q.steps_run.assign((size_t)nprobes, 0);
    q.znorm2.assign((size_t)nprobes, std::nan(""));
    q.alpha.assign((size_t)nprobes * steps, std::nan(""));
    q.beta.assign((size_t)nprobes * steps, std::nan(""));

    const int vb = vec_grid(c->n);
    const double scale = (double)c->n * lanczos_unit_roundoff(c);
    // lam_hip_set_deflation's grouping rule for A W: 4 columns where the symmetric batched product engages for K <= 4
    const int group = multi_sym_wanted(c, kSymvManyMaxK) ? kSymvManyMaxK : kMaxRhs;
    const std::unique_ptr<QuadScalars> h(new QuadScalars);
    BatchTiming timing;
    int last_K = 1, last_ran = 0, most = 0;
    double t_last = 0.0;
    bool finite = true;
    const int saved_K = m.K;
    for (int first = 0; first < nprobes; first += group) {
        const int count = std::min(group, nprobes - first), K = multi_k_for(count);
        const int gb = multi_product_blocks(c, K);
        timing = BatchTiming();
        const double tg = now_s();
        m.K = K;                   // multi_drive reports the K it ran ("multi_rhs_k"); the right-hand sides' own K is put back below
        const int rc = multi_dispatch(c, K, [&](auto impl, auto kc) -> int {
            using I = decltype(impl);
            using TA = typename ImplTraits<I>::TA;
            using TV = typename ImplTraits<I>::TV;
            constexpr int KK = decltype(kc)::value;
            TV *const V = (TV *)m.P, *const U = (TV *)m.AP, *const VOLD = (TV *)m.R;
            auto init = [&]() -> int {
                if (z_host) LAMCHK(multi_upload(c, count, KK, (const char *)z_host + (size_t)first * c->n * ev, V));
                hipLaunchKernelGGL((quad_probe_kernel<TV, KK>), dim3(vb), dim3(kBlock), 0, s0.stream, z_host == nullptr, count, (uint64_t)first,
                                   seed, V, c->n, m.part_vec);
                HIPCHK(c, hipGetLastError());
                hipLaunchKernelGGL((quad_start_scalars_kernel<KK>), dim3(1), dim3(kBlock), 0, s0.stream, (const double *)m.part_vec, vb, count,
                                   q.sc, (volatile int *)m.host_flags);
                HIPCHK(c, hipGetLastError());
                hipLaunchKernelGGL((quad_start_kernel<TV, KK>), dim3(vb), dim3(kBlock), 0, s0.stream, V, VOLD, c->n, (const QuadScalars *)q.sc);
                HIPCHK(c, hipGetLastError());
                return 0;
            };
            auto rest = [&](int k) -> int {
                hipLaunchKernelGGL((quad_three_term_kernel<TV, KK>), dim3(vb), dim3(kBlock), 0, s0.stream, (const double *)m.part_gemv, gb, q.sc,
                                   k, (const TV *)V, (const TV *)VOLD, U, c->n, m.part_vec);
                LAUNCHED(c);
                hipLaunchKernelGGL((quad_next_kernel<TV, KK>), dim3(vb), dim3(kBlock), 0, s0.stream, (const double *)m.part_vec, vb, q.sc, k,
                                   scale, (const TV *)U, V, VOLD, c->n, (volatile int *)m.host_flags);
                LAUNCHED(c);
                return 0;
            };
            return multi_drive<TA, TV, KK>(c, steps, (const TV *)V, U, q.sc, nullptr, init, rest, &timing);
        });
        m.K = saved_K;
        m.last_K = K;
        LAMCHK(rc);
        HIPCHK(c, hipMemcpyAsync(h.get(), q.sc, sizeof(QuadScalars), hipMemcpyDeviceToHost, s0.stream));
        HIPCHK(c, hipStreamSynchronize(s0.stream));
        t_last = now_s() - tg;
        last_K = K;
        last_ran = 0;
        for (int j = 0; j < count; j++) {
            const int p = first + j, ran = std::min(std::max(h->steps_run[j], 0), steps);
            q.steps_run[(size_t)p] = ran;
            q.znorm2[(size_t)p] = h->zz[j];
            for (int k = 0; k < ran; k++) {
                const double a = h->hist_alpha[(size_t)k * K + j], b = h->hist_beta[(size_t)k * K + j];
                q.alpha[(size_t)p * steps + k] = a;
                q.beta[(size_t)p * steps + k] = b;
                finite = finite && std::isfinite(a) && std::isfinite(b);
            }
            last_ran = std::max(last_ran, ran);
            most = std::max(most, ran);
        }
    }
    q.valid = true;
    for (int j = 0; j < nprobes; j++) {
        if (steps_run) steps_run[j] = q.steps_run[(size_t)j];
        if (znorm2) znorm2[j] = q.znorm2[(size_t)j];
    }
    if (alpha) memcpy(alpha, q.alpha.data(), sizeof(double) * q.alpha.size());
    if (beta) memcpy(beta, q.beta.data(), sizeof(double) * q.beta.size());
    if (st) {
        memset(st, 0, sizeof *st);
        st->num_iters = most;
        st->converged = finite ? 1 : 0;
        st->rel_err = 0.0;
        st->t_total = now_s() - t0;
        st->t_iter = last_ran > 0 ? t_last / last_ran : 0.0;
        st->t_gemv = timing.samples > 0 ? timing.gemv_ms * 1e-3 / timing.samples : 0.0;
        st->t_comm_init = c->t_comm_init;
        st->gemv_bytes = multi_gemv_bytes(c, last_K);
    }
    return 0;
}

int lam_hip_get_lanczos_many(lam_hip_ctx *c, int nprobes, int32_t *steps, int32_t *steps_run, double *znorm2, double *alpha, double *beta)
{
    if (!c) return LAM_HIP_EINVAL;
    const char *const fn = "lam_hip_get_lanczos_many";
    LAMCHK(multi_supported(c, fn));
    LAMCHK(quad_readable(c));
    const QuadState &q = c->multi.qd;
    if (nprobes < 1 || nprobes > q.nprobes) return fail(c, LAM_HIP_EINVAL, "%s: nprobes = %d, %d probes were run", fn, nprobes, q.nprobes);
    if (steps) *steps = q.steps;
    for (int j = 0; j < nprobes; j++) {
        if (steps_run) steps_run[j] = q.steps_run[(size_t)j];
        if (znorm2) znorm2[j] = q.znorm2[(size_t)j];
    }
    if (alpha) memcpy(alpha, q.alpha.data(), sizeof(double) * (size_t)nprobes * q.steps);
    if (beta) memcpy(beta, q.beta.data(), sizeof(double) * (size_t)nprobes * q.steps);
    return 0;
}

int lam_hip_trace_quadrature(lam_hip_ctx *c, int fn_id, double param, int nshifts, const double *sigma, double *estimate, double *std_error,
                             double *per_probe)
{
    if (!c) return LAM_HIP_EINVAL;
    const char *const fn = "lam_hip_trace_quadrature";
    LAMCHK(multi_supported(c, fn));
    if (fn_id != LAM_HIP_QUAD_LOG && fn_id != LAM_HIP_QUAD_INV && fn_id != LAM_HIP_QUAD_POW)
        return fail(c, LAM_HIP_EINVAL, "%s: fn = %d, must be LAM_HIP_QUAD_LOG, LAM_HIP_QUAD_INV or LAM_HIP_QUAD_POW", fn, fn_id);
    if (nshifts < 1 || nshifts > LAM_HIP_MAX_SHIFTS)
        return fail(c, LAM_HIP_EINVAL, "%s: nshifts = %d, must be 1..%d (LAM_HIP_MAX_SHIFTS)", fn, nshifts, LAM_HIP_MAX_SHIFTS);
    if (!sigma && nshifts != 1) return fail(c, LAM_HIP_EINVAL, "%s: sigma is NULL with nshifts = %d (NULL means the one shift 0)", fn, nshifts);
    LAMCHK(quad_readable(c));
    const QuadState &q = c->multi.qd;
    try {
        std::vector<double> val((size_t)nshifts * q.nprobes), one((size_t)nshifts);
        for (int j = 0; j < q.nprobes; j++) {
            lam::QuadBad b;
            const int rc = lam::tridiag_quadrature(q.steps_run[(size_t)j], &q.alpha[(size_t)j * q.steps], &q.beta[(size_t)j * q.steps], fn_id, param,
                                                   nshifts, sigma, one.data(), &b);
            if (rc == -4)
                return fail(c, LAM_HIP_EINVAL, "%s: probe %d, shift %d (%g): node %d is %g, which f(t) = %s cannot take (A + sigma I is not "
                            "positive definite on the probe's Krylov space)", fn, j, b.shift, sigma ? sigma[b.shift] : 0.0, b.node, b.value,
                            quad_fn_name(fn_id));
            if (rc == -3) return fail(c, LAM_HIP_EINVAL, "%s: param = %g, LAM_HIP_QUAD_POW needs an integer >= 0", fn, param);
            if (rc == -2) return fail(c, LAM_HIP_EINVAL, "%s: probe %d holds a non-finite coefficient, or a shift is not finite", fn, j);
            if (rc != 0) return fail(c, LAM_HIP_EINVAL, "%s: probe %d completed %d steps", fn, j, q.steps_run[(size_t)j]);
            for (int s = 0; s < nshifts; s++) val[(size_t)s * q.nprobes + j] = q.znorm2[(size_t)j] * one[(size_t)s];
        }
        for (int s = 0; s < nshifts; s++) {
            double mean, err;
            lam::quad_mean_error(q.nprobes, &val[(size_t)s * q.nprobes], &mean, &err);
            if (estimate) estimate[s] = mean;
            if (std_error) std_error[s] = err;
        }
        if (per_probe) memcpy(per_probe, val.data(), sizeof(double) * val.size());
    } catch (const std::bad_alloc &) {
        return fail(c, LAM_HIP_ENOMEM, "%s: out of host memory", fn);
    }
    return 0;
}

}  // extern "C"
