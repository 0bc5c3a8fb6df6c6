// lam_eigs.h -- the Lanczos eigensolver's host side: lam_hip_eigs and its getters, lam_hip_project_out, lam_hip_tridiag_eigen.
// Kernels: lam_kernels.h ("Lanczos"); the small eigenproblem: lam_host_tridiag.h (host only); the recurrence: include/lam_hip.h.
// Part of the one translation unit csrc/lam_hip.hip (included from there behind lam_multi.h, whose product launch site, state and
// helpers it uses; not a stand-alone header).
//
// A step is the K = 1 product launch of the batch (multi_launch_gemv: the general product, or the two launches of the symmetric
// batched product under option "symmetric_many") on basis row v_k, and kLanczosLaunches launches of this file.  Steps are enqueued in
// chunks of check_every; behind each chunk the stream is drained, the scalars are read back and the host decides.
#pragma once

static_assert(lam::kMaxLanczos == LAM_HIP_MAX_LANCZOS, "include/lam_hip.h states the limit");

namespace {

constexpr int kLanczosLaunches = 6;   // three-term, (dots, apply) twice, append: include/lam_hip.h states 1 + 6 per step

// basis rows: a 256-byte multiple of n + kMultiPadRows elements
uint64_t lanczos_pitch(uint64_t n, size_t ev)
{
    const uint64_t bytes = ((n + kMultiPadRows) * ev + 255) / 256 * 256;
    return bytes / ev;
}

// slabs of lanczos_dots_kernel: a quarter of the vector kernels' workgroups, each with kLanczosSplit workgroups to deal the basis rows
// out to -- fewer partials per row for lanczos_apply_kernel to sum, more workgroups on the stream of V
int lanczos_dots_blocks(uint64_t n) { return std::max(1, vec_grid(n) / 4); }

// the unit roundoff of the vector dtype (fp64 / fp32 only: multi_supported)
double lanczos_unit_roundoff(const lam_hip_ctx *c) { return c->dtype == LAM_HIP_F64 ? 0x1p-53 : 0x1p-24; }

// the state for the batch's n (multi_ensure has run) and max_steps steps: grow-only, all of it or none
int lanczos_ensure(lam_hip_ctx *c, int max_steps)
{
    LanczosState &z = c->multi.lz;
    ShardBase &s = c->sh[0];
    if (z.sc && max_steps <= z.cap) return 0;
    HIPCHK(c, hipStreamSynchronize(s.stream));
    free_dev({z.V, z.U, z.Y, z.part, z.part_uu, z.S, z.sc});
    z = LanczosState();
    const size_t ev = c->esz_v();
    const uint64_t pitch = lanczos_pitch(c->n, ev);
    const size_t vbytes = (size_t)(max_steps + 1) * pitch * ev;
    HIPCHK(c, hipMalloc(&z.V, vbytes));
    HIPCHK(c, hipMalloc(&z.U, (size_t)(c->n + kMultiPadRows) * ev));
    HIPCHK(c, hipMalloc(&z.Y, (size_t)max_steps * c->n * ev));
    HIPCHK(c, hipMalloc((void **)&z.part, sizeof(double) * (size_t)(max_steps + 1) * kVecBlocksMax));
    HIPCHK(c, hipMalloc((void **)&z.part_uu, sizeof(double) * kVecBlocksMax));
    HIPCHK(c, hipMalloc((void **)&z.S, sizeof(double) * (size_t)max_steps * max_steps));
    HIPCHK(c, hipMalloc((void **)&z.sc, sizeof(LanczosScalars)));
    // a basis row is the product's input as it stands: zero behind element n, and the kernels write elements below n only
    HIPCHK(c, hipMemsetAsync(z.V, 0, vbytes, s.stream));
    HIPCHK(c, hipMemsetAsync(z.sc, 0, sizeof(LanczosScalars), s.stream));
    HIPCHK(c, hipStreamSynchronize(s.stream));
    z.cap = max_steps;
    z.pitch = pitch;
    return 0;
}

// positions in the ascending spectrum of k values of the `count` pairs `which` asks for, in the order it reports them
void lanczos_wanted(int which, int nev, int k, int count, int *idx)
{
    int ns = which == LAM_HIP_EIG_SMALLEST ? count : (which == LAM_HIP_EIG_LARGEST ? 0 : std::min((nev + 1) / 2, count));
    for (int i = 0; i < ns; i++) idx[i] = i;
    for (int i = ns; i < count; i++) idx[i] = k - 1 - (i - ns);
}

int lanczos_readable(lam_hip_ctx *c, const char *fn, int nev)
{
    const MultiState &m = c->multi;
    if (!m.lz.valid || m.n != c->n) return fail(c, LAM_HIP_ESTATE, "no eigen-solution yet (lam_hip_eigs)");
    if (nev < 1 || nev > m.lz.nfound) return fail(c, LAM_HIP_EINVAL, "%s: nev = %d, %d pairs were found", fn, nev, m.lz.nfound);
    return 0;
}

}  // namespace

extern "C" {

int lam_hip_tridiag_eigen(int k, const double *alpha, const double *beta, double *theta, double *last_row, double *S)
{
    try {
        return lam::tridiag_eigen(k, alpha, beta, theta, last_row, S) == 0 ? 0 : LAM_HIP_EINVAL;
    } catch (const std::bad_alloc &) {
        return LAM_HIP_ENOMEM;
    }
}

int lam_hip_eigs(lam_hip_ctx *c, int which, int nev, int max_steps, double tol, int check_every, const void *v0_host, uint64_t seed,
                 lam_hip_stats *st, int32_t *nfound_out, double *theta_out, double *bound_out, int32_t *converged_out)
{
    if (!c) return LAM_HIP_EINVAL;
    const char *const fn = "lam_hip_eigs";
    LAMCHK(multi_supported(c, fn));
    if (which != LAM_HIP_EIG_SMALLEST && which != LAM_HIP_EIG_LARGEST && which != LAM_HIP_EIG_BOTH)
        return fail(c, LAM_HIP_EINVAL, "%s: which = %d, must be LAM_HIP_EIG_SMALLEST, LAM_HIP_EIG_LARGEST or LAM_HIP_EIG_BOTH", fn, which);
    if (check_every < 1) return fail(c, LAM_HIP_EINVAL, "%s: check_every = %d, must be >= 1", fn, check_every);
    if (!c->have_problem || !c->have_matrix) return fail(c, LAM_HIP_ESTATE, "matrix must be set before %s", fn);
    const int cap = (int)std::min<uint64_t>(c->n, LAM_HIP_MAX_LANCZOS);
    if (max_steps < 1 || max_steps > cap)
        return fail(c, LAM_HIP_EINVAL, "%s: max_steps = %d, must be 1..%d (min(N, LAM_HIP_MAX_LANCZOS))", fn, max_steps, cap);
    if (nev < 1 || nev > max_steps) return fail(c, LAM_HIP_EINVAL, "%s: nev = %d, must be 1..max_steps = %d", fn, nev, max_steps);

    const double t0 = now_s();
    ShardBase &s0 = c->sh[0];
    LAMCHK(set_dev(c, s0));
    LAMCHK(multi_ensure(c));
    LAMCHK(lanczos_ensure(c, max_steps));
    MultiState &m = c->multi;
    LanczosState &z = m.lz;
    HIPCHK(c, hipStreamSynchronize(s0.stream));
    m.solved = m.ms.valid = z.valid = false;      // the batch's product scratch is overwritten, as by lam_hip_gemv_many
    m.last_K = 1;
    m.host_flags[0] = m.host_flags[1] = 0;
    for (int i = 0; i < kLag; i++) m.timed_slot[i] = false;

    const int vb = vec_grid(c->n), gb = multi_product_blocks(c, 1), db = lanczos_dots_blocks(c->n);
    const size_t ev = c->esz_v();
    const double scale = (double)c->n * lanczos_unit_roundoff(c);
    if (v0_host) HIPCHK(c, hipMemcpyAsync(z.U, v0_host, c->n * ev, hipMemcpyHostToDevice, s0.stream));
    BatchTiming timing;
    const std::unique_ptr<LanczosScalars> h(new LanczosScalars);
    std::vector<double> theta(max_steps), row(max_steps), bound(nev), th_w(nev);
    std::vector<int> idx(nev), conv(nev);
    int steps = 0, nfound = 0;
    double theta_norm = 0.0, worst = 0.0, t_loop = 0.0;
    bool all_conv = false;

    LAMCHK(multi_dispatch(c, 1, [&](auto impl, auto) -> int {
        using I = decltype(impl);
        using TA = typename ImplTraits<I>::TA;
        using TV = typename ImplTraits<I>::TV;
        TV *const V = (TV *)z.V, *const U = (TV *)z.U;
        auto row_of = [&](int j) { return V + (uint64_t)j * z.pitch; };
        auto read_scalars = [&]() -> int {
            HIPCHK(c, hipMemcpyAsync(h.get(), z.sc, sizeof(LanczosScalars), hipMemcpyDeviceToHost, s0.stream));
            HIPCHK(c, hipStreamSynchronize(s0.stream));
            return 0;
        };
        // the start vector: given, or lam_hip_generate_random_rhs's law; normalised on the device
        if (!v0_host) {
            hipLaunchKernelGGL((gen_rhs_kernel<TV>), dim3(vb), dim3(kBlock), 0, s0.stream, U, (uint64_t)0, c->n, 1, seed, 0.0);
            HIPCHK(c, hipGetLastError());
        }
        hipLaunchKernelGGL((dot_partial_kernel<TV>), dim3(vb), dim3(kBlock), 0, s0.stream, (const TV *)U, (const TV *)U, c->n, z.part_uu);
        HIPCHK(c, hipGetLastError());
        hipLaunchKernelGGL((lanczos_start_kernel<TV>), dim3(vb), dim3(kBlock), 0, s0.stream, (const double *)z.part_uu, vb, z.sc, (const TV *)U,
                           row_of(0), c->n, (volatile int *)m.host_flags);
        HIPCHK(c, hipGetLastError());
        LAMCHK(read_scalars());
        if (!(h->v0norm > 0.0) || !std::isfinite(h->v0norm))
            return fail(c, LAM_HIP_EINVAL, "%s: the start vector's norm is %g: it must be finite and > 0", fn, h->v0norm);

        const double tl0 = now_s();
        bool done = false;
        while (!done) {
            const int chunk = std::min(check_every, max_steps - steps);
            for (int q = 1; q <= chunk; q++) {
                const int step = steps + q, k = step - 1, slot = k % kLag, mm = k + 1;
                LAMCHK(pack_many_maybe(c, 1));          // option "packed_many": in front of the product step, outside its event pair
                const double te = now_s();
                if (m.timed_slot[slot]) {
                    HIPCHK(c, hipEventSynchronize(m.ev1[slot]));
                    multi_harvest(m, slot, &timing);
                }
                const bool timed = timed_iteration(c, s0, step);
                m.timed_slot[slot] = timed;
                if (timed) RECORD(c, m.ev0[slot], s0.stream);
                LAMCHK((multi_launch_gemv<TA, TV, 1>(c, (const TV *)row_of(k), U, m.part_gemv, z.sc)));
                if (timed) RECORD(c, m.ev1[slot], s0.stream);
                hipLaunchKernelGGL((lanczos_three_term_kernel<TV>), dim3(vb), dim3(kBlock), 0, s0.stream, (const double *)m.part_gemv, gb, z.sc,
                                   step, (const TV *)row_of(k), (const TV *)(k > 0 ? row_of(k - 1) : nullptr), U, c->n);
                LAUNCHED(c);
                for (int pass = 0; pass < 2; pass++) {
                    hipLaunchKernelGGL((lanczos_dots_kernel<TV>), dim3(db, kLanczosSplit), dim3(kBlock), 0, s0.stream, (const LanczosScalars *)z.sc, step,
                                       (const TV *)V, z.pitch, mm, (const TV *)U, c->n, z.part);
                    LAUNCHED(c);
                    if (pass == 0)
                        hipLaunchKernelGGL((lanczos_apply_kernel<TV, false>), dim3(vb), dim3(kBlock), 0, s0.stream, (const LanczosScalars *)z.sc,
                                           step, (const double *)z.part, db, (const TV *)V, z.pitch, mm, U, c->n, (double *)nullptr,
                                           (double *)nullptr);
                    else
                        hipLaunchKernelGGL((lanczos_apply_kernel<TV, true>), dim3(vb), dim3(kBlock), 0, s0.stream, (const LanczosScalars *)z.sc,
                                           step, (const double *)z.part, db, (const TV *)V, z.pitch, mm, U, c->n, (double *)nullptr, z.part_uu);
                    LAUNCHED(c);
                }
                hipLaunchKernelGGL((lanczos_append_kernel<TV>), dim3(vb), dim3(kBlock), 0, s0.stream, (const double *)z.part_uu, vb, z.sc, step,
                                   scale, (const TV *)U, row_of(k + 1), c->n, (volatile int *)m.host_flags);
                LAUNCHED(c);
                c->enqueue_ns += (uint64_t)((now_s() - te) * 1e9);
            }
            // the convergence test, on the host: theta and the bottom row of T_k's eigenvector matrix from a sweep that carries one row
            LAMCHK(read_scalars());
            const bool broke = h->stopped_at != 0;
            steps = broke ? h->stopped_at : steps + chunk;
            if (lam::tridiag_eigen(steps, h->alpha, h->beta, theta.data(), row.data(), nullptr) != 0)
                return fail(c, LAM_HIP_EINVAL, "%s: the Lanczos coefficients of step %d are not finite (a NaN or an Inf in the matrix or the "
                            "start vector)", fn, steps);
            theta_norm = std::max(std::fabs(theta[0]), std::fabs(theta[steps - 1]));
            nfound = std::min(nev, steps);
            lanczos_wanted(which, nev, steps, nfound, idx.data());
            all_conv = nfound == nev;
            worst = 0.0;
            for (int i = 0; i < nfound; i++) {
                th_w[i] = theta[idx[i]];
                bound[i] = h->beta[steps - 1] * std::fabs(row[idx[i]]);
                conv[i] = broke || bound[i] <= tol * theta_norm;
                all_conv = all_conv && conv[i];
                worst = std::max(worst, bound[i] / theta_norm);
            }
            done = broke || steps >= max_steps || (tol > 0.0 && all_conv);
        }
        for (int j = 0; j < kLag; j++)
            if (m.timed_slot[j]) multi_harvest(m, j, &timing);
        t_loop = now_s() - tl0;

        // the Ritz vectors of the wanted pairs: the full eigenvector matrix once, its wanted columns to the device, one launch
        std::vector<double> S((size_t)steps * steps), Sw((size_t)nfound * steps);
        if (lam::tridiag_eigen(steps, h->alpha, h->beta, theta.data(), nullptr, S.data()) != 0)
            return fail(c, LAM_HIP_EINVAL, "%s: the Lanczos coefficients are not finite", fn);
        for (int i = 0; i < nfound; i++) memcpy(&Sw[(size_t)i * steps], &S[(size_t)idx[i] * steps], sizeof(double) * steps);
        HIPCHK(c, hipMemcpyAsync(z.S, Sw.data(), sizeof(double) * Sw.size(), hipMemcpyHostToDevice, s0.stream));
        hipLaunchKernelGGL((lanczos_ritz_kernel<TV>), dim3(vb, nfound), dim3(kBlock), 0, s0.stream, (const TV *)V, z.pitch, steps,
                           (const double *)z.S, (TV *)z.Y, c->n);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(s0.stream));      // Sw is pageable
        return 0;
    }));

    z.steps = steps;
    z.nfound = nfound;
    z.alpha.assign(h->alpha, h->alpha + steps);
    z.beta.assign(h->beta, h->beta + steps);
    z.theta.assign(th_w.begin(), th_w.begin() + nfound);
    z.valid = true;
    if (nfound_out) *nfound_out = nfound;
    for (int i = 0; i < nev; i++) {
        const bool have = i < nfound;
        if (theta_out) theta_out[i] = have ? th_w[i] : std::nan("");
        if (bound_out) bound_out[i] = have ? bound[i] : std::nan("");
        if (converged_out) converged_out[i] = have && conv[i] ? 1 : 0;
    }
    if (st) {
        memset(st, 0, sizeof *st);
        st->num_iters = steps;
        st->converged = all_conv ? 1 : 0;
        st->rel_err = worst;
        st->t_total = now_s() - t0;
        st->t_iter = steps > 0 ? t_loop / steps : 0.0;
        st->t_gemv = timing.samples > 0 ? timing.gemv_ms * 1e-3 / timing.samples : 0.0;
        st->t_comm_init = c->t_comm_init;
        st->gemv_bytes = multi_gemv_bytes(c, 1);
    }
    return 0;
}

int lam_hip_get_lanczos(lam_hip_ctx *c, int32_t *steps, double *alpha, double *beta)
{
    if (!c) return LAM_HIP_EINVAL;
    LAMCHK(multi_supported(c, "lam_hip_get_lanczos"));
    const LanczosState &z = c->multi.lz;
    if (!z.valid || c->multi.n != c->n) return fail(c, LAM_HIP_ESTATE, "no eigen-solution yet (lam_hip_eigs)");
    if (steps) *steps = z.steps;
    for (int i = 0; i < z.steps; i++) {
        if (alpha) alpha[i] = z.alpha[i];
        if (beta) beta[i] = z.beta[i];
    }
    return 0;
}

int lam_hip_get_eigenvectors(lam_hip_ctx *c, int nev, void *y_host)
{
    if (!c) return LAM_HIP_EINVAL;
    const char *const fn = "lam_hip_get_eigenvectors";
    LAMCHK(multi_supported(c, fn));
    if (!y_host) return fail(c, LAM_HIP_EINVAL, "%s: y_host is NULL", fn);
    LAMCHK(lanczos_readable(c, fn, nev));
    ShardBase &s = c->sh[0];
    LAMCHK(set_dev(c, s));
    HIPCHK(c, hipMemcpyAsync(y_host, c->multi.lz.Y, (size_t)nev * c->n * c->esz_v(), hipMemcpyDeviceToHost, s.stream));
    HIPCHK(c, hipStreamSynchronize(s.stream));
    return 0;
}

// lam_hip_true_residual_mshift's shape: per group of up to 8 Ritz vectors (pair i contiguous at Y + i * n is the host interface's
// layout, so multi_interleave_kernel stages a group in P as it stages an upload) one batched product, then one pass.  B, X and the
// eigen-solution are left alone; P, AP, the partials and MultiState::res are scratch.
int lam_hip_eig_residuals(lam_hip_ctx *c, int nev, double *res)
{
    if (!c) return LAM_HIP_EINVAL;
    const char *const fn = "lam_hip_eig_residuals";
    LAMCHK(multi_supported(c, fn));
    if (!res) return fail(c, LAM_HIP_EINVAL, "%s: res is NULL", fn);
    LAMCHK(lanczos_readable(c, fn, nev));
    if (!c->have_matrix) return fail(c, LAM_HIP_ESTATE, "matrix not set");
    MultiState &m = c->multi;
    const LanczosState &z = m.lz;
    ShardBase &s = c->sh[0];
    LAMCHK(set_dev(c, s));
    const int vb = vec_grid(c->n);
    for (int first = 0; first < nev; first += kMaxRhs) {
        const int count = std::min(kMaxRhs, nev - first), K = multi_k_for(count);
        LanczosTheta th;
        for (int j = 0; j < kMaxRhs; j++) th.t[j] = j < count ? z.theta[first + j] : 0.0;
        double out[kMaxRhs];
        LAMCHK(pack_many_maybe(c, K));
        LAMCHK(multi_dispatch(c, K, [&](auto impl, auto kc) -> int {
            using I = decltype(impl);
            using TA = typename ImplTraits<I>::TA;
            using TV = typename ImplTraits<I>::TV;
            constexpr int KK = decltype(kc)::value;
            hipLaunchKernelGGL((multi_interleave_kernel<TV, KK>), dim3(vb), dim3(kBlock), 0, s.stream,
                               (const TV *)z.Y + (uint64_t)first * c->n, count, (TV *)m.P, c->n);
            HIPCHK(c, hipGetLastError());
            LAMCHK((multi_launch_gemv<TA, TV, KK>(c, (const TV *)m.P, (TV *)m.AP, nullptr, nullptr)));
            hipLaunchKernelGGL((lanczos_residual_kernel<TV, KK>), dim3(vb), dim3(kBlock), 0, s.stream, (const TV *)m.P, (const TV *)m.AP, th,
                               c->n, m.part_rr, m.part_vec);
            HIPCHK(c, hipGetLastError());
            hipLaunchKernelGGL((multi_residual_scalars_kernel<KK>), dim3(1), dim3(kBlock), 0, s.stream, (const double *)m.part_rr,
                               (const double *)m.part_vec, vb, m.res);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipMemcpyAsync(out, m.res, sizeof(double) * KK, hipMemcpyDeviceToHost, s.stream));
            HIPCHK(c, hipStreamSynchronize(s.stream));
            return 0;
        }));
        for (int j = 0; j < count; j++) res[first + j] = out[j];
    }
    return 0;
}

// ONE pass of the solve's reorthogonalisation on host vectors: coeff[j] = V_j.u, u -= sum_j (TV)coeff[j] V_j.  Needs no problem and
// no matrix; runs on shard 0's device like lam_hip_dot, for every storage type (LAM_HIP_BF16: float vectors).
int lam_hip_project_out(lam_hip_ctx *c, uint64_t n, int m, const void *V_host, void *u_host, double *coeff)
{
    if (!c) return LAM_HIP_EINVAL;
    const char *const fn = "lam_hip_project_out";
    if (!V_host || !u_host) return fail(c, LAM_HIP_EINVAL, "%s: NULL vector", fn);
    if (n < 1) return fail(c, LAM_HIP_EINVAL, "%s: n must be >= 1", fn);
    if (m < 1 || m > LAM_HIP_MAX_LANCZOS) return fail(c, LAM_HIP_EINVAL, "%s: m = %d, must be 1..%d (LAM_HIP_MAX_LANCZOS)", fn, m, LAM_HIP_MAX_LANCZOS);
    ShardBase &s = c->sh[0];
    LAMCHK(set_dev(c, s));
    const size_t ev = c->esz_v();
    const uint64_t pitch = lanczos_pitch(n, ev);
    const int vb = vec_grid(n), db = lanczos_dots_blocks(n);
    DevBuf bv, bu, bpart, bc;
    HIPCHK(c, hipMalloc(&bv.p, (size_t)m * pitch * ev));
    HIPCHK(c, hipMalloc(&bu.p, (size_t)(n + kMultiPadRows) * ev));
    HIPCHK(c, hipMalloc(&bpart.p, sizeof(double) * (size_t)m * vb));
    HIPCHK(c, hipMalloc(&bc.p, sizeof(double) * (size_t)m));
    HIPCHK(c, hipMemcpy2DAsync(bv.p, pitch * ev, V_host, n * ev, n * ev, (size_t)m, hipMemcpyHostToDevice, s.stream));
    HIPCHK(c, hipMemcpyAsync(bu.p, u_host, n * ev, hipMemcpyHostToDevice, s.stream));
    LAMCHK(dispatch(c, [&](auto impl) -> int {
        using TV = typename ImplTraits<decltype(impl)>::TV;
        hipLaunchKernelGGL((lanczos_dots_kernel<TV>), dim3(db, kLanczosSplit), dim3(kBlock), 0, s.stream, (const LanczosScalars *)nullptr, 0,
                           (const TV *)bv.p, pitch, m, (const TV *)bu.p, n, bpart.as<double>());
        HIPCHK(c, hipGetLastError());
        hipLaunchKernelGGL((lanczos_apply_kernel<TV, false>), dim3(vb), dim3(kBlock), 0, s.stream, (const LanczosScalars *)nullptr, 0,
                           (const double *)bpart.p, db, (const TV *)bv.p, pitch, m, (TV *)bu.p, n, bc.as<double>(), (double *)nullptr);
        HIPCHK(c, hipGetLastError());
        return 0;
    }));
    HIPCHK(c, hipMemcpyAsync(u_host, bu.p, n * ev, hipMemcpyDeviceToHost, s.stream));
    if (coeff) HIPCHK(c, hipMemcpyAsync(coeff, bc.p, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, s.stream));
    HIPCHK(c, hipStreamSynchronize(s.stream));
    return 0;
}

}  // extern "C"
