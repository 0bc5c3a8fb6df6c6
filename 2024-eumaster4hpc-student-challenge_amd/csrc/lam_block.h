// lam_block.h -- block CG for the batch, host side: lam_hip_solve_block, lam_hip_block_factor.  Kernels: lam_kernels.h ("Block CG");
// the s x s matrices: lam_host_block.h (host and device); the recurrence: include/lam_hip.h.  Part of the one translation unit
// csrc/lam_hip.hip (included from there behind lam_multi.h, whose state, product launch site and driver it uses; not a stand-alone
// header).
//
// The vectors are MultiState's own -- B, X, R (as Q), P, AP (as Z) -- so the batch holds a batched solution afterwards.  In front of
// the loop: one block_gram_kernel launch for B^T B, whose partials the host sums (in block_pair_sums' order) and factors, so that a
// rank-deficient block is refused before anything is iterated; then block_init_kernel.  An iteration is multi_drive's product
// launch plus block_gram_kernel, block_step_kernel and block_dir_kernel.
#pragma once

static_assert(lam::kBlockMaxS == LAM_HIP_MAX_RHS, "include/lam_hip.h states the limit");

namespace {

int block_ensure(lam_hip_ctx *c)
{
    BlockState &b = c->multi.bk;
    if (b.sc) return 0;
    free_dev({b.part_h, b.part_g});          // what a failed attempt left: it is retried, never launched on
    b = BlockState();
    const size_t bytes = sizeof(double) * kVecBlocksMax * (size_t)block_pairs<kMaxRhs>();
    HIPCHK(c, hipMalloc((void **)&b.part_h, bytes));
    HIPCHK(c, hipMalloc((void **)&b.part_g, bytes));
    HIPCHK(c, hipMalloc((void **)&b.sc, sizeof(BlockScalars)));
    HIPCHK(c, hipMemsetAsync(b.sc, 0, sizeof(BlockScalars), c->sh[0].stream));
    return 0;
}

// G (s x s) from the nred partials of the K-wide upper triangle, in the order of block_pair_sums
void block_host_pair_sums(const std::vector<double> &part, int nred, int K, int s, double *G)
{
    const int NP = K * (K + 1) / 2;
    int t = 0;
    for (int i = 0; i < K; i++)
        for (int j = i; j < K; j++, t++) {
            double w[kWaves];
            for (int q = 0; q < kWaves; q++) {
                w[q] = 0.0;
                for (int b = q; b < nred; b += kWaves) w[q] += part[(size_t)b * NP + t];
            }
            double a = w[0];
            for (int q = 1; q < kWaves; q++) a += w[q];
            if (j < s) G[i * s + j] = G[j * s + i] = a;
        }
}

}  // namespace

extern "C" {

int lam_hip_block_factor(int s, int dtype, const double *G, double *Ginv, double *S, double *Sinv, int *bad_col)
{
    if (bad_col) *bad_col = -1;
    if (!G || s < 1 || s > LAM_HIP_MAX_RHS || (dtype != LAM_HIP_F64 && dtype != LAM_HIP_F32)) return LAM_HIP_EINVAL;
    constexpr int SS = kMaxRhs * kMaxRhs;
    double l[SS], d[kMaxRhs], gi[SS], su[SS], si[SS];
    const double floor = lam::block_pivot_floor(s, dtype == LAM_HIP_F32, G);
    int bad = -1;
    if (lam::block_ldlt_inverse(s, G, floor, l, d, gi, &bad) != 0 || lam::block_upper(s, G, floor, su, si, &bad) != 0) {
        if (bad_col) *bad_col = bad;
        return LAM_HIP_EINVAL;
    }
    const size_t bytes = sizeof(double) * (size_t)s * s;
    if (Ginv) memcpy(Ginv, gi, bytes);
    if (S) memcpy(S, su, bytes);
    if (Sinv) memcpy(Sinv, si, bytes);
    return 0;
}

int lam_hip_solve_block(lam_hip_ctx *c, int max_iters, double rel_error, lam_hip_stats *st, int32_t *num_iters, int32_t *converged,
                        double *rel_err, int32_t *breakdown)
{
    if (!c) return LAM_HIP_EINVAL;
    const char *const fn = "lam_hip_solve_block";
    LAMCHK(multi_solve_checks(c, fn, LAM_HIP_PC_NONE, max_iters));
    MultiState &m = c->multi;
    for (int j = 0; j < m.nrhs; j++)
        if (m.shift[j] != 0.0)
            return fail(c, LAM_HIP_EINVAL, "%s: shift %d in force is %g: the columns of a block share one operator; clear the shifts "
                        "(lam_hip_set_shifts_many)", fn, j, m.shift[j]);
    const double t0 = now_s();
    ShardBase &s0 = c->sh[0];
    LAMCHK(set_dev(c, s0));
    HIPCHK(c, hipStreamSynchronize(s0.stream));
    LAMCHK(block_ensure(c));
    BlockState &bk = m.bk;
    m.solved = false;
    m.ms.valid = false;
    const int vb = vec_grid(c->n), s = m.nrhs;
    BatchTiming timing;
    LAMCHK(multi_dispatch(c, m.K, [&](auto impl, auto kc) -> int {
        using I = decltype(impl);
        using TA = typename ImplTraits<I>::TA;
        using TV = typename ImplTraits<I>::TV;
        constexpr int K = decltype(kc)::value;
        constexpr int NP = block_pairs<K>();
        TV *const B = (TV *)m.B, *const X = (TV *)m.X, *const Q = (TV *)m.R, *const P = (TV *)m.P, *const Z = (TV *)m.AP;
        // G = B^T B, factored on the host: the refusal comes before anything is iterated
        hipLaunchKernelGGL((block_gram_kernel<TV, K>), dim3(vb), dim3(kBlock), 0, s0.stream, (const MultiScalars *)nullptr, (const TV *)B,
                           (const TV *)B, c->n, bk.part_h);
        HIPCHK(c, hipGetLastError());
        std::vector<double> part((size_t)vb * NP);
        HIPCHK(c, hipMemcpyAsync(part.data(), bk.part_h, sizeof(double) * part.size(), hipMemcpyDeviceToHost, s0.stream));
        HIPCHK(c, hipStreamSynchronize(s0.stream));
        BlockMat G = {}, C = {}, Cinv = {}, bb = {};
        block_host_pair_sums(part, vb, K, s, G.a);
        for (int j = 0; j < s; j++) bb.a[j] = G.a[j * s + j];
        int bad = -1;
        const double floor = lam::block_pivot_floor(s, c->dtype == LAM_HIP_F32, G.a);
        if (lam::block_upper(s, G.a, floor, C.a, Cinv.a, &bad) != 0)
            return fail(c, LAM_HIP_EINVAL, "%s: B^T B is not positive definite to working precision at column %d (its pivot is not finite "
                        "or <= nrhs * u * max_j b_j.b_j = %g): the column is zero, or a combination of the columns in front of it "
                        "(nrhs > N included), or holds a non-finite value", fn, bad, floor);
        auto init = [&]() -> int {
            hipLaunchKernelGGL((block_init_kernel<TV, K>), dim3(vb), dim3(kBlock), 0, s0.stream, (const TV *)B, X, Q, P, c->n, s, C, Cinv,
                               bb, bk.sc, (volatile int *)m.host_flags);
            HIPCHK(c, hipGetLastError());
            return 0;
        };
        auto rest = [&](int k) -> int {
            hipLaunchKernelGGL((block_gram_kernel<TV, K>), dim3(vb), dim3(kBlock), 0, s0.stream, (const MultiScalars *)bk.sc, (const TV *)P,
                               (const TV *)Z, c->n, bk.part_h);
            LAUNCHED(c);
            hipLaunchKernelGGL((block_step_kernel<TV, K>), dim3(vb), dim3(kBlock), 0, s0.stream, (const double *)bk.part_h, vb, bk.sc, k, s,
                               (const TV *)P, (const TV *)Z, X, Q, c->n, bk.part_g, (volatile int *)m.host_flags);
            LAUNCHED(c);
            hipLaunchKernelGGL((block_dir_kernel<TV, K>), dim3(vb), dim3(kBlock), 0, s0.stream, (const double *)bk.part_g, vb, bk.sc, k, s,
                               rel_error, Q, P, c->n, (volatile int *)m.host_flags);
            LAUNCHED(c);
            return 0;
        };
        return multi_drive<TA, TV, K>(c, max_iters, (const TV *)P, Z, bk.sc, nullptr, init, rest, &timing);
    }));
    const std::unique_ptr<BlockScalars> h(new BlockScalars);
    HIPCHK(c, hipMemcpyAsync(h.get(), bk.sc, sizeof(BlockScalars), hipMemcpyDeviceToHost, s0.stream));
    HIPCHK(c, hipStreamSynchronize(s0.stream));
    m.solved = true;
    const double t1 = now_s();
    const int ran = h->iters;            // completed iterations: a breakdown of kind 1 ends iteration bd_iter before its update
    int all_conv = 1;
    double worst = 0.0;
    bool any_nan = false;
    for (int j = 0; j < s; j++) {
        const double re = h->rel_err[j];
        const int cv = re < rel_error;
        if (num_iters) num_iters[j] = h->first_hit[j] != 0 ? h->first_hit[j] : max_iters + 1;
        if (converged) converged[j] = cv;
        if (rel_err) rel_err[j] = re;
        all_conv = all_conv && cv;
        if (re != re) any_nan = true; else worst = std::max(worst, re);
    }
    if (breakdown) { breakdown[0] = h->bd_iter; breakdown[1] = h->bd_kind; }
    if (st) {
        memset(st, 0, sizeof *st);
        st->num_iters = ran;
        st->converged = all_conv;
        st->rel_err = any_nan ? std::nan("") : worst;
        st->t_total = t1 - t0;
        st->t_iter = ran > 0 ? (t1 - t0) / ran : 0.0;
        st->t_gemv = timing.samples > 0 ? timing.gemv_ms * 1e-3 / timing.samples : 0.0;
        st->t_comm_init = c->t_comm_init;
        st->gemv_bytes = multi_gemv_bytes(c, m.K);
    }
    return 0;
}

}  // extern "C"
