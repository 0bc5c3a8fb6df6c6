// lam_iterate.h -- one CG iteration per shard (phases, enqueue), cg_init, the host's view of the progress word, the lag rule.
// Part of the one translation unit csrc/lam_hip.hip (included from there, in order; not a stand-alone header).
#pragma once

namespace {

int do_cg_init(lam_hip_ctx *c)
{
    c->cg_direct = false;
    c->epoch++;
    c->seq_base += c->seq_span;    // hand-over numbers never restart (see seq_base)
    c->seq_span = 1;
    for (auto &sh_ : c->sh) sh_.waited_k = 0;
    if (c->direct_err) memset(c->direct_err, 0, 64);
    LAMCHK(env_symmetric_check(c));
    // how many p.Ap partials the product step leaves (= what the consumer sums) depends on which product runs: settled here, at the
    // one place where that is decided (options, a refused / re-admitted symmetric product)
    for (auto &sh_ : c->sh)
        sh_.gemv_blocks = dispatch(c, [&](auto impl) -> int { return decltype(impl)::gemv_grid(c, sh_.nrows); });
    if (c->exchange2_wanted()) {
        // the state is initialised through RCCL (one-off); the iterations then run on the mailboxes
        LAMCHK(setup_direct(c));
        c->cg_direct = c->direct_ok;
    }
    // The fused vector step (one shard; the direct exchange) is a launch whose workgroups wait for each other: used
    // only when the whole grid (compute workgroups + reducer + waiter) can be resident at once, else the two-kernel form.
    // The gather-Ap exchange has a fused vector step of its own (update_full_fused_kernel, full-length r and p).
    c->fuse_active = false;
    const bool ex1 = !c->cg_direct && c->exchange1_ok();
    if (c->opt_fuse && c->opt_finalize && (c->cg_direct || ex1 || (!c->rank_mode && c->total_shards == 1))) {
        ShardBase &s0 = c->sh[0];
        LAMCHK(set_dev(c, s0));
        c->fuse_active = dispatch(c, [&](auto impl) -> int {
            using TV = typename ImplTraits<decltype(impl)>::TV;
            if (ex1) return full_fused_launch_resident<TV>(c) ? 1 : 0;
            return fused_launch_resident<TV>(c, s0, s0.vec_blocks + 2) ? 1 : 0;
        }) == 1;
    }
    if (c->fuse_active)
        for (auto &sh_ : c->sh) LAMCHK(ensure_mail(c, sh_, nullptr));
    if (c->exchange1_ok()) return do_cg_init_exchange1(c);
    c->cg_exchange1 = false;
    return dispatch(c, [&](auto impl) -> int {
        using TV = typename ImplTraits<decltype(impl)>::TV;
        PtrList pl = plist_p(c);
        for (auto &s : c->sh) {
            LAMCHK(set_dev(c, s));
            hipLaunchKernelGGL((cg_init_kernel<TV>), dim3(s.vec_blocks), dim3(kBlock), 0, s.stream, (const TV *)s.b,
                               (TV *)s.x, (TV *)s.r, pl, s.row0, s.nrows, s.part_vec);
            HIPCHK(c, hipGetLastError());
        }
        LAMCHK(reduce_step(c, /*second=*/true, /*gemv_part=*/false, /*check_stop=*/false, /*finalized=*/false));
        for (auto &s : c->sh) {
            LAMCHK(set_dev(c, s));
            const double *red; int nred;
            red_source(c, s, true, false, /*finalized=*/false, &red, &nred);
            hipLaunchKernelGGL(cg_init_scalars_kernel, dim3(1), dim3(kBlock), 0, s.stream, red, nred, s.sc);
            HIPCHK(c, hipGetLastError());
        }
        LAMCHK(gather_p_step(c));
        LAMCHK(arm_partials(c));
        c->k_done = 0;
        c->cg_ready = true;
        return 0;
    });
}

// ---- the general iteration, one shard at a time -------------------------------------------------------------------
// Four phases per shard; between two phases every shard must have ISSUED the previous one (its event records are
// what the next phase's stream waits refer to).  One host thread: phase by phase over all shards.
//   A  GEMV (+ partial p.Ap; the product step's helpers are lam_exchange.h's) and its post
//   B  wait for the peers' p.Ap; x, r update (+ partial r.r); post
//   C  wait for the peers' r.r; stop test + p update into every replica; post        D  wait for the peers' p slices
template <typename I>
int phase_gemv(lam_hip_ctx *c, ShardBase &s, int k, int slot)
{
    using TV = typename ImplTraits<I>::TV;
    if (c->symv_active()) {
        LAMCHK(timed_product(c, s, k, slot, false, [&] { return I::launch_symv(c, s, (const TV *)s.p, (TV *)s.Ap, s.part_gemv, s.sc); }));
    } else {
        // with an own-slice panel the wait for the all-gather of p comes behind that panel (launch_split_gemv)
        uint64_t lo, hi;
        cg_panel<I>(c, s, &lo, &hi);
        LAMCHK(launch_split_gemv<I>(c, s, k, slot, lo, hi, make_finalize(c, s, false), [&]() -> int {
            if (c->gather_pending) WAITEV(c, s.stream, s.ev_gathered);
            return 0;
        }));
    }
    return reduce_post(c, s, false, true, true, producer_reduces(c, false));
}

template <typename I>
int phase_xr(lam_hip_ctx *c, ShardBase &s, int k, double rel_error)
{
    using TV = typename ImplTraits<I>::TV;
    const bool fin_a = producer_reduces(c, false), fin_b = producer_reduces(c, true);
    LAMCHK(reduce_wait(c, s, false));
    const double *red; int nred;
    red_source(c, s, false, true, fin_a, &red, &nred);
    if (c->fuse_active) {
        // one shard: phases B and C in ONE launch; the r.r total travels through the context's own mailbox
        const unsigned long long seq = c->seq_base + (unsigned)k;
        c->seq_span = std::max<uint64_t>(c->seq_span, (uint64_t)k + 1);
        Finalize fr = no_finalize(c);
        fr.active = 1; fr.seq = seq;                 // one shard: the total goes straight to the broadcast slot
        BlockCounts nb;
        for (auto &v : nb.n) v = 0;
        hipLaunchKernelGGL((update_fused_kernel<TV>), dim3(s.vec_blocks + 1), dim3(kBlock), 0, s.stream, red, nred, s.sc, k, rel_error,
                           (const TV *)s.p + s.row0, (const TV *)s.Ap, (TV *)s.x, (TV *)s.r, s.nrows, s.part_vec, s.vec_blocks, fr,
                           MailWait{nullptr, 0, 0, nullptr}, MailWait{s.mail->rr, 1, seq, c->direct_err}, s.bcast, plist_p(c), s.row0,
                           (volatile int *)s.host_flags, no_post(), (const Mail *)s.mail, nb);
        LAUNCHED(c);
        return 0;
    }
    const Finalize fb = make_finalize(c, s, true);
    hipLaunchKernelGGL((update_xr_kernel<TV>), dim3(s.vec_blocks + (fb.active ? 1 : 0)), dim3(kBlock), 0, s.stream, red, nred,
                       s.sc, k, (const TV *)s.p + s.row0, (const TV *)s.Ap, (TV *)s.x, (TV *)s.r, s.nrows, s.part_vec, fb,
                       MailWait{nullptr, 0, 0, nullptr});
    LAUNCHED(c);
    return reduce_post(c, s, true, false, true, fin_b);
}

template <typename I>
int phase_p(lam_hip_ctx *c, ShardBase &s, int k, double rel_error)
{
    using TV = typename ImplTraits<I>::TV;
    if (c->fuse_active) return 0;
    const bool fin_b = producer_reduces(c, true);
    LAMCHK(reduce_wait(c, s, true));
    const double *red; int nred;
    red_source(c, s, true, false, fin_b, &red, &nred);
    hipLaunchKernelGGL((update_p_kernel<TV>), dim3(s.vec_blocks), dim3(kBlock), 0, s.stream, red, nred, s.sc, k,
                       rel_error, (const TV *)s.r, (const TV *)s.p + s.row0, plist_p(c), s.row0, s.nrows,
                       (volatile int *)s.host_flags, MailWait{nullptr, 0, 0, nullptr}, no_post());
    LAUNCHED(c);
    return gather_post(c, s);
}

int enqueue_iteration_body(lam_hip_ctx *c, int k, double rel_error, int slot);

// one iteration, all local shards; if its GEMV is timed, so are its exchange steps (xt_begin / xt_end, shard 0)
int enqueue_iteration(lam_hip_ctx *c, int k, double rel_error, int slot)
{
    ShardBase &s0 = c->sh[0];
    s0.nx[slot] = 0;
    c->xt_slot = timed_iteration(c, s0, k) ? slot : -1;
    const int rc = enqueue_iteration_body(c, k, rel_error, slot);
    c->xt_slot = -1;
    return rc;
}

int enqueue_iteration_body(lam_hip_ctx *c, int k, double rel_error, int slot)
{
    if (c->cg_direct) return enqueue_iteration_direct(c, k, rel_error, slot);
    if (c->cg_exchange1) return enqueue_iteration_exchange1(c, k, rel_error, slot);
    return dispatch(c, [&](auto impl) -> int {
        using I = decltype(impl);
        for (auto &s : c->sh) {
            LAMCHK(set_dev(c, s));
            LAMCHK(phase_gemv<I>(c, s, k, slot));
        }
        c->gather_pending = false;
        for (auto &s : c->sh) {
            LAMCHK(set_dev(c, s));
            LAMCHK(phase_xr<I>(c, s, k, rel_error));
        }
        if (c->fuse_active) return 0;
        for (auto &s : c->sh) {
            LAMCHK(set_dev(c, s));
            LAMCHK(phase_p<I>(c, s, k, rel_error));
        }
        if (c->rank_mode) return gather_p_rank(c);
        for (auto &s : c->sh) {
            LAMCHK(set_dev(c, s));
            LAMCHK(gather_wait(c, s));
        }
        return 0;
    });
}

// ---- the host's view of the iteration's progress -----------------------------------------------------------------
struct Progress { int iters, stop_at; };
Progress read_progress(const ShardBase &s)
{
    const unsigned long long v = *reinterpret_cast<volatile unsigned long long *>(s.host_flags);
    return {(int)(unsigned)(v & 0xffffffffull), (int)(unsigned)(v >> 32)};
}

// Wait until iteration `target` has made its stop decision (update_p_kernel's progress word in pinned memory), or
// some iteration has stopped, or a bounded in-kernel wait has expired.  No event per iteration is involved: an event
// record is a marker packet between the iteration's kernels.  A stream error (a fault, a lost device) ends the wait.
// The host does not burn a core while it waits (round 4; in rank mode that was one spinning core per GPU next to RCCL's
// proxy threads): after a short spin -- an iteration that is about to report costs nothing -- it SLEEPS between polls,
// for a quarter of the iteration time observed so far (clamped to 20 us .. 1 ms).  The host enqueues kLag iterations
// ahead of the one it awaits, so a wake-up that comes a whole iteration late is still free: the queue never drains.
// `precise` = the wait that ENDS a call (for the last enqueued iteration): there a late wake-up is latency of the call -- a
// 1 ms nap too many is 1 % of a 20-iteration run at N=65536 -- so the naps shrink with the time the awaited iteration is
// expected to need (half of it at a time, from the observed iteration time and the moment the progress word last moved) and
// the last ~300 us are polled.
int await_progress(lam_hip_ctx *c, ShardBase &s0, int target, Progress *out, bool precise = false)
{
    unsigned polls = 0;
    double t_query = 0.0, t_change = 0.0;
    int last_iters = -1;
    for (;;) {
        const Progress pr = read_progress(s0);
        if (precise && pr.iters != last_iters) { last_iters = pr.iters; t_change = now_s(); }
        if (pr.iters >= target || pr.stop_at != 0 || *(volatile int *)c->direct_err != 0) {
            // iteration-time estimate: progress made since the previous successful wait / time since then
            const double t = now_s();
            if (c->prog_t > 0.0 && pr.iters > c->prog_iter && pr.stop_at == 0) {
                const double per = (t - c->prog_t) / (double)(pr.iters - c->prog_iter);
                // smoothed, but a jump by more than 2x (another problem size, another exchange) is taken at once: a stale
                // estimate would oversleep and drain the queue
                const double e = c->iter_est_s;
                c->iter_est_s = (e > 0.0 && per < 2.0 * e && per > 0.5 * e) ? 0.75 * e + 0.25 * per : per;
            }
            c->prog_t = t;
            c->prog_iter = pr.iters;
            *out = pr;
            return 0;
        }
        if (++polls <= 64u) { __builtin_ia32_pause(); continue; }
        const double t = now_s();
        if (t_query == 0.0) t_query = t;
        // Liveness: look at the stream only after 0.25 s of waiting for ONE iteration (a fault, a lost device).  Not more often:
        // a hipStreamQuery on a busy stream makes a helper thread of the runtime wait ACTIVELY for the stream's outstanding
        // signal -- called every 2 ms it kept a second core busy for the whole solve at N=65536 (tools/thread_cpu.py).
        if (t - t_query > 0.25) {
            t_query = t;
            const hipError_t e = hipStreamQuery(s0.stream);
            if (e == hipSuccess) {
                // everything enqueued has run: the word is final (it may have been written since the read above)
                const Progress again = read_progress(s0);
                if (again.iters >= target || again.stop_at != 0 || *(volatile int *)c->direct_err != 0) { *out = again; return 0; }
                return fail(c, LAM_HIP_EHIP, "iteration %d was enqueued but never reported (progress word at %d)", target, again.iters);
            }
            if (e != hipErrorNotReady) return fail(c, LAM_HIP_EHIP, "stream error while iterating: %s", hipGetErrorString(e));
        }
        // Iterations shorter than ~60 us (N below ~7000 on one GPU): a sleep cannot be shorter than the kernel's timer slack
        // (~50 us), i.e. several iterations, and the queue would drain -- keep polling, yielding the core between polls; such
        // solves are short.  Otherwise sleep a quarter of an iteration (at most 1 ms).
        if (c->iter_est_s > 0.0 && c->iter_est_s < 60e-6) {
            if ((polls & 63u) == 0) sched_yield(); else __builtin_ia32_pause();
            continue;
        }
        double nap = std::min(1e-3, std::max(15e-6, 0.25 * c->iter_est_s));
        if (precise) {
            const double est = c->iter_est_s;
            const double left = est > 0.0 ? (double)(target - pr.iters - 1) * est + std::max(0.0, est - (t - t_change)) : 0.0;
            if (left < 300e-6) {                         // nearly there (or nothing known yet): poll
                if ((polls & 63u) == 0) sched_yield(); else __builtin_ia32_pause();
                continue;
            }
            nap = std::min(1e-3, 0.5 * left);
        }
        struct timespec ts = {0, (long)(nap * 1e9)};
        (void)nanosleep(&ts, nullptr);
    }
}

// GEMV device time of the iteration that used ring slot `slot`, per local shard, if that iteration was timed; for shard 0 also the
// time of its exchange steps (xt_begin / xt_end pairs)
struct IterTimes {
    double gemv_ms[kMaxShards] = {};
    int samples[kMaxShards] = {};
    double xch_ms = 0.0;
};
static void harvest_shard(ShardBase &s, int j, int slot, IterTimes *t)
{
    if (!s.timed_slot[slot]) return;
    s.timed_slot[slot] = false;
    const int nx = j == 0 ? s.nx[slot] : 0;
    if (j == 0) s.nx[slot] = 0;
    float ms = 0.f, ms2 = 0.f;
    if (hipEventElapsedTime(&ms, s.ev_g0[slot], s.ev_g1[slot]) != hipSuccess) { (void)hipGetLastError(); return; }
    if (s.split_slot[slot] && hipEventElapsedTime(&ms2, s.ev_g2[slot], s.ev_g3[slot]) != hipSuccess) { (void)hipGetLastError(); return; }
    double xms = 0.0;
    for (int q = 0; q < nx; q++) {
        float x = 0.f;
        hipError_t e = hipEventElapsedTime(&x, s.ev_x[slot][2 * q], s.ev_x[slot][2 * q + 1]);
        if (e == hipErrorNotReady) {
            // the all-gather of p runs on the comm stream and may still be in flight when its iteration has reported (a few
            // microseconds: the next GEMV's second panel waits for it)
            (void)hipGetLastError();
            if (hipEventSynchronize(s.ev_x[slot][2 * q + 1]) == hipSuccess) e = hipEventElapsedTime(&x, s.ev_x[slot][2 * q], s.ev_x[slot][2 * q + 1]);
        }
        if (e != hipSuccess) { (void)hipGetLastError(); return; }
        xms += x;
    }
    t->gemv_ms[j] += ms + ms2;
    t->samples[j]++;
    if (j == 0) t->xch_ms += xms;
}
// all local shards (the caller's current device is restored to shard 0's)
static void harvest_times(lam_hip_ctx *c, int slot, IterTimes *t)
{
    for (size_t j = 0; j < c->sh.size(); j++) {
        if (!c->sh[j].timed_slot[slot]) continue;
        if (c->sh.size() > 1 && set_dev(c, c->sh[j]) != 0) continue;
        harvest_shard(c->sh[j], (int)j, slot, t);
    }
    if (c->sh.size() > 1) (void)set_dev(c, c->sh[0]);
}

// The lag rule (every enqueue loop uses it).  Before enqueueing iteration k the host makes sure iteration k - kLag
// has reported, then looks at the stopping iteration the update kernel left in pinned memory.  Later iterations may
// or may not have finished by now -- that depends on how far this rank's GPU is ahead of its host -- so the value
// only counts if it names an iteration whose report has been AWAITED: stop_at <= k - kLag.  A stop at iteration j
// is therefore acted on at k = j + kLag on every rank, whatever the timing: all ranks enqueue the same number of
// (no-op) iterations and their collectives stay matched.  (The reference broadcasts the decision instead:
// MPI_Bcast(&stop), ConjugateGradient_MultiGPUS_CUDA_NCCL.cu:404-407.)
// Returns 0 go on, 1 stop here, 2 a bounded in-kernel wait expired (reported after the final sync), < 0 error.
static int lag_check(lam_hip_ctx *c, ShardBase &s0, int k)
{
    Progress pr;
    LAMCHK(await_progress(c, s0, k - kLag, &pr));
    if (*(volatile int *)c->direct_err != 0) return 2;
    // LAM_HIP_DEBUG_LEVEL_STOP: test hook that restores the timing-dependent decision ("any stop seen so far") so
    // that the stream-ordered RCCL test double can be shown to catch the rank desynchronisation it causes
    // (tests/test_gpu_rank_mock.py).  Never set it otherwise.
    static const bool level_stop = getenv("LAM_HIP_DEBUG_LEVEL_STOP") != nullptr;
    return (pr.stop_at != 0 && (pr.stop_at <= k - kLag || level_stop)) ? 1 : 0;
}

}  // namespace
