// lam_kernels.h -- hand-written gfx950 (CDNA4, wave64) kernels of the dense CG hot path.
//
// Reference counterparts (semantics only; nothing here is derived from that code):
//   gemv / partialDot / reduce / dot / divide / axpy / minusaxpy / xpby CUDA kernels,
//   challenge/main/LAM/src/GPU/distributed/ConjugateGradient_MultiGPUS_CUDA_NCCL.cu:34-238 of the reference
//   and the CPU members dot/axpby/gemv, LAM/src/CPU/ConjugateGradient_CPU_MPI_OMP.hpp:446-508.
//
// Design:
//   * one CG iteration = 3 launches on a shard, 2 where the vector step is fused into one launch -- update_fused_kernel (one
//     shard, direct exchange), update_full_fused_kernel (gather-Ap exchange: the multi-shard default of one process) --:
//       gemv_coop_kernel   Ap_loc = A_loc p          (+ per-workgroup partials of p.Ap)
//       update_xr_kernel   alpha = rr/(p.Ap); x += alpha p; r -= alpha Ap   (+ partials of r.r)
//       update_p_kernel    rr' = r.r; beta = rr'/rr; stop test; p_slice = r + beta p  (stored into
//                          every shard's replicated p)
//     alpha, beta, rr, the stop flag and the iteration counter live in device memory
//     (CgScalars); the host never has to read a scalar to enqueue the next iteration.
//   * the vector step's recurrence -- alpha, the x / r sweep, the gathered p.Ap, beta and the stop test, the p sweep -- is written
//     ONCE, as the device helpers cg_alpha, sweep_xr, gathered_pap, cg_decide, sweep_p and sweep_p_slice at the head of the
//     section "vector kernels".  Its six kernels (two kernels or one launch, on sliced or on full-length vectors) only say which
//     workgroup reduces, computes or waits, where p.Ap and r.r come from and which elements a thread sweeps.  That the forms agree
//     bit for bit holds by construction.
//   * all reductions are two-stage and fixed-order (no floating-point atomics): results are
//     bit-reproducible run to run and identical on every shard.
//   * GEMV is HBM-bound (0.25 flop/B in fp64).  Production shape (gemv_coop_kernel): the 4 waves of a
//     workgroup stream the same 2 matrix rows with 16-byte non-temporal loads, 4 KiB contiguous per row
//     per super-step; the matching 4096-column tile of p is staged once per workgroup in LDS; lane
//     partials are combined with wave64 shuffles and across waves through LDS.  gemv_tile_kernel (one
//     group of 4 rows per wave) is the production shape for bf16 storage; gemv_generic_kernel handles
//     any N / alignment; gemv_mfma_bf16_kernel is the MFMA experiment (slower, tuning build only: bench.py
//     measures it beside the product kernel).  A launch can cover one or two column panels and
//     accumulate, which is how the rank mode overlaps the all-gather of p with its own-slice panel.
//   * the *_full_kernel family implements the single-exchange iteration (gather of Ap, full-length r and p on every shard);
//     symv_*_kernel implement the opt-in symmetric product (every pair {i, j} read once: the upper triangle on one shard,
//     cyclic half windows on several row shards); symv_many_*_kernel are the batch's entry points into the same two bodies (option
//     "symmetric_many", K interleaved columns).
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>

#include <limits>
#include <type_traits>

#include "lam_host_plan.h"
#include "lam_host_pack.h"
#include "lam_host_tridiag.h"
#include "lam_host_quad.h"
#include "lam_host_chol.h"
#include "lam_host_block.h"

namespace lam {

constexpr int kBlock = 256;          // 4 waves of 64
constexpr int kWaves = kBlock / 64;
// 16 zero bytes: what the GEMV lanes past the end of a ragged tile load in place of matrix elements (zero in every element type)
__device__ __attribute__((aligned(16))) const unsigned int kZeroVec16[4] = {0u, 0u, 0u, 0u};
constexpr int kMaxShards = 64;         // shards of one process / ranks of one communicator (the reference's largest published run: 64 GPUs)
constexpr size_t kAgreeBytes = 256 * (size_t)kMaxShards;   // device scratch of the small set-up collectives: one 256-byte record per rank

struct CgScalars {
    double bb;        // b.b
    double rr[2];     // ping-pong: iteration k reads rr[(k+1)&1], writes rr[k&1]
    double pAp;       // last p.Ap (diagnostics)
    double alpha;
    double beta;
    int iters;        // last completed iteration (the converging one once stop is set)
    int stop;         // set by cg_decide (the vector step) when sqrt(rr/bb) < rel_error
};

// ---------------------------------------------------------------------------------------------
// small helpers
// ---------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// Sum over the workgroup; every thread returns the same value.  Fixed order -> deterministic.
__device__ __forceinline__ double block_sum(double v, double *s_red /*[kWaves]*/)
{
    v = wave_sum(v);
    __syncthreads();  // s_red may still be read from a previous call
    if ((threadIdx.x & 63) == 0 && (threadIdx.x >> 6) < kWaves) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = s_red[0];
#pragma unroll
    for (int w = 1; w < kWaves; w++) t += s_red[w];
    return t;
}

// Sum of src[0..n) by one workgroup, identical on every workgroup that calls it.
__device__ __forceinline__ double block_sum_array(const double *__restrict__ src, int n, double *s_red)
{
    // eight independent loads per step (unrolled twice -> 16 in flight): with up to 32768 GEMV
    // partials a one-load-per-step loop is a chain of L2 latencies (measured 19 us per launch, 9.5 us
    // with four).  The order stays fixed, so the sum is reproducible and the same in every workgroup.
    double v = 0.0;
    int i = threadIdx.x;
#pragma unroll 2
    for (; i + 7 * kBlock < n; i += 8 * kBlock) {
        const double a0 = src[i], a1 = src[i + kBlock], a2 = src[i + 2 * kBlock], a3 = src[i + 3 * kBlock];
        const double a4 = src[i + 4 * kBlock], a5 = src[i + 5 * kBlock], a6 = src[i + 6 * kBlock], a7 = src[i + 7 * kBlock];
        v += ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7));
    }
    for (; i < n; i += kBlock) v += src[i];
    return block_sum(v, s_red);
}

// The iteration's progress word in PINNED HOST memory, written by ONE thread per iteration with ONE 8-byte store:
// low half = the iteration just finished, high half = that same iteration if it met the stop test (else 0).  The host
// polls it instead of waiting on an event per iteration (no marker packets between the iteration's kernels); one
// word, so it can never see a new iteration count next to an old stop decision.  After a stop the later (no-op)
// iterations return before writing, so the stopping iteration stays readable.
// post_progress_word writes the word itself -- the one place that knows its format -- and is called directly only for the one
// report that is not an iteration's: a batch whose every column is born stopped (multi_init_scalars_kernel).
__device__ __forceinline__ void post_progress_word(volatile int *host_flags, int iters, int stop_at)
{
    if (host_flags == nullptr) return;
    *reinterpret_cast<volatile unsigned long long *>(host_flags) =
        ((unsigned long long)(unsigned)stop_at << 32) | (unsigned long long)(unsigned)iters;
}

__device__ __forceinline__ void post_progress(volatile int *host_flags, int k, bool stop)
{
    post_progress_word(host_flags, k, stop ? k : 0);
}

struct PtrList {                      // destinations of a replicated store (one per shard)
    void *p[kMaxShards];
    int n;
};

// In-kernel reduction of the per-workgroup partials (more than one shard only).  With one shard the
// consumer kernel sums the partials itself; with several, the shard's partial has to exist as ONE number
// before the exchange, and a separate 1-workgroup launch for that costs a launch + a kernel boundary on
// the iteration's critical path (measured 6.5 us each, profiles/r02_rank_mode_chain.csv).  Instead the
// producer launch carries ONE EXTRA workgroup, the reducer (block gridDim.x-1):
//   * every compute workgroup stores its partial with a single 8-byte agent-scope (sc1, write-through)
//     store and is done -- no fence, no counter, no wait: the value is its own "ready" flag, because the
//     slot held a sentinel (a NaN bit pattern no computation produces) until then;
//   * the reducer polls the slots with sc1 loads in the fixed order of block_sum_array -- so the sum is
//     bit-identical to a separate reduction launch --, writes the total to slot `slot` of every
//     destination and re-arms the slots with the sentinel for the next launch.
// The reducer is dispatched after the compute workgroups and only ever waits for workgroups that are
// already running; its spin is bounded (SpinGuard) and ends in a NaN total, never in a hang.
// (An arrival counter drawn by every workgroup -- store, drain, fetch_add -- was measured first: the
// two memory round trips at the end of each of 11584 GEMV workgroups cost 45 us per launch, four times
// what the removed launch had cost.)
constexpr unsigned long long kPartialSentinel = 0x7ff8dead5eedbeefull;   // quiet NaN with a payload nothing computes
// Bounded spinning with nothing slow on the fast path: the CU-local shader clock (clock64(), s_memtime -- not the
// shared constant-rate counter behind wall_clock64()) and the abort word are looked at once every 256 failed polls;
// limit ~5 s at 2.4 GHz (longer if the clock is lower -- it only bounds a wait that should never expire).
constexpr unsigned long long kSpinTimeoutCycles = 12000000000ull;
struct SpinGuard {
    unsigned spins = 0;
    unsigned long long t0 = 0;
    // once per failed poll; true once every 256 polls: the moment to look at slow things (the clock, and the
    // abort word in PINNED HOST memory -- a PCIe read: 256 workgroups doing one per poll cost 45-130 us per launch)
    __device__ __forceinline__ bool slow_path() { return (++spins & 255u) == 0; }
    __device__ __forceinline__ bool expired()          // only on the slow path
    {
        const unsigned long long now = (unsigned long long)clock64();
        if (t0 == 0) { t0 = now | 1ull; return false; }
        return now - t0 > kSpinTimeoutCycles;
    }
};

struct Finalize {                     // (the pointer list comes LAST here and in GemvArgs: the scalars keep their kernarg offsets
    int active;                       //  whatever kMaxShards is)
                                      // 0: no in-kernel reduction (the launch has no reducer workgroup)
    int mail;                         // 1: dst.p[j] is a MailSlot of rank j's mailbox (direct exchange, see Mail)
    int slot;
    unsigned long long seq;           // mail: the iteration tag
    int *host_err;                    // pinned host error word of the bounded waits (may be null): an expired wait is an
                                      // error the caller sees (lam_hip_cg_iterate), never a silent NaN
    PtrList dst;
};

// ---------------------------------------------------------------------------------------------
// Direct exchange (rank mode, option exchange = 2): no collective call inside the
// iteration.  Every rank maps every other rank's p replica and MAILBOX (HIP IPC, or plain pointers when
// the ranks are threads of one process) and the producer kernels store straight into them over xGMI:
//   * the reducer workgroup of the GEMV / update_xr launch writes the rank's partial dot product into
//     slot [rank] of EVERY rank's mailbox: value (system-scope write-through store), drain, then the tag
//     `seq` = the context's hand-over number of that iteration.  The consumer kernel (update_xr / update_p) polls the P tags
//     of its own mailbox and sums the P values in rank order: the fused, latency-optimal form of the two
//     scalar all-reduces, deterministic and bit-identical to the RCCL exchange;
//   * update_p stores its p slice into every rank's p replica with system-scope write-through stores,
//     drains them, and raises pflag[rank][workgroup] = seq in every mailbox; a 1-workgroup wait_p_kernel
//     in front of the next GEMV (behind its own-slice panel) polls those flags: the direct all-gather.
// Mailboxes are fine-grained (uncached) device memory; hand-over numbers grow by one per iteration and never restart, so nothing is ever
// reset and a slot can be read by any number of workgroups.  Every poll is bounded (SpinGuard):
// a peer that never shows up ends in an error flag in pinned host memory, not in a hang.
// ---------------------------------------------------------------------------------------------
// A {value, tag} hand-over as TWO SELF-VALIDATING 8-byte words (round 4): word h carries half h of the double's
// bits in its low 32 bits and the 32-bit tag in its high 32 bits.  Each word is written by ONE relaxed atomic store and read
// by ONE relaxed atomic load, and an 8-byte atomic object is its own ready flag: the reader takes the value only from words
// whose tag matches, so nothing is assumed about the order of accesses to DIFFERENT locations -- no fence, no drain, and no
// data race in the HIP memory model's terms.  (Rounds 2-3 wrote {value; s_waitcnt vmcnt(0); tag} and read the tag and then
// the value with two relaxed loads: correct on this hardware, which returns loads in order, but formally a race.)
// Tags are the low 32 bits of a hand-over number that grows by one per iteration over the whole life of a context
// (lam_hip.hip, seq_base): a slot is rewritten every iteration, so a stale tag is the previous iteration's, never equal.
struct MailSlot {
    unsigned long long w[2];
};
template <int SCOPE>
__device__ __forceinline__ void handover_store(MailSlot *slot, double value, unsigned long long seq)
{
    const unsigned long long bits = (unsigned long long)__double_as_longlong(value), tag = (seq & 0xffffffffull) << 32;
    __hip_atomic_store(&slot->w[0], tag | (bits & 0xffffffffull), __ATOMIC_RELAXED, SCOPE);
    __hip_atomic_store(&slot->w[1], tag | (bits >> 32), __ATOMIC_RELAXED, SCOPE);
}
// true (and the value) once BOTH words carry the tag; *seen = what the first word's tag was (diagnostics)
template <int SCOPE>
__device__ __forceinline__ bool handover_try_load(const MailSlot *slot, unsigned long long seq, double *value, unsigned *seen)
{
    const unsigned long long w0 = __hip_atomic_load(&slot->w[0], __ATOMIC_RELAXED, SCOPE);
    const unsigned long long w1 = __hip_atomic_load(&slot->w[1], __ATOMIC_RELAXED, SCOPE);
    const unsigned tag = (unsigned)(seq & 0xffffffffull);
    *seen = (unsigned)(w0 >> 32);
    if ((unsigned)(w0 >> 32) != tag || (unsigned)(w1 >> 32) != tag) return false;
    *value = __longlong_as_double((long long)((w1 << 32) | (w0 & 0xffffffffull)));
    return true;
}
struct Mail {
    MailSlot pap[kMaxShards];
    MailSlot rr[kMaxShards];
    unsigned long long pflag[kMaxShards][256];   // [source rank][its update_p workgroup] (256 == kVecBlocksMax)
};
struct MailWait {                     // consumer side of a scalar exchange; n == 0: not used
    const MailSlot *slots;            // this rank's pap[] or rr[]
    int n;
    unsigned long long seq;
    int *host_err;                    // pinned host memory
};
struct MailPost {                     // update_p: flags to raise after the p slice has been stored; n == 0: not used
    Mail *mail[kMaxShards];
    int n, rank;
    unsigned long long seq;
};

struct BlockCounts { int n[kMaxShards]; };   // update_p workgroups of every rank (p-slice flags to wait for)

__device__ __forceinline__ unsigned long long ld_sys(const unsigned long long *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ void st_sys(unsigned long long *p, unsigned long long v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Sum of the P partials other ranks posted for iteration `w.seq`; every thread of every workgroup gets the
// same value.  Same reduction tree as block_sum_array(src, P), so exchange 2 and exchange 0 agree bit for bit.
__device__ __forceinline__ double mail_sum(const MailWait &w, double *s_red)
{
    double v = 0.0;
    if ((int)threadIdx.x < w.n) {
        const MailSlot *m = w.slots + threadIdx.x;
        SpinGuard guard;
        unsigned seen;
        while (!handover_try_load<__HIP_MEMORY_SCOPE_SYSTEM>(m, w.seq, &v, &seen)) {
            if (guard.slow_path()) {
            // an expired wait anywhere (this kernel or an earlier one) ends all waiting: the solve has failed
            if (*(volatile int *)w.host_err != 0) break;
            if (guard.expired()) {
                w.host_err[1] = (int)threadIdx.x; w.host_err[2] = (int)(unsigned)w.seq; w.host_err[3] = (int)seen;
                w.host_err[4] = (int)(w.seq >> 32); w.host_err[5] = 0;
                *(volatile int *)w.host_err = 2;
                break;
            }
            }
            __builtin_amdgcn_s_sleep(4);
        }
    }
    return block_sum(v, s_red);
}
__device__ __forceinline__ bool is_reducer_block(const Finalize &f) { return f.active && blockIdx.x == gridDim.x - 1; }
__device__ __forceinline__ unsigned compute_blocks(const Finalize &f) { return gridDim.x - (f.active ? 1u : 0u); }

// compute workgroups: thread 0 stores the workgroup's partial (see Finalize)
__device__ __forceinline__ void publish_partial(double t, double *partial, const Finalize &f)
{
    if (threadIdx.x != 0) return;
    if (f.active) __hip_atomic_store(partial + blockIdx.x, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else partial[blockIdx.x] = t;
}

// the reducer workgroup (every thread of it; workgroups wider than kBlock: the extra waves idle)
__device__ __forceinline__ double reduce_partials_sum(double *partial, int n /*compute workgroups*/, double *s_red /*[kWaves]*/,
                                                      int *host_err)
{
    SpinGuard guard;
    bool timed_out = false;
    unsigned long long *slots = reinterpret_cast<unsigned long long *>(partial);
    auto ld = [&](int j) { return __hip_atomic_load(slots + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    // CNT slots (stride kBlock): all loads of a polling round are in flight together, so the reducer is at
    // most a round trip or two behind the last producer; then the slots are re-armed
    auto take = [&](int base, auto cnt_tag, double *out) {
        constexpr int CNT = decltype(cnt_tag)::value;
        unsigned long long b[CNT];
#pragma unroll
        for (int k = 0; k < CNT; k++) b[k] = ld(base + k * kBlock);
        bool pending = true;
        while (pending && !timed_out) {
            pending = false;
#pragma unroll
            for (int k = 0; k < CNT; k++)
                if (b[k] == kPartialSentinel) { b[k] = ld(base + k * kBlock); pending |= b[k] == kPartialSentinel; }
            if (pending) {
                __builtin_amdgcn_s_sleep(8);
                if (guard.slow_path()) {
                    // another bounded wait of this solve has already expired: stop waiting (the solve has failed)
                    if (host_err != nullptr && *(volatile int *)host_err != 0) timed_out = true;
                    else if (guard.expired()) {
                        timed_out = true;
                        if (host_err != nullptr) { host_err[1] = base; host_err[2] = n; *(volatile int *)host_err = 5; }
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < CNT; k++) {
            __hip_atomic_store(slots + base + k * kBlock, kPartialSentinel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            out[k] = __longlong_as_double((long long)b[k]);
        }
    };
    double v = 0.0;
    int i = threadIdx.x < kBlock ? (int)threadIdx.x : n;
    for (; i + 7 * kBlock < n; i += 8 * kBlock) {      // same grouping and order as block_sum_array
        double a[8];
        take(i, std::integral_constant<int, 8>(), a);
        v += ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
    }
    for (; i < n; i += kBlock) {
        double a[1];
        take(i, std::integral_constant<int, 1>(), a);
        v += a[0];
    }
    return block_sum(v, s_red);
}

// thread 0 of the reducer workgroup: hand the shard's total to whoever consumes it (see Finalize)
__device__ __forceinline__ void post_total(const Finalize &f, double total)
{
    if (threadIdx.x != 0) return;
    if (!f.mail) {
        for (int j = 0; j < f.dst.n; j++) reinterpret_cast<double *>(f.dst.p[j])[f.slot] = total;
    } else {
        // direct exchange: the tagged words into every rank's mailbox (system-scope write-through stores)
        for (int j = 0; j < f.dst.n; j++) handover_store<__HIP_MEMORY_SCOPE_SYSTEM>(reinterpret_cast<MailSlot *>(f.dst.p[j]), total, f.seq);
    }
}

__device__ __forceinline__ void reduce_partials(double *partial, int n, const Finalize &f, double *s_red)
{
    post_total(f, reduce_partials_sum(partial, n, s_red, f.host_err));
}

// Hand-over INSIDE a launch (update_fused_kernel): the reducer workgroup publishes a scalar for the launch's
// other workgroups in ordinary device memory -- two tagged words (MailSlot), agent-scope write-through stores -- and
// they poll them with agent-scope loads.  One thread polls; the value reaches the workgroup through block_sum.
// Every listener has a LINE OF ITS OWN (BcastLine, 128 B): hundreds of workgroups polling one word serialise at the
// memory side and the writer's store queues behind them -- measured 0.2-0.35 us per polling workgroup, 45-90 us per
// iteration with 256 of them.  The reducer's threads write the lines in parallel.
constexpr int kBcastLines = 264;      // >= 256 compute workgroups + the waiter
struct BcastLine {
    MailSlot s;
    char pad[128 - sizeof(MailSlot)];
};
__device__ __forceinline__ void bcast_post(BcastLine *lines, int nlisteners, double value, unsigned long long seq)
{
    for (int t = threadIdx.x; t < nlisteners; t += kBlock) handover_store<__HIP_MEMORY_SCOPE_AGENT>(&lines[t].s, value, seq);
}
__device__ __forceinline__ double bcast_wait(const BcastLine *line, unsigned long long seq, int *host_err, double *s_red)
{
    const MailSlot *slot = &line->s;
    double v = 0.0;
    if (threadIdx.x == 0) {
        SpinGuard guard;
        unsigned seen;
        while (!handover_try_load<__HIP_MEMORY_SCOPE_AGENT>(slot, seq, &v, &seen)) {
            if (guard.slow_path()) {
            if (*(volatile int *)host_err != 0) break;
            if (guard.expired()) {
                host_err[1] = -1; host_err[2] = (int)(unsigned)seq; host_err[3] = (int)seen;
                host_err[4] = (int)(seq >> 32); host_err[5] = 0;
                *(volatile int *)host_err = 4;
                break;
            }
            }
            __builtin_amdgcn_s_sleep(4);
        }
    }
    return block_sum(v, s_red);
}

// arm the slots (cg_init, and whenever a launch without a reducer may have written plain values)
__global__ void __launch_bounds__(kBlock)
arm_partials_kernel(double *partial, int n)
{
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock)
        reinterpret_cast<unsigned long long *>(partial)[i] = kPartialSentinel;
}

template <typename TA> struct MatVec;  // 16-byte vector of matrix elements
template <> struct MatVec<double> {
    typedef double vec_t __attribute__((ext_vector_type(2)));
    static constexpr int N = 2;
    static __device__ __forceinline__ double get(const vec_t &v, int i) { return v[i]; }
};
template <> struct MatVec<float> {
    typedef float vec_t __attribute__((ext_vector_type(4)));
    static constexpr int N = 4;
    static __device__ __forceinline__ float get(const vec_t &v, int i) { return v[i]; }
};
// bf16 storage: 8 elements per 16 bytes, widened to fp32 by a 16-bit shift (exact)
template <> struct MatVec<__hip_bfloat16> {
    typedef unsigned short vec_t __attribute__((ext_vector_type(8)));
    static constexpr int N = 8;
    static __device__ __forceinline__ float get(const vec_t &v, int i)
    {
        return __uint_as_float(((unsigned)v[i]) << 16);
    }
};

// non-temporal scalar load of one matrix element (bf16 goes through its 16-bit pattern)
template <typename T> __device__ __forceinline__ T nt_load(const T *p) { return __builtin_nontemporal_load(p); }
template <> __device__ __forceinline__ __hip_bfloat16 nt_load<__hip_bfloat16>(const __hip_bfloat16 *p)
{
    const unsigned short bits = __builtin_nontemporal_load(reinterpret_cast<const unsigned short *>(p));
    return __builtin_bit_cast(__hip_bfloat16, bits);
}

// scalar widening of one matrix element to the vector type
template <typename TV> __device__ __forceinline__ TV widen(double v) { return (TV)v; }
template <typename TV> __device__ __forceinline__ TV widen(float v) { return (TV)v; }
template <typename TV> __device__ __forceinline__ TV widen(__hip_bfloat16 v)
{
    return (TV)__uint_as_float(((unsigned)*reinterpret_cast<const unsigned short *>(&v)) << 16);
}

// The GEMV's multiply-add, fused EXPLICITLY: left to -ffp-contract the fp32 kernels came out as packed multiplies
// followed by separate adds in some instantiations (v_pk_mul_f32 + v_pk_add_f32: twice the VALU work, and a rounding that
// depended on how the loop happened to be vectorised) and as v_pk_fma_f32 in others.  fp64 always compiled to v_fma_f64.
__device__ __forceinline__ double fma_tv(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ float fma_tv(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

// ---------------------------------------------------------------------------------------------
// GEMV  y_loc = A_loc * p        (A_loc: nrows x n row-major, p: n, y_loc: nrows)
// ---------------------------------------------------------------------------------------------
template <typename TA, typename TV>
struct GemvArgs {
    const TA *A;
    const TV *p;            // full-length vector
    TV *y;                  // local rows
    double *partial;        // [gridDim.x] per-workgroup partial of sum_r y[r]*p[row0+r]; may be null
    const CgScalars *sc;    // may be null; if sc->stop the kernel does nothing
    uint64_t nrows;         // local rows
    uint64_t n;             // columns (= global N)
    uint64_t lda;           // row pitch of A in elements (>= n): rows are padded to a 4-KiB multiple (16 B for tiny rows) and the
                            // padding is ZERO, so every row starts aligned and the 16-byte-vector kernels serve any N
    uint64_t row0;          // global index of local row 0 (for the fused dot)
    // column panels: the launch covers columns [seg_begin[i], seg_end[i]) for i < nseg (nseg <= 2).
    // A whole GEMV is one segment [0,n).  In rank mode the iteration's GEMV is two launches: the
    // panel of the rank's OWN p slice first (runs while the all-gather of the other slices is in
    // flight), then the rest with accumulate = 1.
    uint64_t seg_begin[2];
    uint64_t seg_end[2];
    int nseg;
    int accumulate;         // y[row] += ... instead of y[row] = ...
    int n_ypeer;
    Finalize fin;           // in-kernel reduction of `partial` by the last workgroup (several shards)
    // gather-Ap exchange with several shards in one process: y[row] also goes, as a peer store over xGMI, to the same
    // row of this shard's record in every OTHER shard's gather buffer (n_ypeer = 0 everywhere else)
    TV *ypeer[kMaxShards - 1];
};

// the row's result: the shard's own copy and the peers' (see GemvArgs::ypeer)
template <typename TA, typename TV>
__device__ __forceinline__ void store_y(const GemvArgs<TA, TV> &a, uint64_t row, TV v)
{
    a.y[row] = v;
    for (int j = 0; j < a.n_ypeer; j++) a.ypeer[j][row] = v;
}

// Fast path: n % (16/sizeof(TA)) == 0, A and p 16-byte aligned.
//   workgroup = 4 waves, wave w owns rows (4*blockIdx+w)*R .. +R-1, all n columns.
//   TILE elements of p live in LDS at a time; a workgroup starts at tile blockIdx % ntiles (rotated order).
template <typename TA, typename TV, bool NT>
__global__ void __launch_bounds__(kBlock)
gemv_tile_kernel(GemvArgs<TA, TV> a)
{
    using MV = MatVec<TA>;
    using avec_t = typename MV::vec_t;
    constexpr int R = 4, TILE = 4096, UNROLL = 4;
    constexpr int VEC = MV::N;
    constexpr int STEP = 64 * VEC;          // columns one wave instruction covers
    static_assert(TILE % STEP == 0, "tile must be a whole number of wave steps");
    constexpr int STEPS = TILE / STEP;

    __shared__ __attribute__((aligned(16))) TV s_p[TILE];
    __shared__ double s_red[kWaves];

    if (a.sc != nullptr && a.sc->stop) return;
    if (is_reducer_block(a.fin)) { reduce_partials(a.partial, (int)gridDim.x - 1, a.fin, s_red); return; }

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const uint64_t row_first = ((uint64_t)blockIdx.x * kWaves + wave) * R;

    const TA *rowp[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        uint64_t row = row_first + r;
        if (row >= a.nrows) row = a.nrows - 1;   // keep loads in bounds; result discarded below
        rowp[r] = a.A + row * a.lda + (uint64_t)lane * VEC;
    }
    TV acc[R];
#pragma unroll
    for (int r = 0; r < R; r++) acc[r] = (TV)0;

    const uint32_t ntiles0 = (uint32_t)((a.seg_end[0] - a.seg_begin[0] + TILE - 1) / TILE);
    const uint32_t ntiles = ntiles0 + (a.nseg > 1 ? (uint32_t)((a.seg_end[1] - a.seg_begin[1] + TILE - 1) / TILE) : 0u);
    uint32_t tt = blockIdx.x % ntiles;     // rotated start
    for (uint32_t t = 0; t < ntiles; t++) {
        const bool second = tt >= ntiles0;
        const uint64_t c0 = second ? a.seg_begin[1] + (uint64_t)(tt - ntiles0) * TILE : a.seg_begin[0] + (uint64_t)tt * TILE;
        const uint64_t cend = second ? a.seg_end[1] : a.seg_end[0];
        const uint32_t cols = (uint32_t)((cend - c0 < (uint64_t)TILE) ? (cend - c0) : (uint64_t)TILE);
        __syncthreads();                              // previous tile fully consumed
        // stage p[c0 .. c0+cols) -- 16-byte loads, cols is a multiple of VEC (>= 16 B of TV too)
        {
            constexpr int PV = 16 / sizeof(TV);
            typedef TV pvec_t __attribute__((ext_vector_type(PV)));
            const pvec_t *src = reinterpret_cast<const pvec_t *>(a.p + c0);
            pvec_t *dst = reinterpret_cast<pvec_t *>(s_p);
            const uint32_t nv = cols / PV;
            for (uint32_t i = tid; i < nv; i += kBlock) dst[i] = src[i];
            for (uint32_t i = nv * PV + tid; i < cols; i += kBlock) s_p[i] = a.p[c0 + i];
            // ragged tile: zeros up to the next whole wave step (what the lanes past the end multiply with)
            for (uint32_t i = cols + tid; i < (uint32_t)TILE && i < (cols + STEP - 1) / STEP * STEP; i += kBlock) s_p[i] = (TV)0;
        }
        __syncthreads();
        const TV *pt = s_p;

        if (cols == TILE) {
#pragma unroll UNROLL
            for (int s = 0; s < STEPS; s++) {
                avec_t av[R];
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const avec_t *src = reinterpret_cast<const avec_t *>(rowp[r] + c0 + (uint64_t)s * STEP);
                    av[r] = NT ? __builtin_nontemporal_load(src) : *src;
                }
                TV pv[VEC];
#pragma unroll
                for (int i = 0; i < VEC; i++) pv[i] = pt[s * STEP + lane * VEC + i];
#pragma unroll
                for (int r = 0; r < R; r++)
#pragma unroll
                    for (int i = 0; i < VEC; i++) acc[r] = fma_tv((TV)MV::get(av[r], i), pv[i], acc[r]);
            }
        } else {
            // Ragged last tile of a segment (N not a multiple of TILE: 18 % of the columns at N=10000): the SAME
            // streaming body over ceil(cols / STEP) steps.  Lanes past the end of the segment read the row's last
            // vector again (address clamped: in bounds) and multiply a ZERO in its place (and a zero of p: the p tile is
            // zero-filled behind `cols`), so they add exactly +0 -- also when that last vector
            // holds +-Inf or NaN, which times the zero of p alone would turn into a NaN row sum.  No second
            // code path with its own registers: round 2's separately unrolled ragged body doubled the kernels' VGPRs
            // (fp32 54 -> 98, bf16 104 -> 256: occupancy 8 -> 4 and 4 -> 1) and the full-tile path paid for it.
            const int nsteps = (int)((cols + STEP - 1) / STEP);
#pragma unroll UNROLL
            for (int s = 0; s < nsteps; s++) {
                const uint32_t col = (uint32_t)s * STEP + (uint32_t)lane * VEC;
                avec_t av[R];
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const avec_t *src = col < cols ? reinterpret_cast<const avec_t *>(rowp[r] + c0 + (uint64_t)s * STEP)
                                                   : reinterpret_cast<const avec_t *>(kZeroVec16);
                    av[r] = NT ? __builtin_nontemporal_load(src) : *src;
                }
                TV pv[VEC];
#pragma unroll
                for (int i = 0; i < VEC; i++) pv[i] = pt[col + i];
#pragma unroll
                for (int r = 0; r < R; r++)
#pragma unroll
                    for (int i = 0; i < VEC; i++) acc[r] = fma_tv((TV)MV::get(av[r], i), pv[i], acc[r]);
            }
        }
        tt = (tt + 1 == ntiles) ? 0 : tt + 1;
    }

    // lane partials -> row sums (wave64 butterfly), fused p.Ap partial
    double dotp = 0.0;
#pragma unroll
    for (int r = 0; r < R; r++) {
        TV s = wave_sum(acc[r]);
        const uint64_t row = row_first + r;
        if (lane == 0 && row < a.nrows) {
            if (a.accumulate) s += a.y[row];
            store_y(a, row, s);
            dotp += (double)s * (double)a.p[a.row0 + row];
        }
    }
    if (a.partial != nullptr) {
        __syncthreads();
        if (lane == 0) s_red[wave] = dotp;
        __syncthreads();
        double t = 0.0;
        if (tid == 0) {
            t = s_red[0];
#pragma unroll
            for (int w = 1; w < kWaves; w++) t += s_red[w];
        }
        publish_partial(t, a.partial, a.fin);
    }
}

// Cooperative-row variant: the 4 waves of a workgroup stream the SAME R rows, wave w taking every
// 4th 1-KiB step, so a workgroup reads 4 KiB contiguous per row per super-step and the chip has
// 4x fewer concurrent row streams than the wave-per-row shape (DRAM page locality experiment).
// The row sums are combined across waves through LDS in a fixed order.
template <typename TA, typename TV, int R, bool NT, int WAVES>
__global__ void __launch_bounds__(WAVES * 64)
gemv_coop_kernel(GemvArgs<TA, TV> a)
{
    using MV = MatVec<TA>;
    using avec_t = typename MV::vec_t;
    constexpr int TILE = 4096, UNROLL = 4;
    constexpr int VEC = MV::N;
    constexpr int STEP = 64 * VEC;
    static_assert(TILE % (STEP * WAVES) == 0, "tile must be a whole number of workgroup super-steps");
    constexpr int WSTEPS = TILE / (STEP * WAVES);
    constexpr int NTHREADS = WAVES * 64;    // steps per wave per tile

    __shared__ __attribute__((aligned(16))) TV s_p[TILE];
    __shared__ TV s_part[R][WAVES];
    __shared__ double s_dot[R];
    __shared__ double s_red[kWaves];

    if (a.sc != nullptr && a.sc->stop) return;
    if (is_reducer_block(a.fin)) { reduce_partials(a.partial, (int)gridDim.x - 1, a.fin, s_red); return; }

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const uint64_t row_first = (uint64_t)blockIdx.x * R;
    const uint32_t woff = (uint32_t)wave * STEP + (uint32_t)lane * VEC;   // this lane's column inside a super-step

    const TA *rowp[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        uint64_t row = row_first + r;
        if (row >= a.nrows) row = a.nrows - 1;
        rowp[r] = a.A + row * a.lda + woff;
    }
    TV acc[R];
#pragma unroll
    for (int r = 0; r < R; r++) acc[r] = (TV)0;

    const uint32_t ntiles0 = (uint32_t)((a.seg_end[0] - a.seg_begin[0] + TILE - 1) / TILE);
    const uint32_t ntiles = ntiles0 + (a.nseg > 1 ? (uint32_t)((a.seg_end[1] - a.seg_begin[1] + TILE - 1) / TILE) : 0u);
    uint32_t tt = blockIdx.x % ntiles;
    for (uint32_t t = 0; t < ntiles; t++) {
        const bool second = tt >= ntiles0;
        const uint64_t c0 = second ? a.seg_begin[1] + (uint64_t)(tt - ntiles0) * TILE : a.seg_begin[0] + (uint64_t)tt * TILE;
        const uint64_t cend = second ? a.seg_end[1] : a.seg_end[0];
        const uint32_t cols = (uint32_t)((cend - c0 < (uint64_t)TILE) ? (cend - c0) : (uint64_t)TILE);
        __syncthreads();
        {
            constexpr int PV = 16 / sizeof(TV);
            typedef TV pvec_t __attribute__((ext_vector_type(PV)));
            const pvec_t *src = reinterpret_cast<const pvec_t *>(a.p + c0);
            pvec_t *dst = reinterpret_cast<pvec_t *>(s_p);
            const uint32_t nv = cols / PV;
            for (uint32_t i = tid; i < nv; i += NTHREADS) dst[i] = src[i];
            for (uint32_t i = nv * PV + tid; i < cols; i += NTHREADS) s_p[i] = a.p[c0 + i];
            // ragged tile: zeros up to the next whole super-step (what the lanes past the end multiply with)
            for (uint32_t i = cols + tid; i < (uint32_t)TILE && i < (cols + STEP * WAVES - 1) / (STEP * WAVES) * (STEP * WAVES); i += NTHREADS)
                s_p[i] = (TV)0;
        }
        __syncthreads();
        if (cols == TILE) {
#pragma unroll UNROLL
            for (int s = 0; s < WSTEPS; s++) {
                avec_t av[R];
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const avec_t *src = reinterpret_cast<const avec_t *>(rowp[r] + c0 + (uint64_t)s * (STEP * WAVES));
                    av[r] = NT ? __builtin_nontemporal_load(src) : *src;
                }
                TV pv[VEC];
#pragma unroll
                for (int i = 0; i < VEC; i++) pv[i] = s_p[s * (STEP * WAVES) + woff + i];
#pragma unroll
                for (int r = 0; r < R; r++)
#pragma unroll
                    for (int i = 0; i < VEC; i++) acc[r] = fma_tv((TV)MV::get(av[r], i), pv[i], acc[r]);
            }
        } else {
            // ragged last tile of a segment: the same streaming body over ceil(cols / super-step) super-steps; lanes past
            // the end re-read the row's last vector (clamped address) and multiply a zero in its place with the zeros the
            // staging put behind `cols`, so they add exactly +0, a non-finite last vector included (see gemv_tile_kernel:
            // no second unrolled body, no second set of registers)
            const int nsteps = (int)((cols + STEP * WAVES - 1) / (STEP * WAVES));
#pragma unroll UNROLL
            for (int s = 0; s < nsteps; s++) {
                const uint32_t col = (uint32_t)s * (STEP * WAVES) + woff;
                avec_t av[R];
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const avec_t *src = col < cols ? reinterpret_cast<const avec_t *>(rowp[r] + c0 + (uint64_t)s * (STEP * WAVES))
                                                   : reinterpret_cast<const avec_t *>(kZeroVec16);
                    av[r] = NT ? __builtin_nontemporal_load(src) : *src;
                }
                TV pv[VEC];
#pragma unroll
                for (int i = 0; i < VEC; i++) pv[i] = s_p[col + i];
#pragma unroll
                for (int r = 0; r < R; r++)
#pragma unroll
                    for (int i = 0; i < VEC; i++) acc[r] = fma_tv((TV)MV::get(av[r], i), pv[i], acc[r]);
            }
        }
        tt = (tt + 1 == ntiles) ? 0 : tt + 1;
    }

#pragma unroll
    for (int r = 0; r < R; r++) {
        TV s = wave_sum(acc[r]);
        if (lane == 0) s_part[r][wave] = s;
    }
    __syncthreads();
    if (tid < R) {
        const uint64_t row = row_first + tid;
        double d = 0.0;
        if (row < a.nrows) {
            TV s = s_part[tid][0];
#pragma unroll
            for (int w = 1; w < WAVES; w++) s += s_part[tid][w];
            if (a.accumulate) s += a.y[row];
            store_y(a, row, s);
            d = (double)s * (double)a.p[a.row0 + row];
        }
        s_dot[tid] = d;
    }
    if (a.partial != nullptr) {
        __syncthreads();
        double t = 0.0;
        if (tid == 0) {
            t = s_dot[0];
#pragma unroll
            for (int r = 1; r < R; r++) t += s_dot[r];
        }
        publish_partial(t, a.partial, a.fin);
    }
}

// ---------------------------------------------------------------------------------------------
// Packed fp64 matrix (option "packed", format: lam_host_pack.h): the same product from 7/8 of the bytes.
// ---------------------------------------------------------------------------------------------
struct PackedMat {
    const unsigned char *data;   // [nrows][ntiles][kPackGroups][kPackGroupBytes]
    const double *exc;           // [nrows][ntiles][kPackCap]
    const uint32_t *hdr;         // [nrows][ntiles]
    uint32_t ntiles;
};
typedef unsigned int pack_u4 __attribute__((ext_vector_type(4)));
typedef unsigned int pack_u2 __attribute__((ext_vector_type(2)));

// One pass over A: workgroup = one row, tile by tile -- exponent histogram in LDS, the window of kPackWindow binades that holds the
// most elements, the elements in the product kernel's traversal order, the exception list, the header.  info[0] is set when a
// (row, tile) has more than kPackCap exceptions (not packable), info[1] counts the list values a product reads (the first
// kPackFirst of every list whatever its length, then the rest of a longer one).  Thread (wave, lane) encodes lane `lane` of wave groups wave and wave + 4.
__global__ void __launch_bounds__(kBlock)
pack_rows_kernel(const double *__restrict__ A, uint64_t lda, uint64_t ncols, uint32_t ntiles, unsigned char *__restrict__ data,
                 uint64_t *__restrict__ exc, uint32_t *__restrict__ hdr, unsigned long long *__restrict__ info)
{
    typedef double dvec2 __attribute__((ext_vector_type(2)));
    __shared__ uint32_t s_hist[kPackExpBins];
    __shared__ uint32_t s_key[kWaves];
    __shared__ uint32_t s_cnt;
    __shared__ uint64_t s_exc[kPackCap];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t row = blockIdx.x;
    const double *arow = A + row * lda;
    unsigned long long row_exc = 0;
    for (uint32_t tt = 0; tt < ntiles; tt++) {
        const uint64_t c0 = (uint64_t)tt * kPackTile;
        const uint32_t cols = (uint32_t)((ncols - c0 < (uint64_t)kPackTile) ? (ncols - c0) : (uint64_t)kPackTile);   // even
        for (int i = tid; i < (int)kPackExpBins; i += kBlock) s_hist[i] = 0;
        if (tid == 0) s_cnt = 0;
        __syncthreads();
        uint64_t v[2][8];
        uint32_t valid = 0;                    // bit 4 h + s: the pair of step s in wave group wave + 4 h lies inside the row
#pragma unroll
        for (int h = 0; h < 2; h++)
#pragma unroll
            for (int s = 0; s < 4; s++) {
                const uint32_t col = (uint32_t)s * 1024u + (uint32_t)(wave + 4 * h) * 128u + 2u * (uint32_t)lane;
                v[h][2 * s] = v[h][2 * s + 1] = 0;
                if (col < cols) {
                    const dvec2 a = __builtin_nontemporal_load(reinterpret_cast<const dvec2 *>(arow + c0 + col));
                    v[h][2 * s] = (uint64_t)__double_as_longlong(a[0]);
                    v[h][2 * s + 1] = (uint64_t)__double_as_longlong(a[1]);
                    valid |= 1u << (4 * h + s);
                }
            }
#pragma unroll
        for (int h = 0; h < 2; h++)
#pragma unroll
            for (int e = 0; e < 8; e++)
                if ((valid >> (4 * h + (e >> 1)) & 1u) && pack_is_normal(v[h][e])) atomicAdd(&s_hist[pack_exp_of(v[h][e])], 1u);
        __syncthreads();
        uint32_t key = 0;
        for (uint32_t base = (uint32_t)tid * 8u; base < (uint32_t)tid * 8u + 8u; base++)
            if (base >= 1u && base <= 2046u) key = max(key, pack_window_key(pack_window_count(s_hist, base), base));
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) key = max(key, (uint32_t)__shfl_xor((int)key, off, 64));
        if (lane == 0) s_key[wave] = key;
        __syncthreads();
        key = s_key[0];
#pragma unroll
        for (int w = 1; w < kWaves; w++) key = max(key, s_key[w]);
        const uint32_t base = key & 0x7ffu;

        const uint64_t unit = row * ntiles + tt;
#pragma unroll
        for (int h = 0; h < 2; h++) {
            uint32_t lo[8], mid[8], hi[8];
#pragma unroll
            for (int e = 0; e < 8; e++) {
                if (!(valid >> (4 * h + (e >> 1)) & 1u)) pack_encode_exception(kPackZeroIdx, &lo[e], &mid[e], &hi[e]);
                else if (pack_in_window(v[h][e], base)) pack_encode(v[h][e], base, &lo[e], &mid[e], &hi[e]);
                else {
                    const uint32_t idx = atomicAdd(&s_cnt, 1u);
                    if (idx < kPackCap) s_exc[idx] = v[h][e];
                    pack_encode_exception(idx < kPackCap ? idx : kPackZeroIdx, &lo[e], &mid[e], &hi[e]);
                }
            }
            unsigned char *g = data + (unit * kPackGroups + (uint64_t)(wave + 4 * h)) * kPackGroupBytes;
            pack_u4 q;
            q[0] = lo[0]; q[1] = lo[1]; q[2] = lo[2]; q[3] = lo[3];
            *reinterpret_cast<pack_u4 *>(g + pack_off_lo(lane, 0)) = q;
            q[0] = lo[4]; q[1] = lo[5]; q[2] = lo[6]; q[3] = lo[7];
            *reinterpret_cast<pack_u4 *>(g + pack_off_lo(lane, 4)) = q;
            q[0] = mid[0] | mid[1] << 16; q[1] = mid[2] | mid[3] << 16; q[2] = mid[4] | mid[5] << 16; q[3] = mid[6] | mid[7] << 16;
            *reinterpret_cast<pack_u4 *>(g + pack_off_mid(lane, 0)) = q;
            pack_u2 b;
            b[0] = hi[0] | hi[1] << 8 | hi[2] << 16 | hi[3] << 24;
            b[1] = hi[4] | hi[5] << 8 | hi[6] << 16 | hi[7] << 24;
            *reinterpret_cast<pack_u2 *>(g + pack_off_hi(lane, 0)) = b;
        }
        __syncthreads();
        const uint32_t cnt = s_cnt;
        for (uint32_t i = tid; i < cnt && i < kPackCap; i += kBlock) exc[unit * kPackCap + i] = s_exc[i];
        if (tid == 0) {
            hdr[unit] = pack_header(base, cnt);
            row_exc += max(min(cnt, kPackCap), kPackFirst);
            if (cnt > kPackCap) info[0] = 1ull;
        }
        __syncthreads();                       // s_cnt, s_exc and s_hist are free for the next tile
    }
    if (tid == 0) atomicAdd(&info[1], row_exc);
}

// The body of gemv_coop_kernel<double, double, 2, NT, 8> on the packed image: the same grid and reducer workgroup, the same rotated
// tile order, s_p staging, lane-to-column mapping and fma sequence per lane (the +0 terms of a ragged tile included), the same
// wave_sum, s_part order, store_y and publish_partial -- so the result is bit for bit the plain kernel's.  What differs is where an
// element comes from: four coalesced non-temporal loads give a lane its 8 elements of a row and tile, the tile's exception values
// are staged into LDS next to the p tile behind the same barrier, and every element is one LDS read of its (row, tile)'s list --
// an exception's value, or the reserved +0.0 at one address for the rest of the wave -- and a select.  (The source has no branch
// per element; the compiler emits each select as a two-sided exec-mask region, the decode under one mask and the list read under
// the other: 16 such regions a tile and lane.)
// A tile, in order: (1) the element loads, the two headers and the first 64 values of the two lists are issued -- they depend on
// nothing the workgroup shares; (2) first barrier: every wave has finished the previous tile's reads of s_p and s_exc; (3) the
// p tile's four loads a thread, back to back, ONE wait (vmcnt(0): it also covers what (1) issued), four LDS writes; the lists'
// first values are written, the rest of a list longer than 64 is loaded and written (one more round trip, long lists only);
// (4) second barrier; (5) the FMAs.  Between the two barriers lies one L2 round trip for p, which runs under the HBM latency of
// the elements.  DESIGN section 18 has the variants that were measured against this one and lost.
// One whole column segment [0, seg_end[0]) only (the launcher sends panels to the plain kernel).
template <bool NT>
__global__ void __launch_bounds__(512)
gemv_packed_kernel(GemvArgs<double, double> a, PackedMat pk)
{
    constexpr int R = 2, WAVES = 8, TILE = kPackTile, STEP = 128, NTHREADS = WAVES * 64;
    constexpr int WSTEPS = TILE / (STEP * WAVES);
    static_assert(WSTEPS == 4 && STEP * WAVES == 1024, "the packed layout is that of 8 waves x 4 super-steps");

    __shared__ __attribute__((aligned(16))) double s_p[TILE];
    __shared__ double s_exc[R][kPackCap + 1];
    __shared__ double s_part[R][WAVES];
    __shared__ double s_dot[R];
    __shared__ double s_red[kWaves];

    if (a.sc != nullptr && a.sc->stop) return;
    if (is_reducer_block(a.fin)) { reduce_partials(a.partial, (int)gridDim.x - 1, a.fin, s_red); return; }

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // wave-uniform: a tile's addresses are scalar base + lane offset
    const uint64_t row_first = (uint64_t)blockIdx.x * R;
    const uint32_t woff = (uint32_t)wave * STEP + (uint32_t)lane * 2u;

    const uint32_t ntiles = pk.ntiles;
    uint64_t unit0[R];                          // the row's first (row, tile) unit
#pragma unroll
    for (int r = 0; r < R; r++) {
        uint64_t row = row_first + r;
        if (row >= a.nrows) row = a.nrows - 1;
        unit0[r] = row * ntiles;
    }
    double acc[R];
#pragma unroll
    for (int r = 0; r < R; r++) acc[r] = 0.0;
    if (tid < R) s_exc[tid][kPackZeroIdx] = 0.0;      // the reserved index; never overwritten (visible behind the first barrier)

    constexpr uint32_t FIRST = kPackFirst;       // exception values staged before the header is known: one wave's load per row
    static_assert(FIRST == 64, "one value a lane");
    static_assert(R <= WAVES - 1, "waves 1 .. R stage the lists' first values");
    const bool stager = wave >= 1 && wave <= R;
    uint32_t perlane = 0;
    asm volatile("" : "+v"(perlane));
    uint32_t tt = blockIdx.x % ntiles;
    for (uint32_t t = 0; t < ntiles; t++) {
        const uint64_t c0 = (uint64_t)tt * TILE;
        const uint64_t cend = a.seg_end[0];
        const uint32_t cols = (uint32_t)((cend - c0 < (uint64_t)TILE) ? (cend - c0) : (uint64_t)TILE);
        const uint32_t tnext = (tt + 1 == ntiles) ? 0 : tt + 1;
        // the tile's elements: issued in front of the barriers (they depend on nothing the workgroup shares), so that they are in
        // flight while p and the exception lists are staged
        pack_u4 lo0[R], lo1[R], mid[R];
        pack_u2 hi[R];
#pragma unroll
        for (int r = 0; r < R; r++) {
            const unsigned char *g = pk.data + ((unit0[r] + tt) * kPackGroups + (uint64_t)wave) * kPackGroupBytes;
            const pack_u4 *q0 = reinterpret_cast<const pack_u4 *>(g + pack_off_lo(lane, 0));
            const pack_u4 *q1 = reinterpret_cast<const pack_u4 *>(g + pack_off_lo(lane, 4));
            const pack_u4 *qm = reinterpret_cast<const pack_u4 *>(g + pack_off_mid(lane, 0));
            const pack_u2 *qh = reinterpret_cast<const pack_u2 *>(g + pack_off_hi(lane, 0));
            lo0[r] = NT ? __builtin_nontemporal_load(q0) : *q0;
            lo1[r] = NT ? __builtin_nontemporal_load(q1) : *q1;
            mid[r] = NT ? __builtin_nontemporal_load(qm) : *qm;
            hi[r] = NT ? __builtin_nontemporal_load(qh) : *qh;
        }
        // ... and so are the headers and the first FIRST values of the exception lists (the lists have room for kPackCap values;
        // what lies behind a list's count is never indexed): nothing the tile loads waits for another load
        // (the headers are loaded per lane -- `perlane` is zero, but not to the compiler: as a wave-uniform value the header would
        // be moved to a scalar register right behind its load, and the wave would wait there for every load in front of it)
        uint32_t head[R];
#pragma unroll
        for (int r = 0; r < R; r++) head[r] = pk.hdr[unit0[r] + tt + perlane];
        double first = 0.0;
        if (stager) first = pk.exc[(unit0[wave - 1] + tt) * kPackCap + lane];
        __syncthreads();
        {
            // the p tile: four 16-byte loads a thread, issued back to back and written when all have come -- one round trip between
            // the tile's two barriers, not four (a rolled loop waits vmcnt(0) for each load in turn, and with it for every element,
            // header and list load issued in front of the first barrier).  Pairs behind the segment's end are loaded from a
            // 16-byte zero: the zeros the lanes past the end of a ragged tile multiply with (cols is even: the packed product
            // runs on whole 16-byte vectors only)
            typedef double pvec_t __attribute__((ext_vector_type(2)));
            typedef const __attribute__((address_space(1))) pvec_t *gptr_t;
            pvec_t *dst = reinterpret_cast<pvec_t *>(s_p);
            pvec_t v[TILE / 2 / NTHREADS];
#pragma unroll
            for (int k = 0; k < TILE / 2 / NTHREADS; k++) {
                const uint32_t col = 2u * ((uint32_t)tid + (uint32_t)k * NTHREADS);
                v[k] = *(col < cols ? (gptr_t)(a.p + c0 + col) : (gptr_t)kZeroVec16);      // global loads, not flat ones
            }
#pragma unroll
            for (int k = 0; k < TILE / 2 / NTHREADS; k++) dst[tid + k * NTHREADS] = v[k];
        }
        uint32_t shift[R];
#pragma unroll
        for (int r = 0; r < R; r++) {
            shift[r] = pack_exp_shift(pack_header_base(head[r]));
            if (stager && wave == 1 + r) s_exc[r][lane] = first;
            const uint32_t cnt = min(pack_header_count(head[r]), kPackCap);
            const double *e = pk.exc + (unit0[r] + tt) * kPackCap;
            for (uint32_t i = FIRST + tid; i < cnt; i += NTHREADS) s_exc[r][i] = e[i];      // a long list: one more round trip
        }
        __syncthreads();
        // whole tile: 4 super-steps; ragged last tile: ceil(cols / super-step) of them, the columns behind `cols` inside those
        // decode to +0.0 (reserved index) and meet the zeros of the p tile -- the plain kernel's +0 terms
        const int nsteps = (int)((cols + STEP * WAVES - 1) / (STEP * WAVES));
#pragma unroll
        for (int s = 0; s < WSTEPS; s++) {
            if (s < nsteps) {
                double pv[2];
#pragma unroll
                for (int i = 0; i < 2; i++) pv[i] = s_p[s * (STEP * WAVES) + woff + i];
#pragma unroll
                for (int r = 0; r < R; r++)
#pragma unroll
                    for (int i = 0; i < 2; i++) {
                        const int e = 2 * s + i;
                        const uint32_t l = e < 4 ? lo0[r][e & 3] : lo1[r][e & 3];
                        const uint32_t w = ((hi[r][e >> 2] >> (8 * (e & 3))) & 0xffu) << 16 | ((mid[r][e >> 1] >> (16 * (e & 1))) & 0xffffu);
                        // every lane reads the list: its exception's value, or the reserved +0.0 (one address for the whole wave)
                        const bool x = pack_is_exception(w);
                        const double ev = s_exc[r][x ? min(l, kPackZeroIdx) : kPackZeroIdx];
                        const double av = x ? ev : __longlong_as_double((long long)pack_decode(l, w, shift[r]));
                        acc[r] = fma_tv(av, pv[i], acc[r]);
                    }
            }
        }
        tt = tnext;
    }

#pragma unroll
    for (int r = 0; r < R; r++) {
        double s = wave_sum(acc[r]);
        if (lane == 0) s_part[r][wave] = s;
    }
    __syncthreads();
    if (tid < R) {
        const uint64_t row = row_first + tid;
        double d = 0.0;
        if (row < a.nrows) {
            double s = s_part[tid][0];
#pragma unroll
            for (int w = 1; w < WAVES; w++) s += s_part[tid][w];
            if (a.accumulate) s += a.y[row];
            store_y(a, row, s);
            d = (double)s * (double)a.p[a.row0 + row];
        }
        s_dot[tid] = d;
    }
    if (a.partial != nullptr) {
        __syncthreads();
        double t = 0.0;
        if (tid == 0) {
            t = s_dot[0];
#pragma unroll
            for (int r = 1; r < R; r++) t += s_dot[r];
        }
        publish_partial(t, a.partial, a.fin);
    }
}

// ==== From here to the matching #endif: TUNING BUILD ONLY (-DLAM_TUNING_VARIANTS, `make tuning` -> liblam_hip_tuning.so).
// The MFMA-fed bf16 GEMV: built, tested, measured, slower than the VALU kernel; bench.py measures it
// beside the product kernel for BASELINE configs[3].  The product library does not carry it.
#ifdef LAM_TUNING_VARIANTS
// ---------------------------------------------------------------------------------------------
// MFMA experiment for the bf16-storage GEMV (BASELINE configs[3]): can the matrix cores take the
// widening + FMA work off the VALU?  A wave loads 1 KiB = 512 contiguous bf16 of ONE matrix row
// (perfectly coalesced, exactly like the VALU kernels) and feeds the raw bytes as the A fragment of
// v_mfma_f32_32x32x16_bf16: lane l (r = l&31, h = l>>5) holds A[r][8h+j] = row[c + 8l + j].  The B
// fragment is the bf16 image of p at the SAME columns, B[8h+j][r] = p[c + 8l + j], so
//     D[m][n] = sum_{h,j} row[c + 8(32h+m) + j] * p[c + 8(32h+n) + j]
// and the DIAGONAL D[m][m] is the partial dot product of lanes m and m+32: trace(D) accumulated over
// the row is the row's dot product.  31/32 of the MFMA flops are discarded -- they are free, the
// kernel stays HBM-bound.  p is fp32: SPLIT = 3 feeds it as three bf16 terms (p = hi + mid + lo
// exactly, 8 mantissa bits each), i.e. three MFMAs per KiB and fp32-exact products; SPLIT = 1 rounds
// p to bf16 (classical bf16 x bf16 -> fp32 GEMV).
// ---------------------------------------------------------------------------------------------
typedef __bf16 mfma_bf16x8 __attribute__((ext_vector_type(8)));
typedef float mfma_f32x16 __attribute__((ext_vector_type(16)));

template <int R, int TILE, bool NT, int SPLIT>
__global__ void __launch_bounds__(kBlock)
gemv_mfma_bf16_kernel(GemvArgs<__hip_bfloat16, float> a)
{
    typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
    constexpr int STEP = 512;                       // bf16 elements per wave instruction (1 KiB)
    static_assert(TILE % STEP == 0, "tile must be a whole number of wave steps");
    constexpr int STEPS = TILE / STEP;

    __shared__ __attribute__((aligned(16))) unsigned short s_pb[SPLIT][TILE];
    __shared__ double s_red[kWaves];

    if (a.sc != nullptr && a.sc->stop) return;
    if (is_reducer_block(a.fin)) { reduce_partials(a.partial, (int)gridDim.x - 1, a.fin, s_red); return; }

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const uint64_t row_first = ((uint64_t)blockIdx.x * kWaves + wave) * R;

    const __hip_bfloat16 *rowp[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        uint64_t row = row_first + r;
        if (row >= a.nrows) row = a.nrows - 1;
        rowp[r] = a.A + row * a.lda + (uint64_t)lane * 8;
    }
    mfma_f32x16 acc[R];
#pragma unroll
    for (int r = 0; r < R; r++)
#pragma unroll
        for (int i = 0; i < 16; i++) acc[r][i] = 0.f;
    float tail[R];                                   // columns of a ragged last tile (VALU)
#pragma unroll
    for (int r = 0; r < R; r++) tail[r] = 0.f;

    const uint32_t ntiles0 = (uint32_t)((a.seg_end[0] - a.seg_begin[0] + TILE - 1) / TILE);
    const uint32_t ntiles = ntiles0 + (a.nseg > 1 ? (uint32_t)((a.seg_end[1] - a.seg_begin[1] + TILE - 1) / TILE) : 0u);
    uint32_t tt = blockIdx.x % ntiles;
    for (uint32_t t = 0; t < ntiles; t++) {
        const bool second = tt >= ntiles0;
        const uint64_t c0 = second ? a.seg_begin[1] + (uint64_t)(tt - ntiles0) * TILE : a.seg_begin[0] + (uint64_t)tt * TILE;
        const uint64_t cend = second ? a.seg_end[1] : a.seg_end[0];
        const uint32_t cols = (uint32_t)((cend - c0 < (uint64_t)TILE) ? (cend - c0) : (uint64_t)TILE);
        __syncthreads();
        for (uint32_t i = tid; i < (uint32_t)TILE; i += kBlock) {
            float v = i < cols ? a.p[c0 + i] : 0.f;            // zero padding: padded columns add 0
            if (SPLIT == 1) {
                s_pb[0][i] = __builtin_bit_cast(unsigned short, __float2bfloat16(v));
            } else {
#pragma unroll
                for (int sp = 0; sp < SPLIT; sp++) {
                    const unsigned bits = __float_as_uint(v) & 0xFFFF0000u;   // truncate to bf16: exact remainder
                    s_pb[sp][i] = (unsigned short)(bits >> 16);
                    v -= __uint_as_float(bits);
                }
            }
        }
        __syncthreads();
        const int full_steps = (int)(cols / STEP);
        auto step = [&](int s) {
            u16x8 av[R];
#pragma unroll
            for (int r = 0; r < R; r++) {
                const u16x8 *src = reinterpret_cast<const u16x8 *>(rowp[r] + c0 + (uint64_t)s * STEP);
                av[r] = NT ? __builtin_nontemporal_load(src) : *src;
            }
#pragma unroll
            for (int sp = 0; sp < SPLIT; sp++) {
                const u16x8 bv = *reinterpret_cast<const u16x8 *>(&s_pb[sp][s * STEP + lane * 8]);
#pragma unroll
                for (int r = 0; r < R; r++)
                    acc[r] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(mfma_bf16x8, av[r]),
                                                                     __builtin_bit_cast(mfma_bf16x8, bv), acc[r], 0, 0, 0);
            }
        };
        if (cols == TILE) {
#pragma unroll 4
            for (int s = 0; s < STEPS; s++) step(s);
        } else {
            for (int s = 0; s < full_steps; s++) step(s);
        }
        // ragged remainder of the last tile (cols % 512 != 0): plain VALU on the fp32 p
        for (uint32_t c = (uint32_t)full_steps * STEP + lane * 8; c < cols; c += STEP) {
#pragma unroll
            for (int r = 0; r < R; r++) {
                const u16x8 av = *reinterpret_cast<const u16x8 *>(rowp[r] + c0 + c - (uint64_t)lane * 8);
#pragma unroll
                for (int i = 0; i < 8; i++) tail[r] += __uint_as_float(((unsigned)av[i]) << 16) * a.p[c0 + c + i];
            }
        }
        tt = (tt + 1 == ntiles) ? 0 : tt + 1;
    }

    // trace of the accumulator: lane l (n = l&31, h = l>>5) holds D[n][n] in register
    // reg = ((n-4h)&3) + 4*((n-4h)>>3) when ((n-4h)&7) < 4  (C/D map: row = (reg&3) + 8*(reg>>2) + 4h)
    const int nn = lane & 31, hh = lane >> 5;
    const int d = nn - 4 * hh;
    const bool has_diag = d >= 0 && (d & 7) < 4;
    const int myreg = (d & 3) + 4 * (d >> 3);
    double dotp = 0.0;
#pragma unroll
    for (int r = 0; r < R; r++) {
        float v = 0.f;
#pragma unroll
        for (int i = 0; i < 16; i++) v = (has_diag && i == myreg) ? acc[r][i] : v;
        float s = wave_sum(v + tail[r]);
        const uint64_t row = row_first + r;
        if (lane == 0 && row < a.nrows) {
            if (a.accumulate) s += a.y[row];
            store_y(a, row, s);
            dotp += (double)s * (double)a.p[a.row0 + row];
        }
    }
    if (a.partial != nullptr) {
        __syncthreads();
        if (lane == 0) s_red[wave] = dotp;
        __syncthreads();
        double t = 0.0;
        if (tid == 0) {
            t = s_red[0];
#pragma unroll
            for (int w = 1; w < kWaves; w++) t += s_red[w];
        }
        publish_partial(t, a.partial, a.fin);
    }
}

#endif  // LAM_TUNING_VARIANTS (MFMA-fed bf16 GEMV)

// ---------------------------------------------------------------------------------------------
// Symmetric product (option "symmetric", single shard): y = A p reading only the UPPER triangle.
// CG needs A symmetric positive definite, so A[i][j] (j > i) can serve both y_i += A_ij p_j and
// y_j += A_ij p_i: 17.2 GB per product instead of 34.4 GB at N=65536 fp64 -- the only way past the
// HBM roofline of the plain GEMV.  Two passes (round 4: second shape; the round-1 shape flushed a column
// partial per 32 rows -- 0.55 GB written and read again per product -- and kept 32 row partials per lane).  The second pass is ONE body
// (symv_reduce_body: K interleaved columns of p) with two entry points: symv_reduce_kernel is its K = 1 case for one vector, on one
// shard or several, symv_many_reduce_kernel ("Symmetric batched product" below) serves the batch.  The first pass is still written
// twice (symv_task_kernel here, symv_many_task_kernel below): run through the batch's statements the single product measured 1-2 %
// slower at N = 65536 ... 131072 (profiles/symv_unified_parent_vs_branch.txt).
//   symv_task_kernel    one workgroup per TASK = a column strip (4 KiB per row, read contiguously by the
//                       4 waves: 512 fp64 / 1024 fp32 columns; two vectors per lane ran level or 2-5 % behind,
//                       profiles/r04_symv2_probe.txt, and are no longer instantiated: NV = 1) x a run of rows (2048 for the
//                       bulk of the triangle, 512 from 60 % of the work on, 64 for the last 8 %, so that the launch
//                       ends on short tasks; shorter runs for small N).  A lane keeps the column partials of its
//                       columns in registers over ALL rows of the task and 8 row partials at a time: every 8 rows they
//                       are summed across the wave by a transposed butterfly (wave_sum8: 7 exchanged values
//                       for 8 rows instead of 48) and parked in LDS, which is flushed every 256 rows.  Tasks are
//                       dispatched row run by row run, all strips of a run side by side: whole rows stream, as
//                       in the GEMV.  Elements left of the diagonal are masked (not even read where a whole
//                       16-byte vector lies left of it); the diagonal counts once.
//   symv_reduce_kernel  y[i] = the row partials of i's row run + the column partials of the tasks of i's strip,
//                       fixed order (deterministic), plus the workgroup's partial of p.y.
// Partials: ~70 MB written and read per product at N=65536, indexed by task in dispatch order (see symv_reduce_kernel:
// their stores are what separates the first pass from the rate of its loads alone).  Any N (rows are padded to whole
// vectors with zeros, p likewise).  The caller asserts symmetry (lam_hip_check_symmetry measures it).
// ---------------------------------------------------------------------------------------------
constexpr int kSymvRowsLds = 256;      // row partials parked in LDS before they are stored (a task flushes them every 256 rows)
constexpr int kSymvRowsMax = 2048;     // rows of the tallest task
constexpr int kSymvListChunk = 1024;   // entries of a strip's task list the second pass stages in LDS at a time
constexpr int kSymvReduceRows = 32;    // rows per workgroup of the second pass = p.Ap partials per product: ceil(n / 32)
// SymvTask, SymvIndex, the task flags and the use rule symv_use<CYC> live in lam_host_plan.h: the host's planner and its exhaustive
// check are built from the same definitions, also by plain g++ under AddressSanitizer (tests/host_asan).

// lane exchanges of the transposed butterfly.  gfx950: v_permlane32_swap / v_permlane16_swap move both directions of a
// halving step in one instruction (no select, no LDS crossbar); inside a 16-lane row DPP: rotation by 8 (= lane ^ 8),
// half-row mirror (lane -> 7 - lane within 8 lanes), quad permutes (lane ^ 2, lane ^ 1).
template <int CTRL> __device__ __forceinline__ unsigned dpp_u32(unsigned v) { return __builtin_amdgcn_update_dpp(0u, v, CTRL, 0xf, 0xf, false); }
template <int CTRL> __device__ __forceinline__ float dpp_t(float v) { return __uint_as_float(dpp_u32<CTRL>(__float_as_uint(v))); }
template <int CTRL> __device__ __forceinline__ double dpp_t(double v)
{
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = dpp_u32<CTRL>((unsigned)u), hi = dpp_u32<CTRL>((unsigned)(u >> 32));
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
template <int W> __device__ __forceinline__ void permlane_swap(unsigned &x, unsigned &y)
{
    if (W == 32) { auto r = __builtin_amdgcn_permlane32_swap(x, y, false, false); x = r[0]; y = r[1]; }
    else { auto r = __builtin_amdgcn_permlane16_swap(x, y, false, false); x = r[0]; y = r[1]; }
}
// x belongs to the lower half (of 2W lanes), y to the upper: lower lanes return x(l) + x(l + W), upper lanes y(l - W) + y(l)
template <int W> __device__ __forceinline__ float fold_halves(float x, float y)
{
    unsigned a = __float_as_uint(x), b = __float_as_uint(y);
    permlane_swap<W>(a, b);
    return __uint_as_float(a) + __uint_as_float(b);
}
template <int W> __device__ __forceinline__ double fold_halves(double x, double y)
{
    const unsigned long long ux = (unsigned long long)__double_as_longlong(x), uy = (unsigned long long)__double_as_longlong(y);
    unsigned xl = (unsigned)ux, xh = (unsigned)(ux >> 32), yl = (unsigned)uy, yh = (unsigned)(uy >> 32);
    permlane_swap<W>(xl, yl);
    permlane_swap<W>(xh, yh);
    return __longlong_as_double((long long)(((unsigned long long)xh << 32) | xl)) +
           __longlong_as_double((long long)(((unsigned long long)yh << 32) | yl));
}
// 8 per-lane values -> lane L returns the wave total of value (L >> 3) & 7.  Fixed order.
template <typename T>
__device__ __forceinline__ T wave_sum8(const T (&v)[8])
{
    const bool b3 = threadIdx.x & 8;
    T w[4], u[2];
#pragma unroll
    for (int j = 0; j < 4; j++) w[j] = fold_halves<32>(v[j], v[4 + j]);
#pragma unroll
    for (int j = 0; j < 2; j++) u[j] = fold_halves<16>(w[j], w[2 + j]);
    const T keep = b3 ? u[1] : u[0], send = b3 ? u[0] : u[1];
    T t = keep + dpp_t<0x128>(send);      // row_ror:8
    t += dpp_t<0x141>(t);                 // row_half_mirror
    t += dpp_t<0x4e>(t);                  // quad_perm [2,3,0,1]
    t += dpp_t<0xb1>(t);                  // quad_perm [1,0,3,2]
    return t;
}

// Launched with kSymvLdsPerWorkgroup bytes of LDS in all (its row-partial buffer + idle dynamic LDS), i.e. THREE workgroups per
// CU: the tasks' loads alone run at 7.22 TB/s with three workgroups per CU against 7.0 with the five its registers allow, the
// whole pass 1-2 % faster (fewer row streams in flight at a time; profiles/r04_symv2_probe.txt).
constexpr unsigned kSymvLdsPerWorkgroup = 53 * 1024;
template <typename T, int K> constexpr unsigned symv_lds_pad() { return kSymvLdsPerWorkgroup - (unsigned)sizeof(T) * kWaves * kSymvRowsLds * K; }   // T: vector type

template <typename TA, typename T, bool CYC>     // TA: storage of the matrix; T: vectors, products, partials (bf16 storage: float)
__global__ void __launch_bounds__(kBlock)
symv_task_kernel(const TA *__restrict__ A, const T *__restrict__ p, const SymvTask *__restrict__ tasks, T *__restrict__ rowpart,
                 T *__restrict__ colpart, uint64_t lda, uint64_t ncols_vec, uint64_t n, uint64_t row_off, const CgScalars *sc)
{
    using MV = MatVec<TA>;
    using vec_t = typename MV::vec_t;                                // 16 bytes of matrix elements
    constexpr int NV = 1;                                            // 16-byte vectors per lane and row: two ran level or behind (profiles/r04_symv2_probe.txt)
    constexpr int VEC = MV::N, CW = kBlock * VEC, SS = NV * CW;     // CW: columns the workgroup covers with one vector per lane
    typedef T tvec_t __attribute__((ext_vector_type(VEC)));          // the same columns of a vector / a column partial
    __shared__ T s_rows[kWaves][kSymvRowsLds];
    if (sc != nullptr && sc->stop) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    SymvTask t = tasks[blockIdx.x];                                                  // row0: LOCAL row (A, rowpart); global = row_off + row0
    const bool interior = (t.nrows & kSymvInterior) != 0, full = (t.nrows & kSymvFull) != 0;
    t.nrows &= ~kSymvFlags;
    const uint64_t c0 = (uint64_t)t.strip * SS, c = c0 + (uint64_t)tid * VEC;       // this lane's columns: c + v * CW + i
    const uint64_t grow0 = row_off + t.row0;
    bool live[NV];                                                                   // columns behind the row's end: nothing to do
    tvec_t pc[NV];
    T cacc[NV][VEC];
#pragma unroll
    for (int v = 0; v < NV; v++) {
        live[v] = c + (uint64_t)v * CW < ncols_vec;
#pragma unroll
        for (int i = 0; i < VEC; i++) { pc[v][i] = (T)0; cacc[v][i] = (T)0; }
        if (live[v]) pc[v] = *reinterpret_cast<const tvec_t *>(p + c + (uint64_t)v * CW);
    }
    // Interior tasks -- nearly all of them -- take the lean loop: unconditional loads from UNIFORM row bases plus the lane's
    // constant offset (no exec-mask juggling between the loads: the predicated form below issued its loads one branch at a time
    // and spent half of its wave cycles on issue stalls), the rows' values of p by scalar loads; software-pipelined in two halves
    // of 4 rows -- the loads of the next step's half are issued as soon as this step's half has been consumed, so a wave always
    // has 4 * NV ... 8 * NV loads in flight (a loop that drains its loads, computes its ~125 vector instructions and only then
    // issues the next ones measured 1-4 % slower, profiles/r04_symv2_probe.txt).
    // the row partials of the last (up to) 256 rows, ending at row `end` of the task: out of LDS into rowpart (uniform call sites)
    auto flush_rows = [&](uint32_t end) {
        const uint32_t beg = (end - 1) & ~(uint32_t)(kSymvRowsLds - 1);
        __syncthreads();
        for (uint32_t r = beg + tid; r < end && r < t.nrows; r += kBlock) {
            const uint32_t q = r - beg;
#ifdef LAM_SYMV_PROBE_NO_PARTIAL_STORES      /* tools/symv2_probe only: what the partial stores cost (results are wrong without them) */
            if (s_rows[0][q] == (T)123.456)
#endif
            __builtin_nontemporal_store((s_rows[0][q] + s_rows[1][q]) + (s_rows[2][q] + s_rows[3][q]), rowpart + (uint64_t)t.rp + r);
        }
        __syncthreads();
    };
    auto lean_loop = [&](auto masked_tag) {
        constexpr bool MASKED = decltype(masked_tag)::value;
        const TA *rows = A + (uint64_t)t.row0 * lda + c0;          // uniform
        const T *prow = p + grow0;
        vec_t a0[4][NV], a1[4][NV];
#pragma unroll
        for (int k = 0; k < 4; k++)
#pragma unroll
            for (int v = 0; v < NV; v++) {
                a0[k][v] = __builtin_nontemporal_load(reinterpret_cast<const vec_t *>(rows + (uint64_t)k * lda + v * CW) + tid);
                a1[k][v] = __builtin_nontemporal_load(reinterpret_cast<const vec_t *>(rows + (uint64_t)(k + 4) * lda + v * CW) + tid);
            }
        for (uint32_t b = 0; b < t.nrows; b += 8, prow += 8) {
            rows += 8 * lda;
            const bool more = b + 8 < t.nrows;
            T racc[8];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const T pr = prow[k];
                T r = (T)0;
#pragma unroll
                for (int v = 0; v < NV; v++)
#pragma unroll
                    for (int i = 0; i < VEC; i++) {
                        bool rs = true, cs = true;
                        if (MASKED) symv_use<CYC>(c + (uint64_t)v * CW + i, grow0 + b + k, n, &rs, &cs);
                        if (rs) r = fma_tv((T)MV::get(a0[k][v], i), (T)pc[v][i], r);
                        if (cs) cacc[v][i] = fma_tv((T)MV::get(a0[k][v], i), pr, cacc[v][i]);
                    }
                racc[k] = r;
            }
            if (more) {
#pragma unroll
                for (int k = 0; k < 4; k++)
#pragma unroll
                    for (int v = 0; v < NV; v++)
                        a0[k][v] = __builtin_nontemporal_load(reinterpret_cast<const vec_t *>(rows + (uint64_t)k * lda + v * CW) + tid);
            }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const T pr = prow[4 + k];
                T r = (T)0;
#pragma unroll
                for (int v = 0; v < NV; v++)
#pragma unroll
                    for (int i = 0; i < VEC; i++) {
                        bool rs = true, cs = true;
                        if (MASKED) symv_use<CYC>(c + (uint64_t)v * CW + i, grow0 + b + 4 + k, n, &rs, &cs);
                        if (rs) r = fma_tv((T)MV::get(a1[k][v], i), (T)pc[v][i], r);
                        if (cs) cacc[v][i] = fma_tv((T)MV::get(a1[k][v], i), pr, cacc[v][i]);
                    }
                racc[4 + k] = r;
            }
            if (more) {
#pragma unroll
                for (int k = 0; k < 4; k++)
#pragma unroll
                    for (int v = 0; v < NV; v++)
                        a1[k][v] = __builtin_nontemporal_load(reinterpret_cast<const vec_t *>(rows + (uint64_t)(k + 4) * lda + v * CW) + tid);
            }
            const T tot = wave_sum8(racc);
            if ((lane & 7) == 0) s_rows[wave][(b & (kSymvRowsLds - 1)) + (lane >> 3)] = tot;
            if (((b + 8) & (kSymvRowsLds - 1)) == 0 || b + 8 >= t.nrows) flush_rows(b + 8);
        }
    };
    if (interior) lean_loop(std::false_type());
    else if (full) lean_loop(std::true_type());      // the rim of the rows' windows in full strips: the same loads, every product tested
    else {
        // ragged strips and row runs: every load and every product tested
        const TA *Arow = A + (uint64_t)t.row0 * lda + c;
        for (uint32_t b = 0; b < t.nrows; b += 8) {
            vec_t a[8][NV];
            T pr[8];
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const uint64_t grow = grow0 + b + k;
#pragma unroll
                for (int v = 0; v < NV; v++) {
#pragma unroll
                    for (int i = 0; i < VEC; i++) a[k][v][i] = 0;
                    // one shard: a vector whose columns all lie left of the diagonal is not read at all
                    if (live[v] && b + k < t.nrows && (CYC || c + (uint64_t)v * CW + VEC > grow))
                        a[k][v] = __builtin_nontemporal_load(reinterpret_cast<const vec_t *>(Arow + (uint64_t)(b + k) * lda + (uint64_t)v * CW));
                }
                pr[k] = b + k < t.nrows ? p[grow] : (T)0;
            }
            T racc[8];
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const uint64_t grow = grow0 + b + k;
                T r = (T)0;
#pragma unroll
                for (int v = 0; v < NV; v++)
#pragma unroll
                    for (int i = 0; i < VEC; i++) {
                        bool rs, cs;
                        symv_use<CYC>(c + (uint64_t)v * CW + i, grow, n, &rs, &cs);
                        if (rs) r = fma_tv((T)MV::get(a[k][v], i), (T)pc[v][i], r);
                        if (cs) cacc[v][i] = fma_tv((T)MV::get(a[k][v], i), pr[k], cacc[v][i]);
                    }
                racc[k] = r;
            }
            const T tot = wave_sum8(racc);
            if ((lane & 7) == 0) s_rows[wave][(b & (kSymvRowsLds - 1)) + (lane >> 3)] = tot;
            if (((b + 8) & (kSymvRowsLds - 1)) == 0 || b + 8 >= t.nrows) flush_rows(b + 8);
        }
    }
#pragma unroll
    for (int v = 0; v < NV; v++)
        if (live[v]) {
            tvec_t out;
#pragma unroll
            for (int i = 0; i < VEC; i++) out[i] = cacc[v][i];
#ifdef LAM_SYMV_PROBE_NO_PARTIAL_STORES      /* tools/symv2_probe only: what the partial stores cost (results are wrong without them) */
            if (out[0] == (T)123.456)
#endif
            __builtin_nontemporal_store(out, reinterpret_cast<tvec_t *>(colpart + (uint64_t)blockIdx.x * SS + (uint64_t)v * CW + (uint64_t)tid * VEC));
        }
}

// Second pass, written once for both entry points too.  32 rows of y per workgroup, K accumulators per thread; the terms of an
// entry are dealt round-robin to 8 groups of 32 lanes and combined in a fixed order, the same for every column.  Both kinds of
// partial are indexed BY TASK, in dispatch order -- rowpart[task][row of the run], colpart[task][column of the strip] --, so that
// the tasks in flight together write next to each other: with the partials laid out by strip (a 4-KiB column partial every ~1 MiB,
// a 2-KiB row partial every 512 KiB) the first pass ran up to 10 % slower depending on where the buffers happened to be placed
// (2.57 ... 2.85 ms for the same launch at N=65536; with every task writing ONE slot 2.52 ... 2.61: profiles/r04_symv2_probe.txt)
// -- 1 % of the traffic, but scattered over as many pages as tasks.  Row side: the tasks of the row's run (consecutive) for the rows
// this shard owns, [row_off, row_off + nloc); column side: the tasks listed for the column's strip.  The epilogue has one thread per
// (row, column), element e = row * K + j of the workgroup: SHIFT adds shift[j] p_j[row] with one fma, store(global element, value)
// puts the entry where the entry point wants it, and -- want_dot -- publish(j, d) takes the workgroup's partial d of p_j.y_j, the 32
// terms summed in row order.  s_dot is the caller's (the single entry point's reducer workgroup uses it as well).
template <typename T, int SS, int K, bool SHIFT, typename Store, typename Publish>         // T: vectors and partials; SS: columns of a strip
__device__ __forceinline__ void
symv_reduce_body(const T *__restrict__ rowpart, const T *__restrict__ colpart, const uint32_t *__restrict__ index, const SymvIndex &ix,
                 const T *__restrict__ p, uint64_t n, uint64_t row_off, uint64_t nloc, const T *shift, double (&s_dot)[K][kSymvReduceRows],
                 bool want_dot, Store store, Publish publish)
{
    constexpr int RB = kSymvReduceRows, G = kBlock / RB;
    static_assert(RB * K <= kBlock, "one epilogue thread per (row, column)");
    __shared__ T s[G][RB * K];
    __shared__ uint32_t s_list[kSymvListChunk];
    const int l = threadIdx.x % RB, g = threadIdx.x / RB;
    const uint64_t i = (uint64_t)blockIdx.x * RB + l;
    T acc[K];
#pragma unroll
    for (int j = 0; j < K; j++) acc[j] = (T)0;
    if (i < n && i >= row_off && i < row_off + nloc) {
        const uint64_t il = i - row_off;
        const uint32_t *run = index + ix.runs + 5 * index[ix.row8 + (il >> 3)];
        const uint32_t cnt = run[1], h = run[3];
        const T *src = rowpart + ((uint64_t)run[4] + (il - run[2])) * K;
        const uint64_t hk = (uint64_t)h * K;
        uint32_t q = g;
        for (; q + 3 * G < cnt; q += 4 * G) {
#pragma unroll
            for (int j = 0; j < K; j++) {
                const T a0 = src[(uint64_t)q * hk + j], a1 = src[(uint64_t)(q + G) * hk + j];
                const T a2 = src[(uint64_t)(q + 2 * G) * hk + j], a3 = src[(uint64_t)(q + 3 * G) * hk + j];
                acc[j] += (a0 + a1) + (a2 + a3);
            }
        }
        for (; q < cnt; q += G)
#pragma unroll
            for (int j = 0; j < K; j++) acc[j] += src[(uint64_t)q * hk + j];
    }
    // column side: the workgroup's 32 columns lie in ONE strip (32 divides the strip width), so its task list is staged in LDS
    // once per 1024 entries -- a load of the list in front of every load of a partial doubled the chain of memory latencies that
    // this pass is made of at small N
    {
        const uint32_t s0 = (uint32_t)(((uint64_t)blockIdx.x * RB) / SS);
        const uint32_t lb = index[ix.strip_base + s0], le = index[ix.strip_base + s0 + 1];
        const uint32_t *list = index + ix.strip_tasks;
        const T *src = colpart + (i - (uint64_t)s0 * SS) * K;
        constexpr uint64_t SK = (uint64_t)SS * K;
        for (uint32_t base = lb; base < le; base += kSymvListChunk) {
            const uint32_t cnt = le - base < (uint32_t)kSymvListChunk ? le - base : (uint32_t)kSymvListChunk;
            __syncthreads();                                  // the previous chunk has been consumed
            for (uint32_t q = threadIdx.x; q < cnt; q += kBlock) s_list[q] = list[base + q];
            __syncthreads();
            if (i < n) {
                uint32_t k = g;
                for (; k + 7 * G < cnt; k += 8 * G) {
#pragma unroll
                    for (int j = 0; j < K; j++) {
                        T a[8];
#pragma unroll
                        for (int u = 0; u < 8; u++) a[u] = src[(uint64_t)s_list[k + u * G] * SK + j];
                        acc[j] += ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
                    }
                }
                for (; k < cnt; k += G)
#pragma unroll
                    for (int j = 0; j < K; j++) acc[j] += src[(uint64_t)s_list[k] * SK + j];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < K; j++) s[g][l * K + j] = acc[j];
    __syncthreads();
    if (threadIdx.x < RB * K) {
        const int e = threadIdx.x, row = e / K, j = e % K;
        const uint64_t ir = (uint64_t)blockIdx.x * RB + row;
        T t = s[0][e];
#pragma unroll
        for (int k = 1; k < G; k++) t += s[k][e];
        double d = 0.0;
        if (ir < n) {
            const T pj = p[ir * K + j];
            if constexpr (SHIFT) t = fma_tv(shift[j], pj, t);
            store(ir * K + j, t);
            d = (double)t * (double)pj;
        }
        s_dot[j][row] = d;
    }
    if (want_dot) {
        __syncthreads();
        if (threadIdx.x < K) {
            double d = 0.0;
#pragma unroll
            for (int k = 0; k < RB; k++) d += s_dot[threadIdx.x][k];
            publish((int)threadIdx.x, d);
        }
    }
}

// The single product's second pass.  One shard: y is the product, `partial` its p.y per workgroup.  Several shards (dst.n > 0): the
// entry is this shard's CONTRIBUTION to y[i] (row-side partials only for the rows it owns), stored into its record in every shard's
// gather buffer; the consumer adds the shards' records in shard order; the launch carries one extra workgroup (fin.active) that sums
// the workgroups' parts of p.Ap in the fixed order of block_sum_array and writes the total behind the record (see Finalize).
template <typename T, int SS>
__global__ void __launch_bounds__(kBlock)
symv_reduce_kernel(const T *__restrict__ rowpart, const T *__restrict__ colpart, const uint32_t *__restrict__ index, SymvIndex ix,
                   const T *__restrict__ p, T *__restrict__ y, double *__restrict__ partial, uint64_t n, uint64_t row_off,
                   uint64_t nloc, PtrList dst, Finalize fin, const CgScalars *sc)
{
    __shared__ double s_dot[1][kSymvReduceRows];
    if (sc != nullptr && sc->stop) return;
    if (is_reducer_block(fin)) {                        // several shards: the shard's part of p.Ap as ONE number, inside this launch
        reduce_partials(partial, (int)compute_blocks(fin), fin, s_dot[0]);
        return;
    }
    symv_reduce_body<T, SS, 1, false>(
        rowpart, colpart, index, ix, p, n, row_off, nloc, (const T *)nullptr, s_dot, partial != nullptr,
        [&](uint64_t i, T t) {
            if (dst.n == 0) y[i] = t;
            else for (int j = 0; j < dst.n; j++) reinterpret_cast<T *>(dst.p[j])[i] = t;
        },
        [&](int, double d) { publish_partial(d, partial, fin); });   // plain store, or the self-flagging slot the reducer workgroup waits for
}

// The asymmetry of the matrix one process holds, over every pair {A[i][j], A[j][i]}; three per-workgroup maxima, in out[blockIdx.x],
// out[gridDim.x + blockIdx.x] and out[2 * gridDim.x + blockIdx.x]:
//   [0] max |A[i][j] - A[j][i]|.  A pair the two triangles agree on (equal values, infinities of one sign, two NaNs, zeros of either
//       sign) counts 0; a pair they disagree on with a non-finite member (NaN or Inf against anything else) counts +Inf, so that it
//       can neither drop out of a maximum (every comparison with NaN is false) nor hide behind max |A| = Inf;
//   [1] max |A[i][j]| over the FINITE elements (what a tolerance may be scaled by);
//   [2] the largest |A[i][j] - A[j][i]| among the pairs that differ by more than `rel` * max(|A[i][j]|, |A[j][i]|) (finite members
//       only), 0 if there is none: with rel = 2^-7 the pairs that are further apart than one bf16 unit in the last place of the pair;
//       with rel = 0 the same as [0].  A per-pair rule  |d| <= max(rel * max(|u|, |l|), abs_tol)  is violated somewhere iff [2] > abs_tol.
// 32 x 32 tiles of the upper triangle through LDS, so that both the tile and its mirror image are read along rows (one pass over the
// matrix at a useful fraction of the stream rate: this runs once per matrix when a driver asks for the symmetric product through the
// environment, lam_exchange.h env_symmetric_check).
__device__ __forceinline__ double elem_as_double(double v) { return v; }
__device__ __forceinline__ double elem_as_double(float v) { return (double)v; }
__device__ __forceinline__ double elem_as_double(__hip_bfloat16 v) { return (double)__uint_as_float(((unsigned)*reinterpret_cast<const unsigned short *>(&v)) << 16); }
// Several row shards of ONE process (`shards.n` > 1): row i lives in shard min(i / base_rows, shards.n - 1) (the reference's
// partition), whose matrix the launching device reads through peer access -- one-off, at the speed of the links.
template <typename T>
__global__ void __launch_bounds__(kBlock)
asymmetry_kernel(PtrList shards, uint64_t base_rows, uint64_t lda, uint64_t n, double rel, double *__restrict__ out)
{
    auto elem = [&](uint64_t i, uint64_t j) -> double {
        uint64_t q = shards.n > 1 ? i / base_rows : 0;
        if (q >= (uint64_t)shards.n) q = (uint64_t)shards.n - 1;
        return elem_as_double(static_cast<const T *>(shards.p[q])[(i - q * base_rows) * lda + j]);
    };
    constexpr int TS = 32;
    __shared__ double s_up[TS][TS + 1], s_lo[TS][TS + 1];
    __shared__ double s_max[3][kWaves];
    const double inf = __longlong_as_double(0x7FF0000000000000ll);
    double m = 0.0, a = 0.0, x = 0.0;
    const uint64_t nt = (n + TS - 1) / TS, ntiles = nt * (nt + 1) / 2;
    const int tx = threadIdx.x % TS, ty = threadIdx.x / TS;          // 32 x 8 threads: four row passes per tile
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        // tile (bi, bj) with bj >= bi, numbered row by row of the upper block triangle
        uint64_t bi = (uint64_t)((2.0 * (double)nt + 1.0 - sqrt((2.0 * (double)nt + 1.0) * (2.0 * (double)nt + 1.0) - 8.0 * (double)t)) * 0.5);
        while (bi > 0 && bi * nt - bi * (bi - 1) / 2 > t) bi--;
        while ((bi + 1) * nt - (bi + 1) * bi / 2 <= t) bi++;
        const uint64_t bj = bi + (t - (bi * nt - bi * (bi - 1) / 2));
        __syncthreads();
        for (int r = ty; r < TS; r += kBlock / TS) {
            const uint64_t iu = bi * TS + r, ju = bj * TS + tx;       // element (iu, ju) of the upper tile
            const uint64_t il = bj * TS + r, jl = bi * TS + tx;       // element (il, jl) of its mirror image
            s_up[r][tx] = (iu < n && ju < n) ? elem(iu, ju) : 0.0;
            s_lo[r][tx] = (il < n && jl < n) ? elem(il, jl) : 0.0;
        }
        __syncthreads();
        for (int r = ty; r < TS; r += kBlock / TS) {
            const double u = s_up[r][tx], l = s_lo[tx][r];             // A[bi*TS + r][bj*TS + tx] and A[bj*TS + tx][bi*TS + r]
            const double au = fabs(u), al = fabs(l);
            const double fu = au < inf ? au : 0.0, fl = al < inf ? al : 0.0;       // Inf and NaN (the comparison is false): 0
            const double v = fu > fl ? fu : fl;
            const bool same = u == l || (u != u && l != l);
            const double diff = fabs(u - l);
            const double d = same ? 0.0 : (diff < inf ? diff : inf);               // a NaN difference counts as Inf
            m = d > m ? d : m;
            a = v > a ? v : a;
            x = (d > rel * v && d > x) ? d : x;
        }
    }
    // from here on no value is a NaN: plain comparisons keep the maxima
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(m, off, 64), q = __shfl_xor(a, off, 64), e = __shfl_xor(x, off, 64);
        m = o > m ? o : m;
        a = q > a ? q : a;
        x = e > x ? e : x;
    }
    if ((threadIdx.x & 63) == 0) { s_max[0][threadIdx.x >> 6] = m; s_max[1][threadIdx.x >> 6] = a; s_max[2][threadIdx.x >> 6] = x; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 0; k < 3; k++) {
            double t = s_max[k][0];
            for (int w = 1; w < kWaves; w++) t = s_max[k][w] > t ? s_max[k][w] : t;
            out[(size_t)k * gridDim.x + blockIdx.x] = t;
        }
    }
}

// General path (any n, any alignment): one wave per row, per-row alignment peel + 16-B loads, p from L2.
template <typename TA, typename TV>
__global__ void __launch_bounds__(kBlock)
gemv_generic_kernel(GemvArgs<TA, TV> a)
{
    __shared__ double s_red[kWaves];
    if (a.sc != nullptr && a.sc->stop) return;
    if (is_reducer_block(a.fin)) { reduce_partials(a.partial, (int)gridDim.x - 1, a.fin, s_red); return; }
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const uint64_t row = (uint64_t)blockIdx.x * kWaves + wave;
    double dotp = 0.0;
    if (row < a.nrows) {
        const TA *ar = a.A + row * a.lda;
        TV acc = (TV)0;
        using MV = MatVec<TA>;
        using avec_t = typename MV::vec_t;
        constexpr int VEC = MV::N;
        for (int sg = 0; sg < a.nseg; sg++) {
            const uint64_t beg = a.seg_begin[sg], end = a.seg_end[sg];
            // Rows of an odd-N matrix start at any element offset: peel scalar columns up to the next
            // 16-byte boundary of THIS row, stream the aligned middle with 16-B non-temporal loads
            // (p is read element-wise from L2: its alignment differs from the row's), finish scalar.
            const uint64_t addr = reinterpret_cast<uint64_t>(ar + beg);
            uint64_t peel = ((16 - (addr & 15)) & 15) / sizeof(TA);
            if (peel > end - beg) peel = end - beg;
            if ((uint64_t)lane < peel) acc += widen<TV>(ar[beg + lane]) * a.p[beg + lane];
            const uint64_t mid = beg + peel;
            const uint64_t nvec = (end - mid) / VEC;
            uint64_t v = lane;
#pragma unroll 1
            for (; v + 3 * 64 < nvec; v += 4 * 64) {
                avec_t av[4];
#pragma unroll
                for (int u = 0; u < 4; u++)
                    av[u] = __builtin_nontemporal_load(reinterpret_cast<const avec_t *>(ar + mid) + v + u * 64);
#pragma unroll
                for (int u = 0; u < 4; u++)
#pragma unroll
                    for (int i = 0; i < VEC; i++) acc += (TV)MV::get(av[u], i) * a.p[mid + (v + u * 64) * VEC + i];
            }
            for (; v < nvec; v += 64) {
                const avec_t av = *(reinterpret_cast<const avec_t *>(ar + mid) + v);
#pragma unroll
                for (int i = 0; i < VEC; i++) acc += (TV)MV::get(av, i) * a.p[mid + v * VEC + i];
            }
            for (uint64_t c = mid + nvec * VEC + lane; c < end; c += 64) acc += widen<TV>(ar[c]) * a.p[c];
        }
        acc = wave_sum(acc);
        if (lane == 0) {
            if (a.accumulate) acc += a.y[row];
            store_y(a, row, acc);
            dotp = (double)acc * (double)a.p[a.row0 + row];
        }
    }
    if (a.partial != nullptr) {
        if (lane == 0) s_red[wave] = dotp;
        __syncthreads();
        double t = 0.0;
        if (threadIdx.x == 0) {
            t = s_red[0];
#pragma unroll
            for (int w = 1; w < kWaves; w++) t += s_red[w];
        }
        publish_partial(t, a.partial, a.fin);
    }
}

// ---------------------------------------------------------------------------------------------
// vector kernels
//   cg_init: finalize_sum_kernel, cg_init_kernel, cg_init_scalars_kernel (cg_init_full_kernel with the gather-Ap exchange below);
//   the vector step alpha = rr / p.Ap; x += alpha p; r -= alpha Ap; r.r; beta; the stop test; p = r + beta p:
//                         sliced vectors (one shard, exchange 0 and 2)   full-length vectors (gather-Ap exchange)
//       two kernels       update_xr_kernel, update_p_kernel              update_xr_full_kernel, update_p_full_kernel
//       one launch        update_fused_kernel                            update_full_fused_kernel
//   every statement of it is in the helpers in front of update_xr_kernel (and gathered_ap / gathered_pap in front of
//   update_xr_full_kernel); a kernel body is its role split plus calls to them.
// ---------------------------------------------------------------------------------------------
// sum src[0..n) with one workgroup and store it at index `slot` of every destination array
// (cg_init only: inside the iteration the producer kernels do this themselves, see Finalize)
__global__ void __launch_bounds__(kBlock)
finalize_sum_kernel(const double *__restrict__ src, int n, PtrList dst, int slot, const CgScalars *sc)
{
    __shared__ double s_red[kWaves];
    if (sc != nullptr && sc->stop) return;
    double t = block_sum_array(src, n, s_red);
    if (threadIdx.x == 0)
        for (int j = 0; j < dst.n; j++) reinterpret_cast<double *>(dst.p[j])[slot] = t;
}

// x = 0, r = b, p_slice = b (into every shard's p), partials of b.b
template <typename TV>
__global__ void __launch_bounds__(kBlock)
cg_init_kernel(const TV *__restrict__ b, TV *__restrict__ x, TV *__restrict__ r, PtrList pdst,
               uint64_t row0, uint64_t n_loc, double *__restrict__ partial)
{
    __shared__ double s_red[kWaves];
    double acc = 0.0;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n_loc; i += (uint64_t)gridDim.x * kBlock) {
        const TV bi = b[i];
        x[i] = (TV)0;
        r[i] = bi;
        for (int j = 0; j < pdst.n; j++) reinterpret_cast<TV *>(pdst.p[j])[row0 + i] = bi;
        acc += (double)bi * (double)bi;
    }
    double t = block_sum(acc, s_red);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

// bb = rr[0] = sum(red); iters = 0; stop = 0
__global__ void __launch_bounds__(kBlock)
cg_init_scalars_kernel(const double *__restrict__ red, int nred, CgScalars *sc)
{
    __shared__ double s_red[kWaves];
    double t = block_sum_array(red, nred, s_red);
    if (threadIdx.x == 0) {
        sc->bb = t;
        sc->rr[0] = t;
        sc->rr[1] = 0.0;
        sc->pAp = 0.0;
        sc->alpha = 0.0;
        sc->beta = 0.0;
        sc->iters = 0;
        sc->stop = 0;
    }
}

// ---- The recurrence of the vector step, written ONCE.  The six kernels below (update_xr / update_p / update_fused on sliced
// vectors, update_xr_full / update_p_full / update_full_fused on full-length ones) are a role split -- who reduces, who computes,
// who waits, where p.Ap and r.r come from -- around these helpers, so "fused vs two kernels", "one process vs rank mode" and
// "exchange 2 vs 0" run the same statements by construction.  A caller supplies the first index and the stride of its sweeps
// (its element -> thread mapping) and says which thread is the leader that keeps CgScalars.

// alpha = rr / p.Ap, in double and in the vectors' type; rr = r.r of the previous iteration
template <typename TV> struct CgAlpha { double rr, alpha_d; TV alpha; };
template <typename TV>
__device__ __forceinline__ CgAlpha<TV> cg_alpha(const CgScalars *sc, int k, double pAp)
{
    CgAlpha<TV> a;
    a.rr = sc->rr[(k + 1) & 1];
    a.alpha_d = a.rr / pAp;
    a.alpha = (TV)a.alpha_d;
    return a;
}

// r -= alpha Ap over [first, first + stride, ...) of n elements and x += alpha p where the element lies in the x window
// [row0, row0 + n_loc) (sliced vectors: the whole sweep); returns the thread's part of r.r.  ap_at(i) is element i of A p.
// (axpby(alpha,p,1,x); axpby(-alpha,Ap,1,r); dot(r,r): ConjugateGradient_CPU_MPI_OMP.hpp:107-110)
template <bool X_FIRST, typename TV, typename ApAt>
__device__ __forceinline__ double sweep_xr(TV alpha, uint64_t first, uint64_t stride, uint64_t n, const TV *p, TV *x, TV *r,
                                           uint64_t row0, uint64_t n_loc, ApAt ap_at)
{
    auto x_step = [&](uint64_t i) {
        if (i >= row0 && i < row0 + n_loc) x[i - row0] = alpha * p[i] + x[i - row0];
    };
    double acc = 0.0;
    for (uint64_t i = first; i < n; i += stride) {
        if (X_FIRST) x_step(i);
        const TV ri = -alpha * ap_at(i) + r[i];
        r[i] = ri;
        acc += (double)ri * (double)ri;
        if (!X_FIRST) x_step(i);
    }
    return acc;
}

// beta = rr'/rr and the stop test sqrt(rr'/bb) < rel_error (ConjugateGradient_CPU_MPI_OMP.hpp:110-114: the test comes BEFORE the
// p update).  Every workgroup reaches the same decision from the same bits; thread 0 of the leader workgroup records it.
template <typename TV> struct CgDecision { bool stop; TV beta; };
template <typename TV>
__device__ __forceinline__ CgDecision<TV> cg_decide(CgScalars *sc, int k, double rr, double bb, double rr_new, double rel_error,
                                                    volatile int *host_flags /* pinned host progress word, see post_progress */,
                                                    bool leader_block /* the workgroup whose thread 0 keeps CgScalars */)
{
    const double beta_d = rr_new / rr;
    const bool stop = sqrt(rr_new / bb) < rel_error;
    if (leader_block && threadIdx.x == 0) {
        sc->rr[k & 1] = rr_new;
        sc->beta = beta_d;
        sc->iters = k;
        post_progress(host_flags, k, stop);   // WHICH iteration stopped: the host compares it with the iteration whose
                                              // completion it has awaited (lam_hip_cg_iterate)
        if (stop) sc->stop = 1;               // a workgroup that starts after the flag is up returns at the top: the same outcome
    }
    CgDecision<TV> d;
    d.stop = stop;
    d.beta = (TV)beta_d;
    return d;
}

// p = r + beta p over [first, first + stride, ...) of n elements; store(i, p_i) puts the element where the caller keeps p
template <typename TV, typename Store>
__device__ __forceinline__ void sweep_p(TV beta, uint64_t first, uint64_t stride, uint64_t n, const TV *r, const TV *p, Store store)
{
    for (uint64_t i = first; i < n; i += stride) store(i, r[i] + beta * p[i]);
}

// sliced vectors: the p slice goes to [row0, row0 + n_loc) of every replica in pdst -- plain stores, or with the direct exchange
// (post.n > 0) system-scope (write-through) stores, after which workgroup `block` raises its flag in every peer's mailbox
template <typename TV>
__device__ __forceinline__ void sweep_p_slice(TV beta, uint64_t first, uint64_t stride, uint64_t n_loc, const TV *r, const TV *p_loc,
                                              const PtrList &pdst, uint64_t row0, const MailPost &post, int block)
{
    if (post.n == 0) {
        sweep_p(beta, first, stride, n_loc, r, p_loc, [&](uint64_t i, TV pi) {
            for (int j = 0; j < pdst.n; j++) reinterpret_cast<TV *>(pdst.p[j])[row0 + i] = pi;
        });
        return;
    }
    sweep_p(beta, first, stride, n_loc, r, p_loc, [&](uint64_t i, TV pi) {
        for (int j = 0; j < pdst.n; j++)
            __hip_atomic_store(reinterpret_cast<TV *>(pdst.p[j]) + row0 + i, pi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    });
    // every thread: its slice stores happen-before the workgroup's flag stores (system-scope release fence, then the
    // workgroup barrier, then relaxed flag stores; the reader pairs it with an acquire fence behind its poll)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if ((int)threadIdx.x < post.n && (int)threadIdx.x != post.rank)
        st_sys(&post.mail[threadIdx.x]->pflag[post.rank][block], post.seq);
}

// alpha = rr / p.Ap ; x += alpha p ; r -= alpha Ap ; partials of r.r
template <typename TV>
__global__ void __launch_bounds__(kBlock)
update_xr_kernel(const double *__restrict__ red, int nred, CgScalars *sc, int k,
                 const TV *__restrict__ p_loc, const TV *__restrict__ Ap, TV *__restrict__ x,
                 TV *__restrict__ r, uint64_t n_loc, double *__restrict__ partial, Finalize fin, MailWait mw)
{
    __shared__ double s_red[kWaves];
    if (sc->stop) return;
    if (is_reducer_block(fin)) { reduce_partials(partial, (int)gridDim.x - 1, fin, s_red); return; }
    const double pAp = mw.n > 0 ? mail_sum(mw, s_red) : block_sum_array(red, nred, s_red);
    const CgAlpha<TV> a = cg_alpha<TV>(sc, k, pAp);
    const double acc = sweep_xr<true>(a.alpha, (uint64_t)blockIdx.x * kBlock + threadIdx.x, (uint64_t)compute_blocks(fin) * kBlock, n_loc,
                                p_loc, x, r, 0, n_loc, [&](uint64_t i) { return Ap[i]; });
    double t = block_sum(acc, s_red);
    if (threadIdx.x == 0 && blockIdx.x == 0) { sc->pAp = pAp; sc->alpha = a.alpha_d; }
    publish_partial(t, partial, fin);
}

// rr' = r.r ; beta = rr'/rr ; if sqrt(rr'/bb) < tol: stop (p untouched) else p_slice = r + beta p
template <typename TV>
__global__ void __launch_bounds__(kBlock)
update_p_kernel(const double *__restrict__ red, int nred, CgScalars *sc, int k, double rel_error,
                const TV *__restrict__ r, const TV *__restrict__ p_loc, PtrList pdst, uint64_t row0,
                uint64_t n_loc, volatile int *host_flags /* pinned host progress word, see post_progress */,
                MailWait mw, MailPost post)
{
    __shared__ double s_red[kWaves];
    if (sc->stop) return;
    const double rr_new = mw.n > 0 ? mail_sum(mw, s_red) : block_sum_array(red, nred, s_red);
    const double rr = sc->rr[(k + 1) & 1];
    const double bb = sc->bb;
    const CgDecision<TV> d = cg_decide<TV>(sc, k, rr, bb, rr_new, rel_error, host_flags, blockIdx.x == 0);
    if (d.stop) return;
    sweep_p_slice(d.beta, (uint64_t)blockIdx.x * kBlock + threadIdx.x, (uint64_t)gridDim.x * kBlock, n_loc, r, p_loc, pdst, row0, post,
                  (int)blockIdx.x);
}

// direct exchange: wait until every other rank's update_p workgroups have flagged their p slice for `seq`
__device__ __forceinline__ void wait_p_flags(const Mail *mine, int nranks, int rank, const BlockCounts &nb, unsigned long long seq, int *host_err)
{
    SpinGuard guard;
    for (int q = 0; q < nranks; q++) {
        if (q == rank) continue;
        for (int b = threadIdx.x; b < nb.n[q]; b += kBlock) {
            unsigned long long seen;
            while ((seen = ld_sys(&mine->pflag[q][b])) != seq) {
                if (guard.slow_path()) {
                if (*(volatile int *)host_err != 0) return;
                if (guard.expired()) {
                    host_err[1] = q * 1000 + b; host_err[2] = (int)(unsigned)seq; host_err[3] = (int)(unsigned)seen;
                    host_err[4] = (int)(seq >> 32); host_err[5] = (int)(seen >> 32);
                    *(volatile int *)host_err = 3;
                    return;
                }
                }
                __builtin_amdgcn_s_sleep(4);
            }
        }
    }
    // the peers' slices (stored before their release fences) happen-before everything this thread -- and, through the
    // end of the kernel, the next kernel on this stream -- does from here on
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
}

// ---------------------------------------------------------------------------------------------
// Fused vector step: update_xr_kernel + update_p_kernel in ONE launch (one shard, and the direct exchange).
// What separates the two kernels is a grid-wide dependency -- r.r needs every workgroup's partial --, and that
// is exactly what the reducer workgroup + mailbox machinery already provides inside a launch: the compute
// workgroups publish their partials of r.r, the reducer workgroup turns them into the total -- with the direct
// exchange by way of every rank's mailbox, which it alone polls -- and hands {value, tag} to the launch's other
// workgroups through a broadcast slot in ordinary device memory, which they poll (bounded) at agent scope.  All workgroups of the launch are resident
// together (at most 256 + 2 of them), so nobody waits for a workgroup that cannot start.  Arithmetic, element
// -> thread mapping and reduction order are those of the two kernels: results are bit-identical.
// (The same helpers, that is; the first index of a sweep is cb-based here and the stride is ncompute workgroups.)
// Roles by workgroup index: 0 reducer, [1, ncompute] compute, ncompute + 1 (direct exchange without
// the own-slice GEMV panel only) the WAITER that holds the launch open until the peers' p slices for the next
// GEMV have arrived -- which makes wait_p_kernel unnecessary: 2 launches per iteration.
// ---------------------------------------------------------------------------------------------
template <typename TV>
__global__ void __launch_bounds__(kBlock)
update_fused_kernel(const double *__restrict__ red, int nred, CgScalars *sc, int k, double rel_error,
                    const TV *p_loc, const TV *__restrict__ Ap, TV *__restrict__ x, TV *__restrict__ r, uint64_t n_loc,
                    double *partial, int ncompute, Finalize fin, MailWait mw_pap, MailWait mw_rr, BcastLine *bc /*[2][kBcastLines], local*/,
                    PtrList pdst, uint64_t row0, volatile int *host_flags, MailPost post, const Mail *mine, BlockCounts nb)
{
    __shared__ double s_red[kWaves];
    if (sc->stop) return;
    const unsigned long long seq = mw_rr.seq;
    int *host_err = mw_rr.host_err;
    // workgroup 0 is the reducer (dispatched first: everybody else ends up waiting for it), 1..ncompute compute,
    // ncompute + 1 the waiter
    const int cb = (int)blockIdx.x - 1;
    if (blockIdx.x == 0) {
        // reducer: the ONLY workgroup that polls the (uncached) mailbox; everything it learns goes to the launch's
        // other workgroups through the two local broadcast slots
        const int nl = (int)gridDim.x - 1;                                             // listeners: compute workgroups (+ waiter)
        if (mw_pap.n > 0) bcast_post(bc, nl, mail_sum(mw_pap, s_red), seq);            // direct exchange: p.Ap of all ranks
        const double local = reduce_partials_sum(partial, ncompute, s_red, host_err);  // this shard's r.r
        if (fin.mail) {
            post_total(fin, local);                                                    // ... to every rank's mailbox
            bcast_post(bc + kBcastLines, nl, mail_sum(mw_rr, s_red), seq);             // r.r of all ranks
        } else {
            bcast_post(bc + kBcastLines, nl, local, seq);                              // one shard
        }
        return;
    }
    const double bb = sc->bb;
    if (cb >= ncompute) {                               // waiter
        const double rr_w = bcast_wait(bc + kBcastLines + cb, seq, host_err, s_red);
        if (sqrt(rr_w / bb) < rel_error) return;        // the solve stops here: nobody posts a p slice
        wait_p_flags(mine, post.n, post.rank, nb, post.seq, host_err);
        return;
    }
    // ---- update_xr_kernel's part
    const double pAp = mw_pap.n > 0 ? bcast_wait(bc + cb, seq, host_err, s_red) : block_sum_array(red, nred, s_red);
    const CgAlpha<TV> a = cg_alpha<TV>(sc, k, pAp);
    const uint64_t first = (uint64_t)cb * kBlock + threadIdx.x, stride = (uint64_t)ncompute * kBlock;
    const double acc = sweep_xr<true>(a.alpha, first, stride, n_loc, p_loc, x, r, 0, n_loc, [&](uint64_t i) { return Ap[i]; });
    const double t = block_sum(acc, s_red);
    if (threadIdx.x == 0 && cb == 0) { sc->pAp = pAp; sc->alpha = a.alpha_d; }
    if (threadIdx.x == 0) __hip_atomic_store(partial + cb, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // ---- update_p_kernel's part
    const double rr_new = bcast_wait(bc + kBcastLines + cb, seq, host_err, s_red);
    const CgDecision<TV> d = cg_decide<TV>(sc, k, a.rr, bb, rr_new, rel_error, host_flags, cb == 0);
    if (d.stop) return;
    sweep_p_slice(d.beta, first, stride, n_loc, r, p_loc, pdst, row0, post, cb);
}

__global__ void __launch_bounds__(kBlock)
wait_p_kernel(const Mail *mine, int nranks, int rank, BlockCounts nb, unsigned long long seq, const CgScalars *sc, int *host_err)
{
    if (sc->stop) return;
    wait_p_flags(mine, nranks, rank, nb, seq, host_err);
}

// ---------------------------------------------------------------------------------------------
// "gather-Ap" exchange (rank mode, option exchange = 1): ONE collective per iteration.
// After the GEMV every rank all-gathers [Ap_slice | its partial of p.Ap] (the reference CPU path also
// gathers Ap, ConjugateGradient_CPU_MPI_OMP.hpp:505) and then updates FULL-length r and p
// redundantly -- O(N) work per rank, like the reference's full-length axpby (:476) -- so r.r needs
// no collective at all.  Layout of the gathered buffer: rank q's record starts at q*stride_bytes: room for the LONGEST
// slice (base + n % P values of TV; rank q < P-1 fills the first `base`), then -- at stride_bytes - 8 -- one double.
// ---------------------------------------------------------------------------------------------
template <typename TV>
__global__ void __launch_bounds__(kBlock)
cg_init_full_kernel(TV *__restrict__ r_full /* holds b on entry */, TV *__restrict__ p_full, TV *__restrict__ x,
                    uint64_t n, uint64_t n_loc, double *__restrict__ partial)
{
    __shared__ double s_red[kWaves];
    double acc = 0.0;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        const TV bi = r_full[i];
        p_full[i] = bi;
        if (i < n_loc) x[i] = (TV)0;
        acc += (double)bi * (double)bi;
    }
    double t = block_sum(acc, s_red);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

// write this rank's p.Ap partial (sum of the GEMV workgroup partials) behind its Ap slice
__global__ void __launch_bounds__(kBlock)
finalize_tail_kernel(const double *__restrict__ src, int n, char *record, uint64_t tail_offset_bytes, const CgScalars *sc)
{
    __shared__ double s_red[kWaves];
    if (sc != nullptr && sc->stop) return;
    double t = block_sum_array(src, n, s_red);
    if (threadIdx.x == 0) *reinterpret_cast<double *>(record + tail_offset_bytes) = t;
}

// One element of the gathered Ap.  Gather-Ap exchange: shard i / base holds it in its record.  Symmetric product on several
// shards (sum_records): every shard's record is a full-length CONTRIBUTION to A p; they are added in shard order (the same
// order on every shard, so all shards keep identical r and p).
template <typename TV>
__device__ __forceinline__ TV gathered_ap(const char *__restrict__ gathered, uint64_t stride_bytes, uint64_t base, int nranks,
                                          int sum_records, uint64_t i)
{
    if (!sum_records) {
        // the reference's partition: `base` rows per shard, the remainder on the LAST one (its record is the long one)
        uint64_t q = i / base;
        if (q >= (uint64_t)nranks) q = (uint64_t)nranks - 1;
        return reinterpret_cast<const TV *>(gathered + q * stride_bytes)[i - q * base];
    }
    TV v = reinterpret_cast<const TV *>(gathered)[i];
    for (int q = 1; q < nranks; q++) v += reinterpret_cast<const TV *>(gathered + (uint64_t)q * stride_bytes)[i];
    return v;
}

// p.Ap out of the gathered records: the sum of their tails in rank order, the same on every rank
__device__ __forceinline__ double gathered_pap(const char *__restrict__ gathered, uint64_t stride_bytes, int nranks)
{
    double pAp = 0.0;
    for (int q = 0; q < nranks; q++)
        pAp += *reinterpret_cast<const double *>(gathered + (uint64_t)q * stride_bytes + stride_bytes - 8);
    return pAp;
}

template <typename TV>
__global__ void __launch_bounds__(kBlock)
update_xr_full_kernel(const char *__restrict__ gathered, uint64_t stride_bytes, uint64_t base, int nranks,
                      CgScalars *sc, int k, const TV *__restrict__ p_full, TV *__restrict__ x, TV *__restrict__ r_full,
                      uint64_t n, uint64_t row0, uint64_t n_loc, double *__restrict__ partial, int sum_records)
{
    __shared__ double s_red[kWaves];
    if (sc->stop) return;
    const double pAp = gathered_pap(gathered, stride_bytes, nranks);
    const CgAlpha<TV> a = cg_alpha<TV>(sc, k, pAp);
    const double acc = sweep_xr<false>(a.alpha, (uint64_t)blockIdx.x * kBlock + threadIdx.x, (uint64_t)gridDim.x * kBlock, n, p_full, x, r_full,
                                row0, n_loc, [&](uint64_t i) { return gathered_ap<TV>(gathered, stride_bytes, base, nranks, sum_records, i); });
    double t = block_sum(acc, s_red);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = t;
        if (blockIdx.x == 0) { sc->pAp = pAp; sc->alpha = a.alpha_d; }
    }
}

template <typename TV>
__global__ void __launch_bounds__(kBlock)
update_p_full_kernel(const double *__restrict__ red, int nred, CgScalars *sc, int k, double rel_error,
                     const TV *__restrict__ r_full, TV *__restrict__ p_full, uint64_t n, volatile int *host_flags)
{
    __shared__ double s_red[kWaves];
    if (sc->stop) return;
    const double rr_new = block_sum_array(red, nred, s_red);
    const double rr = sc->rr[(k + 1) & 1];
    const double bb = sc->bb;
    const CgDecision<TV> d = cg_decide<TV>(sc, k, rr, bb, rr_new, rel_error, host_flags, blockIdx.x == 0);
    if (d.stop) return;
    sweep_p(d.beta, (uint64_t)blockIdx.x * kBlock + threadIdx.x, (uint64_t)gridDim.x * kBlock, n, r_full, (const TV *)p_full,
            [&](uint64_t i, TV pi) { p_full[i] = pi; });
}

// update_xr_full_kernel + update_p_full_kernel in ONE launch (round 4): what separates them is the grid-wide r.r, which the
// reducer workgroup resolves inside the launch exactly as in update_fused_kernel -- compute workgroups publish their partials in
// self-flagging slots, workgroup 0 sums them in the order of block_sum_array and hands {value, tag} to every compute workgroup on
// a line of its own.  Same element -> thread mapping, same partial grouping and reduction order as the two kernels: bit-identical
// (the number of compute workgroups equals the two-kernel grid).  The gather-Ap iteration is then GEMV + one collective or join +
// this launch: two launches for every shard count, like the single-shard iteration.  All workgroups must be resident at once.
template <typename TV>
__global__ void __launch_bounds__(kBlock)
update_full_fused_kernel(const char *__restrict__ gathered, uint64_t stride_bytes, uint64_t base, int nranks, CgScalars *sc, int k,
                         double rel_error, TV *p_full, TV *__restrict__ x, TV *r_full, uint64_t n, uint64_t row0, uint64_t n_loc,
                         double *partial, int ncompute, BcastLine *bc, unsigned long long seq, int *host_err, volatile int *host_flags,
                         int sum_records)
{
    __shared__ double s_red[kWaves];
    if (sc->stop) return;
    if (blockIdx.x == 0) {                              // reducer: r.r of the full vector, to every compute workgroup
        const double total = reduce_partials_sum(partial, ncompute, s_red, host_err);
        bcast_post(bc, ncompute, total, seq);
        return;
    }
    const int cb = (int)blockIdx.x - 1;
    const double pAp = gathered_pap(gathered, stride_bytes, nranks);
    const CgAlpha<TV> a = cg_alpha<TV>(sc, k, pAp);
    const double bb = sc->bb;
    const uint64_t first = (uint64_t)cb * kBlock + threadIdx.x, stride = (uint64_t)ncompute * kBlock;
    const double acc = sweep_xr<false>(a.alpha, first, stride, n, (const TV *)p_full, x, r_full, row0, n_loc,
                                [&](uint64_t i) { return gathered_ap<TV>(gathered, stride_bytes, base, nranks, sum_records, i); });
    const double t = block_sum(acc, s_red);
    if (threadIdx.x == 0) {
        __hip_atomic_store(partial + cb, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cb == 0) { sc->pAp = pAp; sc->alpha = a.alpha_d; }
    }
    const double rr_new = bcast_wait(bc + cb, seq, host_err, s_red);
    const CgDecision<TV> d = cg_decide<TV>(sc, k, a.rr, bb, rr_new, rel_error, host_flags, cb == 0);
    if (d.stop) return;
    sweep_p(d.beta, first, stride, n, (const TV *)r_full, (const TV *)p_full, [&](uint64_t i, TV pi) { p_full[i] = pi; });
}

// standalone BLAS-1 pieces (lam_hip_dot / lam_hip_axpby and the residual check)
template <typename TV>
__global__ void __launch_bounds__(kBlock)
dot_partial_kernel(const TV *__restrict__ x, const TV *__restrict__ y, uint64_t n, double *__restrict__ partial)
{
    __shared__ double s_red[kWaves];
    double acc = 0.0;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock)
        acc += (double)x[i] * (double)y[i];
    double t = block_sum(acc, s_red);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

template <typename TV>
__global__ void __launch_bounds__(kBlock)
axpby_kernel(TV alpha, const TV *__restrict__ x, TV beta, TV *__restrict__ y, uint64_t n)
{
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock)
        y[i] = alpha * x[i] + beta * y[i];
}

// partial of sum (b - y)^2 over a slice (true-residual check)
template <typename TV>
__global__ void __launch_bounds__(kBlock)
resid_partial_kernel(const TV *__restrict__ b, const TV *__restrict__ y, uint64_t n, double *__restrict__ partial)
{
    __shared__ double s_red[kWaves];
    double acc = 0.0;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        const double d = (double)b[i] - (double)y[i];
        acc += d * d;
    }
    double t = block_sum(acc, s_red);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

// ---------------------------------------------------------------------------------------------
// generators (one-off, not on the hot path)
// ---------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ uint64_t splitmix64(uint64_t z)
{
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__host__ __device__ __forceinline__ double u01(uint64_t h) { return (double)(h >> 11) * (1.0 / 9007199254740992.0); }

template <typename TA>
__device__ __forceinline__ TA to_storage(double v);
template <> __device__ __forceinline__ double to_storage<double>(double v) { return v; }
template <> __device__ __forceinline__ float to_storage<float>(double v) { return (float)v; }
template <> __device__ __forceinline__ __hip_bfloat16 to_storage<__hip_bfloat16>(double v) { return __float2bfloat16((float)v); }

// rows [row0,row0+nrows) of dense tridiag(1,2,1) by GLOBAL row index
template <typename TA>
__global__ void __launch_bounds__(kBlock)
gen_tridiag_kernel(TA *__restrict__ A, uint64_t lda, uint64_t row0, uint64_t nrows, uint64_t n)
{
    const uint64_t total = nrows * n;
    for (uint64_t idx = (uint64_t)blockIdx.x * kBlock + threadIdx.x; idx < total; idx += (uint64_t)gridDim.x * kBlock) {
        const uint64_t i = idx / n + row0, j = idx % n;
        double v = 0.0;
        if (i == j) v = 2.0;
        else if (i + 1 == j || i == j + 1) v = 1.0;
        A[(i - row0) * lda + j] = to_storage<TA>(v);
    }
}

template <typename TA>
__global__ void __launch_bounds__(kBlock)
gen_random_spd_kernel(TA *__restrict__ A, uint64_t lda, uint64_t row0, uint64_t nrows, uint64_t n, uint64_t seed, double cond)
{
    const uint64_t total = nrows * n;
    const double inv_n = 1.0 / (double)n;
    for (uint64_t idx = (uint64_t)blockIdx.x * kBlock + threadIdx.x; idx < total; idx += (uint64_t)gridDim.x * kBlock) {
        const uint64_t i = idx / n + row0, j = idx % n;
        double v;
        if (i == j) {
            v = 1.0 + (cond - 1.0) * u01(splitmix64(seed ^ splitmix64(i * 2 + 1)));
        } else {
            const uint64_t lo = i < j ? i : j, hi = i < j ? j : i;
            v = (2.0 * u01(splitmix64(seed + splitmix64(lo * n + hi))) - 1.0) * inv_n;
        }
        A[(i - row0) * lda + j] = to_storage<TA>(v);
    }
}

// ---- dense SPD matrix with a PRESCRIBED SPECTRUM: A = H_k ... H_1 diag(eig) H_1 ... H_k, H_j = I - tau_j v_j v_j^T
// (the reference generator's law A = Q diag(exp(3.5 u)) Q^T, challenge/main/random_spd_system.cpp:66-97, with Q a product of
// Householder reflectors instead of an O(N^3) Gram-Schmidt: exact spectrum up to rounding, exactly symmetric, O(k N^2)).
// Step 0: the diagonal matrix; then per reflector  w = A v (the GEMV kernel),  u = w - (tau v.w / 2) v (host),
// A <- A - (tau v) u^T - u (tau v)^T  by the kernel below.
template <typename TA, typename TV>
__global__ void __launch_bounds__(kBlock)
gen_diag_kernel(TA *__restrict__ A, uint64_t lda, uint64_t row0, uint64_t nrows, uint64_t n, const TV *__restrict__ eig /* full length */)
{
    const uint64_t total = nrows * n;
    for (uint64_t idx = (uint64_t)blockIdx.x * kBlock + threadIdx.x; idx < total; idx += (uint64_t)gridDim.x * kBlock) {
        const uint64_t i = idx / n + row0, j = idx % n;
        A[(i - row0) * lda + j] = i == j ? to_storage<TA>((double)eig[i]) : to_storage<TA>(0.0);
    }
}

// A[i][j] -= tv[i] u[j] + u[i] tv[j]  with the two products rounded SEPARATELY and then added (no FMA contraction): element
// (j, i) adds the same two products in the other order, and a + b == b + a, so a symmetric A stays symmetric bit for bit.
template <typename TA, typename TV>
__global__ void __launch_bounds__(kBlock)
rank2_update_kernel(TA *__restrict__ A, uint64_t lda, uint64_t row0, uint64_t nrows, uint64_t n, const TV *__restrict__ tv, const TV *__restrict__ u)
{
#pragma clang fp contract(off)      // plain operators under contract(off): nothing here may be fused into an fma -- fma(tv_i, u_j,
                                    // u_i tv_j) rounds one product and not the other, and (i, j) != (j, i) in the last bit.  (The
                                    // __dmul_rn / __dadd_rn intrinsics do NOT help: they are inline functions of the HIP headers
                                    // with the default contract(fast), and came out as v_fmac_f64.)
    const uint64_t total = nrows * n;
    for (uint64_t idx = (uint64_t)blockIdx.x * kBlock + threadIdx.x; idx < total; idx += (uint64_t)gridDim.x * kBlock) {
        const uint64_t i = idx / n + row0, j = idx % n;
        const TV p1 = tv[i] * u[j];
        const TV p2 = u[i] * tv[j];
        const TV s12 = p1 + p2;
        TA *e = A + (i - row0) * lda + j;
        *e = to_storage<TA>((double)((TV)*e - s12));
    }
}

template <typename TV>
__global__ void __launch_bounds__(kBlock)
gen_rhs_kernel(TV *__restrict__ b, uint64_t row0, uint64_t n_loc, int random, uint64_t seed, double value)
{
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n_loc; i += (uint64_t)gridDim.x * kBlock)
        b[i] = random ? (TV)(2.0 * u01(splitmix64(seed ^ splitmix64(0xB5ull + row0 + i))) - 1.0) : (TV)value;
}

// rows of `cols` elements between a dense staging buffer (pitch = cols) and the matrix (pitch = lda), either direction;
// TD <- TS conversion by to_storage (float -> bf16 rounds, bf16 -> float widens, same type copies)
template <typename TS, typename TD>
__global__ void __launch_bounds__(kBlock)
pitch_copy_kernel(const TS *__restrict__ src, uint64_t src_pitch, TD *__restrict__ dst, uint64_t dst_pitch, uint64_t nrows, uint64_t cols)
{
    const uint64_t total = nrows * cols;
    for (uint64_t idx = (uint64_t)blockIdx.x * kBlock + threadIdx.x; idx < total; idx += (uint64_t)gridDim.x * kBlock) {
        const uint64_t r = idx / cols, j = idx % cols;
        if constexpr (std::is_same<TS, TD>::value) dst[r * dst_pitch + j] = src[r * src_pitch + j];
        else if constexpr (std::is_same<TD, __hip_bfloat16>::value) dst[r * dst_pitch + j] = __float2bfloat16((float)src[r * src_pitch + j]);
        else dst[r * dst_pitch + j] = (TD)__bfloat162float(src[r * src_pitch + j]);
    }
}


// ---------------------------------------------------------------------------------------------
// Several right-hand sides on one matrix (lam_hip_solve_many, lam_multi.h): K independent CG recurrences advanced together,
// ONE pass over the matrix per iteration.  Three launches per iteration: multi_gemv_kernel, multi_xr_kernel, multi_p_kernel.
//
// Layout: every batched vector (B, X, R, P, AP) is INTERLEAVED, element i of column j at [i * K + j]: the K values of p that one
// matrix column meets are K * sizeof(TV) contiguous bytes -- 16-byte LDS reads in the product, coalesced K-wide records in the
// vector step.  K is the instantiation (1, 2, 4, 8); nrhs <= K columns are live, the rest are zero padding columns that are born
// stopped (MultiScalars::col[j].stop = 1 for j >= nrhs) and never touched.
// Columns never mix: every quantity of column j is computed from column j alone, in an order that does not depend on j or on
// what the other columns hold.
//
// The vector kernels carry a compile-time PC: false is the plain recurrence, true the Jacobi-preconditioned one of
// lam_hip_solve_many_pc, M = diag(A) (no reference counterpart: the reference is un-preconditioned).  The delta:
//   x = 0, r = b, p = z = dinv o b, rz = r.z ;  alpha = rz / p.Ap ; x += alpha p ; r -= alpha Ap ; rr' = r.r ; rz' = r.(dinv o r) ;
//   stop test on sqrt(rr'/bb) as in the plain recurrence ; beta = rz'/rz ; p = dinv o r + beta p
// z is never stored: dinv (one vector of n elements shared by the K columns, read once per row) is applied where z is needed, and
// r.z gets a second set of partials, reduced right behind r.r's by the same building blocks.  Everything else is the one set of
// statements, so on a matrix whose diagonal is a constant power of two every quantity is the plain recurrence's times an exact power
// of two and x, the iteration counts and rel_err agree bit for bit.  With PC = false, dinv and the r.z partials are null and never
// dereferenced.
//
// Shifted systems (lam_hip_set_shifts_many): column j solves (A + s_j I) x_j = b_j.  (A + s_j I) p_j = A p_j + s_j p_j, so the stream
// of A is shared and the shift is one fma per (row, column) in the product's epilogue, compile-time SHIFT; AP then carries the shift
// and the plain recurrence needs nothing else.  Under PC the preconditioner is M_j = diag(A) + s_j I: dinv becomes K-wide,
// dinv[i * K + j], behind the compile-time DK of the three vector kernels (built and scanned by shifted_dinv_kernel).  SHIFT = false
// and DK = false are the kernels of before, statement for statement.
// ---------------------------------------------------------------------------------------------
constexpr int kMaxRhs = 8;
constexpr int kMultiPadRows = 16;     // zero rows kept behind row n of a batched vector (>= the 8 elements of a bf16-sized vector)
struct MultiScalars {
    CgScalars col[kMaxRhs];   // one recurrence per column, with CgScalars' meaning; a stopped column's entry is frozen (under the
                              // preconditioner alpha and beta are the preconditioned ones)
    int all_stop;             // every live column has met its stop test: the batch's later launches return at once
    int pad;
};
// the batch's device block: the MultiScalars prefix is what the product kernel reads and the host copies back
struct BatchScalars : MultiScalars {
    double rz[kMaxRhs][2];    // PC only: r_j.z_j, ping-pong like CgScalars::rr: iteration k reads [(k+1)&1], writes [k&1]
};

// p tile of the batched product: K * TILE elements of TV in LDS, 32 KiB whatever K (the single-vector fp64 kernel's figure), and at
// least one workgroup super-step (WAVES * 64 lanes * one 16-byte vector)
template <typename TA, typename TV, int K, int WAVES>
constexpr int multi_tile()
{
    constexpr int super = WAVES * 64 * MatVec<TA>::N;
    constexpr int fit = (int)(32768 / (K * sizeof(TV)));
    return fit >= 4096 ? 4096 : (fit / super >= 1 ? fit / super * super : super);
}

template <typename TA, typename TV>
struct MultiGemvArgs {
    const TA *A;
    const TV *p;               // [ncols + padding][K], zeros behind row n
    TV *y;                     // [n][K]
    double *partial;           // [K][nblocks]: column j's p_j.(A p_j) partial of workgroup b at [j * nblocks + b]; may be null
    const MultiScalars *sc;    // may be null; sc->all_stop: nothing to do
    uint64_t nrows, ncols, lda;
    TV shift[kMaxRhs];         // SHIFT only: s_j of Y_j = (A + s_j I) P_j (lam_hip_set_shifts_many); last, so the others keep their offsets
};

// Y = A P for K vectors at once: the streaming body of gemv_coop_kernel (WAVES waves share R rows, 16-byte non-temporal loads of
// the matrix, rotated tile start, zero-filled ragged tile + kZeroVec16 for the lanes past its end, fixed-order reductions) with K
// accumulators per row: each 16-byte piece of a row is multiplied with the K values of p of each of its columns while it is in
// registers.
// SHIFT (lam_hip_set_shifts_many): column j is the product of A + s_j I.  The stream is the same stream; the epilogue's one thread per
// (row, column), which holds p_j[row] for the fused p_j.(A p_j), adds s_j p_j[row] with one fma in front of the store of y and of the
// dot product, so both are the shifted matrix's.  SHIFT = false never reads a.shift.
template <typename TA, typename TV, int K, int R, int WAVES, bool NT, bool SHIFT = false>
__global__ void __launch_bounds__(WAVES * 64)
multi_gemv_kernel(MultiGemvArgs<TA, TV> a)
{
    using MV = MatVec<TA>;
    using avec_t = typename MV::vec_t;
    constexpr int VEC = MV::N;
    constexpr int TILE = multi_tile<TA, TV, K, WAVES>();
    constexpr int SUPER = 64 * VEC * WAVES;             // columns one workgroup super-step covers
    static_assert(TILE % SUPER == 0, "tile must be a whole number of workgroup super-steps");
    constexpr int WSTEPS = TILE / SUPER;
    constexpr int UNROLL = WSTEPS < 4 ? WSTEPS : 4;
    constexpr int NTHREADS = WAVES * 64;
    constexpr int PV = 16 / sizeof(TV);
    typedef TV pvec_t __attribute__((ext_vector_type(PV)));
    constexpr int NPV = VEC * K / PV;                   // 16-byte LDS reads per lane and step
    static_assert((VEC * K) % PV == 0, "a lane's p values are whole 16-byte vectors");

    static_assert(TILE * K >= R * K * WAVES + 2 * R * K, "the reduction scratch fits the p tile it re-uses");
    __shared__ __attribute__((aligned(16))) TV s_p[TILE * K];
    // the wave partials and the rows' dot products re-use the tile once the stream is done (the tile alone is 32 KiB: five
    // workgroups per CU by LDS)
    TV (*s_part)[WAVES] = reinterpret_cast<TV (*)[WAVES]>(s_p);
    double *s_dot = reinterpret_cast<double *>(s_p + R * K * WAVES);

    if (a.sc != nullptr && a.sc->all_stop) return;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const uint64_t row_first = (uint64_t)blockIdx.x * R;
    const uint32_t woff = (uint32_t)wave * (64 * VEC) + (uint32_t)lane * VEC;

    const TA *rowp[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        uint64_t row = row_first + r;
        if (row >= a.nrows) row = a.nrows - 1;
        rowp[r] = a.A + row * a.lda + woff;
    }
    TV acc[R][K];
#pragma unroll
    for (int r = 0; r < R; r++)
#pragma unroll
        for (int j = 0; j < K; j++) acc[r][j] = (TV)0;

    const uint32_t ntiles = (uint32_t)((a.ncols + TILE - 1) / TILE);
    uint32_t tt = blockIdx.x % ntiles;
    for (uint32_t t = 0; t < ntiles; t++) {
        const uint64_t c0 = (uint64_t)tt * TILE;
        const uint32_t cols = (uint32_t)((a.ncols - c0 < (uint64_t)TILE) ? (a.ncols - c0) : (uint64_t)TILE);
        __syncthreads();
        {
            // cols is a multiple of VEC, so cols * K elements are whole 16-byte vectors; the tile starts 16-byte aligned
            const pvec_t *src = reinterpret_cast<const pvec_t *>(a.p + c0 * K);
            pvec_t *dst = reinterpret_cast<pvec_t *>(s_p);
            const uint32_t nv = cols * K / PV;
            for (uint32_t i = tid; i < nv; i += NTHREADS) dst[i] = src[i];
            // ragged tile: zeros up to the next whole super-step (what the lanes past the end multiply with)
            const uint32_t padded = (cols + SUPER - 1) / SUPER * SUPER;
            pvec_t z;
#pragma unroll
            for (int q = 0; q < PV; q++) z[q] = (TV)0;
            for (uint32_t i = nv + tid; i < padded * K / PV; i += NTHREADS) dst[i] = z;
        }
        __syncthreads();
        const int nsteps = cols == (uint32_t)TILE ? WSTEPS : (int)((cols + SUPER - 1) / SUPER);
        const bool full = cols == (uint32_t)TILE;
#pragma unroll UNROLL
        for (int s = 0; s < nsteps; s++) {
            const uint32_t col = (uint32_t)s * SUPER + woff;
            avec_t av[R];
#pragma unroll
            for (int r = 0; r < R; r++) {
                // lanes past the end of a ragged tile load 16 zero bytes instead of matrix elements and meet the zeros the
                // staging put behind `cols`: they add exactly +0, whatever the row holds there
                const avec_t *src = (full || col < cols) ? reinterpret_cast<const avec_t *>(rowp[r] + c0 + (uint64_t)s * SUPER)
                                                         : reinterpret_cast<const avec_t *>(kZeroVec16);
                av[r] = NT ? __builtin_nontemporal_load(src) : *src;
            }
            pvec_t pq[NPV];
            const pvec_t *lp = reinterpret_cast<const pvec_t *>(s_p + (size_t)col * K);
#pragma unroll
            for (int q = 0; q < NPV; q++) pq[q] = lp[q];
#pragma unroll
            for (int i = 0; i < VEC; i++)
#pragma unroll
                for (int j = 0; j < K; j++) {
                    const TV pij = pq[(i * K + j) / PV][(i * K + j) % PV];
#pragma unroll
                    for (int r = 0; r < R; r++) acc[r][j] = fma_tv((TV)MV::get(av[r], i), pij, acc[r][j]);
                }
        }
        tt = (tt + 1 == ntiles) ? 0 : tt + 1;
    }

    __syncthreads();                                    // the last tile has been consumed: s_p becomes the reduction scratch
#pragma unroll
    for (int r = 0; r < R; r++)
#pragma unroll
        for (int j = 0; j < K; j++) {
            TV s = wave_sum(acc[r][j]);
            if (lane == 0) s_part[r * K + j][wave] = s;
        }
    __syncthreads();
    if (tid < R * K) {
        const int r = tid / K, j = tid % K;
        const uint64_t row = row_first + r;
        double d = 0.0;
        if (row < a.nrows) {
            TV s = s_part[tid][0];
#pragma unroll
            for (int w = 1; w < WAVES; w++) s += s_part[tid][w];
            const TV pj = a.p[row * K + j];
            if constexpr (SHIFT) s = fma_tv(a.shift[j], pj, s);
            a.y[row * K + j] = s;
            d = (double)s * (double)pj;
        }
        s_dot[tid] = d;
    }
    if (a.partial != nullptr) {
        __syncthreads();
        if (tid < K) {
            double t = s_dot[tid];
#pragma unroll
            for (int r = 1; r < R; r++) t += s_dot[r * K + tid];
            a.partial[(size_t)tid * gridDim.x + blockIdx.x] = t;
        }
    }
}

// The body of multi_gemv_kernel<double, double, K, 4, 4, NT, SHIFT> on the packed image (option "packed_many", K = 1, 2, 4): the same
// grid, the same rotated order of the batch tiles, p staging target, lane-to-column mapping and fma sequence per accumulator (the +0
// terms of a ragged tile included), the same wave_sum, s_part order, SHIFT fma, store of y and partials -- the result is bit for bit
// the plain kernel's.  What differs is where an element comes from (gemv_packed_kernel's decode: one LDS read of the (row, unit)'s
// list per element and a select).
// A unit of the image (one row x 4096 columns) spans K batch tiles, and thread (wave, lane) reads lane `lane` of its wave groups
// wave and wave + 4 (pack_many_pos).  The batch tiles of the rotated order are therefore walked as VISITS of a unit: the consecutive
// batch tiles [sub_lo, sub_hi) that share it.  At the start of a visit the thread loads its 2 x 56 bytes of each of the 4 rows, the
// 4 headers and the first 64 values of the 4 lists, all in front of the visit's first barrier, and keeps elements, header and list
// for every batch tile of the visit; the rotation can start inside a unit (K = 2, 4), which then gets a first and a last visit, and
// a partial visit skips the low-word vectors none of its batch tiles reads.  A batch tile, as in the plain kernel: barrier, the p
// tile (eight 16-byte loads a thread back to back, one wait, eight LDS writes; the lists behind the first barrier of a visit),
// barrier, the FMAs.
template <int K, bool NT, bool SHIFT>
__global__ void __launch_bounds__(256)
multi_gemv_packed_kernel(MultiGemvArgs<double, double> a, PackedMat pk)
{
    constexpr int R = 4, WAVES = 4, NTHREADS = WAVES * 64, SUPER = 128 * WAVES;
    constexpr int TILE = multi_tile<double, double, K, WAVES>();
    constexpr int SPT = TILE / SUPER;                   // steps of a batch tile
    static_assert(K == 1 || K == 2 || K == 4, "a unit of the image is a whole number of batch tiles");
    static_assert(TILE * K == (int)kPackTile && SPT * K == (int)kPackManySteps, "K batch tiles are one unit");
    static_assert(R == WAVES, "wave r stages the first values of row r's list");
    typedef double pvec_t __attribute__((ext_vector_type(2)));
    typedef const __attribute__((address_space(1))) pvec_t *gptr_t;
    constexpr int NPL = TILE * K / 2 / NTHREADS;        // 16-byte vectors of the p tile a thread stages

    __shared__ __attribute__((aligned(16))) double s_p[TILE * K];
    __shared__ double s_exc[R][kPackCap + 1];
    double (*s_part)[WAVES] = reinterpret_cast<double (*)[WAVES]>(s_p);
    double *s_dot = s_p + R * K * WAVES;

    if (a.sc != nullptr && a.sc->all_stop) return;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint64_t row_first = (uint64_t)blockIdx.x * R;
    const uint32_t woff = (uint32_t)wave * 128u + (uint32_t)lane * 2u;

    const uint32_t nunits = pk.ntiles;
    uint64_t unit0[R];                                  // the row's first unit
#pragma unroll
    for (int r = 0; r < R; r++) {
        uint64_t row = row_first + r;
        if (row >= a.nrows) row = a.nrows - 1;
        unit0[r] = row * nunits;
    }
    uint64_t unit0_mine = unit0[0];                     // of the row whose list this wave stages
#pragma unroll
    for (int r = 1; r < R; r++) if (wave == r) unit0_mine = unit0[r];
    double acc[R][K];
#pragma unroll
    for (int r = 0; r < R; r++)
#pragma unroll
        for (int j = 0; j < K; j++) acc[r][j] = 0.0;
    if (tid < R) s_exc[tid][kPackZeroIdx] = 0.0;        // the reserved index; never overwritten (visible behind the first barrier)

    uint32_t perlane = 0;                               // zero, but not to the compiler (gemv_packed_kernel: the headers stay per lane)
    asm volatile("" : "+v"(perlane));

    const uint32_t ntiles = (uint32_t)((a.ncols + TILE - 1) / TILE);
    const uint32_t tt0 = blockIdx.x % ntiles;
    const uint32_t sub0 = tt0 % (uint32_t)K;
    const uint32_t nvisits = nunits + (sub0 != 0 ? 1u : 0u);
    uint32_t u = tt0 / (uint32_t)K;
    for (uint32_t v = 0; v < nvisits; v++) {
        const uint32_t left = ntiles - u * (uint32_t)K;             // batch tiles of unit u (the last unit may hold fewer than K)
        const uint32_t sub_lo = v == 0 ? sub0 : 0u;
        const uint32_t sub_hi = v == nunits ? sub0 : (left < (uint32_t)K ? left : (uint32_t)K);
        // low words 0..3 of a lane and group are pairs 0 and 1 (the first half of the unit's batch tiles), 4..7 pairs 2 and 3
        const bool need0 = K == 1 || sub_lo < (uint32_t)K / 2, need1 = K == 1 || sub_hi > (uint32_t)K / 2;
        pack_u4 lo0[R][2], lo1[R][2], mid[R][2];
        pack_u2 hi[R][2];
#pragma unroll
        for (int r = 0; r < R; r++)
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const unsigned char *g = pk.data + ((unit0[r] + u) * kPackGroups + (uint64_t)(wave + 4 * h)) * kPackGroupBytes;
                const pack_u4 *q0 = reinterpret_cast<const pack_u4 *>(g + pack_off_lo(lane, 0));
                const pack_u4 *q1 = reinterpret_cast<const pack_u4 *>(g + pack_off_lo(lane, 4));
                const pack_u4 *qm = reinterpret_cast<const pack_u4 *>(g + pack_off_mid(lane, 0));
                const pack_u2 *qh = reinterpret_cast<const pack_u2 *>(g + pack_off_hi(lane, 0));
                lo0[r][h] = 0u;
                lo1[r][h] = 0u;
                if (need0) lo0[r][h] = NT ? __builtin_nontemporal_load(q0) : *q0;
                if (need1) lo1[r][h] = NT ? __builtin_nontemporal_load(q1) : *q1;
                mid[r][h] = NT ? __builtin_nontemporal_load(qm) : *qm;
                hi[r][h] = NT ? __builtin_nontemporal_load(qh) : *qh;
            }
        uint32_t head[R];
#pragma unroll
        for (int r = 0; r < R; r++) head[r] = pk.hdr[unit0[r] + u + perlane];
        const double first = pk.exc[(unit0_mine + u) * kPackCap + lane];
        uint32_t shift[R];
#pragma unroll
        for (int r = 0; r < R; r++) shift[r] = 0u;
#pragma unroll
        for (int sub = 0; sub < K; sub++) {
            if ((uint32_t)sub < sub_lo || (uint32_t)sub >= sub_hi) continue;
            const uint64_t c0 = (uint64_t)(u * (uint32_t)K + (uint32_t)sub) * TILE;
            const uint32_t cols = (uint32_t)((a.ncols - c0 < (uint64_t)TILE) ? (a.ncols - c0) : (uint64_t)TILE);
            __syncthreads();
            {
                // cols is even, so cols * K elements are whole 16-byte vectors; behind them zeros, as the plain kernel stages them
                // (it stops at the next whole step; the rest of the tile is not read)
                const double *src = a.p + c0 * K;
                pvec_t *dst = reinterpret_cast<pvec_t *>(s_p);
                const uint32_t nv = cols * K / 2;
                pvec_t pv[NPL];
#pragma unroll
                for (int k = 0; k < NPL; k++) {
                    const uint32_t i = (uint32_t)tid + (uint32_t)k * NTHREADS;
                    pv[k] = *(i < nv ? (gptr_t)(src + 2 * (size_t)i) : (gptr_t)kZeroVec16);
                }
#pragma unroll
                for (int k = 0; k < NPL; k++) dst[tid + k * NTHREADS] = pv[k];
            }
            if ((uint32_t)sub == sub_lo) {
                s_exc[wave][lane] = first;
#pragma unroll
                for (int r = 0; r < R; r++) {
                    shift[r] = pack_exp_shift(pack_header_base(head[r]));
                    const uint32_t cnt = min(pack_header_count(head[r]), kPackCap);
                    const double *e = pk.exc + (unit0[r] + u) * kPackCap;
                    for (uint32_t i = kPackFirst + tid; i < cnt; i += NTHREADS) s_exc[r][i] = e[i];     // a long list: one more round trip
                }
            }
            __syncthreads();
            const int nsteps = (int)((cols + SUPER - 1) / SUPER);
#pragma unroll
            for (int s = 0; s < SPT; s++) {
                if (s < nsteps) {
                    uint32_t unit_rel, group, pair;
                    pack_many_pos((uint32_t)K, (uint32_t)sub, (uint32_t)s, 0u, &unit_rel, &group, &pair);      // unit_rel == 0
                    const int h = (int)(group >> 2);
                    pvec_t pq[K];
                    const pvec_t *lp = reinterpret_cast<const pvec_t *>(s_p + (size_t)((uint32_t)s * SUPER + woff) * K);
#pragma unroll
                    for (int q = 0; q < K; q++) pq[q] = lp[q];
#pragma unroll
                    for (int i = 0; i < 2; i++) {
                        const int e = 2 * (int)pair + i;
                        double av[R];
#pragma unroll
                        for (int r = 0; r < R; r++) {
                            const uint32_t l = e < 4 ? lo0[r][h][e & 3] : lo1[r][h][e & 3];
                            const uint32_t w = ((hi[r][h][e >> 2] >> (8 * (e & 3))) & 0xffu) << 16 | ((mid[r][h][e >> 1] >> (16 * (e & 1))) & 0xffffu);
                            const bool x = pack_is_exception(w);
                            const double ev = s_exc[r][x ? min(l, kPackZeroIdx) : kPackZeroIdx];
                            av[r] = x ? ev : __longlong_as_double((long long)pack_decode(l, w, shift[r]));
                        }
#pragma unroll
                        for (int j = 0; j < K; j++) {
                            const double pij = pq[(i * K + j) / 2][(i * K + j) % 2];
#pragma unroll
                            for (int r = 0; r < R; r++) acc[r][j] = fma_tv(av[r], pij, acc[r][j]);
                        }
                    }
                }
            }
        }
        u = (u + 1 == nunits) ? 0 : u + 1;
    }

    __syncthreads();                                    // the last tile has been consumed: s_p becomes the reduction scratch
#pragma unroll
    for (int r = 0; r < R; r++)
#pragma unroll
        for (int j = 0; j < K; j++) {
            double s = wave_sum(acc[r][j]);
            if (lane == 0) s_part[r * K + j][wave] = s;
        }
    __syncthreads();
    if (tid < R * K) {
        const int r = tid / K, j = tid % K;
        const uint64_t row = row_first + r;
        double d = 0.0;
        if (row < a.nrows) {
            double s = s_part[tid][0];
#pragma unroll
            for (int w = 1; w < WAVES; w++) s += s_part[tid][w];
            const double pj = a.p[row * K + j];
            if constexpr (SHIFT) s = fma_tv(a.shift[j], pj, s);
            a.y[row * K + j] = s;
            d = s * pj;
        }
        s_dot[tid] = d;
    }
    if (a.partial != nullptr) {
        __syncthreads();
        if (tid < K) {
            double t = s_dot[tid];
#pragma unroll
            for (int r = 1; r < R; r++) t += s_dot[r * K + tid];
            a.partial[(size_t)tid * gridDim.x + blockIdx.x] = t;
        }
    }
}

// Symmetric batched product (option "symmetric_many", lam_multi.h multi_launch_gemv): Y = A P for K = 1, 2, 4 interleaved columns
// reading every pair {A_ij, A_ji} once -- the two passes of the single symmetric product ("Symmetric product" above: one shard, the
// upper triangle, the plan of symv_plan unchanged) with K of everything a lane keeps per column of P: its p values, its column
// partials, its 8 row partials.  The first pass is a statement-for-statement copy of symv_task_kernel with a K loop around those (the
// matrix loads, the tasks, the lean / masked / ragged loops and the use rule are the single path's); the second pass is the single
// path's own body, symv_reduce_body.  The order of every sum of column j is the single path's: column j of Y is bit for bit what
// symv_task_kernel + symv_reduce_kernel give for that vector alone, whatever K is and whatever the other columns hold
// (tests/test_gpu_symmetric_many.py), and tests/test_gpu_symmetric_bits.py pins both against a recorded build.
// Partials are K-wide records: rowpart[(rp + row) * K + j], colpart[(task * SS + column) * K + j] (64-bit offsets: the products with K
// pass 2^32).  The LDS row buffer is K-wide too (fp64 K = 4: 32 KiB); the idle dynamic LDS behind it keeps the launch at three
// workgroups per CU as in the single path (symv_lds_pad<T, K>).
constexpr int kSymvManyMaxK = 4;       // K = 8 stays on the general product (staging- and barrier-bound, not byte-bound: DESIGN §8)
template <typename T> struct ShiftArg { T s[kSymvManyMaxK]; };       // SHIFT only: s_j of Y_j = (A + s_j I) P_j, by value
template <typename TA, typename T, int K>
__global__ void __launch_bounds__(kBlock)
symv_many_task_kernel(const TA *__restrict__ A, const T *__restrict__ p, const SymvTask *__restrict__ tasks, T *__restrict__ rowpart,
                      T *__restrict__ colpart, uint64_t lda, uint64_t ncols_vec, uint64_t n, const MultiScalars *sc)
{
    using MV = MatVec<TA>;
    using vec_t = typename MV::vec_t;
    constexpr int VEC = MV::N, SS = kBlock * VEC;
    typedef T tvec_t __attribute__((ext_vector_type(VEC)));          // 16 bytes of a K-wide record run: flat element f = i * K + j
    static_assert(sizeof(T) == sizeof(TA), "fp64 / fp32 storage: a 16-byte vector holds VEC elements of either");
    __shared__ T s_rows[kWaves][kSymvRowsLds * K];
    if (sc != nullptr && sc->all_stop) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    SymvTask t = tasks[blockIdx.x];
    const bool interior = (t.nrows & kSymvInterior) != 0, full = (t.nrows & kSymvFull) != 0;
    t.nrows &= ~kSymvFlags;
    const uint64_t c0 = (uint64_t)t.strip * SS, c = c0 + (uint64_t)tid * VEC;       // this lane's columns: c + i
    const uint64_t grow0 = t.row0;
    const bool live = c < ncols_vec;
    T pc[K][VEC], cacc[K][VEC];
    {
        tvec_t in[K];
#pragma unroll
        for (int q = 0; q < K; q++) {
#pragma unroll
            for (int i = 0; i < VEC; i++) in[q][i] = (T)0;
            if (live) in[q] = *reinterpret_cast<const tvec_t *>(p + c * K + (uint64_t)q * VEC);
        }
#pragma unroll
        for (int j = 0; j < K; j++)
#pragma unroll
            for (int i = 0; i < VEC; i++) { pc[j][i] = in[(i * K + j) / VEC][(i * K + j) % VEC]; cacc[j][i] = (T)0; }
    }
    // the row partials of the last (up to) 256 rows, ending at row `end` of the task: out of LDS into rowpart, K-wide records
    auto flush_rows = [&](uint32_t end) {
        const uint32_t beg = (end - 1) & ~(uint32_t)(kSymvRowsLds - 1);
        const uint32_t stop = end < t.nrows ? end : t.nrows;
        __syncthreads();
        for (uint32_t e = beg * K + tid; e < stop * K; e += kBlock) {
            const uint32_t q = e - beg * K;
            __builtin_nontemporal_store((s_rows[0][q] + s_rows[1][q]) + (s_rows[2][q] + s_rows[3][q]), rowpart + (uint64_t)t.rp * K + e);
        }
        __syncthreads();
    };
    // one 8-row step's tail: per column the wave's row totals, parked in LDS
    auto park = [&](const T (&racc)[K][8], uint32_t b) {
#pragma unroll
        for (int j = 0; j < K; j++) {
            const T tot = wave_sum8(racc[j]);
            if ((lane & 7) == 0) s_rows[wave][((b & (kSymvRowsLds - 1)) + (lane >> 3)) * K + j] = tot;
        }
        if (((b + 8) & (kSymvRowsLds - 1)) == 0 || b + 8 >= t.nrows) flush_rows(b + 8);
    };
    auto lean_loop = [&](auto masked_tag) {
        constexpr bool MASKED = decltype(masked_tag)::value;
        const TA *rows = A + (uint64_t)t.row0 * lda + c0;          // uniform
        const T *prow = p + grow0 * K;
        vec_t a0[4], a1[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            a0[k] = __builtin_nontemporal_load(reinterpret_cast<const vec_t *>(rows + (uint64_t)k * lda) + tid);
            a1[k] = __builtin_nontemporal_load(reinterpret_cast<const vec_t *>(rows + (uint64_t)(k + 4) * lda) + tid);
        }
        for (uint32_t b = 0; b < t.nrows; b += 8, prow += 8 * K) {
            rows += 8 * lda;
            const bool more = b + 8 < t.nrows;
            T racc[K][8];
#pragma unroll
            for (int k = 0; k < 4; k++)
#pragma unroll
                for (int j = 0; j < K; j++) {
                    const T pr = prow[k * K + j];
                    T r = (T)0;
#pragma unroll
                    for (int i = 0; i < VEC; i++) {
                        bool rs = true, cs = true;
                        if (MASKED) symv_use<false>(c + i, grow0 + b + k, n, &rs, &cs);
                        if (rs) r = fma_tv((T)MV::get(a0[k], i), pc[j][i], r);
                        if (cs) cacc[j][i] = fma_tv((T)MV::get(a0[k], i), pr, cacc[j][i]);
                    }
                    racc[j][k] = r;
                }
            if (more) {
#pragma unroll
                for (int k = 0; k < 4; k++) a0[k] = __builtin_nontemporal_load(reinterpret_cast<const vec_t *>(rows + (uint64_t)k * lda) + tid);
            }
#pragma unroll
            for (int k = 0; k < 4; k++)
#pragma unroll
                for (int j = 0; j < K; j++) {
                    const T pr = prow[(4 + k) * K + j];
                    T r = (T)0;
#pragma unroll
                    for (int i = 0; i < VEC; i++) {
                        bool rs = true, cs = true;
                        if (MASKED) symv_use<false>(c + i, grow0 + b + 4 + k, n, &rs, &cs);
                        if (rs) r = fma_tv((T)MV::get(a1[k], i), pc[j][i], r);
                        if (cs) cacc[j][i] = fma_tv((T)MV::get(a1[k], i), pr, cacc[j][i]);
                    }
                    racc[j][4 + k] = r;
                }
            if (more) {
#pragma unroll
                for (int k = 0; k < 4; k++)
                    a1[k] = __builtin_nontemporal_load(reinterpret_cast<const vec_t *>(rows + (uint64_t)(k + 4) * lda) + tid);
            }
            park(racc, b);
        }
    };
    if (interior) lean_loop(std::false_type());
    else if (full) lean_loop(std::true_type());
    else {
        // ragged strips and row runs: every load and every product tested
        const TA *Arow = A + (uint64_t)t.row0 * lda + c;
        for (uint32_t b = 0; b < t.nrows; b += 8) {
            vec_t a[8];
#pragma unroll
            for (int k = 0; k < 8; k++) {
#pragma unroll
                for (int i = 0; i < VEC; i++) a[k][i] = 0;
                // a vector whose columns all lie left of the diagonal is not read at all
                if (live && b + k < t.nrows && c + VEC > grow0 + b + k)
                    a[k] = __builtin_nontemporal_load(reinterpret_cast<const vec_t *>(Arow + (uint64_t)(b + k) * lda));
            }
            T racc[K][8];
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const uint64_t grow = grow0 + b + k;
#pragma unroll
                for (int j = 0; j < K; j++) {
                    const T pr = b + k < t.nrows ? p[grow * K + j] : (T)0;
                    T r = (T)0;
#pragma unroll
                    for (int i = 0; i < VEC; i++) {
                        bool rs, cs;
                        symv_use<false>(c + i, grow, n, &rs, &cs);
                        if (rs) r = fma_tv((T)MV::get(a[k], i), pc[j][i], r);
                        if (cs) cacc[j][i] = fma_tv((T)MV::get(a[k], i), pr, cacc[j][i]);
                    }
                    racc[j][k] = r;
                }
            }
            park(racc, b);
        }
    }
    if (live) {
        T *dst = colpart + ((uint64_t)blockIdx.x * SS + (uint64_t)tid * VEC) * K;
#pragma unroll
        for (int q = 0; q < K; q++) {
            tvec_t out;
#pragma unroll
            for (int f = 0; f < VEC; f++) out[f] = cacc[(q * VEC + f) % K][(q * VEC + f) / K];
            __builtin_nontemporal_store(out, reinterpret_cast<tvec_t *>(dst) + q);
        }
    }
}

// Second pass of the batch: every row is the one shard's, y[row * K + j] is stored plainly, and the workgroup's p_j.(A p_j) partial goes
// to partial[j * gridDim.x + block] (gridDim.x = ceil(n / 32): what the batch's consumers are told).
template <typename T, int SS, int K, bool SHIFT>
__global__ void __launch_bounds__(kBlock)
symv_many_reduce_kernel(const T *__restrict__ rowpart, const T *__restrict__ colpart, const uint32_t *__restrict__ index, SymvIndex ix,
                        const T *__restrict__ p, T *__restrict__ y, double *__restrict__ partial, uint64_t n, ShiftArg<T> shift,
                        const MultiScalars *sc)
{
    __shared__ double s_dot[K][kSymvReduceRows];
    if (sc != nullptr && sc->all_stop) return;
    symv_reduce_body<T, SS, K, SHIFT>(
        rowpart, colpart, index, ix, p, n, 0, n, shift.s, s_dot, partial != nullptr, [&](uint64_t e, T t) { y[e] = t; },
        [&](int j, double d) { partial[(size_t)j * gridDim.x + blockIdx.x] = d; });
}

// X = 0, R = B, P = B (PC: dinv o B); per-workgroup partials of b_j.b_j (PC: and of r_j.z_j = b_j.(dinv o b_j)), both at
// [j * gridDim.x + block].
// GUESS (lam_hip_solve_many_x0): the guess x0 is in P and AX holds A x0 (one batched product in front of this launch).  X = x0,
// R = B - AX rounded to the vector dtype, P = R (PC: dinv o R); b_j.b_j still goes to `partial`, r_j.r_j to partial_rr and r_j.z_j
// to partial_rz.  r.r and r.z are accumulated by the statements, and so in the order, that take b.b and b.(dinv o b) without a
// guess: with x0 = 0 (AX = 0, R = B exactly) their sums are those sums, bit for bit.
// DK (PC only, the shifted batch): dinv is K-wide, dinv[i * K + j] = 1 / (A_ii + s_j), instead of one value per row.
template <typename TV, int K, bool PC, bool GUESS, bool DK = false>
__global__ void __launch_bounds__(kBlock)
multi_init_kernel(const TV *__restrict__ B, TV *__restrict__ X, TV *__restrict__ R, TV *__restrict__ P, uint64_t n,
                  double *__restrict__ partial, const TV *__restrict__ dinv, double *__restrict__ partial_rz,
                  const TV *__restrict__ AX, double *__restrict__ partial_rr)
{
    __shared__ double s_red[kWaves];
    double acc[K];
    [[maybe_unused]] double accz[K];
    [[maybe_unused]] double accb[K];
#pragma unroll
    for (int j = 0; j < K; j++) {
        acc[j] = 0.0;
        if constexpr (PC) accz[j] = 0.0;
        if constexpr (GUESS) accb[j] = 0.0;
    }
    // the kMultiPadRows rows behind the end of P are what the product's last 16-byte vector of a row meets past column n (against
    // zeros of the row padding): zero in THIS instantiation's layout, whatever another K left there
    if (blockIdx.x == 0 && threadIdx.x < kMultiPadRows * K) P[n * K + threadIdx.x] = (TV)0;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        [[maybe_unused]] TV di;
        if constexpr (PC && !DK) di = dinv[i];
#pragma unroll
        for (int j = 0; j < K; j++) {
            uint64_t e = i * K + j;
            // DK: the K-wide row of dinv would be K more live values next to the rows of B, AX and P, and cost waves at K = 8.  The
            // column's index is made opaque and the columns are kept apart, so the row is met one column at a time and the K-wide
            // instantiations keep the occupancy of their shared-dinv counterparts (one launch per solve: its latency is no matter)
            // This leans on the compiler's scheduling: re-check DESIGN §11's table with -Rpass-analysis=kernel-resource-usage when the
            // compiler changes (the worst case is a one-shot launch at lower occupancy, not a wrong result)
            if constexpr (PC && DK) asm volatile("" : "+v"(e));
            if constexpr (PC && DK) di = dinv[e];
            TV bi = B[e];                        // from here on r0's element: b's without a guess
            if constexpr (GUESS) {
                accb[j] += (double)bi * (double)bi;
                X[e] = P[e];
                bi = bi - AX[e];
            } else {
                X[e] = (TV)0;
            }
            R[e] = bi;
            if constexpr (PC) {
                const TV zi = di * bi;
                P[e] = zi;
                accz[j] += (double)bi * (double)zi;
            } else {
                P[e] = bi;
            }
            acc[j] += (double)bi * (double)bi;
            if constexpr (PC && DK) __builtin_amdgcn_sched_barrier(0);
        }
    }
#pragma unroll
    for (int j = 0; j < K; j++) {
        const double t = block_sum(acc[j], s_red);
        [[maybe_unused]] double tz;
        if constexpr (PC) tz = block_sum(accz[j], s_red);
        [[maybe_unused]] double tb;
        if constexpr (GUESS) tb = block_sum(accb[j], s_red);
        if (threadIdx.x == 0) {
            if constexpr (GUESS) {
                partial[(size_t)j * gridDim.x + blockIdx.x] = tb;
                partial_rr[(size_t)j * gridDim.x + blockIdx.x] = t;
            } else {
                partial[(size_t)j * gridDim.x + blockIdx.x] = t;
            }
            if constexpr (PC) partial_rz[(size_t)j * gridDim.x + blockIdx.x] = tz;
        }
    }
}

// per column: bb = rr[0] = sum of its partials (PC: rz[0] = the sum of its r.z partials), iters = 0; live columns start running,
// padding columns are born stopped.
// GUESS: rr[0] is the sum of the r0.r0 partials (red_rr), and the stop test is taken at k = 0: a live column whose guess already
// meets sqrt(rr0/bb) < rel_error is born stopped -- 0 iterations, converged, x = x0 as it came -- instead of dividing 0 by 0 in
// its first alpha.  If that is every live column the batch is over before its first iteration: all_stop is raised, the iteration's
// launches return at once and never post, so the progress word itself says "stopped before iteration 1" (iteration 0, stop mark
// 1: the smallest mark the lag rule acts on, at the host's first look).
template <int K, bool PC, bool GUESS>
__global__ void __launch_bounds__(kBlock)
multi_init_scalars_kernel(const double *__restrict__ red, int nred, int nrhs, BatchScalars *sc, volatile int *host_flags,
                          const double *__restrict__ red_rz, const double *__restrict__ red_rr, double rel_error)
{
    __shared__ double s_red[kWaves];
    [[maybe_unused]] bool all = true;
    for (int j = 0; j < kMaxRhs; j++) {
        const double t = j < K ? block_sum_array(red + (size_t)j * nred, nred, s_red) : 0.0;
        [[maybe_unused]] double tz;
        if constexpr (PC) tz = j < K ? block_sum_array(red_rz + (size_t)j * nred, nred, s_red) : 0.0;
        double rr0 = t;
        if constexpr (GUESS) rr0 = j < K ? block_sum_array(red_rr + (size_t)j * nred, nred, s_red) : 0.0;
        bool born_stopped = j >= nrhs;
        if constexpr (GUESS) {
            born_stopped = born_stopped || sqrt(rr0 / t) < rel_error;
            all = all && born_stopped;
        }
        if (threadIdx.x == 0) {
            CgScalars &c = sc->col[j];
            c.bb = t; c.rr[0] = rr0; c.rr[1] = 0.0; c.pAp = 0.0; c.alpha = 0.0; c.beta = 0.0; c.iters = 0;
            c.stop = born_stopped ? 1 : 0;
            if constexpr (PC) { sc->rz[j][0] = tz; sc->rz[j][1] = 0.0; }
        }
    }
    if (threadIdx.x == 0) {
        sc->pad = 0;
        if constexpr (GUESS) {
            sc->all_stop = all ? 1 : 0;
            post_progress_word(host_flags, 0, all ? 1 : 0);
        } else {
            sc->all_stop = 0;
            post_progress(host_flags, 0, false);
        }
    }
}

// lam_hip_true_residual_many: with AX = A X from one batched product, per column r = b - A x rounded to the vector dtype;
// per-workgroup fp64 partials of r_j.r_j and of b_j.b_j, both at [j * gridDim.x + block]
template <typename TV, int K>
__global__ void __launch_bounds__(kBlock)
multi_residual_kernel(const TV *__restrict__ B, const TV *__restrict__ AX, uint64_t n, double *__restrict__ partial_rr,
                      double *__restrict__ partial_bb)
{
    __shared__ double s_red[kWaves];
    double acc[K], accb[K];
#pragma unroll
    for (int j = 0; j < K; j++) acc[j] = accb[j] = 0.0;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
#pragma unroll
        for (int j = 0; j < K; j++) {
            const TV bi = B[i * K + j];
            const TV ri = bi - AX[i * K + j];
            acc[j] += (double)ri * (double)ri;
            accb[j] += (double)bi * (double)bi;
        }
    }
#pragma unroll
    for (int j = 0; j < K; j++) {
        const double t = block_sum(acc[j], s_red);
        const double tb = block_sum(accb[j], s_red);
        if (threadIdx.x == 0) {
            partial_rr[(size_t)j * gridDim.x + blockIdx.x] = t;
            partial_bb[(size_t)j * gridDim.x + blockIdx.x] = tb;
        }
    }
}
// out[j] = sqrt(r_j.r_j / b_j.b_j) for the K columns of the instantiation (plain IEEE: b_j = 0 gives 0/0); one workgroup
template <int K>
__global__ void __launch_bounds__(kBlock)
multi_residual_scalars_kernel(const double *__restrict__ red_rr, const double *__restrict__ red_bb, int nred, double *__restrict__ out)
{
    __shared__ double s_red[kWaves];
    for (int j = 0; j < K; j++) {
        const double t = block_sum_array(red_rr + (size_t)j * nred, nred, s_red);
        const double tb = block_sum_array(red_bb + (size_t)j * nred, nred, s_red);
        if (threadIdx.x == 0) out[j] = sqrt(t / tb);
    }
}

// per live, running column j: alpha_j = rr_j / p_j.Ap_j (PC: rz_j / p_j.Ap_j) ; x_j += alpha_j p_j ; r_j -= alpha_j Ap_j ; partials
// of r_j.r_j (PC: and of r_j.(dinv o r_j))
// (update_xr_kernel's statements, column by column; a stopped column is not read and not written)
template <typename TV, int K, bool PC, bool DK = false>
__global__ void __launch_bounds__(kBlock)
multi_xr_kernel(const double *__restrict__ red, int nred, BatchScalars *sc, int k, const TV *__restrict__ P, const TV *__restrict__ AP,
                TV *__restrict__ X, TV *__restrict__ R, uint64_t n, double *__restrict__ partial, const TV *__restrict__ dinv,
                double *__restrict__ partial_rz)
{
    __shared__ double s_red[kWaves];
    if (sc->all_stop) return;
    bool run[K];
    double alpha_d[K], pAp[K], acc[K];
    [[maybe_unused]] double accz[K];
    TV alpha[K];
#pragma unroll
    for (int j = 0; j < K; j++) {
        run[j] = sc->col[j].stop == 0;
        pAp[j] = block_sum_array(red + (size_t)j * nred, nred, s_red);
        if constexpr (PC) alpha_d[j] = sc->rz[j][(k + 1) & 1] / pAp[j];
        else alpha_d[j] = sc->col[j].rr[(k + 1) & 1] / pAp[j];
        alpha[j] = (TV)alpha_d[j];
        acc[j] = 0.0;
        if constexpr (PC) accz[j] = 0.0;
    }
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        [[maybe_unused]] TV di;
        if constexpr (PC && !DK) di = dinv[i];
#pragma unroll
        for (int j = 0; j < K; j++) {
            if (!run[j]) continue;
            const uint64_t e = i * K + j;
            if constexpr (PC && DK) di = dinv[e];
            X[e] = alpha[j] * P[e] + X[e];
            const TV ri = -alpha[j] * AP[e] + R[e];
            R[e] = ri;
            acc[j] += (double)ri * (double)ri;
            if constexpr (PC) {
                const TV zi = di * ri;
                accz[j] += (double)ri * (double)zi;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < K; j++) {
        const double t = block_sum(acc[j], s_red);
        [[maybe_unused]] double tz;
        if constexpr (PC) tz = block_sum(accz[j], s_red);
        if (threadIdx.x == 0) {
            partial[(size_t)j * gridDim.x + blockIdx.x] = t;
            if constexpr (PC) partial_rz[(size_t)j * gridDim.x + blockIdx.x] = tz;
            if (blockIdx.x == 0 && run[j]) { sc->col[j].pAp = pAp[j]; sc->col[j].alpha = alpha_d[j]; }
        }
    }
}

// per running column j: rr' = r_j.r_j (PC: rz' = r_j.z_j) ; beta = rr'/rr (PC: rz'/rz) ; if sqrt(rr'/bb_j) < tol the column stops
// (p_j untouched, its scalars are final) else p_j = r_j + beta p_j (PC: dinv o r_j + beta p_j).  The progress word reports the
// iteration, and "stopped" once EVERY live column has stopped.
// Workgroup 0 is the only writer of the scalars; a workgroup that starts after it has raised a column's stop flag sees that column
// as stopped and leaves p_j alone, which is what it would have decided itself from the same bits (update_p_kernel's argument).
// The PC p statement is an explicit fma(beta, p, z) with z = dinv o r rounded on its own: the plain r + beta p contracts to
// fma(beta, p, r), and z must not be the operand that is fused (fma(dinv, r, beta p) rounds differently).
template <typename TV, int K, bool PC, bool DK = false>
__global__ void __launch_bounds__(kBlock)
multi_p_kernel(const double *__restrict__ red, int nred, BatchScalars *sc, int k, double rel_error, const TV *__restrict__ R,
               TV *__restrict__ P, uint64_t n, volatile int *host_flags, const TV *__restrict__ dinv,
               const double *__restrict__ red_rz)
{
    __shared__ double s_red[kWaves];
    if (sc->all_stop) return;
    bool upd[K];
    TV beta[K];
    bool all = true;
#pragma unroll
    for (int j = 0; j < K; j++) {
        const bool run = sc->col[j].stop == 0;
        const double rr_new = block_sum_array(red + (size_t)j * nred, nred, s_red);
        [[maybe_unused]] double rz_new;
        if constexpr (PC) rz_new = block_sum_array(red_rz + (size_t)j * nred, nred, s_red);
        double rho;                              // what beta divides by: the previous r.r (PC: r.z)
        if constexpr (PC) rho = sc->rz[j][(k + 1) & 1];
        else rho = sc->col[j].rr[(k + 1) & 1];
        const double bb = sc->col[j].bb;
        double beta_d;
        if constexpr (PC) beta_d = rz_new / rho;
        else beta_d = rr_new / rho;
        const bool stop = sqrt(rr_new / bb) < rel_error;
        upd[j] = run && !stop;
        beta[j] = (TV)beta_d;
        all = all && !upd[j];
        if (run && blockIdx.x == 0 && threadIdx.x == 0) {
            CgScalars &c = sc->col[j];
            c.rr[k & 1] = rr_new;
            if constexpr (PC) sc->rz[j][k & 1] = rz_new;
            c.beta = beta_d;
            c.iters = k;
        }
    }
    // a workgroup that saw a flag workgroup 0 raised in THIS launch may count a column as stopped that workgroup 0 counted as
    // stopping: `all` is the same either way, and only workgroup 0's value is used
    if (blockIdx.x == 0) {
        __syncthreads();
        if (threadIdx.x == 0) {
#pragma unroll
            for (int j = 0; j < K; j++)
                if (!upd[j]) sc->col[j].stop = 1;
            if (all) sc->all_stop = 1;
            post_progress(host_flags, k, all);
        }
    }
    if (all) return;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        [[maybe_unused]] TV di;
        if constexpr (PC && !DK) di = dinv[i];
#pragma unroll
        for (int j = 0; j < K; j++) {
            if (!upd[j]) continue;
            const uint64_t e = i * K + j;
            if constexpr (PC && DK) di = dinv[e];
            if constexpr (PC) {
                const TV zi = di * R[e];
                P[e] = fma_tv(beta[j], P[e], zi);
            } else {
                P[e] = R[e] + beta[j] * P[e];
            }
        }
    }
}

// [n][K] interleaved <-> K column vectors of n (device-side transposes of the host interface's layout)
template <typename TV, int K>
__global__ void __launch_bounds__(kBlock)
multi_interleave_kernel(const TV *__restrict__ cols, int ncols, TV *__restrict__ inter, uint64_t n)
{
    if (blockIdx.x == 0 && threadIdx.x < kMultiPadRows * K) inter[n * K + threadIdx.x] = (TV)0;      // see multi_init_kernel
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock)
#pragma unroll
        for (int j = 0; j < K; j++) inter[i * K + j] = j < ncols ? cols[(uint64_t)j * n + i] : (TV)0;
}
template <typename TV, int K>
__global__ void __launch_bounds__(kBlock)
multi_deinterleave_kernel(const TV *__restrict__ inter, int ncols, TV *__restrict__ cols, uint64_t n)
{
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock)
#pragma unroll
        for (int j = 0; j < K; j++)
            if (j < ncols) cols[(uint64_t)j * n + i] = inter[i * K + j];
}

// ---------------------------------------------------------------------------------------------
// Batched MINRES (lam_hip_solve_many_minres, lam_multi.h): K independent Paige-Saunders recurrences on (A + s_j I) x_j = b_j, shifts
// of either sign, advanced together.  Three launches per iteration: multi_gemv_kernel on V (u = (A + s I) v, partials of v.u),
// minres_lanczos_kernel (alpha = v.u ; u -= alpha v + beta v_old ; partials of u.u) and minres_update_kernel (the rotation's
// scalars, w, x, the stop test, v_old = v, v = u / beta').  The recurrence is stated in include/lam_hip.h.
// Vectors: V is the batch's P (the product's input: zero behind row n), U its AP, v_old its R, X its X; W and W_OLD are MINRES' own.
// Scalars: the MultiScalars prefix (what the product kernel reads and the host knows) with col[j].bb = b.b, .alpha = the last v.u,
// .beta = the last beta', .iters, .stop; behind it the rotation's state in a ring of two, iteration k reading slot (k + 1) & 1 and
// workgroup 0 writing slot k & 1, so no workgroup of a launch reads what that launch writes (CgScalars::rr's scheme).
// Who decides: every workgroup of minres_update_kernel recomputes the column's scalars and its stop decision from bits nobody writes
// in that launch; workgroup 0 alone stores them.  A column that stops at k still takes iteration k's w and x update, so "does this
// column run" cannot be col[j].stop, which a workgroup that starts late would find raised: frozen_at[j] is the first iteration in
// which the column does nothing (0: live; k + 1 for a stop at k; 1 for a padding column), one word, and the late workgroup reads
// "ran at k" either way -- multi_p_kernel's argument with mshift_step_kernel's word.  For the same reason minres_update_kernel does
// not return on all_stop, which its own workgroup 0 raises while the stopping iteration's update is still owed: it returns when no
// column runs at k by frozen_at.  The product and minres_lanczos_kernel keep the all_stop guard: neither launch writes it.
// The coefficients that multiply vectors (alpha, beta, eps_old, delta, 1 / gamma, phi, 1 / beta', 1 / beta1) are formed in fp64 and
// rounded to the vector dtype once per column and iteration; every vector statement is an explicit fma_tv chain, so which operand is
// fused is the source's choice and not the compiler's.
// ---------------------------------------------------------------------------------------------
struct MinresRot {                // one ring slot
    double beta, cs, sn, dbar, eps, phibar;
};
struct MinresScalars : MultiScalars {
    double beta1[kMaxRhs];        // sqrt(b.b)
    MinresRot rot[kMaxRhs][2];    // after iteration k at [k & 1]; a stopped column's final state is at [iters & 1]
    double rel_err[kMaxRhs];      // phibar / beta1 of the last completed iteration (the start: beta1 / beta1)
    int frozen_at[kMaxRhs];       // 0: live; else the first iteration in which the column does nothing
};

// x = v_old = w = w_old = 0 ; per-workgroup partials of b_j.b_j at [j * gridDim.x + block] ; V's rows behind row n zero in this K's
// layout (see multi_init_kernel)
template <typename TV, int K>
__global__ void __launch_bounds__(kBlock)
minres_init_kernel(const TV *__restrict__ B, TV *__restrict__ X, TV *__restrict__ VOLD, TV *__restrict__ W, TV *__restrict__ WOLD,
                   TV *__restrict__ V, uint64_t n, double *__restrict__ partial)
{
    __shared__ double s_red[kWaves];
    double acc[K];
#pragma unroll
    for (int j = 0; j < K; j++) acc[j] = 0.0;
    if (blockIdx.x == 0 && threadIdx.x < kMultiPadRows * K) V[n * K + threadIdx.x] = (TV)0;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
#pragma unroll
        for (int j = 0; j < K; j++) {
            const uint64_t e = i * K + j;
            const TV bi = B[e];
            X[e] = (TV)0; VOLD[e] = (TV)0; W[e] = (TV)0; WOLD[e] = (TV)0;
            acc[j] += (double)bi * (double)bi;
        }
    }
#pragma unroll
    for (int j = 0; j < K; j++) {
        const double t = block_sum(acc[j], s_red);
        if (threadIdx.x == 0) partial[(size_t)j * gridDim.x + blockIdx.x] = t;
    }
}

// per column: bb, beta1 = sqrt(bb), the rotation's start (beta = 0, cs = -1, sn = 0, dbar = 0, eps = 0, phibar = beta1) in slot 0,
// iters = 0; live columns start running, padding columns are born stopped.  One workgroup.
template <int K>
__global__ void __launch_bounds__(kBlock)
minres_init_scalars_kernel(const double *__restrict__ red, int nred, int nrhs, MinresScalars *sc, volatile int *host_flags)
{
    __shared__ double s_red[kWaves];
    for (int j = 0; j < kMaxRhs; j++) {
        const double t = j < K ? block_sum_array(red + (size_t)j * nred, nred, s_red) : 0.0;
        if (threadIdx.x == 0) {
            const double beta1 = sqrt(t);
            CgScalars &c = sc->col[j];
            c.bb = t; c.rr[0] = 0.0; c.rr[1] = 0.0; c.pAp = 0.0; c.alpha = 0.0; c.beta = 0.0; c.iters = 0;
            c.stop = j < nrhs ? 0 : 1;
            sc->beta1[j] = beta1;
            MinresRot r0;
            r0.beta = 0.0; r0.cs = -1.0; r0.sn = 0.0; r0.dbar = 0.0; r0.eps = 0.0; r0.phibar = beta1;
            sc->rot[j][0] = r0;
            sc->rot[j][1] = r0;
            sc->rel_err[j] = beta1 / beta1;
            sc->frozen_at[j] = j < nrhs ? 0 : 1;
        }
    }
    if (threadIdx.x == 0) {
        sc->pad = 0;
        sc->all_stop = 0;
        post_progress(host_flags, 0, false);
    }
}

// v_j = b_j * (1 / beta1_j) for the live columns, 0 for the padding columns (the product multiplies them like any other)
template <typename TV, int K>
__global__ void __launch_bounds__(kBlock)
minres_start_kernel(const TV *__restrict__ B, TV *__restrict__ V, uint64_t n, const MinresScalars *sc)
{
    TV ib[K];
    bool live[K];
#pragma unroll
    for (int j = 0; j < K; j++) {
        live[j] = sc->frozen_at[j] == 0;
        ib[j] = (TV)(1.0 / sc->beta1[j]);
    }
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
#pragma unroll
        for (int j = 0; j < K; j++) {
            const uint64_t e = i * K + j;
            V[e] = live[j] ? B[e] * ib[j] : (TV)0;
        }
    }
}

// vector launch 1, per running column j: alpha = v_j.u_j from the product's partials ; u_j = (u_j - alpha v_j) - beta v_old_j ;
// partials of u_j.u_j.  No workgroup writes what another reads: col[j].alpha is for the next launch.
template <typename TV, int K>
__global__ void __launch_bounds__(kBlock)
minres_lanczos_kernel(const double *__restrict__ red, int nred, MinresScalars *sc, int k, const TV *__restrict__ V,
                      const TV *__restrict__ VOLD, TV *__restrict__ U, uint64_t n, double *__restrict__ partial)
{
    __shared__ double s_red[kWaves];
    if (sc->all_stop) return;
    bool run[K];
    double alpha_d[K], acc[K];
    TV nalpha[K], nbeta[K];
#pragma unroll
    for (int j = 0; j < K; j++) {
        run[j] = sc->col[j].stop == 0;
        alpha_d[j] = run[j] ? block_sum_array(red + (size_t)j * nred, nred, s_red) : 0.0;
        nalpha[j] = -(TV)alpha_d[j];
        nbeta[j] = -(TV)sc->rot[j][(k + 1) & 1].beta;
        acc[j] = 0.0;
    }
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
#pragma unroll
        for (int j = 0; j < K; j++) {
            if (!run[j]) continue;
            const uint64_t e = i * K + j;
            const TV ui = fma_tv(nbeta[j], VOLD[e], fma_tv(nalpha[j], V[e], U[e]));
            U[e] = ui;
            acc[j] += (double)ui * (double)ui;
        }
    }
#pragma unroll
    for (int j = 0; j < K; j++) {
        const double t = block_sum(acc[j], s_red);
        if (threadIdx.x == 0) {
            partial[(size_t)j * gridDim.x + blockIdx.x] = t;
            if (blockIdx.x == 0 && run[j]) { sc->col[j].pAp = alpha_d[j]; sc->col[j].alpha = alpha_d[j]; }
        }
    }
}

// vector launch 2, per running column j: beta' = sqrt(u_j.u_j), the rotation, w_j and x_j ; rel_err = phibar / beta1 ; below
// rel_error the column stops (v_j untouched, its scalars final), else v_old_j = v_j, v_j = u_j * (1 / beta').  The progress word
// reports the iteration, and "stopped" once EVERY live column has stopped.
template <typename TV, int K>
__global__ void __launch_bounds__(kBlock)
minres_update_kernel(const double *__restrict__ red, int nred, MinresScalars *sc, int k, double rel_error, const TV *__restrict__ U,
                     TV *__restrict__ V, TV *__restrict__ VOLD, TV *__restrict__ W, TV *__restrict__ WOLD, TV *__restrict__ X,
                     uint64_t n, volatile int *host_flags)
{
    __shared__ double s_red[kWaves];
    // NOT `if (sc->all_stop) return`: workgroup 0 raises all_stop in the launch in which the last live column stops, and that
    // iteration still owes its w and x update -- a workgroup (or one wave of one) that started behind that store would skip its rows.
    // The launch is over only if no column runs at k, which frozen_at says the same way before and after workgroup 0's store: the
    // launches the lag rule enqueues past the batch's stop find k >= frozen_at in every column and return here, before they post.
    bool run[K], adv[K];
    bool any = false;
#pragma unroll
    for (int j = 0; j < K; j++) {
        const int fz = sc->frozen_at[j];
        run[j] = fz == 0 || k < fz;
        any = any || run[j];
    }
    if (!any) return;
    TV neps[K], ndelta[K], igamma[K], phi[K], ibeta[K];
    bool all = true;
#pragma unroll
    for (int j = 0; j < K; j++) {
        const double uu = run[j] ? block_sum_array(red + (size_t)j * nred, nred, s_red) : 0.0;
        const MinresRot o = sc->rot[j][(k + 1) & 1];
        const double alpha = sc->col[j].alpha, beta1 = sc->beta1[j];
        const double betan = sqrt(uu);
        MinresRot r;
        r.beta = betan;
        const double delta = o.cs * o.dbar + o.sn * alpha;
        const double gbar = o.sn * o.dbar - o.cs * alpha;
        r.eps = o.sn * betan;
        r.dbar = -o.cs * betan;
        const double gamma = hypot(gbar, betan);
        r.cs = gbar / gamma;
        r.sn = betan / gamma;
        const double phi_d = r.cs * o.phibar;
        r.phibar = r.sn * o.phibar;
        const double re = r.phibar / beta1;
        const bool stop = re < rel_error;
        adv[j] = run[j] && !stop;
        all = all && !adv[j];
        neps[j] = -(TV)o.eps;
        ndelta[j] = -(TV)delta;
        igamma[j] = (TV)(1.0 / gamma);
        phi[j] = (TV)phi_d;
        ibeta[j] = (TV)(1.0 / betan);
        if (run[j] && blockIdx.x == 0 && threadIdx.x == 0) {
            sc->rot[j][k & 1] = r;
            sc->rel_err[j] = re;
            sc->col[j].beta = betan;
            sc->col[j].iters = k;
        }
    }
    // a workgroup that starts after workgroup 0 has frozen a column in THIS launch reads frozen_at = k + 1 and runs it, as workgroup
    // 0 did; `all` is computed from the same bits everywhere, and only workgroup 0's value is used
    if (blockIdx.x == 0) {
        __syncthreads();
        if (threadIdx.x == 0) {
#pragma unroll
            for (int j = 0; j < K; j++)
                if (run[j] && !adv[j]) { sc->frozen_at[j] = k + 1; sc->col[j].stop = 1; }
            if (all) sc->all_stop = 1;
            post_progress(host_flags, k, all);
        }
    }
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
#pragma unroll
        for (int j = 0; j < K; j++) {
            if (!run[j]) continue;
            const uint64_t e = i * K + j;
            const TV vi = V[e], wi = W[e];
            const TV wn = fma_tv(ndelta[j], wi, fma_tv(neps[j], WOLD[e], vi)) * igamma[j];
            WOLD[e] = wi;
            W[e] = wn;
            X[e] = fma_tv(phi[j], wn, X[e]);
            if (adv[j]) {
                VOLD[e] = vi;
                V[e] = U[e] * ibeta[j];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Batched Lanczos quadrature (lam_hip_lanczos_many, lam_quad.h): K independent plain Lanczos recurrences on A -- three-term only, no
// reorthogonalisation, no stored basis -- advanced together, from K probes.  Three launches per step: multi_gemv_kernel on V
// (u = A v, partials of v.u), quad_three_term_kernel (alpha = v.u ; u -= alpha v + beta v_old ; partials of u.u) and
// quad_next_kernel (beta' = sqrt(u.u), the history store, lam_hip_eigs' breakdown rule, v_old = v, v = u / beta').  The recurrence is
// stated in include/lam_hip.h.  In front of the loop: quad_probe_kernel (the probes into V, partials of z.z),
// quad_start_scalars_kernel and quad_start_kernel (v = z / ||z||, v_old = 0).
// Vectors: V is the batch's P (the product's input: zero behind row n), U its AP, v_old its R.
// Scalars: the MultiScalars prefix (what the product kernel reads) with col[j].alpha = the last v.u, .beta = the last beta', .iters,
// .stop; behind it beta and the breakdown rule's scale in rings of two -- step k reads slot (k + 1) & 1, workgroup 0 writes slot
// k & 1 (MinresScalars::rot's scheme) -- and the history [step][K] the host copies back once per group.
// Who decides: minres_update_kernel's argument to the letter.  Every workgroup of quad_next_kernel recomputes a probe's beta' and
// its breakdown decision from bits no workgroup of that launch writes; workgroup 0 alone stores.  frozen_at[j] is the first step in
// which the probe does nothing (0: live; k + 1 for a breakdown at k; 1 for a padding column), so a workgroup that starts behind
// workgroup 0's store reads "ran at k" as workgroup 0 did.  The launch does not return on all_stop, which its own workgroup 0
// raises: it returns when no probe runs at k by frozen_at.  The product and quad_three_term_kernel keep the all_stop guard.
// Coefficients that multiply vectors (alpha, beta, the reciprocals) are formed in fp64 and rounded to the vector dtype once; every
// vector statement is an explicit fma_tv chain.
// ---------------------------------------------------------------------------------------------
struct QuadScalars : MultiScalars {
    double zz[kMaxRhs];               // z.z of the probe as given
    double beta[kMaxRhs][2];          // beta_k at [k & 1] (beta_0 = 0 in both slots at the start)
    double tmax[kMaxRhs][2];          // max_{i <= k}(|alpha_i| + beta_{i-1} + beta_i) at [k & 1]
    int frozen_at[kMaxRhs];           // 0: live; else the first step in which the probe does nothing
    int steps_run[kMaxRhs];           // the last step the probe completed
    double hist_alpha[kMaxLanczos * kMaxRhs];     // alpha_k of probe j at [(k - 1) * K + j], K the group's instantiation
    double hist_beta[kMaxLanczos * kMaxRhs];
};

// The Rademacher law of the generated probes: z_j[i] = 1 - 2 (h >> 63), h = sm(seed ^ sm(0x51AC + j * n + i)), j the GLOBAL probe index
__host__ __device__ __forceinline__ double quad_rademacher(uint64_t seed, uint64_t probe, uint64_t n, uint64_t i)
{
    const uint64_t h = splitmix64(seed ^ splitmix64(0x51ACull + probe * n + i));
    return 1.0 - 2.0 * (double)(h >> 63);
}

// V = the probes: GENERATE the Rademacher law by global probe index first + j, else what the upload left in V; padding columns
// (j >= count) zero; V's rows behind row n zero in this K's layout (minres_init_kernel); partials of z_j.z_j at [j * gridDim.x + block]
template <typename TV, int K>
__global__ void __launch_bounds__(kBlock)
quad_probe_kernel(bool generate, int count, uint64_t first, uint64_t seed, TV *__restrict__ V, uint64_t n, double *__restrict__ partial)
{
    __shared__ double s_red[kWaves];
    double acc[K];
#pragma unroll
    for (int j = 0; j < K; j++) acc[j] = 0.0;
    if (blockIdx.x == 0 && threadIdx.x < kMultiPadRows * K) V[n * K + threadIdx.x] = (TV)0;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
#pragma unroll
        for (int j = 0; j < K; j++) {
            const uint64_t e = i * K + j;
            TV zi = (TV)0;
            if (j < count) zi = generate ? (TV)quad_rademacher(seed, first + (uint64_t)j, n, i) : V[e];
            V[e] = zi;
            acc[j] += (double)zi * (double)zi;
        }
    }
#pragma unroll
    for (int j = 0; j < K; j++) {
        const double t = block_sum(acc[j], s_red);
        if (threadIdx.x == 0) partial[(size_t)j * gridDim.x + blockIdx.x] = t;
    }
}

// per probe: zz, the rings' start (beta_0 = 0, tmax = 0), iters = 0; live probes start running, padding columns are born stopped.
// One workgroup.
template <int K>
__global__ void __launch_bounds__(kBlock)
quad_start_scalars_kernel(const double *__restrict__ red, int nred, int count, QuadScalars *sc, volatile int *host_flags)
{
    __shared__ double s_red[kWaves];
    for (int j = 0; j < kMaxRhs; j++) {
        const double t = j < K ? block_sum_array(red + (size_t)j * nred, nred, s_red) : 0.0;
        if (threadIdx.x == 0) {
            CgScalars &c = sc->col[j];
            c.bb = t; c.rr[0] = 0.0; c.rr[1] = 0.0; c.pAp = 0.0; c.alpha = 0.0; c.beta = 0.0; c.iters = 0;
            c.stop = j < count ? 0 : 1;
            sc->zz[j] = t;
            sc->beta[j][0] = 0.0; sc->beta[j][1] = 0.0;
            sc->tmax[j][0] = 0.0; sc->tmax[j][1] = 0.0;
            sc->frozen_at[j] = j < count ? 0 : 1;
            sc->steps_run[j] = 0;
        }
    }
    if (threadIdx.x == 0) {
        sc->pad = 0;
        sc->all_stop = 0;
        post_progress(host_flags, 0, false);
    }
}

// v_j = z_j * (1 / sqrt(zz_j)) in place for the live probes (the padding columns are zero already) ; v_old = 0
template <typename TV, int K>
__global__ void __launch_bounds__(kBlock)
quad_start_kernel(TV *__restrict__ V, TV *__restrict__ VOLD, uint64_t n, const QuadScalars *sc)
{
    TV iz[K];
    bool live[K];
#pragma unroll
    for (int j = 0; j < K; j++) {
        live[j] = sc->frozen_at[j] == 0;
        iz[j] = (TV)(1.0 / sqrt(sc->zz[j]));
    }
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
#pragma unroll
        for (int j = 0; j < K; j++) {
            const uint64_t e = i * K + j;
            if (live[j]) V[e] = V[e] * iz[j];
            VOLD[e] = (TV)0;
        }
    }
}

// vector launch 1, per running probe j: alpha = v_j.u_j from the product's partials ; u_j = fma(-beta, v_old_j, fma(-alpha, v_j, u_j)) ;
// partials of u_j.u_j.  minres_lanczos_kernel's statement on this section's scalars.  No workgroup writes what another reads:
// col[j].alpha is for the next launch.
template <typename TV, int K>
__global__ void __launch_bounds__(kBlock)
quad_three_term_kernel(const double *__restrict__ red, int nred, QuadScalars *sc, int k, const TV *__restrict__ V,
                       const TV *__restrict__ VOLD, TV *__restrict__ U, uint64_t n, double *__restrict__ partial)
{
    __shared__ double s_red[kWaves];
    if (sc->all_stop) return;
    bool run[K];
    double alpha_d[K], acc[K];
    TV nalpha[K], nbeta[K];
#pragma unroll
    for (int j = 0; j < K; j++) {
        run[j] = sc->col[j].stop == 0;
        alpha_d[j] = run[j] ? block_sum_array(red + (size_t)j * nred, nred, s_red) : 0.0;
        nalpha[j] = -(TV)alpha_d[j];
        nbeta[j] = -(TV)sc->beta[j][(k + 1) & 1];
        acc[j] = 0.0;
    }
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
#pragma unroll
        for (int j = 0; j < K; j++) {
            if (!run[j]) continue;
            const uint64_t e = i * K + j;
            const TV ui = fma_tv(nbeta[j], VOLD[e], fma_tv(nalpha[j], V[e], U[e]));
            U[e] = ui;
            acc[j] += (double)ui * (double)ui;
        }
    }
#pragma unroll
    for (int j = 0; j < K; j++) {
        const double t = block_sum(acc[j], s_red);
        if (threadIdx.x == 0) {
            partial[(size_t)j * gridDim.x + blockIdx.x] = t;
            if (blockIdx.x == 0 && run[j]) { sc->col[j].pAp = alpha_d[j]; sc->col[j].alpha = alpha_d[j]; }
        }
    }
}

// vector launch 2, per running probe j: beta' = sqrt(u_j.u_j) ; alpha and beta' into the history ; the breakdown rule (beta' zero,
// not finite or <= scale * max_i(|alpha_i| + beta_{i-1} + beta_i), scale = N * unit roundoff of the vector dtype): the probe stops,
// v_j untouched; else v_old_j = v_j, v_j = u_j * (1 / beta').  The progress word reports the step, and "stopped" once EVERY live
// probe has broken down.
template <typename TV, int K>
__global__ void __launch_bounds__(kBlock)
quad_next_kernel(const double *__restrict__ red, int nred, QuadScalars *sc, int k, double scale, const TV *__restrict__ U,
                 TV *__restrict__ V, TV *__restrict__ VOLD, uint64_t n, volatile int *host_flags)
{
    __shared__ double s_red[kWaves];
    // NOT `if (sc->all_stop) return` (see minres_update_kernel): the launch is over only if no probe runs at k, which frozen_at says
    // the same way before and after workgroup 0's store
    bool run[K], adv[K];
    bool any = false;
#pragma unroll
    for (int j = 0; j < K; j++) {
        const int fz = sc->frozen_at[j];
        run[j] = fz == 0 || k < fz;
        any = any || run[j];
    }
    if (!any) return;
    TV ibeta[K];
    bool all = true;
#pragma unroll
    for (int j = 0; j < K; j++) {
        const double uu = run[j] ? block_sum_array(red + (size_t)j * nred, nred, s_red) : 0.0;
        const double betan = sqrt(uu);
        const double alpha = sc->col[j].alpha;                           // the three-term launch of this step wrote it
        const double bprev = sc->beta[j][(k + 1) & 1], tprev = sc->tmax[j][(k + 1) & 1];
        const double tmax = fmax(tprev, fabs(alpha) + bprev + betan);
        const bool stop = !(betan > scale * tmax) || !(betan <= std::numeric_limits<double>::max());
        adv[j] = run[j] && !stop;
        all = all && !adv[j];
        ibeta[j] = (TV)(1.0 / betan);
        if (run[j] && blockIdx.x == 0 && threadIdx.x == 0) {
            sc->beta[j][k & 1] = betan;
            sc->tmax[j][k & 1] = tmax;
            sc->col[j].beta = betan;
            sc->col[j].iters = k;
            sc->steps_run[j] = k;
            sc->hist_alpha[(size_t)(k - 1) * K + j] = alpha;
            sc->hist_beta[(size_t)(k - 1) * K + j] = betan;
        }
    }
    if (blockIdx.x == 0) {
        __syncthreads();
        if (threadIdx.x == 0) {
#pragma unroll
            for (int j = 0; j < K; j++)
                if (run[j] && !adv[j]) { sc->frozen_at[j] = k + 1; sc->col[j].stop = 1; }
            if (all) sc->all_stop = 1;
            post_progress(host_flags, k, all);
        }
    }
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
#pragma unroll
        for (int j = 0; j < K; j++) {
            if (!adv[j]) continue;
            const uint64_t e = i * K + j;
            const TV vi = V[e];
            VOLD[e] = vi;
            V[e] = U[e] * ibeta[j];
        }
    }
}


// ---------------------------------------------------------------------------------------------
// Multi-shift CG (lam_hip_solve_mshift, lam_multi.h): (A + s_j I) x_j = b for up to kMaxShifts shifts and ONE b.  The shifted Krylov
// spaces are one space and the shifted residuals stay collinear with the seed's, r_j = zeta_j r (Jegerlehner; Frommer), so the
// K = 1 batch on the smallest shift (the seed) is the only product, and one launch per iteration behind multi_p_kernel advances
// every other shift from the seed's alpha, beta and r.  With d_j = s_j - s_min, a / b the seed's alpha / beta, Z_0 = Z_1 = 1,
// a_0 = 1, b_0 = 0, iteration k = 1, 2, ...:
//   Z_{k+1} = Z_k Z_{k-1} a_{k-1} / (a_k b_{k-1} (Z_{k-1} - Z_k) + Z_{k-1} a_{k-1} (1 + d_j a_k))
//   x_j += (a_k Z_{k+1} / Z_k) p_j ;  rel_err_j = Z_{k+1} sqrt(rr_k / bb) ;  stop if rel_err_j < rel_error, else
//   p_j = Z_{k+1} r + b_k (Z_{k+1} / Z_k)^2 p_j                          (r: the seed's R, already updated by multi_xr_kernel)
// All scalars fp64; the three coefficients are rounded to the vector dtype once per shift and iteration.
//
// Layout: shifts live in groups of G = 8, XS and PS interleaved [n + kMultiPadRows][G] per group -- the K = 8 batch layout, so the
// true residual hands a group to the K = 8 product as it is.  Slots past nshifts and slots with d_j == 0 (the seed's own shift: their
// x is the batch's X, copied by mshift_copy_seed_kernel) are born frozen with x = p = 0.
// Who decides: every workgroup recomputes Z_{k+1} and the coefficients from slots nobody writes in this launch (the zeta ring's
// slots k % 3 and (k - 1) % 3, the seed ring's slot (k - 1) & 1); workgroup (0, g) alone writes the new ones.  frozen_at is the
// first iteration in which the shift does nothing: a stop at k still takes iteration k's x update, so it writes k + 1, and a
// workgroup that starts later reads "live at k", which is what it would have decided itself from the same bits (multi_p_kernel's
// argument); an underflow at k writes k, and the late workgroup reads what it would have found.
// ---------------------------------------------------------------------------------------------
constexpr int kMaxShifts = 64;
constexpr int kShiftGroup = 8;
struct MshiftScalars {
    double zeta[kMaxShifts][3];   // Z_m at [m % 3]
    double d[kMaxShifts];         // s_j - s_min >= 0
    double rel_err[kMaxShifts];   // of the last completed step
    double seed_ab[2][2];         // the seed's {alpha, beta} of iteration k at [k & 1]
    int frozen_at[kMaxShifts];    // 0: live; else the first iteration in which the shift does nothing
    int iters[kMaxShifts];        // last completed step
    int stop[kMaxShifts];         // met its stop test
};
struct MshiftList { double d[kMaxShifts]; };

// x = 0, p = b for the live slots (0 for the others) of every group, and the scalars' start values; grid (vec_grid(n), groups)
template <typename TV, int G>
__global__ void __launch_bounds__(kBlock)
mshift_init_kernel(const TV *__restrict__ B, TV *__restrict__ XS, TV *__restrict__ PS, uint64_t n, int nshifts, MshiftList dl,
                   MshiftScalars *ms)
{
    const int g = blockIdx.y;
    const uint64_t base = (uint64_t)g * (n + kMultiPadRows) * G;
    bool live[G];
#pragma unroll
    for (int j = 0; j < G; j++) live[j] = g * G + j < nshifts && dl.d[g * G + j] > 0.0;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        const TV bi = B[i];
#pragma unroll
        for (int j = 0; j < G; j++) {
            XS[base + i * G + j] = (TV)0;
            PS[base + i * G + j] = live[j] ? bi : (TV)0;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < G) {
        const int slot = g * G + threadIdx.x;
        const bool lv = slot < nshifts && dl.d[slot] > 0.0;
        ms->zeta[slot][0] = ms->zeta[slot][1] = ms->zeta[slot][2] = 1.0;
        ms->d[slot] = slot < nshifts ? dl.d[slot] : 0.0;
        ms->rel_err[slot] = 1.0;
        ms->frozen_at[slot] = lv ? 0 : 1;
        ms->iters[slot] = 0;
        ms->stop[slot] = 0;
        if (slot == 0) {
            ms->seed_ab[0][0] = 1.0; ms->seed_ab[0][1] = 0.0;
            ms->seed_ab[1][0] = 0.0; ms->seed_ab[1][1] = 0.0;
        }
    }
}

// iteration k of every live shift, behind multi_p_kernel of iteration k; grid (vec_grid(n), groups).  The launches the lag rule
// enqueues past the seed's stop find seed.iters != k and return at once, before they read scalars that belong to another
// iteration.  Results cannot show this guard: a shift that has stopped is frozen by frozen_at anyway, and a shift still live
// behind the seed's stop needs zeta > 1, which only rounding could produce (mutations).
template <typename TV, int G>
__global__ void __launch_bounds__(kBlock)
mshift_step_kernel(const MultiScalars *sc, MshiftScalars *ms, int k, double rel_error, const TV *__restrict__ R, TV *__restrict__ XS,
                   TV *__restrict__ PS, uint64_t n)
{
    const CgScalars &seed = sc->col[0];
    if (seed.iters != k) return;
    const int g = blockIdx.y;
    const double a = seed.alpha, b = seed.beta, rel = sqrt(seed.rr[k & 1] / seed.bb);
    const double a_prev = ms->seed_ab[(k - 1) & 1][0], b_prev = ms->seed_ab[(k - 1) & 1][1];
    bool live[G], cont[G];
    TV cx[G], cr[G], cp[G];
    bool any = false;
#pragma unroll
    for (int j = 0; j < G; j++) {
        const int slot = g * G + j;
        const int fz = ms->frozen_at[slot];
        const bool was_live = fz == 0 || k < fz;
        const double z0 = ms->zeta[slot][k % 3], zm = ms->zeta[slot][(k + 2) % 3], d = ms->d[slot];
        const double z1 = z0 * zm * a_prev / (a * b_prev * (zm - z0) + zm * a_prev * (1.0 + d * a));
        // finite, but zero or subnormal: the shift has converged past what fp64 can scale r by and is frozen BEFORE this step
        // (a NaN is not: it runs to the cap as a batch column's would)
        const bool under = fabs(z1) < std::numeric_limits<double>::min();
        const double ratio = z1 / z0, re = z1 * rel;
        const bool stop = re < rel_error;
        live[j] = was_live && !under;
        cont[j] = live[j] && !stop;
        cx[j] = (TV)(a * ratio);
        cr[j] = (TV)z1;
        cp[j] = (TV)(b * ratio * ratio);
        any = any || live[j];
        if (was_live && blockIdx.x == 0 && threadIdx.x == 0) {
            if (under) {
                ms->frozen_at[slot] = k;
            } else {
                ms->zeta[slot][(k + 1) % 3] = z1;
                ms->rel_err[slot] = re;
                ms->iters[slot] = k;
                if (stop) { ms->stop[slot] = 1; ms->frozen_at[slot] = k + 1; }
            }
        }
    }
    if (g == 0 && blockIdx.x == 0 && threadIdx.x == 0) { ms->seed_ab[k & 1][0] = a; ms->seed_ab[k & 1][1] = b; }
    if (!any) return;
    const uint64_t base = (uint64_t)g * (n + kMultiPadRows) * G;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        const TV ri = R[i];
#pragma unroll
        for (int j = 0; j < G; j++) {
            if (!live[j]) continue;
            const uint64_t e = base + i * G + j;
            const TV pi = PS[e];
            XS[e] = cx[j] * pi + XS[e];
            if (cont[j]) PS[e] = fma_tv(cr[j], ri, cp[j] * pi);
        }
    }
}

// the slots of `mask` (bit = slot) hold the seed's own shift: their x is the batch's X (K = 1 layout), copied, not recomputed
template <typename TV, int G>
__global__ void __launch_bounds__(kBlock)
mshift_copy_seed_kernel(const TV *__restrict__ X, TV *__restrict__ XS, uint64_t n, unsigned long long mask)
{
    const int g = blockIdx.y;
    const unsigned gm = (unsigned)(mask >> (g * G)) & ((1u << G) - 1u);
    if (gm == 0) return;
    const uint64_t base = (uint64_t)g * (n + kMultiPadRows) * G;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        const TV xi = X[i];
#pragma unroll
        for (int j = 0; j < G; j++)
            if (gm >> j & 1u) XS[base + i * G + j] = xi;
    }
}

// lam_hip_true_residual_mshift: multi_residual_kernel against the ONE b: with Y = (A + s_j I) x_j of a group from the K = 8
// product, r = b - y_j rounded to the vector dtype; fp64 partials of r_j.r_j and (the same for every j) of b.b, laid out for
// multi_residual_scalars_kernel
template <typename TV, int G>
__global__ void __launch_bounds__(kBlock)
mshift_residual_kernel(const TV *__restrict__ B, const TV *__restrict__ Y, uint64_t n, double *__restrict__ partial_rr,
                       double *__restrict__ partial_bb)
{
    __shared__ double s_red[kWaves];
    double acc[G], accb = 0.0;
#pragma unroll
    for (int j = 0; j < G; j++) acc[j] = 0.0;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        const TV bi = B[i];
        accb += (double)bi * (double)bi;
#pragma unroll
        for (int j = 0; j < G; j++) {
            const TV ri = bi - Y[i * G + j];
            acc[j] += (double)ri * (double)ri;
        }
    }
    const double tb = block_sum(accb, s_red);
#pragma unroll
    for (int j = 0; j < G; j++) {
        const double t = block_sum(acc[j], s_red);
        if (threadIdx.x == 0) {
            partial_rr[(size_t)j * gridDim.x + blockIdx.x] = t;
            partial_bb[(size_t)j * gridDim.x + blockIdx.x] = tb;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Lanczos (lam_hip_eigs, lam_eigs.h): extreme eigenpairs of A from a Lanczos recurrence with FULL reorthogonalisation, one product
// per step.  The recurrence is stated in include/lam_hip.h.  Step `step` (counted from 1; k = step - 1) is the K = 1 product launch
// on basis row v_k (u = A v_k, partials of v_k.u) and six launches of this section:
//   lanczos_three_term_kernel    alpha_k from the product's partials ; u = fma(-beta_{k-1}, v_{k-1}, fma(-alpha_k, v_k, u))
//   lanczos_dots_kernel          partial[j][block] of c_j = v_j.u, j = 0..k            \  one pass of classical Gram-Schmidt,
//   lanczos_apply_kernel         c_j from the partials ; u = fma(-c_j, v_j, u), j up   /  run twice; the second one ends in u.u
//   lanczos_append_kernel        beta_k = sqrt(u.u), the breakdown rule, v_{k+1} = u * (1 / beta_k), the progress word
// Basis: row j at V + j * pitch, pitch a 256-byte multiple of n + kMultiPadRows elements, zero behind element n, so a row is the
// product's input as it stands.  The two projection kernels cut u into one contiguous slab per workgroup (whole 16-byte vectors;
// the last slab takes the ragged tail element by element): a workgroup reads its slab of u ONCE, holds it in registers
// (kLanczosHold 16-byte vectors per thread and round; a slab longer than that takes further rounds), and streams the same slab of
// every basis row past it with 16-byte loads (lanczos_dots_kernel: of the rows its y index is dealt).  All sums are fp64 and of fixed order: lane, wave (wave_sum), the four waves, then
// the workgroups' partials in block order -- no floating-point atomics, the same bits on every run.
// Who decides: stopped_at (0: running; else the step whose beta met the breakdown rule) is written by workgroup 0 of that step's
// append launch alone; every launch of a LATER step returns on it, and the append launch itself recomputes the decision in every
// workgroup from bits no workgroup of it writes (minres_update_kernel's argument).
// ---------------------------------------------------------------------------------------------
constexpr int kLanczosHold = 4;       // 16-byte vectors of u a thread holds per round of a projection kernel
constexpr int kLanczosSplit = 16;     // gridDim.y of lanczos_dots_kernel: the basis rows are dealt out over this many workgroups per slab
struct LanczosScalars : MultiScalars {            // the prefix is what the product kernel reads (all_stop)
    double alpha[kMaxLanczos];        // alpha_k = v_k.(A v_k), the product's fused partials
    double beta[kMaxLanczos];         // beta_k = ||u|| behind the reorthogonalisation of step k: the norm that made v_{k+1}
    double tmax[kMaxLanczos];         // max over j <= k of |alpha_j| + beta_{j-1} + beta_j: the breakdown rule's scale
    double v0norm;                    // ||v0|| of the start vector as given
    int steps;                        // steps completed
    int stopped_at;                   // 0, or the step (from 1) at which the Krylov space was found invariant
};

template <typename TV>
__device__ __forceinline__ void lanczos_slab(uint64_t n, uint64_t *first, uint64_t *end)
{
    constexpr uint64_t VEC = 16 / sizeof(TV);
    const uint64_t nvec = (n + VEC - 1) / VEC;
    const uint64_t per = (nvec + gridDim.x - 1) / gridDim.x * VEC;
    const uint64_t f = (uint64_t)blockIdx.x * per;
    *first = f < n ? f : n;
    *end = f + per < n ? f + per : n;
}

// VEC elements of x from element idx (a multiple of VEC; x 16-byte aligned): one 16-byte load where they all lie in front of `end`,
// else the ones that do, element by element, and zeros
template <typename TV>
__device__ __forceinline__ void lanczos_load(const TV *__restrict__ x, uint64_t idx, uint64_t end, TV (&out)[16 / sizeof(TV)])
{
    constexpr int VEC = 16 / sizeof(TV);
    typedef TV vec_t __attribute__((ext_vector_type(VEC)));
    if (idx + VEC <= end) {
        const vec_t v = *reinterpret_cast<const vec_t *>(x + idx);
#pragma unroll
        for (int e = 0; e < VEC; e++) out[e] = v[e];
    } else {
#pragma unroll
        for (int e = 0; e < VEC; e++) out[e] = idx + e < end ? x[idx + e] : (TV)0;
    }
}
template <typename TV>
__device__ __forceinline__ void lanczos_store(TV *__restrict__ x, uint64_t idx, uint64_t end, const TV (&in)[16 / sizeof(TV)])
{
    constexpr int VEC = 16 / sizeof(TV);
    typedef TV vec_t __attribute__((ext_vector_type(VEC)));
    if (idx + VEC <= end) {
        vec_t v;
#pragma unroll
        for (int e = 0; e < VEC; e++) v[e] = in[e];
        *reinterpret_cast<vec_t *>(x + idx) = v;
    } else {
#pragma unroll
        for (int e = 0; e < VEC; e++)
            if (idx + e < end) x[idx + e] = in[e];
    }
}

__device__ __forceinline__ bool lanczos_over(const LanczosScalars *sc, int step)
{
    if (sc == nullptr) return false;
    const int st = sc->stopped_at;
    return st != 0 && step > st;
}

// partials of v0.v0 are dot_partial_kernel's; this one: v_0 = v0 * (1 / ||v0||), the scalars' start, the progress word.  v0 is in u.
template <typename TV>
__global__ void __launch_bounds__(kBlock)
lanczos_start_kernel(const double *__restrict__ red, int nred, LanczosScalars *sc, const TV *__restrict__ u, TV *__restrict__ v0, uint64_t n,
                     volatile int *host_flags)
{
    __shared__ double s_red[kWaves];
    const double nrm = sqrt(block_sum_array(red, nred, s_red));
    const TV inv = (TV)(1.0 / nrm);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        for (int j = 0; j < kMaxRhs; j++) {
            CgScalars &c = sc->col[j];
            c.bb = 0.0; c.rr[0] = 0.0; c.rr[1] = 0.0; c.pAp = 0.0; c.alpha = 0.0; c.beta = 0.0; c.iters = 0;
            c.stop = j == 0 ? 0 : 1;
        }
        sc->all_stop = 0;
        sc->pad = 0;
        sc->v0norm = nrm;
        sc->steps = 0;
        sc->stopped_at = 0;
        post_progress(host_flags, 0, false);
    }
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) v0[i] = u[i] * inv;
}

template <typename TV>
__global__ void __launch_bounds__(kBlock)
lanczos_three_term_kernel(const double *__restrict__ red, int nred, LanczosScalars *sc, int step, const TV *__restrict__ vk,
                          const TV *__restrict__ vkm1, TV *__restrict__ u, uint64_t n)
{
    __shared__ double s_red[kWaves];
    if (lanczos_over(sc, step)) return;
    const int k = step - 1;
    const double alpha = block_sum_array(red, nred, s_red);
    const TV nalpha = -(TV)alpha;
    if (k == 0) {
        for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock)
            u[i] = fma_tv(nalpha, vk[i], u[i]);
    } else {
        const TV nbeta = -(TV)sc->beta[k - 1];
        for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock)
            u[i] = fma_tv(nbeta, vkm1[i], fma_tv(nalpha, vk[i], u[i]));
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { sc->alpha[k] = alpha; sc->col[0].alpha = alpha; sc->col[0].pAp = alpha; }
}

// partial[j * gridDim.x + blockIdx.x] = the workgroup's part of v_j.u; the grid's y dimension deals the rows out: workgroup (x, y) takes
// the slab x of u and of the rows j = y, y + gridDim.y, ... < m, so the launch has the same shape whatever m is and the stream of V
// meets gridDim.y times the workgroups a one-dimensional grid of slabs would give it.  sc may be null (lam_hip_project_out).
template <typename TV>
__global__ void __launch_bounds__(kBlock)
lanczos_dots_kernel(const LanczosScalars *sc, int step, const TV *__restrict__ V, uint64_t pitch, int m, const TV *__restrict__ u, uint64_t n,
                    double *__restrict__ partial)
{
    constexpr int VEC = 16 / sizeof(TV);
    __shared__ double s_acc[kMaxLanczos + 1][kWaves];
    if (lanczos_over(sc, step)) return;
    uint64_t first, end;
    lanczos_slab<TV>(n, &first, &end);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr uint64_t ROUND = (uint64_t)kBlock * VEC * kLanczosHold;
    bool round0 = true;
    for (uint64_t base = first; round0 || base < end; base += ROUND) {
        TV ur[kLanczosHold][VEC];
#pragma unroll
        for (int h = 0; h < kLanczosHold; h++) lanczos_load<TV>(u, base + ((uint64_t)h * kBlock + threadIdx.x) * VEC, end, ur[h]);
#pragma unroll 2
        for (int j = blockIdx.y; j < m; j += gridDim.y) {
            const TV *vj = V + (uint64_t)j * pitch;
            double a = 0.0;
#pragma unroll
            for (int h = 0; h < kLanczosHold; h++) {
                TV vr[VEC];
                lanczos_load<TV>(vj, base + ((uint64_t)h * kBlock + threadIdx.x) * VEC, end, vr);
#pragma unroll
                for (int e = 0; e < VEC; e++) a = __builtin_fma((double)vr[e], (double)ur[h][e], a);
            }
            a = wave_sum(a);
            if (lane == 0) s_acc[j][wave] = round0 ? a : s_acc[j][wave] + a;
        }
        round0 = false;
    }
    __syncthreads();
    for (int j = blockIdx.y + threadIdx.x * gridDim.y; j < m; j += kBlock * gridDim.y) {
        double t = s_acc[j][0];
#pragma unroll
        for (int w = 1; w < kWaves; w++) t += s_acc[j][w];
        partial[(size_t)j * gridDim.x + blockIdx.x] = t;
    }
}

// c_j = the nred partials of column j in block order (the same bits in every workgroup) ; u = fma(-(TV)c_j, v_j, u) for j = 0..m-1
// in ascending order on the workgroup's slab ; NORM: partial_uu[block] of the new u.u.  coeff (may be null): c_j in fp64, by
// workgroup 0.
template <typename TV, bool NORM>
__global__ void __launch_bounds__(kBlock)
lanczos_apply_kernel(const LanczosScalars *sc, int step, const double *__restrict__ partial, int nred, const TV *__restrict__ V, uint64_t pitch,
                     int m, TV *__restrict__ u, uint64_t n, double *__restrict__ coeff, double *__restrict__ partial_uu)
{
    constexpr int VEC = 16 / sizeof(TV);
    __shared__ TV s_nc[kMaxLanczos + 1];
    __shared__ double s_red[kWaves];
    if (lanczos_over(sc, step)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int j = wave; j < m; j += kWaves) {
        double a = 0.0;
        for (int b = lane; b < nred; b += 64) a += partial[(size_t)j * nred + b];
        a = wave_sum(a);
        if (lane == 0) {
            s_nc[j] = -(TV)a;
            if (coeff != nullptr && blockIdx.x == 0) coeff[j] = a;
        }
    }
    __syncthreads();
    uint64_t first, end;
    lanczos_slab<TV>(n, &first, &end);
    constexpr uint64_t ROUND = (uint64_t)kBlock * VEC * kLanczosHold;
    double acc = 0.0;
    for (uint64_t base = first; base < end; base += ROUND) {
        TV ur[kLanczosHold][VEC];
#pragma unroll
        for (int h = 0; h < kLanczosHold; h++) lanczos_load<TV>(u, base + ((uint64_t)h * kBlock + threadIdx.x) * VEC, end, ur[h]);
#pragma unroll 4
        for (int j = 0; j < m; j++) {
            const TV *vj = V + (uint64_t)j * pitch;
            const TV nc = s_nc[j];
#pragma unroll
            for (int h = 0; h < kLanczosHold; h++) {
                TV vr[VEC];
                lanczos_load<TV>(vj, base + ((uint64_t)h * kBlock + threadIdx.x) * VEC, end, vr);
#pragma unroll
                for (int e = 0; e < VEC; e++) ur[h][e] = fma_tv(nc, vr[e], ur[h][e]);
            }
        }
#pragma unroll
        for (int h = 0; h < kLanczosHold; h++) {
            lanczos_store<TV>(u, base + ((uint64_t)h * kBlock + threadIdx.x) * VEC, end, ur[h]);
            if constexpr (NORM) {
#pragma unroll
                for (int e = 0; e < VEC; e++) acc = __builtin_fma((double)ur[h][e], (double)ur[h][e], acc);
            }
        }
    }
    if constexpr (NORM) {
        const double t = block_sum(acc, s_red);
        if (threadIdx.x == 0) partial_uu[blockIdx.x] = t;
    }
}

// beta_k = sqrt(u.u) ; the Krylov space is invariant if beta_k is 0, not finite or <= scale * max_{j <= k}(|alpha_j| + beta_{j-1} +
// beta_j), scale = N * (unit roundoff of the vector dtype): the run stops, v_{k+1} is not formed and the progress word says
// "stopped"; else v_{k+1} = u * (1 / beta_k).
template <typename TV>
__global__ void __launch_bounds__(kBlock)
lanczos_append_kernel(const double *__restrict__ red, int nred, LanczosScalars *sc, int step, double scale, const TV *__restrict__ u,
                      TV *__restrict__ vnext, uint64_t n, volatile int *host_flags)
{
    __shared__ double s_red[kWaves];
    if (lanczos_over(sc, step)) return;
    const int k = step - 1;
    const double beta = sqrt(block_sum_array(red, nred, s_red));
    const double alpha = sc->alpha[k];                                   // the three-term launch of this step wrote it
    const double bprev = k > 0 ? sc->beta[k - 1] : 0.0, tprev = k > 0 ? sc->tmax[k - 1] : 0.0;
    const double tmax = fmax(tprev, fabs(alpha) + bprev + beta);
    const bool stop = !(beta > scale * tmax) || !(beta <= std::numeric_limits<double>::max());
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        sc->beta[k] = beta;
        sc->tmax[k] = tmax;
        sc->col[0].beta = beta;
        sc->col[0].iters = step;
        sc->steps = step;
        if (stop) { sc->stopped_at = step; sc->col[0].stop = 1; sc->all_stop = 1; }
        post_progress(host_flags, step, stop);
    }
    if (stop) return;
    const TV ib = (TV)(1.0 / beta);
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) vnext[i] = u[i] * ib;
}

// Ritz vectors: Y[pair][i] = sum_j S[pair][j] V[j][i], fp64 coefficients, fp64 accumulation in ascending j, one rounding to the
// vector dtype.  S: column `pair` of the tridiagonal's eigenvector matrix contiguous at S + pair * k; Y: pair contiguous at Y + pair * n.
template <typename TV>
__global__ void __launch_bounds__(kBlock)
lanczos_ritz_kernel(const TV *__restrict__ V, uint64_t pitch, int k, const double *__restrict__ S, TV *__restrict__ Y, uint64_t n)
{
    __shared__ double s_s[kMaxLanczos];
    const int pair = blockIdx.y;
    for (int j = threadIdx.x; j < k; j += kBlock) s_s[j] = S[(size_t)pair * k + j];
    __syncthreads();
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        double acc = 0.0;
        for (int j = 0; j < k; j++) acc = __builtin_fma(s_s[j], (double)V[(uint64_t)j * pitch + i], acc);
        Y[(uint64_t)pair * n + i] = (TV)acc;
    }
}

// lam_hip_eig_residuals: with AY = A Y from one batched product ([n][K] both), per column the fp64 partials of
// (A y - theta y).(A y - theta y) and of y.y, both at [j * gridDim.x + block]; multi_residual_scalars_kernel forms the quotients
struct LanczosTheta { double t[kMaxRhs]; };
template <typename TV, int K>
__global__ void __launch_bounds__(kBlock)
lanczos_residual_kernel(const TV *__restrict__ Y, const TV *__restrict__ AY, LanczosTheta theta, uint64_t n, double *__restrict__ partial_rr,
                        double *__restrict__ partial_yy)
{
    __shared__ double s_red[kWaves];
    double acc[K], accy[K];
#pragma unroll
    for (int j = 0; j < K; j++) acc[j] = accy[j] = 0.0;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
#pragma unroll
        for (int j = 0; j < K; j++) {
            const double yi = (double)Y[i * K + j];
            const double ri = __builtin_fma(-theta.t[j], yi, (double)AY[i * K + j]);
            acc[j] += ri * ri;
            accy[j] += yi * yi;
        }
    }
#pragma unroll
    for (int j = 0; j < K; j++) {
        const double t = block_sum(acc[j], s_red);
        const double ty = block_sum(accy[j], s_red);
        if (threadIdx.x == 0) {
            partial_rr[(size_t)j * gridDim.x + blockIdx.x] = t;
            partial_yy[(size_t)j * gridDim.x + blockIdx.x] = ty;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Deflated CG for the batch (lam_hip_set_deflation*, lam_hip_solve_many_deflated, lam_hip_deflate_many; host side: lam_deflate.h).
// The operator u_c -= Wa (M (Wd^T u_c)) on the K interleaved columns of a batched vector, as two launches on lanczos_dots_kernel's and
// lanczos_apply_kernel's plan:
//   deflate_dots_kernel    partial[block][i * K + c] of d_ic = Wd_i.u_c, i < m, c < K
//   deflate_apply_kernel   d from the partials in block order ; mu_c = M d_c (fp64, ascending index) ; u_c = fma(-(TV)mu_ic, Wa_i, u_c),
//                          i ascending ; START: u_c = the fma chain of +(TV)mu_ic Wa_i from 0 (the deflated start vector x0)
// The basis rows are the Lanczos basis' (row i at W + i * pitch); the vector is the batch's, element [row * K + c], so the VEC rows of
// one 16-byte load of a basis row meet K 16-byte loads of the vector.  A workgroup holds its slab of the vector in registers
// (deflate_hold<K>() 16-byte vectors of rows per thread and round, K times as many of the vector) and streams the basis rows past it.
// All sums are fp64 and of fixed order; no floating-point atomics; columns never mix: d_c, mu_c and the chain of column c read column c
// alone, so a NaN stays in its column.  sc (may be null): the batch's scalars -- both launches return on all_stop, and the apply launch
// leaves a stopped column's elements with the bits it loaded (it runs behind multi_p_kernel in stream order: the flags are final).
// ---------------------------------------------------------------------------------------------
constexpr int kDeflateSplit = 16;     // gridDim.y of deflate_dots_kernel, as kLanczosSplit
template <int K>
constexpr int deflate_hold() { return K == 1 ? 4 : (K == 2 ? 2 : 1); }

// the VEC * K elements of the K-interleaved x that belong to rows idx .. idx + VEC - 1 (idx a multiple of VEC): K 16-byte loads where
// the rows all lie in front of `end`, else the elements whose row does, and zeros
template <typename TV, int K>
__device__ __forceinline__ void deflate_load(const TV *__restrict__ x, uint64_t idx, uint64_t end, TV (&out)[16 / sizeof(TV) * K])
{
    constexpr int VEC = 16 / sizeof(TV);
    typedef TV vec_t __attribute__((ext_vector_type(VEC)));
    if (idx + VEC <= end) {
#pragma unroll
        for (int q = 0; q < K; q++) {
            const vec_t v = *reinterpret_cast<const vec_t *>(x + idx * K + q * VEC);
#pragma unroll
            for (int e = 0; e < VEC; e++) out[q * VEC + e] = v[e];
        }
    } else {
#pragma unroll
        for (int f = 0; f < VEC * K; f++) out[f] = idx + f / K < end ? x[idx * K + f] : (TV)0;
    }
}
template <typename TV, int K>
__device__ __forceinline__ void deflate_store(TV *__restrict__ x, uint64_t idx, uint64_t end, const TV (&in)[16 / sizeof(TV) * K])
{
    constexpr int VEC = 16 / sizeof(TV);
    typedef TV vec_t __attribute__((ext_vector_type(VEC)));
    if (idx + VEC <= end) {
#pragma unroll
        for (int q = 0; q < K; q++) {
            vec_t v;
#pragma unroll
            for (int e = 0; e < VEC; e++) v[e] = in[q * VEC + e];
            *reinterpret_cast<vec_t *>(x + idx * K + q * VEC) = v;
        }
    } else {
#pragma unroll
        for (int f = 0; f < VEC * K; f++)
            if (idx + f / K < end) x[idx * K + f] = in[f];
    }
}

// workgroup (x, y): slab x of the rows, basis rows i = y, y + gridDim.y, ... < m; partial[x * m * K + i * K + c]
template <typename TV, int K>
__global__ void __launch_bounds__(kBlock)
deflate_dots_kernel(const MultiScalars *sc, const TV *__restrict__ W, uint64_t pitch, int m, const TV *__restrict__ U, uint64_t n,
                    double *__restrict__ partial)
{
    constexpr int VEC = 16 / sizeof(TV), HOLD = deflate_hold<K>();
    __shared__ double s_acc[kMaxDeflation][K][kWaves];
    if (sc != nullptr && sc->all_stop) return;
    uint64_t first, end;
    lanczos_slab<TV>(n, &first, &end);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr uint64_t ROUND = (uint64_t)kBlock * VEC * HOLD;
    bool round0 = true;
    for (uint64_t base = first; round0 || base < end; base += ROUND) {
        TV ur[HOLD][VEC * K];
#pragma unroll
        for (int h = 0; h < HOLD; h++) deflate_load<TV, K>(U, base + ((uint64_t)h * kBlock + threadIdx.x) * VEC, end, ur[h]);
        for (int i = blockIdx.y; i < m; i += gridDim.y) {
            const TV *wi = W + (uint64_t)i * pitch;
            double a[K];
#pragma unroll
            for (int c = 0; c < K; c++) a[c] = 0.0;
#pragma unroll
            for (int h = 0; h < HOLD; h++) {
                TV vr[VEC];
                lanczos_load<TV>(wi, base + ((uint64_t)h * kBlock + threadIdx.x) * VEC, end, vr);
#pragma unroll
                for (int e = 0; e < VEC; e++)
#pragma unroll
                    for (int c = 0; c < K; c++) a[c] = __builtin_fma((double)vr[e], (double)ur[h][e * K + c], a[c]);
            }
#pragma unroll
            for (int c = 0; c < K; c++) {
                const double t = wave_sum(a[c]);
                if (lane == 0) s_acc[i][c][wave] = round0 ? t : s_acc[i][c][wave] + t;
            }
        }
        round0 = false;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < m * K; t += kBlock) {
        const int i = t / K, c = t % K;
        if (i % (int)gridDim.y != (int)blockIdx.y) continue;
        double s = s_acc[i][c][0];
#pragma unroll
        for (int w = 1; w < kWaves; w++) s += s_acc[i][c][w];
        partial[(size_t)blockIdx.x * m * K + t] = s;
    }
}

// M: m x m, row-major, fp64 (Ginv of the space, or the caller's).  coeff (may be null): d_ic in fp64 at coeff[i * ncoeff + c],
// c < ncoeff, by workgroup 0.  START: U is not read; the rows behind row n are zeroed in this K's layout (see multi_init_kernel).
template <typename TV, int K, bool START>
__global__ void __launch_bounds__(kBlock)
deflate_apply_kernel(const MultiScalars *sc, const double *__restrict__ partial, int nred, const double *__restrict__ M,
                     const TV *__restrict__ W, uint64_t pitch, int m, TV *__restrict__ U, uint64_t n, double *__restrict__ coeff, int ncoeff)
{
    constexpr int VEC = 16 / sizeof(TV), HOLD = deflate_hold<K>();
    __shared__ double s_d[kMaxDeflation * K];
    __shared__ TV s_mu[kMaxDeflation * K];
    if (sc != nullptr && sc->all_stop) return;
    const int npairs = m * K;
    for (int t = threadIdx.x; t < npairs; t += kBlock) {
        double a = 0.0;
        for (int b = 0; b < nred; b++) a += partial[(size_t)b * npairs + t];
        s_d[t] = a;
        if (coeff != nullptr && blockIdx.x == 0 && t % K < ncoeff) coeff[(size_t)(t / K) * ncoeff + t % K] = a;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < npairs; t += kBlock) {
        const int i = t / K, c = t % K;
        double mu = 0.0;
        for (int l = 0; l < m; l++) mu = __builtin_fma(M[(size_t)i * m + l], s_d[l * K + c], mu);
        s_mu[t] = START ? (TV)mu : -(TV)mu;
    }
    __syncthreads();
    bool run[K];
#pragma unroll
    for (int c = 0; c < K; c++) run[c] = sc == nullptr || sc->col[c].stop == 0;
    if constexpr (START)
        if (blockIdx.x == 0 && threadIdx.x < kMultiPadRows * K) U[n * K + threadIdx.x] = (TV)0;
    uint64_t first, end;
    lanczos_slab<TV>(n, &first, &end);
    constexpr uint64_t ROUND = (uint64_t)kBlock * VEC * HOLD;
    for (uint64_t base = first; base < end; base += ROUND) {
        TV ur[HOLD][VEC * K];
#pragma unroll
        for (int h = 0; h < HOLD; h++) {
            if constexpr (START) {
#pragma unroll
                for (int f = 0; f < VEC * K; f++) ur[h][f] = (TV)0;
            } else {
                deflate_load<TV, K>(U, base + ((uint64_t)h * kBlock + threadIdx.x) * VEC, end, ur[h]);
            }
        }
#pragma unroll 2
        for (int i = 0; i < m; i++) {
            const TV *wi = W + (uint64_t)i * pitch;
            TV mu[K];
#pragma unroll
            for (int c = 0; c < K; c++) mu[c] = s_mu[i * K + c];
#pragma unroll
            for (int h = 0; h < HOLD; h++) {
                TV vr[VEC];
                lanczos_load<TV>(wi, base + ((uint64_t)h * kBlock + threadIdx.x) * VEC, end, vr);
#pragma unroll
                for (int e = 0; e < VEC; e++)
#pragma unroll
                    for (int c = 0; c < K; c++)
                        ur[h][e * K + c] = run[c] ? fma_tv(mu[c], vr[e], ur[h][e * K + c]) : ur[h][e * K + c];
            }
        }
#pragma unroll
        for (int h = 0; h < HOLD; h++) deflate_store<TV, K>(U, base + ((uint64_t)h * kBlock + threadIdx.x) * VEC, end, ur[h]);
    }
}

// G[i * ldg + c] = the nred partials of (i, c) in block order, i < m, c < count: the columns of W^T (A W) one group of the product at
// a time (lam_hip_set_deflation*); one workgroup
template <int K>
__global__ void __launch_bounds__(kBlock)
deflate_gram_kernel(const double *__restrict__ partial, int nred, int m, int count, double *__restrict__ G, int ldg)
{
    const int npairs = m * K;
    for (int t = threadIdx.x; t < npairs; t += kBlock) {
        if (t % K >= count) continue;
        double a = 0.0;
        for (int b = 0; b < nred; b++) a += partial[(size_t)b * npairs + t];
        G[(size_t)(t / K) * ldg + t % K] = a;
    }
}

// basis rows (row j at rows + j * pitch) <-> the [n][K] interleaved vector of a group of `count` of them, padding columns zero
template <typename TV, int K>
__global__ void __launch_bounds__(kBlock)
deflate_gather_kernel(const TV *__restrict__ rows, uint64_t pitch, int count, TV *__restrict__ inter, uint64_t n)
{
    if (blockIdx.x == 0 && threadIdx.x < kMultiPadRows * K) inter[n * K + threadIdx.x] = (TV)0;      // see multi_init_kernel
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock)
#pragma unroll
        for (int j = 0; j < K; j++) inter[i * K + j] = j < count ? rows[(uint64_t)j * pitch + i] : (TV)0;
}
template <typename TV, int K>
__global__ void __launch_bounds__(kBlock)
deflate_scatter_kernel(const TV *__restrict__ inter, int count, TV *__restrict__ rows, uint64_t pitch, uint64_t n)
{
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock)
#pragma unroll
        for (int j = 0; j < K; j++)
            if (j < count) rows[(uint64_t)j * pitch + i] = inter[i * K + j];
}


// ---------------------------------------------------------------------------------------------
// Block CG for the batch (lam_hip_solve_block; host side: lam_block.h; the s x s matrices: lam_host_block.h; the recurrence,
// Dubrulle's BCGrQ with a Cholesky QR: include/lam_hip.h).  The s = nrhs live columns of the batch span ONE block Krylov space.
// Four launches per iteration: the batch's product Z = A P (multi_launch_gemv, untouched) and
//   block_gram_kernel   per-workgroup fp64 partials of the upper triangle of U^T V (H = P^T Z; the initial B^T B with U = V = B)
//   block_step_kernel   H from the partials, H = L D L^T, T = H^-1 ; X += P (T Phi) ; Q~ = Q - Z T ; partials of Q~^T Q~
//   block_dir_kernel    G from the partials ; rel_err_j = sqrt(Phi_j^T G Phi_j / bb_j) and the stop decision ; G = S^T S ;
//                       Q = Q~ S^-1 ; P = Q + P S^T ; Phi' = S Phi
// Vectors are the batch's (B, X, R as Q, P, AP as Z), K-interleaved; the padding columns c >= s are zero and never written.  One
// thread owns one row at a time (grid-stride): its K values of each vector are K * sizeof(TV) contiguous bytes (16-byte loads where
// a row has them), the s x s coefficient matrices are read from LDS at an address the whole wave shares, and the Gram kernels keep
// the K (K + 1) / 2 fp64 accumulators of the upper triangle (36 at K = 8) next to the one row -- VGPR and scratch use: DESIGN §17.
// Every workgroup sums the partials in the one fixed order of block_pair_sums and factors the s x s matrix itself (thread 0, in
// LDS), so all of them hold the same bits; no floating-point atomics.  The coefficients are rounded to the vector dtype once and
// every row's sums are fma chains in ascending column index.
// Scalars: BlockScalars.  Phi is a ring of two by iteration parity (iteration k reads slot (k + 1) & 1, workgroup 0 of
// block_dir_kernel writes slot k & 1), the other words have workgroup 0 of one launch as their only writer and reader.  all_stop:
// workgroup 0 may raise it inside the launch that also reads it, so every workgroup reads it ONCE (thread 0, handed on through LDS
// behind a barrier) and all its waves take the same branch -- the LDS sums of block_pair_sums need all four.  A workgroup that
// meets the raised flag returns, which is what it decides itself from the same bits; one that does not decides so on its own.  A
// breakdown raises all_stop too and posts "stopped" to the progress word.
// ---------------------------------------------------------------------------------------------
struct BlockScalars : MultiScalars {     // the prefix: what the product reads (all_stop); col[] is not used
    double phi[2][kMaxRhs * kMaxRhs];     // s x s, leading dimension s: R = Q Phi
    double bb[kMaxRhs];                   // b_j.b_j
    double rel_err[kMaxRhs];              // of the last completed iteration
    int first_hit[kMaxRhs];               // first iteration at which column j met the stop test (0: never)
    int iters;                            // last completed iteration
    int bd_iter, bd_kind, bd_col;         // breakdown: iteration (0: none), 1 = H's pivot, 2 = G's pivot, the column of the pivot
};

template <int K> constexpr int block_pairs() { return K * (K + 1) / 2; }

// the K values of row i of a K-interleaved vector
template <typename TV, int K>
__device__ __forceinline__ void block_load_row(const TV *__restrict__ x, uint64_t i, TV (&out)[K])
{
    constexpr int VEC = 16 / sizeof(TV);
    if constexpr (K % VEC == 0) {
        typedef TV vec_t __attribute__((ext_vector_type(VEC)));
#pragma unroll
        for (int q = 0; q < K / VEC; q++) {
            const vec_t v = *reinterpret_cast<const vec_t *>(x + i * K + q * VEC);
#pragma unroll
            for (int e = 0; e < VEC; e++) out[q * VEC + e] = v[e];
        }
    } else {
#pragma unroll
        for (int j = 0; j < K; j++) out[j] = x[i * K + j];
    }
}
template <typename TV, int K>
__device__ __forceinline__ void block_store_row(TV *__restrict__ x, uint64_t i, const TV (&in)[K])
{
    constexpr int VEC = 16 / sizeof(TV);
    if constexpr (K % VEC == 0) {
        typedef TV vec_t __attribute__((ext_vector_type(VEC)));
#pragma unroll
        for (int q = 0; q < K / VEC; q++) {
            vec_t v;
#pragma unroll
            for (int e = 0; e < VEC; e++) v[e] = in[q * VEC + e];
            *reinterpret_cast<vec_t *>(x + i * K + q * VEC) = v;
        }
    } else {
#pragma unroll
        for (int j = 0; j < K; j++) x[i * K + j] = in[j];
    }
}

// acc[pair(i, j)] += u_i v_j for i <= j < K, pairs in row-major order of the upper triangle
template <typename TV, int K>
__device__ __forceinline__ void block_gram_row(const TV (&u)[K], const TV (&v)[K], double (&acc)[K * (K + 1) / 2])
{
    int t = 0;
#pragma unroll
    for (int i = 0; i < K; i++)
#pragma unroll
        for (int j = i; j < K; j++, t++) acc[t] = __builtin_fma((double)u[i], (double)v[j], acc[t]);
}

// the workgroup's totals of the accumulators, in fixed order, to partial[block * NP + pair]
template <int K>
__device__ __forceinline__ void block_gram_flush(const double (&acc)[K * (K + 1) / 2], double (*s_acc)[kWaves], double *__restrict__ partial)
{
    constexpr int NP = block_pairs<K>();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int t = 0; t < NP; t++) {
        const double w = wave_sum(acc[t]);
        if (lane == 0) s_acc[t][wave] = w;
    }
    __syncthreads();
    if (threadIdx.x < NP) {
        double a = s_acc[threadIdx.x][0];
#pragma unroll
        for (int w = 1; w < kWaves; w++) a += s_acc[threadIdx.x][w];
        partial[(size_t)blockIdx.x * NP + threadIdx.x] = a;
    }
}

// s_full[i * s + j] = s_full[j * s + i] = the nred partials of pair (i, j), i <= j < s: wave w sums the workgroups w, w + 4, ... in
// ascending order (lane = pair, so a load is one contiguous run), then the four in ascending order.  The same bits in every workgroup.
template <int K>
__device__ __forceinline__ void block_pair_sums(const double *__restrict__ partial, int nred, int s, double (*s_acc)[kWaves],
                                                double *s_full)
{
    constexpr int NP = block_pairs<K>();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane < NP) {
        double a = 0.0;
#pragma unroll 4
        for (int b = wave; b < nred; b += kWaves) a += partial[(size_t)b * NP + lane];
        s_acc[lane][wave] = a;
    }
    __syncthreads();
    if (threadIdx.x < NP) {
        double a = s_acc[threadIdx.x][0];
#pragma unroll
        for (int w = 1; w < kWaves; w++) a += s_acc[threadIdx.x][w];
        // pair index -> (i, j) of the K-wide upper triangle
        int i = 0, t = threadIdx.x;
        while (t >= K - i) { t -= K - i; i++; }
        const int j = i + t;
        if (j < s) s_full[i * s + j] = s_full[j * s + i] = a;
    }
    __syncthreads();
}

template <typename TV, int K>
__global__ void __launch_bounds__(kBlock)
block_gram_kernel(const MultiScalars *sc, const TV *__restrict__ U, const TV *__restrict__ V, uint64_t n, double *__restrict__ partial)
{
    constexpr int NP = block_pairs<K>();
    __shared__ double s_acc[NP][kWaves];
    __shared__ int s_stop;
    if (threadIdx.x == 0) s_stop = sc != nullptr && sc->all_stop;
    __syncthreads();
    if (s_stop) return;
    double acc[NP];
#pragma unroll
    for (int t = 0; t < NP; t++) acc[t] = 0.0;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        TV u[K], v[K];
        block_load_row<TV, K>(U, i, u);
        block_load_row<TV, K>(V, i, v);
        block_gram_row<TV, K>(u, v, acc);
    }
    block_gram_flush<K>(acc, s_acc, partial);
}

// by-value s x s matrix (leading dimension s) of block_init_kernel
struct BlockMat { double a[kMaxRhs * kMaxRhs]; };

// Q = B C^-1 (fma chain from 0, i ascending, i <= j: C^-1 is upper triangular), P = Q, X = 0 for the s live columns; the padding
// columns of all three and the rows behind row n of P are zeroed in this K's layout (see multi_init_kernel).  Workgroup 0 sets the
// scalars: Phi = C, bb, rel_err = 1 (R = B).
template <typename TV, int K>
__global__ void __launch_bounds__(kBlock)
block_init_kernel(const TV *__restrict__ B, TV *__restrict__ X, TV *__restrict__ Q, TV *__restrict__ P, uint64_t n, int s, BlockMat C,
                  BlockMat Cinv, BlockMat bb, BlockScalars *sc, volatile int *host_flags)
{
    __shared__ TV s_ci[K * K];
    for (int t = threadIdx.x; t < K * K; t += kBlock) {
        const int i = t / K, j = t % K;
        s_ci[t] = i < s && j < s ? (TV)Cinv.a[i * s + j] : (TV)0;
    }
    if (blockIdx.x == 0) {
        for (int t = threadIdx.x; t < kMaxRhs * kMaxRhs; t += kBlock) {
            sc->phi[0][t] = t < s * s ? C.a[t] : 0.0;
            sc->phi[1][t] = 0.0;
        }
        if (threadIdx.x < kMaxRhs) {
            const int j = threadIdx.x;
            sc->bb[j] = j < s ? bb.a[j] : 0.0;
            sc->rel_err[j] = j < s ? 1.0 : 0.0;
            sc->first_hit[j] = 0;
            CgScalars &c = sc->col[j];
            c.bb = j < s ? bb.a[j] : 0.0; c.rr[0] = c.rr[1] = 0.0; c.pAp = 0.0; c.alpha = 0.0; c.beta = 0.0; c.iters = 0; c.stop = 0;
        }
        if (threadIdx.x == 0) {
            sc->all_stop = 0; sc->pad = 0; sc->iters = 0;
            sc->bd_iter = 0; sc->bd_kind = 0; sc->bd_col = -1;
            post_progress(host_flags, 0, false);
        }
        if (threadIdx.x < kMultiPadRows * K) P[n * K + threadIdx.x] = (TV)0;
    }
    __syncthreads();
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        TV b[K], q[K], zero[K];
        block_load_row<TV, K>(B, i, b);
#pragma unroll
        for (int j = 0; j < K; j++) {
            TV a = (TV)0;
            if (j < s) {
#pragma unroll
                for (int l = 0; l <= j; l++) a = fma_tv(b[l], s_ci[l * K + j], a);
            }
            q[j] = a;
            zero[j] = (TV)0;
        }
        block_store_row<TV, K>(Q, i, q);
        block_store_row<TV, K>(P, i, q);
        block_store_row<TV, K>(X, i, zero);
    }
}

template <typename TV, int K>
__global__ void __launch_bounds__(kBlock)
block_step_kernel(const double *__restrict__ part_h, int nred, BlockScalars *sc, int k, int s, const TV *__restrict__ P,
                  const TV *__restrict__ Z, TV *__restrict__ X, TV *__restrict__ Q, uint64_t n, double *__restrict__ part_g,
                  volatile int *host_flags)
{
    constexpr int NP = block_pairs<K>();
    constexpr bool F32 = sizeof(TV) == 4;
    __shared__ double s_acc[NP][kWaves];
    __shared__ double s_h[K * K], s_l[K * K], s_d[K], s_t[K * K];
    __shared__ TV s_ct[K * K], s_cx[K * K];         // -T and T Phi, K-wide, zero outside s x s
    __shared__ int s_bad, s_stop;
    if (threadIdx.x == 0) s_stop = sc->all_stop;       // one read per workgroup: its waves must not part on a flag raised meanwhile
    __syncthreads();
    if (s_stop) return;
    block_pair_sums<K>(part_h, nred, s, s_acc, s_h);
    if (threadIdx.x == 0) {
        int bad;
        block_ldlt_inverse(s, s_h, block_pivot_floor(s, F32, s_h), s_l, s_d, s_t, &bad);
        s_bad = bad;
    }
    __syncthreads();
    if (s_bad >= 0) {                               // breakdown kind 1: X stays iterate k - 1
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            sc->bd_iter = k; sc->bd_kind = 1; sc->bd_col = s_bad;
            sc->all_stop = 1;
            post_progress(host_flags, k, true);
        }
        return;
    }
    const double *phi = sc->phi[(k + 1) & 1];
    for (int t = threadIdx.x; t < K * K; t += kBlock) {
        const int i = t / K, j = t % K;
        double cx = 0.0, ct = 0.0;
        if (i < s && j < s) {
            for (int l = 0; l < s; l++) cx = __builtin_fma(s_t[i * s + l], phi[l * s + j], cx);
            ct = -s_t[i * s + j];
        }
        s_cx[t] = (TV)cx;
        s_ct[t] = (TV)ct;
    }
    __syncthreads();
    double acc[NP];
#pragma unroll
    for (int t = 0; t < NP; t++) acc[t] = 0.0;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        TV p[K], z[K], x[K], q[K];
        block_load_row<TV, K>(P, i, p);
        block_load_row<TV, K>(Z, i, z);
        block_load_row<TV, K>(X, i, x);
        block_load_row<TV, K>(Q, i, q);
#pragma unroll
        for (int j = 0; j < K; j++) {
            if (j >= s) continue;
            TV xj = x[j], qj = q[j];
#pragma unroll
            for (int l = 0; l < K; l++) {
                if (l >= s) continue;
                xj = fma_tv(p[l], s_cx[l * K + j], xj);
                qj = fma_tv(z[l], s_ct[l * K + j], qj);
            }
            x[j] = xj;
            q[j] = qj;
        }
        block_store_row<TV, K>(X, i, x);
        block_store_row<TV, K>(Q, i, q);
        block_gram_row<TV, K>(q, q, acc);
    }
    block_gram_flush<K>(acc, s_acc, part_g);
}

template <typename TV, int K>
__global__ void __launch_bounds__(kBlock)
block_dir_kernel(const double *__restrict__ part_g, int nred, BlockScalars *sc, int k, int s, double rel_error, TV *__restrict__ Q,
                 TV *__restrict__ P, uint64_t n, volatile int *host_flags)
{
    constexpr int NP = block_pairs<K>();
    constexpr bool F32 = sizeof(TV) == 4;
    __shared__ double s_acc[NP][kWaves];
    __shared__ double s_g[K * K], s_s[K * K], s_si[K * K], s_rel[K];
    __shared__ TV s_cs[K * K], s_ci[K * K];         // S and S^-1, K-wide, zero outside s x s
    __shared__ int s_bad, s_stop;
    if (threadIdx.x == 0) s_stop = sc->all_stop;       // as in block_step_kernel
    __syncthreads();
    if (s_stop) return;
    block_pair_sums<K>(part_g, nred, s, s_acc, s_g);
    const double *phi = sc->phi[(k + 1) & 1];
    if (threadIdx.x < s) {
        // Phi_j^T G Phi_j = ||r_j||^2 (R = Q~ Phi); Phi is upper triangular, so rows 0 .. j of column j
        const int j = threadIdx.x;
        double v = 0.0;
        for (int a = 0; a <= j; a++) {
            double w = 0.0;
            for (int b = 0; b <= j; b++) w = __builtin_fma(s_g[a * s + b], phi[b * s + j], w);
            v = __builtin_fma(phi[a * s + j], w, v);
        }
        if (v < 0.0) v = 0.0;                       // rounding of a vanishing residual; a NaN stays one
        s_rel[j] = sqrt(v / sc->bb[j]);
    }
    __syncthreads();
    bool all = true;
    for (int j = 0; j < s; j++) all = all && s_rel[j] < rel_error;
    if (threadIdx.x == 0) {
        int bad = -1;
        if (!all) block_upper(s, s_g, block_pivot_floor(s, F32, s_g), s_s, s_si, &bad);
        s_bad = bad;
    }
    __syncthreads();
    const bool broke = s_bad >= 0;                  // breakdown kind 2: X is iterate k, and valid
    if (blockIdx.x == 0) {
        if (threadIdx.x < s) {
            const int j = threadIdx.x;
            sc->rel_err[j] = s_rel[j];
            if (s_rel[j] < rel_error && sc->first_hit[j] == 0) sc->first_hit[j] = k;
        }
        if (!all && !broke) {
            double *out = sc->phi[k & 1];
            for (int t = threadIdx.x; t < s * s; t += kBlock) {
                const int i = t / s, j = t % s;
                double v = 0.0;
                for (int l = i; l <= j; l++) v = __builtin_fma(s_s[i * s + l], phi[l * s + j], v);
                out[t] = v;
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            sc->iters = k;
            if (broke) { sc->bd_iter = k; sc->bd_kind = 2; sc->bd_col = s_bad; }
            if (all || broke) sc->all_stop = 1;
            post_progress(host_flags, k, all || broke);
        }
    }
    if (all || broke) return;
    for (int t = threadIdx.x; t < K * K; t += kBlock) {
        const int i = t / K, j = t % K;
        const bool in = i < s && j < s;
        s_cs[t] = in ? (TV)s_s[i * s + j] : (TV)0;
        s_ci[t] = in ? (TV)s_si[i * s + j] : (TV)0;
    }
    __syncthreads();
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        TV qt[K], p[K], q[K], pn[K];
        block_load_row<TV, K>(Q, i, qt);
        block_load_row<TV, K>(P, i, p);
#pragma unroll
        for (int j = 0; j < K; j++) {
            q[j] = qt[j];
            pn[j] = p[j];
            if (j >= s) continue;
            TV a = (TV)0;
#pragma unroll
            for (int l = 0; l <= j; l++) a = fma_tv(qt[l], s_ci[l * K + j], a);
            q[j] = a;
            // (P S^T)_j = sum_{l >= j} p_l S_jl
#pragma unroll
            for (int l = j; l < K; l++) {
                if (l >= s) continue;
                a = fma_tv(p[l], s_cs[j * K + l], a);
            }
            pn[j] = a;
        }
        block_store_row<TV, K>(Q, i, q);
        block_store_row<TV, K>(P, i, pn);
    }
}


// ---------------------------------------------------------------------------------------------
// The diagonal of the matrix: lam_hip_get_diagonal, and dinv of the preconditioned batch (PC above).
// ---------------------------------------------------------------------------------------------
// what the extraction found wrong with the diagonal: rows whose A_ii or 1/A_ii is not finite and > 0
struct DiagInfo {
    unsigned long long first_bad; // smallest such GLOBAL row (~0: none)
    unsigned long long count;
};

// diag[i] = A[i][row0 + i] of the shard's rows (vector dtype: bf16 storage widened to float, exactly), dinv[i] = 1 / A_ii computed
// in fp64 from the stored value and rounded to the vector dtype; either output may be null.  info (may be null): integer atomics
// only, so the result does not depend on the order the workgroups run in.
template <typename TA, typename TV>
__global__ void __launch_bounds__(kBlock)
diag_extract_kernel(const TA *__restrict__ A, uint64_t lda, uint64_t row0, uint64_t nrows, TV *__restrict__ diag, TV *__restrict__ dinv,
                    DiagInfo *info)
{
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < nrows; i += (uint64_t)gridDim.x * kBlock) {
        const TV a = widen<TV>(A[i * lda + row0 + i]);
        const TV inv = (TV)(1.0 / (double)a);
        if (diag != nullptr) diag[i] = a;
        if (dinv != nullptr) dinv[i] = inv;
        const bool ok = a > (TV)0 && a <= std::numeric_limits<TV>::max() && inv > (TV)0 && inv <= std::numeric_limits<TV>::max();
        if (!ok && info != nullptr) {
            atomicMin(&info->first_bad, (unsigned long long)(row0 + i));
            atomicAdd(&info->count, 1ull);
        }
    }
}


// by-value shifts of shifted_dinv_kernel, fp64 as the host keeps them (each exactly a value of the vector dtype)
struct ShiftList { double s[kMaxRhs]; };

// The Jacobi preconditioner of the shifted batch, M_j = diag(A) + s_j I: dinv[i * K + j] = 1 / ((double)A_ii + s_j), computed in fp64
// and rounded to the vector dtype, for the nrhs live columns; the padding columns get 0 (their b, r and p are zero and stay so).
// The scan is diag_extract_kernel's, on the SUM: info->first_bad is the smallest i * K + j whose sum or reciprocal is not finite and
// > 0 in the vector dtype, so a zero on A's own diagonal passes where the shift lifts it.
template <typename TA, typename TV, int K>
__global__ void __launch_bounds__(kBlock)
shifted_dinv_kernel(const TA *__restrict__ A, uint64_t lda, uint64_t nrows, int nrhs, ShiftList shift, TV *__restrict__ dinv,
                    DiagInfo *info)
{
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < nrows; i += (uint64_t)gridDim.x * kBlock) {
        const double a = (double)widen<TV>(A[i * lda + i]);
#pragma unroll
        for (int j = 0; j < K; j++) {
            if (j >= nrhs) { dinv[i * K + j] = (TV)0; continue; }
            const TV m = (TV)(a + shift.s[j]);
            const TV inv = (TV)(1.0 / (a + shift.s[j]));
            dinv[i * K + j] = inv;
            const bool ok = m > (TV)0 && m <= std::numeric_limits<TV>::max() && inv > (TV)0 && inv <= std::numeric_limits<TV>::max();
            if (!ok) {
                atomicMin(&info->first_bad, (unsigned long long)(i * K + j));
                atomicAdd(&info->count, 1ull);
            }
        }
    }
}

}  // namespace lam
