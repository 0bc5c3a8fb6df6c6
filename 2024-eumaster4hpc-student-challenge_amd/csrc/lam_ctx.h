// lam_ctx.h -- shard and context state, error plumbing and small host helpers of the MI355X-native dense CG hot path.
// Part of the one translation unit csrc/lam_hip.hip (included from there, in order; not a stand-alone header).
#pragma once

namespace {

thread_local std::string g_create_error;

double now_s()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

uint64_t thread_cpu_ns()
{
    struct timespec ts;
    if (clock_gettime(CLOCK_THREAD_CPUTIME_ID, &ts) != 0) return 0;
    return (uint64_t)ts.tv_sec * 1000000000ull + (uint64_t)ts.tv_nsec;
}

constexpr int kLag = 4;          // iterations the host may run ahead of the stop flag
// Default exchange of new contexts, ONE LINE EACH to flip once a run on separate GPUs has priced the collectives (bench.py records
// every exchange of both topologies under exchange_modes).  Gather-Ap in both since round 5: one collective / one event join per
// iteration instead of three, two launches instead of three, everything on one stream -- 620 + L' against 644 + 2 L us per iteration
// at P = 8 by the one-GPU model, 3 x the iteration rate on the stream-ordered RCCL double.
constexpr int64_t kRankModeDefaultExchange = 1;      // lam_hip_create_rank (round 4: 0)
constexpr int64_t kOneProcessDefaultExchange = 1;    // lam_hip_create with several shards
constexpr int kVecBlocksMax = 256;

// A plan of the symmetric product (lam_host_plan.h, symv_plan) on the device with the partials of its two passes (symv_dev_build
// below): one per shard for the single product (ShardBase::symv), the batch's own (MultiState::sym).
struct SymvDevPlan {
    SymvTask *tasks = nullptr;            // null: not built
    uint32_t *index = nullptr;            // what the second pass needs to find the partials (lam_host_plan.h, SymvIndex)
    SymvIndex ix = {};
    int ntasks = 0;
    uint64_t rowpart_elems = 0;           // row partials per column of p
    void *rowpart = nullptr, *colpart = nullptr;
};

struct ShardBase {
    int dev = 0;
    int index = 0;               // global shard index
    uint64_t row0 = 0, nrows = 0;
    hipStream_t stream = nullptr;
    void *A = nullptr;           // nrows x n
    size_t A_capacity = 0;       // bytes behind A: the allocation is kept across lam_hip_set_problem calls (grow-only)
    void *xfer_stage = nullptr;  // dense staging buffer of padded / bf16 row transfers (lam_hip_upload_rows / download_rows): kept
    size_t xfer_stage_bytes = 0; // for the life of the context, grow-only -- a hipMalloc + hipFree of up to 1 GiB per chunk of a file
                                 // load was a device-wide synchronisation each and left VRAM for the driver to wipe under the next kernels
    void *p = nullptr;           // n (replica)
    void *Ap = nullptr, *x = nullptr, *r = nullptr, *b = nullptr;  // nrows each
    void *tmp = nullptr;         // n: scratch vector (gemv op input / residual)
    void *r_full = nullptr;      // n: replicated r (gather-Ap exchange only)
    void *ap_gather = nullptr;   // P records [Ap slice | double]: gather-Ap exchange only.  One process with several shards:
                                 // TWO such buffers back to back (iteration parity), because there the producers store into
                                 // their peers' buffers themselves and a shard may start the next GEMV while a slower peer is
                                 // still reading this iteration's records (ap_gather_bytes = one buffer)
    size_t ap_gather_bytes = 0;
    SymvDevPlan symv;                     // symmetric product (option "symmetric"): the shard's plan and partials, built at first use
    void *symv_gather = nullptr;          // several shards: P records [full-length contribution to A p | double], double-buffered
                                          // like ap_gather in one process (symv_gather_bytes = one buffer)
    size_t symv_gather_bytes = 0;
    double *part_gemv = nullptr; // [gemv_blocks]
    double *part_vec = nullptr;  // [vec_blocks]
    double *gather_a = nullptr;  // [kMaxShards] p.Ap partials of all shards (or the reduced scalar at [0])
    double *gather_b = nullptr;  // [kMaxShards] r.r partials
    double *part_aux = nullptr;  // [kVecBlocksMax] partials of the checks outside the iteration (true residual)
    int part_gemv_cap = 0;       // entries allocated behind part_gemv
    CgScalars *sc = nullptr;     // device scalars
    CgScalars *sc_host = nullptr;// pinned mirror (filled by an async copy at the end of a call)
    int *host_flags = nullptr;   // pinned, device-visible progress word (lam_kernels.h, post_progress): low half = last
                                 // finished iteration, high half = the stopping iteration (0 = none)
    int gemv_blocks = 0, vec_blocks = 0;
    hipStream_t comm_stream = nullptr;                          // rank mode: the all-gather of p runs here
    hipEvent_t ev_a = nullptr, ev_b = nullptr, ev_p = nullptr;  // cross-shard ordering
    hipEvent_t ev_gathered = nullptr;                           // all-gather on comm_stream finished
    hipEvent_t ev_g0[kLag] = {}, ev_g1[kLag] = {};              // gemv timing ring (whole GEMV, or its first panel)
    hipEvent_t ev_g2[kLag] = {}, ev_g3[kLag] = {};              // second panel of a split GEMV
    bool split_slot[kLag] = {};
    bool timed_slot[kLag] = {};                                 // the slot's iteration recorded its timing events
    hipEvent_t ev_x[kLag][6] = {};                              // exchange timing ring (shard 0): up to three begin / end pairs per timed
    int nx[kLag] = {};                                          // iteration -- one per exchange step (lam_exchange.h, xt_begin / xt_end)
    // in-launch hand-over / direct exchange (lam_kernels.h, Mail): the shard's mailbox (fine-grained device memory where
    // the runtime offers it), the broadcast lines of its fused update launch, and the iteration whose fused launch has
    // already waited for the peers' p slices.  Kept for the life of the context.
    Mail *mail = nullptr;
    bool mail_coarse = false;
    BcastLine *bcast = nullptr;
    int waited_k = 0;
};

// Several right-hand sides (lam_hip_solve_many, lam_multi.h): state of its own, next to the single-vector state of the shard and
// independent of it.  Allocated at the first batched call for LAM_HIP_MAX_RHS columns (5 vectors of 8 n elements: 21 MB at
// n = 65536 in fp64, next to a 34 GB matrix), so it only ever grows with n; released by lam_hip_destroy and by a
// lam_hip_set_problem that changes n.  All vectors are interleaved [n][K] (lam_kernels.h, "Several right-hand sides").
// Multi-shift CG (lam_hip_solve_mshift): x and p of every shift in groups of 8, [n + 16][8] per group, and the per-shift scalars.
// Allocated at the first multi-shift call for the groups it needs, grow-only, released with the batch (multi_release).
struct MshiftState {
    void *XS = nullptr, *PS = nullptr;
    int groups_cap = 0;          // groups XS / PS hold
    MshiftScalars *sc = nullptr; // device
    int nshifts = 0;             // of the last solve
    double shift[kMaxShifts] = {};    // absolute, each exactly a value of the vector dtype
    bool valid = false;          // the multi-shift solution is readable: cleared by whatever clears or replaces the batch's
};

// lam_hip_solve_many_minres: what MINRES needs beyond the batch's own vectors (its v is the batch's P, u its AP, v_old its R).
// Allocated by the first MINRES call for the batch's n (minres_ensure), released with the batch (multi_release).
struct MinresState {
    void *W = nullptr, *WOLD = nullptr;      // (n + 16) * kMaxRhs elements each
    MinresScalars *sc = nullptr;             // device; the last of the three to be allocated: set means all are
};

// lam_hip_eigs (lam_eigs.h): the Lanczos basis, u, the Ritz vectors and the scalars, next to the batch's vectors and independent of
// its right-hand sides and shifts.  Allocated by the first call for the batch's n, grow-only in max_steps (cap), released with the
// batch (multi_release).  What the host keeps of the last run is what the getters serve.
struct LanczosState {
    void *V = nullptr;           // (cap + 1) rows of `pitch` elements, zero behind element n of every row
    void *U = nullptr;           // n elements (+ padding)
    void *Y = nullptr;           // cap Ritz vectors of n elements, pair i contiguous at i * n
    double *part = nullptr;      // [cap + 1][kVecBlocksMax] partials of the projection's dots
    double *part_uu = nullptr;   // [kVecBlocksMax] partials of u.u (and of v0.v0)
    double *S = nullptr;         // device, cap * cap: the wanted columns of the tridiagonal's eigenvector matrix
    LanczosScalars *sc = nullptr;// device; the last to be allocated: set means all are
    int cap = 0;
    uint64_t pitch = 0;          // elements between basis rows
    bool valid = false;          // an eigen-solution is readable
    int steps = 0, nfound = 0;   // of the last run
    std::vector<double> alpha, beta, theta;   // alpha[steps], beta[steps]; theta[nfound] in the order `which` asked for
};

// lam_hip_set_deflation* (lam_deflate.h): the deflation space W of lam_hip_solve_many_deflated, A W and the inverse of W^T A W, next to
// the batch's vectors.  2 * m * pitch elements, built aside and swapped in by a successful call only (a refused call leaves the previous
// space), released with the batch (multi_release).  The space belongs to the matrix content: gen follows lam_hip_ctx::matrix_gen.
struct DeflateState {
    void *W = nullptr, *AW = nullptr;    // m rows of `pitch` elements each, zero behind element n of every row
    double *Ginv = nullptr;      // device, m x m: (W^T A W)^-1, symmetric
    double *part = nullptr;      // [kVecBlocksMax / 4][kMaxDeflation * kMaxRhs] partials of the dots; kept across spaces
    int m = 0;                   // 0: no space
    uint64_t pitch = 0;
    uint64_t gen = ~0ull;        // matrix_gen the space was built on
};

// lam_hip_solve_block (lam_block.h): the scalars and the two sets of Gram partials of block CG; its vectors are the batch's own.
// Allocated by the first call for the batch's n, released with the batch (multi_release).
struct BlockState {
    double *part_h = nullptr, *part_g = nullptr;     // [kVecBlocksMax][36]: upper triangles of P^T Z and of Q~^T Q~ per workgroup
    BlockScalars *sc = nullptr;  // device; the last of the three to be allocated: set means all are
};

// lam_hip_lanczos_many (lam_quad.h): the device block of the batched Lanczos quadrature (scalars and the coefficient history of one
// group), allocated by the first call for the batch's n and released with the batch (multi_release); its vectors are the batch's own.
// What the host keeps of the last run is what lam_hip_get_lanczos_many and lam_hip_trace_quadrature serve: host data, which no other
// batch call touches.
struct QuadState {
    QuadScalars *sc = nullptr;   // device
    bool valid = false;          // the coefficients are readable: cleared by a new matrix content and by lam_hip_set_problem
    int nprobes = 0, steps = 0;  // of the last run
    std::vector<int32_t> steps_run;           // [nprobes]
    std::vector<double> znorm2, alpha, beta;  // [nprobes]; [nprobes][steps] each, NaN past steps_run
};

struct MultiState {
    LanczosState lz;
    DeflateState df;
    BlockState bk;
    QuadState qd;
    uint64_t n = 0;             // the problem size the buffers were allocated for (0: none)
    void *B = nullptr, *X = nullptr, *R = nullptr, *P = nullptr, *AP = nullptr;   // (n + 16) * kMaxRhs elements; P zero behind n
    void *stage = nullptr;       // n * kMaxRhs elements: the host interface's layout (column j contiguous) on its way in or out
    double *part_gemv = nullptr; // [kMaxRhs][n]: p_j.Ap_j partials per product workgroup
    double *part_vec = nullptr;  // [kMaxRhs][kVecBlocksMax]
    double *part_rr = nullptr;   // [kMaxRhs][kVecBlocksMax]: r0.r0 of a start from a guess, r.r of lam_hip_true_residual_many
    double *res = nullptr;       // [kMaxRhs]: lam_hip_true_residual_many's quotients on their way to the host
    BatchScalars *sc = nullptr;  // device; every solve re-initialises it in its init launch
    MultiScalars *sc_host = nullptr;                  // pinned mirror of its MultiScalars prefix
    int *host_flags = nullptr;   // pinned progress word of the batch (post_progress)
    hipEvent_t ev0[kLag] = {}, ev1[kLag] = {};        // product timing ring
    bool timed_slot[kLag] = {};
    int nrhs = 0, K = 0;         // right-hand sides set / instantiation they are stored for
    bool have_rhs = false, solved = false;
    int last_K = 0;              // option "multi_rhs_k": the K the last batched call ran
    // lam_hip_set_shifts_many: column j is the system (A + shift[j] I) x_j = b_j.  Each value is exactly a value of the vector dtype;
    // shifted == some shift[j] != 0, and only then do the SHIFT instantiations run.  Cleared with the right-hand sides.
    // Negative values come from lam_hip_solve_many_minres alone, and the CG entry points refuse to run under them.
    double shift[kMaxRhs] = {};
    bool shifted = false;
    MshiftState ms;
    MinresState mr;
    // symmetric batched product (option "symmetric_many", multi_sym_ensure): the batch's own plan and partials, nothing shared with
    // ShardBase::symv.  The plan is built at first use for the batch's n and the storage's vector width (sym_vec); the partials are
    // K-wide records and grow-only in K (sym_cap_K); released with the batch.
    SymvDevPlan sym;
    int sym_vec = 0, sym_cap_K = 0;
};

// Jacobi preconditioner of the batched solve (lam_hip_solve_many_pc, lam_multi.h): the diagonal of the matrix and its reciprocal,
// extracted on the device once per matrix content (diag_gen follows lam_hip_ctx::matrix_gen, as sym_checked_gen does), and the r.z
// partials.  Allocated by the first preconditioned solve (pcg_ensure) for the batch's n; lives and dies with MultiState (multi_release).
struct PcgState {
    void *diag = nullptr, *dinv = nullptr;   // n elements of the vector dtype each
    double *part_rz = nullptr;   // [kMaxRhs][kVecBlocksMax]
    DiagInfo *info = nullptr;    // device; the last of the four to be allocated: set means all are
    uint64_t diag_gen = ~0ull;   // matrix_gen the diagonal was extracted from
    uint64_t bad_count = 0, bad_row = 0;     // what that extraction found (bad_count == 0: usable)
    double bad_value = 0.0;
    // the shifted batch's K-wide reciprocal, dinv_k[i * K + j] = 1 / (A_ii + shift[j]) (shifted_dinv_kernel): built once per
    // (matrix content, K, nrhs, shifts), which is the key below; kMaxRhs * n elements, allocated by the first shifted Jacobi solve
    void *dinv_k = nullptr;
    uint64_t dinvk_gen = ~0ull;
    int dinvk_K = 0, dinvk_nrhs = 0;
    double dinvk_shift[kMaxRhs] = {};
    uint64_t badk_count = 0, badk_row = 0;
    int badk_col = 0;
    double badk_value = 0.0;
};

// Packed fp64 image of the matrix (options "packed" and "packed_many", lam_host_pack.h): what gemv_packed_kernel and
// multi_gemv_packed_kernel read in place of A.  One allocation,
// grow-only, kept for the life of the context (a large hipFree slows whatever runs next); its content follows
// lam_hip_ctx::matrix_gen, as sym_checked_gen and PcgState::diag_gen do.  A stays where it is: every other path reads it as before.
// Auto packs once a content has served kPackAfter plain products: the measured break-even, pack time / (plain - packed product time),
// at N = 65536 (15.7 ms / 0.244 ms = 64.4) rounded up; 68.7 at N = 32768, 134 at N = 40000 (profiles/packed_parent_vs_branch.txt).
// From kPackMinBytes of matrix on: N = 32768 (8 GiB) runs 1.050 x the plain kernel, 40000 1.024 x, 65536 1.053 x; N = 20000
// 0.998 x and N = 10000 0.85 x (three tiles of which the last holds 1808 columns, and too few workgroups to hide the decode).
constexpr int kPackAfter = 65;
constexpr uint64_t kPackMinBytes = 8ull << 30;
struct PackState {
    void *buf = nullptr;
    size_t cap = 0;
    uint64_t nrows = 0, ntiles = 0;      // of the image in buf
    uint64_t ready_gen = ~0ull;          // matrix_gen the image holds
    uint64_t refused_gen = ~0ull;        // matrix_gen that is not packable (a tile overflowed) or found no memory: not tried again
    uint64_t count_gen = ~0ull;          // matrix_gen `plain` counts for
    uint64_t plain = 0;                  // plain products of an eligible shape, single or batched (K <= 4), since the content changed
    uint64_t exc_total = 0;              // exception-list values a product reads of the whole image (8 bytes each)
    double pack_s = 0.0;                 // seconds the last pack took (host clock around the pass)
};

}  // namespace

struct lam_hip_ctx {
    MultiState multi;
    PcgState pcg;
    PackState pack;
    int64_t opt_packed = -1;       // fp64 general product on the packed image: -1 auto, 0 never, 1 pack in front of the next product
    int64_t opt_packed_after = kPackAfter;                  // testing: auto's two thresholds (plain products served, bytes of matrix),
    int64_t opt_packed_min_bytes = (int64_t)kPackMinBytes;  // so that the switch runs at sizes a test can afford
    int64_t opt_packed_many = -1;  // the batched product (fp64, K <= 4) on the packed image: -1 auto (the admitted K, under "packed"'s
                                   // thresholds), 0 never, 1 pack in front of the next batched product and read the image at every K <= 4
    bool packed_many_effective = false;   // the last batched product launch read the image
    int dtype = LAM_HIP_F64;
    int total_shards = 1;          // P
    int rank = 0, nranks = 1;      // rank mode (one local shard == shard `rank`)
    bool rank_mode = false;
    ncclComm_t comm = nullptr;
    double t_comm_init = 0.0;
    uint64_t n = 0;
    uint64_t lda = 0;              // row pitch of A in ELEMENTS: n rounded up so that a row is a whole number of 4-KiB pages (of
                                   // 16-byte vectors when a row is shorter than a page); the padding is zero.  Every row then
                                   // starts page-aligned -- round decimal sizes (N = 10000 ... 70000, the reference's grid) stream
                                   // 0.5-1.5 % faster than with rows packed back to back (profiles/r04_size_sweep_align.txt) --
                                   // and the 16-byte-vector GEMV kernels serve ANY N, odd ones included (the scalar-peel kernel ran
                                   // those at 5.8-5.9 TB/s)
    bool have_problem = false, have_matrix = false, have_rhs = false, cg_ready = false;
    int k_done = 0;                // CG iterations enqueued since cg_init
    std::vector<ShardBase> sh;     // local shards
    std::string err;
    // options
    int64_t opt_gemv_variant = -1; // -1 = production shape for the dtype (see Impl::variant)
    int64_t opt_nt = 1;
    int64_t opt_generic = 0;       // force the generic kernel
    int64_t opt_probe_rows = 0;    // gemv_only: use only the first probe_rows rows of each shard (0 = all)
    int64_t opt_overlap = 1;       // rank mode: all-gather on its own stream under the own-slice GEMV panel
    int64_t opt_panel_lo = 0, opt_panel_hi = 0;  // testing: split the CG GEMV into [lo,hi) + the rest
    bool gather_pending = false;   // an all-gather of p is in flight on comm_stream
    int64_t opt_symmetric_many = 0;   // the batched product (K <= 4) reads only the upper triangle: 0 never, 1 where it pays, 2 always
    bool symv_many_effective = false; // the last batched product launch ran the symmetric kernels
    int64_t opt_symmetric = 0;     // single shard: read only the upper triangle (caller asserts A == A^T)
    int64_t opt_exchange = 0;      // 0 = sliced vectors, three exchanges per iteration (p.Ap, r.r, p slices); 1 = gather-Ap: ONE
                                   // exchange of [Ap slice | p.Ap partial] per iteration, r and p full-length on every shard;
                                   // 2 = direct (in-kernel flags)
    int64_t opt_join = 1;          // one process, gather-Ap: 1 = the iteration's single join goes through shard 0's stream (it
                                   // waits for the other shards' posts and records ONE join event they wait for: 2(P-1)+1
                                   // runtime calls); 0 = every stream waits for every other one (P(P-1) calls)
    int64_t opt_fuse = 1;          // one shard / direct exchange: x, r and p updates in ONE launch (update_fused_kernel)
    int64_t opt_reuse_matrix = 1;  // lam_hip_set_problem keeps (and re-uses) the matrix allocation when it is large enough
    int64_t opt_upload_staging = 0; // lam_hip_upload_rows: 1 = pipeline through two pinned staging buffers
    int64_t opt_finalize = 1;      // several shards: 1 = producer kernels reduce their partials themselves (Finalize);
                                   // 0 = separate 1-block finalize_sum_kernel launches (A/B measurements)
    uint64_t n_collectives = 0;    // RCCL calls enqueued by this context (diagnostics: must match across ranks)
    int64_t opt_gemv_timing = 8;   // HIP-event pair around the GEMV of every T-th iteration (t_gemv of the stats); 0 = never.
                                   // Every record is a marker packet between the kernels: timing every iteration costs 8 us
                                   // per iteration (profiles/r03_event_cost.txt)
    // One process, several shards: the host orders the shards' streams with events (profiles/r03_host_enqueue_cost.txt).  Every
    // cross-stream event operation costs the host 3-5 us, so the event-based forms all stay above 0.2 ms per iteration
    // at P = 8; the form that does not (no events at all) is the in-kernel flag exchange, option "exchange" = 2.
    hipEvent_t ev_join = nullptr;  // gather-Ap, option exchange_join: recorded on shard 0's stream once every shard has posted
    int64_t opt_assume_cus = 0;    // testing: pretend the device has this many CUs when checking that a launch whose
                                   // workgroups wait for each other is fully resident (0 = ask the device)
    bool fuse_active = false;      // the current CG state uses update_fused_kernel (decided in cg_init: option + residency)
    // runtime calls issued by the iteration loop (diagnostics: host cost of an iteration, tools/host_enqueue_cost.py)
    uint64_t n_launch = 0, n_record = 0, n_wait = 0, n_setdev = 0;
    uint64_t enqueue_ns = 0;       // host time spent issuing iterations (the waits for the device's progress excluded)
    uint64_t host_cpu_ns = 0;      // CPU time (CLOCK_THREAD_CPUTIME_ID) the calling thread spent inside lam_hip_cg_iterate
    double iter_est_s = 0.0;       // observed seconds per iteration (await_progress sleeps a fraction of it between polls)
    double prog_t = 0.0;           // when / at which iteration the last awaited progress was seen
    int prog_iter = 0;
    // direct exchange (option exchange = 2): peer-mapped p replicas and mailboxes (lam_kernels.h, Mail)
    Mail *peer_mail[kMaxShards] = {};           // every shard's mailbox as seen from this process (own included)
    void *peer_p[kMaxShards] = {};              // every shard's p replica as seen from this process (own included)
    void *ipc_opened[2 * kMaxShards] = {};      // mappings to close again
    int n_ipc_opened = 0;
    uint64_t problem_gen = 0, direct_gen = ~0ull;   // direct mappings belong to one set_problem generation
    bool direct_ok = false;
    bool cg_direct = false;                     // the current CG state runs on the direct exchange
    int64_t opt_verify_direct = 1;              // lam_hip_solve on the direct exchange: compare the recomputed residual with
                                                // the recursive one afterwards; on a mismatch solve again on the RCCL exchange
    int64_t direct_fallbacks = 0;               // how often that happened
    uint32_t epoch = 0;                         // bumped by every cg_init
    uint64_t seq_base = 0, seq_span = 1;        // hand-over number of iteration k of the current solve = seq_base + k: grows by one
                                                // per iteration over the whole life of the context and never restarts (cg_init moves
                                                // the base past every iteration of the previous solve), so the 32-bit tags of the
                                                // in-kernel hand-overs (lam_kernels.h, MailSlot) cannot meet a stale equal; the same
                                                // on every rank (all ranks enqueue the same iterations)
    int *direct_err = nullptr;                  // pinned host: a bounded in-kernel wait expired ([0] = which, see cg_iterate)
    double *agree_buf = nullptr;                // kAgreeBytes of device scratch of the small set-up collectives (kept: no hipFree in them)
    bool cg_exchange1 = false;     // the exchange the current CG state was initialised for
    double t_gemv_min = 0.0, t_gemv_max = 0.0;      // fastest / slowest local shard's average GEMV time of the last cg_iterate call (seconds)
    int xt_slot = -1;              // timing-ring slot of the iteration being enqueued if that iteration is timed (option gemv_timing),
                                   // else -1: its exchange steps are bracketed with HIP events too (lam_hip_stats.t_exchange)
    int ranks_on_device = 1;       // rank mode: ranks of the communicator that share THIS rank's GPU (emulations; counted once at
                                   // creation over the communicator): their fused vector-step launches must all be resident together
    bool symmetric_from_env = false;   // option "symmetric" came from LAM_HIP_SYMMETRIC (a driver that cannot call set_option): the
                                       // library then verifies A = A^T itself where it can and says when the option is not effective
    uint64_t matrix_gen = 0, sym_checked_gen = ~0ull;   // the matrix contents changed / were last checked for symmetry
    bool sym_refused = false;      // the environment asked for the symmetric product and the matrix is not symmetric: general GEMV
    bool told_sym_ineffective = false;

    // the symmetric product exists for every storage type and any n: one shard, or several row shards on the gather-Ap exchange
    // (inside CG only: every shard contributes a full-length vector per iteration, lam_exchange.h)
    // Option value 1: where it pays -- for a matrix below ~200 MB the two passes' fixed costs outweigh the halved stream (fp64: N = 3072
    // 1.0 x the general GEMV, 4096 1.13-1.18 x, 5120 1.3 x; fp32: 4096 0.8-1.0 x, 8192 1.1 x; bf16: 8192 0.93 x, 16384 1.24 x;
    // profiles/r04_symmetric_probe.txt): from 192 MiB of matrix on (fp64 N >= 5017, fp32 7095, bf16 10033); value 2: always.
    bool symv_wanted() const
    {
        return n > 0 && !sym_refused && (opt_symmetric >= 2 || (opt_symmetric == 1 && n * n * (uint64_t)esz_a() >= (192ull << 20)));
    }
    bool symv_active() const { return symv_wanted() && !rank_mode && total_shards == 1; }
    bool symv_multi_active() const { return symv_wanted() && exchange1_ok(); }
    // the packed image serves the fp64 general product of one shard in its default shape; everything else runs as before
    bool pack_eligible() const
    {
        return opt_packed != 0 && dtype == LAM_HIP_F64 && !rank_mode && total_shards == 1 && opt_symmetric == 0 && opt_generic == 0 &&
               opt_gemv_variant < 0 && n > 0;
    }
    // the image belongs to the matrix content: either reader (the single product, the batched one) may have caused it to be built
    bool pack_image_ready() const { return pack.buf != nullptr && pack.ready_gen == matrix_gen; }
    bool pack_active() const { return pack_eligible() && pack_image_ready(); }
    // option "packed_many": the batch's own scope (fp64, one shard), independent of "packed"
    bool pack_many_eligible() const { return opt_packed_many != 0 && dtype == LAM_HIP_F64 && !rank_mode && total_shards == 1 && n > 0; }
    // a shard's record in the symmetric product's gather: its full-length contribution, then (8-byte aligned) its part of p.Ap
    uint64_t symv_stride_bytes() const { return (n * esz_v() + 7) / 8 * 8 + 8; }

    bool exchange2_wanted() const { return (rank_mode || total_shards > 1) && opt_exchange == 2 && opt_finalize != 0; }
    // gather-Ap serves the reference's partition as it is (ConjugateGradient_CPU_MPI_OMP.hpp:176-196: n / P rows each, the
    // remainder on the LAST shard, gathered there with MPI_Allgatherv + sendcounts / displs, :505): every record has room for the
    // LONGEST slice (n / P + n % P rows; the shorter ones leave the rest unused -- one equal-count ncclAllGather in rank mode),
    // followed by the shard's part of p.Ap as a double on an 8-byte boundary.  Any n >= P.
    bool exchange1_ok() const { return (rank_mode || total_shards > 1) && opt_exchange == 1 && n >= (uint64_t)total_shards; }
    uint64_t ex1_base() const { return n / (uint64_t)total_shards; }
    uint64_t ex1_maxrows() const { return n / (uint64_t)total_shards + n % (uint64_t)total_shards; }
    uint64_t ex1_stride_bytes() const { return (ex1_maxrows() * esz_v() + 7) / 8 * 8 + 8; }

    size_t esz_a() const { return dtype == LAM_HIP_F64 ? 8 : (dtype == LAM_HIP_F32 ? 4 : 2); }
    static uint64_t pitch_for(uint64_t n, size_t ea) { return lam::row_pitch(n, ea); }      // lam_host_plan.h
    // columns the 16-byte-vector kernels cover: n rounded up to a whole vector (the extra columns are zeros of the padding,
    // met by zeros behind the end of p)
    uint64_t ncols_vec() const { const uint64_t v = 16 / esz_a(); return (n + v - 1) / v * v; }
    size_t esz_v() const { return dtype == LAM_HIP_F64 ? 8 : 4; }
};

namespace {

int fail(lam_hip_ctx *c, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    else g_create_error = buf;
    return code;
}

#define HIPCHK(c, call)                                                                       \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail((c), e_ == hipErrorOutOfMemory ? LAM_HIP_ENOMEM : LAM_HIP_EHIP,       \
                        "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

#define NCCLCHK(c, call)                                                                      \
    do {                                                                                      \
        ncclResult_t r_ = (call);                                                             \
        if (r_ != ncclSuccess)                                                                \
            return fail((c), LAM_HIP_ERCCL, "%s failed: %s (%s:%d)", #call,                   \
                        ncclGetErrorString(r_), __FILE__, __LINE__);                          \
    } while (0)

#define LAMCHK(expr)                 \
    do {                             \
        int rc_ = (expr);            \
        if (rc_ != 0) return rc_;    \
    } while (0)

// the iteration loop's runtime calls, counted (option "hip_calls_*"): what an iteration costs the host
#define LAUNCHED(c)                                  \
    do {                                             \
        (c)->n_launch++;                             \
        HIPCHK((c), hipGetLastError());              \
    } while (0)
#define RECORD(c, ev, st)                            \
    do {                                             \
        (c)->n_record++;                             \
        HIPCHK((c), hipEventRecord((ev), (st)));     \
    } while (0)
#define WAITEV(c, st, ev)                            \
    do {                                             \
        (c)->n_wait++;                               \
        HIPCHK((c), hipStreamWaitEvent((st), (ev), 0)); \
    } while (0)

// the matrix contents changed (upload, generators): the CG state and what was known about the old contents are void
void matrix_changed(lam_hip_ctx *c)
{
    c->have_matrix = true;
    c->cg_ready = false;
    c->matrix_gen++;
    c->sym_refused = false;
    c->multi.solved = c->multi.ms.valid = c->multi.lz.valid = c->multi.qd.valid = false;
}

// ConjugateGradient_CPU_MPI_OMP.hpp:176-184: n/P rows each, the remainder on the LAST rank (lam_host_plan.h)
void partition(uint64_t n, int P, int q, uint64_t *row0, uint64_t *nrows) { lam::partition_rows(n, P, q, row0, nrows); }

// OPT-IN (environment LAM_HIP_QUIET_RCCL=1, set by this package's drivers, whose stdout is a one-line protocol): file
// descriptor 1 points at stderr while at least one of these exists, i.e. for the duration of ncclCommInitRank, which
// prints a version banner to stdout.  A library must not move a host application's stdout around by default, so
// without the variable nothing is touched.  Counted under a lock: contexts may be created from several threads at
// once (the ranks-as-threads test double), and the first one in must be the one that remembers the real stdout, the
// last one out the one that restores it.
struct StdoutToStderr {
    static bool wanted()
    {
        const char *q = getenv("LAM_HIP_QUIET_RCCL");
        return q && *q && strcmp(q, "0") != 0;
    }
    const bool on = wanted();
    static std::mutex &mu() { static std::mutex m; return m; }
    static int &depth() { static int d = 0; return d; }
    static int &saved() { static int fd = -1; return fd; }
    StdoutToStderr()
    {
        if (!on) return;
        std::lock_guard<std::mutex> lk(mu());
        if (depth()++ == 0) {
            fflush(stdout);
            saved() = dup(1);
            if (saved() >= 0) (void)dup2(2, 1);
        }
    }
    ~StdoutToStderr()
    {
        if (!on) return;
        std::lock_guard<std::mutex> lk(mu());
        if (--depth() == 0 && saved() >= 0) {
            fflush(stdout);
            (void)dup2(saved(), 1);
            (void)close(saved());
            saved() = -1;
        }
    }
};

// temporaries of one call: released on every exit path (HIPCHK returns from the middle of a function)
struct DevBuf {
    void *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    template <typename T> T *as() const { return static_cast<T *>(p); }
};
struct PinnedBuf {
    void *p = nullptr;
    ~PinnedBuf() { if (p) (void)hipHostFree(p); }
};

void symv_dev_release(SymvDevPlan &d)
{
    for (void *q : {(void *)d.tasks, (void *)d.index, d.rowpart, d.colpart}) if (q) (void)hipFree(q);
    d = SymvDevPlan();
}

// The partials of `d` for K columns of p (K-wide records of `esz` bytes an element), in place of the ones it holds; both or neither.
// Columns behind the end of a ragged strip are never written by a task: the second pass does not read them either.
int symv_dev_partials(lam_hip_ctx *c, SymvDevPlan &d, uint64_t SS, size_t esz, int K, hipStream_t stream)
{
    const size_t rbytes = (size_t)d.rowpart_elems * K * esz, cbytes = (size_t)d.ntasks * SS * K * esz;
    DevBuf rp, cp;
    HIPCHK(c, hipMalloc(&rp.p, rbytes));
    HIPCHK(c, hipMalloc(&cp.p, cbytes));
    HIPCHK(c, hipMemsetAsync(cp.p, 0, cbytes, stream));
    if (d.rowpart != nullptr) HIPCHK(c, hipStreamSynchronize(stream));     // no launch on the smaller buffers is in flight
    for (void *q : {d.rowpart, d.colpart}) if (q) (void)hipFree(q);
    d.rowpart = rp.p; d.colpart = cp.p;
    rp.p = cp.p = nullptr;
    return 0;
}

// The one place a plan goes to the device: symv_plan for rows [row0, row0 + nrows) in strips of SS columns (cyc: the cyclic half
// windows of several row shards), its tasks and index, the partials for K columns.  All or nothing: a failure leaves `d` unbuilt.
int symv_dev_build(lam_hip_ctx *c, SymvDevPlan &d, uint64_t n, uint64_t ncv, uint64_t SS, uint64_t row0, uint64_t nrows, bool cyc,
                   size_t esz, int K, hipStream_t stream, const char *what)
{
    SymvPlan plan;
    symv_plan(n, ncv, SS, row0, nrows, cyc, &plan);
    if (plan.tasks.empty()) return fail(c, LAM_HIP_EINVAL, "%s: no tasks", what);
    if (plan.rowpart_elems >> 32) return fail(c, LAM_HIP_EINVAL, "%s: too many row partials for 32-bit offsets", what);
    DevBuf t, sb;
    HIPCHK(c, hipMalloc(&t.p, plan.tasks.size() * sizeof(SymvTask)));
    HIPCHK(c, hipMalloc(&sb.p, plan.index.size() * sizeof(uint32_t)));
    HIPCHK(c, hipMemcpy(t.p, plan.tasks.data(), plan.tasks.size() * sizeof(SymvTask), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(sb.p, plan.index.data(), plan.index.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    SymvDevPlan b;
    b.ix = plan.ix;
    b.ntasks = (int)plan.tasks.size();
    b.rowpart_elems = plan.rowpart_elems;
    LAMCHK(symv_dev_partials(c, b, SS, esz, K, stream));
    b.tasks = t.as<SymvTask>(); b.index = sb.as<uint32_t>();
    t.p = sb.p = nullptr;
    d = b;
    return 0;
}

int vec_grid(uint64_t n_loc)
{
    uint64_t b = (n_loc + kBlock - 1) / kBlock;
    return (int)std::max<uint64_t>(1, std::min<uint64_t>(b, kVecBlocksMax));
}

}  // namespace
