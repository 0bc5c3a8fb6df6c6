/*
 * lam_hip.h -- C ABI of the MI355X-native dense Conjugate-Gradient hot path.
 *
 * This is the drop-in boundary: plain pointers, sizes and scalars only (no C++, no torch
 * types).  The reference has no FFI layer; its operator API is the abstract class
 * LAM::ConjugateGradient<T> (challenge/main/LAM/src/ConjugateGradient.hpp:9-28) plus the
 * generate/getter methods of the distributed classes
 * (LAM/src/CPU/ConjugateGradient_CPU_MPI_OMP.hpp:31-35,
 *  LAM/src/GPU/distributed/ConjugateGradient_MultiGPUS_CUDA_NCCL.cuh:37-41).
 * The C++ classes in 2024-eumaster4hpc-student-challenge_amd/LAM/ implement that class
 * interface on top of the functions below; every entry point says which reference member
 * (file:line) it stands in for.  Paths are relative to /root/reference/challenge/main/.
 *
 * Conventions
 *   - return 0 on success, a negative LAM_HIP_E* code on failure; lam_hip_last_error()
 *     gives the message (HIP / RCCL status text included).  Every HIP and RCCL call is
 *     checked.  No exceptions cross the ABI.
 *   - a context owns all device memory, streams, events and the RCCL communicator; host
 *     buffers passed in are borrowed for the duration of the call only.
 *   - a context is not thread-safe; one solve at a time (same as the reference classes).
 *   - "shard" = one block of consecutive matrix rows living on one device, partitioned
 *     exactly like the reference: shard q of P owns rows [q*(N/P), (q+1)*(N/P)), the last
 *     shard also takes N%P (LAM/src/CPU/ConjugateGradient_CPU_MPI_OMP.hpp:176-184).
 *   - the library never falls back to the CPU: without a usable GPU every compute entry
 *     point fails with LAM_HIP_ENODEV.
 */
#ifndef LAM_HIP_H
#define LAM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI history (a caller compares lam_hip_abi_version() with the LAM_HIP_ABI_VERSION it was compiled against):
 *   1  rounds 1-3.
 *   2  + lam_hip_build_id, lam_hip_generate_spectrum_spd.
 *   3  + lam_hip_debug_symv_plan; BEHAVIOUR: lam_hip_create with more than one shard defaults to the gather-Ap exchange
 *      (option "exchange" = 1; was 0), and option "symmetric" = 1 means "from 192 MiB of matrix on, any N, one or several
 *      shards" (was: one shard, N a multiple of 4096).
 *   4  (round 5) lam_hip_stats grows by t_exchange (appended: the older fields keep their offsets, but a caller must pass
 *      the larger struct); BEHAVIOUR: the gather-Ap exchange takes any N >= shards (the reference's uneven partition), so
 *      "exchange_effective" no longer drops to 0 for N % shards != 0; lam_hip_create_rank defaults to the gather-Ap
 *      exchange too (option "exchange" = 1; was 0).
 *      Added under version 4 (purely additive, no struct or existing entry point changes): LAM_HIP_MAX_RHS, lam_hip_set_rhs_many,
 *      lam_hip_solve_many, lam_hip_get_solution_many, lam_hip_gemv_many, lam_hip_gemv_many_only and the get-only option
 *      "multi_rhs_k".  A caller that needs them checks for the symbols (dlsym) or the build id; the version number does not move.
 *      Added under version 4 likewise (purely additive): LAM_HIP_PC_NONE, LAM_HIP_PC_JACOBI, lam_hip_solve_many_pc and
 *      lam_hip_get_diagonal.
 *      Added under version 4 likewise (purely additive): lam_hip_solve_many_x0 and lam_hip_true_residual_many.
 *      Added under version 4 likewise (purely additive): lam_hip_set_shifts_many.
 *      Added under version 4 likewise (purely additive): LAM_HIP_MAX_SHIFTS, lam_hip_solve_mshift, lam_hip_get_solution_mshift and
 *      lam_hip_true_residual_mshift.
 *      Added under version 4 likewise (purely additive): lam_hip_solve_many_minres.  One new refusal becomes reachable with it: a
 *      CG batch call while a negative shift (which only lam_hip_solve_many_minres accepts) is in force.
 *      Added under version 4 likewise (purely additive): option "symmetric_many" and the get-only option "symmetric_many_effective".
 *      With "symmetric_many" at its default 0 every result is what it was.
 *      Added under version 4 likewise (purely additive): option "packed" and the get-only options "packed_effective", "packed_bytes"
 *      and "packed_pack_ns".  Every result is bit for bit what it was, under every value of the option.  Likewise the testing
 *      options "packed_after" and "packed_min_bytes" (defaults: what the automatic mode did before they existed).
 *      Added under version 4 likewise (purely additive): option "packed_many" and the get-only option "packed_many_effective".
 *      Every result is bit for bit what it was, under every value of the option.
 *      Added under version 4 likewise (purely additive): LAM_HIP_MAX_LANCZOS, LAM_HIP_EIG_SMALLEST / _LARGEST / _BOTH, lam_hip_eigs,
 *      lam_hip_get_lanczos, lam_hip_get_eigenvectors, lam_hip_eig_residuals, lam_hip_project_out and lam_hip_tridiag_eigen.
 *      Added under version 4 likewise (purely additive): LAM_HIP_MAX_DEFLATION, lam_hip_set_deflation, lam_hip_set_deflation_eigs,
 *      lam_hip_solve_many_deflated, lam_hip_deflate_many, lam_hip_chol_inverse and the get-only option "deflation_m".
 *      Added under version 4 likewise (purely additive): lam_hip_solve_block and lam_hip_block_factor.
 *      Added under version 4 likewise (purely additive): LAM_HIP_MAX_PROBES, LAM_HIP_QUAD_LOG / _INV / _POW, lam_hip_lanczos_many,
 *      lam_hip_get_lanczos_many, lam_hip_trace_quadrature and lam_hip_tridiag_quadrature. */
#define LAM_HIP_ABI_VERSION 4

/* most row shards of one process (lam_hip_create) / ranks of one communicator (lam_hip_create_rank); more -> LAM_HIP_EINVAL.
 * 16 until round 5; the reference's largest published GPU run has 64 ranks (TESTS/results/STRESS_TEST_GPU_MPI.txt:18). */
#define LAM_HIP_MAX_SHARDS 64

/* storage / arithmetic type of the matrix and vectors */
#define LAM_HIP_F64 0  /* double everywhere (the reference drivers hard-code <double>) */
#define LAM_HIP_F32 1  /* float storage, float FMA, double only for the reduced scalars */
#define LAM_HIP_BF16 2 /* bf16 matrix storage, fp32 vectors and accumulation (config 4) */

#define LAM_HIP_EINVAL (-1)  /* bad argument / call order */
#define LAM_HIP_ENODEV (-2)  /* no usable GPU */
#define LAM_HIP_EHIP (-3)    /* a HIP call failed */
#define LAM_HIP_ERCCL (-4)   /* an RCCL call failed */
#define LAM_HIP_ENOMEM (-5)  /* device or host allocation failed */
#define LAM_HIP_ESTATE (-6)  /* problem / matrix / rhs not set yet */

#define LAM_HIP_UNIQUE_ID_BYTES 128 /* == NCCL_UNIQUE_ID_BYTES */

typedef struct lam_hip_ctx lam_hip_ctx;

/* What the reference prints per run (test/test_CG_CPU_MPI_OMP.cpp:201-203 and
 * ConjugateGradient_MultiGPUS_CUDA_NCCL.cu:332-334,424-427), as numbers. */
typedef struct lam_hip_stats {
    int32_t num_iters;    /* loop counter on exit: converging iteration, or max_iters+1 at the cap */
    int32_t converged;    /* solve()'s bool */
    double rel_err;       /* sqrt(rr/bb), the recursive relative residual */
    double t_gemv;        /* average seconds per iteration in the GEMV kernel (device time; several local shards: the slowest one's) */
    double t_iter;        /* average seconds per iteration (wall, whole loop / iterations run) */
    double t_total;       /* wall seconds of the call */
    double t_comm_init;   /* seconds spent creating the RCCL communicator (0 if none) */
    double gemv_bytes;    /* algorithmic bytes one GEMV launch on this rank reads+writes */
    double t_exchange;    /* average seconds per iteration in the iteration's exchange step(s) on this rank / shard 0: the
                           * RCCL collective(s), or the event join(s) of one process driving several shards (from the post
                           * behind the producer kernel until the consumer's stream has passed its waits); sampled on the
                           * iterations whose GEMV is timed (option "gemv_timing").  0 for one shard and for the direct
                           * exchange (which waits inside its kernels).  t_gemv + t_exchange is what the reference prints
                           * as its t_gemv column, which includes broadcast + gather
                           * (ConjugateGradient_MultiGPUS_CUDA_NCCL.cu:352-377) */
} lam_hip_stats;

/* ---- lifecycle ---------------------------------------------------------------------------- */

int lam_hip_abi_version(void);
/* 16 hex digits identifying the sources (csrc/lam_hip.hip, csrc/lam_kernels.h, this header) the library was built
 * from (sha256 prefix, set by the Makefile).  The Python binding compares it with the sources next to it and refuses
 * a stale library.  No reference counterpart. */
const char *lam_hip_build_id(void);
int lam_hip_device_count(int *count);

/* One process driving `n_shards` row shards, shard q on device_ids[q] (device ids may repeat,
 * which puts several shards on one GPU; device_ids == NULL means 0,1,..,n_shards-1 modulo the
 * device count).  Shards exchange p slices and partial dot products by direct peer stores
 * over xGMI.  Stands in for the constructor + device discovery of the single-process class
 * LAM/src/GPU/local/ConjugateGradient_MultiGPUS_CUDA.cuh:20-22 and, with n_shards == 1, of
 * LAM/src/GPU/local/ConjugateGradient_GPU_CUDA.cuh. */
int lam_hip_create(lam_hip_ctx **out, int dtype, int n_shards, const int *device_ids);

/* One process per GPU: this process owns shard `rank` of `nranks` on `device_id`; the per
 * iteration exchange is RCCL (all-gather of p, and of the ranks' partial dot products).
 * `unique_id` = LAM_HIP_UNIQUE_ID_BYTES bytes obtained from lam_hip_get_unique_id() on one rank
 * and distributed by the caller (MPI_Bcast, torch.distributed, a file ...), exactly the
 * bootstrap of ConjugateGradient_MultiGPUS_CUDA_NCCL.cu:306-334 (ncclGetUniqueId + MPI_Bcast +
 * ncclCommInitRank, timed into the extra CSV column -> lam_hip_stats.t_comm_init). */
/* RCCL prints a version banner to STDOUT when a communicator is created.  The library leaves the process's file
 * descriptors alone by default; a caller whose stdout is a protocol (this package's drivers: one CSV line) sets the
 * environment variable LAM_HIP_QUIET_RCCL=1, and file descriptor 1 then points at stderr for the duration of
 * ncclCommInitRank (process-wide: other threads' stdout goes there too for that window). */
int lam_hip_get_unique_id(void *unique_id_out);
int lam_hip_create_rank(lam_hip_ctx **out, int dtype, int device_id, int rank, int nranks,
                        const void *unique_id);

void lam_hip_destroy(lam_hip_ctx *ctx);
const char *lam_hip_last_error(const lam_hip_ctx *ctx); /* ctx may be NULL: last create error */

/* ---- problem definition ------------------------------------------------------------------- */

/* Fix N, compute the reference row partition and allocate A (rows_loc x N, row-major, per
 * shard; on the device every row is padded to a whole number of 4-KiB pages -- an internal layout, upload / download take and
 * give dense rows -- so that any N, odd ones included, streams through the aligned 16-byte-vector kernels) and the work vectors.  Stands in for the allocation half of load_matrix_from_file /
 * generate_matrix (ConjugateGradient_CPU_MPI_OMP.hpp:176-196,214,250-253;
 * ConjugateGradient_MultiGPUS_CUDA_NCCL.cu:544-568).  Frees the previous problem's vectors first: hipFree waits for the
 * whole device AS THIS PROCESS sees it, so a process that hosts several rank contexts as threads (the test harness's shape;
 * a deployment has one rank per process) must not call it while another of its ranks has a collective in flight that waits
 * for this one.  A new matrix of the SAME size needs no new lam_hip_set_problem. */
int lam_hip_set_problem(lam_hip_ctx *ctx, uint64_t n);

/* The row partition itself, usable without a context (and without a GPU): rows of shard q of P for
 * an n x n matrix, ConjugateGradient_CPU_MPI_OMP.hpp:176-184. */
int lam_hip_partition(uint64_t n, int num_shards, int shard, uint64_t *row0, uint64_t *nrows);

int lam_hip_n(const lam_hip_ctx *ctx, uint64_t *n);
int lam_hip_num_shards(const lam_hip_ctx *ctx, int *total_shards, int *local_shards);
/* rows of global shard q (any q in [0,total_shards), local or not) */
int lam_hip_get_partition(const lam_hip_ctx *ctx, int shard, uint64_t *row0, uint64_t *nrows);

/* Copy rows [row0,row0+nrows) of the global matrix (host, row-major, nrows*N elements of the
 * context dtype; for LAM_HIP_BF16 the host rows are float and are rounded on upload) into the
 * local shard(s) that own them.  Rows owned by other processes are an error.  Stands in for
 * the read + H2D copy of load_matrix_from_file (ConjugateGradient_MultiGPUS_CUDA_NCCL.cu:
 * 568-583), with 64-bit counts. */
int lam_hip_upload_rows(lam_hip_ctx *ctx, uint64_t row0, uint64_t nrows, const void *host_rows);
/* inverse of upload (tests, and save of generated systems) */
int lam_hip_download_rows(lam_hip_ctx *ctx, uint64_t row0, uint64_t nrows, void *host_rows);

/* Dense tridiag(1,2,1) filled on device by GLOBAL row index: generate_matrix,
 * ConjugateGradient_CPU_MPI_OMP.hpp:237-247 / ConjugateGradient_MultiGPUS_CUDA_NCCL.cu:628-714. */
int lam_hip_generate_tridiag(lam_hip_ctx *ctx);
/* Dense symmetric strictly diagonally dominant SPD test matrix, generated on device from a
 * counter-based hash (no reference counterpart; replaces the MKL-based
 * challenge/main/random_spd_system.cpp for sizes that do not fit a file):
 * with sm = SplitMix64's output function, u01(h) = (h >> 11) * 2^-53, all index arithmetic in wrapping uint64, lo / hi the
 * smaller / larger of the GLOBAL indices i, j:
 *   A[i][j] = A[j][i] = (2 u01(sm(seed + sm(lo*N + hi))) - 1) * fl(1/N)   in [-1/N, 1/N)   (`+`, one rounding: the product)
 *   A[i][i] = 1 + (cond-1) * u01(sm(seed ^ sm(2*i + 1)))                  in [1, cond)     (`^`; may be contracted into an fma)
 * ([1, cond) in exact arithmetic; the rounded sum can reach cond itself), computed in fp64 and rounded once to fp32 storage.
 * bf16 storage is written __float2bfloat16((float)v): the compiler may keep the two roundings or merge them into ONE rounding of
 * the fp64 value to the nearest-even bf16; either is the law, for the whole matrix (today's gfx950 compiler merges them, and 8
 * elements per million differ from the fp32 matrix rounded to bf16).  tests/generator_model.py states the law in numpy and
 * tests/test_gpu_generators.py holds every element of the device's matrix to it.
 * eigenvalues lie in (0, cond+1): `cond` spreads the spectrum so CG does not converge at once. */
int lam_hip_generate_random_spd(lam_hip_ctx *ctx, uint64_t seed, double cond);

/* Dense SPD matrix with a PRESCRIBED SPECTRUM, the law of the reference's fixture generator
 * (challenge/main/random_spd_system.cpp:66-97: A = Q diag(d) Q^T, d_i = exp(3.5 U[-1,1]), cond ~ 1.1e3), built on the device:
 *   A = H_k ... H_1 diag(eig) H_1 ... H_k,   H_j = I - 2 v_j v_j^T / (v_j . v_j),   v_j = v[j*N .. j*N+N)
 * i.e. Q is a product of k Householder reflectors instead of the reference's O(N^3) Gram-Schmidt with MKL: the spectrum is
 * `eig` up to rounding, A is symmetric bit for bit, cost O(k N^2) (one GEMV + one rank-2 update pass per reflector).  eig:
 * N positive values, v: k x N (host, double).  fp64 / fp32 storage.  Collective in rank mode (every rank passes the same
 * arrays).  apps/random_spd_system.cpp draws eig, v and the rhs from srand/rand exactly as the reference does. */
int lam_hip_generate_spectrum_spd(lam_hip_ctx *ctx, const double *eig, const double *v, int k);

/* b: load_rhs_from_file (ConjugateGradient_CPU_MPI_OMP.hpp:258-305) / generate_rhs (:144-165).
 * b_host has N elements of the vector dtype (double for F64, float otherwise). */
int lam_hip_set_rhs(lam_hip_ctx *ctx, const void *b_host);
/* b back to the host (N elements of the vector dtype; single-process contexts): lets a generated system be
 * written to files in the reference's format (apps/random_spd_system.cpp, the counterpart of
 * challenge/main/random_spd_system.cpp:160-185). */
int lam_hip_get_rhs(lam_hip_ctx *ctx, void *b_host);
int lam_hip_generate_rhs(lam_hip_ctx *ctx, double value);          /* b == value (reference: 1.0) */
/* b[i] = TV(2 u01(sm(seed ^ sm(0xB5 + i))) - 1) in [-1,1), i the GLOBAL row, sm / u01 as above (tests/generator_model.py) */
int lam_hip_generate_random_rhs(lam_hip_ctx *ctx, uint64_t seed);

/* ---- the hot path ------------------------------------------------------------------------- */

/* solve(): ConjugateGradient_CPU_MPI_OMP.hpp:71-142 (recurrence, stop test BEFORE the p update,
 * num_iters = max_iters+1 at the cap).  Returns 0 whether or not it converged; see
 * stats->converged.  Equivalent to lam_hip_cg_init + lam_hip_cg_iterate(max_iters). */
int lam_hip_solve(lam_hip_ctx *ctx, int max_iters, double rel_error, lam_hip_stats *stats);

/* x=0, r=p=b, bb=b.b (ConjugateGradient_CPU_MPI_OMP.hpp:82-93). */
int lam_hip_cg_init(lam_hip_ctx *ctx);
/* Run up to `iters` further iterations of the loop (:98-116), continuing the iteration count
 * of earlier calls.  rel_error <= 0 never stops early (the stop test is still evaluated). */
int lam_hip_cg_iterate(lam_hip_ctx *ctx, int iters, double rel_error, lam_hip_stats *stats);

/* x (N elements of the vector dtype) to the host: the payload of save_result_to_file
 * (ConjugateGradient_CPU_OMP.hpp:199-217).  In rank mode this is a collective: every rank
 * must call it and every rank receives the full vector. */
int lam_hip_get_solution(lam_hip_ctx *ctx, void *x_host);
/* true relative residual ||b - A x||_2 / ||b||_2 recomputed on device with the GEMV kernel
 * (collective in rank mode).  Not in the reference; used for parity checks at full size. */
int lam_hip_true_residual(lam_hip_ctx *ctx, double *rel_res);

/* ---- several right-hand sides on one matrix ----------------------------------------------------
 * nrhs INDEPENDENT CG recurrences advanced together: per iteration ONE product launch reads the matrix once for all of them
 * (every 16-byte piece of a row meets the nrhs values of p while it is in registers), then one launch updates every x_j, r_j and
 * one every p_j.  This is NOT block CG (that is lam_hip_solve_block, below): column j keeps its own alpha_j, beta_j, r_j.r_j, stop
 * decision and iteration count and follows exactly the recurrence of lam_hip_solve (x = 0, r = p = b; stop test
 * sqrt(rr/bb) < rel_error before the p update; num_iters = max_iters + 1 at the cap).  The reference has no counterpart: its
 * drivers are run once per right-hand-side file.
 *   - a column that has met its stop test is FROZEN: its x, r, scalars and iteration count no longer change while the others run on;
 *   - columns never mix: a NaN or an Inf in one column stays there.  A column with b_j = 0 gives 0/0 in the reference's loop; it
 *     never meets the stop test, so the batch then runs to max_iters, exactly as a single solve of that column would;
 *   - supported: single-process contexts with ONE shard, LAM_HIP_F64 and LAM_HIP_F32.  Several shards, rank mode,
 *     LAM_HIP_BF16 and nrhs outside 1..LAM_HIP_MAX_RHS are refused with LAM_HIP_EINVAL and a message that names what is
 *     unsupported; calls before the matrix / the right-hand sides are set give LAM_HIP_ESTATE;
 *   - option "symmetric" (and LAM_HIP_SYMMETRIC) does not reach these entry points; their own switch is option "symmetric_many"
 *     (lam_hip_set_option), default 0 = the general batched product.  Under it the product of K <= 4 columns -- the loop product of
 *     every batched solve, the guess's A x0, MINRES, the multi-shift seed, lam_hip_true_residual_many, lam_hip_gemv_many and
 *     lam_hip_gemv_many_only -- reads every pair {A[i][j], A[j][i]} once, in two launches instead of one ("hip_calls_launch" counts
 *     it); K = 8, and with it lam_hip_true_residual_mshift, always runs the general product.  Column j of the symmetric batched
 *     product is bit for bit lam_hip_gemv's under "symmetric" = 2 for that vector, whatever K and whatever the other columns hold.
 *     stats.gemv_bytes then reports esz (N (N + 1) / 2 + 2 K N) + 2 esz K (row partials + column partials), the partials being
 *     those of the single symmetric product's plan (one per row of every task + 256 * (16 / esz) per task), written once and read
 *     once; t_gemv brackets both launches;
 *   - option "packed" does not reach these entry points either; their own switch is option "packed_many", default -1 = automatic.
 *     Under it the general batched product of K <= 4 fp64 columns -- the loop product of every batched solve (CG, Jacobi, shifts,
 *     MINRES, deflated, block), the guess's A x0, the multi-shift seed, lam_hip_eigs and its eigen-residuals, lam_hip_lanczos_many,
 *     lam_hip_set_deflation's A W, lam_hip_true_residual_many, lam_hip_gemv_many and lam_hip_gemv_many_only -- reads the lossless
 *     7-byte image of the matrix that "packed" reads, in the same single launch and with the same partials.  Every result is bit
 *     for bit the plain product's, under every value.  K = 8 and "symmetric_many" (which reads half the bytes and wins) are untouched;
 *     stats.gemv_bytes then reports the image's elements, headers and list values, each once, + 8 * 2 K N for the vectors;
 *   - kernels exist for K = 1, 2, 4 and 8 columns; nrhs runs on the smallest K >= nrhs with zero padding columns that are never
 *     updated (get-only option "multi_rhs_k": the K the last batched call ran, 0 before the first);
 *   - the batch state (vectors, scalars, progress word) is the context's own, allocated at the first batched call and independent of
 *     b / x of the single-vector calls: lam_hip_solve and lam_hip_solve_many may be interleaved on one context and neither
 *     disturbs the other's results.  lam_hip_set_problem invalidates the right-hand sides, as it does for lam_hip_set_rhs. */
#define LAM_HIP_MAX_RHS 8
/* B: nrhs vectors of N elements of the vector dtype, vector j contiguous at b_host + j*N (the layout of nrhs reference rhs files
 * read one after the other, ConjugateGradient_CPU_MPI_OMP.hpp:258-305). */
int lam_hip_set_rhs_many(lam_hip_ctx *ctx, int nrhs, const void *b_host);
/* All columns from x = 0.  Returns 0 whether or not every column converged.  stats describes the batch as a whole: num_iters =
 * the largest column's (the iterations the batch ran), converged = every column did, rel_err = the largest column's, NaN if any
 * column's is NaN, t_gemv / t_iter / t_total / gemv_bytes as for lam_hip_solve with the batched product (gemv_bytes =
 * esz (N^2 + 2 K N)).  num_iters / converged / rel_err: nrhs entries each, per column, with lam_hip_solve's meaning; any may be
 * NULL. */
int lam_hip_solve_many(lam_hip_ctx *ctx, int max_iters, double rel_error, lam_hip_stats *stats,
                       int32_t *num_iters, int32_t *converged, double *rel_err);
/* lam_hip_solve_many with a preconditioner.  precond = LAM_HIP_PC_NONE is lam_hip_solve_many itself (same code, same bits).
 * No reference counterpart: the reference is un-preconditioned.
 * LAM_HIP_PC_JACOBI: M = diag(A).  Per column j, independently, with dinv_i = 1 / A[i][i] computed in fp64 from the stored value
 * and rounded to the vector dtype:
 *     x = 0, r = b, bb = b.b, p = z = dinv o b, rz = r.z
 *     k = 1..max_iters:  Ap = A p;  alpha = rz / p.Ap;  x += alpha p;  r -= alpha Ap;  rr' = r.r;  rz' = r.(dinv o r)
 *                        if sqrt(rr'/bb) < rel_error: stop (p untouched);  beta = rz'/rz;  p = dinv o r + beta p
 * The stop test is lam_hip_solve's, on the same quantity (the UNpreconditioned recursive residual), so rel_error means the same
 * with and without the preconditioner.  Three launches per iteration as before, the product launch is the same kernel; the two
 * vector launches read one more vector of N elements each (N against N^2 matrix elements).  Measured at N = 65536 fp64 and
 * N = 131072 fp32, K = 1, 4, 8: an iteration costs 0.9945 ... 1.0004 of a plain one, inside the plain path's run-to-run spread
 * (profiles/pcg_probe.txt; the two vector kernels together take 7 us more at K = 8, profiles/pcg_k8_kernel_stats.txt), so at
 * such sizes every iteration saved is a pass over the matrix saved.
 *   - supports exactly what lam_hip_solve_many supports and refuses the same cases with the same codes; an unknown `precond`
 *     gives LAM_HIP_EINVAL;
 *   - the per-column arrays, the stats, lam_hip_get_solution_many, the frozen state of a stopped column, max_iters + 1 at the cap,
 *     the confinement of NaN / Inf to their column, a b_j = 0 column running to the cap on 0/0 and option "multi_rhs_k" are those
 *     of lam_hip_solve_many.  gemv_bytes counts the product launch alone, esz (N^2 + 2 K N) as without the preconditioner: the
 *     diagonal is read by the vector launches, not by the product;
 *   - the diagonal is extracted on the device once per matrix content (an upload or a generator call is seen by the next solve);
 *     a row whose A[i][i] or whose dinv_i is not finite and > 0 (<= 0, either zero, NaN, Inf, a subnormal whose reciprocal
 *     overflows) is refused with LAM_HIP_EINVAL and a message that names the first such row and its value: nothing is iterated
 *     and there is no batched solution afterwards (lam_hip_get_solution_many: LAM_HIP_ESTATE);
 *   - where it helps: matrices whose diagonal varies (lam_hip_generate_random_spd, badly scaled systems S M S).  For a CONSTANT
 *     diagonal -- lam_hip_generate_tridiag, the heat assembler's matrix, the reference generator's Q D Q^T in expectation -- the
 *     preconditioned recurrence is the plain one up to a scale factor and saves nothing. */
#define LAM_HIP_PC_NONE   0
#define LAM_HIP_PC_JACOBI 1
int lam_hip_solve_many_pc(lam_hip_ctx *ctx, int precond, int max_iters, double rel_error, lam_hip_stats *stats,
                          int32_t *num_iters, int32_t *converged, double *rel_err);
/* lam_hip_solve_many_pc(precond, ...) started from an initial guess instead of from x = 0.  x0_host: the nrhs guesses of the last
 * lam_hip_set_rhs_many, laid out as B (vector j at x0_host + j*N, vector dtype).  x0_host == NULL: from the batch's current
 * solution X -- the restart (fresh r = b - A x in place of a recursive residual that has drifted) or the continuation (a run that
 * hit its cap) of the last lam_hip_solve_many* call on this context; LAM_HIP_ESTATE if there is no readable batched solution:
 * before the first solve, after a refused diagonal, after lam_hip_gemv_many / _many_only, after a new matrix or
 * lam_hip_set_problem.  Per column j, independently:
 *     x = x0, r = b - A x0 (rounded to the vector dtype), bb = b.b, rr = r.r, p = r         (Jacobi: p = dinv o r, rz = r.(dinv o r))
 *     k = 0: if sqrt(rr/bb) < rel_error the column is born stopped: num_iters = 0, converged = 1, x = x0 bit for bit
 *     k = 1..max_iters: the loop of lam_hip_solve_many_pc, unchanged
 * One more product launch (A x0) and a fused K-wide pass in front of the loop; t_total includes them, gemv_bytes is the loop's
 * product launch as before.  bb = b.b stays the stop test's denominator, so rel_error keeps meaning "relative to ||b||" and a
 * continuation stops where the uninterrupted run would be asked to stop.
 *   - the k = 0 test is what keeps an exact guess (r = 0) from alpha = 0/0.  With rel_error <= 0 nothing ever stops, as in every
 *     solve here, k = 0 included: an exact guess then runs on 0/0 to the cap and its column ends as NaN, like a b_j = 0 column;
 *   - IDENTITY: for a finite matrix and rel_error <= 1, an all-zero x0_host gives the x, the per-column num_iters / converged /
 *     rel_err and "multi_rhs_k" of lam_hip_solve_many_pc(precond, ...) bit for bit (r = b - 0 = b exactly, and r.r and r.z are
 *     summed in the order that call sums b.b and b.(dinv o b)).  With rel_error > 1 the zero guess itself meets the test at k = 0;
 *   - max_iters = 0 is legal and returns the k = 0 state: rel_err = sqrt(rr0/bb), num_iters = 0 for a born-stopped column and
 *     max_iters + 1 = 1 otherwise;
 *   - everything else is lam_hip_solve_many_pc's: what is supported and what is refused (same codes), an unknown `precond`, the
 *     frozen state of a stopped column, the confinement of NaN / Inf to their column (a NaN in column j of x0 included),
 *     max_iters + 1 at the cap, the Jacobi diagonal's refusal (after which there is no batched solution). */
int lam_hip_solve_many_x0(lam_hip_ctx *ctx, int precond, const void *x0_host, int max_iters, double rel_error,
                          lam_hip_stats *stats, int32_t *num_iters, int32_t *converged, double *rel_err);
/* rel_res[j] = ||b_j - A x_j||_2 / ||b_j||_2 for the first nrhs columns of the last batched solution: ONE batched product of X,
 * then one K-wide pass (b - A x rounded to the vector dtype, fp64 sums).  The counterpart of lam_hip_true_residual, which serves
 * the single solve only.  The quotient is plain IEEE: b_j = 0 gives 0/0.  nrhs beyond the number solved: LAM_HIP_EINVAL; no
 * batched solution: LAM_HIP_ESTATE.  B and X are left alone: the solution stays readable and a following
 * lam_hip_solve_many_x0(..., NULL, ...) continues from it.  Independent of the single-vector state, as all batch calls are. */
int lam_hip_true_residual_many(lam_hip_ctx *ctx, int nrhs, double *rel_res);
/* Shifted systems: from here on column j of every lam_hip_solve_many, _solve_many_pc, _solve_many_x0 and
 * lam_hip_true_residual_many is the system (A + s_j I) x_j = b_j with s_j = sigma[j] rounded to the vector dtype -- a ridge /
 * Tikhonov sweep, a noise-level scan, implicit time steps of different length: eight different matrices for the passes over A of
 * one.  The product launch adds s_j p_j[row] in its epilogue (one fma per row and column, outside the stream of A), so A p, the
 * fused p.(A p), the guess's A x0 and the true residual's A x are the shifted matrix's; nothing else in the recurrence changes.
 * lam_hip_gemv_many and lam_hip_gemv_many_only stay the plain product of A.
 *   - call it after lam_hip_set_rhs_many (else LAM_HIP_ESTATE) with the nrhs set there (else LAM_HIP_EINVAL); sigma == NULL
 *     clears the shifts.  Every sigma[j] must be finite and >= 0, and finite after rounding to the vector dtype: a negative shift
 *     can make the matrix indefinite, for which CG is the wrong method.  Anything else: LAM_HIP_EINVAL, the message names the
 *     column and the value, and the shifts in force stay.  It refuses what the batch refuses (several shards, rank mode,
 *     LAM_HIP_BF16) with the same codes and words;
 *   - lam_hip_set_rhs_many and lam_hip_set_problem clear the shifts: a caller that never heard of them is unaffected;
 *   - new shifts do NOT invalidate the batched solution: lam_hip_solve_many_x0(..., NULL, ...) after lam_hip_set_shifts_many
 *     continues from the previous shifts' solutions (path-following along a regularisation path), and
 *     lam_hip_true_residual_many measures against the shifts in force;
 *   - no shifts, or every s_j == 0 after rounding: the unshifted kernels run and every result is bit for bit what it is without
 *     this call.  A column with s_j == 0 next to shifted ones computes its unshifted values (fma(0, p, s) == s; only the sign of a
 *     zero may differ);
 *   - LAM_HIP_PC_JACOBI with shifts: M_j = diag(A) + s_j I, dinv_ij = 1 / ((double)A[i][i] + (double)s_j) rounded to the vector
 *     dtype, one K-wide vector built and scanned by one launch per (matrix content, shifts).  The rule of the diagonal is on the
 *     SUM: the first (row, column) whose sum or reciprocal is not finite and > 0 is refused as lam_hip_solve_many_pc refuses a
 *     diagonal -- LAM_HIP_EINVAL naming row, column and value, nothing iterated, no batched solution afterwards -- and a zero on
 *     A's own diagonal is fine where the shift lifts it;
 *   - stats, gemv_bytes, the per-column arrays, frozen columns, NaN confinement, max_iters + 1 at the cap, the born-stopped
 *     column at k = 0 and "multi_rhs_k" are unchanged.  No launch, no device traffic: the shifts travel in the kernel arguments. */
int lam_hip_set_shifts_many(lam_hip_ctx *ctx, int nrhs, const double *sigma);
/* Batched MINRES (Paige and Saunders): (A + s_j I) x_j = b_j for shifts of EITHER sign -- shift-and-invert and inverse iteration
 * inside the spectrum, resolvents, frequency sweeps, any symmetric system that is not positive definite -- on the right-hand sides of
 * the last lam_hip_set_rhs_many, up to 8 columns with different shifts per pass over A.  Three launches per iteration: the batch's
 * product (its SHIFT epilogue does not care about the sign), one vector launch that ends in a norm, one that consumes it.  On SPD
 * systems it is useful too: rel_err decreases monotonically and in exact arithmetic IS the true residual norm, which CG's recursive
 * residual is not.  No reference counterpart.
 *   - always from x = 0 and without a preconditioner: Jacobi with diag(A) + s_j is not positive definite once shifts may be negative,
 *     and MINRES needs an SPD preconditioner.  Out of scope likewise: an initial guess, multi-shift MINRES, several shards, bf16;
 *   - sigma == NULL: the shifts in force (none, or lam_hip_set_shifts_many's).  sigma != NULL: nrhs (of lam_hip_set_rhs_many) shifts
 *     of any sign, each finite and finite after rounding to the vector dtype; anything else is LAM_HIP_EINVAL naming the column and
 *     the value, and the shifts in force stay.  Accepted shifts BECOME the shifts in force: lam_hip_true_residual_many then measures
 *     b_j - (A + s_j I) x_j under them and lam_hip_get_solution_many reads X.  All shifts zero after rounding: the unshifted product;
 *   - existing calls behave as before: lam_hip_set_shifts_many keeps refusing a negative shift, and it, lam_hip_set_rhs_many,
 *     lam_hip_set_problem and lam_hip_solve_mshift replace or clear the shifts as they always did.  NEW: lam_hip_solve_many, _pc and
 *     _x0 while a negative shift is in force are refused -- LAM_HIP_EINVAL naming the column and the value, nothing iterated, the
 *     batched solution still readable;
 *   - the recurrence, per column, all scalars fp64:
 *         bb = b.b ; beta1 = sqrt(bb) ; v = b / beta1 ; v_old = w = w_old = x = 0
 *         beta = 0 ; cs = -1 ; sn = 0 ; dbar = 0 ; eps = 0 ; phibar = beta1
 *         k = 1..max_iters:
 *            u      = (A + s I) v                 product launch; alpha = v.u from its fused partials
 *            u     -= alpha v + beta v_old        vector launch 1; partials of u.u
 *            beta'  = sqrt(u.u)                   vector launch 2, scalars first:
 *            eps_o = eps ; delta = cs dbar + sn alpha ; gbar = sn dbar - cs alpha ; eps = sn beta' ; dbar = -cs beta'
 *            gamma = hypot(gbar, beta') ; cs = gbar / gamma ; sn = beta' / gamma ; phi = cs phibar ; phibar = sn phibar
 *            w_new  = (v - eps_o w_old - delta w) / gamma ; w_old = w ; w = w_new ; x += phi w
 *            rel_err = phibar / beta1 ; if rel_err < rel_error: the column stops (v untouched, scalars final)
 *            else v_old = v ; v = u / beta' ; beta = beta'
 *     alpha is the product's fused v.(A v), NOT v.(A v - beta v_old): equal in exact arithmetic (v.v_old = 0), and the other would
 *     cost a fourth launch.  The coefficients that multiply vectors -- alpha, beta, eps_o, delta, phi and the reciprocals 1 / beta1,
 *     1 / gamma, 1 / beta' (the divisions above are multiplications by these) -- are rounded to the vector dtype once per column and
 *     iteration; the vector statements are fma chains: u = fma(-beta, v_old, fma(-alpha, v, u)),
 *     w_new = fma(-delta, w, fma(-eps_o, w_old, v)) * (1 / gamma), x = fma(phi, w_new, x).  Plain IEEE, no special case: beta' = 0
 *     (b in an invariant subspace) gives phibar = 0 and the column stops with rel_err = 0; a singular A + s_j I never meets the test
 *     and runs to the cap;
 *   - everything else is lam_hip_solve_many's, with the same codes and words: several shards, rank mode, LAM_HIP_BF16 (LAM_HIP_EINVAL),
 *     no matrix or no right-hand sides (LAM_HIP_ESTATE), max_iters < 0; stats, the per-column arrays, "multi_rhs_k" and K in
 *     {1, 2, 4, 8} with zero padding columns born stopped; a stopped column's x and scalars never change again; a NaN or an Inf stays
 *     in its column; b_j = 0 gives 0/0 and runs to the cap as NaN; rel_error <= 0 never stops; at the cap num_iters = max_iters + 1;
 *     max_iters = 0 returns x = 0, converged = 0, num_iters = 1, rel_err = 1.  The batch state afterwards is a batched solution:
 *     lam_hip_solve_many_x0(..., NULL, ...) may continue from it when no negative shift is in force;
 *   - cost: 2 K-wide vectors (w, w_old) and a block of scalars beyond the batch's, allocated by the first call.  Per iteration the two
 *     vector launches move about 14 K N elements (CG's: 9 K N) against N^2 for the product: 0.2 % at K = 8, N = 65536.  Measured on
 *     one MI355X against lam_hip_solve_many of the same build and K, the two alternated in one process (tools/minres_probe.py,
 *     profiles/minres_probe.txt): 0.999 / 1.000 / 1.004 x CG's seconds per iteration at K = 1 / 4 / 8 for fp64
 *     N = 65536 (4.86 / 5.43 / 9.23 ms) and 1.000 / 1.000 / 1.001 x for fp32 N = 131072; under shifts of both signs (the SHIFT
 *     product) 0.999 ... 1.007 x.  The windows of one figure spread by 0.06 ... 0.22 %. */
int lam_hip_solve_many_minres(lam_hip_ctx *ctx, const double *sigma, int max_iters, double rel_error, lam_hip_stats *stats,
                              int32_t *num_iters, int32_t *converged, double *rel_err);
/* The stored diagonal A[i][i], N elements of the vector dtype (LAM_HIP_BF16 storage: the stored bf16 values as float, exactly),
 * extracted on the device(s) from the pitched matrix.  Single-process contexts with any number of shards, every storage type;
 * rank mode: LAM_HIP_EINVAL; no matrix set: LAM_HIP_ESTATE.  No reference counterpart: the reference is un-preconditioned
 * (SURVEY §1). */
int lam_hip_get_diagonal(lam_hip_ctx *ctx, void *d_host);
/* The first nrhs solutions of the last lam_hip_solve_many / lam_hip_solve_many_pc, same layout as B (vector j at x_host + j*N). */
int lam_hip_get_solution_many(lam_hip_ctx *ctx, int nrhs, void *x_host);
/* Y = A X with the batched product kernel, X and Y laid out as B (parity tests, roofline probe).  Leaves the right-hand sides
 * and the single-vector state alone; a batched solution is no longer readable afterwards. */
int lam_hip_gemv_many(lam_hip_ctx *ctx, int nrhs, const void *x_host, void *y_host);
/* `reps` back-to-back launches of the batched product kernel for nrhs columns, timed with HIP events; *sec_per_product =
 * average seconds per launch.  The counterpart of lam_hip_gemv_only. */
int lam_hip_gemv_many_only(lam_hip_ctx *ctx, int nrhs, int reps, double *sec_per_product);

/* ---- multi-shift CG: every shift of (A + s_j I) x_j = b for one pass over A ---------------------
 * ONE right-hand side, 1..LAM_HIP_MAX_SHIFTS shifts -- the ridge / Tikhonov sweep or noise-level scan lam_hip_set_shifts_many names
 * first, without replicating b and without the K = 8 product.  For a common b and x0 = 0 the shifted Krylov spaces are one space
 * and the shifted residuals stay collinear with the seed's, r_j = zeta_j r (Jegerlehner; Frommer), so per iteration there is the
 * single-column product of the seed system and one fused vector launch for all shifts.  No reference counterpart.
 *   - b_host: N elements of the vector dtype.  nshifts outside 1..LAM_HIP_MAX_SHIFTS: LAM_HIP_EINVAL.  Every sigma[j] must be finite
 *     and >= 0, and finite after rounding to the vector dtype (lam_hip_set_shifts_many's rule): anything else is LAM_HIP_EINVAL and
 *     the message names the column and the value.  Supports what the batch supports: several shards, rank mode and LAM_HIP_BF16 are
 *     refused with the same codes and words; no matrix set: LAM_HIP_ESTATE.  No preconditioner and no initial guess: neither
 *     composes with the collinearity (use lam_hip_set_shifts_many for those);
 *   - the SEED is the smallest shift after rounding, s_min, and d_j = (double)s_j - (double)s_min >= 0.  The seed run is the K = 1
 *     batch: lam_hip_set_rhs_many(1, b) + lam_hip_set_shifts_many(1, &s_min) + lam_hip_solve_many, the same launches plus one per
 *     iteration.  The call therefore REPLACES the batch's right-hand sides and shifts, and afterwards the batch state is the
 *     seed's: lam_hip_get_solution_many(1), lam_hip_true_residual_many(1) and lam_hip_solve_many_x0(..., NULL, ...) work on it.
 *     Every j with d_j == 0 reports the seed's x, num_iters, converged and rel_err bit for bit (copied from the batch's X, not
 *     recomputed); s_min == 0 runs the unshifted product;
 *   - the recurrence, per shift j with d_j > 0, a_k / beta_k / rr_k the seed's alpha, beta and r.r of iteration k = 0, 1, ...,
 *     zeta_{-1} = zeta_0 = 1, a_{-1} = 1, beta_{-1} = 0, x_j = 0, p_j = b, behind the seed's x, r and p update of iteration k:
 *         zeta_{k+1} = zeta_k zeta_{k-1} a_{k-1} / (a_k beta_{k-1} (zeta_{k-1} - zeta_k) + zeta_{k-1} a_{k-1} (1 + d_j a_k))
 *         x_j += (a_k zeta_{k+1} / zeta_k) p_j ;  rel_err_j = zeta_{k+1} sqrt(rr_k / bb)
 *         if rel_err_j < rel_error: shift j stops, FROZEN like a batch column, num_iters_j = the iteration (counted from 1)
 *         else p_j = zeta_{k+1} r + beta_k (zeta_{k+1} / zeta_k)^2 p_j                     (r: the seed's, already updated)
 *     all scalars fp64, the three coefficients rounded to the vector dtype once per shift and iteration.  The loop ends when the
 *     seed stops or at the cap: a shift still live when the seed stops gets that iteration's x update and its own test (in exact
 *     arithmetic zeta <= 1, so it passes); at the cap an unconverged shift reports max_iters + 1, the batch's convention;
 *   - max_iters = 0 is legal and completes no step: every x_j = 0, converged = 0, num_iters = max_iters + 1 = 1 and rel_err = the
 *     start's sqrt(bb/bb) = 1 (NaN for b = 0) for every shift, the seed's slots included, as lam_hip_solve_many reports it;
 *   - if zeta_{k+1} is finite but zero or subnormal the shift is frozen BEFORE that step and reports converged = 0, num_iters = the
 *     last completed step and that step's rel_err: its residual is below what fp64 can scale r by, which only rel_error <= 0 or an
 *     absurdly small one lets happen.  A NaN is not frozen: b = 0 gives 0/0 in the seed and every shift runs to the cap as NaN;
 *   - stats as for lam_hip_solve_many: the largest num_iters, all converged, the worst rel_err (NaN if any is); t_gemv and gemv_bytes
 *     are the K = 1 product's.  num_iters / converged / rel_err: nshifts entries each, any may be NULL;
 *   - the multi-shift solution stays readable until lam_hip_set_problem, a new matrix, or any lam_hip_set_rhs_many /
 *     lam_hip_solve_many* / lam_hip_gemv_many* call (then LAM_HIP_ESTATE).  Independent of the single-vector state. */
#define LAM_HIP_MAX_SHIFTS 64
int lam_hip_solve_mshift(lam_hip_ctx *ctx, const void *b_host, int nshifts, const double *sigma, int max_iters, double rel_error,
                         lam_hip_stats *stats, int32_t *num_iters, int32_t *converged, double *rel_err);
/* The first nshifts solutions of the last lam_hip_solve_mshift, shift j contiguous at x_host + j*N (vector dtype).  More than were
 * solved: LAM_HIP_EINVAL; no readable multi-shift solution: LAM_HIP_ESTATE. */
int lam_hip_get_solution_mshift(lam_hip_ctx *ctx, int nshifts, void *x_host);
/* rel_res[j] = ||b - (A + s_j I) x_j||_2 / ||b||_2 for the first nshifts shifts, formed on the device per group of 8 shifts: ONE
 * K = 8 batched product of the group's x with the group's shifts, then one pass b - y against the single b (rounded to the vector
 * dtype, fp64 sums; plain IEEE, b = 0 gives 0/0).  Leaves the seed's batch (B, X) and the multi-shift solution readable. */
int lam_hip_true_residual_mshift(lam_hip_ctx *ctx, int nshifts, double *rel_res);

/* ---- Lanczos eigensolver: extreme eigenpairs of A at one product per step -----------------------
 * The other question asked of a dense symmetric matrix: its smallest and / or largest eigenvalues and their eigenvectors.  Lanczos
 * with FULL reorthogonalisation on the context's matrix A -- the plain product, as lam_hip_gemv_many is: the shifts in force are
 * ignored -- from one start vector, NOT restarted: at most max_steps <= LAM_HIP_MAX_LANCZOS steps.  No reference counterpart.
 *   - start vector: v0_host, N elements of the vector dtype, or v0_host == NULL: the law of lam_hip_generate_random_rhs(seed)
 *     (tests/generator_model.py).  It is normalised on the device; a zero or non-finite ||v0|| is LAM_HIP_EINVAL;
 *   - step k = 0, 1, ..., every scalar fp64:
 *         u = A v_k                                        the K = 1 product launch of the batch; alpha_k = v_k.u from its fused partials
 *         u = fma(-beta_{k-1}, v_{k-1}, fma(-alpha_k, v_k, u))
 *         twice ("twice is enough", classical Gram-Schmidt):  c = V^T u over v_0 .. v_k ;  u = fma(-c_j, v_j, u), j ascending
 *         beta_k = ||u|| ; unless the breakdown rule stops the run: v_{k+1} = u * (1 / beta_k)
 *     the coefficients that multiply vectors (alpha, beta, every c_j, the reciprocal) are rounded to the vector dtype once.  T keeps
 *     the fused alpha_k and the beta_k behind the reorthogonalisation; the Gram-Schmidt corrections are not folded in;
 *   - every sum goes through per-workgroup partials summed in a fixed order (no floating-point atomics): two calls with the same
 *     inputs give the same bits;
 *   - BREAKDOWN: the Krylov space is invariant if at step k beta_k is 0, not finite, or at most
 *     N u max_{j <= k}(|alpha_j| + beta_{j-1} + beta_j), u the unit roundoff of the vector dtype (2^-53 / 2^-24): the size of the
 *     rounding error of A v itself, below which u is noise.  v_{k+1} is then not formed, the run stops, the k + 1 Ritz pairs are
 *     final (reported converged) and nfound = min(nev, k + 1);
 *   - convergence is tested on the host after every check_every >= 1 steps (else LAM_HIP_EINVAL) and at the end: the stream is
 *     drained, theta and the bottom row s_{k,i} of T_k's eigenvector matrix come from a QL sweep that carries one row (O(k^2) per
 *     check), bound_i = beta_k |s_{k,i}|, and pair i is converged when bound_i <= tol * max_j |theta_j| -- relative to the norm,
 *     because the attainable floor is u ||A|| whatever theta_i is.  The run stops when all wanted pairs are converged, at a breakdown
 *     or at max_steps; tol <= 0 never stops early;
 *   - which: LAM_HIP_EIG_SMALLEST (ascending), LAM_HIP_EIG_LARGEST (descending), LAM_HIP_EIG_BOTH (ceil(nev/2) smallest, ascending,
 *     then floor(nev/2) largest, descending).  theta / bound / converged: nev entries each in that order, entries past *nfound are
 *     NaN / NaN / 0; any output pointer may be NULL.  stats: num_iters = the steps run, converged = all nev pairs were found and
 *     converged, rel_err = the worst bound_i / max|theta|, t_gemv / t_iter / t_total / gemv_bytes as for the K = 1 batch;
 *   - the Ritz vectors y_i = V s_i of the nfound wanted pairs are formed by one launch (fp64 coefficients and accumulation, one
 *     rounding to the vector dtype) and kept on the device for lam_hip_get_eigenvectors and lam_hip_eig_residuals;
 *   - launches per step ("hip_calls_launch"): 7 -- the product and six vector launches (three-term, dots / apply twice, append) --
 *     whatever k; 8 under option "symmetric_many", whose two-launch product the step then runs (every pair of A read once);
 *   - refusals: what the batch refuses, with the same codes and words (several shards, rank mode, LAM_HIP_BF16); no matrix:
 *     LAM_HIP_ESTATE; max_steps outside 1..min(N, LAM_HIP_MAX_LANCZOS), nev outside 1..max_steps, an unknown `which`:
 *     LAM_HIP_EINVAL naming the value;
 *   - state: its own (a basis of max_steps + 1 rows, each pitched to a 256-byte multiple of N + 16 elements and zero behind
 *     element N so that a row is the product's input as it stands; u; the Ritz vectors; a block of scalars), allocated at the first
 *     call, grow-only in max_steps, released with the batch.  The batch's right-hand sides and shifts are left alone; a batched or
 *     multi-shift solution is no longer readable afterwards (LAM_HIP_ESTATE), exactly as after lam_hip_gemv_many; the single-vector
 *     state is untouched; "multi_rhs_k" reports 1.  The eigen-solution stays readable until lam_hip_set_problem, a new matrix or the
 *     next lam_hip_eigs.  A symmetric matrix is the caller's statement; lam_hip_check_symmetry measures it;
 *   - out of scope: thick or implicit restart (a caller restarts by passing a combination of Ritz vectors as v0); interior
 *     eigenvalues and shift-invert with an inner MINRES; block Lanczos on K > 1; several shards, rank mode, bf16; a selective or
 *     partial reorthogonalisation;
 *   - cost: per step the six vector launches move about 4 k N elements against N^2 for the product (under 1 % at N = 65536 and
 *     256 steps); the basis takes (max_steps + 1) N elements (135 MB at N = 65536, 256 steps, fp64). */
#define LAM_HIP_MAX_LANCZOS 256
#define LAM_HIP_EIG_SMALLEST 0
#define LAM_HIP_EIG_LARGEST  1
#define LAM_HIP_EIG_BOTH     2
int lam_hip_eigs(lam_hip_ctx *ctx, int which, int nev, int max_steps, double tol, int check_every, const void *v0_host,
                 uint64_t seed, lam_hip_stats *stats, int32_t *nfound, double *theta, double *bound, int32_t *converged);
/* The coefficients of the last lam_hip_eigs: *steps, alpha[steps], beta[steps] (room for LAM_HIP_MAX_LANCZOS each; any may be NULL);
 * beta[k] is the norm that made v_{k+1}, so T_steps is (alpha[0 .. steps), beta[0 .. steps - 1)).  No eigen-solution: LAM_HIP_ESTATE. */
int lam_hip_get_lanczos(lam_hip_ctx *ctx, int32_t *steps, double *alpha, double *beta);
/* The first nev Ritz vectors of the last lam_hip_eigs, pair i contiguous at y_host + i*N (vector dtype), in theta's order.  More than
 * were found: LAM_HIP_EINVAL; no eigen-solution: LAM_HIP_ESTATE. */
int lam_hip_get_eigenvectors(lam_hip_ctx *ctx, int nev, void *y_host);
/* res[i] = ||A y_i - theta_i y_i||_2 / ||y_i||_2 of the first nev pairs, formed on the device as lam_hip_true_residual_mshift forms
 * its residuals: groups of up to 8 Ritz vectors through the batched product, then one pass (fp64 differences and sums).  Leaves the
 * eigen-solution, B and X alone. */
int lam_hip_eig_residuals(lam_hip_ctx *ctx, int nev, double *res);
/* Host-only and context-free, like lam_hip_partition: the eigenvalues of the symmetric tridiagonal matrix with diagonal alpha[0 .. k)
 * and off-diagonal beta[0 .. k-1) in ascending order (theta[k]), the bottom components of its eigenvectors (last_row[k], may be
 * NULL) and, if S != NULL, the whole k x k eigenvector matrix, column i contiguous at S + i*k.  Implicit QL; without S the sweep
 * carries the one row, O(k^2).  This is the routine lam_hip_eigs calls (csrc/lam_host_tridiag.h).  k outside
 * 1..LAM_HIP_MAX_LANCZOS, a NULL array or a non-finite entry: LAM_HIP_EINVAL. */
int lam_hip_tridiag_eigen(int k, const double *alpha, const double *beta, double *theta, double *last_row, double *S);

/* ---- Lanczos quadrature for the batch: log det(A + s I) and tr f(A) -----------------------------
 * The second number next to every solve of a sweep: log det(A + s I) (the other half of a Gaussian marginal likelihood),
 * tr (A + s I)^-1 (effective degrees of freedom, GCV), tr A^p.  Stochastic Lanczos quadrature (Golub & Meurant; Ubaru, Chen & Saad
 * 2017): m steps of plain Lanczos from a probe z give z^T f(A) z ~ ||z||^2 e_1^T f(T_m) e_1, a Gauss rule that is exact for
 * polynomials of degree 2m - 1; with Rademacher probes the mean over the probes estimates tr f(A).  Lanczos on A + s I from the same
 * probe gives T + s I, so ONE run serves every shift of a sweep, on the host, in O(m^2) per shift.  No reference counterpart.
 *
 * lam_hip_lanczos_many runs nprobes <= LAM_HIP_MAX_PROBES independent recurrences on the context's matrix A -- the plain product, as
 * lam_hip_eigs: the shifts in force are ignored -- with the three-term recurrence only: NO reorthogonalisation and NO stored basis
 * (the quadrature tolerates the loss of orthogonality that ruins Ritz vectors: ghost eigenvalues carry the weight of the copies they
 * stand for), nothing kept but 2 * steps doubles per probe.  Probes run in groups of up to 8 -- of up to 4 where option
 * "symmetric_many" engages for K <= 4, lam_hip_set_deflation's grouping rule -- each at the smallest K in {1, 2, 4, 8} that holds
 * it, padding columns zero and born stopped; a group shares one pass over A per step.
 *   - per probe j, every scalar fp64, the coefficients that multiply vectors rounded to the vector dtype (TV) once, every vector
 *     statement an explicit fma chain:
 *         zz = z.z ; v = z * (TV)(1 / sqrt(zz)) ; v_old = 0 ; beta_0 = 0
 *         k = 1 .. steps:
 *            u = A v                                            the batch's product launch; alpha_k = v.u from its fused partials
 *            u = fma(-beta_{k-1}, v_old, fma(-alpha_k, v, u))   vector launch 1; partials of u.u
 *            beta_k = sqrt(u.u) ; store alpha_k, beta_k         vector launch 2
 *            BREAKDOWN (lam_hip_eigs' rule: beta_k zero, not finite, or <= N u_TV max_{i <= k}(|alpha_i| + beta_{i-1} + beta_i)):
 *                 the probe stops, steps_run = k (its Krylov space is invariant: the quadrature is exact)
 *            else v_old = v ; v = u * (TV)(1 / beta_k)
 *   - probes: z_host holds nprobes vectors of N elements of the vector dtype, probe j at z_host + j*N; a probe whose norm is zero or
 *     not finite is LAM_HIP_EINVAL naming it.  z_host == NULL: Rademacher probes built on the device,
 *     z_j[i] = 1 - 2 (h >> 63), h = sm(seed ^ sm(0x51AC + j*N + i)), sm SplitMix64 in wrapping uint64 as in the generators, j the
 *     GLOBAL probe index and i the row (tests/quadrature_reference.py);
 *   - outputs: steps_run[nprobes], znorm2[nprobes] (the device's z.z), alpha and beta with probe j's coefficients at + j*steps,
 *     entries past steps_run[j] NaN.  Any output pointer may be NULL; the same data stays in the context -- host data, which no
 *     other batch call touches -- for lam_hip_get_lanczos_many and lam_hip_trace_quadrature until the next lam_hip_lanczos_many, a new
 *     matrix content or lam_hip_set_problem; otherwise LAM_HIP_ESTATE;
 *   - stats: num_iters = the largest steps_run, converged = every stored coefficient is finite, rel_err = 0, t_gemv / t_iter /
 *     t_total / gemv_bytes the batch's, for the last group's K;
 *   - every sum goes through per-workgroup partials summed in a fixed order (no floating-point atomics): two identical calls give
 *     identical bits, a probe's coefficients do not depend on its neighbours, and a NaN in one probe stays in its column;
 *   - launches per step ("hip_calls_launch"): 3 per group -- the product and two vector launches --, 4 under "symmetric_many" at
 *     K <= 4;
 *   - state: the batch's P (v, the product's input), AP (u) and R (v_old), and a small device block of its own (scalars and one
 *     group's coefficient history), allocated at the first call and released with the batch.  The right-hand sides, the shifts, the
 *     deflation space, the eigen-solution and the single-vector state are left alone; a batched or multi-shift solution is no longer
 *     readable afterwards (LAM_HIP_ESTATE), exactly as after lam_hip_gemv_many; "multi_rhs_k" reports the last group's K;
 *   - refusals: what the batch refuses, with the same codes and words (several shards, rank mode, LAM_HIP_BF16); no matrix:
 *     LAM_HIP_ESTATE; nprobes outside 1..LAM_HIP_MAX_PROBES, steps outside 1..min(N, LAM_HIP_MAX_LANCZOS): LAM_HIP_EINVAL naming
 *     the value;
 *   - out of scope: reorthogonalisation or a stored basis (lam_hip_eigs has both, for one vector); Gauss-Radau or other modified
 *     rules; a function pointer for f; probes other than Rademacher generated on the device (a caller passes any others from the
 *     host); an adaptive number of steps or probes; gradients of log det (they need solves, which the batch provides); several
 *     shards, rank mode, bf16;
 *   - cost: a step is the batch's product launch plus two latency-bound vector launches, the profile of lam_hip_solve_many_minres'
 *     iteration; the ratio of the two has not been measured (tools/quadrature_probe.py, profiles/quadrature_probe.txt). */
#define LAM_HIP_MAX_PROBES 64          /* 8 groups of LAM_HIP_MAX_RHS */
#define LAM_HIP_QUAD_LOG 0             /* f(t) = log t */
#define LAM_HIP_QUAD_INV 1             /* f(t) = 1 / t */
#define LAM_HIP_QUAD_POW 2             /* f(t) = t^p, p = (int)param >= 0 */
int lam_hip_lanczos_many(lam_hip_ctx *ctx, int nprobes, const void *z_host, uint64_t seed, int steps, lam_hip_stats *stats,
                         int32_t *steps_run, double *znorm2, double *alpha, double *beta);
/* What the last lam_hip_lanczos_many left, for its first nprobes probes: *steps (the row length of alpha and beta), steps_run, znorm2,
 * alpha and beta as that call lays them out; any pointer may be NULL.  More probes than were run: LAM_HIP_EINVAL; no coefficients:
 * LAM_HIP_ESTATE. */
int lam_hip_get_lanczos_many(lam_hip_ctx *ctx, int nprobes, int32_t *steps, int32_t *steps_run, double *znorm2, double *alpha,
                             double *beta);
/* Host arithmetic on the coefficients of the last lam_hip_lanczos_many, for nshifts <= LAM_HIP_MAX_SHIFTS shifts (sigma == NULL with
 * nshifts == 1: no shift):  q_{s,j} = znorm2_j * lam_hip_tridiag_quadrature(T_j over its steps_run_j, sigma_s);  estimate[s] = the
 * mean over the probes, summed in ascending j;  std_error[s] = the sample standard deviation (ddof 1) / sqrt(nprobes), NaN for one
 * probe;  per_probe[s * nprobes + j] = q_{s,j} (may be NULL, as may the other two).  For Rademacher probes estimate[s] estimates
 * tr f(A + sigma_s I); with LAM_HIP_QUAD_LOG that is log det(A + sigma_s I).  A node the function cannot take is LAM_HIP_EINVAL
 * naming the probe, the shift and the node; so are a probe with a non-finite coefficient, an unknown fn, a bad param. */
int lam_hip_trace_quadrature(lam_hip_ctx *ctx, int fn, double param, int nshifts, const double *sigma, double *estimate,
                             double *std_error, double *per_probe);
/* Host-only and context-free, like lam_hip_tridiag_eigen, on which it stands (csrc/lam_host_quad.h): for the symmetric tridiagonal T
 * with diagonal alpha[0 .. k) and off-diagonal beta[0 .. k-1),  out[s] = e_1^T f(T + sigma_s I) e_1 = sum_i S_{1i}^2 f(theta_i +
 * sigma_s), i ascending in theta.  The eigenproblem is solved once, on the reversed tridiagonal, so that the one-row QL sweep
 * carries the FIRST components: O(k^2), S is never formed, and each shift is one pass over the k nodes.  sigma == NULL with
 * nshifts == 1 means no shift.  LAM_HIP_EINVAL: k outside 1..LAM_HIP_MAX_LANCZOS, nshifts < 1, a NULL array, an unknown fn; a
 * non-finite coefficient or shift; under LAM_HIP_QUAD_POW a param that is not an integer >= 0; a node theta_i + sigma_s that is <= 0
 * under LAM_HIP_QUAD_LOG, == 0 under LAM_HIP_QUAD_INV, or not finite -- then bad[0] / bad[1] (bad may be NULL) hold the first such
 * shift and node, as lam_hip_chol_inverse reports bad_col, and -1 / -1 otherwise.  lam_hip_last_error(NULL) has the words. */
int lam_hip_tridiag_quadrature(int k, const double *alpha, const double *beta, int fn, double param, int nshifts,
                               const double *sigma, double *out, int *bad);

/* ---- deflated CG for the batch ----------------------------------------------------------------
 * CG whose residuals stay orthogonal to a small subspace W (Nicolaides; Saad, Yeung, Erhel, Guyomarc'h, SISC 2000): it converges as
 * if the eigenvalues W captures were absent.  W is typically the Ritz vectors lam_hip_eigs left on the device, but any W of full
 * rank is legal.  No reference counterpart.  One shard, LAM_HIP_F64 / LAM_HIP_F32, as the batch itself.
 *
 * lam_hip_set_deflation: W_host holds m vectors of N elements (vector dtype), vector i at W_host + i*N; m == 0 clears the space.
 * lam_hip_set_deflation_eigs: the first m Ritz vectors of the last lam_hip_eigs, copied device to device.
 *   - W goes into a device basis pitched and zero-padded like the Lanczos basis; A W comes from the batch's product launch in
 *     groups of up to 8 columns (up to 4 under option "symmetric_many", whose two-launch product then runs) -- the plain product of
 *     A, shifts are not applied; G = W^T (A W) from fp64 sums of fixed order; the host symmetrises G, factors it (Cholesky, fp64:
 *     lam_hip_chol_inverse's routine) and uploads G^-1;
 *   - it uses the batch's staging vectors: a batched or multi-shift solution is no longer readable afterwards (LAM_HIP_ESTATE),
 *     exactly as after lam_hip_gemv_many; the right-hand sides, the shifts, the eigen-solution and the single-vector state are
 *     left alone; "multi_rhs_k" reports the last group's K;
 *   - refusals: what the batch refuses, with the same codes and words (several shards, rank mode, LAM_HIP_BF16); no matrix:
 *     LAM_HIP_ESTATE; m outside 0..min(N, LAM_HIP_MAX_DEFLATION): LAM_HIP_EINVAL; a non-finite value in W_host: LAM_HIP_EINVAL
 *     naming the vector and the element; a pivot of the factorisation that is not finite, or at most N * u * max_i G_ii (u the unit
 *     roundoff of the vector dtype: the rounding error of G's own entries, lam_hip_eigs' breakdown rule): LAM_HIP_EINVAL naming the
 *     column -- W is numerically rank-deficient there; _eigs without an eigen-solution: LAM_HIP_ESTATE, with m above its nfound:
 *     LAM_HIP_EINVAL.  A refused call sets nothing: the previous space stays;
 *   - lifetime: the space belongs to the matrix content.  lam_hip_set_problem, an upload or a generator call invalidates it
 *     (lam_hip_solve_many_deflated then returns LAM_HIP_ESTATE, "deflation_m" reads 0); lam_hip_eigs, lam_hip_set_rhs_many and
 *     every solve leave it alone.  Memory: 2 * m * N elements, built aside and swapped in on success, released with the batch.
 *
 * lam_hip_solve_many_deflated solves the right-hand sides of the last lam_hip_set_rhs_many from x = 0, every column on its own,
 * all scalars fp64 (TV: the vector dtype; Ginv = G^-1):
 *       c = W^T b ; mu = Ginv c ; x0 = the fma chain over i ascending of (TV)mu_i w_i, from 0
 *       r = b - A x0 (rounded to TV) ; bb = b.b ; rr = r.r
 *       k = 0: sqrt(rr/bb) < rel_error -> born stopped (num_iters 0, x = x0)
 *       d = (AW)^T r ; mu = Ginv d ; p = r ; p = fma(-(TV)mu_i, w_i, p), i ascending
 *       k = 1..max_iters:  the plain batch's iteration (product ; alpha = rr / p.Ap, x, r ; stop test, p = r + beta p) ;
 *                          d = (AW)^T r ; mu = Ginv d ; p = fma(-(TV)mu_i, w_i, p)      for the columns still running
 *   - each mu = Ginv d is an m-term fp64 fma sum in ascending index, rounded to TV once per use; the dots are fp64 sums of fixed
 *     order; no floating-point atomics: two identical calls give identical bits;
 *   - the start is lam_hip_solve_many_x0's path with the guess built on the device; an iteration is the plain batch's three
 *     launches, unchanged, and two more behind them ("hip_calls_launch": 5 per iteration, 6 under "symmetric_many" at K <= 4);
 *   - a stopped column's p, x and scalars are never changed again; everything else is lam_hip_solve_many_x0's contract: frozen
 *     columns, NaN and Inf confined to their column, b_j = 0 runs to the cap on 0/0, rel_error <= 0 never stops, max_iters + 1 at
 *     the cap, max_iters = 0 returns the k = 0 state, zero padding columns, "multi_rhs_k", the stats (gemv_bytes: the product alone);
 *   - afterwards the batch holds a batched solution: lam_hip_get_solution_many and lam_hip_true_residual_many work on it, and
 *     lam_hip_solve_many_x0(..., NULL, ...) continues it as plain CG;
 *   - refusals: the batch's own; no space, or an invalidated one: LAM_HIP_ESTATE; a non-zero shift in force: LAM_HIP_EINVAL naming
 *     it (A W and G belong to A, not to A + s_j I);
 *   - out of scope: Jacobi together with deflation; a caller's guess; shifts; MINRES; multi-shift CG; a deflated continuation of an
 *     earlier solve; refreshing W from the CG run's own Lanczos coefficients (recycling); fusing the apply launch into the p
 *     update; several shards, rank mode, bf16. */
#define LAM_HIP_MAX_DEFLATION 32
int lam_hip_set_deflation(lam_hip_ctx *ctx, int m, const void *W_host);
int lam_hip_set_deflation_eigs(lam_hip_ctx *ctx, int m);
int lam_hip_solve_many_deflated(lam_hip_ctx *ctx, int max_iters, double rel_error, lam_hip_stats *stats, int32_t *num_iters,
                                int32_t *converged, double *rel_err);
/* The deflation operator alone, with the kernels the solve uses, on host vectors; needs no problem and no matrix, like
 * lam_hip_project_out (every storage type; LAM_HIP_BF16: float vectors).  Wd_host, Wa_host: m vectors of n elements each (vector
 * dtype), vector i at + i*n, 1 <= m <= LAM_HIP_MAX_DEFLATION; M: m x m doubles, row-major; U_host: nrhs vectors of n elements,
 * vector j at U_host + j*n, 1 <= nrhs <= LAM_HIP_MAX_RHS.  coeff[i*nrhs + j] = Wd_i.u_j, an fp64 sum of fixed order (may be NULL);
 * mu_j = M coeff_j (fp64 fma sum, ascending index); u_j = fma(-(TV)mu_ij, Wa_i, u_j) in ascending i, written back to U_host.
 * Columns do not mix: a NaN in u_j reaches u_j and coeff[.][j] only. */
int lam_hip_deflate_many(lam_hip_ctx *ctx, uint64_t n, int m, int nrhs, const void *Wd_host, const void *Wa_host, const double *M,
                         void *U_host, double *coeff);
/* Host-only and context-free, like lam_hip_tridiag_eigen: Ginv = G^-1 of the symmetric positive definite m x m matrix G (row-major
 * doubles; only the lower triangle is read; Ginv may not alias G) by a square-root-free Cholesky factorisation G = L D L^T in fp64,
 * symmetric bit for bit, and exact where every factor is a power of two.  This
 * is the routine lam_hip_set_deflation* call (csrc/lam_host_chol.h).  A pivot that is not finite or at most m * 2^-52 * max_i G_ii
 * (zero to the rounding of the factorisation's own sums: a duplicated column, a NaN): LAM_HIP_EINVAL with *bad_col (may be NULL)
 * the column; m outside 1..LAM_HIP_MAX_DEFLATION or a NULL matrix: LAM_HIP_EINVAL with *bad_col = -1.  A refused call leaves Ginv
 * alone. */
int lam_hip_chol_inverse(int m, const double *G, double *Ginv, int *bad_col);

/* ---- block CG for the batch ---------------------------------------------------------------------
 * One process, ONE shard, LAM_HIP_F64 / LAM_HIP_F32 storage, like every batched entry point.  No reference counterpart.
 *
 * lam_hip_solve_block solves the right-hand sides of the last lam_hip_set_rhs_many from X = 0 with ONE block Krylov space for the
 * s = nrhs columns: Dubrulle's retooled block CG (BCGrQ) with a Cholesky QR.  Every other batched solver advances nrhs independent
 * recurrences and saves bytes per iteration only; here the s search directions are shared, so the batch converges as if the s - 1
 * smallest eigenvalues of A were absent, at no set-up and with no lam_hip_eigs run.  Every small matrix is s x s and fp64; TV is the
 * vector dtype:
 *     G = B^T B ; bb_j = G_jj ; G = C^T C (C upper) ; Q = B C^-1 ; Phi = C ; P = Q ; X = 0
 *     k = 1 .. max_iters:
 *        Z = A P                             the batch's product launch (option "symmetric_many" serves K <= 4)
 *        H = P^T Z                           the upper triangle, mirrored
 *        H = L D L^T ; T = H^-1              a pivot failure: breakdown kind 1, X stays iterate k - 1
 *        X += P (T Phi) ; Q~ = Q - Z T       coefficients rounded to TV once; fma chains in ascending column index
 *        G = Q~^T Q~
 *        rel_err_j = sqrt(Phi_j^T G Phi_j / bb_j)        == ||r_j|| / ||b_j||, because R = Q~ Phi
 *        every live column < rel_error: stop, converged, X is iterate k
 *        G = S^T S (S upper)                 a pivot failure: breakdown kind 2, X is iterate k and valid
 *        Q = Q~ S^-1 ; P = Q + P S^T ; Phi = S Phi
 * The stop test stands in front of the second factorisation: exact convergence (Q~ = 0) reports "converged, rel_err 0", not a
 * breakdown.  Pivot rule (both factorisations and the initial G): a pivot fails when it is not finite or at most
 * s * u_TV * max_i G_ii, u_TV = 2^-53 (fp64) or 2^-24 (fp32) -- lam_hip_eigs' breakdown rule.  Four launches per iteration (five
 * under "symmetric_many" at K <= 4), all sums fp64 and of fixed order: two identical calls give identical bits.
 *   - The columns are COUPLED.  The batch stops when ALL live columns meet the test, and no column freezes: num_iters[j] is the first
 *     iteration at which column j met the test (max_iters + 1 if it never did), converged[j] and rel_err[j] are the values at exit
 *     (of the last completed iteration).  A NaN or Inf in one column reaches all columns.
 *   - breakdown (may be NULL): breakdown[0] = the iteration of the breakdown (0: none), breakdown[1] = its kind (1 | 2, 0: none).
 *     A breakdown ends the solve with return code 0; stats->num_iters counts the completed iterations (k - 1 for kind 1).
 *   - Afterwards the batch holds a batched solution: lam_hip_get_solution_many and lam_hip_true_residual_many serve it, and after a
 *     breakdown or the cap lam_hip_solve_many_x0(..., NULL, ...) continues from X with the independent recurrences -- the
 *     documented recovery.
 *   - rel_error <= 0 never stops early; a run that converges exactly then ends in breakdown kind 2 and says so.
 *   - max_iters == 0: X = 0, rel_err = 1, num_iters = 1.  max_iters < 0: LAM_HIP_EINVAL, as for the batch.
 *   - refusals, with the batch's codes: several shards, rank mode, LAM_HIP_BF16: LAM_HIP_EINVAL; no matrix or no right-hand sides:
 *     LAM_HIP_ESTATE; a non-zero shift in force: LAM_HIP_EINVAL naming it (a block needs one operator); an initial G = B^T B that
 *     fails the pivot rule -- a zero or duplicated column, nrhs > N: LAM_HIP_EINVAL naming the column, nothing is iterated.
 *   - stats are the batch's: gemv_bytes and t_gemv are the product's alone.
 *   - out of scope: Jacobi or deflation inside the block; a caller's guess; shifts; MINRES; dropping converged columns from the
 *     block (variable block size); several shards. */
int lam_hip_solve_block(lam_hip_ctx *ctx, int max_iters, double rel_error, lam_hip_stats *stats, int32_t *num_iters,
                        int32_t *converged, double *rel_err, int32_t *breakdown /* [2]: iteration (0 = none), kind 1|2 */);
/* Host-only and context-free, like lam_hip_chol_inverse: the s x s routines of lam_hip_solve_block (csrc/lam_host_block.h, the code
 * its kernels run) on the symmetric G (row-major doubles, s in 1..LAM_HIP_MAX_RHS; only the upper triangle is read), under the
 * pivot rule of `dtype` (LAM_HIP_F64 | LAM_HIP_F32).  Ginv = G^-1 by G = L D L^T, symmetric bit for bit; S upper triangular with
 * G = S^T S, and Sinv = S^-1.  Each output may be NULL.  A failed pivot: LAM_HIP_EINVAL with *bad_col (may be NULL) the column and
 * the outputs unspecified; s or dtype out of range, or G NULL: LAM_HIP_EINVAL with *bad_col = -1. */
int lam_hip_block_factor(int s, int dtype, const double *G, double *Ginv, double *S, double *Sinv, int *bad_col);

/* ---- single operators (reference private members / CUDA kernels, for parity tests, roofline
 *      probes and callers that want the BLAS pieces) ------------------------------------------ */

/* y = A x with the production GEMV kernel on the context's matrix.  x_host, y_host: N elements
 * (vector dtype).  Collective in rank mode.  gemv: ConjugateGradient_CPU_MPI_OMP.hpp:482-508,
 * CUDA gemv kernel ConjugateGradient_MultiGPUS_CUDA_NCCL.cu:185-238. */
int lam_hip_gemv(lam_hip_ctx *ctx, const void *x_host, void *y_host);
/* `reps` back-to-back launches of the production GEMV kernel(s) over the local shard(s),
 * timed with HIP events on the launch stream; *sec_per_gemv = average seconds per launch
 * (max over local shards).  No reference counterpart (roofline probe). */
int lam_hip_gemv_only(lam_hip_ctx *ctx, int reps, double *sec_per_gemv);
/* dot (ConjugateGradient_CPU_MPI_OMP.hpp:446-467; CUDA partialDot+reduce :50-131) and axpby
 * (:469-480; CUDA axpy/minusaxpy/xpby :133-183) on host vectors of n elements, run on shard 0's
 * device with the same reduction code the CG kernels use. */
int lam_hip_dot(lam_hip_ctx *ctx, const void *x_host, const void *y_host, uint64_t n, double *result);
int lam_hip_axpby(lam_hip_ctx *ctx, double alpha, const void *x_host, double beta, void *y_host,
                  uint64_t n);
/* The reorthogonalisation pass of lam_hip_eigs alone, ONE pass with the kernels the solve uses, on host vectors; needs no problem
 * and no matrix.  V_host: m vectors of n elements (vector dtype), vector j at V_host + j*n, 1 <= m <= LAM_HIP_MAX_LANCZOS.
 * coeff[j] = V_j.u with fp64 sums of fixed order (may be NULL); then u -= sum_j (TV)coeff[j] V_j as an fma chain in ascending j,
 * written back to u_host.  Columns do not mix in the coefficients: a NaN in V_j reaches coeff[j] and u, and no other coeff. */
int lam_hip_project_out(lam_hip_ctx *ctx, uint64_t n, int m, const void *V_host, void *u_host, double *coeff);

/* max |A[i][j] - A[j][i]| of the matrix held by a single-PROCESS context (one shard or several; every storage type): lets a
 * caller verify the precondition of option "symmetric".  Exact: the fp64 difference of the two stored values, no tolerance.
 * Non-finite elements: a pair the two triangles agree on (infinities of one sign, NaN on both sides, zeros of either sign)
 * counts 0; a pair they disagree on with a NaN or an Inf in it counts +Inf -- the result is then +Inf, never 0 and never NaN.
 * No reference counterpart. */
int lam_hip_check_symmetry(lam_hip_ctx *ctx, double *max_abs_asymmetry);

/* Host-only check of the symmetric product's PLAN (no device needed, no context): builds the task lists of all `shards` row shards
 * of an n x n problem of `dtype` exactly as the launcher does, walks every element of every task through the kernel's own use rule,
 * and reports how many directed products (y_i += A_ij p_j, i and j in [0, n)) are produced not exactly once (*bad_pairs, must be
 * 0) and how many elements of tasks flagged "interior" -- which the kernel processes without any test -- are not used by both
 * sides or lie outside the matrix (*bad_interior, must be 0); *tasks = number of tasks.  shards == 1: the upper triangle; more:
 * cyclic half windows.  O(n^2) time, n^2 / 4 bytes of memory (two bitmaps: 1 GiB at n = 65536, 4 GiB at n = 131072).  The
 * arithmetic is csrc/lam_host_plan.h, which tests/host_asan also builds with g++ -fsanitize=address,undefined.  No reference
 * counterpart. */
int lam_hip_debug_symv_plan(uint64_t n, int shards, int dtype, uint64_t *bad_pairs, uint64_t *bad_interior, uint64_t *tasks);

/* Agreement across ranks (collective in rank mode, identity otherwise): *global_ok = 1 iff every rank passed
 * local_ok != 0.  Lets a step that can fail on ONE rank (reading its row block from a file) fail on ALL of
 * them instead of leaving the others waiting in the next collective.  The reference has MPI_Abort on file
 * errors for this (ConjugateGradient_CPU_MPI_OMP.hpp:325-329). */
int lam_hip_all_ok(lam_hip_ctx *ctx, int local_ok, int *global_ok);

/* Version of the RCCL library this process is bound to (ncclGetVersion; the reference links NCCL 2.18.3,
 * LAM/CMakeLists.txt:11) -- bench.py records it next to its multi-GPU numbers. */
int lam_hip_rccl_version(int *version);
/* Name of the GEMV kernel instantiation the context launches for its current dtype / N / options, e.g.
 * "gemv_coop_kernel<double,double,R=2,TILE=4096,NT=true,UNROLL=4,WAVES=4>" (what a profiler shows).
 * No reference counterpart (the reference has one gemv kernel, NCCL.cu:185-226). */
int lam_hip_gemv_kernel_name(const lam_hip_ctx *ctx, char *buf, size_t len);

/* ---- options --------------------------------------------------------------------------------- */
/* name/value pairs; unknown names -> LAM_HIP_EINVAL.  Options that change which kernels an iteration uses need a new
 * lam_hip_cg_init.  Everything here is the PRODUCT.  Two experiments that were built, measured and lost are kept in
 * liblam_hip_tuning.so only (separate reduction launches, "finalize" = 0; the MFMA-fed bf16 GEMV, "gemv_variant" 20 / 21) and are
 * described in include/lam_hip_tuning.md -- this library refuses to switch them on.  The others (persistent launch, enqueue
 * threads, hub join, 22 GEMV shapes) were removed from both; that file lists them.
 *
 *   "exchange"      how row shards exchange per iteration.  Default 1 in both multi-GPU topologies (rank mode: 0 until round
 *                   4); environment LAM_HIP_EXCHANGE sets the default of new contexts.
 *                     1  gather-Ap: ONE exchange of [Ap slice | p.Ap part] per iteration (one ncclAllGather / one event
 *                        join), r and p full-length on every shard (the reference CPU path's layout, CPU_MPI_OMP.hpp:476,505).
 *                        Any N >= shards: records hold the longest slice of the reference's uneven partition (:176-196).
 *                     0  sliced vectors: 8-byte-per-rank all-gathers for p.Ap and r.r (summed in rank order by the consumer)
 *                        + all-gather of the p slices / three event joins.
 *                     2  DIRECT, EXPERIMENTAL (never yet run on separate GPUs; cross-GPU parity unpinned): peer-mapped
 *                        mailboxes and p replicas, tagged in-kernel hand-overs, no collective and no event in the iteration;
 *                        bit-identical to 0.  lam_hip_solve verifies itself on it ("verify_direct", "direct_fallbacks") and
 *                        falls back to 0; from the environment only together with LAM_HIP_EXPERIMENTAL_DIRECT=1; shards
 *                        sharing a device get it only with LAM_HIP_DIRECT_SAME_DEVICE=1 (tests).
 *                   "exchange_effective" (get) tells what the current CG state runs on.
 *   "exchange_join" one process, exchange 1: 1 (default for > 2 shards) = the join goes through shard 0's stream
 *                   (2(P-1)+1 runtime calls), 0 = every stream waits for every other one (P(P-1)).  Same bits.
 *   "overlap"       rank mode, exchange 0: 1 (default) = all-gather of p on a second stream under the own-slice GEMV panel.
 *                   Exchange 2: 1 = own-slice panel in front of the wait for the peers' slices, 0 = wait first.
 *   "symmetric_many" the batched product (lam_hip_*_many*, lam_hip_solve_mshift's seed) of K <= 4 columns reads every pair once, as
 *                   "symmetric" does for one vector: 0 (default) = the general batched product, bit for bit as before; 2 = always;
 *                   1 = only where it measured faster (a matrix of 192 MiB or more, as "symmetric" has it, and an admitted
 *                   (dtype, K): fp64 and fp32 at K = 1, 2, 4 all are).  Any other value: LAM_HIP_EINVAL, the value in
 *                   force stays.  Setting it is the caller's statement that A = A^T (lam_hip_check_symmetry measures it); no
 *                   environment variable, no automatic check.  One shard, fp64 / fp32, as the batch itself.
 *                   "symmetric_many_effective" (get): 1 if the last batched product launch ran the symmetric kernels, else 0
 *                   (before the first batched product, at K = 8, under value 1 below the threshold).
 *   "packed"        the fp64 general product reads a LOSSLESS 7-byte-per-element image of the matrix instead of A:
 *                   the same bits from 0.89 of the HBM traffic.  -1 (default) = automatic: a matrix content of 8 GiB or more is
 *                   packed (one pass over A, 16 ms at N = 65536) in front of the next product once it has served 65 plain
 *                   products, if the device reports twice the image's size free; 0 = never; 1 = pack in front of the next
 *                   product.  Any other value: LAM_HIP_EINVAL.  Scope: LAM_HIP_F64, one shard, not rank mode, "symmetric" = 0,
 *                   "gemv_variant" = -1, "force_generic" = 0, the whole product (lam_hip_gemv, lam_hip_gemv_only, the
 *                   iteration's and the residual's product; column panels read A); everything else runs as before.  A stays in
 *                   place and every other path reads it; the image (about 0.94 of A's size, grow-only, kept until
 *                   lam_hip_destroy) follows the matrix content: an upload or a generator voids it.  A content with more than
 *                   256 elements of one row and 4096-column tile outside that tile's best window of 7 binades (zero-heavy
 *                   matrices: tridiagonal, heat) is not packable, and a refused allocation is not an error: the plain kernel
 *                   runs.  Results are bit for bit those of the plain kernel, so a switch in the middle of a solve is invisible.
 *                   "packed_effective" (get): 1 if the next product of the context reads the image, else 0;
 *                   "packed_bytes" (get): the bytes one product then reads (0 when not effective) -- stats.gemv_bytes and
 *                   lam_hip_gemv_kernel_name ("gemv_packed_kernel<...>") report the same kernel;
 *                   "packed_pack_ns" (get): what the last pack took (0 when not effective).
 *                   The image belongs to the matrix content: once either reader ("packed", "packed_many") has caused it to be
 *                   built, each reads it wherever its own option is not 0 and its scope holds.
 *   "packed_many"   the general batched product (lam_hip_*_many*, lam_hip_solve_mshift's seed, lam_hip_eigs, lam_hip_solve_block,
 *                   lam_hip_lanczos_many, the deflation set-up) of K <= 4 fp64 columns reads the same image.
 *                   -1 (default) = automatic: under "packed"'s own rules for the content -- 65 products served, single and batched
 *                   ones of K <= 4 counted together, 8 GiB of matrix, twice the image free -- and at the K admitted by measurement:
 *                   K = 1 (0.898 of the plain batched product's time at N = 65536, 0.897 at N = 32768; K = 2: 0.964 and 1.040,
 *                   K = 4: 1.105 and 1.119, both not admitted); 0 = never; 1 = pack in front of the next batched product and
 *                   read the image at every K <= 4.  Any other value: LAM_HIP_EINVAL, the value in force stays.  Independent of
 *                   "packed": "packed" = 0 keeps the single product plain and says nothing about the batch.  Scope: LAM_HIP_F64,
 *                   one shard, as the batch itself (fp32 contexts accept the option and never engage); where "symmetric_many"
 *                   engages it wins.  Results are bit for bit those of the plain batched product under every value, so a switch
 *                   in the middle of a batched solve is invisible; contents that are not packable and refused allocations run
 *                   the plain kernel, as under "packed".
 *                   "packed_many_effective" (get): 1 if the last batched product launch read the image, else 0 (before the
 *                   first batched product, at K = 8, under fp32, where "symmetric_many" engaged, on an unpackable or voided
 *                   content, after a refused allocation).
 *   "symmetric"     the product reads every pair {A[i][j], A[j][i]} ONCE (A must equal its transpose): half the HBM traffic.
 *                   One shard: the upper triangle; several (exchange 1): cyclic half windows per row, each shard contributes
 *                   a full-length vector to the exchange.  1 = where it pays (from 192 MiB of matrix on), 2 = always, 0
 *                   (default) = the reference's general GEMV.  Same results to rounding.  "symmetric_effective" (get).
 *                   Environment LAM_HIP_SYMMETRIC = 1 | 2 (drivers): the library then checks A = A^T itself once per matrix,
 *                   at the first lam_hip_cg_init / lam_hip_solve / lam_hip_gemv / lam_hip_gemv_only on it (one process;
 *                   warns at rounding level, refuses beyond and runs the general GEMV; rank mode: unchecked) and says on
 *                   stderr when the option is not effective (several shards / ranks on an exchange other than 1).
 *                   Rounding level: fp64 / fp32 storage max|A - A^T| <= 64 ulp of the largest finite element; bf16 storage,
 *                   per pair, |A_ij - A_ji| <= max(2^-7 max(|A_ij|, |A_ji|), 64 * 2^-24 max|A|) (one bf16 ulp of the pair).
 *                   A NaN or an Inf on one side of a pair only: refused.  Setting the option with lam_hip_set_option ends
 *                   the environment's check for that context (and lifts a refusal): the caller vouches from then on.
 *   "fuse_update"   1 (default) = the x, r, p updates of an iteration are ONE launch (r.r handed over inside the launch):
 *                   2 launches per shard and iteration.  Used only when the whole grid of all shards / ranks on the device
 *                   is resident ("fuse_effective" tells; "assume_cus" overrides the CU count for tests).  Same bits.
 *   "gemv_timing"   T (default 8): HIP-event pairs bracket the GEMV -- and the exchange step(s) -- of every T-th iteration
 *                   (lam_hip_stats.t_gemv / t_exchange); 0 = never.
 *   "gemv_variant"  -1 (default) = production shape of the dtype (13 fp64, 10 fp32, 0 bf16); 17 = 4 rows per 8-wave
 *                   workgroup (faster at exactly 16 column tiles only); 0, 10 and 13 may be named as well.  20 / 21 (MFMA-fed,
 *                   bf16 storage): tuning build.  Any other number: LAM_HIP_EINVAL.
 *   "nt_loads" 1, "force_generic" 0, "probe_rows", "panel_lo"/"panel_hi"   kernel-level switches for tests and probes.
 *   "packed_after" 65, "packed_min_bytes" 8 GiB   testing, as "assume_cus" / "panel_lo": the two thresholds of "packed" = -1
 *                   (plain products a content serves before it is packed; bytes of matrix from which on), so that the automatic
 *                   switch runs at a size a test can afford.  Negative: LAM_HIP_EINVAL.  No result depends on them; the
 *                   free-memory rule is not theirs to move.
 *   "reuse_matrix"  1 (default) = lam_hip_set_problem keeps the matrix allocation when it is large enough (grow-only).
 *   "upload_staging" 1 = lam_hip_upload_rows copies through two pinned staging buffers (default 0: measured slower).
 *   get only: "row_pitch" (elements between rows on the device), "collectives_enqueued", "rccl_ranks" (ncclCommCount of
 *                   the context's communicator, 0 without one), "ranks_on_device", "gemv_ns_min_shard" / "gemv_ns_max_shard" (fastest /
 *                   slowest local shard's average GEMV of the last cg_iterate call: their difference is the skew), "host_cpu_ns", "host_enqueue_ns",
 *                   "hip_calls_launch" / "_record" / "_wait" / "_setdevice", "tuning_variants" (1 in the tuning build),
 *                   "multi_rhs_k" (columns of the batched kernels the last lam_hip_*_many call ran: 1, 2, 4 or 8; 0 before),
 *                   "deflation_m" (vectors of the deflation space in force, lam_hip_set_deflation*; 0 when none is set or a new
 *                   matrix has invalidated it). */
int lam_hip_set_option(lam_hip_ctx *ctx, const char *name, int64_t value);
int lam_hip_get_option(const lam_hip_ctx *ctx, const char *name, int64_t *value);

#ifdef __cplusplus
}
#endif
#endif /* LAM_HIP_H */
