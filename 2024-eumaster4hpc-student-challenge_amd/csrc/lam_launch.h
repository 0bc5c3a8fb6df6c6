// lam_launch.h -- the blank Finalize (no_finalize), typed kernel launchers (Impl<TA,TV>: GEMV shapes, symmetric product), dtype dispatch, shard resources.
// Part of the one translation unit csrc/lam_hip.hip (included from there, in order; not a stand-alone header).
#pragma once

namespace {

// "no in-kernel reduction" (lam_kernels.h, Finalize): what a launch without a reducer workgroup carries, and the blank every other
// Finalize starts from
Finalize no_finalize(const lam_hip_ctx *c)
{
    Finalize f;
    f.active = 0;
    f.mail = 0;
    f.seq = 0;
    f.dst.n = 0;
    f.slot = 0;
    f.host_err = c ? c->direct_err : nullptr;
    return f;
}

void pack_count_plain(lam_hip_ctx *c);      // below, with the rest of the packed image's host side

// ---- typed implementation ----------------------------------------------------------------------
// (the symmetric product's plan -- SymvPlan, symv_plan -- is host-only arithmetic: lam_host_plan.h)
template <typename TA, typename TV>
struct Impl {
    static constexpr int VEC = MatVec<TA>::N;

    // GEMV shapes (option "gemv_variant"; the numbers are those of the recorded measurements).  The PRODUCT library holds the
    // shapes that are some dtype's default: 13 (gemv_coop_kernel, 2 rows per EIGHT-wave
    // workgroup: fp64 production since round 4 -- half as many concurrent row streams as the 4-wave shape, each read 8 KiB at a
    // time: equal at N=65536, 0.4-2.3 % faster at every other size from 8192 to 131072, profiles/r04_variant_vs_size.txt),
    // 10 (the same with 4 waves: fp32 production, where the two are level), 0 (gemv_tile_kernel, 4 rows per wave: bf16 production)
    // and 17 (4 rows per 8-wave workgroup: an OPTION, 0.5-0.8 % faster than 13 at exactly 16 column tiles -- N=65536, and its row
    // shards -- and slower almost everywhere else; not selected by size).  20 and 21 -- the MFMA-fed bf16
    // GEMV of BASELINE configs[3]'s comparison (slower than the VALU kernel), bf16 storage only -- exist only in the library
    // built with -DLAM_TUNING_VARIANTS (`make tuning` -> liblam_hip_tuning.so; tools/gemv_probe.py, bench.py's MFMA child).
    // Every other number is refused (the shapes that lost: include/lam_hip_tuning.md, "Removed").
    static bool variant_available(int v)
    {
        switch (v) {
        case 0: case 10: case 13: case 17: return true;
#ifdef LAM_TUNING_VARIANTS
        case 20: case 21: return sizeof(TA) == 2;
#endif
        default: return false;
        }
    }
    // rows per WORKGROUP of an available variant
    static int variant_rows_per_block(int v)
    {
        switch (v) {
        case 0: return 16;            // 4 rows per wave
        case 17: return 4;
        case 20: return 8;            // MFMA: 2 rows per wave
        case 21: return 16;           //       4 rows per wave
        default: return 2;            // 10, 13
        }
    }

    // rows are padded to a multiple of 16 bytes at least (lam_hip_ctx::lda), so the vector kernels serve any N; the any-alignment
    // kernel runs on request only (option force_generic: tests, comparisons)
    static bool fast_ok(const lam_hip_ctx *c) { return !c->opt_generic; }
    static int variant(const lam_hip_ctx *c)
    {
        if (c->opt_gemv_variant >= 0 && variant_available((int)c->opt_gemv_variant)) return (int)c->opt_gemv_variant;
        // production shapes: fp64 -> cooperative rows, 8 waves (variant 13); fp32 -> cooperative rows, 4 waves (variant 10);
        // bf16 storage spends more VALU per byte (widening) and measures best with 4 rows per wave (variant 0)
        return sizeof(TA) == 2 ? 0 : (sizeof(TA) == 8 ? 13 : 10);
    }

    // name of the kernel instantiation launch_gemv() picks for this context (roofline records)
    static std::string kernel_name(const lam_hip_ctx *c)
    {
        const char *ta = sizeof(TA) == 8 ? "double" : (sizeof(TA) == 4 ? "float" : "__hip_bfloat16");
        const char *tv = sizeof(TV) == 8 ? "double" : "float";
        char buf[192];
        if (c->symv_active()) { snprintf(buf, sizeof buf, "symv_task_kernel<%s,NV=1> + symv_reduce_kernel<%s,NV=1>", ta, ta); return buf; }
        if (!fast_ok(c)) { snprintf(buf, sizeof buf, "gemv_generic_kernel<%s,%s>", ta, tv); return buf; }
        if (c->pack_active()) {
            snprintf(buf, sizeof buf, "gemv_packed_kernel<double,double,R=2,TILE=4096,NT=%s,WAVES=8>", c->opt_nt ? "true" : "false");
            return buf;
        }
        const int v = variant(c);
        const char *nt = c->opt_nt ? "true" : "false";
        if (v == 0) snprintf(buf, sizeof buf, "gemv_tile_kernel<%s,%s,R=4,TILE=4096,NT=%s,UNROLL=4,LDS=true,ROT=true>", ta, tv, nt);
        else if (v >= 20) snprintf(buf, sizeof buf, "gemv_mfma_bf16_kernel<R=%d,TILE=4096,NT=true,SPLIT=%d>", v == 20 ? 2 : 4, v == 20 ? 1 : 3);
        else
            snprintf(buf, sizeof buf, "gemv_coop_kernel<%s,%s,R=%d,TILE=4096,NT=%s,UNROLL=4,WAVES=%d>", ta, tv, variant_rows_per_block(v), nt,
                     v == 10 ? 4 : 8);
        return buf;
    }

    // number of p.Ap partials the product step of a CG iteration leaves in part_gemv
    static int gemv_grid(const lam_hip_ctx *c, uint64_t nrows)
    {
        if (nrows == 0) return 0;
        if (c->symv_active()) return symv_reduce_grid(c->n);      // symmetric product: one per 32 rows of the second pass
        return kernel_grid(c, nrows);
    }

    // workgroups of the general GEMV kernel (also used on its own by the residual check)
    static int kernel_grid(const lam_hip_ctx *c, uint64_t nrows)
    {
        if (nrows == 0) return 0;
        const uint64_t rows_per_block = fast_ok(c) ? (uint64_t)variant_rows_per_block(variant(c)) : (uint64_t)kWaves;
        return (int)((nrows + rows_per_block - 1) / rows_per_block);
    }

    static void launch_tile(const lam_hip_ctx *c, int grid, hipStream_t st, const GemvArgs<TA, TV> &a)
    {
        if (c->opt_nt)
            hipLaunchKernelGGL((gemv_tile_kernel<TA, TV, true>), dim3(grid), dim3(kBlock), 0, st, a);
        else
            hipLaunchKernelGGL((gemv_tile_kernel<TA, TV, false>), dim3(grid), dim3(kBlock), 0, st, a);
    }

    // y = A p reading every pair {i, j} once (lam_kernels.h, "Symmetric product").  The task list is built on first use.
    // One shard: the upper triangle -- strip st (SS columns) holds rows [0, min(n, c0 + SS)), cut into runs of `tall` rows up to
    // row 0.65 n and of `tall / 8` rows below (the launch dispatches tasks in list order and so ends on short ones).  Several
    // row shards: every row of the shard takes the cyclic window of (N-1)/2 columns behind its diagonal (symv_use), i.e. the
    // strips that window touches; runs of `tall` rows, `tall / 8` for the last 15 % of the shard's rows.  The list is ordered
    // by first row, strips of one row run side by side (whole rows stream, as in the GEMV).  Shapes from tools/symv2_probe
    // (profiles/r04_symv2_probe.txt): one 16-byte vector per lane and row (a 4-KiB strip per workgroup); one shard: tall = 256
    // rows from N = 16384 on; several: tall so that a shard has >= ~6000 tasks.
    // The two passes.  dst null: one shard, y = A p and `partial` = the p.y partials (symv_reduce_grid(n) of them).  dst set:
    // several shards, the shard's full-length contribution goes into dst->p[] (its record in every shard's gather buffer), and `fin`
    // says where the reducer workgroup of the second pass writes the shard's part of p.Ap.
    static int symv_reduce_grid(uint64_t n) { return (int)((n + kSymvReduceRows - 1) / kSymvReduceRows); }
    static int launch_symv(lam_hip_ctx *c, ShardBase &s, const TV *p, TV *y, double *partial, const CgScalars *sc, const PtrList *dst = nullptr,
                           const Finalize *fin = nullptr)
    {
        PtrList d;
        d.n = 0;
        if (dst) d = *dst;
        const Finalize f = fin ? *fin : no_finalize(c);
        const bool cyc = d.n > 0;
        const uint64_t n = c->n, ncv = c->ncols_vec();
        SymvDevPlan &v = s.symv;
        if (v.tasks == nullptr)
            LAMCHK(symv_dev_build(c, v, n, ncv, (uint64_t)kBlock * VEC, s.row0, s.nrows, cyc, sizeof(TV), 1, s.stream, "symmetric product"));
        constexpr unsigned lds_pad = symv_lds_pad<TV, 1>();
        hipLaunchKernelGGL((cyc ? symv_task_kernel<TA, TV, true> : symv_task_kernel<TA, TV, false>), dim3(v.ntasks), dim3(kBlock), lds_pad,
                           s.stream, (const TA *)s.A, p, (const SymvTask *)v.tasks, (TV *)v.rowpart, (TV *)v.colpart, c->lda, ncv, n, s.row0, sc);
        HIPCHK(c, hipGetLastError());
        hipLaunchKernelGGL((symv_reduce_kernel<TV, kBlock * VEC>), dim3(symv_reduce_grid(n) + (f.active ? 1 : 0)), dim3(kBlock), 0, s.stream,
                           (const TV *)v.rowpart, (const TV *)v.colpart, (const uint32_t *)v.index, v.ix, p, y,
                           partial, n, s.row0, s.nrows, d, f, sc);
        HIPCHK(c, hipGetLastError());
        c->n_launch += 2;
        return 0;
    }

    // panel: 0 = whole GEMV; 1 = only columns [lo,hi); 2 = everything but [lo,hi), accumulated onto y
    template <int R, int WAVES>
    static void launch_coop(const lam_hip_ctx *c, int grid, hipStream_t st, const GemvArgs<TA, TV> &a)
    {
        if (c->opt_nt)
            hipLaunchKernelGGL((gemv_coop_kernel<TA, TV, R, true, WAVES>), dim3(grid), dim3(WAVES * 64), 0, st, a);
        else
            hipLaunchKernelGGL((gemv_coop_kernel<TA, TV, R, false, WAVES>), dim3(grid), dim3(WAVES * 64), 0, st, a);
    }

    static int launch_gemv(lam_hip_ctx *c, ShardBase &s, const TV *p, TV *y, double *partial, const CgScalars *sc,
                           int panel = 0, uint64_t lo = 0, uint64_t hi = 0, const Finalize *fin = nullptr, const PtrList *ypeers = nullptr)
    {
        if (s.nrows == 0) return 0;
        GemvArgs<TA, TV> a;
        a.A = (const TA *)s.A; a.p = p; a.y = y; a.partial = partial; a.sc = sc;
        a.n_ypeer = 0;
        for (auto &yp : a.ypeer) yp = nullptr;
        if (ypeers != nullptr)
            for (int j = 0; j < ypeers->n && a.n_ypeer < kMaxShards - 1; j++) a.ypeer[a.n_ypeer++] = (TV *)ypeers->p[j];
        a.fin = (fin != nullptr && partial != nullptr) ? *fin : no_finalize(c);
        a.nrows = s.nrows; a.n = c->n; a.row0 = s.row0; a.lda = c->lda;
        // the vector kernels cover whole 16-byte vectors: for an N that is not a multiple of the vector width the last one
        // reaches into the (zero) padding of the row and behind the end of p (zero too: set_problem)
        const uint64_t ncols = fast_ok(c) ? c->ncols_vec() : c->n;
        if (fast_ok(c) && hi == c->n) hi = ncols;
        a.seg_begin[0] = 0; a.seg_end[0] = ncols; a.seg_begin[1] = a.seg_end[1] = 0; a.nseg = 1; a.accumulate = 0;
        if (panel == 1) { a.seg_begin[0] = lo; a.seg_end[0] = hi; }
        else if (panel == 2) {
            a.accumulate = 1;
            a.nseg = 0;
            if (lo > 0) { a.seg_begin[a.nseg] = 0; a.seg_end[a.nseg] = lo; a.nseg++; }
            if (hi < ncols) { a.seg_begin[a.nseg] = hi; a.seg_end[a.nseg] = ncols; a.nseg++; }
            if (a.nseg == 0) return 0;
            if (a.nseg == 1) { a.seg_begin[1] = a.seg_end[1] = 0; }
        }
        const int grid = kernel_grid(c, s.nrows) + (a.fin.active ? 1 : 0);     // + the reducer workgroup (Finalize)
        if constexpr (sizeof(TA) == 8) {
            // the packed image (option "packed"): the whole product of the default shape only; panels read A
            if (panel == 0 && c->pack_eligible()) {
                PackState &pk = c->pack;
                if (c->pack_active() && s.nrows <= pk.nrows) {
                    const PackLayout L = pack_layout(pk.nrows, pk.ntiles);
                    PackedMat m;
                    m.data = (const unsigned char *)pk.buf + L.data;
                    m.exc = (const double *)((const char *)pk.buf + L.exc);
                    m.hdr = (const uint32_t *)((const char *)pk.buf + L.hdr);
                    m.ntiles = (uint32_t)pk.ntiles;
                    if (c->opt_nt) hipLaunchKernelGGL((gemv_packed_kernel<true>), dim3(grid), dim3(512), 0, s.stream, a, m);
                    else hipLaunchKernelGGL((gemv_packed_kernel<false>), dim3(grid), dim3(512), 0, s.stream, a, m);
                    LAUNCHED(c);
                    return 0;
                }
                pack_count_plain(c);
            }
        }
        if (fast_ok(c)) {
            switch (variant(c)) {
            default:
            case 0: launch_tile(c, grid, s.stream, a); break;
            case 10: launch_coop<2, 4>(c, grid, s.stream, a); break;
            case 13: launch_coop<2, 8>(c, grid, s.stream, a); break;
            case 17: launch_coop<4, 8>(c, grid, s.stream, a); break;
#ifdef LAM_TUNING_VARIANTS
            case 20: case 21:                          // variant_available: bf16 storage only
                if constexpr (sizeof(TA) == 2) {
                    if (variant(c) == 20) hipLaunchKernelGGL((gemv_mfma_bf16_kernel<2, 4096, true, 1>), dim3(grid), dim3(kBlock), 0, s.stream, a);
                    else hipLaunchKernelGGL((gemv_mfma_bf16_kernel<4, 4096, true, 3>), dim3(grid), dim3(kBlock), 0, s.stream, a);
                }
                break;
#endif
            }
        } else {
            hipLaunchKernelGGL((gemv_generic_kernel<TA, TV>), dim3(grid), dim3(kBlock), 0, s.stream, a);
        }
        LAUNCHED(c);
        return 0;
    }
};

// The packed image belongs to the matrix content; either of its readers may cause it to be built (pack_maybe below for the single
// product, pack_many_maybe in lam_multi.h for the batched one), and both read whatever image holds the current matrix_gen.
// pack_auto_due: automatic mode's two thresholds, shared by the readers -- the content has served "packed_after" plain products (kPackAfter;
// single and batched ones of an eligible shape count on the one counter, pack_count_plain) and the matrix has "packed_min_bytes" (kPackMinBytes).
// pack_build: the image of the current content -- allocation (grow-only; automatic mode wants twice the image free), one pass of
// pack_rows_kernel on the shard's stream, outside every timing event pair (the callers sit in front of the product step), the
// refusal bookkeeping.  Never an error of its own: no memory, or a (row, tile) with more than kPackCap exceptions, and the plain
// kernels go on running for this content.
int set_dev(lam_hip_ctx *c, const ShardBase &s);
bool pack_auto_due(const lam_hip_ctx *c)
{
    const PackState &pk = c->pack;
    if (pk.count_gen != c->matrix_gen || pk.plain < (uint64_t)c->opt_packed_after) return false;
    return c->sh[0].nrows * c->lda * 8ull >= (uint64_t)c->opt_packed_min_bytes;
}
void pack_count_plain(lam_hip_ctx *c)
{
    PackState &pk = c->pack;
    if (pk.count_gen != c->matrix_gen) { pk.count_gen = c->matrix_gen; pk.plain = 0; }
    pk.plain++;
}
int pack_build(lam_hip_ctx *c, bool automatic)
{
    PackState &pk = c->pack;
    if (pk.ready_gen == c->matrix_gen || pk.refused_gen == c->matrix_gen) return 0;
    ShardBase &s = c->sh[0];
    const uint64_t ncols = c->ncols_vec();
    const uint64_t ntiles = (ncols + kPackTile - 1) / kPackTile;
    const PackLayout L = pack_layout(s.nrows, ntiles);
    const size_t need = L.total + 256;                      // + the pass's two result words
    LAMCHK(set_dev(c, s));
    if (pk.cap < need) {
        if (automatic) {
            size_t free_b = 0, total_b = 0;
            if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); free_b = 0; }
            if (free_b + pk.cap < 2 * need) { pk.refused_gen = c->matrix_gen; return 0; }
        }
        HIPCHK(c, hipStreamSynchronize(s.stream));
        if (pk.buf != nullptr) { (void)hipFree(pk.buf); pk.buf = nullptr; pk.cap = 0; }
        if (hipMalloc(&pk.buf, need) != hipSuccess) {
            (void)hipGetLastError();
            pk.buf = nullptr;
            pk.refused_gen = c->matrix_gen;
            return 0;
        }
        pk.cap = need;
    }
    pk.ready_gen = ~0ull;
    pk.nrows = s.nrows; pk.ntiles = ntiles;
    unsigned long long *info = (unsigned long long *)((char *)pk.buf + L.total);
    unsigned long long got[2] = {0, 0};
    HIPCHK(c, hipStreamSynchronize(s.stream));
    const double t0 = now_s();
    HIPCHK(c, hipMemsetAsync(info, 0, 16, s.stream));
    hipLaunchKernelGGL(pack_rows_kernel, dim3((unsigned)s.nrows), dim3(kBlock), 0, s.stream, (const double *)s.A, c->lda, ncols, (uint32_t)ntiles,
                       (unsigned char *)pk.buf + L.data, (uint64_t *)((char *)pk.buf + L.exc), (uint32_t *)((char *)pk.buf + L.hdr), info);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(got, info, 16, hipMemcpyDeviceToHost, s.stream));
    HIPCHK(c, hipStreamSynchronize(s.stream));
    pk.pack_s = now_s() - t0;
    if (got[0] != 0) { pk.refused_gen = c->matrix_gen; return 0; }
    pk.exc_total = got[1];
    pk.ready_gen = c->matrix_gen;
    return 0;
}

// Option "packed": who is due for the single product -- value 1: now; auto: pack_auto_due
int pack_maybe(lam_hip_ctx *c)
{
    if (!c->pack_eligible() || !c->have_matrix) return 0;
    const bool automatic = c->opt_packed < 0;
    if (automatic && !pack_auto_due(c)) return 0;
    return pack_build(c, automatic);
}

// bytes one product of the shard reads: the plain kernel's, or the packed image's elements, headers and exception-list values
double gemv_bytes_now(const lam_hip_ctx *c, const ShardBase &s0)
{
    const double vec = (double)c->esz_v() * (double)(c->n + s0.nrows);
    if (!c->pack_active()) return (double)c->esz_a() * (double)s0.nrows * (double)c->n + vec;
    const double units = (double)s0.nrows * (double)c->pack.ntiles;
    return units * (double)(kPackTileBytes + 4) + 8.0 * (double)c->pack.exc_total + vec;
}

// The typed bodies of the host code are written as generic lambdas over Impl<TA,TV>; TA / TV are recovered with this small trait.
template <typename T> struct ImplTraits;
template <typename TA_, typename TV_> struct ImplTraits<Impl<TA_, TV_>> { using TA = TA_; using TV = TV_; };

// Own-slice panel [lo,hi) of the CG GEMV, or lo == hi when the GEMV stays one launch.  Panels need
// 16-byte aligned segment starts (lo, hi multiples of the vector width) unless the generic kernel runs.
template <typename I>
void cg_panel(const lam_hip_ctx *c, const ShardBase &s, uint64_t *lo, uint64_t *hi)
{
    *lo = *hi = 0;
    uint64_t a = 0, b = 0;
    if (c->opt_panel_hi > c->opt_panel_lo) { a = (uint64_t)c->opt_panel_lo; b = std::min<uint64_t>((uint64_t)c->opt_panel_hi, c->n); }
    else if (c->rank_mode && c->opt_overlap && c->nranks > 1) { a = s.row0; b = s.row0 + s.nrows; }
    if (b <= a || (a == 0 && b >= c->n)) return;
    if (I::fast_ok(c) && (a % I::VEC != 0 || (b % I::VEC != 0 && b != c->n))) return;
    *lo = a; *hi = b;
}

template <typename F>
int dispatch(lam_hip_ctx *c, F &&f)
{
    switch (c->dtype) {
    case LAM_HIP_F64: return f(Impl<double, double>());
    case LAM_HIP_F32: return f(Impl<float, float>());
    case LAM_HIP_BF16: return f(Impl<__hip_bfloat16, float>());
    }
    return fail(c, LAM_HIP_EINVAL, "bad dtype %d", c->dtype);
}

int set_dev(lam_hip_ctx *c, const ShardBase &s)
{
    c->n_setdev++;
    HIPCHK(c, hipSetDevice(s.dev));
    // hipGetLastError() is only used to pick up launch failures right after a launch; drop whatever an
    // earlier, already reported failure (possibly of another context) left in the thread's error slot
    (void)hipGetLastError();
    return 0;
}

PtrList plist_p(lam_hip_ctx *c)
{
    PtrList l;
    l.n = (int)c->sh.size();
    for (int j = 0; j < l.n; j++) l.p[j] = c->sh[j].p;
    return l;
}
PtrList plist_gather(lam_hip_ctx *c, bool second)
{
    PtrList l;
    l.n = (int)c->sh.size();
    for (int j = 0; j < l.n; j++) l.p[j] = second ? (void *)c->sh[j].gather_b : (void *)c->sh[j].gather_a;
    return l;
}

// keep_matrix: leave the matrix allocation alone (lam_hip_set_problem re-uses it when it is large enough)
void free_shard(ShardBase &s, bool keep_matrix = false)
{
    if (hipSetDevice(s.dev) != hipSuccess) { (void)hipGetLastError(); return; }   // never created on a real device
    void *const keepA = keep_matrix ? s.A : nullptr;
    const size_t keepCap = keep_matrix ? s.A_capacity : 0;
    if (keep_matrix) s.A = nullptr;
    // the row-transfer staging buffer belongs to the context, not to a problem: released only with the matrix
    if (!keep_matrix && s.xfer_stage) { (void)hipFree(s.xfer_stage); s.xfer_stage = nullptr; s.xfer_stage_bytes = 0; }
    void *ptrs[] = {s.A, s.p, s.Ap, s.x, s.r, s.b, s.tmp, s.part_gemv, s.part_vec, s.gather_a, s.gather_b, s.sc,
                    s.r_full, s.ap_gather, s.symv_gather, s.part_aux};
    for (void *q : ptrs) if (q) (void)hipFree(q);
    symv_dev_release(s.symv);
    s.r_full = s.ap_gather = s.symv_gather = nullptr;
    s.symv_gather_bytes = 0;
    if (s.sc_host) (void)hipHostFree(s.sc_host);
    if (s.host_flags) (void)hipHostFree(s.host_flags);
    s.host_flags = nullptr;
    s.A = s.p = s.Ap = s.x = s.r = s.b = s.tmp = nullptr;
    s.A = keepA;
    s.A_capacity = keepCap;
    s.part_gemv = s.part_vec = s.gather_a = s.gather_b = nullptr;
    s.part_aux = nullptr;
    s.sc = nullptr; s.sc_host = nullptr;
}

// streams and events of one shard (device memory is released by free_shard)
void release_handles(ShardBase &s)
{
    if (hipSetDevice(s.dev) != hipSuccess) { (void)hipGetLastError(); return; }
    hipEvent_t *evs[] = {&s.ev_a, &s.ev_b, &s.ev_p, &s.ev_gathered};
    for (auto e : evs) if (*e) { (void)hipEventDestroy(*e); *e = nullptr; }
    for (int i = 0; i < kLag; i++) {
        hipEvent_t *ring[] = {&s.ev_g0[i], &s.ev_g1[i], &s.ev_g2[i], &s.ev_g3[i]};
        for (auto e : ring) if (*e) { (void)hipEventDestroy(*e); *e = nullptr; }
    }
    for (int i = 0; i < kLag; i++)
        for (auto &e : s.ev_x[i]) if (e) { (void)hipEventDestroy(e); e = nullptr; }
    if (s.comm_stream) { (void)hipStreamSynchronize(s.comm_stream); (void)hipStreamDestroy(s.comm_stream); s.comm_stream = nullptr; }
    if (s.stream) { (void)hipStreamSynchronize(s.stream); (void)hipStreamDestroy(s.stream); s.stream = nullptr; }
}

// the context's join event (gather-Ap exchange, on shard 0's device)
void release_join(lam_hip_ctx *c)
{
    if (c->sh.empty() || hipSetDevice(c->sh[0].dev) != hipSuccess) { (void)hipGetLastError(); return; }
    if (c->ev_join) { (void)hipEventDestroy(c->ev_join); c->ev_join = nullptr; }
}

// a context whose creation failed half-way: give back what it already holds
void abandon(lam_hip_ctx *c)
{
    release_join(c);
    for (auto &s : c->sh) { free_shard(s); release_handles(s); }
    if (c->direct_err) { (void)hipHostFree(c->direct_err); c->direct_err = nullptr; }
}

}  // namespace
