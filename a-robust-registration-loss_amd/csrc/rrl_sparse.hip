// rrl_sparse.hip -- everything after the dense scan, plus the fused forward/backward entries.
//   K2 line_pair_dist   code/loss.py:115-167   (one lane per line, <= 4x4 block in registers)
//   K3+K4 loss_reduce   code/loss.py:223-230   (radix-select median + Welsch min/mean, one
//                                               workgroup per sample, fixed-point bucket sums)
//   K5 backward         autograd of code/loss.py:170-232
// About 9 % of the lines are selected; these kernels touch O(L) data and are latency bound
// (a few microseconds each) next to the O(L*(N+M)) scan.
// The kernels live in the four stage headers below, their argument structs in rrl_stage_args.h; this file keeps the
// argument fillers, the launchers and the extern "C" entries.  The record, the plan and the validation of a call, the
// process-wide knobs and the workspace description: rrl_call.hip.
#include <stdlib.h>

#include "rrl_ws.h"
#include "rrl_stage_pair.h"    // K2: the per-line stage
#include "rrl_stage_reduce.h"  // K3 + K4: single-workgroup and exchange reduce
#include "rrl_stage_tail.h"    // K3 + K4 (+ K5): the tail kernel; the single-tile forward kernel
#include "rrl_stage_bwd.h"     // K5: backward variants

#ifdef RRL_STAMPS  // experiments only: the tables of rrl_stamps.h, read back (tools/stamps*.py)
extern "C" int rrl_debug_stamps(unsigned long long *out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * 32) == hipSuccess ? 0 : -1;
}
extern "C" int rrl_debug_wstamps(unsigned long long *out, int clear) {
    if (clear) { void *p_ = nullptr; if (hipGetSymbolAddress(&p_, HIP_SYMBOL(g_wstamps)) != hipSuccess) return -1; return hipMemset(p_, 0, sizeof(unsigned long long) * 12 * 2048) == hipSuccess ? 0 : -1; }
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wstamps), sizeof(unsigned long long) * 12 * 2048) == hipSuccess ? 0 : -1;
}
extern "C" int rrl_debug_pstamps(unsigned long long *out, int clear) {
    if (clear) { void *p_ = nullptr; if (hipGetSymbolAddress(&p_, HIP_SYMBOL(g_pstamps)) != hipSuccess) return -1; return hipMemset(p_, 0, sizeof(unsigned long long) * 8 * 2048) == hipSuccess ? 0 : -1; }
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_pstamps), sizeof(unsigned long long) * 8 * 2048) == hipSuccess ? 0 : -1;
}
#endif

// Cloud 2's hit counts / hit lists are read where its scan left them (RrlCall::tar_i32) -- with a carried-over target the
// workspace of the evaluation it was carried over from (round 4b: they used to be copied into this workspace first, two
// launches per evaluation).  tally: the launch feeds the tiled reduces' histogram (not the single-tile kernels).
static PairArgs pair_args(const RrlCall &o, const float *tri1, const float *tri2, const float *line, bool tally) {
    PairArgs a;
    a.mhist = tally ? (uint32_t *)o.at<RRL_WS_MHIST>() : nullptr;
    a.mctl = tally ? (uint32_t *)o.at<RRL_WS_MCTL>() : nullptr;
    a.tri1 = tri1;
    a.tri2 = tri2;
    a.line = line;
    a.count1 = o.at<RRL_WS_COUNT1>(); a.hit1 = o.at<RRL_WS_HIT1>();
    a.count2 = o.tar_at<RRL_WS_COUNT2>(); a.hit2 = o.tar_at<RRL_WS_HIT2>();
    a.kj = o.at<RRL_WS_KJ>();
    a.sel_out = o.at<RRL_WS_SEL>(); a.nsel = o.at<RRL_WS_NSEL>();
    a.hs1 = o.at<RRL_WS_HS1>(); a.hs2 = o.at<RRL_WS_HS2>();
    a.w1 = o.at<RRL_WS_W1>(); a.w2 = o.at<RRL_WS_W2>();
    a.Q1 = (float4 *)o.at<RRL_WS_Q1>(); a.Q2 = (float4 *)o.at<RRL_WS_Q2>();
    a.D = o.at<RRL_WS_D>(); a.dc = o.at<RRL_WS_VALS>();
    a.kjc = o.at<RRL_WS_KJC>(); a.blkcnt = o.at<RRL_WS_BLKCNT>();
    a.lidc = (uint32_t *)o.at<RRL_WS_LIDC>();
    a.vlist = o.at<RRL_WS_VLIST>(); a.vlcnt = o.at<RRL_WS_VLCNT>();
    a.B = o.B; a.N = o.N; a.M = o.M; a.L = o.L;
    a.s_m = o.s_m; a.s_n = o.s_n; a.e_m = o.e_m; a.e_n = o.e_n;
    a.st1 = 9; a.st2 = 9;
    a.Bt = o.problems;  // multi-pose (RrlCall::problems)
    a.xcd_align = o.B % 8 == 0 && xcd_align_on();
    a.zc1 = a.zc2 = nullptr;
    return a;
}

static int line_pair_dist_impl(const RrlCall &o, const float *tri1, const float *tri2, const float *line) {
    const int B = o.B, L = o.L;
    if (B == 0 || L == 0) return 0;
    PairArgs pa = pair_args(o, tri1, tri2, line, true);
    if (o.plan.leave_clean) { pa.zc1 = o.at<RRL_WS_COUNT1>(); pa.zc2 = o.at<RRL_WS_COUNT2>(); }
    if (o.plan.reduce != RRL_RED_TAIL) pa.vlist = nullptr;  // only the tail kernel reads VLIST
    if (o.plan.count_rides) {  // the next epoch's count pass rides along (pair_count_kernel)
        RrlCountRider *cr = o.count_rider;
        const int ctiles = (cr->n + 1023) / 1024;
        const CountKArgs c = {cr->rng_state, cr->r, cr->centers, cr->aabb2, cr->rows, cr->accept, cr->n_rows, cr->n,
                              cr->rounds, rrl_sample_prefilter(), ctiles, cr->rounds};
        const int pgx = (L + 1023) / 1024;
        hipLaunchKernelGGL(pair_count_kernel, dim3((unsigned)(ctiles * cr->rounds + pgx * B)), dim3(1024), 0, o.s, pa, c, pgx);
        RRL_LAUNCH_CHECK();
        cr->done = 1;
        return 0;
    }
    hipLaunchKernelGGL(line_pair_dist_kernel, dim3((unsigned)((L + 1023) / 1024), (unsigned)B), dim3(1024), 0, o.s, pa);
    RRL_LAUNCH_CHECK();
    return 0;
}

extern "C" int rrl_line_pair_dist_ex(const float *tri1, const float *tri2, const float *line,
                                     void *ws, size_t ws_bytes, int B, int N, int M, int L, int s_m,
                                     int s_n, int e_m, int e_n, int pool, const rrl_opts *opts, void *stream) {
    RrlCall o = rrl_begin_call(opts, B, N, M, L, ws, ws_bytes, stream);
    o.set(s_m, s_n, e_m, e_n, pool);
    if (const int rc = rrl_check_call(o, tri1 && tri2 && line, RRL_WANT_STAGE)) return rc;
    return line_pair_dist_impl(o, tri1, tri2, line);
}
extern "C" int rrl_line_pair_dist(const float *tri1, const float *tri2, const float *line,
                                  void *ws, size_t ws_bytes, int B, int N, int M, int L, int s_m,
                                  int s_n, int e_m, int e_n, int pool, void *stream) {
    return rrl_line_pair_dist_ex(tri1, tri2, line, ws, ws_bytes, B, N, M, L, s_m, s_n, e_m, e_n, pool, nullptr, stream);
}

// Workgroups of loss_reduce_tiled_kernel that are co-resident on the CURRENT device when it has the device to itself:
// compute units (as the runtime reports them: a CPX partition or a CU mask reports fewer) x the occupancy the
// runtime computes for this kernel.  (Round 3 hard-coded 1024 = 256 CUs x 4.)  Co-residency is a matter of speed only
// since round 4 -- a workgroup that waits in vain is repaired by its sample's last workgroup -- but a grid beyond the
// capacity would make that slow path the usual one, so the exchange kernel is only chosen within it.
long rrl_xchg_capacity() {
    static long cap[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (cap[dev] == 0) {
        hipDeviceProp_t p;
        int per_cu = 0;
        long c = 256;
        if (hipGetDeviceProperties(&p, dev) == hipSuccess &&
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, loss_reduce_tiled_kernel, 256, 0) == hipSuccess && per_cu > 0)
            c = (long)p.multiProcessorCount * per_cu;
#ifdef RRL_EXPERIMENT
        if (const char *e = getenv("RRL_XCHG_CAPACITY")) c = atol(e);
#endif
        cap[dev] = c < 1 ? 1 : (c > 4096 ? 4096 : c);
    }
    return cap[dev];
}

// the direct backward that may ride in the tail kernel's launch (rrl_registration_step)
struct TailBwd {
    const float *grad_loss, *src;
    float *gR, *gt, *payload;
    int transpose_r;
    float *grad_tri1;  // scatter target (rrl_loss_step) instead of (gR, gt)
};

static ReduceArgs reduce_args(const RrlCall &o, float *loss) {
    ReduceArgs r;
    r.kjc = o.at<RRL_WS_KJC>(); r.dc = o.at<RRL_WS_VALS>(); r.blkcnt = o.at<RRL_WS_BLKCNT>();
    r.med_out = o.at<RRL_WS_MED>(); r.bcnt_out = o.at<RRL_WS_BCNT>(); r.bsum_out = o.at<RRL_WS_BSUM>();
    r.info = o.at<RRL_WS_INFO>(); r.loss = loss; r.status = o.at<RRL_WS_STATUS>();
    r.B = o.B; r.nblk = (o.L + 1023) / 1024;
    r.s_m = o.s_m; r.s_n = o.s_n; r.e_m = o.e_m; r.e_n = o.e_n; r.pool = o.pool;
    return r;
}

// tb: the backward that rides in the tail kernel's launch (o.plan.bwd_rides), else NULL
static TailArgs tail_args(const RrlCall &o, float *loss, const TailBwd *tb) {
    TailArgs t;
    t.lidc = (uint32_t *)o.at<RRL_WS_LIDC>(); t.dc = o.at<RRL_WS_VALS>(); t.blkcnt = o.at<RRL_WS_BLKCNT>();
    t.vlist = o.at<RRL_WS_VLIST>(); t.vlcnt = o.at<RRL_WS_VLCNT>();
    t.mhist = (uint32_t *)o.at<RRL_WS_MHIST>(); t.mctl = (uint32_t *)o.at<RRL_WS_MCTL>();
    t.msum = (unsigned long long *)o.at<RRL_WS_MSUM>();
    t.med_out = o.at<RRL_WS_MED>(); t.bcnt_out = o.at<RRL_WS_BCNT>(); t.bsum_out = o.at<RRL_WS_BSUM>();
    t.info = o.at<RRL_WS_INFO>(); t.loss = loss; t.status = o.at<RRL_WS_STATUS>();
    t.B = o.B; t.nblk = (o.L + 1023) / 1024; t.s_m = o.s_m; t.s_n = o.s_n; t.e_m = o.e_m; t.e_n = o.e_n;
    const TailBwd none{}, &b = tb ? *tb : none;  // (no riding backward: all NULL)
    t.do_bwd = tb ? 1 : 0; t.N = o.N; t.L = o.L; t.transpose_r = b.transpose_r;
    t.hs1 = o.at<RRL_WS_HS1>(); t.w1 = o.at<RRL_WS_W1>();
    t.Q1 = (const float4 *)o.at<RRL_WS_Q1>(); t.Q2 = (const float4 *)o.at<RRL_WS_Q2>();
    t.grad_loss = b.grad_loss; t.src = b.src; t.gR = b.gR; t.gt = b.gt; t.payload = b.payload; t.grad_tri1 = b.grad_tri1;
    t.Bt = o.problems;
    t.xcd_align = o.B % 8 == 0 && xcd_align_on();
    t.chain = o.plan.leave_clean ? (uint32_t *)o.at<RRL_WS_CHAIN>() : nullptr;
    t.chain_flags = o.plan.fused_build;
    return t;
}

static TiledArgs tiled_args(const RrlCall &o, float *loss) {
    TiledArgs t;
    t.kjc = o.at<RRL_WS_KJC>(); t.dc = o.at<RRL_WS_VALS>(); t.blkcnt = o.at<RRL_WS_BLKCNT>();
    t.mhist = (uint32_t *)o.at<RRL_WS_MHIST>(); t.mctl = (uint32_t *)o.at<RRL_WS_MCTL>(); t.mcand = (uint32_t *)o.at<RRL_WS_MCAND>();
    t.msum = (unsigned long long *)o.at<RRL_WS_MSUM>();
    t.med_out = o.at<RRL_WS_MED>(); t.bcnt_out = o.at<RRL_WS_BCNT>(); t.bsum_out = o.at<RRL_WS_BSUM>();
    t.info = o.at<RRL_WS_INFO>(); t.loss = loss; t.status = o.at<RRL_WS_STATUS>();
    t.B = o.B; t.nblk = (o.L + 1023) / 1024; t.s_m = o.s_m; t.s_n = o.s_n; t.e_m = o.e_m; t.e_n = o.e_n;
    t.spin_limit = rrl_default_spin_limit();
    t.xcd_align = o.B % 8 == 0 && xcd_align_on();
    t.payload = o.plan.payload_in_reduce ? o.payload : nullptr;
    t.chain = o.plan.leave_clean ? (uint32_t *)o.at<RRL_WS_CHAIN>() : nullptr;
    t.chain_flags = o.plan.fused_build;
    return t;
}

// the next epoch's sampler write pass, riding in the launch that carries the direct backward (rrl_ws.h RrlWriteRider)
static WriteKArgs write_args(const RrlWriteRider *wr) {
    const int wtiles = (wr->n + 1023) / 1024;
    return WriteKArgs{wr->rng_state, wr->r, wr->centers, wr->accept, wr->lines, wr->filled, wr->n, wr->rounds, wtiles, wr->rounds};
}

// o.plan: rrl_plan; tb: the backward that rides in the launch (o.plan.bwd_rides), else NULL
static int loss_reduce_impl(const RrlCall &o, float *loss, const TailBwd *tb) {
    const int B = o.B, nblk = (o.L + 1023) / 1024;
    if (B == 0) return 0;
    if (o.plan.reduce == RRL_RED_TAIL) {
        const TailArgs t = tail_args(o, loss, tb);
        if (tb && o.plan.write_rides) {  // the next epoch's sampler write pass rides along (tail_write_kernel; rrl_demo_epoch)
            const WriteKArgs wk = write_args(o.write_rider);
            const dim3 g((unsigned)(wk.gx * wk.gy + nblk * B * TAIL_SUBS));
            const size_t lds = sizeof(int32_t) * (size_t)wk.rounds * wk.gx;
            if (t.grad_tri1) hipLaunchKernelGGL(tail_write_kernel<true>, g, dim3(TAIL_LANES), lds, o.s, t, wk);
            else hipLaunchKernelGGL(tail_write_kernel<false>, g, dim3(TAIL_LANES), lds, o.s, t, wk);
            o.write_rider->done = 1;
        } else {
            const dim3 g((unsigned)nblk, (unsigned)B, TAIL_SUBS);
#define RRL_TAIL(S_, R_) hipLaunchKernelGGL((loss_tail_kernel<S_, R_>), g, dim3(TAIL_LANES), 0, o.s, t)
            if (t.grad_tri1) { if (o.plan.tail_rpl2) RRL_TAIL(true, 2); else RRL_TAIL(true, TAIL_RPL); }
            else { if (o.plan.tail_rpl2) RRL_TAIL(false, 2); else RRL_TAIL(false, TAIL_RPL); }
#undef RRL_TAIL
        }
        RRL_LAUNCH_CHECK();
        return 0;
    }
    if (o.plan.reduce == RRL_RED_XCHG) {
        hipLaunchKernelGGL(loss_reduce_tiled_kernel, dim3((unsigned)nblk, (unsigned)B), dim3(256), 0, o.s, tiled_args(o, loss));
        RRL_LAUNCH_CHECK();
        return 0;
    }
    // (RRL_RED_TILE here: the reduce stage of a one-tile call issued stage by stage)
    hipLaunchKernelGGL(loss_reduce_kernel, dim3((unsigned)(o.pool ? 1 : B)), dim3(1024), sizeof(int) * (size_t)(nblk + 1), o.s,
                       reduce_args(o, loss));
    RRL_LAUNCH_CHECK();
    return 0;
}

extern "C" int rrl_loss_reduce_ex(void *ws, size_t ws_bytes, float *loss, int B, int N, int M, int L,
                                  int s_m, int s_n, int e_m, int e_n, int pool, const rrl_opts *opts, void *stream) {
    RrlCall o = rrl_begin_call(opts, B, N, M, L, ws, ws_bytes, stream);
    o.set(s_m, s_n, e_m, e_n, pool);
    if (const int rc = rrl_check_call(o, loss != nullptr, RRL_WANT_STAGE)) return rc;
    return loss_reduce_impl(o, loss, nullptr);
}
extern "C" int rrl_loss_reduce(void *ws, size_t ws_bytes, float *loss, int B, int N, int M, int L,
                               int s_m, int s_n, int e_m, int e_n, int pool, void *stream) {
    return rrl_loss_reduce_ex(ws, ws_bytes, loss, B, N, M, L, s_m, s_n, e_m, e_n, pool, nullptr, stream);
}

// K3 + K4 over CALLER-SUPPLIED rows (the merge step of the line-sharded single-sample mode, rrl_hip/dist.py): every rank
// ran the scan and the per-line stage on ITS share of one sample's lines; the selected lines' canonical D tiles and
// (k | j << 4) bytes of all ranks, gathered into one dense list, are reduced here by the single-workgroup kernel exactly
// as if one per-line stage had produced them (full tiles of 1024 rows: blkcnt is filled by a tiny launch).  The median
// is over the same multiset and the bucket sums are order-independent fixed point, so loss, median, bucket counts and
// sums are bit-identical to the unsharded evaluation.
__global__ void rows_blkcnt_kernel(int32_t *__restrict__ blkcnt, int nblk, int nrows) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < nblk) blkcnt[t] = min(1024, nrows - 1024 * t);
}

extern "C" int rrl_loss_reduce_rows(const float *rows16, const uint8_t *kj, int nrows, int32_t *blkcnt_scratch, float *loss,
                                    float *med, int32_t *bcnt, int64_t *bsum, int32_t *info, const int32_t *status,
                                    int s_m, int s_n, int e_m, int e_n, void *stream) {
    if (!rows16 || !kj || !blkcnt_scratch || !loss || !med || !bcnt || !bsum || !info || !status || nrows < 0) return RRL_E_ARG;
    if (s_m < 1 || s_n < 1 || e_m > RRL_MAX_HITS + 1 || e_n > RRL_MAX_HITS + 1) return RRL_E_RANGE;
    const int nblk = nrows > 0 ? (nrows + 1023) / 1024 : 1;
    hipLaunchKernelGGL(rows_blkcnt_kernel, dim3((unsigned)((nblk + 255) / 256)), dim3(256), 0, (hipStream_t)stream, blkcnt_scratch,
                       nblk, nrows);
    ReduceArgs r;
    r.kjc = kj; r.dc = rows16; r.blkcnt = blkcnt_scratch;
    r.med_out = med; r.bcnt_out = bcnt; r.bsum_out = bsum; r.info = info; r.loss = loss; r.status = status;
    r.B = 1; r.nblk = nblk; r.s_m = s_m; r.s_n = s_n; r.e_m = e_m; r.e_n = e_n; r.pool = 0;
    hipLaunchKernelGGL(loss_reduce_kernel, dim3(1), dim3(1024), sizeof(int) * (size_t)(nblk + 1), (hipStream_t)stream, r);
    RRL_LAUNCH_CHECK();
    return 0;
}


static ScatArgs scat_args(const RrlCall &o, const float *grad_loss, float *g1, float *g2) {
    ScatArgs a;
    a.lidc = (uint32_t *)o.at<RRL_WS_LIDC>(); a.blkcnt = o.at<RRL_WS_BLKCNT>();
    a.hs1 = o.at<RRL_WS_HS1>(); a.hs2 = o.at<RRL_WS_HS2>(); a.bcnt = o.at<RRL_WS_BCNT>(); a.info = o.at<RRL_WS_INFO>();
    a.w1 = o.at<RRL_WS_W1>(); a.w2 = o.at<RRL_WS_W2>(); a.D = o.at<RRL_WS_D>(); a.med = o.at<RRL_WS_MED>();
    a.grad_loss = grad_loss;
    a.Q1 = (const float4 *)o.at<RRL_WS_Q1>(); a.Q2 = (const float4 *)o.at<RRL_WS_Q2>();
    a.g1 = g1; a.g2 = g2; a.N = o.N; a.M = o.M; a.L = o.L;
    a.fx = nullptr; a.fxbits = 0; a.fxB = 0;
    return a;
}

static int scat_fx_bits_host(int L) {
    int lg = 1;
    while ((1 << lg) < L && lg < 30) ++lg;
    return 62 - lg;
}

// deterministic: include/rrl.h rrl_set_deterministic -- the scatter accumulates in the workspace's fixed-point field (which this
// call clears and therefore WRITES: the one entry that touches the workspace of a finished forward) and one more launch
// converts; grad_tri1 / grad_tri2 are overwritten, not accumulated.
static int loss_backward_impl(const RrlCall &o, const float *grad_loss, float *grad_tri1, float *grad_tri2, bool zero1,
                              bool deterministic) {
    const int B = o.B, N = o.N, M = o.M, L = o.L;
    int rc;
    if (zero1 && (rc = rrl_fill(grad_tri1, 0u, sizeof(float) * 9 * (size_t)B * N, o.s))) return rc;
    if (grad_tri2 && (rc = rrl_fill(grad_tri2, 0u, sizeof(float) * 9 * (size_t)B * M, o.s))) return rc;
    if (B == 0 || L == 0) return 0;
    ScatArgs sa = scat_args(o, grad_loss, grad_tri1, grad_tri2);
    if (deterministic && (N + M) > 0) {
        sa.fx = (unsigned long long *)o.at<RRL_WS_GFIX>();
        sa.fxbits = scat_fx_bits_host(L);
        sa.fxB = B;
        if ((rc = rrl_fill(sa.fx, 0u, 8 * (size_t)B * (N + M) * 9 + 8 * (size_t)B, o.s))) return rc;
    }
    hipLaunchKernelGGL(loss_bwd_kernel, dim3((unsigned)((L + 1023) / 1024), (unsigned)B, BWDS_SUBS), dim3(256), 0, o.s, sa, B, o.pool,
                       B % 8 == 0 && xcd_align_on() ? 1 : 0);
    RRL_LAUNCH_CHECK();
    if (sa.fx) {
        const int nmax = grad_tri2 && M > N ? M : N;
        hipLaunchKernelGGL(scatter_fix_to_float_kernel, dim3((unsigned)(((size_t)nmax * 9 + 255) / 256), (unsigned)B, grad_tri2 ? 2u : 1u),
                           dim3(256), 0, o.s, sa, B, o.pool);
        RRL_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int rrl_loss_backward(const float *tri1, const float *tri2, const void *ws,
                                 size_t ws_bytes, const float *grad_loss, float *grad_tri1,
                                 float *grad_tri2, int B, int N, int M, int L, int pool,
                                 void *stream) {
    RrlCall o = rrl_begin_call(nullptr, B, N, M, L, const_cast<void *>(ws), ws_bytes, stream);
    o.pool = pool;
    if (const int rc = rrl_check_call(o, tri1 && tri2 && grad_loss && grad_tri1, RRL_WANT_NONE)) return rc;
    return loss_backward_impl(o, grad_loss, grad_tri1, grad_tri2, true, rrl_default_deterministic());
}

// ---------------------------------------------------------------------------------------
// fused forward
// ---------------------------------------------------------------------------------------
// the direct backward that rides in the single-tile kernel's launch (rrl_registration_step)
static SoloBwd solo_bwd_args(const RrlCall &o, float *loss, const TailBwd *tb) {
    SoloBwd sb;
    sb.kj = o.at<RRL_WS_KJ>(); sb.sel = o.at<RRL_WS_SEL>(); sb.nsel = o.at<RRL_WS_NSEL>();
    sb.hs1 = o.at<RRL_WS_HS1>(); sb.bcnt = o.at<RRL_WS_BCNT>(); sb.info = o.at<RRL_WS_INFO>();
    sb.w1 = o.at<RRL_WS_W1>(); sb.D = o.at<RRL_WS_D>(); sb.med = o.at<RRL_WS_MED>();
    sb.grad_loss = tb->grad_loss; sb.src = tb->src; sb.loss = loss;
    sb.Q1 = (const float4 *)o.at<RRL_WS_Q1>(); sb.Q2 = (const float4 *)o.at<RRL_WS_Q2>();
    sb.gR = tb->gR; sb.gt = tb->gt; sb.payload = tb->payload; sb.mctl = (uint32_t *)o.at<RRL_WS_MCTL>();
    sb.B = o.B; sb.N = o.N; sb.L = o.L; sb.transpose_r = tb->transpose_r; sb.Bt = o.problems;
    return sb;
}

// The forward of one checked and planned call (rrl_check_call; o.plan: rrl_plan).  o.tar_ws != NULL: a workspace of the same
// (B, N, M, L) that already went through a forward with the SAME tri2 and line (RPM / FMR evaluate several source poses
// against one target and one line set, rpm/Train_RPM.py:204-231): only the source cloud is prepared, sorted and scanned.
// o.xf != NULL: tri1 is the workspace field TRI1, filled from o.xf->src.  tb: the backward that rides in the reduce's launch
// (o.plan.bwd_rides).
static int loss_forward_impl(RrlCall &o, const float *tri1, const float *tri2, const float *line, float *loss,
                             const TailBwd *tb = nullptr) {
    const RrlPlan &p = o.plan;
    if (o.chain_left) *o.chain_left = p.leave_clean | (p.fused_build << 1);  // bit 0: leaves the workspace chain-clean; bit 1: THIS call's build is fused
    o.tri1_in = tri1;
    int rc;
    RrlRange step("rrl forward");
    if (!p.fused_build) {
        RrlRange r("K1' records + sort + tree");
        if ((rc = rrl_tri_prepare_clouds(o, tri1, tri2, line))) return rc;
    }
    {
        RrlRange r("K1 line<->triangle scan");
        if ((rc = rrl_line_tri_scan_clouds(o, line))) return rc;
    }
    if (p.reduce == RRL_RED_TILE) {  // one tile of lines per sample: K2 + K3 + K4 in one launch
        RrlRange r("K2 + K3 + K4 (single tile)");
        const PairArgs pa = pair_args(o, tri1, tri2, line, false);
        const ReduceArgs ra = reduce_args(o, loss);
        const dim3 grid((unsigned)o.B);
        if (tb && tb->grad_tri1) {  // ... and the scatter backward to points1.grad too (rrl_loss_step_ex)
            hipLaunchKernelGGL(pair_reduce_scatter_kernel, grid, dim3(1024), sizeof(int) * 2, o.s, pa, ra,
                               scat_args(o, tb->grad_loss, tb->grad_tri1, nullptr), tb->payload, (uint32_t *)o.at<RRL_WS_MCTL>());
        } else if (tb) {  // ... and the direct backward too (rrl_registration_step)
            hipLaunchKernelGGL(pair_reduce_bwd_kernel, grid, dim3(1024), sizeof(int) * 2, o.s, pa, ra, solo_bwd_args(o, loss, tb));
        } else {
            hipLaunchKernelGGL(pair_reduce_kernel, grid, dim3(1024), sizeof(int) * 2, o.s, pa, ra);
        }
        RRL_LAUNCH_CHECK();
        return 0;
    }
    {
        RrlRange r("K2 per-line distances");
        if ((rc = line_pair_dist_impl(o, tri1, tri2, line))) return rc;
    }
    RrlRange r("K3+K4 median + Welsch reduce");
    return loss_reduce_impl(o, loss, tb);
}

// rrl_loss_forward_ex on its record (rrl_loss_forward_info reads INFO through the same one)
static int loss_forward_call(RrlCall &o, const float *tri1, const float *tri2, const float *line, float *loss,
                             const void *target_ws) {
    if (const int rc = rrl_check_call(o, tri1 && tri2 && line && loss, RRL_WANT_FORWARD, target_ws)) return rc;
    return loss_forward_impl(o, tri1, tri2, line, loss);
}

extern "C" int rrl_loss_forward_ex(const float *tri1, const float *tri2, const float *line,
                                   void *ws, size_t ws_bytes, float *loss, int B, int N, int M,
                                   int L, int s_m, int s_n, int e_m, int e_n, int pool, int mode,
                                   int chunk, const void *target_ws, const rrl_opts *opts, void *stream) {
    RrlCall o = rrl_begin_call(opts, B, N, M, L, ws, ws_bytes, stream);
    o.set(s_m, s_n, e_m, e_n, pool, mode, chunk);
    return loss_forward_call(o, tri1, tri2, line, loss, target_ws);
}
extern "C" int rrl_loss_forward_cached(const float *tri1, const float *tri2, const float *line,
                                       void *ws, size_t ws_bytes, float *loss, int B, int N, int M,
                                       int L, int s_m, int s_n, int e_m, int e_n, int pool, int mode,
                                       int chunk, const void *target_ws, void *stream) {
    return rrl_loss_forward_ex(tri1, tri2, line, ws, ws_bytes, loss, B, N, M, L, s_m, s_n, e_m, e_n,
                               pool, mode, chunk, target_ws, nullptr, stream);
}

// The drop-in call (code/loss.py:170-232 as the reference's callers use it: one sample, a Python-level
// decision on the result) in ONE entry: the forward, then INFO[0 .. 4 G) (nbuckets, nselected, nvalues, NaN
// flag per group) copied to host_info, then a wait for the stream -- the only entry of the library that
// synchronises, because the reference's return value (a tensor, or None when no bucket is populated, or an
// exit on NaN) is a host-side decision by contract.  host_info: 4 G int32 in host memory (pinned memory makes
// the copy asynchronous up to the wait).
extern "C" int rrl_loss_forward_info(const float *tri1, const float *tri2, const float *line, void *ws,
                                     size_t ws_bytes, float *loss, int B, int N, int M, int L, int s_m,
                                     int s_n, int e_m, int e_n, int pool, int mode, int chunk,
                                     const void *target_ws, int32_t *host_info, void *stream) {
    if (!host_info) return RRL_E_ARG;
    RrlCall o = rrl_begin_call(nullptr, B, N, M, L, ws, ws_bytes, stream);
    o.set(s_m, s_n, e_m, e_n, pool, mode, chunk);
    if (const int rc = loss_forward_call(o, tri1, tri2, line, loss, target_ws)) return rc;
    const int G = pool ? 1 : B;
    if (G <= 0) return 0;
    hipError_t e = hipMemcpyAsync(host_info, o.at<RRL_WS_INFO>(), sizeof(int32_t) * 4 * (size_t)G, hipMemcpyDeviceToHost, o.s);
    if (e != hipSuccess) return (int)e;
    e = hipStreamSynchronize(o.s);
    return e == hipSuccess ? 0 : (int)e;
}

extern "C" int rrl_loss_forward(const float *tri1, const float *tri2, const float *line, void *ws,
                                size_t ws_bytes, float *loss, int B, int N, int M, int L, int s_m,
                                int s_n, int e_m, int e_n, int pool, int mode, int chunk,
                                void *stream) {
    return rrl_loss_forward_cached(tri1, tri2, line, ws, ws_bytes, loss, B, N, M, L, s_m, s_n, e_m,
                                   e_n, pool, mode, chunk, nullptr, stream);
}

// ---------------------------------------------------------------------------------------
// fused training op: rigid transform of the source + loss, and its backward to (dR, dt)
// ---------------------------------------------------------------------------------------
extern "C" int rrl_registration_forward_ex(const float *src, const float *R, const float *t,
                                           const float *tri2, const float *line, void *ws,
                                           size_t ws_bytes, float *loss, int B, int N, int M,
                                           int L, int transpose_r, int s_m, int s_n, int e_m,
                                           int e_n, int mode, int chunk, const void *target_ws,
                                           const rrl_opts *opts, void *stream) {
    RrlCall o = rrl_begin_call(opts, B, N, M, L, ws, ws_bytes, stream);
    o.set(s_m, s_n, e_m, e_n, 0, mode, chunk);
    // the transform runs inside the prepare step
    const RrlXform xf = {src, R, t, transpose_r, 1};  // 1: clear GACC for the backward's atomics
    if (const int rc = rrl_check_call(o, src && R && t && tri2 && line && loss, RRL_WANT_FORWARD, target_ws, &xf)) return rc;
    return rrl_registration_forward_call(o, tri2, line, loss);
}
int rrl_registration_forward_call(RrlCall &o, const float *tri2, const float *line, float *loss) {
    return loss_forward_impl(o, o.at<RRL_WS_TRI1>(), tri2, line, loss);
}
extern "C" int rrl_registration_forward_cached(const float *src, const float *R, const float *t,
                                               const float *tri2, const float *line, void *ws,
                                               size_t ws_bytes, float *loss, int B, int N, int M,
                                               int L, int transpose_r, int s_m, int s_n, int e_m,
                                               int e_n, int mode, int chunk, const void *target_ws,
                                               void *stream) {
    return rrl_registration_forward_ex(src, R, t, tri2, line, ws, ws_bytes, loss, B, N, M, L, transpose_r, s_m, s_n,
                                       e_m, e_n, mode, chunk, target_ws, nullptr, stream);
}

extern "C" int rrl_registration_forward(const float *src, const float *R, const float *t,
                                        const float *tri2, const float *line, void *ws,
                                        size_t ws_bytes, float *loss, int B, int N, int M, int L,
                                        int transpose_r, int s_m, int s_n, int e_m, int e_n, int mode,
                                        int chunk, void *stream) {
    return rrl_registration_forward_cached(src, R, t, tri2, line, ws, ws_bytes, loss, B, N, M, L,
                                           transpose_r, s_m, s_n, e_m, e_n, mode, chunk, nullptr,
                                           stream);
}

// The direct backward accumulates (gR, gt, payload) with atomics: clear them unless they are the workspace's GACC field,
// which the forward's first launch clears
static int clear_direct_grads(const RrlCall &o, float *gR, float *gt, float *payload) {
    const float *gacc = o.at<RRL_WS_GACC>();
    const size_t B = (size_t)o.B;
    if (gR == gacc && gt == gacc + 9 * B && (!payload || payload == gacc + 12 * B)) return 0;
    int rc = rrl_fill(gR, 0u, sizeof(float) * 9 * B, o.s);
    if (!rc) rc = rrl_fill(gt, 0u, sizeof(float) * 3 * B, o.s);
    if (!rc && payload) rc = rrl_fill(payload, 0u, sizeof(float) * 14, o.s);
    return rc;
}

// part: the deterministic variant's partial rows; gx: the backward's workgroups per sample
static BwdKArgs bwd_args(const RrlCall &o, const float *src, const float *loss, const float *grad_loss, float *gR, float *gt,
                         float *payload, int transpose_r, float *part, int gx) {
    return BwdKArgs{o.at<RRL_WS_KJ>(), o.at<RRL_WS_SEL>(), o.at<RRL_WS_NSEL>(), o.at<RRL_WS_HS1>(), o.at<RRL_WS_W1>(),
                    (const float4 *)o.at<RRL_WS_Q1>(), (const float4 *)o.at<RRL_WS_Q2>(), o.at<RRL_WS_D>(), o.at<RRL_WS_MED>(),
                    o.at<RRL_WS_BCNT>(), o.at<RRL_WS_INFO>(), grad_loss, src, gR, gt, payload, loss,
                    o.B, o.N, o.L, transpose_r, part, gx};
}

// The backward of a checked call (rrl_check_call), after its forward on this workspace
static int registration_backward_impl(const RrlCall &o, const float *src, const float *R, const float *loss,
                                      const float *grad_loss, float *grad_src, float *gR, float *gt, float *payload,
                                      int transpose_r) {
    const int B = o.B, N = o.N, M = o.M, L = o.L;
    float *g1 = o.at<RRL_WS_G1>();
    RrlRange step("K5 rrl backward");
    if (!grad_src && B > 0 && L > 0) {
        // only dL/dR, dL/dt (+ payload): ONE launch, straight from the selected lines
        const int nblk = o.deterministic ? 16 * ((L + 1023) / 1024) : (L + BWD_LINES - 1) / BWD_LINES;
        // partials in VALS (the reduce kernel's input tiles: dead after the forward; B * Lp * 16 floats
        // >= B * 16 ceil(L / 1024) * 12), fixed-order sums by a second launch: nothing to clear
        float *part = o.deterministic ? o.at<RRL_WS_VALS>() : nullptr;
        const BwdKArgs a = bwd_args(o, src, loss, grad_loss, gR, gt, payload, transpose_r, part, nblk);
        // the next epoch's sampler write pass rides along (bwd_write_kernel; rrl_demo_epoch)
        RrlWriteRider *wr = o.plan.write_rides ? o.write_rider : nullptr;
        const WriteKArgs wk = wr ? write_args(wr) : WriteKArgs{};
#define RRL_BWD(DET)                                                                                                            \
        if (wr) {                                                                                                               \
            hipLaunchKernelGGL(bwd_write_kernel<DET>, dim3((unsigned)(wk.gx * wk.gy + nblk * B)), dim3(256),                      \
                               sizeof(int32_t) * (size_t)wk.rounds * wk.gx, o.s, a, wk);                                         \
            wr->done = 1;                                                                                                       \
        } else                                                                                                                  \
            hipLaunchKernelGGL(loss_bwd_rt_kernel<DET>, dim3((unsigned)nblk, (unsigned)B), dim3(256), 0, o.s, a.kj, a.sel, a.nsel, \
                               a.hs1, a.w1, a.Q1, a.Q2, a.D, a.med, a.bcnt, a.info, a.grad_loss, a.src, a.gR, a.gt, a.payload,    \
                               a.loss, a.B, a.N, a.L, a.transpose_r, a.part, o.problems, B % 8 == 0 && xcd_align_on() ? 1 : 0)
        if (o.deterministic) {
            RRL_BWD(true);
            hipLaunchKernelGGL(loss_bwd_rt_finalize_kernel, dim3(1), dim3(256), 0, o.s, part, o.at<RRL_WS_INFO>(), loss,
                               gR, gt, payload, B, nblk);
            RRL_LAUNCH_CHECK();
            return 0;
        }
        if (int rc = clear_direct_grads(o, gR, gt, payload)) return rc;
        RRL_BWD(false);
#undef RRL_BWD
        RRL_LAUNCH_CHECK();
        return 0;
    }
    // dL/dsrc wanted too: scatter of the line gradients into G1 (cleared first; in deterministic mode through the fixed-point
    // accumulators, like rrl_loss_backward: the rigid backward behind it sums in a fixed order either way) ...
    if (rrl_fused_backward(B, N, M)) {  // ... then rigid backward + payload (reg_bwd_kernel)
        if (int rc = loss_backward_impl(o, grad_loss, g1, nullptr, true, o.deterministic != 0)) return rc;
        return rrl_launch_reg_bwd(o, src, R, grad_src, gR, gt, payload, loss, transpose_r);
    }
    int rc = loss_backward_impl(o, grad_loss, g1, nullptr, true, o.deterministic != 0);
    if (rc) return rc;
    rc = rrl_rigid_apply_bwd(src, R, g1, grad_src, gR, gt, o.at<RRL_WS_RPART>(), B, 3 * N, transpose_r, 0, o.s);
    if (rc) return rc;
    if (payload) rc = rrl_shard_payload(loss, o.ws, o.ws_bytes, gR, gt, payload, B, N, M, L, o.s);
    return rc;
}

// Forward + direct backward of the fused training op in ONE call (dL/dloss is an input, so nothing has to come back
// to the host in between): when the tail kernel serves the shape, the backward rides in its launch (5 launches per
// step instead of 6, and the reduce's and the backward's chains of dependent loads overlap); otherwise exactly
// rrl_registration_forward_cached followed by rrl_registration_backward.  gR, gt (and payload) should be the
// workspace's GACC field, which the forward's first launch clears; other buffers are cleared here first.
extern "C" int rrl_registration_step_ex(const float *src, const float *R, const float *t, const float *tri2,
                                        const float *line, void *ws, size_t ws_bytes, float *loss,
                                        const float *grad_loss, float *gR, float *gt, float *payload, int B, int N,
                                        int M, int L, int transpose_r, int s_m, int s_n, int e_m, int e_n, int mode,
                                        int chunk, const void *target_ws, const rrl_opts *opts, void *stream) {
    RrlCall o = rrl_begin_call(opts, B, N, M, L, ws, ws_bytes, stream);
    o.set(s_m, s_n, e_m, e_n, 0, mode, chunk);
    const RrlXform xf = {src, R, t, transpose_r, 1};
    const bool pointers = src && R && t && tri2 && line && loss && grad_loss && gR && gt;
    if (const int rc = rrl_check_call(o, pointers, RRL_WANT_DIRECT, target_ws, &xf)) return rc;
    return rrl_registration_step_call(o, xf, tri2, line, loss, grad_loss, gR, gt, payload);
}
int rrl_registration_step_call(RrlCall &o, const RrlXform &xf, const float *tri2, const float *line, float *loss,
                               const float *grad_loss, float *gR, float *gt, float *payload) {
    int rc;
    const bool ride = o.plan.bwd_rides;
    if (ride && (rc = clear_direct_grads(o, gR, gt, payload))) return rc;
    const TailBwd tb = {grad_loss, xf.src, gR, gt, payload, xf.transpose_r, nullptr};
    rc = loss_forward_impl(o, o.at<RRL_WS_TRI1>(), tri2, line, loss, ride ? &tb : nullptr);
    if (rc || ride) return rc;
    return registration_backward_impl(o, xf.src, xf.R, loss, grad_loss, nullptr, gR, gt, payload, xf.transpose_r);
}
extern "C" int rrl_registration_step(const float *src, const float *R, const float *t, const float *tri2,
                                     const float *line, void *ws, size_t ws_bytes, float *loss,
                                     const float *grad_loss, float *gR, float *gt, float *payload, int B, int N,
                                     int M, int L, int transpose_r, int s_m, int s_n, int e_m, int e_n, int mode,
                                     int chunk, const void *target_ws, void *stream) {
    return rrl_registration_step_ex(src, R, t, tri2, line, ws, ws_bytes, loss, grad_loss, gR, gt, payload, B, N, M, L,
                                    transpose_r, s_m, s_n, e_m, e_n, mode, chunk, target_ws, nullptr, stream);
}

// SURVEY 8(d)'s own definition -- T-apply + S + P + median + Welsch reduce + backward to points1.grad -- in ONE call
// (include/rrl.h rrl_loss_step_ex): the forward of rrl_loss_forward_ex / rrl_registration_forward_ex with the scatter
// backward of rrl_loss_backward riding in the reduce's launch where the tail kernel serves the shape (the records launch
// clears grad_tri1 with the per-call state: 4 launches with prepared orders); elsewhere, and when grad_tri2 is wanted,
// forward + loss_bwd_kernel.  Bit-identical loss; gradients to the rounding of the float atomics.
extern "C" int rrl_loss_step_ex(const float *tri1, const float *R, const float *t, const float *tri2, const float *line,
                                void *ws, size_t ws_bytes, float *loss, const float *grad_loss, float *grad_tri1,
                                float *grad_tri2, int B, int N, int M, int L, int transpose_r, int s_m, int s_n, int e_m,
                                int e_n, int mode, int chunk, const void *target_ws, const rrl_opts *opts, void *stream) {
    RrlCall o = rrl_begin_call(opts, B, N, M, L, ws, ws_bytes, stream);
    o.set(s_m, s_n, e_m, e_n, 0, mode, chunk);
    RrlXform xf = {tri1, R, t, transpose_r, 0};
    const bool pointers = tri1 && tri2 && line && loss && grad_loss && grad_tri1 && (R == nullptr) == (t == nullptr);
    int rc = rrl_check_call(o, pointers, grad_tri2 ? RRL_WANT_SCATTER2 : RRL_WANT_SCATTER, target_ws, R ? &xf : nullptr);
    if (rc) return rc;
    o.clear_ptr = grad_tri1;
    o.clear_bytes = sizeof(float) * 9 * (size_t)B * N;
    // the shard payload of the step (rrl_opts.payload): in the workspace's GACC field the records launch clears it with the
    // rest of the accumulator (the fused op's convention); any other buffer is cleared here first
    float *payload = o.payload;
    const bool pay_in_ws = payload && R && payload == o.at<RRL_WS_GACC>() + 12 * (size_t)B;
    xf.zero_g1 = pay_in_ws ? 1 : 0;
    if (payload && !pay_in_ws && (rc = rrl_fill(payload, 0u, sizeof(float) * 14, o.s))) return rc;
    const float *p1 = R ? o.at<RRL_WS_TRI1>() : tri1;  // points1: the moved source, or the caller's triangles as given
    const TailBwd tb = {grad_loss, nullptr, nullptr, nullptr, payload, 0, grad_tri1};
    rc = loss_forward_impl(o, p1, tri2, line, loss, o.plan.bwd_rides ? &tb : nullptr);
    if (rc || o.plan.bwd_rides) return rc;
    // (grad_tri1 was cleared by the build step's first launch -- or by its fill on the unsorted path; an empty batch /
    //  cloud launches nothing: clear here)
    if (B == 0 || (N == 0 && M == 0)) return rrl_fill(grad_tri1, 0u, o.clear_bytes, o.s);
    rc = loss_backward_impl(o, grad_loss, grad_tri1, grad_tri2, false, o.deterministic != 0);
    if (rc || !payload || L <= 0 || o.plan.payload_in_reduce) return rc;
    return rrl_shard_payload(loss, ws, ws_bytes, nullptr, nullptr, payload, B, N, M, L, stream);
}

extern "C" int rrl_registration_backward_ex(const float *src, const float *R, const float *tri2,
                                            void *ws, size_t ws_bytes, const float *loss,
                                            const float *grad_loss, float *grad_src, float *gR, float *gt,
                                            float *payload, int B, int N, int M, int L, int transpose_r,
                                            const rrl_opts *opts, void *stream) {
    RrlCall o = rrl_begin_call(opts, B, N, M, L, ws, ws_bytes, stream);
    bool ok = src && R && tri2 && grad_loss && gR && gt && (loss || !payload);
    if (o.problems > 0 && o.problems < B && grad_src) ok = false;  // multi-pose: the direct backward only (dL/dsrc would sum over the poses)
    // a ragged batch (the counts of the forward, again): the sorted layout's fused tail, which skips the absent source rows
    if (o.ragged() && (o.problems > 0 || !rrl_sorted_layout(N, M))) ok = false;
    if (const int rc = rrl_check_call(o, ok, RRL_WANT_NONE)) return rc;
    return registration_backward_impl(o, src, R, loss, grad_loss, grad_src, gR, gt, payload, transpose_r);
}
extern "C" int rrl_registration_backward(const float *src, const float *R, const float *tri2,
                                         void *ws, size_t ws_bytes, const float *loss,
                                         const float *grad_loss, float *grad_src, float *gR, float *gt,
                                         float *payload, int B, int N, int M, int L, int transpose_r,
                                         void *stream) {
    return rrl_registration_backward_ex(src, R, tri2, ws, ws_bytes, loss, grad_loss, grad_src, gR, gt, payload, B, N, M, L,
                                        transpose_r, nullptr, stream);
}
