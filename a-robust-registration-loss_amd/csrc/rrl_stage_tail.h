// rrl_stage_tail.h -- K3 + K4 (+ K5) in the tail kernel: loss_tail_kernel / tail_write_kernel, and the single-tile pair_reduce_kernel
// This header DEFINES kernels: it is included by rrl_sparse.hip only (one translation unit holds every stage behind the scan).
#pragma once
#include "rrl_ws.h"            // TAIL_MAX_TILES, TAIL_LANES (beside RrlPlan); the control-word map of include/rrl.h
#include "rrl_arith.h"         // FIX_SHIFT
#include "rrl_stage_args.h"
#include "rrl_stamps.h"
#include "rrl_sampler.h"       // the sampler's write pass as a device function: tail_write_kernel carries it
#include "rrl_stage_pair.h"    // pair_body, lds_barrier, wave_scatter_rows, xcd_sample_of
#include "rrl_stage_reduce.h"  // reduce_body, bucket_final, wave_select20, ld_agent / st_agent, tail_payload
// ---------------------------------------------------------------------------------------
// K3 + K4 (+ K5') "tail" kernel (round 3): the tiled reduce WITHOUT the exchange, and optionally the direct
// backward of the fused training op in the same launch.
// loss_reduce_tiled_kernel lets the workgroups of a sample exchange the median bin's values (cursor atomic,
// write-through stores, arrival counter, poll, read-back: four to five dependent cross-workgroup round trips).
// Here every live workgroup reads ALL compact D tiles of its sample itself -- they sit in the L2 (57 KB per
// sample at C2, 168 KB at the demo's shape) -- filters the bin's values into its own LDS and selects the median
// alone: the same bits in every workgroup, nobody waits for anybody.  What remains shared is order-independent:
// the fixed-point bucket sums (MSUM) and ONE arrival counter whose last arriver turns them into the loss.
// Geometry: a workgroup = 512 lanes = up to TAIL_LINES (64) selected lines of one 1024-line tile (16 workgroups
// per tile in the grid; those beyond the tile's count return at once, like loss_bwd_rt_kernel's): the per-line
// arithmetic is exp-heavy (~1200 instructions per lane), and more lines per compute unit would queue on its SIMDs
// (1024-lane workgroups with a whole tile each: 5.6 us in this phase instead of ~2).  Lanes 256 .. 511 only help
// to stream and to pick the bin.
// do_bwd: the gradient of the workgroup's lines to (dL/dR, dL/dt) needs the median, the bucket counts (known
// since the per-line stage: MCTL) and dL/dloss (an input) -- not the loss -- so it runs in the same workgroup:
// its chain of dependent loads (compact slot -> line -> Q1 / Q2 / hit / weights -> source triangle) is requested
// at the START of the kernel and is in flight while the median is found (the LDS-only barriers below do not
// drain vector memory).  As separate launches the reduce and the backward cost 11.2 + 8.3 us at C2.
// payload[0 .. 1] (sum of the valid losses, their number) without a last-of-all hand-over: every sample's
// finaliser adds its loss to a 2^-40 fixed-point sum (returning atomic) and offers float(sum so far) to
// payload[0] by an unsigned atomicMax on the bit pattern -- the partial sums are monotone (losses >= 0), so the
// maximum is the complete sum, independent of the order; a NaN loss offers the (larger) NaN pattern.
// Same arithmetic and summation rules as reduce_body / loss_bwd_rt_kernel: bit-identical median and loss;
// (dR, dt) up to the order of the float atomics, as before; payload[0] may differ from the two-call path's
// double-precision sum in its last bit.
// ---------------------------------------------------------------------------------------
// (TAIL_MAX_TILES = 32 line tiles per sample, TAIL_LANES = 512: rrl_ws.h, the plan reads them)
#define TAIL_LINES 64  // selected lines per workgroup (four lanes each)
#ifndef TAIL_SUBS
#define TAIL_SUBS 4    // workgroups per tile (grid z): workgroup s takes the tile's chunks s, s + 4, ... of TAIL_LINES lines
#endif
#ifndef TAIL_RPL
#define TAIL_RPL 4     // 16-byte groups of D values per lane and streaming round
#endif

// (>= 4 wavefronts per SIMD = two 512-lane workgroups per CU: beyond 128 VGPRs a grid of more than 256 live workgroups -- B >= 16
//  at ten tiles -- would run in two generations: measured 17 -> 23.6 us at B = 16 when an edit pushed the kernel to 132)
//  SCATTER: the backward goes to points1.grad (rrl_loss_step) instead of (dR, dt) -- a template parameter, so that neither
//  instantiation carries the other's registers (source coordinates and 12 sums / the 9-float gradient row).
// RPL: 16-byte groups of D values per lane and streaming round -- 2 where 2 x (lanes per tile) groups cover a tile's list
// (<= 10 tiles per sample: ~100 groups, a tile of ~100 selected lines holds ~50), else TAIL_RPL; chosen by the host.
template <bool SCATTER, int RPL>
__device__ __forceinline__ void tail_body(const TailArgs &a, int tile_in, int b_in, int sub) {  // (tile, sample, sub): the workgroup's place
    __shared__ unsigned s_vals[MCAND_CAP];  // the bin's values (usual route) / histogram of the streaming passes
    __shared__ unsigned s_wtot[TAIL_LANES / 64];
    __shared__ unsigned s_pick[3];          // bin, rank inside it, its population
    __shared__ unsigned s_whist[128];
    __shared__ unsigned long long s_sum[32];
    __shared__ unsigned s_flag[2];          // [0] this workgroup arrived last, [1] non-finite Welsch term (bit 0 own, bit 1 anyone's)
    __shared__ unsigned s_med, s_ncand;
    __shared__ int s_cnt[16];
    __shared__ int s_pref[TAIL_MAX_TILES + 1];
    __shared__ int s_vpref[TAIL_MAX_TILES + 1];  // prefix of the tiles' value lists, in 16-byte groups
    __shared__ int s_misc[3];                    // live workgroups of the sample, its longest value list, its non-empty buckets
    __shared__ float s_red[4][12];
    __shared__ unsigned s_scat[4][64 * SCAT_STRIDE];  // wave_scatter_rows strips of the four wavefronts that hold lines
    constexpr int NW = TAIL_LANES / 64, BPL = 2048 / TAIL_LANES;  // wavefronts; histogram bins per lane
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // (sub is the SLOW grid index: the workgroups that certainly have lines are dispatched first)
    const int nblk = a.nblk;
    int tile = tile_in, b = b_in;
    if (a.xcd_align) xcd_sample_of(tile + nblk * b, nblk, tile, b);  // (uniform; every sub-grid of nblk x B workgroups is a multiple of 8)
    const size_t Lp = (size_t)nblk * 1024;
    uint32_t *ctl = a.mctl + (size_t)b * RRL_MCTL_WORDS;
    const float *__restrict__ dc = a.dc;
    const uint32_t *__restrict__ lidc = a.lidc;
    const size_t slot0 = (size_t)b * Lp + (size_t)tile * 1024;
    const bool do_bwd = a.do_bwd != 0;  // uniform
    constexpr bool scatter = SCATTER;  // gradient to the points (rrl_loss_step), not to (R, t)
    if (wave == 0) STAMPW(0);

    // ---- round 1: the sample's tile counts, histogram and bucket counts; the compact tile of "this lane's" line
    //      (lanes 0 .. 255, four per line: lane h of line r adds hit slot h's gradient, lane 0 the line's Welsch terms).
    //      Round 5: EVERYTHING of this round is requested before the tile's own count is looked at -- the count only decides
    //      whether the workgroup has lines at all and which of its line slots are real, never an address (a tile's compact
    //      slots exist whether or not they are filled): the early exit used to cost every live workgroup one dependent
    //      round trip (count -> the line's slot).  Vector loads return in order, so the wait for the count (requested
    //      first) does not wait for the rest.
    const int mycnt = a.blkcnt[(size_t)b * nblk + tile];
    const int bc = tid < nblk ? a.blkcnt[(size_t)b * nblk + tid] : 0;
    const int vraw = tid < nblk ? a.vlcnt[(size_t)b * nblk + tid] : 0;  // (-1: the per-line stage built no list -- a knob
    const int vc = vraw > 0 ? (vraw + 3) >> 2 : 0;                      // changed between the stages: flagged below)
    const int h = tid & 3;
    int r = sub * TAIL_LINES + (tid >> 2);  // compact rank within the tile of this lane's line (lanes < 256); first chunk
    unsigned kl_raw = 0u;
    float4 dr_raw = make_float4(INFINITY, INFINITY, INFINITY, INFINITY);
    if (tid < 4 * TAIL_LINES) {  // (r <= 255: inside the tile's 1024 slots; a slot beyond the count holds stale data: masked below)
        kl_raw = lidc[slot0 + r];
        dr_raw = ((const float4 *)(dc + (slot0 + r) * 16))[h];
    }
    unsigned hb[BPL];
    {
        const uint4 hq = ((const uint4 *)(a.mhist + (size_t)b * 2048))[tid];
        hb[0] = hq.x; hb[1] = hq.y; hb[2] = hq.z; hb[3] = hq.w;
        static_assert(BPL == 4, "one 16-byte load of the histogram per lane");
    }
    const unsigned bkt = tid < 16 ? ctl[RRL_MCTL_BUCKET0 + tid] : 0u;
    const float gl_in0 = do_bwd ? a.grad_loss[b] : 0.0f;
    // (the scan's NaN flag, for the info row: at the end it would be one more round trip of the last arriver; a chained
    //  step's fused launch keeps it per sample, next to the count of source workgroups that gave up waiting for their records)
    int st0;
    bool chain_tmo = false;
    if (a.chain_flags) {
        static_assert(RRL_CHAIN_WORDS == 4 && RRL_CHAIN_NAN == 1 && RRL_CHAIN_TIMEOUT == 3, "one 16-byte load: .y the NaN flag, .w the time-outs");
        const uint4 cw = *(const uint4 *)(a.chain + RRL_CHAIN_WORDS * (size_t)b);
        st0 = (int)cw.y;
        chain_tmo = cw.w != 0u;
    } else {
        st0 = a.status[0];
    }
    // ... and the sample's D values (the tiles' dense lists, VLIST), which the median's gather streams: lane (vt, vq) = (tile,
    // slot) reads the 16-byte groups vq + LPT u of tile vt -- an address that needs no count either (a list's 16384 slots
    // exist; a group beyond the list's length holds stale data and is masked by the count once it is here).  Round 5: the
    // gather used to map a dense group index through the prefix of the counts -- its loads could only leave after round 1
    // had come back and the bin was picked: one dependent round trip in front of the median (2.25 us of the kernel's 11.7 at
    // C2, in-kernel time stamps of tools/stamps_tail.py).
    const int LPT = TAIL_LANES / nblk;  // lanes per tile (uniform; nblk <= 32: >= 16)
    const int vt = tid / LPT, vq = tid - vt * LPT;
    const bool vlane = vt < nblk;
    const float4 *__restrict__ vbase = (const float4 *)(a.vlist + ((size_t)b * nblk + (vlane ? vt : 0)) * 16384);
    float4 vpre[RPL];
#pragma unroll
    for (int u = 0; u < RPL; ++u)
        vpre[u] = vlane ? vbase[vq + LPT * u] : make_float4(-1.0f, -1.0f, -1.0f, -1.0f);
    if (sub * TAIL_LINES >= mycnt && !(tile == 0 && sub == 0)) return;  // uniform: no line for this workgroup
    bool mine_on = tid < 4 * TAIL_LINES && r < mycnt;
    unsigned kl = mine_on ? kl_raw : 0u;
    float dr[4];  // row h of the line's canonical D tile (the four lanes of a line hold one row each)
    dr[0] = mine_on ? dr_raw.x : INFINITY; dr[1] = mine_on ? dr_raw.y : INFINITY;
    dr[2] = mine_on ? dr_raw.z : INFINITY; dr[3] = mine_on ? dr_raw.w : INFINITY;
    auto load_line = [&]() {  // (the later chunks of a crowded tile: their slots depend on the count)
        kl = 0u;
#pragma unroll
        for (int q = 0; q < 4; ++q) dr[q] = INFINITY;
        if (mine_on) {
            kl = lidc[slot0 + r];
            const float4 v = ((const float4 *)(dc + (slot0 + r) * 16))[h];
            dr[0] = v.x; dr[1] = v.y; dr[2] = v.z; dr[3] = v.w;
        }
    };
    const float gl_in = gl_in0;
    if (tid < 32) s_sum[tid] = 0ull;
    if (tid < 2) s_flag[tid] = 0u;
    if (tid == 0) s_ncand = 0u;
    if (tid < 16) s_cnt[tid] = (int)bkt;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    if (vraw < 0) atomicOr(&s_flag[1], 1u);  // (after the clearing above: same wavefront 0, LDS in order)
    if (wave == 0) {  // exclusive prefix of the tile counts (nblk <= 32) -- and what every wavefront needs of them, once
        const int incl = wave_incl_scan(bc), vincl = wave_incl_scan(vc);
        if (lane < nblk) { s_pref[lane + 1] = incl; s_vpref[lane + 1] = vincl; }
        if (lane == 0) { s_pref[0] = 0; s_vpref[0] = 0; }
        // workgroups of this sample that get past the test above (they all arrive at TICK2); the longest value list (16-byte
        // groups); the non-empty buckets of the range
        const int wl = min((bc + TAIL_LINES - 1) / TAIL_LINES, TAIL_SUBS);
        const int nl = wave_sum_i(lane < nblk ? (lane == 0 && wl == 0 ? 1 : wl) : 0);
        const int vm = (int)wave_max((float)vc);  // (vc <= 4096: exact in fp32)
        const int kk = lane / 4 + 1, jj = (lane & 3) + 1;
        const int cn = __popcll(__ballot(lane < 16 && bkt > 0u && kk >= a.s_m && kk < a.e_m && jj >= a.s_n && jj < a.e_n));
        if (lane == 0) { s_misc[0] = nl; s_misc[1] = vm; s_misc[2] = cn; }
    }
    int k, j;  // 0, 0 for a lane without a line

    // ---- the gradient chain of this lane's line, requested now: hit / Q1 / weights of hit slot h and the line's Q2
    //      points hang off the line index; the source triangle off the hit index (one round later, below) -- none of it
    //      depends on the median
    bool bwd_live;
    float4 q1;
    float qx[4], qy[4], qz[4], wq[3], xs[9];
    int fhit;
    auto request_line = [&]() {
        k = (int)((kl >> 24) & 15u); j = (int)(kl >> 28);
        bwd_live = do_bwd && mine_on && h < k;
        q1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        fhit = 0;
#pragma unroll
        for (int q = 0; q < 3; ++q) wq[q] = 0.0f;
#pragma unroll
        for (int o = 0; o < RRL_MAX_HITS; ++o) { qx[o] = qy[o] = qz[o] = 0.0f; }
        if (bwd_live) {
            const size_t gl = (size_t)b * a.L + (kl & 0xffffffu);
            fhit = a.hs1[gl * 4 + h];
            q1 = a.Q1[gl * 4 + h];
            const float *w = a.w1 + (gl * 4 + h) * 3;
#pragma unroll
            for (int q = 0; q < 3; ++q) wq[q] = w[q];
#pragma unroll
            for (int o = 0; o < RRL_MAX_HITS; ++o)
                if (o < j) { const float4 t = a.Q2[gl * 4 + o]; qx[o] = t.x; qy[o] = t.y; qz[o] = t.z; }
        }
    };
    auto request_source = [&]() {
#pragma unroll
        for (int q = 0; q < 9; ++q) xs[q] = 0.0f;
        if (bwd_live && !scatter) {  // (the scatter needs no source coordinates)
            const float *x = a.src + ((size_t)((a.Bt > 0 && b >= a.Bt) ? b % a.Bt : b) * a.N + fhit) * 9;
#pragma unroll
            for (int q = 0; q < 9; ++q) xs[q] = x[q];
        }
    };
    request_line();
    lds_barrier();  // s_pref, s_cnt
    if (wave == 0) STAMPW(8);
    const int myvc = vlane ? s_vpref[vt + 1] - s_vpref[vt] : 0;  // 16-byte groups of D values in this lane's tile's list
    const int nlive = s_misc[0], vmax = s_misc[1];  // (uniform)

    // ---- pick the bin of a rank among 2048 counts held BPL per lane: exclusive scan over the workgroup, the lane whose
    //      range holds the rank reports (bin, rank inside, population).  Returns the total.
    auto pick_bin = [&](unsigned rank_in, bool have_rank) -> unsigned {
        unsigned tsum = 0;
#pragma unroll
        for (int q = 0; q < BPL; ++q) tsum += hb[q];
        const unsigned incl = (unsigned)wave_incl_scan((int)tsum);
        if (have_rank) lds_barrier();  // s_wtot / s_pick free again (a later call; the first one finds them unused)
        if (lane == 63) s_wtot[wave] = incl;
        lds_barrier();
        unsigned base = 0, total = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const unsigned v = s_wtot[w];
            if (w < wave) base += v;
            total += v;
        }
        const unsigned rank = have_rank ? rank_in : (total ? (total - 1) / 2 : 0u);  // lower median: sorted[(n - 1) / 2]
        unsigned e = base + incl - tsum;
        if (rank >= e && rank < e + tsum) {  // exactly one lane (none when total == 0)
#pragma unroll
            for (int q = 0; q < BPL; ++q) {
                if (rank >= e && rank < e + hb[q]) { s_pick[0] = (unsigned)(BPL * tid + q); s_pick[1] = rank - e; s_pick[2] = hb[q]; }
                e += hb[q];
            }
        }
        lds_barrier();
        return total;
    };
    const unsigned n = pick_bin(0u, false);
    if (wave == 0) STAMPW(1);
    if (n == 0) {  // nothing selected in this sample: its only live workgroup is (tile 0, sub 0): loss 0, no bucket
        if (tid < 16) a.bcnt_out[b * 16 + tid] = 0;
        if (tid < 32) a.bsum_out[(size_t)b * 32 + tid] = 0;
        if (tid == 0) {
            a.med_out[b] = 0.0f;
            a.loss[b] = 0.0f;
            a.info[b * 4 + 0] = 0; a.info[b * 4 + 1] = 0; a.info[b * 4 + 2] = 0; a.info[b * 4 + 3] = st0;
            if (chain_tmo) a.loss[b] = __builtin_nanf("");
            if (a.chain) *(uint4 *)(a.chain + RRL_CHAIN_WORDS * (size_t)b) = make_uint4(0u, 0u, 0u, 0u);
        }
        return;
    }
    const unsigned bin = s_pick[0], r1 = s_pick[1], pop = s_pick[2];
    unsigned prefix = bin << 20;

    // ---- every D value of the sample from the tiles' dense lists (VLIST: only the valid entries, ~2 per line instead of the
    //      16 slots of a canonical tile; -1 pads), RPL 16-byte groups per lane and round, LPT RPL groups of every tile
    //      per round: fn(groups) for each round; the first round's groups are the ones requested in round 1 (pre = true: the
    //      first sweep) or loaded again (a later sweep of the crowded-bin route); after_issue() runs once, when the first
    //      round of loads is in flight
    auto stream_rows = [&](bool pre, auto &&after_issue, auto &&fn) {
        bool first = true;
        for (int g0 = 0; g0 < vmax; g0 += LPT * RPL) {  // uniform trip count
            float4 v[RPL];
#pragma unroll
            for (int u = 0; u < RPL; ++u) {
                const int g = g0 + vq + LPT * u;
                v[u] = make_float4(-1.0f, -1.0f, -1.0f, -1.0f);
                if (g < myvc) v[u] = pre && g0 == 0 ? vpre[u] : vbase[g];
            }
            if (first) { after_issue(); first = false; }
            fn(v);
        }
        if (first) after_issue();
    };
    auto each16 = [](const float4 *v, auto &&g) {
#pragma unroll
        for (int u = 0; u < RPL; ++u) {
            g(__float_as_uint(v[u].x)); g(__float_as_uint(v[u].y));
            g(__float_as_uint(v[u].z)); g(__float_as_uint(v[u].w));
        }
    };

    if (pop <= MCAND_CAP) {
        // the bin's values into this workgroup's own list: count, ONE cursor atomic per wavefront and round, plain stores
        stream_rows(true, [&]() { request_source(); }, [&](const float4 *v) {
            unsigned mine = 0;
            each16(v, [&](unsigned x) { mine += (x >> 20) == bin ? 1u : 0u; });
            const unsigned incl = (unsigned)wave_incl_scan((int)mine);
            unsigned wbase = 0;
            if (lane == 63 && incl) wbase = atomicAdd(&s_ncand, incl);
            wbase = (unsigned)__builtin_amdgcn_readlane((int)wbase, 63);
            unsigned at = wbase + incl - mine;
            each16(v, [&](unsigned x) {
                if ((x >> 20) == bin) { if (at < MCAND_CAP) s_vals[at] = x; ++at; }
            });
        });
        lds_barrier();
        if (wave == 0) STAMPW(9);
        if (tid < 64) {
            const unsigned m = wave_select20(s_vals, pop, prefix, r1, s_whist, tid);
            if (tid == 0) s_med = m;
        }
        if (wave == 0) STAMPW(10);
        lds_barrier();
        prefix = s_med;
    } else {
        // ---- crowded bin (near-identical D values): two more streaming passes (bits 19..9, 8..0), by every workgroup itself
        request_source();
        unsigned rk = r1;
        for (int pass = 1; pass <= 2; ++pass) {
            const int sh = pass == 1 ? 9 : 0, width = pass == 1 ? 11 : 9, hi = sh + width;
            const unsigned dmask = (1u << width) - 1u;
            lds_barrier();
#pragma unroll
            for (int q = 0; q < BPL; ++q) s_vals[tid + TAIL_LANES * q] = 0u;
            lds_barrier();
            const unsigned pre = prefix;
            stream_rows(false, [&]() {}, [&](const float4 *v) {
                each16(v, [&](unsigned x) {
                    if (((x ^ pre) >> hi) == 0u) atomicAdd(&s_vals[(x >> sh) & dmask], 1u);
                });
            });
            lds_barrier();
#pragma unroll
            for (int q = 0; q < BPL; ++q) hb[q] = s_vals[BPL * tid + q];
            pick_bin(rk, true);
            prefix |= s_pick[0] << sh;
            rk = s_pick[1];
        }
    }
    const float med = __uint_as_float(prefix);
    if (wave == 0) STAMPW(2);

    // ---- the workgroup's lines: Welsch terms into the fixed-point sums (lane 0 of a line; as reduce_core::accumulate) and
    //      hit slot h's gradient terms (as loss_bwd_rt_kernel)
    const int C = s_misc[2];
    // ---- the sample-wide part: this workgroup's fixed-point sums -> MSUM, one arrival ticket, and the LAST arriver of the
    //      sample turns the sums into the loss.  ONE wavefront runs it.  Round 5: when all of the workgroup's lines sit in its
    //      first chunk (<= 256 selected lines in the tile: always, at the shapes measured) the wavefront is the workgroup's
    //      LAST one -- it holds no lines, so its vector-memory queue is empty -- and it starts as soon as the Welsch sums are
    //      in LDS, while the wavefronts that hold lines go on with the gradient: the chain sums -> acknowledged -> ticket ->
    //      read-back (5.3 us of a 14.8 us launch at C2: the same kernel returning before it takes 9.5) no longer waits for the
    //      gradient's loads and the scatter's atomics in wavefront 0's queue.
    auto finish = [&]() {
    STAMPW(3);
    if (lane < 32) {
        const unsigned long long v = s_sum[lane];
        if (v) atomicAdd(&a.msum[(size_t)b * 32 + lane], v);
    }
    if (lane == 32 && s_flag[1]) atomicOr(&ctl[RRL_MCTL_BAD], 1u);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wavefront's sums have arrived before it takes its ticket
    STAMPW(4);
    unsigned last = 0;
    if (lane == 0)
        last = __hip_atomic_fetch_add(&ctl[RRL_MCTL_TICK2], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)(nlive - 1) ? 1u : 0u;
    STAMPW(5);
    if (!__builtin_amdgcn_readfirstlane((int)last)) return;

    // ---- the last workgroup of the sample: loss = ( sum_{non-empty (k,j), k-major} exp(-|k-j|/2) (mean_row + mean_col) ) / C
    unsigned long long tot = 0ull;
    unsigned anybad = 0u;
    if (lane < 32) {
        tot = __hip_atomic_load(&a.msum[(size_t)b * 32 + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        a.bsum_out[(size_t)b * 32 + lane] = (int64_t)tot;
        __hip_atomic_store(&a.msum[(size_t)b * 32 + lane], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // a second reduce on this state starts clean
    } else if (lane < 48) {
        a.bcnt_out[b * 16 + lane - 32] = s_cnt[lane - 32];
    } else if (lane == 48) {
        anybad = ld_agent(&ctl[RRL_MCTL_BAD]);
    }
    const bool bad = __builtin_amdgcn_readlane((int)anybad, 48) != 0;
    // lane 2 q + c holds sum c (row / column) of bucket q: one lane per bucket takes both (the double-precision means, as
    // reduce_body)
    const unsigned long long trow = __shfl(tot, (2 * lane) & 63), tcol = __shfl(tot, (2 * lane + 1) & 63);
    const BucketFinal f = bucket_final(trow, tcol, lane < 16 ? s_cnt[lane] : 0, lane, a.s_m, a.s_n, a.e_m, a.e_n);
    STAMPW(11);
    if (lane == 0) {
        const float accl = f.acc;
        const int Cn = f.C, nselected = f.nselected, nvalues = f.nvalues;
        const float lv = bad || chain_tmo ? __builtin_nanf("") : (Cn ? accl / (float)Cn : 0.0f);  // code/loss.py:230
        a.med_out[b] = med;
        a.loss[b] = lv;
        a.info[b * 4 + 0] = Cn;
        a.info[b * 4 + 1] = nselected;
        a.info[b * 4 + 2] = nvalues;
        a.info[b * 4 + 3] = st0;
        st_agent(&ctl[RRL_MCTL_TICK2], 0u); st_agent(&ctl[RRL_MCTL_BAD], 0u);
        if (a.chain) *(uint4 *)(a.chain + RRL_CHAIN_WORDS * (size_t)b) = make_uint4(0u, 0u, 0u, 0u);  // the next chained step finds them cleared
        if (do_bwd && a.payload && Cn > 0) tail_payload(a, lv);
    }
    STAMPW(6);
    };
    const bool single_chunk = mycnt <= TAIL_SUBS * TAIL_LINES;  // uniform
    float acc[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) acc[q] = 0.0f;
    for (int chunk = sub;; chunk += TAIL_SUBS) {  // (a second trip only when the tile has more than 256 selected lines)
    if (chunk != sub) {
        r = chunk * TAIL_LINES + (tid >> 2);
        mine_on = tid < 4 * TAIL_LINES && r < mycnt;
        load_line();
        request_line();
        request_source();
    }
    int arg_b_own = 0, arg_a[4] = {0, 0, 0, 0};
    float er[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // exp(-(D[h][b] / med) / 2): row h of the tile
    if (wave < 4) {  // uniform: the wavefronts that hold lines.  Every lane of them takes part (the four lanes of a line
        // exchange by quad DPP, which reads active lanes only): lanes without a line carry +inf tiles and k = j = 0.
        // The Welsch tile of a line is SHARED by its four lanes: lane h evaluates row h -- <= 4 exponentials and
        // divisions instead of the 16 + 8 every lane of loss_bwd_rt_kernel / reduce_core::accumulate spends -- and
        //   * the line's Welsch terms are those of the row / column minima of D (Welsch1 is evaluated by the same
        //     instructions on the same input: the entry that holds the minimum of D holds Welsch1(min D), bit for bit),
        //   * the gradient's exp(-(D/med)/2) is the very value 1 - Welsch1 was formed from.
        const int jmax = (int)wave_max((float)j);  // bounds the columns worth evaluating (uniform)
        float wr[4];
#pragma unroll
        for (int bb = 0; bb < RRL_MAX_HITS; ++bb) {
            const float d = dr[bb];
            wr[bb] = INFINITY;
            if (bb < jmax) {
                const float e = expf(-(d / med) / 2.0f);  // == welsch(): 1 - e
                er[bb] = e;
                if (d < INFINITY) wr[bb] = 1.0f - e;
            }
        }
        // row h: first-occurrence argmin of the Welsch values (the gradient's routing, welsch_block), and the Welsch value
        // of the row's smallest D (the line's row term)
        float bestw = wr[0];
#pragma unroll
        for (int bb = 1; bb < RRL_MAX_HITS; ++bb)
            if (wr[bb] < bestw) { bestw = wr[bb]; arg_b_own = bb; }
        const float dmin = fminf(fminf(dr[0], dr[1]), fminf(dr[2], dr[3]));
        const float rowterm = dr[0] == dmin ? wr[0] : (dr[1] == dmin ? wr[1] : (dr[2] == dmin ? wr[2] : wr[3]));
        // the whole Welsch tile and the whole D tile, from the other three lanes of the line
        float W[16], Dm[16];
#pragma unroll
        for (int bb = 0; bb < RRL_MAX_HITS; ++bb) {
            W[0 + bb] = quad_bcast<0>(wr[bb]); W[4 + bb] = quad_bcast<1>(wr[bb]);
            W[8 + bb] = quad_bcast<2>(wr[bb]); W[12 + bb] = quad_bcast<3>(wr[bb]);
            Dm[0 + bb] = quad_bcast<0>(dr[bb]); Dm[4 + bb] = quad_bcast<1>(dr[bb]);
            Dm[8 + bb] = quad_bcast<2>(dr[bb]); Dm[12 + bb] = quad_bcast<3>(dr[bb]);
        }
        float colterm[4];
#pragma unroll
        for (int bb = 0; bb < RRL_MAX_HITS; ++bb) {
            float best = W[bb];
            int m = 0;
#pragma unroll
            for (int aa = 1; aa < RRL_MAX_HITS; ++aa)
                if (W[aa * 4 + bb] < best) { best = W[aa * 4 + bb]; m = aa; }
            arg_a[bb] = m;
            const float cmin = fminf(fminf(Dm[bb], Dm[4 + bb]), fminf(Dm[8 + bb], Dm[12 + bb]));
            colterm[bb] = Dm[bb] == cmin ? W[bb] : (Dm[4 + bb] == cmin ? W[4 + bb] : (Dm[8 + bb] == cmin ? W[8 + bb] : W[12 + bb]));
        }
        const float rt0 = quad_bcast<0>(rowterm), rt1 = quad_bcast<1>(rowterm), rt2 = quad_bcast<2>(rowterm), rt3 = quad_bcast<3>(rowterm);
        if (mine_on && h == 0) {  // the line's Welsch terms, summed in reduce_core::accumulate's order
            float row = 0.0f, col = 0.0f;
            if (0 < k) row += rt0;
            if (1 < k) row += rt1;
            if (2 < k) row += rt2;
            if (3 < k) row += rt3;
#pragma unroll
            for (int q = 0; q < RRL_MAX_HITS; ++q)
                if (q < j) col += colterm[q];
            if (!(row <= 4.0f) || !(col <= 4.0f)) { atomicOr(&s_flag[1], 1u); row = col = 0.0f; }
            const int bi = (k - 1) * 4 + (j - 1);
            atomicAdd(&s_sum[bi * 2 + 0], (unsigned long long)((double)row * (double)(1ll << FIX_SHIFT) + 0.5));
            atomicAdd(&s_sum[bi * 2 + 1], (unsigned long long)((double)col * (double)(1ll << FIX_SHIFT) + 0.5));
        }
    }
    if (single_chunk) {  // (uniform) every wavefront's Welsch sums are in LDS: the finisher wavefront takes them from here
        lds_barrier();
        if (wave == NW - 1) finish();  // (then it falls through the rest like the other wavefronts without lines)
    }
    float sv[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};  // this lane's gradient row (scatter)
    bool sc_live = false;
    if (bwd_live && C > 0) {
        const int S = s_cnt[(k - 1) * 4 + (j - 1)];
        const float wkj = expf(-0.5f * (float)abs(k - j));
        const float scale = gl_in * wkj / (float)C;
        const float inv_row = 1.0f / ((float)S * (float)k), inv_col = 1.0f / ((float)S * (float)j);
        float gq[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int o = 0; o < RRL_MAX_HITS; ++o) {
            if (o >= j) continue;
            float sw = 0.0f;
            if (arg_b_own == o) sw += inv_row;
            if (arg_a[o] == h) sw += inv_col;
            if (sw == 0.0f) continue;
            const float gD = scale * sw * er[o] / (2.0f * med);  // er[o] = exp(-(D[h][o] / med) / 2)
            gq[0] += 2.0f * (q1.x - qx[o]) * gD;
            gq[1] += 2.0f * (q1.y - qy[o]) * gD;
            gq[2] += 2.0f * (q1.z - qz[o]) * gD;
        }
        if (scatter) {  // dL/dP1[f][kk] += w_kk / 3 * dL/dq1 (loss_bwd_kernel's expression; the records launch cleared the target)
#pragma unroll
            for (int kk = 0; kk < 3; ++kk) {
                const float wk = wq[kk] / 3.0f;
#pragma unroll
                for (int cc = 0; cc < 3; ++cc) sv[3 * kk + cc] = wk * gq[cc];
            }
            sc_live = true;
        } else {
#pragma unroll
        for (int kk = 0; kk < 3; ++kk) {
            const float wk = wq[kk] / 3.0f;  // q = mean_k(w_k P_k)
            float gv[3];
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) gv[cc] = wk * gq[cc];
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) {
                const float xc = xs[3 * kk + cc];
#pragma unroll
                for (int jj = 0; jj < 3; ++jj) acc[cc * 3 + jj] = fmaf(xc, gv[jj], acc[cc * 3 + jj]);
                acc[9 + cc] += gv[cc];
            }
        }
        }
    }
    if (scatter && wave < 4)  // (wave-uniform) the rows of this wavefront's lines, transposed through its LDS strip
        wave_scatter_rows(sc_live, sv, (unsigned)fhit, a.grad_tri1 + (size_t)b * a.N * 9, nullptr, s_scat[wave], lane);
    if ((chunk + TAIL_SUBS) * TAIL_LINES >= mycnt) break;  // uniform
    }
    if (do_bwd && !scatter && wave < 4) {  // (the lines sit in the first four wavefronts)
#pragma unroll
        for (int q = 0; q < 12; ++q) acc[q] = wave_sum(acc[q]);
        if (lane == 0)
#pragma unroll
            for (int q = 0; q < 12; ++q) s_red[wave][q] = acc[q];
    }
    __syncthreads();
#ifdef TAIL_EXP_NOFINAL  // timing experiment only (results invalid): what do the fixed-point sums -> ticket -> read-back cost?
    return;
#endif
    // ---- from here on wavefront 1 adds the workgroup's gradient sums and wavefront 0 does everything else by itself (its
    //      lanes see each other's LDS writes in program order: no workgroup barrier any more); the rest is done
    if (wave == 1 && do_bwd && !scatter && mycnt > 0 && lane < 12) {
        const int q = lane;
        const float v = (s_red[0][q] + s_red[1][q]) + (s_red[2][q] + s_red[3][q]);
        int o = q;  // m-index (i, j) -> memory order of R
        if (q < 9 && a.transpose_r) o = (q % 3) * 3 + q / 3;
        if (q < 9) atomicAdd(&a.gR[b * 9 + o], v); else atomicAdd(&a.gt[b * 3 + (q - 9)], v);
        if (a.payload) atomicAdd(&a.payload[2 + o], v);
    }
    if (wave == 0) STAMPW(7);
    if (wave != 0 || single_chunk) return;  // (single_chunk: the finisher wavefront took this part on long ago)
    finish();
}

template <bool SCATTER, int RPL>
__global__ __launch_bounds__(TAIL_LANES) __attribute__((amdgpu_waves_per_eu(4, 8))) void loss_tail_kernel(const TailArgs a) {
    tail_body<SCATTER, RPL>(a, (int)blockIdx.x, (int)blockIdx.y, (int)blockIdx.z);
}

// ... with the NEXT epoch's sampler write pass riding along (rrl_demo_epoch: RrlWriteRider; bwd_write_kernel does the same for
// the direct backward's own launch): the first gx * gy workgroups of a 1-D grid run one (tile of 1024 candidates, round) of the
// write pass each, the rest are the tail kernel's (tile fastest, sub slowest, as in its own grid).  The write pass touches the
// sampler's buffers and the line buffer only -- nothing the tail kernel reads.
template <bool SCATTER>
__global__ __launch_bounds__(TAIL_LANES) __attribute__((amdgpu_waves_per_eu(4, 8))) void tail_write_kernel(const TailArgs a,
                                                                                                          const WriteKArgs c) {
    extern __shared__ int s_tc_dyn[];  // the write pass's tile counts [rounds][tiles]
    const int nwrite = c.gx * c.gy, lin = (int)blockIdx.x;
    if (lin < nwrite) {  // uniform per workgroup
        sample_write_body<TAIL_LANES>(s_tc_dyn, nullptr, c.rng_state, c.r, c.centers, nullptr, nullptr, c.accept, c.lines, c.filled, 1,
                                      c.n, c.rounds, lin % c.gx, lin / c.gx, 0, c.gx, (unsigned)nwrite);
        return;
    }
    const int l2 = lin - nwrite, per = a.nblk * a.B;
    tail_body<SCATTER, TAIL_RPL>(a, l2 % a.nblk, (l2 / a.nblk) % a.B, l2 / per);
}

// K2 + K3 + K4 in ONE launch when a sample has a single tile of lines (L <= 1024) and the samples are not pooled:
// the workgroup that ran the per-line stage of sample b owns everything the reduce of sample b reads, so it
// simply carries on (a launch and the reduce's first load round less: small-L shapes such as C5 are nothing
// but launch latency).  Same bodies, same results.
__global__ __launch_bounds__(1024) void pair_reduce_kernel(const PairArgs pa, const ReduceArgs ra) {
    __shared__ __attribute__((aligned(16))) float s_dct[128 * 16];  // the first pass's compact D tiles and (k | j << 4) bytes:
    __shared__ uint8_t s_kjct[128];                                 // at <= 128 selected lines the reduce reads nothing back
    PairKeep kp;
    kp.kjc_lds = s_kjct; kp.dc_lds = s_dct;
    pair_body(pa, (int)blockIdx.x, 0, 1, &kp);
    const bool small = kp.total <= 128;  // (uniform)
    if (!small) __threadfence_block();   // this workgroup's KJC / VALS / BLKCNT stores are complete ...
    __syncthreads();                     // ... before any of its lanes reads them back (small: the LDS copies are)
    SoloReduce so;
    so.total = kp.total; so.kjc = small ? s_kjct : nullptr; so.dc = small ? s_dct : nullptr; so.fwave = 0;
    reduce_body(ra, (int)blockIdx.x, &so);
}

