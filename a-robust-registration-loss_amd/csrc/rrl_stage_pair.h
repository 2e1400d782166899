// rrl_stage_pair.h -- K2, the per-line stage: line_pair_dist_kernel (+ pair_count_kernel: the demo sampler's count pass riding along), the gradient scatter's LDS transpose
// This header DEFINES kernels: it is included by rrl_sparse.hip only (one translation unit holds every stage behind the scan).
#pragma once
#include "rrl_arith.h"  // hit_weights, inter_point, tri_coords (shared with the wide pipeline, rrl_wide.hip)
#include "rrl_stage_args.h"
#include "rrl_stamps.h"   // (ahead of the sampler, whose count pass stamps through STAMPC)
#include "rrl_sampler.h"  // the sampler's count pass as a device function: pair_count_kernel carries it

// LDS-only workgroup barrier: this wavefront's LDS traffic is complete, its vector-memory loads AND STORES stay in flight
// (__syncthreads() waits for both: a barrier behind a store costs the store's acknowledgement, ~0.5 us)
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

__device__ __forceinline__ void sort4(int *h, int n) {  // ascending, n <= 4
#pragma unroll
    for (int i = 1; i < RRL_MAX_HITS; ++i)
#pragma unroll
        for (int j = RRL_MAX_HITS - 1; j >= i; --j)
            if (j < n && h[j] < h[j - 1]) { int t = h[j]; h[j] = h[j - 1]; h[j - 1] = t; }
}

// Scatter of a wavefront's gradient rows (round 5).  Every LIVE lane owns nine products that go to nine CONSECUTIVE floats
// of its triangle's gradient row [9].  One lane per row meant nine instructions of 64 scattered 4-byte atomics -- 64 cache
// lines per instruction through the CU's address path: +4.5 us on the C2 tail kernel against the (dR, dt) variant, 53 us for
// loss_bwd_kernel at B = 64.  Here the rows meet in the wavefront's LDS strip, compacted by rank among the live lanes, and
// lane p of a round adds element (p % 9) of row (p / 9): one instruction covers seven whole rows (8 .. 14 cache lines),
// ceil(9 nlive / 64) instructions per wavefront instead of nine.  The products are computed by the owning lane exactly as
// before; only WHICH lane issues an atomic changes (float atomics: the sums agree to their rounding order, as before).
// rowkey = triangle index | (cloud 2 ? 1u << 31 : 0); g1b / g2b: the sample's gradient rows [n][9]; strip: 64 x 10 words.
#define SCAT_STRIDE 10
// fx1b / fx2b != NULL (deterministic mode, include/rrl.h rrl_set_deterministic): the element goes to the sample's 64-bit
// fixed-point accumulators instead -- llrint(value * inv_unit), inv_unit a power of two: integer atomics commute, so the sums
// do not depend on the order of arrival; a non-finite value raises *nonfinite (the conversion then writes NaN rows).
__device__ __forceinline__ void wave_scatter_rows(bool live, const float (&v)[9], unsigned rowkey, float *__restrict__ g1b,
                                                  float *__restrict__ g2b, unsigned *strip, int lane,
                                                  unsigned long long *fx1b = nullptr, unsigned long long *fx2b = nullptr,
                                                  double inv_unit = 0.0, int32_t *nonfinite = nullptr) {
    const unsigned long long mask = __ballot(live);
    const int nlive = __popcll(mask);
    if (nlive == 0) return;  // uniform
    if (live) {
        unsigned *row = strip + __popcll(mask & ((1ull << lane) - 1ull)) * SCAT_STRIDE;
        row[0] = rowkey;
#pragma unroll
        for (int q = 0; q < 9; ++q) row[1 + q] = __float_as_uint(v[q]);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // one wavefront: its LDS traffic is in order
    const int total = nlive * 9;
    for (int p = lane; p < total; p += 64) {
        const int rk = p / 9, e = p - rk * 9;
        const unsigned key = strip[rk * SCAT_STRIDE];
        const float val = __uint_as_float(strip[rk * SCAT_STRIDE + 1 + e]);
        if (fx1b) {  // uniform
            if (!(fabsf(val) < INFINITY)) { atomicOr(&nonfinite[key >> 31], 1); continue; }
            const long long q = __double2ll_rn((double)val * inv_unit);
            if (q) atomicAdd(((key >> 31) ? fx2b : fx1b) + (size_t)(key & 0x7fffffffu) * 9 + e, (unsigned long long)q);
            continue;
        }
        float *dst = ((key >> 31) ? g2b : g1b) + (size_t)(key & 0x7fffffffu) * 9 + e;
        atomicAdd(dst, val);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // the strip is free for the wavefront's next pass
}

// Phase 2 of line_pair_dist_kernel: EIGHT lanes per selected line, one per (cloud, hit slot) --
// a selected line has up to 4 + 4 hits and one lane doing them in turn was the kernel's long pole
// (8 us of 13).  Each lane gathers its triangle (three 16-byte loads of the prepared record, or
// the raw row with stride 9), recomputes the hit distances with the scan's arithmetic, the
// weights and the intersection point, and stores them; the eight lanes then exchange their
// points through LDS (same wavefront: no barrier) and each fills two entries of the k x j block
// of squared distances -- by line for the backward kernels and as the canonical 4 x 4 tile
// (+inf outside the block) at the line's compact slot for the reduce kernel.
// What a lane of the per-line stage knows about its (selected line, cloud, hit slot) after the FIRST pass (ranks 0 .. 127) --
// kept in registers for the single-tile kernels, whose backward then reads nothing of it back (pair_reduce_scatter_kernel).
struct PairKeep {
    int total;   // the tile's selected lines (uniform)
    int k, j;    // the line's hit counts (0, 0: this lane's rank holds no line)
    int f;       // this lane's triangle (hit slot a = lane & 3 of cloud (lane >> 2) & 1, ascending order), when a < count
    float w[3];  // its weights
    float4 q;    // its intersection point
    float4 *sq;  // LDS: the 8 intersection points of the line (cloud 1: 0..3, cloud 2: 4..7)
    // in: LDS the caller provides for the first pass's compact rows (what the reduce reads back: the (k | j << 4) byte and
    // the canonical 4 x 4 D tile of ranks 0 .. 127), or NULL
    uint8_t *kjc_lds;  // [128]
    float *dc_lds;     // [128][16]
};

__device__ __forceinline__ void pair_hit(const float *__restrict__ tri1, const float *__restrict__ tri2,
                                         const float *__restrict__ line, const int32_t *__restrict__ hit1,
                                         const int32_t *__restrict__ hit2, int32_t *__restrict__ hs1,
                                         int32_t *__restrict__ hs2, float *__restrict__ w1,
                                         float *__restrict__ w2, float4 *__restrict__ Q1,
                                         float4 *__restrict__ Q2, float *__restrict__ D,
                                         float *__restrict__ dc_slot, float4 *s_q /* LDS [8] of this line */,
                                         unsigned *s_mh /* LDS [2048] or NULL */,
                                         int b, int N, int M, size_t gl, int k, int j, int sub, int st1,
                                         int st2, float *t2 /* out: this lane's two tile entries (+inf: outside the block) */,
                                         int bi, size_t gli /* multi-pose: the instance's problem, its line's row there */,
                                         PairKeep *keep = nullptr) {
    const int cloud = sub >> 2, a = sub & 3;
    const int cnt = cloud ? j : k;
    float q[3] = {0.0f, 0.0f, 0.0f};
    if (a < cnt) {
        float ln[6];
        {
            const float2 *lp = (const float2 *)(line + gli * 6);  // 24-byte rows: 8-byte aligned
            const float2 a0 = lp[0], a1 = lp[1], a2 = lp[2];
            ln[0] = a0.x; ln[1] = a0.y; ln[2] = a1.x; ln[3] = a1.y; ln[4] = a2.x; ln[5] = a2.y;
        }
        int h[RRL_MAX_HITS];
        {
            const int4 r = cloud ? ((const int4 *)hit2)[gli] : ((const int4 *)hit1)[gl];  // (cloud 2 was scanned by its problem's first instance)
            const int rr[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
            for (int t = 0; t < RRL_MAX_HITS; ++t) h[t] = t < cnt ? rr[t] : 0x7fffffff;
        }
        sort4(h, cnt);  // ascending triangle index == nonzero() order (code/loss.py:125-131)
        const int f = a == 0 ? h[0] : (a == 1 ? h[1] : (a == 2 ? h[2] : h[3]));
        const float *tb = cloud ? tri2 + (size_t)bi * M * st2 : tri1 + (size_t)b * N * st1;
        float w[3], c[9];
        tri_coords(tb, cloud ? st2 : st1, f, c);
        hit_weights(c, ln, w);
        inter_point(c, w, q);
        (cloud ? hs2 : hs1)[gl * RRL_MAX_HITS + a] = f;
        (cloud ? Q2 : Q1)[gl * RRL_MAX_HITS + a] = make_float4(q[0], q[1], q[2], 0.0f);
        float *wd = (cloud ? w2 : w1) + (gl * RRL_MAX_HITS + a) * 3;
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) wd[cc] = w[cc];
        if (keep) {
            keep->f = f;
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) keep->w[cc] = w[cc];
            keep->q = make_float4(q[0], q[1], q[2], 0.0f);
        }
    }
    s_q[sub] = make_float4(q[0], q[1], q[2], 0.0f);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // the 8 lanes share a wavefront: LDS is in order
    // D[a][b] = sum_c (q1 - q2)^2, code/loss.py:38-52: entries 2 sub and 2 sub + 1 of the 4 x 4 tile
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int ee = 2 * sub + e, ra = ee >> 2, rb = ee & 3;
        t2[e] = INFINITY;
        if (ra < k && rb < j) {
            const float4 p1 = s_q[ra], p2 = s_q[4 + rb];
            float dx = p1.x - p2.x, dy = p1.y - p2.y, dz = p1.z - p2.z;
            float sq = dx * dx;
            sq = sq + dy * dy;
            sq = sq + dz * dz;
            D[gl * 16 + ra * j + rb] = sq;
            t2[e] = sq;
            // the median's first radix pass (bits 30..20 of the bit pattern; D >= 0), tallied where the value is born
            if (s_mh) atomicAdd(&s_mh[(__float_as_uint(sq) >> 20) & 2047u], 1u);
        }
    }
    ((float2 *)dc_slot)[sub] = make_float2(t2[0], t2[1]);
}

// XCD-aware placement of the per-sample stages (round 5).  Workgroups go to the 8 XCDs round-robin by linear id (observed;
// a matter of speed only), each XCD has its own L2, and everything a sample's per-line stage, reduce and backward read was
// written by workgroups of that sample: the culled scan runs the (cloud, sample) pair on the fast grid index, i.e. sample b
// (both clouds, when B % 8 == 0) on XCD b % 8.  With B % 8 == 0 the stages below decode their place in the grid so that
// sample b's workgroups run on XCD b % 8 too: (x, y) of a grid (gx fast, B samples) for linear id `lin`.
__device__ __forceinline__ void xcd_sample_of(int lin, int gx, int &x, int &b) {
    const int slot = lin >> 3;
    x = slot % gx;
    b = (lin & 7) + 8 * (slot / gx);
}
// (the host side's switch: rrl_ws.h xcd_align_on)

// One tile of 1024 lines of sample b by a 1024-lane workgroup.  Phase 1: every lane classifies its line
// and the selected ones (~9 %) are compacted through LDS, so that phase 2 -- the gather-heavy part -- runs
// on dense wavefronts, eight lanes per line; the compacted line ids also go to SEL[b] for the backward.
__device__ __forceinline__ void pair_body(const PairArgs &a, int b, int tile, int ntile, PairKeep *keep = nullptr) {
    __shared__ int s_list[1024];
    __shared__ int s_wave[16];
    __shared__ int s_total;
    __shared__ float4 s_q[128][8];  // intersection points of the lines of one pass
    __shared__ unsigned s_mh[2048];  // this tile's share of MHIST
    __shared__ unsigned s_bc[16];    // ... and of the bucket counts
    __shared__ unsigned s_nv;        // ... and the length of its value list
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int L = a.L;
    const int bi = (a.Bt > 0 && b >= a.Bt) ? b % a.Bt : b;  // the instance's problem (multi-pose)
    int base_reg = 0;
    if (wave == 0) STAMPP(0);
    const bool tally = a.mhist != nullptr;  // uniform
    if (tally) {  // (the barriers of phase 1 publish the clearing)
        s_mh[tid] = 0u;
        s_mh[tid + 1024] = 0u;
        if (tid < 16) s_bc[tid] = 0u;
        if (tid == 0) s_nv = 0u;
    }
    {
        const int l = tile * 1024 + tid;
        bool sel = false;
        unsigned kjb = 0;
        if (l < L) {
            const size_t gl = (size_t)b * L + l;
            const int k = a.count1[gl], j = a.count2[(size_t)bi * L + l];
            if (a.zc1) { a.zc1[gl] = 0; a.zc2[gl] = 0; }  // (chained steps; never multi-pose: bi == b)
            sel = k >= a.s_m && k < a.e_m && j >= a.s_n && j < a.e_n;
            kjb = sel ? (unsigned)(k | (j << 4)) : 0u;
            a.kj[gl] = (uint8_t)kjb;
        }
        const unsigned long long mask = __ballot(sel);
        if (lane == 0) s_wave[wave] = __popcll(mask);
        if (wave == 0) STAMPP(1);
        // (LDS-only barriers in this stage: what they publish is LDS -- the KJ store above, and later the stage's stores, are
        //  read by other launches, or by this workgroup behind a fence of its own in the single-tile kernels)
        lds_barrier();
        if (sel && tally) atomicAdd(&s_bc[((kjb & 15u) - 1u) * 4u + ((kjb >> 4) - 1u)], 1u);
        // every wavefront scans the 16 counts itself -- one LDS read, a DPP prefix -- for its own base and the total (round 5:
        // lane 0 of the workgroup used to walk them, one LDS round trip after the other, between two barriers)
        const int cw = lane < 16 ? s_wave[lane] : 0;
        const int iw = wave_incl_scan(cw);
        const int wbase = __builtin_amdgcn_readlane(iw - cw, wave), acc = __builtin_amdgcn_readlane(iw, 15);
        if (tid == 0) {
            s_total = acc;
            // the slot range in SEL[b] is only needed for the last store of the kernel: the
            // atomic's round trip overlaps the gathers below
            base_reg = acc ? atomicAdd(&a.nsel[b], acc) : 0;
        }
        // the line id (L < 2^24) and its (k, j) byte travel together: phase 2 needs no second look at the counts
        if (sel) s_list[wbase + __popcll(mask & ((1ull << lane) - 1ull))] = (int)((unsigned)l | (kjb << 24));
        lds_barrier();
    }
    // Compact copies for the reduce kernel live at slot = 1024 * tile + rank: no global
    // counter is needed to place them (BLKCNT[b][tile] tells the consumer how many each workgroup
    // wrote), so nothing here waits for an atomic.  SEL[b] (dense list of the selected line ids,
    // for the backward kernels) is written at the end by wavefront 0 alone: lane 0 holds the base
    // returned by the nsel atomic, whose round trip has long been hidden by the gathers.
    const size_t Lp = (size_t)ntile * 1024;
    const int total = s_total;
    STAMP(1);
    if (wave == 0) STAMPP(2);
    if (keep) {
        keep->total = total; keep->k = keep->j = 0; keep->f = 0; keep->sq = s_q[tid >> 3];
        keep->w[0] = keep->w[1] = keep->w[2] = 0.0f; keep->q = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    if (tid == 0) a.blkcnt[(size_t)b * ntile + tile] = total;
    float *vl = tally && a.vlist ? a.vlist + ((size_t)b * ntile + tile) * 16384 : nullptr;
    for (int r0 = 0; r0 < total; r0 += 128) {  // 128 selected lines per pass, 8 lanes each
        const int rank = r0 + (tid >> 3), sub = tid & 7;
        float t2[2] = {INFINITY, INFINITY};
        unsigned nvl = 0;  // this lane's entries inside the line's k x j block
        if (rank < total) {
            const unsigned e = (unsigned)s_list[rank];
            const int l = (int)(e & 0xffffffu), k = (int)((e >> 24) & 15u), j = (int)(e >> 28);
            const size_t gl = (size_t)b * L + l;
            const size_t slot = (size_t)b * Lp + (size_t)tile * 1024 + rank;
            if (sub == 0) {
                a.kjc[slot] = (uint8_t)(k | (j << 4));
                if (a.lidc) a.lidc[slot] = e;
            }
            pair_hit(a.tri1, a.tri2, a.line, a.hit1, a.hit2, a.hs1, a.hs2, a.w1, a.w2, a.Q1, a.Q2, a.D, a.dc + slot * 16,
                     s_q[tid >> 3], tally ? s_mh : nullptr, b, a.N, a.M, gl, k, j, sub, a.st1, a.st2, t2, bi, (size_t)bi * L + l,
                     r0 == 0 ? keep : nullptr);
            if (keep && r0 == 0) {
                keep->k = k; keep->j = j;
                if (keep->dc_lds) {
                    ((float2 *)(keep->dc_lds + rank * 16))[sub] = make_float2(t2[0], t2[1]);
                    if (sub == 0) keep->kjc_lds[rank] = (uint8_t)(k | (j << 4));
                }
            }
            nvl = (((2 * sub) >> 2) < k && ((2 * sub) & 3) < j ? 1u : 0u) | (((2 * sub + 1) >> 2) < k && ((2 * sub + 1) & 3) < j ? 2u : 0u);
        }
        if (vl) {  // (all lanes: uniform) the valid entries join the tile's dense value list: one LDS cursor atomic per wavefront
            const unsigned mine = (nvl & 1u) + (nvl >> 1);
            const unsigned incl = (unsigned)wave_incl_scan((int)mine);
            unsigned wbase = 0;
            if (lane == 63 && incl) wbase = atomicAdd(&s_nv, incl);
            wbase = (unsigned)__builtin_amdgcn_readlane((int)wbase, 63);
            unsigned at = wbase + incl - mine;
            if (nvl & 1u) vl[at++] = t2[0];
            if (nvl & 2u) vl[at] = t2[1];
        }
    }
    STAMP(2);
    if (wave == 0) STAMPP(3);
    if (tally) {  // flush the tile's tallies: <= one device atomic per populated bin and workgroup
        lds_barrier();
        uint32_t *mh = a.mhist + (size_t)b * 2048;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const unsigned v = s_mh[tid + 1024 * q];
            if (v) atomicAdd(&mh[tid + 1024 * q], v);
        }
        if (tid < 16 && s_bc[tid]) atomicAdd(&a.mctl[(size_t)b * RRL_MCTL_WORDS + RRL_MCTL_BUCKET0 + tid], s_bc[tid]);
        if (vl) {  // the list's length; padded with -1 (no D value is negative) to whole 16-byte groups
            const unsigned nv = s_nv;
            if (tid == 0) a.vlcnt[(size_t)b * ntile + tile] = (int)nv;
            if (tid < ((4u - (nv & 3u)) & 3u)) vl[nv + tid] = -1.0f;
        } else if (tid == 0 && a.vlcnt) {
            a.vlcnt[(size_t)b * ntile + tile] = -1;  // no list this time: a tail kernel run on this state reports it (NaN loss)
        }
    }
    if (wave == 0) STAMPP(4);
    if (wave == 0) {
        const int base = __builtin_amdgcn_readfirstlane(base_reg);
        for (int i = lane; i < total; i += 64) a.sel_out[(size_t)b * L + base + i] = s_list[i] & 0xffffff;
    }
    if (wave == 0) STAMPP(5);
}

__global__ __launch_bounds__(1024) void line_pair_dist_kernel(const PairArgs a) {
    int tile = blockIdx.x, b = blockIdx.y;
    if (a.xcd_align) xcd_sample_of(tile + (int)gridDim.x * b, (int)gridDim.x, tile, b);  // (uniform)
    pair_body(a, b, tile, (int)gridDim.x);
}

// tri1 / tri2: the triangles as the loss sees them -- the caller's rows, or TRI1 (the moved source of the fused op) --, raw
// 36-byte rows indexed by triangle.  (The prepared 48-byte records, PTRI, belong to the scans alone since round 4: the
// prepared build keeps them at their SORTED positions, and a target's records may live in another workspace.)
// The per-line stage AND the count pass of the next epoch's line sampler in ONE launch (round 4b; rrl_ws.h RrlCountRider,
// rrl_demo_epoch): both run 1024-lane workgroups, the count pass needs nothing the scan produced, and launches of one
// stream never overlap on this stack.  Workgroups [0, tiles x rounds) count (the long ones start first), the others run
// the per-line stage.  Same bodies, same results as the two launches.
__global__ __launch_bounds__(1024) void pair_count_kernel(const PairArgs a, const CountKArgs c, int pair_gx) {
    __shared__ SampleCountLds clds;
    const int ncount = c.gx * c.gy, lin = (int)blockIdx.x;
    if (lin < ncount) {  // uniform per workgroup
        sample_count_body(clds, nullptr, c.rng_state, c.r, c.centers, nullptr, c.aabb2, c.accept, 1, c.n, c.rounds, c.prefilter, 0,
                          lin % c.gx, lin / c.gx, 0, c.gx, c.rows, c.n_rows);
        return;
    }
    const int l2 = lin - ncount;
    pair_body(a, l2 / pair_gx, l2 % pair_gx, pair_gx);
}

