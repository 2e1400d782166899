// rrl_cull_scan.h -- the culled scan (cull_scan_kernel, cull_scan_chamfer_kernel, cull_scan_build_kernel) and its launch.
// Included ONCE by rrl_cull.hip.  The scan has two geometry variants (round 5), the trait structs Scan8 and Scan16 below;
// everything that depends on a variant's knobs takes the trait as its template parameter V:
//   Scan8   kSPW = 8,  the wavefront's lines in LDS             -- 47 KB of LDS, 3 workgroups per CU: the latency-bound grids
//   Scan16  kSPW = 16, the lines in registers (kRegLines)       -- 34 KB, 4 workgroups per CU: half as many workgroups with
//           twice the slice each -- one prologue per 16 supergroups instead of two, more wavefronts resident; pays as soon
//           as the grid is several generations deep (B = 64 at C2's shape: 152 -> 121 us; B = 8: 26.4 -> 28.2, so not there)
// rrl_launch_cull_scan (rrl_cull.hip) picks the variant per call from the grid size.  Same arithmetic, same labels.
// Experiment builds override the knobs with -D; every override is read HERE and nowhere else: SPW, WCCAP, QA_CAP, QC_CAP
// (the lean variant), SCAN16_QA_CAP, SCAN16_QC_CAP, SCAN16_WCCAP (the fat one), WPB, ROWS, SPLIT_TAIL, SCAN_PARK (both: = 0 gives
// the former per-pass form of levels B / D back, profiles/scan_issue_budget.md).
#pragma once
#ifndef SPW
#define SPW 8      // supergroups per slice (<= 16: SG_BITS); staged once per workgroup
#endif
#ifndef WCCAP
#define WCCAP 128  // parked point-0 candidates per wave
#endif
// queue capacities.  Level A leaves ALL of a wavefront's (line, supergroup) pairs in queue A at once when they fit
// (~128 of the 1024 possible; otherwise supergroup by supergroup with drains in between); level B pops 64 of them
// and pushes their passing halves (~1.4 of 8 each, at most 512: split then) on top of < 64 left-overs of queue C.
#ifndef QA_CAP
#define QA_CAP 256
#endif
#ifndef QC_CAP
#define QC_CAP 256
#endif
#ifndef SCAN16_QA_CAP
#define SCAN16_QA_CAP 384
#endif
#ifndef SCAN16_QC_CAP
#define SCAN16_QC_CAP 256
#endif
#ifndef SCAN16_WCCAP
#define SCAN16_WCCAP 128
#endif
#ifndef SPLIT_TAIL
#define SPLIT_TAIL 1  // a partial pass of level B / D spreads its entries over 2, 4 or 8 lanes each (tail_split below)
#endif
#ifndef SCAN_PARK
#define SCAN_PARK 1   // level D parks a pass's candidates behind one prefix scan of the lanes' counts (proc_c)
#endif
struct Scan8 {
    static constexpr int kSPW = SPW, kQaCap = QA_CAP, kQcCap = QC_CAP, kWcCap = WCCAP;
    static constexpr bool kRegLines = false;
    static constexpr bool kSplitTail = SPLIT_TAIL != 0, kScanPark = SCAN_PARK != 0;
};
// kRegLines: the wavefront's 128 lines stay in REGISTERS (two per lane) and travel between lanes by ds_bpermute instead of
// 24 KB of LDS per workgroup -> 62 VGPRs, 4 workgroups = 32 wavefronts per compute unit instead of 3 / 24.  With 8
// supergroups per slice that measured slower (round 4: 28.3 us against 26.8-27.4 at C2, 13.9 against 12.9 at C1 -- twelve
// cross-lane reads per pass cost more than the extra residency returns); it pays with the fat slice.
struct Scan16 {
    static constexpr int kSPW = 16, kQaCap = SCAN16_QA_CAP, kQcCap = SCAN16_QC_CAP, kWcCap = SCAN16_WCCAP;
    static constexpr bool kRegLines = true;
    static constexpr bool kSplitTail = SPLIT_TAIL != 0, kScanPark = SCAN_PARK != 0;
};
// common to both variants (a -DWPB=n / -DROWS=n of an experiment build stands in for the constant itself)
#ifndef WPB
constexpr int WPB = 8;     // wavefronts per workgroup: same slice, LPW lines each
#endif
#ifndef ROWS
constexpr int ROWS = 17;   // float4 per staged group row: 16 records + 16 bytes of padding (bank spread)
#endif
constexpr int LPW = 128;   // lines per wavefront (two per lane in level A)
constexpr int SG_BITS = 4;            // queue entries: line << SG_BITS | supergroup of the slice,
constexpr int HF_BITS = SG_BITS + 3;  //                line << HF_BITS | half of the slice (7 + 7 bits: 16-bit entries)
static_assert(Scan8::kSPW <= (1 << SG_BITS) && Scan16::kSPW <= (1 << SG_BITS), "slot bits of the queue entries");
static_assert(LPW <= (1 << (32 - CAND_POS_BITS)), "line-in-wave bits of the candidates (rrl_tree.h CAND_POS_BITS)");

// the wavefront's 128 lines during the walk: in registers, or in LDS
template <bool REGLINES> struct WaveLines;
template <> struct WaveLines<true> {
    float v0[6], v1[6];           // this lane's two lines (dir, x0): line `lane` and line `64 + lane` of the wavefront
};
template <> struct WaveLines<false> {
    const float2 *lr;             // this wave's lines in LDS as they lie in memory: 3 float2 per line (dir.xy | dir.z x0.x | x0.yz)
};
template <class V>
struct WaveCtx {
    WaveLines<V::kRegLines> ln;
    const float4 *recs;           // LDS: staged records of the slice, [group][ROWS]
    const float4 *nodes;          // LDS: staged tree nodes of the slice, [supergroup][NODE]
    unsigned short *qa, *qc;      // LDS queues: line << SG_BITS | sg, line << HF_BITS | half (slice-local)
    unsigned *cands;              // LDS [V::kWcCap]
    const int32_t *idx;           // sorted position -> original triangle index
    const float *ptri;            // prepared triangles: rows in original order, or -- psorted -- at their sorted positions
    __amdgpu_buffer_rsrc_t ptri_rs;  // SC1 (the chained step's launch): the same rows through a buffer descriptor, for sc1 loads
    bool sc1;                     // (uniform) ... which only the SOURCE cloud's workgroups need: its rows were written in this launch
    bool psorted;                 // uniform: the layout of ptri (the prepared build leaves sorted rows)
    int32_t *cnt, *hit;           // per-line hit count / slots of the cloud
    int lbase;                    // first line of this wave
    int pos0;                     // sorted position of the slice's first record
    int na, nc, ncand;            // wave-uniform fill levels
    int lane;
    // executed-work counters of the COUNT instantiation (wave-uniform; see rrl_scan_counters)
    unsigned tb, tc, td, tcand;   // level-B half-sphere tests, halves that passed, point-0 prefilter tests, resolved candidates
    int32_t *status;              // NaN flag of the call
};

// line ll of the wave from its raw 24-byte row: (dir, x0.x) and (x0.y, x0.z)
struct LineRow {
    float4 la;
    float2 lb;
};
__device__ __forceinline__ LineRow line_row(const float2 *lr, int ll) {
    const float2 *p = lr + 3 * ll;
    const float2 a = p[0], b = p[1], c = p[2];
    return {make_float4(a.x, a.y, b.x, b.y), c};
}
// Line ll (0 .. 127) of the wavefront from the registers of the lane that holds it: EVERY lane of the wavefront must
// call (a ds_bpermute reads the registers of active lanes only); lanes without work pass any ll.  Twelve cross-lane
// reads + six selects instead of three 8-byte LDS reads -- and 24 KB of LDS per workgroup less: 22.3 KB instead of 47.2,
// so the wavefront limit (8 per SIMD), not LDS, bounds the residency: 4 workgroups per compute unit instead of 3.
__device__ __forceinline__ LineRow line_get(const WaveLines<true> &c, int ll) {
    const int src = (ll & 63) << 2;
    const bool hi = ll >= 64;
    float r[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        const int a = __builtin_amdgcn_ds_bpermute(src, __float_as_int(c.v0[q]));
        const int b = __builtin_amdgcn_ds_bpermute(src, __float_as_int(c.v1[q]));
        r[q] = __int_as_float(hi ? b : a);
    }
    return {make_float4(r[0], r[1], r[2], r[3]), make_float2(r[4], r[5])};
}

// cand = line_in_wave << CAND_POS_BITS | sorted triangle position: a triangle whose point 0 passed the conservative
// prefilter of level D.  The reference's own arithmetic (dist_sq, bit-identical to the strict scan) decides
// on all three points here.
// SC1: the rows may have been written by another workgroup of THIS launch (write-through): loads that bypass the CU's L1.
template <class V, bool SC1 = false>
__device__ __forceinline__ void resolve_candidate(const WaveCtx<V> &c, unsigned cand, const LineRow &lrw) {
    const int ll = cand >> CAND_POS_BITS, spos = cand & CAND_POS_MASK;
    const float4 la = lrw.la;
    const float2 lb = lrw.lb;
    // original-order rows: one more dependent load for the row index (staging the slice's indices in LDS measured 0.8 us
    // slower); sorted rows (prepared build): the row sits at the candidate's position and carries its triangle index
    const int prow = c.psorted ? spos : c.idx[spos];
    float4 r0, r1, r2;  // P0 P1.x | P1.yz P2.xy | P2.z thr2 thr index
    if (SC1 && c.sc1) {
        const unsigned o = (unsigned)prow * (PTRI_STRIDE * 4);
        r0 = ld16_sc1(c.ptri_rs, o); r1 = ld16_sc1(c.ptri_rs, o + 16); r2 = ld16_sc1(c.ptri_rs, o + 32);
    } else {
        const float4 *q = (const float4 *)(c.ptri + PTRI_STRIDE * (size_t)prow);
        r0 = q[0]; r1 = q[1]; r2 = q[2];
    }
    const int f = __float_as_int(r2.w);
    const uint32_t thr2 = __float_as_uint(r2.y);
    const uint32_t x0 = __float_as_uint(dist_sq<float>(r0.x, r0.y, r0.z, la.x, la.y, la.z, la.w, lb.x, lb.y));
    const uint32_t x1 = __float_as_uint(dist_sq<float>(r0.w, r1.x, r1.y, la.x, la.y, la.z, la.w, lb.x, lb.y));
    const uint32_t x2 = __float_as_uint(dist_sq<float>(r1.z, r1.w, r2.x, la.x, la.y, la.z, la.w, lb.x, lb.y));
    // a negative sqrt argument is the reference's NaN (code/loss.py:88-91); candidates are rare
    if ((x0 | x1 | x2) >= 0x80000000u) atomicOr(&c.status[0], 1);
    if (max(max(x0, x1), x2) < thr2) {  // sign bit set (negative / NaN) -> huge: never a hit
        const int l = c.lbase + ll;
        int pos = atomicAdd(&c.cnt[l], 1);
        if (pos < RRL_MAX_HITS) c.hit[(size_t)l * RRL_MAX_HITS + pos] = f;
    }
}

__device__ __forceinline__ void wave_lds_fence() {
    // LDS is processed in order per wave; this only stops the compiler from reordering across it
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}

__device__ __forceinline__ int lane_rank(unsigned long long m) {  // set bits of m below this lane
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// Slack of the culling bound (header) for one (cloud, sample) from the maxima over its cullable lines: s = max |dir|^2,
// o2 = max |x0|^2, pm = max |P|^2.  Every term is monotone in s and o2, so the values cover each admitted line.
struct CloudSlack {
    bool ok;       // pm is finite and moderate (else: every wavefront of this cloud takes the strict loop)
    bool nanwide;  // g > 0: a negative sqrt argument is not excluded at this scale
    float se;      // slack of the node radii
    float s0;      // slack of the point-0 prefilter
};
// max over the wavefront of NON-NEGATIVE floats (or NaN, which then wins: its bit pattern is the largest) on their bit
// patterns: v_max_u32 takes the DPP operand directly (the float version needs a canonicalising v_max per step), and
// the four row results meet in scalar registers.  Every lane receives the result.
__device__ __forceinline__ float wave_max_nonneg(float v) {
    unsigned u = __float_as_uint(v);
    // (old = 0, the identity of max on unsigned: only then does the compiler fold the lane move into v_max_u32's DPP operand --
    //  with old = x it issued a copy, the DPP move and the max, three instructions a step; every lane has a source lane here)
#define RRL_DPP_U(x, ctrl) (unsigned)__builtin_amdgcn_update_dpp(0, (int)(x), ctrl, 0xf, 0xf, false)
    u = max(u, RRL_DPP_U(u, 0xB1)); u = max(u, RRL_DPP_U(u, 0x4E));
    u = max(u, RRL_DPP_U(u, 0x141)); u = max(u, RRL_DPP_U(u, 0x140));
#undef RRL_DPP_U
    const unsigned a = (unsigned)__builtin_amdgcn_readlane((int)u, 0), b = (unsigned)__builtin_amdgcn_readlane((int)u, 16);
    const unsigned c = (unsigned)__builtin_amdgcn_readlane((int)u, 32), d = (unsigned)__builtin_amdgcn_readlane((int)u, 48);
    return __uint_as_float(max(max(a, b), max(c, d)));
}
// square root / reciprocal for the SLACKS only (never for a label): the hardware approximations (1 ulp), nudged upwards
// so that the result is >= the exact one -- a slack may be too large by 1e-6 of itself, never too small.  (The IEEE
// sqrtf / division sequences were ~55 of the ~250 VALU instructions of every wavefront's prologue.)
__device__ __forceinline__ float sqrt_up(float x) { return __builtin_amdgcn_sqrtf(x) * 1.0000005f; }
__device__ __forceinline__ float rcp_up(float x) { return __builtin_amdgcn_rcpf(x) * 1.0000005f; }

__device__ __forceinline__ CloudSlack cull_cloud_slack(float s, float o2, float pm) {
    CloudSlack r;
    r.ok = pm <= 1.0e11f;  // (false for NaN / inf: non-finite coordinates)
    const float A2 = (o2 + pm + 2.0f * sqrt_up(o2 * pm)) * 1.00001f;  // (|x0| + max|P|)^2, rounded up
    const float eta = fmaxf(s - 1.0f, 0.0f) + 2.5e-7f;  // |d|^2 - 1 incl. the rounding of s (<= 3u s)
    const float x = eta * A2;
    const float g = 1.8e-6f * A2 - 2e-4f;  // 30u = 1.788e-6
    r.nanwide = g > 0.0f;
    // (-0.999 g under the root: a smaller divisor, i.e. a larger quotient; the approximations only add to that)
    const float se = g > 0.0f ? sqrt_up(g + x) : fminf(sqrt_up(x), x * 0.5f * rcp_up(__builtin_amdgcn_sqrtf(-0.998f * g)));
    r.se = se * 1.0001f + 1e-12f;
    r.s0 = 3.0e-6f * A2 + 1.0e-9f;  // 44.2 u A^2 of evaluation error on both sides, rounded up, + an absolute floor
    return r;
}

// conservative sphere test of one line against one STAGED tree node (centre, w = (Rs + se)^2 rounded up, or -inf for
// an empty node; see the culling bound above): the node is kept when  d2 - 4e-6 q <= w,  evaluated as ONE FMA chain
// whose SIGN BIT says "cannot be reached":  m = (a.d)^2 + (w - 0.999996 |a|^2)  (exactly the negation of the form
// d2 - 4e-6 q - w; -0 cannot occur, -inf - ... stays negative)
__device__ __forceinline__ float sphere_margin(const float4 nd, const float4 la, const float2 lb) {
    const float ax = nd.x - la.w, ay = nd.y - lb.x, az = nd.z - lb.y;
    const float dot = fmaf(az, la.z, fmaf(ay, la.y, ax * la.x));
    const float q = fmaf(az, az, fmaf(ay, ay, ax * ax));
    return fmaf(dot, dot, fmaf(-q, 0.999996f, nd.w));
}

template <class V, bool COUNT, bool SC1 = false>
__device__ __forceinline__ void flush_cands(WaveCtx<V> &c) {
#ifdef CULL_NO_RESOLVE
    c.ncand = 0;
    return;
#endif
    wave_lds_fence();
    const int nc = min(c.ncand, V::kWcCap);
    if constexpr (COUNT) c.tcand += (unsigned)c.ncand;  // entries past kWcCap were resolved inline: counted here too
    if constexpr (V::kRegLines) {
        for (int i0 = 0; i0 < nc; i0 += 64) {  // uniform trip count: every lane fetches (line_get), the live ones resolve
            const int i = i0 + c.lane;
            const unsigned cand = i < nc ? c.cands[i] : 0u;
            const LineRow lrw = line_get(c.ln, (int)(cand >> CAND_POS_BITS));
            if (i < nc) resolve_candidate<V, SC1>(c, cand, lrw);
        }
    } else {
        for (int i = c.lane; i < nc; i += 64) {
            const unsigned cand = c.cands[i];
            resolve_candidate<V, SC1>(c, cand, line_row(c.ln.lr, (int)(cand >> CAND_POS_BITS)));
        }
    }
    c.ncand = 0;
}

// all = false: only while at least 64 entries wait (full lanes); all = true: drain.

// A drain's LAST pass of level B or D holds `take` < 64 entries (one per wavefront and level at C2: 81 pairs and 96 halves
// wait on average, so the second pass runs 17 and 32 of 64 lanes) and used to issue all 8 tests of an entry for them.
// kSplitTail: 2^k lanes share an entry (k = 1, 2, 3 while take <= 32, 16, 8), each running 8 >> k of its tests -- the same
// test on the same operands, only in another lane; the lanes keep their own bits and push them themselves.
template <int N> struct TailPer { static constexpr int v = N; };  // tests per lane of a pass: 8 (k = 0), 4, 2, 1
template <class V>
__device__ __forceinline__ int tail_split(int take) {
    if constexpr (!V::kSplitTail) return 0;
    return take <= 8 ? 3 : (take <= 16 ? 2 : (take <= 32 ? 1 : 0));  // uniform
}

// level D: pops (line, half) pairs, ONE per lane (8 records = 32 registers in flight), and runs the point-0
// PREFILTER on the half's 8 records: e = fl(Q(P0)) + c by FMAs, with the staged c = -(thr2 - 2e-4 + slack)
// (see "Point-0 prefilter" above): 10 operations and one v_alignbit per record instead of the 16 + 3 of
// the reference's unfused arithmetic.  e < 0 (sign bit) parks the triangle as a candidate; the exact test of
// all three points happens there (resolve_candidate), on ~3 % of the records.
template <class V, bool COUNT, bool SC1 = false>
__device__ __forceinline__ void proc_c(WaveCtx<V> &c, bool all) {
#ifdef CULL_STOP_C  // timing experiments only (tools/attic/knob_sweep.sh): the level is formed but not run
    c.nc = 0;
    return;
#endif
    while (c.nc >= 64 || (all && c.nc > 0)) {
        const int take = min(c.nc, 64), base = c.nc - take;
        c.nc = base;
        if constexpr (COUNT) c.td += 8u * (unsigned)take;
        wave_lds_fence();
        uint32_t passbits = 0;
        unsigned lh = 0;  // line << CAND_POS_BITS | first sorted position of the half
        const int k = tail_split<V>(take), slot = c.lane >> k;  // (k uniform) the lane's entry of this pass
        // (registers: every lane takes part in line_get, so entry and line are fetched in front of the branch; LDS: behind it)
        unsigned e = 0u;
        LineRow lrw;
        if constexpr (V::kRegLines) {
            e = slot < take ? c.qc[base + slot] : 0u;
            lrw = line_get(c.ln, (int)(e >> HF_BITS));
        }
        if (slot < take) {
            if constexpr (!V::kRegLines) {
                e = c.qc[base + slot];
                lrw = line_row(c.ln.lr, (int)(e >> HF_BITS));
            }
            const int ll = e >> HF_BITS, h = e & ((1 << HF_BITS) - 1);
            const float4 la = lrw.la;
            const float2 lb = lrw.lb;
            const float4 *row = c.recs + (h >> 1) * ROWS + (h & 1) * 8;
            auto test = [&](const float4 rec) {  // passbits << 1 | sign(ev)
                const float ax = rec.x - la.w, ay = rec.y - lb.x, az = rec.z - lb.y;
                const float dot = fmaf(az, la.z, fmaf(ay, la.y, ax * la.x));
                const float q = fmaf(az, az, fmaf(ay, ay, fmaf(ax, ax, rec.w)));
                const float ev = fmaf(-dot, dot, q);
                passbits = __builtin_amdgcn_alignbit(passbits, __float_as_uint(ev), 31);
            };
            auto part = [&](auto per_) {  // this lane's records t0 .. t0 + per - 1; record t ends up in bit t
                constexpr int per = decltype(per_)::v;
                const int t0 = (c.lane & (8 / per - 1)) * per;
#pragma unroll
                for (int t = per - 1; t >= 0; --t) test(row[t0 + t]);
                passbits <<= t0;
            };
            if (k == 0) part(TailPer<8>());  // (uniform)
            else if (k == 1) part(TailPer<4>());
            else if (k == 2) part(TailPer<2>());
            else part(TailPer<1>());
            lh = ((unsigned)ll << CAND_POS_BITS) | (unsigned)(c.pos0 + h * 8);
        }
        if constexpr (V::kScanPark) {
            // usual case: the pass's candidates fit the buffer -- every lane parks its own run behind an exclusive prefix of the
            // counts (one DPP scan, as push_halves does, instead of a ballot / rank round per candidate of the fullest lane)
            const int cnt = __popc(passbits);
            const int incl = wave_incl_scan(cnt);
            const int total = __builtin_amdgcn_readlane(incl, 63);
            if (c.ncand + total <= V::kWcCap) {  // uniform
                int at = c.ncand + incl - cnt;
                while (passbits) {
                    const int t = __ffs(passbits) - 1;
                    passbits &= passbits - 1;
                    c.cands[at++] = lh + (unsigned)t;
                }
                c.ncand += total;
            }
        }
        while (__any(passbits != 0)) {  // (kScanPark: only a pass whose candidates do not fit)
            if constexpr (V::kRegLines)  // uniform: room for this round's <= 64 candidates (no inline resolve)
                if (c.ncand > V::kWcCap - 64) flush_cands<V, COUNT, SC1>(c);
            const bool has = passbits != 0;
            const unsigned long long m = __ballot(has);
            const int t = has ? __ffs(passbits) - 1 : 0;
            passbits &= passbits - 1;
            const int pos = c.ncand + lane_rank(m);
            const unsigned cand = lh + (unsigned)t;
            if (has) {
                if constexpr (V::kRegLines) c.cands[pos] = cand;
                else if (pos < V::kWcCap) c.cands[pos] = cand;
                else resolve_candidate<V, SC1>(c, cand, line_row(c.ln.lr, (int)(cand >> CAND_POS_BITS)));
            }
            c.ncand += __popcll(m);
        }
        if (c.ncand > V::kWcCap - 64) flush_cands<V, COUNT, SC1>(c);  // uniform: keep room for the next pass
    }
}

// The passing halves of one level-B pass (bit k of `pass`: half 8 sg + k of the lane's entry; e2 = line << HF_BITS |
// 8 sg) go to queue C.  Usual case: every lane writes its own run of entries behind an exclusive prefix of the
// counts (one DPP scan instead of eight ballot / rank rounds).  Too many for the queue (dense hits): half by half
// with drains in between.
template <class V, bool COUNT, bool SC1 = false>
__device__ __forceinline__ void push_halves(WaveCtx<V> &c, unsigned pass, unsigned e2) {
    const int cnt = __popc(pass);
    const int incl = wave_incl_scan(cnt);
    const int total = __builtin_amdgcn_readlane(incl, 63);
    if (total == 0) return;  // uniform
    if constexpr (COUNT) c.tc += (unsigned)total;
    if (c.nc + total > V::kQcCap) proc_c<V, COUNT, SC1>(c, false);  // leaves < 64
    if (c.nc + total > V::kQcCap) {
        for (int k = 0; k < 8; ++k) {  // uniform
            const bool p = (pass >> k) & 1u;
            const unsigned long long m = __ballot(p);
            if (m == 0ull) continue;
            if (c.nc > V::kQcCap - 64) proc_c<V, COUNT, SC1>(c, false);
            if (p) c.qc[c.nc + lane_rank(m)] = (unsigned short)(e2 | (unsigned)k);
            c.nc += __popcll(m);
        }
        return;
    }
    int at = c.nc + incl - cnt;
    while (pass) {
        const int k = __ffs(pass) - 1;
        pass &= pass - 1;
        c.qc[at++] = (unsigned short)(e2 | (unsigned)k);
    }
    c.nc += total;
}

// level B: pops (line, supergroup) pairs, one per lane, and tests the supergroup's EIGHT half spheres directly
// (round 3: the group level in between -- 4 group tests, then 2 half tests per passing group, 9 tests on average
// -- cost a whole round of queue passes per wavefront for one test less)
template <class V, bool COUNT, bool SC1 = false>
__device__ __forceinline__ void proc_a(WaveCtx<V> &c, bool all) {
#ifdef CULL_STOP_A
    c.na = 0;
    return;
#endif
    while (c.na >= 64 || (all && c.na > 0)) {
        const int take = min(c.na, 64), base = c.na - take;
        c.na = base;
        if constexpr (COUNT) c.tb += 8u * (unsigned)take;
        wave_lds_fence();
        unsigned pass = 0u;  // bit j: half j may be reached (idle lanes: none)
        unsigned e2 = 0;
        const int k = tail_split<V>(take), slot = c.lane >> k;  // (as in proc_c)
        unsigned e = 0u;  // (fetched as in proc_c)
        LineRow lrw;
        if constexpr (V::kRegLines) {
            e = slot < take ? c.qa[base + slot] : 0u;
            lrw = line_get(c.ln, (int)(e >> SG_BITS));
        }
        if (slot < take) {
            if constexpr (!V::kRegLines) {
                e = c.qa[base + slot];
                lrw = line_row(c.ln.lr, (int)(e >> SG_BITS));
            }
            const int ll = e >> SG_BITS, sg = e & ((1 << SG_BITS) - 1);
            const float4 la = lrw.la;
            const float2 lb = lrw.lb;
            const float4 *nd = c.nodes + sg * NODE + 5;
            auto part = [&](auto per_) {  // this lane's halves j0 .. j0 + per - 1; half j ends up in bit j
                constexpr int per = decltype(per_)::v;
                const int j0 = (c.lane & (8 / per - 1)) * per;
                unsigned fail = 0u;  // bit j - j0: half j cannot be reached
#pragma unroll
                for (int j = per - 1; j >= 0; --j)
                    fail = __builtin_amdgcn_alignbit(fail, __float_as_uint(sphere_margin(nd[j0 + j], la, lb)), 31);
                pass = (~fail & ((1u << per) - 1u)) << j0;
            };
            if (k == 0) part(TailPer<8>());  // (uniform)
            else if (k == 1) part(TailPer<4>());
            else if (k == 2) part(TailPer<2>());
            else part(TailPer<1>());
            e2 = ((unsigned)ll << HF_BITS) | (unsigned)(8 * sg);
        }
        push_halves<V, COUNT, SC1>(c, pass, e2);
    }
}

// The strict loop of a wavefront that cannot be culled (a line with |dir|^2 > 1 + 1e-6 or non-finite
// data): ALL pairs of its 128 lines with the records at sorted positions [s0, s1), the reference's
// semantics, NaN included.  The lane's two lines arrive packed (.x = line l0, .y = line l1).
__device__ __forceinline__ void strict_slice(const float *ptri, const int32_t *idx, bool psorted, int s0, int s1, v2f ux,
                                                       v2f uy, v2f uz, v2f ox, v2f oy, v2f oz, int l0, int l1, int L,
                                                       int32_t *cnt, int32_t *hit, int32_t *status) {
    kptr tp0 = (kptr)(uintptr_t)ptri;
    kiptr ik = (kiptr)(uintptr_t)idx;
    uint32_t nanacc = 0;
    for (int sp = s0; sp < s1; ++sp) {
        kptr tp = tp0 + (size_t)(psorted ? sp : ik[sp]) * PTRI_STRIDE;
        const uint32_t thr2 = __float_as_uint(tp[9]);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float dx = h ? ux.y : ux.x, dy = h ? uy.y : uy.x, dz = h ? uz.y : uz.x;
            const float px = h ? ox.y : ox.x, py = h ? oy.y : oy.x, pz = h ? oz.y : oz.x;
            const int l = h ? l1 : l0;
            const uint32_t x0 = __float_as_uint(dist_sq<float>(tp[0], tp[1], tp[2], dx, dy, dz, px, py, pz));
            const uint32_t x1 = __float_as_uint(dist_sq<float>(tp[3], tp[4], tp[5], dx, dy, dz, px, py, pz));
            const uint32_t x2 = __float_as_uint(dist_sq<float>(tp[6], tp[7], tp[8], dx, dy, dz, px, py, pz));
            const uint32_t mm = max(max(x0, x1), x2);  // negative or NaN: sign bit set -> huge
            if (l < L) {
                nanacc = max(nanacc, mm);
                if (mm < thr2) {
                    const int pos = atomicAdd(&cnt[l], 1);
                    if (pos < RRL_MAX_HITS) hit[(size_t)l * RRL_MAX_HITS + pos] = __float_as_int(tp[11]);
                }
            }
        }
    }
    if (nanacc >= 0x80000000u) atomicOr(&status[0], 1);
}

// The culled walk of one wavefront over the STAGED slice (node_lds / ctx.recs): level A on the lane's two lines,
// level B, level D, candidate resolution.  stamps (COUNT): wall clock after level A, after level B's drain, after
// level D's drain.
template <class V, bool COUNT, bool SC1 = false>
__device__ __forceinline__ void cull_walk(WaveCtx<V> &ctx, const float4 *node_lds, int nsl, int lane, bool live0, bool live1,
                                          v2f ux, v2f uy, v2f uz, v2f ox, v2f oy, v2f oz, unsigned long long *stamps) {
    // ---- level A: conservative sphere test of every supergroup of the slice against the lane's two lines
    //      (packed fp32; the staged supergroup nodes come as wave-uniform LDS reads).  No queue traffic inside the
    //      loop: the outcome is one bit per (line, supergroup) in two lane-private masks (sign bits, v_alignbit).
    unsigned f0m = 0u, f1m = 0u;  // bit s: supergroup s cannot be reached by line 0 / line 1 of the lane
#pragma unroll
    for (int s = V::kSPW - 1; s >= 0; --s) {  // supergroup s ends up in bit s
        float4 nd = node_lds[(s < nsl ? s : 0) * NODE];
        if (s >= nsl) nd.w = -INFINITY;  // uniform: not part of this slice
        const v2f ax = nd.x - ox, ay = nd.y - oy, az = nd.z - oz;
        const v2f dot = __builtin_elementwise_fma(az, uz, __builtin_elementwise_fma(ay, uy, ax * ux));
        const v2f q = __builtin_elementwise_fma(az, az, __builtin_elementwise_fma(ay, ay, ax * ax));
        const v2f w2 = {nd.w, nd.w};
        const v2f mg = __builtin_elementwise_fma(dot, dot, __builtin_elementwise_fma(-q, (v2f){0.999996f, 0.999996f}, w2));
        f0m = __builtin_amdgcn_alignbit(f0m, __float_as_uint(mg.x), 31);
        f1m = __builtin_amdgcn_alignbit(f1m, __float_as_uint(mg.y), 31);
    }
    unsigned m0 = live0 ? (~f0m & ((1u << V::kSPW) - 1u)) : 0u, m1 = live1 ? (~f1m & ((1u << V::kSPW) - 1u)) : 0u;
    {
        const int cnt_ = __popc(m0) + __popc(m1);
        const int incl = wave_incl_scan(cnt_);
        const int total = __builtin_amdgcn_readlane(incl, 63);
        if (total <= V::kQaCap) {  // the usual case (~128): every lane writes its own run of entries
            int at = incl - cnt_;
            while (m0) {
                const int s = __ffs(m0) - 1;
                m0 &= m0 - 1;
                ctx.qa[at++] = (unsigned short)((lane << SG_BITS) | s);
            }
            while (m1) {
                const int s = __ffs(m1) - 1;
                m1 &= m1 - 1;
                ctx.qa[at++] = (unsigned short)(((64 + lane) << SG_BITS) | s);
            }
            ctx.na = total;
        } else {  // dense hits: supergroup by supergroup, level B in between
            for (int s = 0; s < nsl; ++s) {
                const bool p0 = (m0 >> s) & 1u, p1 = (m1 >> s) & 1u;
                const unsigned long long b0 = __ballot(p0), b1 = __ballot(p1);
                if ((b0 | b1) == 0ull) continue;
                if (ctx.na > V::kQaCap - 128) proc_a<V, COUNT, SC1>(ctx, false);
                const int c0 = __popcll(b0);
                if (p0) ctx.qa[ctx.na + lane_rank(b0)] = (unsigned short)((lane << SG_BITS) | s);
                if (p1) ctx.qa[ctx.na + c0 + lane_rank(b1)] = (unsigned short)(((64 + lane) << SG_BITS) | s);
                ctx.na += c0 + __popcll(b1);
            }
        }
    }
    if constexpr (COUNT) stamps[0] = wall_clock64();
    proc_a<V, COUNT, SC1>(ctx, true);
    if constexpr (COUNT) stamps[1] = wall_clock64();
    proc_c<V, COUNT, SC1>(ctx, true);
    if constexpr (COUNT) stamps[2] = wall_clock64();
    flush_cands<V, COUNT, SC1>(ctx);
}

// COUNT = true: the same kernel with executed-work counters -- launched instead of the plain one while
// rrl_scan_counters() holds a buffer.  Every wavefront WRITES one row of 16 u64 (plain stores: thousands of
// same-address atomics serialise at ~12 ns each and distort the kernel they measure), row index = linear
// workgroup id x wavefronts per workgroup + wavefront; rows past the buffer's capacity are dropped:
//   row[0] level-A sphere tests (line x supergroup)   [1] level-B half-sphere tests (8 per (line, supergroup) pair)
//           [2] halves that passed (line x half)           [3] point-0 prefilter tests (line x record)
//           [4] candidates resolved (points 1, 2)          [5] wavefronts that ran
//           [6] wavefronts that took the strict fallback   [7] (line, triangle) pairs of the fallback
//           [8] start, [9] end of the wavefront on the 100 MHz wall clock (the kernel lasts as long as its
//           slowest wavefront: tools/scan_tail.py prints the spread), [10..14] phase stamps
// The scan's LDS (47 KiB per 8-wavefront workgroup) as ONE object: cull_scan_chamfer_kernel overlays it with the Chamfer
// walk's (rrl_chamfer_walk.h ChamLds).
template <class V>
struct CullLds {
    __attribute__((aligned(16))) float2 line_lds[V::kRegLines ? 0 : WPB][LPW * 3];  // 24 KiB: raw 24-byte line rows (none: lines in registers)
    __attribute__((aligned(16))) float4 rec_lds[V::kSPW * SGG * ROWS];  //  8.5 KiB (kSPW = 8)
    __attribute__((aligned(16))) float4 node_lds[V::kSPW * NODE];       //  1.6 KiB
    __attribute__((aligned(16))) unsigned short qa_lds[WPB][V::kQaCap];
    unsigned short qc_lds[WPB][V::kQcCap];
    __attribute__((aligned(16))) unsigned cands_lds[WPB][V::kWcCap];
};

// What a scan workgroup reads: the kernel arguments of cull_scan_chamfer_kernel (CullKArgs; its gx, gy are that launch's own grid
// decode) and, beyond them, what only some launches have (ScanArgs).  cull_scan_body takes ONE of these.
struct CullKArgs {
    const float *ptri1, *ptri2;
    const float4 *p0s1, *p0s2;
    const int32_t *idx1, *idx2;
    const float4 *tree1, *tree2;
    const float *line;
    int32_t *count1, *hit1, *count2, *hit2, *status;
    uint32_t *pmax;
    const float *del1, *del2;
    const float2 *lmax;
    const float *apart, *aflag;
    const float *aflag_tar;  // the partial rows of the workspace that holds cloud 2 (== aflag unless the target is carried over)
    int nblk_apart, B, N, M, L, spw, gx, gy, Bt;
};
struct ScanArgs : CullKArgs {                  // (status: the NaN flag / fallback count the body writes)
    unsigned long long *counters = nullptr;    // COUNT: executed-work rows, see below
    long long counter_rows = 0;
    const int32_t *cnt1 = nullptr, *cnt2 = nullptr, *nlines = nullptr;  // a ragged batch's per-sample counts, or null
};

// One workgroup of the culled scan: (bx, by, bz) = its place in the scan's grid (gx, gy: the grid's first two extents)
// -- blockIdx / gridDim in cull_scan_kernel, decoded from a linear index in cull_scan_chamfer_kernel.
// TILEMAX (the chained step's launch, cull_scan_build_kernel): the line maxima behind the slacks are those of the WORKGROUP's
// own tile of lines -- every wavefront reduces its 128 lines, the eight results meet in LDS (one more barrier) -- instead
// of the sample-wide LMAX partials, which that launch has no records kernel in front of it to reduce.  Any bound >= the
// wavefront's own lines is a valid (conservative) slack: same labels, same hit lists.
struct NoWait { __device__ __forceinline__ void operator()() const {} };
template <class V, bool COUNT, bool TILEMAX = false, class Wait = NoWait>
__device__ __forceinline__ void cull_scan_body(CullLds<V> &lds_, const ScanArgs &args, const int bx, const int by, const int bz, const int gx,
                                               const int gy, Wait wait_ready = Wait()) {
    // the chained launch (TILEMAX) always runs 64 * WPB lanes: blockDim.x is a HIDDEN kernel argument, a cache line of its own
    // far behind the explicit ones and one more dependent scalar round in front of the line loads
    // (a copy: its members are plain values to the compiler when it simplifies this function on its own, ahead of inlining it, as
    //  the members of a record behind a reference are not -- all eight kernels' instruction streams depend on it)
    const ScanArgs a = args;
    auto bdim = []() { if constexpr (TILEMAX) return 64u * WPB; else return blockDim.x; };
    auto nwv = []() { if constexpr (TILEMAX) return (int)WPB; else return (int)(blockDim.x >> 6); };
    float4 (&rec_lds)[V::kSPW * SGG * ROWS] = lds_.rec_lds;
    float4 (&node_lds)[V::kSPW * NODE] = lds_.node_lds;
    unsigned short (&qa_lds)[WPB][V::kQaCap] = lds_.qa_lds;
    unsigned short (&qc_lds)[WPB][V::kQcCap] = lds_.qc_lds;
    unsigned (&cands_lds)[WPB][V::kWcCap] = lds_.cands_lds;
    static_assert(WPB * V::kWcCap >= V::kSPW * SGT, "the NaN-reach scratch aliases the (still unused) candidate buffers");
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform for the compiler
#ifdef CULL_DELAY_HALF  // experiment: every second workgroup enters ~2 us late -- does "first loads back" of the
    if ((bx + gx * (by + gy * bz)) & 1) __builtin_amdgcn_s_sleep(75);  // others move with the size of the load burst?
#endif
    const unsigned long long wall0 = COUNT ? wall_clock64() : 0ull;
    unsigned long long *crow = nullptr;
    if constexpr (COUNT) {
        const long long wid = (((long long)bz * gy + by) * gx + bx) * (blockDim.x >> 6) + wave;
        if (wid < a.counter_rows) crow = a.counters + 16 * wid;
    }
    // XCD-aware mapping: workgroups go to the 8 XCDs round-robin by linear id, and x is the fast
    // index -- with (cloud, sample) on x, all workgroups of one cloud land on the same XCD (when
    // 2B is a multiple of 8), so each XCD's L2 holds 1/8 of the records instead of a copy of all
    const int z = bx, cloud = z >= a.B ? 1 : 0, b = z - cloud * a.B;
    // N, M, L: the capacities = the strides of every array.  A ragged batch (include/rrl.h rrl_opts.count1 / count2 / nlines)
    // has n <= ncap records of this cloud and sample -- at the sorted positions [0, n), like the pad of any cloud with
    // n % 64 != 0 -- and nl <= L lines: two uniform loads; without counts the capacities themselves
    const int ncap = cloud ? a.M : a.N;
    const int n = rrl_rows(cloud ? a.cnt2 : a.cnt1, b, ncap);
    const int nsg = (n + SGT - 1) / SGT, nsgc = (ncap + SGT - 1) / SGT;
    const int sg0 = bz * a.spw;
    if (sg0 >= nsg) return;  // uniform: the smaller cloud (or sample) has fewer slices
    const int nl = rrl_rows(a.nlines, input_of(b, a.Bt), a.L);
    if (by * nwv() * LPW >= nl) return;  // uniform: a tile of lines the sample does not have (nl < L only)
    // multi-pose evaluation (rrl_opts.problems): instance b has the target and lines of problem b % Bt -- the target's scan
    // is the same for every pose, so only the first Bt instances scan cloud 2 (the per-line stage reads it there)
    if (cloud && a.Bt > 0 && b >= a.Bt) return;  // uniform
    const int nsl = min(a.spw, nsg - sg0);
    const float4 *p0s = (cloud ? a.p0s2 : a.p0s1) + (size_t)b * nsgc * SGT;
    const float4 *tree = (cloud ? a.tree2 : a.tree1) + (size_t)b * nsgc * NODE;

    // ---- everything the prologue needs is requested up front, in one round of independent loads: the slice's
    //      records and nodes (one per lane in the usual 8-wavefront workgroup), the sample's line maxima, this
    //      wavefront's 128 lines
    constexpr int RPT = (V::kSPW * SGT + 64 * WPB - 1) / (64 * WPB);  // records per lane of a full workgroup
    static_assert(V::kSPW * NODE <= 64 * WPB, "one node per lane");
    const bool one_each = (int)bdim() == 64 * WPB;
    const int32_t *idx = (cloud ? a.idx2 : a.idx1) + (size_t)b * nsgc * SGT;
    float4 rec0[RPT], nd0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    static_assert(LMAX_CHUNKS == 64, "one partial row per lane");
    // (the line maxima and max |P|^2 are requested FIRST: vector loads return in order, so the slack arithmetic below can
    //  start while the records, nodes and lines requested after them are still in flight)
    float2 lm = make_float2(0.0f, 0.0f);  // (max |dir|^2, max |x0|^2) over 1/64 of the sample's cullable lines
    if constexpr (!TILEMAX) lm = a.lmax[(size_t)b * LMAX_CHUNKS + lane];
    // layout of this cloud's PTRI rows, left by the records launch that built it (slot 7 of its first partial row; not
    // needed before the first candidate is resolved)
    // (TILEMAX -- the chained step -- runs on prepared builds only: sorted rows, and no uniform, i.e. scalar-cache, load of a
    //  word another workgroup of this launch has just written)
    const float play = TILEMAX ? 1.0f : a.aflag[(size_t)(cloud * a.B + b) * a.nblk_apart * 8 + 7];
    // max |P|^2 of the cloud: from the sort kernel (PMAX), or -- prepared clouds, whose build has no single-workgroup stage
    // -- from the records kernel's per-workgroup partial rows, reduced here next to the line maxima (one more independent
    // load of the prologue; one workgroup per cloud and sample leaves PMAX for the later consumers)
    // TILEMAX (the chained launch; measured there, profiles/prologue_rounds.txt): the three requests -- partial rows, records,
    // nodes -- are BUFFER loads whose descriptors span exactly the rows this workgroup may read: a lane past the end gets
    // zeros from the range check instead of sitting out behind an exec mask.  Their lane offsets are computed here, ahead
    // of everything; what remains per request is scalar work and the instruction itself, so no vector register is written
    // between two requests and nothing makes the compiler wait for one of them before the next leaves (it used to put a
    // full wait between the record and the node request of a source workgroup, and one behind the partial rows' loop).
    // The values are only TAKEN here; pmv is folded where the slack needs it.  The plain kernel keeps the loop and the
    // predicated loads: its steps (cold, unkept, ragged) have no measurement of the other form.
    float pmv = 0.0f;
    const int off16 = tid * 16, off32 = lane * 32;
    int offk[RPT];  // (in the vector offset: the range check does not see a scalar offset)
#pragma unroll
    for (int k = 0; k < RPT; ++k) offk[k] = off16 + 64 * WPB * 16 * k;
    auto issue_records = [&]() {
        if constexpr (TILEMAX) {
            const bool pub = cloud == 0;  // (uniform; sc1: the source's rows were written by this launch's records workgroups)
            const int nb = (n + REC_BLK - 1) / REC_BLK;
            const float *ap = a.apart != nullptr ? a.apart + (size_t)(cloud * a.B + b) * a.nblk_apart * 8 + 6 : nullptr;
            // (sizes in 32 bits: at most SORT_CAP records of 16 bytes)
            // (ars: row j's word lies at byte 32 j and is 4 bytes long -> the last one ends at 32 (nb - 1) + 4 = 32 nb - 28)
            const __amdgpu_buffer_rsrc_t ars = rrl_rsrc32(ap, a.apart != nullptr ? nb * 32 - 28 : 0);
            const __amdgpu_buffer_rsrc_t prs = rrl_rsrc32(p0s + (size_t)sg0 * SGT, nsl * (SGT * 16));
            const __amdgpu_buffer_rsrc_t trs = rrl_rsrc32(tree + (size_t)sg0 * NODE, nsl * (NODE * 16));
            // (pmv is DEFINED by exactly one of the three sources -- a value merged with an earlier one would be a register copy,
            //  and a copy waits for every load in flight)
            if (a.apart == nullptr) {  // uniform
                pmv = __uint_as_float(a.pmax[cloud * a.B + b]);
            } else if (nb > 64) {  // uniform; clouds beyond 16384 records: more than one partial row per lane
                float m = 0.0f;
                for (int j = lane; j < nb; j += 64) m = fmaxf(m, pub ? ld4_sc1(ap + (size_t)j * 8) : ap[(size_t)j * 8]);
                pmv = m;
            } else if (pub) {
                pmv = ld4_buf<RRL_POLICY_SC1>(ars, off32);
            } else {
                pmv = ld4_buf<0>(ars, off32);
            }
            if (pub) {
#pragma unroll
                for (int k = 0; k < RPT; ++k) rec0[k] = ld16_buf<RRL_POLICY_SC1>(prs, offk[k]);
                nd0 = ld16_buf<RRL_POLICY_SC1>(trs, off16);
            } else {
#pragma unroll
                for (int k = 0; k < RPT; ++k) rec0[k] = ld16_buf<0>(prs, offk[k]);
                nd0 = ld16_buf<0>(trs, off16);
            }
        } else {
            if (a.apart != nullptr) {  // uniform
                const int nb = (n + REC_BLK - 1) / REC_BLK;
                const float *ap = a.apart + (size_t)(cloud * a.B + b) * a.nblk_apart * 8 + 6;
                for (int j = lane; j < nb; j += 64) pmv = fmaxf(pmv, ap[(size_t)j * 8]);
            } else {
                pmv = __uint_as_float(a.pmax[cloud * a.B + b]);
            }
            if (one_each) {
#pragma unroll
                for (int k = 0; k < RPT; ++k)
                    if (tid + 64 * WPB * k < nsl * SGT) rec0[k] = p0s[(size_t)sg0 * SGT + tid + 64 * WPB * k];
                if (tid < nsl * NODE) nd0 = tree[(size_t)sg0 * NODE + tid];
            }
        }
    };
    // (TILEMAX: the lines are requested FIRST and the wait for the source's records of this launch -- `wait_ready`, the
    //  chained step's kernel passes it -- sits between them and the record loads: a waiting workgroup's lines arrive meanwhile,
    //  and for a workgroup that need not wait the poll's round trip hides behind them)
    if constexpr (!TILEMAX) issue_records();
    // this wave's 128 lines: a full, 16-byte aligned tile arrives as three coalesced 16-byte loads per lane straight
    // into its LDS rows; the lanes then pick up their own two lines from there
    const float *ln = a.line + (size_t)input_of(b, a.Bt) * a.L * 6;
    const int lw0 = (by * nwv() + wave) * LPW;
    const int l0 = lw0 + lane, l1 = l0 + 64;
    const bool live0 = l0 < nl, live1 = l1 < nl;
    const bool has_lines = lw0 < nl;  // a wave without lines (the last tile of the line set) still stages records
    // registers (g0, g1): each lane's own two lines straight into them: three 8-byte loads per line (rows are 24 bytes, 8-byte
    // aligned; the three instructions of a line cover the wavefront's 1536 contiguous bytes completely); rows past L: zero lines
    // LDS (lr, t0 .. t2): the wavefront's rows, a full aligned tile as three 16-byte loads per lane.  The variant that does
    // not use a name never reads it.
    float2 g0[3] = {make_float2(0.0f, 0.0f), make_float2(0.0f, 0.0f), make_float2(0.0f, 0.0f)}, g1[3] = {g0[0], g0[0], g0[0]};
    float2 *const lr = lds_.line_lds[V::kRegLines ? 0 : wave];  // (in front of full_tile: the lean kernels' scalar schedule follows this order)
    const float *lsrc = ln + (size_t)lw0 * 6;
    const bool full_tile = has_lines && lw0 + LPW <= nl && (((uintptr_t)lsrc) & 15) == 0;  // uniform
    float4 t0, t1, t2;
    if constexpr (V::kRegLines) {
        const float2 *s2 = (const float2 *)ln;
        if (live0) { g0[0] = s2[3 * (size_t)l0]; g0[1] = s2[3 * (size_t)l0 + 1]; g0[2] = s2[3 * (size_t)l0 + 2]; }
        if (live1) { g1[0] = s2[3 * (size_t)l1]; g1[1] = s2[3 * (size_t)l1 + 1]; g1[2] = s2[3 * (size_t)l1 + 2]; }
    } else if (full_tile) {
        const float4 *s4 = (const float4 *)lsrc;
        t0 = s4[lane]; t1 = s4[64 + lane]; t2 = s4[128 + lane];
    }

    if constexpr (TILEMAX) { wait_ready(); issue_records(); }

    // ---- slack of this (cloud, sample): the same values in every wavefront and workgroup (no exchange, no barrier)
    float pm = pmv;
    if (a.apart != nullptr) {  // uniform
        pm = wave_max_nonneg(TILEMAX ? fmaxf(0.0f, pmv) : pmv);  // (fmaxf(0, row): what the loop computes for a lane with one row)
        if (by == 0 && bz == 0 && tid == 0) a.pmax[cloud * a.B + b] = __float_as_uint(pm);
    }
    // ---- this wavefront's lines into LDS / registers, the lane's own two lines, their norms
    float v0[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, v1[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    float sa, oa, sb, ob;
    auto lines_in = [&]() {
        if constexpr (V::kRegLines) {
            v0[0] = g0[0].x; v0[1] = g0[0].y; v0[2] = g0[1].x; v0[3] = g0[1].y; v0[4] = g0[2].x; v0[5] = g0[2].y;
            v1[0] = g1[0].x; v1[1] = g1[0].y; v1[2] = g1[1].x; v1[3] = g1[1].y; v1[4] = g1[2].x; v1[5] = g1[2].y;
        } else {
            if (full_tile) {
                float4 *d4 = (float4 *)lr;
                d4[lane] = t0; d4[64 + lane] = t1; d4[128 + lane] = t2;
            } else if (has_lines) {  // ragged tail / odd alignment: 8-byte pieces (a row is 24 bytes), zeros past the end
                const float2 *s2 = (const float2 *)lsrc;
                const int nf2 = (nl - lw0) * 3;
                for (int i = lane; i < LPW * 3; i += 64) lr[i] = i < nf2 ? s2[i] : make_float2(0.0f, 0.0f);
            }

            wave_lds_fence();
            if (has_lines) {
                const LineRow r0 = line_row(lr, lane), r1 = line_row(lr, 64 + lane);
                v0[0] = r0.la.x; v0[1] = r0.la.y; v0[2] = r0.la.z; v0[3] = r0.la.w; v0[4] = r0.lb.x; v0[5] = r0.lb.y;
                v1[0] = r1.la.x; v1[1] = r1.la.y; v1[2] = r1.la.z; v1[3] = r1.la.w; v1[4] = r1.lb.x; v1[5] = r1.lb.y;
            }
        }
        line_norms(v0[0], v0[1], v0[2], v0[3], v0[4], v0[5], sa, oa);
        line_norms(v1[0], v1[1], v1[2], v1[3], v1[4], v1[5], sb, ob);
    };
    float smax, o2max;
    if constexpr (TILEMAX) {
        lines_in();
        // the tile's maxima over its cullable lines (rows past L are zero lines: they add nothing), wavefront by wavefront
        // through LDS -- queue A's rows are free until the walk starts, behind the staging barrier
        const bool c0 = line_cullable(sa, oa), c1 = line_cullable(sb, ob);
        const float sm = wave_max_nonneg(fmaxf(c0 ? sa : 0.0f, c1 ? sb : 0.0f));
        const float om = wave_max_nonneg(fmaxf(c0 ? oa : 0.0f, c1 ? ob : 0.0f));
        if (lane == 0) *(float2 *)&qa_lds[wave][0] = make_float2(sm, om);
        __syncthreads();
        smax = 0.0f; o2max = 0.0f;
        const int nw = nwv();
        for (int w_ = 0; w_ < nw; ++w_) {
            const float2 t = *(const float2 *)&qa_lds[w_][0];
            smax = fmaxf(smax, t.x); o2max = fmaxf(o2max, t.y);
        }
    } else {
        smax = wave_max_nonneg(lm.x); o2max = wave_max_nonneg(lm.y);
    }
    const CloudSlack cs = cull_cloud_slack(smax, o2max, pm);
    const float se = cs.se, s0 = cs.s0;
    const bool nanwide = cs.nanwide;  // uniform over the launch's workgroups of this cloud and sample
    // (COUNT: the slack needs the FIRST loads of the prologue -- line maxima, max |P|^2 --: their arrival time)
    unsigned long long wall_slack = 0ull, wall_prebar = 0ull;
    if constexpr (COUNT) { if (se >= 0.0f) wall_slack = wall_clock64(); }
    // nanwide (header, "NaN"): the NaN reach del of this lane's records, requested while the lines are still in flight
    float dv[RPT];
    const bool psorted = __builtin_amdgcn_readfirstlane(__float_as_int(play)) != 0;  // (1.0f: PTRI / DEL rows at sorted positions)
    if (nanwide && one_each) {
        const float *del = (cloud ? a.del2 : a.del1) + (size_t)b * ncap;
        if (psorted) {  // uniform: the prepared build left DEL at the sorted positions -- no dependent gather through IDX
#pragma unroll
            for (int k = 0; k < RPT; ++k)
                dv[k] = sg0 * SGT + tid + 64 * WPB * k < n ? (TILEMAX && cloud == 0 ? ld4_sc1(del + sg0 * SGT + tid + 64 * WPB * k) : del[sg0 * SGT + tid + 64 * WPB * k]) : 0.0f;
        } else {
            int idx0[RPT];
#pragma unroll
            for (int k = 0; k < RPT; ++k) idx0[k] = tid + 64 * WPB * k < nsl * SGT ? idx[sg0 * SGT + tid + 64 * WPB * k] : 0;
#pragma unroll
            for (int k = 0; k < RPT; ++k) dv[k] = sg0 * SGT + tid + 64 * WPB * k < n ? del[idx0[k]] : 0.0f;
        }
    }
    if constexpr (!TILEMAX) lines_in();
    // Culling (and the lazy evaluation of points 1, 2) is only exact for lines with |dir|^2 <= 1 + 1e-6 and finite,
    // moderate data.  A wavefront with an offending line evaluates ALL pairs of its lines with the slice's
    // triangles strictly instead -- the reference's semantics, NaN included.
    const bool fallback = !cs.ok || !__all(line_cullable(sa, oa) && line_cullable(sb, ob));
    unsigned long long fb_pairs = 0;

    const float *ptri = (cloud ? a.ptri2 : a.ptri1) + (size_t)b * ncap * PTRI_STRIDE;
    int32_t *cnt = (cloud ? a.count2 : a.count1) + (size_t)b * a.L;
    int32_t *hit = (cloud ? a.hit2 : a.hit1) + (size_t)b * a.L * RRL_MAX_HITS;

    // nanwide: the slice's del values meet in LDS (a buffer the walk does not use yet) so that every node lane can
    // take the maximum over ITS records -- one more barrier, only on this path
    float *dl = (float *)&cands_lds[0][0];  // [kSPW * SGT]
    if (nanwide) {
        if (one_each) {
#pragma unroll
            for (int k = 0; k < RPT; ++k)
                if (tid + 64 * WPB * k < nsl * SGT) dl[tid + 64 * WPB * k] = dv[k];
        } else {
            const float *del = (cloud ? a.del2 : a.del1) + (size_t)b * ncap;
            for (int i = tid; i < nsl * SGT; i += bdim()) {
                const int sp = sg0 * SGT + i;
                dl[i] = sp < n ? del[psorted ? sp : idx[sp]] : 0.0f;
            }
        }
        __syncthreads();
    }
    // ---- stage the slice: records (padded rows) and tree nodes, slacks folded in
    //   (P0, thr2) -> (P0, c): c = -(thr2 - 2e-4 + slack), slightly widened; pad records never pass
    //   (centre, Rs) -> (centre, (Rs + se)^2 rounded up); an empty node (NaN radius) -> -inf: fails by its sign
    auto stage_rec = [&](int i, float4 r, float d) {
        float tp = r.w - RRL_EPS;
        if (nanwide) {  // also a candidate when point 1 or 2 could see a negative argument: Q(P0) < (se + e01)^2
            const float reach = se + sqrtf(r.w) * 1.000001f + d;  // e01 <= thr + del <= sqrt(thr2) + del
            tp = fmaxf(tp, reach * reach * 1.000002f);
        }
        r.w = sg0 * SGT + i < n ? -(tp + 1.0e-6f * fabsf(tp) + s0) : INFINITY;
        rec_lds[(i >> 4) * ROWS + (i & 15)] = r;
    };
    auto stage_node = [&](int i, float4 nd) {
        float rt = nd.w + se;
        if (nanwide) {  // node j of supergroup sg covers the records [0] all 64, [1..4] 16 each, [5..12] 8 each
            const int sg = i / NODE, j = i - sg * NODE;
            const int o = j == 0 ? 0 : (j < 5 ? (j - 1) * GRP : (j - 5) * (GRP / 2)), c4 = j == 0 ? SGT / 4 : (j < 5 ? GRP / 4 : GRP / 8);
            const float4 *q = (const float4 *)(dl + sg * SGT + o);  // 32-byte aligned
            float m = 0.0f;
            for (int t = 0; t < c4; ++t) {
                const float4 v = q[t];
                m = fmaxf(m, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
            }
            rt += m;
        }
        const float w = rt * rt * 1.0000003f;
        nd.w = w == w ? w : -INFINITY;
        node_lds[i] = nd;
    };
    if (one_each) {
#pragma unroll
        for (int k = 0; k < RPT; ++k)
            if (tid + 64 * WPB * k < nsl * SGT) stage_rec(tid + 64 * WPB * k, rec0[k], nanwide ? dv[k] : 0.0f);
        if (tid < nsl * NODE) stage_node(tid, nd0);
    } else {
        for (int i = tid; i < nsl * SGT; i += bdim()) stage_rec(i, p0s[(size_t)sg0 * SGT + i], nanwide ? dl[i] : 0.0f);
        for (int i = tid; i < nsl * NODE; i += bdim()) stage_node(i, tree[(size_t)sg0 * NODE + i]);
    }
    if constexpr (COUNT) wall_prebar = wall_clock64();  // this wavefront's own share is staged: what follows is the wait for the others
    __syncthreads();  // the one barrier of the (usual) prologue
    if constexpr (TILEMAX) STAMPR(7);
#ifdef CULL_STOP_STAGE
    return;
#endif
    if (!has_lines) return;  // uniform per wavefront
    const unsigned long long wall_staged = COUNT ? wall_clock64() : 0ull;
    unsigned long long wall_a = 0ull, wall_pa = 0ull, wall_pc = 0ull;

    WaveCtx<V> ctx;
    if constexpr (V::kRegLines) {
#pragma unroll
        for (int q = 0; q < 6; ++q) { ctx.ln.v0[q] = v0[q]; ctx.ln.v1[q] = v1[q]; }
    } else {
        ctx.ln.lr = lr;
    }
    ctx.recs = rec_lds;
    ctx.nodes = node_lds;
    ctx.qa = qa_lds[wave];
    ctx.qc = qc_lds[wave];
    ctx.cands = cands_lds[wave];
    ctx.idx = idx;
    ctx.ptri = ptri;
    ctx.ptri_rs = rrl_rsrc(ptri, (size_t)ncap * PTRI_STRIDE * 4);
    ctx.sc1 = TILEMAX && cloud == 0;
    ctx.psorted = psorted;
    ctx.cnt = cnt;
    ctx.hit = hit;
    ctx.lbase = lw0;
    ctx.na = ctx.nc = ctx.ncand = 0;
    ctx.lane = lane;
    ctx.tb = ctx.tc = ctx.td = ctx.tcand = 0;
    ctx.status = a.status;
    ctx.pos0 = sg0 * SGT;
    const v2f ux = {v0[0], v1[0]}, uy = {v0[1], v1[1]}, uz = {v0[2], v1[2]};
    const v2f ox = {v0[3], v1[3]}, oy = {v0[4], v1[4]}, oz = {v0[5], v1[5]};
    unsigned long long ta = 0;

    if (fallback) {  // rare: kept out of line so that its registers do not count against the culled walk
        const int f0 = sg0 * SGT, f1 = min(n, f0 + nsl * SGT);  // real records sit at sorted positions [0, n)
        strict_slice(ptri, idx, ctx.psorted, f0, f1, ux, uy, uz, ox, oy, oz, l0, l1, nl, cnt, hit, a.status);
        if (lane == 0) atomicAdd(&a.status[1], 1);  // always on: wavefronts that left the culled path
        fb_pairs = (unsigned long long)(f1 - f0) * (unsigned long long)min(LPW, nl - lw0);
    } else {
    ta = (unsigned long long)nsl * (unsigned long long)min(LPW, nl - lw0);

    unsigned long long stamps[3] = {0ull, 0ull, 0ull};
    cull_walk<V, COUNT, TILEMAX>(ctx, node_lds, nsl, lane, live0, live1, ux, uy, uz, ox, oy, oz, stamps);
    wall_a = stamps[0]; wall_pa = stamps[1]; wall_pc = stamps[2];
    }
    if constexpr (COUNT) {
        if (lane == 0 && crow && has_lines) {
            crow[0] = ta;
            crow[1] = ctx.tb; crow[2] = ctx.tc; crow[3] = ctx.td; crow[4] = ctx.tcand;
            crow[5] = 1ull;
            crow[6] = fallback ? 1ull : 0ull;
            crow[7] = fb_pairs;
            crow[8] = wall0; crow[9] = wall_clock64();
            // phase stamps of the culled walk: staged (after the staging barrier), level A done, the final drains
            // of levels B and D done (the remainder up to [9] is the last candidate flush)
            crow[10] = wall_staged; crow[11] = wall_a; crow[12] = wall_pa; crow[13] = wall_pa; crow[14] = wall_pc;
            // inside the prologue: (first loads back + slack computed) | (own records, nodes and lines staged), ticks after [8]
            crow[15] = ((wall_prebar - wall0) << 32) | ((wall_slack - wall0) & 0xffffffffull);
        }
    }
}

template <class V, bool COUNT>
__global__ __launch_bounds__(64 * WPB) __attribute__((amdgpu_waves_per_eu(6, 8))) void cull_scan_kernel(
    const float *__restrict__ ptri1, const float *__restrict__ ptri2, const float4 *__restrict__ p0s1,
    const float4 *__restrict__ p0s2, const int32_t *__restrict__ idx1, const int32_t *__restrict__ idx2,
    const float4 *__restrict__ tree1, const float4 *__restrict__ tree2, const float *__restrict__ line,
    int32_t *__restrict__ count1, int32_t *__restrict__ hit1, int32_t *__restrict__ count2,
    int32_t *__restrict__ hit2, int32_t *__restrict__ status, uint32_t *pmax,
    const float *__restrict__ del1, const float *__restrict__ del2, const float2 *__restrict__ lmax,
    const float *__restrict__ apart, const float *__restrict__ aflag, int nblk_apart, int B,
    int N, int M, int L, int spw, unsigned long long *__restrict__ counters, long long counter_rows, int Bt,
    const int32_t *__restrict__ cnt1, const int32_t *__restrict__ cnt2, const int32_t *__restrict__ nlines) {
    __shared__ CullLds<V> lds_;
    ScanArgs a;
    a.ptri1 = ptri1; a.ptri2 = ptri2; a.p0s1 = p0s1; a.p0s2 = p0s2; a.idx1 = idx1; a.idx2 = idx2; a.tree1 = tree1; a.tree2 = tree2;
    a.line = line; a.count1 = count1; a.hit1 = hit1; a.count2 = count2; a.hit2 = hit2; a.status = status; a.pmax = pmax;
    a.del1 = del1; a.del2 = del2; a.lmax = lmax; a.apart = apart; a.aflag = aflag;
    a.nblk_apart = nblk_apart; a.B = B; a.N = N; a.M = M; a.L = L; a.spw = spw; a.Bt = Bt;
    a.counters = counters; a.counter_rows = counter_rows; a.cnt1 = cnt1; a.cnt2 = cnt2; a.nlines = nlines;
    cull_scan_body<V, COUNT>(lds_, a, (int)blockIdx.x, (int)blockIdx.y, (int)blockIdx.z, (int)gridDim.x, (int)gridDim.y);
}

// ---------------------------------------------------------------------------------------
// The culled scan AND the Chamfer walk of the same evaluation in ONE launch (round 4b; rrl_ws.h RrlChamRider, rrl_demo_epoch).
// The walk (rrl_chamfer_from_loss: nearest neighbours between the moved source's and the target's first points through
// the sorted records and sphere trees the records launch just left) depends on that launch only -- not on the scan -- but
// consecutive launches of a stream never overlap on this stack (hipExtAnyOrderLaunch is ignored on gfx9, event edges
// between streams cost tens of microseconds: profiles/r04_experiments.txt 4, 12), so the only way to run two independent
// 512-lane kernels side by side is to issue them as one grid: workgroups [0, ncham) walk (the long ones start first),
// the others scan.  Same bodies, same results as the two launches; the LDS of the two is overlaid.  The walk takes
// max |P|^2 of its target from the partial rows (pm1 == NULL): PMAX is being rebuilt by this launch's scan.
// ---------------------------------------------------------------------------------------
struct ChamKArgs {
    unsigned long long *best_x, *best_y;
    double *partial, *gpart;
    float *value;
    double denom;
    ChamTick tick;
    int gx, gy;
};
static_assert(NWV == WPB, "the walk and the scan share one launch: the same 512-lane workgroups");

template <class V>
__global__ __launch_bounds__(64 * WPB) __attribute__((amdgpu_waves_per_eu(4, 8))) void cull_scan_chamfer_kernel(
    const CullKArgs a, const ChamKArgs c) {
    __shared__ union {
        CullLds<V> scan;
        ChamLds walk;
    } lds_;
    const int ncham = c.gx * c.gy, lin = (int)blockIdx.x;
    if (lin < ncham) {  // uniform per workgroup
        chamfer_tree_body<false, true>(lds_.walk, a.p0s1, a.p0s2, a.tree1, a.tree2, a.aflag, a.nblk_apart, c.best_x, c.best_y,
                                       c.partial, a.B, a.N, a.M, nullptr, 0, a.idx1, a.idx2, nullptr, nullptr, c.tick, c.gpart,
                                       c.value, c.denom, lin % c.gx, lin / c.gx, c.gx, c.gy, a.aflag_tar);
        return;
    }
    const int l2 = lin - ncham, bx = l2 % a.gx, r = l2 / a.gx;
    // (no counters, no per-sample counts: a riding walk excludes both, rrl_plan)
    ScanArgs s;  // (member by member: a block copy of the kernel argument moves this kernel's scalar loads)
    s.ptri1 = a.ptri1; s.ptri2 = a.ptri2; s.p0s1 = a.p0s1; s.p0s2 = a.p0s2; s.idx1 = a.idx1; s.idx2 = a.idx2; s.tree1 = a.tree1; s.tree2 = a.tree2;
    s.line = a.line; s.count1 = a.count1; s.hit1 = a.hit1; s.count2 = a.count2; s.hit2 = a.hit2; s.status = a.status; s.pmax = a.pmax;
    s.del1 = a.del1; s.del2 = a.del2; s.lmax = a.lmax; s.apart = a.apart; s.aflag = a.aflag;
    s.nblk_apart = a.nblk_apart; s.B = a.B; s.N = a.N; s.M = a.M; s.L = a.L; s.spw = a.spw; s.Bt = a.Bt;
    cull_scan_body<V, false>(lds_.scan, s, bx, r % a.gy, r / a.gy, a.gx, a.gy);
}

// ---------------------------------------------------------------------------------------
// The CHAINED step's build + scan in ONE launch (round 6; include/rrl.h RRL_F_CHAIN / RRL_F_CHAINED).
// With a kept target the 640 target-cloud workgroups of the C2 scan need nothing the records launch produces (the reference's
// two scans are independent, code/loss.py:181-184) -- only cleared hit counts, which the previous chained step left behind
// (the per-line stage zeroes them behind its own read).  So the source's records body runs in the LEADING planes of a grid
// (sample, line tile, plane), the target cloud's slices follow, the source cloud's come last, and a source-cloud workgroup
// waits for its sample's ready word (CHAIN[b][0] = records pieces of sample b that have published).  Dispatch goes plane by
// plane, so the records workgroups are resident before any waiter and the source workgroups of a chip-filling grid start a
// generation after the records are out; neither is relied upon for the RESULT.  The hand-off is R1 of
// cdna_hip_programming.md Guideline 16, valid for any workgroup -> XCD placement: the payload the scan reads (PTRI rows,
// (P0, thr2), tree nodes, NaN reach, partial rows) leaves by WRITE-THROUGH (sc1) stores, every storing wave drains, barrier,
// ONE relaxed agent-scope ticket; the consumer requests its lines, one lane polls the ticket relaxed, barrier, and the
// source cloud's rows are read by sc1 loads (past the CU's L1) -- no fence on either side (an agent release per records
// workgroup + an acquire per source workgroup measured +2.7 us on a 29 us launch, profiles/r06_experiments.txt 1).  The wait is
// bounded (RRL_CHAIN_SPIN polls; a time-out is counted in CHAIN[b][3] and makes the sample's loss NaN instead of hanging the
// launch); the records workgroups never wait.  The per-call state that NO scan workgroup touches (NSEL, the reduce's state, the
// accumulators, the gradient target) is cleared by the records workgroups after they have published; COUNT1 / COUNT2 /
// CHAIN arrive cleared.  The scan's NaN flag / fallback count of this launch are per sample (CHAIN[b][1], [2]): STATUS could not
// be cleared under the target workgroups' feet.
// ---------------------------------------------------------------------------------------
// (the head: what a scan workgroup needs for its place in the grid, its line loads and -- one round of scalar loads at kernel
//  entry -- its record loads; the first members are the candidates for kernel-argument preload)
struct ChainKArgs {
    int zrec;              // grid planes [0, zrec): the records pieces
    int z2;                // grid planes [zrec, zrec + z2): the target cloud's slices; the source cloud's follow
    int B, N, M, L, spw, nblk_apart;
    const float *line;
    uint32_t *chain;       // CHAIN words [B][RRL_CHAIN_WORDS]
    const float *apart;
    const float4 *p0s1, *p0s2, *tree1, *tree2;
    uint32_t *pmax;
    int nrec_b;            // records pieces (workgroups) per sample: the ready count a source workgroup waits for
    int gy;                // line tiles: the grid's second extent (gridDim is a hidden argument)
    unsigned spin_limit;   // polls before a waiter gives up
    int exp;               // (experimental builds, -DRRL_CHAIN_EXP: RRL_CHAIN_EXP = 1 nobody waits | 2 the records workgroups return at once
                           //  -- timing only, results invalid)
};

// Grid (B, tiles, zrec + z2 + z1), sample fastest (with B % 8 == 0 everything of sample b runs on XCD b % 8): planes
// [0, zrec) hold the records pieces (piece z * tiles + y of sample x; the surplus exits), planes [zrec, zrec + z2) the target
// cloud's slices, the rest the source cloud's -- dispatch goes plane by plane, so the order is records, target, source,
// and a workgroup's place needs no division.
template <class V>
__global__ __launch_bounds__(64 * WPB) __attribute__((amdgpu_waves_per_eu(6, 8))) void cull_scan_build_kernel(
    const ChainKArgs ch, const float *__restrict__ ptri1, const float *__restrict__ ptri2,
    const int32_t *__restrict__ idx1, const int32_t *__restrict__ idx2, int32_t *__restrict__ count1,
    int32_t *__restrict__ hit1, int32_t *__restrict__ count2, int32_t *__restrict__ hit2,
    const float *__restrict__ del1, const float *__restrict__ del2, const BuildArgs bld,
    const int32_t *__restrict__ order1) {
    __shared__ union {
        CullLds<V> scan;
        float red[WPB][8];
    } lds_;
    asm volatile("" ::"s"(ch.zrec), "s"(ch.z2), "s"(ch.B), "s"(ch.N), "s"(ch.M), "s"(ch.L), "s"(ch.spw), "s"(ch.nblk_apart),
                 "s"(ch.line), "s"(ch.chain), "s"(ch.apart), "s"(ch.p0s1), "s"(ch.p0s2), "s"(ch.tree1), "s"(ch.tree2), "s"(ch.pmax),
                 "s"(ch.nrec_b), "s"(ch.gy), "s"(ch.spin_limit));
    const int B = ch.B;
    const int b = (int)blockIdx.x, by = (int)blockIdx.y, z = (int)blockIdx.z;
    STAMPR(0);
    if (z < ch.zrec) {  // uniform per workgroup: one 512-lane piece of the source's records (+ tree refit, partial rows)
        RecPlace pl;
        pl.cloud = 0; pl.b = b; pl.bxr = z * ch.gy + by; pl.lch = -1;
        if (pl.bxr >= ch.nrec_b) return;
#ifdef RRL_CHAIN_EXP
        if (ch.exp & 2) return;
#endif
        RecLate late;
        records_sorted_body<true>(bld, order1, nullptr, pl, lds_.red, &late);
#ifdef RRL_NO_LATE  // (A/B: the moved rows and index entries stored BEFORE the drain, as the plain records kernel does)
        rec_late_stores(bld, pl, late);
#endif
        STAMPR(1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave drains ...
        __syncthreads();
        STAMPR(2);
        if (threadIdx.x == 0)  // ... then ONE lane publishes: the payload went out write-through, so a relaxed ticket is all
            __hip_atomic_fetch_add(&ch.chain[RRL_CHAIN_WORDS * b + RRL_CHAIN_READY], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (threadIdx.x < 64) STAMPR(3);
        // what nobody in this launch waits for: the moved rows (TRI1) and index entries, then the clearing
#ifndef RRL_NO_LATE
        rec_late_stores(bld, pl, late);
#endif
        build_clear_state(bld, ((size_t)(pl.bxr * B + b)) * (64 * WPB) + threadIdx.x, (size_t)ch.nrec_b * B * (64 * WPB));
        STAMPR(4);
        return;
    }
    const int cloud = z < ch.zrec + ch.z2 ? 1 : 0, bz = z - ch.zrec - (cloud ? 0 : ch.z2);
    // the source's records are written by THIS launch: its workgroups wait for the sample's ready word -- after requesting their
    // lines (cull_scan_body) -- and then read the records by sc1 loads
    auto wait_ready = [&]() {
#ifdef RRL_CHAIN_EXP
        if (cloud == 0 && !(ch.exp & 1)) {
#else
        if (cloud == 0) {  // the source's records of THIS launch: wait for the sample's ready word (its records are then read by sc1 loads)
#endif
            if (threadIdx.x == 0) {
                const uint32_t *rdy = ch.chain + RRL_CHAIN_WORDS * b + RRL_CHAIN_READY;
                bool ok = false;
                for (unsigned it = 0; it <= ch.spin_limit; ++it) {
                    if (__hip_atomic_load(rdy, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= (unsigned)ch.nrec_b) { ok = true; break; }
                    __builtin_amdgcn_s_sleep(8);
                }
                if (!ok) __hip_atomic_fetch_add(&ch.chain[RRL_CHAIN_WORDS * b + RRL_CHAIN_TIMEOUT], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            __syncthreads();
            STAMPR(5);
        }
    };
    ScanArgs a;  // (no counters, no per-sample counts, one problem: rrl_cull_scan_can_fuse declines the calls that have them)
    a.ptri1 = ptri1; a.ptri2 = ptri2; a.p0s1 = ch.p0s1; a.p0s2 = ch.p0s2; a.idx1 = idx1; a.idx2 = idx2; a.tree1 = ch.tree1; a.tree2 = ch.tree2;
    a.line = ch.line; a.count1 = count1; a.hit1 = hit1; a.count2 = count2; a.hit2 = hit2;
    a.status = (int32_t *)(ch.chain + RRL_CHAIN_WORDS * b + RRL_CHAIN_NAN);  // this launch's NaN flag / fallback count ([FALLBACK] = [NAN] + 1, rrl_ws.h) are per sample
    a.pmax = ch.pmax; a.del1 = del1; a.del2 = del2; a.lmax = nullptr; a.apart = ch.apart; a.aflag = ch.apart;
    a.nblk_apart = ch.nblk_apart; a.B = B; a.N = ch.N; a.M = ch.M; a.L = ch.L; a.spw = ch.spw; a.Bt = 0;
    cull_scan_body<V, false, true>(lds_.scan, a, cloud * B + b, by, bz, 2 * B, ch.gy, wait_ready);
    STAMPR(6);
}

// The arguments of a culled scan over o.plan.clouds clouds; tws: the workspace that holds cloud 2's records (this call's, or
// the one a riding walk takes a carried-over target from)
static CullKArgs cull_args(const RrlCall &o, const float *line, const CullGeom &g, const void *tws) {
    CullKArgs a;
    a.ptri1 = o.at<RRL_WS_PTRI1>(); a.ptri2 = o.w.at<RRL_WS_PTRI2>(tws);
    a.p0s1 = (const float4 *)o.at<RRL_WS_P0S1>(); a.p0s2 = (const float4 *)o.w.at<RRL_WS_P0S2>(tws);
    a.idx1 = o.at<RRL_WS_IDX1>(); a.idx2 = o.w.at<RRL_WS_IDX2>(tws);
    a.tree1 = (const float4 *)o.at<RRL_WS_GRP1>(); a.tree2 = (const float4 *)o.w.at<RRL_WS_GRP2>(tws);
    a.line = line;
    a.count1 = o.at<RRL_WS_COUNT1>(); a.hit1 = o.at<RRL_WS_HIT1>();
    a.count2 = o.at<RRL_WS_COUNT2>(); a.hit2 = o.at<RRL_WS_HIT2>();
    a.status = o.at<RRL_WS_STATUS>(); a.pmax = (uint32_t *)o.at<RRL_WS_PMAX>();
    a.del1 = o.at<RRL_WS_DEL1>(); a.del2 = o.at<RRL_WS_DEL2>();
    a.lmax = (const float2 *)o.at<RRL_WS_LMAX>();
    a.apart = o.prepared() ? o.at<RRL_WS_APART>() : nullptr;  // prepared build: PMAX comes from the partial rows
    a.aflag = o.at<RRL_WS_APART>(); a.aflag_tar = o.w.at<RRL_WS_APART>(tws);
    a.nblk_apart = ((o.N > o.M ? o.N : o.M) + REC_BLK - 1) / REC_BLK;
    a.B = o.B; a.N = o.N; a.M = o.M; a.L = o.L; a.spw = g.spw;
    a.gx = o.plan.clouds * o.B; a.gy = g.tiles; a.Bt = o.problems;
    return a;
}

// The launch of variant V for a geometry chosen by rrl_launch_cull_scan: (waves per workgroup, supergroups per slice,
// line tiles, slices); g.may_ride: the evaluation's Chamfer walk may be carried (full 512-lane workgroups).
template <class V>
static int launch_variant(const RrlCall &o, const float *line, const CullGeom &g) {
    const int B = o.B, N = o.N, M = o.M, clouds = o.plan.clouds, waves = g.waves, spw = g.spw, tiles = g.tiles;
    if (o.plan.fused_build) {  // the chained step: source records + target scan + source scan as ONE launch (cull_scan_build_kernel)
        if (waves != WPB || clouds != 2 || !o.prepared()) return RRL_E_ARG;
        CullKArgs a = cull_args(o, line, g, o.ws);  // (lmax is not read: the tile's own maxima; no multi-pose: rrl_cull_scan_can_fuse)
        a.status = nullptr;
        // the source's records body: the arguments of a records launch of cloud 1 alone, in 512-lane pieces; it clears what
        // no scan workgroup of this launch touches: NSEL (+ NVALS), the reduce's state, the accumulators, the gradient target
        BuildArgs bld = make_build_args(o, o.tri1_in, nullptr, 1, nullptr, false);
        bld.L = 0;
        bld.nblk_tri = (int)(((size_t)(N + SGT - 1) / SGT * SGT + 64 * WPB - 1) / (64 * WPB));
        bld.zero_base = (uint4 *)o.at<RRL_WS_NVALS>();
        bld.zero_vec4 = (o.w.off[RRL_WS_PMAX] - o.w.off[RRL_WS_NVALS]) / 16;
        bld.z2 = nullptr; bld.z2_vec4 = 0;
        bld.z5 = nullptr; bld.z5_words = 0;
        ChainKArgs ch;
        ch.B = a.B; ch.N = a.N; ch.M = a.M; ch.L = a.L; ch.spw = a.spw; ch.nblk_apart = a.nblk_apart;
        ch.line = a.line; ch.apart = a.apart; ch.p0s1 = a.p0s1; ch.p0s2 = a.p0s2; ch.tree1 = a.tree1; ch.tree2 = a.tree2;
        ch.pmax = a.pmax; ch.gy = tiles;
        ch.chain = (uint32_t *)o.at<RRL_WS_CHAIN>();
        ch.nrec_b = bld.nblk_tri;
        ch.zrec = (bld.nblk_tri + tiles - 1) / tiles;
        const int nsg1 = (N + SGT - 1) / SGT, nsg2 = (M + SGT - 1) / SGT;
        const int z1 = (nsg1 + spw - 1) / spw;  // slices per cloud: no empty workgroups
        ch.z2 = (nsg2 + spw - 1) / spw;
        ch.spin_limit = rrl_chain_spin_limit();
        ch.exp = 0;
#ifdef RRL_CHAIN_EXP
        if (const char *e = getenv("RRL_CHAIN_EXP")) ch.exp = atoi(e);
#endif
        hipLaunchKernelGGL(cull_scan_build_kernel<V>, dim3((unsigned)B, (unsigned)tiles, (unsigned)(ch.zrec + ch.z2 + z1)), dim3(64 * WPB), 0,
                           o.s, ch, a.ptri1, a.ptri2, a.idx1, a.idx2, a.count1, a.hit1, a.count2, a.hit2, a.del1, a.del2, bld,
                           o.order1);
        RRL_LAUNCH_CHECK();
        return 0;
    }
    if (g.may_ride && waves == WPB) {
        // the evaluation's Chamfer walk rides along (cull_scan_chamfer_kernel): ONE launch for both.  A carried-over target
        // (clouds == 1: only the source is scanned here) is walked in the workspace that holds its records.
        const ChamLayout C(B, N, M);
        if (o.rider->ws && o.rider->ws_bytes >= C.total && o.rider->best_x && o.rider->best_y && o.rider->value) {
            const CullKArgs a = cull_args(o, line, g, clouds == 2 ? o.ws : o.tar_ws);
            ChamKArgs c;
            char *cw = (char *)o.rider->ws;
            c.best_x = (unsigned long long *)o.rider->best_x; c.best_y = (unsigned long long *)o.rider->best_y;
            c.partial = (double *)(cw + C.partial); c.gpart = (double *)(cw + C.gpart);
            c.value = o.rider->value;
            c.denom = (double)B * (double)(N + M);
            uint32_t *mctl = (uint32_t *)o.at<RRL_WS_MCTL>();  // arrival counters of the walk's mean (rrl_chamfer_from_loss_ex)
            c.tick = cham_tick_in_mctl(mctl);
            c.gx = 2 * B; c.gy = ((N > M ? N : M) + SGT - 1) / SGT;  // patches of the larger cloud (either direction)
            const unsigned nwg = (unsigned)(c.gx * c.gy) + (unsigned)(a.gx * a.gy * g.slices);
            hipLaunchKernelGGL(cull_scan_chamfer_kernel<V>, dim3(nwg), dim3(64 * WPB), 0, o.s, a, c);
            RRL_LAUNCH_CHECK();
            o.rider->done = 1;
            return 0;
        }
    }
    const CullKArgs a = cull_args(o, line, g, o.ws);
    auto plain = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)a.gx, (unsigned)a.gy, (unsigned)g.slices), dim3(64 * waves), 0, o.s, a.ptri1, a.ptri2,
                           a.p0s1, a.p0s2, a.idx1, a.idx2, a.tree1, a.tree2, a.line, a.count1, a.hit1, a.count2, a.hit2, a.status, a.pmax,
                           a.del1, a.del2, a.lmax, a.apart, a.aflag, a.nblk_apart, a.B, a.N, a.M, a.L, a.spw, o.counters, o.counter_rows,
                           a.Bt, o.count1, o.count2, o.nlines);
    };
    if (o.counters) plain(cull_scan_kernel<V, true>);
    else plain(cull_scan_kernel<V, false>);
    RRL_LAUNCH_CHECK();
    return 0;
}
