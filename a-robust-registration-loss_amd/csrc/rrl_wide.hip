// rrl_wide.hip -- the WIDE pipeline: bucket ranges of up to 8 hits per line and cloud (1 <= s < e <= 9; include/rrl.h
// rrl_loss_forward_wide / rrl_loss_backward_wide).  The narrow stages (rrl_sparse.hip) are built around a 4 x 4 register
// tile and 16 buckets and stay exactly as they are; this file reuses only
//   * the scan, as is: records / sort / tree / scan of any mode (and prepared orders) into an ordinary loss workspace.
//     COUNT1 / COUNT2 count every hit, HIT1 / HIT2 hold the first 4 (in the order the scan found them);
//   * the per-value arithmetic: the scan's label predicate on the PTRI records (dist_sq, thr2), hit_weights, inter_point,
//     tri_coords and welsch (rrl_arith.h), the bucket weights exp(-|k-j|/2) and the 2^-40 fixed-point bucket sums.
// Stages, one launch each (DESIGN.md "Wide bucket ranges"):
//   W1 select    one lane per line: (count1, count2) inside the range -> a compact slot (SEL, KJ); every cloud of such a
//                line with more than 4 hits becomes a hit-recovery entry (REC)
//   W2 recover   one wavefront per entry: the line against ALL records of that cloud with the strict predicate; the hits
//                in ascending original index (nonzero() order).  Invariant: as many hits as the scan counted -- else
//                STATUS[0] counts the line and the host refuses the result (the culled scan equals the strict one bit
//                for bit, DESIGN 3: a mismatch is a bug, not noise)
//   W3 pair      one lane per selected line: weights and intersection points of <= 8 + 8 hits, the k x j block of D
//   W4 reduce    one workgroup per group: exact lower median (radix select on the bit patterns: D >= 0), Welsch row /
//                column minima, bucket sums in 2^-40 fixed point (order-independent: the forward is deterministic), loss
//   W5 backward  one lane per selected line: dL/dD at the first-occurrence argmin entries, scattered to the rows of
//                points1 (and points2) with float atomics
// The lines with more than 4 hits are a few percent of L; the stages touch O(selected lines) data next to the O(L (N + M))
// scan.
#include <string.h>

#include "rrl_arith.h"
#include "rrl_ws.h"

#define WIDE_HITS 8      // hits kept per line and cloud (RRL_WIDE_MAX_HITS)

static_assert(WIDE_HITS == RRL_WIDE_MAX_HITS, "include/rrl.h");

struct WideArgs {
    const float *tri1, *tri2, *line;                 // raw 36-byte rows (what the narrow per-line stage reads), lines
    const int32_t *count1, *count2, *hit1, *hit2;    // the scan's results (loss workspace)
    const float *ptri1, *ptri2;                      // the scan's records: 9 coords, thr2, thr, original index
    const int32_t *scan_status;                      // STATUS of the loss workspace ([0]: NaN seen)
    int32_t *status, *nsel, *rec, *sel;
    uint8_t *kj;
    int32_t *hs1, *hs2;
    float *w1, *w2;
    float4 *Q1, *Q2;
    float *D, *med;
    int32_t *bcnt;
    unsigned long long *bsum;
    int32_t *info;
    float *loss;
    const float *grad_loss;  // backward
    float *g1, *g2;
    int B, N, M, L, s_m, s_n, e_m, e_n, pool;
};

// ---- W1: selection.  One lane per line; one slot atomic per wavefront.
__global__ __launch_bounds__(256) void wide_select_kernel(const WideArgs a) {
    const int b = blockIdx.y, l = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    int k = 0, j = 0;
    bool sel = false;
    if (l < a.L) {
        const size_t gl = (size_t)b * a.L + l;
        k = a.count1[gl];
        j = a.count2[gl];
        sel = k >= a.s_m && k < a.e_m && j >= a.s_n && j < a.e_n;
    }
    const unsigned long long mask = __ballot(sel);
    if (mask == 0ull) return;  // uniform
    const int leader = __ffsll((long long)mask) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(&a.nsel[b], __popcll(mask));
    base = __builtin_amdgcn_readlane(base, leader);
    if (!sel) return;
    const size_t g = (size_t)b * a.L + base + __popcll(mask & ((1ull << lane) - 1ull));
    a.sel[g] = l;
    a.kj[g] = (uint8_t)(k | (j << 4));
    if (k > RRL_MAX_HITS) a.rec[atomicAdd(&a.status[1], 1)] = (int)g;
    if (j > RRL_MAX_HITS) a.rec[atomicAdd(&a.status[1], 1)] = (int)((unsigned)g | 0x80000000u);
}

// ---- W2: hit recovery.  One wavefront per (selected line, cloud with > 4 hits): 64 records per step, the scan's strict
//      predicate (scan_strict, rrl_scan.hip: the largest of the three points' dist_sq bit patterns below thr2's -- a
//      negative argument, whose sqrt is NaN, never is), hits compacted in discovery order and ranked by original index.
#define WIDE_REC_WAVES 4
__global__ __launch_bounds__(64 * WIDE_REC_WAVES) void wide_recover_kernel(const WideArgs a) {
    __shared__ int s_h[WIDE_REC_WAVES][WIDE_HITS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nrec = a.status[1];
    for (int e = blockIdx.x * WIDE_REC_WAVES + wave; e < nrec; e += gridDim.x * WIDE_REC_WAVES) {  // uniform per wavefront
        const unsigned ent = (unsigned)a.rec[e];
        const int cloud = (int)(ent >> 31);
        const size_t g = ent & 0x7fffffffu;
        const int b = (int)(g / (size_t)a.L);
        const int l = a.sel[g];
        const unsigned kjb = a.kj[g];
        const int want = cloud ? (int)(kjb >> 4) : (int)(kjb & 15u);
        const float *lp = a.line + ((size_t)b * a.L + l) * 6;
        const float ux = lp[0], uy = lp[1], uz = lp[2], ox = lp[3], oy = lp[4], oz = lp[5];
        const int n = cloud ? a.M : a.N;
        const float *pt = (cloud ? a.ptri2 : a.ptri1) + (size_t)b * n * PTRI_STRIDE;
        int cnt = 0;
        for (int t0 = 0; t0 < n; t0 += 64) {
            const int t = t0 + lane;
            bool hit = false;
            int f = 0;
            if (t < n) {
                const float4 *row = (const float4 *)(pt + (size_t)t * PTRI_STRIDE);
                const float4 r0 = row[0], r1 = row[1], r2 = row[2];
                const float x0 = dist_sq<float>(r0.x, r0.y, r0.z, ux, uy, uz, ox, oy, oz);
                const float x1 = dist_sq<float>(r0.w, r1.x, r1.y, ux, uy, uz, ox, oy, oz);
                const float x2 = dist_sq<float>(r1.z, r1.w, r2.x, ux, uy, uz, ox, oy, oz);
                const uint32_t m = max(max(f2u(x0), f2u(x1)), f2u(x2));
                hit = m < f2u(r2.y);          // slot 9: thr2
                f = __float_as_int(r2.w);     // slot 11: the original triangle index
            }
            const unsigned long long hm = __ballot(hit);
            if (hit) {
                const int pos = cnt + __popcll(hm & ((1ull << lane) - 1ull));
                if (pos < WIDE_HITS) s_h[wave][pos] = f;
            }
            cnt += __popcll(hm);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // one wavefront: its LDS traffic is in order
        const int nh = cnt < WIDE_HITS ? cnt : WIDE_HITS;
        if (lane < nh) {
            const int x = s_h[wave][lane];
            int r = 0;
            for (int u = 0; u < nh; ++u) r += s_h[wave][u] < x ? 1 : 0;  // distinct indices: the rank is the position
            (cloud ? a.hs2 : a.hs1)[g * WIDE_HITS + r] = x;
        }
        if (cnt != want && lane == 0) atomicAdd(&a.status[0], 1);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // s_h is free for the next entry
    }
}

// ---- W3: the per-line stage.  Hits of one cloud of a selected line: ascending triangle indices (from HIT when the scan
//      kept them all, else from W2), their weights and intersection points (the narrow stage's arithmetic).
__device__ __forceinline__ void wide_hits(const float *__restrict__ tb, int n, const int32_t *__restrict__ hit, int32_t *hs,
                                          float *w, float4 *Q, size_t gl, size_t g, int cnt, const float *ln,
                                          float (&q)[WIDE_HITS][3], int32_t *status) {
    int h[WIDE_HITS];
    if (cnt <= RRL_MAX_HITS) {
        const int4 r = ((const int4 *)hit)[gl];
        h[0] = 0 < cnt ? r.x : 0x7fffffff;
        h[1] = 1 < cnt ? r.y : 0x7fffffff;
        h[2] = 2 < cnt ? r.z : 0x7fffffff;
        h[3] = 3 < cnt ? r.w : 0x7fffffff;
#pragma unroll
        for (int t = RRL_MAX_HITS; t < WIDE_HITS; ++t) h[t] = 0x7fffffff;
#pragma unroll
        for (int i = 1; i < RRL_MAX_HITS; ++i)  // ascending triangle index == nonzero() order (code/loss.py:125-131)
#pragma unroll
            for (int jj = RRL_MAX_HITS - 1; jj >= i; --jj)
                if (h[jj] < h[jj - 1]) { const int x = h[jj]; h[jj] = h[jj - 1]; h[jj - 1] = x; }
    } else {
#pragma unroll
        for (int t = 0; t < WIDE_HITS; ++t) h[t] = t < cnt ? hs[g * WIDE_HITS + t] : 0x7fffffff;  // (W2: ascending)
    }
#pragma unroll
    for (int t = 0; t < WIDE_HITS; ++t) {
        q[t][0] = q[t][1] = q[t][2] = 0.0f;
        if (t < cnt) {
            int f = h[t];
            if ((unsigned)f >= (unsigned)n) { atomicAdd(&status[0], 1); f = 0; }  // (never: the lists would be inconsistent)
            float c[9], wt[3], qq[3];
            tri_coords(tb, 9, f, c);
            hit_weights(c, ln, wt);
            inter_point(c, wt, qq);
            hs[g * WIDE_HITS + t] = f;
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) w[(g * WIDE_HITS + t) * 3 + cc] = wt[cc];
            Q[g * WIDE_HITS + t] = make_float4(qq[0], qq[1], qq[2], 0.0f);
            q[t][0] = qq[0]; q[t][1] = qq[1]; q[t][2] = qq[2];
        }
    }
}

__global__ __launch_bounds__(256) void wide_pair_kernel(const WideArgs a) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.nsel[b]) return;
    const size_t g = (size_t)b * a.L + i;
    const int l = a.sel[g];
    const unsigned kjb = a.kj[g];
    const int k = (int)(kjb & 15u), j = (int)(kjb >> 4);
    const size_t gl = (size_t)b * a.L + l;
    float ln[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) ln[c] = a.line[gl * 6 + c];
    float q1[WIDE_HITS][3], q2[WIDE_HITS][3];
    wide_hits(a.tri1 + (size_t)b * a.N * 9, a.N, a.hit1, a.hs1, a.w1, a.Q1, gl, g, k, ln, q1, a.status);
    wide_hits(a.tri2 + (size_t)b * a.M * 9, a.M, a.hit2, a.hs2, a.w2, a.Q2, gl, g, j, ln, q2, a.status);
    float *Dl = a.D + g * (WIDE_HITS * WIDE_HITS);
#pragma unroll
    for (int p = 0; p < WIDE_HITS; ++p)
#pragma unroll
        for (int r = 0; r < WIDE_HITS; ++r)
            if (p < k && r < j) {  // D[p][r] = sum_c (q1 - q2)^2, code/loss.py:38-52 (the narrow stage's expression)
                const float dx = q1[p][0] - q2[r][0], dy = q1[p][1] - q2[r][1], dz = q1[p][2] - q2[r][2];
                float sq = dx * dx;
                sq = sq + dy * dy;
                sq = sq + dz * dz;
                Dl[p * WIDE_HITS + r] = sq;
            }
}

// ---- W4: median + Welsch reduce + loss, one 1024-lane workgroup per group (a sample, or with pool all samples and the
//      LAST sample's median: SURVEY Q2).  The median is the element of rank (n - 1) / 2 (torch.median), selected MSB first
//      on the bit patterns (D >= 0: unsigned order == float order) in three passes of 11 + 11 + 10 bits over the group's
//      k x j blocks; any n up to L * 64.
__global__ __launch_bounds__(1024) void wide_reduce_kernel(const WideArgs a) {
    __shared__ unsigned s_hist[2048];
    __shared__ unsigned s_wtot[16];
    __shared__ unsigned s_prefix[3], s_rank[4];  // one slot per pass: no barrier between read and rewrite
    __shared__ unsigned s_n;
    __shared__ unsigned long long s_sum[2 * WIDE_HITS * WIDE_HITS];
    __shared__ int s_cnt[WIDE_HITS * WIDE_HITS];
    __shared__ int s_bad;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int gi = blockIdx.x;
    const int bm = a.pool ? a.B - 1 : gi, b0 = a.pool ? 0 : gi, b1 = a.pool ? a.B : gi + 1;
    const int st0 = a.scan_status[0];
    if (tid < 2 * WIDE_HITS * WIDE_HITS) s_sum[tid] = 0ull;
    if (tid < WIDE_HITS * WIDE_HITS) s_cnt[tid] = 0;
    if (tid == 0) { s_n = 0; s_bad = 0; }
    __syncthreads();
    const int ns = a.nsel[bm];
    const size_t gb = (size_t)bm * a.L;
    {
        unsigned mine = 0;
        for (int i = tid; i < ns; i += 1024) {
            const unsigned c = a.kj[gb + i];
            mine += (c & 15u) * (c >> 4);
        }
        const unsigned tot = (unsigned)wave_sum_i((int)mine);
        if (lane == 0 && tot) atomicAdd(&s_n, tot);
    }
    __syncthreads();
    const unsigned n = s_n;
    if (tid == 0) s_rank[0] = n ? (n - 1) / 2 : 0;
    unsigned prefix = 0;
    for (int pass = 0; pass < 3 && n > 0; ++pass) {  // (uniform)
        const int sh = pass == 0 ? 21 : (pass == 1 ? 10 : 0);
        const int width = pass == 2 ? 10 : 11;
        const unsigned dmask = (1u << width) - 1u;
        const int hi = sh + width;  // bits >= hi must equal the prefix (none on the first pass)
        s_hist[tid] = 0;
        s_hist[tid + 1024] = 0;
        __syncthreads();
        for (int i = tid; i < ns; i += 1024) {
            const unsigned c = a.kj[gb + i];
            const int k = (int)(c & 15u), j = (int)(c >> 4);
            const float *Dl = a.D + (gb + i) * (WIDE_HITS * WIDE_HITS);
            for (int p = 0; p < k; ++p)
                for (int r = 0; r < j; ++r) {
                    const unsigned x = __float_as_uint(Dl[p * WIDE_HITS + r]);
                    if (hi >= 32 || ((x ^ prefix) >> hi) == 0u) atomicAdd(&s_hist[(x >> sh) & dmask], 1u);
                }
        }
        __syncthreads();
        const unsigned h0 = s_hist[2 * tid], h1 = s_hist[2 * tid + 1];
        const unsigned incl = (unsigned)wave_incl_scan((int)(h0 + h1));
        if (lane == 63) s_wtot[wave] = incl;
        __syncthreads();
        unsigned base = 0;
        for (int w = 0; w < wave; ++w) base += s_wtot[w];
        const unsigned excl = base + incl - (h0 + h1), r = s_rank[pass];
        if (r >= excl && r < excl + h0 + h1) {  // exactly one lane
            const unsigned second = r >= excl + h0 ? 1u : 0u;
            s_prefix[pass] = prefix | ((2u * tid + second) << sh);
            s_rank[pass + 1] = r - excl - (second ? h0 : 0u);
        }
        __syncthreads();
        prefix = s_prefix[pass];
    }
    const float med = n ? __uint_as_float(prefix) : 0.0f;

    // Welsch + symmetric min per selected line (the narrow reduce's accumulate(): Welsch1 is non-decreasing, so the
    // Welsch term of a row / column minimum is the minimum of the terms), bucket sums in 2^-40 fixed point
    for (int bb = b0; bb < b1; ++bb) {
        const int nsb = a.nsel[bb];
        const size_t gbb = (size_t)bb * a.L;
        for (int i = tid; i < nsb; i += 1024) {
            const unsigned c = a.kj[gbb + i];
            const int k = (int)(c & 15u), j = (int)(c >> 4);
            const float *Dl = a.D + (gbb + i) * (WIDE_HITS * WIDE_HITS);
            float row = 0.0f, col = 0.0f;
            for (int p = 0; p < k; ++p) {
                float mn = Dl[p * WIDE_HITS];
                for (int r = 1; r < j; ++r) mn = fminf(mn, Dl[p * WIDE_HITS + r]);
                row += welsch(mn, med);
            }
            for (int r = 0; r < j; ++r) {
                float mn = Dl[r];
                for (int p = 1; p < k; ++p) mn = fminf(mn, Dl[p * WIDE_HITS + r]);
                col += welsch(mn, med);
            }
            // Wl in [0, 1], <= 8 terms; a NaN term (median 0: code/loss.py:20-21 gives NaN too) cannot be carried by the
            // fixed-point sums: flag it
            if (!(row <= (float)WIDE_HITS) || !(col <= (float)WIDE_HITS)) { atomicOr(&s_bad, 1); row = col = 0.0f; }
            const int bi = (k - 1) * WIDE_HITS + (j - 1);
            atomicAdd(&s_sum[bi * 2 + 0], (unsigned long long)((double)row * (double)(1ll << FIX_SHIFT) + 0.5));
            atomicAdd(&s_sum[bi * 2 + 1], (unsigned long long)((double)col * (double)(1ll << FIX_SHIFT) + 0.5));
            atomicAdd(&s_cnt[bi], 1);
        }
    }
    __syncthreads();
    if (wave != 0) return;
    // loss = ( sum_{non-empty (k,j), k-major} exp(-|k-j|/2) (mean_row + mean_col) ) / C, one lane per bucket (the narrow
    // bucket_final's arithmetic: an empty bucket's term is +0 and changes no bit of the k-major sum)
    const int S = s_cnt[lane];
    const int k = lane / WIDE_HITS + 1, j = lane % WIDE_HITS + 1;
    const unsigned long long srow = s_sum[2 * lane], scol = s_sum[2 * lane + 1];
    a.bcnt[(size_t)gi * 64 + lane] = S;
    a.bsum[((size_t)gi * 64 + lane) * 2 + 0] = srow;
    a.bsum[((size_t)gi * 64 + lane) * 2 + 1] = scol;
    const bool in = S > 0 && k >= a.s_m && k < a.e_m && j >= a.s_n && j < a.e_n;
    float term = 0.0f;
    if (in) {
        const double sc = 1.0 / (double)(1ll << FIX_SHIFT);
        const float mrow = (float)((double)srow * sc / ((double)S * k));
        const float mcol = (float)((double)scol * sc / ((double)S * j));
        const float wkj = expf(-0.5f * (float)abs(k - j));  // code/loss.py:215
        term = wkj * (mrow + mcol);
    }
    const int C = __popcll(__ballot(in));
    const int nselected = wave_sum_i(in ? S : 0);
    float acc = 0.0f;
#pragma unroll
    for (int bi = 0; bi < 64; ++bi) acc = acc + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(term), bi));
    if (lane == 0) {
        const float lv = s_bad ? __builtin_nanf("") : (C ? acc / (float)C : 0.0f);  // code/loss.py:230
        a.med[gi] = med;
        a.loss[gi] = lv;
        a.info[gi * 4 + 0] = C;
        a.info[gi * 4 + 1] = nselected;
        a.info[gi * 4 + 2] = (int)n;
        a.info[gi * 4 + 3] = st0;
    }
}

// ---- W5: backward.  dL/dD[p][r] = gout w_kj / C exp(-D / (2 med)) / (2 med) ([r = argmin row p] / (S k) +
//      [p = argmin column r] / (S j)), dL/dq1[p] = sum_r 2 (q1_p - q2_r) dL/dD = -dL/dq2 summed the other way,
//      dL/dP[f][kk] += w_kk / 3 dL/dq.  The narrow scatter's expressions and accumulation orders (rrl_stage_bwd.h
//      bwd_scatter_math: row p over r ascending, column r over p ascending); only the order of the float atomics differs.
__global__ __launch_bounds__(256) void wide_bwd_kernel(const WideArgs a) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.nsel[b]) return;
    const int gi = a.pool ? 0 : b;
    const int C = a.info[gi * 4];
    if (C <= 0) return;
    const float m = a.med[gi], gl_in = a.grad_loss[gi];
    const size_t g = (size_t)b * a.L + i;
    const unsigned c = a.kj[g];
    const int k = (int)(c & 15u), j = (int)(c >> 4);
    const int S = a.bcnt[(size_t)gi * 64 + (k - 1) * WIDE_HITS + (j - 1)];
    const float *Dl = a.D + g * (WIDE_HITS * WIDE_HITS);
    int argb[WIDE_HITS], arga[WIDE_HITS];  // first-occurrence argmin of the Welsch values (torch.min)
#pragma unroll
    for (int p = 0; p < WIDE_HITS; ++p) {
        argb[p] = 0;
        if (p < k) {
            float best = welsch(Dl[p * WIDE_HITS], m);
#pragma unroll
            for (int r = 1; r < WIDE_HITS; ++r)
                if (r < j) {
                    const float wv = welsch(Dl[p * WIDE_HITS + r], m);
                    if (wv < best) { best = wv; argb[p] = r; }
                }
        }
    }
#pragma unroll
    for (int r = 0; r < WIDE_HITS; ++r) {
        arga[r] = 0;
        if (r < j) {
            float best = welsch(Dl[r], m);
#pragma unroll
            for (int p = 1; p < WIDE_HITS; ++p)
                if (p < k) {
                    const float wv = welsch(Dl[p * WIDE_HITS + r], m);
                    if (wv < best) { best = wv; arga[r] = p; }
                }
        }
    }
    float4 q1[WIDE_HITS], q2[WIDE_HITS];
#pragma unroll
    for (int t = 0; t < WIDE_HITS; ++t) {
        q1[t] = t < k ? a.Q1[g * WIDE_HITS + t] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        q2[t] = t < j ? a.Q2[g * WIDE_HITS + t] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    const float wkj = expf(-0.5f * (float)abs(k - j));
    const float scale = gl_in * wkj / (float)C;
    const float inv_row = 1.0f / ((float)S * (float)k), inv_col = 1.0f / ((float)S * (float)j);
    float gq1[WIDE_HITS][3], gq2[WIDE_HITS][3];
#pragma unroll
    for (int t = 0; t < WIDE_HITS; ++t) gq1[t][0] = gq1[t][1] = gq1[t][2] = gq2[t][0] = gq2[t][1] = gq2[t][2] = 0.0f;
#pragma unroll
    for (int p = 0; p < WIDE_HITS; ++p)
#pragma unroll
        for (int r = 0; r < WIDE_HITS; ++r) {
            if (!(p < k && r < j)) continue;
            float sw = 0.0f;
            if (argb[p] == r) sw += inv_row;
            if (arga[r] == p) sw += inv_col;
            if (sw == 0.0f) continue;
            const float ex = expf(-(Dl[p * WIDE_HITS + r] / m) / 2.0f);  // dWl/dD = exp(-D/(2 med)) / (2 med)
            const float gD = scale * sw * ex / (2.0f * m);
            gq1[p][0] += 2.0f * (q1[p].x - q2[r].x) * gD;
            gq1[p][1] += 2.0f * (q1[p].y - q2[r].y) * gD;
            gq1[p][2] += 2.0f * (q1[p].z - q2[r].z) * gD;
            gq2[r][0] += 2.0f * (q2[r].x - q1[p].x) * gD;
            gq2[r][1] += 2.0f * (q2[r].y - q1[p].y) * gD;
            gq2[r][2] += 2.0f * (q2[r].z - q1[p].z) * gD;
        }
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        float *gb = side ? a.g2 : a.g1;
        if (!gb) continue;
        const int cnt = side ? j : k;
        const int32_t *hs = side ? a.hs2 : a.hs1;
        const float *w = side ? a.w2 : a.w1;
        gb += (size_t)b * (side ? a.M : a.N) * 9;
#pragma unroll
        for (int t = 0; t < WIDE_HITS; ++t) {
            if (t >= cnt) continue;
            const int f = hs[g * WIDE_HITS + t];
#pragma unroll
            for (int kk = 0; kk < 3; ++kk) {
                const float wk = w[(g * WIDE_HITS + t) * 3 + kk] / 3.0f;  // q = mean_k(w_k P_k)
#pragma unroll
                for (int cc = 0; cc < 3; ++cc) atomicAdd(&gb[(size_t)f * 9 + 3 * kk + cc], wk * (side ? gq2[t][cc] : gq1[t][cc]));
            }
        }
    }
}

// ---------------------------------------------------------------------------------------
// host entries
// ---------------------------------------------------------------------------------------
extern "C" size_t rrl_wide_workspace_bytes(int B, int N, int M, int L) { return WwLayout(B, N, M, L).total; }

extern "C" int rrl_wide_workspace_layout(int B, int N, int M, int L, size_t *offsets) {
    if (!offsets || B < 0 || N < 0 || M < 0 || L < 0) return RRL_E_ARG;
    WwLayout w(B, N, M, L);
    for (int i = 0; i < RRL_WW_FIELDS; ++i) offsets[i] = w.off[i];
    return 0;
}

// The fields of the wide workspace; with a record (the forward) also the scan's results in the narrow one, the range and
// the loss -- the backward (o == NULL) reads none of them
static WideArgs wide_args(void *wws, const WwLayout &v, int B, int N, int M, int L, int pool, const RrlCall *o = nullptr,
                          float *loss = nullptr) {
    WideArgs a;
    memset(&a, 0, sizeof a);
    a.status = v.at<RRL_WW_STATUS>(wws); a.nsel = v.at<RRL_WW_NSEL>(wws);
    a.rec = v.at<RRL_WW_REC>(wws); a.sel = v.at<RRL_WW_SEL>(wws); a.kj = v.at<RRL_WW_KJ>(wws);
    a.hs1 = v.at<RRL_WW_HS1>(wws); a.hs2 = v.at<RRL_WW_HS2>(wws);
    a.w1 = v.at<RRL_WW_W1>(wws); a.w2 = v.at<RRL_WW_W2>(wws);
    a.Q1 = (float4 *)v.at<RRL_WW_Q1>(wws); a.Q2 = (float4 *)v.at<RRL_WW_Q2>(wws);
    a.D = v.at<RRL_WW_D>(wws); a.med = v.at<RRL_WW_MED>(wws);
    a.bcnt = v.at<RRL_WW_BCNT>(wws); a.bsum = (unsigned long long *)v.at<RRL_WW_BSUM>(wws);
    a.info = v.at<RRL_WW_INFO>(wws);
    a.B = B; a.N = N; a.M = M; a.L = L; a.pool = pool ? 1 : 0;
    if (o) {
        a.count1 = o->at<RRL_WS_COUNT1>(); a.count2 = o->at<RRL_WS_COUNT2>();
        a.hit1 = o->at<RRL_WS_HIT1>(); a.hit2 = o->at<RRL_WS_HIT2>();
        a.ptri1 = o->at<RRL_WS_PTRI1>(); a.ptri2 = o->at<RRL_WS_PTRI2>();
        a.scan_status = o->at<RRL_WS_STATUS>();
        a.loss = loss;
        a.s_m = o->s_m; a.s_n = o->s_n; a.e_m = o->e_m; a.e_n = o->e_n;
    }
    return a;
}

// The wide entries refuse in the narrow ones' order (include/rrl.h "Refusals") with their own limits: RRL_E_ARG, then
// RRL_E_RANGE (1 .. RRL_WIDE_MAX_HITS), then RRL_E_WS (either workspace)
extern "C" int rrl_loss_forward_wide(const float *tri1, const float *tri2, const float *line, void *ws, size_t ws_bytes,
                                     void *wws, size_t wws_bytes, float *loss, int B, int N, int M, int L, int s_m,
                                     int s_n, int e_m, int e_n, int pool, int mode, int chunk, const rrl_opts *opts,
                                     void *stream) {
    if (!tri1 || !tri2 || !line || !ws || !wws || !loss) return RRL_E_ARG;
    if (B < 0 || N < 0 || M < 0 || L < 0 || L >= (1 << 24) || (long long)B * L >= (1ll << 31) || mode < RRL_SCAN_STRICT ||
        mode > RRL_SCAN_CULL || chunk < 0)
        return RRL_E_ARG;
    // the scan, as the narrow forward runs it (rrl_sparse.hip loss_forward_impl): prepared orders and the scan knobs of the
    // options are honoured; target carry-over, chains, riders, multi-pose and the payload are not (narrow-only features)
    RrlCall o = rrl_begin_call(opts, B, N, M, L, ws, ws_bytes, stream);
    o.set(s_m, s_n, e_m, e_n, pool, mode, chunk);
    if (o.ragged()) return RRL_E_ARG;  // (rrl_opts.count1 / count2 / nlines: the narrow entries only)
    if (s_m < 1 || s_n < 1 || e_m > RRL_WIDE_MAX_HITS + 1 || e_n > RRL_WIDE_MAX_HITS + 1) return RRL_E_RANGE;
    const WwLayout v(B, N, M, L);
    if (ws_bytes < o.w.total || wws_bytes < v.total) return RRL_E_WS;
    if (B == 0) return 0;
    hipStream_t s = o.s;
    const int G = pool ? 1 : B;
    WideArgs a = wide_args(wws, v, B, N, M, L, pool, &o, loss);
    a.tri1 = tri1; a.tri2 = tri2; a.line = line;
    int rc;
    if (L == 0) {  // no line: no bucket (INFO, loss zero)
        if ((rc = rrl_fill(a.info, 0u, sizeof(int32_t) * 4 * (size_t)G, s))) return rc;
        return rrl_fill(loss, 0u, sizeof(float) * (size_t)G, s);
    }
    o.flags = 0;
    o.problems = 0;
    o.rider = nullptr;
    o.payload = nullptr;
    o.chain_left = nullptr;
    const bool sorted = rrl_sorted_layout(N, M);
    if (o.prepared() && (mode != RRL_SCAN_CULL || !sorted || !o.order2)) o.order1 = o.order2 = nullptr;
    o.tri1_in = tri1;
    // (no rrl_plan: what the build and the scan read of it)
    o.plan.scan_mode = mode == RRL_SCAN_CULL && !sorted ? RRL_SCAN_AUTO : mode;
    o.plan.clouds = o.plan.build_clouds = 2;
    o.plan.lmax_ready = sorted && (M > N ? M : N) > 0;
    {
        RrlRange r("K1' records + sort + tree");
        if ((rc = rrl_tri_prepare_clouds(o, tri1, tri2, line))) return rc;
    }
    {
        RrlRange r("K1 line<->triangle scan");
        if ((rc = rrl_line_tri_scan_clouds(o, line))) return rc;
    }
    RrlRange r("W1..W4 wide stages");
    if ((rc = rrl_fill(wws, 0u, v.zero_bytes, s))) return rc;  // STATUS, NSEL
    const dim3 lines((unsigned)((L + 255) / 256), (unsigned)B);
    hipLaunchKernelGGL(wide_select_kernel, lines, dim3(256), 0, s, a);
    RRL_LAUNCH_CHECK();
    const long ents = 2l * B * L;  // an upper bound of the recovery entries (their number is on the device)
    long rg = (ents + WIDE_REC_WAVES - 1) / WIDE_REC_WAVES;
    if (rg > 2048) rg = 2048;
    hipLaunchKernelGGL(wide_recover_kernel, dim3((unsigned)rg), dim3(64 * WIDE_REC_WAVES), 0, s, a);
    RRL_LAUNCH_CHECK();
    hipLaunchKernelGGL(wide_pair_kernel, lines, dim3(256), 0, s, a);
    RRL_LAUNCH_CHECK();
    hipLaunchKernelGGL(wide_reduce_kernel, dim3((unsigned)G), dim3(1024), 0, s, a);
    RRL_LAUNCH_CHECK();
    return 0;
}

extern "C" int rrl_loss_backward_wide(const void *wws, size_t wws_bytes, const float *grad_loss, float *grad_tri1,
                                      float *grad_tri2, int B, int N, int M, int L, int pool, void *stream) {
    if (!wws || !grad_loss || !grad_tri1) return RRL_E_ARG;
    if (B < 0 || N < 0 || M < 0 || L < 0 || L >= (1 << 24) || (long long)B * L >= (1ll << 31)) return RRL_E_ARG;
    const WwLayout v(B, N, M, L);
    if (wws_bytes < v.total) return RRL_E_WS;
    hipStream_t s = (hipStream_t)stream;
    int rc;
    if ((rc = rrl_fill(grad_tri1, 0u, sizeof(float) * 9 * (size_t)B * N, s))) return rc;
    if (grad_tri2 && (rc = rrl_fill(grad_tri2, 0u, sizeof(float) * 9 * (size_t)B * M, s))) return rc;
    if (B == 0 || L == 0) return 0;
    WideArgs a = wide_args(const_cast<void *>(wws), v, B, N, M, L, pool);
    a.grad_loss = grad_loss;
    a.g1 = grad_tri1;
    a.g2 = grad_tri2;
    hipLaunchKernelGGL(wide_bwd_kernel, dim3((unsigned)((L + 255) / 256), (unsigned)B), dim3(256), 0, s, a);
    RRL_LAUNCH_CHECK();
    return 0;
}
