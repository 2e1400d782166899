// rrl_stage_bwd.h -- K5 backward variants: loss_bwd_kernel (scatter to points; fixed-point deterministic mode), loss_bwd_rt_kernel (to dR, dt), the single-tile kernels that carry them
// This header DEFINES kernels: it is included by rrl_sparse.hip only (one translation unit holds every stage behind the scan).
#pragma once
#include "rrl_stage_args.h"
#include "rrl_stamps.h"
#include "rrl_sampler.h"       // the sampler's write pass as a device function: bwd_write_kernel carries it
#include "rrl_stage_pair.h"    // pair_body, wave_scatter_rows, xcd_sample_of
#include "rrl_stage_reduce.h"  // reduce_body, tiled_payload
// ---------------------------------------------------------------------------------------
// K5 backward.  dL/dD[a][b] = gout * w_kj / C * exp(-D/(2 med)) / (2 med)
//                              * ( [b = argmin_b(a)] / (S k) + [a = argmin_a(b)] / (S j) )
// dL/dq1[a] = sum_b 2 (q1_a - q2_b) dL/dD;  dL/dP1[f_a][kk] += w_kk / 3 * dL/dq1[a];
// weights, median and labels carry no gradient (code/loss.py:112, 224).
// ---------------------------------------------------------------------------------------
// Grid (round 5): (line tiles, samples, BWDS_SUBS) over the COMPACT slots the per-line stage left per 1024-line tile
// (BLKCNT[b][tile] selected lines at slots 1024 tile + rank, LIDC = line | kj << 24): a workgroup takes the tile's lines
// rank 32 (sub + BWDS_SUBS i) ..., eight lanes per line; workgroups beyond the tile's count return after one load.  The
// round-1 grid covered every POSSIBLE slot of the sample's dense list (8 L lanes per sample, ~9 % live, every dead lane
// walking the same chain of loads up to the DPP exchange): 11 us at C2, 53 us at B = 64; and every live lane issued its
// nine atomics itself (wave_scatter_rows, rrl_stage_pair.h).
#define BWDS_LINES 32  // selected lines per pass of a 256-lane workgroup
#define BWDS_SUBS 4
// Deterministic scatter: the exponent e with |any single contribution| < 2^e for a sample with upstream gradient gl, C valid
// buckets and median m.  A contribution is w/3 * sum_{o < 4} 2 (q1 - q2)_c * scale * sw * exp(-D / 2m) / (2m) with w <= 1,
// scale <= |gl| / C, sw <= 2 and |q1 - q2| exp(-D / 2m) / m <= sqrt(D) exp(-D / 2m) / m <= 0.607 / sqrt(m): below
// 1.62 |gl| / (C sqrt(m)); two more binades of slack.  Non-positive / non-finite bound: 0 (such a sample's contributions are
// zero or non-finite).  The SAME expression in the scatter and in the conversion: same bits.
__device__ __forceinline__ int scat_unit_exp(float gl, int C, float m) {
    const float bnd = 1.62f * fabsf(gl) / ((float)(C > 0 ? C : 1) * sqrtf(m));
    if (!(bnd > 0.0f) || !(bnd < INFINITY)) return 0;
    return ilogbf(bnd) + 3;
}
__device__ __forceinline__ int scat_fx_bits(int L) {  // <= L contributions per element: 62 - ceil(log2 L) fractional bits
    int lg = 1;
    while ((1 << lg) < L && lg < 30) ++lg;
    return 62 - lg;
}

// The arithmetic of the scatter backward for one lane = (selected line, side, hit slot h), 8 lanes per line ((side, h) =
// lane bits 2 and 0..1); every lane of the wavefront calls (DPP exchange, LDS transpose).  valid: the lane has a line;
// live: ... and a hit whose gradient row is wanted; d[o]: row h (cloud 1) / column h (cloud 2) of the line's D tile (+inf
// outside the block); S: the (k, j) bucket's line count; mine / f / wq: this hit's intersection point, triangle and weights;
// other_of(o): intersection point o of the OTHER cloud (asked for only where an entry carries gradient).
template <class OtherF>
__device__ __forceinline__ void bwd_scatter_math(bool live, int k, int j, int side, int h, const float (&d)[4], int S,
                                                 float4 mine, int f, const float (&wq)[3], int C, float m, float gl_in,
                                                 OtherF other_of, float *__restrict__ g1b, float *__restrict__ g2b,
                                                 unsigned *strip, int lane, unsigned long long *fx1b = nullptr,
                                                 unsigned long long *fx2b = nullptr, double inv_unit = 0.0, int32_t *nonfinite = nullptr) {
    const int ocnt = side ? k : j;
    const int omax = (int)wave_max((float)(k > j ? k : j));  // uniform
    float er[4] = {0.0f, 0.0f, 0.0f, 0.0f}, wr[4];
#pragma unroll
    for (int o = 0; o < RRL_MAX_HITS; ++o) {
        wr[o] = INFINITY;
        if (o < omax) {
            const float ex = expf(-(d[o] / m) / 2.0f);  // == welsch(): 1 - e
            er[o] = ex;
            if (d[o] < INFINITY) wr[o] = 1.0f - ex;
        }
    }
    int own = 0;  // first-occurrence argmin of this row / column
    {
        float bestw = wr[0];
#pragma unroll
        for (int o = 1; o < RRL_MAX_HITS; ++o)
            if (wr[o] < bestw) { bestw = wr[o]; own = o; }
    }
    // the other quad's minima: lane (side, .) reads lane (1 - side, .) of its line, then slot o of that quad
    const int up = __builtin_amdgcn_update_dpp(0, own, 0x104, 0xf, 0xf, true);  // row_shl:4: from lane + 4
    const int dn = __builtin_amdgcn_update_dpp(0, own, 0x114, 0xf, 0xf, true);  // row_shr:4: from lane - 4
    const float oth = __int_as_float(side ? dn : up);
    const int oarg[4] = {__float_as_int(quad_bcast<0>(oth)), __float_as_int(quad_bcast<1>(oth)),
                         __float_as_int(quad_bcast<2>(oth)), __float_as_int(quad_bcast<3>(oth))};
    float sv[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (live) {
        const float wkj = expf(-0.5f * (float)abs(k - j));
        const float scale = gl_in * wkj / (float)C;
        const float inv_row = 1.0f / ((float)S * (float)k), inv_col = 1.0f / ((float)S * (float)j);
        float gq[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int o = 0; o < RRL_MAX_HITS; ++o) {
            if (o >= ocnt) continue;
            // entry (a, bb) = (h, o) for cloud 1, (o, h) for cloud 2: it is the row minimum when arg_b[a] == bb and the column
            // minimum when arg_a[bb] == a
            float sw = 0.0f;
            if (side) {
                if (oarg[o] == h) sw += inv_row;  // arg_b[o] == h
                if (own == o) sw += inv_col;      // arg_a[h] == o
            } else {
                if (own == o) sw += inv_row;      // arg_b[h] == o
                if (oarg[o] == h) sw += inv_col;  // arg_a[o] == h
            }
            if (sw == 0.0f) continue;
            // dWl/dD = exp(-D/(2 med)) / (2 med);  dD/dq1 = 2 (q1 - q2) = -dD/dq2
            const float gD = scale * sw * er[o] / (2.0f * m);
            const float4 other = other_of(o);
            gq[0] += 2.0f * (mine.x - other.x) * gD;
            gq[1] += 2.0f * (mine.y - other.y) * gD;
            gq[2] += 2.0f * (mine.z - other.z) * gD;
        }
#pragma unroll
        for (int kk = 0; kk < 3; ++kk) {
            const float wk = wq[kk] / 3.0f;  // q = mean_k(w_k P_k)
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) sv[3 * kk + cc] = wk * gq[cc];
        }
    }
    wave_scatter_rows(live, sv, (unsigned)f | (side ? 0x80000000u : 0u), g1b, g2b, strip, lane, fx1b, fx2b, inv_unit, nonfinite);
}

// One pass of the scatter backward from the workspace: this lane = (the tile's selected line of rank r, side, hit slot h);
// slot0: the tile's first compact slot, cnt its selected lines, C / m / gl_in the sample's valid count, median and upstream
// gradient.  Every lane of the wavefront calls.
__device__ __forceinline__ void bwd_scatter_pass(const ScatArgs &a, int b, size_t slot0, int cnt, int r, int g, int C, float m,
                                                 float gl_in, unsigned *strip, int lane) {
    const float *__restrict__ D = a.D;
    const int side = (lane >> 2) & 1, h = lane & 3;
    const bool valid = r < cnt && C > 0;
    const unsigned e = valid ? a.lidc[slot0 + r] : 0u;  // line | k << 24 | j << 28: no second look at the counts
    const int k = (int)((e >> 24) & 15u), j = (int)(e >> 28);
    const size_t gl = (size_t)b * a.L + (e & 0xffffffu);
    const int mycnt = side ? j : k, ocnt = side ? k : j;  // this lane's hit slots, the other cloud's
    const bool live = valid && h < mycnt && !(side && !a.g2);
    float d[4] = {INFINITY, INFINITY, INFINITY, INFINITY};
    if (valid && h < mycnt) {
#pragma unroll
        for (int o = 0; o < RRL_MAX_HITS; ++o)
            if (o < ocnt) d[o] = D[gl * 16 + (side ? o * j + h : h * j + o)];  // row h (cloud 1) / column h (cloud 2)
    }
    // (requested now, used after the exchange: the loads of the gradient's own chain overlap the Welsch arithmetic)
    int f = 0, S = 1;
    float4 mine = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float wq[3] = {0.0f, 0.0f, 0.0f};
    if (live) {
        S = a.bcnt[g * 16 + (k - 1) * 4 + (j - 1)];
        mine = (side ? a.Q2 : a.Q1)[gl * 4 + h];
        f = (side ? a.hs2 : a.hs1)[gl * 4 + h];
        const float *w = (side ? a.w2 : a.w1) + (gl * 4 + h) * 3;
#pragma unroll
        for (int q = 0; q < 3; ++q) wq[q] = w[q];
    }
    const float4 *__restrict__ Qo = side ? a.Q1 : a.Q2;
    if (a.fx) {  // uniform: deterministic mode -- fixed-point accumulators, unit 2^(scat_unit_exp - fxbits)
        unsigned long long *fx1b = a.fx + (size_t)b * (a.N + a.M) * 9, *fx2b = fx1b + (size_t)a.N * 9;
        int32_t *flags = (int32_t *)(a.fx + (size_t)a.fxB * (a.N + a.M) * 9) + 2 * b;
        bwd_scatter_math(live, k, j, side, h, d, S, mine, f, wq, C, m, gl_in, [&](int o) { return Qo[gl * 4 + o]; }, nullptr, nullptr,
                         strip, lane, fx1b, fx2b, ldexp(1.0, a.fxbits - scat_unit_exp(gl_in, C, m)), flags);
        return;
    }
    bwd_scatter_math(live, k, j, side, h, d, S, mine, f, wq, C, m, gl_in, [&](int o) { return Qo[gl * 4 + o]; },
                     a.g1 + (size_t)b * a.N * 9, a.g2 ? a.g2 + (size_t)b * a.M * 9 : nullptr, strip, lane);
}

// Deterministic mode: the fixed-point accumulators -> fp32 gradients.  grid (ceil(max(N, M) * 9 / 256), B, clouds)
__global__ __launch_bounds__(256) void scatter_fix_to_float_kernel(const ScatArgs a, int B, int pool) {
    const int b = blockIdx.y, side = blockIdx.z, g = pool ? 0 : b;
    const int n = side ? a.M : a.N;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n * 9) return;
    const int C = a.info[g * 4];
    const float m = a.med[g], gl_in = a.grad_loss[g];
    const double unit = ldexp(1.0, scat_unit_exp(gl_in, C, m) - a.fxbits);
    const long long q = (long long)(a.fx + (size_t)b * (a.N + a.M) * 9 + (side ? (size_t)a.N * 9 : 0))[i];
    const int32_t bad = ((const int32_t *)(a.fx + (size_t)B * (a.N + a.M) * 9))[2 * b + side];
    (side ? a.g2 + (size_t)b * a.M * 9 : a.g1 + (size_t)b * a.N * 9)[i] = bad ? __builtin_nanf("") : (float)((double)q * unit);
}

__global__ __launch_bounds__(256) void loss_bwd_kernel(const ScatArgs a, int B, int pool, int xcd_align) {
    __shared__ unsigned s_scat[4][64 * SCAT_STRIDE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sub = blockIdx.z, ntile = gridDim.x;
    int tile = blockIdx.x, b = blockIdx.y;
    if (xcd_align) xcd_sample_of(tile + ntile * b, ntile, tile, b);  // (uniform) sample b's workgroups on XCD b % 8
    const int g = pool ? 0 : b;
    const int cnt = a.blkcnt[(size_t)b * ntile + tile];
    if (sub * BWDS_LINES >= cnt) return;  // uniform: no line for this workgroup
    const int C = a.info[g * 4];
    const float m = a.med[g], gl_in = a.grad_loss[g];
    const size_t slot0 = ((size_t)b * ntile + tile) * 1024;
    for (int r0 = sub * BWDS_LINES; r0 < cnt; r0 += BWDS_LINES * BWDS_SUBS)  // uniform; a second trip only beyond 128 lines
        bwd_scatter_pass(a, b, slot0, cnt, r0 + (tid >> 3), g, C, m, gl_in, s_scat[wave], lane);
}

// K2 + K3 + K4 + K5 in ONE launch for a single tile of lines (L <= 1024; C5: N = M = 16384, L = 512) -- SURVEY 8(d)'s step
// (rrl_loss_step_ex: backward to points1.grad) at the shapes pair_reduce_kernel serves: the workgroup of sample b ran the
// per-line stage and the reduce of sample b, so it carries on with the scatter backward of the
// sample's selected lines (loss_bwd_kernel's arithmetic, 8 lines per wavefront and pass).  Same bodies, same
// results; payload[0 .. 1] as in the tail kernel.  grad_tri1 is zero on entry (the records launch cleared it).
// At most 128 selected lines (one pass of the per-line stage: every (line, cloud, hit) lane still HOLDS its triangle, weights and
// intersection point, and the line's eight points sit in the stage's LDS) nothing is read back: the reduce takes the compact
// rows from an LDS copy, the backward re-evaluates its D row / column from the points with the stage's own expression
// (bit-identical to the stored tile), takes the median from the reduce's registers and the bucket counts from its LDS -- and
// starts as soon as those exist, while the workgroup's last wavefront turns the sums into the loss (SoloReduce).  More lines:
// through the workspace, as above.
__global__ __launch_bounds__(1024) void pair_reduce_scatter_kernel(const PairArgs pa, const ReduceArgs ra, const ScatArgs a,
                                                                    float *__restrict__ payload, uint32_t *__restrict__ mctl) {
    __shared__ unsigned s_scat[16][64 * SCAT_STRIDE];
    __shared__ __attribute__((aligned(16))) float s_dct[128 * 16];  // the first pass's compact D tiles ...
    __shared__ uint8_t s_kjct[128];                                 // ... and (k | j << 4) bytes, for the reduce
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float gl_in = a.grad_loss[b];  // (requested now)
    PairKeep kp;
    kp.kjc_lds = s_kjct; kp.dc_lds = s_dct;
    STAMP(0);
    pair_body(pa, b, 0, 1, &kp);
    const int cnt = kp.total;       // (uniform)
    const bool small = cnt <= 128;  // one pass of the per-line stage: the reduce and the backward read nothing back
    if (!small) __threadfence_block();  // this workgroup's KJC / VALS / BLKCNT / LIDC stores are complete ...
    __syncthreads();                    // ... before any of its lanes reads them back (small: the LDS copies are)
    STAMP(3);
    SoloReduce so;
    so.total = cnt; so.kjc = small ? s_kjct : nullptr; so.dc = small ? s_dct : nullptr; so.fwave = 15;
    reduce_body(ra, b, &so);  // (every wavefront but the last returns once the median and the bucket counts exist)
    STAMP(6);
    // the non-empty buckets of the range (code/loss.py:230's C), by every wavefront from the counts in LDS
    const int sc = lane < 16 ? so.s_cnt[lane] : 0, kk = (lane & 15) / 4 + 1, jj = (lane & 3) + 1;
    const int C = __popcll(__ballot(lane < 16 && sc > 0 && kk >= ra.s_m && kk < ra.e_m && jj >= ra.s_n && jj < ra.e_n));
    const float m = so.out_med;
    if (tid == 64 * 15 && payload && C > 0) tiled_payload(payload, mctl, so.out_loss);  // (order-independent: fixed-point sum of the valid samples' losses)
    if (small) {
        if ((tid & ~63) >> 3 >= cnt) return;  // wave-uniform: none of this wavefront's eight ranks holds a line
        const int side = (lane >> 2) & 1, h = lane & 3, k = kp.k, j = kp.j;
        const int mycnt = side ? j : k, ocnt = side ? k : j;
        const bool valid = (tid >> 3) < cnt && C > 0;
        const bool live = valid && h < mycnt && !side;  // (grad_tri2 never rides here)
        float d[4] = {INFINITY, INFINITY, INFINITY, INFINITY};
        if (valid && h < mycnt) {
#pragma unroll
            for (int o = 0; o < RRL_MAX_HITS; ++o)
                if (o < ocnt) {  // pair_hit's expression for entry (ra, rb) = (h, o) / (o, h): cloud 1's point minus cloud 2's
                    const float4 p1 = kp.sq[side ? o : h], p2 = kp.sq[4 + (side ? h : o)];
                    const float dx = p1.x - p2.x, dy = p1.y - p2.y, dz = p1.z - p2.z;
                    float sq = dx * dx;
                    sq = sq + dy * dy;
                    sq = sq + dz * dz;
                    d[o] = sq;
                }
        }
        const int S = live ? so.s_cnt[(k - 1) * 4 + (j - 1)] : 1;
        const float4 *sq = kp.sq;
        bwd_scatter_math(live, k, j, side, h, d, S, kp.q, kp.f, kp.w, C, m, gl_in, [&](int o) { return sq[side ? o : 4 + o]; },
                         a.g1 + (size_t)b * a.N * 9, nullptr, s_scat[wave], lane);
        STAMP(8);
        return;
    }
    __threadfence_block();  // (more than one pass: from the workspace -- the finishing wavefront's BCNT is read back)
    __syncthreads();
    for (int r0 = 0; r0 < cnt; r0 += 128)  // uniform
        bwd_scatter_pass(a, b, (size_t)b * 1024, cnt, r0 + (tid >> 3), b, C, m, gl_in, s_scat[wave], lane);
}

// ---------------------------------------------------------------------------------------
// K5' backward of the fused training op when only dL/dR and dL/dt are wanted (the usual case:
// the source cloud is data).  The gradient of a moved point y = x m + t contributes x (x) g to
// dL/dm and g to dL/dt, so every (selected line, hit) lane adds its three points' terms straight
// into 12 per-lane sums: no scatter into a per-triangle gradient, no pass over the N points
// afterwards.  Every live workgroup adds its 12 sums to dL/dR, dL/dt of its sample and to the
// 14-float shard payload with float atomics (26 fire-and-forget adds per workgroup); the outputs
// must be ZERO on entry (the forward clears the workspace field GACC for this).  ONE launch.
// Handing the partials to a "last workgroup" for a fixed-order sum (write-through stores, ticket,
// agent-scope loads: four dependent cross-XCD round trips) cost 5 us more, a second tiny launch
// for it 2 us more (measured); the price of the atomics is run-to-run rounding noise in the
// gradient (the loss itself stays bit-deterministic).
// ---------------------------------------------------------------------------------------
#define BWD_LINES 64  // selected lines per 256-lane workgroup (4 hit slots each)

__device__ __forceinline__ int bwd_live_blocks(int ns) { return ns > 0 ? (ns + BWD_LINES - 1) / BWD_LINES : 1; }

// The (dL/dR, dL/dt) terms of ONE selected line's hit slot h (li: its index within sample b, or -1) added to acc[12]
// (9 sums of x (x) g in m-index order, 3 of g).  ALL lanes of the wavefront must call it: the four lanes of a line share
// its Welsch tile by quad DPP.
// The arithmetic of the direct (dR, dt) backward for one lane = (selected line, hit slot h of cloud 1), four lanes per line (a
// DPP quad); every lane of the wavefront calls, lanes without a line or hit carry +inf rows and k = j = 0.  dr: row h of the
// line's D tile; S: the (k, j) bucket's line count; mine / wq / xs: this hit's intersection point, weights and SOURCE triangle
// (unmoved); qx / qy / qz: cloud 2's intersection points; acc: 9 sums for dL/dm (m-index order) + 3 for dL/dt.
__device__ __forceinline__ void bwd_rt_math(bool live, int k, int j, int h, const float (&dr)[4], int S, float4 mine,
                                            const float (&qx)[4], const float (&qy)[4], const float (&qz)[4],
                                            const float (&wq)[3], const float (&xs)[9], int C, float m, float gl_in, float *acc) {
    const int jmax = (int)wave_max((float)j);  // uniform
    float er[4] = {0.0f, 0.0f, 0.0f, 0.0f}, wr[4];
#pragma unroll
    for (int o = 0; o < RRL_MAX_HITS; ++o) {
        wr[o] = INFINITY;
        if (o < jmax) {
            const float e = expf(-(dr[o] / m) / 2.0f);  // == welsch(): 1 - e
            er[o] = e;
            if (dr[o] < INFINITY) wr[o] = 1.0f - e;
        }
    }
    int arg_b_own = 0, arg_a[4];
    {
        float bestw = wr[0];
#pragma unroll
        for (int o = 1; o < RRL_MAX_HITS; ++o)
            if (wr[o] < bestw) { bestw = wr[o]; arg_b_own = o; }
#pragma unroll
        for (int o = 0; o < RRL_MAX_HITS; ++o) {
            const float w0 = quad_bcast<0>(wr[o]), w1_ = quad_bcast<1>(wr[o]), w2_ = quad_bcast<2>(wr[o]), w3 = quad_bcast<3>(wr[o]);
            float best = w0;
            int mm = 0;
            if (w1_ < best) { best = w1_; mm = 1; }
            if (w2_ < best) { best = w2_; mm = 2; }
            if (w3 < best) { best = w3; mm = 3; }
            arg_a[o] = mm;
        }
    }
    if (live) {
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
            // same expressions as loss_bwd_kernel
            const float gD = scale * sw * er[o] / (2.0f * m);
            gq[0] += 2.0f * (mine.x - qx[o]) * gD;
            gq[1] += 2.0f * (mine.y - qy[o]) * gD;
            gq[2] += 2.0f * (mine.z - qz[o]) * gD;
        }
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

__device__ __forceinline__ void bwd_rt_line(int li, int h, int b, int L, int N, const uint8_t *__restrict__ kj,
                                            const int32_t *__restrict__ hs1, const float *__restrict__ w1,
                                            const float4 *__restrict__ Q1, const float4 *__restrict__ Q2,
                                            const float *__restrict__ D, const float *__restrict__ med,
                                            const int32_t *__restrict__ bcnt, const int32_t *__restrict__ info,
                                            const float *__restrict__ grad_loss, const float *__restrict__ src, float *acc,
                                            int bs /* the source entry of sample b (multi-pose: b % Bt) */) {
    const int C = info[b * 4];
    // The four lanes of a line SHARE its Welsch tile (round 3): lane h evaluates row h -- <= 4 exponentials and divisions
    // where every lane used to evaluate all 16 entries -- and the rows travel by quad DPP; all lanes take part (DPP
    // reads active lanes only), lanes without a line or hit slot carry +inf rows and k = j = 0.  Same expressions, same
    // first-occurrence minima, same results as welsch_block on the whole tile.
    const bool valid = li >= 0 && C > 0;
    const size_t gl = (size_t)b * L + (valid ? li : 0);
    const unsigned c = valid ? kj[gl] : 0u;
    const int k = c & 15, j = c >> 4;
    const bool live = valid && h < k;
    const float m = med[b];
    float dr[4] = {INFINITY, INFINITY, INFINITY, INFINITY};
    float4 mine = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float qx[4] = {0.0f, 0.0f, 0.0f, 0.0f}, qy[4] = {0.0f, 0.0f, 0.0f, 0.0f}, qz[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float wq[3] = {0.0f, 0.0f, 0.0f}, xs[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    int S = 1;
    if (live) {
#pragma unroll
        for (int o = 0; o < RRL_MAX_HITS; ++o)
            if (o < j) {
                dr[o] = D[gl * 16 + h * j + o];
                const float4 t = Q2[gl * 4 + o];
                qx[o] = t.x; qy[o] = t.y; qz[o] = t.z;
            }
        S = bcnt[b * 16 + (k - 1) * 4 + (j - 1)];
        mine = Q1[gl * 4 + h];
        const int f = hs1[gl * 4 + h];
        const float *w = w1 + (gl * 4 + h) * 3;
#pragma unroll
        for (int q = 0; q < 3; ++q) wq[q] = w[q];
        const float *x = src + ((size_t)bs * N + f) * 9;
#pragma unroll
        for (int q = 0; q < 9; ++q) xs[q] = x[q];
    }
    bwd_rt_math(live, k, j, h, dr, S, mine, qx, qy, qz, wq, xs, C, m, live ? grad_loss[b] : 0.0f, acc);
}

// DET = true (rrl_set_deterministic): instead of the atomics every workgroup stores its 12 sums to
// part[b][workgroup][12] and loss_bwd_rt_finalize_kernel adds them in index order; the assignment of
// lines to workgroups is fixed too (see below) -- bit-reproducible from run to run, one more (tiny) launch.
// (bx, by: the workgroup's place in the backward's grid, gx its first extent -- blockIdx / gridDim in loss_bwd_rt_kernel,
//  decoded from a linear index in bwd_write_kernel)
template <bool DET>
__device__ __forceinline__ void loss_bwd_rt_body(
    const uint8_t *__restrict__ kj, const int32_t *__restrict__ sel, const int32_t *__restrict__ nsel,
    const int32_t *__restrict__ hs1, const float *__restrict__ w1, const float4 *__restrict__ Q1,
    const float4 *__restrict__ Q2, const float *__restrict__ D, const float *__restrict__ med,
    const int32_t *__restrict__ bcnt, const int32_t *__restrict__ info,
    const float *__restrict__ grad_loss, const float *__restrict__ src, float *__restrict__ gR,
    float *__restrict__ gt, float *__restrict__ payload, const float *__restrict__ loss, int B, int N,
    int L, int transpose_r, float *__restrict__ part, const int bx, const int by, const int gx, const int Bt = 0) {
    __shared__ float red[4][12];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = by;
    const int h = tid & 3;
    int li = -1;  // this lane's selected line (index within the sample), or none
    if constexpr (DET) {
        // SEL lists the selected lines in the order the pair kernel's workgroups happened to reserve their
        // slots (an atomic): grouping lines into workgroups by SEL position would change the rounding of
        // the partial sums from run to run.  Here workgroup (tile, sub) takes the selected lines of its
        // 1024-line tile with rank 64 sub .. 64 sub + 63 in a FIXED order (round r, then thread), found
        // from the KJ bytes of the tile.
        __shared__ int s_line[BWD_LINES];
        __shared__ int s_wc[4][4];
        const int tile = bx >> 4, sub = bx & 15;
        bool sl[4];
        unsigned long long bm[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int l = tile * 1024 + r * 256 + tid;
            sl[r] = l < L && kj[(size_t)b * L + l] != 0;
            bm[r] = __ballot(sl[r]);
            if (lane == 0) s_wc[r][wave] = __popcll(bm[r]);
        }
        if (tid < BWD_LINES) s_line[tid] = -1;
        __syncthreads();
        int before = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            int mine = before;
            for (int w = 0; w < 4; ++w) {
                if (w < wave) mine += s_wc[r][w];
                before += s_wc[r][w];
            }
            const int rel = mine + __popcll(bm[r] & ((1ull << lane) - 1ull)) - BWD_LINES * sub;
            if (sl[r] && rel >= 0 && rel < BWD_LINES) s_line[rel] = tile * 1024 + r * 256 + tid;
        }
        __syncthreads();
        li = s_line[tid >> 2];
    } else {
        const int ns = nsel[b];
        if (bx >= bwd_live_blocks(ns)) return;  // uniform: nothing selected in this slice
        const int i = bx * BWD_LINES + (tid >> 2);
        if (i < ns) li = sel[(size_t)b * L + i];
    }
    float acc[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) acc[q] = 0.0f;
    bwd_rt_line(li, h, b, L, N, kj, hs1, w1, Q1, Q2, D, med, bcnt, info, grad_loss, src, acc, (Bt > 0 && b >= Bt) ? b % Bt : b);
#pragma unroll
    for (int q = 0; q < 12; ++q) acc[q] = wave_sum(acc[q]);
    if (lane == 0)
#pragma unroll
        for (int q = 0; q < 12; ++q) red[wave][q] = acc[q];
    __syncthreads();
    if (tid < 12) {
        const float v = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
        int o = tid;  // m-index (i, j) -> memory order of R
        if (tid < 9 && transpose_r) o = (tid % 3) * 3 + tid / 3;
        if constexpr (DET) {
            part[((size_t)b * gx + bx) * 12 + o] = v;
        } else {
            if (tid < 9) atomicAdd(&gR[b * 9 + o], v); else atomicAdd(&gt[b * 3 + (tid - 9)], v);
            if (payload) atomicAdd(&payload[2 + o], v);
        }
    }
    if (!DET && payload && bx == 0 && b == 0 && tid >= 64 && tid < 66) {  // [sum of valid losses, #valid]
        double sp = 0.0;
        for (int k = 0; k < B; ++k) sp += info[k * 4] > 0 ? (tid == 64 ? (double)loss[k] : 1.0) : 0.0;
        payload[tid - 64] = (float)sp;
    }
}

template <bool DET>
__global__ __launch_bounds__(256) void loss_bwd_rt_kernel(
    const uint8_t *__restrict__ kj, const int32_t *__restrict__ sel, const int32_t *__restrict__ nsel,
    const int32_t *__restrict__ hs1, const float *__restrict__ w1, const float4 *__restrict__ Q1,
    const float4 *__restrict__ Q2, const float *__restrict__ D, const float *__restrict__ med,
    const int32_t *__restrict__ bcnt, const int32_t *__restrict__ info,
    const float *__restrict__ grad_loss, const float *__restrict__ src, float *__restrict__ gR,
    float *__restrict__ gt, float *__restrict__ payload, const float *__restrict__ loss, int B, int N,
    int L, int transpose_r, float *__restrict__ part, int Bt, int xcd_align) {
    int bx = blockIdx.x, by = blockIdx.y;
    if (xcd_align) xcd_sample_of(bx + (int)gridDim.x * by, (int)gridDim.x, bx, by);  // (uniform) sample `by` on XCD by % 8
    loss_bwd_rt_body<DET>(kj, sel, nsel, hs1, w1, Q1, Q2, D, med, bcnt, info, grad_loss, src, gR, gt, payload, loss, B, N, L,
                          transpose_r, part, bx, by, (int)gridDim.x, Bt);
}

// The direct backward AND the write pass of the next epoch's line sampler in ONE launch (round 4b; rrl_ws.h RrlWriteRider,
// rrl_demo_epoch): 256-lane workgroups both; workgroups [0, tiles x rounds) write, the others run the backward.
template <bool DET>
__global__ __launch_bounds__(256) void bwd_write_kernel(const BwdKArgs a, const WriteKArgs c) {
    extern __shared__ int s_tc_dyn[];  // the write pass's tile counts [rounds][tiles]
    const int nwrite = c.gx * c.gy, lin = (int)blockIdx.x;
    if (lin < nwrite) {  // uniform per workgroup
        sample_write_body<256>(s_tc_dyn, nullptr, c.rng_state, c.r, c.centers, nullptr, nullptr, c.accept, c.lines, c.filled, 1, c.n,
                               c.rounds, lin % c.gx, lin / c.gx, 0, c.gx, (unsigned)nwrite);
        return;
    }
    const int l2 = lin - nwrite;
    loss_bwd_rt_body<DET>(a.kj, a.sel, a.nsel, a.hs1, a.w1, a.Q1, a.Q2, a.D, a.med, a.bcnt, a.info, a.grad_loss, a.src, a.gR, a.gt,
                          a.payload, a.loss, a.B, a.N, a.L, a.transpose_r, a.part, l2 % a.gx, l2 / a.gx, a.gx);
}

// Fixed-order tail of the deterministic direct backward: one lane per (sample, entry) adds the live
// workgroups' partials in index order (double accumulator), then 14 lanes build the payload over the
// samples in index order.  One workgroup; B * 12 <= a few hundred sums of <= L / 64 terms.
__global__ __launch_bounds__(256) void loss_bwd_rt_finalize_kernel(const float *__restrict__ part,
                                                                   const int32_t *__restrict__ info,
                                                                   const float *__restrict__ loss, float *__restrict__ gR,
                                                                   float *__restrict__ gt, float *__restrict__ payload,
                                                                   int B, int nblk) {
    for (int e = threadIdx.x; e < B * 12; e += 256) {
        const int b = e / 12, o = e % 12;
        double s = 0.0;
        for (int k = 0; k < nblk; ++k) s += (double)part[((size_t)b * nblk + k) * 12 + o];
        if (o < 9) gR[b * 9 + o] = (float)s; else gt[b * 3 + (o - 9)] = (float)s;
    }
    if (!payload) return;
    __syncthreads();  // gR / gt of every sample are written (same workgroup)
    if (threadIdx.x < 14) {
        const int q = threadIdx.x;
        double s = 0.0;
        for (int b = 0; b < B; ++b) {
            if (q == 0) s += info[b * 4] > 0 ? (double)loss[b] : 0.0;
            else if (q == 1) s += info[b * 4] > 0 ? 1.0 : 0.0;
            else if (q < 11) s += (double)gR[b * 9 + (q - 2)];
            else s += (double)gt[b * 3 + (q - 11)];
        }
        payload[q] = (float)s;
    }
}

// K2 + K3 + K4 + K5' in ONE launch for a single tile of lines (L <= 1024; C5: N = M = 16384, L = 512): the workgroup of
// sample b ran the per-line stage and the reduce of sample b, so it holds everything the direct backward of sample b
// reads -- no other workgroup is involved at all.  Same bodies (pair_body, reduce_body, bwd_rt_line), same results;
// (dR, dt) of a sample by ONE workgroup in a fixed order (deterministic here), payload[0 .. 1] as in the tail kernel.
__global__ __launch_bounds__(1024) void pair_reduce_bwd_kernel(const PairArgs pa, const ReduceArgs ra, const SoloBwd a) {
    __shared__ float s_red[16][12];
    __shared__ __attribute__((aligned(16))) float s_dct[128 * 16];  // the first pass's compact D tiles and (k | j << 4) bytes
    __shared__ uint8_t s_kjct[128];                                 // for the reduce (pair_reduce_scatter_kernel)
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int bs = (a.Bt > 0 && b >= a.Bt) ? b % a.Bt : b;  // the instance's source entry (multi-pose)
    const float gl_in = a.grad_loss[b];  // (requested now)
    PairKeep kp;
    kp.kjc_lds = s_kjct; kp.dc_lds = s_dct;
    pair_body(pa, b, 0, 1, &kp);
    const int ns = kp.total;       // (uniform)
    const bool small = ns <= 128;  // one pass of the per-line stage: the reduce and the backward read nothing of it back
    // small: this lane's SOURCE triangle (lanes of cloud 1 with a hit), requested now -- the only load of the backward
    const int side = (lane >> 2) & 1, h = lane & 3;
    float xs[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (small && !side && h < kp.k) {
        const float *x = a.src + ((size_t)bs * a.N + kp.f) * 9;
#pragma unroll
        for (int q = 0; q < 9; ++q) xs[q] = x[q];
    }
    if (!small) __threadfence_block();  // this workgroup's KJC / VALS / BLKCNT stores are complete ...
    __syncthreads();                    // ... before any of its lanes reads them back (small: the LDS copies are)
    SoloReduce so;
    so.total = ns; so.kjc = small ? s_kjct : nullptr; so.dc = small ? s_dct : nullptr; so.fwave = 15;
    reduce_body(ra, b, &so);
    const int sc = lane < 16 ? so.s_cnt[lane] : 0, kk = (lane & 15) / 4 + 1, jj = (lane & 3) + 1;
    const int C = __popcll(__ballot(lane < 16 && sc > 0 && kk >= ra.s_m && kk < ra.e_m && jj >= ra.s_n && jj < ra.e_n));
    if (tid == 64 * 15 && a.payload && C > 0) tiled_payload(a.payload, a.mctl, so.out_loss);  // payload[0 .. 1] as in the tail kernel (order-independent)
    float acc[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) acc[q] = 0.0f;
    if (small) {
        if ((tid & ~63) >> 3 < ns) {  // wave-uniform: this wavefront's eight ranks hold lines
            const int k = kp.k, j = kp.j;  // (0, 0 beyond the last line)
            const bool live = (tid >> 3) < ns && C > 0 && !side && h < k;
            float dr[4] = {INFINITY, INFINITY, INFINITY, INFINITY};
            float qx[4] = {0.0f, 0.0f, 0.0f, 0.0f}, qy[4] = {0.0f, 0.0f, 0.0f, 0.0f}, qz[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (live) {
#pragma unroll
                for (int o = 0; o < RRL_MAX_HITS; ++o)
                    if (o < j) {  // pair_hit's expression for entry (h, o): cloud 1's point minus cloud 2's
                        const float4 p1 = kp.sq[h], p2 = kp.sq[4 + o];
                        const float dx = p1.x - p2.x, dy = p1.y - p2.y, dz = p1.z - p2.z;
                        float sq = dx * dx;
                        sq = sq + dy * dy;
                        sq = sq + dz * dz;
                        dr[o] = sq;
                        qx[o] = p2.x; qy[o] = p2.y; qz[o] = p2.z;
                    }
            }
            const int S = live ? so.s_cnt[(k - 1) * 4 + (j - 1)] : 1;
            // (the cloud-2 lanes of a line form a quad of their own: they carry +inf rows and k = j = 0 like lanes without a line)
            bwd_rt_math(live, side ? 0 : k, side ? 0 : j, h, dr, S, kp.q, qx, qy, qz, kp.w, xs, C, so.out_med, gl_in, acc);
        }
    } else {
        __threadfence_block();  // (more than one pass: through the workspace -- MED / BCNT / INFO of the finishing wavefront too)
        __syncthreads();
        for (int i0 = 0; i0 < ns; i0 += 256) {  // uniform: 256 selected lines per pass, four lanes each
            const int i = i0 + (tid >> 2);
            const int li = i < ns ? a.sel[(size_t)b * a.L + i] : -1;
            bwd_rt_line(li, tid & 3, b, a.L, a.N, a.kj, a.hs1, a.w1, a.Q1, a.Q2, a.D, a.med, a.bcnt, a.info, a.grad_loss, a.src, acc, bs);
        }
    }
#pragma unroll
    for (int q = 0; q < 12; ++q) acc[q] = wave_sum(acc[q]);
    if (lane == 0)
#pragma unroll
        for (int q = 0; q < 12; ++q) s_red[wave][q] = acc[q];
    __syncthreads();
    if (tid < 12) {
        float v = 0.0f;
        for (int w = 0; w < 16; ++w) v += s_red[w][tid];
        int o = tid;  // m-index (i, j) -> memory order of R
        if (tid < 9 && a.transpose_r) o = (tid % 3) * 3 + tid / 3;
        if (tid < 9) atomicAdd(&a.gR[b * 9 + o], v); else atomicAdd(&a.gt[b * 3 + (tid - 9)], v);  // (zero on entry)
        if (a.payload) atomicAdd(&a.payload[2 + o], v);
    }
}

