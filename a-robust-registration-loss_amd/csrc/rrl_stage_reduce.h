// rrl_stage_reduce.h -- K3 + K4, median + Welsch reduce: loss_reduce_kernel (one workgroup per sample) and loss_reduce_tiled_kernel (the exchange reduce)
// This header DEFINES kernels: it is included by rrl_sparse.hip only (one translation unit holds every stage behind the scan).
#pragma once
#include "rrl_ws.h"          // (the control-word map of include/rrl.h, asserted there)
#include "rrl_arith.h"       // welsch(), FIX_SHIFT (shared with the wide pipeline, rrl_wide.hip)
#include "rrl_stage_args.h"
#include "rrl_stamps.h"
#include "rrl_stage_pair.h"  // xcd_sample_of
// ---------------------------------------------------------------------------------------
// K3+K4: one 1024-lane workgroup per sample
// ---------------------------------------------------------------------------------------

// The k x j block of D values is stored row-major with stride j; bring it into a 4 x 4
// register tile (static indices only; entries outside the block are +inf).
__device__ __forceinline__ void load_block(const float *__restrict__ Dl, int k, int j, float *Dm) {
#pragma unroll
    for (int a = 0; a < RRL_MAX_HITS; ++a)
#pragma unroll
        for (int b = 0; b < RRL_MAX_HITS; ++b) Dm[a * 4 + b] = (a < k && b < j) ? Dl[a * j + b] : INFINITY;
}

// Row/column minima of the Welsch-weighted tile with first-occurrence argmin (torch.min,
// SURVEY.md Q11).  All indices static after unrolling (no scratch).  Welsch1(inf) = 1 - exp(-inf)
// = 1 would tie with saturated entries, so padding is forced back to +inf.
__device__ __forceinline__ void welsch_block(const float *Dm, float med, float *rowmin, float *colmin,
                                             int *arg_b, int *arg_a) {
    float Wl[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) Wl[q] = Dm[q] < INFINITY ? welsch(Dm[q], med) : INFINITY;
#pragma unroll
    for (int a = 0; a < RRL_MAX_HITS; ++a) {
        float best = Wl[a * 4];
        int m = 0;
#pragma unroll
        for (int b = 1; b < RRL_MAX_HITS; ++b)
            if (Wl[a * 4 + b] < best) { best = Wl[a * 4 + b]; m = b; }
        rowmin[a] = best;
        arg_b[a] = m;
    }
#pragma unroll
    for (int b = 0; b < RRL_MAX_HITS; ++b) {
        float best = Wl[b];
        int m = 0;
#pragma unroll
        for (int a = 1; a < RRL_MAX_HITS; ++a)
            if (Wl[a * 4 + b] < best) { best = Wl[a * 4 + b]; m = a; }
        colmin[b] = best;
        arg_a[b] = m;
    }
}

// Dense index i of a sample's selected lines -> compact slot.  s_pref[x] = selected lines of the
// pair kernel's workgroups 0 .. x-1 (exclusive prefix of BLKCNT, nblk + 1 entries in LDS).
__device__ __forceinline__ size_t slot_of(const int *s_pref, int nblk, int i) {
    int lo = 0, hi = nblk;  // largest x with s_pref[x] <= i
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (s_pref[mid] <= i) lo = mid; else hi = mid;
    }
    return (size_t)lo * 1024 + (size_t)(i - s_pref[lo]);
}

// exclusive prefix of one sample's BLKCNT row into s_pref[0 .. nblk]; returns the total (all lanes)
__device__ __forceinline__ int load_prefix(const int32_t *__restrict__ cnt, int nblk, int *s_pref, int tid) {
    __syncthreads();  // s_pref may still be in use for the previous sample
    if (nblk <= 64) {  // the usual case (L <= 65536): one wavefront scans
        if (tid < 64) {
            const int c = tid < nblk ? cnt[tid] : 0;
            const int incl = wave_incl_scan(c);
            if (tid < nblk) s_pref[tid] = incl - c;
            if (tid == 63) s_pref[nblk] = incl;
        }
    } else if (tid == 0) {
        int acc = 0;
        for (int x = 0; x < nblk; ++x) { s_pref[x] = acc; acc += cnt[x]; }
        s_pref[nblk] = acc;
    }
    __syncthreads();
    return s_pref[nblk];
}

struct ReduceLds {
    int *s_pref;
    unsigned *s_hist, *s_wtot, *s_prefix, *s_rank, *s_nvals;
    unsigned *s_cand;   // [0] population of the bin chosen by pass 0, [1] gather cursor (zero between uses)
    unsigned *s_whist;  // [128] histogram of the wave-private passes
    unsigned long long *s_sum;
    int *s_cnt;
    int *s_bad;  // a Welsch term was not finite (median 0: identical clouds): the loss is NaN like the reference's
};

// Median + Welsch sums of one reduce workgroup with the first RT selected lines of every lane kept
// in registers (RT = 1 covers ns <= 1024, the usual case; RT = 3 up to 3072; beyond that the
// tiles are re-read).  Returns the median and n (the number of D values) through refs.
template <int RT>
__device__ __forceinline__ void reduce_core(const uint8_t *__restrict__ kjc, const float *__restrict__ dc,
                                            const int32_t *__restrict__ blkcnt, const ReduceLds &L_, int ns_m,
                                            int B, int nblk, int bm, int b0, int b1, int tid, float &med_o,
                                            unsigned &n_o) {
    int *s_pref = L_.s_pref;
    unsigned *s_hist = L_.s_hist, *s_wtot = L_.s_wtot, *s_prefix = L_.s_prefix, *s_rank = L_.s_rank;
    unsigned long long *s_sum = L_.s_sum;
    int *s_cnt = L_.s_cnt;
    unsigned &s_nvals = *L_.s_nvals;
    const size_t Lp = (size_t)nblk * 1024;
    float tile[RT][16];
    unsigned c0[RT];
    unsigned myvals = 0;
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        c0[r] = 0;
#pragma unroll
        for (int q = 0; q < 16; ++q) tile[r][q] = INFINITY;
        const int i = tid + 1024 * r;
        if (i < ns_m) {
            const size_t slot = (size_t)bm * Lp + slot_of(s_pref, nblk, i);
            c0[r] = kjc[slot];
            const float4 *row = (const float4 *)(dc + slot * 16);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 v = row[q];
                tile[r][4 * q] = v.x; tile[r][4 * q + 1] = v.y; tile[r][4 * q + 2] = v.z; tile[r][4 * q + 3] = v.w;
            }
            myvals += (c0[r] & 15u) * (c0[r] >> 4);
        }
    }
    for (int i = tid + 1024 * RT; i < ns_m; i += 1024) {
        const unsigned c = kjc[(size_t)bm * Lp + slot_of(s_pref, nblk, i)];
        myvals += (c & 15u) * (c >> 4);
    }
    {
        const unsigned tot = (unsigned)wave_sum_i((int)myvals);
        if ((tid & 63) == 0 && tot) atomicAdd(&s_nvals, tot);
    }
    __syncthreads();
    const unsigned n = s_nvals;
    if (tid == 0) s_rank[0] = n ? (n - 1) / 2 : 0;
    __syncthreads();
    STAMP(9);

    // ---- lower median = element of rank (n-1)/2 (torch.median): MSB-first radix select on the
    //      bit patterns (D >= 0: unsigned order == float order).  Pass 0 (bits 30..20) is
    //      workgroup-wide: LDS histogram, block-wide exclusive scan (DPP wave scans + wave
    //      totals), pick the bin that holds the rank; the histogram is cleared as it is read.
    //      The values of that bin (~n/20 of them) are then gathered into LDS and ONE wavefront
    //      finishes the remaining 20 bits in three wave-private passes (7 + 7 + 6 bits, 128-bin
    //      histogram, no workgroup barrier): 5 barriers in all instead of 9.  More than 2048
    //      values in the bin (near-identical D values): the workgroup-wide passes 1, 2 as before.
    unsigned prefix = 0;
    auto wg_pass = [&](int pass) {
        const int sh = pass == 0 ? 20 : (pass == 1 ? 9 : 0);
        const int width = pass == 2 ? 9 : 11;
        const unsigned dmask = (1u << width) - 1u;
        const int hi = sh + width;  // bits >= hi must equal the prefix (hi = 31 on the first pass)
        auto tally = [&](unsigned x) {  // +inf (padding of a tile) never agrees with a prefix of finite data
            if (x != 0x7f800000u && ((x ^ prefix) >> hi) == 0u) atomicAdd(&s_hist[(x >> sh) & dmask], 1u);
        };
#pragma unroll
        for (int r = 0; r < RT; ++r)
#pragma unroll
            for (int q = 0; q < 16; ++q) tally(__float_as_uint(tile[r][q]));
        for (int i = tid + 1024 * RT; i < ns_m; i += 1024) {
            const float *row = dc + ((size_t)bm * Lp + slot_of(s_pref, nblk, i)) * 16;
            for (int q = 0; q < 16; ++q) tally(__float_as_uint(row[q]));
        }
        __syncthreads();
        const unsigned h0 = s_hist[2 * tid], h1 = s_hist[2 * tid + 1];
        s_hist[2 * tid] = 0;
        s_hist[2 * tid + 1] = 0;
        const unsigned incl = (unsigned)wave_incl_scan((int)(h0 + h1));
        if ((tid & 63) == 63) s_wtot[tid >> 6] = incl;
        __syncthreads();
        unsigned base = 0;
        for (int w = 0; w < (tid >> 6); ++w) base += s_wtot[w];
        const unsigned excl = base + incl - (h0 + h1), r = s_rank[pass];
        if (r >= excl && r < excl + h0 + h1) {  // exactly one lane
            const unsigned second = r >= excl + h0 ? 1u : 0u;
            s_prefix[pass] = prefix | ((2u * tid + second) << sh);
            s_rank[pass + 1] = r - excl - (second ? h0 : 0u);
            if (pass == 0) L_.s_cand[0] = second ? h1 : h0;  // population of the chosen bin
        }
        __syncthreads();
        prefix = s_prefix[pass];
    };
    if (n > 0 && n <= 128u) {
        // ---- a tiny sample (<= 128 values: C5's 512 lines select ~13): the values meet in LDS (s_hist is all zero and free
        //      until the next evaluation) and every one counts the smaller ones itself -- the element of rank (n-1)/2 by
        //      definition, ties broken by position (bit patterns of non-negative floats order like the values); two barriers instead of the radix select's five and its 2048-bin scans
        //      (3.1 us of the single-tile kernel's 12.0 at C5, tools/stamps.py).
        unsigned at = myvals ? atomicAdd(&L_.s_cand[1], myvals) : 0u;
#pragma unroll
        for (int r = 0; r < RT; ++r)
#pragma unroll
            for (int q = 0; q < 16; ++q)  // the k x j block of the canonical tile (myvals entries: the cursor's share)
                if ((unsigned)(q >> 2) < (c0[r] & 15u) && (unsigned)(q & 3) < (c0[r] >> 4) && at < 128u) s_hist[at++] = __float_as_uint(tile[r][q]);
        if ((unsigned)tid >= n && (unsigned)tid < n + 3u) s_hist[tid] = 0xffffffffu;  // pad to whole 16-byte groups: never counted
        __syncthreads();
        if ((unsigned)tid < n) {
            const unsigned x = s_hist[tid];
            unsigned c = 0;
            for (unsigned u = 0; u < n; u += 4) {  // (uniform addresses: one LDS read serves the wavefront)
                const uint4 y = *(const uint4 *)&s_hist[u];
                c += (y.x < x || (y.x == x && u < (unsigned)tid)) ? 1u : 0u;
                c += (y.y < x || (y.y == x && u + 1 < (unsigned)tid)) ? 1u : 0u;
                c += (y.z < x || (y.z == x && u + 2 < (unsigned)tid)) ? 1u : 0u;
                c += (y.w < x || (y.w == x && u + 3 < (unsigned)tid)) ? 1u : 0u;
            }
            if (c == s_rank[0]) s_prefix[2] = x;
        }
        __syncthreads();
        prefix = s_prefix[2];
        if ((unsigned)tid < 132u) s_hist[tid] = 0;
        if (tid == 0) L_.s_cand[1] = 0;
    } else if (n > 0) {
        wg_pass(0);
        STAMP(10);
        const unsigned ncand = L_.s_cand[0];
        if (ncand <= 2048u) {
            // gather the bin's values into s_hist (all zero now, free until the next evaluation)
            auto in_bin = [&](unsigned x) { return x != 0x7f800000u && ((x ^ prefix) >> 20) == 0u; };
            unsigned mine = 0;
#pragma unroll
            for (int r = 0; r < RT; ++r)
#pragma unroll
                for (int q = 0; q < 16; ++q) mine += in_bin(__float_as_uint(tile[r][q])) ? 1u : 0u;
            for (int i = tid + 1024 * RT; i < ns_m; i += 1024) {
                const float *row = dc + ((size_t)bm * Lp + slot_of(s_pref, nblk, i)) * 16;
                for (int q = 0; q < 16; ++q) mine += in_bin(__float_as_uint(row[q])) ? 1u : 0u;
            }
            const unsigned incl = (unsigned)wave_incl_scan((int)mine);
            unsigned wbase = 0;
            if ((tid & 63) == 63 && incl) wbase = atomicAdd(&L_.s_cand[1], incl);  // one atomic per wavefront
            wbase = (unsigned)__builtin_amdgcn_readlane((int)wbase, 63);
            unsigned at = wbase + incl - mine;
#pragma unroll
            for (int r = 0; r < RT; ++r)
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const unsigned x = __float_as_uint(tile[r][q]);
                    if (in_bin(x)) s_hist[at++] = x;
                }
            for (int i = tid + 1024 * RT; i < ns_m; i += 1024) {
                const float *row = dc + ((size_t)bm * Lp + slot_of(s_pref, nblk, i)) * 16;
                for (int q = 0; q < 16; ++q) {
                    const unsigned x = __float_as_uint(row[q]);
                    if (in_bin(x)) s_hist[at++] = x;
                }
            }
            __syncthreads();
            if (tid < 64) {  // wave 0 alone: LDS operations of one wavefront execute in order
                unsigned pre = prefix, rk = s_rank[1];
                unsigned *wh = L_.s_whist;
#pragma unroll
                for (int wp = 0; wp < 3; ++wp) {
                    const int sh = wp == 0 ? 13 : (wp == 1 ? 6 : 0);
                    const int width = wp == 2 ? 6 : 7;
                    const unsigned dmask = (1u << width) - 1u;
                    const int hi = sh + width;
                    wh[2 * tid] = 0;
                    wh[2 * tid + 1] = 0;
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    for (unsigned i = tid; i < ncand; i += 64) {
                        const unsigned x = s_hist[i];
                        if (((x ^ pre) >> hi) == 0u) atomicAdd(&wh[(x >> sh) & dmask], 1u);
                    }
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    const unsigned h0 = wh[2 * tid], h1 = wh[2 * tid + 1];
                    const unsigned inc2 = (unsigned)wave_incl_scan((int)(h0 + h1));
                    const unsigned excl = inc2 - (h0 + h1);
                    const bool here = rk >= excl && rk < excl + h0 + h1;  // exactly one lane
                    const unsigned second = rk >= excl + h0 ? 1u : 0u;
                    const unsigned long long who = __ballot(here);
                    const int src = __ffsll((long long)who) - 1;
                    pre |= (unsigned)__builtin_amdgcn_readlane((int)((2u * tid + second) << sh), src);
                    rk = (unsigned)__builtin_amdgcn_readlane((int)(rk - excl - (second ? h0 : 0u)), src);
                }
                if (tid == 0) s_prefix[2] = pre;
            }
            __syncthreads();
            prefix = s_prefix[2];
            // the gathered values leave s_hist non-zero: clear it for the next use (pool mode, later samples)
            for (unsigned i = tid; i < ncand; i += 1024) s_hist[i] = 0;
            if (tid == 0) L_.s_cand[1] = 0;
        } else {
            wg_pass(1);
            wg_pass(2);
        }
    }
    const float med = n ? __uint_as_float(prefix) : 0.0f;
    STAMP(11);

    // ---- Welsch + symmetric min per selected line, bucket sums in LDS (fixed point)
    // The forward needs the VALUES of the row / column minima only, and Welsch1 is non-decreasing
    // in D: min_b Welsch(D[a][b]) = Welsch(min_b D[a][b]) -- k + j exponentials instead of 16
    // (which entry attains the minimum matters to the backward alone: welsch_block there).
    auto accumulate = [&](const float *Dl, int k, int j) {
        float row = 0.0f, col = 0.0f;
#pragma unroll
        for (int a = 0; a < RRL_MAX_HITS; ++a)
            if (a < k) row += welsch(fminf(fminf(Dl[a * 4], Dl[a * 4 + 1]), fminf(Dl[a * 4 + 2], Dl[a * 4 + 3])), med);
#pragma unroll
        for (int bb = 0; bb < RRL_MAX_HITS; ++bb)
            if (bb < j) col += welsch(fminf(fminf(Dl[bb], Dl[4 + bb]), fminf(Dl[8 + bb], Dl[12 + bb])), med);
        // Wl in [0,1], <= 4 terms: 2^-40 fixed point keeps ~2^-38 relative resolution.  A NaN term (0 / 0 with
        // median 0, code/loss.py:20-21 gives NaN there too) cannot be carried by the fixed-point sums: flag it
        if (!(row <= 4.0f) || !(col <= 4.0f)) { atomicOr(L_.s_bad, 1); row = col = 0.0f; }
        const int bi = (k - 1) * 4 + (j - 1);
        atomicAdd(&s_sum[bi * 2 + 0], (unsigned long long)((double)row * (double)(1ll << FIX_SHIFT) + 0.5));
        atomicAdd(&s_sum[bi * 2 + 1], (unsigned long long)((double)col * (double)(1ll << FIX_SHIFT) + 0.5));
        atomicAdd(&s_cnt[bi], 1);
    };
    for (int b = b0; b < b1; ++b) {
        int ns = ns_m;
        if (b != bm) ns = load_prefix(blkcnt + (size_t)b * nblk, nblk, s_pref, tid);  // pool mode only
        if (b == bm) {
#pragma unroll
            for (int r = 0; r < RT; ++r)
                if (tid + 1024 * r < ns) accumulate(tile[r], (int)(c0[r] & 15u), (int)(c0[r] >> 4));
        }
        for (int i = b == bm ? tid + 1024 * RT : tid; i < ns; i += 1024) {
            {
                const size_t slot = (size_t)b * Lp + slot_of(s_pref, nblk, i);
                const unsigned c = kjc[slot];
                float Dl[16];
                const float4 *row = (const float4 *)(dc + slot * 16);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 r = row[q];
                    Dl[4 * q] = r.x; Dl[4 * q + 1] = r.y; Dl[4 * q + 2] = r.z; Dl[4 * q + 3] = r.w;
                }
                accumulate(Dl, (int)(c & 15u), (int)(c >> 4));
            }
        }
    }
    STAMP(12);
    med_o = med;
    n_o = n;
}

// The loss of a sample from its sixteen (k, j) buckets, by ONE wavefront (all 64 lanes call; lane bi < 16 brings bucket bi =
// (k - 1) 4 + (j - 1): its line count S and fixed-point row / column sums): the double-precision means, the bucket terms
// exp(-|k-j|/2) (mean_row + mean_col) (code/loss.py:215), and their sum in the reference's k-major order over the
// non-empty buckets of the range -- taken lane by lane through v_readlane in bucket order: an empty or out-of-range
// bucket's term is +0 and adding it changes nothing, so the sum has the bits of the loop that skips them.  (Round 5: that
// loop, one lane walking s_cnt[] / s_term[] in LDS -- ~40 dependent LDS round trips -- took 3.2 us of the single-tile
// kernel's 15.9, in-kernel time stamps of tools/stamps.py.)
struct BucketFinal {
    float acc;  // sum of the terms (the loss is acc / C)
    int C, nselected, nvalues;
};
__device__ __forceinline__ BucketFinal bucket_final(unsigned long long srow, unsigned long long scol, int S, int lane, int s_m,
                                                    int s_n, int e_m, int e_n) {
    const int k = (lane & 15) / 4 + 1, j = (lane & 3) + 1;
    const bool in = lane < 16 && S > 0 && k >= s_m && k < e_m && j >= s_n && j < e_n;
    float term = 0.0f;
    if (in) {
        const double sc = 1.0 / (double)(1ll << FIX_SHIFT);
        float mrow = (float)((double)srow * sc / ((double)S * k));
        float mcol = (float)((double)scol * sc / ((double)S * j));
        float wkj = expf(-0.5f * (float)abs(k - j));  // code/loss.py:215
        term = wkj * (mrow + mcol);
    }
    BucketFinal r;
    r.C = __popcll(__ballot(in));
    r.nselected = wave_sum_i(in ? S : 0);
    r.nvalues = wave_sum_i(lane < 16 ? S * k * j : 0);
    float acc = 0.0f;
#pragma unroll
    for (int bi = 0; bi < 16; ++bi)  // k-major, the reference's accumulation order
        acc = acc + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(term), bi));
    r.acc = acc;
    return r;
}


// K3+K4 of one group g (a sample, or all samples with the last one's median when pool) by a 1024-lane workgroup
// SOLO (the single-tile kernels, round 5): the workgroup has just run the per-line stage of sample g itself --
//   total    its selected lines (no BLKCNT read-back),
//   kjc / dc LDS copies of its compact rows when total <= 128 (no read-back of KJC / VALS and no fence in front of it), else NULL,
//   fwave    the wavefront that turns the sums into the loss (the last one: at <= 120 lines it holds none), while the others
//            return as soon as the bucket counts and the median exist -- all the backward needs: out_med, s_cnt (LDS [16]),
//   out_loss the loss (lane 0 of wavefront fwave).
struct SoloReduce {
    int total;
    const uint8_t *kjc;
    const float *dc;
    int fwave;
    float out_med, out_loss;
    const int *s_cnt;
};

__device__ __forceinline__ void reduce_body(const ReduceArgs &ra, int g, SoloReduce *solo = nullptr) {
    const uint8_t *__restrict__ kjc = ra.kjc;
    const float *__restrict__ dc = ra.dc;
    const int32_t *__restrict__ blkcnt = ra.blkcnt;
    float *__restrict__ med_out = ra.med_out;
    int32_t *__restrict__ bcnt_out = ra.bcnt_out;
    int64_t *__restrict__ bsum_out = ra.bsum_out;
    int32_t *__restrict__ info = ra.info;
    float *__restrict__ loss = ra.loss;
    const int32_t *__restrict__ status = ra.status;
    const int B = ra.B, nblk = ra.nblk, s_m = ra.s_m, s_n = ra.s_n, e_m = ra.e_m, e_n = ra.e_n, pool = ra.pool;
    extern __shared__ int s_pref[];  // nblk + 1
    __shared__ __attribute__((aligned(16))) unsigned s_hist[2048];
    __shared__ unsigned s_wtot[16];
    __shared__ unsigned s_prefix[3], s_rank[4];  // one slot per pass: no barrier between read and rewrite
    __shared__ unsigned s_nvals;
    __shared__ unsigned s_cand[2], s_whist[128];
    __shared__ unsigned long long s_sum[32];
    __shared__ int s_cnt[16];
    __shared__ int s_bad;
    const int tid = threadIdx.x;
    const int bm = pool ? B - 1 : g;  // whose values define the median
    const int b0 = pool ? 0 : g, b1 = pool ? B : g + 1;
    const int st0 = status[0];  // (the scan's NaN flag, for the info row: requested now -- at the end it would be one more round trip)
    if (tid < 32) s_sum[tid] = 0ull;
    if (tid < 16) s_cnt[tid] = 0;
    if (tid == 0) { s_nvals = 0; s_cand[0] = 0; s_cand[1] = 0; s_bad = 0; }
    s_hist[tid] = 0;
    s_hist[tid + 1024] = 0;

    int ns_m;
    if (solo) {  // (one tile: the prefix is (0, total))
        ns_m = solo->total;
        if (tid == 0) { s_pref[0] = 0; s_pref[1] = ns_m; }
        __syncthreads();
    } else {
        ns_m = load_prefix(blkcnt + (size_t)bm * nblk, nblk, s_pref, tid);
    }
    STAMP(4);
    const ReduceLds lds = {s_pref, s_hist, s_wtot, s_prefix, s_rank, &s_nvals, s_cand, s_whist, s_sum, s_cnt, &s_bad};
    float med;
    unsigned n;
    if (solo && solo->kjc) reduce_core<1>(solo->kjc, solo->dc, blkcnt, lds, ns_m, 1, 1, 0, 0, 1, tid, med, n);  // (<= 128 rows, from LDS)
    else if (ns_m <= 1024) reduce_core<1>(kjc, dc, blkcnt, lds, ns_m, B, nblk, bm, b0, b1, tid, med, n);
    else reduce_core<3>(kjc, dc, blkcnt, lds, ns_m, B, nblk, bm, b0, b1, tid, med, n);
    __syncthreads();
    STAMP(5);

    // ---- loss = ( sum_{non-empty (k,j), k-major} exp(-|k-j|/2) (mean_row + mean_col) ) / C
    const int ft = tid - (solo ? 64 * solo->fwave : 0);  // lane of the finishing wavefront (wavefront 0 but for SOLO)
    if (solo) { solo->out_med = med; solo->s_cnt = s_cnt; solo->out_loss = 0.0f; }
    if (ft < 0 || ft >= 64) return;
    if (ft < 16) bcnt_out[g * 16 + ft] = s_cnt[ft];
    if (ft < 32) bsum_out[(size_t)g * 32 + ft] = (int64_t)s_sum[ft];
    const BucketFinal f = bucket_final(ft < 16 ? s_sum[ft * 2 + 0] : 0ull, ft < 16 ? s_sum[ft * 2 + 1] : 0ull,
                                       ft < 16 ? s_cnt[ft] : 0, ft, s_m, s_n, e_m, e_n);  // one lane per bucket
    if (ft == 0) {
        const float lv = s_bad ? __builtin_nanf("") : (f.C ? f.acc / (float)f.C : 0.0f);  // code/loss.py:230
        med_out[g] = med;
        loss[g] = lv;
        info[g * 4 + 0] = f.C;
        info[g * 4 + 1] = f.nselected;
        info[g * 4 + 2] = (int)n;
        info[g * 4 + 3] = st0;  // the scan's NaN flag next to the bucket count: one 16-byte read-back decides the call
        if (solo) solo->out_loss = lv;
    }
}

__global__ __launch_bounds__(1024) void loss_reduce_kernel(const ReduceArgs ra) { reduce_body(ra, (int)blockIdx.x); }

// ---------------------------------------------------------------------------------------
// K3+K4, TILED (round 3): one 256-lane workgroup per 1024-line tile of the per-line stage instead of one
// 1024-lane workgroup per sample.  The single workgroup was bound by ONE compute unit: 11.3 us at C2 on 8 of
// 256 CUs, 24.7 us at the demo's shape (2600 selected lines of one sample through one CU).  Here
//   * the median's first radix pass (top 11 bits) arrives as a per-sample histogram that the per-line stage
//     tallied where the D values were born (MHIST) -- complete at the kernel boundary, so EVERY workgroup of a
//     sample finds the median's bin, the rank inside it and n by itself, without talking to anyone;
//   * the values of that bin (~n / 20) are published to a per-sample list (MCAND; one returning cursor atomic
//     per wavefront, write-through stores), the sample's workgroups meet at an arrival counter, and each then
//     finishes the select on the whole list by itself (the wave-private passes of the single-workgroup
//     kernel): one hop, no broadcast of the result;
//   * every workgroup adds the Welsch terms of its own lines to the sample's fixed-point bucket sums (MSUM,
//     64-bit device atomics: order-independent, so the loss keeps its bits) and the LAST one to arrive at a
//     second counter turns them into the loss.
// Cross-workgroup words follow the guide's hand-off rules: relaxed agent-scope atomic stores / loads (sc1:
// write-through, L1-bypassing), every storing wavefront drains (s_waitcnt vmcnt(0)) before its workgroup
// arrives, one lane polls.  The spin needs the sample's workgroups co-resident: the host takes this path only
// while B x tiles <= 1024 workgroups of 256 lanes (4 per CU) and bounds every spin (MCTL[b][RRL_MCTL_ERR] + a NaN loss
// instead of a hang).  More than 2048 values in the bin (near-identical D values): tile 0 finishes the
// select alone with two more streaming passes and publishes the median; the others wait for it.
// Same arithmetic and summation rules as reduce_body: bit-identical median and loss.
// ---------------------------------------------------------------------------------------
// (the control words: include/rrl.h RRL_MCTL_*)
#define MCAND_CAP 2048

__device__ __forceinline__ unsigned ld_agent(const uint32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent(uint32_t *p, unsigned v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// one lane polls one word until it reaches `want`; bounded (limit polls of ~1-2 us each: a fraction of a second by
// default), so workgroups that are not co-resident -- a partitioned device, a CU mask, another process or stream holding
// the slots -- become a flag, and the sample is then REPAIRED by its last workgroup (loss_reduce_tiled_kernel), not lost
__device__ __forceinline__ bool spin_reach(const uint32_t *p, unsigned want, unsigned limit) {
    for (unsigned it = 0; it < limit; ++it) {
        if (ld_agent(p) >= want) return true;
        __builtin_amdgcn_s_sleep(2);
    }
    return false;
}

// The remaining 20 bits of the radix select by ONE wavefront over vals[0, ncand) in LDS (the values of the bin
// `pre` chosen by the 11-bit pass; rk = rank inside it): three wave-private passes of 7 + 7 + 6 bits, 128-bin
// histogram wh, no workgroup barrier.  Every lane returns the median's bit pattern.
__device__ __forceinline__ unsigned wave_select20(const unsigned *vals, unsigned ncand, unsigned pre, unsigned rk,
                                                  unsigned *wh, int lane) {
#pragma unroll
    for (int wp = 0; wp < 3; ++wp) {
        const int sh = wp == 0 ? 13 : (wp == 1 ? 6 : 0);
        const int width = wp == 2 ? 6 : 7;
        const unsigned dmask = (1u << width) - 1u;
        const int hi = sh + width;
        wh[2 * lane] = 0;
        wh[2 * lane + 1] = 0;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        for (unsigned i = lane; i < ncand; i += 64) {
            const unsigned x = vals[i];
            if (((x ^ pre) >> hi) == 0u) atomicAdd(&wh[(x >> sh) & dmask], 1u);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const unsigned h0 = wh[2 * lane], h1 = wh[2 * lane + 1];
        const unsigned inc2 = (unsigned)wave_incl_scan((int)(h0 + h1));
        const unsigned excl = inc2 - (h0 + h1);
        const bool here = rk >= excl && rk < excl + h0 + h1;  // exactly one lane
        const unsigned second = rk >= excl + h0 ? 1u : 0u;
        const unsigned long long who = __ballot(here);
        const int src = who ? __ffsll((long long)who) - 1 : 0;
        pre |= (unsigned)__builtin_amdgcn_readlane((int)((2u * lane + second) << sh), src);
        rk = (unsigned)__builtin_amdgcn_readlane((int)(rk - excl - (second ? h0 : 0u)), src);
    }
    return pre;
}


// One sample's final loss into payload[0 .. 1] (one lane), without a last-of-all hand-over: every sample's finaliser adds
// its loss to a 2^-40 fixed-point sum (row 0's RRL_MCTL_LSUM, a returning atomic) and offers float(sum so far) to payload[0]
// by an unsigned atomicMax on the bit pattern (rrl_stage_tail.h's header).  Defined here, ahead of every kernel that calls
// it: the tail kernel in the TailArgs form, the exchange reduce and the single-tile kernels in the pointer form.
__device__ __forceinline__ void tail_payload(const TailArgs &a, float lv) {
    atomicAdd(&a.payload[1], 1.0f);
    if (lv != lv) { atomicMax((unsigned *)&a.payload[0], 0x7fc00000u); return; }
    const unsigned long long mine = (unsigned long long)((double)lv * (double)(1ll << FIX_SHIFT) + 0.5);
    const unsigned long long old = __hip_atomic_fetch_add((unsigned long long *)(a.mctl + RRL_MCTL_LSUM), mine, __ATOMIC_RELAXED,
                                                          __HIP_MEMORY_SCOPE_AGENT);
    const float tot = (float)((double)(old + mine) * (1.0 / (double)(1ll << FIX_SHIFT)));
    atomicMax((unsigned *)&a.payload[0], __float_as_uint(tot));
}
__device__ __forceinline__ void tiled_payload(float *payload, uint32_t *mctl, float lv) {
    TailArgs t;
    t.payload = payload; t.mctl = mctl;
    tail_payload(t, lv);
}

// Hand-offs between the workgroups of this launch (candidate list + TICK1, MEDRDY) are bounded spins.  A workgroup whose
// spin times out (the others were not resident in time) adds NOTHING to the sample's sums, raises RRL_MCTL_ERR and still
// draws its TICK2 ticket; the sample's LAST workgroup then sees the flag and recomputes the whole sample by itself --
// median from all tiles' values, Welsch sums over all its lines, the single-workgroup kernel's arithmetic on the same
// multiset -- so the result is bit-identical to the undisturbed one instead of NaN (round 3), at the cost of one
// workgroup's serial pass over ~1000 lines.  STATUS[2] counts such samples.
__global__ __launch_bounds__(256) void loss_reduce_tiled_kernel(const TiledArgs a) {
    __shared__ unsigned s_vals[MCAND_CAP];  // the bin's values (usual route) / histogram of the streaming passes
    __shared__ unsigned s_wtot[4];
    __shared__ unsigned s_pick[3];          // bin, rank inside it, its population
    __shared__ unsigned s_whist[128];
    __shared__ unsigned long long s_sum[32];
    __shared__ unsigned s_flag[3];          // [0] spin ok, [1] this workgroup arrived last, [2] non-finite Welsch term
    __shared__ unsigned s_med;
    __shared__ int s_cnt[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nblk = a.nblk;
    int tile = blockIdx.x, b = blockIdx.y;
    if (a.xcd_align) xcd_sample_of(tile + nblk * b, nblk, tile, b);  // (uniform)
    const size_t Lp = (size_t)nblk * 1024;
    uint32_t *ctl = a.mctl + (size_t)b * RRL_MCTL_WORDS;
    uint32_t *cand = a.mcand + (size_t)b * MCAND_CAP;
    const float *__restrict__ dc = a.dc;
    const uint8_t *__restrict__ kjc = a.kjc;

    // ---- one round of independent loads: the tile's count, its first 256 compact rows (speculative: the slots
    //      exist whether or not they were written), the sample's histogram
    const int cnt = a.blkcnt[(size_t)b * nblk + tile];
    int st0;  // (for the info row: requested with round 1)
    bool chain_tmo = false;
    if (a.chain_flags) {
        static_assert(RRL_CHAIN_WORDS == 4 && RRL_CHAIN_NAN == 1 && RRL_CHAIN_TIMEOUT == 3, "one 16-byte load: .y the NaN flag, .w the time-outs");
        const uint4 cw = *(const uint4 *)(a.chain + RRL_CHAIN_WORDS * (size_t)b);
        st0 = (int)cw.y;
        chain_tmo = cw.w != 0u;
    } else {
        st0 = a.status[0];
    }
    const size_t slot0 = (size_t)b * Lp + (size_t)tile * 1024;
    float tl[16];
    unsigned c0;
    {
        const float4 *row = (const float4 *)(dc + (slot0 + tid) * 16);
        const float4 v0 = row[0], v1 = row[1], v2 = row[2], v3 = row[3];
        c0 = kjc[slot0 + tid];
        tl[0] = v0.x; tl[1] = v0.y; tl[2] = v0.z; tl[3] = v0.w; tl[4] = v1.x; tl[5] = v1.y; tl[6] = v1.z; tl[7] = v1.w;
        tl[8] = v2.x; tl[9] = v2.y; tl[10] = v2.z; tl[11] = v2.w; tl[12] = v3.x; tl[13] = v3.y; tl[14] = v3.z; tl[15] = v3.w;
    }
    unsigned hb[8];
    {
        const uint4 *hp = (const uint4 *)(a.mhist + (size_t)b * 2048) + 2 * tid;
        const uint4 h0 = hp[0], h1 = hp[1];
        hb[0] = h0.x; hb[1] = h0.y; hb[2] = h0.z; hb[3] = h0.w; hb[4] = h1.x; hb[5] = h1.y; hb[6] = h1.z; hb[7] = h1.w;
    }
    if (tid < 32) s_sum[tid] = 0ull;
    if (tid < 3) s_flag[tid] = tid == 0 ? 1u : 0u;
    if (tid >= cnt) {  // not a selected line of this tile
        c0 = 0u;
#pragma unroll
        for (int q = 0; q < 16; ++q) tl[q] = INFINITY;
    }

    // ---- pick the bin of the rank among 2048 counts held 8 per lane (hb): exclusive scan over the workgroup,
    //      the lane whose range holds the rank reports (bin, rank inside, population).  Returns the total.
    auto pick_bin = [&](unsigned rank_or_none, bool have_rank) -> unsigned {
        unsigned tsum = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) tsum += hb[k];
        const unsigned incl = (unsigned)wave_incl_scan((int)tsum);
        __syncthreads();  // s_wtot / s_pick free again
        if (lane == 63) s_wtot[wave] = incl;
        __syncthreads();
        unsigned base = 0;
        for (int w = 0; w < wave; ++w) base += s_wtot[w];
        const unsigned total = s_wtot[0] + s_wtot[1] + s_wtot[2] + s_wtot[3];
        const unsigned rank = have_rank ? rank_or_none : (total ? (total - 1) / 2 : 0u);  // lower median: sorted[(n - 1) / 2]
        unsigned e = base + incl - tsum;
        if (rank >= e && rank < e + tsum) {  // exactly one lane (none when total == 0)
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (rank >= e && rank < e + hb[k]) { s_pick[0] = 8u * tid + k; s_pick[1] = rank - e; s_pick[2] = hb[k]; }
                e += hb[k];
            }
        }
        __syncthreads();
        return total;
    };
    const unsigned n = pick_bin(0u, false);
    if (n == 0) {  // nothing selected in this sample (the same for all its workgroups): loss 0, no bucket
        if (tile == 0) {
            if (tid < 16) a.bcnt_out[b * 16 + tid] = 0;
            if (tid < 32) a.bsum_out[(size_t)b * 32 + tid] = 0;
            if (tid == 0) {
                a.med_out[b] = 0.0f;
                a.loss[b] = 0.0f;
                a.info[b * 4 + 0] = 0; a.info[b * 4 + 1] = 0; a.info[b * 4 + 2] = 0; a.info[b * 4 + 3] = st0;
                if (chain_tmo) a.loss[b] = __builtin_nanf("");
                if (a.chain) *(uint4 *)(a.chain + RRL_CHAIN_WORDS * (size_t)b) = make_uint4(0u, 0u, 0u, 0u);
            }
        }
        return;
    }
    const unsigned bin = s_pick[0], r1 = s_pick[1], pop = s_pick[2];
    unsigned prefix = bin << 20;

    // rows of this tile beyond the 256 held in registers (a tile has more than 256 selected lines only when more
    // than a quarter of its lines are selected): re-read per phase
    auto for_extra_rows = [&](auto &&fn) {
        for (int i = tid + 256; i < cnt; i += 256) {
            const float4 *row = (const float4 *)(dc + (slot0 + i) * 16);
            float D_[16];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 v = row[q];
                D_[4 * q] = v.x; D_[4 * q + 1] = v.y; D_[4 * q + 2] = v.z; D_[4 * q + 3] = v.w;
            }
            fn(D_, (unsigned)kjc[slot0 + i]);
        }
    };

    // the remaining 20 bits when the bin is crowded (near-identical D values): this workgroup alone streams over ALL the
    // sample's values twice more (bits 19..9, 8..0); returns the median's bit pattern in every lane
    auto crowded_select = [&]() -> unsigned {
        unsigned pre = bin << 20, rk = r1;
        for (int pass = 1; pass <= 2; ++pass) {
            const int sh = pass == 1 ? 9 : 0, width = pass == 1 ? 11 : 9, hi = sh + width;
            const unsigned dmask = (1u << width) - 1u;
            __syncthreads();
            for (int i = tid; i < MCAND_CAP; i += 256) s_vals[i] = 0u;
            __syncthreads();
            for (int t = 0; t < nblk; ++t) {
                const int ct = a.blkcnt[(size_t)b * nblk + t];
                const float *base = dc + ((size_t)b * Lp + (size_t)t * 1024) * 16;
                for (int i = tid; i < ct * 16; i += 256) {
                    const unsigned x = __float_as_uint(base[i]);
                    if (x != 0x7f800000u && ((x ^ pre) >> hi) == 0u) atomicAdd(&s_vals[(x >> sh) & dmask], 1u);
                }
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < 8; ++k) hb[k] = s_vals[8 * tid + k];
            pick_bin(rk, true);
            pre |= s_pick[0] << sh;
            rk = s_pick[1];
        }
        return pre;
    };

    if (pop <= MCAND_CAP) {
        // ---- publish this tile's values of the bin, meet, read the whole list, finish the select
        auto in_bin = [&](unsigned x) { return x != 0x7f800000u && (x >> 20) == bin; };
        unsigned mine = 0;
#pragma unroll
        for (int q = 0; q < 16; ++q) mine += in_bin(__float_as_uint(tl[q])) ? 1u : 0u;
        for_extra_rows([&](const float *D_, unsigned) {
            for (int q = 0; q < 16; ++q) mine += in_bin(__float_as_uint(D_[q])) ? 1u : 0u;
        });
        const unsigned incl = (unsigned)wave_incl_scan((int)mine);
        unsigned wbase = 0;
        if (lane == 63 && incl) wbase = __hip_atomic_fetch_add(&ctl[RRL_MCTL_CURSOR], incl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        wbase = (unsigned)__builtin_amdgcn_readlane((int)wbase, 63);
        unsigned at = wbase + incl - mine;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const unsigned x = __float_as_uint(tl[q]);
            if (in_bin(x)) { if (at < MCAND_CAP) st_agent(&cand[at], x); ++at; }
        }
        for_extra_rows([&](const float *D_, unsigned) {
            for (int q = 0; q < 16; ++q) {
                const unsigned x = __float_as_uint(D_[q]);
                if (in_bin(x)) { if (at < MCAND_CAP) st_agent(&cand[at], x); ++at; }
            }
        });
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wavefront drains before the workgroup arrives
        __syncthreads();
        if (tid == 0) {  // the last to arrive learns it from its own ticket and does not poll at all
            const unsigned prev = __hip_atomic_fetch_add(&ctl[RRL_MCTL_TICK1], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (prev + 1u < (unsigned)nblk && !spin_reach(&ctl[RRL_MCTL_TICK1], (unsigned)nblk, a.spin_limit)) s_flag[0] = 0u;
        }
        __syncthreads();
        for (unsigned i = tid; i < pop; i += 256) s_vals[i] = ld_agent(&cand[i]);
        __syncthreads();
        if (tid < 64) {
            const unsigned m = wave_select20(s_vals, pop, prefix, r1, s_whist, tid);
            if (tid == 0) s_med = m;
        }
        __syncthreads();
        prefix = s_med;
    } else if (tile == 0) {
        // ---- crowded bin: this workgroup alone streams over ALL the sample's values twice more (bits 19..9, 8..0)
        prefix = crowded_select();
        if (tid == 0) {
            st_agent(&ctl[RRL_MCTL_MEDBITS], prefix);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            st_agent(&ctl[RRL_MCTL_MEDRDY], 1u);
        }
    } else {
        if (tid == 0) {
            if (!spin_reach(&ctl[RRL_MCTL_MEDRDY], 1u, a.spin_limit)) s_flag[0] = 0u;
            s_med = ld_agent(&ctl[RRL_MCTL_MEDBITS]);
        }
        __syncthreads();
        prefix = s_med;
    }
    float med = __uint_as_float(prefix);

    // ---- Welsch terms of this tile's lines into the workgroup's fixed-point sums (as reduce_core::accumulate)
    auto accumulate = [&](const float *Dl, int k, int j) {
        float row = 0.0f, col = 0.0f;
#pragma unroll
        for (int q = 0; q < RRL_MAX_HITS; ++q)
            if (q < k) row += welsch(fminf(fminf(Dl[q * 4], Dl[q * 4 + 1]), fminf(Dl[q * 4 + 2], Dl[q * 4 + 3])), med);
#pragma unroll
        for (int q = 0; q < RRL_MAX_HITS; ++q)
            if (q < j) col += welsch(fminf(fminf(Dl[q], Dl[4 + q]), fminf(Dl[8 + q], Dl[12 + q])), med);
        if (!(row <= 4.0f) || !(col <= 4.0f)) { atomicOr(&s_flag[2], 1u); row = col = 0.0f; }
        const int bi = (k - 1) * 4 + (j - 1);
        atomicAdd(&s_sum[bi * 2 + 0], (unsigned long long)((double)row * (double)(1ll << FIX_SHIFT) + 0.5));
        atomicAdd(&s_sum[bi * 2 + 1], (unsigned long long)((double)col * (double)(1ll << FIX_SHIFT) + 0.5));
    };
    const bool handoff_ok = s_flag[0] != 0u;  // uniform (written before the last barrier): false = a spin timed out: this
    if (handoff_ok) {                         // workgroup's median may be wrong -- it adds nothing; the last one repairs
        if (c0) accumulate(tl, (int)(c0 & 15u), (int)(c0 >> 4));
        for_extra_rows([&](const float *D_, unsigned c) { if (c) accumulate(D_, (int)(c & 15u), (int)(c >> 4)); });
    }
    __syncthreads();
    if (tid < 32) {
        const unsigned long long v = s_sum[tid];
        if (v) atomicAdd(&a.msum[(size_t)b * 32 + tid], v);
    }
    if (tid == 32 && (s_flag[2] || !s_flag[0])) {
        if (s_flag[2]) atomicOr(&ctl[RRL_MCTL_BAD], 1u);
        if (!s_flag[0]) atomicOr(&ctl[RRL_MCTL_ERR], 1u);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0)
        s_flag[1] = __hip_atomic_fetch_add(&ctl[RRL_MCTL_TICK2], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)(nblk - 1) ? 1u : 0u;
    __syncthreads();
    if (!s_flag[1]) return;

    // ---- the last workgroup of the sample.  A hand-off timed out somewhere (RRL_MCTL_ERR): recompute the sample alone.
    const bool repair = ld_agent(&ctl[RRL_MCTL_ERR]) != 0u;  // uniform: every producer's flag precedes its ticket
    if (repair) {
        __syncthreads();
        if (tid < 32) s_sum[tid] = 0ull;
        if (tid == 0) { s_flag[2] = 0u; s_flag[0] = 0u; }  // s_flag[0]: cursor of the gathered values
        __syncthreads();
        unsigned pre = bin << 20;
        if (pop <= MCAND_CAP) {  // the bin's values of ALL tiles into LDS (any order), then the wave-private passes
            for (int t = 0; t < nblk; ++t) {
                const int ct = a.blkcnt[(size_t)b * nblk + t];
                const float *base = dc + ((size_t)b * Lp + (size_t)t * 1024) * 16;
                for (int i = tid; i < ct * 16; i += 256) {
                    const unsigned x = __float_as_uint(base[i]);
                    if (x != 0x7f800000u && (x >> 20) == bin) {
                        const unsigned at = atomicAdd(&s_flag[0], 1u);
                        if (at < MCAND_CAP) s_vals[at] = x;
                    }
                }
            }
            __syncthreads();
            if (tid < 64) {
                const unsigned m = wave_select20(s_vals, pop, pre, r1, s_whist, tid);
                if (tid == 0) s_med = m;
            }
            __syncthreads();
            pre = s_med;
        } else {
            pre = crowded_select();
        }
        med = __uint_as_float(pre);
        for (int t = 0; t < nblk; ++t) {  // every selected line of the sample, the same per-line arithmetic
            const int ct = a.blkcnt[(size_t)b * nblk + t];
            const size_t s0 = (size_t)b * Lp + (size_t)t * 1024;
            for (int i = tid; i < ct; i += 256) {
                const float4 *row = (const float4 *)(dc + (s0 + i) * 16);
                float D_[16];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 v = row[q];
                    D_[4 * q] = v.x; D_[4 * q + 1] = v.y; D_[4 * q + 2] = v.z; D_[4 * q + 3] = v.w;
                }
                const unsigned c = kjc[s0 + i];
                if (c) accumulate(D_, (int)(c & 15u), (int)(c >> 4));
            }
        }
        __syncthreads();
        if (tid == 0) atomicAdd(&a.status[2], 1);
    }
    // loss = ( sum_{non-empty (k,j), k-major} exp(-|k-j|/2) (mean_row + mean_col) ) / C
    if (tid < 32) {
        const unsigned long long v = repair ? s_sum[tid]
                                            : __hip_atomic_load(&a.msum[(size_t)b * 32 + tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_sum[tid] = v;
        a.bsum_out[(size_t)b * 32 + tid] = (int64_t)v;
        __hip_atomic_store(&a.msum[(size_t)b * 32 + tid], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // a second reduce on this state starts clean
    }
    static_assert(RRL_MCTL_BUCKET0 == 0 && RRL_MCTL_BAD < 32, "lanes 32 .. 63 read words 0 .. 31: the sixteen buckets first");
    if (tid >= 32 && tid < 64) {  // the sample's control words in the same round of loads: bucket counts, error / bad flags
        const unsigned v = ld_agent(&ctl[tid - 32]);
        if (tid < 48) {
            s_cnt[tid - 32] = (int)v;
            a.bcnt_out[b * 16 + tid - 32] = (int)v;
        } else if (tid - 32 == RRL_MCTL_BAD && !repair) {
            if (v) atomicOr(&s_flag[2], 2u);  // (s_flag[2] bit 0 was this workgroup's own; bit 1: anyone's)
        }
    }
    __syncthreads();
    if (tid >= 64) return;  // wavefront 0: one lane per bucket (bucket_final)
    const BucketFinal f = bucket_final(tid < 16 ? s_sum[tid * 2 + 0] : 0ull, tid < 16 ? s_sum[tid * 2 + 1] : 0ull,
                                       tid < 16 ? s_cnt[tid] : 0, tid, a.s_m, a.s_n, a.e_m, a.e_n);
    if (tid == 0) {
        const float acc = f.acc;
        const int C = f.C, nselected = f.nselected, nvalues = f.nvalues;
        const bool bad = repair ? (s_flag[2] & 1u) != 0u : (s_flag[2] & 2u) != 0u;  // a non-finite Welsch term (median 0)
        const float lv = bad || chain_tmo ? __builtin_nanf("") : (C ? acc / (float)C : 0.0f);  // code/loss.py:230
        a.med_out[b] = med;
        a.loss[b] = lv;
        a.info[b * 4 + 0] = C;
        a.info[b * 4 + 1] = nselected;
        a.info[b * 4 + 2] = nvalues;
        a.info[b * 4 + 3] = st0;
        if (a.chain) *(uint4 *)(a.chain + RRL_CHAIN_WORDS * (size_t)b) = make_uint4(0u, 0u, 0u, 0u);  // the next chained step finds them cleared
        st_agent(&ctl[RRL_MCTL_CURSOR], 0u); st_agent(&ctl[RRL_MCTL_TICK1], 0u); st_agent(&ctl[RRL_MCTL_TICK2], 0u);
        st_agent(&ctl[RRL_MCTL_MEDRDY], 0u); st_agent(&ctl[RRL_MCTL_BAD], 0u); st_agent(&ctl[RRL_MCTL_ERR], 0u);
        if (a.payload && C > 0) tiled_payload(a.payload, a.mctl, lv);  // (order-independent: tail_payload)
    }
}

