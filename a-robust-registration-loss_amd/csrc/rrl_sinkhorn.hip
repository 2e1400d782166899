// rrl_sinkhorn.hip -- RPM's match head on the device (include/rrl.h rrl_sinkhorn_fwd / rrl_sinkhorn_bwd; DESIGN.md section
// 17): log-domain Sinkhorn normalisation with slack (rpm/models/rpmnet.py:48-118) as a dual-potential iteration, and the
// soft correspondences taken from it (rpmnet.py:214-222), with their gradient.  The normalised matrix is never stored:
//   u^{t+1}[j] = log(sum_k exp(A[j][k] - v^t[k]) + sigma),   v^{t+1}[k] = log(sum_j exp(A[j][k] - u^{t+1}[j]) + sigma),
//   P = exp(A - u^n - v^n),   s = sum_k P,   c = sum_j P,   N = sum_k P x,   W = N / (s + eps).
// Every pass over A is one of two shapes.  A ROW pass gives one wavefront a row: lanes stride the contiguous k, the lanes
// are merged by a fixed butterfly.  A COLUMN pass gives a 256-lane workgroup 64 columns x SK_CROWS rows: a lane owns a
// column, its wavefront shares the row (so loads stay coalesced and the row's scalars are wave-uniform), the four
// wavefronts are merged in order into one partial per (column, row slice), and a finish launch adds the slices in index
// order.  Each half-iteration is its own launch: it needs the complete result of the one before.
//
// The arithmetic rule: potentials, adjoint vectors and every sum are double; a matrix term is sk_exp(double(A) - u - v), the
// exponential of the DOUBLE argument good to 2^-36 -- neither A nor the difference is rounded to float32 before or after the
// cancellation (an expf of the rounded difference, one ulp off on a dominant entry, measured up to 3.5 x the deviation of
// torch's float32 evaluation from a float64 twin); logsumexp runs under a running maximum; lanes, then wavefronts, then
// slices, all in a fixed order; no atomics.  Results are rounded to float32 once.  Same bits on every call.
// Nothing indexes by data: a NaN or +inf entry can only spread as a value, and sets info[b].
#include <cstddef>
#include <cstdint>

#include "rrl_common.h"
#include "rrl_wave_sum_d.h"

#define SK_MAX_DIM 16384  // J, K of one call (a 1 GiB matrix per sample)
#define SK_MAX_ITERS 64
#define SK_CROWS 128      // rows of A per workgroup of a column pass: ceil(J / 128) slices per column
#define SK_PART 4         // doubles per (column, slice) partial
#define SK_AROWS 8        // rows per wavefront of the assembly pass (32 per workgroup)

struct SkArgs {
    int B, J, K, n, slack, nsplit;
    const float *A, *x;
    const int32_t *cs, *cr;
    double eps;
    double *U, *V, *UB, *VB;  // [B][n + 1][J or K]: potentials u^t, v^t and their adjoints (slot 0 of U, UB, VB unused; v^0 = 0)
    double *SD, *ND, *GR;     // [B][J], [B][J][3], [B][J][4]: s and N in double; the backward's row scalars (gs', gN)
    double *PART;             // [B][nsplit][K][SK_PART]
    float *W, *s, *c, *logp;
    int32_t *info;
    const float *gW, *gs, *gc;  // backward
    float *gA, *gx;
};

__device__ __forceinline__ size_t sk_hist(const SkArgs &a, int b, int t, int len) { return ((size_t)b * (a.n + 1) + t) * (size_t)len; }

// exp(x) for a double x, good to 2^-36 (the Taylor remainder of degree 9 on |r| <= ln 2 / 2 is at most 1.0e-11 of the value): the
// argument is reduced in double and never rounded to float32, and the polynomial is a dozen double FMAs -- a third of the
// library routine, which these passes would otherwise be bound by.  -inf (and anything below the double range) gives 0, NaN
// stays NaN, exp(0) is exactly 1.
__device__ __forceinline__ double sk_exp(double x) {
    if (!(x > -708.0)) return x != x ? x : 0.0;
    if (x > 709.0) return (double)INFINITY;
    const double t = fma(x, 1.4426950408889634, 6755399441055744.0);  // + 1.5 2^52: the integer k = rint(x log2 e) sits in the low word
    const double k = t - 6755399441055744.0;
    double r = fma(-k, 6.93147180369123816490e-01, x);
    r = fma(-k, 1.90821492927058770002e-10, r);
    double p = 1.0 / 362880.0;
    p = fma(p, r, 1.0 / 40320.0);
    p = fma(p, r, 1.0 / 5040.0);
    p = fma(p, r, 1.0 / 720.0);
    p = fma(p, r, 1.0 / 120.0);
    p = fma(p, r, 1.0 / 24.0);
    p = fma(p, r, 1.0 / 6.0);
    p = fma(p, r, 0.5);
    p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);
    return __hiloint2double(__double2hiint(p) + (__double2loint(t) << 20), __double2loint(p));  // p 2^k, k in [-1021, 1023]: normal
}

// (m, s) <- the logsumexp state of both: sum = s exp(m); an empty state is (-inf, 0) and changes nothing, bit for bit
__device__ __forceinline__ void lse_merge(double &m, double &s, double m2, double s2) {
    const double M = fmax(m, m2);
    if (M == -INFINITY) {
        s = 0.0;
        return;
    }
    s = s * sk_exp(m - M) + s2 * sk_exp(m2 - M);
    m = M;
}

// four terms of a running logsumexp: x[i] = -inf is an absent (or excluded) term
__device__ __forceinline__ void lse_add4(double &m, double &s, const double (&x)[4]) {
    const double cm = fmax(fmax(x[0], x[1]), fmax(x[2], x[3]));
    if (cm > m) {
        s *= sk_exp(m - cm);
        m = cm;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (x[i] > -INFINITY) s += sk_exp(x[i] - m);
}

// log(s exp(m) + sigma)
__device__ __forceinline__ double lse_close(double m, double s, int slack) {
    const double M = slack ? fmax(m, 0.0) : m;
    if (M == -INFINITY) return -INFINITY;
    return M + log(s * sk_exp(m - M) + (slack ? sk_exp(-M) : 0.0));
}

// ---- row passes: grid (ceil(J / 4), B), one wavefront per row -----------------------------------------------------------
// u^{t+1} from v^t
__global__ __launch_bounds__(256) void sk_row_lse_kernel(const SkArgs a, int t) {
    const int lane = threadIdx.x & 63, j = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
    const int cs = rrl_rows(a.cs, b, a.J), cr = rrl_rows(a.cr, b, a.K);
    if (j >= cs) return;  // (wave-uniform; the kernel has no barrier)
    const float *__restrict__ row = a.A + ((size_t)b * a.J + j) * a.K;
    const double *__restrict__ v = t > 0 ? a.V + sk_hist(a, b, t, a.K) : nullptr;
    double m = -INFINITY, s = 0.0;
    bool bad = false;
    for (int k0 = 0; k0 < cr; k0 += 256) {
        double x[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = k0 + i * 64 + lane;
            x[i] = -INFINITY;
            if (k < cr) {
                double xa = (double)row[k];
                if (v) xa -= v[k];
                bad = bad || !(xa < (double)INFINITY);
                if (xa < (double)INFINITY) x[i] = xa;
            }
        }
        lse_add4(m, s, x);
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) lse_merge(m, s, __shfl_xor(m, off), __shfl_xor(s, off));
    if (lane == 0) a.U[sk_hist(a, b, t + 1, a.J) + j] = lse_close(m, s, a.slack);
    if (bad) a.info[b] = 1;
}

// s, N, W (and log_perm) from u^n, v^n; rows beyond the count get zeros
__global__ __launch_bounds__(256) void sk_row_out_kernel(const SkArgs a) {
    const int lane = threadIdx.x & 63, j = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
    if (j >= a.J) return;
    const int cs = rrl_rows(a.cs, b, a.J), cr = rrl_rows(a.cr, b, a.K);
    const size_t at = (size_t)b * a.J + j;
    float *__restrict__ lp = a.logp ? a.logp + at * a.K : nullptr;
    if (j >= cs) {
        if (lane == 0) {
            a.s[at] = 0.0f;
            a.W[at * 3] = a.W[at * 3 + 1] = a.W[at * 3 + 2] = 0.0f;
        }
        if (lp)
            for (int k = lane; k < a.K; k += 64) lp[k] = -INFINITY;
        return;
    }
    const float *__restrict__ row = a.A + at * a.K;
    const float *__restrict__ xr = a.x + (size_t)b * a.K * 3;
    const double *__restrict__ v = a.n > 0 ? a.V + sk_hist(a, b, a.n, a.K) : nullptr;
    const double u = a.n > 0 ? a.U[sk_hist(a, b, a.n, a.J) + j] : 0.0;
    double s = 0.0, n0 = 0.0, n1 = 0.0, n2 = 0.0;
    bool bad = false;
    for (int k = lane; k < cr; k += 64) {
        double xa = (double)row[k] - u;
        if (v) xa -= v[k];
        bad = bad || !(xa < (double)INFINITY);
        const double p = sk_exp(xa);
        s += p;
        n0 += p * (double)xr[3 * k];
        n1 += p * (double)xr[3 * k + 1];
        n2 += p * (double)xr[3 * k + 2];
        if (lp) lp[k] = (float)xa;
    }
    if (lp)
        for (int k = cr + lane; k < a.K; k += 64) lp[k] = -INFINITY;
    s = wave_sum_d(s);
    n0 = wave_sum_d(n0);
    n1 = wave_sum_d(n1);
    n2 = wave_sum_d(n2);
    if (lane == 0) {
        const double den = s + a.eps;
        a.SD[at] = s;
        a.ND[at * 3] = n0;
        a.ND[at * 3 + 1] = n1;
        a.ND[at * 3 + 2] = n2;
        a.s[at] = (float)s;
        a.W[at * 3] = (float)(n0 / den);
        a.W[at * 3 + 1] = (float)(n1 / den);
        a.W[at * 3 + 2] = (float)(n2 / den);
    }
    if (bad) a.info[b] = 1;
}

// backward, first row pass: the row scalars gN = gW / (s + eps), gs' = gs - (gW . W) / (s + eps) -> GR, and
// ubar^n[j] = -sum_k P (gs' + gc[k] + gN . x[k])
__global__ __launch_bounds__(256) void sk_row_first_kernel(const SkArgs a) {
    const int lane = threadIdx.x & 63, j = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
    const int cs = rrl_rows(a.cs, b, a.J), cr = rrl_rows(a.cr, b, a.K);
    if (j >= cs) return;
    const size_t at = (size_t)b * a.J + j;
    const double den = a.SD[at] + a.eps;
    double gn[3], dot = 0.0;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const double gw = a.gW ? (double)a.gW[at * 3 + q] : 0.0;
        gn[q] = gw / den;
        dot += gw * (a.ND[at * 3 + q] / den);
    }
    const double gsp = (a.gs ? (double)a.gs[at] : 0.0) - dot / den;
    if (lane == 0) {
        a.GR[at * 4] = gsp;
        a.GR[at * 4 + 1] = gn[0];
        a.GR[at * 4 + 2] = gn[1];
        a.GR[at * 4 + 3] = gn[2];
    }
    const float *__restrict__ row = a.A + at * a.K;
    const float *__restrict__ xr = a.x + (size_t)b * a.K * 3;
    const float *__restrict__ gc = a.gc ? a.gc + (size_t)b * a.K : nullptr;
    const double *__restrict__ v = a.n > 0 ? a.V + sk_hist(a, b, a.n, a.K) : nullptr;
    const double u = a.n > 0 ? a.U[sk_hist(a, b, a.n, a.J) + j] : 0.0;
    double acc = 0.0;
    for (int k = lane; k < cr; k += 64) {
        double xa = (double)row[k] - u;
        if (v) xa -= v[k];
        const double p = sk_exp(xa);
        const double g = (gsp + (gc ? (double)gc[k] : 0.0)) +
                         ((gn[0] * (double)xr[3 * k] + gn[1] * (double)xr[3 * k + 1]) + gn[2] * (double)xr[3 * k + 2]);
        acc += p * g;
    }
    acc = wave_sum_d(acc);
    if (lane == 0) a.UB[sk_hist(a, b, a.n, a.J) + j] = -acc;
}

// backward through v^{tt} = g(A, u^{tt}): ubar^{tt}[j] -= sum_k vbar^{tt}[k] exp(A - u^{tt}[j] - v^{tt}[k])   (tt = n .. 1;
// ubar^{tt} starts from the first pass for tt = n, from 0 otherwise)
__global__ __launch_bounds__(256) void sk_row_adj_kernel(const SkArgs a, int tt) {
    const int lane = threadIdx.x & 63, j = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
    const int cs = rrl_rows(a.cs, b, a.J), cr = rrl_rows(a.cr, b, a.K);
    if (j >= cs) return;
    const float *__restrict__ row = a.A + ((size_t)b * a.J + j) * a.K;
    const double *__restrict__ v = a.V + sk_hist(a, b, tt, a.K);
    const double *__restrict__ vb = a.VB + sk_hist(a, b, tt, a.K);
    const size_t uat = sk_hist(a, b, tt, a.J) + j;
    const double u = a.U[uat];
    double acc = 0.0;
    for (int k = lane; k < cr; k += 64) acc += vb[k] * sk_exp(((double)row[k] - u) - v[k]);
    acc = wave_sum_d(acc);
    if (lane == 0) a.UB[uat] = (tt == a.n ? a.UB[uat] : 0.0) - acc;
}

// ---- column passes: grid (ceil(K / 64), nsplit, B) -> PART; then sk_col_finish_kernel, grid (ceil(K / 256), B) ----------
enum { SK_C_LSE = 0, SK_C_SUM = 1, SK_C_FIRST = 2, SK_C_ADJ = 3 };
// LSE:   v^{t+1} from u^{t+1}                                       (partial: m, s)
// SUM:   c = sum_j P at n = 0                                        (partial: sum)
// FIRST: gx = sum_j P gN[j], vbar^n = -sum_j P G                     (partial: 3 + 1 sums)
// ADJ:   vbar^t[k] = -sum_j ubar^{t+1}[j] exp(A - u^{t+1}[j] - v^t[k])   (t = n - 1 .. 1; partial: sum)
template <int MODE>
__global__ __launch_bounds__(256) void sk_col_kernel(const SkArgs a, int t) {
    __shared__ double s_red[4][64][SK_PART];
    const int tx = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int k = blockIdx.x * 64 + tx, sp = blockIdx.y, b = blockIdx.z;
    const int cs = rrl_rows(a.cs, b, a.J), cr = rrl_rows(a.cr, b, a.K);
    const int r0 = sp * SK_CROWS, r1 = min(r0 + SK_CROWS, cs);
    const bool live = k < cr;
    const float *__restrict__ col = a.A + (size_t)b * a.J * a.K + k;
    const int tu = MODE == SK_C_LSE || MODE == SK_C_ADJ ? t + 1 : a.n;  // which u
    const int tv = MODE == SK_C_ADJ ? t : a.n;                          // which v (LSE: none)
    const double *__restrict__ u = tu > 0 ? a.U + sk_hist(a, b, tu, a.J) : nullptr;
    const double *__restrict__ ub = MODE == SK_C_ADJ ? a.UB + sk_hist(a, b, t + 1, a.J) : nullptr;
    const double *__restrict__ gr = a.GR + (size_t)b * a.J * 4;
    const double vk = (MODE != SK_C_LSE && tv > 0 && live) ? a.V[sk_hist(a, b, tv, a.K) + k] : 0.0;
    double acc[SK_PART] = {MODE == SK_C_LSE ? -INFINITY : 0.0, 0.0, 0.0, 0.0};
    double gck = 0.0, xk[3] = {0.0, 0.0, 0.0};
    if (MODE == SK_C_FIRST && live) {
        gck = a.gc ? (double)a.gc[(size_t)b * a.K + k] : 0.0;
#pragma unroll
        for (int q = 0; q < 3; ++q) xk[q] = (double)a.x[((size_t)b * a.K + k) * 3 + q];
    }
    bool bad = false;
    if (live) {
        for (int j0 = r0 + wave; j0 < r1; j0 += 16) {
            double x[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int j = j0 + 4 * i;
                x[i] = -INFINITY;
                if (j < r1) {
                    const double xa = ((double)col[(size_t)j * a.K] - (u ? u[j] : 0.0)) - vk;
                    if (MODE == SK_C_LSE) {
                        bad = bad || !(xa < (double)INFINITY);
                        if (xa < (double)INFINITY) x[i] = xa;
                    } else {
                        x[i] = xa;
                    }
                }
            }
            if (MODE == SK_C_LSE) {
                lse_add4(acc[0], acc[1], x);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int j = j0 + 4 * i;
                    if (j >= r1) continue;
                    const double p = sk_exp(x[i]);
                    if (MODE == SK_C_SUM) acc[0] += p;
                    if (MODE == SK_C_ADJ) acc[0] += ub[j] * p;
                    if (MODE == SK_C_FIRST) {
                        const double g0 = gr[4 * j], g1 = gr[4 * j + 1], g2 = gr[4 * j + 2], g3 = gr[4 * j + 3];
                        acc[0] += p * g1;
                        acc[1] += p * g2;
                        acc[2] += p * g3;
                        acc[3] += p * ((g0 + gck) + ((g1 * xk[0] + g2 * xk[1]) + g3 * xk[2]));
                    }
                }
            }
        }
    }
    if (bad) a.info[b] = 1;
#pragma unroll
    for (int q = 0; q < SK_PART; ++q) s_red[wave][tx][q] = acc[q];
    __syncthreads();
    if (threadIdx.x >= 64 || !live) return;
    double tot[SK_PART];
#pragma unroll
    for (int q = 0; q < SK_PART; ++q) tot[q] = s_red[0][tx][q];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
        if (MODE == SK_C_LSE) {
            lse_merge(tot[0], tot[1], s_red[w][tx][0], s_red[w][tx][1]);
        } else {
#pragma unroll
            for (int q = 0; q < SK_PART; ++q) tot[q] += s_red[w][tx][q];
        }
    }
    double *__restrict__ out = a.PART + (((size_t)b * a.nsplit + sp) * a.K + k) * SK_PART;
#pragma unroll
    for (int q = 0; q < SK_PART; ++q) out[q] = tot[q];
}

template <int MODE>
__global__ __launch_bounds__(256) void sk_col_finish_kernel(const SkArgs a, int t) {
    const int k = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (k >= a.K) return;
    const bool live = k < rrl_rows(a.cr, b, a.K);
    double tot[SK_PART] = {MODE == SK_C_LSE ? -INFINITY : 0.0, 0.0, 0.0, 0.0};
    if (live) {
        for (int sp = 0; sp < a.nsplit; ++sp) {
            const double *__restrict__ p = a.PART + (((size_t)b * a.nsplit + sp) * a.K + k) * SK_PART;
            if (MODE == SK_C_LSE) {
                lse_merge(tot[0], tot[1], p[0], p[1]);
            } else {
#pragma unroll
                for (int q = 0; q < SK_PART; ++q) tot[q] += p[q];
            }
        }
    }
    const size_t at = (size_t)b * a.K + k;
    if (MODE == SK_C_LSE) {
        const double v = live ? lse_close(tot[0], tot[1], a.slack) : 0.0;
        a.V[sk_hist(a, b, t + 1, a.K) + k] = v;
        // the last half-iteration has the column sum already: c = sum_j exp(A - u^n) / exp(v^n)
        if (t + 1 == a.n) a.c[at] = (live && tot[1] > 0.0) ? (float)(tot[1] * sk_exp(tot[0] - v)) : 0.0f;
    }
    if (MODE == SK_C_SUM) a.c[at] = (float)tot[0];
    if (MODE == SK_C_ADJ) a.VB[sk_hist(a, b, t, a.K) + k] = -tot[0];
    if (MODE == SK_C_FIRST) {
        a.VB[sk_hist(a, b, a.n, a.K) + k] = -tot[3];
        if (a.gx) {
            a.gx[at * 3] = (float)tot[0];
            a.gx[at * 3 + 1] = (float)tot[1];
            a.gx[at * 3 + 2] = (float)tot[2];
        }
    }
}

// ---- the assembly pass: grid (ceil(K / 64), ceil(J / 32), B); one read of A, one write of dA ------------------------------
// dA[j][k] = P G + sum_{tt = 1 .. n} ( vbar^{tt}[k] exp(A - u^{tt}[j] - v^{tt}[k]) + ubar^{tt}[j] exp(A - u^{tt}[j] - v^{tt-1}[k]) ),
// a lane holding SK_AROWS entries of its column so that the column's vectors are loaded once per eight entries; the terms of
// an entry are added in the order tt = 1 .. n, P G last.  Entries beyond the counts are written as 0 and never read.
__global__ __launch_bounds__(256) void sk_assemble_kernel(const SkArgs a) {
    const int tx = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int k = blockIdx.x * 64 + tx, b = blockIdx.z;
    const int j0 = blockIdx.y * (4 * SK_AROWS) + wave * SK_AROWS;
    if (k >= a.K || j0 >= a.J) return;  // (no barrier below)
    const int cs = rrl_rows(a.cs, b, a.J), cr = rrl_rows(a.cr, b, a.K);
    const size_t base = (size_t)b * a.J * a.K + k;
    const bool live = k < cr;
    double av[SK_AROWS], acc[SK_AROWS];
#pragma unroll
    for (int r = 0; r < SK_AROWS; ++r) {
        const int j = j0 + r;
        av[r] = (live && j < cs) ? (double)a.A[base + (size_t)j * a.K] : 0.0;
        acc[r] = 0.0;
    }
    if (live) {
        double vprev = 0.0;
        for (int tt = 1; tt <= a.n; ++tt) {
            const double vk = a.V[sk_hist(a, b, tt, a.K) + k], vbk = a.VB[sk_hist(a, b, tt, a.K) + k];
            const double *__restrict__ u = a.U + sk_hist(a, b, tt, a.J);
            const double *__restrict__ ub = a.UB + sk_hist(a, b, tt, a.J);
#pragma unroll
            for (int r = 0; r < SK_AROWS; ++r) {
                const int j = j0 + r;
                if (j >= cs) continue;
                const double d = av[r] - u[j];
                if (tt < a.n) acc[r] += vbk * sk_exp(d - vk);  // (tt = n: folded into P G below)
                acc[r] += ub[j] * sk_exp(d - vprev);
            }
            vprev = vk;
        }
        const double vbn = a.n > 0 ? a.VB[sk_hist(a, b, a.n, a.K) + k] : 0.0;
        const double *__restrict__ un = a.n > 0 ? a.U + sk_hist(a, b, a.n, a.J) : nullptr;
        const double gck = a.gc ? (double)a.gc[(size_t)b * a.K + k] : 0.0;
        const float *__restrict__ xr = a.x + ((size_t)b * a.K + k) * 3;
        const double x0 = (double)xr[0], x1 = (double)xr[1], x2 = (double)xr[2];
#pragma unroll
        for (int r = 0; r < SK_AROWS; ++r) {
            const int j = j0 + r;
            if (j >= cs) continue;
            const double *__restrict__ gr = a.GR + ((size_t)b * a.J + j) * 4;
            const double g = (gr[0] + gck) + ((gr[1] * x0 + gr[2] * x1) + gr[3] * x2);
            const double p = sk_exp((av[r] - (un ? un[j] : 0.0)) - vprev);
            acc[r] += (g + vbn) * p;
        }
    }
#pragma unroll
    for (int r = 0; r < SK_AROWS; ++r) {
        const int j = j0 + r;
        if (j < a.J) a.gA[base + (size_t)j * a.K] = (live && j < cs) ? (float)acc[r] : 0.0f;
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------
static size_t sk_layout(int B, int J, int K, int n, size_t (&off)[8]) {
    const size_t b = (size_t)B, j = (size_t)J, k = (size_t)K, h = (size_t)n + 1, nsplit = (j + SK_CROWS - 1) / SK_CROWS;
    const size_t len[8] = {b * h * j, b * h * k, b * h * j, b * h * k, b * j, b * j * 3, b * j * 4, b * nsplit * k * SK_PART};
    size_t at = 0;
    for (int i = 0; i < 8; ++i) {
        off[i] = at;
        at += len[i];
    }
    return at * sizeof(double);
}

extern "C" size_t rrl_sinkhorn_workspace_bytes(int B, int J, int K, int n_iters) {
    if (B < 1 || B > 32767 || J < 1 || K < 1 || J > SK_MAX_DIM || K > SK_MAX_DIM || n_iters < 0 || n_iters > SK_MAX_ITERS) return 0;
    size_t off[8];
    return sk_layout(B, J, K, n_iters, off);
}

// every refusal of both entries; 0: `k` is filled
static int sk_check(const rrl_sinkhorn_args *p, SkArgs &k) {
    if (!p || p->struct_bytes != (int32_t)sizeof(rrl_sinkhorn_args)) return RRL_E_ARG;
    if (p->B < 1 || p->B > 32767 || p->J < 1 || p->K < 1 || p->J > SK_MAX_DIM || p->K > SK_MAX_DIM) return RRL_E_ARG;
    if (p->n_iters < 0 || p->n_iters > SK_MAX_ITERS) return RRL_E_ARG;
    if (!p->log_alpha || !p->xyz_ref || !p->ws || !p->W || !p->s || !p->c || !p->info || (((uintptr_t)p->ws) & 7) != 0) return RRL_E_ARG;
    size_t off[8];
    if (p->ws_bytes < sk_layout(p->B, p->J, p->K, p->n_iters, off)) return RRL_E_WS;
    double *w = (double *)p->ws;
    k = {};
    k.B = p->B; k.J = p->J; k.K = p->K; k.n = p->n_iters; k.slack = p->slack != 0; k.nsplit = (p->J + SK_CROWS - 1) / SK_CROWS;
    k.A = p->log_alpha; k.x = p->xyz_ref; k.cs = p->count_src; k.cr = p->count_ref; k.eps = p->eps;
    k.U = w + off[0]; k.V = w + off[1]; k.UB = w + off[2]; k.VB = w + off[3]; k.SD = w + off[4]; k.ND = w + off[5]; k.GR = w + off[6];
    k.PART = w + off[7];
    k.W = p->W; k.s = p->s; k.c = p->c; k.logp = p->log_perm; k.info = p->info;
    return 0;
}

template <int MODE>
static void sk_col_pass(const SkArgs &k, int t, hipStream_t st) {
    hipLaunchKernelGGL(sk_col_kernel<MODE>, dim3((unsigned)((k.K + 63) / 64), (unsigned)k.nsplit, (unsigned)k.B), dim3(256), 0, st, k, t);
    hipLaunchKernelGGL(sk_col_finish_kernel<MODE>, dim3((unsigned)((k.K + 255) / 256), (unsigned)k.B), dim3(256), 0, st, k, t);
}

extern "C" int rrl_sinkhorn_fwd(const rrl_sinkhorn_args *p, void *stream) {
    SkArgs k;
    if (const int rc = sk_check(p, k)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const dim3 rows((unsigned)((k.J + 3) / 4), (unsigned)k.B);
    if (hipError_t e = hipMemsetAsync(k.info, 0, sizeof(int32_t) * (size_t)k.B, st)) return (int)e;
    for (int t = 0; t < k.n; ++t) {
        hipLaunchKernelGGL(sk_row_lse_kernel, rows, dim3(256), 0, st, k, t);
        sk_col_pass<SK_C_LSE>(k, t, st);
    }
    hipLaunchKernelGGL(sk_row_out_kernel, rows, dim3(256), 0, st, k);
    if (k.n == 0) sk_col_pass<SK_C_SUM>(k, 0, st);
    RRL_LAUNCH_CHECK();
    return 0;
}

extern "C" int rrl_sinkhorn_bwd(const rrl_sinkhorn_args *p, const float *gW, const float *gs, const float *gc, float *g_log_alpha,
                                float *g_xyz_ref, void *stream) {
    SkArgs k;
    if (const int rc = sk_check(p, k)) return rc;
    if (!g_log_alpha) return RRL_E_ARG;
    k.gW = gW; k.gs = gs; k.gc = gc; k.gA = g_log_alpha; k.gx = g_xyz_ref;
    hipStream_t st = (hipStream_t)stream;
    const dim3 rows((unsigned)((k.J + 3) / 4), (unsigned)k.B);
    hipLaunchKernelGGL(sk_row_first_kernel, rows, dim3(256), 0, st, k);
    sk_col_pass<SK_C_FIRST>(k, 0, st);
    for (int tt = k.n; tt >= 1; --tt) {
        hipLaunchKernelGGL(sk_row_adj_kernel, rows, dim3(256), 0, st, k, tt);
        if (tt > 1) sk_col_pass<SK_C_ADJ>(k, tt - 1, st);
    }
    hipLaunchKernelGGL(sk_assemble_kernel, dim3((unsigned)((k.K + 63) / 64), (unsigned)((k.J + 4 * SK_AROWS - 1) / (4 * SK_AROWS)), (unsigned)k.B),
                       dim3(256), 0, st, k);
    RRL_LAUNCH_CHECK();
    return 0;
}
