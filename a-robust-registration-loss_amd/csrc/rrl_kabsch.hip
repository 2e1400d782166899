// rrl_kabsch.hip -- closed-form rigid fits on the device (include/rrl.h rrl_kabsch_fwd, rrl_kabsch_bwd, rrl_icp_step_batch,
// rrl_icp_epoch): the weighted Kabsch solve every trainer of this loss ends in
// (rpm/models/rpmnet.py:121-157 compute_rigid_transform, dcp/model.py:405-455 SVDHead), batched, ragged, from dense pairs or
// from the keys a Chamfer walk left -- and, around the keyed form, one epoch of point-to-point ICP as one C call.
//
// The arithmetic rule: every sum is a fixed-order double sum (kabsch_part_kernel has pose_normal_eq_kernel's shape, and its
// block sum, rrl_pair_sums.h: per-lane double accumulators, wave_sum_d, four wavefronts, one partial row per workgroup, no
// atomics; the pair walk and the total of the partial rows sit there too, shared with rrl_plane.hip), and everything after the
// sums -- H, its SVD, delta, R, T -- is double on one lane, rounded to float32 once.
#include <cstddef>
#include <cstdint>

#include "rrl_ws.h"
#include "rrl_pose_tail.h"
#include "rrl_pair_sums.h"
#include "rrl_cloud_epoch.h"
#include "rrl_icp_step.h"

#define KB_ROWS 512  // rows of `a` per 256-lane workgroup (two rounds)
// the sums of a sample, about the pivots pa, pb (q = a - pa, r = b - pb): sum w, sum w q (3), sum w r (3), sum w q^T r (9),
// sum w |q|^2, sum w |r|^2, sum w (key distance word), pairs used, pairs skipped
enum { KB_W = 0, KB_Q = 1, KB_R = 4, KB_QR = 7, KB_QQ = 16, KB_RR = 17, KB_KD = 18, KB_USED = 19, KB_SKIP = 20, KB_SUMS = 21 };

struct KabschArgs {
    int B, n, m, sa, sb, transpose_r;
    const float *a, *b, *w;
    const unsigned long long *keys;
    const int32_t *count_a, *count_b;
    const float *gate_sq;
    double eps_w;
    float rank_tol;
    double *part;
    float *R, *T;
    double *fit;
    int32_t *info;
};

// the sample's pivot: row 0 of a cloud as doubles (a non-finite coordinate -- filler of an empty sample -- pivots at 0)
__device__ __forceinline__ void kabsch_pivot(const float *__restrict__ row, double (&p)[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v = row[c];
        p[c] = fabsf(v) < INFINITY ? (double)v : 0.0;
    }
}

template <int P, int Q>
__device__ __forceinline__ bool jacobi_pair(double (&A)[3][3], double (&V)[3][3]) {
    const double al = A[0][P] * A[0][P] + A[1][P] * A[1][P] + A[2][P] * A[2][P];
    const double be = A[0][Q] * A[0][Q] + A[1][Q] * A[1][Q] + A[2][Q] * A[2][Q];
    const double ga = A[0][P] * A[0][Q] + A[1][P] * A[1][Q] + A[2][P] * A[2][Q];
    if (ga == 0.0 || !(fabs(ga) > 1e-17 * sqrt(al * be))) return false;  // (orthogonal to rounding, or not a number)
    const double zeta = (be - al) / (2.0 * ga);
    const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double x = A[i][P], y = A[i][Q];
        A[i][P] = c * x - s * y;
        A[i][Q] = s * x + c * y;
        const double vx = V[i][P], vy = V[i][Q];
        V[i][P] = c * vx - s * vy;
        V[i][Q] = s * vx + c * vy;
    }
    return true;
}

template <int P, int Q>
__device__ __forceinline__ void swap_cols(double (&A)[3][3], double (&V)[3][3], double (&s)[3]) {
    if (s[P] < s[Q]) {
        const double t = s[P]; s[P] = s[Q]; s[Q] = t;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double x = A[i][P]; A[i][P] = A[i][Q]; A[i][Q] = x;
            const double y = V[i][P]; V[i][P] = V[i][Q]; V[i][Q] = y;
        }
    }
}

__device__ __forceinline__ double det3(const double (&M)[3][3]) {
    return M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) +
           M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]);
}

// H = U diag(s) V^T, s descending and non-negative, U and V orthonormal (their determinants may be -1), by one-sided Jacobi
// rotations of the columns of A = H V: small singular values keep their relative accuracy.  A fixed bound of sweeps (a 3 x 3
// matrix converges in five or six).  Columns of U that H does not determine (s_j = 0) are completed to an orthonormal basis.
__device__ void svd3(const double (&H)[3][3], double (&U)[3][3], double (&s)[3], double (&V)[3][3]) {
    double A[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            A[i][j] = H[i][j];
            V[i][j] = i == j ? 1.0 : 0.0;
        }
    for (int sweep = 0; sweep < 20; ++sweep) {
        const bool r01 = jacobi_pair<0, 1>(A, V), r02 = jacobi_pair<0, 2>(A, V), r12 = jacobi_pair<1, 2>(A, V);
        if (!(r01 || r02 || r12)) break;
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) s[j] = sqrt(A[0][j] * A[0][j] + A[1][j] * A[1][j] + A[2][j] * A[2][j]);
    swap_cols<0, 1>(A, V, s);
    swap_cols<0, 2>(A, V, s);
    swap_cols<1, 2>(A, V, s);
    double u0[3] = {1.0, 0.0, 0.0}, u1[3], u2[3];
    if (s[0] > 0.0) {
        u0[0] = A[0][0] / s[0]; u0[1] = A[1][0] / s[0]; u0[2] = A[2][0] / s[0];
    }
    {   // u1: the second column, once more orthogonalised against u0; without one, any unit vector orthogonal to u0
        const double d = u0[0] * A[0][1] + u0[1] * A[1][1] + u0[2] * A[2][1];
        double v[3] = {A[0][1] - d * u0[0], A[1][1] - d * u0[1], A[2][1] - d * u0[2]};
        double nv = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        if (!(s[1] > 1e-290) || !(nv > 0.5 * s[1])) {
            const double ax = fabs(u0[0]), ay = fabs(u0[1]), az = fabs(u0[2]);
            const int k = (ax <= ay && ax <= az) ? 0 : (ay <= az ? 1 : 2);
            const double uk = k == 0 ? u0[0] : (k == 1 ? u0[1] : u0[2]);
            v[0] = (k == 0 ? 1.0 : 0.0) - uk * u0[0];
            v[1] = (k == 1 ? 1.0 : 0.0) - uk * u0[1];
            v[2] = (k == 2 ? 1.0 : 0.0) - uk * u0[2];
            nv = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        }
        u1[0] = v[0] / nv; u1[1] = v[1] / nv; u1[2] = v[2] / nv;
    }
    {   // u2 = +-(u0 x u1), the sign of the third column (R = U D V^T does not depend on it: delta follows)
        double c[3] = {u0[1] * u1[2] - u0[2] * u1[1], u0[2] * u1[0] - u0[0] * u1[2], u0[0] * u1[1] - u0[1] * u1[0]};
        const double nc = sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
        const double sg = (c[0] * A[0][2] + c[1] * A[1][2] + c[2] * A[2][2]) < 0.0 ? -1.0 : 1.0;
        u2[0] = sg * c[0] / nc; u2[1] = sg * c[1] / nc; u2[2] = sg * c[2] / nc;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        U[i][0] = u0[i]; U[i][1] = u1[i]; U[i][2] = u2[i];
    }
}

// One lane: the fit of sample b from its sums about the pivots.
__device__ void kabsch_finish(const KabschArgs &a, int b, const double (&S)[KB_SUMS], const double (&pa)[3], const double (&pb)[3]) {
    double *__restrict__ fit = a.fit + (size_t)b * RRL_FIT_DOUBLES;
    float *__restrict__ Ro = a.R + (size_t)b * 9, *__restrict__ To = a.T + (size_t)b * 3;
    int32_t *__restrict__ info = a.info + (size_t)b * 4;
    const int used = (int)S[KB_USED], skipped = (int)S[KB_SKIP];
    const double W = S[KB_W];
    for (int i = 0; i < RRL_FIT_DOUBLES; ++i) fit[i] = 0.0;
    fit[RRL_FIT_W] = W;
    info[0] = used;
    info[3] = skipped;
    if (used < 3 || !(W > 0.0)) {
        for (int i = 0; i < 9; ++i) Ro[i] = (i % 4 == 0) ? 1.0f : 0.0f;
        for (int i = 0; i < 3; ++i) To[i] = 0.0f;
        info[1] = RRL_FIT_FEW;
        info[2] = 0;
        return;
    }
    const double den = W + a.eps_w, inv = 1.0 / den, c = W * inv, omc = a.eps_w * inv;  // c = sum wn, omc = 1 - c
    double sq[3], sr[3], da[3], db[3], abar[3], bbar[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        sq[j] = S[KB_Q + j] * inv;
        sr[j] = S[KB_R + j] * inv;
        da[j] = sq[j] - omc * pa[j];  // abar - pa
        db[j] = sr[j] - omc * pb[j];
        abar[j] = pa[j] + da[j];
        bbar[j] = pb[j] + db[j];
    }
    double H[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int k = 0; k < 3; ++k) H[j][k] = ((S[KB_QR + 3 * j + k] * inv - sq[j] * db[k]) - da[j] * sr[k]) + c * da[j] * db[k];
    const double m2a = (S[KB_QQ] * inv - 2.0 * (sq[0] * da[0] + sq[1] * da[1] + sq[2] * da[2])) + c * (da[0] * da[0] + da[1] * da[1] + da[2] * da[2]);
    const double m2b = (S[KB_RR] * inv - 2.0 * (sr[0] * db[0] + sr[1] * db[1] + sr[2] * db[2])) + c * (db[0] * db[0] + db[1] * db[1] + db[2] * db[2]);
    double U[3][3], s[3], V[3][3];
    svd3(H, U, s, V);
    const double delta = det3(U) * det3(V) < 0.0 ? -1.0 : 1.0;
    const double d[3] = {1.0, 1.0, delta};
    double Rm[3][3], Tm[3];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int k = 0; k < 3; ++k) Rm[j][k] = (U[j][0] * V[k][0] + U[j][1] * V[k][1]) + d[2] * U[j][2] * V[k][2];
#pragma unroll
    for (int k = 0; k < 3; ++k) Tm[k] = bbar[k] - ((abar[0] * Rm[0][k] + abar[1] * Rm[1][k]) + abar[2] * Rm[2][k]);
    const double gap = s[1] + delta * s[2];
    const double res = (m2a + m2b) - 2.0 * (s[0] + gap);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        fit[RRL_FIT_ABAR + j] = abar[j];
        fit[RRL_FIT_BBAR + j] = bbar[j];
        fit[RRL_FIT_S + j] = s[j];
        To[j] = (float)Tm[j];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            fit[RRL_FIT_U + 3 * j + k] = U[j][k];
            fit[RRL_FIT_V + 3 * j + k] = V[j][k];
            Ro[3 * j + k] = (float)(a.transpose_r ? Rm[k][j] : Rm[j][k]);
        }
    }
    fit[RRL_FIT_DELTA] = delta;
    fit[RRL_FIT_RES] = res > 0.0 ? res : 0.0;
    fit[RRL_FIT_KEYMEAN] = S[KB_KD] * inv;
    info[1] = gap <= (double)a.rank_tol * s[0] ? RRL_FIT_DEGENERATE : RRL_FIT_OK;  // (a NaN fit compares false: not degenerate, NaN out)
    info[2] = delta < 0.0 ? 1 : 0;
}

// Grid (ceil(n / KB_ROWS), B).  Lane tid takes rows bx KB_ROWS + tid and + 256 of sample b, in that order; every term is a
// double product of float32 inputs (their differences to the pivots); the workgroup's row of sums goes to part[b][bx] -- and,
// when the grid has one workgroup per sample, lane 0 finishes the fit in the same launch.
__global__ __launch_bounds__(256) void kabsch_part_kernel(const KabschArgs a) {
    __shared__ double s_red[4][KB_SUMS];
    __shared__ double s_tot[KB_SUMS];
    const int tid = threadIdx.x, bx = blockIdx.x, b = blockIdx.y, n = a.n, m = a.m;
    const int ca = rrl_rows(a.count_a, b, n), cb = rrl_rows(a.count_b, b, m);
    const float *__restrict__ A = a.a + (size_t)b * n * a.sa;
    const float *__restrict__ Bp = a.b + (size_t)b * m * a.sb;
    double pa[3], pb[3];
    kabsch_pivot(A, pa);
    kabsch_pivot(Bp, pb);
    const float gate = (a.keys && a.gate_sq) ? a.gate_sq[b] : INFINITY;
    double acc[KB_SUMS];
#pragma unroll
    for (int q = 0; q < KB_SUMS; ++q) acc[q] = 0.0;
#pragma unroll
    for (int r = 0; r < KB_ROWS / 256; ++r) {
        const int i = bx * KB_ROWS + r * 256 + tid;
        if (i >= n) continue;
        const PairRow pair = pair_walk(a.keys, b, n, i, ca, m, cb, gate);
        if (pair.skip) {
            acc[KB_SKIP] += 1.0;
            continue;
        }
        if (pair.gated) continue;
        const double w = a.w ? (double)a.w[(size_t)b * n + i] : 1.0;
        const float *__restrict__ pr = A + (size_t)i * a.sa;
        const float *__restrict__ qr = Bp + (size_t)pair.idx * a.sb;  // idx < min(m, cb): inside sample b's rows
        const double q[3] = {(double)pr[0] - pa[0], (double)pr[1] - pa[1], (double)pr[2] - pa[2]};
        const double t[3] = {(double)qr[0] - pb[0], (double)qr[1] - pb[1], (double)qr[2] - pb[2]};
        acc[KB_W] += w;
        acc[KB_USED] += 1.0;
        acc[KB_KD] += w * (double)pair.dist;
        acc[KB_QQ] += w * ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]);
        acc[KB_RR] += w * ((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double wq = w * q[j];
            acc[KB_Q + j] += wq;
            acc[KB_R + j] += w * t[j];
#pragma unroll
            for (int k = 0; k < 3; ++k) acc[KB_QR + 3 * j + k] += wq * t[k];
        }
    }
    const double tot = block_sum_d(acc, s_red, a.part + ((size_t)b * gridDim.x + bx) * KB_SUMS);
    if (gridDim.x != 1) return;  // (uniform)
    if (tid < KB_SUMS) s_tot[tid] = tot;
    __syncthreads();
    if (tid == 0) {
        double S[KB_SUMS];
#pragma unroll
        for (int q = 0; q < KB_SUMS; ++q) S[q] = s_tot[q];
        kabsch_finish(a, b, S, pa, pb);
    }
}

// One wavefront per sample: lane q adds sum q of the sample's partial rows in index order, lane 0 finishes the fit.
__global__ __launch_bounds__(64) void kabsch_finish_kernel(const KabschArgs a, int nblk) {
    __shared__ double s_tot[KB_SUMS];
    const int b = blockIdx.x, lane = threadIdx.x;
    if (lane < KB_SUMS) s_tot[lane] = part_rows_total<KB_SUMS>(a.part, b, nblk, lane);
    __syncthreads();
    if (lane != 0) return;
    double pa[3], pb[3], S[KB_SUMS];
    kabsch_pivot(a.a + (size_t)b * a.n * a.sa, pa);
    kabsch_pivot(a.b + (size_t)b * a.m * a.sb, pb);
#pragma unroll
    for (int q = 0; q < KB_SUMS; ++q) S[q] = s_tot[q];
    kabsch_finish(a, b, S, pa, pb);
}

extern "C" size_t rrl_kabsch_part_bytes(int B, int n) {
    if (B <= 0 || n <= 0) return 0;
    return sizeof(double) * KB_SUMS * (size_t)B * (size_t)((n + KB_ROWS - 1) / KB_ROWS);
}

// the refusals shared by the forward and the backward; 0: `k` is filled
static int kabsch_check(const rrl_kabsch_args *p, KabschArgs &k) {
    if (!p || p->struct_bytes != (int32_t)sizeof(rrl_kabsch_args)) return RRL_E_ARG;
    if (p->B < 0 || p->B > 32767 || p->n <= 0 || p->m <= 0 || p->a_stride < 3 || p->b_stride < 3) return RRL_E_ARG;
    if (!p->a || !p->b || !p->fit || !p->info || (((uintptr_t)p->fit) & 7) != 0) return RRL_E_ARG;
    if ((!p->keys && p->m != p->n) || (p->gate_sq && !p->keys)) return RRL_E_ARG;
    k = {p->B, p->n, p->m, p->a_stride, p->b_stride, p->transpose_r, p->a, p->b, p->w, (const unsigned long long *)p->keys,
         p->count_a, p->count_b, p->gate_sq, p->eps_w, p->rank_tol, (double *)p->part, p->R, p->T, p->fit, p->info};
    return 0;
}

extern "C" int rrl_kabsch_fwd(const rrl_kabsch_args *p, void *stream) {
    KabschArgs k;
    if (const int rc = kabsch_check(p, k)) return rc;
    if (!p->R || !p->T || !p->part || (((uintptr_t)p->part) & 7) != 0) return RRL_E_ARG;
    if (p->part_bytes < rrl_kabsch_part_bytes(p->B, p->n)) return RRL_E_WS;
    if (p->B == 0) return 0;
    const int nblk = (p->n + KB_ROWS - 1) / KB_ROWS;
    hipLaunchKernelGGL(kabsch_part_kernel, dim3((unsigned)nblk, (unsigned)p->B), dim3(256), 0, (hipStream_t)stream, k);
    if (nblk > 1) hipLaunchKernelGGL(kabsch_finish_kernel, dim3((unsigned)p->B), dim3(64), 0, (hipStream_t)stream, k, nblk);
    RRL_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------
// Backward of the dense fit (include/rrl.h rrl_kabsch_bwd has the formulas).  Grid (ceil(n / 256), B): lane 0 of a workgroup
// turns (gR, gT) and the forward's fit into the sample's gH (9), the gradients of the two centroids (3 + 3) and the constant
// of the weight normalisation, all double; then one row per lane.
// ---------------------------------------------------------------------------------------
struct KabschBwdArgs {
    KabschArgs f;
    const float *gR, *gT;
    float *ga, *gb, *gw;
};

__global__ __launch_bounds__(256) void kabsch_bwd_kernel(const KabschBwdArgs g) {
    __shared__ double s_p[24];  // gH [9], g abar [3], g bbar [3], abar [3], bbar [3], K, 1 / (W + eps), live
    const KabschArgs &a = g.f;
    const int tid = threadIdx.x, b = blockIdx.y, n = a.n;
    const int i = blockIdx.x * 256 + tid;
    if (tid == 0) {
        const double *__restrict__ fit = a.fit + (size_t)b * RRL_FIT_DOUBLES;
        const bool live = a.info[(size_t)b * 4 + 1] == RRL_FIT_OK;
        for (int q = 0; q < 24; ++q) s_p[q] = 0.0;
        if (live) {
            double U[3][3], V[3][3], G[3][3], Rm[3][3], abar[3], bbar[3], gT[3], s[3];
            const double delta = fit[RRL_FIT_DELTA], W = fit[RRL_FIT_W];
            const double d[3] = {1.0, 1.0, delta};
            const double den = W + a.eps_w, omc = a.eps_w / den;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                abar[j] = fit[RRL_FIT_ABAR + j];
                bbar[j] = fit[RRL_FIT_BBAR + j];
                s[j] = d[j] * fit[RRL_FIT_S + j];
                gT[j] = g.gT ? (double)g.gT[(size_t)b * 3 + j] : 0.0;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    U[j][k] = fit[RRL_FIT_U + 3 * j + k];
                    V[j][k] = fit[RRL_FIT_V + 3 * j + k];
                }
            }
            double gab[3], gbb[3];
#pragma unroll
            for (int j = 0; j < 3; ++j)
#pragma unroll
                for (int k = 0; k < 3; ++k) Rm[j][k] = (U[j][0] * V[k][0] + U[j][1] * V[k][1]) + d[2] * U[j][2] * V[k][2];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                gbb[j] = gT[j];  // T = bbar - abar R
                gab[j] = -((Rm[j][0] * gT[0] + Rm[j][1] * gT[1]) + Rm[j][2] * gT[2]);
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double up = g.gR ? (double)g.gR[(size_t)b * 9 + (a.transpose_r ? 3 * k + j : 3 * j + k)] : 0.0;
                    G[j][k] = up - abar[j] * gT[k];
                }
            }
            double Gt[3][3], Z[3][3], gH[3][3];  // Gt = U^T G V
#pragma unroll
            for (int p = 0; p < 3; ++p)
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    double v = 0.0;
#pragma unroll
                    for (int j = 0; j < 3; ++j)
#pragma unroll
                        for (int k = 0; k < 3; ++k) v += U[j][p] * G[j][k] * V[k][q];
                    Gt[p][q] = v;
                }
#pragma unroll
            for (int p = 0; p < 3; ++p)
#pragma unroll
                for (int q = 0; q < 3; ++q) Z[p][q] = p == q ? 0.0 : (Gt[p][q] - d[p] * d[q] * Gt[q][p]) / (s[p] + s[q]);
#pragma unroll
            for (int j = 0; j < 3; ++j)
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    double v = 0.0;
#pragma unroll
                    for (int p = 0; p < 3; ++p)
#pragma unroll
                        for (int q = 0; q < 3; ++q) v += U[j][p] * Z[p][q] * V[k][q];
                    gH[j][k] = v;
                }
            // sum wn (b - bbar) = (1 - c) bbar (zero without eps_w): H's centring reaches the centroids through it
#pragma unroll
            for (int j = 0; j < 3; ++j)
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    gab[j] -= gH[j][k] * omc * bbar[k];
                    gbb[k] -= omc * abar[j] * gH[j][k];
                }
            double K = 0.0;  // sum_j wn_j (d / d wn_j): <gH, H> = tr(Z^T S) = 0 drops out
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                K += abar[j] * gab[j] + bbar[j] * gbb[j];
                s_p[9 + j] = gab[j];
                s_p[12 + j] = gbb[j];
                s_p[15 + j] = abar[j];
                s_p[18 + j] = bbar[j];
#pragma unroll
                for (int k = 0; k < 3; ++k) s_p[3 * j + k] = gH[j][k];
            }
            s_p[21] = K;
            s_p[22] = 1.0 / den;
            s_p[23] = 1.0;
        }
    }
    __syncthreads();
    if (i >= n) return;
    const int rows = min(rrl_rows(a.count_a, b, n), rrl_rows(a.count_b, b, n));
    const size_t at = (size_t)b * n + i;
    float oa[3] = {0.0f, 0.0f, 0.0f}, ob[3] = {0.0f, 0.0f, 0.0f}, ow = 0.0f;
    if (s_p[23] != 0.0 && i < rows) {
        const float *__restrict__ pr = a.a + at * a.sa;
        const float *__restrict__ qr = a.b + at * a.sb;
        const double w = a.w ? (double)a.w[at] : 1.0, inv = s_p[22], wn = w * inv;
        const double x[3] = {(double)pr[0], (double)pr[1], (double)pr[2]}, y[3] = {(double)qr[0], (double)qr[1], (double)qr[2]};
        double dx[3], dy[3], hy[3], xh[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            dx[j] = x[j] - s_p[15 + j];
            dy[j] = y[j] - s_p[18 + j];
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            hy[j] = (s_p[3 * j] * dy[0] + s_p[3 * j + 1] * dy[1]) + s_p[3 * j + 2] * dy[2];  // gH (b - bbar)
            xh[j] = (dx[0] * s_p[j] + dx[1] * s_p[3 + j]) + dx[2] * s_p[6 + j];              // (a - abar) gH
        }
        double gwn = -s_p[21];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            oa[j] = (float)(wn * (hy[j] + s_p[9 + j]));
            ob[j] = (float)(wn * (xh[j] + s_p[12 + j]));
            gwn += dx[j] * hy[j] + x[j] * s_p[9 + j] + y[j] * s_p[12 + j];
        }
        ow = (float)(gwn * inv);
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        if (g.ga) g.ga[at * 3 + j] = oa[j];
        if (g.gb) g.gb[at * 3 + j] = ob[j];
    }
    if (g.gw) g.gw[at] = ow;
}

extern "C" int rrl_kabsch_bwd(const rrl_kabsch_args *p, const float *gR, const float *gT, float *ga, float *gb, float *gw,
                              void *stream) {
    KabschBwdArgs g;
    if (const int rc = kabsch_check(p, g.f)) return rc;
    if (p->keys) return RRL_E_ARG;  // (the keyed fit has no gradient: the pairing is not differentiable)
    if (p->B == 0) return 0;
    g.gR = gR; g.gT = gT; g.ga = ga; g.gb = gb; g.gw = gw;
    hipLaunchKernelGGL(kabsch_bwd_kernel, dim3((unsigned)((p->n + 255) / 256), (unsigned)p->B), dim3(256), 0, (hipStream_t)stream, g);
    RRL_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------
// The ICP pose step and epoch: the step's body, its refusals and the epoch's front are rrl_icp_step.h's, shared with the robust
// loop of rrl_robust.hip; the kernel here is that body without the annealing rule, in its own launch.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void icp_step_kernel(const IcpStepArgs a) { icp_step_one<false>(a, IcpAnneal{}); }

extern "C" int rrl_icp_step_batch(const float *Rk, const float *Tk, const int32_t *info, const double *fit, float *R, float *T,
                                  const float *tol_rot, const float *tol_trans, int patience, const float *value, float *table,
                                  long long *cursor, long long nrows, float *row, float *last_step, int32_t *state, int B,
                                  void *stream) {
    if (B < 0 || !icp_step_args_ok(Rk, Tk, info, fit, R, T, state, patience, tol_rot, tol_trans)) return RRL_E_ARG;
    if (B == 0) return 0;
    const IcpStepArgs a = {Rk, Tk, info, fit, R, T, tol_rot, tol_trans, patience, value, table, cursor, nrows, row, last_step, state, B};
    hipLaunchKernelGGL(icp_step_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, a);
    RRL_LAUNCH_CHECK();
    return 0;
}

// One ICP epoch: four public entries back to back, every refusal before the first launch (host code only).
extern "C" int rrl_icp_epoch(const rrl_icp_epoch_args *a, void *stream) {
    if (!cloud_epoch_front_ok(a)) return RRL_E_ARG;
    if (!icp_step_args_ok(a->Rk, a->Tk, a->info, a->fit, a->R, a->T, a->state, a->patience, a->tol_rot, a->tol_trans)) return RRL_E_ARG;
    if ((((uintptr_t)a->fit) & 7) != 0) return RRL_E_ARG;
    if (!icp_epoch_ws_ok(a)) return RRL_E_WS;
    int rc = cloud_epoch_pair(a, stream);
    if (rc) return rc;
    rc = icp_epoch_fit(a, a->w, stream);
    if (rc) return rc;
    return rrl_icp_step_batch(a->Rk, a->Tk, a->info, a->fit, a->R, a->T, a->tol_rot, a->tol_trans, a->patience, a->values, a->table,
                              a->cursor, a->table_rows, a->row, a->last_step, a->state, a->B, stream);
}
