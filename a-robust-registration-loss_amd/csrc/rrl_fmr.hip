// rrl_fmr.hip -- FMR's inverse-compositional pose head (fmr/model.py:318-439 SolveRegistration.ic_algo / approx_Jac, with
// se_math/se3.py:57-80, 133-165 and se_math/invmat.py:6-13, 83-112) as three pairs of entries (include/rrl.h, DESIGN.md
// section 23): rrl_ic_perturb_fwd / _bwd (the six perturbed templates), rrl_ic_pinv_fwd / _bwd (J, H = J^T J, H^-1, pinv =
// H^-1 J^T) and rrl_ic_update_fwd / _bwd (r, dx, the batch-wide stop rule and g <- exp(dx) g).  The encoder between them stays
// torch.  Everything here is O(B K) or O(B N) and latency-bound: the point is few launches, no host read-back, fixed-order
// double sums and the reference's OWN gradient rules (ExpMap.backward, InvMatrix.backward) stated once.
//
// One workgroup of 256 lanes per sample wherever a sum runs over K or N: a lane takes the indices tid, tid + 256, ... in
// ascending order, the 64 lanes of a wavefront are added by wave_sum_d's fixed tree, the four wavefronts in index order.
// The small algebra (6 x 6 Cholesky, exponential, 4 x 4 products) is one lane's, in double, broadcast through LDS.
#include <cstddef>
#include <cstdint>
#include <cmath>

#include "rrl_common.h"
#include "rrl_wave_sum_d.h"

#define IC_T 256           // lanes per workgroup
#define IC_MAX_B 65535
#define IC_WS_FLAG 36      // the sample's flag, behind its 36 doubles of H^-1

// ---- shared pieces -------------------------------------------------------------------------------------------------------
// sums of NV doubles over the workgroup, valid in every lane: wavefront tree, then the four wavefronts in index order
template <int NV>
__device__ __forceinline__ void ic_block_sum(double (&v)[NV], double (*red)[NV]) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int q = 0; q < NV; ++q) {
        const double s = wave_sum_d(v[q]);
        if (lane == 0) red[w][q] = s;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NV; ++q) v[q] = ((red[0][q] + red[1][q]) + red[2][q]) + red[3][q];
    __syncthreads();
}

// rows 0..2 of exp(x), x = (w, v): rrl_se3_exp's arithmetic (rrl_geom.hip se3_exp3: the same expressions in the same order,
// the reference's Taylor polynomials inside |t| < 0.01) in double.  E[i][3] = (V v)_i; the fourth row is (0, 0, 0, 1).
__device__ __forceinline__ void ic_exp(const double (&x)[6], double (&E)[3][4]) {
    const double a = x[0], b = x[1], c = x[2];
    const double n2 = a * a + b * b + c * c;
    const double t = n2 > 0.0 ? sqrt(n2) : 0.0;
    const double t2 = t * t;
    double s1, s2, s3;
    if (fabs(t) < 0.01) {
        s1 = 1.0 - t2 / 6.0 * (1.0 - t2 / 20.0 * (1.0 - t2 / 42.0));
        s2 = 0.5 * (1.0 - t2 / 12.0 * (1.0 - t2 / 30.0 * (1.0 - t2 / 56.0)));
        s3 = (1.0 / 6.0) * (1.0 - t2 / 20.0 * (1.0 - t2 / 42.0 * (1.0 - t2 / 72.0)));
    } else {
        const double sn = sin(t), cs = cos(t);
        s1 = sn / t;
        s2 = (1.0 - cs) / (t * t);
        s3 = (t - sn) / (t * t * t);
    }
    const double W[9] = {0.0, -c, b, c, 0.0, -a, -b, a, 0.0};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double V[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double sq = W[3 * i] * W[j] + W[3 * i + 1] * W[3 + j] + W[3 * i + 2] * W[6 + j];
            const double id = i == j ? 1.0 : 0.0;
            E[i][j] = id + s1 * W[3 * i + j] + s2 * sq;
            V[j] = id + s2 * W[3 * i + j] + s3 * sq;
        }
        E[i][3] = V[0] * x[3] + V[1] * x[4] + V[2] * x[5];
    }
}

// sum_ij M[i][j] [gen_k E]_ij for the six generators (se_math/se3.py genmat): for a rotation k < 3, with a = (k + 1) % 3 and
// b = (k + 2) % 3, row b of gen_k E is row a of E and row a is minus row b; for a translation, row k - 3 is (0, 0, 0, 1).
// Each q is the sum over j ascending of (M[b][j] E[a][j] - M[a][j] E[b][j]).
__device__ __forceinline__ void ic_gen_dot(const double (&M)[3][4], const double (&E)[3][4], double (&q)[6]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int a = (k + 1) % 3, b = (k + 2) % 3;
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) s += M[b][j] * E[a][j] - M[a][j] * E[b][j];
        q[k] = s;
        q[3 + k] = M[k][3];
    }
}

// H^-1 of the symmetric H by the unpivoted, undamped Cholesky of rrl_pose_solve.h's newton_solve (the same loops), each
// column of the inverse solved from its unit vector.  false: a pivot that does not exceed tol[j] (the rounding of H's own
// sums: below it the pivot is not told from 0) or is not finite, or an inverse that is not finite.
__device__ __forceinline__ bool ic_chol_inverse(const double (&H)[6][6], double tol_rel, double (&Hi)[6][6]) {
    double Lm[6][6];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double p = H[j][j];
#pragma unroll
        for (int q = 0; q < j; ++q) p -= Lm[j][q] * Lm[j][q];
        if (!(p > tol_rel * H[j][j]) || !(p > 0.0) || !(p < (double)INFINITY)) { ok = false; p = 1.0; }
        const double d = sqrt(p);
        Lm[j][j] = d;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double v = H[i][j];
#pragma unroll
            for (int q = 0; q < j; ++q) v -= Lm[i][q] * Lm[j][q];
            Lm[i][j] = v / d;
        }
    }
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        double y[6], x[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            double v = i == c ? 1.0 : 0.0;
#pragma unroll
            for (int q = 0; q < i; ++q) v -= Lm[i][q] * y[q];
            y[i] = v / Lm[i][i];
        }
#pragma unroll
        for (int i = 5; i >= 0; --i) {
            double v = y[i];
#pragma unroll
            for (int q = i + 1; q < 6; ++q) v -= Lm[q][i] * x[q];
            x[i] = v / Lm[i][i];
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            if (!(fabs(x[i]) < (double)INFINITY)) ok = false;
            Hi[i][c] = x[i];
        }
    }
    return ok;
}

__device__ __forceinline__ bool ic_finite(float v) { return fabsf(v) < INFINITY; }

// ---- 1. the perturbed templates ------------------------------------------------------------------------------------------
// D_i = exp(-dt_i e_i) of one (sample, axis), rows 0..2, in double
__device__ __forceinline__ void ic_perturbation(const float *__restrict__ dt, int b, int i, double (&D)[3][4]) {
    double x[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) x[q] = q == i ? -(double)dt[b * 6 + i] : 0.0;
    ic_exp(x, D);
}

__global__ __launch_bounds__(IC_T) void ic_perturb_fwd_kernel(const float *__restrict__ p0, const float *__restrict__ dt,
                                                              float *__restrict__ out, int N) {
    __shared__ float Ds[12];
    const int i = blockIdx.y, b = blockIdx.z;
    if (threadIdx.x == 0) {
        double D[3][4];
        ic_perturbation(dt, b, i, D);
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int c = 0; c < 4; ++c) Ds[4 * j + c] = (float)D[j][c];
    }
    __syncthreads();
    const int n = blockIdx.x * IC_T + threadIdx.x;
    if (n >= N) return;
    const float *p = p0 + ((size_t)b * N + n) * 3;
    float *o = out + (((size_t)b * 6 + i) * N + n) * 3;
    const float v0 = p[0], v1 = p[1], v2 = p[2];
#pragma unroll
    for (int j = 0; j < 3; ++j) o[j] = fmaf(v2, Ds[4 * j + 2], fmaf(v1, Ds[4 * j + 1], v0 * Ds[4 * j])) + Ds[4 * j + 3];
}

__global__ __launch_bounds__(IC_T) void ic_perturb_bwd_kernel(const float *__restrict__ p0, const float *__restrict__ dt,
                                                              const float *__restrict__ g_out, float *__restrict__ g_dt, int N) {
    __shared__ double red[4][12];
    const int i = blockIdx.x, b = blockIdx.y;
    const float *p = p0 + (size_t)b * N * 3;
    const float *g = g_out + ((size_t)b * 6 + i) * N * 3;
    double m[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) m[q] = 0.0;
    for (int n = threadIdx.x; n < N; n += IC_T) {
        const double v[4] = {(double)p[3 * (size_t)n], (double)p[3 * (size_t)n + 1], (double)p[3 * (size_t)n + 2], 1.0};
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double gj = (double)g[3 * (size_t)n + j];
#pragma unroll
            for (int c = 0; c < 4; ++c) m[4 * j + c] += gj * v[c];
        }
    }
    ic_block_sum<12>(m, red);
    if (threadIdx.x != 0) return;
    double D[3][4], M[3][4], q[6];
    ic_perturbation(dt, b, i, D);
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int c = 0; c < 4; ++c) M[j][c] = m[4 * j + c];
    ic_gen_dot(M, D, q);
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k)
        if (k == i) s = q[k];
    g_dt[b * 6 + i] = (float)(-s);
}

// ---- 2. J, H, H^-1, pinv ------------------------------------------------------------------------------------------------
// J[k][0..5] of one feature index, in double
__device__ __forceinline__ void ic_jac_row(const float *__restrict__ f0, const float *__restrict__ fp, const double (&dtd)[6],
                                           int K, int k, double (&J)[6]) {
    const double f = (double)f0[k];
#pragma unroll
    for (int i = 0; i < 6; ++i) J[i] = (f - (double)fp[(size_t)i * K + k]) / dtd[i];
}

__global__ __launch_bounds__(IC_T) void ic_pinv_fwd_kernel(const float *__restrict__ f0_, const float *__restrict__ fp_,
                                                           const float *__restrict__ dt, double *__restrict__ ws,
                                                           float *__restrict__ pinv_, int32_t *__restrict__ info, int K) {
    __shared__ double red[4][21];
    __shared__ double His[37];
    const int b = blockIdx.x;
    const float *f0 = f0_ + (size_t)b * K, *fp = fp_ + (size_t)b * 6 * K;
    float *pinv = pinv_ + (size_t)b * 6 * K;
    double dtd[6];
    int bad = K < 6;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const float d = dt[b * 6 + i];
        bad |= !ic_finite(d) || d == 0.0f;
        dtd[i] = (double)d;
    }
    double h[21];
#pragma unroll
    for (int q = 0; q < 21; ++q) h[q] = 0.0;
    for (int k = threadIdx.x; k < K; k += IC_T) {
        double J[6];
        ic_jac_row(f0, fp, dtd, K, k, J);
        bad |= !ic_finite(f0[k]);
#pragma unroll
        for (int i = 0; i < 6; ++i) bad |= !ic_finite(fp[(size_t)i * K + k]);
        int q = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) h[q++] += J[i] * J[j];
    }
    bad = __syncthreads_or(bad);
    ic_block_sum<21>(h, red);
    if (threadIdx.x == 0) {
        double H[6][6], Hi[6][6];
        int q = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) {
                H[i][j] = h[q];
                H[j][i] = h[q++];
            }
        const bool ok = ic_chol_inverse(H, (double)(K + 6) * 0x1p-52, Hi) && !bad;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                const double v = ok ? Hi[i][j] : 0.0;
                His[6 * i + j] = v;
                ws[(size_t)b * RRL_IC_WS_DOUBLES + 6 * i + j] = v;
            }
        His[36] = ok ? 0.0 : 1.0;
        ws[(size_t)b * RRL_IC_WS_DOUBLES + IC_WS_FLAG] = His[36];
#pragma unroll
        for (int q2 = IC_WS_FLAG + 1; q2 < RRL_IC_WS_DOUBLES; ++q2) ws[(size_t)b * RRL_IC_WS_DOUBLES + q2] = 0.0;
        if (info) info[b] = ok ? 0 : 1;
    }
    __syncthreads();
    const bool flagged = His[36] != 0.0;
    for (int k = threadIdx.x; k < K; k += IC_T) {
        double J[6];
        if (!flagged) ic_jac_row(f0, fp, dtd, K, k, J);
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            double s = 0.0;
            if (!flagged) {
#pragma unroll
                for (int j = 0; j < 6; ++j) s += His[6 * i + j] * J[j];
            }
            pinv[(size_t)i * K + k] = flagged ? 0.0f : (float)s;
        }
    }
}

__global__ __launch_bounds__(IC_T) void ic_pinv_bwd_kernel(const float *__restrict__ f0_, const float *__restrict__ fp_,
                                                           const float *__restrict__ dt, const double *__restrict__ ws,
                                                           const float *__restrict__ g_pinv, float *__restrict__ d_f0,
                                                           float *__restrict__ d_fp, float *__restrict__ d_dt, int K) {
    __shared__ double red[4][36];
    __shared__ double Hs[36], Ss[36];
    const int b = blockIdx.x;
    const float *f0 = f0_ + (size_t)b * K, *fp = fp_ + (size_t)b * 6 * K, *G = g_pinv + (size_t)b * 6 * K;
    const double *wsb = ws + (size_t)b * RRL_IC_WS_DOUBLES;
    if (wsb[IC_WS_FLAG] != 0.0) {  // a flagged sample: zero gradients (uniform over the workgroup)
        for (int k = threadIdx.x; k < K; k += IC_T) {
            if (d_f0) d_f0[(size_t)b * K + k] = 0.0f;
            if (d_fp)
#pragma unroll
                for (int i = 0; i < 6; ++i) d_fp[((size_t)b * 6 + i) * K + k] = 0.0f;
        }
        if (d_dt && threadIdx.x < 6) d_dt[b * 6 + threadIdx.x] = 0.0f;
        return;
    }
    double dtd[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) dtd[i] = (double)dt[b * 6 + i];
    if (threadIdx.x < 36) Hs[threadIdx.x] = wsb[threadIdx.x];
    // P = G J
    double P[36];
#pragma unroll
    for (int q = 0; q < 36; ++q) P[q] = 0.0;
    for (int k = threadIdx.x; k < K; k += IC_T) {
        double J[6];
        ic_jac_row(f0, fp, dtd, K, k, J);
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const double gi = (double)G[(size_t)i * K + k];
#pragma unroll
            for (int j = 0; j < 6; ++j) P[6 * i + j] += gi * J[j];
        }
    }
    ic_block_sum<36>(P, red);  // (its barriers also publish Hs)
    // S = -(H^-1 P) H^-1, every inner sum ascending; Ss = S + S^T
    if (threadIdx.x == 0) {
        double T[36], S[36];
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                double s = 0.0;
#pragma unroll
                for (int a = 0; a < 6; ++a) s += Hs[6 * i + a] * P[6 * a + j];
                T[6 * i + j] = s;
            }
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                double s = 0.0;
#pragma unroll
                for (int a = 0; a < 6; ++a) s += T[6 * i + a] * Hs[6 * a + j];
                S[6 * i + j] = -s;
            }
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = 0; j < 6; ++j) Ss[6 * i + j] = S[6 * i + j] + S[6 * j + i];
    }
    __syncthreads();
    // dJ[k][i] = sum_j G[j][k] Hi[j][i] + sum_j J[k][j] Ss[j][i], j ascending in each, the first sum first
    double ddt[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) ddt[i] = 0.0;
    for (int k = threadIdx.x; k < K; k += IC_T) {
        double J[6], g[6];
        ic_jac_row(f0, fp, dtd, K, k, J);
#pragma unroll
        for (int j = 0; j < 6; ++j) g[j] = (double)G[(size_t)j * K + k];
        double sf = 0.0;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            double s1 = 0.0, s2 = 0.0;
#pragma unroll
            for (int j = 0; j < 6; ++j) s1 += g[j] * Hs[6 * j + i];
#pragma unroll
            for (int j = 0; j < 6; ++j) s2 += J[j] * Ss[6 * j + i];
            const double dJ = s1 + s2, dq = dJ / dtd[i];
            sf += dq;
            if (d_fp) d_fp[((size_t)b * 6 + i) * K + k] = (float)(-dq);
            ddt[i] += dJ * J[i];
        }
        if (d_f0) d_f0[(size_t)b * K + k] = (float)sf;
    }
    if (!d_dt) return;
    __shared__ double red6[4][6];
    ic_block_sum<6>(ddt, red6);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < 6; ++i) d_dt[b * 6 + i] = (float)(-ddt[i] / dtd[i]);
    }
}

// ---- 3. the update ---------------------------------------------------------------------------------------------------------
// first launch, one workgroup per sample: r, dx and the sample's float32 step length
__global__ __launch_bounds__(IC_T) void ic_update_sums_kernel(const float *__restrict__ pinv_, const float *__restrict__ f0,
                                                              const float *__restrict__ f1, float *__restrict__ r,
                                                              float *__restrict__ dx, float *__restrict__ norms, int K) {
    __shared__ double red[4][6];
    const int b = blockIdx.x;
    const float *pinv = pinv_ + (size_t)b * 6 * K;
    double s[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) s[i] = 0.0;
    for (int k = threadIdx.x; k < K; k += IC_T) {
        const float rk = f1[(size_t)b * K + k] - f0[(size_t)b * K + k];
        r[(size_t)b * K + k] = rk;
#pragma unroll
        for (int i = 0; i < 6; ++i) s[i] += (double)pinv[(size_t)i * K + k] * (double)rk;
    }
    ic_block_sum<6>(s, red);
    if (threadIdx.x != 0) return;
    double n2 = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const float d = (float)(-s[i]);
        dx[b * 6 + i] = d;
        n2 += (double)d * (double)d;
    }
    norms[b] = (float)sqrt(n2);
    if (b + 1 == (int)gridDim.x && (gridDim.x & 1)) norms[b + 1] = 0.0f;  // the workspace's padding word: every byte is written
}

// second launch, one workgroup for the batch: the stop rule and the poses
__global__ __launch_bounds__(IC_T) void ic_update_pose_kernel(const float *__restrict__ dx, const float *__restrict__ norms,
                                                              const float *__restrict__ g, float xtol, int32_t *stop,
                                                              int32_t *__restrict__ stopped, float *__restrict__ g_new, int B) {
    // check = max_b norm_b with torch's NaN rule, check < xtol: no sample may fail norm_b < xtol
    int moving = 0;
    for (int b = threadIdx.x; b < B; b += IC_T) moving |= !(norms[b] < xtol);
    const int before = *stop;
    moving = __syncthreads_or(moving);  // (every lane has read `stop` before lane 0 writes it)
    const bool halt = before != 0 || !moving;
    if (threadIdx.x == 0) {
        *stop = halt ? 1 : 0;
        *stopped = halt ? 1 : 0;
    }
    for (int b = threadIdx.x; b < B; b += IC_T) {
        const float *gb = g + (size_t)b * 16;
        float *o = g_new + (size_t)b * 16;
        if (halt) {
#pragma unroll
            for (int q = 0; q < 16; ++q) o[q] = gb[q];
            continue;
        }
        double x[6], E[3][4];
#pragma unroll
        for (int i = 0; i < 6; ++i) x[i] = (double)dx[b * 6 + i];
        ic_exp(x, E);
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                double s = 0.0;
#pragma unroll
                for (int m = 0; m < 3; ++m) s += E[i][m] * (double)gb[4 * m + j];
                s += E[i][3] * (double)gb[12 + j];
                o[4 * i + j] = (float)s;
            }
#pragma unroll
        for (int j = 0; j < 4; ++j) o[12 + j] = gb[12 + j];
    }
}

__global__ __launch_bounds__(IC_T) void ic_update_bwd_kernel(const float *__restrict__ pinv_, const float *__restrict__ r_,
                                                             const float *__restrict__ dx, const float *__restrict__ g,
                                                             const int32_t *__restrict__ stopped, const float *__restrict__ G_g,
                                                             const float *__restrict__ G_r, const float *__restrict__ G_dx,
                                                             float *__restrict__ d_g, float *__restrict__ d_pinv,
                                                             float *__restrict__ d_f0, float *__restrict__ d_f1, int K) {
    __shared__ double qs[6];
    const int b = blockIdx.x;
    const bool halt = *stopped != 0;
    if (threadIdx.x == 0) {
        const float *gb = g + (size_t)b * 16;
        double Gd[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) Gd[i][j] = G_g ? (double)G_g[(size_t)b * 16 + 4 * i + j] : 0.0;
        if (halt) {
            if (d_g)
#pragma unroll
                for (int q = 0; q < 16; ++q) d_g[(size_t)b * 16 + q] = G_g ? G_g[(size_t)b * 16 + q] : 0.0f;
        } else {
            double x[6], E[3][4], M[3][4], q[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) x[i] = (double)dx[b * 6 + i];
            ic_exp(x, E);
            if (d_g) {  // d_g = exp(dx)^T G', the sum over the rows i ascending, exp's fourth row (0, 0, 0, 1) last
#pragma unroll
                for (int m = 0; m < 4; ++m)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        double s = 0.0;
#pragma unroll
                        for (int i = 0; i < 3; ++i) s += E[i][m] * Gd[i][j];
                        if (m == 3) s += Gd[3][j];
                        d_g[(size_t)b * 16 + 4 * m + j] = (float)s;
                    }
            }
            // M = G' g^T, rows 0..2 (gen_k's fourth row is 0)
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    double s = 0.0;
#pragma unroll
                    for (int m = 0; m < 4; ++m) s += Gd[i][m] * (double)gb[4 * j + m];
                    M[i][j] = s;
                }
            // [gen_k exp(dx)] needs exp's fourth row for the translations only: ic_gen_dot has it built in
            ic_gen_dot(M, E, q);
#pragma unroll
            for (int k = 0; k < 6; ++k) qs[k] = q[k] + (G_dx ? (double)G_dx[b * 6 + k] : 0.0);
        }
    }
    __syncthreads();
    const float *pinv = pinv_ + (size_t)b * 6 * K, *r = r_ + (size_t)b * K;
    for (int k = threadIdx.x; k < K; k += IC_T) {
        const double gr = G_r ? (double)G_r[(size_t)b * K + k] : 0.0;
        double s = 0.0;
        if (!halt) {
            const double rk = (double)r[k];
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                s += (double)pinv[(size_t)i * K + k] * qs[i];
                if (d_pinv) d_pinv[((size_t)b * 6 + i) * K + k] = (float)(-(qs[i] * rk));
            }
        } else if (d_pinv) {
#pragma unroll
            for (int i = 0; i < 6; ++i) d_pinv[((size_t)b * 6 + i) * K + k] = 0.0f;
        }
        const double df1 = halt ? gr : gr - s;
        if (d_f1) d_f1[(size_t)b * K + k] = (float)df1;
        if (d_f0) d_f0[(size_t)b * K + k] = (float)(-df1);
    }
}

// ---- host entries ----------------------------------------------------------------------------------------------------------
static bool ic_aligned8(const void *p) { return (((uintptr_t)p) & 7) == 0; }

extern "C" int rrl_ic_perturb_fwd(const float *p0, const float *dt, float *out, int B, int N, void *stream) {
    if (!p0 || !dt || !out || B < 0 || B > IC_MAX_B || N < 1) return RRL_E_ARG;
    if (B == 0) return 0;
    hipLaunchKernelGGL(ic_perturb_fwd_kernel, dim3((unsigned)((N + IC_T - 1) / IC_T), 6, (unsigned)B), dim3(IC_T), 0,
                       (hipStream_t)stream, p0, dt, out, N);
    RRL_LAUNCH_CHECK();
    return 0;
}

extern "C" int rrl_ic_perturb_bwd(const float *p0, const float *dt, const float *g_out, float *g_dt, int B, int N, void *stream) {
    if (!p0 || !dt || !g_out || !g_dt || B < 0 || B > IC_MAX_B || N < 1) return RRL_E_ARG;
    if (B == 0) return 0;
    hipLaunchKernelGGL(ic_perturb_bwd_kernel, dim3(6, (unsigned)B), dim3(IC_T), 0, (hipStream_t)stream, p0, dt, g_out, g_dt, N);
    RRL_LAUNCH_CHECK();
    return 0;
}

static bool ic_shape_ok(int B, int K) { return B >= 0 && B <= IC_MAX_B && K >= 1 && K <= RRL_IC_MAX_K; }

extern "C" size_t rrl_ic_pinv_workspace_bytes(int B, int K) {
    return ic_shape_ok(B, K) ? (size_t)B * RRL_IC_WS_DOUBLES * sizeof(double) : 0;
}

extern "C" int rrl_ic_pinv_fwd(const float *f0, const float *fp, const float *dt, void *ws, size_t ws_bytes, float *pinv,
                               int32_t *info, int B, int K, void *stream) {
    if (!f0 || !fp || !dt || !ws || !pinv || !ic_shape_ok(B, K)) return RRL_E_ARG;
    if (!ic_aligned8(ws) || ws_bytes < rrl_ic_pinv_workspace_bytes(B, K)) return RRL_E_WS;
    if (B == 0) return 0;
    hipLaunchKernelGGL(ic_pinv_fwd_kernel, dim3((unsigned)B), dim3(IC_T), 0, (hipStream_t)stream, f0, fp, dt, (double *)ws, pinv,
                       info, K);
    RRL_LAUNCH_CHECK();
    return 0;
}

extern "C" int rrl_ic_pinv_bwd(const float *f0, const float *fp, const float *dt, const void *ws, size_t ws_bytes,
                               const float *g_pinv, float *d_f0, float *d_fp, float *d_dt, int B, int K, void *stream) {
    if (!f0 || !fp || !dt || !ws || !g_pinv || !ic_shape_ok(B, K)) return RRL_E_ARG;
    if (!ic_aligned8(ws) || ws_bytes < rrl_ic_pinv_workspace_bytes(B, K)) return RRL_E_WS;
    if (B == 0 || (!d_f0 && !d_fp && !d_dt)) return 0;
    hipLaunchKernelGGL(ic_pinv_bwd_kernel, dim3((unsigned)B), dim3(IC_T), 0, (hipStream_t)stream, f0, fp, dt, (const double *)ws,
                       g_pinv, d_f0, d_fp, d_dt, K);
    RRL_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t rrl_ic_update_workspace_bytes(int B) {
    return B >= 0 && B <= IC_MAX_B ? (((size_t)B * sizeof(float) + 7) & ~(size_t)7) : 0;
}

extern "C" int rrl_ic_update_fwd(const float *pinv, const float *f0, const float *f1, const float *g, float xtol, int32_t *stop,
                                 void *ws, size_t ws_bytes, float *r, float *dx, float *g_new, int32_t *stopped, int B, int K,
                                 void *stream) {
    if (!pinv || !f0 || !f1 || !g || !stop || !ws || !r || !dx || !g_new || !stopped || !ic_shape_ok(B, K)) return RRL_E_ARG;
    if (!ic_aligned8(ws) || ws_bytes < rrl_ic_update_workspace_bytes(B)) return RRL_E_WS;
    if (B == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ic_update_sums_kernel, dim3((unsigned)B), dim3(IC_T), 0, st, pinv, f0, f1, r, dx, (float *)ws, K);
    hipLaunchKernelGGL(ic_update_pose_kernel, dim3(1), dim3(IC_T), 0, st, dx, (const float *)ws, g, xtol, stop, stopped, g_new, B);
    RRL_LAUNCH_CHECK();
    return 0;
}

extern "C" int rrl_ic_update_bwd(const float *pinv, const float *r, const float *dx, const float *g, const int32_t *stopped,
                                 const float *g_g_new, const float *g_r, const float *g_dx, float *d_g, float *d_pinv, float *d_f0,
                                 float *d_f1, int B, int K, void *stream) {
    if (!pinv || !r || !dx || !g || !stopped || !ic_shape_ok(B, K)) return RRL_E_ARG;
    if (B == 0 || (!d_g && !d_pinv && !d_f0 && !d_f1)) return 0;
    hipLaunchKernelGGL(ic_update_bwd_kernel, dim3((unsigned)B), dim3(IC_T), 0, (hipStream_t)stream, pinv, r, dx, g, stopped, g_g_new,
                       g_r, g_dx, d_g, d_pinv, d_f0, d_f1, K);
    RRL_LAUNCH_CHECK();
    return 0;
}
