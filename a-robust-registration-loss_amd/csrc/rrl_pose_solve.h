// rrl_pose_solve.h -- what the Gauss-Newton pose steps share (se3_newton_step_kernel, rrl_newton.hip; plane_step_kernel,
// rrl_plane.hip), one lane, double throughout: the damped 6 x 6 Cholesky solve, and the composition of the solved twist onto
// the pose (step scale, clamps, Rodrigues, composition about the step's pivot, Gram-Schmidt, the finite check, the one rounding
// to float32).  What a step does around them (its sums, the state words, the log row) is its kernel's own.
#pragma once

// solves (A + damping diag(A) + eps I) x = -g for the symmetric A; false: a pivot that does not exceed eps (what the
// undamped matrix contributes there is not positive) or is not finite, or a solution that is not finite
__device__ __forceinline__ bool newton_solve(const double (&H)[6][6], const double (&g)[6], double damping, double eps, double (&x)[6]) {
    double Lm[6][6];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double p = H[j][j] + damping * H[j][j] + eps;
#pragma unroll
        for (int q = 0; q < j; ++q) p -= Lm[j][q] * Lm[j][q];
        if (!(p > eps) || !(p < (double)INFINITY)) { ok = false; p = 1.0; }
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
    double y[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double v = -g[i];
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
    for (int i = 0; i < 6; ++i)
        if (!(fabs(x[i]) < (double)INFINITY)) ok = false;
    return ok;
}

// The step of the solved twist x = (omega, v), scaled by sc and clamped to (mr, mt), composed onto the pose of one sample
// (R [9], T [3], y = x R + T): R <- R Rot^T, T <- (T - c) Rot^T + c + v about the pivot c, one Gram-Schmidt pass over R's rows.
// PIVOT = false is the form without a pivot, T <- T Rot^T + v: not the other one at c = 0, which turns a -0 into +0; with
// PIVOT a null `pivot` is c = 0 in the pivoted form.  false: a step length, clamp, pivot or pose that is not finite -- nothing
// is written.  rot, trans: |omega|, |v| as applied.
template <bool PIVOT>
__device__ __forceinline__ bool pose_compose(const double (&x)[6], double sc, double mr, double mt, const float *__restrict__ pivot,
                                             float *__restrict__ R, float *__restrict__ T, double &rot, double &trans) {
    double w[3] = {sc * x[0], sc * x[1], sc * x[2]}, v[3] = {sc * x[3], sc * x[4], sc * x[5]};
    double nw = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]), nv = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    if (nw > mr) {
        const double f = mr / nw;
        w[0] *= f; w[1] *= f; w[2] *= f;
        nw = mr;
    }
    if (nv > mt) {
        const double f = mt / nv;
        v[0] *= f; v[1] *= f; v[2] *= f;
        nv = mt;
    }
    // Rot = I + A K + Bc K K, K = [w]x, theta = |w| as composed (Rodrigues; the series below 1e-4: their next terms are < 1e-26)
    const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], th = sqrt(th2);
    double A, Bc;
    if (th < 1e-4) {
        A = 1.0 - th2 / 6.0 * (1.0 - th2 / 20.0);
        Bc = 0.5 - th2 / 24.0 * (1.0 - th2 / 30.0);
    } else {
        A = sin(th) / th;
        Bc = (1.0 - cos(th)) / th2;
    }
    const double K[3][3] = {{0.0, -w[2], w[1]}, {w[2], 0.0, -w[0]}, {-w[1], w[0], 0.0}};
    double Rot[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double kk = K[i][0] * K[0][j] + K[i][1] * K[1][j] + K[i][2] * K[2][j];
            Rot[i][j] = (i == j ? 1.0 : 0.0) + A * K[i][j] + Bc * kk;
        }
    double Ro[3][3], To[3], Rn[3][3], Tn[3], c[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        To[i] = (double)T[i];
        if constexpr (PIVOT) {
            if (pivot) c[i] = (double)pivot[i];
            To[i] -= c[i];
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) Ro[i][j] = (double)R[3 * i + j];
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        Tn[j] = To[0] * Rot[j][0] + To[1] * Rot[j][1] + To[2] * Rot[j][2];
        if constexpr (PIVOT) Tn[j] += c[j];
        Tn[j] += v[j];
#pragma unroll
        for (int i = 0; i < 3; ++i) Rn[i][j] = Ro[i][0] * Rot[j][0] + Ro[i][1] * Rot[j][1] + Ro[i][2] * Rot[j][2];
    }
    // one Gram-Schmidt pass over the rows: hundreds of compositions of float-rounded matrices do not drift
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int p = 0; p < i; ++p) {
            const double d = Rn[i][0] * Rn[p][0] + Rn[i][1] * Rn[p][1] + Rn[i][2] * Rn[p][2];
            Rn[i][0] -= d * Rn[p][0]; Rn[i][1] -= d * Rn[p][1]; Rn[i][2] -= d * Rn[p][2];
        }
        const double n = sqrt(Rn[i][0] * Rn[i][0] + Rn[i][1] * Rn[i][1] + Rn[i][2] * Rn[i][2]);
        Rn[i][0] /= n; Rn[i][1] /= n; Rn[i][2] /= n;
    }
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        finite = finite && fabs(Tn[i]) < (double)INFINITY;
#pragma unroll
        for (int j = 0; j < 3; ++j) finite = finite && fabs(Rn[i][j]) < (double)INFINITY;
    }
    if (!finite) return false;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        T[i] = (float)Tn[i];
#pragma unroll
        for (int j = 0; j < 3; ++j) R[3 * i + j] = (float)Rn[i][j];
    }
    rot = nw;
    trans = nv;
    return true;
}
