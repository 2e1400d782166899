// rrl_pose_solve.h -- the solver the Gauss-Newton pose steps share (se3_newton_step_kernel, rrl_newton.hip; plane_step_kernel,
// rrl_plane.hip): the damped 6 x 6 Cholesky solve, one lane, double throughout.  What a step does around it (clamps, Rodrigues,
// composition about its pivot, Gram-Schmidt, rounding, state) is its kernel's own.
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
