// rrl_arith.h -- the per-value arithmetic of the sparse stages, shared by the narrow pipeline (the rrl_stage_*.h kernels of
// rrl_sparse.hip) and the wide one (rrl_wide.hip): weights, intersection points, triangle gathers, the Welsch term and the
// fixed-point unit of the bucket sums are the same source in both, so the same inputs give the same bits.
#pragma once
#include "rrl_common.h"

constexpr int FIX_SHIFT = 40;  // bucket sums in 2^-40 fixed point: order-independent, bit-deterministic

// sqrt(dist_sq) of the three points of triangle f and the detached weights of
// code/loss.py:92: w_k = d_k / ((d0 + d1) + d2).  Same arithmetic as the scan, so the
// distances are bit-identical to the ones that decided the label.
__device__ __forceinline__ void hit_weights(const float *p, const float *ln, float *w) {
    float d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
        d[k] = sqrtf(dist_sq<float>(p[3 * k], p[3 * k + 1], p[3 * k + 2], ln[0], ln[1], ln[2],
                                    ln[3], ln[4], ln[5]));
    float s = (d[0] + d[1]) + d[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) w[k] = d[k] / s;
}

// q = mean_k(w_k * P_k), code/loss.py:155-163 (a mean: 1/3 of the convex combination)
__device__ __forceinline__ void inter_point(const float *p, const float *w, float *q) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float s = w[0] * p[c];
        s = s + w[1] * p[3 + c];
        s = s + w[2] * p[6 + c];
        q[c] = s / 3.0f;
    }
}

// the 9 coordinates of triangle f from its 48-byte prepared record: three 16-byte loads instead
// of nine 4-byte gathers from the 36-byte input rows (a wavefront-level gather costs ~64 cycles
// of the CU's address path per instruction, whatever its width)
__device__ __forceinline__ void tri_coords(const float *__restrict__ ptri, int stride, int f, float *c) {
    if (stride != PTRI_STRIDE) {  // raw 36-byte rows (what the per-line stage reads since round 4)
#pragma unroll
        for (int i = 0; i < 9; ++i) c[i] = ptri[9 * (size_t)f + i];
        return;
    }
    const float4 *row = (const float4 *)(ptri + PTRI_STRIDE * (size_t)f);
    const float4 r0 = row[0], r1 = row[1], r2 = row[2];
    c[0] = r0.x; c[1] = r0.y; c[2] = r0.z; c[3] = r0.w;
    c[4] = r1.x; c[5] = r1.y; c[6] = r1.z; c[7] = r1.w;
    c[8] = r2.x;
}

// Welsch1(x, c) = 1 - exp(-(x / c) / 2), code/loss.py:20-21
__device__ __forceinline__ float welsch(float d, float med) {
    return 1.0f - expf(-(d / med) / 2.0f);
}

