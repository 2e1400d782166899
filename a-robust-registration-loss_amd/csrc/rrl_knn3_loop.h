// rrl_knn3_loop.h -- knn3_kernel's brute-force loop (rrl_neigh.hip) as a device function, for the kernels that run the same
// loop on a sample's own points: knn3_counted_kernel (rrl_neigh.hip) and the non-finite branch of knn3_tree_kernel
// (rrl_knn_tree.hip).  knn3_kernel itself keeps its own text: routed through this function it grows from 576 to 624 bytes of
// code and takes 16 bytes of scratch, as the two callers here already do (measured on the device assembly).
#pragma once
#include "rrl_common.h"

// The three nearest of the n points p [n][3] to point qi, by float64 squared distances (dx dx + dy dy) + dz dz from the float32
// coordinates, ascending index and `<`: the lowest index among equals.  p is wave-uniform (scalar loads); fewer than three
// points leave index 0 in the open slots.
__device__ __forceinline__ void knn3_brute_loop(const float *__restrict__ p, int n, int qi, int &i0, int &i1, int &i2) {
    const double qx = p[3 * qi], qy = p[3 * qi + 1], qz = p[3 * qi + 2];
    double d0 = 1e300, d1 = 1e300, d2 = 1e300;
    i0 = i1 = i2 = 0;
    kptr tp = (kptr)(uintptr_t)p;
    for (int j = 0; j < n; ++j, tp += 3) {
        const double dx = qx - (double)tp[0], dy = qy - (double)tp[1], dz = qz - (double)tp[2];
        const double d = (dx * dx + dy * dy) + dz * dz;
        if (d < d2) {
            if (d < d1) {
                d2 = d1; i2 = i1;
                if (d < d0) { d1 = d0; i1 = i0; d0 = d; i0 = j; }
                else { d1 = d; i1 = j; }
            } else { d2 = d; i2 = j; }
        }
    }
}
