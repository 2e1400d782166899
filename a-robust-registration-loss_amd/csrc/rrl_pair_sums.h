// rrl_pair_sums.h -- what the kernels that sum over the rows of a pairing share (kabsch_part_kernel / kabsch_finish_kernel,
// rrl_kabsch.hip; plane_part_kernel / plane_finish_kernel, rrl_plane.hip; the block sum also pose_normal_eq_kernel,
// rrl_newton.hip): which partner a row has and whether it counts, and the fixed-order double sum from the lanes' accumulators
// to the sample's totals.  No atomics; the order of every addition is written here once.
#pragma once

#include "rrl_wave_sum_d.h"

struct PairRow {
    bool skip;     // no partner inside both samples' rows: the row counts as skipped
    bool gated;    // a partner beyond the sample's gate: neither used nor skipped
    unsigned idx;  // the partner's row; < min(m, cb) unless skip
    float dist;    // the key's distance word (0 for a dense pairing)
};

// Row i (< the capacity n) of sample b: keyed, the partner and its distance word are those of keys[b][i] (a Chamfer walk's
// word: distance << 32 | index, all ones = none); dense (keys == nullptr), row i of the other cloud.  ca, cb: the sample's row
// counts in the two clouds, m: the other cloud's capacity, gate: the largest distance word that is used
__device__ __forceinline__ PairRow pair_walk(const unsigned long long *__restrict__ keys, int b, int n, int i, int ca, int m, int cb,
                                             float gate) {
    PairRow p = {i >= ca, false, (unsigned)i, 0.0f};
    if (!p.skip) {
        if (keys) {
            const unsigned long long key = keys[(size_t)b * n + i];
            p.idx = (unsigned)(key & 0xffffffffull);
            p.dist = __uint_as_float((unsigned)(key >> 32));
            p.skip = key == ~0ull || p.idx >= (unsigned)m || p.idx >= (unsigned)cb;
            p.gated = p.dist > gate;
        } else {
            p.skip = i >= cb;
        }
    }
    return p;
}

// The sums of a 256-lane workgroup from its lanes' accumulators: wave_sum_d, one row per wavefront in s_red, the four rows
// added as (0 + 1) + (2 + 3) by lanes tid < SUMS, which store the workgroup's partial row and return their sum (the other
// lanes: 0).  Every lane of the workgroup calls it.
template <int SUMS>
__device__ __forceinline__ double block_sum_d(double (&acc)[SUMS], double (&s_red)[4][SUMS], double *__restrict__ part_row) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int q = 0; q < SUMS; ++q) acc[q] = wave_sum_d(acc[q]);
    if (lane == 0)
#pragma unroll
        for (int q = 0; q < SUMS; ++q) s_red[wave][q] = acc[q];
    __syncthreads();
    if (tid >= SUMS) return 0.0;
    const double tot = (s_red[0][tid] + s_red[1][tid]) + (s_red[2][tid] + s_red[3][tid]);
    part_row[tid] = tot;
    return tot;
}

// sum q of sample b over its nblk partial rows, in index order
template <int SUMS>
__device__ __forceinline__ double part_rows_total(const double *__restrict__ part, int b, int nblk, int q) {
    double s = 0.0;
    for (int k = 0; k < nblk; ++k) s += part[((size_t)b * nblk + k) * SUMS + q];
    return s;
}
