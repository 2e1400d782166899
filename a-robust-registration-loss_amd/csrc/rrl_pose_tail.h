// rrl_pose_tail.h -- what every pose step does besides its pose (se3_adam_step_kernel<> / <Se3Batch>, rrl_geom.hip;
// se3_newton_step_kernel, rrl_newton.hip; the store also log_row_kernel): the epoch's log row and the next epoch's sampler
// box, for ONE sample on that sample's own pointers -- the caller advances them to its slices; k = the lane of the step's
// single wavefront.  Lane 0 logs, lanes 8 .. 13 reduce the box; the pose arithmetic sits between the load and the store.
#pragma once

struct PoseLog {
    long long at;  // the sample's cursor word as found (-1: nothing is logged)
    float q0, q1;  // loss, value
};

// (the log row's inputs are requested with the first loads, not after the arithmetic)
__device__ __forceinline__ PoseLog pose_log_load(int k, const float *table, const long long *cursor, const float *loss,
                                                 const float *value) {
    PoseLog p = {-1, 0.0f, 0.0f};
    if (k == 0 && table && cursor) {
        p.at = cursor[0];
        p.q0 = loss ? loss[0] : 0.0f;
        p.q1 = value ? value[0] : 0.0f;
    }
    return p;
}

// the moved source's AABB for the NEXT epoch's sampler (code/test_demo_optimized_Lie_Algebra.py:46-51 samples against
// the previous epoch's moved source) from the per-workgroup partial rows the records launch just left (APART: min xyz,
// max xyz of the moved first points) -- one launch (rigid apply + AABB) less per epoch.  n_rows = ceil(the sample's rows
// / 256): rows beyond a sample's count are never read (a ragged build does not write them); no rows: (+inf, -inf), as
// aabb_kernel
__device__ __forceinline__ void pose_next_box(int k, float *box, const float *rows, int n_rows) {
    if (box != nullptr && k >= 8 && k < 14) {
        const int c = k - 8;
        float v = c < 3 ? INFINITY : -INFINITY;
        for (int r = 0; r < n_rows; ++r) {
            const float q = rows[(size_t)r * 8 + c];
            v = c < 3 ? fminf(v, q) : fmaxf(v, q);
        }
        box[c] = v;
    }
}

// row = table[at] = (loss, value, gate open), cursor += 1 (log_row_kernel's whole work).  tstride: floats from one row of
// the log table to the next (3, or 3 B with the table at the sample's column); a cursor outside [0, nrows) still advances,
// unlogged
__device__ __forceinline__ void pose_log_row(const PoseLog &p, bool ok, float *table, long long tstride, long long nrows,
                                             long long *cursor, float *row) {
    const float q[3] = {p.q0, p.q1, ok ? 1.0f : 0.0f};
    for (int c = 0; c < 3; ++c) {
        if (row) row[c] = q[c];
        if (p.at >= 0 && p.at < nrows) table[p.at * tstride + c] = q[c];
    }
    cursor[0] = p.at + 1;
}

// lane 0, last: the row of what pose_log_load found, where a pose step has a table and a cursor
__device__ __forceinline__ void pose_log_store(const PoseLog &p, bool ok, float *table, long long tstride, long long nrows,
                                               long long *cursor, float *row) {
    if (table && cursor) pose_log_row(p, ok, table, tstride, nrows, cursor, row);
}
