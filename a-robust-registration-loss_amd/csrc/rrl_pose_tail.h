// rrl_pose_tail.h -- what every pose step does besides its pose (se3_adam_step_kernel<> / <Se3Batch>, rrl_geom.hip;
// se3_newton_step_kernel, rrl_newton.hip; the store also log_row_kernel): the epoch's log row and the next epoch's sampler
// box, for ONE sample on that sample's own pointers -- the caller advances them to its slices; k = the lane of the step's
// single wavefront.  Lane 0 logs, lanes 8 .. 13 reduce the box; the pose arithmetic sits between the load and the store.
// Below them: the state words and the stopping rule of the steps that stop by themselves (also icp_step_one, rrl_icp_step.h:
// icp_step_kernel and robust_step_kernel; plane_step_kernel, rrl_plane.hip), and that rule's host-side refusal.
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

// ---------------------------------------------------------------------------------------
// The state words and the stopping rule of the steps that stop by themselves (se3_newton_step_kernel, icp_step_one;
// include/rrl.h "pose-step state").  state [B][4] int32: [0] epochs issued, [1] consecutive calm epochs, [2] the epoch count
// at which the pair was declared done (-1: not yet), [3] what this call did (RRL_POSE_*, or the caller's own failure code).
// Lane 0 of a pose's wavefront: load, the kernel's own arithmetic and pose write, pose_stop_update where a step was applied,
// store.  No arithmetic on floats here: the lengths arrive as the floats the kernel formed.
// ---------------------------------------------------------------------------------------
struct PoseStop {
    // as found (the state load)
    int epochs;    // epochs issued, this call included
    int calm_was;  // word 1
    int done_at;   // word 2
    bool done;     // done before this call: the pose is frozen, words 1 and 2 are kept
    // to store: a done pair's as found, else (0, done_at) unless pose_stop_update counts this epoch
    int calm, done_new;
};

__device__ __forceinline__ PoseStop pose_stop_load(const int32_t *st) {
    PoseStop p;
    p.epochs = st[0] + 1;
    p.calm_was = st[1];
    p.done_at = st[2];
    p.done = p.done_at >= 0;
    p.calm = p.done ? p.calm_was : 0;
    p.done_new = p.done_at;
    return p;
}

// after an applied step of lengths (rot, trans) of pose b: last_step (optional), then the rule -- `patience` consecutive
// epochs whose step stayed below both tolerances end the pair
__device__ __forceinline__ void pose_stop_update(PoseStop &p, size_t b, float rot, float trans, float *last_step, const float *tol_rot,
                                                 const float *tol_trans, int patience) {
    if (last_step) {
        last_step[b * 2] = rot;
        last_step[b * 2 + 1] = trans;
    }
    if (patience > 0 && tol_rot && tol_trans) {
        p.calm = (rot < tol_rot[b] && trans < tol_trans[b]) ? p.calm_was + 1 : 0;
        if (p.calm >= patience) p.done_new = p.epochs;
    }
}

__device__ __forceinline__ void pose_stop_store(const PoseStop &p, int status, int32_t *st) {
    st[0] = p.epochs;
    st[1] = p.calm;
    st[2] = p.done_new;
    st[3] = status;
}

// the refusal every entry with the rule makes (host): a positive patience needs both tolerances
static inline bool pose_stop_args_ok(int patience, const float *tol_rot, const float *tol_trans) {
    return patience <= 0 || (tol_rot && tol_trans);
}
