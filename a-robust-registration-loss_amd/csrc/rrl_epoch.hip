// rrl_epoch.hip -- one registration epoch as ONE C call, host code only: rrl_demo_epoch (a single pair, the demo's loop, the
// next epoch's sampler pipelined into this epoch's launches) and the two batched epochs rrl_register_epoch (first order: fused
// step + Adam on se(3)) and rrl_register_newton_epoch (second order: forward + normal equations + Gauss-Newton step), which
// share one sequence written once below (include/rrl.h).
//
// code/test_demo_optimized_Lie_Algebra.py:46-82 does, per epoch: sample lines through both clouds' boxes (against the
// PREVIOUS epoch's moved source), move the source by the current pose, evaluate the loss, backward, Adam step, Chamfer
// monitor, log.  Every piece has its entry in this library already; this file only issues them back to back on the
// caller's stream -- sampler (2 launches) -> fused registration step on prepared clouds (4; 5 at the demo's 20 line tiles),
// the Chamfer walk of the step's clouds riding in its scan launch (round 4b; a launch of its own before) -> pose step (1:
// exp-map backward, gated Adam, next exp map, log row, next sampler box) -- so that a loop pays one
// host call (~5 us) per epoch instead of a hipGraph replay (~8 us fixed + ~1.5 us per node on this stack,
// tools/attic/graph_node_cost.py) or eight Python-level calls.  No new arithmetic: the results are those of the four entries.
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include "rrl_ws.h"
#include "rrl_pose_tail.h"  // (pose_stop_args_ok: the stopping rule's refusal)

extern "C" int rrl_demo_epoch(const rrl_demo_epoch_args *a, void *stream) {
    if (!a || a->struct_bytes < (int32_t)offsetof(rrl_demo_epoch_args, pipeline)) return RRL_E_ARG;  // (pipeline: appended in round 4b)
    const int N = a->N, M = a->M, L = a->L;
    if (N <= 0 || M <= 0 || L <= 0 || a->rounds <= 0) return RRL_E_ARG;
    // the record of the epoch's fused step: one sample, the reference's bucket range, scan mode cull
    RrlCall o = rrl_begin_call(a->opts, 1, N, M, L, a->ws, a->ws_bytes, stream);
    if (o.ragged()) return RRL_E_ARG;  // (one sample, the sampler's own line set: no counts)
    const char *env = getenv("RRL_DEMO_RIDE");  // (read per call: tests switch it between epochs) 0: no launch carries another's work
    const bool rides = !(env && env[0] == '0');
    int32_t *pipe = a->struct_bytes >= (int32_t)sizeof(rrl_demo_epoch_args) && rides ? a->pipeline : nullptr;
    if (pipe && ((long)((L + 1023) / 1024) * a->rounds >= 512 || L <= 1024)) pipe = nullptr;  // (the rider's limits: rrl_plan)
    // The Chamfer monitor needs the step's records launch only (the sorted moved source + the kept target), and launches of
    // one stream never overlap on this stack: its walk RIDES in the culled scan's launch (rrl_ws.h RrlChamRider; same
    // arithmetic, same value) -- one launch and ~12 us per epoch less.  RRL_DEMO_RIDE=0: the separate launch, as before.
    RrlChamRider rider = {a->cham_ws, a->cham_ws_bytes, a->best_x, a->best_y, a->cham_value, 0};
    o.rider = rides ? &rider : nullptr;
    // ... and so does the NEXT epoch's count pass, in the per-line launch (RrlCountRider): it samples against the moved source
    // of THIS epoch (code/test_demo_optimized_Lie_Algebra.py:46-51), whose box is in the records launch's partial rows
    const float *rows = o.at<RRL_WS_APART>();  // cloud 1, sample 0: the moved first points' partial boxes
    RrlCountRider counter = {(const unsigned long long *)a->rng_state, a->radius, a->centers, a->box2, rows,
                             (N + 255) / 256, (unsigned long long *)a->tile_counts, L, a->rounds, 0};
    // ... and its WRITE pass in the direct backward's launch (RrlWriteRider): the ballots are there by then (the per-line
    // launch precedes it), and nothing after the per-line stage reads the line buffer it overwrites
    RrlWriteRider writer = {(unsigned long long *)a->rng_state, a->radius, a->centers, (const unsigned long long *)a->tile_counts,
                            a->lines, a->filled, L, a->rounds, 0};
    if (pipe && (((uintptr_t)a->tile_counts) & 7) == 0) {
        o.count_rider = &counter;
        o.write_rider = &writer;
    }
    // the step's refusals before the epoch's first launch (the sampler's)
    const RrlXform xf = {a->src_tri, a->R, a->T, a->transpose_r, 1};
    const bool pointers = a->src_tri && a->R && a->T && a->tar_tri && a->lines && a->loss && a->grad_loss && a->gR && a->gt;
    int rc = rrl_check_call(o, pointers, RRL_WANT_DIRECT, nullptr, &xf);
    if (rc) return rc;
    if (pipe && *pipe == 3) {  // ... and its backward launch the write pass too: this epoch's lines are in place
        rc = 0;
    } else if (pipe && (*pipe & 1)) {  // the previous epoch's per-line launch carried this epoch's count pass: the write pass remains
        rc = rrl_sample_write_pass(a->rng_state, a->radius, a->centers, a->lines, a->filled, a->tile_counts, 1, L, a->rounds, stream);
    } else {
        rc = rrl_sample_lines_rng(a->rng_state, a->radius, a->centers, a->box1, a->box2, a->lines, a->filled, a->tile_counts,
                                  1, L, a->rounds, stream);
    }
    if (a->pipeline && a->struct_bytes >= (int32_t)sizeof(rrl_demo_epoch_args)) *a->pipeline = 0;
    if (rc) return rc;
    rc = rrl_registration_step_call(o, xf, a->tar_tri, a->lines, a->loss, a->grad_loss, a->gR, a->gt, nullptr);
    if (rc) return rc;
    if (pipe) *pipe = counter.done ? (writer.done ? 3 : 1) : 0;  // (a write pass without its count pass cannot have ridden)
    if (!rider.done) {
        rc = rrl_chamfer_from_loss(a->ws, a->ws, a->ws_bytes, 1, N, M, L, a->cham_ws, a->cham_ws_bytes, a->best_x, a->best_y,
                                   a->cham_value, stream);
        if (rc) return rc;
    }
    const int32_t *info = o.at<RRL_WS_INFO>();  // gate: the loss's bucket count (`if loss_di is not None`)
    return rrl_se3_adam_step(a->xi, a->gR, a->gt, a->m, a->v, a->adam_state, a->lr, info, a->b1, a->b2, a->eps, a->R, a->T,
                             nullptr, a->loss, a->cham_value, a->table, a->cursor, a->table_rows, a->row, rows,
                             (N + 255) / 256, a->box1, stream);
}

// ---------------------------------------------------------------------------------------
// The batched epochs (include/rrl.h rrl_register_epoch, rrl_register_newton_epoch): the same entries, B samples each --
// sampler (2 launches, 3 from 512 workgroups on; skipped without rng_state) -> the loss with the caller's options (prepared
// orders, counts, kept target) -> optionally the Chamfer monitor per sample (walk + group means, 2) -> the pose side, whose
// last launch is a batched pose step.  No riders, no pipelining across epochs, no environment switch, no host read-back;
// every refusal before the first launch, RRL_E_ARG first.  What both do is written once, as templates over the argument
// struct: rrl_register_epoch_args and rrl_register_newton_args name every shared field alike.
// ---------------------------------------------------------------------------------------
// RRL_E_ARG before there is a record: the struct, the shape, and the sampler's fields when the epoch samples (rng_state)
template <class A>
static bool epoch_front_ok(const A *a) {
    if (!a || a->struct_bytes < (int32_t)sizeof(A)) return false;
    if (a->B <= 0 || a->N <= 0 || a->M <= 0 || a->L <= 0) return false;
    return !a->rng_state || (a->rounds > 0 && a->rounds <= 65535 && a->B <= 65535 && a->radius && a->centers && a->box2 &&
                             a->filled && a->tile_counts && (((uintptr_t)a->tile_counts) & 7) == 0);
}
// RRL_E_ARG on the record of rrl_begin_call: one pose per pair, the sampler owns the line set; and the monitor's (value):
// the walk of rrl_chamfer_from_loss reads whole clouds -- not on a ragged workspace (include/rrl.h rrl_opts.count1)
template <class A>
static bool epoch_record_ok(const A *a, const RrlCall &o) {
    if (o.problems > 0 || o.nlines) return false;
    return !a->value || !(o.ragged() || !a->cham_ws || !a->best_x || !a->best_y || !a->cham_mean || !rrl_sorted_layout(a->N, a->M) ||
                          a->B > 32767);
}
// no launch of a one-call epoch carries another's work or leaves something for a later call (the chain flags are dropped, not
// refused; the payload belongs to rrl_loss_step_ex)
static void epoch_own_launches(RrlCall &o) {
    o.rider = nullptr;
    o.flags &= ~(RRL_F_CHAIN | RRL_F_CHAINED);
    o.chain_left = nullptr;
    o.payload = nullptr;
}
// RRL_E_WS after rrl_check_call's own: the monitor's scratch
template <class A>
static bool epoch_cham_ws_ok(const A *a) {
    return !a->value || a->cham_ws_bytes >= rrl_chamfer_workspace_bytes(a->B, a->N, a->M);
}
template <class A>
static int epoch_sample(const A *a, void *stream) {
    if (!a->rng_state) return 0;
    return rrl_sample_lines_rng(a->rng_state, a->radius, a->centers, a->box1, a->box2, a->lines, a->filled, a->tile_counts, a->B,
                                a->L, a->rounds, stream);
}
template <class A>
static int epoch_monitor(const A *a, void *stream) {
    if (!a->value) return 0;
    const int B = a->B, N = a->N, M = a->M;
    if (const int rc = rrl_chamfer_from_loss(a->ws, a->ws, a->ws_bytes, B, N, M, a->L, a->cham_ws, a->cham_ws_bytes, a->best_x,
                                             a->best_y, a->cham_mean, stream))
        return rc;
    return rrl_chamfer_group_means(a->cham_ws, a->cham_ws_bytes, a->value, B, B, N, M, stream);
}
// What a batched pose step takes from the call's workspace: its gate, the loss's bucket counts (INFO, stride 4); the partial
// rows of the moved sources, cloud 1 of APART [2][B][nblk][8]; the floats from one sample's rows to the next
struct EpochPoseInputs {
    const int32_t *gate;
    const float *rows;
    long long row_stride;
};
static EpochPoseInputs epoch_pose_inputs(const RrlCall &o) {
    const int nblk = ((o.N > o.M ? o.N : o.M) + 255) / 256;
    return {o.at<RRL_WS_INFO>(), o.at<RRL_WS_APART>(), (long long)nblk * 8};
}

// fused registration step (4 or 5 launches) -> batched Adam pose step (1), whose box output is box1
extern "C" int rrl_register_epoch(const rrl_register_epoch_args *a, void *stream) {
    if (!epoch_front_ok(a)) return RRL_E_ARG;
    RrlCall o = rrl_begin_call(a->opts, a->B, a->N, a->M, a->L, a->ws, a->ws_bytes, stream);
    if (!epoch_record_ok(a, o)) return RRL_E_ARG;
    if (!a->xi || !a->m || !a->v || !a->adam_state || !a->lr || !a->box1) return RRL_E_ARG;
    epoch_own_launches(o);
    const RrlXform xf = {a->src_tri, a->R, a->T, a->transpose_r, 1};
    const bool pointers = a->src_tri && a->R && a->T && a->tar_tri && a->lines && a->loss && a->grad_loss && a->gR && a->gt;
    int rc = rrl_check_call(o, pointers, RRL_WANT_DIRECT, nullptr, &xf);
    if (rc) return rc;
    if (!epoch_cham_ws_ok(a)) return RRL_E_WS;
    if ((rc = epoch_sample(a, stream))) return rc;
    rc = rrl_registration_step_call(o, xf, a->tar_tri, a->lines, a->loss, a->grad_loss, a->gR, a->gt, nullptr);
    if (rc) return rc;
    if ((rc = epoch_monitor(a, stream))) return rc;
    const EpochPoseInputs p = epoch_pose_inputs(o);
    return rrl_se3_adam_step_batch(a->xi, a->gR, a->gt, a->m, a->v, a->adam_state, a->lr, p.gate, 4, a->b1, a->b2, a->eps, a->R, a->T,
                                   a->gxi, a->loss, a->value, a->table, a->cursor, a->table_rows, a->row, p.rows, p.row_stride,
                                   o.count1, a->N, a->box1, a->B, stream);
}

// registration FORWARD (y = x R + T; the record's defaults are its arguments: range 1 .. 4, pool 0, scan mode cull, chunk 0)
// -> rrl_pose_normal_eq (2 launches) -> rrl_se3_newton_step_batch (1): the two entries of rrl_newton.hip.  The grids of the
// normal equations take B <= 65535 whether or not the epoch samples
extern "C" int rrl_register_newton_epoch(const rrl_register_newton_args *a, void *stream) {
    if (!epoch_front_ok(a) || a->B > 65535) return RRL_E_ARG;
    RrlCall o = rrl_begin_call(a->opts, a->B, a->N, a->M, a->L, a->ws, a->ws_bytes, stream);
    if (!epoch_record_ok(a, o)) return RRL_E_ARG;
    if (!a->box1 || !a->neq || !a->part || (((uintptr_t)a->part) & 7) != 0 || !a->state || !a->damping || !a->step || !a->max_rot ||
        !a->max_trans || !(a->eps >= 0.0) || !pose_stop_args_ok(a->patience, a->tol_rot, a->tol_trans))
        return RRL_E_ARG;
    epoch_own_launches(o);
    const RrlXform xf = {a->src_tri, a->R, a->T, 0, 1};
    const bool pointers = a->src_tri && a->R && a->T && a->tar_tri && a->lines && a->loss;
    int rc = rrl_check_call(o, pointers, RRL_WANT_FORWARD, nullptr, &xf);
    if (rc) return rc;
    if (!epoch_cham_ws_ok(a) || a->part_bytes < rrl_pose_normal_eq_part_bytes(a->B, a->L)) return RRL_E_WS;
    if ((rc = epoch_sample(a, stream))) return rc;
    rc = rrl_registration_forward_call(o, a->tar_tri, a->lines, a->loss);
    if (rc) return rc;
    if ((rc = epoch_monitor(a, stream))) return rc;
    rc = rrl_pose_normal_eq(a->ws, a->ws_bytes, a->B, a->N, a->M, a->L, 1, 1, RRL_MAX_HITS + 1, RRL_MAX_HITS + 1, a->neq, a->part,
                            a->part_bytes, nullptr, stream);
    if (rc) return rc;
    const EpochPoseInputs p = epoch_pose_inputs(o);
    return rrl_se3_newton_step_batch(a->neq, p.gate, 4, a->damping, a->step, a->max_rot, a->max_trans, a->tol_rot, a->tol_trans,
                                     a->patience, a->eps, a->R, a->T, a->loss, a->value, a->table, a->cursor, a->table_rows, a->row,
                                     p.rows, p.row_stride, o.count1, a->N, a->box1, a->delta, a->last_step, a->state, a->B, stream);
}
