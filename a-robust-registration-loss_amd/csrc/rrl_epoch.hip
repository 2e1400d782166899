// rrl_epoch.hip -- one epoch of the single-pair demo as ONE C call (include/rrl.h rrl_demo_epoch).
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
#include <cstring>
#include "rrl_ws.h"

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

// One epoch for a BATCH of pairs as one call (include/rrl.h rrl_register_epoch): the same entries, B samples each -- sampler
// (2 launches, 3 from 512 workgroups on; skipped without rng_state) -> fused registration step with the caller's options (prepared orders, counts, kept
// target; 4 or 5 launches) -> optionally the Chamfer monitor per sample (walk + group means, 2) -> batched pose step (1), whose
// gate is the workspace's INFO (stride 4), whose rows are cloud 1 of APART and whose box output is box1.  No riders, no
// pipelining across epochs, no environment switch, no host read-back; every refusal before the first launch, RRL_E_ARG first.
extern "C" int rrl_register_epoch(const rrl_register_epoch_args *a, void *stream) {
    if (!a || a->struct_bytes < (int32_t)sizeof(rrl_register_epoch_args)) return RRL_E_ARG;
    const int B = a->B, N = a->N, M = a->M, L = a->L;
    if (B <= 0 || N <= 0 || M <= 0 || L <= 0) return RRL_E_ARG;
    const bool sample = a->rng_state != nullptr, monitor = a->value != nullptr;
    if (sample && (a->rounds <= 0 || a->rounds > 65535 || B > 65535 || !a->radius || !a->centers || !a->box2 || !a->filled ||
                   !a->tile_counts || (((uintptr_t)a->tile_counts) & 7) != 0))
        return RRL_E_ARG;
    RrlCall o = rrl_begin_call(a->opts, B, N, M, L, a->ws, a->ws_bytes, stream);
    if (o.problems > 0 || o.nlines) return RRL_E_ARG;  // (one pose per pair; the sampler owns the line set)
    // the walk of rrl_chamfer_from_loss reads whole clouds: not on a ragged workspace (include/rrl.h rrl_opts.count1)
    if (monitor && (o.ragged() || !a->cham_ws || !a->best_x || !a->best_y || !a->cham_mean || !rrl_sorted_layout(N, M) || B > 32767))
        return RRL_E_ARG;
    if (!a->xi || !a->m || !a->v || !a->adam_state || !a->lr || !a->box1) return RRL_E_ARG;
    o.rider = nullptr;  // (no launch of this epoch carries another's work)
    o.flags &= ~(RRL_F_CHAIN | RRL_F_CHAINED);
    o.chain_left = nullptr;
    const RrlXform xf = {a->src_tri, a->R, a->T, a->transpose_r, 1};
    const bool pointers = a->src_tri && a->R && a->T && a->tar_tri && a->lines && a->loss && a->grad_loss && a->gR && a->gt;
    int rc = rrl_check_call(o, pointers, RRL_WANT_DIRECT, nullptr, &xf);
    if (rc) return rc;
    if (monitor && a->cham_ws_bytes < rrl_chamfer_workspace_bytes(B, N, M)) return RRL_E_WS;
    if (sample) {
        rc = rrl_sample_lines_rng(a->rng_state, a->radius, a->centers, a->box1, a->box2, a->lines, a->filled, a->tile_counts, B, L,
                                  a->rounds, stream);
        if (rc) return rc;
    }
    rc = rrl_registration_step_call(o, xf, a->tar_tri, a->lines, a->loss, a->grad_loss, a->gR, a->gt, nullptr);
    if (rc) return rc;
    if (monitor) {
        rc = rrl_chamfer_from_loss(a->ws, a->ws, a->ws_bytes, B, N, M, L, a->cham_ws, a->cham_ws_bytes, a->best_x, a->best_y,
                                   a->cham_mean, stream);
        if (rc) return rc;
        rc = rrl_chamfer_group_means(a->cham_ws, a->cham_ws_bytes, a->value, B, B, N, M, stream);
        if (rc) return rc;
    }
    const int nblk = ((N > M ? N : M) + 255) / 256;  // APART [2][B][nblk][8]: cloud 1 first
    return rrl_se3_adam_step_batch(a->xi, a->gR, a->gt, a->m, a->v, a->adam_state, a->lr, o.at<RRL_WS_INFO>(), 4, a->b1, a->b2,
                                   a->eps, a->R, a->T, a->gxi, a->loss, a->value, a->table, a->cursor, a->table_rows, a->row,
                                   o.at<RRL_WS_APART>(), (long long)nblk * 8, o.count1, N, a->box1, B, stream);
}

// One Gauss-Newton epoch for a batch of pairs as one call (include/rrl.h rrl_register_newton_epoch): rrl_register_epoch's
// sequence with the FORWARD in place of the fused step and the second-order pose side -- sampler -> registration forward with
// the caller's options -> optionally the monitor -> rrl_pose_normal_eq (2 launches) -> rrl_se3_newton_step_batch (1).  Existing
// entries plus the two of rrl_newton.hip, nothing else; every refusal before the first launch, RRL_E_ARG first.
extern "C" int rrl_register_newton_epoch(const rrl_register_newton_args *a, void *stream) {
    if (!a || a->struct_bytes < (int32_t)sizeof(rrl_register_newton_args)) return RRL_E_ARG;
    const int B = a->B, N = a->N, M = a->M, L = a->L;
    if (B <= 0 || B > 65535 || N <= 0 || M <= 0 || L <= 0) return RRL_E_ARG;
    const bool sample = a->rng_state != nullptr, monitor = a->value != nullptr;
    if (sample && (a->rounds <= 0 || a->rounds > 65535 || !a->radius || !a->centers || !a->box2 || !a->filled ||
                   !a->tile_counts || (((uintptr_t)a->tile_counts) & 7) != 0))
        return RRL_E_ARG;
    // the forward's options: the caller's, without what would make a launch of this epoch carry or leave something for another
    rrl_opts fo;
    memset(&fo, 0, sizeof fo);
    fo.reduce_mode = fo.deterministic = fo.sort_parts = fo.scan_variant = -1;
    if (a->opts && a->opts->struct_bytes >= 8)
        memcpy(&fo, a->opts, (size_t)a->opts->struct_bytes < sizeof fo ? (size_t)a->opts->struct_bytes : sizeof fo);
    fo.struct_bytes = (int32_t)sizeof fo;
    fo.flags &= ~(RRL_F_CHAIN | RRL_F_CHAINED);
    fo.chamfer = nullptr;
    fo.chain_left = nullptr;
    fo.payload = nullptr;
    RrlCall o = rrl_begin_call(&fo, B, N, M, L, a->ws, a->ws_bytes, stream);
    if (o.problems > 0 || o.nlines) return RRL_E_ARG;  // (one pose per pair; the sampler owns the line set)
    if (monitor && (o.ragged() || !a->cham_ws || !a->best_x || !a->best_y || !a->cham_mean || !rrl_sorted_layout(N, M) || B > 32767))
        return RRL_E_ARG;
    // the pose side's own pointers (rrl_pose_normal_eq, rrl_se3_newton_step_batch)
    if (!a->box1 || !a->neq || !a->part || (((uintptr_t)a->part) & 7) != 0 || !a->state || !a->damping || !a->step || !a->max_rot ||
        !a->max_trans || !(a->eps >= 0.0) || (a->patience > 0 && (!a->tol_rot || !a->tol_trans)))
        return RRL_E_ARG;
    const RrlXform xf = {a->src_tri, a->R, a->T, 0, 1};
    const bool pointers = a->src_tri && a->R && a->T && a->tar_tri && a->lines && a->loss;
    int rc = rrl_check_call(o, pointers, RRL_WANT_FORWARD, nullptr, &xf);
    if (rc) return rc;
    if (monitor && a->cham_ws_bytes < rrl_chamfer_workspace_bytes(B, N, M)) return RRL_E_WS;
    if (a->part_bytes < rrl_pose_normal_eq_part_bytes(B, L)) return RRL_E_WS;
    if (sample) {
        rc = rrl_sample_lines_rng(a->rng_state, a->radius, a->centers, a->box1, a->box2, a->lines, a->filled, a->tile_counts, B, L,
                                  a->rounds, stream);
        if (rc) return rc;
    }
    rc = rrl_registration_forward_ex(a->src_tri, a->R, a->T, a->tar_tri, a->lines, a->ws, a->ws_bytes, a->loss, B, N, M, L, 0, 1, 1,
                                     RRL_MAX_HITS + 1, RRL_MAX_HITS + 1, RRL_SCAN_CULL, 0, nullptr, &fo, stream);
    if (rc) return rc;
    if (monitor) {
        rc = rrl_chamfer_from_loss(a->ws, a->ws, a->ws_bytes, B, N, M, L, a->cham_ws, a->cham_ws_bytes, a->best_x, a->best_y,
                                   a->cham_mean, stream);
        if (rc) return rc;
        rc = rrl_chamfer_group_means(a->cham_ws, a->cham_ws_bytes, a->value, B, B, N, M, stream);
        if (rc) return rc;
    }
    rc = rrl_pose_normal_eq(a->ws, a->ws_bytes, B, N, M, L, 1, 1, RRL_MAX_HITS + 1, RRL_MAX_HITS + 1, a->neq, a->part, a->part_bytes,
                            nullptr, stream);
    if (rc) return rc;
    const int nblk = ((N > M ? N : M) + 255) / 256;  // APART [2][B][nblk][8]: cloud 1 first
    return rrl_se3_newton_step_batch(a->neq, o.at<RRL_WS_INFO>(), 4, a->damping, a->step, a->max_rot, a->max_trans, a->tol_rot,
                                     a->tol_trans, a->patience, a->eps, a->R, a->T, a->loss, a->value, a->table, a->cursor,
                                     a->table_rows, a->row, o.at<RRL_WS_APART>(), (long long)nblk * 8, o.count1, N, a->box1,
                                     a->delta, a->last_step, a->state, B, stream);
}
