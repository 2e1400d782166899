// rrl_cloud_epoch.h -- the host front the three cloud epochs share (rrl_icp_epoch, rrl_kabsch.hip; rrl_robust_icp_epoch,
// rrl_robust.hip; rrl_plane_icp_epoch, rrl_plane.hip), host code only, rrl_epoch.hip's idiom: templates over the argument
// structs, which name every shared field alike (include/rrl.h rrl_icp_epoch_args, rrl_plane_epoch_args).  An epoch asks
// cloud_epoch_front_ok and its fit's own RRL_E_ARG checks, then cloud_epoch_cham_ws_ok and its fit's own RRL_E_WS check, and
// only then cloud_epoch_pair: every refusal before the first launch, RRL_E_ARG first.  What the two point-to-point epochs
// share beyond this is rrl_icp_step.h's.
#pragma once

// RRL_E_ARG: the struct, the shape, what both fits take (the clouds, the moved source, the Chamfer walk's outputs, the partial
// rows), counts or orders given for one cloud only
template <class A>
static bool cloud_epoch_front_ok(const A *a) {
    if (!a || a->struct_bytes != (int32_t)sizeof(A)) return false;
    const int B = a->B, N = a->N, M = a->M;
    if (B <= 0 || B > 32767 || N <= 0 || M <= 0 || (N > M ? N : M) > rrl_sort_capacity()) return false;
    if (!a->src || !a->tar || !a->moved || !a->cham_ws || !a->best_x || !a->best_y || !a->values || !a->part) return false;
    if ((((uintptr_t)a->part) & 7) != 0) return false;
    return (a->count1 == nullptr) == (a->count2 == nullptr) && (a->order_x == nullptr) == (a->order_y == nullptr);
}
// RRL_E_WS: the Chamfer walk's scratch
template <class A>
static bool cloud_epoch_cham_ws_ok(const A *a) {
    return a->cham_ws_bytes >= rrl_chamfer_workspace_bytes(a->B, a->N, a->M);
}
// moved = src R + T, then the walk that leaves the keys of the pairing in best_x (and the monitor's values)
template <class A>
static int cloud_epoch_pair(const A *a, void *stream) {
    if (const int rc = rrl_rigid_apply_fwd(a->src, a->R, a->T, a->moved, a->B, a->N, 0, 0, stream)) return rc;
    return rrl_chamfer_tree_fwd_counted(a->moved, a->tar, a->count1, a->count2, a->cham_ws, a->cham_ws_bytes, a->best_x, a->best_y,
                                        a->values, nullptr, a->B, a->N, a->M, a->order_x, a->order_y, stream);
}
