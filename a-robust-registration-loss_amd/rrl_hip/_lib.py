"""ctypes binding of librrl_hip.so (C ABI: include/rrl.h).

There is NO fallback: if the library is missing, or no MI355X is visible, every op raises.
"""
import ctypes
import os

import torch  # noqa: F401  -- FIRST: librrl_hip.so must bind to the libamdhip64 PyTorch loaded,
#                              or its streams / device pointers belong to another HIP runtime

from .build import LIB

_c = ctypes
_P = _c.c_void_p
_I = _c.c_int

# name -> argtypes (all return int unless noted)
_Z = _c.c_size_t
_SIGS = {
    "rrl_workspace_layout": [_I, _I, _I, _I, _P],
    "rrl_wide_workspace_layout": [_I, _I, _I, _I, _P],
    "rrl_workspace_field": [_I] * 7 + [_P, _P, _P],
    "rrl_loss_forward_wide": [_P, _P, _P, _P, _Z, _P, _Z, _P] + [_I] * 11 + [_P, _P],
    "rrl_loss_backward_wide": [_P, _Z, _P, _P, _P] + [_I] * 5 + [_P],
    "rrl_loss_forward": [_P, _P, _P, _P, _Z, _P] + [_I] * 11 + [_P],
    "rrl_loss_backward": [_P, _P, _P, _Z, _P, _P, _P] + [_I] * 5 + [_P],
    "rrl_registration_forward": [_P] * 6 + [_Z, _P] + [_I] * 11 + [_P],
    "rrl_registration_forward_cached": [_P] * 6 + [_Z, _P] + [_I] * 11 + [_P, _P],
    "rrl_loss_forward_cached": [_P, _P, _P, _P, _Z, _P] + [_I] * 11 + [_P, _P],
    "rrl_loss_forward_info": [_P, _P, _P, _P, _Z, _P] + [_I] * 11 + [_P, _P, _P],
    "rrl_registration_backward": [_P] * 4 + [_Z] + [_P] * 6 + [_I] * 5 + [_P],
    "rrl_registration_step": [_P] * 6 + [_Z] + [_P] * 5 + [_I] * 11 + [_P, _P],
    "rrl_loss_forward_ex": [_P, _P, _P, _P, _Z, _P] + [_I] * 11 + [_P, _P, _P],
    "rrl_registration_forward_ex": [_P] * 6 + [_Z, _P] + [_I] * 11 + [_P, _P, _P],
    "rrl_registration_backward_ex": [_P] * 4 + [_Z] + [_P] * 6 + [_I] * 5 + [_P, _P],
    "rrl_registration_step_ex": [_P] * 6 + [_Z] + [_P] * 5 + [_I] * 11 + [_P, _P, _P],
    "rrl_loss_step_ex": [_P] * 6 + [_Z] + [_P] * 4 + [_I] * 11 + [_P, _P, _P],
    "rrl_cloud_order": [_P, _P, _P, _Z, _I, _I, _P],
    "rrl_cloud_order_points": [_P, _P, _P, _Z, _I, _I, _P],
    "rrl_cloud_order_counted": [_P, _P, _P, _P, _Z, _I, _I, _P],
    "rrl_tri_prepare_ex": [_P, _P, _P, _Z, _I, _I, _I, _I, _P, _P],
    "rrl_line_tri_scan_ex": [_P, _P, _Z] + [_I] * 6 + [_P, _P],
    "rrl_loss_reduce_ex": [_P, _Z, _P] + [_I] * 9 + [_P, _P],
    "rrl_line_pair_dist_ex": [_P, _P, _P, _P, _Z] + [_I] * 9 + [_P, _P],
    "rrl_tri_prepare": [_P, _P, _P, _Z, _I, _I, _I, _I, _P],
    "rrl_line_tri_scan": [_P, _P, _Z] + [_I] * 6 + [_P],
    "rrl_line_pair_dist": [_P, _P, _P, _P, _Z] + [_I] * 9 + [_P],
    "rrl_loss_reduce": [_P, _Z, _P] + [_I] * 9 + [_P],
    "rrl_loss_reduce_rows": [_P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P],
    "rrl_shard_payload": [_P, _P, _Z, _P, _P, _P, _I, _I, _I, _I, _P],
    "rrl_set_scan_variant": [_I],
    "rrl_demo_epoch": [_P, _P],
    "rrl_set_spin_limit": [_c.c_longlong],
    "rrl_debug_occupy": [_I, _I, _c.c_longlong, _P],
    "rrl_set_deterministic": [_I],
    "rrl_set_reduce_mode": [_I],
    "rrl_set_sort_parts": [_I],
    "rrl_scan_timing_enable": [_I],
    "rrl_scan_timing_collect": [_P, _I],
    "rrl_scan_counters": [_P, _c.c_longlong],
    "rrl_chamfer_counters": [_P, _c.c_longlong],
    "rrl_chamfer_group_means": [_P, _Z, _P, _I, _I, _I, _I, _P],
    "rrl_rigid_apply_fwd": [_P, _P, _P, _P, _I, _I, _I, _I, _P],
    "rrl_rigid_bwd_blocks": [_I],
    "rrl_rigid_apply_bwd": [_P] * 7 + [_I] * 4 + [_P],
    "rrl_chamfer_fwd": [_P] * 5 + [_I] * 3 + [_P],
    "rrl_chamfer_bwd": [_P] * 7 + [_I] * 3 + [_P],
    "rrl_chamfer_tree_fwd": [_P, _P, _P, _Z, _P, _P, _P, _I, _I, _I, _P],
    "rrl_chamfer_from_loss": [_P, _P, _Z, _I, _I, _I, _I, _P, _Z, _P, _P, _P, _P],
    "rrl_chamfer_tree_fwd_ex": [_P, _P, _P, _Z, _P, _P, _P, _I, _I, _I, _P, _P, _P, _c.c_longlong, _P],
    "rrl_chamfer_tree_fwd_counted": [_P, _P, _P, _P, _P, _Z, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P],
    "rrl_chamfer_bwd_counted": [_P] * 9 + [_I] * 3 + [_P],
    "rrl_chamfer_from_loss_ex": [_P, _P, _Z, _I, _I, _I, _I, _P, _Z, _P, _P, _P, _P, _c.c_longlong, _P],
    "rrl_aabb": [_P, _P, _I, _I, _P],
    "rrl_aabb_counted": [_P, _P, _P, _I, _I, _P],
    "rrl_box_accept": [_P, _P, _P, _P, _P, _I, _I, _P],
    "rrl_log_row": [_P, _P, _P, _P, _P, _c.c_longlong, _P, _P],
    "rrl_se3_adam_step": [_P] * 8 + [_c.c_double] * 3 + [_P] * 7 + [_c.c_longlong, _P, _P, _I, _P, _P],
    "rrl_se3_adam_step_batch": [_P] * 8 + [_c.c_longlong] + [_c.c_double] * 3 + [_P] * 7 + [_c.c_longlong, _P, _P, _c.c_longlong,
                                                                                            _P, _I, _P, _I, _P],
    "rrl_register_epoch": [_P, _P],
    "rrl_pose_normal_eq": [_P, _Z] + [_I] * 8 + [_P, _P, _Z, _P, _P],
    "rrl_se3_newton_step_batch": [_P, _P, _c.c_longlong] + [_P] * 6 + [_I, _c.c_double] + [_P] * 6 + [_c.c_longlong, _P, _P,
                                                                                                  _c.c_longlong, _P, _I] + [_P] * 4 + [_I, _P],
    "rrl_register_newton_epoch": [_P, _P],
    "rrl_kabsch_fwd": [_P, _P],
    "rrl_kabsch_bwd": [_P] * 7,
    "rrl_icp_step_batch": [_P] * 8 + [_I, _P, _P, _P, _c.c_longlong, _P, _P, _P, _I, _P],
    "rrl_icp_epoch": [_P, _P],
    "rrl_sinkhorn_fwd": [_P, _P],
    "rrl_sinkhorn_bwd": [_P] * 7,
    "rrl_rigid_apply_aabb": [_P, _P, _P, _P, _P, _I, _I, _I, _P],
    "rrl_se3_exp": [_P, _P, _P, _I, _P],
    "rrl_se3_exp_bwd": [_P, _P, _P, _P, _I, _P],
    "rrl_adam_gated": [_P] * 7 + [_I, _c.c_double, _c.c_double, _c.c_double, _P],
    "rrl_dense_scan": [_P, _P, _P, _P, _P, _I, _I, _I, _P],
    "rrl_fps": [_P, _P, _P, _P, _I, _I, _I, _P],
    "rrl_knn3": [_P, _P, _P, _I, _I, _I, _P],
    "rrl_fps_counted": [_P] * 6 + [_I] * 3 + [_P],
    "rrl_knn3_counted": [_P] * 7 + [_I] * 3 + [_P],
    "rrl_knn3_self": [_P, _P, _P, _Z, _P, _P, _P, _I, _I, _P],
    "rrl_ball_group": [_P] * 5 + [_c.c_float, _I, _I, _I, _P, _P, _P, _I, _I, _I, _P],
    "rrl_idx_normals": [_P, _I, _P, _P, _P, _I, _c.c_float, _P, _P, _I, _I, _I, _P],
    "rrl_plane_normal_eq": [_P, _P],
    "rrl_plane_step_batch": [_P] * 9 + [_I, _c.c_double] + [_P] * 5 + [_c.c_longlong, _P, _P, _P, _I, _P],
    "rrl_plane_icp_epoch": [_P, _P],
    "rrl_sample_lines": [_P] * 8 + [_I] * 3 + [_P],
    "rrl_sample_lines_rng": [_P] * 8 + [_I] * 3 + [_P],
}
EXPORTS = sorted(list(_SIGS) + ["rrl_version", "rrl_workspace_bytes", "rrl_chamfer_workspace_bytes",
                                 "rrl_cloud_order_workspace_bytes", "rrl_wide_workspace_bytes", "rrl_sort_capacity",
                                 "rrl_knn3_self_workspace_bytes", "rrl_pose_normal_eq_part_bytes", "rrl_kabsch_part_bytes",
                                 "rrl_sinkhorn_workspace_bytes", "rrl_plane_part_bytes"])

GROUP_XYZ, GROUP_DXYZ, GROUP_PPF, GROUP_MAX_SAMPLE = 1, 2, 4, 64  # include/rrl.h RRL_GROUP_*
F_TARGET_KEPT = 1  # include/rrl.h RRL_F_TARGET_KEPT
F_CHAIN = 2        # RRL_F_CHAIN: leave the hit counts / CHAIN words cleared for the next step on this workspace
F_CHAINED = 4      # RRL_F_CHAINED: the previous step did (chain_left = 1): records + both scans as one launch
# control words of a sample's MCTL / CHAIN row that Python reads (include/rrl.h RRL_MCTL_* / RRL_CHAIN_*: the one map)
MCTL_ERR = 19      # RRL_MCTL_ERR: a hand-off of the exchange reduce ran into its time-out
CHAIN_TIMEOUT = 3  # RRL_CHAIN_TIMEOUT: source workgroups of a chained step that gave up waiting for their records


class ChamferRider(ctypes.Structure):
    """include/rrl.h rrl_chamfer_rider: the evaluation's Chamfer walk, carried by its culled scan's launch."""
    _fields_ = [("ws", _P), ("ws_bytes", _Z), ("best_x", _P), ("best_y", _P), ("value", _P), ("done", _c.c_int32)]


class Opts(ctypes.Structure):
    """include/rrl.h rrl_opts: the per-call options of the *_ex entry points (-1 / NULL = the library default)."""
    _fields_ = [("struct_bytes", _c.c_int32), ("flags", _c.c_int32), ("reduce_mode", _c.c_int32),
                ("deterministic", _c.c_int32), ("sort_parts", _c.c_int32), ("scan_variant", _c.c_int32),
                ("order1", _P), ("order2", _P), ("scan_counters", _P), ("scan_counter_rows", _c.c_longlong),
                ("chamfer", _P), ("payload", _P), ("problems", _c.c_int32), ("chain_left", _P),
                ("count1", _P), ("count2", _P), ("nlines", _P)]

    def __init__(self, flags=0, reduce_mode=-1, deterministic=-1, sort_parts=-1, scan_variant=-1, order1=None,
                 order2=None, scan_counters=None, scan_counter_rows=0, chamfer=None, payload=None, problems=0,
                 chain_left=None, count1=None, count2=None, nlines=None):
        super().__init__(ctypes.sizeof(Opts), int(flags), int(reduce_mode), int(deterministic), int(sort_parts),
                         int(scan_variant), order1, order2, scan_counters, int(scan_counter_rows), chamfer, payload,
                         int(problems), chain_left, count1, count2, nlines)

class DemoEpochArgs(ctypes.Structure):
    """include/rrl.h rrl_demo_epoch_args (same field order)."""
    _fields_ = [("struct_bytes", _c.c_int32), ("N", _c.c_int32), ("M", _c.c_int32), ("L", _c.c_int32),
                ("rounds", _c.c_int32), ("transpose_r", _c.c_int32),
                ("rng_state", _P), ("radius", _P), ("centers", _P), ("box1", _P), ("box2", _P), ("lines", _P),
                ("filled", _P), ("tile_counts", _P),
                ("src_tri", _P), ("tar_tri", _P), ("R", _P), ("T", _P), ("ws", _P), ("ws_bytes", _Z), ("loss", _P),
                ("grad_loss", _P), ("gR", _P), ("gt", _P), ("opts", _P),
                ("cham_ws", _P), ("cham_ws_bytes", _Z), ("best_x", _P), ("best_y", _P), ("cham_value", _P),
                ("xi", _P), ("m", _P), ("v", _P), ("adam_state", _P), ("lr", _P), ("b1", _c.c_double), ("b2", _c.c_double),
                ("eps", _c.c_double), ("table", _P), ("cursor", _P), ("table_rows", _c.c_longlong), ("row", _P),
                ("pipeline", _P)]


class RegisterEpochArgs(ctypes.Structure):
    """include/rrl.h rrl_register_epoch_args (same field order)."""
    _fields_ = [("struct_bytes", _c.c_int32), ("B", _c.c_int32), ("N", _c.c_int32), ("M", _c.c_int32), ("L", _c.c_int32),
                ("rounds", _c.c_int32), ("transpose_r", _c.c_int32), ("reserved", _c.c_int32),
                ("rng_state", _P), ("radius", _P), ("centers", _P), ("box1", _P), ("box2", _P), ("lines", _P),
                ("filled", _P), ("tile_counts", _P),
                ("src_tri", _P), ("tar_tri", _P), ("R", _P), ("T", _P), ("ws", _P), ("ws_bytes", _Z), ("loss", _P),
                ("grad_loss", _P), ("gR", _P), ("gt", _P), ("opts", _P),
                ("cham_ws", _P), ("cham_ws_bytes", _Z), ("best_x", _P), ("best_y", _P), ("cham_mean", _P), ("value", _P),
                ("xi", _P), ("m", _P), ("v", _P), ("adam_state", _P), ("lr", _P), ("b1", _c.c_double), ("b2", _c.c_double),
                ("eps", _c.c_double), ("gxi", _P), ("table", _P), ("cursor", _P), ("table_rows", _c.c_longlong), ("row", _P)]


class RegisterNewtonArgs(ctypes.Structure):
    """include/rrl.h rrl_register_newton_args (same field order)."""
    _fields_ = [("struct_bytes", _c.c_int32), ("B", _c.c_int32), ("N", _c.c_int32), ("M", _c.c_int32), ("L", _c.c_int32),
                ("rounds", _c.c_int32), ("patience", _c.c_int32), ("reserved", _c.c_int32),
                ("rng_state", _P), ("radius", _P), ("centers", _P), ("box1", _P), ("box2", _P), ("lines", _P),
                ("filled", _P), ("tile_counts", _P),
                ("src_tri", _P), ("tar_tri", _P), ("R", _P), ("T", _P), ("ws", _P), ("ws_bytes", _Z), ("loss", _P), ("opts", _P),
                ("cham_ws", _P), ("cham_ws_bytes", _Z), ("best_x", _P), ("best_y", _P), ("cham_mean", _P), ("value", _P),
                ("neq", _P), ("part", _P), ("part_bytes", _Z),
                ("damping", _P), ("step", _P), ("max_rot", _P), ("max_trans", _P), ("tol_rot", _P), ("tol_trans", _P),
                ("eps", _c.c_double), ("delta", _P), ("last_step", _P), ("state", _P),
                ("table", _P), ("cursor", _P), ("table_rows", _c.c_longlong), ("row", _P)]


class KabschArgs(ctypes.Structure):
    """include/rrl.h rrl_kabsch_args (same field order)."""
    _fields_ = [("struct_bytes", _c.c_int32), ("B", _c.c_int32), ("n", _c.c_int32), ("m", _c.c_int32), ("a_stride", _c.c_int32),
                ("b_stride", _c.c_int32), ("transpose_r", _c.c_int32), ("reserved", _c.c_int32),
                ("a", _P), ("b", _P), ("w", _P), ("keys", _P), ("count_a", _P), ("count_b", _P), ("gate_sq", _P),
                ("eps_w", _c.c_double), ("rank_tol", _c.c_float), ("reserved_f", _c.c_float),
                ("part", _P), ("part_bytes", _Z), ("R", _P), ("T", _P), ("fit", _P), ("info", _P)]


class IcpEpochArgs(ctypes.Structure):
    """include/rrl.h rrl_icp_epoch_args (same field order)."""
    _fields_ = [("struct_bytes", _c.c_int32), ("B", _c.c_int32), ("N", _c.c_int32), ("M", _c.c_int32), ("patience", _c.c_int32),
                ("reserved", _c.c_int32),
                ("src", _P), ("tar", _P), ("count1", _P), ("count2", _P), ("R", _P), ("T", _P), ("moved", _P),
                ("cham_ws", _P), ("cham_ws_bytes", _Z), ("best_x", _P), ("best_y", _P), ("values", _P), ("order_x", _P),
                ("order_y", _P), ("w", _P), ("gate_sq", _P), ("eps_w", _c.c_double), ("rank_tol", _c.c_float),
                ("reserved_f", _c.c_float),
                ("part", _P), ("part_bytes", _Z), ("Rk", _P), ("Tk", _P), ("fit", _P), ("info", _P),
                ("tol_rot", _P), ("tol_trans", _P), ("last_step", _P), ("state", _P),
                ("table", _P), ("cursor", _P), ("table_rows", _c.c_longlong), ("row", _P)]


class SinkhornArgs(ctypes.Structure):
    """include/rrl.h rrl_sinkhorn_args (same field order)."""
    _fields_ = [("struct_bytes", _c.c_int32), ("B", _c.c_int32), ("J", _c.c_int32), ("K", _c.c_int32), ("n_iters", _c.c_int32),
                ("slack", _c.c_int32), ("reserved0", _c.c_int32), ("reserved1", _c.c_int32),
                ("log_alpha", _P), ("xyz_ref", _P), ("count_src", _P), ("count_ref", _P), ("eps", _c.c_double),
                ("ws", _P), ("ws_bytes", _Z), ("W", _P), ("s", _P), ("c", _P), ("log_perm", _P), ("info", _P)]


class PlaneArgs(ctypes.Structure):
    """include/rrl.h rrl_plane_args (same field order)."""
    _fields_ = [("struct_bytes", _c.c_int32), ("B", _c.c_int32), ("N", _c.c_int32), ("M", _c.c_int32), ("tar_stride", _c.c_int32),
                ("reserved", _c.c_int32),
                ("moved", _P), ("keys", _P), ("tar", _P), ("normals", _P), ("count1", _P), ("count2", _P),
                ("w", _P), ("gate_sq", _P), ("pivot", _P),
                ("part", _P), ("part_bytes", _Z), ("neq", _P), ("info", _P)]


class PlaneEpochArgs(ctypes.Structure):
    """include/rrl.h rrl_plane_epoch_args (same field order)."""
    _fields_ = [("struct_bytes", _c.c_int32), ("B", _c.c_int32), ("N", _c.c_int32), ("M", _c.c_int32), ("patience", _c.c_int32),
                ("reserved", _c.c_int32),
                ("src", _P), ("tar", _P), ("normals", _P), ("count1", _P), ("count2", _P), ("R", _P), ("T", _P), ("moved", _P),
                ("cham_ws", _P), ("cham_ws_bytes", _Z), ("best_x", _P), ("best_y", _P), ("values", _P), ("order_x", _P),
                ("order_y", _P), ("w", _P), ("gate_sq", _P), ("pivot", _P),
                ("part", _P), ("part_bytes", _Z), ("neq", _P), ("info", _P),
                ("damping", _P), ("step", _P), ("max_rot", _P), ("max_trans", _P), ("tol_rot", _P), ("tol_trans", _P),
                ("eps", _c.c_double), ("last_step", _P), ("state", _P),
                ("table", _P), ("cursor", _P), ("table_rows", _c.c_longlong), ("row", _P)]


# rrl_kabsch_fwd's fit [B][32] doubles and info[b][1] (include/rrl.h RRL_FIT_*); rrl_icp_step_batch's state[b][3]
FIT_W, FIT_ABAR, FIT_BBAR, FIT_U, FIT_S, FIT_V, FIT_DELTA, FIT_RES, FIT_KEYMEAN, FIT_DOUBLES = 0, 1, 4, 7, 16, 19, 28, 29, 30, 32
FIT_OK, FIT_FEW, FIT_DEGENERATE, ICP_DONE = 0, 1, 2, 3

# rrl_plane_normal_eq's neq [B][32] doubles (include/rrl.h RRL_PLANE_*); rrl_plane_step_batch's state[b][3]
PLANE_H, PLANE_G, PLANE_W, PLANE_RES, PLANE_KEYMEAN, PLANE_USED, PLANE_SKIPPED, PLANE_DOUBLES = 0, 21, 27, 28, 29, 30, 31, 32
PLANE_STEPPED, PLANE_FEW, PLANE_FAILED, PLANE_DONE = 0, 1, 2, 3

# rrl_se3_newton_step_batch's state[b][3] (include/rrl.h RRL_NEWTON_*)
NEWTON_STEPPED, NEWTON_GATED, NEWTON_FAILED, NEWTON_DONE = 0, 1, 2, 3

_lib = None


class RRLError(RuntimeError):
    pass


def load():
    """Load librrl_hip.so; raises RRLError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB):
        raise RRLError(
            f"{LIB} is missing: build it with `python __graft_entry__.py` (hipcc, gfx950). "
            "This package has no CPU or PyTorch fallback.")
    lib = ctypes.CDLL(LIB)
    for name, args in _SIGS.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = _I
    lib.rrl_version.restype = ctypes.c_char_p
    lib.rrl_workspace_bytes.argtypes = [_I, _I, _I, _I]
    lib.rrl_workspace_bytes.restype = _Z
    lib.rrl_wide_workspace_bytes.argtypes = [_I, _I, _I, _I]
    lib.rrl_wide_workspace_bytes.restype = _Z
    lib.rrl_chamfer_workspace_bytes.argtypes = [_I, _I, _I]
    lib.rrl_chamfer_workspace_bytes.restype = _Z
    lib.rrl_cloud_order_workspace_bytes.argtypes = [_I, _I]
    lib.rrl_cloud_order_workspace_bytes.restype = _Z
    lib.rrl_knn3_self_workspace_bytes.argtypes = [_I, _I]
    lib.rrl_knn3_self_workspace_bytes.restype = _Z
    lib.rrl_pose_normal_eq_part_bytes.argtypes = [_I, _I]
    lib.rrl_pose_normal_eq_part_bytes.restype = _Z
    lib.rrl_kabsch_part_bytes.argtypes = [_I, _I]
    lib.rrl_kabsch_part_bytes.restype = _Z
    lib.rrl_sinkhorn_workspace_bytes.argtypes = [_I, _I, _I, _I]
    lib.rrl_sinkhorn_workspace_bytes.restype = _Z
    lib.rrl_plane_part_bytes.argtypes = [_I, _I]
    lib.rrl_plane_part_bytes.restype = _Z
    lib.rrl_sort_capacity.argtypes = []
    lib.rrl_sort_capacity.restype = _I
    _lib = lib
    return lib


def check(rc, what):
    if rc == 0:
        return
    if rc < 0:
        raise RRLError(f"{what}: argument error {rc} (see RRL_E_* in include/rrl.h)")
    raise RRLError(f"{what}: HIP error {rc}")
