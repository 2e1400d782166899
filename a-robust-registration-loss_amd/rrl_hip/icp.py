"""Point-to-point ICP for a BATCH of pairs, one C call per epoch (include/rrl.h rrl_icp_epoch): move
the source by the current pose -> the ragged Chamfer walk (nearest-neighbour keys, and each pair's Chamfer distance for
free) -> the closed-form fit of the source AS GIVEN onto its keyed partners -> the pose step with its stopping rule.

    icp = IcpRegistration(src_tri, tar_tri, counts1=c1, counts2=c2)       # points (B, N, 3) or pseudo-triangles (B, N, 9)
    icp.run(60, check_every=10)
    reg = NewtonRegistration(src_tri, tar_tri, L, R0=icp.R, T0=icp.T)     # the coarse pose starts the fine loop

The closed form has a wide basin where the loops that follow the loss are local; it is the coarse stage, they are the fine one.
Nothing is read back unless .run is asked to check.
"""
import ctypes

import torch

from . import _lib, ops
from .kabsch import RANK_TOL
from .register import PoseLoop, StoppingLoop

# The defaults of the stopping rule, from tools/icp_timing.py (profiles/icp_timing.json: eight make_pair pairs at 20 degrees,
# N = M = 1024).  An ICP pose changes only when a nearest neighbour changes: in that run every step that still moved a pair
# measured >= 2.3e-4 rad and >= 3.5e-5 of the target box's diagonal, and once the pairing had settled the steps were exactly 0
# (the same keys give the same fit, bit for bit).  The tolerances sit between the two; three calm epochs in a row ended the eight
# pairs after 41 ... 85 epochs, 0.3 ... 3.0 degrees from the generating rotation.
TOL_ROT = 1e-4     # radians
TOL_TRANS = 1e-5   # as a fraction of the target box's diagonal
PATIENCE = 3


def check_request(src_shape, tar_shape, capacity, max_dist=None, patience=PATIENCE):
    """The refusals of IcpRegistration that need no GPU (ValueError)."""
    if len(src_shape) != 3 or len(tar_shape) != 3 or src_shape[0] != tar_shape[0] or src_shape[0] < 1:
        raise ValueError("src / tar must be (B, n, 3) points or (B, n, 9) pseudo-triangles with the same B >= 1")
    if src_shape[2] not in (3, 9) or tar_shape[2] not in (3, 9):
        raise ValueError("src / tar rows must be points (.., 3) or pseudo-triangles (.., 9)")
    if src_shape[0] > 32767:
        raise ValueError(f"IcpRegistration serves up to 32767 pairs per batch; got {src_shape[0]}")
    N, M = src_shape[1], tar_shape[1]
    if min(N, M) < 1 or max(N, M) > capacity:
        raise ValueError(f"IcpRegistration serves clouds of 1 .. ops.sort_capacity() = {capacity} points (the Chamfer walk's "
                         f"sorted layout); got {(N, M)}")
    if max_dist is not None and not float(max_dist) > 0.0:
        raise ValueError("max_dist must be positive (a fraction of the target box's diagonal), or None for no gate")
    if int(patience) < 0:
        raise ValueError("patience must be non-negative (0 turns the stopping rule off)")


class IcpRegistration(StoppingLoop, PoseLoop):
    """B pairs src (B, N, 3 or 9) / tar (B, M, 3 or 9); N, M are capacities when counts1 / counts2 are given (both, or one:
    the other is then full).  R0 (B, 3, 3) with T0 (B, 3), or xi0 (B, 6): starting poses (default: the identity); the poses
    move x -> x R + T.  max_dist: partners farther than this fraction of the target box's diagonal get weight 0 (None: no
    gate).  tol_rot (radians), tol_trans (fraction of that diagonal), patience: a pair is done after `patience` epochs in a
    row whose pose moved by less than both (patience = 0: never); a done pair's pose is frozen.  table_rows: epochs logged.

    .R, .T: the poses.  .done_epoch (B,) int32 (-1: not yet), .failed (B,) int32: what the latest epoch did -- 0 stepped, 1
    fewer than 3 pairs, 2 degenerate pairs (pose kept in both), 3 done.  .last_step (B, 2): (angle, centroid motion) of the
    latest step.  .value (B,): each pair's Chamfer distance before the latest step.  All device tensors.
    .history(): PairRegistration's row format -- (epoch, the fit's mean squared residual, the pair's Chamfer distance)."""

    _ARGS, _ENTRY = _lib.IcpEpochArgs, "rrl_icp_epoch"  # .epoch(): ONE C call

    def __init__(self, src, tar, *, counts1=None, counts2=None, R0=None, T0=None, xi0=None, max_dist=None, tol_rot=TOL_ROT,
                 tol_trans=TOL_TRANS, patience=PATIENCE, table_rows=4096):
        if not isinstance(src, torch.Tensor) or not isinstance(tar, torch.Tensor):
            raise TypeError("src / tar must be torch.Tensors")
        self._check_start(R0, T0, xi0)
        if int(table_rows) < 0:
            raise ValueError("table_rows must be non-negative")
        check_request(tuple(src.shape), tuple(tar.shape), ops.sort_capacity(), max_dist, patience)
        dev = self.dev = ops._home(src, tar)
        B, N, M = src.shape[0], src.shape[1], tar.shape[1]
        self.B, self.N, self.M = B, N, M
        f32 = dict(dtype=torch.float32, device=dev)
        s, t = ops._prep(src, "src", None, dev), ops._prep(tar, "tar", None, dev)
        self.src, self.tar = s[:, :, :3].contiguous(), t[:, :, :3].contiguous()
        ragged = counts1 is not None or counts2 is not None
        self.counts1 = self.counts2 = None
        if ragged:
            self.counts1 = ops.check_counts(counts1 if counts1 is not None else [N] * B, B, N, dev, "counts1")
            self.counts2 = ops.check_counts(counts2 if counts2 is not None else [M] * B, B, M, dev, "counts2")

        def order(pts, tri, counts):  # ops.cloud_order(counts=) takes 9-wide rows: made once, here
            if counts is None:
                return ops.cloud_order(pts)
            if tri.shape[2] != 9:
                tri = torch.zeros(pts.shape[0], pts.shape[1], 9, **f32)
                tri[:, :, :3] = pts
            return ops.cloud_order(tri, counts=counts)
        self.order_x, self.order_y = order(self.src, s, self.counts1), order(self.tar, t, self.counts2)
        self.box2 = ops.aabb(self.tar, self.counts2)
        self.radius = (self.box2[:, 3:] - self.box2[:, :3]).norm(p=2, dim=1).contiguous()
        self._start_poses(R0, T0, xi0)
        self._init_stop(tol_rot, tol_trans, patience)
        self.gate_sq = (self._per_pair(max_dist, self.radius) ** 2).contiguous() if max_dist is not None else None
        lib = _lib.load()
        self.moved = torch.empty(B, N, 3, **f32)
        self.cham_ws = torch.empty(int(lib.rrl_chamfer_workspace_bytes(B, N, M)), dtype=torch.uint8, device=dev)
        self.best_x = torch.empty(B, N, dtype=torch.int64, device=dev)
        self.best_y = torch.empty(B, M, dtype=torch.int64, device=dev)
        self.value = torch.zeros(B, **f32)
        self.part = torch.empty(max(int(lib.rrl_kabsch_part_bytes(B, N)) // 8, 1), dtype=torch.float64, device=dev)
        self.Rk, self.Tk = torch.zeros(B, 3, 3, **f32), torch.zeros(B, 3, **f32)
        self.fit = torch.zeros(B, _lib.FIT_DOUBLES, dtype=torch.float64, device=dev)
        self.info = torch.zeros(B, 4, dtype=torch.int32, device=dev)
        self._init_log(table_rows)
        self._bind()

    def _make_args(self):
        P = ops._p
        a = self._ARGS()
        a.struct_bytes = ctypes.sizeof(a)
        a.B, a.N, a.M = self.B, self.N, self.M
        a.src, a.tar, a.count1, a.count2 = P(self.src), P(self.tar), P(self.counts1), P(self.counts2)
        a.R, a.T, a.moved = P(self.R), P(self.T), P(self.moved)
        a.cham_ws, a.cham_ws_bytes, a.best_x, a.best_y, a.values = P(self.cham_ws), self.cham_ws.numel(), P(self.best_x), P(self.best_y), P(self.value)
        a.order_x, a.order_y = P(self.order_x), P(self.order_y)
        a.w, a.gate_sq, a.eps_w, a.rank_tol = None, P(self.gate_sq), 0.0, RANK_TOL
        a.part, a.part_bytes = P(self.part), self.part.numel() * 8
        a.Rk, a.Tk, a.fit, a.info = P(self.Rk), P(self.Tk), P(self.fit), P(self.info)
        self._stop_args(a)
        self._log_args(a)
        return a

    def moved_points(self):
        """(B, N, 3): the source points under the CURRENT pose (one rigid apply; rows beyond a count are not meaningful)."""
        out = torch.empty_like(self.moved)
        ops._run(self.dev, "rrl_rigid_apply_fwd", ops._p(self.src), ops._p(self.R), ops._p(self.T), ops._p(out), self.B, self.N, 0, 0)
        return out


def icp_pairs(src, tar, n_epoch=60, check_every=0, **kw):
    """IcpRegistration(...).run(n_epoch, check_every) -> (R (B, 3, 3), T (B, 3), history)."""
    reg = IcpRegistration(src, tar, **kw)
    reg.run(n_epoch, check_every)
    return reg.R, reg.T, reg.history()
