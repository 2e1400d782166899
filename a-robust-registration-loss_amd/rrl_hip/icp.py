"""Point-to-point ICP for a BATCH of pairs, one C call per epoch (include/rrl.h rrl_icp_epoch): move
the source by the current pose -> the ragged Chamfer walk (nearest-neighbour keys, and each pair's Chamfer distance for
free) -> the closed-form fit of the source AS GIVEN onto its keyed partners -> the pose step with its stopping rule.

    icp = IcpRegistration(src_tri, tar_tri, counts1=c1, counts2=c2)       # points (B, N, 3) or pseudo-triangles (B, N, 9)
    icp.run(60, check_every=10)
    reg = NewtonRegistration(src_tri, tar_tri, L, R0=icp.R, T0=icp.T)     # the coarse pose starts the fine loop

The closed form has a wide basin where the loops that follow the loss are local; it is the coarse stage, they are the fine one.
Nothing is read back unless .run is asked to check.

PlaneIcpRegistration is the point-to-plane form of the same epoch (include/rrl.h rrl_plane_icp_epoch): the
fit is one damped Gauss-Newton step of the distances to the target's tangent planes, which lets a surface slide along itself
where point-to-point pairs hold it back.

    icp = PlaneIcpRegistration(src, tar, normals_tar)                     # or normal_radius=0.25: normals estimated once
    icp.run(20, check_every=5)
"""
import ctypes

import torch

from . import _lib, ops
from .kabsch import RANK_TOL
from .newton import DAMPING, MAX_ROT, MAX_TRANS, STEP
from .newton import EPS as NEWTON_EPS
from .register import PoseLoop, StoppingLoop

# The defaults of the stopping rule, from tools/icp_timing.py (profiles/icp_timing.json: eight make_pair pairs at 20 degrees,
# N = M = 1024).  An ICP pose changes only when a nearest neighbour changes: in that run every step that still moved a pair
# measured >= 2.3e-4 rad and >= 3.5e-5 of the target box's diagonal, and once the pairing had settled the steps were exactly 0
# (the same keys give the same fit, bit for bit).  The tolerances sit between the two; three calm epochs in a row ended the eight
# pairs after 41 ... 85 epochs, 0.3 ... 3.0 degrees from the generating rotation.
TOL_ROT = 1e-4     # radians
TOL_TRANS = 1e-5   # as a fraction of the target box's diagonal
PATIENCE = 3

# PlaneIcpRegistration's step controls are NewtonRegistration's (rrl_hip.newton).  Its stopping tolerances, from
# tools/plane_icp_timing.py (profiles/plane_icp_timing.json: eight make_pair pairs at 20 degrees, N = M = 1024): a damped
# Gauss-Newton step shrinks about tenfold per epoch once the pairing has settled (down to the float32 rounding of the pose, 1e-8 ...
# 4e-7 rad), so three calm epochs in a row mean the same pose under any tolerance below the first of them; but a pairing can
# also settle into a cycle of a few pairs, which moved one of the eight poses by 3.2e-4 ... 3.8e-4 rad and 2.8e-5 ... 4.8e-5 of
# the diagonal per epoch for good, 0.02 degrees about a pose 0.15 degrees from the generating rotation.  IcpRegistration's values
# (1e-4, 1e-5) sit below that cycle and never end such a pair; these sit above it and below every step that still converged.
PLANE_TOL_ROT = 1e-3     # radians
PLANE_TOL_TRANS = 1e-4   # as a fraction of the target box's diagonal


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


class _CloudLoop(StoppingLoop, PoseLoop):
    """What the two ICP loops share: the request's refusals, the clouds' first points with their counts, prepared orders and
    the target's box, the starting poses, the stopping rule, the gate and the Chamfer walk's buffers."""

    def _init_clouds(self, src, tar, counts1, counts2, R0, T0, xi0, max_dist, tol_rot, tol_trans, patience, table_rows):
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
        return lib

    def _cloud_args(self, a):
        """The fields both epoch structs name alike."""
        P = ops._p
        a.struct_bytes = ctypes.sizeof(a)
        a.B, a.N, a.M = self.B, self.N, self.M
        a.src, a.tar, a.count1, a.count2 = P(self.src), P(self.tar), P(self.counts1), P(self.counts2)
        a.R, a.T, a.moved = P(self.R), P(self.T), P(self.moved)
        a.cham_ws, a.cham_ws_bytes, a.best_x, a.best_y, a.values = P(self.cham_ws), self.cham_ws.numel(), P(self.best_x), P(self.best_y), P(self.value)
        a.order_x, a.order_y = P(self.order_x), P(self.order_y)
        a.w, a.gate_sq = None, P(self.gate_sq)
        self._stop_args(a)
        self._log_args(a)

    def moved_points(self):
        """(B, N, 3): the source points under the CURRENT pose (one rigid apply; rows beyond a count are not meaningful)."""
        out = torch.empty_like(self.moved)
        ops._run(self.dev, "rrl_rigid_apply_fwd", ops._p(self.src), ops._p(self.R), ops._p(self.T), ops._p(out), self.B, self.N, 0, 0)
        return out


class IcpRegistration(_CloudLoop):
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
        lib = self._init_clouds(src, tar, counts1, counts2, R0, T0, xi0, max_dist, tol_rot, tol_trans, patience, table_rows)
        self._init_fit(lib, table_rows)

    def _init_fit(self, lib, table_rows):
        """The closed-form fit's buffers, the log and the bound call: what a constructor does last."""
        B, dev, f32 = self.B, self.dev, dict(dtype=torch.float32, device=self.dev)
        self.part = torch.empty(max(int(lib.rrl_kabsch_part_bytes(B, self.N)) // 8, 1), dtype=torch.float64, device=dev)
        self.Rk, self.Tk = torch.zeros(B, 3, 3, **f32), torch.zeros(B, 3, **f32)
        self.fit = torch.zeros(B, _lib.FIT_DOUBLES, dtype=torch.float64, device=dev)
        self.info = torch.zeros(B, 4, dtype=torch.int32, device=dev)
        self._init_log(table_rows)
        self._bind()

    def _make_args(self):
        P = ops._p
        a = self._ARGS()
        self._cloud_args(a)
        a.eps_w, a.rank_tol = 0.0, RANK_TOL
        a.part, a.part_bytes = P(self.part), self.part.numel() * 8
        a.Rk, a.Tk, a.fit, a.info = P(self.Rk), P(self.Tk), P(self.fit), P(self.info)
        return a


def icp_pairs(src, tar, n_epoch=60, check_every=0, **kw):
    """IcpRegistration(...).run(n_epoch, check_every) -> (R (B, 3, 3), T (B, 3), history)."""
    reg = IcpRegistration(src, tar, **kw)
    reg.run(n_epoch, check_every)
    return reg.R, reg.T, reg.history()


# ---- robust ICP: Welsch weights with an annealed scale (include/rrl.h rrl_robust_icp_epoch) ----------
# The defaults are the settings of the float64 twin's acceptance run (tests/robust_refs.py outlier_pair: a 10 degree pose, 20 %
# of the source replaced by uniform outliers): at a starting scale of three median residuals a pair at the median still weighs
# exp(-1 / 18), halving reaches the end scale in four or five levels, and the level cap ends a level whose
# pairing cycles instead of settling.
NU_START = 3.0    # times the first epoch's median residual
ANNEAL = 0.5
LEVEL_CAP = 10    # epochs at one scale, at the most (0: no cap)


def check_robust_request(nu_start=NU_START, nu_end=None, anneal=ANNEAL, level_cap=LEVEL_CAP, patience=PATIENCE, B=None):
    """The refusals of RobustIcpRegistration beyond check_request's that need no GPU (ValueError)."""
    if not float(nu_start) > 0.0:
        raise ValueError("nu_start must be positive (a multiple of the first epoch's median residual)")
    if not 0.0 < float(anneal) < 1.0:
        raise ValueError("anneal must lie in (0, 1): the factor a settled pair's scale is multiplied by")
    if isinstance(level_cap, bool) or int(level_cap) != level_cap or int(level_cap) < 0:
        raise ValueError("level_cap must be a non-negative integer (0: no cap)")
    if int(patience) <= 0 and int(level_cap) == 0:
        raise ValueError("patience = 0 with level_cap = 0: no level would ever end, nothing would anneal")
    if nu_end is not None:
        ends = nu_end.detach().reshape(-1).tolist() if isinstance(nu_end, torch.Tensor) else \
            [float(x) for x in (nu_end if isinstance(nu_end, (list, tuple)) else [nu_end])]
        if B is not None and len(ends) not in (1, int(B)):
            raise ValueError(f"nu_end must be a number or one per pair ({B}); got {len(ends)}")
        if not all(x > 0.0 for x in ends):
            raise ValueError("nu_end must be positive (the final scale, in the clouds' units), or None for the target's spacing")


def target_spacing(tar, counts=None):
    """(B,) float32: per cloud, the lower median distance from a point to its nearest OTHER point of the cloud (tar (B, M, 3),
    counts (B,) int32 or None), from the library's own 3-NN; 0 where no point has another (a capacity below three, a count below two)."""
    from .neighbors import knn3_self
    B, M = tar.shape[0], tar.shape[1]
    if M < 3:
        return torch.zeros(B, dtype=torch.float32, device=tar.device)
    nn = knn3_self(tar, counts=counts).to(torch.int64)
    rows = torch.arange(M, device=tar.device)[None, :, None]
    d = (tar[torch.arange(B, device=tar.device)[:, None, None], nn] - tar[:, :, None, :]).norm(dim=3)  # (B, M, 3)
    inf = torch.full_like(d[:, :, 0], float("inf"))
    d = torch.where(nn == rows, float("inf"), d).amin(dim=2)  # (the point itself is among its three nearest)
    if counts is not None:
        d = torch.where(rows[:, :, 0] < counts[:, None], d, inf)
    d = torch.where(torch.isfinite(d), d, inf)  # (NaN filler, a cloud of one point's copies)
    k = torch.isfinite(d).sum(1)
    med = torch.gather(torch.sort(d, dim=1).values, 1, ((k - 1).clamp(min=0) // 2)[:, None])[:, 0]
    return torch.where(k > 0, med, torch.zeros_like(med)).contiguous()


class RobustIcpRegistration(IcpRegistration):
    """IcpRegistration whose pairs carry Welsch weights exp(-d^2 / (2 nu^2)) -- the loss's own function of the nearest
    neighbour's distance d -- with a per-pair scale nu annealed from coarse to fine (Fast-Robust-ICP without its Anderson
    acceleration): source points with no partner in the target fade out instead of pulling the pose.  One C call per epoch.

    src, tar, counts1, counts2, R0 / T0 / xi0, max_dist, tol_rot, tol_trans, patience, table_rows: as IcpRegistration; here
    `patience` calm epochs end a LEVEL, and the pair is done when a level ends at the final scale.
    nu_start: the first epoch sets nu = nu_start x the median residual of its pairing (never below nu_end).  nu_end: the
    final scale, a number or one per pair, in the clouds' units; None: each target's median nearest-neighbour spacing over
    3 sqrt(3), computed once here.  anneal: the factor of a level's end.  level_cap: a level also ends after this many epochs
    (0: only by patience).

    .nu (B,): the current scales; .weights (B, N): the latest epoch's weights (0 on rows without a partner); .levels (B,)
    int32: levels finished; .level (B, 2) int32: (epochs at this scale, levels finished); .med_sq (B,): the first epoch's median
    squared residual.  Everything else as IcpRegistration; .history()'s residual is the fit's WEIGHTED mean squared residual."""

    _ENTRY = "rrl_robust_icp_epoch"  # .epoch(): ONE C call, on rrl_icp_epoch's own struct (_ARGS)

    def __init__(self, src, tar, *, counts1=None, counts2=None, R0=None, T0=None, xi0=None, max_dist=None, tol_rot=TOL_ROT,
                 tol_trans=TOL_TRANS, patience=PATIENCE, table_rows=4096, nu_start=NU_START, nu_end=None, anneal=ANNEAL,
                 level_cap=LEVEL_CAP):
        check_robust_request(nu_start, nu_end, anneal, level_cap, patience,
                             src.shape[0] if isinstance(src, torch.Tensor) and src.dim() == 3 else None)
        lib = self._init_clouds(src, tar, counts1, counts2, R0, T0, xi0, max_dist, tol_rot, tol_trans, patience, table_rows)
        B, dev, f32 = self.B, self.dev, dict(dtype=torch.float32, device=self.dev)
        self.nu_start, self.anneal, self.level_cap = float(nu_start), float(anneal), int(level_cap)
        if nu_end is None:
            self.nu_end = (target_spacing(self.tar, self.counts2) / (3.0 * 3.0 ** 0.5)).contiguous()
        else:
            self.nu_end = self._per_pair(nu_end)
        self.nu = self.nu_end.clone()
        self.weights = torch.zeros(B, self.N, **f32)
        self.med_sq = torch.zeros(B, **f32)
        self.med_info = torch.zeros(B, 2, dtype=torch.int32, device=dev)
        self.level = torch.zeros(B, 2, dtype=torch.int32, device=dev)
        self._init_fit(lib, table_rows)

    def _make_args(self):
        P = ops._p
        a = super()._make_args()
        # what the annealing adds travels as plain arguments, after `init`; the struct's w stays NULL
        self._extra = (P(self.weights), P(self.nu), P(self.nu_end), P(self.med_sq), P(self.med_info), self.nu_start, self.anneal,
                       self.level_cap, P(self.level))
        return a

    def epoch(self):
        """One epoch of all B pairs: ONE C call, nothing read back.  The first sets the starting scales from its own pairing
        (init = 1); every later one is the steady epoch, which is what a graph captured after the first replays."""
        with ops._guard(self.dev):
            _lib.check(self._call(self._aref, 1 if self.epochs == 0 else 0, *self._extra, ops._stream(self.dev)), self._ENTRY)
        self.epochs += 1

    @property
    def levels(self):
        return self.level[:, 1]


def robust_icp_pairs(src, tar, n_epoch=80, check_every=0, **kw):
    """RobustIcpRegistration(...).run(n_epoch, check_every) -> (R (B, 3, 3), T (B, 3), history)."""
    reg = RobustIcpRegistration(src, tar, **kw)
    reg.run(n_epoch, check_every)
    return reg.R, reg.T, reg.history()


def check_plane_request(tar_shape, normals_shape, normal_radius, nsample, eps=NEWTON_EPS):
    """The refusals of PlaneIcpRegistration beyond check_request's that need no GPU (ValueError)."""
    if normals_shape is None and normal_radius is None:
        raise ValueError("PlaneIcpRegistration needs the target's normals: give normals (B, M, 3), or normal_radius to "
                         "estimate them (neighbors.estimate_normals); no radius is assumed")
    if normals_shape is not None and tuple(normals_shape) != (tar_shape[0], tar_shape[1], 3):
        raise ValueError(f"normals must be (B, M, 3) = {(tar_shape[0], tar_shape[1], 3)}, one per target point; got {tuple(normals_shape)}")
    if normals_shape is None:
        if not float(normal_radius) > 0.0:
            raise ValueError("normal_radius must be positive")
        if isinstance(nsample, bool) or int(nsample) != nsample or not 3 <= int(nsample) <= _lib.GROUP_MAX_SAMPLE:
            raise ValueError(f"nsample must be an integer in [3, {_lib.GROUP_MAX_SAMPLE}] (a plane needs three members)")
    if not float(eps) >= 0.0:
        raise ValueError("eps must be non-negative")


class PlaneIcpRegistration(_CloudLoop):
    """Point-to-plane ICP for a batch of pairs, one C call per epoch (include/rrl.h rrl_plane_icp_epoch; DESIGN.md section
    19): move the source -> the ragged Chamfer walk -> the sums of the fit linearised about the current pose, each source
    point against the PLANE of its nearest target point -> one damped Gauss-Newton pose step about the target box's centre.
    Where point-to-point pairs hold a surface back from sliding along itself, the plane residual lets it: a handful of
    epochs where IcpRegistration takes tens.

    src, tar, counts1, counts2, R0 / T0 / xi0, max_dist, tol_rot, tol_trans, patience, table_rows: as IcpRegistration.
    normals (B, M, 3): the TARGET's normals (a dataset's normals_tar; unit length, any orientation; a zero or non-finite row
    takes its point out of the fit).  Without them, normal_radius (in the clouds' units) and nsample estimate them once with
    neighbors.estimate_normals(tar, normal_radius, nsample, counts=counts2); giving neither is a ValueError.
    damping, step, max_rot, max_trans, eps: NewtonRegistration's step controls with its defaults (a number or one per pair;
    max_trans is a fraction of the target box's diagonal).

    .R, .T, .done_epoch, .last_step ((|omega|, |v|) of the latest step), .value, .history() (epoch, the mean squared plane
    residual, the pair's Chamfer distance), .moved_points(): as IcpRegistration.  .normals (B, M, 3): the normals in use.
    .failed (B,) int32: 0 stepped, 1 fewer than 6 usable pairs, 2 a singular or non-finite system (pose kept in both), 3 done."""

    _ARGS, _ENTRY = _lib.PlaneEpochArgs, "rrl_plane_icp_epoch"  # .epoch(): ONE C call

    def __init__(self, src, tar, normals=None, *, normal_radius=None, nsample=64, counts1=None, counts2=None, R0=None, T0=None,
                 xi0=None, max_dist=None, damping=DAMPING, step=STEP, max_rot=MAX_ROT, max_trans=MAX_TRANS, eps=NEWTON_EPS,
                 tol_rot=PLANE_TOL_ROT, tol_trans=PLANE_TOL_TRANS, patience=PATIENCE, table_rows=4096):
        if not isinstance(tar, torch.Tensor):
            raise TypeError("src / tar must be torch.Tensors")
        check_plane_request(tuple(tar.shape), None if normals is None else tuple(normals.shape), normal_radius, nsample, eps)
        lib = self._init_clouds(src, tar, counts1, counts2, R0, T0, xi0, max_dist, tol_rot, tol_trans, patience, table_rows)
        B, dev = self.B, self.dev
        if normals is not None:
            self.normals = ops._prep(normals, "normals", 3, dev).reshape(B, self.M, 3).contiguous()
        else:
            from .neighbors import estimate_normals
            self.normals = estimate_normals(self.tar, float(normal_radius), int(nsample), counts=self.counts2)
        centre = 0.5 * (self.box2[:, :3] + self.box2[:, 3:])  # (an empty target's box is (+inf, -inf): the origin)
        self.pivot = torch.where(torch.isfinite(centre), centre, torch.zeros_like(centre)).contiguous()
        self.damping, self.step_scale = self._per_pair(damping), self._per_pair(step)
        self.max_rot, self.max_trans = self._per_pair(max_rot), self._per_pair(max_trans, self.radius)
        self.eps = float(eps)
        self.part = torch.empty(max(int(lib.rrl_plane_part_bytes(B, self.N)) // 8, 1), dtype=torch.float64, device=dev)
        self.neq = torch.zeros(B, _lib.PLANE_DOUBLES, dtype=torch.float64, device=dev)
        self.info = torch.zeros(B, 4, dtype=torch.int32, device=dev)
        self._init_log(table_rows)
        self._bind()

    def _make_args(self):
        P = ops._p
        a = self._ARGS()
        self._cloud_args(a)
        a.normals, a.pivot = P(self.normals), P(self.pivot)
        a.part, a.part_bytes, a.neq, a.info = P(self.part), self.part.numel() * 8, P(self.neq), P(self.info)
        a.damping, a.step, a.max_rot, a.max_trans, a.eps = P(self.damping), P(self.step_scale), P(self.max_rot), P(self.max_trans), self.eps
        return a


def plane_icp_pairs(src, tar, normals=None, n_epoch=20, check_every=0, **kw):
    """PlaneIcpRegistration(...).run(n_epoch, check_every) -> (R (B, 3, 3), T (B, 3), history)."""
    reg = PlaneIcpRegistration(src, tar, normals, **kw)
    reg.run(n_epoch, check_every)
    return reg.R, reg.T, reg.history()
