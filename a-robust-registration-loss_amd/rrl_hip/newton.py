"""Registration of a BATCH of pairs by damped Gauss-Newton steps on the loss's own pairs -- the second-order companion of
rrl_hip.register (include/rrl.h rrl_register_newton_epoch: line sampler -> registration forward ->
optional Chamfer monitor -> normal equations -> batched Gauss-Newton pose step, one C call per epoch).

    reg = NewtonRegistration(src_tri, tar_tri, 4000, counts1=c1, counts2=c2)   # (B, N, 9), (B, M, 9): capacities
    reg.run(200, check_every=10)                                               # returns early when every pair is done
    R, T, done = reg.R, reg.T, reg.done_epoch

With the weights, the median and the labels frozen for one step -- they carry no gradient in the loss either -- the loss is a
weighted sum of squared point distances, and one step is one IRLS step of a Welsch-weighted point-to-point fit: tens of epochs
where the first-order loop takes a thousand, and a step whose length means something, so that "converged" is decided on the
device (`patience` consecutive epochs below tol_rot / tol_trans).  Nothing is read back unless .run is asked to check.
"""
import torch

from . import _lib, ops
from .register import PairRegistration, StoppingLoop

# The defaults, from the sweep of tools/register_newton_sweep.py (profiles/register_newton_sweep.json)
DAMPING = 1e-2     # Levenberg-Marquardt: H + damping diag(H)
STEP = 1.0         # fraction of the solved step that is applied
MAX_ROT = 0.2      # radians per epoch
MAX_TRANS = 0.1    # per epoch, as a fraction of the sampler radius (the target box's diagonal)
TOL_ROT = 5e-3     # radians: an epoch below both tolerances is calm (the line sets' own noise moves a converged pose by
                   # 3e-3 .. 4e-3 rad and 7e-4 .. 9e-4 of the radius per epoch at 20000 lines: the sweep's tail columns)
TOL_TRANS = 1.5e-3  # as a fraction of the sampler radius
PATIENCE = 3       # calm epochs in a row that end a pair
EPS = 1e-12        # H + eps I: a pivot that does not exceed it fails the step


class NewtonRegistration(StoppingLoop, PairRegistration):
    """PairRegistration's constructor contract, sampler geometry, .history(), .moved_points(), .loss, .R, .T -- with
    Gauss-Newton steps in place of Adam on se(3).

    Starting poses: R0 (B, 3, 3) and T0 (B, 3), or xi0 (B, 6) (default: the identity).  damping, step, max_rot, max_trans,
    tol_rot, tol_trans: a number or one per pair; max_trans and tol_trans are FRACTIONS of each pair's sampler radius (the
    target box's diagonal), multiplied once here.  patience = 0 turns the stopping rule off.

    .done_epoch (B,) int32: the number of epochs after which pair b was declared done, or -1; a done pair's pose is frozen.
    .last_step (B, 2): (|omega|, |v|) of the latest applied step.  .failed (B,) int32: what the latest epoch did per pair --
    0 stepped, 1 no populated bucket, 2 the factorisation failed (pose unchanged), 3 done.  All device tensors."""

    _ARGS, _ENTRY = _lib.RegisterNewtonArgs, "rrl_register_newton_epoch"

    def __init__(self, src_tri, tar_tri, n_lines, *, counts1=None, counts2=None, R0=None, T0=None, xi0=None, damping=DAMPING,
                 step=STEP, max_rot=MAX_ROT, max_trans=MAX_TRANS, tol_rot=TOL_ROT, tol_trans=TOL_TRANS, patience=PATIENCE,
                 eps=EPS, rounds=10, seed=None, lines=None, monitor=False, table_rows=4096):
        self._check_start(R0, T0, xi0)
        if int(patience) < 0 or not float(eps) >= 0.0:
            raise ValueError("patience and eps must be non-negative")
        pose = dict(R0=R0, T0=T0, xi0=xi0, damping=damping, step=step, max_rot=max_rot, max_trans=max_trans, tol_rot=tol_rot,
                    tol_trans=tol_trans, patience=patience, eps=eps)
        self._build(src_tri, tar_tri, n_lines, counts1=counts1, counts2=counts2, rounds=rounds, seed=seed, monitor=monitor,
                    deterministic=None, table_rows=table_rows, lines=lines, pose=pose)

    def _init_pose_side(self, R0, T0, xi0, damping, step, max_rot, max_trans, tol_rot, tol_trans, patience, eps):
        """The second-order state: (R, T) as given or exp(xi0), the controls one per pair, the normal equations with their
        scratch, the step's outputs and the stopping rule's state."""
        dev, B, per_pair = self.dev, self.B, self._per_pair
        f32 = dict(dtype=torch.float32, device=dev)
        self._start_poses(R0, T0, xi0)
        self.damping, self.step_scale = per_pair(damping), per_pair(step)
        self.max_rot, self.max_trans = per_pair(max_rot), per_pair(max_trans, self.radius)
        self._init_stop(tol_rot, tol_trans, patience)
        self.eps = float(eps)
        self.neq = torch.zeros(B, 16, **f32)
        self.part = ops.pose_normal_eq_part(B, self.step.dims[3], dev)
        self.delta = torch.zeros(B, 6, **f32)

    def _pose_args(self, a):
        P = ops._p
        self._stop_args(a)
        a.eps = self.eps
        a.neq, a.part, a.part_bytes = P(self.neq), P(self.part), self.part.numel() * 8
        a.damping, a.step, a.max_rot, a.max_trans = P(self.damping), P(self.step_scale), P(self.max_rot), P(self.max_trans)
        a.delta = P(self.delta)

    def set_lr(self, lr):
        raise AttributeError("NewtonRegistration has no learning rate: see damping / step")

    def epoch(self):
        """One epoch of all B pairs: ONE C call (rrl_register_newton_epoch), nothing read back."""
        super().epoch()

    def xi(self):
        """(B, 6) on the host: LieAlgebra.se3.log of the current poses (rrl_se3_exp of it gives R, T back), on request."""
        from LieAlgebra import se3
        g = torch.zeros(self.B, 4, 4, dtype=torch.float64)
        g[:, :3, :3], g[:, :3, 3], g[:, 3, 3] = self.R.double().cpu(), self.T.double().cpu(), 1.0
        return se3.log(g).to(torch.float32)


def register_pairs_newton(src_tri, tar_tri, n_lines, n_epoch=100, check_every=0, **kw):
    """NewtonRegistration(...).run(n_epoch, check_every) -> (R (B, 3, 3), T (B, 3), history)."""
    reg = NewtonRegistration(src_tri, tar_tri, n_lines, **kw)
    reg.run(n_epoch, check_every)
    return reg.R, reg.T, reg.history()
