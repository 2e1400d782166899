"""Registration of a BATCH of pairs by direct optimisation of one se(3) vector per pair -- the loop of
test_demo_optimized_Lie_Algebra.py for B pairs at once, ragged or not, one C call per epoch (include/rrl.h
rrl_register_epoch: line sampler -> fused registration step -> optional Chamfer monitor -> batched pose step).

    reg = PairRegistration(src_tri, tar_tri, 4000, counts1=c1, counts2=c2)   # (B, N, 9), (B, M, 9): capacities
    reg.run(1000)                                                            # the demo's learning-rate schedule
    R, T, history = reg.R, reg.T, reg.history()

or `register_pairs(src_tri, tar_tri, 4000, n_epoch=1000, ...)`.  Sample b of the batch computes what the demo's one-call
epoch computes for that pair alone with the same lines; nothing is read back before .history().
"""
import ctypes

import torch

from . import _lib, ops

DEMO_LR = 2e-2  # test_demo_optimized_Lie_Algebra.py: torch.optim.Adam(lr=2e-2), halved whenever epoch % 1000 == 0


def scheduled_lr(epoch, lr):
    """The demo's adjust_learning_rate as a function: the rate of `epoch` from the rate before it (halved when
    epoch % 1000 == 0 -- at epoch 0 too)."""
    return lr * 0.5 if epoch % 1000 == 0 else lr


def check_request(N, M, ragged, monitor, capacity):
    """The refusals of PairRegistration that need no GPU (ValueError naming the alternative)."""
    if max(N, M) > capacity:
        raise ValueError(f"PairRegistration serves clouds up to ops.sort_capacity() = {capacity} triangles (prepared orders, "
                         f"the sorted layout); got {max(N, M)}: register larger pairs one by one with ops.RegistrationStep("
                         "prepared=False) and ops.se3_adam_step")
    if monitor and ragged:
        raise ValueError("monitor=True with counts1 / counts2: the step's Chamfer walk reads whole clouds and must not run on "
                         "a ragged workspace; evaluate ops.chamfer(reg.moved_points(), target first points, counts_x=counts1, "
                         "counts_y=counts2, per_sample=True) instead")


class PoseLoop:
    """What every batched pose loop is made of besides its own epoch: per-pair controls, starting poses, the log table with
    .history(), and the one C call per epoch (the struct _ARGS filled by the subclass's _make_args, passed to _ENTRY).  The
    subclass sets .dev and .B first."""

    _ARGS = _ENTRY = None
    monitor = True  # the log's value column is reported by .history() (the loss loops: only when they were asked to monitor)

    def _per_pair(self, x, scale=None):
        """A number or a tensor -> contiguous float32 (B,), times `scale` (B,) where one is given (the sampler radius)."""
        t = x.detach() if isinstance(x, torch.Tensor) else torch.as_tensor(x, dtype=torch.float32)
        t = t.to(dtype=torch.float32, device=self.dev).reshape(-1).expand(self.B).clone()
        return (t * scale if scale is not None else t).contiguous()

    @staticmethod
    def _check_start(R0, T0, xi0):
        if (R0 is None) != (T0 is None) or (R0 is not None and xi0 is not None):
            raise ValueError("starting poses: R0 and T0 together, or xi0, not both")

    def _pose_from_xi(self, xi):
        """(R, T) = exp(xi), per pair."""
        ops._run(self.dev, "rrl_se3_exp", ops._p(xi), ops._p(self.R), ops._p(self.T), self.B)

    def _start_poses(self, R0=None, T0=None, xi0=None):
        """.R (B, 3, 3), .T (B, 3): R0 and T0 as given, else exp(xi0) (default: the identity); returns the xi used, or None."""
        B, dev, f32 = self.B, self.dev, dict(dtype=torch.float32, device=self.dev)
        self.R, self.T = torch.empty(B, 3, 3, **f32), torch.empty(B, 3, **f32)
        if R0 is not None:
            self.R.copy_(ops._prep(R0, "R0", 3, dev).reshape(B, 3, 3))
            self.T.copy_(ops._prep(T0, "T0", 3, dev).reshape(B, 3))
            return None
        xi = torch.zeros(B, 6, **f32) if xi0 is None else ops._prep(xi0, "xi0", 6, dev).reshape(B, 6)
        self._pose_from_xi(xi)
        return xi

    def _init_log(self, table_rows):
        f32 = dict(dtype=torch.float32, device=self.dev)
        self.table = torch.zeros(int(table_rows), self.B, 3, **f32)
        self.cursor = torch.zeros(self.B, dtype=torch.int64, device=self.dev)
        self.row = torch.zeros(self.B, 3, **f32)

    def _log_args(self, a):
        a.table, a.cursor, a.table_rows, a.row = ops._p(self.table), ops._p(self.cursor), self.table.shape[0], ops._p(self.row)

    def _bind(self):
        """Last in a constructor: the argument struct, its reference and the entry, looked up once."""
        self.epochs = 0  # epochs issued (the schedule's clock)
        self._args = self._make_args()
        self._aref = ctypes.byref(self._args)
        self._call = getattr(_lib.load(), self._ENTRY)

    def epoch(self):
        """One epoch of all B pairs: ONE C call, nothing read back."""
        with ops._guard(self.dev):
            _lib.check(self._call(self._aref, ops._stream(self.dev)), self._ENTRY)
        self.epochs += 1

    def history(self):
        """[per pair][(epoch, loss or None, value or None)] of the logged epochs, read from the device table once; value is
        the pair's Chamfer distance with monitor=True, else None.  An epoch whose loss had no populated bucket: (e, None, None).
        IcpRegistration: the fit's mean squared residual and, always, the Chamfer distance; an epoch whose fit failed: (e, None, None)."""
        n = min(self.epochs, self.table.shape[0])
        rows = self.table[:n].cpu().tolist()
        out = [[] for _ in range(self.B)]
        for e, per in enumerate(rows):
            for b, (di, cf, ok) in enumerate(per):
                out[b].append((e, di, cf if self.monitor else None) if ok else (e, None, None))
        return out


class StoppingLoop:
    """For a PoseLoop whose step stops by itself (include/rrl.h, the pose-step state): the tolerances, the state words and
    last_step, .done_epoch, .failed and the .run that may return early."""

    def _init_stop(self, tol_rot, tol_trans, patience):
        """tol_trans is a FRACTION of each pair's sampler radius (.radius), multiplied once here."""
        self.tol_rot, self.tol_trans = self._per_pair(tol_rot), self._per_pair(tol_trans, self.radius)
        self.patience = int(patience)
        self.last_step = torch.zeros(self.B, 2, dtype=torch.float32, device=self.dev)
        self.state = torch.zeros(self.B, 4, dtype=torch.int32, device=self.dev)
        self.state[:, 2] = -1

    def _stop_args(self, a):
        P = ops._p
        a.patience, a.tol_rot, a.tol_trans, a.last_step, a.state = self.patience, P(self.tol_rot), P(self.tol_trans), P(self.last_step), P(self.state)

    def run(self, n_epoch, check_every=0):
        """Up to n_epoch epochs.  check_every = k > 0: .done_epoch is read once every k epochs and the loop returns early when
        every pair is done -- the only synchronisation, and only on request."""
        k = int(check_every)
        for i in range(int(n_epoch)):
            self.epoch()
            if k > 0 and (i + 1) % k == 0 and bool((self.done_epoch >= 0).all()):
                break
        return self

    @property
    def done_epoch(self):
        return self.state[:, 2]

    @property
    def failed(self):
        return self.state[:, 3]


class PairRegistration(PoseLoop):
    """B pairs src_tri (B, N, 9) / tar_tri (B, M, 9) (pseudo-triangles whose first points are the clouds' points; N, M are
    capacities when counts1 / counts2 -- lists, CPU or int32 GPU tensors (B,) -- are given), n_lines lines per pair.

    xi0 (B, 6): starting poses (default 0).  lr: the starting rate of .run's schedule, or the rate of .epoch.  rounds: the
    sampler's rejection rounds.  seed: the line sampler's own generator state (None: the process's, ops.sampler_rng).
    lines (B, n_lines, 6): use these lines in every epoch instead of sampling.  monitor: also each pair's Chamfer distance
    (moved first points against the target's) per epoch -- uniform batches only.  deterministic: rrl_opts.deterministic of
    the step (bit-reproducible gradients).  table_rows: epochs the log table holds (later epochs run, unlogged).

    The poses move x -> x R + T (Reconstruction_point's row convention)."""

    _ARGS, _ENTRY = _lib.RegisterEpochArgs, "rrl_register_epoch"  # the epoch's argument struct and its C entry

    def __init__(self, src_tri, tar_tri, n_lines, *, counts1=None, counts2=None, xi0=None, lr=DEMO_LR, rounds=10, seed=None,
                 monitor=False, deterministic=None, table_rows=4096, lines=None):
        self._build(src_tri, tar_tri, n_lines, counts1=counts1, counts2=counts2, rounds=rounds, seed=seed, monitor=monitor,
                    deterministic=deterministic, table_rows=table_rows, lines=lines, pose=dict(xi0=xi0, lr=lr))

    def _build(self, src_tri, tar_tri, n_lines, *, counts1, counts2, rounds, seed, monitor, deterministic, table_rows, lines, pose):
        """What every batched registration loop is made of: the request's refusals, the step, the sampler, the log and the
        monitor; then the pose side (_init_pose_side(**pose): the subclass's), then the epoch's argument struct."""
        ragged = counts1 is not None or counts2 is not None
        if src_tri.dim() != 3 or tar_tri.dim() != 3 or src_tri.shape[0] != tar_tri.shape[0]:
            raise ValueError("src_tri / tar_tri must be (B, n, 9) with the same B")
        check_request(src_tri.shape[1], tar_tri.shape[1], ragged, monitor, ops.sort_capacity())
        if int(rounds) <= 0 or int(table_rows) < 0:
            raise ValueError("rounds must be positive, table_rows non-negative")
        self.step = ops.RegistrationStep(src_tri, tar_tri, n_lines, transpose_r=False, prepared=True, chain=False,
                                         deterministic=deterministic, counts1=counts1, counts2=counts2)
        st = self.step
        if not st.prepared:
            raise ValueError("PairRegistration needs prepared orders (scan mode cull; RRL_PREPARED must not be 0)")
        dev = self.dev = st.dev
        B, N, M, L = st.dims
        self.B, self.rounds, self.monitor = B, int(rounds), bool(monitor)
        f32 = dict(dtype=torch.float32, device=dev)
        # the sampler's geometry, the demo's way and once: box2 and radius = the target's AABB and its diagonal, centers = the
        # mean of the target's points, box1 = the source's AABB as given (every later one comes out of the pose launch)
        src_pts, tar_pts = st.src[:, :, :3].contiguous(), st.tar[:, :, :3].contiguous()
        self.box2 = ops.aabb(tar_pts, st.counts2)
        self.box1 = ops.aabb(src_pts, st.counts1)
        self.radius = (self.box2[:, 3:] - self.box2[:, :3]).norm(p=2, dim=1).contiguous()
        if st.counts2 is None:
            self.centers = tar_pts.mean(1).contiguous()
        else:
            keep = (torch.arange(M, device=dev)[None, :] < st.counts2[:, None]).unsqueeze(-1)
            self.centers = (torch.where(keep, tar_pts, torch.zeros_like(tar_pts)).sum(1)
                            / st.counts2.clamp(min=1)[:, None].to(torch.float32)).contiguous()
        self.sampling = lines is None
        if self.sampling:
            self.lines = torch.zeros(B, L, 6, **f32)
            self.rng = ops.sampler_rng(dev) if seed is None else \
                torch.tensor([int(seed) & 0x7FFFFFFFFFFFFFFF, 0, 0, 0], dtype=torch.int64, device=dev)
        else:
            self.lines = ops._prep(lines, "lines", 6, dev).reshape(B, L, 6).clone()
            self.rng = None
        self.filled = torch.zeros(B, dtype=torch.int32, device=dev)
        self.tiles = torch.empty(B * self.rounds * ((L + 1023) // 1024) * 32, dtype=torch.int32, device=dev)
        self._init_log(table_rows)
        self.value = self.cham = None
        if self.monitor:
            nb = int(_lib.load().rrl_chamfer_workspace_bytes(B, N, M))
            self.cham = (torch.empty(nb, dtype=torch.uint8, device=dev), torch.empty(B, N, dtype=torch.int64, device=dev),
                         torch.empty(B, M, dtype=torch.int64, device=dev), torch.empty(1, **f32))
            self.value = torch.zeros(B, **f32)
        self._init_pose_side(**pose)
        self._target_built = False
        self._opts_first, self._opts_kept = ctypes.addressof(st._opts), ctypes.addressof(st._opts_kept)
        self._bind()

    def _init_pose_side(self, xi0, lr):
        """The first-order state: xi (B, 6) with Adam's moments, step counts and rates, and (R, T) = exp(xi)."""
        B, f32 = self.B, dict(dtype=torch.float32, device=self.dev)
        self.xi = self._start_poses(xi0=xi0).clone()  # (the parameter: never the caller's tensor)
        self.m, self.v = torch.zeros(B, 6, **f32), torch.zeros(B, 6, **f32)
        self.adam_state = torch.zeros(B, **f32)
        self.lr_value = float(lr)
        self.lr = torch.full((B,), self.lr_value, **f32)
        self.gxi = torch.zeros(B, 6, **f32)

    def _make_args(self):
        """The epoch's argument struct: the fields both structs name alike, then the pose side's (_pose_args)."""
        st, P = self.step, ops._p
        a = self._ARGS()
        a.struct_bytes = ctypes.sizeof(a)
        a.B, a.N, a.M, a.L = st.dims
        a.rounds = self.rounds
        a.rng_state, a.radius, a.centers, a.box1, a.box2 = P(self.rng), P(self.radius), P(self.centers), P(self.box1), P(self.box2)
        a.lines, a.filled, a.tile_counts = P(self.lines), P(self.filled), P(self.tiles)
        a.src_tri, a.tar_tri, a.R, a.T = P(st.src), P(st.tar), P(self.R), P(self.T)
        a.ws, a.ws_bytes, a.loss = P(st.st.ws), st.st.nbytes, P(st.st.loss)
        if self.monitor:
            ws, bx, by, mean = self.cham
            a.cham_ws, a.cham_ws_bytes, a.best_x, a.best_y, a.cham_mean, a.value = P(ws), ws.numel(), P(bx), P(by), P(mean), P(self.value)
        self._log_args(a)
        self._pose_args(a)
        return a

    def _pose_args(self, a):
        st, P = self.step, ops._p
        a.transpose_r, a.grad_loss, a.gR, a.gt = st.tr, P(st.ones), P(st.gR), P(st.gt)
        a.xi, a.m, a.v, a.adam_state, a.lr = P(self.xi), P(self.m), P(self.v), P(self.adam_state), P(self.lr)
        a.b1, a.b2, a.eps = 0.9, 0.999, 1e-8
        a.gxi = P(self.gxi)

    def invalidate_target(self):
        """The next epoch rebuilds the targets' records (after a write into tar_tri or counts2)."""
        self._target_built = False

    def set_lr(self, lr):
        """Write a new rate into lr [B] (only when it differs from the current one)."""
        lr = float(lr)
        if lr != self.lr_value:
            self.lr.fill_(lr)
            self.lr_value = lr

    def epoch(self, lr=None):
        """One epoch of all B pairs: ONE C call (rrl_register_epoch), nothing read back."""
        if lr is not None:
            self.set_lr(lr)
        self._args.opts = self._opts_kept if self._target_built else self._opts_first
        super().epoch()
        self._target_built = True
        self.step.st.ragged = self.step.ragged

    def run(self, n_epoch):
        """n_epoch epochs under the demo's schedule (adjust_learning_rate: the rate is halved when epoch % 1000 == 0, epoch
        0 included), continuing where the previous .run / .epoch calls stopped; lr [B] is written only when it changes."""
        for _ in range(int(n_epoch)):
            self.epoch(scheduled_lr(self.epochs, self.lr_value))
        return self

    def moved_points(self):
        """(B, N, 3): the sources' first points as the latest epoch's step moved them (a view of the step's workspace; rows
        beyond a count are not meaningful).  Before the first epoch: the points as given."""
        if not self.epochs:
            return self.step.src[:, :, :3]
        return self.step.st.tri1t[:, :, :3]

    @property
    def loss(self):
        """(B,) the latest epoch's losses (a view of the step's buffer)."""
        return self.step.st.loss.view(-1)


def register_pairs(src_tri, tar_tri, n_lines, n_epoch=1000, **kw):
    """PairRegistration(...).run(n_epoch) -> (R (B, 3, 3), T (B, 3), history)."""
    reg = PairRegistration(src_tri, tar_tri, n_lines, **kw)
    reg.run(n_epoch)
    return reg.R, reg.T, reg.history()
