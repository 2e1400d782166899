"""The loss fragments of the reference's three trainers, each as one call.

Every trainer wraps the loss in the same Python pattern: transform the source cloud and its
pseudo-triangles with the predicted (R, t), draw lines once from the target's bounding sphere,
then `for j in range(B): acc += cal_loss_...(…[j:j+1]…)` with a trainer-specific scaling:

  RPM  rpm/Train_RPM.py:204-259   radius = |box diagonal|,     10000 lines, per iteration
                                  sum_j / num_iter, discount 0.5**(num_iter-ni-1)
  DCP  dcp/Train_DCP.py:233-270   radius = |box diagonal| / 2, 15000 lines, sum_j (loss/5) / B
  FMR  fmr/model.py:266-310       radius = |box diagonal| / 2, 15000 lines from the LAST
                                  estimate, last three estimates, sum_j (loss/5) * discount / B

Here the B per-sample calls and the transforms are ONE fused launch set per predicted
transform (ops.registration_loss: rigid apply + loss, backward straight to dR / dt), with no
host synchronisation; a sample whose line set populates no (k, j) bucket contributes 0 (the
reference would fail on `tensor += (None, None)`).  All functions take and return GPU tensors.
"""
import os

import torch

from . import ops as _ops

RNG = (1, 1, 5, 5)  # every reference call site


def _mode(mode):
    import loss as _loss  # the drop-in module next to this package
    return _loss._scan_mode(mode)


def bounding_radius(tar_box, scale=1.0):
    """|corner 0 - corner 7| * scale of (B, 8, 3) boxes -> (B, 1) (Train_RPM.py:201-203)."""
    return (torch.norm(tar_box[:, 0, :] - tar_box[:, -1, :], dim=-1, p=2) * scale).reshape(-1, 1)


DEVICE_RNG = False  # True: draw the candidate lines' uniforms on the GPU (opt-in, see draw_lines)
CHAMFER_FROM_LOSS = "auto"  # the Chamfer monitor walks the clouds the loss evaluation just sorted (ops.chamfer_from_state:
#   no second sort, ~1/3 less device time).  That is the distance between the FIRST POINTS of the pseudo-triangles:
#   identical to chamfer_dist(points_src_sample moved, points_tar_sample) when those samples are exactly the rows
#   0, 3, 6, ... of points_based_neighs_* (what Sample_neighs emits, code/loss.py:473-485).  "auto" (round 3): used when
#   that contract holds for the batch -- taken from the dataset's per-item flag `p0_rows` (pre_dataloader sets it when it
#   builds an item: checked once per dataset item on the host), else checked once per data dict on the device and
#   remembered in it.  True: always (the caller vouches), False: never.


def _first_points_contract(data, channel_first=False):
    """Do the point samples of this batch equal the first points of its pseudo-triangles?  One answer per data dict
    AND per state of the four tensors it was decided on (stored under '_rrl_p0' together with their data pointers and
    version counters -- round 4, ADVICE r3: a trainer that jitters or resamples `points_*_sample` in the same dict gets
    a fresh check instead of a stale True).  The value ops.chamfer_from_state returns carries no grad_fn: the
    reference's callers only log the monitor (FMR multiplies it by 0.0)."""
    keys = ('points_src_sample', 'points_based_neighs_src', 'points_tar_sample', 'points_based_neighs_tar')
    stamp = tuple(_ops._write_key(data[k]) for k in keys if isinstance(data.get(k), torch.Tensor))
    cached = data.get('_rrl_p0_key')
    ok = data.get('_rrl_p0') if cached == stamp else None
    if ok is None:
        flag = data.get('p0_rows')
        if flag is not None and cached is None:  # the dataset's per-item mark (pre_dataloader): valid for the tensors it built
            ok = bool(torch.as_tensor(flag).all())
        else:
            ok = True
            for pts, nb in (('points_src_sample', 'points_based_neighs_src'), ('points_tar_sample', 'points_based_neighs_tar')):
                p, q = data[pts], data[nb]
                if channel_first:
                    p, q = p.transpose(2, 1), q.transpose(2, 1)
                B = p.shape[0]
                ok = ok and q.shape[1] == 3 * p.shape[1] and bool(torch.equal(p[..., :3], q.reshape(B, -1, 9)[..., :3]))
        try:
            data['_rrl_p0'] = ok
            data['_rrl_p0_key'] = stamp
        except TypeError:  # an immutable mapping: decide again next time
            pass
    return ok


def _ride_monitor(data, channel_first=False):
    """Will _monitor take the value from the loss evaluation's own clouds?  Then that evaluation carries the walk inside
    its scan launch (ops.ChamferRide: round 4b) and the monitor costs no launch of its own.  Decided WITHOUT touching the
    device (a comparison here would drain the stream before the loss is even issued: +0.1 ms per DCP fragment, measured):
    the caller's switch, the verdict already stored in the dict, the dataset's host-side per-item mark -- and when none of
    these says anything yet, ride speculatively: _monitor decides after the evaluation as before, a walk that is not used
    costs ~10 us of device time once per data dict."""
    if not CHAMFER_FROM_LOSS:
        return False
    if CHAMFER_FROM_LOSS is True:
        return True
    if data is None:
        return False
    keys = ('points_src_sample', 'points_based_neighs_src', 'points_tar_sample', 'points_based_neighs_tar')
    stamp = tuple(_ops._write_key(data[k]) for k in keys if isinstance(data.get(k), torch.Tensor))
    if data.get('_rrl_p0_key') == stamp and data.get('_rrl_p0') is not None:
        return bool(data['_rrl_p0'])
    flag = data.get('p0_rows')
    if flag is not None and data.get('_rrl_p0_key') is None and not (isinstance(flag, torch.Tensor) and flag.is_cuda):
        return bool(torch.as_tensor(flag).all())
    return True


def _monitor(moved, tar, data=None, channel_first=False):
    """The trainers' Chamfer monitor next to a loss evaluation: from the evaluation's own sorted clouds when that is
    the same quantity (CHAMFER_FROM_LOSS), else the standalone kernel on (moved, tar)."""
    st = _ops.last_state()
    if CHAMFER_FROM_LOSS and st is not None and max(st.dims[1], st.dims[2]) <= _ops.sort_capacity() and \
            st.dims[1] == moved.shape[1] and st.dims[2] == tar.shape[1]:
        if CHAMFER_FROM_LOSS is True or (data is not None and _first_points_contract(data, channel_first)):
            return _ops.chamfer_from_state(st)
    return _ops.chamfer(tar, moved)


def draw_lines(radius, centers, n_lines, moved_src, tar, device=None, device_rng=None):
    """The trainers' sampler call: (B, n_lines, 6) lines crossing both clouds' boxes.
    The reference draws 4 * 10 * B * n_lines uniforms from torch's CPU generator per call (3.2 M
    floats at B = 8, n = 10000: milliseconds of host time and a 13 MB upload, against 0.12 ms for
    the loss).  DEFAULT = the reference's behaviour: the CPU stream, reproducible under
    torch.manual_seed exactly like the reference's trainers.  device_rng=True (or
    callsites.DEVICE_RNG = True) draws them from the GPU generator instead (same distribution,
    seeded by torch.cuda.manual_seed) -- the fast path for training loops."""
    import loss as _loss
    device = device or moved_src.device
    if device_rng is None:
        device_rng = DEVICE_RNG
    return _loss.Random_uniform_distribution_lines_batch_efficient_resample(
        radius, centers, n_lines, moved_src, tar, device, device_rng=device_rng)


USE_ORDERS = True  # hand the dataset's 'order_src' / 'order_tar' (pre_dataloader.kd_order, or ops.cloud_order) to the fused
#   op: the prepared build -- no cell sort in any pose's step; same loss bits.  False: ignore them.


def _orders(data, n_src, n_tar, B=None, dev=None):
    """(order1, order2) from the trainer's dict when it carries usable ones -- contiguous int32 (B, 64 ceil(n / 64))
    tensors on the op's GPU, as the DataLoader collates pre_dataloader's per-item arrays -- else (None, None): the fused
    op then sorts.  (Batch dimension and device are part of "usable": the kernels read the tensor as [B][npad] on the
    GPU that owns the clouds.)"""
    if not USE_ORDERS or data is None:
        return None, None
    o1, o2 = data.get('order_src'), data.get('order_tar')
    ok = all(isinstance(o, torch.Tensor) and o.is_cuda and o.dtype == torch.int32 and o.dim() == 2 and o.is_contiguous()
             and o.shape[1] == (n + 63) // 64 * 64 and (B is None or o.shape[0] == B) and (dev is None or o.device == dev)
             for o, n in ((o1, n_src), (o2, n_tar)))
    return (o1, o2) if ok else (None, None)


def per_sample_loss(src_nb, R, t, tar_tri, lines, mode=None, target_from=None, data=None, chamfer=False):
    """loss[b] of the pseudo-triangles `src_nb` (B, 3N, 3) or (B, N, 9) moved by x -> R x + t,
    against tar_tri (B, M, 9) along lines (B, L, 6).  (loss (B,), valid (B,) bool).
    target_from: ops.last_state() of an earlier call with the same tar_tri and lines, whose
    target scan is reused (the iterative trainers keep target and lines fixed across poses).
    data: the trainer's dict; when it carries the clouds' spatial orders ('order_src', 'order_tar') the prepared build
    is used (the source's order holds for every pose: a rigid motion preserves it).
    chamfer: the caller will monitor the Chamfer distance of this evaluation's clouds (_monitor): its walk then rides in
    the evaluation's scan launch (with a carried-over target too: the walk then reads the target in the state that holds it)."""
    B = src_nb.shape[0]
    src_tri, tar_tri = src_nb.reshape(B, -1, 9), tar_tri.reshape(B, -1, 9)
    o1, o2 = _orders(data, src_tri.shape[1], tar_tri.shape[1], B, src_tri.device if src_tri.is_cuda else None)
    ride = bool(chamfer) and max(src_tri.shape[1], tar_tri.shape[1]) <= _ops.sort_capacity()
    loss, info, _ = _ops.registration_loss(src_tri, R, t, tar_tri, lines, RNG, transpose_r=True, mode=_mode(mode),
                                           target_from=target_from, order1=o1, order2=o2, chamfer=ride)
    return loss, info[:, 0] > 0


MULTI_POSE = os.environ.get("RRL_MULTI_POSE", "1") != "0"  # the iterative trainers' poses in ONE evaluation (round 5)


class _PackedPoses(torch.autograd.Function):
    """k x B poses given as ONE (k, B, 3, 4) tensor [R | t] -> loss (k * B,), info (k * B, 4): the (multi-pose) evaluation
    behind a node that takes and returns the PACKED transforms -- the fragment's own torch ops shrink to a stack in front
    and one product + sum behind (the fragments' device time was half tiny torch kernels: 40 launches of ~2 us around 6
    of ours; eager, their host time dominates).  Forward AND backward of the evaluation are ONE C call in the forward
    (ops.registration_step_raw: the gradients for dL/dloss = 1; the backward rides in the reduce's launch where the tail
    kernel serves the shape): the loss is linear in the upstream gradient, so this node's backward only scales them."""

    @staticmethod
    def forward(ctx, P, src_tri, tar_tri, lines, o1, o2, ride):
        k, B = P.shape[:2]
        Pd = P.detach().reshape(k * B, 3, 4)
        dev = _ops._home(src_tri, tar_tri, lines, Pd)
        R = _ops._prep(Pd[:, :, :3], "R", None, dev)
        t = _ops._prep(Pd[:, :, 3], "t", None, dev)
        loss, gR, gt, info, st = _ops.registration_step_raw(
            _ops._prep(src_tri, "src_tri", 9, dev), R, t, _ops._prep(tar_tri, "tar_tri", 9, dev), _ops._prep(lines, "line", 6, dev),
            RNG, True, o1, o2, ride)
        ctx.grads, ctx.shape, ctx.st = (gR, gt), P.shape, st  # (views of the state's workspace: the state stays alive with the node)
        ctx.mark_non_differentiable(info)
        ctx.set_materialize_grads(False)
        return loss.clone(), info  # (a fresh tensor: the state's loss buffer must not become an autograd output)

    @staticmethod
    def backward(ctx, g, _gi):
        if g is None:
            return (None,) * 7
        gR, gt = ctx.grads
        g = g.reshape(-1, 1, 1)
        return torch.cat([gR * g, (gt * g.reshape(-1, 1)).unsqueeze(-1)], -1).reshape(ctx.shape), None, None, None, None, None, None


_weights = {}  # (values, B, device) -> (k * B,) per-instance weights of a fragment's discounted sum


def _instance_weights(per_pose, B, dev):
    key = (tuple(per_pose), B, str(dev))
    w = _weights.get(key)
    if w is None:
        if len(_weights) > 64:
            _weights.clear()
        w = _weights[key] = torch.tensor(per_pose, dtype=torch.float32).repeat_interleave(B).to(dev)
    return w


def multi_pose_loss(src_nb, transforms, tar_tri, lines, mode=None, data=None, chamfer=False):
    """The iterative trainers' loop over poses as ONE evaluation (include/rrl.h rrl_opts.problems): `transforms` are the k
    per-iteration (B, 3, 4) / (B, 4, 4) estimates [R | t] -- all known before the first loss call (rpm/Train_RPM.py:207-231,
    fmr/model.py:292-308) --, target and lines are shared.  Returns (loss (k * B,) -- instance i * B + b = pose i of sample
    b, differentiable back into every transform --, valid (k, B) bool), bit-identical per instance to per_sample_loss pose
    after pose (target scanned once, the k source scans side by side, one per-line stage, one reduce + backward); or None
    where the multi-pose path does not serve the call (clouds beyond the sort capacity, a scan mode other than cull,
    RRL_MULTI_POSE=0): the caller then loops.
    chamfer: the walk of the evaluation's monitor rides in its scan launch over all k * B instances (ops.chamfer_group_means)."""
    k = len(transforms)
    B = src_nb.shape[0]
    src_tri, tar_tri = src_nb.reshape(B, -1, 9), tar_tri.reshape(B, -1, 9)
    if not MULTI_POSE or k < 1 or _mode(mode) != "cull" or max(src_tri.shape[1], tar_tri.shape[1]) > _ops.sort_capacity():
        return None
    #  the packed node differentiates with respect to the TRANSFORMS only: a source (or target) that requires grad
    # takes the per-pose loop, whose registration_loss produces dL/dsrc (or raises for the target) -- never a silent None
    if torch.is_grad_enabled() and (src_nb.requires_grad or tar_tri.requires_grad):
        return None
    o1, o2 = _orders(data, src_tri.shape[1], tar_tri.shape[1], B, src_tri.device if src_tri.is_cuda else None)
    P = torch.stack([x[..., :3, :] for x in transforms])  # (k, B, 3, 4)
    loss, info = _PackedPoses.apply(P, src_tri, tar_tri, lines, o1, o2, bool(chamfer))
    return loss, (info[:, 0] > 0).view(k, B)


def _split(transform):
    """(B, 3, 4) [R | t] (RPM's se3 matrices) -> R (B, 3, 3), t (B, 3)."""
    return transform[..., :3, :3], transform[..., :3, 3]


def rpm_intersection_loss(pred_transforms, data, n_lines=10000, lines=None, mode=None):
    """rpm/Train_RPM.py:188-259.  pred_transforms: list of (B, 3, 4); data: the trainer's dict
    with 'points_src_sample' (B, N, >=3), 'points_based_neighs_src' (B, 3N, 3),
    'points_tar_sample' (B, M, 3), 'points_based_neighs_tar' (B, 3M, 3), 'tar_box' (B, 8, 3),
    'centers' (B, 3).  Returns a dict: 'loss_intersection' (1,), 'loss_chamfer' (scalar,
    detached), 'per_iter' (list of (1,) tensors, already / num_iter), 'lines', 'valid'."""
    num_iter = len(pred_transforms)
    tar = data['points_tar_sample'].contiguous()
    B = tar.shape[0]
    tar_tri = data['points_based_neighs_tar'].reshape(B, -1, 9)
    src = data['points_src_sample'][..., :3]
    per_iter, chamfers, valid = [], [], []
    first = None  # LossState of iteration 0: target + lines are the same in every iteration
    if num_iter >= 1:  # all poses are known up front: ONE evaluation of num_iter * B instances (round 5, multi_pose_loss)
        moved0 = None
        if lines is None:
            moved0 = _ops.rigid_apply(src, *_split(pred_transforms[0]), transpose_r=True)
            lines = draw_lines(bounding_radius(data['tar_box']), data['centers'], n_lines, moved0.detach(), tar)
        got = multi_pose_loss(data['points_based_neighs_src'], pred_transforms, tar_tri, lines, mode, data=data,
                              chamfer=_ride_monitor(data))
        if got is not None:
            loss, ok = got
            st = _ops.last_state()
            disc = [0.5 ** (num_iter - ni - 1) for ni in range(num_iter)]
            own = CHAMFER_FROM_LOSS and max(st.dims[1], st.dims[2]) <= _ops.sort_capacity() and st.dims[1] == src.shape[1] and \
                st.dims[2] == tar.shape[1] and (CHAMFER_FROM_LOSS is True or _first_points_contract(data))
            if own:  # the monitor of every iteration from the evaluation's own clouds (the walk rode in its scan launch)
                cham = (_ops.chamfer_group_means(st, num_iter) * _instance_weights(disc, 1, loss.device)).sum()
            else:
                cham = sum(_ops.chamfer(tar, (moved0 if (ni == 0 and moved0 is not None) else
                                              _ops.rigid_apply(src, *_split(pred_transforms[ni]), transpose_r=True))).detach() * disc[ni]
                           for ni in range(num_iter))
            # sum_i disc_i (sum_b loss[i, b]) / num_iter as ONE weighted sum; the per-iteration values (reporting) detached
            total = (loss * _instance_weights([d / num_iter for d in disc], B, loss.device)).sum().reshape(1)
            per = loss.detach().view(num_iter, B).sum(1) / num_iter
            return {'loss_intersection': total, 'loss_chamfer': cham,
                    'per_iter': [per[ni:ni + 1] for ni in range(num_iter)], 'lines': lines, 'valid': ok}
    for ni in range(num_iter):
        R, t = _split(pred_transforms[ni])
        moved = _ops.rigid_apply(src, R, t, transpose_r=True)
        if lines is None:
            lines = draw_lines(bounding_radius(data['tar_box']), data['centers'], n_lines,
                               moved.detach(), tar)
        loss, ok = per_sample_loss(data['points_based_neighs_src'], R, t, tar_tri, lines, mode, first, data=data,
                                   chamfer=_ride_monitor(data))
        first = first or _ops.last_state()
        per_iter.append(loss.sum().reshape(1) / num_iter)
        chamfers.append(_monitor(moved, tar, data).detach())
        valid.append(ok)
    disc = [0.5 ** (num_iter - ni - 1) for ni in range(num_iter)]
    return {'loss_intersection': sum(l * d for l, d in zip(per_iter, disc)),
            'loss_chamfer': sum(c * d for c, d in zip(chamfers, disc)),
            'per_iter': per_iter, 'lines': lines, 'valid': torch.stack(valid)}


def dcp_intersection_loss(data, rotation_ab_pred, translation_ab_pred, n_lines=15000, lines=None,
                          mode=None):
    """dcp/Train_DCP.py:233-270.  The DCP dict holds channel-first clouds: 'points_src_sample'
    (B, 3, N), 'points_based_neighs_src' (B, 3, 3N), 'points_tar_sample' (B, 3, M),
    'points_based_neighs_tar' (B, 3, 3M).  Returns (loss_intersection / batch_size (1,),
    loss_chamfer, lines, valid)."""
    tar = data['points_tar_sample'].transpose(2, 1).contiguous()
    B = tar.shape[0]
    tar_tri = data['points_based_neighs_tar'].transpose(2, 1).reshape(B, -1, 9)
    moved = _ops.rigid_apply(data['points_src_sample'], rotation_ab_pred, translation_ab_pred,
                             transpose_r=True, channel_first=True).transpose(2, 1).contiguous()
    if lines is None:
        lines = draw_lines(bounding_radius(data['tar_box'], 0.5), data['centers'], n_lines,
                           moved.detach(), tar)
    src_nb = data['points_based_neighs_src'].transpose(2, 1).contiguous()
    ride = _ride_monitor(data, channel_first=True)
    got = multi_pose_loss(src_nb, [torch.cat([rotation_ab_pred.reshape(B, 3, 3), translation_ab_pred.reshape(B, 3, 1)], -1)],
                          tar_tri, lines, mode, data=data, chamfer=ride)  # (one pose: the packed node, forward + backward in one C call)
    if got is not None:
        loss, ok = got
        chamfer = _monitor(moved, tar, data, channel_first=True)
        return (loss * _instance_weights([1.0 / 5.0 / B], B, loss.device)).sum().reshape(1), chamfer, lines, ok[0]
    loss, ok = per_sample_loss(src_nb, rotation_ab_pred, translation_ab_pred, tar_tri, lines, mode, data=data, chamfer=ride)
    chamfer = _monitor(moved, tar, data, channel_first=True)  # the reference evaluates it before the loss; it depends on neither
    return (loss / 5.0).sum().reshape(1) / B, chamfer, lines, ok


def fmr_intersection_loss(g_series, data, n_lines=15000, lines=None, last=3, mode=None):
    """fmr/model.py:266-310.  g_series: sequence of (B, 4, 4) estimates (self.g_series_gpu), of
    which the final `last` enter the loss; channel-last clouds as in RPM.  Returns
    (loss_intersection / batch_size (1,), loss_chamfer of the last estimate, lines, valid)."""
    maxiter = len(g_series)
    tar = data['points_tar_sample'].contiguous()
    B = tar.shape[0]
    tar_tri = data['points_based_neighs_tar'].reshape(B, -1, 9)
    src = data['points_src_sample'][..., :3].contiguous()
    R, t = _split(g_series[maxiter - 1])
    moved = _ops.rigid_apply(src, R, t, transpose_r=True)
    if lines is None:
        lines = draw_lines(bounding_radius(data['tar_box'], 0.5), data['centers'], n_lines,
                           moved.detach(), tar)
    total, valid, first = 0.0, [], None
    idx = list(range(max(maxiter - last, 0), maxiter))
    if len(idx) >= 1:  # the last estimates as ONE evaluation (round 5, multi_pose_loss)
        got = multi_pose_loss(data['points_based_neighs_src'], [g_series[i] for i in idx], tar_tri, lines, mode, data=data,
                              chamfer=_ride_monitor(data))
        if got is not None:
            loss, ok = got
            st = _ops.last_state()
            w = _instance_weights([0.5 ** (maxiter - i - 1) / 5.0 / B for i in idx], B, loss.device)
            own = CHAMFER_FROM_LOSS and max(st.dims[1], st.dims[2]) <= _ops.sort_capacity() and st.dims[1] == moved.shape[1] and \
                st.dims[2] == tar.shape[1] and (CHAMFER_FROM_LOSS is True or _first_points_contract(data))
            cham = _ops.chamfer_group_means(st, len(idx))[-1] if own else _ops.chamfer(tar, moved)  # the LAST estimate's monitor
            return (loss * w).sum().reshape(1), cham, lines, ok
    for i in range(maxiter - last, maxiter):
        R, t = _split(g_series[i])
        loss, ok = per_sample_loss(data['points_based_neighs_src'], R, t, tar_tri, lines, mode, first, data=data,
                                   chamfer=i == maxiter - 1 and _ride_monitor(data))  # (the last estimate's monitor)
        first = first or _ops.last_state()
        total = total + (loss / 5.0).sum().reshape(1) * 0.5 ** (maxiter - i - 1)
        valid.append(ok)
    return total / B, _monitor(moved, tar, data), lines, torch.stack(valid)  # the last estimate's evaluation is the latest


# ---- the trainers' pose heads: the weighted Kabsch solve the loss fragments above take their (R, t) from ---------------
def rpm_compute_rigid_transform(a, b, weights):
    """rpm/models/rpmnet.py:121-157 compute_rigid_transform as ONE node (rrl_hip.kabsch): a (B, n, 3), b (B, n, 3), weights
    (B, n) -> (B, 3, 4) = [rot_mat | translation] with rot_mat moving column vectors, differentiable in all three; the
    reference's 1e-5 in the weight normalisation included.  Where the reference's assert on det(rot_mat) would pass and
    torch.svd's backward is finite this is the same function; on collinear correspondences it returns a rotation with zero
    gradient instead of NaN."""
    from .kabsch import kabsch
    R, T = kabsch(a, b, weights, eps=1e-5, transpose_r=True)
    return torch.cat([R, T.unsqueeze(-1)], dim=2)


def dcp_svd_head_pose(src, src_corr):
    """dcp/model.py:405-455 SVDHead's pose from its correspondences, channel-first as DCP holds its clouds: src, src_corr
    (B, 3, n) -> (R (B, 3, 3), t (B, 3)) with R moving column vectors -- the head's per-sample torch.svd loop as one call."""
    from .kabsch import kabsch
    return kabsch(src.transpose(2, 1).contiguous(), src_corr.transpose(2, 1).contiguous(), None, eps=0.0, transpose_r=True)


def dcp_soft_pointer(src_embedding, tgt_embedding, tgt):
    """dcp/model.py:419-425, SVDHead's correspondences as ONE node (rrl_hip.pointer): src_embedding (B, C, N), tgt_embedding
    (B, C, M), tgt (B, 3, M) -> src_corr (B, 3, N) = tgt softmax(src_embedding^T tgt_embedding / sqrt(C), dim=2)^T,
    differentiable in all three; the (B, N, M) score matrix is never stored."""
    from .pointer import soft_pointer
    return soft_pointer(src_embedding, tgt_embedding, tgt)


def dcp_svd_head(src_embedding, tgt_embedding, src, tgt):
    """SVDHead.forward (dcp/model.py:414-455) as TWO nodes: dcp_soft_pointer, then dcp_svd_head_pose(src, src_corr).
    src (B, 3, N), tgt (B, 3, M) -> (R (B, 3, 3), t (B, 3))."""
    return dcp_svd_head_pose(src, dcp_soft_pointer(src_embedding, tgt_embedding, tgt))


def dcp_attention(query, key, value, n_heads):
    """dcp/model.py:232-245, the attention step of MultiHeadedAttention.forward as ONE node (rrl_hip.attention): the projected
    query (B, N, D), key and value (B, M, D) as the nn.Linear layers leave them -> x (B, N, D), what the reference holds after
    its `x.transpose(1, 2).contiguous().view(nbatches, -1, h * d_k)`; differentiable in all three; neither the (B, h, N, M)
    matrix nor a head-major copy exists."""
    from .attention import attend
    return attend(query, key, value, n_heads)


def dcp_transformer(module, src_embedding, tgt_embedding):
    """Transformer.forward (dcp/model.py:392-401) on an rrl_hip.attention.Transformer (its state_dict is the reference's:
    module.load_state_dict(dcp_net.pointer.state_dict(), strict=True)): src_embedding (B, C, N), tgt_embedding (B, C, M),
    channel-first as DCP holds them -> (src_embedding_p, tgt_embedding_p) of the same shapes, six attention nodes."""
    return module(src_embedding, tgt_embedding)


# ---- RPM's match head: Sinkhorn soft assignment in front of the solve above ----------------------------------------------
def rpm_soft_correspondences(affinity, xyz_ref, n_iters=5, slack=True):
    """rpm/models/rpmnet.py:211-222 up to the solve, as ONE node (rrl_hip.sinkhorn): affinity (B, J, K), xyz_ref (B, K, 3) ->
    (weighted_ref (B, J, 3), src_weights (B, J), ref_weights (B, K)) with perm = exp(sinkhorn(affinity, n_iters, slack)),
    weighted_ref = perm @ xyz_ref / (perm.sum(2, keepdim=True) + 1e-5), src_weights = perm.sum(2) -- the weights of the
    solve -- and ref_weights = perm.sum(1); the two sums are what the trainer's outlier regulariser takes
    (rpm/Train_RPM.py:237-240).  Differentiable in affinity and xyz_ref; perm itself is never stored."""
    from .sinkhorn import soft_assign
    return soft_assign(affinity, xyz_ref, n_iters=n_iters, slack=slack, eps=1e-5)


def rpm_match_head(affinity, xyz_src, xyz_ref, n_iters=5, slack=True):
    """The loop body of RPMNet.forward behind compute_affinity (rpmnet.py:211-222) as TWO nodes: rpm_soft_correspondences,
    then rpm_compute_rigid_transform(xyz_src, weighted_ref, src_weights).  Returns (transform (B, 3, 4), weighted_ref,
    src_weights, ref_weights)."""
    weighted_ref, src_weights, ref_weights = rpm_soft_correspondences(affinity, xyz_ref, n_iters, slack)
    return rpm_compute_rigid_transform(xyz_src, weighted_ref, src_weights), weighted_ref, src_weights, ref_weights


# ---- RPM's feature extractor: ball-query grouping and the raw xyz / dxyz / ppf features in front of its prepool layers -------
def rpm_sample_and_group_multi(xyz, normals, radius=0.3, nsample=64, npoint=-1, returnfps=False):
    """rpm/models/pointnet_util.py:197-244 sample_and_group_multi(npoint, radius, nsample, xyz, normals, returnfps) as ONE
    launch (neighbors.ball_group): xyz, normals (B, N, 3) -> {'xyz': (B, S, 3), 'dxyz': (B, S, nsample, 3), 'ppf': (B, S,
    nsample, 4)}, S = N unless npoint > 0 (then the farthest-point sampler first, neighbors.fps, with the reference's CPU
    draw of its first index).  returnfps: also (grouped_xyz (B, S, nsample, 3), fps_idx (B, S) int64).  Forward only: the
    reference calls it on detached clouds (rpm/models/rpmnet.py:204-205)."""
    from . import neighbors
    B, N = xyz.shape[0], xyz.shape[1]
    fps_idx = neighbors.fps(xyz, npoint) if npoint > 0 else None
    feat, idx, _ = neighbors.ball_group(xyz, normals, radius, nsample, features=("dxyz", "ppf"), query_idx=fps_idx)
    pts = _ops._prep(xyz, "xyz", 3, feat.device)
    new_xyz = pts if fps_idx is None else torch.gather(pts, 1, fps_idx.long().unsqueeze(-1).expand(-1, -1, 3))
    out = {'xyz': new_xyz, 'dxyz': feat[..., :3], 'ppf': feat[..., 3:]}
    if not returnfps:
        return out
    if fps_idx is None:
        fps_idx = torch.arange(N, device=feat.device)[None].repeat(B, 1)
    grouped = torch.gather(pts, 1, idx.long().reshape(B, -1, 1).expand(-1, -1, 3)).reshape(*idx.shape, 3)
    return out, grouped, fps_idx.long()


def rpm_raw_features(xyz, normals, features, radius=0.3, nsample=64):
    """The tensor FeatExtractionEarlyFusion.forward concatenates before its permute (rpm/models/feature_nets.py:184-193):
    (B, N, nsample, C) with the chosen channels sorted xyz, dxyz, ppf as the reference sorts them, written by the kernel
    directly -- no expand, no cat."""
    from . import neighbors
    return neighbors.ball_group(xyz, normals, radius, nsample, features=features)[0]


def rpm_feat_prepool_pool(net, raw):
    """rpm/models/feature_nets.py:196-199 -- the permute to (B, C, nsample, N), self.prepool and torch.max(new_feat, 2)[0] -- as
    ONE node (pointnet.encode_grouped): raw (B, N, nsample, C) from rpm_raw_features, net a
    pointnet.GroupedEncoder (GroupedEncoder.rpm_feat_prepool loads the reference's prepool weights with strict=True) -> the pooled
    features (B, 2 feature_dim, N).  No (B, C, nsample, N) activation is written; where slots tie (ball-query pads short groups
    with repeated slots) the gradient goes to the lowest slot, where torch picks its own."""
    return net(raw)


def rpm_feat_extractor(net, postpool, xyz, normals, features, radius=0.3, nsample=64):
    """rpm/models/feature_nets.py:173-205 FeatExtractionEarlyFusion.forward: xyz, normals (B, N, 3) -> cluster features (B, N, C).
    Lines 184-193 are one launch (rpm_raw_features), lines 196-199 one node (rpm_feat_prepool_pool); `postpool` is the reference's
    torch module of line 201 (get_postpool, :134-152), which works on N positions only and stays in torch; then the permute and
    the division by the norm of lines 202-203."""
    raw = rpm_raw_features(xyz, normals, features, radius, nsample)
    post = postpool(rpm_feat_prepool_pool(net, raw)).permute(0, 2, 1)
    return post / torch.norm(post, dim=-1, keepdim=True)


# ---- DCP's feature extractor: the k-NN graph and its edge features in front of DGCNN's convolutions ------------------------
def _dcp_cloud(x, k):
    if not isinstance(x, torch.Tensor) or x.dim() != 3 or x.shape[1] != 3:
        raise ValueError("x must be a (B, 3, N) tensor, channel-first as DCP holds its clouds")
    if isinstance(k, bool) or int(k) != k or k < 1:
        raise ValueError(f"k must be a positive integer, got {k!r}")
    if k > x.shape[2]:  # (the reference's topk raises here)
        raise ValueError(f"k = {k} neighbours out of {x.shape[2]} points: selected index k out of range")
    return x.detach().transpose(2, 1).contiguous()


def dcp_knn(x, k):
    """dcp/model.py:46-52 knn(x, k) as one call (neighbors.knn): x (B, 3, N) -> (B, N, k) int64, every point's k nearest
    points, itself first -- by exact float64 distances with ties to the lower index, where the reference ranks the float32
    matmul expansion -xx - inner - xx^T with topk (rows with two candidates within a few float32 roundings of each other can
    differ).  No (B, N, N) matrix.  ValueError for k > N.  Forward only."""
    from . import neighbors
    return neighbors.knn(_dcp_cloud(x, k), k)[0].long()


def dcp_graph_feature(x, k=20):
    """dcp/model.py:55-78 get_graph_feature(x, k) as one call (neighbors.knn_group): x (B, 3, N) -> (B, 6, N, k) float32, the
    neighbours' coordinates on channels 0-2 and the centre's own on 3-5, channel-first as the reference's permute leaves it --
    written by the kernel directly: no distance matrix, no topk, no index-offset tensor, no repeat, no cat.  ValueError for
    k > N.  Forward only: the reference feeds the input clouds, which carry no gradient."""
    from . import neighbors
    return neighbors.knn_group(_dcp_cloud(x, k), k, features=("nbr", "ctr"), channel_first=True)[0]


# ---- FMR's pose head: the inverse-compositional solver around its encoder ------------------------------
def fmr_approx_jac(encoder, p0, f0, dt, features_only=False):
    """fmr/model.py:408-433 approx_Jac(p0, f0, dt): the finite-difference Jacobian of the encoder's features in the six twist
    coordinates, J (B, K, 6) = (f0 - f(exp(-dt_i e_i) p0)) / dt_i, from p0 (B, N, 3), f0 (B, K) and dt (B, 6).  The six perturbed
    clouds are ONE launch (fmr.ic_perturb: no Python loop over the batch, no diag / exp / matmul per sample) and one encoder call
    on (6 B, N, 3), as in the reference.  features_only=True returns the perturbed features fp (B, 6, K) instead -- what
    fmr.ic_pinv takes: it forms J itself, in double."""
    from . import fmr
    B, N = p0.shape[0], p0.shape[1]
    fp = encoder(fmr.ic_perturb(p0, dt).reshape(6 * B, N, 3)).reshape(B, 6, -1)
    if features_only:
        return fp
    return (f0.unsqueeze(-1) - fp.transpose(1, 2)) / dt.to(fp).unsqueeze(1)


def fmr_ic_algo(encoder, p0, p1, maxiter=5, xtol=1e-7, dt=None, g0=None):
    """fmr/model.py:318-405 SolveRegistration.ic_algo behind the decoder branch, as 2 + 2 maxiter launches of the head (perturb 1,
    pinv 1, update 2 per iteration; 12 at maxiter = 5) plus one ops.rigid_apply per iteration, around the encoder's calls:
    f0 = encoder(p0); the perturbed features (fmr_approx_jac); pinv (fmr.ic_pinv); then `maxiter` times
    p = g p1 (ops.rigid_apply with R and t sliced from g, so gradients reach g through it), f1 = encoder(p) and fmr.ic_update.
    p0, p1 (B, N, 3) on the GPU; dt the reference's (1, 6) parameter or (B, 6) (default 1e-2 everywhere); g0 (B, 4, 4) (default
    the identity).  Returns (r (B, K), g (B, 4, 4), g_series (maxiter, B, 4, 4), stop int32 (1,), info int32 (B,)).

    No host read-back: the reference's `float(check) < xtol` is evaluated on the device, every iteration is issued, and a loop
    that has stopped leaves g unchanged bit for bit -- so g_series holds the LAST pose where the reference's g_series_gpu keeps
    zeros (`stop` is 1 then: torch.where puts the zeros back), r is the stopping iteration's, and the call can be captured
    (rrl_hip/graph.py) when the encoder can.  A singular H does not raise: info is 1 for that sample and its pose stays g0."""
    from . import fmr
    if isinstance(maxiter, bool) or int(maxiter) != maxiter or maxiter < 1:
        raise ValueError(f"maxiter must be a positive integer, got {maxiter!r}")
    B = p0.shape[0]
    if dt is None:
        dt = torch.full((1, 6), 1.0e-2, device=p0.device)
    dt = dt.to(p0).reshape(-1, 6).expand(B, 6)
    g = torch.eye(4, device=p0.device).expand(B, 4, 4).contiguous() if g0 is None else g0
    f0 = encoder(p0)
    fp = fmr_approx_jac(encoder, p0, f0, dt, features_only=True)
    pinv, info = fmr.ic_pinv(f0, fp, dt, with_info=True)
    stop = fmr.new_stop(p0.device)
    series, r = [], None
    for _ in range(int(maxiter)):
        p = _ops.rigid_apply(p1, g[:, :3, :3], g[:, :3, 3], transpose_r=True)
        r, _, g, stop = fmr.ic_update(pinv, f0, encoder(p), g, stop, xtol)
        series.append(g)
    return r, g, torch.stack(series), stop, info


# ---- FMR's feature extractor: the PointNet encoder as one node ------------------------------------------
def fmr_encoder(dim_k=1024, state_dict=None):
    """fmr/model.py:105-126 PointNet(dim_k) as pointnet.Encoder: a torch.nn.Module with the reference's state_dict keys and shapes
    (h1.0.weight (64, 3, 1) ... h2.7.bias), on the current GPU, whose forward (B, N, 3) -> (B, dim_k) is ONE node of the library.
    state_dict: a reference checkpoint's encoder weights, loaded with strict=True.  fmr_ic_algo(fmr_encoder(...), p0, p1) is then
    the whole ic_algo with nothing of it in eager torch."""
    from . import pointnet
    net = pointnet.Encoder.fmr(dim_k)
    if state_dict is not None:
        net.load_state_dict({k: torch.as_tensor(v) for k, v in state_dict.items()}, strict=True)
    return net.to(_ops.require_gpu())
