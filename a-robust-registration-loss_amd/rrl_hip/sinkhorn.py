"""Sinkhorn soft assignment on the device (include/rrl.h rrl_sinkhorn_fwd / rrl_sinkhorn_bwd): RPM's
match head -- sinkhorn(affinity), exp, the weighted reference points and the two sums of the permutation matrix
(rpm/models/rpmnet.py:48-118, 211-222) -- as one node in front of the Kabsch solve.

    W, s, c = soft_assign(log_alpha, xyz_ref, n_iters=5, slack=True)    # differentiable in log_alpha and xyz_ref

The normalised matrix is never stored: the iteration runs on two dual potentials per sample, held in double; every sum is a
fixed-order double sum and the result is the same bits on every call.  There is no fallback: without the library or a GPU
every call raises.
"""
import ctypes

import torch

from . import _lib, ops

MAX_B = 32767
MAX_DIM = 16384   # J, K of one call
MAX_ITERS = 64


def check_request(log_alpha_shape, xyz_ref_shape, n_iters=5, eps=1e-5, counts_src_shape=None, counts_ref_shape=None,
                  early_stop_eps=-1.0):
    """The refusals of soft_assign that need no GPU (ValueError)."""
    if early_stop_eps is not None and early_stop_eps > 0:
        raise ValueError("soft_assign: the reference's early termination (sinkhorn(eps > 0), handcrafted RPM only) is not "
                         "offered: the number of iterations is fixed when the call is issued")
    if len(log_alpha_shape) != 3 or len(xyz_ref_shape) != 3 or log_alpha_shape[0] != xyz_ref_shape[0]:
        raise ValueError("soft_assign takes log_alpha (B, J, K) and xyz_ref (B, K, 3) with the same B")
    B, J, K = log_alpha_shape
    if tuple(xyz_ref_shape[1:]) != (K, 3):
        raise ValueError(f"soft_assign: xyz_ref must be (B, K, 3) = {(B, K, 3)}, one point per column of log_alpha; got "
                         f"{tuple(xyz_ref_shape)}")
    if B < 1 or B > MAX_B:
        raise ValueError(f"soft_assign serves 1 to {MAX_B} samples per call; got {B}: split the batch")
    if J < 1 or K < 1 or J > MAX_DIM or K > MAX_DIM:
        raise ValueError(f"soft_assign: J and K must lie in [1, {MAX_DIM}]; got {J} and {K}")
    if int(n_iters) != n_iters or n_iters < 0 or n_iters > MAX_ITERS:
        raise ValueError(f"soft_assign: n_iters must be an integer in [0, {MAX_ITERS}]; got {n_iters}")
    if not eps >= 0.0:
        raise ValueError(f"soft_assign: eps (added to the row sums in W's denominator) must be >= 0; got {eps}")
    for shape, name in ((counts_src_shape, "counts_src"), (counts_ref_shape, "counts_ref")):
        if shape is not None and tuple(shape) != (B,):
            raise ValueError(f"soft_assign: {name} must be (B,) = {(B,)}; got {tuple(shape)}")


def _call(A, x, n_iters, slack, eps, cs, cr, want_log_perm):
    """The filled rrl_sinkhorn_args of one call and the buffers it points into: (k, ws, W, s, c, log_perm, info)."""
    dev = A.device
    B, J, K = A.shape
    lib = _lib.load()
    ws = torch.empty(int(lib.rrl_sinkhorn_workspace_bytes(B, J, K, n_iters)) // 8, dtype=torch.float64, device=dev)
    W, s, c = torch.empty(B, J, 3, device=dev), torch.empty(B, J, device=dev), torch.empty(B, K, device=dev)
    log_perm = torch.empty(B, J, K, device=dev) if want_log_perm else None
    info = torch.empty(B, dtype=torch.int32, device=dev)
    P = ops._p
    k = _lib.SinkhornArgs()
    k.struct_bytes = ctypes.sizeof(k)
    k.B, k.J, k.K, k.n_iters, k.slack = B, J, K, int(n_iters), int(bool(slack))
    k.log_alpha, k.xyz_ref, k.count_src, k.count_ref, k.eps = P(A), P(x), P(cs), P(cr), float(eps)
    k.ws, k.ws_bytes, k.W, k.s, k.c, k.log_perm, k.info = P(ws), ws.numel() * 8, P(W), P(s), P(c), P(log_perm), P(info)
    return k, ws, W, s, c, log_perm, info


class _SoftAssign(torch.autograd.Function):
    """ONE autograd node: rrl_sinkhorn_fwd forwards, rrl_sinkhorn_bwd backwards, on the potentials the forward kept."""

    @staticmethod
    def forward(ctx, log_alpha, xyz_ref, n_iters, slack, eps, counts_src, counts_ref, want_log_perm):
        dev = ops._home(log_alpha, xyz_ref)
        A, x = ops._prep(log_alpha, "log_alpha", None, dev), ops._prep(xyz_ref, "xyz_ref", 3, dev)
        B, J, K = A.shape
        cs, cr = ops.check_counts(counts_src, B, J, dev, "counts_src"), ops.check_counts(counts_ref, B, K, dev, "counts_ref")
        k, ws, W, s, c, log_perm, info = _call(A, x, n_iters, slack, eps, cs, cr, want_log_perm)
        ops._run(dev, "rrl_sinkhorn_fwd", ctypes.byref(k))
        ctx.k, ctx.keep = k, (A, x, cs, cr, ws, W, s, c, log_perm, info)
        ctx.devs = (log_alpha.device, xyz_ref.device)
        if log_perm is None:
            log_perm = torch.empty(0, device=dev)
        ctx.mark_non_differentiable(info, log_perm)
        to = log_alpha.device
        return W.to(to), s.to(to), c.to(to), info, log_perm

    @staticmethod
    def backward(ctx, gW, gs, gc, _gi, _gl):
        A, x = ctx.keep[0], ctx.keep[1]
        dev = A.device
        f32 = dict(dtype=torch.float32, device=dev)
        up = [g.detach().to(**f32).contiguous() if g is not None else None for g in (gW, gs, gc)]
        gA = torch.empty_like(A)
        gx = torch.empty_like(x) if ctx.needs_input_grad[1] else None
        P = ops._p
        ops._run(dev, "rrl_sinkhorn_bwd", ctypes.byref(ctx.k), P(up[0]), P(up[1]), P(up[2]), P(gA), P(gx))
        return (gA.to(ctx.devs[0]) if ctx.needs_input_grad[0] else None, gx.to(ctx.devs[1]) if gx is not None else None,
                None, None, None, None, None, None)


def soft_assign(log_alpha, xyz_ref, n_iters=5, slack=True, eps=1e-5, counts_src=None, counts_ref=None, with_info=False,
                return_log_perm=False, early_stop_eps=-1.0):
    """(W (B, J, 3), s (B, J), c (B, K)) from log_alpha (B, J, K) and xyz_ref (B, K, 3): with
    P = exp(sinkhorn(log_alpha, n_iters, slack)) of rpm/models/rpmnet.py:48-118, s = P.sum(2), c = P.sum(1) and
    W = P @ xyz_ref / (s + eps) (rpmnet.py:214-222; eps: RPM's 1e-5).  Differentiable in log_alpha and in xyz_ref (through W)
    by one node; n_iters = 0 is P = exp(log_alpha).
    counts_src / counts_ref ((B,) list or int32 GPU tensor): sample b has its first counts_src[b] rows and counts_ref[b]
    columns; the rest is never read and gets s = 0, W = 0, c = 0 and zero gradient.
    -inf entries are legal with slack (P = 0, gradient 0).  with_info=True also returns info (B,) int32: 1 where a NaN or
    +inf entry was met inside the counts (that sample's outputs are then NaN or inf where the entry reaches), else 0.
    return_log_perm=True also returns log_perm (B, J, K) = sinkhorn(...) itself, detached (for the trainer's endpoints; -inf
    beyond the counts): no gradient flows through it.
    The reference's early termination (its eps > 0; here early_stop_eps) is refused with a ValueError.
    Returns W, s, c [, info] [, log_perm]."""
    for t, name in ((log_alpha, "log_alpha"), (xyz_ref, "xyz_ref")):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")

    def shape_of(cnt):
        if cnt is None:
            return None
        return tuple(cnt.shape) if isinstance(cnt, torch.Tensor) else tuple(torch.as_tensor(cnt).shape)
    check_request(tuple(log_alpha.shape), tuple(xyz_ref.shape), n_iters, eps, shape_of(counts_src), shape_of(counts_ref),
                  early_stop_eps)
    B, J, K = log_alpha.shape
    for cnt, cap, name in ((counts_src, J, "counts_src"), (counts_ref, K, "counts_ref")):
        if cnt is not None:
            ops.check_counts_host(cnt, B, cap, name)
    W, s, c, info, log_perm = _SoftAssign.apply(log_alpha, xyz_ref, int(n_iters), bool(slack), float(eps), counts_src,
                                                counts_ref, bool(return_log_perm))
    out = (W, s, c)
    if with_info:
        out += (info,)
    if return_log_perm:
        out += (log_perm,)
    return out
