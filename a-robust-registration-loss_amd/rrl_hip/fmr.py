"""FMR's inverse-compositional pose head on the device (include/rrl.h rrl_ic_*): what
SolveRegistration.ic_algo and approx_Jac (fmr/model.py:318-439) do between the encoder's outputs and the poses, as three nodes --

    out  = ic_perturb(p0, dt)                       # (B, 6, N, 3): exp(-dt_i e_i) applied to the template, gradient to dt
    pinv = ic_pinv(f0, fp, dt)                      # (B, 6, K): J = (f0 - fp) / dt, H = J^T J, H^-1 J^T; all three get gradients
    r, dx, g_new, stop = ic_update(pinv, f0, f1, g, stop, xtol)      # r = f1 - f0, dx = -pinv r, the stop rule, exp(dx) g

The encoder between them stays the caller's torch module.  Sums are fixed-order double sums, the gradients follow the
reference's own rules (InvMatrix.backward; ExpMap.backward, which for a general twist is not the exact derivative of exp), the
stop rule is evaluated on the device (no host read-back: a loop of these nodes can be captured), and every call gives the same
bits.  A singular H does not raise: that sample is flagged (info = 1), its pinv is exactly 0 and its pose does not move.

Deviation from the reference: once the batch has stopped, the reference leaves the later entries of g_series_gpu zero (its loss
then evaluates a collapsed cloud); here every later g_new is the last pose, and `stop` (1 from the stopping call on) lets a caller
put the zeros back.  A NaN dx does not stop the batch (NaN < xtol is false, as in the reference): that sample's pose becomes NaN.
There is no fallback: without the library or a GPU every call raises.
"""
import torch

from . import _lib, ops
from ._abi import CONSTANTS

MAX_B = 65535
MAX_K = CONSTANTS["RRL_IC_MAX_K"]
WS_DOUBLES = CONSTANTS["RRL_IC_WS_DOUBLES"]   # per sample: H^-1 (36), the flag, padding


def _batch(B, who):
    if B < 1 or B > MAX_B:
        raise ValueError(f"{who} serves 1 to {MAX_B} samples per call; got {B}: split the batch")


def check_perturb(p0_shape, dt_shape):
    """The refusals of ic_perturb that need no GPU (ValueError)."""
    if len(p0_shape) != 3 or p0_shape[2] != 3:
        raise ValueError(f"ic_perturb: p0 must be (B, N, 3); got {tuple(p0_shape)}")
    B, N = p0_shape[:2]
    _batch(B, "ic_perturb")
    if N < 1:
        raise ValueError("ic_perturb: an empty cloud")
    if tuple(dt_shape) != (B, 6):
        raise ValueError(f"ic_perturb: dt must be (B, 6) = {(B, 6)} (expand the reference's (1, 6) parameter); got {tuple(dt_shape)}")


def check_pinv(f0_shape, fp_shape, dt_shape):
    """The refusals of ic_pinv that need no GPU (ValueError)."""
    if len(f0_shape) != 2:
        raise ValueError(f"ic_pinv: f0 must be (B, K); got {tuple(f0_shape)}")
    B, K = f0_shape
    _batch(B, "ic_pinv")
    if K < 1 or K > MAX_K:
        raise ValueError(f"ic_pinv: the feature dimension K must lie in [1, {MAX_K}]; got {K}")
    if tuple(fp_shape) != (B, 6, K):
        raise ValueError(f"ic_pinv: fp must be (B, 6, K) = {(B, 6, K)}, the encoder's output on the perturbed clouds viewed as "
                         f"(B, 6, K); got {tuple(fp_shape)}")
    if tuple(dt_shape) != (B, 6):
        raise ValueError(f"ic_pinv: dt must be (B, 6) = {(B, 6)}; got {tuple(dt_shape)}")


def check_update(pinv_shape, f0_shape, f1_shape, g_shape, stop_shape=(1,), xtol=0.0):
    """The refusals of ic_update that need no GPU (ValueError)."""
    if len(pinv_shape) != 3 or pinv_shape[1] != 6:
        raise ValueError(f"ic_update: pinv must be (B, 6, K); got {tuple(pinv_shape)}")
    B, _, K = pinv_shape
    _batch(B, "ic_update")
    if K < 1 or K > MAX_K:
        raise ValueError(f"ic_update: the feature dimension K must lie in [1, {MAX_K}]; got {K}")
    for shape, name in ((f0_shape, "f0"), (f1_shape, "f1")):
        if tuple(shape) != (B, K):
            raise ValueError(f"ic_update: {name} must be (B, K) = {(B, K)}; got {tuple(shape)}")
    if tuple(g_shape) != (B, 4, 4):
        raise ValueError(f"ic_update: g must be (B, 4, 4) = {(B, 4, 4)}; got {tuple(g_shape)}")
    if tuple(stop_shape) != (1,):
        raise ValueError(f"ic_update: stop must be one int32 word, shape (1,); got {tuple(stop_shape)}")
    if not xtol >= 0.0:
        raise ValueError(f"ic_update: xtol must be a number >= 0; got {xtol!r}")


def check_request(kind, *shapes, **kw):
    """check_request("perturb" | "pinv" | "update", shapes...): the refusals of a node that need no GPU (ValueError)."""
    table = {"perturb": check_perturb, "pinv": check_pinv, "update": check_update}
    if kind not in table:
        raise ValueError(f"check_request: kind must be one of {sorted(table)}; got {kind!r}")
    return table[kind](*shapes, **kw)


def _grad(t, like):
    """An incoming gradient as the kernels read it, or None."""
    return None if t is None else t.detach().to(dtype=torch.float32, device=like.device).contiguous()


class _Perturb(torch.autograd.Function):
    """ONE autograd node: rrl_ic_perturb_fwd forwards, rrl_ic_perturb_bwd backwards (to dt only)."""

    @staticmethod
    def forward(ctx, p0, dt):
        dev = ops._home(p0, dt)
        p, d = ops._prep(p0, "p0", 3, dev), ops._prep(dt, "dt", 6, dev)
        B, N = p.shape[:2]
        out = torch.empty(B, 6, N, 3, device=dev)
        ops._run(dev, "rrl_ic_perturb_fwd", ops._p(p), ops._p(d), ops._p(out), B, N)
        ctx.keep = (p, d)
        ctx.dev = dt.device
        ctx.set_materialize_grads(False)
        return out.to(p0.device)

    @staticmethod
    def backward(ctx, g_out):
        p, d = ctx.keep
        if g_out is None or not ctx.needs_input_grad[1]:
            return None, None
        g = _grad(g_out, p)
        g_dt = torch.empty_like(d)
        ops._run(p.device, "rrl_ic_perturb_bwd", ops._p(p), ops._p(d), ops._p(g), ops._p(g_dt), p.shape[0], p.shape[1])
        return None, g_dt.to(ctx.dev)


def ic_perturb(p0, dt):
    """(B, 6, N, 3): the template p0 (B, N, 3) under the six perturbations D_i = exp(-dt_i e_i) of approx_Jac
    (fmr/model.py:416-424), dt (B, 6): D_i in double, rounded once, each point one float32 fmaf chain (rrl_rigid_apply_fwd's).
    Differentiable in dt only: p0 carries no gradient in the reference.  One launch each way."""
    for t, name in ((p0, "p0"), (dt, "dt")):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
    check_perturb(tuple(p0.shape), tuple(dt.shape))
    return _Perturb.apply(p0, dt)


class _Pinv(torch.autograd.Function):
    """ONE autograd node: rrl_ic_pinv_fwd forwards, rrl_ic_pinv_bwd backwards on the H^-1 and the flag the forward kept."""

    @staticmethod
    def forward(ctx, f0, fp, dt):
        dev = ops._home(f0, fp, dt)
        a, p, d = ops._prep(f0, "f0", None, dev), ops._prep(fp, "fp", None, dev), ops._prep(dt, "dt", 6, dev)
        B, K = a.shape
        ws = torch.empty(B * WS_DOUBLES, dtype=torch.float64, device=dev)
        pinv = torch.empty(B, 6, K, device=dev)
        info = torch.empty(B, dtype=torch.int32, device=dev)
        P = ops._p
        ctx.call = (P(a), P(p), P(d), P(ws), ws.numel() * 8)
        ctx.dims = (B, K)
        ops._run(dev, "rrl_ic_pinv_fwd", *ctx.call, P(pinv), P(info), B, K)
        ctx.keep = (a, p, d, ws)
        ctx.devs = (f0.device, fp.device, dt.device)
        ctx.mark_non_differentiable(info)
        ctx.set_materialize_grads(False)
        return pinv.to(f0.device), info

    @staticmethod
    def backward(ctx, g_pinv, _gi):
        a, p, d, _ = ctx.keep
        if g_pinv is None:
            return None, None, None
        g = _grad(g_pinv, a)
        need = ctx.needs_input_grad
        out = [torch.empty_like(t) if need[i] else None for i, t in enumerate((a, p, d))]
        P = ops._p
        if any(o is not None for o in out):
            ops._run(a.device, "rrl_ic_pinv_bwd", *ctx.call, P(g), P(out[0]), P(out[1]), P(out[2]), *ctx.dims)
        return tuple(o.to(dv) if o is not None else None for o, dv in zip(out, ctx.devs))


def ic_pinv(f0, fp, dt, with_info=False):
    """pinv (B, 6, K) = H^-1 J^T with J[k][i] = (f0[k] - fp[i][k]) / dt[i] and H = J^T J (fmr/model.py:367-374, 426-431), from
    f0 (B, K), fp (B, 6, K) -- the encoder's output on ic_perturb's clouds viewed as (B, 6, K) -- and dt (B, 6); differentiable
    in all three by one node (InvMatrix.backward composed with the two bmm's).  Double throughout, one rounding per output.
    with_info=True also returns info (B,) int32: 1 where H is singular to the rounding of its own sums (K < 6 included), an
    input of the sample is NaN or infinite, or a dt_i is 0 -- that sample's pinv is exactly 0 (its pose will not move) and it gets
    zero gradients -- else 0.  This replaces the reference's `except RuntimeError`."""
    for t, name in ((f0, "f0"), (fp, "fp"), (dt, "dt")):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
    check_pinv(tuple(f0.shape), tuple(fp.shape), tuple(dt.shape))
    pinv, info = _Pinv.apply(f0, fp, dt)
    return (pinv, info) if with_info else pinv


class _Update(torch.autograd.Function):
    """ONE autograd node: rrl_ic_update_fwd forwards, rrl_ic_update_bwd backwards on the r, dx and decision the forward kept."""

    @staticmethod
    def forward(ctx, pinv, f0, f1, g, stop, xtol):
        dev = stop.device
        pv, a, b, gg = (ops._prep(t, n, None, dev) for t, n in ((pinv, "pinv"), (f0, "f0"), (f1, "f1"), (g, "g")))
        B, _, K = pv.shape
        ws = torch.empty((B + 1) // 2, dtype=torch.float64, device=dev)
        r, dx, g_new = torch.empty(B, K, device=dev), torch.empty(B, 6, device=dev), torch.empty(B, 4, 4, device=dev)
        stopped = torch.empty(1, dtype=torch.int32, device=dev)
        P = ops._p
        ops._run(dev, "rrl_ic_update_fwd", P(pv), P(a), P(b), P(gg), float(xtol), P(stop), P(ws), ws.numel() * 8, P(r), P(dx),
                 P(g_new), P(stopped), B, K)
        ops._touched(stop)
        ctx.keep = (pv, r, dx, gg, stopped)
        ctx.dims = (B, K)
        ctx.devs = (pinv.device, f0.device, f1.device, g.device)
        ctx.set_materialize_grads(False)   # an output the loss left out reaches the kernel as NULL, not as a zero tensor
        return r, dx, g_new

    @staticmethod
    def backward(ctx, g_r, g_dx, g_g):
        pv, r, dx, gg, stopped = ctx.keep
        if g_r is None and g_dx is None and g_g is None:
            return (None,) * 6
        need = ctx.needs_input_grad
        d_pinv = torch.empty_like(pv) if need[0] else None
        d_f0 = torch.empty_like(r) if need[1] else None
        d_f1 = torch.empty_like(r) if need[2] else None
        d_g = torch.empty_like(gg) if need[3] else None
        P = ops._p
        if any(o is not None for o in (d_pinv, d_f0, d_f1, d_g)):
            ops._run(pv.device, "rrl_ic_update_bwd", P(pv), P(r), P(dx), P(gg), P(stopped), P(_grad(g_g, pv)), P(_grad(g_r, pv)),
                     P(_grad(g_dx, pv)), P(d_g), P(d_pinv), P(d_f0), P(d_f1), *ctx.dims)
        out = (d_pinv, d_f0, d_f1, d_g)
        return tuple(o.to(dv) if o is not None else None for o, dv in zip(out, ctx.devs)) + (None, None)


def new_stop(device=None):
    """The stop word of one ic_update loop: a zeroed int32 (1,) on the GPU."""
    return torch.zeros(1, dtype=torch.int32, device=device if device is not None else ops.require_gpu())


def ic_update(pinv, f0, f1, g, stop, xtol=1e-7):
    """One iteration of ic_algo behind the encoder (fmr/model.py:389-399): r = f1 - f0 (B, K), dx = -pinv r (B, 6), the
    reference's batch-wide test max_b |dx_b| < xtol, and g_new = exp(dx) g (B, 4, 4).  `stop` is the loop's int32 (1,) word on
    the GPU (new_stop(); zero it once per loop): when it is already set, or the test holds, it becomes 1 and g_new = g bit for
    bit for EVERY sample; else the poses move.  Nothing is read back.  Returns (r, dx, g_new, stop) -- stop is the same tensor,
    updated in place.  One node, differentiable in pinv, f0, f1 and g; the gradient through exp is ExpMap.backward's rule
    (se_math/se3.py:146-165) word for word, d g_new / d dx_k = gen_k exp(dx) g, which for a general twist is not the exact
    derivative; a stopped call passes the pose gradient through and sends nothing to pinv."""
    for t, name in ((pinv, "pinv"), (f0, "f0"), (f1, "f1"), (g, "g"), (stop, "stop")):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
    check_update(tuple(pinv.shape), tuple(f0.shape), tuple(f1.shape), tuple(g.shape), tuple(stop.shape), float(xtol))
    if not stop.is_cuda or stop.dtype != torch.int32 or not stop.is_contiguous():
        raise ValueError(f"ic_update: stop must be a contiguous int32 tensor on the GPU (fmr.new_stop()); got {stop.dtype} on {stop.device}")
    r, dx, g_new = _Update.apply(pinv, f0, f1, g, stop, float(xtol))
    return r, dx, g_new, stop
