"""Closed-form rigid fits on the device (include/rrl.h rrl_kabsch_fwd / rrl_kabsch_bwd): the weighted
Kabsch solve the trainers of this loss end in, for a batch, in one or two launches, with its gradient.

    R, T = kabsch(a, b, w)                                   # x -> x R + T fits a onto b; differentiable in a, b, w
    R, T, info, fit = kabsch_from_keys(a, keys, b)           # partners from a Chamfer walk's keys; no gradient

Every sum is a fixed-order double sum, the 3 x 3 SVD is a double Jacobi iteration, the result is rounded to float32 once and
is the same bits on every call.  There is no fallback: without the library or a GPU every call raises.
"""
import ctypes

import torch

from . import _lib, ops

RANK_TOL = 1e-6  # (s1 + delta s2) <= RANK_TOL s0: the rotation is not determined.  The inputs are float32: a gap below
#                  2^-24 ~ 6e-8 of s0 is their own rounding, and the gradient grows like 1 / gap; 1e-6 keeps an order of
#                  magnitude above that noise
MAX_B = 32767


def check_request(a_shape, b_shape, w_shape=None, keys_shape=None, counts_shape=None, max_sqdist=None):
    """The refusals of kabsch / kabsch_from_keys that need no GPU (ValueError)."""
    if len(a_shape) != 3 or len(b_shape) != 3 or a_shape[0] != b_shape[0]:
        raise ValueError("kabsch takes a (B, n, 3 or 9) and b (B, m, 3 or 9) with the same B")
    if a_shape[2] not in (3, 9) or b_shape[2] not in (3, 9):
        raise ValueError("kabsch: rows are points (.., 3) or pseudo-triangles (.., 9), whose first points are read in place")
    B, n, m = a_shape[0], a_shape[1], b_shape[1]
    if B > MAX_B:
        raise ValueError(f"kabsch serves up to {MAX_B} samples per call; got {B}: split the batch")
    if n < 1 or m < 1:
        raise ValueError("kabsch: empty clouds (n == 0 or m == 0) have no fit")
    if keys_shape is None and n != m:
        raise ValueError(f"kabsch pairs a[i] with b[i]: n must equal m, got {n} and {m}; for partners from a Chamfer walk use "
                         "kabsch_from_keys")
    if keys_shape is not None and tuple(keys_shape) != (B, n):
        raise ValueError(f"kabsch_from_keys: keys must be (B, n) = {(B, n)}, one key per row of a; got {tuple(keys_shape)}")
    if w_shape is not None and tuple(w_shape) != (B, n):
        raise ValueError(f"kabsch: w must be (B, n) = {(B, n)}; got {tuple(w_shape)}")
    if counts_shape is not None and tuple(counts_shape) != (B,):
        raise ValueError(f"kabsch: counts must be (B,) = {(B,)}; got {tuple(counts_shape)}")
    if max_sqdist is not None and keys_shape is None:
        raise ValueError("kabsch: max_sqdist gates on the keys' distance words and needs keys (kabsch_from_keys)")


def _rows(t, name, dev):
    """float32, contiguous, on dev; (B, n, 3) or (B, n, 9) -> (tensor, floats per row)."""
    t = ops._prep(t, name, None, dev)
    return t, t.shape[2]


def _fit(a, b, w, keys, count_a, count_b, gate, eps, transpose_r, rank_tol, dev):
    """One rrl_kabsch_fwd call -> (args kept for a backward, R, T, info, fit)."""
    B, n, m = a.shape[0], a.shape[1], b.shape[1]
    lib = _lib.load()
    part = torch.empty(max(int(lib.rrl_kabsch_part_bytes(B, n)) // 8, 1), dtype=torch.float64, device=dev)
    R, T = torch.empty(B, 3, 3, device=dev), torch.empty(B, 3, device=dev)
    fit = torch.empty(B, _lib.FIT_DOUBLES, dtype=torch.float64, device=dev)
    info = torch.empty(B, 4, dtype=torch.int32, device=dev)
    P = ops._p
    k = _lib.KabschArgs()
    k.struct_bytes = ctypes.sizeof(k)
    k.B, k.n, k.m, k.a_stride, k.b_stride, k.transpose_r = B, n, m, a.shape[2], b.shape[2], int(bool(transpose_r))
    k.a, k.b, k.w, k.keys, k.count_a, k.count_b, k.gate_sq = P(a), P(b), P(w), P(keys), P(count_a), P(count_b), P(gate)
    k.eps_w, k.rank_tol = float(eps), float(rank_tol)
    k.part, k.part_bytes, k.R, k.T, k.fit, k.info = P(part), part.numel() * 8, P(R), P(T), P(fit), P(info)
    ops._run(dev, "rrl_kabsch_fwd", ctypes.byref(k))
    return k, R, T, info, fit


class _Kabsch(torch.autograd.Function):
    """The dense fit as ONE autograd node: rrl_kabsch_fwd forwards, one rrl_kabsch_bwd launch backwards."""

    @staticmethod
    def forward(ctx, a, b, w, counts, eps, transpose_r, rank_tol):
        dev = ops._home(a, b, w)
        av, bv = ops._prep(a, "a", None, dev), ops._prep(b, "b", None, dev)
        wv = ops._prep(w, "w", None, dev) if w is not None else None
        B, n = av.shape[0], av.shape[1]
        cnt = ops.check_counts(counts, B, n, dev, "counts")
        k, R, T, info, fit = _fit(av, bv, wv, None, cnt, cnt, None, eps, transpose_r, rank_tol, dev)
        ctx.k, ctx.keep = k, (av, bv, wv, cnt, fit, info)
        ctx.devs = (a.device, b.device, w.device if w is not None else None)
        ctx.shapes = (a.shape, b.shape)
        ctx.mark_non_differentiable(info, fit)
        return R.to(a.device), T.to(a.device), info, fit

    @staticmethod
    def backward(ctx, gR, gT, _gi, _gf):
        av, bv, wv, cnt, fit, info = ctx.keep
        dev = av.device
        B, n = av.shape[0], av.shape[1]
        f32 = dict(dtype=torch.float32, device=dev)
        gRv = gR.detach().to(**f32).reshape(B, 9).contiguous() if gR is not None else None
        gTv = gT.detach().to(**f32).reshape(B, 3).contiguous() if gT is not None else None
        need = ctx.needs_input_grad
        ga = torch.empty(B, n, 3, **f32) if need[0] else None
        gb = torch.empty(B, n, 3, **f32) if need[1] else None
        gw = torch.empty(B, n, **f32) if need[2] else None
        P = ops._p
        ops._run(dev, "rrl_kabsch_bwd", ctypes.byref(ctx.k), P(gRv), P(gTv), P(ga), P(gb), P(gw))

        def widen(g, shape, to):  # a (B, n, 9) input: the gradient lives in its first three columns
            if g is None:
                return None
            if shape[2] != 3:
                full = torch.zeros(shape, **f32)
                full[:, :, :3] = g
                g = full
            return g.to(to)
        return (widen(ga, ctx.shapes[0], ctx.devs[0]), widen(gb, ctx.shapes[1], ctx.devs[1]),
                gw.to(ctx.devs[2]) if gw is not None else None, None, None, None, None)


def kabsch(a, b, w=None, *, counts=None, eps=0.0, transpose_r=False, rank_tol=RANK_TOL, with_info=False):
    """(R (B, 3, 3), T (B, 3)): the weighted least-squares rigid fit of a (B, n, 3) onto b (B, n, 3), a[i] paired with b[i],
    in the row convention x -> x R + T (transpose_r=True returns R^T, the matrix that moves column vectors: RPM's rot_mat,
    DCP's r).  w (B, n): weights, default 1; eps: added to sum w in the normalisation (RPM: 1e-5).  (B, n, 9) inputs are
    pseudo-triangles whose first points are read in place.  counts ((B,) list or int32 GPU tensor): sample b has its first
    counts[b] pairs; the rest is never read.  Differentiable in a, b and w through one node.  A sample with fewer than 3
    pairs or no weight gets (I, 0); one whose points are collinear gets a fit whose rotation about the line is arbitrary; both
    get ZERO gradient, and info[:, 1] (with_info=True: also returns info (B, 4) int32 and fit (B, 32) float64) says which."""
    for t, name in ((a, "a"), (b, "b")) + (((w, "w"),) if w is not None else ()):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
    check_request(tuple(a.shape), tuple(b.shape), tuple(w.shape) if w is not None else None, None,
                  tuple(torch.as_tensor(counts).shape) if counts is not None and not isinstance(counts, torch.Tensor)
                  else (tuple(counts.shape) if counts is not None else None))
    if counts is not None:
        ops.check_counts_host(counts, a.shape[0], a.shape[1], "counts")
    R, T, info, fit = _Kabsch.apply(a, b, w, counts, float(eps), bool(transpose_r), float(rank_tol))
    return (R, T, info, fit) if with_info else (R, T)


def kabsch_from_keys(a, keys, b, *, w=None, counts_a=None, counts_b=None, max_sqdist=None, eps=0.0, transpose_r=False,
                     rank_tol=RANK_TOL):
    """(R, T, info (B, 4) int32, fit (B, 32) float64): the fit of a (B, n, 3 or 9) onto its partners b[key & 0xffffffff]
    among b (B, m, 3 or 9), keys (B, n) int64 as ops.chamfer's walk leaves them (distance bits << 32 | index).  A row beyond
    counts_a, an all-ones key and an index beyond m or counts_b contribute nothing and are counted in info[:, 3];
    max_sqdist (a number or (B,)): pairs whose key distance exceeds it get weight 0.  info[:, 0] pairs used, [:, 1] status
    (0 fitted, 1 fewer than 3 pairs or no weight: (I, 0), 2 degenerate), [:, 2] reflection fixed.  No gradient: the pairing
    is not differentiable."""
    for t, name in ((a, "a"), (b, "b"), (keys, "keys")):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
    if keys.dtype != torch.int64:
        raise ValueError("kabsch_from_keys: keys must be int64 (the u64 keys of the Chamfer walk)")
    check_request(tuple(a.shape), tuple(b.shape), tuple(w.shape) if w is not None else None, tuple(keys.shape), None, max_sqdist)
    B, n, m = a.shape[0], a.shape[1], b.shape[1]
    for c, cap, name in ((counts_a, n, "counts_a"), (counts_b, m, "counts_b")):
        if c is not None:
            ops.check_counts_host(c, B, cap, name)
    dev = ops._home(a, b, keys)
    av, bv = ops._prep(a, "a", None, dev), ops._prep(b, "b", None, dev)
    wv = ops._prep(w, "w", None, dev) if w is not None else None
    kv = keys.detach().to(dev).contiguous()
    ca, cb = ops.check_counts(counts_a, B, n, dev, "counts_a"), ops.check_counts(counts_b, B, m, dev, "counts_b")
    gate = None
    if max_sqdist is not None:
        gate = torch.as_tensor(max_sqdist, dtype=torch.float32).to(dev).reshape(-1).expand(B).contiguous()
    _, R, T, info, fit = _fit(av, bv, wv, kv, ca, cb, gate, eps, transpose_r, rank_tol, dev)
    return R, T, info, fit
