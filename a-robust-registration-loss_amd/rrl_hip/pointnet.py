"""A shared-MLP + GroupNorm + ReLU + max-pool encoder on the device (include/rrl.h rrl_pointnet_fwd):
FMR's PointNet (fmr/model.py:57-126) and RPM's ParameterPredictionNet.prepool (rpm/models/feature_nets.py:31-52) --

    x = points.transpose(1, 2)                      # (B, c0, N)
    for every layer: x = relu(group_norm(conv1d(x, W, b), G, gamma, beta))
    features = x.max(dim=2)                         # (B, K)

as one node:

    features = encode(points, params, groups)       # points (B, N, c0)
    net = Encoder.fmr(dim_k=1024)                   # a torch.nn.Module with the reference's state_dict keys and shapes
    features = net(points)

The pre-activations are float32 fmaf chains over the input channels (the matrix cores from 64 channels upward), the group
statistics fixed-order double sums, the last layer's (B, K, N) activation is never formed: the pooled feature is the
activation at the channel's extremum.  Every call gives the same bits.  There is no fallback: without the library or a GPU
every call raises.

The backward (rrl_pointnet_bwd) is double arithmetic on what the forward kept -- the hidden y_l, the statistics, the extrema and
their indices --: the last layer in closed form from S1 and the Gram matrix of its input (no N x K work), the hidden layers by
GroupNorm's dense rule; gradients reach the points and every parameter, an absent one reaches the entry as NULL.

The grouped form (rrl_pointnet_group_fwd / _bwd) runs the same layers over every (point, neighbour slot)
position of x (B, N, S, c0) and takes the max over each point's S slots -- RPM's FeatExtractionEarlyFusion.prepool and its
torch.max(new_feat, 2)[0] (rpm/models/feature_nets.py:196-199):

    out = encode_grouped(x, params, groups)         # (B, K, N)
    net = GroupedEncoder.rpm_feat_prepool()         # keys prepool.0.weight (96, 10, 1, 1) ... prepool.7.bias
"""
import ctypes

import torch

from . import _lib, ops
from ._abi import CONSTANTS

MAX_B = 65535
MAX_N = 1 << 20
MAX_C0 = CONSTANTS["RRL_PN_MAX_C0"]
MAX_LAYERS = CONSTANTS["RRL_PN_MAX_LAYERS"]
MAX_HIDDEN = CONSTANTS["RRL_PN_MAX_HIDDEN"]
MAX_K = CONSTANTS["RRL_IC_MAX_K"]
FIELDS = ("STAT", "COEF", "PART", "EPART", "EXT", "FLAG", "Y")   # include/rrl.h RRL_PN_*
CHUNK = 128   # points per partial sum

FMR_WIDTHS, FMR_GROUPS = (64, 64, 64, 128), (8, 8, 8, 8, 8)
RPM_WIDTHS, RPM_GROUPS = (64, 64, 64, 128, 1024), (8, 8, 8, 8, 16)


def check_request(points_shape, param_shapes, groups, eps=1e-5):
    """The refusals of encode that need no GPU (ValueError).  param_shapes: the shapes of W_1, b_1, gamma_1, beta_1, W_2, ...;
    a W may be (c, c_in) or a Conv1d's (c, c_in, 1).  Returns (B, N, c0, widths)."""
    if len(points_shape) != 3:
        raise ValueError(f"encode: points must be (B, N, c0); got {tuple(points_shape)}")
    B, N, c0 = points_shape
    if B < 1 or B > MAX_B:
        raise ValueError(f"encode serves 1 to {MAX_B} clouds per call; got {B}: split the batch")
    if N < 1 or N > MAX_N:
        raise ValueError(f"encode: N must lie in [1, {MAX_N}]; got {N}")
    if c0 < 1 or c0 > MAX_C0:
        raise ValueError(f"encode: the points' channels c0 must lie in [1, {MAX_C0}]; got {c0}")
    groups = tuple(groups)
    L = len(groups)
    if L < 2 or L > MAX_LAYERS:
        raise ValueError(f"encode: 2 to {MAX_LAYERS} layers; got {L} group counts")
    if len(param_shapes) != 4 * L:
        raise ValueError(f"encode: params must hold W, b, gamma, beta of each of the {L} layers ({4 * L} tensors); got {len(param_shapes)}")
    widths, last = [], c0
    for l in range(L):
        ws, rest = tuple(param_shapes[4 * l]), [tuple(s) for s in param_shapes[4 * l + 1:4 * l + 4]]
        if len(ws) == 3 and ws[2] == 1:
            ws = ws[:2]
        if len(ws) != 2 or ws[1] != last:
            raise ValueError(f"encode: W of layer {l + 1} must be (c, {last}) or (c, {last}, 1); got {tuple(param_shapes[4 * l])}")
        c, G = ws[0], groups[l]
        if any(s != (c,) for s in rest):
            raise ValueError(f"encode: b, gamma and beta of layer {l + 1} must be ({c},); got {rest}")
        if isinstance(G, bool) or int(G) != G or G < 1 or c < 1 or c % G:
            raise ValueError(f"encode: width {c} of layer {l + 1} is no multiple of its group count {G!r}")
        cap = MAX_HIDDEN if l + 1 < L else MAX_K
        if c > cap:
            raise ValueError(f"encode: width {c} of layer {l + 1} exceeds {cap} ({'a hidden layer' if l + 1 < L else 'the last layer'})")
        widths.append(c)
        last = c
    if not eps > 0.0:
        raise ValueError(f"encode: eps must be a number > 0; got {eps!r}")
    return B, N, c0, tuple(widths)


def _ints(values):
    return (ctypes.c_int32 * len(values))(*values)


def workspace_layout(B, N, c0, widths, groups):
    """(bytes, {field: byte offset}) of the workspace (rrl_pointnet_workspace_bytes); bytes is 0 for a refused shape."""
    off = (ctypes.c_size_t * len(FIELDS))()
    n = int(_lib.load().rrl_pointnet_workspace_bytes(B, N, c0, len(widths), _ints(widths), _ints(groups), off))
    return n, dict(zip(FIELDS, (int(o) for o in off)))


def workspace_views(ws, B, N, c0, widths, groups):
    """Named views of a workspace the forward filled (ws: a float32 tensor of the whole workspace): stat (B, sum G, 4) f64,
    coef (B, sum c, 2) f64, part [per layer (B, chunks, c_l, 2)] f64, epart (B, chunks, K, 2) f32 (the index's bits in
    word 1), ext (B, K) f32, flag (B,) int32, y [per hidden layer (B, c_l, N)] f32."""
    nbytes, off = workspace_layout(B, N, c0, widths, groups)
    raw = ws.view(torch.uint8)[:nbytes]
    P, K, ctot, gtot, hid = (N + CHUNK - 1) // CHUNK, widths[-1], sum(widths), sum(groups), sum(widths[:-1])

    def part(name, dtype, count, size):
        return raw[off[name]:off[name] + count * size].view(dtype)
    out = dict(stat=part("STAT", torch.float64, B * gtot * 4, 8).view(B, gtot, 4),
               coef=part("COEF", torch.float64, B * ctot * 2, 8).view(B, ctot, 2),
               epart=part("EPART", torch.float32, B * P * K * 2, 4).view(B, P, K, 2),
               ext=part("EXT", torch.float32, B * K, 4).view(B, K),
               flag=part("FLAG", torch.int32, B, 4),
               y=[], part=[])
    allp = part("PART", torch.float64, B * P * ctot * 2, 8)
    ally = part("Y", torch.float32, B * hid * N, 4).view(B, hid, N)
    c_at = 0
    for l, c in enumerate(widths):
        out["part"].append(allp[2 * B * P * c_at:2 * B * P * (c_at + c)].view(B, P, c, 2))
        if l + 1 < len(widths):
            out["y"].append(ally[:, c_at:c_at + c])
        c_at += c
    return out


def _forward(pts, prm, groups, eps, ws=None):
    """rrl_pointnet_fwd on prepared tensors -> (feat, arg, info, ws); ws: a float32 tensor to use as the workspace."""
    dev = pts.device
    B, N, c0 = pts.shape
    widths = tuple(prm[4 * l].shape[0] for l in range(len(groups)))
    L, K = len(groups), widths[-1]
    wd, gr = _ints(widths), _ints(groups)
    nbytes = int(_lib.load().rrl_pointnet_workspace_bytes(B, N, c0, L, wd, gr, None))
    if ws is None:
        ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=dev)
    feat = torch.empty(B, K, device=dev)
    arg = torch.empty(B, K, dtype=torch.int32, device=dev)
    info = torch.empty(B, dtype=torch.int32, device=dev)
    ptrs = (ctypes.c_void_p * (4 * L))(*[p.data_ptr() for p in prm])
    P = ops._p
    ops._run(dev, "rrl_pointnet_fwd", P(pts), ptrs, wd, gr, float(eps), P(ws), ws.numel() * 4, P(feat), P(arg), P(info), B, N, c0, L)
    return feat, arg, info, ws


def _backward(pts, prm, groups, ws, arg, g_feat, want_points=True, want=None, bws=None, fill=None):
    """rrl_pointnet_bwd on prepared tensors and the forward's ws and arg -> (d_points or None, [dW_1, db_1, dgamma_1, dbeta_1, ...]
    with None where want[i] is false).  want: 4 L booleans (default: all); fill: a value the outputs are pre-filled with (tests)."""
    dev = pts.device
    B, N, c0 = pts.shape
    widths = tuple(prm[4 * l].shape[0] for l in range(len(groups)))
    L = len(groups)
    wd, gr = _ints(widths), _ints(groups)
    want = [True] * (4 * L) if want is None else list(want)
    if bws is None:
        bws = torch.empty(int(_lib.load().rrl_pointnet_bwd_workspace_bytes(B, N, c0, L, wd, gr)) // 8, dtype=torch.float64, device=dev)
    new = torch.empty if fill is None else (lambda *a, **kw: torch.full(*a, fill_value=fill, **kw))
    d_points = new(tuple(pts.shape), device=dev) if want_points else None
    d_prm = [new(tuple(p.shape), device=dev) if w else None for p, w in zip(prm, want)]
    ptrs = (ctypes.c_void_p * (4 * L))(*[p.data_ptr() for p in prm])
    dptrs = (ctypes.c_void_p * (4 * L))(*[d.data_ptr() if d is not None else None for d in d_prm]) if any(want) else None
    P = ops._p
    g = g_feat.detach().to(dtype=torch.float32, device=dev).contiguous()
    ops._run(dev, "rrl_pointnet_bwd", P(pts), ptrs, wd, gr, P(ws), ws.numel() * 4, P(arg), P(g), P(bws), bws.numel() * 8, P(d_points), dptrs,
             B, N, c0, L)
    return d_points, d_prm


class _Encode(torch.autograd.Function):
    """ONE autograd node: rrl_pointnet_fwd forwards, rrl_pointnet_bwd backwards on the y_l, statistics, ext and arg the forward kept."""

    @staticmethod
    def forward(ctx, points, groups, eps, *params):
        dev = ops._home(points, *params)
        pts = ops._prep(points, "points", None, dev)
        prm = [ops._prep(p, "params", None, dev) for p in params]
        feat, arg, info, ws = _forward(pts, prm, groups, eps)
        ctx.keep = (pts, prm, ws, arg)
        ctx.groups = groups
        ctx.devs = (points.device,) + tuple(p.device for p in params)
        ctx.shapes = tuple(p.shape for p in params)
        ctx.mark_non_differentiable(arg, info)
        return feat.to(points.device), arg, info

    @staticmethod
    def backward(ctx, g_feat, _ga, _gi):
        pts, prm, ws, arg = ctx.keep
        need = ctx.needs_input_grad
        if g_feat is None or not (need[0] or any(need[3:])):
            return (None,) * (3 + len(prm))
        d_points, d_prm = _backward(pts, prm, ctx.groups, ws, arg, g_feat, bool(need[0]), need[3:])
        out = [d_points.to(ctx.devs[0]) if d_points is not None else None, None, None]
        out += [d.reshape(sh).to(dv) if d is not None else None for d, sh, dv in zip(d_prm, ctx.shapes, ctx.devs[1:])]
        return tuple(out)


def encode(points, params, groups, eps=1e-5, with_info=False, with_arg=False):
    """features (B, K) of points (B, N, c0) through the layers params = [W_1, b_1, gamma_1, beta_1, W_2, ...] (a W as (c, c_in)
    or a Conv1d's (c, c_in, 1)) with groups[l] GroupNorm groups each, ReLU after every layer and the max over the points at
    the end -- the reference's PointNet.forward as one node, differentiable in the points and every parameter.  with_info=True also returns info (B,) int32: 1 where a group sum
    of the sample is NaN or infinite (its features are then NaN), else 0.  with_arg=True also returns arg (B, K) int32, the
    lowest index of the point that gives each feature.  Returns features [, info] [, arg]."""
    if not isinstance(points, torch.Tensor):
        raise TypeError("points must be a torch.Tensor")
    params = list(params)
    for p in params:
        if not isinstance(p, torch.Tensor):
            raise TypeError("params must be torch.Tensors")
    groups = tuple(int(g) if not isinstance(g, bool) and int(g) == g else g for g in groups)
    check_request(tuple(points.shape), [tuple(p.shape) for p in params], groups, float(eps))
    feat, arg, info = _Encode.apply(points, groups, float(eps), *params)
    out = (feat,)
    if with_info:
        out += (info,)
    if with_arg:
        out += (arg,)
    return out[0] if len(out) == 1 else out


class Encoder(torch.nn.Module):
    """The encoder as a torch.nn.Module.  Its parameters live in torch's own Conv1d / GroupNorm modules, laid out in
    Sequential blocks so that state_dict() has the reference's keys and shapes; forward() is encode().
    blocks: {name: number of layers}, in order -- Encoder.fmr: h1 (2 layers), h2 (3); Encoder.rpm_prepool: prepool (5)."""

    def __init__(self, c0, widths, groups, blocks=None, eps=1e-5):
        super().__init__()
        widths, groups = tuple(int(w) for w in widths), tuple(int(g) for g in groups)
        blocks = dict(blocks) if blocks else {"layers": len(widths)}
        if len(widths) != len(groups) or sum(blocks.values()) != len(widths):
            raise ValueError(f"Encoder: {len(widths)} widths, {len(groups)} group counts and blocks of {sum(blocks.values())} layers")
        shapes, last = [], c0
        for c in widths:
            shapes += [(c, last, 1), (c,), (c,), (c,)]
            last = c
        check_request((1, 1, c0), shapes, groups, eps)
        self.c0, self.widths, self.groups, self.eps = int(c0), widths, groups, float(eps)
        self._blocks = tuple(blocks)
        at, last = 0, c0
        for name, count in blocks.items():
            mods = []
            for c, G in zip(widths[at:at + count], groups[at:at + count]):
                mods += [torch.nn.Conv1d(last, c, 1), torch.nn.GroupNorm(G, c, eps=self.eps), torch.nn.ReLU()]
                last = c
            setattr(self, name, torch.nn.Sequential(*mods))
            at += count

    @classmethod
    def fmr(cls, dim_k=1024):
        """fmr/model.py PointNet(dim_k): keys h1.0.weight (64, 3, 1) ... h2.7.bias."""
        return cls(3, FMR_WIDTHS + (int(dim_k),), FMR_GROUPS, blocks={"h1": 2, "h2": 3})

    @classmethod
    def rpm_prepool(cls):
        """rpm/models/feature_nets.py ParameterPredictionNet.prepool: keys prepool.0.weight (64, 4, 1) ... prepool.13.bias."""
        return cls(4, RPM_WIDTHS, RPM_GROUPS, blocks={"prepool": 5})

    def params(self):
        """[W_1, b_1, gamma_1, beta_1, W_2, ...] as encode takes them."""
        out = []
        for name in self._blocks:
            mods = list(getattr(self, name))
            for conv, norm in zip(mods[0::3], mods[1::3]):
                out += [conv.weight, conv.bias, norm.weight, norm.bias]
        return out

    def forward(self, points, with_info=False, with_arg=False):
        return encode(points, self.params(), self.groups, self.eps, with_info=with_info, with_arg=with_arg)


# ---- the grouped encoder: shared layers over every (point, slot) position, max over each point's slots ---
PG_MAX_C0 = CONSTANTS["RRL_PG_MAX_C0"]
PG_MAX_S = CONSTANTS["RRL_PG_MAX_S"]
PG_MAX_K = CONSTANTS["RRL_PG_MAX_K"]
PG_MAX_P = 1 << 22
PG_FIELDS = ("STAT", "COEF", "PART", "EXT", "FLAG", "Y")   # include/rrl.h RRL_PG_*
RPM_FEAT_GROUPS = (8, 8, 8)


def check_group_request(x_shape, param_shapes, groups, eps=1e-5):
    """The refusals of encode_grouped that need no GPU (ValueError).  param_shapes: the shapes of W_1, b_1, gamma_1, beta_1,
    W_2, ...; a W may be (c, c_in) or a Conv2d's (c, c_in, 1, 1).  Returns (B, N, S, c0, widths)."""
    if len(x_shape) != 4:
        raise ValueError(f"encode_grouped: x must be (B, N, S, c0); got {tuple(x_shape)}")
    B, N, S, c0 = x_shape
    if B < 1 or B > MAX_B:
        raise ValueError(f"encode_grouped serves 1 to {MAX_B} samples per call; got {B}: split the batch")
    if N < 1 or N > MAX_N:
        raise ValueError(f"encode_grouped: N must lie in [1, {MAX_N}]; got {N}")
    if S < 1 or S > PG_MAX_S:
        raise ValueError(f"encode_grouped: the slots per point S must lie in [1, {PG_MAX_S}]; got {S}")
    if N * S > PG_MAX_P:
        raise ValueError(f"encode_grouped: N S must not exceed {PG_MAX_P}; got {N * S}")
    if c0 < 1 or c0 > PG_MAX_C0:
        raise ValueError(f"encode_grouped: the input channels c0 must lie in [1, {PG_MAX_C0}]; got {c0}")
    groups = tuple(groups)
    L = len(groups)
    if L < 2 or L > MAX_LAYERS:
        raise ValueError(f"encode_grouped: 2 to {MAX_LAYERS} layers; got {L} group counts")
    if len(param_shapes) != 4 * L:
        raise ValueError(f"encode_grouped: params must hold W, b, gamma, beta of each of the {L} layers ({4 * L} tensors); got {len(param_shapes)}")
    widths, last = [], c0
    for l in range(L):
        ws, rest = tuple(param_shapes[4 * l]), [tuple(s) for s in param_shapes[4 * l + 1:4 * l + 4]]
        if len(ws) == 4 and ws[2:] == (1, 1):
            ws = ws[:2]
        if len(ws) != 2 or ws[1] != last:
            raise ValueError(f"encode_grouped: W of layer {l + 1} must be (c, {last}) or (c, {last}, 1, 1); got {tuple(param_shapes[4 * l])}")
        c, G = ws[0], groups[l]
        if any(s != (c,) for s in rest):
            raise ValueError(f"encode_grouped: b, gamma and beta of layer {l + 1} must be ({c},); got {rest}")
        if isinstance(G, bool) or int(G) != G or G < 1 or c < 1 or c % G:
            raise ValueError(f"encode_grouped: width {c} of layer {l + 1} is no multiple of its group count {G!r}")
        cap = MAX_HIDDEN if l + 1 < L else PG_MAX_K
        if c > cap:
            raise ValueError(f"encode_grouped: width {c} of layer {l + 1} exceeds {cap} ({'a hidden layer' if l + 1 < L else 'the last layer'})")
        widths.append(c)
        last = c
    if not eps > 0.0:
        raise ValueError(f"encode_grouped: eps must be a number > 0; got {eps!r}")
    return B, N, S, c0, tuple(widths)


def group_chunks(N, S):
    """(points per chunk, chunks) of the forward's partial sums: a chunk is floor(128 / S) whole points."""
    ppc = 128 // S
    return ppc, (N + ppc - 1) // ppc


def group_workspace_layout(B, N, S, c0, widths, groups):
    """(bytes, {field: byte offset}) of the workspace (rrl_pointnet_group_workspace_bytes); bytes is 0 for a refused shape."""
    off = (ctypes.c_size_t * len(PG_FIELDS))()
    n = int(_lib.load().rrl_pointnet_group_workspace_bytes(B, N, S, c0, len(widths), _ints(widths), _ints(groups), off))
    return n, dict(zip(PG_FIELDS, (int(o) for o in off)))


def group_workspace_views(ws, B, N, S, c0, widths, groups):
    """Named views of a workspace the grouped forward filled: stat (B, sum G, 4) f64, coef (B, sum c, 2) f64, part [per layer
    (B, chunks, c_l, 2)] f64, ext (B, K, N) f32, flag (B,) int32, y [per hidden layer (B, c_l, N S)] f32."""
    nbytes, off = group_workspace_layout(B, N, S, c0, widths, groups)
    raw = ws.view(torch.uint8)[:nbytes]
    NC, K, ctot, gtot, hid, P = group_chunks(N, S)[1], widths[-1], sum(widths), sum(groups), sum(widths[:-1]), N * S

    def part(name, dtype, count, size):
        return raw[off[name]:off[name] + count * size].view(dtype)
    out = dict(stat=part("STAT", torch.float64, B * gtot * 4, 8).view(B, gtot, 4),
               coef=part("COEF", torch.float64, B * ctot * 2, 8).view(B, ctot, 2),
               ext=part("EXT", torch.float32, B * K * N, 4).view(B, K, N),
               flag=part("FLAG", torch.int32, B, 4),
               y=[], part=[])
    allp = part("PART", torch.float64, B * NC * ctot * 2, 8)
    ally = part("Y", torch.float32, B * hid * P, 4).view(B, hid, P)
    c_at = 0
    for l, c in enumerate(widths):
        out["part"].append(allp[2 * B * NC * c_at:2 * B * NC * (c_at + c)].view(B, NC, c, 2))
        if l + 1 < len(widths):
            out["y"].append(ally[:, c_at:c_at + c])
        c_at += c
    return out


def _group_forward(x, prm, groups, eps, ws=None):
    """rrl_pointnet_group_fwd on prepared tensors -> (out, arg, info, ws); ws: a float32 tensor to use as the workspace."""
    dev = x.device
    B, N, S, c0 = x.shape
    widths = tuple(prm[4 * l].shape[0] for l in range(len(groups)))
    L, K = len(groups), widths[-1]
    wd, gr = _ints(widths), _ints(groups)
    nbytes = int(_lib.load().rrl_pointnet_group_workspace_bytes(B, N, S, c0, L, wd, gr, None))
    if ws is None:
        ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=dev)
    out = torch.empty(B, K, N, device=dev)
    arg = torch.empty(B, K, N, dtype=torch.int32, device=dev)
    info = torch.empty(B, dtype=torch.int32, device=dev)
    ptrs = (ctypes.c_void_p * (4 * L))(*[p.data_ptr() for p in prm])
    P = ops._p
    ops._run(dev, "rrl_pointnet_group_fwd", P(x), ptrs, wd, gr, float(eps), P(ws), ws.numel() * 4, P(out), P(arg), P(info), B, N, S, c0, L)
    return out, arg, info, ws


def _group_backward(x, prm, groups, ws, arg, g_out, want_x=True, want=None, bws=None, fill=None):
    """rrl_pointnet_group_bwd on prepared tensors and the forward's ws and arg -> (d_x or None, [dW_1, db_1, dgamma_1, dbeta_1,
    ...] with None where want[i] is false).  want: 4 L booleans (default: all); fill: a value the outputs are pre-filled with."""
    dev = x.device
    B, N, S, c0 = x.shape
    widths = tuple(prm[4 * l].shape[0] for l in range(len(groups)))
    L = len(groups)
    wd, gr = _ints(widths), _ints(groups)
    want = [True] * (4 * L) if want is None else list(want)
    if bws is None:
        bws = torch.empty(int(_lib.load().rrl_pointnet_group_bwd_workspace_bytes(B, N, S, c0, L, wd, gr)) // 8, dtype=torch.float64, device=dev)
    new = torch.empty if fill is None else (lambda *a, **kw: torch.full(*a, fill_value=fill, **kw))
    d_x = new(tuple(x.shape), device=dev) if want_x else None
    d_prm = [new(tuple(p.shape), device=dev) if w else None for p, w in zip(prm, want)]
    ptrs = (ctypes.c_void_p * (4 * L))(*[p.data_ptr() for p in prm])
    dptrs = (ctypes.c_void_p * (4 * L))(*[d.data_ptr() if d is not None else None for d in d_prm]) if any(want) else None
    P = ops._p
    g = g_out.detach().to(dtype=torch.float32, device=dev).contiguous()
    ops._run(dev, "rrl_pointnet_group_bwd", P(x), ptrs, wd, gr, P(ws), ws.numel() * 4, P(arg), P(g), P(bws), bws.numel() * 8, P(d_x), dptrs,
             B, N, S, c0, L)
    return d_x, d_prm


class _EncodeGrouped(torch.autograd.Function):
    """ONE autograd node: rrl_pointnet_group_fwd forwards, rrl_pointnet_group_bwd backwards on what the forward kept."""

    @staticmethod
    def forward(ctx, x, groups, eps, *params):
        dev = ops._home(x, *params)
        xs = ops._prep(x, "x", None, dev)
        prm = [ops._prep(p, "params", None, dev) for p in params]
        out, arg, info, ws = _group_forward(xs, prm, groups, eps)
        ctx.keep = (xs, prm, ws, arg)
        ctx.groups = groups
        ctx.devs = (x.device,) + tuple(p.device for p in params)
        ctx.shapes = tuple(p.shape for p in params)
        ctx.mark_non_differentiable(arg, info)
        return out.to(x.device), arg, info

    @staticmethod
    def backward(ctx, g_out, _ga, _gi):
        xs, prm, ws, arg = ctx.keep
        need = ctx.needs_input_grad
        if g_out is None or not (need[0] or any(need[3:])):
            return (None,) * (3 + len(prm))
        d_x, d_prm = _group_backward(xs, prm, ctx.groups, ws, arg, g_out, bool(need[0]), need[3:])
        out = [d_x.to(ctx.devs[0]) if d_x is not None else None, None, None]
        out += [d.reshape(sh).to(dv) if d is not None else None for d, sh, dv in zip(d_prm, ctx.shapes, ctx.devs[1:])]
        return tuple(out)


def encode_grouped(x, params, groups, eps=1e-5, with_info=False, with_arg=False):
    """out (B, K, N) of x (B, N, S, c0) -- N points of S neighbour slots, as neighbors.ball_group writes them -- through the layers
    params = [W_1, b_1, gamma_1, beta_1, W_2, ...] (a W as (c, c_in) or a Conv2d's (c, c_in, 1, 1)) with groups[l] GroupNorm groups
    each over all N S positions, ReLU after every layer and the max over each point's S slots at the end:
    rpm/models/feature_nets.py:196-199 as one node, differentiable in x and every parameter.  with_info=True also returns info (B,)
    int32: 1 where a group sum of the sample is NaN or infinite (its output is then NaN).  with_arg=True also returns arg
    (B, K, N) int32, the LOWEST slot that gives each output (torch picks its own among equal slots).  Returns out [, info] [, arg]."""
    if not isinstance(x, torch.Tensor):
        raise TypeError("x must be a torch.Tensor")
    params = list(params)
    for p in params:
        if not isinstance(p, torch.Tensor):
            raise TypeError("params must be torch.Tensors")
    groups = tuple(int(g) if not isinstance(g, bool) and int(g) == g else g for g in groups)
    check_group_request(tuple(x.shape), [tuple(p.shape) for p in params], groups, float(eps))
    out, arg, info = _EncodeGrouped.apply(x, groups, float(eps), *params)
    res = (out,)
    if with_info:
        res += (info,)
    if with_arg:
        res += (arg,)
    return res[0] if len(res) == 1 else res


class GroupedEncoder(torch.nn.Module):
    """The grouped encoder as a torch.nn.Module.  Its parameters live in torch's own Conv2d / GroupNorm modules, laid out in
    Sequential blocks so that state_dict() has the reference's keys and shapes; forward() is encode_grouped().
    blocks: {name: number of layers}, in order -- GroupedEncoder.rpm_feat_prepool: prepool (3)."""

    def __init__(self, c0, widths, groups, blocks=None, eps=1e-5):
        super().__init__()
        widths, groups = tuple(int(w) for w in widths), tuple(int(g) for g in groups)
        blocks = dict(blocks) if blocks else {"layers": len(widths)}
        if len(widths) != len(groups) or sum(blocks.values()) != len(widths):
            raise ValueError(f"GroupedEncoder: {len(widths)} widths, {len(groups)} group counts and blocks of {sum(blocks.values())} layers")
        shapes, last = [], c0
        for c in widths:
            shapes += [(c, last, 1, 1), (c,), (c,), (c,)]
            last = c
        check_group_request((1, 1, 1, c0), shapes, groups, eps)
        self.c0, self.widths, self.groups, self.eps = int(c0), widths, groups, float(eps)
        self._blocks = tuple(blocks)
        at, last = 0, c0
        for name, count in blocks.items():
            mods = []
            for c, G in zip(widths[at:at + count], groups[at:at + count]):
                mods += [torch.nn.Conv2d(last, c, 1), torch.nn.GroupNorm(G, c, eps=self.eps), torch.nn.ReLU()]
                last = c
            setattr(self, name, torch.nn.Sequential(*mods))
            at += count

    @classmethod
    def rpm_feat_prepool(cls, raw_dim=10, feature_dim=96):
        """rpm/models/feature_nets.py:118-131, 170 get_prepool(raw_dim, 2 feature_dim): keys prepool.0.weight (feature_dim,
        raw_dim, 1, 1) ... prepool.7.bias (2 feature_dim,)."""
        f = int(feature_dim)
        return cls(int(raw_dim), (f, f, 2 * f), RPM_FEAT_GROUPS, blocks={"prepool": 3})

    def params(self):
        """[W_1, b_1, gamma_1, beta_1, W_2, ...] as encode_grouped takes them."""
        out = []
        for name in self._blocks:
            mods = list(getattr(self, name))
            for conv, norm in zip(mods[0::3], mods[1::3]):
                out += [conv.weight, conv.bias, norm.weight, norm.bias]
        return out

    def forward(self, x, with_info=False, with_arg=False):
        return encode_grouped(x, self.params(), self.groups, self.eps, with_info=with_info, with_arg=with_arg)
