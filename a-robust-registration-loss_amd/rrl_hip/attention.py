"""DCP's multi-head attention on the device (include/rrl.h rrl_attention_fwd / rrl_attention_bwd): the
core of MultiHeadedAttention.forward (dcp/model.py:27-34, 212-246) --

    q, k, v  = l(x).view(B, -1, h, d_k).transpose(1, 2).contiguous()          # three head-major copies
    x        = softmax(q k^T / sqrt(d_k), dim=-1) v                            # (B, h, N, M) float32, kept for the backward
    x        = x.transpose(1, 2).contiguous().view(B, -1, h d_k)               # a fourth copy

as one node on the projections as nn.Linear leaves them:

    x = attend(q, k, v, n_heads)                                               # (B, N, h d_k), differentiable in all three

The scores are float32 fmaf chains over a head's channels on the matrix cores, recomputed where they are needed and never
stored; the weighted sum is a second matrix-core chain over the columns; the backward keeps two doubles per row.  The result
is the same bits on every call.  There is no fallback: without the library or a GPU every call raises.

MultiHeadedAttention and Transformer are torch modules with the reference's state_dict keys (strict=True loads a DCP
checkpoint's `pointer.` sub-dict): projections, LayerNorm and feed-forward stay torch, the attention step is the node.
"""
import copy

import torch
from torch import nn

from . import _lib, ops
from ._abi import CONSTANTS

MAX_B = 32767
MAX_DIM = 16384   # N, M of one call
MAX_H = 16
MAX_DK = CONSTANTS["RRL_ATTENTION_MAX_DK"]


def check_request(q_shape, k_shape, v_shape, n_heads, counts_q_shape=None, counts_kv_shape=None):
    """The refusals of attend that need no GPU (ValueError)."""
    if len(q_shape) != 3 or len(k_shape) != 3 or len(v_shape) != 3:
        raise ValueError("attend takes q (B, N, D), k (B, M, D) and v (B, M, D), token-major as nn.Linear leaves them")
    B, N, D = q_shape
    M = k_shape[1]
    if tuple(k_shape) != (B, M, D) or tuple(v_shape) != (B, M, D):
        raise ValueError(f"attend: k and v must both be (B, M, D) with q's B and D = {(B, D)}; got {tuple(k_shape)} and "
                         f"{tuple(v_shape)}")
    if not isinstance(n_heads, int) or n_heads < 1 or n_heads > MAX_H:
        raise ValueError(f"attend: n_heads must be an integer in [1, {MAX_H}]; got {n_heads!r}")
    if D < 1 or D % n_heads:
        raise ValueError(f"attend: the model dimension D = {D} must be a positive multiple of n_heads = {n_heads}")
    if D // n_heads > MAX_DK:
        raise ValueError(f"attend: the head dimension D / n_heads must lie in [1, {MAX_DK}]; got {D // n_heads}")
    if B < 1 or B > MAX_B:
        raise ValueError(f"attend serves 1 to {MAX_B} samples per call; got {B}: split the batch")
    if N < 1 or M < 1 or N > MAX_DIM or M > MAX_DIM:
        raise ValueError(f"attend: N and M must lie in [1, {MAX_DIM}]; got {N} and {M}")
    for shape, name in ((counts_q_shape, "counts_q"), (counts_kv_shape, "counts_kv")):
        if shape is not None and tuple(shape) != (B,):
            raise ValueError(f"attend: {name} must be (B,) = {(B,)}; got {tuple(shape)}")


class _Attend(torch.autograd.Function):
    """ONE autograd node: rrl_attention_fwd forwards, rrl_attention_bwd backwards, on the row maxima and sums the forward kept.
    What the backward needs -- the output among it -- goes through save_for_backward: a tensor kept as a plain attribute of
    the context would tie the output to its own grad_fn and leave every call's buffers to the cyclic collector."""

    @staticmethod
    def forward(ctx, q, k, v, n_heads, counts_q, counts_kv, want_info):
        dev = ops._home(q, k, v)
        tq, tk, tv = ops._prep(q, "q", None, dev), ops._prep(k, "k", None, dev), ops._prep(v, "v", None, dev)
        B, N, D = tq.shape
        M = tk.shape[1]
        cq, ckv = ops.check_counts(counts_q, B, N, dev, "counts_q"), ops.check_counts(counts_kv, B, M, dev, "counts_kv")
        ws = torch.empty(int(_lib.load().rrl_attention_workspace_bytes(B, n_heads, N, M)) // 8, dtype=torch.float64, device=dev)
        out = torch.empty(B, N, D, device=dev)
        info = torch.empty(B if want_info else 0, dtype=torch.int32, device=dev)   # (not asked for: NULL, no second launch)
        P = ops._p
        ctx.dims = (B, n_heads, D // n_heads, N, M)
        ops._run(dev, "rrl_attention_fwd", P(tq), P(tk), P(tv), P(cq), P(ckv), P(ws), ws.numel() * 8, P(out),
                 P(info) if want_info else None, *ctx.dims)
        ctx.devs = (q.device, k.device, v.device)
        ctx.save_for_backward(tq, tk, tv, cq, ckv, ws, out)
        ctx.mark_non_differentiable(info)
        return out.to(q.device), info

    @staticmethod
    def backward(ctx, g_out, _gi):
        tq, tk, tv, cq, ckv, ws, out = ctx.saved_tensors
        dev = tq.device
        g = g_out.detach().to(dtype=torch.float32, device=dev).contiguous()
        need = ctx.needs_input_grad
        grads = [torch.empty_like(t) if need[i] else None for i, t in enumerate((tq, tk, tv))]
        P = ops._p
        if any(t is not None for t in grads):
            ops._run(dev, "rrl_attention_bwd", P(tq), P(tk), P(tv), P(cq), P(ckv), P(ws), ws.numel() * 8, P(out), P(g),
                     P(grads[0]), P(grads[1]), P(grads[2]), *ctx.dims)
        return tuple(t.to(d) if t is not None else None for t, d in zip(grads, ctx.devs)) + (None, None, None, None)


def attend(q, k, v, n_heads, counts_q=None, counts_kv=None, with_info=False):
    """out (B, N, D) from q (B, N, D), k (B, M, D) and v (B, M, D), token-major with head h in channels h D / n_heads ..
    (h + 1) D / n_heads - 1: out = concat_h softmax(q_h k_h^T / sqrt(d_k), dim=-1) v_h (dcp/model.py:27-34, 232-245), differentiable
    in all three by one node; no (B, h, N, M) matrix and no head-major copy exists, forward or backward.
    counts_q / counts_kv ((B,) list or int32 GPU tensor): sample b has its first counts_q[b] query rows and counts_kv[b] key /
    value rows; the rest is never read, out is 0 on the rows beyond (and on every row of a sample without keys) and those
    rows and columns get zero gradient.
    with_info=True also returns info (B,) int32: 1 where a score or an output entry inside the counts is NaN or infinite.
    Returns out [, info]."""
    for t, name in ((q, "q"), (k, "k"), (v, "v")):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")

    def shape_of(cnt):
        if cnt is None:
            return None
        return tuple(cnt.shape) if isinstance(cnt, torch.Tensor) else tuple(torch.as_tensor(cnt).shape)
    check_request(tuple(q.shape), tuple(k.shape), tuple(v.shape), n_heads, shape_of(counts_q), shape_of(counts_kv))
    B, N, _ = q.shape
    M = k.shape[1]
    for cnt, cap, name in ((counts_q, N, "counts_q"), (counts_kv, M, "counts_kv")):
        if cnt is not None:
            ops.check_counts_host(cnt, B, cap, name)
    out, info = _Attend.apply(q, k, v, n_heads, counts_q, counts_kv, bool(with_info))
    return (out, info) if with_info else out


def scores(q, k, n_heads, counts_q=None, counts_kv=None):
    """The scaled scores z (B, n_heads, N, M) the node takes its softmax of (rrl_attention_scores: the same chains, the same
    bits), -inf at and beyond the counts; detached.  For tests and a trainer's endpoints: the node itself never stores them."""
    check_request(tuple(q.shape), tuple(k.shape), tuple(k.shape), n_heads)
    dev = ops._home(q, k)
    tq, tk = ops._prep(q, "q", None, dev), ops._prep(k, "k", None, dev)
    B, N, D = tq.shape
    M = tk.shape[1]
    cq, ckv = ops.check_counts(counts_q, B, N, dev, "counts_q"), ops.check_counts(counts_kv, B, M, dev, "counts_kv")
    z = torch.empty(B, n_heads, N, M, device=dev)
    P = ops._p
    ops._run(dev, "rrl_attention_scores", P(tq), P(tk), P(cq), P(ckv), P(z), B, n_heads, D // n_heads, N, M)
    return z


# ---- the reference's modules around the node (written from their structure; state_dict keys as dcp/model.py's) ---------------
class LayerNorm(nn.Module):
    """a_2 (x - mean) / (std + eps) + b_2 over the last dimension: the UNBIASED std, eps added to the std (model.py:158-168)."""

    def __init__(self, features, eps=1e-6):
        super().__init__()
        self.a_2 = nn.Parameter(torch.ones(features))
        self.b_2 = nn.Parameter(torch.zeros(features))
        self.eps = eps

    def forward(self, x):
        mean = x.mean(-1, keepdim=True)
        return self.a_2 * (x - mean) / (x.std(-1, keepdim=True) + self.eps) + self.b_2


class MultiHeadedAttention(nn.Module):
    """Four d_model x d_model projections (linears.0 .. 3: query, key, value, output) around attend."""

    def __init__(self, h, d_model):
        super().__init__()
        if d_model % h:
            raise ValueError(f"d_model = {d_model} is no multiple of h = {h}")
        self.h, self.d_k = h, d_model // h
        self.linears = nn.ModuleList([nn.Linear(d_model, d_model) for _ in range(4)])

    def forward(self, query, key, value, counts_q=None, counts_kv=None):
        q, k, v = (lin(x) for lin, x in zip(self.linears, (query, key, value)))
        return self.linears[3](attend(q, k, v, self.h, counts_q, counts_kv))


class PositionwiseFeedForward(nn.Module):
    def __init__(self, d_model, d_ff):
        super().__init__()
        self.w_1 = nn.Linear(d_model, d_ff)
        self.w_2 = nn.Linear(d_ff, d_model)

    def forward(self, x):
        return self.w_2(torch.relu(self.w_1(x)))


class _Sublayer(nn.Module):
    """x + sublayer(norm(x)) (model.py:171-177)."""

    def __init__(self, size):
        super().__init__()
        self.norm = LayerNorm(size)

    def forward(self, x, sublayer):
        return x + sublayer(self.norm(x))


class _EncoderLayer(nn.Module):
    def __init__(self, size, self_attn, feed_forward):
        super().__init__()
        self.self_attn, self.feed_forward = self_attn, feed_forward
        self.sublayer = nn.ModuleList([_Sublayer(size) for _ in range(2)])

    def forward(self, x):
        x = self.sublayer[0](x, lambda y: self.self_attn(y, y, y))
        return self.sublayer[1](x, self.feed_forward)


class _DecoderLayer(nn.Module):
    def __init__(self, size, self_attn, src_attn, feed_forward):
        super().__init__()
        self.self_attn, self.src_attn, self.feed_forward = self_attn, src_attn, feed_forward
        self.sublayer = nn.ModuleList([_Sublayer(size) for _ in range(3)])

    def forward(self, x, memory):
        x = self.sublayer[0](x, lambda y: self.self_attn(y, y, y))
        x = self.sublayer[1](x, lambda y: self.src_attn(y, memory, memory))
        return self.sublayer[2](x, self.feed_forward)


class _Stack(nn.Module):
    """n copies of a layer, then a LayerNorm (Encoder / Decoder, model.py:132-155)."""

    def __init__(self, layer, size, n):
        super().__init__()
        self.layers = nn.ModuleList([copy.deepcopy(layer) for _ in range(n)])
        self.norm = LayerNorm(size)

    def forward(self, x, *memory):
        for layer in self.layers:
            x = layer(x, *memory)
        return self.norm(x)


class _EncoderDecoder(nn.Module):
    def __init__(self, encoder, decoder):
        super().__init__()
        self.encoder, self.decoder = encoder, decoder

    def forward(self, src, tgt):
        return self.decoder(tgt, self.encoder(src))


class Transformer(nn.Module):
    """DCP's pointer transformer (model.py:373-401): n_blocks encoder layers (self-attention, feed-forward) and decoder layers
    (self-attention, cross-attention onto the encoder's output, feed-forward), no masks, no dropout (the reference builds both
    as None).  forward(src, tgt) takes the embeddings channel-first (B, emb_dims, N) and (B, emb_dims, M) and returns
    (src_embedding, tgt_embedding) of the same shapes: the decoder's output for (tgt, src) and for (src, tgt)."""

    def __init__(self, emb_dims, n_heads, ff_dims, n_blocks=1):
        super().__init__()
        self.emb_dims, self.n_heads, self.ff_dims, self.n_blocks = emb_dims, n_heads, ff_dims, n_blocks

        def attn():
            return MultiHeadedAttention(n_heads, emb_dims)

        def ff():
            return PositionwiseFeedForward(emb_dims, ff_dims)
        self.model = _EncoderDecoder(_Stack(_EncoderLayer(emb_dims, attn(), ff()), emb_dims, n_blocks),
                                     _Stack(_DecoderLayer(emb_dims, attn(), attn(), ff()), emb_dims, n_blocks))

    def forward(self, src, tgt):
        src, tgt = src.transpose(2, 1).contiguous(), tgt.transpose(2, 1).contiguous()
        tgt_embedding = self.model(src, tgt).transpose(2, 1).contiguous()
        src_embedding = self.model(tgt, src).transpose(2, 1).contiguous()
        return src_embedding, tgt_embedding
