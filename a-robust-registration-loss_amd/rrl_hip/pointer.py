"""DCP's softmax pointer on the device (include/rrl.h rrl_pointer_fwd / rrl_pointer_bwd): the part of
SVDHead.forward between the embeddings and the Kabsch fit (dcp/model.py:419-425) --

    scores   = softmax(src_emb^T tgt_emb / sqrt(C), dim=2)      # (B, N, M), never stored
    src_corr = tgt scores^T                                     # (B, 3, N)

as one node:

    corr = soft_pointer(src_emb, tgt_emb, tgt)                  # differentiable in all three

The scores are float32 fmaf chains over the channels on the matrix cores, the softmax sums are fixed-order double sums,
the backward recomputes the scores; the result is the same bits on every call.  There is no fallback: without the library
or a GPU every call raises.
"""
import torch

from . import _lib, ops
from ._abi import CONSTANTS

MAX_B = 32767
MAX_DIM = 16384   # N, M of one call
MAX_C = CONSTANTS["RRL_POINTER_MAX_C"]
SLICE = CONSTANTS["RRL_POINTER_SLICE"]   # columns per slice of the forward


def check_request(src_emb_shape, tgt_emb_shape, tgt_shape, counts_src_shape=None, counts_tgt_shape=None):
    """The refusals of soft_pointer that need no GPU (ValueError)."""
    if len(src_emb_shape) != 3 or len(tgt_emb_shape) != 3 or len(tgt_shape) != 3:
        raise ValueError("soft_pointer takes src_emb (B, C, N), tgt_emb (B, C, M) and tgt (B, 3, M), channel-first")
    B, C, N = src_emb_shape
    M = tgt_emb_shape[2]
    if tuple(tgt_emb_shape[:2]) != (B, C):
        raise ValueError(f"soft_pointer: tgt_emb must be (B, C, M) with src_emb's B and C = {(B, C)}; got {tuple(tgt_emb_shape)}")
    if tuple(tgt_shape) != (B, 3, M):
        raise ValueError(f"soft_pointer: tgt must be (B, 3, M) = {(B, 3, M)}, one point per column of tgt_emb; got "
                         f"{tuple(tgt_shape)}")
    if B < 1 or B > MAX_B:
        raise ValueError(f"soft_pointer serves 1 to {MAX_B} samples per call; got {B}: split the batch")
    if C < 1 or C > MAX_C:
        raise ValueError(f"soft_pointer: the embedding dimension C must lie in [1, {MAX_C}]; got {C}")
    if N < 1 or M < 1 or N > MAX_DIM or M > MAX_DIM:
        raise ValueError(f"soft_pointer: N and M must lie in [1, {MAX_DIM}]; got {N} and {M}")
    for shape, name in ((counts_src_shape, "counts_src"), (counts_tgt_shape, "counts_tgt")):
        if shape is not None and tuple(shape) != (B,):
            raise ValueError(f"soft_pointer: {name} must be (B,) = {(B,)}; got {tuple(shape)}")


class _SoftPointer(torch.autograd.Function):
    """ONE autograd node: rrl_pointer_fwd forwards, rrl_pointer_bwd backwards, on the row maxima and sums the forward kept."""

    @staticmethod
    def forward(ctx, src_emb, tgt_emb, tgt, counts_src, counts_tgt, want_scores):
        dev = ops._home(src_emb, tgt_emb, tgt)
        se, te, x = ops._prep(src_emb, "src_emb", None, dev), ops._prep(tgt_emb, "tgt_emb", None, dev), ops._prep(tgt, "tgt", None, dev)
        B, C, N = se.shape
        M = te.shape[2]
        cs, ct = ops.check_counts(counts_src, B, N, dev, "counts_src"), ops.check_counts(counts_tgt, B, M, dev, "counts_tgt")
        ws = torch.empty(int(_lib.load().rrl_pointer_workspace_bytes(B, C, N, M)) // 8, dtype=torch.float64, device=dev)
        corr = torch.empty(B, 3, N, device=dev)
        scores = torch.empty(B, N, M, device=dev) if want_scores else None
        info = torch.empty(B, dtype=torch.int32, device=dev)
        P = ops._p
        ctx.call = (P(se), P(te), P(x), P(cs), P(ct), P(ws), ws.numel() * 8)
        ctx.dims = (B, C, N, M)
        ops._run(dev, "rrl_pointer_fwd", *ctx.call, P(corr), P(scores), P(info), B, C, N, M)
        ctx.keep = (se, te, x, cs, ct, ws)
        ctx.devs = (src_emb.device, tgt_emb.device, tgt.device)
        if scores is None:
            scores = torch.empty(0, device=dev)
        ctx.mark_non_differentiable(info, scores)
        return corr.to(src_emb.device), info, scores

    @staticmethod
    def backward(ctx, g_corr, _gi, _gs):
        se, te, x = ctx.keep[:3]
        dev = se.device
        g = g_corr.detach().to(dtype=torch.float32, device=dev).contiguous()
        need = ctx.needs_input_grad
        out = [torch.empty_like(t) if need[i] else None for i, t in enumerate((se, te, x))]
        P = ops._p
        if any(o is not None for o in out):
            ops._run(dev, "rrl_pointer_bwd", *ctx.call, P(g), P(out[0]), P(out[1]), P(out[2]), *ctx.dims)
        return tuple(o.to(d) if o is not None else None for o, d in zip(out, ctx.devs)) + (None, None, None)


def soft_pointer(src_emb, tgt_emb, tgt, counts_src=None, counts_tgt=None, with_info=False, return_scores=False):
    """corr (B, 3, N) from src_emb (B, C, N), tgt_emb (B, C, M) and tgt (B, 3, M), channel-first as DCP holds them:
    corr = tgt softmax(src_emb^T tgt_emb / sqrt(C), dim=2)^T (dcp/model.py:419-425), differentiable in all three by one node;
    the (B, N, M) matrix is never stored, forward or backward.
    counts_src / counts_tgt ((B,) list or int32 GPU tensor): sample b has its first counts_src[b] source points and
    counts_tgt[b] target points; the rest is never read, corr is 0 on the rows beyond (and on every row of a sample without
    targets) and those rows and columns get zero gradient.
    with_info=True also returns info (B,) int32: 1 where a score inside the counts is NaN or infinite (that sample's
    outputs are then NaN where it reaches), else 0.  return_scores=True also returns the scaled scores (B, N, M) the softmax
    is taken of, detached (for a trainer's endpoints; -inf beyond the counts): no gradient flows through them.
    Returns corr [, info] [, scores]."""
    for t, name in ((src_emb, "src_emb"), (tgt_emb, "tgt_emb"), (tgt, "tgt")):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")

    def shape_of(cnt):
        if cnt is None:
            return None
        return tuple(cnt.shape) if isinstance(cnt, torch.Tensor) else tuple(torch.as_tensor(cnt).shape)
    check_request(tuple(src_emb.shape), tuple(tgt_emb.shape), tuple(tgt.shape), shape_of(counts_src), shape_of(counts_tgt))
    B, _, N = src_emb.shape
    M = tgt_emb.shape[2]
    for cnt, cap, name in ((counts_src, N, "counts_src"), (counts_tgt, M, "counts_tgt")):
        if cnt is not None:
            ops.check_counts_host(cnt, B, cap, name)
    corr, info, scores = _SoftPointer.apply(src_emb, tgt_emb, tgt, counts_src, counts_tgt, bool(return_scores))
    out = (corr,)
    if with_info:
        out += (info,)
    if return_scores:
        out += (scores,)
    return out[0] if len(out) == 1 else out
