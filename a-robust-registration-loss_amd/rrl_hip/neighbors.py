"""Pseudo-triangle builder on the GPU (reference: Sample_neighs, code/loss.py:473-485 with
utils.farthest_point_sample, code/utils.py:275-296, and sklearn's KDTree).  SURVEY.md §8f row 1."""
import numpy as np
import torch

from .ops import _home, _p, _run


def _check_index(idx, n, name, shape):
    """The kernels follow these indices into the cloud unchecked: refuse one outside [0, n) on the host, before any launch
    (preprocessing: reading a GPU-resident index tensor back synchronises, once per cloud)."""
    if not isinstance(idx, torch.Tensor) or idx.dtype.is_floating_point or idx.dtype == torch.bool:
        raise ValueError(f"{name} must be an integer tensor")
    if tuple(idx.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, got {tuple(idx.shape)}")
    if idx.numel() and bool(((idx < 0) | (idx >= n)).any()):
        raise ValueError(f"{name} holds an index outside [0, {n})")


def fps(points, num_sample, start=None):
    """points (B, n, 3) tensor -> (B, S) int32 indices in farthest-point order.  `start` (B,)
    defaults to torch.randint(0, n, (B,)) from the CPU generator, like the reference; a given start
    outside [0, n) is a ValueError."""
    B, n, _ = points.shape
    if start is None:
        start = torch.randint(0, n, (B,), dtype=torch.long)
    else:
        _check_index(start, n, "start", (B,))
    dev = _home(points)
    pts = points.detach().to(device=dev, dtype=torch.float32).contiguous()
    S = min(int(num_sample), n)
    st = start.to(device=dev, dtype=torch.int32).contiguous()
    out = torch.empty(B, S, dtype=torch.int32, device=dev)
    scratch = torch.empty(B, n, dtype=torch.float32, device=dev)
    _run(dev, "rrl_fps", _p(pts), _p(st), _p(out), _p(scratch), B, n, S)
    return out


def knn3(points, query_idx):
    """points (B, n, 3), query_idx (B, S) -> (B, S, 3) int32: the 3 nearest of the cloud's n points to each query point,
    the query itself and its duplicates included, ascending distance, the lowest index among equals (so a query comes first
    unless a duplicate of it has a lower index).  ValueError for n < 3 or a query index outside [0, n)."""
    B, n, _ = points.shape
    if n < 3:
        raise ValueError(f"knn3 needs at least 3 points per cloud, got {n}")
    if query_idx.dim() != 2:
        raise ValueError(f"query_idx must have shape (B, S), got {tuple(query_idx.shape)}")
    _check_index(query_idx, n, "query_idx", (B, query_idx.shape[1]))
    dev = _home(points, query_idx)
    pts = points.detach().to(device=dev, dtype=torch.float32).contiguous()
    qi = query_idx.to(device=dev, dtype=torch.int32).contiguous()
    S = qi.shape[1]
    nn = torch.empty(B, S, 3, dtype=torch.int32, device=dev)
    _run(dev, "rrl_knn3", _p(pts), _p(qi), _p(nn), B, n, S)
    return nn


def sample_neighs(points, num_sample=5000, num_neigh=3):
    """numpy (n, 3) -> numpy (3 S, 3): rows [p, nn1, nn2] of the S farthest-point samples
    (S = min(num_sample, n)), the row layout every caller reshapes to (S, 9)."""
    if num_neigh != 3:
        raise ValueError("the loss uses pseudo-triangles: num_neigh must be 3")
    pts_np = np.asarray(points)
    if pts_np.ndim != 2 or pts_np.shape[0] < 3:
        raise ValueError(f"sample_neighs needs at least 3 points, got an array of shape {pts_np.shape}")
    pts = torch.from_numpy(np.ascontiguousarray(pts_np, dtype=np.float32))[None]
    idx = fps(pts, num_sample)
    nn = knn3(pts, idx)[0].long().cpu().numpy()
    out = pts_np[nn.reshape(-1)]  # gathers from the caller's array: keeps its dtype
    return out.reshape(-1, 3)
