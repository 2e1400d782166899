"""Ragged batches: lists of per-sample arrays -> the capacity-shaped tensors + counts that the batched entries take
(ops.intersection_loss / registration_loss / LossStep / RegistrationStep, loss.batched_intersection_loss: counts1=,
counts2=, nlines=; include/rrl.h rrl_opts.count1) and the ragged Chamfer distance (pack_points -> ops.chamfer(counts_x=, counts_y=)).  Host-side helpers (numpy / torch on the CPU): move the results to the
GPU with `.cuda()`.  A DataLoader collate_fn for items with `src_tri`, `tar_tri`, `lines` (and `kd_order` rows):

    def collate(items):
        p1, c1 = ragged.pack_clouds([it["src_tri"] for it in items])
        p2, c2 = ragged.pack_clouds([it["tar_tri"] for it in items])
        ln, nl = ragged.pack_lines([it["lines"] for it in items])
        return p1, p2, ln, c1, c2, nl

The rows beyond a count are never read as data by the library; `fill` only decides what a reader of the tensors sees there.
"""
import numpy as np
import torch


def _pack(items, width, capacity, fill, multiple, what):
    arrs = [np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a, dtype=np.float32).reshape(-1, width)
            for a in items]
    counts = np.array([len(a) for a in arrs], dtype=np.int32)
    cap = int(counts.max()) if len(arrs) else 0
    if capacity is not None:
        if int(capacity) < cap:
            raise ValueError(f"{what}: capacity {capacity} is below the largest sample ({cap} rows)")
        cap = int(capacity)
    if multiple > 1:
        cap = (cap + multiple - 1) // multiple * multiple
    out = np.full((len(arrs), cap, width), fill, dtype=np.float32)
    for b, a in enumerate(arrs):
        out[b, :len(a)] = a
    return torch.from_numpy(out), torch.from_numpy(counts)


def pack_clouds(clouds, capacity=None, fill=0.0, multiple=1):
    """[(n_b, 9) pseudo-triangles] -> (tri (B, cap, 9) fp32, counts (B,) int32); cap = the largest n_b (or `capacity`),
    rounded up to `multiple`; rows beyond counts[b] hold `fill`."""
    return _pack(clouds, 9, capacity, fill, multiple, "pack_clouds")


def pack_points(clouds, capacity=None, fill=0.0, multiple=1):
    """[(n_b, 3) points] -> (pts (B, cap, 3) fp32, counts (B,) int32): the inputs of ops.chamfer(x, y, counts_x=, counts_y=)
    / loss.chamfer_dist(..., counts_x=, counts_y=); cap and fill as in pack_clouds."""
    return _pack(clouds, 3, capacity, fill, multiple, "pack_points")


def pack_lines(lines, capacity=None, fill=0.0, multiple=1):
    """[(l_b, 6) lines (dir, x0)] -> (line (B, cap, 6) fp32, nlines (B,) int32)."""
    return _pack(lines, 6, capacity, fill, multiple, "pack_lines")


def pack_orders(orders, counts, capacity=None):
    """[order row of sample b: at least counts[b] entries, the first counts[b] a permutation of [0, counts[b])] -- e.g. the
    `kd_order` rows of dataset items (pre_dataloader) -- -> int32 (B, 64 ceil(cap / 64)), the layout of
    ops.cloud_order(tri, counts=); cap = `capacity` (the clouds' capacity) or the largest count.  Entries beyond a count
    are 0 (not read).  ValueError when a row's head is not such a permutation."""
    counts = np.asarray(counts.cpu() if isinstance(counts, torch.Tensor) else counts, dtype=np.int64).reshape(-1)
    if len(orders) != len(counts):
        raise ValueError("pack_orders: one order row per sample")
    cap = int(counts.max()) if len(counts) else 0
    if capacity is not None:
        if int(capacity) < cap:
            raise ValueError(f"pack_orders: capacity {capacity} is below the largest count ({cap})")
        cap = int(capacity)
    out = np.zeros((len(counts), (cap + 63) // 64 * 64), dtype=np.int32)
    for b, (o, n) in enumerate(zip(orders, counts)):
        row = np.asarray(o.cpu() if isinstance(o, torch.Tensor) else o, dtype=np.int64).reshape(-1)
        n = int(n)
        if len(row) < n or not np.array_equal(np.sort(row[:n]), np.arange(n)):
            raise ValueError(f"pack_orders: the first {n} entries of row {b} must be a permutation of [0, {n})")
        out[b, :n] = row[:n]
    return torch.from_numpy(out)
