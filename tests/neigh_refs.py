"""Numpy twin of the COUNTED pseudo-triangle builder (include/rrl.h rrl_fps_counted / rrl_knn3_counted / rrl_knn3_self;
rrl_hip.neighbors.pseudo_triangles), built from prep_refs.fps_ref / knn3_ref on each sample's TRUNCATED cloud -- nothing
here is computed from the code under test.  Sample b has n_b = counts[b] points (None: all n); with a sampler it has
S_b = min(S, n_b) queries, in fps_ref's order, without one its n_b rows in row order; a sample of fewer than three points has
no triangles (tri_counts 0).  Rows beyond a count are zero."""
import numpy as np

import prep_refs as PF

KNN_CHUNK = 256  # knn3_ref materialises (S, n, 3) float64: a few hundred queries at a time


def knn3_chunked(points, query_idx):
    """prep_refs.knn3_ref, KNN_CHUNK queries at a time: (S, 3) int64."""
    q = np.asarray(query_idx, np.int64)
    if len(q) == 0:
        return np.zeros((0, 3), np.int64)
    return np.concatenate([PF.knn3_ref(points, q[i:i + KNN_CHUNK]) for i in range(0, len(q), KNN_CHUNK)])


def fps_counted_ref(points, counts, S, start):
    """points (B, n, 3) float32 -> (idx (B, S) int64, S_b (B,)): fps_ref on points[b, :n_b] with start[b], zeros beyond S_b."""
    B, n, _ = points.shape
    counts = np.full(B, n) if counts is None else np.asarray(counts)
    idx, sb = np.zeros((B, S), np.int64), np.zeros(B, np.int64)
    for b in range(B):
        nb = int(counts[b])
        sb[b] = min(S, nb)
        if sb[b]:
            idx[b, :sb[b]] = PF.fps_ref(points[b, :nb], int(sb[b]), int(start[b]))
    return idx, sb


def pseudo_triangles_ref(points, counts=None, num_sample=None, start=None):
    """dict(idx (B, S) int64 -- the row numbers without a sampler --, nn (B, S, 3) int64, tri (B, S, 9) in points' dtype,
    tri_counts (B,) int64, fps_counts (B,))."""
    points = np.asarray(points)
    B, n, _ = points.shape
    cnt = np.full(B, n) if counts is None else np.asarray(counts)
    if num_sample is None:
        S = n
        idx = np.zeros((B, S), np.int64)
        sb = cnt.astype(np.int64).copy()
        for b in range(B):
            idx[b, :sb[b]] = np.arange(sb[b])
    else:
        S = min(int(num_sample), n)
        idx, sb = fps_counted_ref(points, cnt, S, start)
    nn = np.zeros((B, S, 3), np.int64)
    tri = np.zeros((B, S, 9), points.dtype)
    tc = np.zeros(B, np.int64)
    for b in range(B):
        nb = int(cnt[b])
        if nb < 3:
            continue
        tc[b] = sb[b]
        nn[b, :sb[b]] = knn3_chunked(points[b, :nb], idx[b, :sb[b]])
        tri[b, :sb[b]] = points[b][nn[b, :sb[b]].reshape(-1)].reshape(-1, 9)
    return dict(idx=idx, nn=nn, tri=tri, tri_counts=tc, fps_counts=sb)
