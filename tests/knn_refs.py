"""Host twin of rrl_knn (include/rrl.h "k nearest neighbours") in numpy: the rule restated, not the
kernel's loops.  d = (dx dx + dy dy) + dz dz from the float64 differences of the float32 coordinates; the result of a query is
its k smallest keys (d, index) in lexicographic order (np.lexsort); a NaN or infinite d is no neighbour; found = min(k,
neighbours); the slots beyond found repeat slot 0; a row with found == 0 is zero."""
import numpy as np

import group_refs as GR

FEATURES = ("nbr", "dxyz", "ctr")
BORDER = GR.BORDER  # a row is borderline when two consecutive keys among its first k + 1 differ by <= BORDER (|x_i|^2 + |x_j|^2)

# name -> (seed, B, N, kind) of group_refs.make_cloud: the clouds of tests/golden/knn_dcp.npz
DCP_CASES = {
    "cube_b4_1024": (0, 4, 1024, "cube"),
    "sphere_b4_1024": (1, 4, 1024, "sphere"),
    "sphere_b2_717": (2, 2, 717, "sphere"),
    "cube_b3_257": (3, 3, 257, "cube"),
    "sphere_b2_130": (4, 2, 130, "sphere"),
    "cube_b2_65": (5, 2, 65, "cube"),
}
DCP_KS = (20, 4, 1)
ROWS = 512  # queries per block of the twin
BORDER_SHARE_MAX = 0.02  # per case: the condition of the fixture, not a measurement


def knn(points, k, query=None, counts=None, qcounts=None, exclude_self=False):
    """numpy (B, n, 3) float32 [, query (B, S, 3)] -> dict(idx (B, S, k) int32, found (B, S) int32, d (B, S, k) float64 -- dist2 is
    its float32 rounding --, border (B, S) bool)."""
    points = np.asarray(points, np.float32)
    B, n, _ = points.shape
    self_form = query is None
    qpts = points if self_form else np.asarray(query, np.float32)
    S = qpts.shape[1]
    idx = np.zeros((B, S, k), np.int32)
    found = np.zeros((B, S), np.int32)
    d = np.zeros((B, S, k), np.float64)
    border = np.zeros((B, S), bool)
    for b in range(B):
        nb = n if counts is None else min(max(int(counts[b]), 0), n)
        Sb = nb if self_form else (S if qcounts is None else min(max(int(qcounts[b]), 0), S))
        if nb == 0 or Sb == 0:
            continue
        x = points[b, :nb]
        with np.errstate(invalid="ignore", over="ignore"):
            sq = (x.astype(np.float64) ** 2).sum(-1)
        for r0 in range(0, Sb, ROWS):  # (blocks of queries: the (rows, n) matrices stay small)
            q = qpts[b, r0:min(r0 + ROWS, Sb)]
            m_ = len(q)
            with np.errstate(invalid="ignore", over="ignore"):
                d2 = GR.dist2(q, x)
                sqq = (q.astype(np.float64) ** 2).sum(-1)
            ok = np.isfinite(d2)
            if exclude_self and self_form:
                ok[np.arange(m_), r0 + np.arange(m_)] = False
            key = np.where(ok, d2, np.inf)
            cols = np.broadcast_to(np.arange(nb), key.shape)
            order = np.lexsort((cols, key), axis=-1)  # by d, then by index
            have = ok.sum(1)
            f = np.minimum(have, k)
            m = min(k + 1, nb)
            first = order[:, :m]
            dk = np.take_along_axis(key, first, 1)
            rows = np.zeros((m_, k), np.int64)
            dd = np.zeros((m_, k), np.float64)
            kk = min(k, nb)
            rows[:, :kk], dd[:, :kk] = first[:, :kk], dk[:, :kk]
            pad = np.arange(k)[None, :] >= f[:, None]
            rows = np.where(pad, rows[:, :1], rows)
            dd = np.where(pad, dd[:, :1], dd)
            none = f == 0
            rows[none], dd[none] = 0, 0.0
            idx[b, r0:r0 + m_], found[b, r0:r0 + m_], d[b, r0:r0 + m_] = rows, f, dd
            if m > 1:
                with np.errstate(invalid="ignore"):
                    gap = dk[:, 1:] - dk[:, :-1]
                    scale = sqq[:, None] + np.maximum(sq[first[:, 1:]], sq[first[:, :-1]])
                    both = np.arange(1, m)[None, :] < np.minimum(have, k + 1)[:, None]  # both keys of the pair are neighbours
                    border[b, r0:r0 + m_] = (both & (gap <= BORDER * scale)).any(1)
    return dict(idx=idx, found=found, d=d, border=border)


def features(points, twin, names, query=None, channel_first=False):
    """The float32 feature tensor of a twin result: (B, S, k, C), or (B, C, S, k) with channel_first; channels in FEATURES' order."""
    points = np.asarray(points, np.float32)
    qpts = points if query is None else np.asarray(query, np.float32)
    idx, found = twin["idx"], twin["found"]
    B, S, k = idx.shape
    nbr = np.stack([points[b][idx[b]] for b in range(B)])  # (B, S, k, 3)
    ctr = np.broadcast_to(qpts[:, :, None, :], nbr.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        parts = {"nbr": nbr, "dxyz": nbr - ctr, "ctr": ctr}
    out = np.concatenate([parts[f] for f in FEATURES if f in names], -1).astype(np.float32)
    out = np.where((found == 0)[:, :, None, None], np.float32(0), out)
    return np.ascontiguousarray(out.transpose(0, 3, 1, 2)) if channel_first else out


def dcp_cloud(name):
    """(B, N, 3) float32 numpy: the cloud of a fixture case as the recorder drew it."""
    seed, B, N, kind = DCP_CASES[name]
    return GR.make_cloud(seed, B, N, kind)[0].numpy()
